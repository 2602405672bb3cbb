"""GPU against the oracle on inputs with a non-zero disc offset and rotated, unequal-axis
ellipsoids with chi != 1 (tests/geometry_cases.py; tests/test_geometry_inputs.py shows on the
oracle alone that these inputs keep the perturbed rows active).

With the generators' own inputs (offset 0, circles, chi 1) the kernel's M01, M00 - M11,
sqrt(chi), the rows' psi derivatives, the constraint Hessians' psi blocks, the scenario /
decomp rows' psi terms, the compact row storage's disc path and MIRROR on a stage block where
{x, y} couples to psi are multiplied by zero.  Here they are not:

  (a) 10 SQP-RTI iterations, trajectories and multipliers;
  (b) one iteration from the oracle's carried multipliers of (a): the one QP whose Hessian
      holds the constraint Hessians weighted by given multipliers;
  (c) solver_type SQP on C2 and C1 (the FULL kernel variant).

Bars: equal exit codes, SQP iteration counts and selection; the north-star 1e-4 on states and
inputs, 1e-6 relative on pobj; and max|dx|, max|du| <= max(1e-9, 100 x spread), spread being
the distance between the oracle's default and literal builds on the same batch (1e-9: the
project's figure for rounding, test_c5_rounding_decided_copy; 100 x: the kernel's classical
Riccati is a third arithmetic form beside the two builds).  The 1e-4 bar alone would pass a
kernel without the scenario / decomp rows' Hessian on C3 (8e-6 on the oracle).  No solve is
excluded by index; a solve may part only where the oracle itself parts
(geometry_cases.compare_with_oracle), and at most one per batch.

Measured on an MI355X (max|dx| / max|du| / multipliers relative; bound):
see README.md "Checking".
"""
import numpy as np
import pytest

import geometry_cases as gc

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from oscar_mpc_planner_mr_modification_amd import native as nat
    return nat


def _gpu(native, dev, name, lam_in=None, **opts):
    import torch
    lay, b, params = gc.case_inputs(name)
    pr = native.problem_from_layout(lay, **opts)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731  (a copy: the shared inputs are read-only)
    out = native.solve_batch_device(pr, t(params), t(b.warm), t(b.xinit),
                                    lam_in=None if lam_in is None else t(lam_in), lam_out=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(name, label, ref, lit, got, converged_only=False, check_lam=False, lam_in=None, **opts):
    lay, b, params = gc.case_inputs(name)
    return gc.compare_with_oracle(label, ref, lit, got, converged_only=converged_only, check_lam=check_lam,
                                  scatter=lambda i: gc.oracle_scatter(lay, params, b.warm, b.xinit, i, lam_in=lam_in,
                                                                      **opts))


def _selection(native, dev, name, got, ref):
    """FindBestPlanner (T-MPC++) / the lowest-cost copy (SH-MPC) on GPU and oracle results"""
    import torch
    case = gc.CASES[name]
    lay, b, _ = gc.case_inputs(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    if case.kind == "tmpc":
        from oscar_mpc_planner_mr_modification_amd.selection import find_best_planner_host
        S, G, N = b.n_scenes, b.n_guesses, lay.N
        cons = b.consistency_on.astype(np.uint8)
        psel = b.previously_selected.astype(np.uint8)
        best, _ = native.select_best_device(S, G, N, t(got["xtraj"]), t(got["pobj"]), t(got["exit"]),
                                            prev_traj=t(b.prev_traj), w_cons=0.05, consistency_enabled=t(cons),
                                            previously_selected=t(psel), selection_weight=0.8)
        torch.cuda.synchronize()
        hb, _ = find_best_planner_host(S, G, N, ref["xtraj"], ref["pobj"], ref["status"], b.prev_traj, 0.05, cons,
                                       psel, 0.8)
        assert np.array_equal(best.cpu().numpy(), hb)
        assert (hb >= 0).any()
    elif case.kind == "shmpc":
        from conftest import picks_equivalent
        from oscar_mpc_planner_mr_modification_amd.scenario import select_lowest_cost
        best = native.select_lowest_cost_device(b.n_scenes, b.n_solvers, t(got["pobj"]), t(got["exit"]))
        torch.cuda.synchronize()
        assert picks_equivalent(best.cpu().numpy(), select_lowest_cost(ref["pobj"], ref["status"], b.n_solvers),
                                ref["pobj"])


@pytest.mark.parametrize("name", list(gc.CASES))
def test_rti_and_carried_multipliers(native, dev, oracle_mod, name):
    """(a) 10 RTI iterations with trajectories, multipliers and the selection; (b) one iteration from
    the oracle's carried multipliers of (a), zeroed for failed solves."""
    ref, lit = gc.oracle_run(name), gc.oracle_run(name, literal=True)
    got = _gpu(native, dev, name)
    _compare(name, f"{name} (a) 10 RTI iterations", ref, lit, got, check_lam=True)
    _selection(native, dev, name, got, ref)
    lam = gc.carried_lam(name)
    assert np.abs(lam[:, :, gc.row_slice(gc.case_inputs(name)[0], gc.CASES[name].kind)]).max() > 1e-6
    ref1 = gc.oracle_run(name, carried=True, sqp_iters=1)
    lit1 = gc.oracle_run(name, literal=True, carried=True, sqp_iters=1)
    got1 = _gpu(native, dev, name, lam_in=lam, sqp_iters=1)
    _compare(name, f"{name} (b) 1 iteration, carried multipliers", ref1, lit1, got1, converged_only=True,
             lam_in=lam, sqp_iters=1)


@pytest.mark.parametrize("name", ["C2", "C1"])
def test_full_sqp(native, dev, oracle_mod, name):
    """(c) solver_type SQP: one full acados SQP call per solve, the FULL kernel variant"""
    ref = gc.oracle_run(name, solver_type="SQP")
    lit = gc.oracle_run(name, literal=True, solver_type="SQP")
    got = _gpu(native, dev, name, solver_type="SQP")
    assert (ref["sqp_iter"] > 1).any()
    _compare(name, f"{name} (c) solver_type SQP", ref, lit, got, solver_type="SQP")
