"""GPU against the oracle with the box bounds binding, on every family of the kernel's slot map
(tests/bound_cases.py; tests/test_bound_inputs.py shows on the oracle alone that these inputs make
every bound class bind in successful solves of every family).

The kernel gives a lane a lower and an upper row per variable (slots 2j, 2j + 1 <-> variable
part + PARTS j; LaneRows::box_on: inputs on stages 0..N-1, states on 1..N-1).  Those rows feed the
barrier diagonal, the per-variable sums, the step length, the qp_t_min floor and the FULL variant's
QP memory.  With the models' own bounds they almost never bind on the generators' batches, so a
wrong slot-to-variable map for one variable of one family, an upper row read as a lower one, a stage
rule off by one at k = 0 or k = N - 1, or an error in how a box row limits the step moves nothing the
other parity tests see.  Here the same lb / ub options go to native.problem_from_layout and to the
oracle:

  (a) every case: 10 SQP-RTI iterations (the lean HPIPM kernels), trajectories and multipliers;
  (b) every case: one iteration from the oracle's carried multipliers of (a);
  (c) C2brake, C1brake: solver_type SQP (the FULL variant with the run-time profile);
  (d) C2, JS: qp_profile robust (the lean PROF_ROBUST kernels, whose qp_t_min floor acts on these rows);
  (e) C2, C4: two consecutive solves with the QP memory carried and qp_warm_first = 1: the second
      solve's first QP starts from the stored slacks and multipliers of the box rows;
  (f) C2, C5: the stats buffer (stationarity, dynamics, inequality violation, complementarity)
      against the oracle's residuals, the one place the box multipliers are exported.

Bars: geometry_cases.compare_with_oracle's own -- equal exit codes and SQP iteration counts;
max|dx|, max|du| <= max(1e-9, 100 x the oracle builds' spread), below the north-star 1e-4; pobj
within 1e-6 relative; in (a) and (b) the multipliers within 1e-6 of their largest; at most one solve
per batch accepted, and only where the oracle's own one-ulp runs or its literal build part.  In (e)
no solve is accepted (the one-ulp runs do not take QP memory).  (f): the tolerances of
test_nlp_residual_stats (rtol 1e-6, atol 1e-9) on every solve, failed ones included; a solve on
which the oracle's own two builds miss that tolerance against each other is rounding-decided and
left out, at most one per batch (C5 solve 47: its QP iteration counts differ between the builds).

Measured on an MI355X against the default build (max|dx| / max|du| / multipliers relative to their
largest / the oracle builds' spread); every exit code and SQP iteration count agrees, no solve was
accepted as rounding-decided in (a) - (e), and the GPU's results hold the same binding rows per
bound class as the oracle's (the counts of test_bound_inputs.py):

             (a) 10 RTI iterations                      (b) one iteration, carried multipliers
  C2       5.4e-14 / 2.5e-14 / 7.1e-14 / 2.0e-14     2.5e-14 / 3.7e-14 / 2.9e-14 / 2.0e-13
  C2brake  4.9e-15 / 1.5e-14 / 1.2e-13 / 3.8e-14     6.0e-14 / 7.9e-14 / 2.1e-15 / 3.2e-14
  C1       1.0e-14 / 5.5e-14 / 1.1e-13 / 9.6e-14     8.9e-14 / 1.2e-13 / 1.4e-14 / 3.0e-14
  C1brake  5.3e-15 / 2.3e-15 / 6.5e-15 / 3.6e-15     7.7e-14 / 1.0e-13 / 1.1e-14 / 6.7e-14
  T10      3.6e-15 / 1.7e-15 / 9.6e-16 / 2.7e-15     7.1e-15 / 9.3e-15 / 7.4e-15 / 2.7e-15
  C4       5.3e-12 / 2.5e-12 / 1.1e-12 / 1.4e-12     5.9e-14 / 1.9e-13 / 5.4e-13 / 2.3e-13
  JS       4.4e-13 / 1.7e-13 / 4.7e-14 / 3.2e-14     5.4e-14 / 1.4e-13 / 1.1e-13 / 5.1e-14
  C4brake  7.4e-14 / 1.1e-13 / 1.3e-13 / 2.3e-13     8.8e-14 / 6.3e-13 / 5.7e-13 / 1.3e-12
  C5       1.9e-09 / 3.8e-10 / 5.8e-13 / 1.9e-09     2.6e-14 / 6.9e-14 / 3.6e-13 / 9.4e-14
  C5N10    3.3e-15 / 3.5e-15 / 1.5e-13 / 3.2e-15     3.2e-15 / 7.1e-15 / 7.3e-13 / 4.0e-15
  C5brake  5.3e-14 / 6.5e-14 / 9.3e-14 / 4.1e-14     3.9e-14 / 2.4e-14 / 8.2e-14 / 4.6e-14
  C3       6.1e-14 / 1.9e-14 / 2.3e-14 / 8.9e-15     3.9e-13 / 9.1e-14 / 3.4e-14 / 2.6e-13
  C3N10    1.8e-15 / 2.7e-15 / 3.0e-15 / 1.8e-15     2.2e-15 / 4.4e-15 / 1.4e-15 / 4.4e-16
  C3brake  5.3e-15 / 4.1e-15 / 2.9e-15 / 3.6e-15     1.1e-14 / 8.3e-14 / 1.4e-15 / 1.6e-13
  (c) full SQP         C2brake 1.2e-14 / 5.2e-14 / 1.2e-13 / 1.4e-14, C1brake 1.9e-13 / 7.8e-14 / 1.6e-13 / 1.1e-13
  (d) robust profile   C2 8.3e-14 / 1.9e-13 / 7.7e-14 / 1.6e-13, JS 1.2e-13 / 4.4e-14 / 1.5e-14 / 6.8e-13
  (e) second solve     C2 6.2e-14 / 4.4e-14 / 5.9e-14 / 4.6e-14, C4 2.5e-13 / 2.5e-13 / 6.5e-14 / 4.8e-14
      (the first: C2 2.3e-14 / 1.9e-14 / 3.0e-14 / 3.4e-14, C4 3.4e-12 / 1.6e-12 / 1.1e-12 / 9.1e-13)
  (f) stats            C2 within 9.1e-5 of the tolerance on all 64 solves; C5 within 0.41 of it on 47 solves,
      solve 47 left out (there the GPU misses the default build's stationarity as the literal build does)

C5 (a): the 1.9e-9 equals the builds' own spread, which is solve 47 (test_bound_inputs.py).
"""
import numpy as np
import pytest

import bound_cases as bc

pytestmark = pytest.mark.gpu

STATS_RTOL, STATS_ATOL = 1e-6, 1e-9   # test_nlp_residual_stats


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from oscar_mpc_planner_mr_modification_amd import native as nat
    return nat


def _gpu(native, dev, name, lam_in=None, qp_in=None, qp_out=False, stats=False, **opts):
    import torch
    lay, b, lb, ub = bc.case_inputs(name)
    pr = native.problem_from_layout(lay, lb=lb, ub=ub, **opts)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731  (a copy: the shared inputs are read-only)
    out = native.solve_batch_device(pr, t(b.params), t(b.warm), t(b.xinit),
                                    lam_in=None if lam_in is None else t(lam_in), lam_out=True,
                                    qp_in=qp_in, qp_out=qp_out, stats=stats)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if k != "qp"}
    return (got, out["qp"]) if qp_out else got


def _binding(name, label, ref, got):
    """the compared solves hold binding box rows, on the GPU's result as on the oracle's"""
    lay, _, lb, ub = bc.case_inputs(name)
    ok = (got["exit"] == 1) & (ref["status"] == 1)
    a = bc.active_rows(lay, lb, ub, ref, ok, show=f"{label}, oracle")
    g = bc.active_rows(lay, lb, ub, got, ok, show=f"{label}, gpu")
    assert sum(a.values()) > 0 and sum(g.values()) > 0


@pytest.mark.parametrize("name", list(bc.CASES))
def test_rti_and_carried_multipliers(native, dev, oracle_mod, name):
    """(a) 10 RTI iterations with trajectories and multipliers; (b) one iteration from the oracle's
    carried multipliers of (a), zeroed for failed solves."""
    ref, lit = bc.oracle_run(name), bc.oracle_run(name, literal=True)
    got = _gpu(native, dev, name)
    label = f"{name} (a) 10 RTI iterations"
    bc.compare_with_oracle(label, ref, lit, got, scatter=bc.scatter_of(name), check_lam=True)
    _binding(name, label, ref, got)
    lam = bc.carried_lam(name)
    ref1 = bc.oracle_run(name, carried=True, sqp_iters=1)
    lit1 = bc.oracle_run(name, literal=True, carried=True, sqp_iters=1)
    got1 = _gpu(native, dev, name, lam_in=lam, sqp_iters=1)
    bc.compare_with_oracle(f"{name} (b) 1 iteration, carried multipliers", ref1, lit1, got1,
                           scatter=bc.scatter_of(name, lam_in=lam, sqp_iters=1), converged_only=True, check_lam=True)


@pytest.mark.parametrize("name", ["C2brake", "C1brake"])
def test_full_sqp(native, dev, oracle_mod, name):
    """(c) solver_type SQP: one full acados SQP call per solve, the FULL kernel variant"""
    ref = bc.oracle_run(name, solver_type="SQP")
    lit = bc.oracle_run(name, literal=True, solver_type="SQP")
    got = _gpu(native, dev, name, solver_type="SQP")
    assert (ref["sqp_iter"] > 1).any()
    label = f"{name} (c) solver_type SQP"
    bc.compare_with_oracle(label, ref, lit, got, scatter=bc.scatter_of(name, solver_type="SQP"))
    _binding(name, label, ref, got)


@pytest.mark.parametrize("name", ["C2", "JS"])
def test_robust_profile(native, dev, oracle_mod, name):
    """(d) qp_profile robust on both sides: the qp_t_min floor of 1e-12 acts on the binding rows"""
    ref = bc.oracle_run(name, qp_profile="robust")
    lit = bc.oracle_run(name, literal=True, qp_profile="robust")
    got = _gpu(native, dev, name, qp_profile="robust")
    label = f"{name} (d) qp_profile robust"
    bc.compare_with_oracle(label, ref, lit, got, scatter=bc.scatter_of(name, qp_profile="robust"))
    _binding(name, label, ref, got)


@pytest.mark.parametrize("name", ["C2", "C4"])
def test_qp_memory_carried_between_solves(native, dev, oracle_mod, name):
    """(e) the second of two solves starts its first QP from the QP memory the first one left (each
    side in its own opaque layout; failed solves: memory marked absent, zero multipliers)"""
    import torch
    m = bc.oracle_qp_memory(name)
    none = lambda i: (False, 0.0)  # noqa: E731  (no oracle-side evidence with QP memory: no solve may part)
    got1, q_gpu = _gpu(native, dev, name, qp_out=True, **bc.QP_MEMORY)
    bc.compare_with_oracle(f"{name} (e) first solve, qp_warm_first", m["first"], m["first_literal"], got1,
                           scatter=bc.scatter_of(name, **bc.QP_MEMORY))
    ok = m["first"]["status"] == 1
    q_gpu = q_gpu.clone()
    q_gpu[torch.from_numpy(~ok).to(dev), 0] = float("nan")
    got2 = _gpu(native, dev, name, lam_in=m["lam"], qp_in=q_gpu, **bc.QP_MEMORY)
    label = f"{name} (e) second solve, QP memory carried"
    bc.compare_with_oracle(label, m["second"], m["second_literal"], got2, scatter=none)
    _binding(name, label, m["second"], got2)
    # the stored start matters: without the QP memory the second solve's QPs take other iteration counts
    assert not np.array_equal(m["cold"]["qp_iter"][ok], m["second"]["qp_iter"][ok])


@pytest.mark.parametrize("name", ["C2", "C5"])
def test_nlp_residual_stats(native, dev, oracle_mod, name):
    """(f) mpcg_io.stats == the oracle's NLP residuals at the last linearisation point"""
    ref, lit = bc.oracle_run(name), bc.oracle_run(name, literal=True)
    got = _gpu(native, dev, name, stats=True)
    assert np.array_equal(got["exit"], ref["status"]) and np.array_equal(got["info"][:, 0], ref["sqp_iter"])
    cols = lambda r: np.stack([r["res_stat"], r["res_eq"], r["res_ineq"], r["res_comp"]], 1)  # noqa: E731
    want, other, st = cols(ref), cols(lit), got["stats"]
    assert (st >= 0).all() and np.isfinite(st).all()
    miss = lambda a: (np.abs(a - want) > STATS_ATOL + STATS_RTOL * np.abs(want)).any(1)  # noqa: E731
    decided = miss(other)      # the oracle's own builds part on these solves
    rel = np.abs(st - want) / (STATS_ATOL / STATS_RTOL + np.abs(want))
    print(f"{name} (f) stats: {len(st)} solves, largest distance in units of the tolerance "
          f"{rel[~decided].max() / STATS_RTOL:.2e}, rounding-decided on the oracle {np.flatnonzero(decided)} "
          f"(gpu misses there: {miss(st)[decided]}), largest res_comp {want[:, 3].max():.2e}")
    assert decided.sum() <= 1
    np.testing.assert_allclose(st[~decided], want[~decided], rtol=STATS_RTOL, atol=STATS_ATOL)
