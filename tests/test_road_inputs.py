"""The inputs of tests/test_gpu_road.py have not degenerated (oracle only, no GPU).

road_cases.PARITY puts the two road rows into synthetic.make_batch scenes.  The GPU comparison can only
notice an error in how the kernel treats those rows while they bind in successful solves, and while
the oracle's two arithmetic builds agree on every exit code and far below the bound the comparison
applies.  The success share is far below the usual 0.9 by design -- a guess that passes an obstacle
outside the road has no feasible plan any more --, so no share is asked for: per case at least 16
solves successful in both builds and, except at the shipped width 6.0, at least 6 of them with a road
row within 1e-4 of active.

Measured on the committed cases (the test prints them; successful in both builds / solves, with an
active road row, default-to-literal distance of trajectories and of multipliers relative to the
largest):

    C2R-W2.5-twoway   44/64   11   2.8e-14  6.9e-14      robust profile 44/64, 9, 7.1e-14;  SQP 44/64, 11, 3.3e-13
    C2R-W1.6          22/64   16   1.4e-14  2.1e-14
    C2R-W6.0          44/64    4   1.3e-13  2.2e-13
    JSR-W2.5          21/40   14   1.0e-13  1.8e-13

The closed loop of road_cases.LOOP (C2R, 4 x 8, W 2.5 two-way, 3 steps): both builds give the same
exit codes, winners and closest segments at every step (24 of 32 solves successful per step, the
builds 3.1e-13 apart, road rows active in 3 successful solves of the run).
"""
import copy

import numpy as np
import pytest

import road_cases as rc

EXTRA = "C2R-W2.5-twoway"     # the case of the FULL-variant, full-SQP and robust-profile runs


def _both(name, **opts):
    d, lit = rc.oracle_run(name, **opts), rc.oracle_run(name, literal=True, **opts)
    return d, lit, (d["status"] == 1) & (lit["status"] == 1)


def _check(name, label, **opts):
    d, lit, both = _both(name, **opts)
    act = rc.active_solves(name, d, both)
    sp = rc.spread(d, lit, both)
    lsp = rc.lam_spread(d, lit, both)
    gaps = rc.road_gaps(name, d["xtraj"])[both]
    print(f"{label}: successful in both builds {both.sum()}/{len(both)}, with an active road row {act.sum()}, "
          f"build-to-build distance x/u {sp:.2e}, multipliers {lsp:.2e}, smallest road gap {gaps.min():.2e}")
    assert np.array_equal(d["status"], lit["status"]), f"{label}: the builds part on an exit code: choose another seed"
    assert both.sum() >= rc.MIN_SOLVES
    if name in rc.NEEDS_ACTIVE:
        assert act.sum() >= rc.MIN_ACTIVE
    # a successful solve respects its road rows
    assert gaps.min() >= -1e-6
    assert max(rc.ROUNDING, rc.MARGIN * sp) <= rc.X_TOL
    return d, both, act


@pytest.mark.parametrize("name", list(rc.PARITY))
def test_road_rows_bind_and_the_builds_agree(oracle_mod, name):
    _check(name, name)


def test_rows_are_where_the_reference_puts_them(oracle_mod):
    """guided planners carry the road rows after their obstacle rows, the non-guided one first"""
    lay, b, hs, guided = rc.parity_inputs("C2R-W1.6")
    S, G = guided.shape
    l0, mo = lay.idx("lin_constraint_0_a1"), lay.max_obstacles
    P = b.params.reshape(S, G, lay.N, lay.npar)
    assert guided[:, :G - 1].all() and not guided[:, G - 1].any()
    np.testing.assert_array_equal(P[:, 0, 1:, l0 + 3 * mo:l0 + 3 * mo + 6], hs[:, 1:].reshape(S, lay.N - 1, 6))
    np.testing.assert_array_equal(P[:, G - 1, 1:, l0:l0 + 6], hs[:, 1:].reshape(S, lay.N - 1, 6))
    assert (P[:, :, 0, l0:l0 + 3 * lay.n_lin].reshape(S, G, -1, 3)[..., :2] == (1.0, 0.0)).all()


@pytest.mark.parametrize("opts", [dict(qp_profile="robust"), dict(solver_type="SQP")], ids=["robust", "sqp"])
def test_extra_runs_have_something_to_compare(oracle_mod, opts):
    d, both, act = _check(EXTRA, f"{EXTRA} {opts}", **opts)
    if "solver_type" in opts:
        assert (d["sqp_iter"][both] > 1).any()


def test_closed_loop_is_not_decided_by_rounding(oracle_mod):
    """the CPU loop of road_cases.LOOP in both oracle builds: equal exit codes, winners and closest segments
    on every step, trajectories within 1e-9; road rows bind in some successful solve of the run"""
    import producers_oracle
    case = rc.loop_case()
    loops = [rc.RoadCpuLoop(case, copy.deepcopy(case["scenes"]), oracle_mod, producers_oracle, literal=lit)
             for lit in (False, True)]
    dist, active = 0.0, 0
    for t in range(rc.LOOP["steps"]):
        ha, hb = (lp.step() for lp in loops)
        np.testing.assert_array_equal(ha["exit"], hb["exit"], err_msg=f"step {t}")
        np.testing.assert_array_equal(ha["best"], hb["best"], err_msg=f"step {t}")
        np.testing.assert_array_equal(ha["closest_segment"], hb["closest_segment"], err_msg=f"step {t}")
        ok = ha["exit"] == 1
        assert ok.any()
        dist = max(dist, float(np.abs(ha["xtraj"][ok] - hb["xtraj"][ok]).max()))
        hs = ha["halfspaces"]
        rows = np.repeat(hs[:, None], case["G"], 1).reshape(-1, case["lay"].N, 2, 3)[:, 1:]
        p = ha["xtraj"][:, 1:case["lay"].N, 0:2]
        gap = rows[..., 2] - (rows[..., 0] * p[:, :, None, 0] + rows[..., 1] * p[:, :, None, 1])
        active += int(((gap <= rc.ACTIVE).any((1, 2)) & ok).sum())
        print(f"step {t}: successful {int(ok.sum())}/{len(ok)}, winners {ha['best'].tolist()}, segments "
              f"{ha['closest_segment'].tolist()}, active road rows in {active} solves so far, "
              f"default-to-literal distance so far {dist:.2e}")
        for lp, h in zip(loops, (ha, hb)):
            lp.advance(h["best"])
    assert dist <= 1e-9
    assert active >= 1
    assert (np.array([h for h in ha["best"]]) >= 0).any()
