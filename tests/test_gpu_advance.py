"""The kernels that carry one control step into the next, each against a plain statement of its rule:
advance_kernel (mpcg_advance) against oracle/producers_oracle.py advance on every case of
advance_cases.py, select_best_kernel against selection.find_best_planner_host and
select_lowest_cost_kernel against scenario.select_lowest_cost on synthetic batches of more than two
64-thread blocks.

Everything mpcg_advance writes is a copy, a flag or a correctly rounded sum (mpcg_prepare.hip is
built without contraction), so the comparison is bit for bit; only the x and y columns of braking
plans (the device's cos / sin) get 1e-12.  The selection inputs are small multiples of 1/8 and the
weights 0.5 and 0.75, so every objective is exact whether or not the compiler fuses the consistency
sum, and the comparison is bit for bit too.
"""
import functools

import numpy as np
import pytest

import advance_cases as ac
from oscar_mpc_planner_mr_modification_amd.scenario import select_lowest_cost
from oscar_mpc_planner_mr_modification_amd.selection import find_best_planner_host


def _dev(a, dtype):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).to(device="cuda:0", dtype=dtype)   # (a copy: read-only inputs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ac.CASES))
def test_device_advance_matches_oracle(name):
    """every output is filled with NaN / 0xFF before the call, so an element the kernel leaves
    unwritten shows; no output may hold a NaN but prev_elapsed of the scenes without a feasible
    planner (advance_cases.assert_matches_reference)"""
    import torch
    from oscar_mpc_planner_mr_modification_amd import native

    c = ac.CASES[name]
    lay, i = ac.case_inputs(name)
    pr = native.problem_from_layout(lay)
    S, G, N, LS = c.S, c.G, lay.N, native.lam_stride(pr)
    f64, u8, i32 = torch.float64, torch.uint8, torch.int32
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=f64, device="cuda:0")  # noqa: E731
    ff = lambda *shape: torch.full(shape, 0xFF, dtype=u8, device="cuda:0")  # noqa: E731
    out = dict(main_warm=nan(S, N + 1, 7), prev_traj=nan(S, N, 2), prev_elapsed=torch.zeros(S, dtype=f64, device="cuda:0"),
               consistency_on=ff(S, G), previously_selected=ff(S, G), lam=nan(S * G, N, LS) if c.lam_next else None)
    got = native.advance_device(pr, S, G, _dev(i.best, i32), _dev(i.exit_code, i32), _dev(i.xtraj, f64),
                                _dev(i.utraj, f64), _dev(i.warm, f64), _dev(i.lam_out, f64), _dev(i.state_next, f64),
                                _dev(i.guided, u8), ac.ELAPSED, ac.DECELERATION, c.shift_forward,
                                c.consistency_on_non_guided, topology=_dev(i.topology, i32),
                                topology_next=_dev(i.topology_next, i32),
                                previously_selected=_dev(i.previously_selected, u8), out=out)
    torch.cuda.synchronize()
    assert got is out
    res = {k: None if v is None else v.cpu().numpy() for k, v in got.items()}
    if not c.lam_next:
        expected = None
    elif not c.lam_in:
        expected = np.zeros((S * G, N, LS))     # no multipliers in: the device writes zeros
    else:
        expected = "reference"
    ac.assert_matches_reference(name, res, ac.BRAKING_XY_ATOL_DEVICE, lam_expected=expected)


# ---------------------------------------------------------------------------------------------
# selection kernels
W_CONS, SEL_W = 0.5, 0.75
SPECIAL = ("two-way tie", "three-way tie", "none qualifies", "only success at 1e10", "only success just below 1e10")


@functools.lru_cache(maxsize=None)
def select_inputs(S, G, N, seed=5):
    """Synthetic select_best inputs, entries multiples of 1/8 (exact objectives).  With G 3 the scenes
    at 63, 64, 127, 128 and S - 1 (the ends of the 64-thread blocks and the tail) are, in SPECIAL's
    order: planners 1 and 2 tie below planner 0; all three tie (through the plain cost, the selection
    weight and the consistency term); every planner failed or disabled; the only success has
    objective exactly 1e10; the only success lies one ulp below 1e10."""
    rng = np.random.default_rng(seed)
    B = S * G
    eighth = lambda lo, hi, shape: rng.integers(lo, hi, shape) / 8.0  # noqa: E731
    d = dict(xtraj=eighth(-16, 17, (B, N + 1, 5)), prev=eighth(-16, 17, (S, N, 2)), pobj=eighth(0, 4096, B),
             exit=rng.choice(np.array([1, 0, 4], np.int32), size=B, p=(0.6, 0.2, 0.2)),
             cons=(rng.uniform(size=B) < 0.5).astype(np.uint8), psel=(rng.uniform(size=B) < 0.3).astype(np.uint8),
             dis=(rng.uniform(size=B) < 0.2).astype(np.uint8))
    where = {}
    if G == 3:
        where = dict(zip(SPECIAL, (63, 64, 127, 128, S - 1)))

        def acc(s, g):
            dxy = d["xtraj"][s * G + g, 1:N - 1, :2] - d["prev"][s, 1:N - 1]
            return float((dxy * dxy).sum())

        def put(s, pobj, exit_=(1, 1, 1), cons=(0, 0, 0), psel=(0, 0, 0), dis=(0, 0, 0)):
            sl = slice(s * G, s * G + G)
            d["pobj"][sl], d["exit"][sl], d["cons"][sl], d["psel"][sl], d["dis"][sl] = pobj, exit_, cons, psel, dis

        s = where["two-way tie"]
        put(s, (3.5, 3.0, 4.0), psel=(0, 0, 1))                      # 3.5 | 3.0 | 4.0 * 0.75
        s = where["three-way tie"]
        put(s, (3.0, 4.0, 3.0 + W_CONS * acc(s, 2)), cons=(0, 0, 1), psel=(0, 1, 0))
        s = where["none qualifies"]
        put(s, (1.0, 2.0, 3.0), exit_=(0, 1, 4), dis=(0, 1, 0))
        s = where["only success at 1e10"]
        put(s, (1.0, 1e10, 2.0), exit_=(0, 1, 4))
        s = where["only success just below 1e10"]
        put(s, (1.0, 2.0, np.nextafter(1e10, 0.0)), exit_=(4, 0, 1))
    for a in d.values():
        a.setflags(write=False)
    return d, where


def _host(S, G, N, d, prev=True, flags=True):
    return find_best_planner_host(S, G, N, d["xtraj"], d["pobj"], d["exit"], d["prev"] if prev else None, W_CONS,
                                  d["cons"] if flags else None, d["psel"] if flags else None, SEL_W,
                                  d["dis"] if flags else None)


def test_selection_cases_on_host():
    """the constructed scenes decide what they are meant to decide, on exact objectives"""
    S, G, N = 131, 3, 20
    d, where = select_inputs(S, G, N)
    best, obj = _host(S, G, N, d)
    obj = obj.reshape(S, G)
    s = where["two-way tie"]
    assert obj[s, 1] == obj[s, 2] == 3.0 < obj[s, 0] and best[s] == 1
    s = where["three-way tie"]
    assert obj[s, 0] == obj[s, 1] == obj[s, 2] == 3.0 and best[s] == 0 and d["pobj"][s * G + 2] > 3.0
    assert best[where["none qualifies"]] == -1 and best[where["only success at 1e10"]] == -1
    s = where["only success just below 1e10"]
    assert best[s] == 2 and obj[s, 2] < 1e10
    exact = np.delete(obj, s, 0)                           # (the scene one ulp below 1e10 aside)
    assert (exact * 512 == np.round(exact * 512)).all() and np.abs(exact).max() <= 1e10   # nothing was rounded
    rest = np.setdiff1d(np.arange(S), list(where.values()))
    assert set(best[rest].tolist()) == {-1, 0, 1, 2}
    for f in ("cons", "psel", "dis"):
        per_scene = d[f].reshape(S, G)[rest]
        assert ((per_scene.min(1) == 0) & (per_scene.max(1) == 1)).any(), f    # mixed within a scene


@pytest.mark.gpu
@pytest.mark.parametrize("S,G", [(131, 3), (2, 1)])
@pytest.mark.parametrize("variant", ["all flags", "no previous plan", "no objective out", "no flags"])
def test_device_select_best_matches_host(S, G, variant):
    import torch
    from oscar_mpc_planner_mr_modification_amd import native

    N = 20
    d, _ = select_inputs(S, G, N)
    prev, flags = variant != "no previous plan", variant != "no flags"
    ref_best, ref_obj = _host(S, G, N, d, prev=prev, flags=flags)
    f64, u8 = torch.float64, torch.uint8
    best, obj = native.select_best_device(
        S, G, N, _dev(d["xtraj"], f64), _dev(d["pobj"], f64), _dev(d["exit"], torch.int32),
        prev_traj=_dev(d["prev"], f64) if prev else None, w_cons=W_CONS,
        consistency_enabled=_dev(d["cons"], u8) if flags else None,
        previously_selected=_dev(d["psel"], u8) if flags else None, selection_weight=SEL_W,
        disabled=_dev(d["dis"], u8) if flags else None, with_objective=variant != "no objective out")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(best.cpu().numpy(), ref_best)
    if variant == "no objective out":
        assert obj is None
    else:
        np.testing.assert_array_equal(obj.cpu().numpy(), ref_obj)
    if variant == "no previous plan":     # flags given, no previous plan: no consistency term
        plain = d["pobj"] * np.where(d["psel"] > 0, SEL_W, 1.0)
        np.testing.assert_array_equal(ref_obj, plain)


@functools.lru_cache(maxsize=None)
def lowest_cost_inputs(S=131, P=4, seed=6):
    """pobj multiples of 1/8 in a narrow range (natural ties), and at 63, 64, 127, 128, S - 1: the two
    lowest successful costs tie; all four tie; every copy failed; the only success costs exactly 1e9;
    the only success costs one ulp less"""
    rng = np.random.default_rng(seed)
    pobj = rng.integers(0, 24, (S, P)) / 8.0
    ex = rng.choice(np.array([1, 0, 4], np.int32), size=(S, P), p=(0.6, 0.2, 0.2))
    pobj[63], ex[63] = (5.0, 2.0, 7.0, 2.0), (1, 1, 1, 1)
    pobj[64], ex[64] = (2.5, 2.5, 2.5, 2.5), (0, 1, 1, 1)
    ex[127] = (0, 4, 0, 4)
    pobj[128], ex[128] = (1.0, 2.0, 1e9, 3.0), (0, 4, 1, 0)
    pobj[S - 1], ex[S - 1] = (1.0, 2.0, 3.0, np.nextafter(1e9, 0.0)), (0, 4, 0, 1)
    return pobj.reshape(-1), ex.reshape(-1)


def test_lowest_cost_cases_on_host():
    S, P = 131, 4
    pobj, ex = lowest_cost_inputs()
    best = select_lowest_cost(pobj, ex, P)
    assert (best[63], best[64], best[127], best[128], best[S - 1]) == (1, 1, -1, -1, 3)
    po, ok = pobj.reshape(S, P), ex.reshape(S, P) == 1
    low = np.where(ok, po, np.inf).min(1)
    ties = ((po == low[:, None]) & ok).sum(1) >= 2
    assert ties.sum() >= 5 and (best == -1).sum() >= 2


@pytest.mark.gpu
def test_device_select_lowest_cost_matches_host():
    import torch
    from oscar_mpc_planner_mr_modification_amd import native

    S, P = 131, 4
    pobj, ex = lowest_cost_inputs()
    out = torch.full((S,), -7, dtype=torch.int32, device="cuda:0")
    best = native.select_lowest_cost_device(S, P, _dev(pobj, torch.float64), _dev(ex, torch.int32), out=out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(best.cpu().numpy(), select_lowest_cost(pobj, ex, P))
