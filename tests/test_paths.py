"""Reference-path tracking on the host (paths.py) and its C ABI (include/mpcg_path.h): the spline
fit, the closest-point search against known answers, the segment window, the goal test, the
command, the CPU reference loop of tests/test_gpu_paths.py, and the library's exports.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import path_cases as pc
from oscar_mpc_planner_mr_modification_amd import paths
from oscar_mpc_planner_mr_modification_amd.layouts import config_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oscar_mpc_planner_mr_modification_amd", "libmpcg.so")
HDR = os.path.join(ROOT, "include", "mpcg_path.h")
SHRINK = (2.0 / 63.0) ** 5


# ------------------------------------------------------------------ fit_path


def _derivatives(path, j, t):
    c = path["coef"][j].reshape(2, 4)
    return (c[:, 0] * t + c[:, 1]) * t * t + c[:, 2] * t + c[:, 3], (3 * c[:, 0] * t + 2 * c[:, 1]) * t + c[:, 2], \
        6 * c[:, 0] * t + 2 * c[:, 1]


def test_fit_of_collinear_equally_spaced_waypoints_is_a_line():
    d = np.array([0.6, -0.8])
    pts = np.array([1.0, 2.0])[None] + 1.5 * np.arange(7)[:, None] * d[None]
    p = paths.fit_path(pts[:, 0], pts[:, 1])
    np.testing.assert_allclose(p["knots"], 1.5 * np.arange(7), rtol=0, atol=1e-12)
    c = p["coef"].reshape(6, 2, 4)
    assert np.abs(c[:, :, 0]).max() <= 1e-12 and np.abs(c[:, :, 1]).max() <= 1e-12
    np.testing.assert_allclose(c[:, :, 2], np.tile(d, (6, 1)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(c[:, :, 3], pts[:6], rtol=0, atol=1e-12)


def test_fit_interpolates_and_is_twice_continuously_differentiable():
    rng = np.random.default_rng(7)
    x, y = np.cumsum(rng.uniform(0.5, 2.0, 9)), np.cumsum(rng.normal(0.0, 0.7, 9))
    p = paths.fit_path(x, y)
    K, m = p["knots"], 8
    np.testing.assert_allclose(np.diff(K), np.hypot(np.diff(x), np.diff(y)), rtol=0, atol=1e-12)   # chord length
    for j in range(m):
        p0, _, _ = _derivatives(p, j, 0.0)
        p1, d1, dd1 = _derivatives(p, j, K[j + 1] - K[j])
        np.testing.assert_allclose(p0, [x[j], y[j]], rtol=0, atol=1e-12)
        np.testing.assert_allclose(p1, [x[j + 1], y[j + 1]], rtol=0, atol=1e-12)
        if j < m - 1:
            _, d0n, dd0n = _derivatives(p, j + 1, 0.0)
            np.testing.assert_allclose(d1, d0n, rtol=0, atol=1e-12)
            np.testing.assert_allclose(dd1, dd0n, rtol=0, atol=1e-12)
    assert np.abs(_derivatives(p, 0, 0.0)[2]).max() <= 1e-12
    assert np.abs(_derivatives(p, m - 1, K[m] - K[m - 1])[2]).max() <= 1e-12


def test_fit_uses_a_supplied_parameter_as_given():
    x, y = np.array([0.0, 1.0, 2.5, 3.0]), np.array([0.0, 0.5, 0.2, 1.0])
    s = np.array([2.0, 3.5, 7.0, 7.25])
    p = paths.fit_path(x, y, s)
    np.testing.assert_array_equal(p["knots"], s)
    for j in range(3):
        np.testing.assert_allclose(_derivatives(p, j, s[j + 1] - s[j])[0], [x[j + 1], y[j + 1]], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        paths.fit_path(x, y, np.array([0.0, 1.0, 1.0, 2.0]))


# ------------------------------------------------------------------ closest point


def test_closest_point_recovers_known_answers_within_the_shrink_bound():
    """300 synthetic paths (synthetic._path(rng, 12); its first 11 segments, the twelfth supplying the
    end knot), q = p(s*) + d n(s*) with |d| <= 1, searched over the +-2 segments of the segment that
    holds s*: |closest_s - s*| <= W (2/63)^5 with W the interval's length."""
    worst, worst_bound = 0.0, 0.0
    for seed in range(300):
        path = pc.synthetic_path(1000 + seed, 11)
        K, m = path["knots"], 11
        rng = np.random.default_rng(seed)
        s_true = rng.uniform(K[0] + 0.05, K[m] - 0.05)
        c = int(np.searchsorted(K[:m], s_true, side="right") - 1)
        pos, _, nrm = pc.eval_path(path, s_true)
        q = pos + rng.uniform(-1.0, 1.0) * nrm
        W = K[min(m, c + 3)] - K[max(0, c - 2)]
        cs, seg = paths.closest_point_host(path["coef"], K, m, q, c)
        err = abs(cs - s_true)
        worst, worst_bound = max(worst, err), max(worst_bound, W * SHRINK)
        assert err <= W * SHRINK, (seed, err, W * SHRINK)
        assert K[seg] <= cs and (seg == m - 1 or cs < K[seg + 1])
    print(f"largest error {worst:.2e}, largest bound {worst_bound:.2e}")


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_uninitialised_search_covers_the_whole_path(seed):
    path = pc.synthetic_path(2000 + seed, 11)
    K, m = path["knots"], 11
    rng = np.random.default_rng(seed)
    s_true = rng.uniform(K[8], K[m] - 0.05)            # far from segment 0
    pos, _, nrm = pc.eval_path(path, s_true)
    cs, seg = paths.closest_point_host(path["coef"], K, m, pos + 0.5 * nrm, -1)
    c = int(np.searchsorted(K[:m], s_true, side="right") - 1)
    # the first round's bracket is two sample steps of one segment
    assert abs(cs - s_true) <= np.diff(K).max() * SHRINK
    assert seg == c


def test_points_before_the_start_and_beyond_the_end():
    path = pc.synthetic_path(31, 11)
    K, m = path["knots"], 11
    p0, t0, n0 = pc.eval_path(path, K[0])
    for c in (0, -1):
        cs, seg = paths.closest_point_host(path["coef"], K, m, p0 - 0.7 * t0 + 0.2 * n0, c)
        assert cs == K[0] and seg == 0
    pe, te, ne = pc.eval_path(path, K[m])
    for c in (m - 1, -1):
        cs, seg = paths.closest_point_host(path["coef"], K, m, pe + 0.9 * te - 0.1 * ne, c)
        assert abs(cs - K[m]) <= (K[m] - K[m - 3]) * SHRINK and cs <= K[m] and seg == m - 1


# ------------------------------------------------------------------ segment, window, reached


def _update(path_list, q, c, n_seg=5, i0=3, npar=60, path_of=None):
    table = paths.PathTable.from_paths(path_list)
    S = len(q)
    state = np.zeros((S, 5))
    state[:, 0:2] = q
    sp = np.full((S, npar), 7.5)
    po = np.zeros(S, np.int32) if path_of is None else path_of
    out = paths.path_update_host(state, np.asarray(c, np.int32), table, po, sp, i0, n_seg)
    assert (np.delete(out["stage_params"], np.arange(i0, i0 + 9 * n_seg), axis=1) == 7.5).all()
    return table, out, out["stage_params"][:, i0:i0 + 9 * n_seg].reshape(S, n_seg, 9)


def test_window_is_the_table_rows_from_the_closest_segment():
    path = pc.synthetic_path(41, 11)
    K = path["knots"]
    q = [pc.eval_path(path, K[3] + 0.5)[0], pc.eval_path(path, K[6] + 1.0)[0] + 0.3 * pc.eval_path(path, K[6] + 1.0)[2]]
    _, out, win = _update([path, pc.synthetic_path(42, 4)], q, [2, 5])
    assert out["closest_segment"].tolist() == [3, 6]
    for s, c in enumerate((3, 6)):
        np.testing.assert_array_equal(win[s, :, :8], path["coef"][c:c + 5])
        np.testing.assert_array_equal(win[s, :, 8], K[c:c + 5])


def test_window_past_the_end_holds_the_end_point():
    path = pc.synthetic_path(43, 11)
    K, m = path["knots"], 11
    q = [pc.eval_path(path, K[m - 2] + 0.4)[0]]
    table, out, win = _update([path], q, [m - 3])
    assert out["closest_segment"].tolist() == [m - 2]
    np.testing.assert_array_equal(win[0, :2, :8], path["coef"][m - 2:])
    np.testing.assert_array_equal(win[0, :2, 8], K[m - 2:m])
    end = table.point(0, K[m])
    np.testing.assert_allclose(end, pc.eval_path(path, K[m])[0], rtol=0, atol=1e-12)
    for i in (2, 3, 4):
        np.testing.assert_array_equal(win[0, i], [0, 0, 0, end[0], 0, 0, 0, end[1], K[m]])


def test_reached_on_either_side_of_the_radius():
    path = pc.synthetic_path(44, 6)
    K, m = path["knots"], 6
    pe, te, ne = pc.eval_path(path, K[m])
    q = [pe - 1.4 * te, pe - 1.6 * te, pe + 1.49 * ne, pe + 1.51 * ne, pe]
    _, out, _ = _update([path], q, [m - 1] * 5)
    assert out["reached"].tolist() == [1, 0, 1, 0, 1]


def test_update_rejects_a_path_index_outside_the_table():
    with pytest.raises(ValueError):
        _update([pc.synthetic_path(45, 4)], [np.zeros(2)], [0], path_of=np.array([1], np.int32))


def test_the_gpu_update_inputs_take_every_case():
    """pc.update_case on the host: the segments and goal flags the GPU test's scenes are meant to give,
    the point on a knot within the shrink bound of it, the window past the end of the long path."""
    lay = config_layout("C2")
    c = pc.update_case(lay)
    i0 = lay.idx("spline_x0_a")
    first = paths.path_update_host(c["state"][0], c["closest_segment"], c["table"], c["path_of"], c["stage_params"], i0,
                                   lay.n_seg)
    second = paths.path_update_host(c["state"][1], first["closest_segment"], c["table"], c["path_of"],
                                    first["stage_params"], i0, lay.n_seg)
    pc.assert_update_case(first, second)
    K1, K2 = c["paths"][1]["knots"], c["paths"][2]["knots"]
    assert abs(first["closest_s"][1] - K1[5]) <= (K1[7] - K1[2]) * SHRINK
    assert first["closest_s"][5] == K1[0]
    win = second["stage_params"][6, i0:i0 + 9 * lay.n_seg].reshape(lay.n_seg, 9)
    np.testing.assert_array_equal(win[0, :8], c["paths"][2]["coef"][63])
    assert (win[1:, 8] == K2[64]).all() and (win[1:, [0, 1, 2, 4, 5, 6]] == 0.0).all()


# ------------------------------------------------------------------ command


def test_command_by_hand():
    c = pc.command_case()
    st = paths.PathSettings(control_frequency=20.0, deceleration=3.0, plant=True)
    out = paths.command_host(c["best"], c["xtraj"], c["utraj"], c["state"], st, c["closest_s"], 4)
    G, x = c["G"], c["state"]
    # success: v of the winner's stage 1, w of its stage 0
    for s, b in ((0, 0), (1, 2), (4, 1)):
        assert out["cmd"][s].tolist() == [c["xtraj"][s * G + b, 1, 3], c["utraj"][s * G + b, 0, 1]]
    # failure: v - 3 / 20, not below zero (scene 3: 0.05 < 0.15), no rotation
    assert out["cmd"][2].tolist() == [1.7 - 3.0 * (1.0 / 20.0), 0.0]
    assert out["cmd"][3].tolist() == [0.0, 0.0]
    # the stand-in plant over 0.05 s
    v, w = out["cmd"][:, 0], out["cmd"][:, 1]
    np.testing.assert_allclose(out["state_next"][:, 0], x[:, 0] + v * np.cos(x[:, 2]) * 0.05, rtol=0, atol=1e-15)
    np.testing.assert_allclose(out["state_next"][:, 1], x[:, 1] + v * np.sin(x[:, 2]) * 0.05, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(out["state_next"][:, 2], x[:, 2] + w * 0.05)
    np.testing.assert_array_equal(out["state_next"][:, 3], v)
    np.testing.assert_array_equal(out["state_next"][:, 4], c["closest_s"])
    off = paths.command_host(c["best"], c["xtraj"], c["utraj"], c["state"], paths.PathSettings(plant=False))
    assert off["state_next"] is None
    np.testing.assert_array_equal(off["cmd"], out["cmd"])


# ------------------------------------------------------------------ the CPU loop of the GPU test


@pytest.mark.parametrize("name", ["C2", "C1"])
def test_cpu_path_loop_moves_the_window(oracle_mod, name):
    """The CPU reference loop of tests/test_gpu_paths.py on its own: the seeds of pc.LOOP_CASES give
    scenes whose closest segment changes within the four steps, away from every knot."""
    import copy

    import producers_oracle
    case = pc.loop_case(name)
    loop = pc.PathCpuLoop(case, copy.deepcopy(case["scenes"]), oracle_mod, producers_oracle)
    hist = []
    for _ in range(4):
        h = loop.step()
        hist.append(h)
        loop.advance(h["best"])
    pc.assert_cpu_loop_moves_the_window(case, hist)
    assert any((h["exit"] == 1).any() for h in hist)
    # step t's xinit carries closest_s(t - 1) in the spline entry
    np.testing.assert_array_equal(hist[0]["xinit_spline"], case["scenes"].state[:, pc.SPLINE_SLOT])
    for t in (1, 2, 3):
        np.testing.assert_array_equal(hist[t]["xinit_spline"], hist[t - 1]["closest_s"])
    print(name, [h["closest_segment"].tolist() for h in hist])


# ------------------------------------------------------------------ C ABI


def test_python_binding_lists_the_path_symbols_and_mirrors_the_header():
    """(the functions: tests/test_layer_abi.py)"""
    from oscar_mpc_planner_mr_modification_amd import native_spec as ns
    raw = open(HDR).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, mirror in (("mpcg_path_table", ns.MpcgPathTable), ("mpcg_path_settings", ns.MpcgPathSettings)):
        body = txt[txt.index(f"typedef struct {struct} {{"):txt.index(f"}} {struct};")]
        names = []
        for decl in re.findall(r"(?:const\s+)?(?:int|double)\s+([^;]+);", body):
            names += [p.replace("*", "").strip() for p in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], struct
    macros = dict(re.findall(r"#define (MPCG_PATH_\w+) ([\d.]+)", raw))
    assert (int(macros["MPCG_PATH_MAX_SEGMENTS"]), int(macros["MPCG_PATH_SAMPLES"]), int(macros["MPCG_PATH_ROUNDS"]),
            float(macros["MPCG_PATH_REACHED_RADIUS"])) == (ns.PATH_MAX_SEGMENTS, ns.PATH_SAMPLES, ns.PATH_ROUNDS,
                                                           ns.PATH_REACHED_RADIUS)


def test_path_sources_are_linked_outside_the_source_hash():
    from oscar_mpc_planner_mr_modification_amd import _build
    assert _build.LAYERS["mpcg_path.h"] == {"sources": {"mpcg_path.hip": ["-ffp-contract=off"]},
                                            "headers": ["mpcg_path.h"]}
    assert "mpcg_path.hip" not in _build.SOURCES and "mpcg_path.h" not in _build.HEADERS


def test_bad_arguments_are_reported_without_a_launch():
    """Every error return of the two entry points (host-side checks only; the pointers are never read
    on the device)."""
    from oscar_mpc_planner_mr_modification_amd.native_spec import (MpcgPathSettings, MpcgPathTable,
                                                                   problem_from_layout)
    lib = C.CDLL(LIB)
    lib.mpcg_last_error.restype = C.c_char_p
    vp = C.c_void_p
    lib.mpcg_path_update.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcg_path_command.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    lay = config_layout("C2")
    pr = problem_from_layout(lay)
    S = 3
    po = (C.c_int * S)(0, 1, 1)

    def update(pr_=pr, tb=None, po_=po, state=1, seg=1, cs=1, sp=1, reached=1, null_table=False):
        tb = MpcgPathTable(1, 1, 1, 1, 2, 64) if tb is None else tb
        return lib.mpcg_path_update(C.byref(pr_), S, None if null_table else C.byref(tb), po_, state, seg, cs, sp,
                                    reached, None)

    def bad(rc, word):
        assert rc == -1 and word in lib.mpcg_last_error().decode(), (rc, lib.mpcg_last_error())

    bad(update(null_table=True), "null path table")
    for field in ("coef", "knots", "n_segments", "path_of"):
        tb = MpcgPathTable(1, 1, 1, 1, 2, 64)
        setattr(tb, field, None)
        bad(update(tb=tb), "null path table")
    bad(update(tb=MpcgPathTable(1, 1, 1, 1, 2, 65)), "M <= 64")
    bad(update(tb=MpcgPathTable(1, 1, 1, 1, 2, 0)), "M <= 64")
    bad(update(tb=MpcgPathTable(1, 1, 1, 1, 0, 8)), "at least one path")
    pr0 = problem_from_layout(lay)
    pr0.n_seg = 0
    bad(update(pr_=pr0), "n_seg >= 1")
    prw = problem_from_layout(lay)
    prw.i_spline0 = lay.npar - 9 * lay.n_seg + 1
    bad(update(pr_=prw), "mpcg_path_update: the spline window lies outside the stage parameters")
    prw.i_spline0 = -1
    bad(update(pr_=prw), "the spline window lies outside the stage parameters")
    pr1 = problem_from_layout(lay)
    pr1.nx = 1
    bad(update(pr_=pr1), "the spline window lies outside the stage parameters")
    for kw in ("state", "seg", "cs", "sp", "reached"):
        bad(update(**{kw: None}), "invalid arguments")
    bad(update(po_=None), "invalid arguments")
    bad(update(po_=(C.c_int * S)(0, 2, 1)), "path_of[1] = 2")
    bad(update(po_=(C.c_int * S)(0, 1, -1)), "path_of[2] = -1")

    def command(pr_=pr, G=4, st=None, best=1, xt=1, ut=1, state=1, cs=1, slot=4, cmd=1, nxt=1, null_set=False):
        st = MpcgPathSettings(20.0, 3.0, 1) if st is None else st
        return lib.mpcg_path_command(C.byref(pr_), S, G, None if null_set else C.byref(st), best, xt, ut, state, cs,
                                     slot, cmd, nxt, None)

    bad(command(null_set=True), "invalid arguments")
    bad(command(G=0), "invalid arguments")
    for kw in ("best", "xt", "ut", "state", "cmd"):
        bad(command(**{kw: None}), "invalid arguments")
    bad(command(st=MpcgPathSettings(0.0, 3.0, 0)), "control_frequency")
    bad(command(slot=lay.nx), "spline_slot")
    bad(command(nxt=None), "needs state_next")
    # no launch for an empty batch
    assert lib.mpcg_path_update(C.byref(pr), 0, C.byref(MpcgPathTable(1, 1, 1, 1, 2, 64)), po, 1, 1, 1, 1, 1, None) == 0
    assert lib.mpcg_path_command(C.byref(pr), 0, 4, C.byref(MpcgPathSettings(20.0, 3.0, 0)), 1, 1, 1, 1, None, -1, 1,
                                 None, None) == 0
