"""Decomp halfspaces on the host (decomp.py; include/mpcg_decomp.h): known answers derived by hand, the
properties of the polyhedra on seeded scenes, what the kernel cases hold, and the entry point's argument
checks (host-only calls of libmpcg.so: every rejection happens before a HIP call).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import decomp_cases as dc
from oscar_mpc_planner_mr_modification_amd import decomp
from oscar_mpc_planner_mr_modification_amd.layouts import config_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "oscar_mpc_planner_mr_modification_amd")
DUMMY = 100.0


def _rows(q0, q1, pts, R=3.0, nd=6):
    return decomp.decomp_segment_host(q0, q1, pts, R, nd, DUMMY)


# ------------------------------------------------------------------ hand-derived answers


def test_one_point_beside_a_segment_along_x():
    """segment (0,0) -> (2,0), R 3, one point (1, 0.5): e = (1,0), c = (1,0), a = 1; the point lies inside the
    circle, so b = 0.5 / sqrt(1 - 0) = 0.5; its hyperplane is tangent at (1, 0.5) with n = (0, 1); then the box"""
    r = _rows((0, 0), (2, 0), [(1, 0.5)])
    assert r["minor_axis"] == 0.5 and r["n_found"] == 5 and r["kept"].tolist() == [True]
    want = [(0, 1, 0.5), (0, -1, 3), (0, 1, 3), (1, 0, 5), (-1, 0, 3), (1, 0, DUMMY)]
    assert np.array_equal(r["rows"], np.array(want, float))


def test_the_same_rotated_by_a_quarter_turn():
    r = _rows((0, 0), (0, 2), [(-0.5, 1)])
    assert r["minor_axis"] == 0.5 and r["n_found"] == 5
    want = [(-1, 0, 0.5), (1, 0, 3), (-1, 0, 3), (0, 1, 5), (0, -1, 3), (1, 0, DUMMY)]
    assert np.array_equal(r["rows"], np.array(want, float))


def test_a_point_outside_the_box_gives_only_the_four_box_rows():
    r = _rows((0, 0), (2, 0), [(1, 3.5), (5.5, 0), (-3.5, 0)])
    assert r["kept"].tolist() == [False] * 3 and r["n_found"] == 4 and r["minor_axis"] == 1.0
    want = [(0, -1, 3), (0, 1, 3), (1, 0, 5), (-1, 0, 3), (1, 0, DUMMY), (1, 0, DUMMY)]
    assert np.array_equal(r["rows"], np.array(want, float))
    # on the box (within eps) is inside it
    assert _rows((0, 0), (2, 0), [(1, 3.0)])["kept"].tolist() == [True]


def test_two_equal_points_give_one_row_from_the_lower_index():
    r = _rows((0, 0), (2, 0), [(1, 0.5), (1, 0.5)])
    assert r["n_found"] == 5 and np.array_equal(r["rows"][0], (0, 1, 0.5))
    # two points at the same dist on either side: the lower index comes first
    r = _rows((0, 0), (2, 0), [(1, -0.5), (1, 0.5)])
    assert r["n_found"] == 6
    assert np.array_equal(r["rows"][:2], np.array([(0, -1, 0.5), (0, 1, 0.5)], float))
    r = _rows((0, 0), (2, 0), [(1, 0.5), (1, -0.5)])
    assert np.array_equal(r["rows"][:2], np.array([(0, 1, 0.5), (0, -1, 0.5)], float))


def test_more_hyperplanes_than_rows_are_counted_but_not_written():
    # a ring around the segment: every tangent cuts off only its own point
    pts = [(1 + 2.5 * np.cos(t), 2.5 * np.sin(t)) for t in np.linspace(0.2, 6.0, 8)]
    full, cut = _rows((0, 0), (2, 0), pts, nd=16), _rows((0, 0), (2, 0), pts, nd=3)
    assert full["n_found"] == cut["n_found"] == 8 + 4
    assert np.array_equal(cut["rows"], full["rows"][:3])


def test_ieee_cases_a_standing_segment_and_a_point_on_the_segment():
    r = _rows((1, 1), (1, 1), [(1, 1.5)])
    assert (r["rows"] == (1, 0, DUMMY)).all() and r["n_found"] == 4 and r["minor_axis"] == 0.0
    r = _rows((0, 0), (2, 0), [(1.5, 1.0), (1, 0)])
    assert r["minor_axis"] == 0.0 and (r["rows"] == (1, 0, DUMMY)).all()


def test_path_points_follow_the_warm_start_s_speed_and_the_braking_plan():
    lay = dc.layout(10)
    sc = decomp.make_c3_decomp_scenes(lay, 2, 77)
    q = decomp.decomp_path_points_host(sc.table, sc.path_of, sc.xinit, sc.warm, 10, lay.dt, lay.nu)
    s = sc.xinit[:, 5, None] + lay.dt * np.concatenate([np.zeros((2, 1)), np.cumsum(sc.warm[:, :9, 6], 1)], 1)
    for i in range(2):
        for k in range(10):
            np.testing.assert_allclose(q[i, k], sc.table.point(i, s[i, k]), rtol=0, atol=1e-12)
    qb = decomp.decomp_path_points_host(sc.table, sc.path_of, sc.xinit, None, 10, lay.dt, lay.nu, 3.0)
    from oscar_mpc_planner_mr_modification_amd.bicycle import braking_warm
    for i in range(2):
        w = braking_warm(sc.xinit[i].copy(), 10, lay.dt, 3.0)
        for k in range(10):
            np.testing.assert_allclose(qb[i, k], sc.table.point(i, w[k, 8]), rtol=0, atol=1e-12)


def test_placement_writes_the_decomp_block_of_every_planner_and_nothing_else():
    lay = dc.layout(10)
    rng = np.random.default_rng(3)
    params, rows = rng.normal(size=(6, 10, lay.npar)), rng.normal(size=(2, 10, 4, 3))
    out = decomp.apply_decomp_host(lay, params, 3, rows)
    i0 = lay.idx("disc_0_decomp_0_a1")
    keep = np.delete(np.arange(lay.npar), np.arange(i0, i0 + 12))
    assert np.array_equal(out[..., keep], params[..., keep])
    assert np.array_equal(out.reshape(2, 3, 10, lay.npar)[:, :, :, i0:i0 + 12],
                          np.repeat(rows.reshape(2, 1, 10, 12), 3, 1))
    with pytest.raises(ValueError):
        decomp.apply_decomp_host(lay, params, 3, rows[:, :9])


# ------------------------------------------------------------------ properties on seeded scenes


def _dummy_rows(rows, x0):
    return (rows[..., 0] == 1.0) & (rows[..., 1] == 0.0) & (rows[..., 2] == (x0 + 100.0)[:, None, None])


@pytest.mark.parametrize("N", [10, 30])
def test_polyhedra_hold_the_segment_and_exclude_every_kept_point(N):
    c = dc.property_case(N)
    lay, sc, h = c.lay, c.sc, c.host
    nd = lay.n_scen
    checked = 0
    for s in range(dc.PROPERTY_SCENES):
        pts = sc.occ[s, :sc.n_occ[s]]
        for k in range(N - 1):
            rows = h["rows"][s, k + 1]
            if h["n_found"][s, k + 1] > nd or not np.isfinite(rows).all():
                continue
            if _dummy_rows(rows[None], sc.xinit[s:s + 1, 0]).all():
                continue
            A, b = rows[:, :2], rows[:, 2]
            for q in (h["points"][s, k], h["points"][s, k + 1]):
                assert (A @ q - b).max() <= 1e-9, (s, k)
            kept = decomp.decomp_segment_host(h["points"][s, k], h["points"][s, k + 1], pts, dc.SETTINGS.range, nd,
                                              0.0)["kept"]
            if kept.any():
                assert ((pts[kept] @ A.T - b).max(1) >= -1e-9).all(), (s, k)
            checked += 1
    assert checked >= 40
    assert np.array_equal(h["rows"][:, 0], np.broadcast_to(np.stack(
        [np.ones(len(sc.xinit)), np.zeros(len(sc.xinit)), sc.xinit[:, 0] + 100.0], 1)[:, None], h["rows"][:, 0].shape))
    assert (h["n_found"][:, 0] == 0).all() and (h["minor_axis"][:, 0] == 0).all()


def test_the_property_scenes_hold_every_kind_of_stage():
    """n_found above the rows (N 10 / 4 rows) and below them (N 30 / 12 rows), all-dummy stages from L = 0 (the
    braking scenes), and the NaN cut of the point put on a segment"""
    seen = {}
    for N in (10, 30):
        c = dc.property_case(N)
        h, nd = c.host, c.lay.n_scen
        nf = h["n_found"][:, 1:]
        q = h["points"]
        still = (q[:, 1:] == q[:, :-1]).all(-1)
        dummies = _dummy_rows(h["rows"][:, 1:], c.sc.xinit[:, 0]).all(-1)
        assert dummies[still].all() and (h["minor_axis"][:, 1:][still] == 0.0).all()
        assert still[c.n_warm:].any() and not still[:c.n_warm].any()
        s, k = c.on_segment
        assert dummies[s, k - 1] and h["minor_axis"][s, k] == 0.0 and not still[s, k - 1]
        seen[N] = dict(above=int((nf > nd).sum()), below=int((nf < nd).sum()), still=int(still.sum()))
    print(seen)
    assert seen[10]["above"] > 0 and seen[30]["below"] > 0 and seen[10]["still"] > 0 and seen[30]["still"] > 0
    # the kernel cases reach past the rows at N 30 as well (the ring of scene 4)
    _, h, _ = dc.kernel_case("N30-G3-warm-special")
    assert (h["n_found"][4] > 12).any()


def test_kernel_cases_cover_what_they_claim():
    got = {name: dc.kernel_case(name) for name in dc.KERNEL_CASES}
    shapes = {(i.lay.N, i.lay.n_scen, i.G, i.main_warm is not None) for i, _, _ in got.values()}
    assert {(10, 4), (30, 12)} == {s[:2] for s in shapes} and {1, 3} == {s[2] for s in shapes}
    assert {True, False} == {s[3] for s in shapes}
    counts = set()
    for i, h, want in got.values():
        assert 3 <= i.S <= 5
        counts |= set(i.n_occ.tolist())
        for s in range(i.S):
            assert np.isnan(i.occ[s, i.n_occ[s]:]).all() and np.isfinite(i.occ[s, :i.n_occ[s]]).all()
        assert not np.array_equal(want, i.params)
    assert {0, 1, 63, 64, 65, 130, 1024} <= counts
    for name in ("N10-G1-warm-small-counts", "N10-G3-braking", "N30-G1-braking", "N30-G3-warm-special"):
        i = got[name][0]
        assert i.occ.shape[1] > i.n_occ.max(), name
    for name in ("N30-G3-warm-special", "N10-G1-warm-special"):
        i, h, _ = got[name]
        x0 = i.state[:, 0]
        dummies = _dummy_rows(h["rows"][:, 1:], x0).all(-1)
        q = h["points"]
        still = (q[:, 1:] == q[:, :-1]).all(-1)
        assert h["minor_axis"][0, 4] == 0.0 and dummies[0, 3] and not still[0, 3]     # the point on segment 3 -> 4
        assert len(np.unique(i.occ[1, :i.n_occ[1]], axis=0)) * 2 <= i.n_occ[1]          # duplicates
        assert (h["n_found"][2, 1:] == 4).all() and i.n_occ[2] > 0                      # all outside the box
        assert still[3].any() and not still[3, 0] and dummies[3][still[3]].all()        # s past the end
    for name in ("N10-G3-braking", "N30-G1-braking"):
        i, h, _ = got[name]
        still = (h["points"][:, 1:] == h["points"][:, :-1]).all(-1)
        assert still[1].all() and still[0].any() and not still[0, 0]


# ------------------------------------------------------------------ the entry point's checks


def test_decomp_entry_point_is_exported_and_checks_its_arguments():
    from oscar_mpc_planner_mr_modification_amd import _build
    from oscar_mpc_planner_mr_modification_amd.native_spec import (DECOMP_EXPORTS, MpcgDecompIo, MpcgDecompSettings,
                                                                   MpcgPathTable, problem_from_layout)
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    lib = C.CDLL(os.path.join(PKG, "libmpcg.so"))
    for name in DECOMP_EXPORTS:
        assert hasattr(lib, name), name
    lib.mpcg_last_error.restype = C.c_char_p
    fn = lib.mpcg_decomp_halfspaces
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10
    # every rejection happens before a pointer is followed on the device: dummy non-null addresses
    # (host arrays) stand in for device memory and no launch is reached
    keep = np.zeros(16)
    d = keep.ctypes.data
    po, no = np.zeros(1, np.int32), np.array([3], np.int32)
    tb = MpcgPathTable(d, d, d, d, 1, 4)
    io = MpcgDecompIo(d, None, d, d, 8)
    st = MpcgDecompSettings(2.0, 3.0)
    c3 = problem_from_layout(dc.layout(10))

    def call(pr=c3, G=1, sett=st, table=tb, path_of=po, dio=io, n_occ=no, params=d):
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        arr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return fn(ref(pr), 1, G, ref(sett), ref(table), arr(path_of), ref(dio), arr(n_occ), params, None, None, None,
                  None)

    def bad(rc, text):
        assert rc == -1 and lib.mpcg_last_error().decode() == "mpcg_decomp_halfspaces: " + text, lib.mpcg_last_error()

    def changed(**kw):
        pr = problem_from_layout(dc.layout(10))
        for k, v in kw.items():
            setattr(pr, k, v)
        return pr

    # a null pointer
    for kw in (dict(pr=None), dict(sett=None), dict(dio=None), dict(params=None), dict(path_of=None), dict(n_occ=None),
               dict(dio=MpcgDecompIo(None, None, d, d, 8)), dict(dio=MpcgDecompIo(d, None, None, d, 8)),
               dict(dio=MpcgDecompIo(d, None, d, None, 8))):
        bad(call(**kw), "invalid arguments")
    bad(call(pr=changed(n_scen=0)), "needs 1 <= max_constraints (n_scen) <= 64")
    bad(call(pr=problem_from_layout(config_layout("C2"))), "needs 1 <= max_constraints (n_scen) <= 64")
    bad(call(pr=changed(n_scen=65)), "needs 1 <= max_constraints (n_scen) <= 64")
    bad(call(pr=changed(i_scen0=c3.npar - 11)), "the decomp block lies outside the stage parameters")
    bad(call(pr=changed(i_scen0=-1)), "the decomp block lies outside the stage parameters")
    bad(call(pr=changed(nx=4)), "needs the states x y psi v .. spline (nx >= 5)")
    bad(call(pr=changed(N=1)), "needs 2 <= N <= 32")
    bad(call(pr=changed(N=33)), "needs 2 <= N <= 32")
    bad(call(G=0), "needs at least one planner per scene")
    bad(call(sett=MpcgDecompSettings(0.0, 3.0)), "needs range > 0")
    bad(call(sett=MpcgDecompSettings(float("nan"), 3.0)), "needs range > 0")
    bad(call(dio=MpcgDecompIo(d, None, d, d, 1025)), "needs 0 <= P <= 1024 occupied points per scene")
    bad(call(dio=MpcgDecompIo(d, None, d, d, -1)), "needs 0 <= P <= 1024 occupied points per scene")
    bad(call(n_occ=np.array([9], np.int32)), "n_occ[0] = 9 outside 0 .. P")
    bad(call(n_occ=np.array([-1], np.int32)), "n_occ[0] = -1 outside 0 .. P")
    # the path-table and path_of checks it shares with mpcg_path_update and mpcg_road_halfspaces, text for text
    for field in ("coef", "knots", "n_segments", "path_of"):
        nulled = MpcgPathTable(d, d, d, d, 1, 4)
        setattr(nulled, field, None)
        bad(call(table=nulled), "null path table")
    bad(call(table=None), "null path table")
    bad(call(table=MpcgPathTable(d, d, d, d, 1, 65)), "needs 1 <= M <= 64 segments per path")
    bad(call(table=MpcgPathTable(d, d, d, d, 1, 0)), "needs 1 <= M <= 64 segments per path")
    bad(call(table=MpcgPathTable(d, d, d, d, 0, 4)), "needs at least one path")
    bad(call(path_of=np.array([1], np.int32)), "path_of[0] = 1 outside the table")
    bad(call(path_of=np.array([-1], np.int32)), "path_of[0] = -1 outside the table")
    # the host restatement refuses the same shapes
    sc = decomp.make_c3_decomp_scenes(dc.layout(10), 1, 5)
    for kw in (dict(N=1), dict(N=33), dict(nd=0), dict(nd=65), dict(R=0.0), dict(n_occ=[sc.occ.shape[1] + 1])):
        with pytest.raises(ValueError):
            decomp.decomp_halfspaces_host(decomp.DecompSettings(range=kw.get("R", 2.0)), sc.table, sc.path_of, sc.xinit,
                                          sc.warm, sc.occ, kw.get("n_occ", sc.n_occ), kw.get("N", 10), 0.2, 3,
                                          kw.get("nd", 4))
