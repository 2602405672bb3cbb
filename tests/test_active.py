"""The active-solve compaction on the host (active.py) and its C ABI (include/mpcg_active.h): the plan
against np.flatnonzero, gather and scatter as inverses on the enabled solves with the header's fill on
the others, the composite around a solve function, the library's exports and error returns.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oscar_mpc_planner_mr_modification_amd import active
from oscar_mpc_planner_mr_modification_amd import native_spec as ns
from oscar_mpc_planner_mr_modification_amd.layouts import config_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oscar_mpc_planner_mr_modification_amd", "libmpcg.so")
HDR = os.path.join(ROOT, "include", "mpcg_active.h")
BATCHES = (1, 63, 64, 65, 1023, 1024, 1025, 2051)
MASKS = ("ones", "zeros", "alternating", "last", "random")


def mask(kind, B, seed=0):
    if kind == "ones":
        return np.ones(B, np.uint8)
    if kind == "zeros":
        return np.zeros(B, np.uint8)
    if kind == "alternating":
        return (np.arange(B) % 2).astype(np.uint8)
    if kind == "last":
        m = np.zeros(B, np.uint8)
        m[-1] = 1
        return m
    # non-zero bytes other than 1 count as enabled
    return (np.random.default_rng(1000 * seed + B).integers(0, 3, B) * 100).astype(np.uint8)


def check_plan(plan, en):
    idx = np.flatnonzero(en)
    n = len(idx)
    assert plan["n_active"] == n
    slot_of, solve_of = np.asarray(plan["slot_of"]), np.asarray(plan["solve_of"])
    assert slot_of.dtype == np.int32 and solve_of.dtype == np.int32 and slot_of.shape == solve_of.shape == en.shape
    np.testing.assert_array_equal(solve_of[:n], idx)
    assert (solve_of[n:] == -1).all()
    np.testing.assert_array_equal(slot_of[idx], np.arange(n))
    assert (slot_of[en == 0] == -1).all()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", MASKS)
def test_plan_host_is_flatnonzero(B, kind):
    en = mask(kind, B)
    check_plan(active.plan_host(en), en)
    # the shape of the flags does not matter
    if B % 2 == 0:
        check_plan(active.plan_host(en.reshape(2, -1)), en)


def random_io(lay, B, rng, lam=True, qp=0, stats=False):
    """Random inputs and outputs of B solves of `lay`, keys as native.solve_batch_device's."""
    N, nx, nu = lay.N, lay.nx, lay.nu
    LS = nx + lay.nh
    full = dict(params=rng.normal(size=(B, N, lay.npar)), warm=rng.normal(size=(B, N + 1, nu + nx)),
                xinit=rng.normal(size=(B, nx)))
    outs = dict(xtraj=rng.normal(size=(B, N + 1, nx)), utraj=rng.normal(size=(B, N, nu)), pobj=rng.normal(size=B),
                exit=rng.integers(0, 5, B).astype(np.int32), info=rng.integers(0, 50, (B, 4)).astype(np.int32))
    if lam:
        full["lam_in"] = rng.normal(size=(B, N, LS))
        outs["lam"] = rng.normal(size=(B, N, LS))
    if qp:
        full["qp_in"] = rng.normal(size=(B, qp))
        outs["qp"] = rng.normal(size=(B, qp))
    if stats:
        outs["stats"] = rng.normal(size=(B, 4))
    return full, outs


def check_fill(out, warm, nu, off):
    """every output of the solves `off` holds the header's fill"""
    np.testing.assert_array_equal(out["xtraj"][off], warm[off][:, :, nu:])
    np.testing.assert_array_equal(out["utraj"][off], warm[off][:, :-1, :nu])
    assert (out["pobj"][off] == np.inf).all()
    assert (out["exit"][off] == ns.ACTIVE_EXIT_SKIPPED).all() and out["exit"].dtype == np.int32
    if "info" in out:
        assert (out["info"][off] == 0).all()
    if "lam" in out:
        assert (out["lam"][off] == 0.0).all()
    if "qp" in out:
        assert np.isnan(out["qp"][off][:, 0]).all() and (out["qp"][off][:, 1:] == 0.0).all()
    if "stats" in out:
        assert np.isnan(out["stats"][off]).all()


@pytest.mark.parametrize("cfg,S,G", [("C2", 4, 8), ("JS", 3, 5)])
@pytest.mark.parametrize("kind", MASKS)
def test_scatter_of_gather_is_the_identity_on_the_enabled_solves(cfg, S, G, kind):
    lay = config_layout(cfg)
    B = S * G
    rng = np.random.default_rng(7)
    en = mask(kind, B, seed=1)
    on, off = en != 0, en == 0
    full, outs = random_io(lay, B, rng, qp=11, stats=True)
    plan = active.plan_host(en)
    n = plan["n_active"]
    dense = active.gather_host(plan["slot_of"], full)
    for k, v in full.items():
        assert dense[k].shape == (n,) + v.shape[1:]
        np.testing.assert_array_equal(dense[k], v[on], err_msg=k)          # stable: the enabled solves in order
    # into given buffers: rows no solve maps to keep their content
    room = {k: np.full((B,) + v.shape[1:], 7.5) for k, v in full.items()}
    got = active.gather_host(plan["slot_of"], full, room)
    for k, v in full.items():
        np.testing.assert_array_equal(got[k][:n], v[on], err_msg=k)
        assert (got[k][n:] == 7.5).all() and (room[k] == 7.5).all()
    # the outputs of the dense batch, scattered back
    dense_out = {k: v[on] for k, v in outs.items()}
    back = active.scatter_host(plan["slot_of"], dense_out, full["warm"], lay.nu)
    assert set(back) == set(outs)
    for k, v in outs.items():
        assert back[k].shape == v.shape and back[k].dtype == v.dtype
        np.testing.assert_array_equal(back[k][on], v[on], err_msg=k)
    check_fill(back, full["warm"], lay.nu, off)


def test_solve_active_host_solves_the_enabled_solves_only():
    lay = config_layout("C2")
    B, nu = 12, lay.nu
    rng = np.random.default_rng(3)
    full, _ = random_io(lay, B, rng)
    calls = []

    def solve(params, warm, xinit, lam_in=None, tag=None):
        calls.append((params.shape[0], tag))
        return dict(xtraj=warm[:, :, nu:] * 2.0, utraj=warm[:, :-1, :nu] * 3.0, pobj=params[:, 0, 0] + xinit[:, 0],
                    status=np.ones(len(params), np.int32), lam=lam_in + 1.0)

    ref = solve(full["params"], full["warm"], full["xinit"], lam_in=full["lam_in"])
    en = mask("random", B, seed=2)
    on = en != 0
    assert 0 < on.sum() < B
    calls.clear()
    r = active.solve_active_host(solve, full["params"], full["warm"], full["xinit"], en, nu, lam_in=full["lam_in"],
                                 tag="t")
    assert calls == [(int(on.sum()), "t")] and r["n_active"] == on.sum()
    np.testing.assert_array_equal(r["slot_of"], active.plan_host(en)["slot_of"])
    for k in ("xtraj", "utraj", "pobj", "status", "lam"):
        np.testing.assert_array_equal(r[k][on], ref[k][on], err_msg=k)
    assert (r["status"][~on] == ns.ACTIVE_EXIT_SKIPPED).all() and (r["pobj"][~on] == np.inf).all()
    np.testing.assert_array_equal(r["xtraj"][~on], full["warm"][~on][:, :, nu:])
    assert (r["lam"][~on] == 0.0).all()
    # no enabled solve: the solve function is not called, everything is the fill
    calls.clear()
    r0 = active.solve_active_host(solve, full["params"], full["warm"], full["xinit"], np.zeros(B, np.uint8), nu,
                                  lam_in=full["lam_in"])
    assert calls == [] and r0["n_active"] == 0 and (r0["slot_of"] == -1).all()
    check_fill(r0, full["warm"], nu, np.ones(B, bool))
    with pytest.raises(ValueError):
        active.solve_active_host(solve, full["params"], full["warm"], full["xinit"], np.ones(B + 1, np.uint8), nu)


# ------------------------------------------------------------------ the C ABI


def test_skipped_exit_code_is_the_guidance_layers_disabled_code():
    assert ns.ACTIVE_EXIT_SKIPPED == ns.GUIDANCE_EXIT_DISABLED == -100
    macro = lambda path, name: int(re.search(rf"#define {name} \((-?\d+)\)", open(path).read()).group(1))  # noqa: E731
    assert macro(HDR, "MPCG_ACTIVE_EXIT_SKIPPED") == ns.ACTIVE_EXIT_SKIPPED
    assert macro(os.path.join(ROOT, "include", "mpcg_guidance.h"), "MPCG_GUIDANCE_EXIT_DISABLED") == ns.ACTIVE_EXIT_SKIPPED
    assert ns.ACTIVE_EXIT_SKIPPED not in (0, 1, 2, 3, 4)


def test_active_sources_are_linked_outside_the_source_hash():
    from oscar_mpc_planner_mr_modification_amd import _build
    assert _build.LAYERS["mpcg_active.h"] == {"sources": {"mpcg_active.hip": ["-ffp-contract=off"]},
                                              "headers": ["mpcg_active.h"]}
    assert "mpcg_active.hip" not in _build.SOURCES and "mpcg_active.h" not in _build.HEADERS


def test_bad_arguments_are_reported_without_a_launch():
    """Every NULL-pointer and negative-size error of the calls (host-side checks only: the pointers are never
    read on the device, and no workspace can be created without a GPU)."""
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgIo, problem_from_layout
    lib = C.CDLL(LIB)
    lib.mpcg_last_error.restype = C.c_char_p
    vp = C.c_void_p
    lib.mpcg_active_plan.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    lib.mpcg_active_gather.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.mpcg_active_scatter.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.mpcg_active_ws_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.mpcg_active_ws_create.restype = vp
    lib.mpcg_active_ws_destroy.argtypes = [vp]
    lib.mpcg_active_ws_destroy.restype = None
    lib.mpcg_active_ws_read_plan.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.mpcg_solve_active.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    pr = problem_from_layout(config_layout("C2"))
    B = 5
    FIELDS = [f[0] for f in MpcgIo._fields_]

    def io(**null):
        x = MpcgIo(*([1] * len(FIELDS)))
        for k in null:
            setattr(x, k, None)
        return x

    def bad(rc, word):
        assert rc == -1 and word in lib.mpcg_last_error().decode(), (rc, lib.mpcg_last_error())

    # plan
    bad(lib.mpcg_active_plan(-1, 1, 1, 1, 1, None), "negative batch")
    for i in range(4):
        a = [1, 1, 1, 1]
        a[i] = None
        bad(lib.mpcg_active_plan(B, *a, None), "invalid arguments")

    # gather
    def gather(pr_=C.byref(pr), batch=B, slot=1, full=None, dense=None, null_full=False, null_dense=False):
        full, dense = full or io(), dense or io()
        return lib.mpcg_active_gather(pr_, batch, slot, None if null_full else C.byref(full),
                                      None if null_dense else C.byref(dense), None)

    bad(gather(batch=-1), "negative batch")
    bad(gather(pr_=None), "invalid arguments")
    bad(gather(slot=None), "invalid arguments")
    bad(gather(null_full=True), "invalid arguments")
    bad(gather(null_dense=True), "invalid arguments")
    for k in ("params", "warm", "xinit"):
        bad(gather(full=io(**{k: 1})), "null input of the full batch")
        bad(gather(dense=io(**{k: 1})), "null input of the dense batch")
    prn = problem_from_layout(config_layout("C2"))
    prn.N = 0
    bad(gather(pr_=C.byref(prn)), "invalid problem dimensions")

    # scatter
    def scatter(pr_=C.byref(pr), batch=B, slot=1, dense=None, full=None, null_full=False, null_dense=False):
        full, dense = full or io(), dense or io()
        return lib.mpcg_active_scatter(pr_, batch, slot, None if null_dense else C.byref(dense),
                                       None if null_full else C.byref(full), None)

    bad(scatter(batch=-1), "negative batch")
    bad(scatter(pr_=None), "invalid arguments")
    bad(scatter(slot=None), "invalid arguments")
    bad(scatter(null_full=True), "invalid arguments")
    bad(scatter(null_dense=True), "invalid arguments")
    bad(scatter(full=io(warm=1)), "needs the warm start")
    for k in ("xtraj", "utraj", "pobj", "exit_code", "info", "lam_out", "qp_out", "stats"):
        bad(scatter(dense=io(**{k: 1})), "no dense counterpart")
    bad(scatter(pr_=C.byref(prn)), "invalid problem dimensions")

    # the workspace and the composite
    assert lib.mpcg_active_ws_create(None, 4, 0, 0, 0) is None and "invalid arguments" in lib.mpcg_last_error().decode()
    assert lib.mpcg_active_ws_create(C.byref(pr), 0, 0, 0, 0) is None
    assert "invalid arguments" in lib.mpcg_last_error().decode()
    assert lib.mpcg_active_ws_create(C.byref(prn), 4, 0, 0, 0) is None
    assert "invalid problem dimensions" in lib.mpcg_last_error().decode()
    lib.mpcg_active_ws_destroy(None)
    bad(lib.mpcg_active_ws_read_plan(None, B, 1, 1, None), "invalid arguments")
    x = io()
    bad(lib.mpcg_solve_active(C.byref(pr), -1, C.byref(x), 1, 1, None, None), "negative batch")
    bad(lib.mpcg_solve_active(None, B, C.byref(x), 1, 1, None, None), "invalid arguments")
    bad(lib.mpcg_solve_active(C.byref(pr), B, None, 1, 1, None, None), "invalid arguments")
    bad(lib.mpcg_solve_active(C.byref(pr), B, C.byref(x), None, 1, None, None), "invalid arguments")
    bad(lib.mpcg_solve_active(C.byref(pr), B, C.byref(x), 1, None, None, None), "invalid arguments")
    # no launch for an empty batch
    assert gather(batch=0) == 0 and scatter(batch=0) == 0


def test_skip_disabled_needs_a_guidance_layer():
    import inspect

    from oscar_mpc_planner_mr_modification_amd.control_loop import ControlLoop
    from oscar_mpc_planner_mr_modification_amd.fleet import FleetLoop
    from oscar_mpc_planner_mr_modification_amd.paths import PathLoop
    from oscar_mpc_planner_mr_modification_amd.synthetic import make_scenes
    assert inspect.signature(ControlLoop.__init__).parameters["skip_disabled"].default is False
    lay = config_layout("C2")
    sc = make_scenes(lay, 2, 8, seed=1)
    with pytest.raises(ValueError, match="guidance_layer"):
        ControlLoop(lay, sc, "cpu", 0.3, 1.0, 0.75, skip_disabled=True)
    # the fleet's and the path loop's options reach ControlLoop
    from oscar_mpc_planner_mr_modification_amd import fleet
    with pytest.raises(ValueError, match="guidance_layer"):
        FleetLoop(lay, sc, 1, 2, "cpu", fleet.FleetSettings(n_paths=7), 0.3, 1.0, 0.75, skip_disabled=True)
    for cls in (FleetLoop, PathLoop):
        assert "skip_disabled" in cls.__doc__


def test_cpu_guidance_loop_skipping_equals_the_masked_cpu_loop(oracle_mod):
    """The argument of DESIGN.md §6.6 on the CPU: gc.GuidanceCpuLoop (every planner solved by the oracle,
    the disabled ones masked) against the same loop with solve_active_host around the oracle, three steps
    of gc.LOOP_CASE with warmstart_with_mpc_solution.  best, the exit codes, the layer's outputs and the
    carried state are equal at every step, trajectories and objectives on the enabled planners."""
    import copy

    import guidance_cases as gc
    import producers_oracle
    from oscar_mpc_planner_mr_modification_amd import guidance as gd
    from oscar_mpc_planner_mr_modification_amd.selection import find_best_planner_host
    from oscar_mpc_planner_mr_modification_amd.synthetic import DECELERATION, ROBOT_RADIUS
    from test_control_loop import SEL_W, W_CONS

    class SkippingCpuLoop(gc.GuidanceCpuLoop):
        def step(self):
            lay, sc = self.lay, self.sc
            u = gd.guidance_update_host(lay, sc.state, sc.stage_params, sc.obst, sc.obst_meta, self.gstate, sc.guidance,
                                        self.G, gc.SETTINGS, details=True)
            self.details.append(u["details"])
            sc.guidance = u["guidance"]
            sc.consistency_on, sc.previously_selected = u["consistency_on"] > 0, u["previously_selected"] > 0
            self.gstate["class_traj"], self.gstate["class_used"] = u["class_traj"], u["class_used"]
            if self.own_warm and self.prev is not None:
                sc.planner_xtraj, sc.planner_utraj = self.prev["xtraj"], self.prev["utraj"]
                sc.existing_guidance = u["existing_guidance"] > 0
            p = self.prod.prepare(lay, sc, ROBOT_RADIUS, W_CONS, DECELERATION, warmstart_with_mpc_solution=self.own_warm)
            r = active.solve_active_host(self.orc.solve_batch, p["params"], p["warm"], p["xinit"], u["enabled"], lay.nu,
                                         lam_in=self.lam, return_lam=True)
            self.n_active = r["n_active"]
            best, obj = find_best_planner_host(self.S, self.G, self.N, r["xtraj"], r["pobj"], r["status"],
                                               p["prev_interp"], W_CONS, p["consistency_active"],
                                               sc.previously_selected.reshape(-1), SEL_W)
            self.p, self.r, self.u = p, r, u
            return dict(best=best, obj=np.asarray(obj).reshape(self.S, self.G), exit=r["status"], xtraj=r["xtraj"],
                        n_found=u["n_found"], topology=u["topology"], enabled=u["enabled"])

    lay, sc0 = gc.loop_scenes()
    off = gc.GuidanceCpuLoop(lay, copy.deepcopy(sc0), oracle_mod, producers_oracle, own_warm=True)
    on = SkippingCpuLoop(lay, copy.deepcopy(sc0), oracle_mod, producers_oracle, own_warm=True)
    S, G = sc0.n_scenes, sc0.n_guesses
    sets = []
    for t in range(3):
        a, b = off.step(), on.step()
        en = a["enabled"].reshape(-1) != 0
        sets.append(en.reshape(S, G))
        assert on.n_active == en.sum() and 0 < on.n_active < S * G
        for k in ("best", "exit", "n_found", "topology", "enabled"):
            np.testing.assert_array_equal(b[k], a[k], err_msg=f"step {t}: {k}")
        for k in ("params", "warm", "xinit"):
            np.testing.assert_array_equal(on.p[k], off.p[k], err_msg=f"step {t}: prepared {k}")
        for k in ("xtraj", "utraj", "pobj", "lam"):
            np.testing.assert_array_equal(on.r[k][en], off.r[k][en], err_msg=f"step {t}: {k} of the enabled planners")
        np.testing.assert_array_equal(b["obj"].reshape(-1)[en], a["obj"].reshape(-1)[en])
        assert (on.r["status"][~en] == ns.ACTIVE_EXIT_SKIPPED).all() and np.isfinite(on.r["xtraj"][~en]).all()
        off.advance(a["best"])
        on.advance(b["best"])
        for k in off.gstate:
            np.testing.assert_array_equal(on.gstate[k], off.gstate[k], err_msg=f"step {t}: layer state {k}")
        np.testing.assert_array_equal(on.lam, off.lam, err_msg=f"step {t}: carried multipliers")
        np.testing.assert_array_equal(on.sc.state, off.sc.state, err_msg=f"step {t}: next state")
    assert any((x != y).any() for x, y in zip(sets, sets[1:]))
