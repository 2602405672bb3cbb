"""The multi-robot layer on the host (fleet.py) and its C ABI (include/mpcg_fleet.h): the publish
decision against a loop form written from the reference (tests/fleet_reference.py), hand-written
cases for every trigger reason and the priority order, the batched obstacle driver against the
tracker, and the library's exports.  No GPU."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import fleet_reference as fr
from oscar_mpc_planner_mr_modification_amd import fleet
from oscar_mpc_planner_mr_modification_amd import obstacles as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oscar_mpc_planner_mr_modification_amd", "libmpcg.so")
HDR = os.path.join(ROOT, "include", "mpcg_fleet.h")
DT = 0.2
SETTINGS = fleet.FleetSettings(max_geometric_deviation=0.5, heartbeat_time=2.0, n_paths=4)


def assert_publish_equal(got, want, failed):
    """integers, times and winner-copied plans exactly; braking plans (cos / sin) to 1e-12"""
    for k in ("selected", "reason", "published", "prev_topology"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("sent_time", "last_send_time"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)      # NaN == NaN here
    S = len(failed)
    for k in ("plan", "sent_plan"):
        a, b = got[k].reshape(S, -1, 3), want[k].reshape(S, -1, 3)
        np.testing.assert_array_equal(a[~failed], b[~failed], err_msg=k)
        np.testing.assert_allclose(a[failed], b[failed], rtol=0, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("filter_on", [True, False])
def test_publish_host_equals_the_loop_form_on_random_batches(seed, filter_on):
    c = fr.publish_case(seed=seed)
    st = fleet.FleetSettings(max_geometric_deviation=0.5, heartbeat_time=2.0, n_paths=4,
                             communicate_on_topology_switch_only=filter_on)
    want = fr.publish_batch(c["best"], c["xtraj"], c["state"], c["fstate"], c["topology"], c["now"], DT, st)
    failed = c["best"] < 0
    # the default topology (planner index, 2 n_paths for the non-guided planner) and an explicit one
    for kw in (dict(guided=c["guided"]), dict(topology=c["topology"])):
        got = fleet.publish_host(c["best"], c["xtraj"], c["state"], c["fstate"], c["now"], DT, st, **kw)
        assert_publish_equal(got, want, failed)
    if filter_on:
        assert want["reason"][:9].tolist() == c["expect"]
        assert set(want["reason"].tolist()) == {0, 1, 3, 4, 5, 6}
    else:
        assert (want["reason"] == 0).all() and (want["published"] == 1).all()


def _one(best, prev, sent_time=math.nan, last_send=math.nan, sent_offset=0.1, topology=None, settings=SETTINGS,
         now=5.0, v=1.0):
    """One robot (in a 1 x 2 fleet; the second robot is a copy), G 3 planners (planner 2 non-guided)."""
    N, G = 6, 3
    xt = np.zeros((2 * G, N + 1, 5))
    for g in range(G):
        xt[g::G, :, 0] = 0.3 * np.arange(N + 1)[None, :] + g
        xt[g::G, :, 2] = 0.1 * g
    state = np.array([[0.0, 0.0, 0.5, v, 0.0]] * 2)
    plan = xt[max(best, 0), :N, :3] + sent_offset
    fs = dict(sent_plan=np.stack([plan, plan])[None], sent_time=np.full((1, 2), sent_time),
              last_send_time=np.full((1, 2), last_send), prev_topology=np.full((1, 2), prev, np.int32))
    guided = np.array([[1, 1, 0]] * 2, np.uint8)
    topo = np.array([[0, 1, 8]] * 2, np.int32) if topology is None else np.array([topology] * 2, np.int32)
    b = np.array([best, best], np.int32)
    got = fleet.publish_host(b, xt, state, fs, now, DT, settings, guided=guided if topology is None else None,
                             topology=None if topology is None else topo)
    ref = fr.publish_batch(b, xt, state, fs, topo, now, DT, settings)
    assert_publish_equal(got, ref, b < 0)
    return got, xt, state


def test_each_reason_and_the_priority_order():
    now = 5.0
    # 0: same guided topology, close to the communicated plan, sent recently -> nothing changes
    g, xt, _ = _one(1, 1, sent_time=now - 0.05, last_send=now - 0.05)
    assert g["reason"][0] == 0 and g["published"][0] == 0
    assert g["sent_time"][0, 0] == now - 0.05 and g["last_send_time"][0, 0] == now - 0.05
    np.testing.assert_array_equal(g["sent_plan"][0, 0], xt[1, :6, :3] + 0.1)
    # 1: infeasible beats everything (deviating, heartbeat due); the braking plan is sent
    g, _, state = _one(-1, 1, sent_time=now - 0.05, last_send=now - 9.0, sent_offset=50.0)
    assert g["reason"][0] == 1 and g["published"][0] == 1 and g["selected"][0] == -1
    vb = 1.0 - 3.0 / 20.0
    want = [(vb * math.cos(0.5) * DT * i, vb * math.sin(0.5) * DT * i, 0.5) for i in range(6)]
    np.testing.assert_allclose(g["sent_plan"][0, 0], want, rtol=0, atol=1e-12)
    assert g["sent_time"][0, 0] == now and g["last_send_time"][0, 0] == now
    # ... and the braking speed does not go below zero
    g, _, _ = _one(-1, 1, v=0.1)
    np.testing.assert_array_equal(g["plan"][0, :, 0:2], np.zeros((6, 2)))
    # 6: the non-guided planner wins; beats the topology change (prev 1 -> 8)
    g, _, _ = _one(2, 1, sent_time=now - 0.05, last_send=now - 0.05)
    assert g["reason"][0] == 6 and g["published"][0] == 1 and g["prev_topology"][0, 0] == 8
    # ... also when it is no change at all (prev 8)
    assert _one(2, 8, sent_time=now - 0.05, last_send=now - 0.05)[0]["reason"][0] == 6
    # 3: guided 0 -> guided 1; beats geometric and time
    g, xt, _ = _one(1, 0, sent_time=now - 0.05, last_send=now - 9.0, sent_offset=50.0)
    assert g["reason"][0] == 3 and g["published"][0] == 1
    np.testing.assert_array_equal(g["sent_plan"][0, 0], xt[1, :6, :3])
    # ... and from the non-guided topology back to a guided one
    assert _one(1, 8, sent_time=now - 0.05, last_send=now - 0.05)[0]["reason"][0] == 3
    # 4: same topology, one point further than max_geometric_deviation from the communicated plan; beats time
    g, _, _ = _one(1, 1, sent_time=now - 0.05, last_send=now - 9.0, sent_offset=0.4)
    assert g["reason"][0] == 4                      # 0.4 in x and y: 0.566 > 0.5
    assert _one(1, 1, sent_time=now - 0.05, last_send=now - 0.05, sent_offset=0.3)[0]["reason"][0] == 0
    # ... no communicated plan yet: nothing to deviate from
    assert _one(1, 1, sent_time=math.nan, last_send=now - 0.05, sent_offset=50.0)[0]["reason"][0] == 0
    # 5: never sent, or the heartbeat period has passed (>=)
    assert _one(1, 1, sent_time=now - 0.05, last_send=math.nan)[0]["reason"][0] == 5
    assert _one(1, 1, sent_time=now - 0.05, last_send=now - 2.0)[0]["reason"][0] == 5
    assert _one(1, 1, sent_time=now - 0.05, last_send=now - 1.75)[0]["reason"][0] == 0
    # an explicit topology map: two planners in the same class are no change
    assert _one(1, 4, sent_time=now - 0.05, last_send=now - 0.05, topology=[4, 4, 8])[0]["reason"][0] == 0


def test_filter_off_publishes_everything_with_reason_zero():
    off = fleet.FleetSettings(communicate_on_topology_switch_only=False)
    for best in (-1, 0, 2):
        g, _, _ = _one(best, 0, sent_time=4.0, last_send=4.9, settings=off)
        assert g["reason"].tolist() == [0, 0] and g["published"].tolist() == [1, 1]
        assert g["sent_time"][0, 0] == 5.0 and g["last_send_time"][0, 0] == 5.0
        assert g["prev_topology"][0, 0] == {-1: -1, 0: 0, 2: 8}[best]


def test_a_failed_step_resets_the_topology_so_the_next_success_is_a_change():
    now = 5.0
    g, xt, state = _one(-1, 1, sent_time=now - 0.05, last_send=now - 0.05)
    assert g["prev_topology"][0, 0] == -1
    fs = {k: g[k] for k in ("sent_plan", "sent_time", "last_send_time", "prev_topology")}
    b = np.array([1, 1], np.int32)
    nxt = fleet.publish_host(b, xt, state, fs, now + 0.05, DT, SETTINGS, guided=np.array([[1, 1, 0]] * 2, np.uint8))
    assert nxt["reason"].tolist() == [3, 3] and nxt["prev_topology"][0, 0] == 1    # the topology it had before


def _line_plan(x0, y0, vx, vy, N, dt):
    return [(x0 + vx * k * dt, y0 + vy * k * dt) for k in range(N)], [math.atan2(vy, vx)] * N


def test_obstacle_driver_reproduces_the_tracker_replay():
    """The inputs of test_obstacles.test_recording_replay_through_the_tracker as a 1 x 3 fleet:
    jackal2 publishes at t = 0, jackal3 at t = 0.05, one array obstacle (id 5), lists of 6."""
    N, dt, R = 30, 0.2, 3
    st = fleet.FleetSettings(v_max=2.0, w_max=2.0)       # the tracker's defaults
    p2, a2 = _line_plan(4.0, 0.0, -0.5, 0.0, N, dt)
    p3, a3 = _line_plan(0.0, 4.0, 0.0, -0.5, N, dt)
    arr_pos, arr_ang = _line_plan(8.0, 8.0, 0.0, 0.0, N, dt)
    array_obst = np.zeros((1, 1, N, 5))
    array_obst[0, 0, :, 0:2], array_obst[0, 0, :, 2] = arr_pos, arr_ang
    array_meta = np.array([[[0.325, 1.0]]])
    state = np.array([[0.0, 0.0, 0.0, 1.0, 0.0]] * R)
    fs = fleet.initial_state(1, R, N)
    tr = ob.RobotObstacleTracker(["/jackal1", "/jackal2", "/jackal3"], "/jackal1", 0.325, N, dt, max_obstacles=6)
    for t in (0.0, 0.05, 0.1):
        for q, ns, pos, ang, t_pub in ((1, "/jackal2", p2, a2, 0.0), (2, "/jackal3", p3, a3, 0.05)):
            if t == t_pub:                   # received before this step's prepareObstacleData
                fs["sent_plan"][0, q, :, 0:2], fs["sent_plan"][0, q, :, 2], fs["sent_time"][0, q] = pos, ang, t
                tr.on_trajectory(ns, ob.direct_trajectory_msg(q, (*pos[0], ang[0]), pos, ang, dt, stamp=t), t)
        got = fleet.fleet_obstacles_host(state, fs, t, N, dt, 6, st, array_obst, array_meta, np.array([[5]]))
        fs["sent_plan"], fs["sent_time"] = got["sent_plan"], got["sent_time"]
        arr = ob.obstacles_from_array({"obstacles": [ob.obstacle_gmm_msg(5, 8.0, 8.0, 0.0, arr_pos, arr_ang)]}, 0.325)
        lst = tr.prepare(arr, state[0], t)
    # the expectations of the tracker test, for the ego (robot 0) ...
    assert got["kept"][0] == [("array", 0), ("robot", 1), ("robot", 2)] + [("dummy", -1)] * 3
    np.testing.assert_allclose(got["obst"][0, 1, 0, 0:2], (4.0 - 0.5 * 0.1, 0.0), atol=1e-12)
    np.testing.assert_allclose(got["obst"][0, 2, 0, 0:2], (0.0, 4.0 - 0.5 * 0.05), atol=1e-12)
    assert got["obst"].shape == (R, 6, N, 5) and (got["obst_meta"][0, 3:] == [0.0, 1.0]).all()
    # ... and the tracker's own arrays (a plan's angle goes through a quaternion on its way into the
    # tracker, and comes back to an ulp)
    obst, meta = ob.scene_obstacle_arrays(lst, N)
    np.testing.assert_array_equal(got["obst"][0][:, :, [0, 1, 3, 4]], obst[:, :, [0, 1, 3, 4]])
    np.testing.assert_allclose(got["obst"][0][:, :, 2], obst[:, :, 2], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got["obst_meta"][0], meta)
    assert got["sent_time"].tolist()[0][1:] == [0.1, 0.1]
    # the other robots see the ego's slot empty: robot 1's list has robot 2 only
    assert got["kept"][1][:2] == [("array", 0), ("robot", 2)]


@pytest.mark.parametrize("cfg", ["C1", "C4"])
def test_the_gpu_test_inputs_take_every_branch(cfg):
    """The crafted inputs of tests/test_fleet_gpu.py on the host: every sender's age takes the
    branch it is meant to, the clamp and the +-pi crossing happen, and nothing sits on a decision
    boundary."""
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    lay = config_layout(cfg)
    N, dt = lay.N, lay.dt
    st = fleet.FleetSettings(control_frequency=fr.CASE_CONTROL_FREQUENCY)
    c = fr.obstacles_case(N, dt)
    got = fleet.fleet_obstacles_host(c["state"], c["fstate"], c["now"], N, dt, lay.n_ell, st, c["array_obst"],
                                     c["array_meta"], c["array_id"])
    cut = fr.assert_away_from_boundaries(c, N, dt, lay.n_ell, st.control_frequency, got["sent_plan"])
    shifted = (got["sent_time"] == c["now"]).reshape(-1)
    assert shifted.tolist() == [False, False, False, True, True, True, False, True, True, True, True, True]
    old, new = c["fstate"]["sent_plan"].reshape(-1, N, 3), got["sent_plan"].reshape(-1, N, 3)
    np.testing.assert_array_equal(new[~shifted], old[~shifted])
    np.testing.assert_array_equal(new[5, :N - 1], old[5, 1:])          # alpha <= 0.001: a pure drop of k = 1
    q = fr.CLAMPED_SENDER                                              # extrapolated at v_max, w_max
    step = new[q, N - 1] - new[q, N - 2]
    assert abs(math.hypot(step[0], step[1]) - st.v_max * dt) < 1e-9 and abs(step[2] - st.w_max * dt) < 1e-9
    q = fr.WRAPPING_SENDER
    assert new[q, :, 2].max() > 3.0 and new[q, :, 2].min() < -3.0 and np.abs(new[q, :, 2]).max() <= math.pi
    kept = [src for lst in got["kept"] for src in lst]
    if lay.n_ell < 7:
        assert cut == 12 and ("dummy", -1) not in kept
    else:
        assert cut == 0 and ("dummy", -1) in kept
    assert any(s[0] == "robot" for s in kept)
    # the colliding array obstacle (slot 2, id 1) is replaced where robot 1 has been received, and
    # stays in robot 1's own list
    if lay.n_ell >= 7:
        assert got["kept"][0][2] == ("robot", 1) and ("array", 2) not in got["kept"][0]
        assert got["kept"][1][2] == ("array", 2)


def test_python_binding_lists_the_fleet_symbols_and_mirrors_the_structs():
    """(the functions: tests/test_layer_abi.py)"""
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgFleetSettings, MpcgFleetState
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for struct, mirror in (("mpcg_fleet_settings", MpcgFleetSettings), ("mpcg_fleet_state", MpcgFleetState)):
        body = txt[txt.index(f"typedef struct {struct} {{"):txt.index(f"}} {struct};")]
        names = []
        for decl in re.findall(r"(?:int|double)\s+([^;]+);", body):
            names += [p.replace("*", "").strip() for p in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], struct


def test_limits_are_reported_without_a_launch():
    """Outside the kernels' limits the entry points return -2 with an error text (host-side checks only)."""
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.native_spec import (MpcgFleetSettings, MpcgFleetState,
                                                                   problem_from_layout)
    lib = C.CDLL(LIB)
    lib.mpcg_last_error.restype = C.c_char_p
    pr = problem_from_layout(config_layout("C1"))
    st, fs = MpcgFleetState(1, 1, 1, 1), MpcgFleetSettings()
    vp = C.c_void_p
    lib.mpcg_fleet_obstacles.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp]
    for F, R, A in ((1, 9, 0), (1, 1, 0), (1, 4, 62)):
        rc = lib.mpcg_fleet_obstacles(C.byref(pr), F, R, A, C.byref(fs), C.byref(st), 1, 1, 1, None, 0.0, 1, 1, None)
        assert rc == -2 and b"mpcg_fleet_obstacles" in lib.mpcg_last_error()
    pr5 = problem_from_layout(config_layout("C5"))       # 6 states
    assert lib.mpcg_fleet_obstacles(C.byref(pr5), 1, 4, 0, C.byref(fs), C.byref(st), 1, 1, 1, None, 0.0, 1, 1, None) == -2
    assert lib.mpcg_fleet_obstacles(C.byref(pr), 1, 4, 0, C.byref(fs), None, 1, 1, 1, None, 0.0, 1, 1, None) == -1


def test_counter_profiles_still_match_the_hashed_sources():
    """The fleet sources are linked into libmpcg.so but are not part of source_hash(): the committed
    counter summaries keep matching the solve / producer kernels they were taken on."""
    from oscar_mpc_planner_mr_modification_amd import _build
    with open(os.path.join(ROOT, "profiles", "traffic_C2.json")) as fh:
        assert _build.source_hash() == json.load(fh)["source_sha256"]
    assert _build.LAYERS["mpcg_fleet.h"] == {"sources": {"mpcg_fleet.hip": ["-ffp-contract=off"]},
                                             "headers": ["mpcg_fleet.h"]}
    assert "mpcg_fleet.hip" not in _build.SOURCES and "mpcg_fleet.h" not in _build.HEADERS
    assert not set(_build.LAYER_SHARED_HEADERS) & set(_build.HEADERS)
