"""The guidance layer on the GPU (mpcg_guidance_update / _mask / _select, guidance.GuidanceLayer) against
the host restatement (guidance.guidance_update_host, mask_host, select_host) and, in closed loops,
against CPU loops built from the restatement and the oracle solve (tests/guidance_cases.py).

Comparison rule: with the kernel's own heading (cos psi, sin psi, itself within 1e-15 of numpy's)
given to the restatement, every output and all layer state agree bit for bit."""
import copy

import numpy as np
import pytest

import guidance_cases as gc
from oscar_mpc_planner_mr_modification_amd import fleet, producers
from oscar_mpc_planner_mr_modification_amd import guidance as gd
from oscar_mpc_planner_mr_modification_amd import native_spec as ns
from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
from oscar_mpc_planner_mr_modification_amd.synthetic import DECELERATION, ROBOT_RADIUS, step_scenes
from test_control_loop import SEL_W, W_CONS, _next_state

pytestmark = pytest.mark.gpu
STATE_KEYS = ("class_traj", "class_used", "planner_class", "selected_topology", "prev_was_original")
OUT_KEYS = ("guidance", "existing_guidance", "previously_selected", "consistency_on", "topology", "enabled", "n_found",
            "sig_mask", "sig_side", "clearance", "cost")


class _Loop:
    """What GuidanceLayer.update reads of a ControlLoop: the scene tensors."""

    def __init__(self, dsc):
        self.dsc = dsc


@pytest.mark.parametrize("cfg,G,case,best", [("C2", 8, gc.update_case, [0, 1, 7, 0, -1, 0]),
                                             ("JS", 5, gc.js_case, [0, 4])])
def test_update_kernel_matches_the_host_bit_for_bit(cfg, G, case, best):
    """First layout: N 20, 8 obstacle slots, 8 planners, the six scenes of gc.SCENE_NAMES; second: the JS
    layout (N 30, 4 slots, 5 planners), two scenes.  Two consecutive updates (the second with the
    obstacle rows reversed) with a select between them."""
    import torch

    lay = config_layout(cfg)
    assert (lay.N, lay.n_ell) == ((20, 8) if cfg == "C2" else (30, 4))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    S = len(case(lay, 0)[0])
    layer = gd.GuidanceLayer(lay, S, G, dev, gc.SETTINGS)
    hstate = gd.initial_state(S, G, lay.N)
    guided = np.ones((S, G), np.uint8)
    guided[:, G - 1] = 0
    rng = np.random.default_rng(3)
    gdn = rng.normal(size=(S, G, lay.N + 1, 4))
    dsc = dict(guidance=t(gdn), guided=t(guided),
               previously_selected=torch.full((S, G), 9, dtype=torch.uint8, device=dev),
               consistency_on=torch.full((S, G), 9, dtype=torch.uint8, device=dev))
    for step in range(2):
        state, sp, ob, me = case(lay, step)
        dsc.update(state=t(state), stage_params=t(sp), obst=t(ob), obst_meta=t(me))
        layer.update(_Loop(dsc))
        torch.cuda.synchronize()
        heading = layer.heading.cpu().numpy()
        assert np.abs(heading - np.stack([np.cos(state[:, 2]), np.sin(state[:, 2])], 1)).max() <= 1e-15
        host = gd.guidance_update_host(lay, state, sp, ob, me, hstate, gdn, G, gc.SETTINGS, heading=heading)
        got = dict(guidance=dsc["guidance"], previously_selected=dsc["previously_selected"],
                   consistency_on=dsc["consistency_on"],
                   **{k: getattr(layer, k) for k in OUT_KEYS if k not in ("guidance", "previously_selected",
                                                                         "consistency_on")})
        for k in OUT_KEYS:
            g = got[k].cpu().numpy()
            h = host[k].astype(np.int32) if k in ("sig_mask", "sig_side") else host[k]
            np.testing.assert_array_equal(g, h.reshape(g.shape), err_msg=f"{cfg} update {step}: {k}")
        hstate["class_traj"], hstate["class_used"] = host["class_traj"], host["class_used"]
        gdn = host["guidance"]
        # the selection record
        b = np.array(best, np.int32) if step == 0 else np.full(S, -1, np.int32)
        layer.after_select(_Loop(dsc), dict(best=t(b)))
        torch.cuda.synchronize()
        hstate.update(gd.select_host(b, guided, host["topology"], host["enabled"]))
        for k in STATE_KEYS:
            np.testing.assert_array_equal(layer.state[k].cpu().numpy(), hstate[k], err_msg=f"{cfg} step {step}: {k}")
        print(f"{cfg} update {step}: n_found {host['n_found'].tolist()}, topology {host['topology'].tolist()}")
    assert host["existing_guidance"].any() and host["n_found"].max() >= 2


def test_mask_keeps_disabled_planners_out_of_the_selection():
    import torch
    from oscar_mpc_planner_mr_modification_amd import native

    dev = torch.device("cuda:0")
    S, G, N = 3, 4, 6
    rng = np.random.default_rng(1)
    enabled = np.array([[1, 0, 0, 1], [1, 1, 0, 1], [0, 0, 0, 1]], np.uint8)
    # scene 0: the only successful solve is the disabled planner 1; scene 1: the cheapest success is
    # the disabled planner 2; scene 2: only the non-guided planner is enabled
    exit_code = np.array([[0, 1, 2, 4], [1, 1, 1, 3], [1, 1, 1, 1]], np.int32)
    pobj = np.array([[1.0, 0.5, 2.0, 3.0], [5.0, 4.0, 1.0, 0.1], [1.0, 2.0, 3.0, 9.0]])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ex = t(exit_code.reshape(-1))
    native.guidance_mask_device(S, G, t(enabled), ex)
    xt = t(rng.normal(size=(S * G, N + 1, 5)))
    best, _ = native.select_best_device(S, G, N, xt, t(pobj.reshape(-1)), ex)
    torch.cuda.synchronize()
    got = ex.cpu().numpy().reshape(S, G)
    assert (got[enabled == 0] == ns.GUIDANCE_EXIT_DISABLED).all()
    np.testing.assert_array_equal(got[enabled == 1], exit_code[enabled == 1])
    np.testing.assert_array_equal(got.reshape(-1), gd.mask_host(exit_code, enabled))
    assert best.cpu().numpy().tolist() == [-1, 1, 3]


def _carried(c):
    return producers.Carried(main_warm=c["main_warm"].cpu().numpy(), prev_traj=c["prev_traj"].cpu().numpy(),
                             prev_elapsed=c["prev_elapsed"].cpu().numpy(),
                             consistency_on=c["consistency_on"].cpu().numpy() > 0,
                             previously_selected=c["previously_selected"].cpu().numpy() > 0, lam=None)


def test_control_loop_with_the_layer_matches_the_cpu_loop(oracle_mod):
    """gc.LOOP_CASE (C2, 4 scenes x 8 planners), three steps: ControlLoop with the layer against
    gc.GuidanceCpuLoop.  n_found, topology, enabled, best and the exit codes equal at every step,
    successful trajectories within 1e-4 (the tolerance of tests/test_gpu_paths.py's closed loop).  The
    CPU loop takes numpy's cos / sin for the heading: gc.assert_loop_is_decisive checks that no
    clearance or relevance test of it lies within 1e-6 of its threshold, so the last-bit difference
    cannot flip a decision, and that at least one scene changes its set of classes."""
    import producers_oracle
    import torch
    from oscar_mpc_planner_mr_modification_amd.control_loop import ControlLoop

    lay, sc0 = gc.loop_scenes()
    S, G = sc0.n_scenes, sc0.n_guesses
    cpu = gc.GuidanceCpuLoop(lay, copy.deepcopy(sc0), oracle_mod, producers_oracle)
    dev = torch.device("cuda:0")
    layer = gd.GuidanceLayer(lay, S, G, dev, gc.SETTINGS)
    loop = ControlLoop(lay, sc0, dev, ROBOT_RADIUS, W_CONS, SEL_W, DECELERATION, guidance_layer=layer)
    sc, hist = copy.deepcopy(sc0), []
    for t in range(3):
        ref = cpu.step()
        hist.append(ref)
        out = loop.step()
        torch.cuda.synchronize()
        best, ex, xt = out["best"].cpu().numpy(), out["exit"].cpu().numpy(), out["xtraj"].cpu().numpy()
        for k in ("n_found", "topology", "enabled"):
            np.testing.assert_array_equal(getattr(layer, k).cpu().numpy(), ref[k], err_msg=f"step {t}: {k}")
        np.testing.assert_array_equal(ex, ref["exit"], err_msg=f"step {t}")
        np.testing.assert_array_equal(best, ref["best"], err_msg=f"step {t}")
        ok = ex == 1
        assert ok.any() and np.abs(xt[ok] - ref["xtraj"][ok]).max() <= 1e-4
        dg = np.abs(loop.dsc["guidance"].cpu().numpy() - cpu.sc.guidance).max()
        assert dg <= 1e-12
        print(f"step {t}: n_found {ref['n_found'].tolist()}, best {best.tolist()}, success {ok.mean():.2f}, "
              f"max|dx| {np.abs(xt[ok] - ref['xtraj'][ok]).max():.2e}, max|d guidance| {dg:.2e}")
        cpu.advance(best)
        sn = _next_state(xt, best, sc.state, G)
        c = loop.advance(sn)
        # the scene data of the next step from outside: the state and the obstacle rows; the guidance rows
        # (read back from the device) only matter for the disabled planners, whose rows the layer leaves
        sc.guidance = loop.dsc["guidance"].cpu().numpy()
        nxt = step_scenes(lay, sc, sn, _carried(c))
        loop.set_scene_data(nxt.state, nxt.obst, nxt.guidance)
        sc = nxt
    gc.assert_loop_is_decisive(cpu.details, hist)


def test_fleet_loop_with_the_layer_and_no_host_topology(oracle_mod):
    """gc.FLEET_CASE (C2, 2 fleets x 2 robots, 8 planners, 8 array obstacles per fleet), three steps at
    20 Hz: FleetLoop with the layer and no host topology against gc.FleetGuidanceCpuLoop
    (fleet_obstacles_host -> guidance_update_host -> the oracle -> publish_host on the layer's class
    ids).  n_found, topology, enabled, best, exit codes, reason and published equal at every step,
    successful trajectories within 1e-4; the scenes are decisive as in the test above."""
    import producers_oracle
    import torch

    case = gc.fleet_case()
    lay, sc0, F, R, G = case["lay"], case["scenes"], case["F"], case["R"], case["G"]
    S = F * R
    cpu = gc.fleet_cpu_loop(case, copy.deepcopy(sc0), oracle_mod, producers_oracle)
    dev = torch.device("cuda:0")
    layer = gd.GuidanceLayer(lay, S, G, dev, gc.SETTINGS)
    layer.state["selected_topology"].fill_(case["selected_topology"])
    fl = fleet.FleetLoop(lay, sc0, F, R, dev, case["settings"], ROBOT_RADIUS, W_CONS, SEL_W, guidance_layer=layer)
    fl.set_array_obstacles(case["array_obst"], case["array_meta"])
    sc, hist = copy.deepcopy(sc0), []
    for t in range(3):
        now = 0.05 * t
        ref = cpu.step(now)
        hist.append(ref)
        out = fl.step(now)
        torch.cuda.synchronize()
        best, ex, xt = out["best"].cpu().numpy(), out["exit"].cpu().numpy(), out["xtraj"].cpu().numpy()
        for k in ("n_found", "topology", "enabled"):
            np.testing.assert_array_equal(getattr(layer, k).cpu().numpy(), ref[k], err_msg=f"step {t}: {k}")
        np.testing.assert_array_equal(ex, ref["exit"], err_msg=f"step {t}")
        np.testing.assert_array_equal(best, ref["best"], err_msg=f"step {t}")
        np.testing.assert_array_equal(out["reason"].cpu().numpy(), ref["reason"], err_msg=f"step {t}")
        np.testing.assert_array_equal(out["published"].cpu().numpy(), ref["published"], err_msg=f"step {t}")
        np.testing.assert_array_equal(fl.state["prev_topology"].cpu().numpy().reshape(-1),
                                      cpu.publish(best)["prev_topology"].reshape(-1), err_msg=f"step {t}")
        ok = ex == 1
        assert ok.any() and np.abs(xt[ok] - ref["xtraj"][ok]).max() <= 1e-4
        print(f"step {t}: n_found {ref['n_found'].tolist()}, best {best.tolist()}, reasons {ref['reason'].tolist()}, "
              f"max|dx| {np.abs(xt[ok] - ref['xtraj'][ok]).max():.2e}")
        cpu.advance(best)
        sn = _next_state(xt, best, sc.state, G)
        c = fl.advance(sn)
        sc.guidance = fl.loop.dsc["guidance"].cpu().numpy()
        nxt = step_scenes(lay, sc, sn, _carried(c))
        fl.loop.set_scene_data(nxt.state, nxt.obst, nxt.guidance)     # (the obstacle rows are the fleet's own)
        sc = nxt
    gc.assert_loop_is_decisive(cpu.details, hist)
    assert any((h["best"] == G - 1).any() for h in hist)
