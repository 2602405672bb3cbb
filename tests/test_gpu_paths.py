"""Reference-path tracking on the GPU (mpcg_path_update / mpcg_path_command, paths.PathLoop) against
the host restatement (paths.path_update_host, paths.command_host) and, in a closed loop, against the
CPU loop of tests/path_cases.py (the oracle solve around path_update_host).

Comparison rule: segments, closest_s, the window, reached and the command bit for bit; the two
positions the stand-in plant derives with cos / sin to 1e-12."""
import copy

import numpy as np
import pytest

import path_cases as pc
from oscar_mpc_planner_mr_modification_amd import paths, producers
from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
from oscar_mpc_planner_mr_modification_amd.synthetic import ROBOT_RADIUS, step_scenes
from test_control_loop import SEL_W, W_CONS, _next_state

pytestmark = pytest.mark.gpu
TOL = 1e-12


def test_update_kernel_matches_the_host_bit_for_bit():
    """7 scenes over 3 paths of 3, 12 and 64 segments (pc.update_case): inside a segment, exactly on a
    knot, uninitialised starts, the last segment, beyond the end, a window past the end; two
    consecutive updates, the second from the first one's closest_segment."""
    import torch
    from oscar_mpc_planner_mr_modification_amd import native

    lay = config_layout("C2")
    c = pc.update_case(lay)
    S = len(c["path_of"])
    assert S == 7
    i0 = lay.idx("spline_x0_a")
    dev = torch.device("cuda:0")
    pr = native.problem_from_layout(lay)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dtab = native.path_table_device(c["table"], c["path_of"], dev)
    seg = t(c["closest_segment"])
    cs = torch.full((S,), float("nan"), dtype=torch.float64, device=dev)
    sp = t(c["stage_params"])
    reached = torch.full((S,), 9, dtype=torch.uint8, device=dev)
    h_seg, h_sp = c["closest_segment"], c["stage_params"]
    seen = []
    for k in range(2):
        host = paths.path_update_host(c["state"][k], h_seg, c["table"], c["path_of"], h_sp, i0, lay.n_seg)
        native.path_update_device(pr, dtab, t(c["state"][k]), seg, cs, sp, reached)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(seg.cpu().numpy(), host["closest_segment"], err_msg=f"update {k}")
        np.testing.assert_array_equal(cs.cpu().numpy(), host["closest_s"], err_msg=f"update {k}")
        np.testing.assert_array_equal(sp.cpu().numpy(), host["stage_params"], err_msg=f"update {k}")
        np.testing.assert_array_equal(reached.cpu().numpy(), host["reached"], err_msg=f"update {k}")
        h_seg, h_sp = host["closest_segment"], host["stage_params"]
        seen.append(host)
        print(f"update {k}: segments {host['closest_segment'].tolist()}, reached {host['reached'].tolist()}")
    pc.assert_update_case(*seen)
    # everything outside the window is untouched
    keep = np.delete(np.arange(lay.npar), np.arange(i0, i0 + 9 * lay.n_seg))
    np.testing.assert_array_equal(sp.cpu().numpy()[:, keep], c["stage_params"][:, keep])


@pytest.mark.parametrize("plant", [True, False])
def test_command_kernel_matches_command_host(plant):
    import torch
    from oscar_mpc_planner_mr_modification_amd import native

    lay = config_layout("C1")
    c = pc.command_case(N=lay.N, nx=lay.nx, nu=lay.nu)
    S, G = len(c["best"]), c["G"]
    assert S == 5 and (c["best"] < 0).any()
    st = paths.PathSettings(control_frequency=20.0, deceleration=3.0, plant=plant)
    host = paths.command_host(c["best"], c["xtraj"], c["utraj"], c["state"], st, c["closest_s"], pc.SPLINE_SLOT)
    dev = torch.device("cuda:0")
    pr = native.problem_from_layout(lay)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cmd = torch.full((S, 2), float("nan"), dtype=torch.float64, device=dev)
    nxt = torch.full((S, lay.nx), -77.0, dtype=torch.float64, device=dev)
    native.path_command_device(pr, G, st.native(), t(c["best"]), t(c["xtraj"]), t(c["utraj"]), t(c["state"]), cmd,
                               closest_s=t(c["closest_s"]), spline_slot=pc.SPLINE_SLOT, state_next=nxt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cmd.cpu().numpy(), host["cmd"])
    got = nxt.cpu().numpy()
    if plant:
        np.testing.assert_array_equal(got[:, 2:], host["state_next"][:, 2:])
        assert np.abs(got[:, :2] - host["state_next"][:, :2]).max() <= TOL
    else:
        assert (got == -77.0).all()


@pytest.mark.parametrize("name", ["C2", "C1"])
def test_path_loop_matches_the_cpu_loop(oracle_mod, name):
    """C2, 4 scenes x 8 planners, the next state from the winner's stage 1; C1, 3 x 5, the next state
    from the stand-in plant; 4 steps each.  Exit codes equal, successful trajectories within 1e-4,
    closest_segment equal at every step; on the CPU loop the fast scenes cross a knot and no closest_s
    comes within 1e-3 of one (pc.assert_cpu_loop_moves_the_window)."""
    import producers_oracle
    import torch

    case = pc.loop_case(name)
    lay, sc0, S, G, st = case["lay"], case["scenes"], case["S"], case["G"], case["settings"]
    cpu = pc.PathCpuLoop(case, copy.deepcopy(sc0), oracle_mod, producers_oracle)
    dev = torch.device("cuda:0")
    loop = paths.PathLoop(lay, sc0, case["table"], case["path_of"], dev, st, ROBOT_RADIUS, W_CONS, SEL_W,
                          spline_slot=pc.SPLINE_SLOT)
    sc, hist = sc0, []
    for t in range(4):
        ref = cpu.step()
        hist.append(ref)
        out = loop.step()
        torch.cuda.synchronize()
        best, ex, xt = out["best"].cpu().numpy(), out["exit"].cpu().numpy(), out["xtraj"].cpu().numpy()
        np.testing.assert_array_equal(out["closest_segment"].cpu().numpy(), ref["closest_segment"], err_msg=f"step {t}")
        np.testing.assert_array_equal(out["reached"].cpu().numpy(), ref["reached"], err_msg=f"step {t}")
        ds = np.abs(out["closest_s"].cpu().numpy() - ref["closest_s"]).max()
        i0 = cpu.i0
        np.testing.assert_array_equal(loop.loop.dsc["stage_params"].cpu().numpy()[:, i0:i0 + 9 * lay.n_seg],
                                      ref["window"], err_msg=f"step {t}")
        np.testing.assert_array_equal(ex, ref["exit"], err_msg=f"step {t}")
        ok = ex == 1
        assert ok.any() and np.abs(xt[ok] - ref["xtraj"][ok]).max() <= 1e-4
        # a different winner only where the two winners' objectives tie to rounding, as in
        # tests/test_control_loop.py; the CPU loop then carries the GPU's choice
        for s_ in np.flatnonzero(best != ref["best"]):
            a, b = int(best[s_]), int(ref["best"][s_])
            assert a >= 0 and b >= 0, (t, s_, a, b)
            assert abs(ref["obj"][s_, a] - ref["obj"][s_, b]) <= 1e-9 * max(1.0, abs(ref["obj"][s_, b]))
            assert np.abs(ref["xtraj"][s_ * G + a] - ref["xtraj"][s_ * G + b]).max() <= 1e-6
        # the command from the GPU's own winner and state
        want = paths.command_host(best, xt, out["utraj"].cpu().numpy(), loop.loop.dsc["state"].cpu().numpy(), st)
        np.testing.assert_array_equal(out["cmd"].cpu().numpy(), want["cmd"], err_msg=f"step {t}")
        print(f"{name} step {t}: segments {ref['closest_segment'].tolist()}, success {ok.mean():.2f}, "
              f"max|dx| {np.abs(xt[ok] - ref['xtraj'][ok]).max():.2e}, max|d closest_s| {ds:.2e}")
        cpu.advance(best)
        c = loop.advance(None if st.plant else _next_state(xt, best, sc.state, G))
        sn = loop.loop.dsc["state"].cpu().numpy()
        # the spline entry of the next state is this step's closest_s
        np.testing.assert_array_equal(sn[:, pc.SPLINE_SLOT], out["closest_s"].cpu().numpy())
        nxt = step_scenes(lay, sc, sn, producers.Carried(
            main_warm=c["main_warm"].cpu().numpy(), prev_traj=c["prev_traj"].cpu().numpy(),
            prev_elapsed=c["prev_elapsed"].cpu().numpy(), consistency_on=c["consistency_on"].cpu().numpy() > 0,
            previously_selected=c["previously_selected"].cpu().numpy() > 0, lam=None))
        loop.loop.set_scene_data(nxt.state, nxt.obst, nxt.guidance)
        sc = nxt
    pc.assert_cpu_loop_moves_the_window(case, hist)
