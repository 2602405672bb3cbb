#!/usr/bin/env python3
"""What the device-resident reference-path tracking costs per control step: event-timed medians of
paths.PathLoop.step and of a bare ControlLoop.step on the same scenes, alternating in one process
after warm-up, and of the two new launches on their own (mpcg_path_update, mpcg_path_command).

    python scripts/path_step_timing.py [--config C2] [--scenes 1024] [--guesses 8] [--reps 40]
                                       [--warmup 5] [--out FILE]

Default: the C2 bench layout, 1024 scenes x 8 planners; every scene follows its own path, a table of
its five synthetic segments.  Prints one JSON line; needs an MI355X.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, start, end):
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)),
            "p90_ms": float(np.percentile(ms, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--guesses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from oscar_mpc_planner_mr_modification_amd import _build, native, paths
    from oscar_mpc_planner_mr_modification_amd.control_loop import ControlLoop
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import (DECELERATION, ROBOT_RADIUS, SETTINGS_WEIGHTS,
                                                                 make_batch)

    lay = config_layout(args.config)
    S, G = args.scenes, args.guesses
    sc = make_batch(lay, S, G, seed=20251212, workers=args.workers).scenes
    # every scene's path: its synthetic window as a table of n_seg - 1 segments (the last segment's
    # start is the end knot), so the windows the update writes run past the end for some scenes
    i0, m = lay.idx("spline_x0_a"), lay.n_seg - 1
    win = sc.stage_params[:, i0:i0 + 9 * lay.n_seg].reshape(S, lay.n_seg, 9)
    table = paths.PathTable(np.ascontiguousarray(win[:, :m, :8]), np.ascontiguousarray(win[:, :, 8]),
                            np.full(S, m, np.int32))
    if not torch.cuda.is_available():
        raise SystemExit("path_step_timing: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    st = paths.PathSettings(control_frequency=20.0, deceleration=DECELERATION, plant=True)
    w_cons, sel_w = SETTINGS_WEIGHTS["consistency"], 0.75
    pl = paths.PathLoop(lay, copy.deepcopy(sc), table, np.arange(S), dev, st, ROBOT_RADIUS, w_cons, sel_w)
    bare = ControlLoop(lay, copy.deepcopy(sc), dev, ROBOT_RADIUS, w_cons, sel_w, DECELERATION)
    for _ in range(args.warmup):
        pl.step()
        bare.step()
    # the bare loop solves the path loop's windows from here on (the same scenes)
    bare.dsc["stage_params"] = pl.loop.dsc["stage_params"].clone()
    bare.step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_path, t_bare, t_upd, t_cmd = [], [], [], []
    for _ in range(args.reps):
        t_path.append(timed(pl.step, *ev))
        t_bare.append(timed(bare.step, *ev))
    lp, last = pl.loop, pl.loop.last
    for _ in range(args.reps):
        t_upd.append(timed(lambda: native.path_update_device(
            lp.pr, pl.table, lp.dsc["state"], pl.closest_segment, pl.closest_s, lp.dsc["stage_params"], pl.reached),
            *ev))
        t_cmd.append(timed(lambda: native.path_command_device(
            lp.pr, G, pl._set, last["best"], last["xtraj"], last["utraj"], lp.dsc["state"], pl.cmd,
            closest_s=pl.closest_s, spline_slot=pl.spline_slot, state_next=pl.state_next), *ev))
    p_ms, b_ms, u_ms, c_ms = stats(t_path), stats(t_bare), stats(t_upd), stats(t_cmd)
    diff = p_ms["median_ms"] - b_ms["median_ms"]
    out = {"what": "path_step_timing", "config": args.config, "scenes": S, "guesses": G, "path_segments": m,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "source_sha256": _build.source_hash(),
           "path_step": p_ms, "bare_control_loop_step": b_ms, "path_update_launch": u_ms, "path_command_launch": c_ms,
           "step_difference_ms": diff,
           "difference_inside_bare_p10_p90": bool(b_ms["p10_ms"] - b_ms["median_ms"] <= diff
                                                  <= b_ms["p90_ms"] - b_ms["median_ms"]),
           "path_launches_share_of_path_step": (u_ms["median_ms"] + c_ms["median_ms"]) / p_ms["median_ms"],
           "reached_fraction": float(pl.reached.float().mean().item())}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
