#!/usr/bin/env python3
"""What the road-boundary halfspaces cost per control step: event-timed medians of paths.PathLoop.step
on the C2R layout with a road (mpcg_road_halfspaces + the Cfg<20, 10, 8, 0, 5, 0> solve) and on the C2
layout without one, the same scenes, alternating in one process after warm-up; and of the
mpcg_road_halfspaces launch on its own next to mpcg_path_update's.

    python scripts/road_step_timing.py [--scenes 1024] [--guesses 8] [--width 6.0] [--reps 40]
                                       [--warmup 5] [--out FILE]

Default: the C2 bench batch, 1024 scenes x 8 planners, the shipped road width; every scene follows its
own path, a table of its five synthetic segments.  Prints one JSON line; needs an MI355X.
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
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--guesses", type=int, default=8)
    ap.add_argument("--width", type=float, default=6.0)
    ap.add_argument("--two-way", action="store_true")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from oscar_mpc_planner_mr_modification_amd import _build, native, paths, roads
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import (DECELERATION, ROBOT_RADIUS, SETTINGS_WEIGHTS,
                                                                 make_batch)

    if not torch.cuda.is_available():
        raise SystemExit("road_step_timing: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    S, G = args.scenes, args.guesses
    st = paths.PathSettings(control_frequency=20.0, deceleration=DECELERATION, plant=True)
    road = roads.RoadSettings(width=args.width, two_way=args.two_way, robot_radius=ROBOT_RADIUS)
    w_cons, sel_w = SETTINGS_WEIGHTS["consistency"], 0.75
    loops = {}
    for cfg in ("C2R", "C2"):
        lay = config_layout(cfg)
        # the same scenes on both layouts (the generator does not read n_lin)
        sc = make_batch(lay, S, G, seed=20251212, workers=args.workers).scenes
        i0, m = lay.idx("spline_x0_a"), lay.n_seg - 1
        win = sc.stage_params[:, i0:i0 + 9 * lay.n_seg].reshape(S, lay.n_seg, 9)
        table = paths.PathTable(np.ascontiguousarray(win[:, :m, :8]), np.ascontiguousarray(win[:, :, 8]),
                                np.full(S, m, np.int32))
        loops[cfg] = paths.PathLoop(lay, copy.deepcopy(sc), table, np.arange(S), dev, st, ROBOT_RADIUS, w_cons, sel_w,
                                    road=road if cfg == "C2R" else None)
    rl, pl = loops["C2R"], loops["C2"]
    for _ in range(args.warmup):
        rl.step()
        pl.step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_road, t_plain, t_launch, t_upd = [], [], [], []
    for _ in range(args.reps):
        t_road.append(timed(rl.step, *ev))
        t_plain.append(timed(pl.step, *ev))
    lp = rl.loop
    prep = lp.last["prepared"]
    for _ in range(args.reps):
        t_launch.append(timed(lambda: native.road_halfspaces_device(
            lp.pr, G, lp.lay.max_obstacles, lp._road, lp.road_table, prep["params"], state=lp.dsc["state"],
            main_warm=lp.dsc.get("main_warm"), guided=lp.dsc["guided"], deceleration=lp.dec,
            halfspaces=lp.road_halfspaces), *ev))
        t_upd.append(timed(lambda: native.path_update_device(
            lp.pr, rl.table, lp.dsc["state"], rl.closest_segment, rl.closest_s, lp.dsc["stage_params"], rl.reached),
            *ev))
    r_ms, p_ms, l_ms, u_ms = stats(t_road), stats(t_plain), stats(t_launch), stats(t_upd)
    ok_r = float((rl.loop.last["exit"] == 1).float().mean().item())
    ok_p = float((pl.loop.last["exit"] == 1).float().mean().item())
    out = {"what": "road_step_timing", "scenes": S, "guesses": G, "road_width": args.width, "two_way": args.two_way,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "source_sha256": _build.source_hash(),
           "c2r_path_step_with_road": r_ms, "c2_path_step": p_ms, "road_halfspaces_launch": l_ms,
           "path_update_launch": u_ms,
           "c2r_over_c2": r_ms["median_ms"] / p_ms["median_ms"],
           "road_launch_share_of_c2r_step": l_ms["median_ms"] / r_ms["median_ms"],
           "success_share_c2r": ok_r, "success_share_c2": ok_p}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
