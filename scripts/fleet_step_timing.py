#!/usr/bin/env python3
"""What the device-resident multi-robot layer costs per control step: event-timed medians of
fleet.FleetLoop.step and of a bare ControlLoop.step on the same scenes, alternating in one
process after warm-up, and of the fleet layer's launches on their own (mpcg_fleet_obstacles: the
time shift and the obstacle lists; mpcg_fleet_publish).

    python scripts/fleet_step_timing.py [--config C4] [--fleets 512] [--robots 4] [--guesses 8]
                                        [--array 9] [--reps 40] [--warmup 5] [--out FILE]

Default: the C4 layout (N 30, 12 obstacle rows), 512 fleets x 4 robots = 2048 planner scenes as in
C4's bench, 8 planners, 9 array obstacles per fleet (with the 3 other robots: full lists).
Prints one JSON line; needs an MI355X.
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
    ap.add_argument("--config", default="C4")
    ap.add_argument("--fleets", type=int, default=512)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--guesses", type=int, default=8)
    ap.add_argument("--array", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from oscar_mpc_planner_mr_modification_amd import _build, fleet, native
    from oscar_mpc_planner_mr_modification_amd.control_loop import ControlLoop
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import (DECELERATION, ROBOT_RADIUS, SETTINGS_WEIGHTS,
                                                                 make_batch)

    lay = config_layout(args.config)
    F, R, G, A = args.fleets, args.robots, args.guesses, args.array
    S, N = F * R, lay.N
    assert A <= lay.n_ell
    sc = make_batch(lay, S, G, seed=20251212, workers=args.workers).scenes
    array_obst = np.ascontiguousarray(sc.obst.reshape(F, R, lay.n_ell, N, 5)[:, 0, :A])
    array_meta = np.ascontiguousarray(sc.obst_meta.reshape(F, R, lay.n_ell, 2)[:, 0, :A])
    if not torch.cuda.is_available():
        raise SystemExit("fleet_step_timing: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    st = fleet.FleetSettings()
    w_cons, sel_w = SETTINGS_WEIGHTS["consistency"], 0.75
    fl = fleet.FleetLoop(lay, copy.deepcopy(sc), F, R, dev, st, ROBOT_RADIUS, w_cons, sel_w)
    fl.set_array_obstacles(array_obst, array_meta)
    bare = ControlLoop(lay, copy.deepcopy(sc), dev, ROBOT_RADIUS, w_cons, sel_w, DECELERATION)
    period = 1.0 / st.control_frequency
    now = 0.0
    for _ in range(args.warmup):
        fl.step(now)
        bare.step()
        now += period
    # the bare loop solves the fleet's obstacle rows from here on (the same scenes)
    bare.dsc["obst"] = fl.loop.dsc["obst"].clone()
    bare.dsc["obst_meta"] = fl.loop.dsc["obst_meta"].clone()
    bare.step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_fleet, t_bare, t_obst, t_pub, published = [], [], [], [], []
    for _ in range(args.reps):
        t_fleet.append(timed(lambda: fl.step(now), *ev))
        published.append(float(fl.published.float().mean().item()))
        t_bare.append(timed(bare.step, *ev))
        now += period
    # the fleet layer's launches on their own, on the state the loop has reached
    lp, last = fl.loop, fl.loop.last
    for _ in range(args.reps):
        now += period
        t_obst.append(timed(lambda: native.fleet_obstacles_device(
            lp.pr, F, R, fl._set, fl.state, lp.dsc["state"], now, lp.dsc["obst"], lp.dsc["obst_meta"],
            fl.array_obst, fl.array_meta, fl.array_id), *ev))
        t_pub.append(timed(lambda: native.fleet_publish_device(
            lp.pr, F, R, G, fl._set, fl.state, last["best"], last["xtraj"], lp.dsc["state"], now, fl.reason,
            fl.published, guided=lp.dsc["guided"]), *ev))
    f_ms, b_ms = stats(t_fleet), stats(t_bare)
    o_ms, p_ms = stats(t_obst), stats(t_pub)
    out = {"what": "fleet_step_timing", "config": args.config, "fleets": F, "robots": R, "scenes": S, "guesses": G,
           "array_obstacles": A, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "source_sha256": _build.source_hash(),
           "fleet_step": f_ms, "bare_control_loop_step": b_ms,
           "fleet_obstacles_launches": o_ms, "fleet_publish_launch": p_ms,
           "step_ratio_fleet_over_bare": f_ms["median_ms"] / b_ms["median_ms"],
           "fleet_launches_share_of_fleet_step": (o_ms["median_ms"] + p_ms["median_ms"]) / f_ms["median_ms"],
           "published_fraction_mean": float(np.mean(published))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
