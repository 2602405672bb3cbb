#!/usr/bin/env python3
"""What skipping the solves of disabled planners saves per control step: ControlLoop.step with a
guidance.GuidanceLayer, skip_disabled on and off alternating in one process after warm-up (off is the
masked loop: every planner solved, the disabled ones masked afterwards), timed with device events and
with the wall clock around a synchronised step, because the skipping step synchronises once itself.
Also: the same pair with every planner enabled (the layer's `enabled` overridden to all ones), where
gather + scatter + the synchronisation buy nothing, and the new launches on their own (mpcg_active_plan,
mpcg_active_gather, the 4-byte count copy with its synchronisation, mpcg_active_scatter) next to the
full and the dense mpcg_solve.

    python scripts/active_step_timing.py [--config C2] [--scenes 1024] [--guesses 8] [--reps 40]
                                         [--warmup 5] [--out FILE]

Default: the C2 bench layout, 1024 scenes x 8 planners.  Prints one JSON line; needs an MI355X.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from oscar_mpc_planner_mr_modification_amd import _build, guidance, native
    from oscar_mpc_planner_mr_modification_amd.control_loop import ControlLoop
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import (DECELERATION, ROBOT_RADIUS, SETTINGS_WEIGHTS,
                                                                 make_batch)

    lay = config_layout(args.config)
    S, G = args.scenes, args.guesses
    B = S * G
    sc = make_batch(lay, S, G, seed=20251212, workers=args.workers).scenes
    if not torch.cuda.is_available():
        raise SystemExit("active_step_timing: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    w_cons, sel_w = SETTINGS_WEIGHTS["consistency"], 0.75
    st = guidance.GuidanceSettings(robot_radius=ROBOT_RADIUS, v_ref=SETTINGS_WEIGHTS["reference_velocity"])

    class AllEnabled(guidance.GuidanceLayer):
        """the layer with its `enabled` overridden to all ones after every update"""

        def update(self, loop, stream=None):
            super().update(loop, stream=stream)
            self.enabled.fill_(1)

    def make(cls, skip):
        return ControlLoop(lay, copy.deepcopy(sc), dev, ROBOT_RADIUS, w_cons, sel_w, DECELERATION,
                           guidance_layer=cls(lay, S, G, dev, st), skip_disabled=skip)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        """(device-event ms, wall ms of the call with the device drained before and after)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]), 1e3 * (time.perf_counter() - t0)

    def pair(cls):
        off, on = make(cls, False), make(cls, True)
        for _ in range(args.warmup):
            off.step()
            on.step()
        r = {"masked": [], "skipping": []}
        for _ in range(args.reps):
            r["masked"].append(timed(off.step))
            r["skipping"].append(timed(on.step))
        res = {}
        for k, v in r.items():
            v = np.asarray(v)
            res[k] = {"events": stats(v[:, 0]), "wall": stats(v[:, 1])}
        m, s = res["masked"]["events"], res["skipping"]["events"]
        res["saving_ms"] = m["median_ms"] - s["median_ms"]
        res["masked_p10_p90_spread_ms"] = m["p90_ms"] - m["p10_ms"]
        res["saving_exceeds_masked_spread"] = bool(res["saving_ms"] > res["masked_p10_p90_spread_ms"])
        res["wall_saving_ms"] = res["masked"]["wall"]["median_ms"] - res["skipping"]["wall"]["median_ms"]
        res["active_share"] = on.last["n_active"] / B
        res["mean_classes_found"] = float(on.guidance_layer.n_found.float().mean().item())
        res["same_best"] = bool(torch.equal(off.last["best"], on.last["best"]))
        res["success"] = float((on.last["best"] >= 0).float().mean().item())
        return res, on

    natural, on = pair(guidance.GuidanceLayer)
    every, _ = pair(AllEnabled)

    # the new launches on their own, on the last step's inputs of the skipping loop
    pr, prep, enabled = on.pr, on.last["prepared"], on.guidance_layer.enabled.reshape(-1)
    slot_of, solve_of, n_dev = native.active_plan_device(enabled)
    full_in = dict(params=prep["params"], warm=prep["warm"], xinit=prep["xinit"], lam_in=on.lam)
    dense_in = {k: torch.empty_like(v) for k, v in full_in.items()}
    full_out = native.solve_batch_device(pr, prep["params"], prep["warm"], prep["xinit"], lam_in=on.lam, lam_out=True)
    dense_out = {k: torch.empty_like(v) for k, v in full_out.items()}
    back = {k: torch.empty_like(v) for k, v in full_out.items()}
    back["warm"] = prep["warm"]
    pinned = torch.empty((1,), dtype=torch.int32).pin_memory()
    n = int(n_dev.cpu()[0])

    def count_to_host():
        pinned.copy_(n_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    calls = {
        "active_plan_launch": lambda: native.active_plan_device(enabled, slot_of, solve_of, n_dev),
        "active_gather_launch": lambda: native.active_gather_device(pr, slot_of, full_in, dense_in),
        "count_copy_and_synchronise": count_to_host,
        "active_scatter_launch": lambda: native.active_scatter_device(pr, slot_of, dense_out, back),
        "full_solve_launch": lambda: native.solve_batch_device(pr, prep["params"], prep["warm"], prep["xinit"],
                                                               out=full_out, lam_in=on.lam, lam_out=True),
        "dense_solve_launch": lambda: native.solve_batch_device(pr, dense_in["params"][:n], dense_in["warm"][:n],
                                                                dense_in["xinit"][:n],
                                                                out={k: v[:n] for k, v in dense_out.items()},
                                                                lam_in=dense_in["lam_in"][:n], lam_out=True),
    }
    launches = {}
    for k, fn in calls.items():
        for _ in range(args.warmup):
            fn()
        v = np.asarray([timed(fn) for _ in range(args.reps)])
        launches[k] = {"events": stats(v[:, 0]), "wall": stats(v[:, 1])}
    out = {"what": "active_step_timing", "config": args.config, "scenes": S, "guesses": G, "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "source_sha256": _build.source_hash(),
           "layer_natural_share": natural, "every_planner_enabled": every, "launches": launches,
           "launch_active_solves": n,
           "bytes_gathered_per_active_solve": 8 * sum(int(v[0].numel()) for v in full_in.values()),
           "bytes_scattered_per_solve": sum(int(v[0].numel()) * v.element_size() for v in full_out.values())}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
