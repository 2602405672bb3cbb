#!/usr/bin/env python3
"""What the decomp halfspaces cost per control step at C3's size: event-timed medians of the
mpcg_decomp_halfspaces launch on its own, and of launch + C3 solve alternating with the bare solve on the
same parameters in one process after warm-up; beside them the wall time of the host generator
(decomp.decomp_halfspaces_host) for the same scenes, whose rows the device's are compared with bit for bit.

    python scripts/decomp_step_timing.py [--config C3] [--scenes 4096] [--reps 40] [--warmup 5] [--out FILE]

Default: the C3 layout (N 30, 12 rows), 4096 scenes of decomp.make_c3_decomp_scenes with the generator's
point counts.  Prints one JSON line; needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--config", default="C3")
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=20251212)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from oscar_mpc_planner_mr_modification_amd import _build, decomp, native
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout

    if not torch.cuda.is_available():
        raise SystemExit("decomp_step_timing: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    lay = config_layout(args.config)
    S, N, nd = args.scenes, lay.N, lay.n_scen
    t0 = time.perf_counter()
    sc = decomp.make_c3_decomp_scenes(lay, S, args.seed)
    t_scenes = time.perf_counter() - t0
    st = decomp.DecompSettings()
    t0 = time.perf_counter()
    h = decomp.decomp_halfspaces_host(st, sc.table, sc.path_of, sc.xinit, sc.warm, sc.occ, sc.n_occ, N, lay.dt, lay.nu,
                                      nd)
    host_params = decomp.apply_decomp_host(lay, sc.params, 1, h["rows"])
    t_host = time.perf_counter() - t0
    pr = native.problem_from_layout(lay)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dtab = native.path_table_device(sc.table, sc.path_of, dev)
    pts = native.decomp_points_device(sc.occ, sc.n_occ, dev)
    params, warm, xinit = t(sc.params), t(sc.warm), t(sc.xinit)
    nf = torch.zeros((S, N), dtype=torch.int32, device=dev)

    def launch():
        native.decomp_halfspaces_device(pr, 1, st.native(), dtab, pts, params, xinit, main_warm=warm, n_found=nf)

    def solve():
        return native.solve_batch_device(pr, params, warm, xinit)

    def step():
        launch()
        return solve()

    launch()
    torch.cuda.synchronize()
    same = bool(np.array_equal(params.cpu().numpy().view(np.int64), host_params.view(np.int64)) and
                np.array_equal(nf.cpu().numpy(), h["n_found"]))
    for _ in range(args.warmup):
        step()
        solve()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_step, t_bare, t_launch = [], [], []
    for _ in range(args.reps):
        t_step.append(timed(step, *ev))
        t_bare.append(timed(solve, *ev))
    for _ in range(args.reps):
        t_launch.append(timed(launch, *ev))
    out_solve = solve()
    torch.cuda.synchronize()
    s_ms, b_ms, l_ms = stats(t_step), stats(t_bare), stats(t_launch)
    nfh = h["n_found"][:, 1:]
    out = {"what": "decomp_step_timing", "config": args.config, "scenes": S, "N": N, "max_constraints": nd,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "source_sha256": _build.source_hash(),
           "points_per_scene": {"min": int(sc.n_occ.min()), "median": float(np.median(sc.n_occ)),
                                "max": int(sc.n_occ.max()), "P": int(sc.occ.shape[1])},
           "n_found": {"max": int(nfh.max()), "mean": float(nfh.mean()), "above_rows": int((nfh > nd).sum())},
           "device_rows_equal_host_bit_for_bit": same,
           "decomp_launch": l_ms, "launch_plus_solve": s_ms, "bare_solve": b_ms,
           "step_ratio_with_over_bare": s_ms["median_ms"] / b_ms["median_ms"],
           "solve_success": float((out_solve["exit"] == 1).float().mean().item()),
           "host_generator_wall_s": t_host, "host_scene_generation_wall_s": t_scenes}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
