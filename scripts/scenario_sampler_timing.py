#!/usr/bin/env python3
"""What the SH-MPC scenario sampler costs per control step at C5's size: event-timed medians, taken in
alternation in one process after warm-up, of
  (a) mpcg_scenario_sample_prepare (samples formed and reduced in one launch, no tensor),
  (b) mpcg_prepare_scenario on the device-resident sample tensor of the same samples,
  (c) mpcg_scenario_samples (writes the tensor) followed by (b),
  (d) each of (a) and (b) followed by the C5 solve;
beside them the bytes each path holds resident, whether (a) and (b) give the same parameters bit for bit, and
the wall time of the host sampler (scenario_sampler.draw_samples + prepare_scenario_sampled_host) on one core
for the first --host-scenes scenes.

    python scripts/scenario_sampler_timing.py [--scenes 2048] [--reps 40] [--warmup 5] [--out FILE]

Default: the C5 layout (N 20, 24 rows), 2048 scenes x 4 copies, 12 obstacles x 100 samples.  Prints one JSON
line; needs an MI355X.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _chunk(args):
    from oscar_mpc_planner_mr_modification_amd import scenario_sampler as ss
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    first, count, P, n_obs, n_per, seed = args
    return ss.make_shmpc_prediction_scenes(config_layout("C5"), count, P, n_obs, n_per, seed=seed, first_scene=first)


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
    ap.add_argument("--scenes", type=int, default=2048)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--obstacles", type=int, default=12)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--seed", type=int, default=20251212)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-scenes", type=int, default=32)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oscar_mpc_planner_mr_modification_amd import scenario_sampler as ss
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import DECELERATION, ROBOT_RADIUS

    lay = config_layout("C5")
    S, P, n_obs, n_per, N = args.scenes, args.copies, args.obstacles, args.samples, lay.N
    # the scenes, generated in worker processes before this process touches the GPU
    t0 = time.perf_counter()
    step = max(1, (S + args.workers - 1) // args.workers)
    jobs = [(f, min(step, S - f), P, n_obs, n_per, args.seed) for f in range(0, S, step)]
    with ProcessPoolExecutor(max_workers=min(args.workers, len(jobs))) as ex:
        parts = list(ex.map(_chunk, jobs))
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])  # noqa: E731
    sc = ss.PredictionScenes(stage_params=cat("stage_params"), state=cat("state"), obst=cat("obst"),
                             obst_meta=cat("obst_meta"), bank=parts[0].bank, n_solvers=P, seed=args.seed,
                             main_warm=cat("main_warm"))
    t_scenes = time.perf_counter() - t0
    # the host sampler on one core, for the first scenes
    H = min(args.host_scenes, S)
    t0 = time.perf_counter()
    bidx = ss.batch_index(sc.seed, 0, S * P, n_obs, sc.bank.shape[0])
    smp = ss.draw_samples(sc.obst[:H], sc.obst_meta[:H], sc.bank, bidx[:H * P], P, N)
    t_draw = time.perf_counter() - t0
    hb = ss.prepare_scenario_sampled_host(lay, sc.stage_params[:H], sc.state[:H], smp, sc.obst_meta[:H], P,
                                          main_warm=sc.main_warm[:H])
    t_host = time.perf_counter() - t0

    import torch
    from oscar_mpc_planner_mr_modification_amd import _build, native
    if not torch.cuda.is_available():
        raise SystemExit("scenario_sampler_timing: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    pr = native.problem_from_layout(lay)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731
    d = {k: t(getattr(sc, k)) for k in ("stage_params", "state", "obst", "obst_meta", "bank", "main_warm")}
    radius = ROBOT_RADIUS + float(sc.obst_meta[0, 0, 0])
    B = S * P
    f64 = dict(dtype=torch.float64, device=dev)
    out_a = dict(params=torch.empty((B, N, pr.npar), **f64), warm=torch.empty((B, N + 1, pr.nu + pr.nx), **f64),
                 xinit=torch.empty((B, pr.nx), **f64))
    out_b = {k: torch.empty_like(v) for k, v in out_a.items()}
    tensor = torch.empty((B, N, n_obs * n_per, 2), **f64)
    sol = native._solve_outputs(pr, B, dev, None, False, False, False)

    def fused():
        native.scenario_sample_prepare_device(pr, P, d["stage_params"], d["state"], d["obst"], d["obst_meta"], d["bank"],
                                              ROBOT_RADIUS, DECELERATION, main_warm=d["main_warm"], seed=sc.seed, draw=0,
                                              out=out_a)

    def write_tensor():
        native.scenario_samples_device(pr, P, d["obst"], d["obst_meta"], d["bank"], seed=sc.seed, draw=0, out=tensor)

    def reduce_tensor():
        native.prepare_scenario_device(pr, P, d["stage_params"], d["state"], tensor, radius, DECELERATION,
                                       main_warm=d["main_warm"], out=out_b)

    def tensor_path():
        write_tensor()
        reduce_tensor()

    def solve(inp):
        return native.solve_batch_device(pr, inp["params"], inp["warm"], inp["xinit"], out=sol)

    def fused_solve():
        fused()
        solve(out_a)

    def reduce_solve():
        reduce_tensor()
        solve(out_b)

    write_tensor()
    fused()
    reduce_tensor()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(out_a[k], out_b[k])) for k in out_a)
    host_same = bool(np.array_equal(out_a["params"][:H * P].cpu().numpy(), hb.params))
    runs = dict(a_sample_prepare=fused, b_prepare_scenario_on_tensor=reduce_tensor,
                c_samples_then_prepare_scenario=tensor_path, d_sample_prepare_plus_solve=fused_solve,
                d_prepare_scenario_plus_solve=reduce_solve)
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn, *ev))
    ok = float((sol["exit"] == 1).float().mean().item())
    nbytes = lambda *ts: int(sum(x.numel() * x.element_size() for x in ts))  # noqa: E731
    res = {k: stats(v) for k, v in ms.items()}
    out = {"what": "scenario_sampler_timing", "config": "C5", "scenes": S, "copies": P, "N": N, "rows": lay.n_scen,
           "obstacles": n_obs, "samples_per_obstacle": n_per, "bank_batches": int(sc.bank.shape[0]),
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "source_sha256": _build.source_hash(), **res,
           "ratio_a_over_b": res["a_sample_prepare"]["median_ms"] / res["b_prepare_scenario_on_tensor"]["median_ms"],
           "fused_equals_tensor_path_bit_for_bit": same, "fused_equals_host_bit_for_bit": host_same,
           "resident_bytes": {"predictions_and_bank": nbytes(d["obst"], d["obst_meta"], d["bank"]),
                              "sample_tensor": nbytes(tensor)},
           "solve_success": ok,
           "host_sampler": {"scenes": H, "draw_samples_wall_s": t_draw, "draw_and_prepare_wall_s": t_host,
                            "scaled_to_all_scenes_s": t_host * S / H},
           "host_scene_generation_wall_s": t_scenes}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
