"""bench.py's launch contract, checked without a GPU: `bench.py --gpus N` starts its own
N ranks (a child torch.distributed.run) when no launcher is present, --gpus must match a
launcher's world size, and both are decided before any GPU call."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_spawns_its_own_ranks():
    """plain `bench.py --gpus 2` (no launcher) runs two ranks that rendezvous on 127.0.0.1;
    rank 0 alone prints, and it saw both ranks (--spawn-check: the rank plumbing on gloo)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--spawn-check"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["ranks_seen"] == 2 and line["n_gpus"] == 2
    assert line["gather_ok"], line


def test_gpus_8_spawns_eight_ranks_and_gathers_the_c4_shards():
    """the width the driver's scaling run uses: `bench.py --gpus 8` (no launcher) starts eight ranks,
    and the step's winner all-gather is exact over BASELINE config 4's 16,384 scenes (2,048 per rank,
    N 30 records) and over an uneven 16,387-scene sharding"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--config", "C4", "--spawn-check"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["ranks_seen"] == 8 and line["n_gpus"] == 8
    assert line["scenes_per_rank"] == 2048 and line["gather_even_scenes"] == 16384
    assert line["gather_uneven_scenes"] == 16387 and line["gather_ok"], line


def test_gpus_flag_must_match_launcher_world_size():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK")}
    env["WORLD_SIZE"] = "1"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr and "torch.distributed.run" in r.stderr


def test_cpu_share_is_bounded_by_the_host():
    sys.path.insert(0, ROOT)
    import bench
    s = bench.cpu_share()
    assert 1 <= s["share"] <= s["affinity"] <= s["nproc"]


def test_unknown_collective_backend_is_refused():
    """MPCG_BENCH_BACKEND selects RCCL (default) or the gloo rehearsal; anything else stops
    before any GPU call."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["MPCG_BENCH_BACKEND"] = "mpi"
    r = subprocess.run([sys.executable, "bench.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "MPCG_BENCH_BACKEND=mpi" in r.stderr


def test_dump_outputs_writes_float64_and_samples_a_larger_output(tmp_path):
    """--dump-outputs: one float64 <name>.npy per output, integers exact; above the byte budget
    every array keeps the same seeded rows (arrays of one row count the same rows), the files
    stay within the budget, and a second call writes the same bytes"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(7)
    arrays = {"xtraj": rng.standard_normal((300, 21, 5)), "pobj": rng.standard_normal(300),
              "exit": rng.integers(-3, 2, 300).astype(np.int32), "winners": rng.standard_normal((37, 11))}
    rows = bench.dump_outputs(str(tmp_path / "all"), arrays)
    assert rows == {"xtraj": 300, "pobj": 300, "exit": 300, "winners": 37}
    for k, a in arrays.items():
        got = np.load(tmp_path / "all" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    budget = 100_000
    rows = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    assert 0 < rows["xtraj"] == rows["pobj"] == rows["exit"] < 300 and 0 < rows["winners"] < 37
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    for k in arrays:
        assert (tmp_path / "a" / (k + ".npy")).read_bytes() == (tmp_path / "b" / (k + ".npy")).read_bytes()
    # the sample is rows of the output, in order; arrays of one row count keep the same rows
    x, p = np.load(tmp_path / "a" / "xtraj.npy"), np.load(tmp_path / "a" / "pobj.npy")
    idx = [int(np.flatnonzero(arrays["pobj"] == v)[0]) for v in p]
    assert idx == sorted(idx) and np.array_equal(x, arrays["xtraj"][idx])


@pytest.mark.gpu
def test_plain_run_times_its_steps_only_and_dumps_the_last_step(tmp_path):
    """a plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line without the legs that
    take runs of their own (other QP profile, CPU baseline, oracle parity: --full), and
    --dump-outputs writes the last timed step's outputs: finite float64 arrays of the batch's shapes
    whose winner records are rows of the dumped solves"""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--scenes", "16",
                        "--dump-outputs", str(d)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "solves/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    # value = solves per second of the timed steps: 16 scenes x 8 guesses per step
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / (16 * 8) - 1) < 1e-3
    assert not {"qp_profile_alt", "cpu_baseline", "vs_cpu_baseline", "parity"} & set(line)
    shapes = {"xtraj": (128, 21, 5), "utraj": (128, 20, 2), "pobj": (128,), "exit": (128,), "info": (128, 4)}
    out = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(out) == set(shapes) | {"winners"}
    for k, a in out.items():
        assert a.dtype == np.float64 and a.shape[0] in (16, 128)
        assert k == "winners" or a.shape == shapes[k]
    ok = out["exit"] == 1
    assert ok.any() and np.isfinite(out["xtraj"][ok]).all() and np.isfinite(out["pobj"][ok]).all()
    assert line["solver_stats"]["success_frac"] == ok.mean()
    # winners: xtraj | utraj | pobj | planner index of the selected planner (index -1: planner 0's)
    w = out["winners"]
    assert w.shape == (16, 21 * 5 + 20 * 2 + 2)
    pick = np.arange(16) * 8 + np.maximum(w[:, -1], 0).astype(int)
    assert np.array_equal(w[:, :105], out["xtraj"][pick].reshape(16, -1), equal_nan=True)
    assert np.array_equal(w[:, 105:145], out["utraj"][pick].reshape(16, -1), equal_nan=True)
    assert np.array_equal(w[:, 145], out["pobj"][pick], equal_nan=True)


def test_source_hash_tracks_kernel_sources():
    sys.path.insert(0, ROOT)
    from oscar_mpc_planner_mr_modification_amd import _build
    h = _build.source_hash()
    assert len(h) == 64 and h == _build.source_hash()


def test_flop_model_uses_executed_iterations():
    """roofline.achieved counts the algorithm's fp64 operations (flopmodel.py) times the SQP and
    IPM iterations each solve executed: linear in both counts, more rows -> more operations."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from oscar_mpc_planner_mr_modification_amd import flopmodel
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    c1, c2, c4 = (config_layout(c) for c in ("C1", "C2", "C4"))
    lin, ipm = flopmodel.linearisation_ops(c2), flopmodel.ipm_iteration_ops(c2)
    info = np.array([[10, 40, 0, 0], [1, 7, 1, 0], [0, 0, 0, 0]])
    np.testing.assert_array_equal(flopmodel.solve_ops(c2, info), [10 * lin + 40 * ipm, lin + 7 * ipm, 0])
    assert flopmodel.ipm_iteration_ops(c1) < ipm < flopmodel.ipm_iteration_ops(c4)
    # C2 (N 20, nu 2, nx 5): 5-12 MFLOP per solve at 10 SQP and ~40 IPM iterations
    assert 5e6 < 10 * lin + 40 * ipm < 12e6
