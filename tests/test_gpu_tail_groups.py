"""Grouped level tickets and the fence pair of the hand-over (csrc/mpcg_tail.h, the ticket loop
of mpcg_sqp.h, the group's end in mpcg_sqp_body.inc).

A level ticket stands for a group of SQP-RTI iterations: iteration 0, then G iterations per ticket, G a
compile-time constant.  The builds with G = 1, 2 and 3 (_build.TAIL_AB tail_g1 .. tail_g3, made by
__graft_entry__.build()) each run, in a child process with MPCG_LIB set, the two batches of
tests/test_gpu_tail_levels.py -- the N 10 shape, 140 scenes x 8, and C2, 148 seeded scenes plus bench scenes 14
and 15, 1,200 solves: more than the 1,024 resident workgroups -- on HPIPM's profile with K forced to the batch,
the batch - 37 and 0, at sqp_iters 10, 3 and 4.  Every one of the five outputs must be the build's without level
tickets (tail_off) bit for bit, and within 1e-8 of the C oracle (the tolerance of tests/test_gpu_tail_levels.py
for these shapes).

The three horizons make solves end in every place a group can end (asserted from tail_off's sqp_iter alone,
for G = 2 and 3, over the last batch - 37 solves, the tail region of every forced K > 0):
  on the last iteration of a full group    G 2: 3 of 3 iterations (group {1, 2}); G 3: 4 of 4, 10 of 10
  in a short last group                    G 2: 4 of 4, 10 of 10 (groups {3}, {9}); G 3: 3 of 3 (group {1, 2})
  in the middle of a group                 2 iterations of 3, 4 or 10: a QP that did not succeed at iteration 1
and first-QP failures (1 iteration) besides.  The K = batch - 37 launches mix whole solves and groups: the
uneven load under which a hand-over without its release or its acquire shows as a changed bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
KEYS = ("xtraj", "utraj", "pobj", "exit", "info")
GROUPS = (1, 2, 3)
ITERS = (10, 3, 4)
CUT = 37
KNAMES = ("all", "all-37", "none")


def _inputs():
    """name -> (layout, params, warm, xinit): the batches of tests/test_gpu_tail_levels.py, built the same way"""
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import make_batch

    t10, c2 = config_layout("T10"), config_layout("C2")
    a = make_batch(t10, 140, 8, seed=7)
    b, piv = make_batch(c2, 148, 8, seed=7), make_batch(c2, 2, 8, first_scene=14)
    cat = lambda f: np.concatenate([getattr(b, f), getattr(piv, f)])  # noqa: E731
    cases = {"T10": (t10, a.params, a.warm, a.xinit), "C2": (c2, cat("params"), cat("warm"), cat("xinit"))}
    assert [len(c[3]) for c in cases.values()] == [1120, 1200]
    return cases


def _ks(B):
    return {"all": B, "all-37": B - CUT, "none": 0}


def _child(path, forced):
    """the library of this process: "case/iters/K name/key" -> array (forced: K forced on the stream; else the
    library's own launch, K name "lib")"""
    import torch

    from oscar_mpc_planner_mr_modification_amd import native
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    s = torch.cuda.current_stream()
    res = {}
    for name, (lay, P, W, X) in _inputs().items():
        P, W, X = t(P), t(W), t(X)
        for it in ITERS:
            pr = native.problem_from_layout(lay, qp_profile="hpipm", sqp_iters=it)
            for kn, k in (_ks(len(X)) if forced else {"lib": -1}).items():
                if forced:
                    assert native.lib.mpcg_debug_set_tail_levels(C.c_void_p(s.cuda_stream), k) == 0
                out = native.solve_batch_device(pr, P, W, X)
                torch.cuda.synchronize()
                for key in KEYS:
                    res[f"{name}/{it}/{kn}/{key}"] = out[key].cpu().numpy()
    np.savez(path, **res)


def _run_child(tmp, name, forced):
    from oscar_mpc_planner_mr_modification_amd import _build

    lib = _build.build_tail_ab(name)  # built on demand (__graft_entry__.build() makes it too)
    out = str(tmp / f"{name}.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, "forced" if forced else "lib"],
                       cwd=ROOT, env=dict(os.environ, MPCG_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, f"child {name} failed ({p.returncode})\n{p.stdout[-2000:]}"
    return dict(np.load(out))


@pytest.fixture(scope="module")
def cases():
    return _inputs()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tail_groups")


@pytest.fixture(scope="module")
def tail_off(tmp):
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    return _run_child(tmp, "tail_off", False)


@pytest.fixture(scope="module")
def grouped(tmp):
    return {g: _run_child(tmp, f"tail_g{g}", True) for g in GROUPS}


@pytest.fixture(scope="module")
def oracle_refs(cases, oracle_mod):
    return {(name, it): oracle_mod.Oracle(lay, qp_profile="hpipm", sqp_iters=it).solve_batch(P, W, X)
            for name, (lay, P, W, X) in cases.items() for it in ITERS}


def endings(sqp_iter, iters, G):
    """per solve, where its last SQP-RTI iteration stands in the groups of G: "first" (iteration 0), "full" (the
    last iteration of a full group), "short" (the solve's last iteration, in a last group of fewer than G) or
    "middle" (an earlier iteration of a group that the solve did not finish)"""
    last = np.asarray(sqp_iter) - 1
    out = np.full(last.shape, "middle", dtype=object)
    out[(last > 0) & (last % G != 0) & (last == iters - 1)] = "short"
    out[(last > 0) & (last % G == 0)] = "full"
    out[last <= 0] = "first"
    return out


def tail_endings(info_of, G):
    """the endings met in the tail region (the last batch - 37 solves) of the C2 batch over the three horizons"""
    met = set()
    for it in ITERS:
        n = info_of(it)
        assert n.min() >= 1 and n.max() == it
        met |= set(endings(n[CUT:], it, G))
    return met


@pytest.mark.parametrize("G", [2, 3])
def test_solves_end_at_group_ends_in_short_groups_and_mid_group(tail_off, G):
    met = tail_endings(lambda it: tail_off[f"C2/{it}/lib/info"][:, 0], G)
    assert {"first", "full", "short", "middle"} <= met, met


@pytest.mark.parametrize("kn", KNAMES)
@pytest.mark.parametrize("it", ITERS)
@pytest.mark.parametrize("name", ["T10", "C2"])
@pytest.mark.parametrize("G", GROUPS)
def test_every_output_is_the_build_without_level_tickets_bit_for_bit(grouped, tail_off, G, name, it, kn):
    got = {k: grouped[G][f"{name}/{it}/{kn}/{k}"] for k in KEYS}
    ref = {k: tail_off[f"{name}/{it}/lib/{k}"] for k in KEYS}
    differ = [k for k in KEYS if got[k].dtype != ref[k].dtype or got[k].tobytes() != ref[k].tobytes()]
    assert not differ, f"outputs that differ from the build without level tickets: {differ}"


@pytest.mark.parametrize("kn", KNAMES)
@pytest.mark.parametrize("it", ITERS)
@pytest.mark.parametrize("name", ["T10", "C2"])
@pytest.mark.parametrize("G", GROUPS)
def test_within_1e_8_of_the_oracle(grouped, oracle_refs, G, name, it, kn):
    got, ref = {k: grouped[G][f"{name}/{it}/{kn}/{k}"] for k in KEYS}, oracle_refs[(name, it)]
    same_exit = got["exit"] == ref["status"]
    ok = (got["exit"] == 1) & (ref["status"] == 1)
    dx = np.abs(got["xtraj"] - ref["xtraj"]).reshape(len(ok), -1).max(1)
    du = np.abs(got["utraj"] - ref["utraj"]).reshape(len(ok), -1).max(1)
    dp = np.abs(got["pobj"] - ref["pobj"])
    print(f"G {G} {name} sqp_iters {it} K {kn}: {len(ok)} solves, compared {int(ok.sum())}, exit agreement "
          f"{same_exit.mean():.4f}, max|dx| {dx[ok].max():.2e}, max|du| {du[ok].max():.2e}, max|dpobj| {dp[ok].max():.2e}")
    assert same_exit.all(), f"exit codes differ at {np.flatnonzero(~same_exit)[:10]}"
    assert (got["info"][:, 0] == ref["sqp_iter"]).all()
    # (the comparison is over the solves that exit with 1, as in tests/test_gpu_tail_levels.py: most of them at the
    # full horizon; after 3 or 4 iterations fewer have got there -- 454 of the 1,200 C2 solves after 3)
    assert ok.sum() >= (len(ok) // 2 if it == 10 else len(ok) // 4)
    assert dx[ok].max() <= TOL and du[ok].max() <= TOL and dp[ok].max() <= TOL


if __name__ == "__main__":
    assert len(sys.argv) == 4 and sys.argv[1] == "--child"
    sys.path.insert(0, ROOT)
    _child(sys.argv[2], sys.argv[3] == "forced")
