"""The Riccati step that reads only the varying rows of [B A] again and selects its first pivot's zero
(Cfg::FAC_INVARIANT_ROWS, Cfg::FAC_PIVOT_SELECT).

Both changes keep every bit: the rows psi+, v+, s+ kept in registers are the values the loop read again
before (tests/test_fac_invariant_rows.py, tests/test_gpu_fac_rows_probe.py), and the reciprocal square
root computed for a non-positive first pivot is never read.  So every output of the production library
is compared bit for bit with the outputs of two switch-off builds of the same tree
(_build.build_fac_ab, build/ab/): `fac_rows0` (-DMPCG_FAC_INVARIANT_ROWS=0: every row read again) and
`fac_off` (that and -DMPCG_FAC_PIVOT_SELECT=0: the parent commit's loop, instruction for instruction).
Each switch-off build runs in a child process of its own with MPCG_LIB set, as scripts/bitcmp.py runs
them: a process holds one libmpcg.so.  Every case is also held to the C oracle at 1e-8, the tolerance of
tests/test_gpu_res_carry.py for C1 and C2.

Cases: the N 10 shape with 192 solves, 64 solves of C1 and of C2 from the seeded generator, and scenes
14 and 15 of the C2 bench batch, whose solves 4 and 10 diverge in their first QP until the Riccati pivots
turn non-positive (tests/test_oracle_modes.py test_blasfeo_pivot_rule_on_diverging_qps; in the kernel's
arithmetic forms the first pivot m00 of the 2 x 2 block is non-positive at stages 7 to 9 of those QPs and
the second at others).  Each on HPIPM's profile and the robust one, through the lean
variant and the FULL one (a statistics buffer asks for it).  (A work-queue launch takes min(resident
workgroups, solves) workgroups, so the 192 solves of the N 10 shape are one ticket each; launches with
second tickets are tests/test_queue.py's and tests/test_gpu_res_carry.py's.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
KEYS = ("xtraj", "utraj", "pobj", "exit", "info")
PROFILES = ("hpipm", "robust")
VARIANTS = ("lean", "full")
DIVERGING = (4, 10)            # of the 16 solves of scenes 14, 15 of the C2 bench batch


def _inputs():
    """name -> (layout, batch); seeded, the same in the test and in its children"""
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import make_batch

    t10, c1, c2 = config_layout("T10"), config_layout("C1"), config_layout("C2")
    cases = {"T10": (t10, make_batch(t10, 24, 8, seed=7)),
             "C1": (c1, make_batch(c1, 8, 8, seed=99)),
             "C2": (c2, make_batch(c2, 8, 8)),
             "C2_pivot": (c2, make_batch(c2, 2, 8, first_scene=14))}
    assert [len(b.xinit) for _, b in cases.values()] == [192, 64, 64, 16]
    return cases


def _solve_all(cases):
    """every case x profile x variant through the libmpcg.so this process loaded: "case/profile/variant/key" -> array"""
    import torch

    from oscar_mpc_planner_mr_modification_amd import native
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = {}
    for name, (lay, b) in cases.items():
        P, W, X = t(b.params), t(b.warm), t(b.xinit)
        for prof in PROFILES:
            pr = native.problem_from_layout(lay, qp_profile=prof)
            for var in VARIANTS:
                o = native.solve_batch_device(pr, P, W, X, stats=(var == "full"))
                torch.cuda.synchronize()
                for k in KEYS:
                    out[f"{name}/{prof}/{var}/{k}"] = o[k].cpu().numpy()
    return out


def _child(path):
    np.savez(path, **_solve_all(_inputs()))


@pytest.fixture(scope="module")
def cases():
    return _inputs()


@pytest.fixture(scope="module")
def switch_off(tmp_path_factory):
    """outputs of the two switch-off builds, one child process each, both started before either is waited for"""
    from oscar_mpc_planner_mr_modification_amd import _build

    d = tmp_path_factory.mktemp("fac_rows")
    procs = {}
    for name in _build.FAC_AB:
        lib = _build.build_fac_ab(name)          # built on demand (__graft_entry__.build() makes them too)
        out = str(d / f"{name}.npz")
        procs[name] = (subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", out], cwd=ROOT,
                                        env=dict(os.environ, MPCG_LIB=lib), stdout=subprocess.PIPE,
                                        stderr=subprocess.STDOUT, text=True), out)
    res = {}
    for name, (p, out) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{name}: child failed ({p.returncode})\n{log[-2000:]}"
        res[name] = dict(np.load(out))
    return res


@pytest.fixture(scope="module")
def prod(cases):
    return _solve_all(cases)


@pytest.fixture(scope="module")
def oracle_refs(cases, oracle_mod):
    return {(name, prof): oracle_mod.Oracle(lay, qp_profile=prof).solve_batch(b.params, b.warm, b.xinit)
            for name, (lay, b) in cases.items() for prof in PROFILES}


@pytest.mark.parametrize("build", ["fac_rows0", "fac_off"])
def test_every_output_is_the_switch_off_builds_bit_for_bit(prod, switch_off, build):
    ref = switch_off[build]
    assert sorted(ref) == sorted(prod) and len(prod) == 4 * 2 * 2 * len(KEYS)
    differ = [k for k in sorted(prod) if prod[k].dtype != ref[k].dtype or prod[k].tobytes() != ref[k].tobytes()]
    assert not differ, f"outputs that differ from the {build} build: {differ}"


def test_full_variant_ends_every_solve_like_the_lean_one(prod):
    """tests/test_queue.py's statement, on these cases and both profiles"""
    for k in sorted(prod):
        name, prof, var, key = k.split("/")
        if var == "lean":
            assert np.array_equal(prod[k], prod[f"{name}/{prof}/full/{key}"], equal_nan=True), k


@pytest.mark.parametrize("prof", PROFILES)
@pytest.mark.parametrize("name", ["T10", "C1", "C2", "C2_pivot"])
def test_within_1e_8_of_the_oracle(prod, oracle_refs, name, prof):
    ref = oracle_refs[(name, prof)]
    for var in VARIANTS:
        got = {k: prod[f"{name}/{prof}/{var}/{k}"] for k in KEYS}
        same_exit = got["exit"] == ref["status"]
        ok = (got["exit"] == 1) & (ref["status"] == 1)
        dx = np.abs(got["xtraj"] - ref["xtraj"]).reshape(len(ok), -1).max(1)
        du = np.abs(got["utraj"] - ref["utraj"]).reshape(len(ok), -1).max(1)
        dp = np.abs(got["pobj"] - ref["pobj"])
        print(f"{name} {prof} {var}: {len(ok)} solves, compared {int(ok.sum())}, exit agreement {same_exit.mean():.3f}, "
              f"max|dx| {dx[ok].max():.2e}, max|du| {du[ok].max():.2e}, max|dpobj| {dp[ok].max():.2e} "
              f"(max |pobj| {np.abs(ref['pobj'][ok]).max():.3g}), IPM iterations equal on "
              f"{(got['info'][:, 1] == ref['qp_iter']).mean():.3f}")
        assert same_exit.all(), f"exit codes differ at {np.flatnonzero(~same_exit)[:10]}"
        assert ok.sum() >= len(ok) // 2
        assert dx[ok].max() <= TOL and du[ok].max() <= TOL and dp[ok].max() <= TOL


def test_non_positive_pivots_take_blasfeos_zero_path(cases, prod, oracle_refs):
    """solves 4 and 10 of the pivot case on HPIPM's profile.  With the pivot rule alone switched
    (qp_pivot_zero 0: a failed pivot ends the QP) their QP ends with status 1 (NaN), so a non-positive
    pivot does occur there; with BLASFEO's rule the recursion goes on with the zero inverse -- the selected
    zero -- for more iterations, and the QP ends on its step length (status 3, MINSTEP): a QP failure
    (exit 4) either way, as in the oracle.  The switch-off builds' bits for these solves are compared in
    test_every_output_is_the_switch_off_builds_bit_for_bit."""
    import torch

    from oscar_mpc_planner_mr_modification_amd import native
    div = np.array(DIVERGING)
    lay, b = cases["C2_pivot"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    o = native.solve_batch_device(native.problem_from_layout(lay, qp_pivot_zero=0), t(b.params), t(b.warm), t(b.xinit))
    torch.cuda.synchronize()
    stop = {k: o[k].cpu().numpy() for k in KEYS}
    assert (stop["info"][div, 2] == 1).all() and (stop["exit"][div] == 4).all(), (stop["info"][div], stop["exit"][div])
    for var in VARIANTS:
        h = {k: prod[f"C2_pivot/hpipm/{var}/{k}"] for k in KEYS}
        assert (h["info"][div, 2] == 3).all() and (h["exit"][div] == 4).all(), (var, h["info"][div], h["exit"][div])
        assert (h["info"][div, 1] > stop["info"][div, 1]).all(), (var, h["info"][div, 1], stop["info"][div, 1])
    ref = oracle_refs[("C2_pivot", "hpipm")]
    assert (ref["qp_status"][div] == 3).all() and (ref["status"][div] == 4).all()


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--child"
    sys.path.insert(0, ROOT)
    _child(sys.argv[2])
