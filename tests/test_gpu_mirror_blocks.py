"""The block form of the MIRROR regularisation (MPCG_MIRROR_BLOCKS): with a zero
disc offset the unicycle's 7 x 7 stage Hessian is exactly block-diagonal, {a, w, psi, v} and
{x, y, s}, and the linearisation mirrors the two blocks separately -- the full-size sweep without
the operations on exact zeros -- wherever every stage lane of the wave holds such a block.

tests/cpp/mirror_probe.hip (built by _build.build_mirror_probe into build/probe/) runs the block
form, the general form mirror<7> and the decision on given matrices, one per lane, one wavefront per
workgroup: all 49 outputs of the two forms are compared bit for bit, and the decision is checked on
blocks the block form does not reproduce (a cross-block coupling, a non-finite entry).

The solver-level tests run the N 10 shape with offsets 0 and 0.2 alternating inside one work-queue
launch (1,200 solves on 1,024 resident workgroups: second tickets) against launches of one kind and
the oracle, and a C1 batch against the oracle, at the tolerances of tests/test_gpu_res_carry.py."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IA, IB = [0, 1, 4, 5], [2, 3, 6]     # z = [a w x y psi v s]
EPS = 1e-4                           # reg_eps
X_TOL = 1e-4      # the N 10 shape (tests/test_gpu_res_carry.py test_n10_second_instantiation)
TIGHT = 1e-8      # C1 (tests/test_gpu_res_carry.py test_c1_every_carry_path)


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    from oscar_mpc_planner_mr_modification_amd import _build, native
    lib = C.CDLL(_build.build_mirror_probe())     # built on demand (__graft_entry__.build() makes it too)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    lib.probe_mirror.argtypes = [C.c_int, C.c_double, dp, dp, dp, dp, dp, dp]
    assert lib.probe_abi_version() == native.lib.mpcg_abi_version()

    def run(A):
        A = np.ascontiguousarray(A, np.float64)
        n = len(A)
        Hb, Hg, Hs = np.zeros_like(A), np.zeros_like(A), np.zeros_like(A)
        ok, took = np.zeros(n), np.zeros(n)
        assert lib.probe_mirror(n, EPS, A, Hb, Hg, Hs, ok, took) == 0
        return dict(Hb=Hb, Hg=Hg, Hs=Hs, ok=ok.astype(bool), took=took.astype(bool))
    return run


def _embed(a4, b3):
    """7 x 7 matrices with the 4 x 4 blocks a4 on IA, the 3 x 3 blocks b3 on IB and zero couplings"""
    A = np.zeros((len(a4), 7, 7))
    A[np.ix_(range(len(a4)), IA, IA)] = a4
    A[np.ix_(range(len(a4)), IB, IB)] = b3
    return A


def _sym(rng, n, m, scale=1.0):
    M = rng.standard_normal((n, m, m)) * scale
    return 0.5 * (M + M.transpose(0, 2, 1))


def _spectrum(rng, n, m, lam):
    """Q diag(lam) Q' with a random orthogonal Q (symmetrised); lam [n][m]"""
    Q = np.linalg.qr(rng.standard_normal((n, m, m)))[0]
    M = Q @ (lam[:, :, None] * Q.transpose(0, 2, 1))
    return 0.5 * (M + M.transpose(0, 2, 1))


def _cases():
    """name -> [n][7][7] block-diagonal matrices; 64 per case (one wavefront each), 448 in all"""
    rng = np.random.default_rng(20251212)
    n = 64
    c = {}
    c["indefinite"] = _embed(_sym(rng, n, 4), _sym(rng, n, 3))
    c["inside_eps"] = _embed(_spectrum(rng, n, 4, rng.uniform(-EPS, EPS, (n, 4))),
                             _spectrum(rng, n, 3, rng.uniform(-EPS, EPS, (n, 3))))
    c["diagonal"] = _embed(rng.standard_normal((n, 4))[:, :, None] * np.eye(4),
                           rng.standard_normal((n, 3))[:, :, None] * np.eye(3))
    c["zero"] = np.zeros((n, 7, 7))
    tiny = _embed(rng.standard_normal((n, 4))[:, :, None] * np.eye(4), rng.standard_normal((n, 3))[:, :, None] * np.eye(3))
    # one in-block coupling under the rotation's skip (|a_pq| < 1e-300), next to an ordinary one in the other block
    tiny[:, 0, 4] = tiny[:, 4, 0] = 1e-301
    tiny[:, 2, 6] = tiny[:, 6, 2] = rng.standard_normal(n)
    tiny[n // 2:, 3, 6] = tiny[n // 2:, 6, 3] = -1e-301
    c["skip_1e-301"] = tiny
    c["near_equal"] = _embed(_spectrum(rng, n, 4, 1.0 + 1e-13 * rng.standard_normal((n, 4))),
                             _spectrum(rng, n, 3, -2.0 + 1e-12 * rng.standard_normal((n, 3))))
    s4 = 10.0 ** rng.uniform(-4, 4, (n, 4))       # entries s_i s_j m_ij: 1e-8 .. 1e8
    s3 = 10.0 ** rng.uniform(-4, 4, (n, 3))
    c["1e-8..1e8"] = _embed(_sym(rng, n, 4) * s4[:, :, None] * s4[:, None, :],
                            _sym(rng, n, 3) * s3[:, :, None] * s3[:, None, :])
    return c


@pytest.fixture(scope="module")
def probe_cases(probe):
    cases = _cases()
    A = np.concatenate(list(cases.values()))
    A.setflags(write=False)
    return cases, A, probe(A)


def _same_bits(x, y):
    return x.tobytes() == y.tobytes()


def test_block_form_is_the_general_form_bit_for_bit(probe_cases):
    cases, A, r = probe_cases
    assert len(A) == 448
    assert r["ok"].all() and r["took"].all()          # every lane's block qualifies, every wave took the block form
    lo = 0
    for name, a in cases.items():
        hb, hg, hs = (r[k][lo:lo + len(a)] for k in ("Hb", "Hg", "Hs"))
        lo += len(a)
        diff = (hb.view(np.uint64) != hg.view(np.uint64)).reshape(len(a), -1)
        print(f"{name}: {len(a)} matrices, {int(diff.any(1).sum())} differ, max |block - general| "
              f"{np.abs(hb - hg).max():.2e}, max |H| {np.abs(hg).max():.2e}")
        assert not diff.any(), f"{name}: matrices {np.flatnonzero(diff.any(1))[:8]} differ"
        assert _same_bits(hs, hg), name
        assert np.isfinite(hg).all(), name
    # the cross entries are +0.0, not -0.0
    cross = r["Hb"][:, IA][:, :, IB]
    assert not cross.any() and not np.signbit(cross).any()
    # and the result is the MIRROR: eigenvalues |d|, at least eps
    w = np.linalg.eigvalsh(A[:64])
    np.testing.assert_allclose(np.linalg.eigvalsh(r["Hb"][:64]), np.sort(np.maximum(np.abs(w), EPS), axis=1),
                               rtol=1e-12, atol=1e-14)
    assert np.array_equal(r["Hb"][192:256], np.broadcast_to(EPS * np.eye(7), (64, 7, 7)))   # all zero -> eps I


@pytest.mark.parametrize("what", ["cross", "nan", "inf"])
def test_decision_takes_the_general_form(probe, probe_cases, what):
    """one lane of the second of three waves holds a block the block form does not reproduce: that wave
    runs the general form on all its matrices, the other two waves the block form"""
    cases, _, _ = probe_cases
    A = np.concatenate([cases["indefinite"], cases["1e-8..1e8"], cases["near_equal"]]).copy()
    bad = 64 + 17
    if what == "cross":
        A[bad, 5, 3] = 1e-7            # lower triangle only: v - y
    elif what == "nan":
        A[bad, 2, 3] = A[bad, 3, 2] = np.nan
    else:
        A[bad, 4, 4] = np.inf
    r = probe(A)
    want_ok = np.ones(192, bool)
    want_ok[bad] = False
    assert np.array_equal(r["ok"], want_ok)
    assert np.array_equal(r["took"], np.repeat([True, False, True], 64))
    assert _same_bits(r["Hs"], r["Hg"])                 # what ran is the general form's result everywhere
    good = np.delete(np.arange(192), bad)
    assert _same_bits(r["Hb"][good], r["Hg"][good])
    if what == "cross":                                  # and the coupling is in the result
        assert r["Hs"][bad, 5, 3] != 0.0 and np.isfinite(r["Hs"][bad]).all()


# ---------------------------------------------------------------------------------------------------------
# solver level
# ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    return torch.device("cuda:0")


def _gpu(torch_dev, lay, params, warm, xinit):
    import torch

    from oscar_mpc_planner_mr_modification_amd import native
    pr = native.problem_from_layout(lay)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_dev)  # noqa: E731
    out = native.solve_batch_device(pr, t(params), t(warm), t(xinit))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(ref, got, label, tol):
    """tests/test_gpu_res_carry.py _compare"""
    same_exit = got["exit"] == ref["status"]
    ok = (got["exit"] == 1) & (ref["status"] == 1)
    dx = np.abs(got["xtraj"] - ref["xtraj"]).reshape(len(ok), -1).max(1)
    du = np.abs(got["utraj"] - ref["utraj"]).reshape(len(ok), -1).max(1)
    rel = np.abs(got["pobj"] - ref["pobj"]) / np.maximum(1.0, np.abs(ref["pobj"]))
    print(f"{label}: {len(ok)} solves, compared {int(ok.sum())}, exit agreement {same_exit.mean():.4f}, "
          f"max|dx| {dx[ok].max() if ok.any() else 0:.2e}, max|du| {du[ok].max() if ok.any() else 0:.2e}, "
          f"pobj rel {rel[ok].max() if ok.any() else 0:.2e}")
    assert same_exit.all(), f"exit codes differ at {np.where(~same_exit)[0][:10]}: gpu {got['exit'][~same_exit][:10]} " \
                            f"oracle {ref['status'][~same_exit][:10]}"
    assert ok.any()
    assert dx[ok].max() <= tol, f"max |x - x_ref| = {dx[ok].max():.3e}"
    assert du[ok].max() <= tol, f"max |u - u_ref| = {du[ok].max():.3e}"
    assert rel[ok].max() <= 1e-6, rel[ok].max()


def test_n10_offsets_alternate_within_one_launch(torch_dev, oracle_mod):
    """1,200 solves of the N 10 shape, the odd ones with disc offset 0.2 and rotated ellipsoids
    (geometry_cases.perturb_geometry): the general form; the even ones the block form.  A wave takes one
    kind after the other from the queue.  Every solve is bit for bit the same solve in a launch of its own
    kind, and agrees with the oracle."""
    from geometry_cases import PERTURB_SEED, perturb_geometry
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import make_batch

    lay = config_layout("T10")
    b = make_batch(lay, 150, 8, seed=7)
    B = len(b.xinit)
    assert B == 1200 > 1024
    assert not b.params[:, :, lay.idx("ego_disc_0_offset")].any()
    params = np.array(b.params, copy=True)
    odd = np.arange(B) % 2 == 1
    params[odd] = perturb_geometry(lay, b.params[odd], PERTURB_SEED, 0.2)
    assert (params[odd][:, :, lay.idx("ego_disc_0_offset")] == 0.2).all()
    mixed = _gpu(torch_dev, lay, params, b.warm, b.xinit)
    assert (mixed["exit"] >= 0).all()
    for kind, sel in (("offset 0", ~odd), ("offset 0.2", odd)):
        own = _gpu(torch_dev, lay, params[sel], b.warm[sel], b.xinit[sel])
        for key in ("xtraj", "utraj", "pobj", "exit", "info"):
            assert _same_bits(np.ascontiguousarray(mixed[key][sel]), own[key]), (kind, key)
    ref = oracle_mod.Oracle(lay).solve_batch(params, b.warm, b.xinit)
    assert ((ref["status"] == 1) & odd).sum() > 100 and ((ref["status"] == 1) & ~odd).sum() > 100
    _compare(ref, mixed, "T10 150x8, offsets 0 / 0.2 alternating", X_TOL)


def test_c1_offset_zero_against_the_oracle(torch_dev, oracle_mod):
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.synthetic import make_batch

    lay = config_layout("C1")
    b = make_batch(lay, 8, 8, seed=99)
    assert len(b.xinit) == 64 and not b.params[:, :, lay.idx("ego_disc_0_offset")].any()
    ref = oracle_mod.Oracle(lay).solve_batch(b.params, b.warm, b.xinit)
    got = _gpu(torch_dev, lay, b.params, b.warm, b.xinit)
    _compare(ref, got, "C1 8x8", TIGHT)
