"""erk_unicycle with sin / cos of psi given by the caller (Cfg::PSI_SHARED; mpcg_device.h).

sincos(psi) in the caller is the same function of the same argument as the one erk_unicycle forms, and every
operand and the order of every accumulation stay as they are, so xn, all of [B A] and the Hessian accumulated onto
a given block must be the plain form's bit for bit.  tests/cpp/erk_psi_probe.hip (built by
_build.build_erk_psi_probe into build/probe/) runs both forms at 64 (z, pi) on the lanes of one wavefront, for 1,
2, 3 and 4 substeps; the turn rates include +0, -0 and magnitudes up to 10 (the box bound is 1.5).

(The reuse of sincos(tau w) between substeps that DESIGN.md §3.14 records was held to the same statement by this
probe and did not meet it -- [B A] differed on 8 and more of the 64 lanes at one substep already -- so it is not in
the tree.)"""
import ctypes as C

import numpy as np
import pytest

from oscar_mpc_planner_mr_modification_amd.layouts import config_layout

pytestmark = pytest.mark.gpu

N_LANES, NX, NZ = 64, 5, 7


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    from oscar_mpc_planner_mr_modification_amd import _build, native
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgProblem
    lib = C.CDLL(_build.build_erk_psi_probe())     # built on demand (__graft_entry__.build() makes it too)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    lib.probe_erk_psi.argtypes = [C.POINTER(MpcgProblem), C.c_int, C.c_int, dp, dp, dp, dp, dp, dp]
    assert lib.probe_abi_version() == native.lib.mpcg_abi_version()
    return lib


def _points(seed):
    rng = np.random.default_rng(seed)
    n = N_LANES
    w = rng.uniform(-1.5, 1.5, n)
    w[0], w[1], w[2], w[3] = 0.0, -0.0, 10.0, -10.0
    w[4:12] = rng.uniform(-10.0, 10.0, 8)
    w[12], w[13] = 5e-324, -1e-300
    z = np.column_stack([rng.uniform(-3, 3, n), w, rng.uniform(-50, 50, n), rng.uniform(-50, 50, n),
                         rng.uniform(-2 * np.pi, 2 * np.pi, n), rng.uniform(-1, 4, n), rng.uniform(-5, 200, n)])
    H0 = rng.standard_normal((n, NZ, NZ))
    return np.ascontiguousarray(z), np.ascontiguousarray(rng.standard_normal((n, NX))), np.ascontiguousarray(H0)


@pytest.fixture(scope="module")
def results(probe):
    """(rk_steps, form) -> (xn, F, H), both forms at the same points"""
    from oscar_mpc_planner_mr_modification_amd.native_spec import problem_from_layout
    lay = config_layout("C2")
    z, pi, H0 = _points(20251221)
    assert np.signbit(z[1, 1]) and z[1, 1] == 0.0 and np.abs(z[:, 1]).max() == 10.0
    res = {}
    for ns in (1, 2, 3, 4):
        pr = problem_from_layout(lay, rk_steps=ns)
        for form in (0, 1):
            xn, F, H = np.zeros((N_LANES, NX)), np.zeros((N_LANES, NX, NZ)), np.zeros((N_LANES, NZ, NZ))
            assert probe.probe_erk_psi(C.byref(pr), form, N_LANES, z, pi, H0, xn, F, H) == 0
            res[(ns, form)] = (xn, F, H)
    return res, H0


@pytest.mark.parametrize("ns", [1, 2, 3, 4])
def test_given_psi_is_the_plain_form_bit_for_bit(results, ns):
    res, H0 = results
    ref, got = res[(ns, 0)], res[(ns, 1)]
    assert all(np.isfinite(a).all() for a in ref)
    for what, a, b in zip(("xn", "F", "H"), ref, got):
        lanes = [i for i in range(N_LANES) if a[i].tobytes() != b[i].tobytes()]
        assert not lanes, f"rk_steps {ns}: {what} differs on lanes {lanes[:8]}"
    # the probe did run the map and its adjoint Hessian: x+ depends on psi, and H moved on the (a, w, psi, v)
    # block only
    assert (ref[1][:, 0, 4] != 0.0).all()
    moved = ref[2] != H0
    zi = [0, 1, 4, 5]
    assert moved[:, 4, 4].all() and not np.delete(np.delete(moved, zi, axis=1), zi, axis=2).any()
