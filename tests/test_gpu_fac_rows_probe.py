"""The device side of the assumption behind Cfg::FAC_INVARIANT_ROWS (the oracle's side
is tests/test_fac_invariant_rows.py): erk_unicycle of mpcg_device.h, run at 64 random (z, pi) on the 64
lanes of one wavefront (tests/cpp/fac_rows_probe.hip, built by _build.build_fac_rows_probe into
build/probe/), writes bit-identical rows psi+, v+, s+ (and slack+ on the slack model) of [B A] on every
lane -- the values the Riccati loop keeps in registers over the stages -- while the x+ and y+ rows differ
from lane to lane."""
import ctypes as C

import numpy as np
import pytest

from oscar_mpc_planner_mr_modification_amd.layouts import config_layout

pytestmark = pytest.mark.gpu

N_LANES = 64


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available(), "gpu test on a box without a GPU"
    from oscar_mpc_planner_mr_modification_amd import _build, native
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgProblem
    lib = C.CDLL(_build.build_fac_rows_probe())     # built on demand (__graft_entry__.build() makes it too)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    lib.probe_erk_wave.argtypes = [C.POINTER(MpcgProblem), C.c_int, dp, dp, dp, dp]
    assert lib.probe_abi_version() == native.lib.mpcg_abi_version()
    return lib


def _points(nx, n, seed):
    """tests/test_fac_invariant_rows.py _points"""
    rng = np.random.default_rng(seed)
    z = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-50, 50, n),
                         rng.uniform(-50, 50, n), rng.uniform(-2 * np.pi, 2 * np.pi, n), rng.uniform(-1, 4, n),
                         rng.uniform(-5, 200, n)] + ([rng.uniform(0, 2, n)] if nx == 6 else []))
    return np.ascontiguousarray(z), np.ascontiguousarray(rng.standard_normal((n, nx)))


@pytest.mark.parametrize("cfg", ["C2", "C5"])     # nx 5 (C1, C2, T10, C4, JS, JD share dt and substeps) and the slack model
def test_constant_rows_are_bit_identical_across_the_lanes_of_a_wave(probe, cfg):
    from oscar_mpc_planner_mr_modification_amd.native_spec import problem_from_layout

    lay = config_layout(cfg)
    pr = problem_from_layout(lay)
    nx, nz = lay.nx, lay.nx + 2
    z, pi = _points(nx, N_LANES, 20251220)
    F, xn = np.zeros((N_LANES, nx, nz)), np.zeros((N_LANES, nx))
    assert probe.probe_erk_wave(C.byref(pr), N_LANES, z, pi, F, xn) == 0
    assert np.isfinite(F).all() and np.isfinite(xn).all()
    for m in range(2, nx):
        rows = np.ascontiguousarray(F[:, m, :])
        differ = [i for i in range(N_LANES) if rows[i].tobytes() != rows[0].tobytes()]
        assert not differ, f"{cfg}: row {m} of [B A] differs on lanes {differ[:8]}"
    # what the kernel's FCONST instances write for the rows they do not store (mpcg_sqp_body.inc FatB)
    dt = pr.dt
    want = np.zeros((nx, nz))
    want[2, 1], want[2, 4] = dt, 1.0
    want[3, 0], want[3, 5] = dt, 1.0
    want[4, 0], want[4, 5], want[4, 6] = 0.5 * dt * dt, dt, 1.0
    if nx == 6:
        want[5, 7] = 1.0
    assert F[0, 2:].tobytes() == want[2:].tobytes()
    for m in (0, 1):
        assert len({F[i, m].tobytes() for i in range(N_LANES)}) == N_LANES, f"row {m} (x+ / y+) should vary"
    # and the map is the stage map: psi+ = psi + dt w, v+ = v + dt a on every lane
    np.testing.assert_allclose(xn[:, 2], z[:, 4] + dt * z[:, 1], rtol=0, atol=1e-14)
    np.testing.assert_allclose(xn[:, 3], z[:, 5] + dt * z[:, 0], rtol=0, atol=1e-14)
