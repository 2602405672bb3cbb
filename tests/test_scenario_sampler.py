"""The host restatement of the SH-MPC scenario sampler (scenario_sampler.py, include/mpcg_scenario.h): known
answers of the sample construction and of the batch index, equality with scenario.prepare_scenario_host where
the radii are equal, and the step bookkeeping against plans written out by hand.  No GPU."""
import numpy as np

from oscar_mpc_planner_mr_modification_amd import scenario as sn
from oscar_mpc_planner_mr_modification_amd import scenario_sampler as ss
from oscar_mpc_planner_mr_modification_amd.layouts import safe_horizon_layout

AXIS_BANK = np.array([[[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]])   # one batch: the axis ends
# the big seed is above 2^63: a signed 64-bit restatement would get other values
BIG_SEED, SMALL_SEED = 0x8000000000000005 + 0x1234567800000000, 20251212
# mix(seed, draw, e) mod 16 for e = 0 .. 5 and mix(seed, draw, 0), from the header's C function compiled for the host
MIX_KNOWN = {
    (BIG_SEED, 0): ([10, 1, 5, 8, 2, 3], 5749190112111584474),
    (BIG_SEED, 3): ([5, 12, 9, 10, 1, 8], 14265135534550026277),
    (SMALL_SEED, 0): ([2, 13, 5, 8, 6, 11], 208445985741065986),
    (SMALL_SEED, 3): ([14, 11, 2, 8, 3, 4], 9350243980479520398),
}


def _one_obstacle(N, angle, major, minor, mean=(3.0, -2.0), vel=(0.5, 0.25)):
    obst = np.zeros((1, 1, N, 5))
    for k in range(N):
        obst[0, 0, k] = (mean[0] + vel[0] * k, mean[1] + vel[1] * k, angle, major * (k + 1), minor * (k + 1))
    return obst, np.array([[[0.4, 0.0]]])


def test_axis_bank_puts_the_samples_on_the_ellipse_axis_ends():
    N, ang = 5, 0.7
    obst, meta = _one_obstacle(N, ang, 0.5, 0.2)
    q = ss.draw_samples(obst, meta, AXIS_BANK, np.zeros((2, 1), np.int32), 2, N)
    assert q.shape == (2, N, 4, 2)
    c, s = np.cos(ang), np.sin(ang)
    for k in range(1, N):
        mx, my, _, a, b = obst[0, 0, k - 1]
        want = np.array([(mx + a * c, my + a * s), (mx - a * c, my - a * s), (mx - b * s, my + b * c),
                         (mx + b * s, my - b * c)])
        np.testing.assert_allclose(q[0, k], want, rtol=0, atol=1e-15)
        assert np.array_equal(q[0, k], q[1, k])
    assert np.array_equal(q[:, 0], q[:, 1])     # stage 0 holds the stage-1 values


def test_angle_zero_takes_the_exact_branch():
    N = 4
    obst, meta = _one_obstacle(N, 0.0, 0.3, 0.1)
    z = np.random.default_rng(3).normal(size=(2, 5, 2))
    bidx = np.array([[1]], np.int32)
    q = ss.draw_samples(obst, meta, z, bidx, 1, N)
    for k in range(1, N):
        mx, my, _, a, b = obst[0, 0, k - 1]
        assert np.array_equal(q[0, k, :, 0], mx + a * z[1, :, 0]) and np.array_equal(q[0, k, :, 1], my + b * z[1, :, 1])
    # -0.0 == 0.0 takes it too; a tiny angle does not
    obst[..., 2] = -0.0
    assert np.array_equal(ss.draw_samples(obst, meta, z, bidx, 1, N), q)
    obst[..., 2] = 1e-3
    assert not np.array_equal(ss.draw_samples(obst, meta, z, bidx, 1, N), q)


def test_deterministic_obstacle_gives_coincident_samples():
    N = 4
    obst, meta = _one_obstacle(N, 0.3, 0.0, 0.0)
    q = ss.draw_samples(obst, meta, np.random.default_rng(0).normal(size=(1, 6, 2)), np.zeros((1, 1), np.int32), 1, N)
    for k in range(1, N):
        assert np.array_equal(q[0, k], np.repeat(obst[0, 0, k - 1, None, 0:2], 6, 0))


def test_sample_order_is_obstacle_major():
    N = 3
    obst = np.zeros((1, 2, N, 5))
    obst[0, 0, :, 0], obst[0, 1, :, 0] = 10.0, 20.0
    obst[..., 3:5] = 1.0
    bank = np.arange(12.0).reshape(2, 3, 2)
    q = ss.draw_samples(obst, np.zeros((1, 2, 2)), bank, np.array([[1, 0]], np.int32), 1, N)
    assert np.array_equal(q[0, 1, :, 0], [16.0, 18.0, 20.0, 20.0, 22.0, 24.0])


def test_batch_index_known_answers():
    for (seed, draw), (mod16, raw0) in MIX_KNOWN.items():
        assert ss.mix(seed, draw, 0) == raw0
        got = ss.batch_index(seed, draw, 2, 3, 16)
        assert got.dtype == np.int32 and got.shape == (2, 3)
        assert got.reshape(-1).tolist() == mod16, (seed, draw)
    assert ss.batch_index(SMALL_SEED, 0, 2, 3, 1).tolist() == [[0, 0, 0], [0, 0, 0]]
    # the seed is taken modulo 2^64
    assert np.array_equal(ss.batch_index(BIG_SEED + (1 << 64), 3, 2, 3, 16), ss.batch_index(BIG_SEED, 3, 2, 3, 16))


def test_equal_radii_match_prepare_scenario_host_bit_for_bit():
    lay = safe_horizon_layout(N=10, n_constraints=4)
    for warm in (True, False):
        sc = ss.make_shmpc_prediction_scenes(lay, 3, 2, n_obs=3, n_samples=7, seed=9, previous_plan_warm=warm)
        samples = ss.draw_samples(sc.obst, sc.obst_meta, sc.bank, sc.batch_index(2), sc.n_solvers, lay.N)
        got = ss.prepare_scenario_sampled_host(lay, sc.stage_params, sc.state, samples, sc.obst_meta, sc.n_solvers,
                                               main_warm=sc.main_warm, robot_radius=0.325)
        assert np.all(sc.obst_meta[..., 0] == sc.obst_meta[0, 0, 0])
        old = sn.ScenarioScenes(stage_params=sc.stage_params, state=sc.state, samples=samples, n_solvers=sc.n_solvers,
                                main_warm=sc.main_warm)
        want = sn.prepare_scenario_host(lay, old, radius=0.325 + sc.obst_meta[0, 0, 0])
        for k in ("params", "warm", "xinit"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), k
        # radii that differ move each row's b by its own obstacle's difference (0.25 (j + 1) for obstacle j) and
        # leave the normals alone
        meta = sc.obst_meta.copy()
        meta[:, :, 0] += 0.25 * (1 + np.arange(3))
        other = ss.prepare_scenario_sampled_host(lay, sc.stage_params, sc.state, samples, meta, sc.n_solvers,
                                                 main_warm=sc.main_warm, robot_radius=0.325)
        i0 = lay.idx("disc_0_scenario_constraint_0_a1")
        rows = lambda b: b.params[:, 1:, i0:i0 + 12].reshape(-1, 3)  # noqa: E731
        assert np.array_equal(rows(other)[:, 0:2], rows(got)[:, 0:2])
        dist = np.linalg.norm(samples[:, 1:] - got.warm[:, 1:lay.N, None, 2:4], axis=3)
        owner = np.argsort(dist, axis=2, kind="stable")[:, :, :4] // 7          # the obstacle of every picked sample
        assert len(set(owner.reshape(-1))) >= 2
        np.testing.assert_allclose(rows(got)[:, 2] - rows(other)[:, 2], 0.25 * (1 + owner.reshape(-1)), rtol=0,
                                   atol=1e-12)


def test_prediction_scenes_share_the_draws_of_make_shmpc_scenes():
    lay = safe_horizon_layout(N=10, n_constraints=4)
    sc = ss.make_shmpc_prediction_scenes(lay, 2, n_obs=3, n_samples=7, seed=77)
    old = sn.make_shmpc_scenes(lay, 2, n_obs=3, n_samples=7, seed=77)
    for k in ("stage_params", "state", "main_warm"):
        assert np.array_equal(getattr(sc, k), getattr(old, k)), k
    # GAUSSIAN constant-velocity predictions: angle 0, sigma 0.3 dt sqrt(k + 1) at prediction step k, the
    # mean of stage k + 1 of make_shmpc_scenes' samples
    k = np.arange(lay.N)
    np.testing.assert_allclose(sc.obst[..., 3], np.broadcast_to(0.3 * lay.dt * np.sqrt(k + 1), sc.obst.shape[:3]),
                               rtol=1e-14)
    assert np.array_equal(sc.obst[..., 3], sc.obst[..., 4]) and not sc.obst[..., 2].any()
    assert sc.bank.shape == (ss.BANK_BATCHES, 7, 2) and sc.obst_meta[0, 0, 0] > 0


def test_advance_host_shift_and_braking_written_out():
    lay = safe_horizon_layout(N=4, n_constraints=4)
    N, nx, nu, P = 4, lay.nx, lay.nu, 2
    assert (nx, nu) == (6, 2)
    x = np.arange(2 * P * (N + 1) * nx, dtype=float).reshape(2 * P, N + 1, nx) + 1000.0
    u = -np.arange(2 * P * N * nu, dtype=float).reshape(2 * P, N, nu) - 1.0
    lam = np.arange(2 * P * N * (nx + lay.nh), dtype=float).reshape(2 * P, N, nx + lay.nh) + 1.0
    exit_code = np.array([1, 1, 4, 1], np.int32)
    best = np.array([1, -1], np.int32)
    state_next = np.array([[1.0, 2.0, 0.5, 1.5, 0.25, 0.125], [0.0, 1.0, 0.0, 0.5, 2.0, 9.0]])
    mw, ln = ss.advance_host(lay, best, exit_code, x, u, lam, state_next, P, deceleration=3.0)
    # scene 0, feasible, winner = solve 1: [state, out_2, out_3, out_3, out_3]; stage 0's inputs out_1's
    w = 1
    want = np.array([np.r_[u[w, 1], state_next[0]], np.r_[u[w, 2], x[w, 2]], np.r_[u[w, 3], x[w, 3]],
                     np.r_[u[w, 3], x[w, 3]], np.r_[u[w, 3], x[w, 3]]])
    assert np.array_equal(mw[0], want)
    assert mw[0, 0, 7] == 0.125          # the slack of stage 0 is the state's
    # scene 1, infeasible: braking from v 0.5 with a = -3 and dt 0.2 along psi = 0; the slack and the rest 0
    dt = lay.dt
    assert dt == 0.2
    rows = [(-3.0, 0.0, 0.0, 1.0, 0.0, 0.5, 2.0, 0.0),
            (-3.0, 0.0, 0.0 + 0.5 * dt, 1.0, 0.0, 0.0, 2.0 + 0.5 * dt, 0.0)]
    rows += [rows[1]] * 3
    assert np.array_equal(mw[1], np.array(rows))
    # multipliers: kept where the exit code is 1
    assert np.array_equal(ln[[0, 1, 3]], lam[[0, 1, 3]]) and not ln[2].any()
    assert ss.advance_host(lay, best, exit_code, x, u, None, state_next, P)[1] is None
