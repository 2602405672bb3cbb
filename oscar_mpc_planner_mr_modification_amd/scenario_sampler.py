"""The SH-MPC scenario sampler on the host: the restatement of include/mpcg_scenario.h.

In the reference every parallel solver draws its own obstacle samples from the uncertain predictions
at every control step (ScenarioConstraints::onDataReceived ->
GetSampler().IntegrateAndTranslateToMeanAndVariance, scenario_constraints.cpp:110-130) and the external
`scenario_module` reduces them to halfspaces.  `scenario_module` is not part of the reference, so the
sampler here restates its published scheme, PARITY UNPINNED like the reduction (scenario.py): a
pre-drawn bank of standard-normal pairs, scaled by each stage's covariance, rotated by the
prediction's angle and translated to its mean.  The definition (the batch index `mix`, the order of
the operations, the order of the samples, the row of a picked sample with the radius per obstacle,
deterministic obstacles) is stated once, in include/mpcg_scenario.h; this module follows it
operation by operation in numpy (which fuses no multiply-add), so that the kernels of
csrc/mpcg_scenario.h agree with it bit for bit wherever no cos / sin enters (angle == 0).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import obstacles as ob
from .layouts import Layout
from .native_spec import SCENARIO_MIX_C1, SCENARIO_MIX_C2, SCENARIO_MIX_M1, SCENARIO_MIX_M2
from .scenario import (DUMMY_B, PARALLEL_SOLVERS, SEED0, ScenarioBatch, braking_warm, shmpc_previous_plan,
                       shmpc_scene_world)
from .synthetic import DECELERATION, OBSTACLE_RADIUS, ROBOT_RADIUS

BANK_BATCHES = 16             # batches of the generated scenes' bank
_MASK = (1 << 64) - 1


def mix(seed: int, draw: int, index: int) -> int:
    """include/mpcg_scenario.h, mix: Python integers masked to 64 bits"""
    x = ((seed ^ ((draw * SCENARIO_MIX_C1) & _MASK)) + index * SCENARIO_MIX_C2) & _MASK
    x = ((x ^ (x >> 30)) * SCENARIO_MIX_M1) & _MASK
    x = ((x ^ (x >> 27)) * SCENARIO_MIX_M2) & _MASK
    return x ^ (x >> 31)


def batch_index(seed: int, draw: int, n_solves: int, n_obs: int, n_batches: int) -> np.ndarray:
    """(n_solves, n_obs) int32: the bank batch of copy sol for obstacle j, mix(seed, draw, sol n_obs + j) mod
    n_batches"""
    seed, draw = int(seed) & _MASK, int(draw) & _MASK
    out = [mix(seed, draw, e) % n_batches for e in range(n_solves * n_obs)]
    return np.array(out, np.int32).reshape(n_solves, n_obs)


def draw_samples(obst: np.ndarray, meta: np.ndarray, bank: np.ndarray, batch_idx: np.ndarray, P: int,
                 N: int) -> np.ndarray:
    """The sample tensor (S*P, N, M, 2) of mpcg_scenario_io from obst (S, n_obs, N, 5), the bank
    (n_batches, n_per, 2) and batch_idx (S*P, n_obs): sample m = j n_per + i of stage k >= 1 from prediction
    k - 1 of obstacle j and z = bank[batch_idx[sol, j], i]; stage 0 holds the stage-1 values.  `meta`
    (S, n_obs, 2) is not read (the radius enters the rows, not the samples)."""
    S, n_obs = obst.shape[0], obst.shape[1]
    n_per = bank.shape[1]
    assert obst.shape == (S, n_obs, N, 5) and batch_idx.shape == (S * P, n_obs) and bank.shape[2] == 2
    out = np.zeros((S * P, N, n_obs * n_per, 2))
    for sol in range(S * P):
        z = bank[batch_idx[sol]]                                  # (n_obs, n_per, 2)
        z0, z1 = z[:, :, 0], z[:, :, 1]
        for k in range(1, N):
            o = obst[sol // P, :, k - 1]                          # (n_obs, 5)
            mx, my, ang, major, minor = (o[:, c][:, None] for c in range(5))
            ex, ey = major * z0, minor * z1
            exact = ang == 0.0
            c = np.where(exact, 1.0, np.cos(ang))
            s = np.where(exact, 0.0, np.sin(ang))
            qx = mx + (c * ex - s * ey)
            qy = my + (s * ex + c * ey)
            out[sol, k, :, 0] = qx.reshape(-1)
            out[sol, k, :, 1] = qy.reshape(-1)
        out[sol, 0] = out[sol, 1]
    return out


def reduce_samples_radii(samples: np.ndarray, ref: np.ndarray, n_constraints: int, radius: np.ndarray) -> np.ndarray:
    """scenario.reduce_samples with the radius per sample, radius (M,)"""
    d = samples - ref[None, :]
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    order = np.argsort(dist, kind="stable")[:n_constraints]
    dd, dn = d[order], dist[order]
    n = dd / np.maximum(dn, 1e-9)[:, None]
    b = n[:, 0] * samples[order, 0] + n[:, 1] * samples[order, 1] - radius[order]
    out = np.zeros((n_constraints, 3))
    out[:len(order), 0:2] = n
    out[:len(order), 2] = b
    return out


def prepare_scenario_sampled_host(layout: Layout, stage_params: np.ndarray, state: np.ndarray, samples: np.ndarray,
                                  meta: np.ndarray, P: int, main_warm: np.ndarray | None = None,
                                  robot_radius: float = ROBOT_RADIUS,
                                  deceleration: float = DECELERATION) -> ScenarioBatch:
    """scenario.prepare_scenario_host with the radius per obstacle: the rows of sample m = j n_per + i use
    robot_radius + meta[scene, j, 0].  samples (S*P, N, M, 2) (draw_samples), meta (S, n_obs, 2)."""
    N, npar, nc, nv = layout.N, layout.npar, layout.n_scen, layout.nvar
    S, n_obs = meta.shape[0], meta.shape[1]
    M = samples.shape[2]
    n_per = M // n_obs
    assert samples.shape == (S * P, N, M, 2) and n_per * n_obs == M
    i_scen = layout.idx("disc_0_scenario_constraint_0_a1")
    params = np.repeat(np.repeat(stage_params[:, None, None, :], P, 1), N, 2).reshape(S * P, N, npar)
    warm = np.zeros((S * P, N + 1, nv))
    xinit = np.repeat(state, P, 0).copy()
    for s_ in range(S):
        w = main_warm[s_] if main_warm is not None else braking_warm(state[s_], N, layout.dt, nv, deceleration)
        radius = np.repeat(robot_radius + meta[s_, :, 0], n_per)
        for p_ in range(P):
            b = s_ * P + p_
            warm[b] = w
            rows = np.zeros((N, nc, 3))
            rows[0] = (0.0, 0.0, DUMMY_B)
            for k in range(1, N):
                rows[k] = reduce_samples_radii(samples[b, k], w[k, 2:4], nc, radius)
            params[b, :, i_scen:i_scen + 3 * nc] = rows.reshape(N, 3 * nc)
    return ScenarioBatch(params=params, warm=warm, xinit=xinit, n_scenes=S, n_solvers=P)


def advance_host(layout: Layout, best: np.ndarray, exit_code: np.ndarray, xtraj: np.ndarray, utraj: np.ndarray,
                 lam_out: np.ndarray | None, state_next: np.ndarray, P: int, deceleration: float = DECELERATION):
    """mpcg_scenario_advance on the host -> (main_warm (S, N+1, nu+nx), lam_next like lam_out or None).
    best >= 0: Solver::initializeWarmstart(state_next, true) of the winner's output, [state, out_2 .. out_{N-1},
    out_{N-1}, out_{N-1}], stage 0's inputs out_1's; else Solver::initializeWithBraking(state_next), the slack 0.
    lam_next: a copy's lam_out when its exit code is 1, zero otherwise."""
    N, nu, nv = layout.N, layout.nu, layout.nvar
    S = len(best)
    main_warm = np.zeros((S, N + 1, nv))
    for sc in range(S):
        if best[sc] < 0:
            main_warm[sc] = braking_warm(state_next[sc], N, layout.dt, nv, deceleration)
            continue
        b = sc * P + int(best[sc])
        for k in range(N + 1):
            src = 1 if k == 0 else min(k + 1, N - 1)
            main_warm[sc, k, :nu] = utraj[b, src]
            main_warm[sc, k, nu:] = state_next[sc] if k == 0 else xtraj[b, src]
    lam_next = None
    if lam_out is not None:
        ok = np.asarray(exit_code).reshape(-1) == 1
        lam_next = np.where(ok[:, None, None], lam_out, 0.0)
    return main_warm, lam_next


@dataclass
class PredictionScenes:
    """Scene-level SH-MPC inputs with predictions in place of samples (the mpcg_scenario_sample_io buffers)."""
    stage_params: np.ndarray  # (S, npar)
    state: np.ndarray         # (S, nx)
    obst: np.ndarray          # (S, n_obs, N, 5)
    obst_meta: np.ndarray     # (S, n_obs, 2)
    bank: np.ndarray          # (n_batches, n_per, 2)
    n_solvers: int
    seed: int                 # of the derived batch index
    main_warm: np.ndarray | None = None  # (S, N+1, nu+nx) or None = braking plan

    @property
    def n_per(self) -> int:
        return self.bank.shape[1]

    def batch_index(self, draw: int) -> np.ndarray:
        S, n_obs = self.obst.shape[0], self.obst.shape[1]
        return batch_index(self.seed, draw, S * self.n_solvers, n_obs, self.bank.shape[0])


def make_shmpc_prediction_scenes(layout: Layout, n_scenes: int, n_solvers: int = PARALLEL_SOLVERS, n_obs: int = 12,
                                 n_samples: int = 100, seed: int = SEED0, first_scene: int = 0,
                                 previous_plan_warm: bool = True, n_batches: int = BANK_BATCHES) -> PredictionScenes:
    """The scenes of scenario.make_shmpc_scenes (the same draws: path, state, obstacle mean paths, previous
    plan) with every obstacle as a GAUSSIAN constant-velocity prediction in place of the drawn samples:
    obstacles.constant_velocity_prediction(..., probabilistic=True), the per-step sigma 0.3 propagated over
    the horizon, so that stage k (prediction k - 1) has the mean of make_shmpc_scenes' stage k and its
    spread 0.3 dt sqrt(k).  The bank is drawn from stream 99 of `seed`."""
    assert layout.model == "unicycle_slack" and layout.n_scen > 0
    N, dt = layout.N, layout.dt
    S = n_scenes
    stage_params = np.zeros((S, layout.npar))
    state = np.zeros((S, layout.nx))
    obst = np.zeros((S, n_obs, N, 5))
    meta = np.zeros((S, n_obs, 2))
    main_warm = np.zeros((S, N + 1, layout.nvar)) if previous_plan_warm else None
    for sc in range(S):
        world = shmpc_scene_world(layout, n_obs, seed + first_scene + sc)
        state[sc], stage_params[sc] = world["state"], world["stage_params"]
        obs = []
        for j in range(n_obs):
            o = ob.DynamicObstacle(j, tuple(world["means"][j, 0]), 0.0, OBSTACLE_RADIUS)
            # prediction step k - 1 is read by stage k: it starts one step ahead
            o.prediction_type, o.mode = ob.constant_velocity_prediction(world["means"][j, 1], world["velocity"][j], dt,
                                                                        N, probabilistic=True)
            obs.append(o)
        obst[sc], meta[sc] = ob.scene_obstacle_arrays(obs, N)
        if main_warm is not None:
            main_warm[sc] = shmpc_previous_plan(layout, world, seed + first_scene + sc)
    bank = np.random.default_rng([seed, 99]).normal(size=(n_batches, n_samples, 2))
    return PredictionScenes(stage_params=stage_params, state=state, obst=obst, obst_meta=meta, bank=bank,
                            n_solvers=n_solvers, seed=seed, main_warm=main_warm)
