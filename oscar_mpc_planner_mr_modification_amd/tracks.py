"""Tracked objects -> obstacle predictions -> the obstacle rows of a scene: the host restatement of
include/mpcg_tracks.h, composed from obstacles.py.

What the real-robot wrappers of the reference do with the tracked objects they receive at every
control step (pose, body-frame twist, shape):

  object -> discs           JackalPlanner::obstacleCallback, parseObstacle (ros1_jackal.cpp:269-389),
                            DingoPlanner::obstacleCallback (ros1_planner.cpp:242-310),
                            JulesRealJackalPlanner::obstacleCallback (jules_ros1_real_jackalplanner.cpp:532-628),
                            initializeOtherRobotsAsObstacles (:208-231)              -- `tracks_rows_host`
  discs -> predictions      getConstantVelocityPrediction (data_preparation.cpp:60-81) -- obstacles.py
  keep the closest / pad    ensureObstacleSize, then the callback's propagatePredictionUncertainty
                            (data_preparation.cpp:97-197)                            -- `obstacle_select_host`

The specification both this module and the kernels (csrc/mpcg_tracks.h) implement is the text of
include/mpcg_tracks.h.  `rotationMatrixFromHeading` lives in the external ros_tools package: the global
twist is read as the body twist rotated by +yaw (parity unpinned there, as for the other ros_tools
functions in obstacles.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import obstacles as ob

# shape of a slot (include/mpcg_tracks.h, MPCG_TRACK_*)
NONE, UNSEEN, DISC, CYLINDER, BOX = -1, 0, 1, 2, 3
FAR_AWAY = (100.0, 100.0)   # FAR_AWAY_POSITION


@dataclass
class TrackSettings:
    """The settings the tracked-object layer reads (config/settings.yaml of the wrappers)."""
    obstacle_radius: float = 0.5           # obstacle_radius (mpc_planner_jackal)
    probabilistic: bool = False            # probabilistic.enable
    risk: float = 0.05                     # probabilistic.risk

    @property
    def chi_gaussian(self) -> float:
        return ob.exponential_quantile(0.5, 1.0 - self.risk)

    def native(self):
        from .native_spec import MpcgTrackSettings
        return MpcgTrackSettings(self.obstacle_radius, int(self.probabilistic), self.chi_gaussian)


def _cos_sin(a: float):
    """(1, 0) for a == 0.0, else (cos a, sin a): the rule of include/mpcg_scenario.h"""
    return (1.0, 0.0) if a == 0.0 else (math.cos(a), math.sin(a))


def parse_object(pose, twist, dims, shape: int, obstacle_radius: float):
    """One tracked object -> (global twist, [(position, radius), ...]): 0, 1 or 2 discs in parseObstacle's
    order (ros1_jackal.cpp:286-325, 351-389)."""
    shape = int(shape)
    if shape == UNSEEN:
        return (0.0, 0.0), [(FAR_AWAY, float(obstacle_radius))]
    if shape not in (DISC, CYLINDER, BOX):
        return (0.0, 0.0), []
    x, y, yaw = (float(v) for v in pose)
    tx, ty = (float(v) for v in twist)
    m0, m1 = (float(v) for v in dims)
    c, s = _cos_sin(yaw)
    g = (c * tx - s * ty, s * tx + c * ty)
    if shape == DISC:
        return g, [((x, y), float(obstacle_radius))]
    if shape == CYLINDER:
        return g, [((x, y), m1)]
    if m0 == m1:
        return g, [((x, y), math.sqrt(2) * m0)]
    vel = math.sqrt(tx * tx + ty * ty)
    angle = yaw if vel < 0.01 else yaw + math.atan2(ty, tx) + math.pi / 2
    cb, sb = _cos_sin(angle - math.pi / 2)
    small, large = min(m0, m1), max(m0, m1)
    ox, oy = cb * large / 2, sb * large / 2
    radius = math.sqrt(2) * small + 0.05
    return g, [((x + ox, y + oy), radius), ((x - ox, y - oy), radius)]


def world_obstacles(pose, twist, dims, shape, N: int, dt: float, settings: TrackSettings) -> list:
    """The candidate obstacles of one world before ensureObstacleSize: objects in slot order, each disc
    with its constant-velocity prediction (obstacles.constant_velocity_prediction)."""
    out = []
    for a in range(len(shape)):
        g, discs = parse_object(pose[a], twist[a], dims[a], shape[a], settings.obstacle_radius)
        for position, radius in discs:
            o = ob.DynamicObstacle(len(out), position, 0.0, radius)
            o.prediction_type, o.mode = ob.constant_velocity_prediction(position, g, dt, N, settings.probabilistic)
            out.append(o)
    return out


def tracks_rows_host(pose, twist, dims, shape, N: int, dt: float, settings: TrackSettings) -> dict:
    """mpcg_tracks_rows on the host.  pose (W, A, 3), twist (W, A, 2), dims (W, A, 2), shape (W, A).
    Returns dict(rows (W, C, N, 5), rows_meta (W, C, 2), rows_type (W, C) int32, n_rows (W,) int32), C = 2 A;
    what lies past n_rows (the device leaves it unwritten) is zero."""
    pose, twist, dims = (np.asarray(v, np.float64) for v in (pose, twist, dims))
    shape = np.asarray(shape)
    W, A = shape.shape
    Cn = 2 * A
    rows, meta = np.zeros((W, Cn, N, 5)), np.zeros((W, Cn, 2))
    kind, n_rows = np.zeros((W, Cn), np.int32), np.zeros((W,), np.int32)
    for w in range(W):
        lst = world_obstacles(pose[w], twist[w], dims[w], shape[w], N, dt, settings)
        n = n_rows[w] = len(lst)
        if n:
            rows[w, :n], meta[w, :n] = ob.scene_obstacle_arrays(lst, N, settings.risk)
            kind[w, :n] = [o.prediction_type for o in lst]
    return dict(rows=rows, rows_meta=meta, rows_type=kind, n_rows=n_rows)


def _row_obstacle(index: int, rows, meta, kind: int) -> ob.DynamicObstacle:
    """a candidate row as the obstacle it stands for"""
    o = ob.DynamicObstacle(index, (float(rows[0, 0]), float(rows[0, 1])), 0.0, float(meta[0]))
    o.prediction_type = ob.GAUSSIAN if int(kind) == ob.GAUSSIAN else ob.DETERMINISTIC
    for k in range(rows.shape[0]):
        o.mode.append(rows[k, 0:2], rows[k, 2], rows[k, 3], rows[k, 4])
    o.candidate, o.chi = index, float(meta[1])
    return o


def obstacle_select_host(rows, rows_meta, rows_type, n_rows, state, n_ell: int, dt: float, settings: TrackSettings,
                         propagate: bool = False) -> dict:
    """mpcg_obstacle_select on the host: obstacles.ensure_obstacle_size, then (propagate) one more pass of
    obstacles.propagate_uncertainty over every row, then obstacles.scene_obstacle_arrays.
    rows (S, max_rows, N, 5), rows_meta (S, max_rows, 2), rows_type (S, max_rows), n_rows (S,), state (S, nx).
    Returns dict(obst (S, n_ell, N, 5), obst_meta (S, n_ell, 2), kept (S, n_ell) int32: the candidate index of
    every output row, -1 for a dummy)."""
    rows, rows_meta = np.asarray(rows, np.float64), np.asarray(rows_meta, np.float64)
    S, max_rows, N, _ = rows.shape
    state = np.asarray(state, np.float64).reshape(S, -1)
    obst, meta = np.zeros((S, n_ell, N, 5)), np.zeros((S, n_ell, 2))
    kept = np.full((S, n_ell), -1, np.int32)
    for s in range(S):
        n = min(max(int(n_rows[s]), 0), max_rows)
        cand = [_row_obstacle(c, rows[s, c], rows_meta[s, c], rows_type[s][c]) for c in range(n)]
        lst = ob.ensure_obstacle_size(cand, state[s], n_ell, N, dt, settings.probabilistic)
        if propagate:
            for o in lst:
                ob.propagate_uncertainty(o.prediction_type, o.mode, dt, N)
        obst[s], meta[s] = ob.scene_obstacle_arrays(lst, N, settings.risk)
        for j, o in enumerate(lst):
            kept[s, j] = getattr(o, "candidate", -1)
            if hasattr(o, "chi") and o.prediction_type == ob.GAUSSIAN:
                meta[s, j, 1] = o.chi    # a GAUSSIAN row keeps the chi it came with
    return dict(obst=obst, obst_meta=meta, kept=kept)


def tracks_obstacles_host(pose, twist, dims, shape, state, n_ell: int, N: int, dt: float, settings: TrackSettings,
                          propagate: bool = False) -> dict:
    """tracks_rows_host, then obstacle_select_host: the obst / obst_meta of every scene from its tracked objects
    (scene s reads world s).  Returns obstacle_select_host's dict plus the candidate rows."""
    r = tracks_rows_host(pose, twist, dims, shape, N, dt, settings)
    out = obstacle_select_host(r["rows"], r["rows_meta"], r["rows_type"], r["n_rows"], state, n_ell, dt, settings,
                               propagate)
    return dict(out, **r)


def single_row_shapes(shape, dims) -> bool:
    """whether every slot gives exactly one row: UNSEEN, DISC, CYLINDER or a square BOX (FleetLoop.set_tracks)"""
    shape, dims = np.asarray(shape), np.asarray(dims, np.float64)
    one = (shape == UNSEEN) | (shape == DISC) | (shape == CYLINDER) | ((shape == BOX) & (dims[..., 0] == dims[..., 1]))
    return bool(one.all())
