"""Fleets of robots that plan around each other, device-resident across control steps.

F fleets (independent worlds) x R robots; robot r of fleet f is planner scene
s = f * R + r of a `ControlLoop` with S = F * R scenes.  The robots of all fleets
step in lockstep at the same time `now`: a plan published at step t is what the
other robots of the fleet see at step t + 1, so reception and publication coincide
and one copy per sender (`sent_plan`, `sent_time`) is both what the receivers hold
of that sender and the sender's own `last_communicated_trajectory`.

  obstacle lists    JulesJackalPlanner::prepareObstacleData (jules_ros1_jackalplanner.cpp:800-850):
                    time shift of every received plan (Trajectory::interpolateTrajectoryByElapsedTime,
                    data_types.cpp:257-429), merge with the array obstacles
                    (MultiRobot::updateRobotObstaclesFromTrajectories, data_preparation.cpp:202-237),
                    keep the closest / pad (ensureObstacleSize, :97-173) -- obstacles.py on the host
                    (`fleet_obstacles_host`), fleet_shift_kernel + fleet_obstacles_kernel on the GPU
  plan of a step    success: the selected planner's stages 0..N-1 (Planner::solveMPC, planner.cpp:204-208);
                    failure: applyBrakingCommand + buildOutputFromBrakingCommand
                    (jules_ros1_jackalplanner.cpp:1169-1217)
  topology          _output is rebuilt every solve (planner.cpp:89-92): the previous topology of a
                    failed step is -1; following_new_topology (:221)
  triggers          shouldCommunicate (jules_ros1_jackalplanner.cpp:1420-1501) over
                    CommunicationTriggers::* (mpc_planner_communication/src/communication_triggers.cpp),
                    decideCommunication (:1401-1418), publishDirectTrajectory (:1265-1328)
                    -- `publish_host` here, fleet_publish_kernel on the GPU

C ABI: include/mpcg_fleet.h.  `RosTools::angleToQuaternion` / `quaternionToAngle`, which
a plan passes through on its way over the network in the reference, are skipped (the angle
is carried as it is; parity unpinned there, as in obstacles.py), and ties of equal scores in
ensureObstacleSize's `std::sort` are broken by the lower candidate index.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import obstacles as ob

# CommunicationTriggerReason (communication_triggers.h)
NO_COMMUNICATION, INFEASIBLE, TOPOLOGY_CHANGE, GEOMETRIC, TIME, NON_GUIDED_HOMOLOGY_FAIL = 0, 1, 3, 4, 5, 6


@dataclass
class FleetSettings:
    """The settings the multi-robot layer reads (mpc_planner_jackalsimulator/config/settings.yaml)."""
    control_frequency: float = 20.0
    v_max: float = 2.5                     # JULES.robot_max_velocity
    w_max: float = 2.5                     # JULES.robot_max_angular_velocity
    robot_obstacle_radius: float = 0.325
    probabilistic: bool = False            # probabilistic.enable
    risk: float = 0.05                     # probabilistic.risk
    communicate_on_topology_switch_only: bool = True
    n_paths: int = 4
    max_geometric_deviation: float = 5.0
    heartbeat_time: float = 2.0
    deceleration: float = 3.0              # deceleration_at_infeasible

    @property
    def chi_gaussian(self) -> float:
        return ob.exponential_quantile(0.5, 1.0 - self.risk)

    def native(self):
        from .native_spec import MpcgFleetSettings
        return MpcgFleetSettings(self.control_frequency, self.v_max, self.w_max, self.robot_obstacle_radius,
                                 int(self.probabilistic), self.chi_gaussian,
                                 int(self.communicate_on_topology_switch_only), self.n_paths,
                                 self.max_geometric_deviation, self.heartbeat_time, self.deceleration)


def initial_state(F: int, R: int, N: int) -> dict:
    """The per-sender state before the first step: nothing received, never sent, topology -1."""
    return dict(sent_plan=np.zeros((F, R, N, 3)), sent_time=np.full((F, R), np.nan),
                last_send_time=np.full((F, R), np.nan), prev_topology=np.full((F, R), -1, np.int32))


# ------------------------------------------------------------------ publication


def publish_host(best, xtraj, state, fstate: dict, now: float, dt: float, settings: FleetSettings, topology=None,
                 guided=None) -> dict:
    """The publish step of every robot after the solves of step `now` (NumPy, batched).

    best (S,), xtraj (S*G, N+1, nx), state (S, nx); fstate: dict sent_plan (F, R, N, 3), sent_time,
    last_send_time, prev_topology (F, R) (not modified); topology (S, G) or None = the planner index
    for guided planners and 2 n_paths for the non-guided one (guided (S, G), None = all guided).
    Returns dict(plan (S, N, 3), selected, reason, published (S,), and the new sent_plan, sent_time,
    last_send_time, prev_topology in fstate's shapes)."""
    best = np.asarray(best).astype(np.int64)
    S = best.shape[0]
    state = np.asarray(state, np.float64).reshape(S, -1)
    shape = np.asarray(fstate["sent_time"]).shape
    sent_plan = np.array(fstate["sent_plan"], np.float64)
    N = sent_plan.shape[-2]
    sent_plan = sent_plan.reshape(S, N, 3)
    sent_time = np.array(fstate["sent_time"], np.float64).reshape(S)
    last_send = np.array(fstate["last_send_time"], np.float64).reshape(S)
    prev = np.asarray(fstate["prev_topology"]).reshape(S).astype(np.int64)
    xt = np.asarray(xtraj, np.float64)
    xt = xt.reshape(S, -1, N + 1, xt.shape[-1])
    G = xt.shape[1]
    non_guided_id = 2 * settings.n_paths
    ok = (best >= 0) & (best < G)
    b = np.where(ok, best, 0)
    rows = np.arange(S)
    # the plan: the winner's stages 0..N-1 (planner.cpp:204-208) ...
    plan = xt[rows, b, :N, :3].copy()
    # ... or the braking plan (applyBrakingCommand, buildOutputFromBrakingCommand, :1169-1217; positions
    # of getConstantVelocityPrediction, data_preparation.cpp:75: position + velocity * dt * i)
    after = state[:, 3] - settings.deceleration * (1.0 / settings.control_frequency)
    vb = np.where(after < 0.0, 0.0, after)
    i = np.arange(N, dtype=np.float64)[None, :]
    psi = state[:, 2]
    brake = np.empty((S, N, 3))
    brake[:, :, 0] = state[:, 0:1] + (np.cos(psi) * vb)[:, None] * dt * i
    brake[:, :, 1] = state[:, 1:2] + (np.sin(psi) * vb)[:, None] * dt * i
    brake[:, :, 2] = psi[:, None]
    plan[~ok] = brake[~ok]
    # selected topology: _output is rebuilt every solve, so a failed step leaves -1 (planner.cpp:89-92)
    if topology is not None:
        topo = np.asarray(topology).reshape(S, G).astype(np.int64)
    else:
        g = np.ones((S, G), bool) if guided is None else np.asarray(guided).reshape(S, G).astype(bool)
        topo = np.where(g, np.arange(G)[None, :], non_guided_id)
    selected = np.where(ok, topo[rows, b], -1)
    following_new = selected != prev                       # planner.cpp:221
    # triggers, highest priority first (shouldCommunicate, :1439-1493)
    received = ~np.isnan(sent_time)
    ex, ey = plan[:, :, 0] - sent_plan[:, :, 0], plan[:, :, 1] - sent_plan[:, :, 1]
    max_sq = settings.max_geometric_deviation * settings.max_geometric_deviation
    geometric = received & ((ex * ex + ey * ey) > max_sq).any(axis=1)      # geomtricDeviationTrigger
    with np.errstate(invalid="ignore"):
        heartbeat = np.isnan(last_send) | ((now - last_send) >= settings.heartbeat_time)   # checkTime
    if settings.communicate_on_topology_switch_only:
        reason = np.select([~ok, selected == non_guided_id, following_new, geometric, heartbeat],
                           [INFEASIBLE, NON_GUIDED_HOMOLOGY_FAIL, TOPOLOGY_CHANGE, GEOMETRIC, TIME],
                           NO_COMMUNICATION).astype(np.int32)
        published = reason != NO_COMMUNICATION
    else:                                                  # decideCommunication, :1407-1412
        reason = np.zeros(S, np.int32)
        published = np.ones(S, bool)
    # publishDirectTrajectory: the plan as sent, last_send_trajectory_time, last_communicated_trajectory
    sent_plan[published] = plan[published]
    sent_time[published] = now
    last_send[published] = now
    return dict(plan=plan, selected=selected.astype(np.int32), reason=reason, published=published.astype(np.uint8),
                sent_plan=sent_plan.reshape(*shape, N, 3), sent_time=sent_time.reshape(shape),
                last_send_time=last_send.reshape(shape), prev_topology=selected.astype(np.int32).reshape(shape))


# ------------------------------------------------------------------ obstacle lists


def _row_obstacle(index: int, rows, meta) -> ob.DynamicObstacle:
    """An array obstacle given as solver rows (N, 5) / (radius, chi), as a DynamicObstacle."""
    rows = np.asarray(rows, np.float64)
    o = ob.DynamicObstacle(int(index), (float(rows[0, 0]), float(rows[0, 1])), float(rows[0, 2]), float(meta[0]))
    o.prediction_type = ob.DETERMINISTIC if meta[1] == 1.0 else ob.GAUSSIAN
    for k in range(rows.shape[0]):
        o.mode.append(rows[k, 0:2], rows[k, 2], rows[k, 3], rows[k, 4])
    o.rows, o.meta = rows, np.asarray(meta, np.float64)
    return o


def fleet_obstacles_host(state, fstate: dict, now: float, N: int, dt: float, n_ell: int, settings: FleetSettings,
                         array_obst=None, array_meta=None, array_id=None) -> dict:
    """The obstacle rows of every robot at step `now`, through obstacles.py: per receiver the
    robot obstacles of the other senders (`RobotObstacleTracker`'s state, filled from the fleet's
    per-sender copies), `interpolate_by_elapsed_time`, `update_robot_obstacles`,
    `ensure_obstacle_size` and `scene_obstacle_arrays`.

    state (S, nx); fstate: dict sent_plan (F, R, N, 3), sent_time (F, R) (not modified); array_obst
    (F, A, N, 5), array_meta (F, A, 2), array_id (F, A) or None = ids R + a.
    Returns dict(obst (S, n_ell, N, 5), obst_meta (S, n_ell, 2), sent_plan, sent_time (shifted),
    kept: per robot the source of each row -- ("array", a), ("robot", q) or ("dummy", -1))."""
    sent_plan = np.array(fstate["sent_plan"], np.float64)
    sent_time = np.array(fstate["sent_time"], np.float64)
    F, R = sent_time.shape
    S = F * R
    state = np.asarray(state, np.float64).reshape(S, -1)
    A = 0 if array_obst is None else np.asarray(array_obst).shape[1]
    obst = np.zeros((S, n_ell, N, 5))
    meta = np.zeros((S, n_ell, 2))
    new_plan, new_time = sent_plan.copy(), sent_time.copy()
    kept = []
    for f in range(F):
        for r in range(R):
            s = f * R + r
            # the receiver's robot obstacles (trajectoryCallback's result, held since sent_time)
            robots, validated = {}, set()
            for q in range(R):
                if q == r:
                    continue
                ro = ob.DynamicObstacle(q, (100.0, 100.0), 0.0, settings.robot_obstacle_radius)
                if not math.isnan(sent_time[f, q]):
                    for k in range(N):
                        ro.mode.append(sent_plan[f, q, k, 0:2], sent_plan[f, q, k, 2], -1.0, -1.0)
                    ro.position, ro.angle = ro.mode.positions[0], ro.mode.angles[0]
                    ro.last_update_time = float(sent_time[f, q])
                    validated.add(q)
                ro.source = ("robot", q)
                robots[q] = ro
            # prepareObstacleData
            for q in sorted(robots):
                if ob.interpolate_by_elapsed_time(robots[q], now, N, dt, settings.control_frequency,
                                                  v_max=settings.v_max, w_max=settings.w_max):
                    new_plan[f, q, :, 0:2] = robots[q].mode.positions
                    new_plan[f, q, :, 2] = robots[q].mode.angles
                    new_time[f, q] = robots[q].last_update_time
            arr = []
            for a in range(A):
                o = _row_obstacle(R + a if array_id is None else array_id[f][a], array_obst[f][a], array_meta[f][a])
                o.source = ("array", a)
                arr.append(o)
            merged = ob.update_robot_obstacles(arr, robots, validated)
            lst = ob.ensure_obstacle_size(merged, state[s], n_ell, N, dt, settings.probabilistic)
            obst[s], meta[s] = ob.scene_obstacle_arrays(lst, N, settings.risk)
            for j, o in enumerate(lst):       # array obstacles keep the rows they came with
                if hasattr(o, "rows"):
                    obst[s, j], meta[s, j] = o.rows, o.meta
            kept.append([getattr(o, "source", ("dummy", -1)) for o in lst])
    return dict(obst=obst, obst_meta=meta, sent_plan=new_plan, sent_time=new_time, kept=kept)


# ------------------------------------------------------------------ the device loop


class FleetLoop:
    """Consecutive control steps of F fleets x R robots on one GPU: a `ControlLoop` over the
    S = F * R planner scenes whose obstacle predictions are the other robots' published plans.

        step(now):  mpcg_fleet_obstacles (shift the published plans to `now`, obstacle rows of every
                    robot, straight into the loop's obst / obst_meta) -> ControlLoop.step ->
                    mpcg_fleet_publish (plan, topology, trigger, the per-sender state)

    Guidance trajectories still come from outside (`loop.set_scene_data`).  loop_options are ControlLoop's
    keywords (guidance_layer=..., skip_disabled=True: the planners the layer disables are not solved)."""

    def __init__(self, layout, scenes, F: int, R: int, device, settings: FleetSettings, robot_radius: float,
                 w_consistency: float, selection_weight: float, **loop_options):
        import torch

        from .control_loop import ControlLoop

        if scenes.n_scenes != F * R:
            raise ValueError(f"{scenes.n_scenes} scenes for {F} fleets x {R} robots")
        loop_options.setdefault("deceleration", settings.deceleration)
        self.loop = ControlLoop(layout, scenes, device, robot_radius, w_consistency, selection_weight, **loop_options)
        self.F, self.R, self.settings = F, R, settings
        self._set = settings.native()
        S, N = F * R, layout.N
        init = initial_state(F, R, N)
        self.state = {k: torch.from_numpy(v).to(device) for k, v in init.items()}
        self.reason = torch.zeros((S,), dtype=torch.int32, device=device)
        self.published = torch.zeros((S,), dtype=torch.uint8, device=device)
        self.array_obst = self.array_meta = self.array_id = None
        # the table of the fleets' tracked objects (set_tracks) or None: nothing is launched
        self.tracks = None

    def set_tracks(self, pose, twist, dims, shape, settings=None):
        """The fleets' non-communicating objects as tracked objects (include/mpcg_tracks.h), in place of
        set_array_obstacles: pose (F, A, 3), twist (F, A, 2), dims (F, A, 2), shape (F, A) int32.  Every step
        first runs mpcg_tracks_rows over the F worlds; its rows are what mpcg_fleet_obstacles then reads as
        array_obst / array_meta, ids R + a.  Every slot must give exactly one row (UNSEEN, DISC, CYLINDER or a
        square BOX; checked here on the host copy of shape and dims), so that row a is object a.  settings:
        tracks.TrackSettings (None: the defaults with the fleet's probabilistic and risk).  Device tensors are
        taken as they are -- self.tracks holds them -- so the caller may update them in place between steps
        (a shape that changes must keep to the one-row shapes)."""
        import torch

        from . import native
        from .tracks import TrackSettings, single_row_shapes

        host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
        if not single_row_shapes(host(shape), host(dims)):
            raise ValueError("FleetLoop.set_tracks: every slot must give exactly one row (UNSEEN, DISC, CYLINDER or a "
                             "square BOX)")
        lp = self.loop
        table = native.track_table_device(pose, twist, dims, shape, lp.dev)
        W, A = table["shape"].shape
        if W != self.F:
            raise ValueError(f"FleetLoop.set_tracks: {W} worlds for {self.F} fleets")
        if settings is None:
            settings = TrackSettings(probabilistic=self.settings.probabilistic, risk=self.settings.risk)
        self._track_set = settings.native()
        self._track_rows = native.track_rows_buffers(self.F, A, lp.lay.N, lp.dev)
        f64 = dict(dtype=torch.float64, device=lp.dev)
        self.array_obst = torch.zeros((self.F, A, lp.lay.N, 5), **f64)
        self.array_meta = torch.zeros((self.F, A, 2), **f64)
        self.array_id = None
        self.tracks = table

    def set_array_obstacles(self, array_obst, array_meta, array_id=None):
        """The fleets' non-communicating obstacles: array_obst (F, A, N, 5), array_meta (F, A, 2) rows as in
        mpcg_scene_io.obst / obst_meta, array_id (F, A) (None: ids R + a)."""
        import torch

        dev = self.loop.dev
        self.tracks = None
        self.array_obst = torch.as_tensor(array_obst, dtype=torch.float64, device=dev).contiguous()
        self.array_meta = torch.as_tensor(array_meta, dtype=torch.float64, device=dev).contiguous()
        self.array_id = None if array_id is None else torch.as_tensor(array_id, dtype=torch.int32,
                                                                      device=dev).contiguous()

    def step(self, now: float, topology=None, stream=None):
        """One control step of every robot at time `now`.  topology (S, G) int32 device tensor: the
        topology id of every planner (None: the loop's guidance layer's class ids, or without a layer the
        planner index / 2 n_paths for the non-guided one).
        Returns ControlLoop.step's dict plus reason (S,) int32 and published (S,) uint8."""
        import contextlib

        import torch

        from . import native

        lp = self.loop
        if self.tracks is not None:
            # C = 2 A rows per world, of which the first A are written: the dense [F][A] rows
            # mpcg_fleet_obstacles reads are their copy
            A = self.array_obst.shape[1]
            native.tracks_rows_device(lp.pr, self._track_set, self.tracks, out=self._track_rows, stream=stream)
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                self.array_obst.copy_(self._track_rows["rows"][:, :A])
                self.array_meta.copy_(self._track_rows["rows_meta"][:, :A])
        native.fleet_obstacles_device(lp.pr, self.F, self.R, self._set, self.state, lp.dsc["state"], now,
                                      lp.dsc["obst"], lp.dsc["obst_meta"], self.array_obst, self.array_meta,
                                      self.array_id, stream=stream)
        out = lp.step(stream=stream)
        if topology is None and lp.guidance_layer is not None:
            topology = lp.guidance_layer.topology
        native.fleet_publish_device(lp.pr, self.F, self.R, lp.G, self._set, self.state, out["best"], out["xtraj"],
                                    lp.dsc["state"], now, self.reason, self.published, topology=topology,
                                    guided=lp.dsc["guided"], stream=stream)
        return dict(out, reason=self.reason, published=self.published)

    def advance(self, state_next, stream=None):
        return self.loop.advance(state_next, stream=stream)
