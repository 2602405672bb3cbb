"""Reference-path tracking of the control loop, device-resident across control steps.

What the contouring module does outside the solve, once per control step and scene:

  path table        Contouring::onDataReceived (contouring.cpp:128-159): RosTools::Spline2D(x, y[, s]),
                    one natural cubic spline per axis over the cumulative chord length -- `fit_path`,
                    on the host, once per path; `PathTable` stacks P paths for the device
  update            Contouring::update (:28-50): findClosestPoint from the current segment,
                    state.set("spline", closest_s); setSplineParameters (:96-126): the window of n_seg
                    segments from the closest one; isObjectiveReached (:169-177)
                    -- `path_update_host` here, path_update_kernel on the GPU
  command           the wrapper's loop (ros1_jackalsimulator.cpp:181-201): v of the plan's stage 1 and w
                    of its stage 0, or braking at deceleration_at_infeasible
                    -- `command_host` here, path_command_kernel on the GPU

C ABI and the search rule: include/mpcg_path.h.  ros_tools is not part of the reference tree, so the
spline fit and the closest-point search restate its interface, not its code: the contract of the
search is the minimiser of |p(s) - q|^2 over the +-2 segments around the current one (the whole path
after a new path), and what `Spline2D::getParameters` returns for an index past the last segment is
replaced by the rule the reference documents for that case (contouring.cpp:425-444).  Parity with
ros_tools is unpinned for both.

Order of a step (planner.cpp:139 setXinit before :146-147 update; the odometry callbacks set only
x, y, psi, v): the window of step t comes from closest_s(t), while the `spline` entry of the state
the solve of step t starts from is closest_s(t - 1) -- the update of step t leaves its closest_s in
the state of step t + 1 (`PathLoop.advance`).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .native_spec import PATH_MAX_SEGMENTS, PATH_REACHED_RADIUS, PATH_ROUNDS, PATH_SAMPLES

_LAST = float(PATH_SAMPLES - 1)
_LANES = np.arange(PATH_SAMPLES, dtype=np.float64)


# ------------------------------------------------------------------ the path table


def _natural_cubic(t, y):
    """Natural cubic spline through (t_i, y_i): rows (a, b, c, d) of y_i(u) = a u^3 + b u^2 + c u + d,
    u = t - t_i, with zero second derivative at both ends."""
    n = len(t)
    h = np.diff(t)
    b = np.zeros(n)
    if n > 2:
        A = np.zeros((n, n))
        r = np.zeros(n)
        A[0, 0] = A[n - 1, n - 1] = 1.0
        for i in range(1, n - 1):
            A[i, i - 1] = h[i - 1] / 3.0
            A[i, i] = 2.0 * (h[i - 1] + h[i]) / 3.0
            A[i, i + 1] = h[i] / 3.0
            r[i] = (y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1]
        b = np.linalg.solve(A, r)
        b[0] = b[n - 1] = 0.0
    a = (b[1:] - b[:-1]) / (3.0 * h)
    c = (y[1:] - y[:-1]) / h - (2.0 * b[:-1] + b[1:]) * h / 3.0
    return np.stack([a, b[:-1], c, y[:-1]], 1)


def fit_path(x, y, s=None) -> dict:
    """RosTools::Spline2D(x, y[, s]) as Contouring::onDataReceived builds it: the parameter is `s`, or
    the cumulative chord length of the waypoints; one natural cubic spline per axis.
    Returns dict(coef (m, 8) rows xa xb xc xd ya yb yc yd, knots (m + 1,)), m = len(x) - 1 segments;
    knots[m] is parameterLength()."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.ndim != 1 or x.shape != y.shape or len(x) < 2:
        raise ValueError("fit_path: needs two equally long waypoint lists of at least two points")
    if s is None:
        s = np.concatenate([[0.0], np.cumsum(np.sqrt(np.diff(x) ** 2 + np.diff(y) ** 2))])
    s = np.asarray(s, np.float64)
    if s.shape != x.shape or not (np.diff(s) > 0.0).all():
        raise ValueError("fit_path: the path parameter must increase strictly from waypoint to waypoint")
    return dict(coef=np.concatenate([_natural_cubic(s, x), _natural_cubic(s, y)], 1), knots=s.copy())


@dataclass
class PathTable:
    """P paths stacked for the device (include/mpcg_path.h): coef (P, M, 8), knots (P, M + 1),
    n_segments (P,) int32; rows past a path's n_segments are zero, knots past it repeat its length."""
    coef: np.ndarray
    knots: np.ndarray
    n_segments: np.ndarray

    @classmethod
    def from_paths(cls, paths, M: int | None = None) -> "PathTable":
        """paths: dicts of `fit_path` (or any coef (m, 8) / knots (m + 1,) pair)."""
        ms = [len(p["knots"]) - 1 for p in paths]
        M = max(ms) if M is None else M
        if not paths or min(ms) < 1 or max(ms) > M or M > PATH_MAX_SEGMENTS:
            raise ValueError(f"PathTable: needs 1 <= segments <= M <= {PATH_MAX_SEGMENTS} for every path")
        coef = np.zeros((len(paths), M, 8))
        knots = np.zeros((len(paths), M + 1))
        for p, (path, m) in enumerate(zip(paths, ms)):
            coef[p, :m] = np.asarray(path["coef"], np.float64).reshape(m, 8)
            knots[p, :m + 1] = path["knots"]
            knots[p, m + 1:] = path["knots"][m]
        return cls(coef, knots, np.asarray(ms, np.int32))

    def point(self, p: int, s: float) -> np.ndarray:
        """getPoint(s) of path p (s clipped to the path)."""
        m = int(self.n_segments[p])
        K = self.knots[p]
        s = min(max(float(s), K[0]), K[m])
        j = _segment(K, m, np.array([s]))[0]
        return np.array(_point(self.coef[p], K, np.array([j]), np.array([s])))[:, 0]


# ------------------------------------------------------------------ the update (host restatement)
# One rounding per operation, in the kernel's order (csrc/mpcg_path.h, compiled without contraction).


def _sample(lo, hi, i):
    return np.minimum(lo + ((hi - lo) * i) / _LAST, hi)


def _segment(K, m, s):
    return (K[None, 1:m] <= np.asarray(s)[:, None]).sum(1)


def _point(coef, K, j, s):
    t = s - K[j]
    c = coef[j]
    return (((c[:, 0] * t + c[:, 1]) * t + c[:, 2]) * t + c[:, 3],
            ((c[:, 4] * t + c[:, 5]) * t + c[:, 6]) * t + c[:, 7])


def _dist2(px, py, qx, qy):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = px - qx, py - qy
        d = dx * dx + dy * dy
    return np.where(np.isnan(d), np.inf, d)


def closest_point_host(coef, K, m: int, q, c_in: int):
    """The search of include/mpcg_path.h on one path (coef (>= m, 8), knots K (>= m + 1,)) for the
    point q = (x, y) from segment c_in (< 0: not initialised).  Returns (closest_s, segment)."""
    qx, qy = float(q[0]), float(q[1])
    rnd = 0
    if c_in < 0:
        bd = np.full(PATH_SAMPLES, np.inf)
        bp = np.zeros(PATH_SAMPLES, np.int64)
        for j in range(m):
            sj = _sample(K[j], K[j + 1], _LANES)
            px, py = _point(coef, K, np.full(PATH_SAMPLES, j), sj)
            d = _dist2(px, py, qx, qy)
            better = d < bd
            bd, bp = np.where(better, d, bd), np.where(better, j, bp)
        w = int(np.argmin(bd))          # the first of equal minima: the lowest lane
        j = int(bp[w])
        best = _sample(K[j], K[j + 1], float(w))
        if w > 0:
            lo = _sample(K[j], K[j + 1], float(w - 1))
        else:
            lo = _sample(K[j - 1], K[j], float(PATH_SAMPLES - 2)) if j > 0 else best
        if w < PATH_SAMPLES - 1:
            hi = _sample(K[j], K[j + 1], float(w + 1))
        else:
            hi = _sample(K[j + 1], K[j + 2], 1.0) if j < m - 1 else best
        rnd = 1
    else:
        c = min(int(c_in), m - 1)
        lo, hi = K[max(0, c - 2)], K[min(m, c + 3)]
        best = lo
    for _ in range(rnd, PATH_ROUNDS):
        si = _sample(lo, hi, _LANES)
        px, py = _point(coef, K, _segment(K, m, si), si)
        w = int(np.argmin(_dist2(px, py, qx, qy)))
        best = si[w]
        lo, hi = si[max(w - 1, 0)], si[min(w + 1, PATH_SAMPLES - 1)]
    return float(best), int(_segment(K, m, np.array([best]))[0])


def path_update_host(state, closest_segment, table: PathTable, path_of, stage_params, i_spline0: int,
                     n_seg: int) -> dict:
    """The reference-path update of every scene (NumPy; the restatement of path_update_kernel).
    state (S, nx), closest_segment (S,) (-1: not initialised), path_of (S,), stage_params (S, npar);
    none is modified.  Returns dict(closest_segment (S,) int32, closest_s (S,), stage_params (S, npar)
    with the window of n_seg segments at i_spline0, reached (S,) uint8)."""
    state = np.asarray(state, np.float64)
    S = state.shape[0]
    if n_seg < 1:
        raise ValueError("path_update_host: n_seg < 1")
    sp = np.array(stage_params, np.float64)
    seg = np.zeros(S, np.int32)
    cs = np.zeros(S)
    reached = np.zeros(S, np.uint8)
    for s in range(S):
        p = int(path_of[s])
        if not 0 <= p < len(table.n_segments):
            raise ValueError(f"path_update_host: path_of[{s}] = {p} outside the table")
        m, K, coef = int(table.n_segments[p]), table.knots[p], table.coef[p]
        cs[s], c = closest_point_host(coef, K, m, state[s, 0:2], int(closest_segment[s]))
        seg[s] = c
        ex, ey = (float(v[0]) for v in _point(coef, K, np.array([m - 1]), np.array([K[m]])))
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = state[s, 0] - ex, state[s, 1] - ey
            reached[s] = np.sqrt(dx * dx + dy * dy) < PATH_REACHED_RADIUS
        for i in range(n_seg):
            j = c + i
            row = np.concatenate([coef[j], [K[j]]]) if j < m else np.array([0, 0, 0, ex, 0, 0, 0, ey, K[m]], float)
            sp[s, i_spline0 + 9 * i:i_spline0 + 9 * i + 9] = row
    return dict(closest_segment=seg, closest_s=cs, stage_params=sp, reached=reached)


# ------------------------------------------------------------------ the command


@dataclass
class PathSettings:
    control_frequency: float = 20.0       # settings.yaml: control_frequency
    deceleration: float = 3.0             # deceleration_at_infeasible
    plant: bool = False                   # the kinematic stand-in for the simulator (next state)

    def native(self):
        from .native_spec import MpcgPathSettings
        return MpcgPathSettings(self.control_frequency, self.deceleration, int(self.plant))


def command_host(best, xtraj, utraj, state, settings: PathSettings, closest_s=None, spline_slot: int = -1) -> dict:
    """The command of every scene (NumPy; the restatement of path_command_kernel): best (S,), xtraj
    (S*G, N+1, nx), utraj (S*G, N, nu), state (S, nx).  Returns dict(cmd (S, 2) = (v, w), state_next
    (S, nx) or None without the plant: the kinematic stand-in over one control period, entry
    spline_slot = closest_s)."""
    best = np.asarray(best).astype(np.int64)
    S = best.shape[0]
    state = np.asarray(state, np.float64).reshape(S, -1)
    xt, ut = np.asarray(xtraj, np.float64), np.asarray(utraj, np.float64)
    G = xt.shape[0] // S
    ok = (best >= 0) & (best < G)
    rows = np.arange(S) * G + np.where(ok, best, 0)
    period = 1.0 / settings.control_frequency
    after = state[:, 3] - settings.deceleration * period
    v = np.where(ok, xt[rows, 1, 3], np.where(after < 0.0, 0.0, after))
    w = np.where(ok, ut[rows, 0, 1], 0.0)
    nxt = None
    if settings.plant:
        psi = state[:, 2]
        nxt = state.copy()
        nxt[:, 0] = state[:, 0] + (v * np.cos(psi)) * period
        nxt[:, 1] = state[:, 1] + (v * np.sin(psi)) * period
        nxt[:, 2] = psi + w * period
        nxt[:, 3] = v
        if closest_s is not None and spline_slot >= 0:
            nxt[:, spline_slot] = closest_s
    return dict(cmd=np.stack([v, w], 1), state_next=nxt)


# ------------------------------------------------------------------ the device loop


class PathLoop:
    """Consecutive control steps of scenes that track reference paths on one GPU: a `ControlLoop`
    whose contouring window and `spline` state entry are kept up on the device.

        step():     mpcg_path_update (closest point, window into the loop's stage_params, goal test)
                    -> ControlLoop.step -> mpcg_path_command (v, w; with settings.plant the next state)
        advance():  carries closest_segment / closest_s, writes closest_s into the `spline` entry of
                    the next state and, with the plant, takes that state from the command kernel

    Guidance trajectories and obstacle predictions still come from outside (`loop.set_scene_data`,
    or a `FleetLoop`'s launches around the same scenes), unless the loop has a guidance layer
    (loop_options guidance_layer=guidance.GuidanceLayer): the path update runs before the layer's
    update inside ControlLoop.step, because the layer's nominal needs this step's window.  With the
    layer, loop_options skip_disabled=True leaves the planners it disables unsolved.

    road=roads.RoadSettings: the loop's steps also write the two road-boundary halfspaces along the
    tracked paths (include/mpcg_road.h); the bounds mode takes its bound tables (P, M, 8) through
    `set_path`.  road=None: nothing is launched."""

    def __init__(self, layout, scenes, table: PathTable, path_of, device, settings: PathSettings, robot_radius: float,
                 w_consistency: float, selection_weight: float, spline_slot: int | None = None, road=None,
                 left_coef=None, right_coef=None, **loop_options):
        import torch

        from . import native
        from .control_loop import ControlLoop

        if len(path_of) != scenes.n_scenes:
            raise ValueError(f"path_of has {len(path_of)} entries for {scenes.n_scenes} scenes")
        loop_options.setdefault("deceleration", settings.deceleration)
        self.loop = ControlLoop(layout, scenes, device, robot_radius, w_consistency, selection_weight, road=road,
                                **loop_options)
        self.settings, self._set = settings, settings.native()
        self.spline_slot = layout.nx - 1 if spline_slot is None else spline_slot
        S = scenes.n_scenes
        self.closest_segment = torch.full((S,), -1, dtype=torch.int32, device=device)
        self.closest_s = torch.full((S,), float("nan"), dtype=torch.float64, device=device)
        self.reached = torch.zeros((S,), dtype=torch.uint8, device=device)
        self.cmd = torch.zeros((S, 2), dtype=torch.float64, device=device)
        self.state_next = torch.zeros((S, layout.nx), dtype=torch.float64, device=device)
        self._native = native
        self.set_path(table, path_of, left_coef, right_coef)

    def set_path(self, table: PathTable, path_of, left_coef=None, right_coef=None):
        """New paths (onDataReceived): every scene's closest_segment is reset to -1, so the next update
        searches its whole path.  left_coef / right_coef (P, M, 8): the bound splines over the paths' knots
        (roads.fit_bounds, roads.stack_bounds), read by a road in the bounds mode."""
        self.table = self._native.path_table_device(table, path_of, self.loop.dev)
        self.closest_segment.fill_(-1)
        if self.loop.road is not None:
            both = left_coef is not None and right_coef is not None
            self.loop.set_road_path(self.table, self._native.road_bounds_device(left_coef, right_coef, self.loop.dev)
                                    if both else None)

    def set_tracks(self, pose, twist, dims, shape, **options):
        """ControlLoop.set_tracks of the inner loop: the obstacle predictions from tracked objects."""
        self.loop.set_tracks(pose, twist, dims, shape, **options)

    def step(self, stream=None):
        """One control step of every scene.  Returns ControlLoop.step's dict plus closest_segment,
        closest_s, reached, cmd (S, 2) and, with the plant, state_next (S, nx)."""
        lp, nat = self.loop, self._native
        nat.path_update_device(lp.pr, self.table, lp.dsc["state"], self.closest_segment, self.closest_s,
                               lp.dsc["stage_params"], self.reached, stream=stream)
        out = lp.step(stream=stream)
        plant = self.settings.plant
        nat.path_command_device(lp.pr, lp.G, self._set, out["best"], out["xtraj"], out["utraj"], lp.dsc["state"],
                                self.cmd, closest_s=self.closest_s, spline_slot=self.spline_slot,
                                state_next=self.state_next if plant else None, stream=stream)
        return dict(out, closest_segment=self.closest_segment, closest_s=self.closest_s, reached=self.reached,
                    cmd=self.cmd, state_next=self.state_next if plant else None)

    def advance(self, state_next=None, stream=None):
        """Carry the loop into the next step.  With the plant, state_next defaults to the command
        kernel's; a given state_next (S, nx: x, y, psi, v from outside) gets this step's closest_s in
        its `spline` entry."""
        import torch

        if state_next is None:
            if not self.settings.plant:
                raise ValueError("PathLoop.advance: no state_next and the stand-in plant is off")
            sn = self.state_next.clone()
        else:
            sn = torch.as_tensor(state_next, dtype=torch.float64, device=self.loop.dev).clone().contiguous()
            if self.spline_slot >= 0:
                sn[:, self.spline_slot] = self.closest_s
        return self.loop.advance(sn, stream=stream)
