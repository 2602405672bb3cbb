"""Road-boundary halfspaces of the T-MPC path: the one kind of static constraint the reference has.

Every control step Contouring::update builds two halfspaces per stage (constructRoadConstraints,
contouring.cpp:48-49, 183-264) and LinearizedConstraints::update / setParameters append them to every
planner's lin_constraint rows (linearized_constraints.cpp:107-124, 173-187) of a solver generated with
n_lin = max_obstacles + add_halfspaces, add_halfspaces = 2 (guidance_constraints.py:37-41, 67-71;
`layouts.tmpc_layout(add_halfspaces=2)`, the built-in shapes C2R and JSR).

  halfspaces   `road_halfspaces_host` here, road_halfspaces_kernel on the GPU (include/mpcg_road.h has
               the formulas): per scene and stage k = 1 .. N-1, at cur_s(k) = the `spline` entry of
               stage k of the main solver's warm start (the braking plan without one)
  placement    `apply_road_host`: rows max_obstacles, max_obstacles + 1 of a guided planner, rows 0, 1
               of the non-guided one (its update runs on empty data, guidance_constraints.cpp:328,
               349); stage 0 and every other row stay as `producers.prepare_host` left them

ros_tools is not part of the reference tree.  Two points are therefore unpinned: the sign of
getOrthogonal -- here n = (-dy, dx) / |(dx, dy)|, left of the direction of travel, which the
reference's own comment at contouring.cpp:229 and its "LEFT HALFSPACE" wording support -- and getPoint
past the path's end, here the end point (cur_s clamped to the path).

One rounding per operation, in the kernel's order (csrc/mpcg_road.h, compiled without contraction):
the host values are the device's bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .layouts import Layout
from .paths import PathTable
from .producers import braking

ROAD_CENTERLINE, ROAD_BOUNDS = 0, 1
ROAD_MODES = {"centerline": ROAD_CENTERLINE, "bounds": ROAD_BOUNDS}
ROAD_MAX_N = 32


@dataclass
class RoadSettings:
    width: float = 6.0                    # settings.yaml road.width
    two_way: bool = False                 # contouring two_way_road: the left row at 3 W / 2
    robot_radius: float = 0.325           # robot_area[0].radius
    mode: str = "centerline"              # "bounds": the rows come from the left / right bound splines

    def __post_init__(self):
        if self.mode not in ROAD_MODES:
            raise ValueError(f"RoadSettings: mode {self.mode!r} is none of {sorted(ROAD_MODES)}")

    def native(self):
        from .native_spec import MpcgRoadSettings
        return MpcgRoadSettings(float(self.width), float(self.robot_radius), int(bool(self.two_way)),
                                ROAD_MODES[self.mode])


def fit_bounds(center: dict, left_xy, right_xy) -> tuple[np.ndarray, np.ndarray]:
    """The left and right bound splines over the centre path's knots (Contouring::onDataReceived fits
    _bound_left / _bound_right over the centre line's parameter): waypoints (m + 1, 2) each, one per
    knot of `center` (paths.fit_path).  Returns the two coefficient blocks (m, 8)."""
    from .paths import fit_path

    s = center["knots"]
    out = []
    for xy in (left_xy, right_xy):
        xy = np.asarray(xy, np.float64)
        if xy.shape != (len(s), 2):
            raise ValueError("fit_bounds: needs one bound waypoint per knot of the centre path")
        out.append(fit_path(xy[:, 0], xy[:, 1], s)["coef"])
    return out[0], out[1]


def stack_bounds(table: PathTable, bounds) -> np.ndarray:
    """Coefficient blocks (m_p, 8) of P paths -> (P, M, 8) in the layout of `table.coef`."""
    out = np.zeros_like(table.coef)
    for p, c in enumerate(bounds):
        m = int(table.n_segments[p])
        out[p, :m] = np.asarray(c, np.float64).reshape(m, 8)
    return out


def _point(c, t):
    return (((c[..., 0] * t + c[..., 1]) * t + c[..., 2]) * t + c[..., 3],
            ((c[..., 4] * t + c[..., 5]) * t + c[..., 6]) * t + c[..., 7])


def _normal(c, t):
    dx = ((3.0 * c[..., 0]) * t + 2.0 * c[..., 1]) * t + c[..., 2]
    dy = ((3.0 * c[..., 4]) * t + 2.0 * c[..., 5]) * t + c[..., 6]
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(dx * dx + dy * dy)
        return -dy / ln, dx / ln


def _offset_dot(nx, ny, px, py, off):
    qx, qy = px + nx * off, py + ny * off
    return nx * qx + ny * qy


def main_spline(state, main_warm, N: int, dt: float, deceleration: float = 3.0) -> np.ndarray:
    """cur_s (S, N+1): the `spline` entries of the main solver's warm start as mpcg_prepare sees it
    (main_warm (S, N+1, 7), or the braking plan from state (S, 5) when it is None)."""
    if main_warm is not None:
        return np.array(np.asarray(main_warm, np.float64)[:, :, 6])
    return braking(np.asarray(state, np.float64), N, dt, deceleration)[:, :, 6]


def road_halfspaces_host(road: RoadSettings, table: PathTable, path_of, cur_s, left_coef=None,
                         right_coef=None) -> np.ndarray:
    """The road halfspaces of every scene (NumPy; the restatement of road_halfspaces_kernel): cur_s
    (S, N+1) from `main_spline`, path_of (S,), the bound tables (P, M, 8) in the bounds mode.
    Returns (S, N, 2, 3): (a1, a2, b) of row 0 and row 1 per stage, stage 0 zero."""
    cur_s = np.asarray(cur_s, np.float64)
    S, N = cur_s.shape[0], cur_s.shape[1] - 1
    if not 2 <= N <= ROAD_MAX_N:
        raise ValueError(f"road_halfspaces_host: needs 2 <= N <= {ROAD_MAX_N}")
    bounds = ROAD_MODES[road.mode] == ROAD_BOUNDS
    if bounds and (left_coef is None or right_coef is None):
        raise ValueError("road_halfspaces_host: the bounds mode needs the left and right bound tables")
    out = np.zeros((S, N, 2, 3))
    r = float(road.robot_radius)
    half = float(road.width) / 2.0
    wl = (3.0 if road.two_way else 1.0) * half - r
    wr = half - r
    for sc in range(S):
        p = int(path_of[sc])
        if not 0 <= p < len(table.n_segments):
            raise ValueError(f"road_halfspaces_host: path_of[{sc}] = {p} outside the table")
        m, K = int(table.n_segments[p]), table.knots[p]
        # s inside the path (a NaN goes to the start); the segment that holds it
        s = np.fmin(np.fmax(cur_s[sc, 1:N], K[0]), K[m])
        j = (K[None, 1:m] <= s[:, None]).sum(1)
        t = s - K[j]
        o = out[sc, 1:N]
        if not bounds:
            c = table.coef[p][j]
            px, py = _point(c, t)
            nx, ny = _normal(c, t)
            o[:, 0, 0], o[:, 0, 1], o[:, 0, 2] = nx, ny, _offset_dot(nx, ny, px, py, wl)
            o[:, 1, 0], o[:, 1, 1], o[:, 1, 2] = -nx, -ny, -_offset_dot(nx, ny, px, py, -wr)
        else:
            c = np.asarray(left_coef, np.float64)[p][j]
            px, py = _point(c, t)
            nx, ny = _normal(c, t)
            o[:, 0, 0], o[:, 0, 1], o[:, 0, 2] = -nx, -ny, -_offset_dot(nx, ny, px, py, r)
            c = np.asarray(right_coef, np.float64)[p][j]
            px, py = _point(c, t)
            nx, ny = _normal(c, t)
            o[:, 1, 0], o[:, 1, 1], o[:, 1, 2] = nx, ny, _offset_dot(nx, ny, px, py, -r)
    return out


def apply_road_host(layout: Layout, params, guided, halfspaces) -> np.ndarray:
    """The placement of `road_halfspaces_host`'s rows (S, N, 2, 3) into a copy of params (S*G, N, npar):
    stages 1 .. N-1, rows max_obstacles, max_obstacles + 1 of the guided planners (guided (S, G)) and
    rows 0, 1 of the others; nothing else is touched."""
    mo = layout.max_obstacles
    if layout.n_lin < mo + 2:
        raise ValueError(f"apply_road_host: n_lin {layout.n_lin} < max_obstacles + 2 = {mo + 2}: the solver was "
                         "generated without add_halfspaces 2")
    guided = np.asarray(guided, bool)
    S, G = guided.shape
    N = layout.N
    out = np.array(params, np.float64).reshape(S, G, N, layout.npar)
    hs = np.asarray(halfspaces, np.float64).reshape(S, N, 6)
    l0 = layout.idx("lin_constraint_0_a1")
    for s in range(S):
        for g in range(G):
            at = l0 + 3 * (mo if guided[s, g] else 0)
            out[s, g, 1:, at:at + 6] = hs[s, 1:]
    return out.reshape(S * G, N, layout.npar)
