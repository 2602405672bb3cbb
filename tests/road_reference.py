"""Plain-loop restatement of the road-boundary halfspaces (test helper, like fleet_reference.py; no
test functions): include/mpcg_road.h read line by line with Python floats, one rounding per
operation, for checking roads.road_halfspaces_host / roads.apply_road_host and, through them, the
kernel."""
import math

import numpy as np


def _segment(K, m, s):
    j = 0
    for k in range(1, m):
        if K[k] <= s:
            j += 1
    return j


def _point(c, t):
    c = [float(v) for v in c]
    return ((c[0] * t + c[1]) * t + c[2]) * t + c[3], ((c[4] * t + c[5]) * t + c[6]) * t + c[7]


def _orthogonal(c, t):
    c = [float(v) for v in c]
    dx = ((3.0 * c[0]) * t + 2.0 * c[1]) * t + c[2]
    dy = ((3.0 * c[4]) * t + 2.0 * c[5]) * t + c[6]
    ln = math.sqrt(dx * dx + dy * dy)
    return -dy / ln, dx / ln


def _dot_offset(nx, ny, px, py, off):
    qx = px + nx * off
    qy = py + ny * off
    return nx * qx + ny * qy


def braking_spline(state, N, dt, deceleration):
    """the `spline` entries of Solver::initializeWithBraking from one state (x y psi v s)"""
    v, s = float(state[3]), float(state[4])
    a = -abs(deceleration)
    out = [s]
    for _ in range(N):
        s = s + v * dt
        v = max(v + a * dt, 0.0)
        out.append(s)
    return out


def road_halfspaces_reference(width, two_way, radius, mode, coef, knots, n_segments, path_of, cur_s, left=None,
                              right=None):
    """(S, N, 2, 3): per scene and stage the rows (a1, a2, b), stage 0 zero.  coef (P, M, 8), knots
    (P, M + 1), n_segments (P,), cur_s (S, N + 1); mode "centerline" or "bounds" (left / right (P, M, 8))."""
    S, N = len(cur_s), len(cur_s[0]) - 1
    out = np.zeros((S, N, 2, 3))
    for sc in range(S):
        p = int(path_of[sc])
        m = int(n_segments[p])
        K = [float(v) for v in knots[p]]
        for k in range(1, N):
            s = float(cur_s[sc][k])
            if not s >= K[0]:       # before the path, or NaN
                s = K[0]
            if s > K[m]:
                s = K[m]
            j = _segment(K, m, s)
            t = s - K[j]
            if mode == "centerline":
                px, py = _point(coef[p][j], t)
                nx, ny = _orthogonal(coef[p][j], t)
                half = width / 2.0
                wl = (3.0 if two_way else 1.0) * half - radius
                wr = half - radius
                out[sc, k, 0] = (nx, ny, _dot_offset(nx, ny, px, py, wl))
                out[sc, k, 1] = (-nx, -ny, -_dot_offset(nx, ny, px, py, -wr))
            else:
                px, py = _point(left[p][j], t)
                nx, ny = _orthogonal(left[p][j], t)
                out[sc, k, 0] = (-nx, -ny, -_dot_offset(nx, ny, px, py, radius))
                px, py = _point(right[p][j], t)
                nx, ny = _orthogonal(right[p][j], t)
                out[sc, k, 1] = (nx, ny, _dot_offset(nx, ny, px, py, -radius))
    return out


def apply_road_reference(N, npar, i_lin0, max_obstacles, params, guided, halfspaces):
    """params (S*G, N, npar) with the rows placed: stages 1 .. N-1, rows max_obstacles, max_obstacles + 1
    of a guided planner, rows 0, 1 of a non-guided one"""
    out = np.array(params, float, copy=True)
    S, G = np.asarray(guided).shape
    for s in range(S):
        for g in range(G):
            first = max_obstacles if guided[s][g] else 0
            for k in range(1, N):
                for h in range(2):
                    for c in range(3):
                        out[s * G + g, k, i_lin0 + 3 * (first + h) + c] = halfspaces[s, k, h, c]
    return out
