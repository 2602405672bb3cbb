"""Decomp halfspaces: the static constraints of the rosnavigation configurations.

Every control step DecompConstraints::update (mpc_planner_modules/src/decomp_constraints.cpp:52-120) feeds
the occupied cells of the costmap to DecompUtil, dilates the reference path points predicted along the
horizon and writes the first decomp.max_constraints halfspaces of every segment's polyhedron into the
decomp rows of the next stage (the slack rows n_scen of the kernel; `layouts.ca_decomp_layout`, C3).

  path points   `decomp_path_points_host`: q_k = getPoint(s_k), s advanced by the predicted speed
  halfspaces    `decomp_halfspaces_host` here, decomp_halfspaces_kernel on the GPU: the ellipsoid
                free-space decomposition of every segment (`decomp_segment_host`); include/mpcg_decomp.h
                states the construction step by step and is the specification of both
  placement     `apply_decomp_host`: the rows of all N stages, every planner of a scene alike
  scenes        `make_c3_decomp_scenes`: the paths, states and warm starts of bicycle.make_c3_batch with
                occupied points as costmap cells and the path as a `paths.PathTable`

DecompUtil is not part of the reference tree: EllipsoidDecomp2D is restated from the published method (Liu
et al., RA-L 2017, safe flight corridors).  The frame's rotation is built from the segment's direction
where the library goes through atan2 / cos / sin.  Parity with the library is unpinned.

One rounding per operation, in the kernel's order (csrc/mpcg_decomp.h, compiled without contraction):
the host values are the device's bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .layouts import Layout
from .native_spec import DECOMP_EPS, DECOMP_MAX_N, DECOMP_MAX_POINTS, DECOMP_MAX_ROWS
from .paths import PathTable

RESOLUTION = 0.25       # costmap cell size of the synthetic scenes [m]


@dataclass
class DecompSettings:
    range: float = 2.0                    # settings.yaml decomp.range: the local bounding box (R, R)
    deceleration: float = 3.0             # deceleration_at_infeasible: the braking plan without a warm start

    def native(self):
        from .native_spec import MpcgDecompSettings
        return MpcgDecompSettings(float(self.range), float(self.deceleration))


def decomp_path_points_host(table: PathTable, path_of, state, main_warm, N: int, dt: float, nu: int,
                            deceleration: float = 3.0) -> np.ndarray:
    """q (S, N, 2): the path points q_k = getPoint(s_k), k = 0 .. N-1, with s_0 the `spline` entry of
    state (S, nx) (slot nx - 1) and s_{k+1} = s_k + v_k dt, v_k the `v` entry of stage k of main_warm
    (S, N+1, nu+nx), or of the braking plan from state when it is None."""
    state = np.asarray(state, np.float64)
    S, nx = state.shape
    dt = np.float64(dt)
    s = np.array(state[:, nx - 1])
    v = np.array(state[:, 3])
    a = np.float64(-abs(deceleration))
    cur = np.zeros((S, N))
    for k in range(N):
        cur[:, k] = s
        vk = v if main_warm is None else np.asarray(main_warm, np.float64)[:, k, nu + 3]
        s = s + vk * dt
        v = np.fmax(v + a * dt, 0.0)
    q = np.zeros((S, N, 2))
    for sc in range(S):
        p = int(path_of[sc])
        if not 0 <= p < len(table.n_segments):
            raise ValueError(f"decomp_path_points_host: path_of[{sc}] = {p} outside the table")
        m, K, coef = int(table.n_segments[p]), table.knots[p], table.coef[p]
        # s inside the path (a NaN goes to the start); the segment that holds it
        sk = np.fmin(np.fmax(cur[sc], K[0]), K[m])
        j = (K[None, 1:m] <= sk[:, None]).sum(1)
        t = sk - K[j]
        c = coef[j]
        q[sc, :, 0] = ((c[:, 0] * t + c[:, 1]) * t + c[:, 2]) * t + c[:, 3]
        q[sc, :, 1] = ((c[:, 4] * t + c[:, 5]) * t + c[:, 6]) * t + c[:, 7]
    return q


def _nan_to_inf(d):
    return np.where(np.isnan(d), np.inf, d)


def decomp_segment_host(q0, q1, points, R: float, max_constraints: int, dummy_b: float) -> dict:
    """The construction of include/mpcg_decomp.h (steps 3 - 8) for one segment q0 -> q1 and the occupied
    points (n, 2).  Returns dict(rows (max_constraints, 3), n_found: the hyperplanes found including the
    four box rows, minor_axis: the ellipsoid's b, kept (n,) bool: the points inside the bounding box)."""
    f8 = np.float64
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    ox, oy = pts[:, 0], pts[:, 1]
    q0x, q0y, q1x, q1y, R = f8(q0[0]), f8(q0[1]), f8(q1[0]), f8(q1[1]), f8(R)
    eps = f8(DECOMP_EPS)
    with np.errstate(all="ignore"):
        # ---- the frame
        dx, dy = q1x - q0x, q1y - q0y
        ln = np.sqrt(dx * dx + dy * dy)
        ex, ey = dx / ln, dy / ln
        hx, hy = ey, -ex
        gx, gy = -hx, -hy
        cx, cy = (q0x + q1x) / f8(2.0), (q0y + q1y) / f8(2.0)
        a = ln / f8(2.0)
        # the bounding box's four hyperplanes (p, n), in the order they are appended
        box = [(q0x + hx * R, q0y + hy * R, hx, hy), (q0x - hx * R, q0y - hy * R, -hx, -hy),
               (q1x + ex * R, q1y + ey * R, ex, ey), (q0x - ex * R, q0y - ey * R, -ex, -ey)]

        def side(nx, ny, x, y, px, py):
            return nx * (x - px) + ny * (y - py)

        def uw(x, y):
            ddx, ddy = x - cx, y - cy
            return ex * ddx + ey * ddy, gx * ddx + gy * ddy

        def dist(b, x, y):
            u, w = uw(x, y)
            ua, wb = u / a, w / b
            return np.sqrt(ua * ua + wb * wb)

        # ---- the box filter
        kept = np.ones(len(pts), bool)
        for px, py, nx, ny in box:
            kept &= side(nx, ny, ox, oy, px, py) <= eps
        idx = np.flatnonzero(kept)
        # ---- the ellipsoid: shrink b until no kept point lies inside
        b = a
        inside = idx[dist(b, ox[idx], oy[idx]) <= 1.0]
        for _ in range(len(inside)):
            if not len(inside):
                break
            win = inside[np.argmin(_nan_to_inf(dist(b, ox[inside], oy[inside])))]   # the first of equal minima
            us, ws = uw(ox[win], oy[win])
            if us < a:
                ua = us / a
                b = np.abs(ws) / np.sqrt(f8(1.0) - ua * ua)
            inside = inside[(f8(1.0) - dist(b, ox[inside], oy[inside])) > eps]
        # ---- the polyhedron
        dk = np.full(len(pts), np.inf)
        dk[idx] = _nan_to_inf(dist(b, ox[idx], oy[idx]))
        aa, bb = a * a, b * b
        planes, count, rm = [], 0, idx
        for _ in range(len(idx)):
            if not len(rm):
                break
            win = rm[np.argmin(dk[rm])]
            wx, wy = ox[win], oy[win]
            us, ws = uw(wx, wy)
            ca, cb = us / aa, ws / bb
            nx, ny = ex * ca + gx * cb, ey * ca + gy * cb
            nl = np.sqrt(nx * nx + ny * ny)
            nx, ny = nx / nl, ny / nl
            if count < max_constraints:
                planes.append((wx, wy, nx, ny))
            count += 1      # counted on past max_constraints: n_found is the full count
            rm = rm[side(nx, ny, ox[rm], oy[rm], wx, wy) < 0.0]
        # ---- rows
        rows = np.tile(np.array([1.0, 0.0, dummy_b]), (max_constraints, 1))
        for r, (px, py, nx, ny) in enumerate((planes + box)[:max_constraints]):
            rb = px * nx + py * ny
            a1, a2 = nx, ny
            if (nx * cx + ny * cy) - rb > 0.0:
                a1, a2, rb = -a1, -a2, -rb
            if np.isnan(a1) or np.isnan(a2) or np.isnan(rb) or np.sqrt(a1 * a1 + a2 * a2) < 1e-3:
                break       # this row and all after it stay dummies (decomp_constraints.cpp:98-101)
            rows[r] = (a1, a2, rb)
    return dict(rows=rows, n_found=count + 4, minor_axis=float(b), kept=kept)


def decomp_halfspaces_host(settings: DecompSettings, table: PathTable, path_of, state, main_warm, occ, n_occ,
                           N: int, dt: float, nu: int, max_constraints: int) -> dict:
    """The decomp halfspaces of every scene (NumPy; the restatement of decomp_halfspaces_kernel): state
    (S, nx), main_warm (S, N+1, nu+nx) or None, occ (S, P, 2) of which the first n_occ[s] points of scene s
    count.  Returns dict(rows (S, N, max_constraints, 3), n_found (S, N) int32, minor_axis (S, N),
    points (S, N, 2)); stage 0 holds the dummies, n_found 0 and minor_axis 0."""
    state = np.asarray(state, np.float64)
    occ = np.asarray(occ, np.float64)
    S = state.shape[0]
    if not 2 <= N <= DECOMP_MAX_N:
        raise ValueError(f"decomp_halfspaces_host: needs 2 <= N <= {DECOMP_MAX_N}")
    if not 1 <= max_constraints <= DECOMP_MAX_ROWS:
        raise ValueError(f"decomp_halfspaces_host: needs 1 <= max_constraints <= {DECOMP_MAX_ROWS}")
    if not settings.range > 0.0:
        raise ValueError("decomp_halfspaces_host: needs range > 0")
    if occ.shape[:1] != (S,) or occ.shape[2:] != (2,) or occ.shape[1] > DECOMP_MAX_POINTS:
        raise ValueError(f"decomp_halfspaces_host: occ must be (S, P <= {DECOMP_MAX_POINTS}, 2)")
    q = decomp_path_points_host(table, path_of, state, main_warm, N, dt, nu, settings.deceleration)
    rows = np.zeros((S, N, max_constraints, 3))
    n_found = np.zeros((S, N), np.int32)
    minor = np.zeros((S, N))
    for sc in range(S):
        n = int(n_occ[sc])
        if not 0 <= n <= occ.shape[1]:
            raise ValueError(f"decomp_halfspaces_host: n_occ[{sc}] = {n} outside 0 .. P")
        dummy_b = state[sc, 0] + 100.0
        rows[sc, 0] = (1.0, 0.0, dummy_b)
        for k in range(N - 1):
            r = decomp_segment_host(q[sc, k], q[sc, k + 1], occ[sc, :n], settings.range, max_constraints, dummy_b)
            rows[sc, k + 1], n_found[sc, k + 1], minor[sc, k + 1] = r["rows"], r["n_found"], r["minor_axis"]
    return dict(rows=rows, n_found=n_found, minor_axis=minor, points=q)


def apply_decomp_host(layout: Layout, params, n_guesses: int, rows) -> np.ndarray:
    """The placement of `decomp_halfspaces_host`'s rows (S, N, max_constraints, 3) into a copy of params
    (S*G, N, npar): the decomp block of all N stages, every planner of a scene alike; nothing else is touched."""
    rows = np.asarray(rows, np.float64)
    S, N, nd = rows.shape[0], layout.N, layout.n_scen
    if rows.shape != (S, N, nd, 3):
        raise ValueError(f"apply_decomp_host: rows {rows.shape} are not (S, {N}, {nd}, 3)")
    i0 = layout.index_struct()["i_scen0"]
    out = np.array(params, np.float64).reshape(S, n_guesses, N, layout.npar)
    out[:, :, :, i0:i0 + 3 * nd] = rows.reshape(S, 1, N, 3 * nd)
    return out.reshape(S * n_guesses, N, layout.npar)


# ------------------------------------------------------------------ seeded scenes


@dataclass
class C3DecompScenes:
    params: np.ndarray    # (S, N, npar): weights and spline window; the decomp rows all dummies
    warm: np.ndarray      # (S, N+1, 9) [a w slack | x y psi v delta s]: the main warm start
    xinit: np.ndarray     # (S, 6): the state
    table: PathTable      # one path per scene
    path_of: np.ndarray   # (S,) int32
    occ: np.ndarray       # (S, P, 2): occupied cell centres, NaN past n_occ
    n_occ: np.ndarray     # (S,) int32


def _rectangle_cells(centre, t, n, half_along, half_across):
    """centres of the costmap cells (RESOLUTION grid through the origin) inside a rectangle around `centre`
    with its sides along the unit vectors t and n, in row-major order of the grid"""
    reach = np.hypot(half_along, half_across)
    lo = np.floor((centre - reach) / RESOLUTION).astype(int)
    hi = np.ceil((centre + reach) / RESOLUTION).astype(int)
    ix, iy = np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1), indexing="ij")
    cells = (np.stack([ix.ravel(), iy.ravel()], 1) + 0.5) * RESOLUTION
    d = cells - centre
    return cells[(np.abs(d @ t) <= half_along) & (np.abs(d @ n) <= half_across)]


def make_c3_decomp_scenes(layout: Layout, n_scenes: int, seed: int, first_scene: int = 0) -> C3DecompScenes:
    """Seeded C3 scenes for the decomp layer: the path, state and warm start of scene i are those of
    bicycle.make_c3_batch at the same seed (the same draws in the same order); the path is also a table
    entry (the end knot 3 m after the last start, inside the last segment's own length), and the occupied
    points are costmap cells: the centres of a 0.25 m grid inside 3 - 12 rectangles placed along the next
    16 m of the path, most beside it (0.3 - 4 m along the path, the near edge 0.9 - 2.6 m off the centre line)
    and about one in four across it (long side across, ending 0.4 - 1 m from the centre line).  With decomp.range 2
    some rectangles fall outside a segment's box and some stages meet more hyperplanes than rows."""
    from .bicycle import C3_WEIGHTS, path_warm
    from .synthetic import _path, _path_eval

    N, dt, npar, ix = layout.N, layout.dt, layout.npar, layout.idx
    nd = layout.n_scen
    params = np.zeros((n_scenes, N, npar))
    warm = np.zeros((n_scenes, N + 1, 9))
    xinit = np.zeros((n_scenes, 6))
    i_dec = ix("disc_0_decomp_0_a1")
    tab, clouds = [], []
    for sc in range(n_scenes):
        rng = np.random.default_rng(seed + first_scene + sc)
        coef, starts = _path(rng, layout.n_seg)
        s_ego = rng.uniform(0.0, 1.0)
        p_on, t_on = _path_eval(coef, starts, s_ego)
        n_on = np.array([-t_on[1], t_on[0]])
        pos = p_on + rng.normal(0, 0.2) * n_on
        v0 = rng.uniform(0.0, 3.0)
        psi0 = np.arctan2(t_on[1], t_on[0]) + rng.normal(0.0, 0.05)
        x0 = np.array([pos[0], pos[1], psi0, v0, rng.uniform(-0.1, 0.1), s_ego])
        xinit[sc] = x0
        base = np.zeros(npar)
        for name, v in C3_WEIGHTS.items():
            base[ix(name)] = v
        for j in range(layout.n_seg):
            for ax, axn in enumerate("xy"):
                for ci, cn in enumerate("abcd"):
                    base[ix(f"spline_{axn}{j}_{cn}")] = coef[j, ax, ci]
            base[ix(f"spline{j}_start")] = starts[j]
        base[ix("ego_disc_0_offset")] = 0.0
        base[i_dec:i_dec + 3 * nd] = np.tile((1.0, 0.0, x0[0] + 100.0), nd)
        params[sc] = base[None, :]
        warm[sc] = path_warm(x0, coef, starts, N, dt)
        tab.append(dict(coef=coef.reshape(layout.n_seg, 8).copy(), knots=np.concatenate([starts, [starts[-1] + 3.0]])))
        # ---- occupied cells
        cells = []
        for _ in range(int(rng.integers(3, 13))):
            s_r = s_ego + rng.uniform(0.0, 16.0)
            pp, tp = _path_eval(coef, starts, s_r)
            nrm = np.array([-tp[1], tp[0]])
            sign = rng.choice([-1.0, 1.0])
            if rng.uniform() < 0.25:
                half_along, half_across = rng.uniform(0.15, 0.4), rng.uniform(0.75, 2.0)
                lat = half_across + rng.uniform(0.4, 1.0)
            else:
                half_along, half_across = rng.uniform(0.15, 2.0), rng.uniform(0.1, 0.75)
                lat = rng.uniform(0.9, 2.6) + half_across
            cells.append(_rectangle_cells(pp + sign * lat * nrm, tp, nrm, half_along, half_across))
        clouds.append(np.unique(np.concatenate(cells), axis=0)[:DECOMP_MAX_POINTS])
    P = max(1, max(len(c) for c in clouds))
    occ = np.full((n_scenes, P, 2), np.nan)
    for sc, c in enumerate(clouds):
        occ[sc, :len(c)] = c
    return C3DecompScenes(params=params, warm=warm, xinit=xinit, table=PathTable.from_paths(tab),
                          path_of=np.arange(n_scenes, dtype=np.int32), occ=occ,
                          n_occ=np.array([len(c) for c in clouds], np.int32))
