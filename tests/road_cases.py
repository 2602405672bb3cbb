"""Inputs shared by tests/test_road.py, tests/test_road_inputs.py and tests/test_gpu_road.py (test
helper; no test functions): the producer's kernel cases, the SQP parity batches with road rows, and
the closed-loop case with its CPU reference loop.

Parity batches: synthetic.make_batch scenes, each scene's path the 5-segment window of its stage
parameters as a table entry (the end knot 3 m after the last start, inside the last segment's own
length), the road rows from roads.road_halfspaces_host at the braking plan's `spline` entries (the
batch has no previous solution) placed by roads.apply_road_host.  tests/test_road_inputs.py shows on
the oracle alone that the rows bind in successful solves.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import path_cases as pc
from geometry_cases import MARGIN, ROUNDING, X_TOL, spread  # noqa: F401  (the bars, re-exported)
from oscar_mpc_planner_mr_modification_amd import paths, roads
from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
from oscar_mpc_planner_mr_modification_amd.synthetic import DECELERATION, ROBOT_RADIUS, make_batch, make_scenes

ACTIVE = 1e-4          # a road row binds when its gap b - a . p is at most this (bound_cases.ACTIVE)
MIN_SOLVES, MIN_ACTIVE = 16, 6


# ------------------------------------------------------------------ the producer's kernel cases

# (layout, mode, two_way, main_warm given): both modes, two_way on and off, the warm start given and
# NULL (the braking plan), N 20 and N 30
KERNEL_CASES = {
    "C2R-center-warm": ("C2R", "centerline", False, True),
    "C2R-center-twoway-braking": ("C2R", "centerline", True, False),
    "C2R-bounds-braking": ("C2R", "bounds", False, False),
    "JSR-bounds-warm": ("JSR", "bounds", False, True),
    "JSR-center-twoway-warm": ("JSR", "centerline", True, True),
    "JSR-center-braking": ("JSR", "centerline", False, False),
}


def offset_bounds(path: dict, left: float, right: float):
    """bound waypoints at the knots of a table entry: the centre point moved `left` to the left and
    `right` to the right along the normal"""
    pts = [pc.eval_path(path, s) for s in path["knots"]]
    return (np.array([p + left * n for p, _, n in pts]), np.array([p - right * n for p, _, n in pts]))


@functools.lru_cache(maxsize=None)
def kernel_case(name: str):
    """7 scenes x 8 planners over 3 paths of 3, 12 and 64 segments (the tables of pc.update_case).
    The stage 1 .. N-1 `spline` entries of the scenes: inside one segment; starting exactly on a knot;
    crossing several segments of the long path; in the last segment of the short path; running past
    its end; starting before the path's start; a NaN among ordinary values (given warm start only).
    Scene 5 has no guided planner, the others G - 1 guided ones and the non-guided last."""
    cfg, mode, two_way, given = KERNEL_CASES[name]
    lay = config_layout(cfg)
    N, dt, G = lay.N, lay.dt, 8
    tab = [pc.synthetic_path(11, 3), pc.synthetic_path(12, 12), pc.long_path(64)]
    table = paths.PathTable.from_paths(tab)
    K0, K1, K2 = (t["knots"] for t in tab)
    # (path, s at stage 0, speed): the braking plan advances s by v dt while v falls by 3 dt per stage
    rows = [(1, K1[4] + 0.3, 0.9), (1, K1[5], 1.6), (2, K2[30] + 0.2, 2.9), (0, K0[2] + 0.1, 1.2),
            (0, K0[3] - 0.4, 2.5), (1, K1[0] - 0.5, 2.0), (2, K2[62] + 0.1, 2.2)]
    S = len(rows)
    rng = np.random.default_rng(17)
    state = rng.normal(size=(S, 5))
    for s, (_, s0, v) in enumerate(rows):
        state[s, 3], state[s, 4] = v, s0
    main_warm = None
    if given:
        # a previous solution: constant speed along the path
        main_warm = rng.normal(size=(S, N + 1, 7))
        for s, (_, s0, v) in enumerate(rows):
            main_warm[s, :, 6] = s0 + v * dt * np.arange(N + 1)
        main_warm[6, 3, 6] = np.nan
        main_warm[1, 1, 6] = K1[6]            # exactly on a knot at a written stage
    guided = np.zeros((S, G), np.uint8)
    guided[:, :G - 1] = 1
    guided[5] = 0
    left = right = None
    if mode == "bounds":
        b = [roads.fit_bounds(t, *offset_bounds(t, 2.0 + 0.3 * i, 1.5 + 0.2 * i)) for i, t in enumerate(tab)]
        left, right = roads.stack_bounds(table, [x[0] for x in b]), roads.stack_bounds(table, [x[1] for x in b])
    road = roads.RoadSettings(width=3.2, two_way=two_way, robot_radius=ROBOT_RADIUS, mode=mode)
    params = rng.normal(size=(S * G, N, lay.npar))
    for a in (state, params, guided) + ((main_warm,) if given else ()):
        a.setflags(write=False)
    cur_s = roads.main_spline(state, main_warm, N, dt, DECELERATION)
    return SimpleNamespace(lay=lay, road=road, table=table, tab=tab, path_of=np.array([r[0] for r in rows], np.int32),
                           state=state, main_warm=main_warm, guided=guided, left=left, right=right, params=params,
                           cur_s=cur_s, S=S, G=G)


# ------------------------------------------------------------------ the SQP parity batches

# name: (layout, scenes, planners, seed, road width, two_way)
PARITY = {
    "C2R-W2.5-twoway": ("C2R", 8, 8, 7100, 2.5, True),
    "C2R-W1.6": ("C2R", 8, 8, 7100, 1.6, False),
    "C2R-W6.0": ("C2R", 8, 8, 7100, 6.0, False),
    "JSR-W2.5": ("JSR", 8, 5, 7200, 2.5, False),
}
NEEDS_ACTIVE = {n for n in PARITY if n != "C2R-W6.0"}     # the shipped width is kept although few rows bind


def window_table(lay, stage_params) -> paths.PathTable:
    """every scene's 5-segment window as a path of the table (the end knot 3 m after the last start)"""
    i0 = lay.idx("spline_x0_a")
    tab = []
    for sp in stage_params:
        win = sp[i0:i0 + 9 * lay.n_seg].reshape(lay.n_seg, 9)
        tab.append(dict(coef=win[:, :8].copy(), knots=np.concatenate([win[:, 8], [win[-1, 8] + 3.0]])))
    return paths.PathTable.from_paths(tab)


@functools.lru_cache(maxsize=None)
def parity_inputs(name: str):
    """(layout, inputs with params / warm / xinit, the road rows (S, N, 2, 3), guided (S, G)); shared,
    never modified"""
    cfg, S, G, seed, width, two_way = PARITY[name]
    lay = config_layout(cfg)
    b = make_batch(lay, S, G, seed=seed)
    sc = b.scenes
    road = roads.RoadSettings(width=width, two_way=two_way, robot_radius=ROBOT_RADIUS)
    table = window_table(lay, sc.stage_params)
    hs = roads.road_halfspaces_host(road, table, np.arange(S), roads.main_spline(sc.state, None, lay.N, lay.dt,
                                                                                DECELERATION))
    params = roads.apply_road_host(lay, b.params, sc.guided, hs)
    warm, xinit = np.array(b.warm), np.array(b.xinit)
    for a in (params, warm, xinit, hs):
        a.setflags(write=False)
    return lay, SimpleNamespace(params=params, warm=warm, xinit=xinit), hs, sc.guided.copy()


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, literal, opts):
    import oracle_py
    lay, b, _, _ = parity_inputs(name)
    r = oracle_py.Oracle(lay, literal=literal, **dict(opts)).solve_batch(b.params, b.warm, b.xinit, return_lam=True)
    for v in r.values():
        v.setflags(write=False)
    return r


def oracle_run(name, literal=False, **opts):
    """the oracle (default or literal build) on parity batch `name`, computed once per process"""
    return _oracle_cached(name, bool(literal), tuple(sorted(opts.items())))


def lam_spread(a, b, mask):
    """largest distance of the multipliers of two runs over the solves of `mask`, relative to the largest
    multiplier of the first (the scale geometry_cases.compare_with_oracle measures multipliers on)"""
    if not mask.any():
        return 0.0
    return float(np.abs(a["lam"][mask] - b["lam"][mask]).max() / max(1.0, np.abs(a["lam"][mask]).max()))


def road_gaps(name, xtraj):
    """(B, N - 1, 2): the gaps b - a . (x, y) of both road rows on the stages 1 .. N-1 of every solve"""
    lay, _, hs, guided = parity_inputs(name)
    S, G = guided.shape
    rows = np.repeat(hs[:, None], G, 1).reshape(S * G, lay.N, 2, 3)[:, 1:]
    p = xtraj[:, 1:lay.N, 0:2]
    return rows[..., 2] - (rows[..., 0] * p[:, :, None, 0] + rows[..., 1] * p[:, :, None, 1])


def active_solves(name, result, mask):
    """the solves of `mask` in which a road row binds (gap <= ACTIVE on some stage)"""
    return (road_gaps(name, result["xtraj"]) <= ACTIVE).any((1, 2)) & np.asarray(mask, bool)


# ------------------------------------------------------------------ the closed loop

LOOP = dict(cfg="C2R", S=4, G=8, seed=2024, width=2.5, two_way=True, steps=3)


@functools.lru_cache(maxsize=None)
def loop_case():
    """pc.loop_case's construction on the C2R layout with the stand-in plant: 4 scenes x 8 planners, a
    path table fitted through waypoints on each scene's synthetic path."""
    from oscar_mpc_planner_mr_modification_amd.synthetic import _path_eval
    lay = config_layout(LOOP["cfg"])
    S, G = LOOP["S"], LOOP["G"]
    sc = make_scenes(lay, S, G, seed=LOOP["seed"])
    i0 = lay.idx("spline_x0_a")
    tab, fast = [], []
    for s in range(S):
        win = sc.stage_params[s, i0:i0 + 9 * lay.n_seg].reshape(lay.n_seg, 9)
        coef, starts = win[:, :8].reshape(lay.n_seg, 2, 4), win[:, 8].copy()
        s_ego, total = sc.state[s, pc.SPLINE_SLOT], starts[-1] + 3.0
        fast.append(bool(sc.state[s, 3] >= 1.0))
        first = s_ego + (pc.KNOT_AHEAD if fast[-1] else 0.5 * pc.SPACING)
        ws = np.concatenate([[0.0], np.arange(first, total - 0.5, pc.SPACING), [total]])
        pts = _path_eval(coef, starts, ws)[0]
        tab.append(paths.fit_path(pts[:, 0], pts[:, 1]))
    settings = paths.PathSettings(control_frequency=1.0 / lay.dt, deceleration=DECELERATION, plant=True)
    road = roads.RoadSettings(width=LOOP["width"], two_way=LOOP["two_way"], robot_radius=ROBOT_RADIUS)
    return dict(lay=lay, scenes=sc, table=paths.PathTable.from_paths(tab), path_of=np.arange(S, dtype=np.int32),
                fast=np.array(fast), settings=settings, S=S, G=G, road=road)


class _RoadProducers:
    """the loop-form producers with the host road producer behind prepare()"""

    def __init__(self, prod, case, record):
        self.prod, self.case, self.record = prod, case, record

    def prepare(self, lay, sc, *a, **kw):
        c = self.case
        p = self.prod.prepare(lay, sc, *a, **kw)
        hs = roads.road_halfspaces_host(c["road"], c["table"], c["path_of"],
                                        roads.main_spline(sc.state, sc.main_warm, lay.N, lay.dt, DECELERATION))
        p = dict(p)
        p["params"] = roads.apply_road_host(lay, p["params"], sc.guided, hs)
        self.record["halfspaces"] = hs
        return p


class RoadCpuLoop(pc.PathCpuLoop):
    """pc.PathCpuLoop (the oracle solve around paths.path_update_host) with the road rows written into
    the prepared parameters before every solve"""

    def __init__(self, case, sc, oracle_mod, prod_oracle, literal=False):
        self.road_record = {}
        super().__init__(case, sc, oracle_mod, _RoadProducers(prod_oracle, case, self.road_record))
        if literal:
            self.orc = oracle_mod.Oracle(case["lay"], literal=True)

    def step(self):
        h = super().step()
        return dict(h, halfspaces=self.road_record["halfspaces"], utraj=self.r["utraj"], lam=self.r["lam"])
