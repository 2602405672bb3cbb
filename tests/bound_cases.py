"""Solve inputs whose box bounds bind (test helper, like geometry_cases.py; no test functions).

The kernel keeps a lower and an upper row per variable of a lane (slots 2j, 2j + 1 <-> variable
part + PARTS j; LaneRows::box_on: inputs on stages 0..N-1, states on 1..N-1), and that map differs
between the instance families (PARTS / NZ: 3 / 7 C1, C2, the N 10 shape; 2 / 7 C4, JS; 3 / 8 C5;
2 / 9 C3).  With the models' own bounds almost no box row binds on the generators' batches.  CASES
tightens the run-time bounds (mpcg_problem lbu / ubu / lbx / ubx, the lb= / ub= options of
problem_from_layout on both sides) on the batches of tests/test_gpu_parity.py, and the braking cases
rewrite the scene (start velocity and the warm start's velocity column raised, reference velocity
lowered) so that the lower acceleration and velocity bounds bind too.  The start state is no
bounded row: several cases start outside the tightened state bounds on purpose.

test_bound_inputs.py (oracle only: the inputs have not degenerated, every bound class binds) and
test_gpu_bounds.py (GPU against the oracle) run these cases.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from geometry_cases import (LAM_RTOL, MARGIN, POBJ_RTOL, ROUNDING, X_TOL,  # noqa: F401  (the bars, re-exported)
                            compare_with_oracle, oracle_scatter, spread)

ACTIVE = 1e-4     # a row binds when its gap is at most this: a classification threshold (two orders
                  # below the narrowest range used here; the IPM stops at a complementarity of
                  # about 1e-5, which leaves binding rows 1e-6 .. 1e-4 from their bound)
ACTIVE_TIGHT = 1e-6


@dataclass(frozen=True)
class Braking:
    """scene rewrite: xinit's velocity and the warm start's velocity column raised by dv, the
    reference velocity of every stage set to v_ref"""
    dv: float
    v_ref: float


@dataclass(frozen=True)
class Case:
    name: str
    family: str        # "PARTS/NZ" of the kernel instance
    kind: str          # "tmpc" (make_batch), "shmpc" (make_shmpc_batch), "c3" (make_c3_batch)
    layout: str        # config_layout name, or "C5N10" / "C3N10"
    n_scenes: int
    n_guesses: int
    seed: int
    bounds: tuple      # ((variable, lower or None, upper or None), ...) replacing the model's bounds
    braking: Braking | None = None


TIGHT = (("a", -0.8, 0.8), ("w", -0.4, 0.4), ("v", None, 2.0))
TIGHTER = (("a", -0.5, 0.5), ("w", -0.3, 0.3), ("v", None, 1.8))   # below the reference velocity 2.0
BRAKE = (("a", -0.4, 0.8), ("w", -0.4, 0.4), ("v", 0.9, 2.0))
TIGHT_C3 = (("a", -0.6, 0.6), ("w", -0.25, 0.25), ("delta", -0.3, 0.3))
BRAKE_C3 = (("a", -0.4, 0.6), ("w", -0.25, 0.25), ("delta", -0.3, 0.3), ("v", 0.9, 2.5))
BRAKING = Braking(0.7, 1.0)

# The batches of tests/test_gpu_parity.py (C1, C2, C4, both C5 shapes, C3 N 30) and of
# tests/geometry_cases.py (JS) with their seeds.  T10 has no parity batch of its own: the C1 batch's
# shape and seed.  C3N10: the parity batch's 16 scenes, seed 9.  The braking case of the 2 / 7
# family is C4's: JS's 20 and 40 solve batches keep 8 and 12 successful solves under braking, below
# the share test_bound_inputs.py asks for.
CASES = {c.name: c for c in (
    Case("C2", "3/7", "tmpc", "C2", 8, 8, 20251212, TIGHT),
    Case("C2brake", "3/7", "tmpc", "C2", 8, 8, 20251212, BRAKE, BRAKING),
    Case("C1", "3/7", "tmpc", "C1", 8, 5, 777, TIGHT),
    Case("C1brake", "3/7", "tmpc", "C1", 8, 5, 777, BRAKE, BRAKING),
    Case("T10", "3/7", "tmpc", "T10", 8, 5, 777, TIGHTER),
    Case("C4", "2/7", "tmpc", "C4", 4, 8, 4242, TIGHTER),
    Case("JS", "2/7", "tmpc", "JS", 4, 5, 4242, TIGHT),
    Case("C4brake", "2/7", "tmpc", "C4", 4, 8, 4242, BRAKE, BRAKING),
    Case("C5", "3/8", "shmpc", "C5", 12, 4, 20251212, TIGHT),
    Case("C5N10", "3/8", "shmpc", "C5N10", 8, 4, 31, TIGHT),
    Case("C5brake", "3/8", "shmpc", "C5", 12, 4, 20251212, BRAKE, BRAKING),
    Case("C3", "2/9", "c3", "C3", 48, 1, 20251212, TIGHT_C3 + (("v", None, 2.0),)),
    Case("C3N10", "2/9", "c3", "C3N10", 16, 1, 9, TIGHT_C3),
    Case("C3brake", "2/9", "c3", "C3", 48, 1, 20251212, BRAKE_C3, BRAKING),
)}
FAMILIES = ("3/7", "2/7", "3/8", "2/9")


def case_layout(case: Case):
    from oscar_mpc_planner_mr_modification_amd.layouts import ca_decomp_layout, config_layout, safe_horizon_layout
    if case.layout == "C5N10":
        return safe_horizon_layout(N=10, n_constraints=4)
    if case.layout == "C3N10":
        return ca_decomp_layout(N=10, max_constraints=4)
    return config_layout(case.layout)


def variables(lay):
    """the stage variables' names in z order (inputs, then states)"""
    return tuple(lay.inputs) + tuple(lay.states)


def case_bounds(case: Case, lay):
    names = variables(lay)
    lb, ub = list(lay.lb), list(lay.ub)
    for var, lo, hi in case.bounds:
        i = names.index(var)
        if lo is not None:
            lb[i] = lo
        if hi is not None:
            ub[i] = hi
    return tuple(lb), tuple(ub)


@functools.lru_cache(maxsize=None)
def case_inputs(name: str):
    """(layout, inputs with params / warm / xinit, lb, ub); shared and never modified"""
    case = CASES[name]
    lay = case_layout(case)
    if case.kind == "tmpc":
        from oscar_mpc_planner_mr_modification_amd.synthetic import make_batch
        b = make_batch(lay, case.n_scenes, case.n_guesses, seed=case.seed)
    elif case.kind == "shmpc":
        from oscar_mpc_planner_mr_modification_amd.scenario import make_shmpc_batch
        b = make_shmpc_batch(lay, case.n_scenes, n_solvers=case.n_guesses, seed=case.seed)
    else:
        from oscar_mpc_planner_mr_modification_amd.bicycle import make_c3_batch
        b = make_c3_batch(lay, case.n_scenes, seed=case.seed)
    params, warm, xinit = (np.array(a, float, copy=True) for a in (b.params, b.warm, b.xinit))
    if case.braking is not None:
        iv = list(lay.states).index("v")
        xinit[:, iv] += case.braking.dv
        warm[:, :, lay.nu + iv] += case.braking.dv
        params[:, :, lay.idx("reference_velocity")] = case.braking.v_ref
    for a in (params, warm, xinit):
        a.setflags(write=False)
    lb, ub = case_bounds(case, lay)
    return lay, SimpleNamespace(params=params, warm=warm, xinit=xinit), lb, ub


def _frozen(opts):
    return tuple(sorted(opts.items()))


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, literal, lam_key, opts):
    import oracle_py
    lay, b, lb, ub = case_inputs(name)
    lam_in = None if lam_key is None else carried_lam(name)
    r = oracle_py.Oracle(lay, literal=literal, lb=lb, ub=ub, **dict(opts)).solve_batch(
        b.params, b.warm, b.xinit, lam_in=lam_in, return_lam=True)
    for v in r.values():
        v.setflags(write=False)
    return r


def oracle_run(name, literal=False, carried=False, **opts):
    """The oracle (default or literal build) on the inputs and bounds of case `name`, computed once
    per process.  carried: lam_in = carried_lam(name)."""
    return _oracle_cached(name, bool(literal), "carried" if carried else None, _frozen(opts))


def carried_lam(name):
    """The default oracle's multipliers of the 10-iteration solve, zeroed for failed solves (the
    wrapper's rule: a failed solve resets the capsule)."""
    r = oracle_run(name)
    return np.where((r["status"] == 1)[:, None, None], r["lam"], 0.0)


QP_MEMORY = dict(qp_warm_start=2, qp_warm_first=1)


@functools.lru_cache(maxsize=None)
def oracle_qp_memory(name):
    """Two consecutive solves of case `name` with the QP memory carried (QP_MEMORY options), set up
    as test_qp_memory_carried_between_solves: `first` (both builds), then `second` from the default
    build's multipliers `lam` and QP memory `qp` (failed solves: zero multipliers, memory marked
    absent) in both builds, and `cold`: the second solve without the QP memory."""
    import oracle_py
    lay, b, lb, ub = case_inputs(name)
    orc = oracle_py.Oracle(lay, lb=lb, ub=ub, **QP_MEMORY)
    lit = oracle_py.Oracle(lay, literal=True, lb=lb, ub=ub, **QP_MEMORY)
    first = orc.solve_batch(b.params, b.warm, b.xinit, return_lam=True, return_qp=True)
    first_lit = lit.solve_batch(b.params, b.warm, b.xinit, return_lam=True)
    ok = first["status"] == 1
    lam = np.where(ok[:, None, None], first["lam"], 0.0)
    qp = first["qp"].copy()
    qp[~ok, 0] = np.nan
    run = lambda o, **kw: o.solve_batch(b.params, b.warm, b.xinit, lam_in=lam, return_lam=True, **kw)  # noqa: E731
    return dict(first=first, first_literal=first_lit, lam=lam, qp=qp, second=run(orc, qp_in=qp),
                second_literal=run(lit, qp_in=qp), cold=run(orc))


def scatter_of(name, lam_in=None, **opts):
    """oracle_scatter on the inputs and bounds of case `name`, as compare_with_oracle's `scatter`"""
    lay, b, lb, ub = case_inputs(name)
    return lambda i: oracle_scatter(lay, b.params, b.warm, b.xinit, i, lam_in=lam_in, lb=lb, ub=ub, **opts)


def active_rows(lay, lb, ub, result, mask, tol=ACTIVE, show=None):
    """Per bound class ("a lo", "a hi", ..., in z order) the number of solves of `mask` in which
    that bound binds in `result` (xtraj [B, N + 1, nx], utraj [B, N, nu]): a gap of at most `tol`
    on a bounded row -- input rows on stages 0..N-1, state rows on stages 1..N-1 (the start state
    and stage N carry none).  show: a label under which the counts at ACTIVE and at 1e-6 are printed."""
    N, nu = lay.N, lay.nu
    names = variables(lay)
    mask = np.asarray(mask, bool)
    out, tight = {}, {}
    for i, v in enumerate(names):
        val = result["utraj"][:, :N, i] if i < nu else result["xtraj"][:, 1:N, i - nu]
        for side, gap in (("lo", val - lb[i]), ("hi", ub[i] - val)):
            out[f"{v} {side}"] = int(((gap <= tol).any(1) & mask).sum())
            tight[f"{v} {side}"] = int(((gap <= ACTIVE_TIGHT).any(1) & mask).sum())
    if show is not None:
        fmt = lambda d: ", ".join(f"{k} {n}" for k, n in d.items() if n)  # noqa: E731
        print(f"{show}: binding in (of {int(mask.sum())} solves) at {tol:.0e}: {fmt(out) or 'none'}; "
              f"at {ACTIVE_TIGHT:.0e}: {fmt(tight) or 'none'}")
    return out
