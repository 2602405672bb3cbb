"""Solve inputs with rotated ellipsoids and a non-zero disc offset (test helper, like
fleet_reference.py; no test functions).

Every batch the synthetic generators build has ego_disc_0_offset 0 and circular obstacles
(major = minor = 0, angle 0, chi 1): the offset, rotation and chi terms of the inequality
rows, their psi derivatives and the constraint Hessians' psi blocks are then multiplied by
zero.  perturb_geometry() rewrites those parameters the way the reference's probabilistic
mode fills them; CASES lists the batches test_geometry_inputs.py (oracle only: the inputs
have not degenerated) and test_gpu_geometry.py (GPU against the oracle) run.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

PERTURB_SEED = 5


def perturb_geometry(layout, params, seed, offset):
    """A copy of params [B, N, npar] with ego_disc_0_offset = offset on every stage and every
    ellipsoid row of a real obstacle (_r > 0) rewritten: per solve and obstacle
    psi = U(-pi, pi) + 0.05 k, major = 0.4 U(0.02, 0.15) sqrt(1 + k) (the growth of
    obstacles.propagate_uncertainty along the horizon), minor = major U(0.3, 0.8),
    chi = ExponentialQuantile(0.5, 0.95).  Dummies (_r == 0) keep 0, 0, 0, chi 1."""
    from oscar_mpc_planner_mr_modification_amd.obstacles import exponential_quantile

    p = np.array(params, float, copy=True)
    B, N, _ = p.shape
    ix = layout.idx
    assert ix("ego_disc_0_offset") >= 0
    p[:, :, ix("ego_disc_0_offset")] = offset
    rng = np.random.default_rng(seed)
    k = np.arange(N)[None, :]
    chi = exponential_quantile(0.5, 0.95)
    for j in range(layout.n_ell):
        f = {n: ix(f"ellipsoid_obst_{j}_{n}") for n in ("psi", "major", "minor", "chi", "r")}
        psi0 = rng.uniform(-math.pi, math.pi, size=(B, 1))
        sig = rng.uniform(0.02, 0.15, size=(B, 1))
        ratio = rng.uniform(0.3, 0.8, size=(B, 1))
        real = p[:, :, f["r"]] > 0.0
        major = 0.4 * sig * np.sqrt(1.0 + k)
        p[:, :, f["psi"]] = np.where(real, psi0 + 0.05 * k, 0.0)
        p[:, :, f["major"]] = np.where(real, major, 0.0)
        p[:, :, f["minor"]] = np.where(real, major * ratio, 0.0)
        p[:, :, f["chi"]] = np.where(real, chi, 1.0)
    return p


@dataclass(frozen=True)
class Case:
    name: str
    kind: str          # "tmpc" (make_batch), "shmpc" (make_shmpc_batch), "c3" (make_c3_batch)
    n_scenes: int
    n_guesses: int
    seed: int
    offset: float


# the batches of tests/test_gpu_parity.py (their seeds); JS: the seed is chosen so that the batch
# meets the conditions of test_geometry_inputs.py (figures in that module's docstring)
CASES = {c.name: c for c in (
    Case("C2", "tmpc", 8, 8, 20251212, 0.2),
    Case("C1", "tmpc", 8, 5, 777, -0.15),
    Case("C4", "tmpc", 4, 8, 4242, 0.2),
    Case("JS", "tmpc", 4, 5, 4242, 0.2),
    Case("C5", "shmpc", 12, 4, 20251212, 0.2),
    Case("C5N10", "shmpc", 8, 4, 31, 0.2),
    Case("C3", "c3", 48, 1, 20251212, 0.2),
)}
# rows that carry the perturbed terms: the ellipsoid rows, or the scenario / decomp rows (the offset)
ROWS = {"tmpc": "ell", "shmpc": "scen", "c3": "scen"}


def case_layout(case: Case):
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout, safe_horizon_layout
    if case.name == "C5N10":
        return safe_horizon_layout(N=10, n_constraints=4)
    return config_layout(case.name)


@functools.lru_cache(maxsize=None)
def case_inputs(name: str):
    """(layout, unperturbed batch, perturbed params); shared and never modified"""
    case = CASES[name]
    lay = case_layout(case)
    if case.kind == "tmpc":
        from oscar_mpc_planner_mr_modification_amd.synthetic import make_batch
        b = make_batch(lay, case.n_scenes, case.n_guesses, seed=case.seed)
    elif case.kind == "shmpc":
        from oscar_mpc_planner_mr_modification_amd.scenario import make_shmpc_batch
        b = make_shmpc_batch(lay, case.n_scenes, seed=case.seed)
    else:
        from oscar_mpc_planner_mr_modification_amd.bicycle import make_c3_batch
        b = make_c3_batch(lay, case.n_scenes, seed=case.seed)
    params = perturb_geometry(lay, b.params, PERTURB_SEED, case.offset)
    params.setflags(write=False)
    return lay, b, params


def _frozen(opts):
    return tuple(sorted(opts.items()))


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, literal, lam_key, opts):
    import oracle_py
    lay, b, params = case_inputs(name)
    lam_in = None if lam_key is None else carried_lam(name)
    r = oracle_py.Oracle(lay, literal=literal, **dict(opts)).solve_batch(params, b.warm, b.xinit, lam_in=lam_in,
                                                                         return_lam=True)
    for v in r.values():
        v.setflags(write=False)
    return r


def oracle_run(name, literal=False, carried=False, **opts):
    """The oracle (default or literal build) on the perturbed inputs of case `name`, computed once
    per process.  carried: lam_in = carried_lam(name)."""
    return _oracle_cached(name, bool(literal), "carried" if carried else None, _frozen(opts))


def carried_lam(name):
    """The default oracle's multipliers of the 10-iteration solve, zeroed for failed solves (the
    wrapper's rule: a failed solve resets the capsule)."""
    r = oracle_run(name)
    return np.where((r["status"] == 1)[:, None, None], r["lam"], 0.0)


@functools.lru_cache(maxsize=None)
def oracle_unperturbed(name):
    import oracle_py
    lay, b, _ = case_inputs(name)
    return oracle_py.Oracle(lay).solve_batch(b.params, b.warm, b.xinit)


def row_slice(lay, kind):
    """columns of the multiplier block [nx + nh] that belong to the perturbed rows (h order:
    linear, ellipsoid, scenario / decomp rows)"""
    lo = lay.nx + (lay.n_lin if ROWS[kind] == "ell" else lay.n_lin + lay.n_ell)
    return slice(lo, lo + (lay.n_ell if ROWS[kind] == "ell" else lay.n_scen))


def spread(a, b, mask):
    """largest |x|, |u| distance between two runs over the solves of `mask`"""
    if not mask.any():
        return 0.0
    return max(float(np.abs(a["xtraj"][mask] - b["xtraj"][mask]).max()),
               float(np.abs(a["utraj"][mask] - b["utraj"][mask]).max()))


# ---- the bars of the GPU comparisons (test_gpu_geometry.py, test_obstacles.py)
X_TOL = 1e-4          # north_star: states and inputs
POBJ_RTOL = 1e-6
LAM_RTOL = 1e-6       # test_multipliers_carried_between_solves
ROUNDING = 1e-9       # the project's own figure for rounding (test_c5_rounding_decided_copy)
MARGIN = 100.0        # the kernel's classical Riccati is a third arithmetic form beside the two oracle builds


def oracle_scatter(lay, params, warm, xinit, i, lam_in=None, K=16, **opts):
    """Oracle-side evidence on solve i: the default build on K copies whose warm start moved by at
    most one ulp per entry (copy 0 unmoved), as scripts/parity_full.py's perturbed_outcomes, plus
    the literal build.  Returns (whether those runs end with different exit codes or SQP iteration
    counts, their largest |x|, |u| distance to the unmoved run)."""
    import oracle_py
    rng = np.random.default_rng(1)
    W = np.repeat(warm[i:i + 1], K, 0).copy()
    st = rng.integers(-1, 2, size=W.shape)
    st[0] = 0
    W = np.where(st > 0, np.nextafter(W, np.inf), np.where(st < 0, np.nextafter(W, -np.inf), W))
    P, X = np.repeat(params[i:i + 1], K, 0), np.repeat(xinit[i:i + 1], K, 0)
    li = None if lam_in is None else np.repeat(lam_in[i:i + 1], K, 0)
    runs = [oracle_py.Oracle(lay, **opts).solve_batch(P, W, X, lam_in=li),
            oracle_py.Oracle(lay, literal=True, **opts).solve_batch(P[:1], W[:1], X[:1],
                                                                    lam_in=None if li is None else li[:1])]
    ex = np.concatenate([r["status"] for r in runs])
    it = np.concatenate([r["sqp_iter"] for r in runs])
    xt = np.concatenate([r["xtraj"] for r in runs])
    ut = np.concatenate([r["utraj"] for r in runs])
    scatter = max(float(np.abs(xt - xt[0]).max()), float(np.abs(ut - ut[0]).max()))
    return bool((ex != ex[0]).any() or (it != it[0]).any()), scatter


def compare_with_oracle(label, ref, lit, got, scatter, converged_only=False, check_lam=False):
    """GPU result `got` (solve_batch_device outputs as numpy arrays) against the default oracle
    build `ref`, with the literal build `lit` of the same batch giving the oracle's own spread:

      equal exit codes and SQP iteration counts on every solve;
      on the compared solves (successful on both sides; converged_only: the last QP converged on
      both sides) max|dx|, max|du| <= max(1e-9, 100 x spread) -- which is below the north-star
      1e-4 --, pobj within 1e-6 relative and, with check_lam, the multipliers within 1e-6 of
      their largest.

    A solve that parts is accepted only on oracle-side evidence that rounding decides it
    (scatter(i) = oracle_scatter of that solve): its one-ulp runs or the literal build end with
    another exit code or iteration count, or scatter so far that the solve's own bound
    max(1e-9, 100 x scatter) covers the distance (beyond 1e-4 only when the runs themselves
    scatter beyond 1e-4); at most one such solve per batch, found by that property and not by
    its index.  Returns the measured figures."""
    B = len(ref["status"])
    same = (got["exit"] == ref["status"]) & (got["info"][:, 0] == ref["sqp_iter"])
    if converged_only:
        # exit 4 after one iteration only comes from the res_eq > 1e-2 rule at the first linearisation point
        ok = (got["info"][:, 2] == 0) & (ref["qp_status"] == 0)
    else:
        ok = (got["exit"] == 1) & (ref["status"] == 1)
    assert ok.any(), f"{label}: nothing to compare"
    sp = spread(ref, lit, ok & (lit["status"] == ref["status"]))
    bound = max(ROUNDING, MARGIN * sp)
    assert bound <= X_TOL, f"{label}: the oracle builds are {sp:.2e} apart"
    dx = np.abs(got["xtraj"] - ref["xtraj"]).reshape(B, -1).max(1)
    du = np.abs(got["utraj"] - ref["utraj"]).reshape(B, -1).max(1)
    d = np.maximum(dx, du)
    rel = np.abs(got["pobj"] - ref["pobj"]) / np.maximum(1.0, np.abs(ref["pobj"]))
    dl = np.zeros(B)
    if "lam" in got and "lam" in ref:
        dl = np.abs(got["lam"] - ref["lam"]).reshape(B, -1).max(1) / max(1.0, np.abs(ref["lam"][ok]).max())
    fig = dict(solves=B, compared=int(ok.sum()), dx=float(dx[ok].max()), du=float(du[ok].max()),
               pobj_rel=float(rel[ok].max()), lam_rel=float(dl[ok].max()), spread=sp, bound=bound)
    print(f"{label}: {B} solves, compared {fig['compared']}, exit and sqp_iter agreement {same.mean():.3f}, "
          f"max|dx| {fig['dx']:.2e}, max|du| {fig['du']:.2e}, pobj rel {fig['pobj_rel']:.2e}, "
          f"lam rel {fig['lam_rel']:.2e}, oracle builds' spread {sp:.2e}, bound {bound:.2e}, "
          f"qp iters gpu {got['info'][:, 1].mean():.1f} oracle {ref['qp_iter'].mean():.1f}")
    other = ok & ((rel > POBJ_RTOL) | (dl > LAM_RTOL if check_lam else False))
    parted = ~same | (ok & (d > bound)) | other
    idx = np.flatnonzero(parted)
    what = (f"exits gpu {got['exit'][idx][:10]} oracle {ref['status'][idx][:10]}, sqp_iter gpu {got['info'][idx, 0][:10]} "
            f"oracle {ref['sqp_iter'][idx][:10]}, |dx| {dx[idx][:10]}, |du| {du[idx][:10]}, pobj rel {rel[idx][:10]}, "
            f"lam rel {dl[idx][:10]}, bound {bound:.2e}")
    assert len(idx) <= 1, f"{label}: solves {idx[:10]} part from the oracle: {what}"
    for i in idx:
        parts, sc = scatter(int(i))
        near = same[i] and not other[i] and d[i] <= max(ROUNDING, MARGIN * sc) and (d[i] <= X_TOL or sc > X_TOL)
        assert parts or near, (f"{label}: solve {i} parts from the oracle ({what}) and the oracle's own one-ulp runs "
                               f"do not (they scatter by {sc:.2e})")
        print(f"{label}: solve {i} accepted as rounding-decided (oracle runs part: {parts}, scatter {sc:.2e}): {what}")
    return fig
