"""Host restatement of the active-solve compaction (include/mpcg_active.h): solve only the enabled
solves of a batch.  With a guidance layer a planner whose index is at least the number of classes
found is disabled; the reference skips it before solve() (guidance_constraints.cpp:311-318).

    plan_host      mpcg_active_plan     enabled -> slot_of, solve_of, n_active (a stable compaction)
    gather_host    mpcg_active_gather   the inputs of the enabled solves -> a dense batch
    scatter_host   mpcg_active_scatter  the dense outputs -> the full batch, the fill for the others
    solve_active_host(solve_fn, ...)    the three around any full-batch solve function

Everything here copies or counts, so the device kernels agree with it bit for bit.  Importable
without a GPU.  Array dicts use the keys of native.solve_batch_device ("exit", "lam", "qp"); the
oracle's "status" is accepted for the exit code."""
from __future__ import annotations

import numpy as np

from .native_spec import ACTIVE_EXIT_SKIPPED, INFO_STRIDE

INPUT_KEYS = ("params", "warm", "xinit", "lam_in", "qp_in")
OUTPUT_KEYS = ("xtraj", "utraj", "pobj", "exit", "status", "info", "lam", "qp", "stats")


def plan_host(enabled) -> dict:
    """slot_of (B,) int32: the number of enabled solves before b, -1 for a disabled one; solve_of (B,)
    int32: solve_of[slot] = b ascending, -1 from n_active on; n_active int."""
    en = np.asarray(enabled).reshape(-1) != 0
    B = en.size
    slot_of = np.where(en, np.cumsum(en) - 1, -1).astype(np.int32)
    solve_of = np.full(B, -1, np.int32)
    n = int(en.sum())
    solve_of[slot_of[en]] = np.arange(B, dtype=np.int32)[en]
    return dict(slot_of=slot_of, solve_of=solve_of, n_active=n)


def gather_host(slot_of, full: dict, dense: dict | None = None) -> dict:
    """The blocks of every enabled solve b of full[k] (k in INPUT_KEYS, None entries skipped) at row
    slot_of[b] of dense[k].  dense None: fresh arrays of n_active rows; otherwise copies of the given
    arrays (rows that no solve maps to keep their content), keys missing or None in either are skipped."""
    slot_of = np.asarray(slot_of).reshape(-1)
    en = slot_of >= 0
    out = {}
    for k in INPUT_KEYS:
        a = full.get(k)
        if a is None or (dense is not None and dense.get(k) is None):
            continue
        a = np.asarray(a)
        d = np.zeros((int(en.sum()),) + a.shape[1:], a.dtype) if dense is None else np.array(dense[k])
        d[slot_of[en]] = a[en]
        out[k] = d
    return out


def fill_host(key: str, warm, nu: int, shape, dtype=None):
    """The fill of output `key` for every solve of the batch (include/mpcg_active.h): what a disabled
    solve holds after the scatter.  warm (B, N+1, nu+nx); shape: the output's full shape."""
    warm = np.asarray(warm)
    N = warm.shape[1] - 1
    if key == "xtraj":
        return np.array(warm[:, :, nu:])
    if key == "utraj":
        return np.array(warm[:, :N, :nu])
    if key == "pobj":
        return np.full(shape, np.inf)
    if key in ("exit", "status"):
        return np.full(shape, ACTIVE_EXIT_SKIPPED, dtype or np.int32)
    if key == "info":
        return np.zeros(shape, dtype or np.int32)
    if key == "lam":
        return np.zeros(shape)
    if key == "qp":
        q = np.zeros(shape)
        if q.size:
            q.reshape(shape[0], -1)[:, 0] = np.nan
        return q
    if key == "stats":
        return np.full(shape, np.nan)
    raise KeyError(f"no fill rule for output {key!r}")


def scatter_host(slot_of, dense: dict, warm, nu: int) -> dict:
    """Every output dense[k] (k in OUTPUT_KEYS, None skipped; n_active rows or more) back to the full batch:
    row b is dense[k][slot_of[b]] for an enabled solve and the fill for a disabled one."""
    slot_of = np.asarray(slot_of).reshape(-1)
    en = slot_of >= 0
    B = slot_of.size
    out = {}
    for k, d in dense.items():
        if d is None or k not in OUTPUT_KEYS:
            continue
        d = np.asarray(d)
        o = fill_host(k, warm, nu, (B,) + d.shape[1:], d.dtype if d.dtype.kind == "i" else None)
        o[en] = d[slot_of[en]]
        out[k] = o
    return out


def solve_active_host(solve_fn, params, warm, xinit, enabled, nu: int, lam_in=None, qp_in=None, outputs=None, **kw):
    """mpcg_solve_active around any full-batch solve function: solve_fn(params, warm, xinit, **kw) (plus
    lam_in= / qp_in= when given) on the dense batch of the enabled solves, its dict of outputs scattered
    back.  When no solve is enabled solve_fn is not called and `outputs` (key -> shape of one solve's
    block; default xtraj, utraj, pobj, exit and info, plus lam shaped like lam_in) names what to fill.
    Returns the outputs plus n_active and slot_of."""
    params, warm, xinit = np.asarray(params), np.asarray(warm), np.asarray(xinit)
    plan = plan_host(enabled)
    slot_of, n = plan["slot_of"], plan["n_active"]
    if slot_of.size != params.shape[0]:
        raise ValueError(f"{slot_of.size} flags for {params.shape[0]} solves")
    B = params.shape[0]
    if n > 0:
        d = gather_host(slot_of, dict(params=params, warm=warm, xinit=xinit, lam_in=lam_in, qp_in=qp_in))
        extra = {k: d[k] for k in ("lam_in", "qp_in") if k in d}
        r = solve_fn(d["params"], d["warm"], d["xinit"], **extra, **kw)
        out = scatter_host(slot_of, r, warm, nu)
    else:
        N, nx = warm.shape[1] - 1, warm.shape[2] - nu
        if outputs is None:
            outputs = dict(xtraj=(N + 1, nx), utraj=(N, nu), pobj=(), exit=(), info=(INFO_STRIDE,))
            if lam_in is not None:
                outputs["lam"] = np.asarray(lam_in).shape[1:]
        out = {k: fill_host(k, warm, nu, (B,) + tuple(s)) for k, s in outputs.items()}
    out["n_active"], out["slot_of"] = n, slot_of
    return out


__all__ = ["plan_host", "gather_host", "fill_host", "scatter_host", "solve_active_host", "ACTIVE_EXIT_SKIPPED"]
