"""Guidance of the control loop, device-resident across control steps.

What surrounds the solves of GuidanceConstraints (mpc_planner_modules/src/guidance_constraints.cpp) on
the guidance side, once per control step and scene:

  generator         a stand-in for the *output* of the external guidance_planner (its space-time
                    visibility PRM is not part of the reference tree; parity unpinned): up to 8
                    collision-free, kinematically reachable trajectories that pass the relevant
                    obstacles on requested sides, reduced to distinct classes with persistent ids
                    -- the idea of synthetic._guess_trajectory as a per-step producer
  mapping           mapGuidanceTrajectoriesToPlanners (:208-257) -> existing_guidance
  enabling          a planner whose index is at least the number of classes found is disabled (:311-318)
  flags             previously_selected (:418) and shouldEnableConsistencyForPlanner (:951-984), keyed
                    to the topology class selected last step (_prev_selected_topology_id)
  selection record  :436-437, :538-539 and each planner's result.guidance_ID (:379, :399)

C ABI, the generator's rules and constants: include/mpcg_guidance.h.  `guidance_update_host`,
`map_planners_host` and `select_host` restate the kernels of csrc/mpcg_guidance.h in the same
operation order with one rounding per operation (Python floats): everything agrees bit for bit once
the restatement is given the ego heading (cos psi, sin psi) the kernel took.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .native_spec import (GUIDANCE_ACCEL, GUIDANCE_BITS, GUIDANCE_CANDIDATES, GUIDANCE_CLEARANCE,
                          GUIDANCE_EXIT_DISABLED, GUIDANCE_FINE, GUIDANCE_MAX_ELL, GUIDANCE_MAX_N, GUIDANCE_MAX_SEG,
                          GUIDANCE_OFFSET, GUIDANCE_ONSET, GUIDANCE_PUSH_MARGIN, GUIDANCE_RELEVANT, GUIDANCE_SWEEPS,
                          GUIDANCE_V_FLOOR, GUIDANCE_WIDTH)

INF = float("inf")
FINE = GUIDANCE_FINE


@dataclass
class GuidanceSettings:
    robot_radius: float = 0.325
    v_ref: float = 2.0
    consistency_on_non_guided: bool = True

    def native(self):
        from .native_spec import MpcgGuidanceSettings
        return MpcgGuidanceSettings(self.robot_radius, self.v_ref, int(self.consistency_on_non_guided))


def initial_state(S: int, G: int, N: int) -> dict:
    """The layer's per-scene state before the first step (include/mpcg_guidance.h, mpcg_guidance_state)."""
    K = 2 * (G - 1)
    return dict(class_traj=np.zeros((S, K, N + 1, 2)), class_used=np.zeros((S, K), np.uint8),
                planner_class=np.full((S, G), -1, np.int32), selected_topology=np.full(S, -1, np.int32),
                prev_was_original=np.zeros(S, np.uint8))


# ------------------------------------------------------------------ scalar helpers (C semantics)


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a >= b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a <= b else b


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else float("nan")


def _obs_at(ox, oy, i, N):
    """obstacle position at fine index i (time i h): linear between rows k and k + 1, k = min(i / FINE, N - 2)"""
    k = min(i // FINE, N - 2)
    f = float(i - FINE * k) / float(FINE)
    return ox[k] + (ox[k + 1] - ox[k]) * f, oy[k] + (oy[k + 1] - oy[k]) * f


def _side_bits(px, py, N, obs, real, mask):
    """The side word of a trajectory (positions at k dt, k = 0 .. N) against the obstacles of `mask`:
    bit j set when cross(p_{k+1} - p_k, obstacle_j - p_k) > 0 at the stage k of the trajectory's own
    closest approach to obstacle j."""
    side = 0
    for j in range(len(obs)):
        if not (mask >> j) & 1:
            continue
        ox, oy = obs[j]
        bd, bk, bx, by = INF, 0, 0.0, 0.0
        for k in range(N + 1):
            qx, qy = _obs_at(ox, oy, FINE * k, N)
            dx, dy = qx - px[k], qy - py[k]
            d2 = dx * dx + dy * dy
            if d2 != d2:
                d2 = INF
            if d2 < bd or k == 0:
                bd, bk, bx, by = d2, k, dx, dy
        k0 = bk if bk < N else N - 1
        tx, ty = px[k0 + 1] - px[k0], py[k0 + 1] - py[k0]
        if tx * by - ty * bx > 0.0:
            side |= 1 << j
    return side


def _scene_update(state, window, obst, radius, N, dt, G, settings, heading, class_traj, class_used):
    """One scene of mpcg_guidance_update up to the class ids (steps 1-6 of include/mpcg_guidance.h)."""
    n_seg, ne = len(window), len(radius)
    h = dt / float(FINE)
    NF = FINE * N + 1
    x0, y0, v0, s0 = float(state[0]), float(state[1]), float(state[3]), float(state[4])
    c0, s0h = float(heading[0]), float(heading[1])
    rr = float(settings.robot_radius)
    # ---- 1 nominal
    vmax = _fmax(float(settings.v_ref), v0)
    vt = [_fmin(v0 + GUIDANCE_ACCEL * (float(i) * h), vmax) for i in range(NF)]
    sn = [s0] * NF
    for i in range(1, NF):
        sn[i] = sn[i - 1] + (0.5 * (vt[i] + vt[i - 1])) * h
    W = [[float(v) for v in row] for row in window]
    nomx, nomy, nrx, nry = [0.0] * NF, [0.0] * NF, [0.0] * NF, [0.0] * NF
    for i in range(NF):
        s = sn[i]
        j = 0
        for k in range(1, n_seg):
            j += 1 if W[k][8] <= s else 0
        w = W[j]
        t = s - w[8]
        nomx[i] = ((w[0] * t + w[1]) * t + w[2]) * t + w[3]
        nomy[i] = ((w[4] * t + w[5]) * t + w[6]) * t + w[7]
        dx = ((3.0 * w[0]) * t + 2.0 * w[1]) * t + w[2]
        dy = ((3.0 * w[4]) * t + 2.0 * w[5]) * t + w[6]
        nr = _sqrt(dx * dx + dy * dy)
        if nr > 1e-12:
            tx, ty = dx / nr, dy / nr
        else:
            tx, ty = c0, s0h
        nrx[i], nry[i] = -ty, tx
    # ---- 2 relevant obstacles
    obs = [([float(v) for v in obst[j, :, 0]], [float(v) for v in obst[j, :, 1]]) for j in range(ne)]
    real = [float(radius[j]) > 0.0 for j in range(ne)]
    R = [rr + float(radius[j]) for j in range(ne)]
    rel, ic, lat, cdist = [False] * ne, [0] * ne, [0.0] * ne, [INF] * ne
    for j in range(ne):
        ox, oy = obs[j]
        bd, bi = INF, 0
        for i in range(NF):
            qx, qy = _obs_at(ox, oy, i, N)
            dx, dy = nomx[i] - qx, nomy[i] - qy
            d2 = dx * dx + dy * dy
            if d2 != d2:
                d2 = INF
            if d2 < bd:
                bd, bi = d2, i
        qx, qy = _obs_at(ox, oy, bi, N)
        cdist[j] = _sqrt(bd)
        rel[j] = real[j] and cdist[j] < GUIDANCE_RELEVANT
        ic[j] = bi
        lat[j] = (qx - nomx[bi]) * nrx[bi] + (qy - nomy[bi]) * nry[bi]
    rank = [sum(1 for q in range(ne) if rel[q] and (ic[q] < ic[j] or (ic[q] == ic[j] and q < j))) for j in range(ne)]
    mask = 0
    for j in range(ne):
        if rel[j]:
            mask |= 1 << j
    # ---- 3, 4 candidates
    C = GUIDANCE_CANDIDATES
    pos = np.zeros((C, N + 1, 2))
    vel = np.zeros((C, N + 1, 2))
    clearance, cost, side = [INF] * C, [0.0] * C, [0] * C
    requested = [0] * C
    heading_end = np.zeros((C, 2))
    for c in range(C):
        want = [0.0] * ne
        use = [False] * ne
        for j in range(ne):
            if not rel[j]:
                continue
            left = ((c >> rank[j]) & 1) == 1 if rank[j] < GUIDANCE_BITS else lat[j] >= 0.0
            if left:
                requested[c] |= 1 << j
                want[j] = lat[j] - GUIDANCE_OFFSET
                use[j] = not want[j] > 0.0
            else:
                want[j] = lat[j] + GUIDANCE_OFFSET
                use[j] = not want[j] < 0.0
        desx, desy = [0.0] * NF, [0.0] * NF
        for i in range(NF):
            t = float(i) * h
            off = 0.0
            for j in range(ne):
                if not use[j]:
                    continue
                u = (t - float(ic[j]) * h) / GUIDANCE_WIDTH
                q = 1.0 + u * u
                off = off + (want[j] * (1.0 / (q * q))) * (t / (t + GUIDANCE_ONSET))
            px = ((nomx[i] + off * nrx[i]) - nomx[0]) + x0
            py = ((nomy[i] + off * nry[i]) - nomy[0]) + y0
            # push-out sweeps, a fixed number: from the obstacle that violates its distance most
            for _ in range(GUIDANCE_SWEEPS):
                for back in (1, 0):
                    io = max(i - FINE * back, 0)
                    bg, bdist, bqx, bqy, bdx, bdy, bR = INF, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
                    for j in range(ne):
                        if not real[j]:
                            continue
                        qx, qy = _obs_at(obs[j][0], obs[j][1], io, N)
                        dx, dy = px - qx, py - qy
                        dist = _sqrt(dx * dx + dy * dy)
                        g = dist - (R[j] + GUIDANCE_PUSH_MARGIN)
                        if g != g:
                            g = INF
                        if g < bg:
                            bg, bdist, bqx, bqy, bdx, bdy, bR = g, dist, qx, qy, dx, dy, R[j] + GUIDANCE_PUSH_MARGIN
                    if bg < 0.0:
                        dm = _fmax(bdist, 1e-9)
                        px = bqx + (bdx / dm) * bR
                        py = bqy + (bdy / dm) * bR
            desx[i], desy[i] = px, py
        # pure-pursuit unicycle inside |a| <= 2, |w| <= 0.8, the heading a unit vector
        x, y, ch, sh, v = x0, y0, c0, s0h, v0
        for i in range(NF):
            if i % FINE == 0:
                k = i // FINE
                pos[c, k] = (x, y)
                vf = _fmax(v, GUIDANCE_V_FLOOR)
                vel[c, k] = (vf * ch, vf * sh)
            look = _fmax(0.6, 0.6 * v)
            q = _fmin((look / _fmax(vt[i], 0.3)) / h - 1e-9, float(NF))
            if not q > 0.0:
                q = 0.0
            n = int(q)
            if float(n) < q:
                n += 1
            jj = min(NF - 1, i + n)
            tx, ty = desx[jj] - x, desy[jj] - y
            dist = _sqrt(tx * tx + ty * ty)
            dot = ch * tx + sh * ty
            crs = ch * ty - sh * tx
            sa = crs / _fmax(dist, 1e-9)
            if dot < 0.0:
                sa = 1.0 if crs >= 0.0 else -1.0
            w = _fmin(0.8, _fmax(-0.8, ((2.0 * _fmax(v, 0.3)) * sa) / _fmax(dist, 0.3)))
            a = _fmin(2.0, _fmax(-2.0, 2.0 * (vt[i] - v)))
            x = x + (h * v) * ch
            y = y + (h * v) * sh
            tau = (h * w) * 0.5
            t2 = tau * tau
            den = 1.0 + t2
            cn = ((1.0 - t2) * ch - (2.0 * tau) * sh) / den
            sn_ = ((1.0 - t2) * sh + (2.0 * tau) * ch) / den
            ch, sh = cn, sn_
            v = _fmax(v + h * a, 0.0)
        heading_end[c] = (ch, sh)
        px_, py_ = [float(p) for p in pos[c, :, 0]], [float(p) for p in pos[c, :, 1]]
        # ---- 4 clearance, cost, signature
        cl = INF
        for k in range(1, N + 1):
            for back in (1, 0):
                for j in range(ne):
                    if not real[j]:
                        continue
                    qx, qy = _obs_at(obs[j][0], obs[j][1], FINE * (k - back), N)
                    dx, dy = px_[k] - qx, py_[k] - qy
                    d = _sqrt(dx * dx + dy * dy) - R[j]
                    if d != d:
                        d = -INF
                    if d < cl:
                        cl = d
        clearance[c] = cl
        co = 0.0
        for k in range(N + 1):
            dx, dy = px_[k] - nomx[FINE * k], py_[k] - nomy[FINE * k]
            co = co + (dx * dx + dy * dy)
        cost[c] = co if co == co else INF
        side[c] = _side_bits(px_, py_, N, obs, real, mask)
    # ---- 5 classes found
    n_paths = G - 1
    keep = []
    for c in range(C):
        if not clearance[c] >= GUIDANCE_CLEARANCE:
            continue
        dup = False
        for q in range(C):
            if q != c and clearance[q] >= GUIDANCE_CLEARANCE and side[q] == side[c] and \
                    (cost[q] < cost[c] or (cost[q] == cost[c] and q < c)):
                dup = True
        if not dup:
            keep.append(c)
    order = sorted(keep, key=lambda c: (cost[c], c))[:n_paths]
    n_found = len(order)
    # ---- 6 class ids
    K = 2 * n_paths
    used = [bool(class_used[q]) for q in range(K)]
    stored = [0] * K
    for q in range(K):
        if used[q]:
            stored[q] = _side_bits([float(v) for v in class_traj[q, :, 0]], [float(v) for v in class_traj[q, :, 1]],
                                   N, obs, real, mask)
    taken = [False] * K
    ids = [-1] * n_found
    for p, c in enumerate(order):
        for q in range(K):
            if used[q] and not taken[q] and stored[q] == side[c]:
                ids[p], taken[q] = q, True
                break
    for p in range(n_found):
        if ids[p] < 0:
            for q in range(K):
                if not used[q] and not taken[q]:
                    ids[p], taken[q] = q, True
                    break
    new_traj = np.array(class_traj, np.float64)
    for p, c in enumerate(order):
        new_traj[ids[p]] = pos[c]
    return dict(pos=pos, vel=vel, clearance=np.array(clearance), cost=np.array(cost), side=side, mask=mask,
                requested=requested, order=order, ids=ids, n_found=n_found, class_traj=new_traj,
                class_used=np.array(taken, np.uint8), relevant=np.array(rel), rank=np.array(rank),
                closest_index=np.array(ic), lateral=np.array(lat), heading_end=heading_end,
                closest_distance=np.array(cdist), real=np.array(real))


def map_planners_host(planner_class, found_ids) -> dict:
    """mapGuidanceTrajectoriesToPlanners (guidance_constraints.cpp:208-257), literally: planner_class (G,)
    the planners' result.guidance_ID of the previous step, found_ids the classes of this step's
    trajectories.  Returns dict(existing_guidance (G,) bool, taken (G,) bool, mapping {trajectory: planner}).

    Quirk kept: the second loop has no `break`, so the first remaining trajectory marks EVERY untaken
    planner taken and is mapped to the last of them; later remaining trajectories map to nothing.  (The
    map itself is not read afterwards -- planner p takes trajectory p, :398 -- so only existing_guidance
    reaches the solves.)"""
    G = len(planner_class)
    taken = [False] * G
    existing = [False] * G
    mapping = {}
    remaining = []
    for i, cls in enumerate(found_ids):
        found = False
        for p in range(G):
            if int(planner_class[p]) == int(cls) and not taken[p]:
                mapping[i] = p
                taken[p] = existing[p] = True
                found = True
                break
        if not found:
            remaining.append(i)
    for i in remaining:
        for p in range(G):
            if not taken[p]:
                mapping[i] = p
                taken[p] = True
                existing[p] = False
    return dict(existing_guidance=np.array(existing), taken=np.array(taken), mapping=mapping)


def planner_flags_host(topology, enabled, guided, selected_topology: int, prev_was_original: bool,
                       consistency_on_non_guided: bool):
    """previously_selected (:418) and shouldEnableConsistencyForPlanner (:951-984, without the
    _has_previous_trajectory test, which stays with the prev_elapsed rule of the producers) of one
    scene's planners.  Returns (previously_selected (G,), consistency_on (G,)) bool."""
    G = len(topology)
    ps, on = np.zeros(G, bool), np.zeros(G, bool)
    sel, orig = int(selected_topology), bool(prev_was_original)
    for p in range(G):
        ps[p] = bool(guided[p]) and bool(enabled[p]) and int(topology[p]) == sel
        if sel == -1 and not orig:
            on[p] = False
        elif not guided[p]:
            on[p] = bool(consistency_on_non_guided) and orig
        else:
            on[p] = (not orig) and bool(enabled[p]) and int(topology[p]) == sel
    return ps, on


def guidance_update_host(layout, state, stage_params, obst, obst_meta, lstate: dict, guidance, G: int,
                         settings: GuidanceSettings, heading=None, details: bool = False) -> dict:
    """The restatement of mpcg_guidance_update for every scene.  state (S, nx), stage_params (S, npar),
    obst (S, n_ell, N, 5), obst_meta (S, n_ell, 2), lstate: the layer state (`initial_state`), guidance
    (S, G, N+1, 4) the rows before the step; none is modified.  heading (S, 2): the (cos psi, sin psi)
    to use instead of numpy's.  Returns the outputs of include/mpcg_guidance.h plus the new class_traj /
    class_used (and, with details, the per-scene intermediate results)."""
    state = np.asarray(state, np.float64)
    S, N, dt = state.shape[0], layout.N, layout.dt
    ne, n_seg = layout.n_ell, layout.n_seg
    if layout.nx != 5 or not 2 <= N <= GUIDANCE_MAX_N or ne > GUIDANCE_MAX_ELL or not 1 <= n_seg <= GUIDANCE_MAX_SEG \
            or not 1 <= G - 1 <= GUIDANCE_CANDIDATES:
        raise ValueError("guidance_update_host: shape outside the limits of include/mpcg_guidance.h")
    i0 = layout.idx("spline_x0_a")
    if heading is None:
        heading = np.stack([np.cos(state[:, 2]), np.sin(state[:, 2])], 1)
    heading = np.asarray(heading, np.float64)
    gd = np.array(guidance, np.float64)
    K = 2 * (G - 1)
    out = dict(guidance=gd, existing_guidance=np.zeros((S, G), np.uint8), previously_selected=np.zeros((S, G), np.uint8),
               consistency_on=np.zeros((S, G), np.uint8), topology=np.full((S, G), -1, np.int32),
               enabled=np.zeros((S, G), np.uint8), n_found=np.zeros(S, np.int32), heading=heading.copy(),
               sig_mask=np.zeros((S, G), np.uint32), sig_side=np.zeros((S, G), np.uint32),
               clearance=np.zeros((S, GUIDANCE_CANDIDATES)), cost=np.zeros((S, GUIDANCE_CANDIDATES)),
               class_traj=np.array(lstate["class_traj"], np.float64), class_used=np.array(lstate["class_used"], np.uint8))
    det = []
    guided = np.ones(G, bool)
    guided[G - 1] = False
    for s in range(S):
        window = np.asarray(stage_params[s][i0:i0 + 9 * n_seg], np.float64).reshape(n_seg, 9)
        r = _scene_update(state[s], window, np.asarray(obst[s], np.float64), np.asarray(obst_meta[s], np.float64)[:, 0],
                          N, dt, G, settings, heading[s], out["class_traj"][s], out["class_used"][s])
        det.append(r)
        nf = r["n_found"]
        out["n_found"][s] = nf
        out["clearance"][s], out["cost"][s] = r["clearance"], r["cost"]
        out["class_traj"][s], out["class_used"][s] = r["class_traj"], r["class_used"]
        # ---- 7 planner bookkeeping
        for p in range(nf):
            c = r["order"][p]
            gd[s, p, :, 0:2], gd[s, p, :, 2:4] = r["pos"][c], r["vel"][c]
            out["topology"][s, p], out["enabled"][s, p] = r["ids"][p], 1
            out["sig_mask"][s, p], out["sig_side"][s, p] = r["mask"], r["side"][c]
        out["topology"][s, G - 1], out["enabled"][s, G - 1] = K, 1
        out["existing_guidance"][s] = map_planners_host(lstate["planner_class"][s], r["ids"])["existing_guidance"]
        ps, on = planner_flags_host(out["topology"][s], out["enabled"][s], guided, lstate["selected_topology"][s],
                                    lstate["prev_was_original"][s], settings.consistency_on_non_guided)
        out["previously_selected"][s], out["consistency_on"][s] = ps, on
    if details:
        out["details"] = det
    return out


def mask_host(exit_code, enabled):
    """mpcg_guidance_mask: the exit codes (S*G,) with those of disabled planners replaced."""
    ex = np.array(exit_code, np.int32).reshape(-1)
    ex[np.asarray(enabled).reshape(-1) == 0] = GUIDANCE_EXIT_DISABLED
    return ex


def select_host(best, guided, topology, enabled) -> dict:
    """mpcg_guidance_select: selected_topology (S,), prev_was_original (S,), planner_class (S, G)
    (guidance_constraints.cpp:379, :399, :436-437, :538-539)."""
    best = np.asarray(best).astype(np.int64)
    guided, topology, enabled = np.asarray(guided), np.asarray(topology), np.asarray(enabled)
    S, G = topology.shape
    sel = np.full(S, -1, np.int32)
    orig = np.zeros(S, np.uint8)
    for s in range(S):
        b = int(best[s])
        if 0 <= b < G:
            sel[s] = topology[s, b]
            orig[s] = 0 if guided[s, b] else 1
    return dict(selected_topology=sel, prev_was_original=orig,
                planner_class=np.where(enabled != 0, topology, -1).astype(np.int32))


# ------------------------------------------------------------------ the device layer


class GuidanceLayer:
    """The device-resident guidance of a `ControlLoop` (ControlLoop(..., guidance_layer=layer)):

        update(loop)              mpcg_guidance_update: guidance, existing_guidance, previously_selected and
                                  consistency_on written into the loop's scene tensors, topology / enabled /
                                  n_found kept here
        mask(exit)                mpcg_guidance_mask, between the solve and the selection
        after_select(loop, out)   mpcg_guidance_select: the selection record of the next step
    """

    def __init__(self, layout, S: int, G: int, device, settings: GuidanceSettings | None = None):
        import torch

        from . import native

        self.lay, self.S, self.G, self.dev = layout, S, G, device
        self.settings = settings or GuidanceSettings()
        self._set = self.settings.native()
        self._native = native
        self.pr = native.problem_from_layout(layout)
        self.state = {k: torch.from_numpy(v).to(device) for k, v in initial_state(S, G, layout.N).items()}
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        C = GUIDANCE_CANDIDATES
        self.existing_guidance = z((S, G), torch.uint8)
        self.topology = torch.full((S, G), -1, dtype=torch.int32, device=device)
        self.enabled = z((S, G), torch.uint8)
        self.n_found = z((S,), torch.int32)
        self.heading = z((S, 2), torch.float64)
        self.sig_mask, self.sig_side = z((S, G), torch.int32), z((S, G), torch.int32)
        self.clearance, self.cost = z((S, C), torch.float64), z((S, C), torch.float64)

    def update(self, loop, stream=None):
        d = loop.dsc
        for k in ("previously_selected", "consistency_on"):
            if d[k].dtype != self.enabled.dtype or not d[k].is_contiguous():
                raise ValueError(f"GuidanceLayer.update: the loop's {k} must be a contiguous uint8 tensor")
        self._native.guidance_update_device(self.pr, self.S, self.G, self._set, d["state"], d["stage_params"], d["obst"],
                                            d["obst_meta"], self.state, d["guidance"], self.existing_guidance,
                                            d["previously_selected"], d["consistency_on"], self.topology,
                                            self.enabled, self.n_found, self.heading, self.sig_mask, self.sig_side,
                                            self.clearance, self.cost, stream=stream)

    def mask(self, exit_code, stream=None):
        self._native.guidance_mask_device(self.S, self.G, self.enabled, exit_code, stream=stream)

    def after_select(self, loop, out, stream=None):
        self._native.guidance_select_device(self.S, self.G, out["best"], loop.dsc["guided"], self.topology,
                                            self.enabled, self.state, stream=stream)
