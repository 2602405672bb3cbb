// mpcg_guidance.h — the guidance layer of one control step on the GPU: a per-step
// producer of side-pattern guidance trajectories (a stand-in for the output of the
// external guidance_planner), their topology class ids, and the reference's planner
// bookkeeping around them (guidance_constraints.cpp:208-257, :311-318, :418, :951-984).
// ABI, the generator's rules and the constants: include/mpcg_guidance.h; host
// restatement: guidance.py (guidance_update_host, select_host).
//
// Three kernels:
//   guidance_update_kernel  one 64-lane workgroup (one wavefront) per scene, everything staged in LDS, no
//                           scratch; the LDS block is sized for the launch's shape (gd_lds_bytes).
//                           Phases, each uniform over the wavefront and closed by a barrier:
//                             A  window, obstacle rows, heading; nominal (lane i = fine samples i, i + 64, ..;
//                                the arc-length prefix sum on lane 0)
//                             B  lane j = obstacle j: closest approach, relevance, rank
//                             C  lane 8 c + r = candidate c, fine samples r, r + 8, ..: offset and push-out
//                             D  lane c = candidate c: the unicycle, clearance, cost, signature;
//                                lane 8 + q = stored class q: its signature against this step's obstacles
//                             E  lane 0: classes found, class ids, planner bookkeeping
//                             F  all lanes: the guidance rows and the stored trajectories
//   guidance_mask_kernel    one thread per planner
//   guidance_select_kernel  one thread per scene
// Compiled only into mpcg_guidance.hip with -ffp-contract=off, in the host
// restatement's operation order with one rounding per operation.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_guidance.h"  // the public header of the same name

namespace mpcg {

constexpr int GD_C = MPCG_GUIDANCE_CANDIDATES;
constexpr int GD_FINE = MPCG_GUIDANCE_FINE;
constexpr int GD_MAX_N = MPCG_GUIDANCE_MAX_N;
constexpr int GD_MAX_ELL = MPCG_GUIDANCE_MAX_ELL;
constexpr int GD_MAX_SEG = MPCG_GUIDANCE_MAX_SEG;
constexpr int GD_MAX_K = 2 * GD_C;

// The workgroup's LDS, carved out of one dynamic block sized for the launch's own N, n_ell and n_seg
// (gd_lds_bytes; C2: 23 KB, the limits N 32 / 32 slots / 8 segments: 49 KB), so that more workgroups
// share a CU than arrays sized for the limits would allow.  Rows: win [n_seg][9], ox / oy [n_ell][N],
// desx / desy [8][NF], px / py / vx / vy [8][N + 1], NF = FINE N + 1.
struct GuidanceLds {
    double *win, *ox, *oy, *R, *lat, *vt, *sn, *nomx, *nomy, *nrx, *nry, *desx, *desy, *px, *py, *vx, *vy, *clear,
        *cost, *head;
    int *real, *rel, *ic, *rank, *order, *ids, *n_found;
    unsigned *side, *stored;
};

__host__ __device__ inline int gd_lds_doubles(int N, int ne, int n_seg) {
    const int NF = GD_FINE * N + 1;
    return 9 * n_seg + 2 * ne * N + 2 * ne + 6 * NF + 2 * GD_C * NF + 4 * GD_C * (N + 1) + 2 * GD_C + 2;
}

__host__ __device__ inline int gd_lds_bytes(int N, int ne, int n_seg) {
    return 8 * gd_lds_doubles(N, ne, n_seg) + 4 * (4 * ne + 3 * GD_C + GD_MAX_K + 1);
}

__device__ __forceinline__ GuidanceLds gd_carve(double* base, int N, int ne, int n_seg) {
    const int NF = GD_FINE * N + 1;
    GuidanceLds L;
    double* d = base;
    L.win = d; d += 9 * n_seg;
    L.ox = d; d += ne * N;
    L.oy = d; d += ne * N;
    L.R = d; d += ne;
    L.lat = d; d += ne;
    L.vt = d; d += NF;
    L.sn = d; d += NF;
    L.nomx = d; d += NF;
    L.nomy = d; d += NF;
    L.nrx = d; d += NF;
    L.nry = d; d += NF;
    L.desx = d; d += GD_C * NF;
    L.desy = d; d += GD_C * NF;
    L.px = d; d += GD_C * (N + 1);
    L.py = d; d += GD_C * (N + 1);
    L.vx = d; d += GD_C * (N + 1);
    L.vy = d; d += GD_C * (N + 1);
    L.clear = d; d += GD_C;
    L.cost = d; d += GD_C;
    L.head = d; d += 2;
    int* i = reinterpret_cast<int*>(d);
    L.real = i; i += ne;
    L.rel = i; i += ne;
    L.ic = i; i += ne;
    L.rank = i; i += ne;
    L.order = i; i += GD_C;
    L.ids = i; i += GD_C;
    L.n_found = i; i += 1;
    L.side = reinterpret_cast<unsigned*>(i); i += GD_C;
    L.stored = reinterpret_cast<unsigned*>(i);
    return L;
}

__device__ __forceinline__ double gd_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// obstacle j at fine index i (time i h): linear between rows k and k + 1, k = min(i / FINE, N - 2)
__device__ __forceinline__ void gd_obs_at(const GuidanceLds& L, int j, int i, int N, double& x, double& y) {
    const int k = min(i / GD_FINE, N - 2);
    const double f = __ddiv_rn((double)(i - GD_FINE * k), (double)GD_FINE);
    x = L.ox[j * N + k] + (L.ox[j * N + k + 1] - L.ox[j * N + k]) * f;
    y = L.oy[j * N + k] + (L.oy[j * N + k + 1] - L.oy[j * N + k]) * f;
}

// the side word of a trajectory (x at px[k * stride], y at py[k * stride], k = 0 .. N) against the obstacles of mask
__device__ __forceinline__ unsigned gd_side_bits(const GuidanceLds& L, const double* px, const double* py, int stride,
                                                 int N, int ne, unsigned mask) {
    unsigned side = 0;
    for (int j = 0; j < ne; ++j) {
        if (!((mask >> j) & 1u)) continue;
        double bd = gd_inf(), bx = 0.0, by = 0.0;
        int bk = 0;
        for (int k = 0; k <= N; ++k) {
            double qx, qy;
            gd_obs_at(L, j, GD_FINE * k, N, qx, qy);
            const double dx = qx - px[k * stride], dy = qy - py[k * stride];
            double d2 = dx * dx + dy * dy;
            if (!(d2 == d2)) d2 = gd_inf();
            if (d2 < bd || k == 0) {
                bd = d2;
                bk = k;
                bx = dx;
                by = dy;
            }
        }
        const int k0 = bk < N ? bk : N - 1;
        const double tx = px[(k0 + 1) * stride] - px[k0 * stride], ty = py[(k0 + 1) * stride] - py[k0 * stride];
        if (tx * by - ty * bx > 0.0) side |= 1u << j;
    }
    return side;
}

__global__ __launch_bounds__(64) void guidance_update_kernel(int n_scenes, int G, int N, int nx, int npar, int i_spline0,
                                                             int n_seg, int ne, double dt, mpcg_guidance_settings set,
                                                             const double* __restrict__ state,
                                                             const double* __restrict__ stage_params,
                                                             const double* __restrict__ obst,
                                                             const double* __restrict__ obst_meta,
                                                             mpcg_guidance_state st, mpcg_guidance_out out) {
    extern __shared__ double gd_lds[];
    const int s = blockIdx.x;
    if (s >= n_scenes) return;
    const GuidanceLds L = gd_carve(gd_lds, N, ne, n_seg);
    const int lane = threadIdx.x;
    const int NF = GD_FINE * N + 1;
    const int n_paths = G - 1, K = 2 * n_paths;
    const double h = __ddiv_rn(dt, (double)GD_FINE);
    const double* x = state + (size_t)s * nx;
    const double x0 = x[0], y0 = x[1], v0 = x[3], s0 = x[4];
    // ---- A: staging and the nominal
    for (int e = lane; e < 9 * n_seg; e += 64) L.win[e] = stage_params[(size_t)s * npar + i_spline0 + e];
    for (int e = lane; e < ne * N; e += 64) {
        const int j = e / N, k = e - j * N;
        const double* row = obst + (((size_t)s * ne + j) * N + k) * 5;
        L.ox[j * N + k] = row[0];
        L.oy[j * N + k] = row[1];
    }
    for (int j = lane; j < ne; j += 64) {
        const double r = obst_meta[((size_t)s * ne + j) * 2];
        L.real[j] = r > 0.0 ? 1 : 0;
        L.R[j] = set.robot_radius + r;
    }
    if (lane == 0) {
        L.head[0] = cos(x[2]);
        L.head[1] = sin(x[2]);
        out.heading[(size_t)s * 2 + 0] = L.head[0];
        out.heading[(size_t)s * 2 + 1] = L.head[1];
    }
    const double vmax = fmax(set.v_ref, v0);
    for (int i = lane; i < NF; i += 64) L.vt[i] = fmin(v0 + MPCG_GUIDANCE_ACCEL * ((double)i * h), vmax);
    __syncthreads();
    if (lane == 0) {
        double acc = s0;
        L.sn[0] = acc;
        for (int i = 1; i < NF; ++i) {
            acc = acc + (0.5 * (L.vt[i] + L.vt[i - 1])) * h;
            L.sn[i] = acc;
        }
    }
    __syncthreads();
    const double c0 = L.head[0], s0h = L.head[1];
    for (int i = lane; i < NF; i += 64) {
        const double sv = L.sn[i];
        int j = 0;
        for (int k = 1; k < n_seg; ++k) j += L.win[9 * k + 8] <= sv ? 1 : 0;
        const double* w = L.win + 9 * j;
        const double t = sv - w[8];
        L.nomx[i] = ((w[0] * t + w[1]) * t + w[2]) * t + w[3];
        L.nomy[i] = ((w[4] * t + w[5]) * t + w[6]) * t + w[7];
        const double dx = ((3.0 * w[0]) * t + 2.0 * w[1]) * t + w[2];
        const double dy = ((3.0 * w[4]) * t + 2.0 * w[5]) * t + w[6];
        const double nr = __dsqrt_rn(dx * dx + dy * dy);
        double tx = c0, ty = s0h;
        if (nr > 1e-12) {
            tx = __ddiv_rn(dx, nr);
            ty = __ddiv_rn(dy, nr);
        }
        L.nrx[i] = -ty;
        L.nry[i] = tx;
    }
    __syncthreads();
    // ---- B: relevant obstacles
    for (int j = lane; j < ne; j += 64) {
        double bd = gd_inf();
        int bi = 0;
        for (int i = 0; i < NF; ++i) {
            double qx, qy;
            gd_obs_at(L, j, i, N, qx, qy);
            const double dx = L.nomx[i] - qx, dy = L.nomy[i] - qy;
            double d2 = dx * dx + dy * dy;
            if (!(d2 == d2)) d2 = gd_inf();
            if (d2 < bd) {
                bd = d2;
                bi = i;
            }
        }
        double qx, qy;
        gd_obs_at(L, j, bi, N, qx, qy);
        L.rel[j] = (L.real[j] && __dsqrt_rn(bd) < MPCG_GUIDANCE_RELEVANT) ? 1 : 0;
        L.ic[j] = bi;
        L.lat[j] = (qx - L.nomx[bi]) * L.nrx[bi] + (qy - L.nomy[bi]) * L.nry[bi];
    }
    __syncthreads();
    for (int j = lane; j < ne; j += 64) {
        int r = 0;
        for (int q = 0; q < ne; ++q)
            r += (L.rel[q] && (L.ic[q] < L.ic[j] || (L.ic[q] == L.ic[j] && q < j))) ? 1 : 0;
        L.rank[j] = r;
    }
    unsigned mask = 0;
    for (int j = 0; j < ne; ++j) mask |= L.rel[j] ? 1u << j : 0u;
    __syncthreads();
    // ---- C: the desired path of candidate c, fine samples r, r + 8, ..
    {
        const int c = lane >> 3;
        for (int i = lane & 7; i < NF; i += 8) {
            const double t = (double)i * h;
            double off = 0.0;
            for (int j = 0; j < ne; ++j) {
                if (!L.rel[j]) continue;
                const bool left = L.rank[j] < MPCG_GUIDANCE_BITS ? ((c >> L.rank[j]) & 1) == 1 : L.lat[j] >= 0.0;
                double want;
                bool use;
                if (left) {
                    want = L.lat[j] - MPCG_GUIDANCE_OFFSET;
                    use = !(want > 0.0);
                } else {
                    want = L.lat[j] + MPCG_GUIDANCE_OFFSET;
                    use = !(want < 0.0);
                }
                if (!use) continue;
                const double u = __ddiv_rn(t - (double)L.ic[j] * h, MPCG_GUIDANCE_WIDTH);
                const double q = 1.0 + u * u;
                off = off + (want * __ddiv_rn(1.0, q * q)) * __ddiv_rn(t, t + MPCG_GUIDANCE_ONSET);
            }
            double px = ((L.nomx[i] + off * L.nrx[i]) - L.nomx[0]) + x0;
            double py = ((L.nomy[i] + off * L.nry[i]) - L.nomy[0]) + y0;
            // push-out sweeps, a fixed number: from the obstacle that violates its distance most
            for (int sw = 0; sw < MPCG_GUIDANCE_SWEEPS; ++sw) {
                for (int back = 1; back >= 0; --back) {
                    const int io = max(i - GD_FINE * back, 0);
                    double bg = gd_inf(), bdist = 0.0, bqx = 0.0, bqy = 0.0, bdx = 0.0, bdy = 0.0, bR = 0.0;
                    for (int j = 0; j < ne; ++j) {
                        if (!L.real[j]) continue;
                        double qx, qy;
                        gd_obs_at(L, j, io, N, qx, qy);
                        const double dx = px - qx, dy = py - qy;
                        const double dist = __dsqrt_rn(dx * dx + dy * dy);
                        const double Rj = L.R[j] + MPCG_GUIDANCE_PUSH_MARGIN;
                        double g = dist - Rj;
                        if (!(g == g)) g = gd_inf();
                        if (g < bg) {
                            bg = g;
                            bdist = dist;
                            bqx = qx;
                            bqy = qy;
                            bdx = dx;
                            bdy = dy;
                            bR = Rj;
                        }
                    }
                    if (bg < 0.0) {
                        const double dm = fmax(bdist, 1e-9);
                        px = bqx + __ddiv_rn(bdx, dm) * bR;
                        py = bqy + __ddiv_rn(bdy, dm) * bR;
                    }
                }
            }
            L.desx[c * NF + i] = px;
            L.desy[c * NF + i] = py;
        }
    }
    __syncthreads();
    // ---- D: the unicycle, clearance, cost and signature of candidate `lane`; stored classes on lanes 8 ..
    if (lane < GD_C) {
        const int c = lane;
        double xx = x0, yy = y0, ch = c0, sh = s0h, v = v0;
        for (int i = 0; i < NF; ++i) {
            if (i % GD_FINE == 0) {
                const int k = i / GD_FINE;
                const double vf = fmax(v, MPCG_GUIDANCE_V_FLOOR);
                L.px[c * (N + 1) + k] = xx;
                L.py[c * (N + 1) + k] = yy;
                L.vx[c * (N + 1) + k] = vf * ch;
                L.vy[c * (N + 1) + k] = vf * sh;
            }
            const double look = fmax(0.6, 0.6 * v);
            double q = fmin(__ddiv_rn(__ddiv_rn(look, fmax(L.vt[i], 0.3)), h) - 1e-9, (double)NF);
            if (!(q > 0.0)) q = 0.0;
            int n = (int)q;
            if ((double)n < q) n += 1;
            const int jj = min(NF - 1, i + n);
            const double tx = L.desx[c * NF + jj] - xx, ty = L.desy[c * NF + jj] - yy;
            const double dist = __dsqrt_rn(tx * tx + ty * ty);
            const double dot = ch * tx + sh * ty;
            const double crs = ch * ty - sh * tx;
            double sa = __ddiv_rn(crs, fmax(dist, 1e-9));
            if (dot < 0.0) sa = crs >= 0.0 ? 1.0 : -1.0;
            const double w = fmin(0.8, fmax(-0.8, __ddiv_rn((2.0 * fmax(v, 0.3)) * sa, fmax(dist, 0.3))));
            const double a = fmin(2.0, fmax(-2.0, 2.0 * (L.vt[i] - v)));
            xx = xx + (h * v) * ch;
            yy = yy + (h * v) * sh;
            // the Cayley rotation of tau = h w / 2: exactly orthogonal, the heading stays a unit vector
            const double tau = (h * w) * 0.5;
            const double t2 = tau * tau;
            const double den = 1.0 + t2;
            const double cn = __ddiv_rn((1.0 - t2) * ch - (2.0 * tau) * sh, den);
            const double sn = __ddiv_rn((1.0 - t2) * sh + (2.0 * tau) * ch, den);
            ch = cn;
            sh = sn;
            v = fmax(v + h * a, 0.0);
        }
        double cl = gd_inf();
        for (int k = 1; k <= N; ++k)
            for (int back = 1; back >= 0; --back)
                for (int j = 0; j < ne; ++j) {
                    if (!L.real[j]) continue;
                    double qx, qy;
                    gd_obs_at(L, j, GD_FINE * (k - back), N, qx, qy);
                    const double dx = L.px[c * (N + 1) + k] - qx, dy = L.py[c * (N + 1) + k] - qy;
                    double d = __dsqrt_rn(dx * dx + dy * dy) - L.R[j];
                    if (!(d == d)) d = -gd_inf();
                    if (d < cl) cl = d;
                }
        double co = 0.0;
        for (int k = 0; k <= N; ++k) {
            const double dx = L.px[c * (N + 1) + k] - L.nomx[GD_FINE * k], dy = L.py[c * (N + 1) + k] - L.nomy[GD_FINE * k];
            co = co + (dx * dx + dy * dy);
        }
        L.clear[c] = cl;
        L.cost[c] = co == co ? co : gd_inf();
        L.side[c] = gd_side_bits(L, L.px + c * (N + 1), L.py + c * (N + 1), 1, N, ne, mask);
        out.clearance[(size_t)s * GD_C + c] = cl;
        out.cost[(size_t)s * GD_C + c] = L.cost[c];
    } else if (lane < GD_C + K) {
        const int q = lane - GD_C;
        unsigned sd = 0;
        if (st.class_used[(size_t)s * K + q]) {
            const double* tr = st.class_traj + ((size_t)s * K + q) * (N + 1) * 2;
            sd = gd_side_bits(L, tr, tr + 1, 2, N, ne, mask);
        }
        L.stored[q] = sd;
    }
    __syncthreads();
    // ---- E: classes found, class ids and the planner bookkeeping
    if (lane == 0) {
        int nf = 0;
        for (int c = 0; c < GD_C; ++c) {
            bool keep = L.clear[c] >= MPCG_GUIDANCE_CLEARANCE;
            int before = 0;   // kept candidates ordered before c by (cost, c)
            for (int q = 0; q < GD_C && keep; ++q) {
                if (q == c || !(L.clear[q] >= MPCG_GUIDANCE_CLEARANCE)) continue;
                const bool better = L.cost[q] < L.cost[c] || (L.cost[q] == L.cost[c] && q < c);
                if (L.side[q] == L.side[c] && better) keep = false;
            }
            if (!keep) continue;
            for (int q = 0; q < GD_C; ++q) {
                if (q == c || !(L.clear[q] >= MPCG_GUIDANCE_CLEARANCE)) continue;
                // q is kept itself unless an equal signature beats it
                bool qkeep = true;
                for (int r = 0; r < GD_C; ++r) {
                    if (r == q || !(L.clear[r] >= MPCG_GUIDANCE_CLEARANCE)) continue;
                    if (L.side[r] == L.side[q] && (L.cost[r] < L.cost[q] || (L.cost[r] == L.cost[q] && r < q)))
                        qkeep = false;
                }
                if (qkeep && (L.cost[q] < L.cost[c] || (L.cost[q] == L.cost[c] && q < c))) ++before;
            }
            if (before < n_paths) {
                L.order[before] = c;
                ++nf;
            }
        }
        *L.n_found = nf;
        unsigned used = 0, taken = 0;
        for (int q = 0; q < K; ++q) used |= st.class_used[(size_t)s * K + q] ? 1u << q : 0u;
        for (int p = 0; p < nf; ++p) {
            int id = -1;
            for (int q = 0; q < K && id < 0; ++q)
                if (((used >> q) & 1u) && !((taken >> q) & 1u) && L.stored[q] == L.side[L.order[p]]) id = q;
            if (id >= 0) taken |= 1u << id;
            L.ids[p] = id;
        }
        for (int p = 0; p < nf; ++p) {
            if (L.ids[p] >= 0) continue;
            int id = -1;
            for (int q = 0; q < K && id < 0; ++q)
                if (!((used >> q) & 1u) && !((taken >> q) & 1u)) id = q;
            // (at most n_paths ids are in use and at most n_paths are taken: one of the 2 n_paths is free)
            id = id < 0 ? 0 : id;
            taken |= 1u << id;
            L.ids[p] = id;
        }
        for (int q = 0; q < K; ++q) st.class_used[(size_t)s * K + q] = (taken >> q) & 1u;
        // mapGuidanceTrajectoriesToPlanners (guidance_constraints.cpp:208-257): the first loop.  The second
        // loop (no `break`: one remaining trajectory marks every untaken planner taken, see
        // guidance.map_planners_host) only changes `taken` and the map, which nothing reads afterwards
        // (planner p takes trajectory p, :398), and leaves existing_guidance false.
        unsigned ptaken = 0, existing = 0;
        for (int i = 0; i < nf; ++i)
            for (int p = 0; p < G; ++p)
                if (st.planner_class[(size_t)s * G + p] == L.ids[i] && !((ptaken >> p) & 1u)) {
                    ptaken |= 1u << p;
                    existing |= 1u << p;
                    break;
                }
        const int sel = st.selected_topology[s];
        const bool orig = st.prev_was_original[s] != 0;
        const bool none = sel == -1 && !orig;
        for (int p = 0; p < G; ++p) {
            const size_t i = (size_t)s * G + p;
            const bool guided = p < G - 1;
            const bool en = guided ? p < nf : true;
            const int topo = guided ? (en ? L.ids[p] : -1) : K;
            out.topology[i] = topo;
            out.enabled[i] = en ? 1 : 0;
            out.existing_guidance[i] = (existing >> p) & 1u;
            out.sig_mask[i] = guided && en ? mask : 0u;
            out.sig_side[i] = guided && en ? L.side[L.order[p]] : 0u;
            // :418 and shouldEnableConsistencyForPlanner (:951-984)
            out.previously_selected[i] = (guided && en && topo == sel) ? 1 : 0;
            bool on = false;
            if (!none) on = guided ? (!orig && en && topo == sel) : (set.consistency_on_non_guided && orig);
            out.consistency_on[i] = on ? 1 : 0;
        }
        out.n_found[s] = nf;
    }
    __syncthreads();
    // ---- F: the guidance rows of the enabled planners and the stored trajectories
    const int nf = *L.n_found;
    for (int e = lane; e < nf * (N + 1); e += 64) {
        const int p = e / (N + 1), k = e - p * (N + 1);
        const int c = L.order[p];
        double* g = out.guidance + (((size_t)s * G + p) * (N + 1) + k) * 4;
        g[0] = L.px[c * (N + 1) + k];
        g[1] = L.py[c * (N + 1) + k];
        g[2] = L.vx[c * (N + 1) + k];
        g[3] = L.vy[c * (N + 1) + k];
        double* tr = st.class_traj + (((size_t)s * K + L.ids[p]) * (N + 1) + k) * 2;
        tr[0] = L.px[c * (N + 1) + k];
        tr[1] = L.py[c * (N + 1) + k];
    }
}

__global__ void guidance_mask_kernel(int n, const unsigned char* __restrict__ enabled, int* __restrict__ exit_code) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !enabled[i]) exit_code[i] = MPCG_GUIDANCE_EXIT_DISABLED;
}

__global__ void guidance_select_kernel(int n_scenes, int G, const int* __restrict__ best,
                                       const unsigned char* __restrict__ guided, const int* __restrict__ topology,
                                       const unsigned char* __restrict__ enabled, mpcg_guidance_state st) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_scenes) return;
    const int b = best[s];
    const bool ok = b >= 0 && b < G;
    // guidance_constraints.cpp:436-437 (all failed) and :538-539
    st.selected_topology[s] = ok ? topology[(size_t)s * G + b] : -1;
    st.prev_was_original[s] = ok && !guided[(size_t)s * G + b] ? 1 : 0;
    // result.guidance_ID of every planner that ran (:379, :399); Reset() leaves -1 for a disabled one
    for (int p = 0; p < G; ++p) {
        const size_t i = (size_t)s * G + p;
        st.planner_class[i] = enabled[i] ? topology[i] : -1;
    }
}

}  // namespace mpcg
