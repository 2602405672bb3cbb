// mpcg_decomp.h — the decomp halfspaces of one control step on the GPU: the ellipsoid free-space
// decomposition around every segment of the predicted path points (DecompConstraints::update,
// decomp_constraints.cpp:52-120, with DecompUtil's EllipsoidDecomp2D restated from the published
// method) and its placement into the decomp rows of every planner.
// ABI, the construction step by step and the reference lines: include/mpcg_decomp.h; host
// restatement: decomp.py (decomp_halfspaces_host, apply_decomp_host).
//
// One kernel, one 64-lane workgroup (one wavefront) per (scene, segment k): the rows of stage k + 1;
// the workgroup of segment 0 also writes stage 0's dummies.
//   stage     the path's knots and coefficients in LDS (static), the scene's occupied points in LDS
//             (dynamic, 3 P doubles: x y interleaved, then the cached dist of the polyhedron loop)
//   points    every lane redoes the recurrence s_0 .. s_{k+1} (uniform, at most 32 steps) and
//             evaluates q_k, q_{k+1}
//   members   points are strided over lanes, lane l holds the points l, l + 64, ..; the kept set, I and
//             Rm are one bit per slot in a lane's mask
//   arg-min   a per-lane minimum in ascending slot order, then wave_argmin (mpcg_wave.h) on
//             (dist, point index): the lowest index among equal minima, as np.argmin on the host
//   rows      lane r forms row r in LDS; all lanes stream the block to the G planners
// No atomics, no communication between workgroups; every loop is bounded by a count taken before it.
// Compiled only into mpcg_decomp.hip with -ffp-contract=off and written with explicitly rounded
// operations in the host restatement's operation order: every value agrees bit for bit (no
// transcendental enters: the frame is built from the segment's direction).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_decomp.h"  // the public header of the same name
#include "mpcg_spline.h"
#include "mpcg_wave.h"

namespace mpcg {

constexpr int DECOMP_MAX_ROWS = MPCG_DECOMP_MAX_ROWS;
constexpr int DECOMP_MAX_SLOTS = MPCG_DECOMP_MAX_POINTS / WAVE_LANES;
constexpr int DECOMP_NO_POINT = 0x7fffffff;
static_assert(DECOMP_MAX_SLOTS <= 32, "one mask bit per slot");
static_assert(DECOMP_MAX_ROWS <= WAVE_LANES, "one row per lane");

struct DecompLds {
    PathLds path;
    double hp[DECOMP_MAX_ROWS][4];    // the polyhedron's first max_constraints hyperplanes: p_x p_y n_x n_y
    double rows[DECOMP_MAX_ROWS * 3];
};

struct DecompFrame {
    double ex, ey, gx, gy, cx, cy, a;
};

__device__ __forceinline__ double decomp_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ double decomp_dot(double ax, double ay, double bx, double by) {
    return __dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by));
}

// n . (o - p)
__device__ __forceinline__ double decomp_side(double nx, double ny, double ox, double oy, double px, double py) {
    return decomp_dot(nx, ny, __dsub_rn(ox, px), __dsub_rn(oy, py));
}

// u = e . (o - c), w = g . (o - c)
__device__ __forceinline__ void decomp_uw(const DecompFrame& F, double ox, double oy, double& u, double& w) {
    const double dx = __dsub_rn(ox, F.cx), dy = __dsub_rn(oy, F.cy);
    u = decomp_dot(F.ex, F.ey, dx, dy);
    w = decomp_dot(F.gx, F.gy, dx, dy);
}

// sqrt((u / a)^2 + (w / b)^2)
__device__ __forceinline__ double decomp_dist(const DecompFrame& F, double b, double ox, double oy) {
    double u, w;
    decomp_uw(F, ox, oy, u, w);
    const double ua = __ddiv_rn(u, F.a), wb = __ddiv_rn(w, b);
    return __dsqrt_rn(__dadd_rn(__dmul_rn(ua, ua), __dmul_rn(wb, wb)));
}

// getPoint(s): s inside the path (a NaN goes to the start), the segment that holds it
__device__ __forceinline__ void decomp_path_point(const PathLds& P, int m, double s, double& x, double& y) {
    const double sc = fmin(fmax(s, P.knots[0]), P.knots[m]);
    path_point(P, path_segment(P, m, sc), sc, x, y);
}

// the winner of (dist, point index) over the members of `mask`, dist(i) given by `dist_of`; a NaN counts as
// +inf.  Some lane must hold a member.
template <class D>
__device__ __forceinline__ int decomp_argmin(unsigned mask, int slots, int lane, D&& dist_of) {
    double bd = decomp_inf();
    int bi = DECOMP_NO_POINT;
    for (int j = 0; j < slots; ++j) {
        if (!((mask >> j) & 1u)) continue;
        const int i = lane + WAVE_LANES * j;
        double d = dist_of(i);
        d = d == d ? d : decomp_inf();
        if (bi == DECOMP_NO_POINT || d < bd) {
            bd = d;
            bi = i;
        }
    }
    return wave_argmin(bd, bi);
}

// the members of the wavefront's masks
__device__ __forceinline__ int decomp_count(unsigned mask) {
    int n = __popc(mask);
    for (int off = WAVE_LANES / 2; off > 0; off >>= 1) n += __shfl_xor(n, off, WAVE_LANES);
    return __builtin_amdgcn_readfirstlane(n);
}

__global__ __launch_bounds__(64) void decomp_halfspaces_kernel(mpcg_problem pr, int n_scenes, int G,
                                                               mpcg_decomp_settings set, mpcg_path_table tb,
                                                               mpcg_decomp_io io, double* __restrict__ params,
                                                               double* __restrict__ halfspaces,
                                                               int* __restrict__ n_found,
                                                               double* __restrict__ minor_axis) {
    __shared__ DecompLds L;
    extern __shared__ double decomp_dyn[];   // [P][2] points, [P] dist
    const int N = pr.N, npar = pr.npar, nx = pr.nx, nvar = pr.nu + pr.nx;
    const int sc = blockIdx.x / (N - 1), k = blockIdx.x - sc * (N - 1);
    if (sc >= n_scenes) return;
    const int lane = threadIdx.x;
    const int maxc = min(pr.n_scen, DECOMP_MAX_ROWS);
    const int P = min(max(io.max_points, 0), MPCG_DECOMP_MAX_POINTS);
    double* pts = decomp_dyn;
    double* dist = decomp_dyn + 2 * P;
    // (the entry point checked its host copies of path_of and n_occ; the clamps keep every index inside)
    const int p = min(max(tb.path_of[sc], 0), tb.n_paths - 1);
    const int M = tb.max_segments;
    const int m = min(max(tb.n_segments[p], 1), M);
    for (int e = lane; e <= m; e += WAVE_LANES) L.path.knots[e] = tb.knots[(size_t)p * (M + 1) + e];
    for (int e = lane; e < m * 8; e += WAVE_LANES) (&L.path.coef[0][0])[e] = tb.coef[(size_t)p * M * 8 + e];
    const int n = P > 0 ? min(max(io.n_occ[sc], 0), P) : 0;
    const int slots = (n + WAVE_LANES - 1) / WAVE_LANES;
    for (int e = lane; e < 2 * n; e += WAVE_LANES) pts[e] = io.occ[(size_t)sc * P * 2 + e];
    // ---- s_k, s_{k+1}: s advanced by the predicted speed (decomp_constraints.cpp:68-82)
    const double* st = io.state + (size_t)sc * nx;
    const double* mw = io.main_warm ? io.main_warm + (size_t)sc * (N + 1) * nvar + pr.nu + 3 : nullptr;
    const double brake = -fabs(set.deceleration);
    double s = st[nx - 1], v = st[3], s0 = s;
    for (int i = 0; i <= k; ++i) {
        const double vi = mw ? mw[i * nvar] : v;
        s0 = s;
        s = __dadd_rn(s, __dmul_rn(vi, pr.dt));
        v = fmax(__dadd_rn(v, __dmul_rn(brake, pr.dt)), 0.0);
    }
    const double dummy_b = __dadd_rn(st[0], 100.0);
    __syncthreads();
    // ---- the frame of segment k
    double q0x, q0y, q1x, q1y;
    decomp_path_point(L.path, m, s0, q0x, q0y);
    decomp_path_point(L.path, m, s, q1x, q1y);
    const double R = set.range;
    const double dx = __dsub_rn(q1x, q0x), dy = __dsub_rn(q1y, q0y);
    const double len = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
    const double ex = __ddiv_rn(dx, len), ey = __ddiv_rn(dy, len);
    const double hx = ey, hy = -ex;
    DecompFrame F;
    F.ex = ex, F.ey = ey, F.gx = -hx, F.gy = -hy;
    F.cx = __ddiv_rn(__dadd_rn(q0x, q1x), 2.0), F.cy = __ddiv_rn(__dadd_rn(q0y, q1y), 2.0);
    F.a = __ddiv_rn(len, 2.0);
    // the bounding box's four hyperplanes (p, n), in the order they are appended
    const double bpx[4] = {__dadd_rn(q0x, __dmul_rn(hx, R)), __dsub_rn(q0x, __dmul_rn(hx, R)),
                           __dadd_rn(q1x, __dmul_rn(ex, R)), __dsub_rn(q0x, __dmul_rn(ex, R))};
    const double bpy[4] = {__dadd_rn(q0y, __dmul_rn(hy, R)), __dsub_rn(q0y, __dmul_rn(hy, R)),
                           __dadd_rn(q1y, __dmul_rn(ey, R)), __dsub_rn(q0y, __dmul_rn(ey, R))};
    const double bnx[4] = {hx, -hx, ex, -ex}, bny[4] = {hy, -hy, ey, -ey};
    // ---- the box filter
    unsigned kept = 0;
    for (int j = 0; j < slots; ++j) {
        const int i = lane + WAVE_LANES * j;
        if (i >= n) continue;
        const double ox = pts[2 * i], oy = pts[2 * i + 1];
        bool in = true;
#pragma unroll
        for (int f = 0; f < 4; ++f) in = in && decomp_side(bnx[f], bny[f], ox, oy, bpx[f], bpy[f]) <= MPCG_DECOMP_EPS;
        kept |= in ? 1u << j : 0u;
    }
    const int n_kept = decomp_count(kept);
    // ---- the ellipsoid: shrink b until no kept point lies inside
    double b = F.a;
    unsigned I = 0;
    for (int j = 0; j < slots; ++j) {
        if (!((kept >> j) & 1u)) continue;
        const int i = lane + WAVE_LANES * j;
        I |= decomp_dist(F, b, pts[2 * i], pts[2 * i + 1]) <= 1.0 ? 1u << j : 0u;
    }
    const int n_inside = decomp_count(I);
    for (int it = 0; it < n_inside && __ballot(I != 0) != 0; ++it) {
        const double bb = b;
        const int win =
            decomp_argmin(I, slots, lane, [&](int i) { return decomp_dist(F, bb, pts[2 * i], pts[2 * i + 1]); });
        double us, ws;
        decomp_uw(F, pts[2 * win], pts[2 * win + 1], us, ws);
        if (us < F.a) {
            const double ua = __ddiv_rn(us, F.a);
            b = __ddiv_rn(fabs(ws), __dsqrt_rn(__dsub_rn(1.0, __dmul_rn(ua, ua))));
        }
        unsigned next = 0;
        for (int j = 0; j < slots; ++j) {
            if (!((I >> j) & 1u)) continue;
            const int i = lane + WAVE_LANES * j;
            next |= __dsub_rn(1.0, decomp_dist(F, b, pts[2 * i], pts[2 * i + 1])) > MPCG_DECOMP_EPS ? 1u << j : 0u;
        }
        I = next;
    }
    // ---- the polyhedron: one hyperplane per closest remaining point, tangent to the ellipsoid scaled through it
    for (int j = 0; j < slots; ++j) {
        if (!((kept >> j) & 1u)) continue;
        const int i = lane + WAVE_LANES * j;
        dist[i] = decomp_dist(F, b, pts[2 * i], pts[2 * i + 1]);   // (a lane reads back only its own entries)
    }
    unsigned Rm = kept;
    int count = 0;
    const double aa = __dmul_rn(F.a, F.a), bb2 = __dmul_rn(b, b);
    for (int it = 0; it < n_kept && __ballot(Rm != 0) != 0; ++it) {
        const int win = decomp_argmin(Rm, slots, lane, [&](int i) { return dist[i]; });
        const double ox = pts[2 * win], oy = pts[2 * win + 1];
        double us, ws;
        decomp_uw(F, ox, oy, us, ws);
        const double ca = __ddiv_rn(us, aa), cb = __ddiv_rn(ws, bb2);
        double nx_ = __dadd_rn(__dmul_rn(F.ex, ca), __dmul_rn(F.gx, cb));
        double ny_ = __dadd_rn(__dmul_rn(F.ey, ca), __dmul_rn(F.gy, cb));
        const double nl = __dsqrt_rn(__dadd_rn(__dmul_rn(nx_, nx_), __dmul_rn(ny_, ny_)));
        nx_ = __ddiv_rn(nx_, nl);
        ny_ = __ddiv_rn(ny_, nl);
        if (count < maxc && lane == 0) {
            L.hp[count][0] = ox;
            L.hp[count][1] = oy;
            L.hp[count][2] = nx_;
            L.hp[count][3] = ny_;
        }
        ++count;   // (counted on past max_constraints: n_found is the full count)
        unsigned next = 0;
        for (int j = 0; j < slots; ++j) {
            if (!((Rm >> j) & 1u)) continue;
            const int i = lane + WAVE_LANES * j;
            next |= decomp_side(nx_, ny_, pts[2 * i], pts[2 * i + 1], ox, oy) < 0.0 ? 1u << j : 0u;
        }
        Rm = next;
    }
    __syncthreads();
    // ---- rows: lane r <-> row r of the sequence polyhedron, box
    {
        const int r = lane;
        double a1 = 1.0, a2 = 0.0, rb = dummy_b;
        bool bad = false;
        const bool is_row = r < maxc && r < count + 4;
        if (is_row) {
            double px, py, nx_, ny_;
            if (r < count) {
                px = L.hp[r][0], py = L.hp[r][1], nx_ = L.hp[r][2], ny_ = L.hp[r][3];
            } else {
                const int f = r - count;
                px = f == 0 ? bpx[0] : f == 1 ? bpx[1] : f == 2 ? bpx[2] : bpx[3];
                py = f == 0 ? bpy[0] : f == 1 ? bpy[1] : f == 2 ? bpy[2] : bpy[3];
                nx_ = f == 0 ? bnx[0] : f == 1 ? bnx[1] : f == 2 ? bnx[2] : bnx[3];
                ny_ = f == 0 ? bny[0] : f == 1 ? bny[1] : f == 2 ? bny[2] : bny[3];
            }
            a1 = nx_, a2 = ny_, rb = decomp_dot(px, py, nx_, ny_);
            if (__dsub_rn(decomp_dot(nx_, ny_, F.cx, F.cy), rb) > 0.0) a1 = -a1, a2 = -a2, rb = -rb;
            const double nrm = __dsqrt_rn(__dadd_rn(__dmul_rn(a1, a1), __dmul_rn(a2, a2)));
            bad = a1 != a1 || a2 != a2 || rb != rb || nrm < 1e-3;
        }
        // the first row that is a NaN or (near) zero cuts the block: it and all after it are dummies
        const unsigned long long cut = __ballot(bad);
        const int first_bad = cut ? __ffsll((long long)cut) - 1 : WAVE_LANES;
        if (r >= first_bad) a1 = 1.0, a2 = 0.0, rb = dummy_b;
        if (r < maxc) {
            L.rows[3 * r + 0] = a1;
            L.rows[3 * r + 1] = a2;
            L.rows[3 * r + 2] = rb;
        }
    }
    __syncthreads();
    // ---- placement: 3 max_constraints consecutive doubles per (planner, stage); segment 0 also stage 0's dummies
    const int W = 3 * maxc, stage = k + 1;
    for (int g = 0; g < G; ++g) {
        double* o = params + ((size_t)(sc * G + g) * N + stage) * npar + pr.i_scen0;
        for (int e = lane; e < W; e += WAVE_LANES) o[e] = L.rows[e];
        if (k == 0) {
            double* o0 = params + (size_t)(sc * G + g) * N * npar + pr.i_scen0;
            for (int e = lane; e < W; e += WAVE_LANES) o0[e] = e % 3 == 0 ? 1.0 : (e % 3 == 1 ? 0.0 : dummy_b);
        }
    }
    if (halfspaces) {
        double* o = halfspaces + ((size_t)sc * N + stage) * W;
        for (int e = lane; e < W; e += WAVE_LANES) o[e] = L.rows[e];
        if (k == 0)
            for (int e = lane; e < W; e += WAVE_LANES)
                halfspaces[(size_t)sc * N * W + e] = e % 3 == 0 ? 1.0 : (e % 3 == 1 ? 0.0 : dummy_b);
    }
    if (lane == 0) {
        if (n_found) n_found[(size_t)sc * N + stage] = count + 4;
        if (minor_axis) minor_axis[(size_t)sc * N + stage] = b;
        if (k == 0) {
            if (n_found) n_found[(size_t)sc * N] = 0;
            if (minor_axis) minor_axis[(size_t)sc * N] = 0.0;
        }
    }
}

}  // namespace mpcg
