// mpcg_path.h — reference-path tracking of one control step on the GPU: the
// closest point on each scene's path, the window of spline segments the
// contouring cost reads, the goal test and the command of the winner.
// ABI, the search rule and the reference lines: include/mpcg_path.h; host
// restatement: paths.py (path_update_host, command_host).
//
// Two kernels:
//   path_update_kernel   one 64-lane workgroup (one wavefront) per scene; the path's knots and coefficients staged in LDS; PATH_ROUNDS = 5 rounds of
//                        64 samples (lane i = sample i), a wave arg-min on (distance^2, lane) by
//                        cross-lane exchanges, the bracket shrunk to the winner's neighbours; then
//                        closest_segment, closest_s, reached and the 9 n_seg window doubles
//                        streamed into stage_params
//   path_command_kernel  one thread per scene: the command and, with the stand-in plant, state_next
// Compiled only into mpcg_path.hip with -ffp-contract=off and written with
// explicitly rounded operations in the host restatement's operation order:
// every value that does not pass through cos / sin agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_path.h"  // the public header of the same name
#include "mpcg_spline.h"              // PathLds, path_segment, path_point
#include "mpcg_wave.h"                // wave_argmin

namespace mpcg {

constexpr int PATH_LANES = MPCG_PATH_SAMPLES;
constexpr int PATH_ROUNDS = MPCG_PATH_ROUNDS;
constexpr double PATH_LAST = (double)(PATH_LANES - 1);

// sample i of the bracket [lo, hi]
__device__ __forceinline__ double path_sample(double lo, double hi, int i) {
    const double w = __dsub_rn(hi, lo);
    return fmin(__dadd_rn(lo, __ddiv_rn(__dmul_rn(w, (double)i), PATH_LAST)), hi);
}

// |p - q|^2, a NaN counting as +inf (a total order for the arg-min)
__device__ __forceinline__ double path_dist2(double px, double py, double qx, double qy) {
    const double dx = __dsub_rn(px, qx), dy = __dsub_rn(py, qy);
    const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    return d == d ? d : __longlong_as_double(0x7ff0000000000000LL);
}

// the lane of the smallest (d, lane) of the wavefront, the same value in every lane (mpcg_wave.h)
static_assert(PATH_LANES == WAVE_LANES, "one sample per lane of the wavefront");
__device__ __forceinline__ int path_argmin(double d, int lane) { return wave_argmin(d, lane); }

__global__ __launch_bounds__(64) void path_update_kernel(int n_scenes, int nx, int npar, int i_spline0, int n_seg,
                                                         mpcg_path_table tb, const double* __restrict__ state,
                                                         int* __restrict__ closest_segment,
                                                         double* __restrict__ closest_s,
                                                         double* __restrict__ stage_params,
                                                         unsigned char* __restrict__ reached) {
    __shared__ PathLds L;
    const int s = blockIdx.x;
    if (s >= n_scenes) return;
    const int lane = threadIdx.x;
    // (the entry point checked its host copy of path_of; the clamps keep every index inside the table)
    const int p = min(max(tb.path_of[s], 0), tb.n_paths - 1);
    const int M = tb.max_segments;
    const int m = min(max(tb.n_segments[p], 1), M);
    for (int e = lane; e <= m; e += PATH_LANES) L.knots[e] = tb.knots[(size_t)p * (M + 1) + e];
    for (int e = lane; e < m * 8; e += PATH_LANES) (&L.coef[0][0])[e] = tb.coef[(size_t)p * M * 8 + e];
    const double qx = state[(size_t)s * nx + 0], qy = state[(size_t)s * nx + 1];
    const int c_in = closest_segment[s];
    __syncthreads();
    // every branch below is uniform over the wavefront
    double lo, hi, best_s;
    int round = 0;
    if (c_in < 0) {
        // ---- not initialised: the 64 samples in every segment, one segment per pass
        double bd = __longlong_as_double(0x7ff0000000000000LL);
        int bp = 0;
        for (int j = 0; j < m; ++j) {
            double px, py;
            path_point(L, j, path_sample(L.knots[j], L.knots[j + 1], lane), px, py);
            const double d = path_dist2(px, py, qx, qy);
            if (d < bd) {
                bd = d;
                bp = j;
            }
        }
        const int w = path_argmin(bd, lane);
        const int j = __shfl(bp, w, PATH_LANES);
        best_s = path_sample(L.knots[j], L.knots[j + 1], w);
        // the winner's neighbours in the concatenated sample sequence
        if (w > 0)
            lo = path_sample(L.knots[j], L.knots[j + 1], w - 1);
        else
            lo = j > 0 ? path_sample(L.knots[j - 1], L.knots[j], PATH_LANES - 2) : best_s;
        if (w < PATH_LANES - 1)
            hi = path_sample(L.knots[j], L.knots[j + 1], w + 1);
        else
            hi = j < m - 1 ? path_sample(L.knots[j + 1], L.knots[j + 2], 1) : best_s;
        round = 1;
    } else {
        const int c = min(c_in, m - 1);
        lo = L.knots[max(0, c - 2)];
        hi = L.knots[min(m, c + 3)];
        best_s = lo;
    }
    for (; round < PATH_ROUNDS; ++round) {
        const double si = path_sample(lo, hi, lane);
        double px, py;
        path_point(L, path_segment(L, m, si), si, px, py);
        const int w = path_argmin(path_dist2(px, py, qx, qy), lane);
        best_s = path_sample(lo, hi, w);
        const double nlo = path_sample(lo, hi, max(w - 1, 0)), nhi = path_sample(lo, hi, min(w + 1, PATH_LANES - 1));
        lo = nlo;
        hi = nhi;
    }
    const int c = path_segment(L, m, best_s);
    // the end point getPoint(parameterLength()): the goal test and the window past the end
    double ex, ey;
    path_point(L, m - 1, L.knots[m], ex, ey);
    if (lane == 0) {
        closest_segment[s] = c;
        closest_s[s] = best_s;
        const double dx = __dsub_rn(qx, ex), dy = __dsub_rn(qy, ey);
        reached[s] = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))) < MPCG_PATH_REACHED_RADIUS ? 1 : 0;
    }
    // ---- the window: segment c + i, or the end point held beyond the path
    double* out = stage_params + (size_t)s * npar + i_spline0;
    for (int e = lane; e < 9 * n_seg; e += PATH_LANES) {
        const int i = e / 9, k = e - i * 9;
        const int j = c + i;
        double v;
        if (j < m)
            v = k < 8 ? L.coef[j][k] : L.knots[j];
        else
            v = k == 3 ? ex : (k == 7 ? ey : (k == 8 ? L.knots[m] : 0.0));
        out[e] = v;
    }
}

__global__ __launch_bounds__(64) void path_command_kernel(int n_scenes, int G, int N, int nx, int nu,
                                                          mpcg_path_settings set, const int* __restrict__ best,
                                                          const double* __restrict__ xtraj,
                                                          const double* __restrict__ utraj,
                                                          const double* __restrict__ state,
                                                          const double* __restrict__ closest_s, int spline_slot,
                                                          double* __restrict__ cmd, double* __restrict__ state_next) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_scenes) return;
    const double* x = state + (size_t)s * nx;
    const int b = best[s];
    const double period = __ddiv_rn(1.0, set.control_frequency);
    double v, w;
    if (b >= 0 && b < G) {
        // ros1_jackalsimulator.cpp:183-186: v of the plan's stage 1, w of its stage 0
        const size_t r = (size_t)s * G + b;
        v = xtraj[(r * (N + 1) + 1) * nx + 3];
        w = utraj[r * N * nu + 1];
    } else {
        // :188-201: brake at deceleration_at_infeasible, no rotation
        const double after = __dsub_rn(x[3], __dmul_rn(set.deceleration, period));
        v = after < 0.0 ? 0.0 : after;
        w = 0.0;
    }
    cmd[(size_t)s * 2 + 0] = v;
    cmd[(size_t)s * 2 + 1] = w;
    if (!set.plant) return;
    // the kinematic stand-in for the (external) simulator, one control period
    double* o = state_next + (size_t)s * nx;
    const double psi = x[2];
    for (int k = 4; k < nx; ++k) o[k] = x[k];
    o[0] = __dadd_rn(x[0], __dmul_rn(__dmul_rn(v, cos(psi)), period));
    o[1] = __dadd_rn(x[1], __dmul_rn(__dmul_rn(v, sin(psi)), period));
    o[2] = __dadd_rn(psi, __dmul_rn(w, period));
    o[3] = v;
    if (closest_s && spline_slot >= 0) o[spline_slot] = closest_s[s];
}

}  // namespace mpcg
