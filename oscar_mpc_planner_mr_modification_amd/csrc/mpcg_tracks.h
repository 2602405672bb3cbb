// mpcg_tracks.h — the tracked-object layer of one control step on the GPU: constant-velocity
// predictions of the tracked objects, and their reduction to the n_ell obstacle rows of a scene.
// ABI, specification and the reference lines: include/mpcg_tracks.h; host restatement: tracks.py
// (over obstacles.py).
//
// Two kernels, one 64-lane workgroup per world / scene, values staged in LDS and streamed out
// with coalesced stores (the form of mpcg_fleet.h):
//   tracks_rows_kernel      per world: lane a parses object a (global twist, 0 / 1 / 2 discs); the row
//                           offset of every object is the wave prefix sum of the disc counts (two
//                           ballots and mbcnt); then all lanes stream the n_rows N 5 values
//   obstacle_select_kernel  per scene: lane c scores candidate c, stable rank by counting over LDS
//                           (the keep-closest / pad rule of fleet_obstacles_kernel, restated here so
//                           that mpcg_fleet.h keeps its bits); lane j owns output row j's semi-axes: the
//                           dummy's sigma table and the second propagation pass are a serial
//                           recurrence over k on that lane
// Compiled only into mpcg_tracks.hip with -ffp-contract=off and written with explicitly rounded
// operations in the host restatement's operation order: every value that does not pass through
// cos / sin / atan2 / hypot agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_tracks.h"  // the public header of the same name

namespace mpcg {

constexpr int TRACKS_MAX_N = MPCG_TRACKS_MAX_N;
constexpr int TRACKS_MAX_A = MPCG_TRACKS_MAX_OBJECTS;
constexpr int TRACKS_MAX_ROWS = MPCG_TRACKS_MAX_ROWS;
constexpr int TRACKS_MAX_ELL = MPCG_TRACKS_MAX_ELL;
constexpr int TRACKS_DUMMY = -1;      // source of an output row: a candidate index, or this
constexpr int TRACKS_GAUSSIAN = 1;    // PredictionType (data_types.h:35-41)

constexpr double TRACKS_HALF_PI = 1.5707963267948966;
constexpr double TRACKS_SQRT2 = 1.4142135623730951;
constexpr double TRACKS_NOISE = 0.3;  // getConstantVelocityPrediction
constexpr double TRACKS_FAR = 100.0;  // FAR_AWAY_POSITION, getDummyObstacle

// one step of propagatePredictionUncertainty: sqrt(run^2 + (sigma dt)^2)
__device__ __forceinline__ double tracks_propagate(double run, double sigma, double dt) {
    const double sd = __dmul_rn(sigma, dt);
    return __dsqrt_rn(__dadd_rn(__dmul_rn(run, run), __dmul_rn(sd, sd)));
}

// the number of set bits of `mask` below this lane
__device__ __forceinline__ int tracks_count_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// ---------------------------------------------------------------- predictions of the tracked objects
struct TracksDisc {
    double x, y, gdx, gdy, radius;   // position, global twist times dt
};

__global__ __launch_bounds__(64) void tracks_rows_kernel(int n_worlds, int A, int N, double dt, mpcg_track_settings set,
                                                         const double* __restrict__ pose,
                                                         const double* __restrict__ twist,
                                                         const double* __restrict__ dims,
                                                         const int* __restrict__ shape, double* __restrict__ rows,
                                                         double* __restrict__ rows_meta, int* __restrict__ rows_type,
                                                         int* __restrict__ n_rows) {
    __shared__ TracksDisc D[TRACKS_MAX_ROWS];
    __shared__ double sigma[TRACKS_MAX_N];
    const int w = blockIdx.x;
    if (w >= n_worlds) return;
    const int lane = threadIdx.x;
    const int C = 2 * A;
    // ---- lane a: object a
    int count = 0;
    TracksDisc d0 = {0.0, 0.0, 0.0, 0.0, 0.0}, d1 = d0;
    if (lane < A) {
        const size_t o = (size_t)w * A + lane;
        const int sh = shape[o];
        if (sh == MPCG_TRACK_UNSEEN) {
            count = 1;
            d0.x = d0.y = TRACKS_FAR;
            d0.radius = set.obstacle_radius;
        } else if (sh == MPCG_TRACK_DISC || sh == MPCG_TRACK_CYLINDER || sh == MPCG_TRACK_BOX) {
            const double x = pose[o * 3 + 0], y = pose[o * 3 + 1], yaw = pose[o * 3 + 2];
            const double tx = twist[o * 2 + 0], ty = twist[o * 2 + 1];
            const double m0 = dims[o * 2 + 0], m1 = dims[o * 2 + 1];
            double c = 1.0, s = 0.0;
            if (yaw != 0.0) {
                c = cos(yaw);
                s = sin(yaw);
            }
            const double gx = __dsub_rn(__dmul_rn(c, tx), __dmul_rn(s, ty));
            const double gy = __dadd_rn(__dmul_rn(s, tx), __dmul_rn(c, ty));
            count = 1;
            d0.x = x;
            d0.y = y;
            d0.gdx = __dmul_rn(gx, dt);
            d0.gdy = __dmul_rn(gy, dt);
            if (sh == MPCG_TRACK_DISC) {
                d0.radius = set.obstacle_radius;
            } else if (sh == MPCG_TRACK_CYLINDER) {
                d0.radius = m1;
            } else if (m0 == m1) {
                d0.radius = __dmul_rn(TRACKS_SQRT2, m0);
            } else {
                // two discs along the object's long axis (parseObstacle)
                const double vel = __dsqrt_rn(__dadd_rn(__dmul_rn(tx, tx), __dmul_rn(ty, ty)));
                const double angle = vel < 0.01 ? yaw : __dadd_rn(__dadd_rn(yaw, atan2(ty, tx)), TRACKS_HALF_PI);
                const double b = __dsub_rn(angle, TRACKS_HALF_PI);
                double cb = 1.0, sb = 0.0;
                if (b != 0.0) {
                    cb = cos(b);
                    sb = sin(b);
                }
                const double small = m0 < m1 ? m0 : m1, large = m0 < m1 ? m1 : m0;
                const double ox = __ddiv_rn(__dmul_rn(cb, large), 2.0), oy = __ddiv_rn(__dmul_rn(sb, large), 2.0);
                count = 2;
                d1 = d0;
                d0.x = __dadd_rn(x, ox);
                d0.y = __dadd_rn(y, oy);
                d1.x = __dsub_rn(x, ox);
                d1.y = __dsub_rn(y, oy);
                d0.radius = d1.radius = __dadd_rn(__dmul_rn(TRACKS_SQRT2, small), 0.05);
            }
        }
    }
    // ---- row offset of every object: the exclusive prefix sum of count over the wave.  count is 0, 1 or
    // 2, so it is the number of lanes below with count >= 1 plus the number with count == 2.
    const unsigned long long has = __ballot(count >= 1), two = __ballot(count == 2);
    const int offset = tracks_count_below(has) + tracks_count_below(two);
    const int n = __popcll(has) + __popcll(two);   // <= 2 A = C <= TRACKS_MAX_ROWS, uniform
    if (count >= 1) D[offset] = d0;
    if (count == 2) D[offset + 1] = d1;
    if (set.probabilistic && lane == 0) {
        double run = 0.0;
        for (int k = 0; k < N; ++k) {
            run = tracks_propagate(run, TRACKS_NOISE, dt);
            sigma[k] = run;
        }
    }
    __syncthreads();
    // ---- rows out
    double* rw = rows + (size_t)w * C * N * 5;
    for (int e = lane; e < n * N * 5; e += 64) {
        const int j = e / (N * 5), rem = e - j * (N * 5);
        const int k = rem / 5, c = rem - k * 5;
        double v;
        if (c == 0)
            v = __dadd_rn(D[j].x, __dmul_rn(D[j].gdx, (double)k));
        else if (c == 1)
            v = __dadd_rn(D[j].y, __dmul_rn(D[j].gdy, (double)k));
        else
            v = (c == 2 || !set.probabilistic) ? 0.0 : sigma[k];
        rw[e] = v;
    }
    for (int j = lane; j < n; j += 64) {
        double* m = rows_meta + ((size_t)w * C + j) * 2;
        m[0] = D[j].radius;
        m[1] = set.probabilistic ? set.chi_gaussian : 1.0;
        rows_type[(size_t)w * C + j] = set.probabilistic ? TRACKS_GAUSSIAN : 0;
    }
    if (lane == 0) n_rows[w] = n;
}

// ---------------------------------------------------------------- keep the closest / pad, second pass
struct TracksSelectLds {
    double sig[TRACKS_MAX_N][TRACKS_MAX_ELL][2];   // semi-axes of output row j at step k: [k][j]
    double score[TRACKS_MAX_ROWS];
    int slot[TRACKS_MAX_ELL];                      // source of output row j
    int gauss[TRACKS_MAX_ELL];                     // whether output row j is GAUSSIAN
};

__global__ __launch_bounds__(64) void obstacle_select_kernel(int n_scenes, int max_rows, int N, int NE, int nx,
                                                             double dt, mpcg_track_settings set,
                                                             const double* __restrict__ rows,
                                                             const double* __restrict__ rows_meta,
                                                             const int* __restrict__ rows_type,
                                                             const int* __restrict__ n_rows,
                                                             const double* __restrict__ state, int propagate,
                                                             double* __restrict__ obst, double* __restrict__ obst_meta,
                                                             int* __restrict__ kept) {
    __shared__ TracksSelectLds L;
    const int s = blockIdx.x;
    if (s >= n_scenes) return;
    const int lane = threadIdx.x;
    const double* st = state + (size_t)s * nx;
    const double x0 = st[0], y0 = st[1];
    int n = n_rows[s];
    n = n < 0 ? 0 : (n > max_rows ? max_rows : n);   // <= TRACKS_MAX_ROWS = 64 lanes
    const double* rw = rows + (size_t)s * max_rows * N * 5;
    if (n > NE) {
        // ---- ensureObstacleSize, more than n_ell: the n_ell smallest of min_k (k + 1) 0.6 |p_k - ego_k|
        // along a constant-velocity roll-out of the ego state; stable (ties: lower candidate index)
        if (lane < n) {
            const double dirx = cos(st[2]), diry = sin(st[2]), v = st[3];
            double best = 1e5;
            for (int k = 0; k < N; ++k) {
                const double* p = rw + ((size_t)lane * N + k) * 5;
                const double vk = __dmul_rn(v, (double)k);
                const double ex = __dadd_rn(x0, __dmul_rn(vk, dirx)), ey = __dadd_rn(y0, __dmul_rn(vk, diry));
                const double d = __dmul_rn(__dmul_rn((double)(k + 1), 0.6), hypot(__dsub_rn(p[0], ex), __dsub_rn(p[1], ey)));
                if (d < best) best = d;
            }
            L.score[lane] = best;   // never NaN: the ranks below are a permutation of 0..n-1
        }
        __syncthreads();
        if (lane < n) {
            const double mine = L.score[lane];
            int rank = 0;
            for (int c = 0; c < n; ++c) {
                const double o = L.score[c];
                rank += (o < mine || (o == mine && c < lane)) ? 1 : 0;
            }
            if (rank < NE) L.slot[rank] = lane;
        }
    } else if (lane < NE) {
        L.slot[lane] = lane < n ? lane : TRACKS_DUMMY;
    }
    __syncthreads();
    // ---- lane j: the semi-axes of output row j (the dummy's sigma table, the second pass)
    if (lane < NE) {
        const int src = L.slot[lane];
        const bool dummy = src == TRACKS_DUMMY;
        const bool gauss = dummy ? set.probabilistic != 0 : rows_type[(size_t)s * max_rows + src] == TRACKS_GAUSSIAN;
        L.gauss[lane] = gauss ? 1 : 0;
        if (gauss) {
            double once = 0.0, major = 0.0, minor = 0.0;
            for (int k = 0; k < N; ++k) {
                double a, b;
                if (dummy) {
                    once = tracks_propagate(once, TRACKS_NOISE, dt);
                    a = b = once;
                } else {
                    const double* p = rw + ((size_t)src * N + k) * 5;
                    a = p[3];
                    b = p[4];
                }
                if (propagate) {
                    major = tracks_propagate(major, a, dt);
                    minor = tracks_propagate(minor, b, dt);
                    a = major;
                    b = minor;
                }
                L.sig[k][lane][0] = a;
                L.sig[k][lane][1] = b;
            }
        }
        double* m = obst_meta + ((size_t)s * NE + lane) * 2;
        m[0] = dummy ? 0.0 : rows_meta[((size_t)s * max_rows + src) * 2 + 0];
        m[1] = !gauss ? 1.0 : (dummy ? set.chi_gaussian : rows_meta[((size_t)s * max_rows + src) * 2 + 1]);
        if (kept) kept[(size_t)s * NE + lane] = src;
    }
    __syncthreads();
    // ---- rows out (EllipsoidConstraints::setParameters layout): x y angle major minor
    double* ob = obst + (size_t)s * NE * N * 5;
    const double dx = __dadd_rn(x0, TRACKS_FAR), dy = __dadd_rn(y0, TRACKS_FAR);
    for (int e = lane; e < NE * N * 5; e += 64) {
        const int j = e / (N * 5), rem = e - j * (N * 5);
        const int k = rem / 5, c = rem - k * 5;
        const int src = L.slot[j];
        double v;
        if (c >= 3)
            v = L.gauss[j] ? L.sig[k][j][c - 3] : 0.0;
        else if (src == TRACKS_DUMMY)
            v = c == 0 ? dx : (c == 1 ? dy : 0.0);
        else
            v = rw[((size_t)src * N + k) * 5 + c];
        ob[e] = v;
    }
}

}  // namespace mpcg
