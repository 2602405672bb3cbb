// mpcg_road.h — the two road-boundary halfspaces of one control step on the GPU
// (Contouring::constructRoadConstraints, contouring.cpp:183-264) and their placement
// into every planner's lin_constraint rows (linearized_constraints.cpp:107-124, 173-187).
// ABI, the formulas and the reference lines: include/mpcg_road.h; host restatement:
// roads.py (road_halfspaces_host, apply_road_host).
//
// One kernel, one 64-lane workgroup (one wavefront) per scene:
//   stage     the path's knots and coefficients (and, bounds mode, both bounds' coefficients) in LDS
//   cur_s     the `spline` entries of the main solver's warm start: main_warm, or the braking plan
//             of mpcg_braking.h (the function prepare_kernel copies into every planner)
//   rows      lane k-1 forms both rows of stage k in LDS
//   place     all lanes stream the rows into params, 6 consecutive doubles per (planner, stage):
//             rows max_obstacles.. of a guided planner, rows 0, 1 of the non-guided one
// Compiled only into mpcg_road.hip with -ffp-contract=off and written with explicitly rounded
// operations in the host restatement's operation order: every value agrees bit for bit
// (the braking plan's cos / sin do not reach its `spline` entries).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_road.h"  // the public header of the same name
#include "mpcg_braking.h"
#include "mpcg_spline.h"

namespace mpcg {

constexpr int ROAD_MAX_N = MPCG_ROAD_MAX_N;

struct RoadLds {
    PathLds path;
    double left[PATH_MAX_M][8];
    double right[PATH_MAX_M][8];
    double cur_s[ROAD_MAX_N + 1];
    double rows[ROAD_MAX_N][6];   // stage k: row 0 (a1 a2 b), row 1 (a1 a2 b); stage 0 zero
};

// getOrthogonal of one segment's cubics at t: (-dy, dx) / |(dx, dy)|
__device__ __forceinline__ void road_normal(const double* c, double t, double& nx, double& ny) {
    double dx, dy;
    cubic_deriv(c, t, dx, dy);
    const double len = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
    nx = __ddiv_rn(-dy, len);
    ny = __ddiv_rn(dx, len);
}

// n . (p + sign n off)
__device__ __forceinline__ double road_offset_dot(double nx, double ny, double px, double py, double off) {
    const double qx = __dadd_rn(px, __dmul_rn(nx, off)), qy = __dadd_rn(py, __dmul_rn(ny, off));
    return __dadd_rn(__dmul_rn(nx, qx), __dmul_rn(ny, qy));
}

__global__ __launch_bounds__(64) void road_halfspaces_kernel(mpcg_problem pr, int n_scenes, int G, int max_obs,
                                                             mpcg_road_settings set, mpcg_path_table tb,
                                                             mpcg_road_io io, double* __restrict__ params,
                                                             double* __restrict__ halfspaces) {
    __shared__ RoadLds L;
    const int sc = blockIdx.x;
    if (sc >= n_scenes) return;
    const int lane = threadIdx.x;
    const int N = pr.N, npar = pr.npar;
    const bool bounds = set.mode == MPCG_ROAD_BOUNDS;
    // (the entry point checked its host copy of path_of; the clamps keep every index inside the table)
    const int p = min(max(tb.path_of[sc], 0), tb.n_paths - 1);
    const int M = tb.max_segments;
    const int m = min(max(tb.n_segments[p], 1), M);
    for (int e = lane; e <= m; e += 64) L.path.knots[e] = tb.knots[(size_t)p * (M + 1) + e];
    for (int e = lane; e < m * 8; e += 64) (&L.path.coef[0][0])[e] = tb.coef[(size_t)p * M * 8 + e];
    if (bounds) {
        for (int e = lane; e < m * 8; e += 64) {
            (&L.left[0][0])[e] = io.left_coef[(size_t)p * M * 8 + e];
            (&L.right[0][0])[e] = io.right_coef[(size_t)p * M * 8 + e];
        }
    }
    // ---- cur_s(k): the main warm start's `spline` entries, as prepare_kernel sees them
    if (io.main_warm) {
        const double* mw = io.main_warm + (size_t)sc * (N + 1) * MPCG_NVAR;
        if (lane <= N) L.cur_s[lane] = mw[lane * MPCG_NVAR + MPCG_NU + 4];
    } else if (lane == 0) {
        braking_plan(io.state + (size_t)sc * MPCG_NX, io.deceleration, pr.dt, N,
                     [&](int k, double, double, double, double, double, double s) { L.cur_s[k] = s; });
    }
    if (lane < 6) L.rows[0][lane] = 0.0;
    __syncthreads();
    // ---- both rows of stage k, lane k-1 <-> stage k
    if (lane < N - 1) {
        const int k = lane + 1;
        // s inside the path (a NaN goes to the start); the segment that holds it
        const double s = fmin(fmax(L.cur_s[k], L.path.knots[0]), L.path.knots[m]);
        const int j = path_segment(L.path, m, s);
        const double t = __dsub_rn(s, L.path.knots[j]);
        const double r = set.robot_radius;
        double* o = L.rows[k];
        if (!bounds) {
            double px, py, nx, ny;
            cubic_point(L.path.coef[j], t, px, py);
            road_normal(L.path.coef[j], t, nx, ny);
            const double half = __ddiv_rn(set.width, 2.0);
            const double wl = __dsub_rn(__dmul_rn(set.two_way ? 3.0 : 1.0, half), r);
            const double wr = __dsub_rn(half, r);
            o[0] = nx;
            o[1] = ny;
            o[2] = road_offset_dot(nx, ny, px, py, wl);
            o[3] = -nx;
            o[4] = -ny;
            o[5] = -road_offset_dot(nx, ny, px, py, -wr);
        } else {
            double px, py, nx, ny;
            cubic_point(L.left[j], t, px, py);
            road_normal(L.left[j], t, nx, ny);
            o[0] = -nx;
            o[1] = -ny;
            o[2] = -road_offset_dot(nx, ny, px, py, r);
            cubic_point(L.right[j], t, px, py);
            road_normal(L.right[j], t, nx, ny);
            o[3] = nx;
            o[4] = ny;
            o[5] = road_offset_dot(nx, ny, px, py, -r);
        }
    }
    __syncthreads();
    const double* R = &L.rows[0][0];
    if (halfspaces)
        for (int e = lane; e < N * 6; e += 64) halfspaces[(size_t)sc * N * 6 + e] = R[e];
    // ---- placement: 6 consecutive doubles per (planner, stage), stages 1 .. N-1
    for (int g = 0; g < G; ++g) {
        const bool guided = io.guided && io.guided[(size_t)sc * G + g];
        double* P = params + (size_t)(sc * G + g) * N * npar + pr.i_lin0 + 3 * (guided ? max_obs : 0);
        for (int e = lane; e < (N - 1) * 6; e += 64) {
            const int k = 1 + e / 6, c = e - (k - 1) * 6;
            P[(size_t)k * npar + c] = R[k * 6 + c];
        }
    }
}

}  // namespace mpcg
