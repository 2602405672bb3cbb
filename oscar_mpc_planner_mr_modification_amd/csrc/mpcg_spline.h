// mpcg_spline.h — one path of the table of include/mpcg_path.h staged in LDS and its piecewise
// cubic evaluation, shared by the reference-path tracking (mpcg_path.h), the road-boundary
// halfspaces (mpcg_road.h) and the decomp halfspaces (mpcg_decomp.h).  Explicitly rounded operations
// in the host restatements' order (paths.py, roads.py, decomp.py): compiled without contraction, the
// values agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_path.h"

namespace mpcg {

constexpr int PATH_MAX_M = MPCG_PATH_MAX_SEGMENTS;

struct PathLds {
    double knots[PATH_MAX_M + 1];
    double coef[PATH_MAX_M][8];
};

// the segment that holds s: the last j < m with knots[j] <= s (0 before the path, m - 1 beyond it)
__device__ __forceinline__ int path_segment(const PathLds& L, int m, double s) {
    int j = 0;
    for (int k = 1; k < m; ++k) j += L.knots[k] <= s ? 1 : 0;
    return j;
}

// the point (x, y) of one segment's cubics c = (xa xb xc xd ya yb yc yd) at the local parameter t
__device__ __forceinline__ void cubic_point(const double* c, double t, double& x, double& y) {
    x = __dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(c[0], t), c[1]), t), c[2]), t), c[3]);
    y = __dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(c[4], t), c[5]), t), c[6]), t), c[7]);
}

// their derivative (3 a t + 2 b) t + c per axis
__device__ __forceinline__ void cubic_deriv(const double* c, double t, double& dx, double& dy) {
    dx = __dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dmul_rn(3.0, c[0]), t), __dmul_rn(2.0, c[1])), t), c[2]);
    dy = __dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dmul_rn(3.0, c[4]), t), __dmul_rn(2.0, c[5])), t), c[6]);
}

// the point of segment j at s
__device__ __forceinline__ void path_point(const PathLds& L, int j, double s, double& x, double& y) {
    cubic_point(L.coef[j], __dsub_rn(s, L.knots[j]), x, y);
}

}  // namespace mpcg
