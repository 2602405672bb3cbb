// mpcg_braking.h — Solver::initializeWithBraking (acados_solver_interface.cpp:303-342) as one
// device function: the main solver's warm start when no previous solution exists.  Shared by
// prepare_kernel (mpcg_prepare.h), which copies the plan into every planner, and
// road_halfspaces_kernel (mpcg_road.h), which reads its `spline` entries, so that both see the
// same bits.  Explicitly rounded operations in the host restatement's order (producers.py).
#pragma once
#include <hip/hip_runtime.h>

namespace mpcg {

// put(k, a, x, y, psi, v, s) for the stages k = 0 .. N of the plan from state st = (x y psi v s)
template <class F>
__device__ __forceinline__ void braking_plan(const double* st, double deceleration, double dt, int N, F&& put) {
    double x = st[0], y = st[1], psi = st[2], v = st[3], s = st[4];
    const double a = -fabs(deceleration);
    const double c = cos(psi), sn = sin(psi);
    put(0, a, x, y, psi, v, s);
    for (int k = 1; k <= N; ++k) {
        x = __dadd_rn(x, __dmul_rn(__dmul_rn(v, dt), c));
        y = __dadd_rn(y, __dmul_rn(__dmul_rn(v, dt), sn));
        s = __dadd_rn(s, __dmul_rn(v, dt));
        v = fmax(__dadd_rn(v, __dmul_rn(a, dt)), 0.0);
        put(k, a, x, y, psi, v, s);
    }
}

}  // namespace mpcg
