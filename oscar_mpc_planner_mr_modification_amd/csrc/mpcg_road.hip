// mpcg_road.hip — entry point of the road-boundary halfspaces (include/mpcg_road.h).
// Compiled on its own with -ffp-contract=off, like mpcg_prepare.hip and mpcg_path.hip:
// the kernel must agree with the host restatement (roads.py) bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_road.h"
#include "mpcg_host.h"

using namespace mpcg::host;

extern "C" {

int mpcg_road_halfspaces(const mpcg_problem* pr, int n_scenes, int n_guesses, int max_obstacles,
                         const mpcg_road_settings* set, const mpcg_path_table* tb, const int* path_of_host,
                         const mpcg_road_io* io, double* params, double* halfspaces, void* stream) {
    const char* who = "mpcg_road_halfspaces";
    if (!pr || !set || !io || n_scenes < 0 || n_guesses < 1) return fail(who, "invalid arguments");
    if (pr->nx != MPCG_NX || pr->nu != MPCG_NU) return fail(who, "needs the unicycle's states x y psi v spline");
    if (pr->N < 2 || pr->N > MPCG_ROAD_MAX_N) return fail(who, "needs 2 <= N <= 32");
    if (max_obstacles < 0) return fail(who, "max_obstacles < 0");
    if (pr->n_lin < max_obstacles + 2)
        return fail(who, "needs n_lin >= max_obstacles + 2 (a solver generated with add_halfspaces 2)");
    if (pr->i_lin0 < 0 || pr->i_lin0 + 3 * pr->n_lin > pr->npar)
        return fail(who, "the lin_constraint block lies outside the stage parameters");
    if (int rc = check_path_table(who, tb)) return rc;
    if (set->mode != MPCG_ROAD_CENTERLINE && set->mode != MPCG_ROAD_BOUNDS) return fail(who, "unknown mode");
    if (set->mode == MPCG_ROAD_BOUNDS && (!io->left_coef || !io->right_coef))
        return fail(who, "the bounds mode needs the left and right bound tables");
    if (!path_of_host || !params || (!io->main_warm && !io->state)) return fail(who, "invalid arguments");
    if (int rc = check_path_of(who, path_of_host, n_scenes, tb->n_paths)) return rc;
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::road_halfspaces_kernel, dim3(n_scenes), dim3(64), 0, (hipStream_t)stream, *pr, n_scenes,
                       n_guesses, max_obstacles, *set, *tb, *io, params, halfspaces);
    return launched("road halfspaces");
}

}  // extern "C"
