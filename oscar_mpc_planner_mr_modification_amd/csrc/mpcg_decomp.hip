// mpcg_decomp.hip — entry point of the decomp halfspaces (include/mpcg_decomp.h).
// Compiled on its own with -ffp-contract=off, like mpcg_road.hip and mpcg_path.hip:
// the kernel must agree with the host restatement (decomp.py) bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_decomp.h"
#include "mpcg_host.h"

using namespace mpcg::host;

extern "C" {

int mpcg_decomp_halfspaces(const mpcg_problem* pr, int n_scenes, int n_guesses, const mpcg_decomp_settings* set,
                           const mpcg_path_table* tb, const int* path_of_host, const mpcg_decomp_io* io,
                           const int* n_occ_host, double* params, double* halfspaces, int* n_found,
                           double* minor_axis, void* stream) {
    const char* who = "mpcg_decomp_halfspaces";
    if (!pr || !set || !io || !params || n_scenes < 0) return fail(who, "invalid arguments");
    if (n_guesses < 1) return fail(who, "needs at least one planner per scene");
    if (pr->n_scen < 1 || pr->n_scen > MPCG_DECOMP_MAX_ROWS)
        return fail(who, "needs 1 <= max_constraints (n_scen) <= 64");
    if (pr->i_scen0 < 0 || pr->i_scen0 + 3 * pr->n_scen > pr->npar)
        return fail(who, "the decomp block lies outside the stage parameters");
    if (pr->nx < 5 || pr->nu < 0) return fail(who, "needs the states x y psi v .. spline (nx >= 5)");
    if (pr->N < 2 || pr->N > MPCG_DECOMP_MAX_N) return fail(who, "needs 2 <= N <= 32");
    if (!(set->range > 0.0)) return fail(who, "needs range > 0");
    if (io->max_points < 0 || io->max_points > MPCG_DECOMP_MAX_POINTS)
        return fail(who, "needs 0 <= P <= 1024 occupied points per scene");
    if (int rc = check_path_table(who, tb)) return rc;
    if (!path_of_host || !n_occ_host || !io->state || !io->n_occ || (io->max_points > 0 && !io->occ))
        return fail(who, "invalid arguments");
    if (int rc = check_path_of(who, path_of_host, n_scenes, tb->n_paths)) return rc;
    for (int s = 0; s < n_scenes; ++s)
        if (n_occ_host[s] < 0 || n_occ_host[s] > io->max_points)
            return fail(who, "n_occ[" + std::to_string(s) + "] = " + std::to_string(n_occ_host[s]) + " outside 0 .. P");
    if (n_scenes == 0) return 0;
    const size_t dyn = (size_t)3 * io->max_points * sizeof(double);
    hipLaunchKernelGGL(mpcg::decomp_halfspaces_kernel, dim3((unsigned)n_scenes * (pr->N - 1)), dim3(64), dyn,
                       (hipStream_t)stream, *pr, n_scenes, n_guesses, *set, *tb, *io, params, halfspaces, n_found,
                       minor_axis);
    return launched("decomp halfspaces");
}

}  // extern "C"
