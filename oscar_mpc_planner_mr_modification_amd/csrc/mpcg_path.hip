// mpcg_path.hip — entry points of the reference-path tracking (include/mpcg_path.h).
// Compiled on its own with -ffp-contract=off, like mpcg_prepare.hip and
// mpcg_fleet.hip: the kernels must agree with the host restatement (paths.py)
// bit for bit wherever no cos / sin is involved.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_path.h"
#include "mpcg_host.h"

using namespace mpcg::host;

extern "C" {

int mpcg_path_update(const mpcg_problem* pr, int n_scenes, const mpcg_path_table* tb, const int* path_of_host,
                     const double* state, int* closest_segment, double* closest_s, double* stage_params,
                     unsigned char* reached, void* stream) {
    const char* who = "mpcg_path_update";
    if (!pr || n_scenes < 0) return fail(who, "invalid arguments");
    if (int rc = check_path_table(who, tb)) return rc;
    if (pr->n_seg < 1) return fail(who, "needs n_seg >= 1");
    if (int rc = check_spline_window(who, pr)) return rc;
    if (!path_of_host || !state || !closest_segment || !closest_s || !stage_params || !reached)
        return fail(who, "invalid arguments");
    if (int rc = check_path_of(who, path_of_host, n_scenes, tb->n_paths)) return rc;
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::path_update_kernel, dim3(n_scenes), dim3(64), 0, (hipStream_t)stream, n_scenes, pr->nx,
                       pr->npar, pr->i_spline0, pr->n_seg, *tb, state, closest_segment, closest_s, stage_params,
                       reached);
    return launched("path update");
}

int mpcg_path_command(const mpcg_problem* pr, int n_scenes, int n_guesses, const mpcg_path_settings* set,
                      const int* best, const double* xtraj, const double* utraj, const double* state,
                      const double* closest_s, int spline_slot, double* cmd, double* state_next, void* stream) {
    const char* who = "mpcg_path_command";
    if (!pr || !set || n_scenes < 0 || n_guesses < 1 || !best || !xtraj || !utraj || !state || !cmd)
        return fail(who, "invalid arguments");
    if (pr->nx < 4 || pr->nu < 2 || pr->N < 1) return fail(who, "needs the states x y psi v and the inputs a w");
    if (!(set->control_frequency > 0.0)) return fail(who, "needs control_frequency > 0");
    if (spline_slot >= pr->nx) return fail(who, "spline_slot outside the state");
    if (set->plant && !state_next) return fail(who, "the plant needs state_next");
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::path_command_kernel, dim3((n_scenes + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       n_scenes, n_guesses, pr->N, pr->nx, pr->nu, *set, best, xtraj, utraj, state, closest_s,
                       spline_slot, cmd, state_next);
    return launched("path command");
}

}  // extern "C"
