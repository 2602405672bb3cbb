// mpcg_guidance.hip — entry points of the guidance layer (include/mpcg_guidance.h).
// Compiled on its own with -ffp-contract=off, like mpcg_prepare.hip, mpcg_fleet.hip
// and mpcg_path.hip: the kernels must agree with the host restatement (guidance.py)
// bit for bit once it is given the heading the kernel took.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_guidance.h"
#include "mpcg_host.h"

using namespace mpcg::host;

namespace {

bool null_state(const mpcg_guidance_state* st) {
    return !st || !st->class_traj || !st->class_used || !st->planner_class || !st->selected_topology ||
           !st->prev_was_original;
}

}  // namespace

extern "C" {

int mpcg_guidance_update(const mpcg_problem* pr, int n_scenes, int n_guesses, const mpcg_guidance_settings* set,
                         const double* state, const double* stage_params, const double* obst,
                         const double* obst_meta, const mpcg_guidance_state* st, const mpcg_guidance_out* out,
                         void* stream) {
    const char* who = "mpcg_guidance_update";
    if (!pr || !set || n_scenes < 0 || !state || !stage_params) return fail(who, "invalid arguments");
    if (null_state(st)) return fail(who, "null layer state");
    if (!out || !out->guidance || !out->existing_guidance || !out->previously_selected || !out->consistency_on ||
        !out->topology || !out->enabled || !out->n_found || !out->heading || !out->sig_mask || !out->sig_side ||
        !out->clearance || !out->cost)
        return fail(who, "null output");
    if (pr->n_ell > 0 && (!obst || !obst_meta)) return fail(who, "null obstacle rows");
    if (!(pr->dt > 0.0)) return fail(who, "needs dt > 0");
    if (!(set->robot_radius >= 0.0)) return fail(who, "needs robot_radius >= 0");
    if (pr->nx != 5) return fail(who, "needs nx 5 (x y psi v spline)", -2);
    if (pr->N < 2 || pr->N > MPCG_GUIDANCE_MAX_N) return fail(who, "needs 2 <= N <= 32", -2);
    if (pr->n_ell < 0 || pr->n_ell > MPCG_GUIDANCE_MAX_ELL) return fail(who, "needs n_ell <= 32", -2);
    if (pr->n_seg < 1 || pr->n_seg > MPCG_GUIDANCE_MAX_SEG) return fail(who, "needs 1 <= n_seg <= 8", -2);
    if (n_guesses - 1 < 1 || n_guesses - 1 > MPCG_GUIDANCE_CANDIDATES)
        return fail(who, "needs 1 <= G - 1 <= 8 guided planners", -2);
    if (int rc = check_spline_window(who, pr)) return rc;  // (nx is 5 here)
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::guidance_update_kernel, dim3(n_scenes), dim3(64),
                       mpcg::gd_lds_bytes(pr->N, pr->n_ell, pr->n_seg), (hipStream_t)stream, n_scenes,
                       n_guesses, pr->N, pr->nx, pr->npar, pr->i_spline0, pr->n_seg, pr->n_ell, pr->dt, *set, state,
                       stage_params, obst, obst_meta, *st, *out);
    return launched("guidance update");
}

int mpcg_guidance_mask(int n_scenes, int n_guesses, const unsigned char* enabled, int* exit_code, void* stream) {
    const char* who = "mpcg_guidance_mask";
    if (n_scenes < 0 || n_guesses < 1 || !enabled || !exit_code) return fail(who, "invalid arguments");
    if (n_guesses - 1 > MPCG_GUIDANCE_CANDIDATES) return fail(who, "needs G - 1 <= 8 guided planners", -2);
    if (n_scenes == 0) return 0;
    const int n = n_scenes * n_guesses;
    hipLaunchKernelGGL(mpcg::guidance_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, enabled,
                       exit_code);
    return launched("guidance mask");
}

int mpcg_guidance_select(int n_scenes, int n_guesses, const int* best, const unsigned char* guided,
                         const int* topology, const unsigned char* enabled, const mpcg_guidance_state* st,
                         void* stream) {
    const char* who = "mpcg_guidance_select";
    if (n_scenes < 0 || n_guesses < 1 || !best || !guided || !topology || !enabled)
        return fail(who, "invalid arguments");
    if (null_state(st)) return fail(who, "null layer state");
    if (n_guesses - 1 > MPCG_GUIDANCE_CANDIDATES) return fail(who, "needs G - 1 <= 8 guided planners", -2);
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::guidance_select_kernel, dim3((n_scenes + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       n_scenes, n_guesses, best, guided, topology, enabled, *st);
    return launched("guidance select");
}

}  // extern "C"
