// mpcg_tracks.hip — entry points of the tracked-object layer (include/mpcg_tracks.h).
// Compiled on its own with -ffp-contract=off, like mpcg_fleet.hip: the kernels must agree
// with the host restatement (tracks.py, obstacles.py) bit for bit wherever no
// cos / sin / atan2 / hypot is involved.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_host.h"
#include "mpcg_tracks.h"

using namespace mpcg::host;

namespace {

int horizon_check(const char* who, const mpcg_problem* pr) {
    if (pr->N < 2 || pr->N > mpcg::TRACKS_MAX_N) return fail(who, "needs 2 <= N <= 32", -2);
    return 0;
}

}  // namespace

extern "C" {

int mpcg_tracks_rows(const mpcg_problem* pr, int n_worlds, int n_objects, const mpcg_track_settings* set,
                     const double* pose, const double* twist, const double* dims, const int* shape, double* rows,
                     double* rows_meta, int* rows_type, int* n_rows, void* stream) {
    const char* who = "mpcg_tracks_rows";
    if (!pr || !set || n_worlds < 0 || !pose || !twist || !dims || !shape || !rows || !rows_meta || !rows_type ||
        !n_rows)
        return fail(who, "invalid arguments");
    if (int rc = horizon_check(who, pr)) return rc;
    if (n_objects < 1 || n_objects > mpcg::TRACKS_MAX_A) return fail(who, "needs 1 <= A <= 32 object slots", -2);
    if (n_worlds == 0) return 0;
    hipLaunchKernelGGL(mpcg::tracks_rows_kernel, dim3(n_worlds), dim3(64), 0, (hipStream_t)stream, n_worlds, n_objects,
                       pr->N, pr->dt, *set, pose, twist, dims, shape, rows, rows_meta, rows_type, n_rows);
    return launched("tracks rows");
}

int mpcg_obstacle_select(const mpcg_problem* pr, int n_scenes, int max_rows, const mpcg_track_settings* set,
                         const double* rows, const double* rows_meta, const int* rows_type, const int* n_rows,
                         const double* state, int propagate, double* obst, double* obst_meta, int* kept,
                         void* stream) {
    const char* who = "mpcg_obstacle_select";
    if (!pr || !set || n_scenes < 0 || !rows || !rows_meta || !rows_type || !n_rows || !state || !obst || !obst_meta)
        return fail(who, "invalid arguments");
    if (int rc = horizon_check(who, pr)) return rc;
    if (pr->nx < 4) return fail(who, "needs nx >= 4 (x, y, psi, v)", -2);
    if (max_rows < 1 || max_rows > mpcg::TRACKS_MAX_ROWS) return fail(who, "needs 1 <= max_rows <= 64", -2);
    if (pr->n_ell < 1 || pr->n_ell > mpcg::TRACKS_MAX_ELL) return fail(who, "needs 1 <= n_ell <= 32", -2);
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::obstacle_select_kernel, dim3(n_scenes), dim3(64), 0, (hipStream_t)stream, n_scenes,
                       max_rows, pr->N, pr->n_ell, pr->nx, pr->dt, *set, rows, rows_meta, rows_type, n_rows, state,
                       propagate, obst, obst_meta, kept);
    return launched("obstacle select");
}

}  // extern "C"
