// mpcg_host.h — host-side plumbing shared by the entry points of the layers
// (mpcg_fleet.hip, mpcg_path.hip, mpcg_guidance.hip, mpcg_active.hip, mpcg_road.hip, mpcg_decomp.hip,
// mpcg_scenario.hip, mpcg_tracks.hip):
// the error text behind mpcg_last_error() and the argument checks more than one
// entry point makes.  Host code only, internal; no kernel reads it.
//
// Every check returns 0, or the return code with g_err set to "<who>: <what>".
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mpcg_path.h"  // mpcg_problem, mpcg_path_table

namespace mpcg {

extern thread_local std::string g_err;  // defined in mpcg_kernels.hip

namespace host {

inline int fail(const char* who, const std::string& what, int rc = -1) {
    g_err = std::string(who) + ": " + what;
    return rc;
}

inline int hip_fail(const char* who, const char* what, hipError_t e) {
    return fail(who, std::string(what) + ": " + hipGetErrorString(e));
}

// after a kernel launch
inline int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    g_err = std::string(what) + " launch: " + hipGetErrorString(e);
    return -1;
}

inline int check_path_table(const char* who, const mpcg_path_table* tb) {
    if (!tb || !tb->coef || !tb->knots || !tb->n_segments || !tb->path_of) return fail(who, "null path table");
    if (tb->max_segments < 1 || tb->max_segments > MPCG_PATH_MAX_SEGMENTS)
        return fail(who, "needs 1 <= M <= 64 segments per path");
    if (tb->n_paths < 1) return fail(who, "needs at least one path");
    return 0;
}

// path_of_host: the host copy of the table's path_of, one entry per scene
inline int check_path_of(const char* who, const int* path_of_host, int n_scenes, int n_paths) {
    for (int s = 0; s < n_scenes; ++s)
        if (path_of_host[s] < 0 || path_of_host[s] >= n_paths)
            return fail(who, "path_of[" + std::to_string(s) + "] = " + std::to_string(path_of_host[s]) +
                                 " outside the table");
    return 0;
}

// the n_seg segments of 9 entries from i_spline0 (and the states x, y the spline is evaluated at)
inline int check_spline_window(const char* who, const mpcg_problem* pr) {
    if (pr->nx < 2 || pr->i_spline0 < 0 || pr->i_spline0 + 9 * pr->n_seg > pr->npar)
        return fail(who, "the spline window lies outside the stage parameters");
    return 0;
}

}  // namespace host
}  // namespace mpcg
