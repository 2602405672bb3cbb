// mpcg_fleet.hip — entry points of the multi-robot layer (include/mpcg_fleet.h).
// Compiled on its own with -ffp-contract=off, like mpcg_prepare.hip: the
// kernels must agree with the host restatement (fleet.py, obstacles.py)
// bit for bit wherever no cos / sin / hypot is involved.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_fleet.h"
#include "mpcg_host.h"

using namespace mpcg::host;

namespace {

// the limits shared by both entry points; 0, or the return code with g_err set
int fleet_check(const char* who, const mpcg_problem* pr, int F, int R, int A, const mpcg_fleet_settings* set,
                const mpcg_fleet_state* st) {
    if (!pr || !set || !st || F < 0 || A < 0 || !st->sent_plan || !st->sent_time || !st->last_send_time ||
        !st->prev_topology)
        return fail(who, "invalid arguments");
    if (pr->nx != MPCG_NX) return fail(who, "the fleet layer needs the 5-state model", -2);
    if (pr->N < 2 || pr->N > mpcg::FLEET_MAX_N || pr->n_ell < 0 || pr->n_ell > mpcg::FLEET_MAX_ELL || R < 2 ||
        R > mpcg::FLEET_MAX_R || A + R - 1 > mpcg::FLEET_MAX_CAND)
        return fail(who, "needs 2 <= N <= 32, n_ell <= 32, 2 <= R <= 8 and A + R - 1 <= 64", -2);
    return 0;
}

}  // namespace

extern "C" {

int mpcg_fleet_obstacles(const mpcg_problem* pr, int n_fleets, int n_robots, int n_array,
                         const mpcg_fleet_settings* set, const mpcg_fleet_state* st, const double* state,
                         const double* array_obst, const double* array_meta, const int* array_id, double now,
                         double* obst, double* obst_meta, void* stream) {
    if (int rc = fleet_check("mpcg_fleet_obstacles", pr, n_fleets, n_robots, n_array, set, st)) return rc;
    if (!state || (pr->n_ell > 0 && (!obst || !obst_meta)) || (n_array > 0 && (!array_obst || !array_meta)))
        return fail("mpcg_fleet_obstacles", "invalid arguments");
    const int S = n_fleets * n_robots;
    if (S == 0) return 0;
    hipLaunchKernelGGL(mpcg::fleet_shift_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, S, pr->N, pr->dt, *set,
                       *st, now);
    if (int rc = launched("fleet shift")) return rc;
    if (pr->n_ell == 0) return 0;
    hipLaunchKernelGGL(mpcg::fleet_obstacles_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, S, n_robots, n_array,
                       pr->N, pr->n_ell, pr->dt, *set, st->sent_plan, st->sent_time, state, array_obst, array_meta,
                       array_id, obst, obst_meta);
    return launched("fleet obstacles");
}

int mpcg_fleet_publish(const mpcg_problem* pr, int n_fleets, int n_robots, int n_guesses,
                       const mpcg_fleet_settings* set, const mpcg_fleet_state* st, const int* best,
                       const double* xtraj, const double* state, const int* topology, const unsigned char* guided,
                       double now, int* reason, unsigned char* published, void* stream) {
    if (int rc = fleet_check("mpcg_fleet_publish", pr, n_fleets, n_robots, 0, set, st)) return rc;
    if (n_guesses < 1 || !best || !xtraj || !state || !reason || !published)
        return fail("mpcg_fleet_publish", "invalid arguments");
    const int S = n_fleets * n_robots;
    if (S == 0) return 0;
    hipLaunchKernelGGL(mpcg::fleet_publish_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, S, n_guesses, pr->N,
                       pr->dt, *set, *st, best, xtraj, state, topology, guided, now, reason, published);
    return launched("fleet publish");
}

}  // extern "C"
