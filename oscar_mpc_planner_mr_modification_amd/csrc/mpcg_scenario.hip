// mpcg_scenario.hip — entry points of the SH-MPC scenario sampler (include/mpcg_scenario.h).
// Compiled on its own with -ffp-contract=off, like mpcg_prepare.hip and mpcg_decomp.hip:
// the kernels must agree with the host restatement (scenario_sampler.py) bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_scenario.h"
#include "mpcg_host.h"

using namespace mpcg::host;

namespace {

// the model and the sizes the sampler's kernels are written for
int check_model(const char* who, const mpcg_problem* pr) {
    if (pr->n_scen < 1 || pr->i_scen0 < 0 || pr->i_scen0 + 3 * pr->n_scen > pr->npar || pr->nx < 5 ||
        pr->nx > MPCG_MAX_NX || pr->nu != MPCG_NU)
        return fail(who, "needs a model with scenario rows (n_scen >= 1 inside npar, nx 5 .. 6, nu 2)");
    if (pr->N < 2 || pr->N > MPCG_SCENARIO_MAX_N) return fail(who, "needs 2 <= N <= 32");
    if (pr->n_scen > MPCG_SCENARIO_MAX_ROWS) return fail(who, "needs n_scen <= 32");
    return 0;
}

int check_sampler(const char* who, const mpcg_scenario_sample_io* io) {
    if (!io->obst || !io->obst_meta || !io->bank) return fail(who, "invalid arguments");
    if (io->n_obs < 1 || io->n_obs > MPCG_SCENARIO_MAX_OBS) return fail(who, "needs 1 <= n_obs <= 64");
    if (io->n_per < 1 || (long long)io->n_obs * io->n_per > MPCG_SCENARIO_MAX_SAMPLES)
        return fail(who, "needs 1 <= M = n_obs n_per <= 2048");
    if (io->n_batches < 1) return fail(who, "needs n_batches >= 1");
    return 0;
}

}  // namespace

extern "C" {

int mpcg_scenario_sample_prepare(const mpcg_problem* pr, int n_scenes, int n_solvers,
                                 const mpcg_scenario_sample_io* io, double* params, double* warm, double* xinit,
                                 void* stream) {
    const char* who = "mpcg_scenario_sample_prepare";
    if (!pr || !io || n_scenes < 0 || n_solvers < 1 || !params || !warm || !xinit || !io->stage_params || !io->state)
        return fail(who, "invalid arguments");
    if (int rc = check_model(who, pr)) return rc;
    if (int rc = check_sampler(who, io)) return rc;
    if (n_scenes == 0) return 0;
    const int M = io->n_obs * io->n_per;
    auto kern = M <= 64 * 8 ? mpcg::scen::scenario_sample_prepare_kernel<8>
                            : (M <= 64 * 20 ? mpcg::scen::scenario_sample_prepare_kernel<20>
                                            : mpcg::scen::scenario_sample_prepare_kernel<32>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_scenes * n_solvers), dim3(256), 0, (hipStream_t)stream, *pr, n_scenes,
                       n_solvers, *io, params, warm, xinit);
    return launched("scenario sample-prepare");
}

int mpcg_scenario_samples(const mpcg_problem* pr, int n_scenes, int n_solvers, const mpcg_scenario_sample_io* io,
                          double* samples, void* stream) {
    const char* who = "mpcg_scenario_samples";
    if (!pr || !io || n_scenes < 0 || n_solvers < 1 || !samples) return fail(who, "invalid arguments");
    if (pr->N < 2 || pr->N > MPCG_SCENARIO_MAX_N) return fail(who, "needs 2 <= N <= 32");
    if (int rc = check_sampler(who, io)) return rc;
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::scen::scenario_samples_kernel, dim3((unsigned)n_scenes * n_solvers), dim3(256), 0,
                       (hipStream_t)stream, *pr, n_scenes, n_solvers, *io, samples);
    return launched("scenario samples");
}

int mpcg_scenario_advance(const mpcg_problem* pr, int n_scenes, int n_solvers, const mpcg_scenario_step_io* io,
                          double* main_warm_next, double* lam_next, void* stream) {
    const char* who = "mpcg_scenario_advance";
    if (!pr || !io || n_scenes < 0 || n_solvers < 1 || !main_warm_next || !io->best || !io->exit_code || !io->xtraj ||
        !io->utraj || !io->state_next)
        return fail(who, "invalid arguments");
    if (int rc = check_model(who, pr)) return rc;
    if (n_scenes == 0) return 0;
    hipLaunchKernelGGL(mpcg::scen::scenario_advance_kernel, dim3((unsigned)n_scenes), dim3(64), 0, (hipStream_t)stream,
                       *pr, n_scenes, n_solvers, *io, main_warm_next, lam_next);
    return launched("scenario advance");
}

}  // extern "C"
