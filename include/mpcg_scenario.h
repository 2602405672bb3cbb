/*
 * mpcg_scenario.h — C ABI of the SH-MPC scenario sampler: the obstacle samples every parallel
 * solver draws from the uncertain predictions at every control step
 * (ScenarioConstraints::onDataReceived -> GetSampler().IntegrateAndTranslateToMeanAndVariance(
 * data.dynamic_obstacles, dt), scenario_constraints.cpp:110-130), fused with their reduction to the
 * scenario halfspaces (mpcg_prepare_scenario, include/mpcg.h), and the bookkeeping between two
 * SH-MPC control steps, for S scenes x P parallel solvers.
 * Host restatement: oscar_mpc_planner_mr_modification_amd/scenario_sampler.py.
 *
 * `scenario_module` is not part of the reference tree.  The sampler restates its published scheme:
 * a pre-drawn bank of standard-normal samples, scaled by each stage's covariance and translated to
 * the mean.  PARITY UNPINNED, for the sampler as for the reduction of the samples to halfspaces
 * (include/mpcg.h, mpcg_scenario_io).  The construction below is the specification the kernels and
 * the host restatement both implement.
 *
 * Inputs (device pointers):
 *   obst      [S][n_obs][N][5]       x y angle major minor, the buffer of mpcg_scene_io: solver stage
 *                                    k >= 1 reads prediction step k - 1 (ellipsoid_constraints.cpp:66-70,
 *                                    prepare_kernel)
 *   obst_meta [S][n_obs][2]          meta[0] the obstacle's radius; meta[1] (chi) is not read
 *   bank      [n_batches][n_per][2]  standard-normal pairs, drawn and uploaded once by the caller
 *                                    (numpy.random.default_rng(seed).normal); M = n_obs n_per <= 2048
 *   batch_idx [S*P][n_obs] int32     optional: the bank batch of copy sol = scene P + p for obstacle j,
 *                                    each entry in 0 .. n_batches - 1 (device data: an entry outside is
 *                                    clamped to the range)
 *   seed, draw                       without batch_idx the batch is
 *                                        mix(seed, draw, sol n_obs + j) mod n_batches,
 *                                    `draw` a step counter the caller advances
 *   robot_radius, deceleration, stage_params, state, main_warm: as in mpcg_scenario_io
 *
 * mix, on 64-bit unsigned integers with wrapping arithmetic (a splitmix64 finaliser):
 *     x  = (seed ^ (draw * 0x9E3779B97F4A7C15)) + index * 0xD1B54A32D192ED03
 *     x  = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9
 *     x  = (x ^ (x >> 27)) * 0x94D049BB133111EB
 *     mix = x ^ (x >> 31)
 * Integer operations only: a restatement that masks to 64 bits equals it bit for bit.
 *
 * Sample i of obstacle j at stage k >= 1, (mx, my, angle, major, minor) = obst[sc][j][k-1],
 * z = bank[batch][i]:
 *     ex = major z0,  ey = minor z1
 *     (c, s) = (1, 0) when angle == 0.0, else (cos angle, sin angle)
 *     q = (mx + (c ex - s ey), my + (s ex + c ey))
 * every operation rounded on its own, in this order (no fused multiply-add).  With angle == 0 no
 * transcendental enters and device and host agree bit for bit; otherwise cos / sin may differ in
 * the last place between the device's and the host's library.  The sample's index within the stage is
 * m = j n_per + i, the order of the tensor of mpcg_scenario_io, so ties between equal distances go to
 * the lower index as there.  z does not depend on the stage: the samples of a copy are
 * time-correlated through the shared z, the marginal of every stage is N(mean_k, Sigma_k).
 *
 * Row of a picked sample (the n_scen samples closest to p_k, the warm start's position at stage k,
 * closest first):  n = (q - p_k) / max(|q - p_k|, 1e-9),  b = n . q - (robot_radius + radius_j).
 * Stage 0 rows are (0, 0, 100); rows past M are zero.  This is mpcg_prepare_scenario's reduction with
 * the radius taken per obstacle.
 *
 * A deterministic obstacle (major = minor = 0) has n_per coincident samples at its mean, so its rows
 * repeat.  The reference refuses such predictions under SH-MPC (scenario_constraints.cpp:119,
 * 149-153); here it is defined behaviour with no special case: equal distances are picked in index
 * order.
 *
 * Kernel of mpcg_scenario_sample_prepare: one 256-thread workgroup per (scene, copy), 39,744 bytes of
 * LDS per workgroup (the warm start, the picked rows, the copy's batch and radius per obstacle and each
 * wave's stage constants of up to MPCG_SCENARIO_MAX_OBS obstacles); the samples live in registers only.
 *
 * Out of scope: independent draws per stage, multi-modal predictions, n_discs > 1.
 *
 * This header is separate from mpcg.h (whose ABI version stays as it is): the functions are exported
 * from the same libmpcg.so.  Pointers are device pointers, the launches are asynchronous on `stream`;
 * every function returns 0 on a successful launch, -1 on invalid arguments or a failed launch, with
 * mpcg_last_error().
 */
#ifndef MPCG_SCENARIO_H
#define MPCG_SCENARIO_H

#include "mpcg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCG_SCENARIO_MAX_SAMPLES 2048   /* M = n_obs n_per */
#define MPCG_SCENARIO_MAX_OBS 64         /* obstacles per scene */
#define MPCG_SCENARIO_MAX_N 32
#define MPCG_SCENARIO_MAX_ROWS 32        /* n_scen */

typedef struct mpcg_scenario_sample_io {
    const double *stage_params;      /* [S][npar] */
    const double *state;             /* [S][nx] */
    const double *main_warm;         /* [S][N+1][nu+nx] or NULL: the braking plan */
    const double *obst;              /* [S][n_obs][N][5] */
    const double *obst_meta;         /* [S][n_obs][2] */
    const double *bank;              /* [n_batches][n_per][2] */
    const int *batch_idx;            /* [S*P][n_obs] or NULL: derived from seed and draw */
    int n_obs, n_per, n_batches;
    unsigned long long seed, draw;
    double robot_radius;
    double deceleration;             /* deceleration_at_infeasible (braking plan) */
} mpcg_scenario_sample_io;

/* Inputs of mpcg_scenario_advance (step t):
 *   best [S]                 mpcg_select_lowest_cost_device's pick, -1: no copy succeeded
 *   exit_code [S*P], xtraj [S*P][N+1][nx], utraj [S*P][N][nu]   the solves of step t
 *   lam_out [S*P][N][nx+nh]  multipliers after the solves, or NULL
 *   state_next [S][nx]       ego state at step t + 1 */
typedef struct mpcg_scenario_step_io {
    const int *best, *exit_code;
    const double *xtraj, *utraj, *lam_out, *state_next;
    double deceleration;
} mpcg_scenario_step_io;

/* Sample and reduce in one launch: what mpcg_prepare_scenario produces (params [S*P][N][npar], warm
 * [S*P][N+1][nu+nx], xinit [S*P][nx]) from the predictions; no sample is stored to global memory.
 * -1: a null pointer, a model without scenario rows (n_scen < 1, the block outside npar, nx outside 5 .. 6),
 * N < 2 or > 32, n_scen > 32, n_obs outside 1 .. 64, n_per < 1, M > 2048, n_batches < 1, P < 1. */
int mpcg_scenario_sample_prepare(const mpcg_problem *pr, int n_scenes, int n_solvers,
                                 const mpcg_scenario_sample_io *io, double *params, double *warm, double *xinit,
                                 void *stream);

/* The sample tensor [S*P][N][M][2] of mpcg_scenario_io (stage 0: the stage-1 values), for tests, recordings
 * and visualisation; not on the control loop's path.  stage_params, state and main_warm are not read. */
int mpcg_scenario_samples(const mpcg_problem *pr, int n_scenes, int n_solvers, const mpcg_scenario_sample_io *io,
                          double *samples, void *stream);

/* Between two SH-MPC control steps, on the model with the slack state:
 *   main_warm_next [S][N+1][nu+nx]  best >= 0: Solver::initializeWarmstart(state_next, true) of the winner's
 *                                   output, [state, out_2 .. out_{N-1}, out_{N-1}, out_{N-1}]
 *                                   (acados_solver_interface.cpp:344-364), every state including the slack:
 *                                   stage 0 takes the state's; stage 0's inputs are out_1's (the choice of
 *                                   mpcg_advance).  Otherwise Solver::initializeWithBraking(state_next), the
 *                                   slack and every entry it does not write 0.
 *   lam_next [S*P][N][nx+nh]        optional: each copy's lam_out when its exit code is 1, zero otherwise
 *                                   (Solver_acados_reset), mpcg_lam_size(pr) doubles per copy */
int mpcg_scenario_advance(const mpcg_problem *pr, int n_scenes, int n_solvers, const mpcg_scenario_step_io *io,
                          double *main_warm_next, double *lam_next, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_SCENARIO_H */
