/*
 * mpcg_active.h — C ABI of the active-solve compaction: solve only the enabled
 * solves of a batch.  With a guidance layer (mpcg_guidance.h) a planner whose index
 * is at least the number of topology classes found is disabled, and the reference
 * skips it inside its fan-out (guidance_constraints.cpp:311-318: `continue` before
 * the solver copy and solve()).  Here the solve kernel is left as it is: a stable
 * compaction of the enabled solves into a dense batch, one ordinary mpcg_solve of
 * that smaller batch, and a scatter that puts the results back:
 *
 *   mpcg_active_plan     enabled [batch] -> slot_of [batch], solve_of [batch], n_active [1]
 *   mpcg_active_gather   the inputs of every enabled solve b -> slot slot_of[b] of the dense buffers
 *   mpcg_solve           batch n_active, on the dense buffers (include/mpcg.h)
 *   mpcg_active_scatter  the outputs of slot slot_of[b] -> solve b; a disabled solve gets the fill below
 *
 * mpcg_solve_active composes the four around a workspace that owns the dense buffers.
 * Host restatement (exact, every copy is bit for bit): oscar_mpc_planner_mr_modification_amd/active.py.
 *
 * The fill of a disabled solve (mpcg_active_scatter), the outputs of a solver that was not run:
 *   exit_code  MPCG_ACTIVE_EXIT_SKIPPED (-100, the value of MPCG_GUIDANCE_EXIT_DISABLED: neither 1 nor any
 *              solver code, so mpcg_select_best_device never selects the solve and mpcg_advance resets its
 *              multipliers, as after mpcg_guidance_mask)
 *   xtraj      the x part of the solve's own warm start, xtraj[k][j] = full->warm[b][k][nu + j], k = 0 .. N
 *   utraj      its u part, utraj[k][j] = full->warm[b][k][j], k = 0 .. N - 1 (finite whenever the warm start
 *              is, so the planner-0 record of mpcg_winner_records_device at best == -1 stays finite)
 *   pobj       +inf
 *   info       0 (MPCG_INFO_STRIDE ints)
 *   lam_out    0
 *   qp_out     a NaN in the first double (the "no QP memory" convention of mpcg_io.qp_in), 0 in the others
 *   stats      NaN (MPCG_STATS_STRIDE doubles)
 *
 * This header is separate from mpcg.h (whose ABI version stays as it is): the
 * functions are exported from the same libmpcg.so.  All pointers are device
 * pointers (n_active_host excepted), every launch is enqueued on `stream`
 * (hipStream_t, NULL = default stream); every call returns 0, or -1 with
 * mpcg_last_error() set.  Block sizes are those of mpcg_io: params [N][npar], warm
 * [N+1][nu+nx], xinit [nx], xtraj [N+1][nx], utraj [N][nu], lam [mpcg_lam_size],
 * qp [mpcg_qp_mem_size], info [MPCG_INFO_STRIDE], stats [MPCG_STATS_STRIDE].
 */
#ifndef MPCG_ACTIVE_H
#define MPCG_ACTIVE_H

#include "mpcg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* exit code of a solve that was skipped: the value of MPCG_GUIDANCE_EXIT_DISABLED */
#define MPCG_ACTIVE_EXIT_SKIPPED (-100)

/* Stable stream compaction of enabled [batch] (a byte per solve, non-zero = enabled):
 *   slot_of [batch]   the number of enabled solves before b, or -1 when enabled[b] == 0
 *   solve_of [batch]  solve_of[slot] = b, ascending, for slot < n_active; -1 from n_active on
 *   n_active [1]      the number of enabled solves
 * One launch of one workgroup.  The order is a function of `enabled` alone (ranks come from wave-wide
 * ballots and a fixed-order sum of the wave totals; no atomic decides a position). */
int mpcg_active_plan(int batch, const unsigned char *enabled, int *slot_of, int *solve_of, int *n_active,
                     void *stream);

/* The inputs of every enabled solve b of `full` (batch solves) to slot slot_of[b] of `dense`:
 * params, warm and xinit, which must be non-NULL in both, and lam_in and qp_in where non-NULL in both.
 * Outputs of the two mpcg_io are not read.  `dense` needs room for as many solves as are enabled (at most
 * batch); a slot outside 0 .. batch - 1 is skipped.  It needs no count on the host. */
int mpcg_active_gather(const mpcg_problem *pr, int batch, const int *slot_of, const mpcg_io *full,
                       const mpcg_io *dense, void *stream);

/* The outputs of slot slot_of[b] of `dense` to solve b of `full`, for every output that is non-NULL in
 * `full` (xtraj, utraj, pobj, exit_code, info, lam_out, qp_out, stats; such an output must be non-NULL in
 * `dense` too); a disabled solve (slot_of[b] < 0) gets the fill stated at the top of this header, which
 * reads full->warm (required with xtraj or utraj). */
int mpcg_active_scatter(const mpcg_problem *pr, int batch, const int *slot_of, const mpcg_io *dense,
                        const mpcg_io *full, void *stream);

/* The dense buffers of up to max_batch solves of `pr` (inputs, outputs, and with_lam / with_qp / with_stats
 * the multiplier blocks, the QP memory and the NLP residuals, in and out), slot_of, solve_of, the device
 * count and one pinned host word.  Lives on the current device, as contexts do.  NULL on failure. */
typedef struct mpcg_active_ws mpcg_active_ws;
mpcg_active_ws *mpcg_active_ws_create(const mpcg_problem *pr, int max_batch, int with_lam, int with_qp,
                                      int with_stats);
void mpcg_active_ws_destroy(mpcg_active_ws *ws);

/* Copies the plan of the workspace's last mpcg_solve_active (slot_of, solve_of [batch]; either may be NULL)
 * into device buffers of the caller, asynchronously on `stream`. */
int mpcg_active_ws_read_plan(const mpcg_active_ws *ws, int batch, int *slot_of, int *solve_of, void *stream);

/* mpcg_solve of the enabled solves of `io` only: plan and gather, one asynchronous 4-byte copy of the count
 * to the workspace's pinned word and a synchronisation of `stream`, mpcg_solve(pr, n_active, dense, stream)
 * (skipped when the count is 0), scatter.  Optional buffers of `io` (lam_in, lam_out, qp_in, qp_out, stats,
 * info) are passed on exactly when they are non-NULL, so the dense launch runs the kernel variant the full
 * launch would; lam / qp / stats need a workspace created with them.  n_active_host (host, may be NULL)
 * receives the count.
 * The one host synchronisation is inherent while the solve kernel takes its batch size by value: the call
 * CANNOT be captured into a graph (it fails on a capturing stream), and it returns with the solve and the
 * scatter still in flight on `stream`. */
int mpcg_solve_active(const mpcg_problem *pr, int batch, const mpcg_io *io, const unsigned char *enabled,
                      mpcg_active_ws *ws, int *n_active_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_ACTIVE_H */
