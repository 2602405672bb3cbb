/*
 * mpcg_path.h — C ABI of the device-resident reference-path tracking: what
 * Contouring::update and setSplineParameters do once per control step
 * (mpc_planner_modules/src/contouring.cpp:28-50, 96-126: closest point on the
 * path, the window of n_seg spline segments from the closest segment, the
 * `spline` entry of the state), isObjectiveReached (:169-177) and the command
 * the wrapper derives from the winner (mpc_planner_jackalsimulator/src/
 * ros1_jackalsimulator.cpp:181-201), for S scenes that follow P paths.
 * Host restatement: oscar_mpc_planner_mr_modification_amd/paths.py.
 *
 * Path table (built on the host once per path, paths.fit_path / paths.PathTable;
 * RosTools::Spline2D restated, parity unpinned: ros_tools is not part of the
 * reference tree):
 *   coef       [P][M][8]   xa xb xc xd ya yb yc yd of segment j, a cubic .. d constant in the
 *                          local variable s - knots[j]
 *   knots      [P][M+1]    knots[j] the start of segment j, knots[n_segments] = parameterLength();
 *                          non-decreasing, entries past n_segments unused
 *   n_segments [P]         1 <= n_segments[p] <= M <= MPCG_PATH_MAX_SEGMENTS
 *   path_of    [S]         the path of scene s
 *
 * The closest point is the minimiser of |p(s) - q|^2 over a search interval,
 * found by MPCG_PATH_ROUNDS rounds of MPCG_PATH_SAMPLES equispaced samples
 *   s_i = min(lo + ((hi - lo) * i) / 63, hi),  i = 0 .. 63,
 * each evaluated in the segment that holds it (the last j with knots[j] <= s_i), the
 * arg-min taken on (distance^2, i) with the lowest i winning ties (a NaN distance
 * counts as +inf), and the bracket shrunk to the winner's neighbours
 * [s_{max(i-1, 0)}, s_{min(i+1, 63)}].  The result is the last round's winner: an
 * interval W shrinks to W (2/63)^5, below 1e-6 m for W <= 30 m.
 *   closest_segment >= 0:  the interval is knots[max(0, c-2)] .. knots[min(m, c+3)]
 *   closest_segment  < 0:  (after a new path, onDataReceived) the whole path; the first round
 *                          takes the 64 samples in every segment, one segment per pass, the
 *                          arg-min on (distance^2, i) with the earlier pass winning ties, and the
 *                          bracket is the winner's neighbours in the concatenated sample
 *                          sequence; four ordinary rounds follow
 * closest_segment becomes the segment that holds the result (<= m - 1).
 *
 * This header is separate from mpcg.h (whose ABI version stays as it is): the
 * functions are exported from the same libmpcg.so.  Pointers are device
 * pointers unless stated otherwise, launches are asynchronous on `stream`;
 * return 0 on a successful launch, -1 on invalid arguments or a failed
 * launch, with mpcg_last_error().
 */
#ifndef MPCG_PATH_H
#define MPCG_PATH_H

#include "mpcg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCG_PATH_MAX_SEGMENTS 64
#define MPCG_PATH_SAMPLES 64
#define MPCG_PATH_ROUNDS 5
#define MPCG_PATH_REACHED_RADIUS 1.5

typedef struct mpcg_path_table {
    const double *coef, *knots;
    const int *n_segments, *path_of;
    int n_paths;                     /* P */
    int max_segments;                /* M */
} mpcg_path_table;

typedef struct mpcg_path_settings {
    double control_frequency;        /* the control period is 1 / control_frequency */
    double deceleration;             /* deceleration_at_infeasible */
    int plant;                       /* 1: write state_next from the kinematic stand-in plant */
} mpcg_path_settings;

/* The reference-path update of one control step, one launch:
 *   state           [S][nx]   x, y read
 *   closest_segment [S]       in / out, -1: not initialised
 *   closest_s       [S]       out
 *   stage_params    [S][npar] the window written at i_spline0 + 9 i + (xa xb xc xd ya yb yc yd start)
 *                             for i < n_seg: segment closest_segment + i, and past the path's end
 *                             a = b = c = 0, d = the end point getPoint(parameterLength()),
 *                             start = parameterLength() (contouring.cpp:425-444)
 *   reached         [S]       1: |q - getPoint(parameterLength())| < 1.5
 * path_of_host [S] is the host copy of table->path_of the entries are checked on.
 * -1: a null pointer, M > 64 or < 1, P < 1, n_seg < 1, the window outside npar, a path_of_host entry
 * outside 0 .. P - 1. */
int mpcg_path_update(const mpcg_problem *pr, int n_scenes, const mpcg_path_table *table, const int *path_of_host,
                     const double *state, int *closest_segment, double *closest_s, double *stage_params,
                     unsigned char *reached, void *stream);

/* The command of one control step, one launch:
 *   best [S], xtraj [S*G][N+1][nx], utraj [S*G][N][nu], state [S][nx]
 *   cmd  [S][2]   success (0 <= best < G): v of the winner's stage 1, w of its stage 0;
 *                 otherwise max(v - deceleration / control_frequency, 0), 0
 * With set->plant, state_next [S][nx] is the state one control period D = 1 / control_frequency later
 * under a kinematic stand-in for the simulator (which is external to the planner):
 *   x + cmd_v cos(psi) D, y + cmd_v sin(psi) D, psi + cmd_w D, cmd_v, the other entries copied;
 * and, with closest_s [S] and 0 <= spline_slot < nx, its entry spline_slot is closest_s (the `spline`
 * entry Contouring::update leaves in the State for the next step's setXinit).
 * -1: a null pointer, G < 1, control_frequency <= 0, spline_slot >= nx, plant without state_next. */
int mpcg_path_command(const mpcg_problem *pr, int n_scenes, int n_guesses, const mpcg_path_settings *set,
                      const int *best, const double *xtraj, const double *utraj, const double *state,
                      const double *closest_s, int spline_slot, double *cmd, double *state_next, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_PATH_H */
