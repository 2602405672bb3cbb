/*
 * mpcg_decomp.h — C ABI of the decomp halfspaces: the static halfspaces
 * DecompConstraints::update builds every control step from the occupied cells of a
 * costmap and the reference path (mpc_planner_modules/src/decomp_constraints.cpp:52-120)
 * and DecompConstraints::setParameters writes into the decomp rows of a solver generated
 * with DecompConstraintModule (decomp.max_constraints rows per stage, the slack rows
 * n_scen of the kernel), for S scenes x G planners.
 * Host restatement: oscar_mpc_planner_mr_modification_amd/decomp.py.
 *
 * DecompUtil is not part of the reference tree.  Its ellipsoid decomposition
 * (EllipsoidDecomp2D / LineSegment; Liu et al., "Planning dynamically feasible
 * trajectories for quadrotors using safe flight corridors in 3-D complex environments",
 * RA-L 2017) is restated here from the published method; parity with the library is
 * unpinned.  The construction below is the specification the kernel and the host
 * restatement both implement, bit for bit.
 *
 * Settings: R = range (decomp.range, the local bounding box (R, R)), max_constraints =
 * pr->n_scen, eps = 1e-10.  A row is (a1, a2, b) at i_scen0 + 3 row: a1 x + a2 y <= b.
 * Per scene:
 *
 *  1 path points   s_0 = state[nx - 1] (`spline`), s_{k+1} = s_k + v_k dt, v_k the `v` entry
 *                  (state slot 3) of stage k of main_warm, or of the braking plan when
 *                  main_warm is NULL (v_0 = state[3], v_{k+1} = max(v_k - |deceleration| dt, 0)).
 *                  q_k = getPoint(s_k), k = 0 .. N-1: s clamped to [knots[0], parameterLength()]
 *                  and evaluated in the segment that holds it, as mpcg_road_halfspaces does.
 *                  Segment k (q_k -> q_{k+1}, k = 0 .. N-2) gives the rows of stage k + 1
 *                  (decomp_constraints.cpp:90-106).
 *  2 dummies       stage 0 and every unused row hold (1, 0, state x + 100)
 *                  (decomp_constraints.h:35, .cpp:60, 108-113)
 *  3 frame         d = q_{k+1} - q_k, L = |d|, e = d / L, h = (e_y, -e_x), g = -h,
 *                  c = (q_k + q_{k+1}) / 2, a = L / 2.  The frame's rotation is built from e
 *                  directly; DecompUtil goes through atan2 / cos / sin, which is equal in exact
 *                  arithmetic and is left out so that no transcendental enters.
 *  4 box filter    (set_obs) an occupied point o is kept iff
 *                     h . (o - (q_k + h R)) <= eps,   -h . (o - (q_k - h R)) <= eps,
 *                     e . (o - (q_{k+1} + e R)) <= eps,  -e . (o - (q_k - e R)) <= eps
 *  5 ellipsoid     (find_ellipsoid, offset 0) semi-axes (a, b), b = a at first;
 *                  u = e . (o - c), w = g . (o - c), dist(o) = sqrt((u / a)^2 + (w / b)^2);
 *                  I = kept points with dist <= 1.  While I is not empty: o* = arg-min of dist over I
 *                  (the lowest point index wins ties, a NaN counts as +inf); if u* < a,
 *                  b = |w*| / sqrt(1 - (u* / a)^2); then I <- {o in I : 1 - dist(o) > eps} with the new b.
 *                  At most the initial |I| passes.
 *  6 polyhedron    (find_polyhedron) Rm = all kept points.  While Rm is not empty: o* = arg-min of dist
 *                  over Rm, same tie rule; n = normalise(e u* / a^2 + g w* / b^2); hyperplane (o*, n);
 *                  Rm <- {o in Rm : n . (o - o*) < 0}.  Only the first max_constraints hyperplanes are
 *                  kept; the loop counts on without forming rows, so n_found is the full count.
 *  7 box           appended in this order: (q_k + h R, h), (q_k - h R, -h), (q_{k+1} + e R, e), (q_k - e R, -e)
 *  8 rows          (LinearConstraint) for a hyperplane (p, n): b = p . n; if n . c - b > 0 both are
 *                  negated.  The first max_constraints of the sequence are written.  At the first row
 *                  that holds a NaN or whose (a1, a2) has a norm below 1e-3 that row and all after it
 *                  become dummies (decomp_constraints.cpp:98-101).
 *  9 IEEE cases    follow from the above with no special code: L = 0 (standing still, braking to a stop,
 *                  s clamped at the path's end) makes e NaN, every row NaN and so every row a dummy; a
 *                  point exactly on the segment gives b = 0 and a NaN normal: the rows from it on are dummies.
 *
 * Out of scope: DecompUtil's offset_x and global bounding box, n_discs > 1.
 *
 * This header is separate from mpcg.h (whose ABI version stays as it is): the function is
 * exported from the same libmpcg.so.  Pointers are device pointers unless stated
 * otherwise, the launch is asynchronous on `stream`; returns 0 on a successful launch,
 * -1 on invalid arguments or a failed launch, with mpcg_last_error().
 */
#ifndef MPCG_DECOMP_H
#define MPCG_DECOMP_H

#include "mpcg.h"
#include "mpcg_path.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCG_DECOMP_MAX_POINTS 1024   /* occupied points per scene */
#define MPCG_DECOMP_MAX_N 32
#define MPCG_DECOMP_MAX_ROWS 64       /* max_constraints the kernel stages per stage */
#define MPCG_DECOMP_EPS 1e-10

typedef struct mpcg_decomp_settings {
    double range;                    /* decomp.range */
    double deceleration;             /* deceleration_at_infeasible: the braking plan without main_warm */
} mpcg_decomp_settings;

typedef struct mpcg_decomp_io {
    const double *state;             /* [S][nx] */
    const double *main_warm;         /* [S][N+1][nu+nx] or NULL: the braking plan */
    const double *occ;               /* [S][P][2]: the occupied points (x, y); entries past n_occ[s] are not read */
    const int *n_occ;                /* [S] */
    int max_points;                  /* P */
} mpcg_decomp_io;

/* The decomp halfspaces of one control step, one launch, before the solve (after mpcg_path_update
 * where the path is tracked on the device):
 *   params      [S*G][N][npar]               in / out: the max_constraints decomp rows of all N stages,
 *                                            every planner of a scene alike; nothing else is touched
 *   halfspaces  [S][N][max_constraints][3]   out, optional (NULL: not written): the same rows per scene
 *   n_found     [S][N]                       out, optional: hyperplanes found including the 4 box rows
 *                                            (the reference's max_decomp_constraints), 0 at stage 0
 *   minor_axis  [S][N]                       out, optional: the ellipsoid's b, 0 at stage 0
 * path_of_host [S] and n_occ_host [S] are the host copies of table->path_of and io->n_occ the entries
 * are checked on.
 * -1: a null pointer, n_scen < 1 or > 64, the decomp block outside npar, nx < 5, N < 2 or N > 32,
 * G < 1, range <= 0, P outside 0 .. 1024 (or P > 0 without occ), an n_occ_host entry outside 0 .. P,
 * a path_of_host entry outside 0 .. P_paths - 1, M > 64 or < 1, no path. */
int mpcg_decomp_halfspaces(const mpcg_problem *pr, int n_scenes, int n_guesses, const mpcg_decomp_settings *set,
                           const mpcg_path_table *table, const int *path_of_host, const mpcg_decomp_io *io,
                           const int *n_occ_host, double *params, double *halfspaces, int *n_found,
                           double *minor_axis, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_DECOMP_H */
