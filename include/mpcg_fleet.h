/*
 * mpcg_fleet.h — C ABI of the device-resident multi-robot layer: F fleets
 * (independent worlds) x R robots, robot r of fleet f being planner scene
 * s = f * R + r of a batch of S = F * R scenes (mpcg_prepare / mpcg_solve /
 * mpcg_select_best_device / mpcg_advance, mpcg.h).  The winners of step t
 * become the other robots' obstacle predictions of step t + 1, and a robot
 * re-sends its plan only when one of the reference's triggers fires.
 *
 * Restated from JulesJackalPlanner (mpc_planner_jackalsimulator/src/jules_ros1_jackalplanner.cpp:
 * prepareObstacleData, trajectoryCallback, publishDirectTrajectory, shouldCommunicate),
 * mpc_planner_communication/src/communication_triggers.cpp, MultiRobot::* and
 * ensureObstacleSize in mpc_planner/src/data_preparation.cpp and
 * Trajectory::interpolateTrajectoryByElapsedTime (mpc_planner_types/src/data_types.cpp:257-429).
 * Host restatement: oscar_mpc_planner_mr_modification_amd/fleet.py and obstacles.py.
 *
 * All robots of all fleets step in lockstep at the same time `now` (seconds);
 * a plan published at step t is seen by the others at step t + 1.  Reception
 * and publication therefore coincide, and one copy per sender is both what
 * the receivers hold of that sender and the sender's own
 * last_communicated_trajectory.
 *
 * This header is separate from mpcg.h (whose ABI version stays as it is): the
 * functions are exported from the same libmpcg.so.  Pointers are device
 * pointers, launches are asynchronous on `stream`; return 0 on a successful
 * launch, -1 on invalid arguments or a failed launch, -2 on a shape outside the
 * kernels' limits, with mpcg_last_error().
 */
#ifndef MPCG_FLEET_H
#define MPCG_FLEET_H

#include "mpcg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mpcg_fleet_publish: reason [S] (CommunicationTriggerReason, communication_triggers.h) */
#define MPCG_FLEET_NO_COMMUNICATION 0
#define MPCG_FLEET_INFEASIBLE 1
#define MPCG_FLEET_TOPOLOGY_CHANGE 3
#define MPCG_FLEET_GEOMETRIC 4
#define MPCG_FLEET_TIME 5
#define MPCG_FLEET_NON_GUIDED_HOMOLOGY_FAIL 6

typedef struct mpcg_fleet_settings {
    /* time shift of a received plan */
    double control_frequency;        /* plans younger than 1 / control_frequency are left as they are */
    double v_max, w_max;             /* robot_max_velocity / robot_max_angular_velocity of the extrapolation */
    /* obstacle list */
    double robot_obstacle_radius;    /* radius of another robot as an obstacle */
    int probabilistic;               /* probabilistic.enable: the dummies are GAUSSIAN */
    double chi_gaussian;             /* chi of a GAUSSIAN obstacle (ExponentialQuantile(0.5, 1 - risk)) */
    /* communication triggers (CONFIG["JULES"]) */
    int communicate_on_topology_switch_only;   /* 0: every robot publishes every step, reason 0 */
    int n_paths;                     /* the non-guided planner's topology id is 2 * n_paths */
    double max_geometric_deviation, heartbeat_time;
    double deceleration;             /* deceleration_at_infeasible (the braking plan of a failed step) */
} mpcg_fleet_settings;

/* Per-sender state, sender q of fleet f at index f * R + q:
 *   sent_plan      [F][R][N][3]  x y psi of the last published plan, shifted to sent_time
 *   sent_time      [F][R]        NaN: nothing received yet (not in _validated_trajectory_robots)
 *   last_send_time [F][R]        NaN: never sent (ros::Time(0))
 *   prev_topology  [F][R]        the topology followed in the previous step, initially -1 */
typedef struct mpcg_fleet_state {
    double *sent_plan, *sent_time, *last_send_time;
    int *prev_topology;
} mpcg_fleet_state;

/* The obstacle lists of step `now` for every robot, two launches on `stream`:
 * shift every sender's plan to `now` in place (sent_time = now exactly when it was
 * shifted), then per receiver merge the fleet's A array obstacles
 *   array_obst [F][A][N][5], array_meta [F][A][2], array_id [F][A] (NULL: ids R + a)
 * (rows as in mpcg_scene_io.obst / obst_meta) with the other robots' plans (index q,
 * DETERMINISTIC; a robot replaces the array obstacle of the same id, otherwise it is
 * appended), keep the n_ell closest or pad with dummies, and write
 *   obst [S][n_ell][N][5], obst_meta [S][n_ell][2]
 * for mpcg_prepare.  state [S][nx] is the ego state.  Requires nx 5, 2 <= N <= 32,
 * A + R - 1 <= 64, n_ell <= 32 and 2 <= R <= 8 (else -2). */
int mpcg_fleet_obstacles(const mpcg_problem *pr, int n_fleets, int n_robots, int n_array,
                         const mpcg_fleet_settings *set, const mpcg_fleet_state *st, const double *state,
                         const double *array_obst, const double *array_meta, const int *array_id, double now,
                         double *obst, double *obst_meta, void *stream);

/* After the solves of step `now`: each robot's plan (the winner's stages 0..N-1, or the
 * braking plan when best < 0), its selected topology, the trigger that fires and, for the
 * publishers, the update of the per-sender state.
 *   best [S], xtraj [S*G][N+1][nx], state [S][nx]
 *   topology [S][G] the topology id of each planner, or NULL: the planner index for guided
 *            planners and 2 * n_paths for the non-guided one (guided [S][G], NULL: all guided)
 *   reason [S] (MPCG_FLEET_*), published [S]
 * prev_topology is updated for every robot.  Same limits as mpcg_fleet_obstacles. */
int mpcg_fleet_publish(const mpcg_problem *pr, int n_fleets, int n_robots, int n_guesses,
                       const mpcg_fleet_settings *set, const mpcg_fleet_state *st, const int *best,
                       const double *xtraj, const double *state, const int *topology,
                       const unsigned char *guided, double now, int *reason, unsigned char *published,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_FLEET_H */
