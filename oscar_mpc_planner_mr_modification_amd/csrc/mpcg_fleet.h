// mpcg_fleet.h — the multi-robot layer of one control step on the GPU: plan
// exchange between the robots of a fleet and the communication triggers.
// ABI and the reference lines: include/mpcg_fleet.h; host restatement:
// fleet.py (publish) and obstacles.py (time shift, merge, keep-closest / pad).
//
// Three kernels, one 64-lane workgroup per item, values staged in LDS and
// streamed out with coalesced stores:
//   fleet_shift_kernel      per sender: the published plan shifted to `now`
//                           (Trajectory::interpolateTrajectoryByElapsedTime), lane i = point i
//                           of the extended sequence in closed form
//   fleet_obstacles_kernel  per receiver: candidate list (array obstacles, then the other
//                           robots' plans), keep the n_ell closest (lane c scores candidate c,
//                           stable rank) or pad with dummies, obst / obst_meta rows
//   fleet_publish_kernel    per robot, after the solves: plan of this step, selected topology,
//                           trigger reason, update of the per-sender state
// Compiled only into mpcg_fleet.hip with -ffp-contract=off and written with
// explicitly rounded operations in the host restatement's operation order:
// every value that does not pass through cos / sin / hypot agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_fleet.h"  // the public header of the same name

namespace mpcg {

constexpr int FLEET_MAX_N = 32;
constexpr int FLEET_MAX_CAND = 64;
constexpr int FLEET_MAX_ELL = 32;
constexpr int FLEET_MAX_R = 8;
constexpr int FLEET_ROBOT = 1 << 8;   // candidate source: a < FLEET_ROBOT array row a, FLEET_ROBOT + q robot q
constexpr int FLEET_DUMMY = 1 << 16;

constexpr double FLEET_PI = 3.14159265358979323846;
constexpr double FLEET_TWO_PI = 2.0 * FLEET_PI;

// MultiRobot::wrapAngle (multi_robot_utility_functions.cpp:143-150).  The reference loops
// until the angle is in [-pi, pi]; the arguments here stay within a few turns (solver
// bounds +- 4 pi plus w_max * horizon), and the bound keeps a non-finite input from
// holding the wave forever.
__device__ __forceinline__ double fleet_wrap(double a) {
    for (int it = 0; it < 64 && a > FLEET_PI; ++it) a = __dsub_rn(a, FLEET_TWO_PI);
    for (int it = 0; it < 64 && a < -FLEET_PI; ++it) a = __dadd_rn(a, FLEET_TWO_PI);
    return a;
}

// ---------------------------------------------------------------- time shift
__global__ __launch_bounds__(64) void fleet_shift_kernel(int n_senders, int N, double dt, mpcg_fleet_settings set,
                                                         mpcg_fleet_state st, double now) {
    __shared__ double P[FLEET_MAX_N][3];   // the plan as received
    __shared__ double O[FLEET_MAX_N][3];   // the shifted plan
    const int q = blockIdx.x;
    if (q >= n_senders) return;
    const int lane = threadIdx.x;
    double* plan = st.sent_plan + (size_t)q * N * 3;
    for (int e = lane; e < N * 3; e += 64) (&P[0][0])[e] = plan[e];
    const double t0 = st.sent_time[q];
    __syncthreads();
    // every condition below is uniform over the workgroup
    if (!(t0 == t0)) return;   // nothing received yet
    const double el = __dsub_rn(now, t0);
    if (!(el >= __ddiv_rn(1.0, set.control_frequency))) return;   // fresher than one control period
    const double kd = floor(__ddiv_rn(el, dt));
    if (!(kd < (double)N)) return;   // critically stale: left as it is
    const int k = (int)kd;
    const double alpha = __ddiv_rn(__dsub_rn(el, __dmul_rn((double)k, dt)), dt);
    if (k == 0 && alpha < 0.01) return;
    // constant-velocity extrapolation from the last two points, speed and turn rate clamped
    const double lx = P[N - 1][0], ly = P[N - 1][1], la = P[N - 1][2];
    double vx = __ddiv_rn(__dsub_rn(lx, P[N - 2][0]), dt), vy = __ddiv_rn(__dsub_rn(ly, P[N - 2][1]), dt);
    double psi_dot = __ddiv_rn(fleet_wrap(__dsub_rn(la, P[N - 2][2])), dt);
    const double vm = hypot(vx, vy);
    if (vm > set.v_max) {
        vx = __dmul_rn(__ddiv_rn(vx, vm), set.v_max);
        vy = __dmul_rn(__ddiv_rn(vy, vm), set.v_max);
    }
    if (fabs(psi_dot) > set.w_max) psi_dot = fmin(fmax(psi_dot, -set.w_max), set.w_max);
    // point j of [plan_0 .. plan_{N-1}, ext_1 .. ext_{k+1}]
    auto ext = [&](int j, double& x, double& y, double& a) {
        if (j < N) {
            x = P[j][0];
            y = P[j][1];
            a = P[j][2];
        } else {
            const double te = __dmul_rn((double)(j - N + 1), dt);
            x = __dadd_rn(lx, __dmul_rn(vx, te));
            y = __dadd_rn(ly, __dmul_rn(vy, te));
            a = fleet_wrap(__dadd_rn(la, __dmul_rn(psi_dot, te)));
        }
    };
    if (lane < N) {
        // the first k points are dropped; alpha > 0.001: pairwise interpolation (angles along the
        // shortest arc, MultiRobot::interpolateAngle), otherwise the extra point is dropped
        double cx, cy, ca;
        ext(lane + k, cx, cy, ca);
        if (alpha > 0.001) {
            double nx, ny, na;
            ext(lane + k + 1, nx, ny, na);
            const double om = __dsub_rn(1.0, alpha);
            cx = __dadd_rn(__dmul_rn(om, cx), __dmul_rn(alpha, nx));
            cy = __dadd_rn(__dmul_rn(om, cy), __dmul_rn(alpha, ny));
            ca = fleet_wrap(__dadd_rn(ca, __dmul_rn(fleet_wrap(__dsub_rn(na, ca)), alpha)));
        }
        O[lane][0] = cx;
        O[lane][1] = cy;
        O[lane][2] = ca;
    }
    __syncthreads();
    for (int e = lane; e < N * 3; e += 64) plan[e] = (&O[0][0])[e];
    if (lane == 0) st.sent_time[q] = now;
}

// ---------------------------------------------------------------- obstacle lists
struct FleetObsLds {
    double score[FLEET_MAX_CAND];
    double sigma[FLEET_MAX_N];     // semi-axes of a GAUSSIAN dummy
    int cand[FLEET_MAX_CAND];      // source of candidate c
    int slot[FLEET_MAX_ELL];       // source of output row j
    int n_cand;
};

__global__ __launch_bounds__(64) void fleet_obstacles_kernel(int n_scenes, int R, int A, int N, int NE, double dt,
                                                             mpcg_fleet_settings set,
                                                             const double* __restrict__ sent_plan,
                                                             const double* __restrict__ sent_time,
                                                             const double* __restrict__ state,
                                                             const double* __restrict__ array_obst,
                                                             const double* __restrict__ array_meta,
                                                             const int* __restrict__ array_id,
                                                             double* __restrict__ obst, double* __restrict__ obst_meta) {
    __shared__ FleetObsLds L;
    const int s = blockIdx.x;
    if (s >= n_scenes) return;
    const int lane = threadIdx.x;
    const int f = s / R, r = s - f * R;
    const double* st = state + (size_t)s * MPCG_NX;
    const double x0 = st[0], y0 = st[1];
    // ---- candidate list (updateRobotObstaclesFromTrajectories): the array obstacles in order; each
    // validated sender replaces the first array obstacle with its index, or is appended
    if (lane == 0) {
        int n = A;
        for (int a = 0; a < A; ++a) L.cand[a] = a;
        for (int q = 0; q < R; ++q) {
            if (q == r) continue;
            const double t = sent_time[(size_t)f * R + q];
            if (!(t == t)) continue;
            int hit = -1;
            for (int a = 0; a < A && hit < 0; ++a) {
                const int id = array_id ? array_id[(size_t)f * A + a] : R + a;
                if (L.cand[a] < FLEET_ROBOT && id == q) hit = a;
            }
            if (hit >= 0)
                L.cand[hit] = FLEET_ROBOT + q;
            else
                L.cand[n++] = FLEET_ROBOT + q;
        }
        L.n_cand = n;
    }
    __syncthreads();
    const int n = L.n_cand;   // <= A + R - 1 <= FLEET_MAX_CAND
    // position k of candidate source src
    auto cpos = [&](int src, int k, double& px, double& py) {
        const double* p = src < FLEET_ROBOT ? array_obst + (((size_t)f * A + src) * N + k) * 5
                                            : sent_plan + (((size_t)f * R + (src - FLEET_ROBOT)) * N + k) * 3;
        px = p[0];
        py = p[1];
    };
    if (n > NE) {
        // ---- ensureObstacleSize, more than n_ell: the n_ell smallest of min_k (k + 1) 0.6 |p_k - ego_k|
        // along a constant-velocity roll-out of the ego state; stable (ties: lower candidate index)
        if (lane < n) {
            const double dirx = cos(st[2]), diry = sin(st[2]), v = st[3];
            const int src = L.cand[lane];
            double best = 1e5;
            for (int k = 0; k < N; ++k) {
                double px, py;
                cpos(src, k, px, py);
                const double vk = __dmul_rn(v, (double)k);
                const double ex = __dadd_rn(x0, __dmul_rn(vk, dirx)), ey = __dadd_rn(y0, __dmul_rn(vk, diry));
                const double d = __dmul_rn(__dmul_rn((double)(k + 1), 0.6), hypot(__dsub_rn(px, ex), __dsub_rn(py, ey)));
                if (d < best) best = d;
            }
            L.score[lane] = best;   // never NaN: the ranks below are a permutation of 0..n-1
        }
        if (lane < NE) L.slot[lane] = FLEET_DUMMY;
        __syncthreads();
        if (lane < n) {
            const double mine = L.score[lane];
            int rank = 0;
            for (int c = 0; c < n; ++c) {
                const double o = L.score[c];
                rank += (o < mine || (o == mine && c < lane)) ? 1 : 0;
            }
            if (rank < NE) L.slot[rank] = L.cand[lane];
        }
    } else if (lane < NE) {
        L.slot[lane] = lane < n ? L.cand[lane] : FLEET_DUMMY;
    }
    // ---- GAUSSIAN dummies: noise 0.3 integrated over the horizon (propagatePredictionUncertainty)
    if (set.probabilistic && n < NE && lane == 0) {
        const double step = __dmul_rn(0.3, dt);
        double major = 0.0;
        for (int k = 0; k < N; ++k) {
            major = __dsqrt_rn(__dadd_rn(__dmul_rn(major, major), __dmul_rn(step, step)));
            L.sigma[k] = major;
        }
    }
    __syncthreads();
    // ---- rows out (EllipsoidConstraints::setParameters layout): x y angle major minor
    double* ob = obst + (size_t)s * NE * N * 5;
    const double dx = __dadd_rn(x0, 100.0), dy = __dadd_rn(y0, 100.0);
    for (int e = lane; e < NE * N * 5; e += 64) {
        const int j = e / (N * 5), rem = e - j * (N * 5);
        const int k = rem / 5, c = rem - k * 5;
        const int src = L.slot[j];
        double v;
        if (src == FLEET_DUMMY)
            v = c == 0 ? dx : (c == 1 ? dy : (c == 2 || !set.probabilistic ? 0.0 : L.sigma[k]));
        else if (src >= FLEET_ROBOT)
            v = c < 3 ? sent_plan[(((size_t)f * R + (src - FLEET_ROBOT)) * N + k) * 3 + c] : 0.0;
        else
            v = array_obst[(((size_t)f * A + src) * N + k) * 5 + c];
        ob[e] = v;
    }
    if (lane < NE) {
        const int src = L.slot[lane];
        double rad, chi;
        if (src == FLEET_DUMMY) {
            rad = 0.0;
            chi = set.probabilistic ? set.chi_gaussian : 1.0;
        } else if (src >= FLEET_ROBOT) {
            rad = set.robot_obstacle_radius;
            chi = 1.0;
        } else {
            rad = array_meta[((size_t)f * A + src) * 2 + 0];
            chi = array_meta[((size_t)f * A + src) * 2 + 1];
        }
        double* m = obst_meta + ((size_t)s * NE + lane) * 2;
        m[0] = rad;
        m[1] = chi;
    }
}

// ---------------------------------------------------------------- publication
__global__ __launch_bounds__(64) void fleet_publish_kernel(int n_scenes, int G, int N, double dt,
                                                           mpcg_fleet_settings set, mpcg_fleet_state st,
                                                           const int* __restrict__ best,
                                                           const double* __restrict__ xtraj,
                                                           const double* __restrict__ state,
                                                           const int* __restrict__ topology,
                                                           const unsigned char* __restrict__ guided, double now,
                                                           int* __restrict__ reason,
                                                           unsigned char* __restrict__ published) {
    __shared__ double P[FLEET_MAX_N][3];
    const int s = blockIdx.x;
    if (s >= n_scenes) return;
    const int lane = threadIdx.x;
    const int b = best[s];
    const bool ok = b >= 0 && b < G;
    const int non_guided_id = 2 * set.n_paths;
    double* plan = st.sent_plan + (size_t)s * N * 3;
    const double t_sent = st.sent_time[s], t_last = st.last_send_time[s];
    const int prev = st.prev_topology[s];
    // ---- the plan of this step, lane i = point i
    int deviates = 0;
    if (lane < N) {
        double px, py, pa;
        if (ok) {
            // Planner::solveMPC (planner.cpp:204-208): stages 0..N-1 of the selected planner's output
            const double* row = xtraj + (((size_t)s * G + b) * (N + 1) + lane) * MPCG_NX;
            px = row[0];
            py = row[1];
            pa = row[2];
        } else {
            // applyBrakingCommand + buildOutputFromBrakingCommand (jules_ros1_jackalplanner.cpp:1169-1217)
            const double* x = state + (size_t)s * MPCG_NX;
            const double after = __dsub_rn(x[3], __dmul_rn(set.deceleration, __ddiv_rn(1.0, set.control_frequency)));
            const double vb = after < 0.0 ? 0.0 : after;
            pa = x[2];
            px = __dadd_rn(x[0], __dmul_rn(__dmul_rn(__dmul_rn(cos(pa), vb), dt), (double)lane));
            py = __dadd_rn(x[1], __dmul_rn(__dmul_rn(__dmul_rn(sin(pa), vb), dt), (double)lane));
        }
        P[lane][0] = px;
        P[lane][1] = py;
        P[lane][2] = pa;
        // Trajectory::geomtricDeviationTrigger (data_types.cpp:233-255) against the communicated plan
        if (t_sent == t_sent) {
            const double ex = __dsub_rn(px, plan[lane * 3 + 0]), ey = __dsub_rn(py, plan[lane * 3 + 1]);
            deviates = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)) >
                       __dmul_rn(set.max_geometric_deviation, set.max_geometric_deviation);
        }
    }
    // (the barrier also orders every lane's reads of the per-sender state before the writes below)
    const bool geometric = __syncthreads_or(deviates) != 0;
    // ---- selected topology and the trigger, in the reference's priority order (shouldCommunicate)
    int selected = -1;
    if (ok) {
        const size_t p = (size_t)s * G + b;
        selected = topology ? topology[p] : ((!guided || guided[p]) ? b : non_guided_id);
    }
    int why = MPCG_FLEET_NO_COMMUNICATION;
    bool pub = true;
    if (set.communicate_on_topology_switch_only) {
        if (!ok)
            why = MPCG_FLEET_INFEASIBLE;
        else if (selected == non_guided_id)
            why = MPCG_FLEET_NON_GUIDED_HOMOLOGY_FAIL;
        else if (selected != prev)
            why = MPCG_FLEET_TOPOLOGY_CHANGE;
        else if (geometric)
            why = MPCG_FLEET_GEOMETRIC;
        else if (!(t_last == t_last) || __dsub_rn(now, t_last) >= set.heartbeat_time)
            why = MPCG_FLEET_TIME;
        else
            pub = false;
    }
    if (pub)
        for (int e = lane; e < N * 3; e += 64) plan[e] = (&P[0][0])[e];
    if (lane == 0) {
        if (pub) {
            st.sent_time[s] = now;
            st.last_send_time[s] = now;
        }
        st.prev_topology[s] = selected;
        reason[s] = why;
        published[s] = pub ? 1 : 0;
    }
}

}  // namespace mpcg
