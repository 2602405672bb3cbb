"""The publish decision of one robot after one solve, as a plain loop (test helper, not a test).

Written line by line from the reference, independently of fleet.publish_host:
  Planner::solveMPC                         mpc_planner/src/planner.cpp:89-92, 194-222
  applyBrakingCommand,
  buildOutputFromBrakingCommand             mpc_planner_jackalsimulator/src/jules_ros1_jackalplanner.cpp:1169-1217
  getConstantVelocityPrediction             mpc_planner/src/data_preparation.cpp:60-81
  decideCommunication, shouldCommunicate    jules_ros1_jackalplanner.cpp:1401-1501
  CommunicationTriggers::*                  mpc_planner_communication/src/communication_triggers.cpp
  Trajectory::geomtricDeviationTrigger      mpc_planner_types/src/data_types.cpp:233-255
  publishCmdAndVisualize,
  publishDirectTrajectory                   jules_ros1_jackalplanner.cpp:1219-1247, 1265-1328
"""
import math


class Robot:
    """What one JulesJackalPlanner keeps between steps (`None` stands for ros::Time(0) / an empty trajectory)."""

    def __init__(self):
        self.output_topology = -1            # _output.selected_topology_id, default -1
        self.last_communicated = None        # _data.last_communicated_trajectory: list of (x, y, psi)
        self.last_send_time = None           # _data.last_send_trajectory_time


def solve_output(robot, success, xtraj_winner, topology_id, N):
    """Planner::solveMPC's bookkeeping around the solve: returns (trajectory, selected, following_new)."""
    prev_followed_topology = robot.output_topology           # :89
    selected, following_new, traj = -1, False, []            # :92, a fresh PlannerOutput
    if success:
        for k in range(N):                                   # :204-208
            traj.append((xtraj_winner[k][0], xtraj_winner[k][1], xtraj_winner[k][2]))
        selected = topology_id                               # :216
        following_new = not (prev_followed_topology == selected)   # :221
    robot.output_topology = selected
    return traj, selected, following_new


def braking_trajectory(state, N, dt, deceleration, control_frequency):
    x, y, psi, v = state[0], state[1], state[2], state[3]
    dt_control = 1.0 / control_frequency                     # applyBrakingCommand
    velocity_after_braking = v - deceleration * dt_control
    new_speed = max(velocity_after_braking, 0.0)
    new_vx = math.cos(psi) * new_speed                       # buildOutputFromBrakingCommand
    new_vy = math.sin(psi) * new_speed
    traj = []
    for i in range(N):                                       # getConstantVelocityPrediction
        traj.append((x + new_vx * dt * i, y + new_vy * dt * i, psi))
    return traj


def geometric_deviation(traj, last, max_deviation):
    if len(traj) == 0 or last is None or len(last) == 0:     # checkGeometricDeviation
        return False
    if len(traj) != len(last):                               # geomtricDeviationTrigger
        return False
    max_sq = max_deviation * max_deviation
    for i in range(len(traj)):
        dx_sq = (traj[i][0] - last[i][0]) * (traj[i][0] - last[i][0])
        dy_sq = (traj[i][1] - last[i][1]) * (traj[i][1] - last[i][1])
        if dx_sq + dy_sq > max_sq:
            return True
    return False


def should_communicate(success, selected, following_new, traj, robot, now, n_paths, max_deviation, heartbeat):
    """shouldCommunicate in PLANNING_ACTIVE: (reason, communicate)."""
    non_guided = 2 * n_paths
    if not success:                                          # checkInfeasible
        return 1, True
    if success and selected == non_guided:                   # checkNonGuidedHomologyFail
        return 6, True
    if success and following_new and selected != non_guided:  # checkTopologyChange
        return 3, True
    if geometric_deviation(traj, robot.last_communicated, max_deviation):
        return 4, True
    if robot.last_send_time is None or (now - robot.last_send_time) >= heartbeat:   # checkTime
        return 5, True
    return 0, False


def wrap(a):
    while a > math.pi:
        a -= 2.0 * math.pi
    while a < -math.pi:
        a += 2.0 * math.pi
    return a


# control_frequency of obstacles_case: high enough that a plan can be older than one control
# period and still k = 0, alpha < 0.01 (the reference's third skip)
CASE_CONTROL_FREQUENCY = 1000.0
CLAMPED_SENDER, WRAPPING_SENDER = 7, 8


def obstacles_case(N, dt, seed=11, F=3, R=4, A=5, now=10.0):
    """Inputs of the obstacle-list kernels that take every branch of the time shift: per sender
    (F * R = 12) an age -- never received, fresher than one control period, k = 0 with alpha < 0.01,
    k = 0 with alpha 0.25, k = 2 with a fractional alpha, alpha <= 0.001 with k = 1, k >= N -- a plan
    whose last two points exceed v_max and w_max (CLAMPED_SENDER), one whose angles cross +-pi
    (WRAPPING_SENDER), and one array obstacle whose id is a robot index."""
    import numpy as np

    rng = np.random.default_rng(seed)
    S = F * R
    ages = [np.nan, 0.0005, 0.0015, 0.05, 0.47, 0.2001, N * dt + 0.1, 0.47, 0.47, 0.13, 0.31, 0.05]
    assert len(ages) == S
    state = np.zeros((S, 5))
    state[:, 0:2] = rng.uniform(-2.0, 2.0, (S, 2))
    state[:, 2] = rng.uniform(-3.0, 3.0, S)
    state[:, 3] = rng.uniform(0.2, 1.5, S)
    sent_plan = np.zeros((S, N, 3))
    k = np.arange(N)
    for q in range(S):
        p0, psi, v = rng.uniform(-4.0, 4.0, 2), rng.uniform(-2.5, 2.5), rng.uniform(0.3, 1.2)
        bend = rng.uniform(-0.02, 0.02)
        ang = psi + bend * k
        sent_plan[q, :, 0] = p0[0] + np.cumsum(v * dt * np.cos(ang))
        sent_plan[q, :, 1] = p0[1] + np.cumsum(v * dt * np.sin(ang))
        sent_plan[q, :, 2] = ang
    sent_plan[CLAMPED_SENDER, N - 1, 0:2] = sent_plan[CLAMPED_SENDER, N - 2, 0:2] + (0.8, 0.6)    # 5 m/s
    sent_plan[CLAMPED_SENDER, N - 1, 2] = sent_plan[CLAMPED_SENDER, N - 2, 2] + 0.8               # 4 rad/s
    sent_plan[WRAPPING_SENDER, :, 2] = [wrap(math.pi - 0.1 + 0.02 * i) for i in range(N)]
    sent_time = now - np.array(ages)
    array_obst = np.zeros((F, A, N, 5))
    array_meta = np.zeros((F, A, 2))
    for f in range(F):
        for a in range(A):
            p0, vel = rng.uniform(-5.0, 5.0, 2), rng.uniform(-0.5, 0.5, 2)
            array_obst[f, a, :, 0] = p0[0] + vel[0] * dt * k
            array_obst[f, a, :, 1] = p0[1] + vel[1] * dt * k
            array_obst[f, a, :, 2] = math.atan2(vel[1], vel[0])
            array_obst[f, a, :, 3:5] = rng.uniform(0.0, 0.3, (N, 2))
            array_meta[f, a] = (rng.uniform(0.2, 0.5), rng.choice([1.0, 5.991464547107982]))
    array_id = np.tile(np.arange(R, R + A, dtype=np.int32), (F, 1))
    array_id[:, 2] = 1                                   # collides with robot 1
    fstate = dict(sent_plan=sent_plan.reshape(F, R, N, 3), sent_time=sent_time.reshape(F, R),
                  last_send_time=np.full((F, R), np.nan), prev_topology=np.full((F, R), -1, np.int32))
    return dict(state=state, fstate=fstate, array_obst=array_obst, array_meta=array_meta, array_id=array_id,
                now=now, F=F, R=R, A=A)


def assert_away_from_boundaries(case, N, dt, n_ell, control_frequency, shifted_plan):
    """The CPU-side precondition of the GPU comparison: no input of `case` sits on a decision
    boundary of the reference.  `shifted_plan` (F, R, N, 3): the plans after the host's time shift
    (the positions the keep-closest scores are taken on).  Returns the number of robots whose
    list was cut."""
    import numpy as np

    F, R, A = case["F"], case["R"], case["A"]
    st = case["fstate"]["sent_time"]
    for t0 in st.reshape(-1):
        if math.isnan(t0):
            continue
        el = case["now"] - t0
        assert abs(el - 1.0 / control_frequency) >= 1e-9
        ratio = el / dt
        assert abs(ratio - round(ratio)) >= 1e-6
        alpha = (el - math.floor(ratio) * dt) / dt
        assert abs(alpha - 0.01) >= 1e-6 and abs(alpha - 0.001) >= 1e-6
    cut = 0
    for f in range(F):
        for r in range(R):
            x = case["state"][f * R + r]
            cand = [case["array_obst"][f, a, :, 0:2] for a in range(A)]
            for q in range(R):
                if q == r or math.isnan(st[f, q]):
                    continue
                hit = [a for a in range(A) if case["array_id"][f, a] == q]
                if hit:
                    cand[hit[0]] = shifted_plan[f, q, :, 0:2]
                else:
                    cand.append(shifted_plan[f, q, :, 0:2])
            if len(cand) <= n_ell:
                continue
            cut += 1
            scores = []
            for p in cand:                               # ensureObstacleSize's score
                best = 1e5
                for k in range(N):
                    ex, ey = x[0] + x[3] * k * math.cos(x[2]), x[1] + x[3] * k * math.sin(x[2])
                    best = min(best, (k + 1) * 0.6 * math.hypot(p[k, 0] - ex, p[k, 1] - ey))
                scores.append(best)
            srt = np.sort(scores)
            assert np.all(np.diff(srt[:n_ell + 1]) >= 1e-6), (f, r, srt)
    return cut


def publish_case(seed=7, F=4, R=4, G=5, N=20, now=12.0):
    """A crafted batch in which every trigger reason occurs (robots 0..8 by hand, the rest random):
    returns dict(best, xtraj, state, fstate, guided, topology, expect) -- `expect` the reason of
    robots 0..8 with max_geometric_deviation 0.5, heartbeat_time 2, n_paths 4 (planner G-1 is the
    non-guided one, topology id 8)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    S = F * R
    xtraj = rng.uniform(-3.0, 3.0, (S * G, N + 1, 5))
    state = rng.uniform(-1.0, 1.0, (S, 5))
    state[:, 3] = rng.uniform(0.0, 2.0, S)
    state[8, 3] = 0.05                                   # braking to a standstill (max(., 0))
    guided = np.ones((S, G), np.uint8)
    guided[:, G - 1] = 0
    topology = np.where(guided == 1, np.arange(G)[None, :], 8).astype(np.int32)
    best = rng.integers(-1, G, S).astype(np.int32)
    prev = rng.integers(-1, G, S).astype(np.int32)
    sent_time = np.where(rng.random(S) < 0.7, now - rng.uniform(0.0, 1.0, S), np.nan)
    last_send = np.where(rng.random(S) < 0.7, now - rng.uniform(0.0, 4.0, S), np.nan)
    sent_plan = rng.uniform(-3.0, 3.0, (S, N, 3))
    xt = xtraj.reshape(S, G, N + 1, 5)
    near = lambda s, b: xt[s, b, :N, :3] + 0.1           # noqa: E731  within 0.5 m of the winner's plan
    best[0], prev[0] = -1, 2                                                              # 1 INFEASIBLE
    best[1], prev[1] = G - 1, 2                                                           # 6 beats 3
    best[2], prev[2] = 2, 1                                                               # 3 TOPOLOGY_CHANGE
    best[3], prev[3], sent_time[3], last_send[3] = 2, 2, now - 0.05, now - 0.05           # 4 GEOMETRIC
    sent_plan[3] = near(3, 2)
    sent_plan[3, N - 1, 0] += 1.0
    best[4], prev[4], sent_time[4], last_send[4] = 2, 2, now - 0.05, np.nan               # 5 TIME: never sent
    sent_plan[4] = near(4, 2)
    best[5], prev[5], sent_time[5], last_send[5] = 2, 2, now - 0.05, now - 3.0            # 5 TIME: heartbeat
    sent_plan[5] = near(5, 2)
    best[6], prev[6], sent_time[6], last_send[6] = 2, 2, now - 0.05, now - 0.5            # 0
    sent_plan[6] = near(6, 2)
    best[7], prev[7], sent_time[7], last_send[7] = 2, 2, np.nan, now - 0.5                # 0: nothing to deviate from
    best[8], prev[8] = -1, -1                                                             # 1
    fstate = dict(sent_plan=sent_plan.reshape(F, R, N, 3), sent_time=sent_time.reshape(F, R),
                  last_send_time=last_send.reshape(F, R), prev_topology=prev.reshape(F, R))
    return dict(best=best, xtraj=xtraj, state=state, fstate=fstate, guided=guided, topology=topology, now=now,
                expect=[1, 6, 3, 4, 5, 5, 0, 0, 1])


def publish_batch(best, xtraj, state, fstate, topology, now, dt, settings):
    """publish_step over every robot of a batch given in fleet.publish_host's arrays (explicit
    topology (S, G)); returns the same keys as NumPy arrays."""
    import numpy as np

    S = len(best)
    N = np.asarray(fstate["sent_plan"]).shape[-2]
    shape = np.asarray(fstate["sent_time"]).shape
    sp = np.asarray(fstate["sent_plan"], np.float64).reshape(S, N, 3)
    stime = np.asarray(fstate["sent_time"], np.float64).reshape(S)
    lst = np.asarray(fstate["last_send_time"], np.float64).reshape(S)
    pt = np.asarray(fstate["prev_topology"]).reshape(S)
    xt = np.asarray(xtraj, np.float64)
    xt = xt.reshape(S, -1, N + 1, xt.shape[-1])
    topo = np.asarray(topology).reshape(S, -1)
    out = dict(plan=np.zeros((S, N, 3)), selected=np.zeros(S, np.int32), reason=np.zeros(S, np.int32),
               published=np.zeros(S, np.uint8), sent_plan=sp.copy(), sent_time=stime.copy(),
               last_send_time=lst.copy(), prev_topology=np.zeros(S, np.int32))
    for s in range(S):
        rb = Robot()
        rb.output_topology = int(pt[s])
        rb.last_communicated = None if math.isnan(stime[s]) else [tuple(p) for p in sp[s].tolist()]
        rb.last_send_time = None if math.isnan(lst[s]) else float(lst[s])
        reason, pub, traj = publish_step(rb, int(best[s]), xt[s].tolist(), np.asarray(state)[s].tolist(),
                                         topo[s].tolist(), now, N, dt, settings)
        out["plan"][s] = traj
        out["selected"][s] = out["prev_topology"][s] = rb.output_topology
        out["reason"][s], out["published"][s] = reason, pub
        if pub:
            out["sent_plan"][s], out["sent_time"][s], out["last_send_time"][s] = traj, now, now
    for k in ("sent_time", "last_send_time", "prev_topology"):
        out[k] = out[k].reshape(shape)
    out["sent_plan"] = out["sent_plan"].reshape(*shape, N, 3)
    return out


def publish_step(robot, best, xtraj_robot, state, topology_robot, now, N, dt, settings):
    """One robot, one step.  xtraj_robot [G][N+1][nx], topology_robot [G].  Returns
    (reason, published, plan) and updates `robot`."""
    G = len(xtraj_robot)
    success = 0 <= best < G
    traj, selected, following_new = solve_output(robot, success, xtraj_robot[best] if success else None,
                                                 topology_robot[best] if success else -1, N)
    if not success:
        traj = braking_trajectory(state, N, dt, settings.deceleration, settings.control_frequency)
    if not settings.communicate_on_topology_switch_only:     # decideCommunication
        reason, communicate = 0, True
    else:
        reason, communicate = should_communicate(success, selected, following_new, traj, robot, now,
                                                 settings.n_paths, settings.max_geometric_deviation,
                                                 settings.heartbeat_time)
    if communicate:                                          # publishDirectTrajectory
        robot.last_send_time = now
        robot.last_communicated = list(traj)
    return reason, communicate, traj
