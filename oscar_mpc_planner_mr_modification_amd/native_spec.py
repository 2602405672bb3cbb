"""Host-side description of the C ABI (include/mpcg.h): the `mpcg_problem`
struct, the solver options restated from the reference's acados generator
and the unicycle bounds.  Importable without a GPU and without loading
libmpcg.so (the CPU tests use it)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .layouts import Layout

NX, NU, NVAR = 5, 2, 7   # the T-MPC unicycle; the SH-MPC slack model has nx 6, the C3 bicycle nu 3 / nx 6
MAX_NX, MAX_NU = 6, 3
INFO_STRIDE = 4
STATS_STRIDE = 4   # NLP residuals: stationarity, res_eq, inequality violation, complementarity


class MpcgProblem(C.Structure):
    """Mirror of `mpcg_problem` (include/mpcg.h)."""
    _fields_ = [
        ("N", C.c_int), ("npar", C.c_int),
        ("n_lin", C.c_int), ("n_ell", C.c_int), ("n_seg", C.c_int),
        ("i_w_acc", C.c_int), ("i_w_ang", C.c_int), ("i_w_vel", C.c_int), ("i_v_ref", C.c_int),
        ("i_w_contour", C.c_int), ("i_w_lag", C.c_int),
        ("i_spline0", C.c_int),
        ("i_cons_w", C.c_int), ("i_prev_x", C.c_int), ("i_prev_y", C.c_int),
        ("i_lin0", C.c_int),
        ("i_disc_r", C.c_int), ("i_disc_off", C.c_int),
        ("i_ell0", C.c_int),
        ("n_scen", C.c_int), ("i_scen0", C.c_int), ("i_w_slack", C.c_int), ("nx", C.c_int),
        ("dt", C.c_double), ("rk_steps", C.c_int),
        ("lbu", C.c_double * MAX_NU), ("ubu", C.c_double * MAX_NU),
        ("lbx", C.c_double * MAX_NX), ("ubx", C.c_double * MAX_NX),
        ("sqp_iters", C.c_int), ("qp_tol", C.c_double), ("qp_iter_max", C.c_int),
        ("reg_eps", C.c_double), ("qp_mu0", C.c_double), ("qp_thr0", C.c_double),
        ("res_eq_fail", C.c_double),
        ("nu", C.c_int), ("model", C.c_int), ("i_w_tangle", C.c_int), ("i_w_tcont", C.c_int),
        ("qp_warm_start", C.c_int), ("qp_ws_thr", C.c_double),
        # ABI 6
        ("nlp_solver", C.c_int), ("nlp_max_iter", C.c_int), ("nlp_tol", C.c_double), ("qp_warm_first", C.c_int),
        # ABI 7
        ("qp_t_min", C.c_double), ("qp_mu_max", C.c_double),
        # ABI 8: the interior point's profile
        ("qp_profile", C.c_int), ("qp_init_move", C.c_int), ("qp_cond_pred_corr", C.c_int),
        ("qp_itref_corr_max", C.c_int), ("qp_sigma_clip", C.c_int), ("qp_maxit_first", C.c_int),
        # ABI 9: BLASFEO's rule for a non-positive Cholesky pivot
        ("qp_pivot_zero", C.c_int),
    ]


# acados options restated (generate_acados_solver.py:88-173: qp_tol, qp_solver_iter_max, MIRROR
# epsilon, tol) + the IPM's cold start; qp_warm_start=2 (the reference's qp_solver_warm_start, :173)
# with acados' warm_start_first_qp off (qp_warm_first=0) starts every SQP-RTI QP cold and the
# later QPs of a full SQP call (solver_type="SQP") warm (DESIGN.md §2 "QP start")
DEFAULT_OPTIONS = dict(qp_tol=1e-5, qp_iter_max=50, reg_eps=1e-4, res_eq_fail=1e-2,
                       qp_warm_start=2, qp_ws_thr=0.1, qp_warm_first=0, solver_type="SQP_RTI", nlp_max_iter=100,
                       nlp_tol=1e-2, qp_profile="hpipm")
# The interior point's profiles (mpcg_problem_set_qp_profile in libmpcg.so writes the
# same values): "hpipm", the default, restates HPIPM's BALANCE mode as acados configures it (the
# reference sets four QP options and leaves the rest at acados' defaults, generate_acados_solver.py:162-173);
# "robust" is round 4's interior point.  Any field can be overridden by name.
QP_PROFILES = {
    "hpipm": dict(qp_profile_id=0, qp_mu0=10.0, qp_thr0=0.1, qp_t_min=1e-16, qp_mu_max=0.0, qp_init_move=1,
                  qp_cond_pred_corr=1, qp_itref_corr_max=2, qp_sigma_clip=0, qp_maxit_first=1, qp_pivot_zero=1),
    "robust": dict(qp_profile_id=1, qp_mu0=1.0, qp_thr0=1.0, qp_t_min=1e-12, qp_mu_max=1e8, qp_init_move=0,
                   qp_cond_pred_corr=0, qp_itref_corr_max=0, qp_sigma_clip=1, qp_maxit_first=0, qp_pivot_zero=0),
}
QP_FIELDS = ("qp_mu0", "qp_thr0", "qp_t_min", "qp_mu_max", "qp_init_move", "qp_cond_pred_corr", "qp_itref_corr_max",
             "qp_sigma_clip", "qp_maxit_first", "qp_pivot_zero")
NLP_SOLVER = {"SQP_RTI": 0, "SQP": 1}
# ContouringSecondOrderUnicycleModel bounds (solver_model.py:204-205), z = [a, w, x, y, psi, v, s]
UNICYCLE_LB = (-2.0, -0.8, -2000.0, -2000.0, -4 * np.pi, -0.01, -1.0)
UNICYCLE_UB = (2.0, 0.8, 2000.0, 2000.0, 4 * np.pi, 3.0, 10000.0)


def problem_from_layout(layout: Layout, **opts) -> MpcgProblem:
    o = dict(DEFAULT_OPTIONS)
    o.update(opts)
    pr = MpcgProblem()
    pr.N, pr.npar = layout.N, layout.npar
    pr.n_lin, pr.n_ell, pr.n_seg = layout.n_lin, layout.n_ell, layout.n_seg
    pr.n_scen = layout.n_scen
    pr.nx = nx = layout.nx
    pr.nu = nu = layout.nu
    pr.model = layout.model_id
    for k, v in layout.index_struct().items():
        setattr(pr, k, v)
    pr.dt = o.get("dt", layout.dt)
    pr.rk_steps = o.get("rk_steps", layout.rk_steps)
    lb, ub = o.get("lb", layout.lb), o.get("ub", layout.ub)
    for i in range(nu):
        pr.lbu[i], pr.ubu[i] = lb[i], ub[i]
    for i in range(nx):
        pr.lbx[i], pr.ubx[i] = lb[nu + i], ub[nu + i]
    pr.sqp_iters = o.get("sqp_iters", layout.sqp_iters)
    pr.qp_tol = o["qp_tol"]
    pr.qp_iter_max = o["qp_iter_max"]
    pr.reg_eps = o["reg_eps"]
    pr.res_eq_fail = o["res_eq_fail"]
    pr.qp_warm_start = o["qp_warm_start"]
    pr.qp_ws_thr = o["qp_ws_thr"]
    pr.qp_warm_first = o["qp_warm_first"]
    pr.nlp_solver = NLP_SOLVER[o["solver_type"]]
    pr.nlp_max_iter = o["nlp_max_iter"]
    pr.nlp_tol = o["nlp_tol"]
    prof = QP_PROFILES[o["qp_profile"]]
    pr.qp_profile = prof["qp_profile_id"]
    for f in QP_FIELDS:
        setattr(pr, f, o.get(f, prof[f]))
    return pr


def needs_full(pr: MpcgProblem) -> bool:
    """whether a launch of `pr` runs the FULL kernel variant whatever buffers it is given
    (mpcg_sqp.h needs_full: a full SQP call, or a first QP that starts warm); otherwise the
    lean variant runs unless the call passes QP memory or a stats buffer"""
    return pr.nlp_solver == NLP_SOLVER["SQP"] or (pr.qp_warm_start == 2 and bool(pr.qp_warm_first))


class MpcgIo(C.Structure):
    """Mirror of `mpcg_io` (include/mpcg.h)."""
    _fields_ = [("params", C.c_void_p), ("warm", C.c_void_p), ("xinit", C.c_void_p), ("lam_in", C.c_void_p),
                ("xtraj", C.c_void_p), ("utraj", C.c_void_p), ("pobj", C.c_void_p),
                ("exit_code", C.c_void_p), ("info", C.c_void_p), ("lam_out", C.c_void_p),
                ("qp_in", C.c_void_p), ("qp_out", C.c_void_p), ("stats", C.c_void_p)]


class MpcgSceneIo(C.Structure):
    """Mirror of `mpcg_scene_io` (include/mpcg.h)."""
    _fields_ = [("stage_params", C.c_void_p), ("state", C.c_void_p), ("obst", C.c_void_p),
                ("obst_meta", C.c_void_p), ("guidance", C.c_void_p), ("guided", C.c_void_p),
                ("main_warm", C.c_void_p), ("prev_traj", C.c_void_p), ("prev_elapsed", C.c_void_p),
                ("consistency_on", C.c_void_p), ("robot_radius", C.c_double), ("w_consistency", C.c_double),
                ("deceleration", C.c_double),
                # ABI 6: t-mpc.warmstart_with_mpc_solution
                ("planner_xtraj", C.c_void_p), ("planner_utraj", C.c_void_p), ("existing_guidance", C.c_void_p),
                ("warmstart_with_mpc_solution", C.c_int), ("shift_forward", C.c_int)]


class MpcgStepIo(C.Structure):
    """Mirror of `mpcg_step_io` (include/mpcg.h)."""
    _fields_ = [("best", C.c_void_p), ("exit_code", C.c_void_p), ("xtraj", C.c_void_p), ("utraj", C.c_void_p),
                ("warm", C.c_void_p), ("lam_out", C.c_void_p), ("state_next", C.c_void_p), ("guided", C.c_void_p),
                ("topology", C.c_void_p), ("topology_next", C.c_void_p), ("previously_selected", C.c_void_p),
                ("shift_forward", C.c_int), ("consistency_on_non_guided", C.c_int), ("elapsed", C.c_double),
                ("deceleration", C.c_double)]


class MpcgScenarioIo(C.Structure):
    """Mirror of `mpcg_scenario_io` (include/mpcg.h)."""
    _fields_ = [("stage_params", C.c_void_p), ("state", C.c_void_p), ("main_warm", C.c_void_p),
                ("samples", C.c_void_p), ("n_samples", C.c_int), ("radius", C.c_double),
                ("deceleration", C.c_double)]


ABI_VERSION = 9


class MpcgFleetSettings(C.Structure):
    """Mirror of `mpcg_fleet_settings` (include/mpcg_fleet.h)."""
    _fields_ = [("control_frequency", C.c_double), ("v_max", C.c_double), ("w_max", C.c_double),
                ("robot_obstacle_radius", C.c_double), ("probabilistic", C.c_int), ("chi_gaussian", C.c_double),
                ("communicate_on_topology_switch_only", C.c_int), ("n_paths", C.c_int),
                ("max_geometric_deviation", C.c_double), ("heartbeat_time", C.c_double),
                ("deceleration", C.c_double)]


class MpcgFleetState(C.Structure):
    """Mirror of `mpcg_fleet_state` (include/mpcg_fleet.h)."""
    _fields_ = [("sent_plan", C.c_void_p), ("sent_time", C.c_void_p), ("last_send_time", C.c_void_p),
                ("prev_topology", C.c_void_p)]


# mpcg_fleet_publish's reason (CommunicationTriggerReason)
FLEET_REASONS = {0: "NO_COMMUNICATION", 1: "INFEASIBLE", 3: "TOPOLOGY_CHANGE", 4: "GEOMETRIC", 5: "TIME",
                 6: "NON_GUIDED_HOMOLOGY_FAIL"}


class MpcgPathTable(C.Structure):
    """Mirror of `mpcg_path_table` (include/mpcg_path.h)."""
    _fields_ = [("coef", C.c_void_p), ("knots", C.c_void_p), ("n_segments", C.c_void_p), ("path_of", C.c_void_p),
                ("n_paths", C.c_int), ("max_segments", C.c_int)]


class MpcgPathSettings(C.Structure):
    """Mirror of `mpcg_path_settings` (include/mpcg_path.h)."""
    _fields_ = [("control_frequency", C.c_double), ("deceleration", C.c_double), ("plant", C.c_int)]


# the reference-path tracking (include/mpcg_path.h)
PATH_MAX_SEGMENTS, PATH_SAMPLES, PATH_ROUNDS, PATH_REACHED_RADIUS = 64, 64, 5, 1.5


class MpcgRoadSettings(C.Structure):
    """Mirror of `mpcg_road_settings` (include/mpcg_road.h)."""
    _fields_ = [("width", C.c_double), ("robot_radius", C.c_double), ("two_way", C.c_int), ("mode", C.c_int)]


class MpcgRoadIo(C.Structure):
    """Mirror of `mpcg_road_io` (include/mpcg_road.h)."""
    _fields_ = [("state", C.c_void_p), ("main_warm", C.c_void_p), ("deceleration", C.c_double),
                ("guided", C.c_void_p), ("left_coef", C.c_void_p), ("right_coef", C.c_void_p)]


# the road-boundary halfspaces (include/mpcg_road.h)
ROAD_CENTERLINE, ROAD_BOUNDS, ROAD_MAX_N = 0, 1, 32


class MpcgDecompSettings(C.Structure):
    """Mirror of `mpcg_decomp_settings` (include/mpcg_decomp.h)."""
    _fields_ = [("range", C.c_double), ("deceleration", C.c_double)]


class MpcgDecompIo(C.Structure):
    """Mirror of `mpcg_decomp_io` (include/mpcg_decomp.h)."""
    _fields_ = [("state", C.c_void_p), ("main_warm", C.c_void_p), ("occ", C.c_void_p), ("n_occ", C.c_void_p),
                ("max_points", C.c_int)]


# the decomp halfspaces (include/mpcg_decomp.h)
DECOMP_MAX_POINTS, DECOMP_MAX_N, DECOMP_MAX_ROWS, DECOMP_EPS = 1024, 32, 64, 1e-10


class MpcgGuidanceSettings(C.Structure):
    """Mirror of `mpcg_guidance_settings` (include/mpcg_guidance.h)."""
    _fields_ = [("robot_radius", C.c_double), ("v_ref", C.c_double), ("consistency_on_non_guided", C.c_int)]


class MpcgGuidanceState(C.Structure):
    """Mirror of `mpcg_guidance_state` (include/mpcg_guidance.h)."""
    _fields_ = [("class_traj", C.c_void_p), ("class_used", C.c_void_p), ("planner_class", C.c_void_p),
                ("selected_topology", C.c_void_p), ("prev_was_original", C.c_void_p)]


class MpcgGuidanceOut(C.Structure):
    """Mirror of `mpcg_guidance_out` (include/mpcg_guidance.h)."""
    _fields_ = [("guidance", C.c_void_p), ("existing_guidance", C.c_void_p), ("previously_selected", C.c_void_p),
                ("consistency_on", C.c_void_p), ("topology", C.c_void_p), ("enabled", C.c_void_p),
                ("n_found", C.c_void_p), ("heading", C.c_void_p), ("sig_mask", C.c_void_p), ("sig_side", C.c_void_p),
                ("clearance", C.c_void_p), ("cost", C.c_void_p)]


# the guidance layer (include/mpcg_guidance.h)
GUIDANCE_CANDIDATES, GUIDANCE_BITS, GUIDANCE_FINE, GUIDANCE_SWEEPS = 8, 3, 4, 4
GUIDANCE_MAX_N, GUIDANCE_MAX_ELL, GUIDANCE_MAX_SEG = 32, 32, 8
GUIDANCE_ACCEL, GUIDANCE_RELEVANT, GUIDANCE_OFFSET, GUIDANCE_WIDTH, GUIDANCE_ONSET = 1.0, 2.5, 1.2, 2.0, 0.8
GUIDANCE_PUSH_MARGIN, GUIDANCE_CLEARANCE, GUIDANCE_V_FLOOR = 0.75, 0.25, 1e-3
GUIDANCE_EXIT_DISABLED = -100

# the active-solve compaction (include/mpcg_active.h)
ACTIVE_EXIT_SKIPPED = -100


def _signatures() -> dict:
    i, d, vp, ptr = C.c_int, C.c_double, C.c_void_p, C.POINTER
    P, IO = ptr(MpcgProblem), ptr(MpcgIo)
    FS, FT, GT = ptr(MpcgFleetSettings), ptr(MpcgFleetState), ptr(MpcgGuidanceState)
    strs, ints, dbls = ptr(C.c_char_p), ptr(i), ptr(d)
    return {
        "mpcg.h": {
            "mpcg_abi_version": (i, []),
            "mpcg_last_error": (C.c_char_p, []),
            "mpcg_supported": (i, [P]),
            "mpcg_num_h": (i, [P]),
            "mpcg_lam_size": (i, [P]),
            "mpcg_qp_mem_size": (i, [P]),
            "mpcg_problem_from_map": (i, [P, i, i, i, i, strs, ints, dbls, dbls, d, i]),
            "mpcg_problem_from_map_model": (i, [P, i, i, i, i, i, strs, ints, dbls, dbls, d, i]),
            "mpcg_solve": (i, [P, i, IO, vp]),
            "mpcg_context_create": (vp, [P, i]),
            "mpcg_context_destroy": (None, [vp]),
            "mpcg_context_solve": (i, [vp, i, IO]),
            "mpcg_context_set_iterations": (i, [vp, i]),
            "mpcg_solve_batch_device": (i, [P, i] + [vp] * 9),
            "mpcg_solve_batch_host": (i, [P, i] + [vp] * 8),
            "mpcg_select_best_device": (i, [i, i, i, vp, vp, vp, vp, d, vp, vp, d, vp, vp, vp, vp]),
            "mpcg_prepare": (i, [P, i, i, ptr(MpcgSceneIo)] + [vp] * 6),
            "mpcg_advance": (i, [P, i, i, ptr(MpcgStepIo)] + [vp] * 7),
            "mpcg_prepare_scenario": (i, [P, i, i, ptr(MpcgScenarioIo)] + [vp] * 4),
            "mpcg_select_lowest_cost_device": (i, [i, i, vp, vp, vp, vp]),
            "mpcg_winner_records_device": (i, [i, i, i, i, i] + [vp] * 6),
            "mpcg_release_stream_workspace": (i, [vp]),
            "mpcg_debug_set_tail_levels": (i, [vp, i]),
            "mpcg_instance_traits": (i, [P, C.c_char_p, i]),
            "mpcg_problem_set_qp_profile": (i, [P, i]),
        },
        "mpcg_fleet.h": {
            "mpcg_fleet_obstacles": (i, [P, i, i, i, FS, FT, vp, vp, vp, vp, d, vp, vp, vp]),
            "mpcg_fleet_publish": (i, [P, i, i, i, FS, FT, vp, vp, vp, vp, vp, d, vp, vp, vp]),
        },
        "mpcg_path.h": {
            "mpcg_path_update": (i, [P, i, ptr(MpcgPathTable)] + [vp] * 7),
            "mpcg_path_command": (i, [P, i, i, ptr(MpcgPathSettings), vp, vp, vp, vp, vp, i, vp, vp, vp]),
        },
        "mpcg_road.h": {
            "mpcg_road_halfspaces": (i, [P, i, i, i, ptr(MpcgRoadSettings), ptr(MpcgPathTable), vp, ptr(MpcgRoadIo),
                                         vp, vp, vp]),
        },
        "mpcg_guidance.h": {
            "mpcg_guidance_update": (i, [P, i, i, ptr(MpcgGuidanceSettings), vp, vp, vp, vp, GT, ptr(MpcgGuidanceOut),
                                         vp]),
            "mpcg_guidance_mask": (i, [i, i, vp, vp, vp]),
            "mpcg_guidance_select": (i, [i, i, vp, vp, vp, vp, GT, vp]),
        },
        "mpcg_active.h": {
            "mpcg_active_plan": (i, [i, vp, vp, vp, vp, vp]),
            "mpcg_active_gather": (i, [P, i, vp, IO, IO, vp]),
            "mpcg_active_scatter": (i, [P, i, vp, IO, IO, vp]),
            "mpcg_active_ws_create": (vp, [P, i, i, i, i]),
            "mpcg_active_ws_destroy": (None, [vp]),
            "mpcg_active_ws_read_plan": (i, [vp, i, vp, vp, vp]),
            "mpcg_solve_active": (i, [P, i, IO, vp, vp, ints, vp]),
        },
        # exported without a public header: instance registration (csrc/mpcg_instance.h), test and
        # diagnostic hooks (mpcg_kernels.hip)
        None: {
            "mpcg_rejected_instances": (i, []),
            "mpcg_debug_set_queue": (i, [vp, C.c_uint]),
            "mpcg_debug_set_stamp_buffer": (None, [vp]),
        },
    }


# Every function of libmpcg.so that Python calls, by the public header under include/ that declares it:
# name -> (restype, argtypes).  native._load() applies it; a new layer adds its group here
# (DESIGN.md "The host-side seam").  The *_EXPORTS tuples are the groups' names.
SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES["mpcg.h"])
FLEET_EXPORTS = tuple(SIGNATURES["mpcg_fleet.h"])
PATH_EXPORTS = tuple(SIGNATURES["mpcg_path.h"])
ROAD_EXPORTS = tuple(SIGNATURES["mpcg_road.h"])
GUIDANCE_EXPORTS = tuple(SIGNATURES["mpcg_guidance.h"])
ACTIVE_EXPORTS = tuple(SIGNATURES["mpcg_active.h"])


def _later_signatures() -> dict:
    i, vp, ptr = C.c_int, C.c_void_p, C.POINTER
    return {
        "mpcg_decomp.h": {
            "mpcg_decomp_halfspaces": (i, [ptr(MpcgProblem), i, i, ptr(MpcgDecompSettings), ptr(MpcgPathTable), vp,
                                           ptr(MpcgDecompIo), vp, vp, vp, vp, vp, vp]),
        },
    }


# The layers of _build.LATER_LAYERS, in the form of SIGNATURES (whose key set tests/test_layer_abi.py pins to the
# first five layers); native._load() applies both tables in one loop.
LATER_SIGNATURES = _later_signatures()
DECOMP_EXPORTS = tuple(LATER_SIGNATURES["mpcg_decomp.h"])


class MpcgScenarioSampleIo(C.Structure):
    """Mirror of `mpcg_scenario_sample_io` (include/mpcg_scenario.h)."""
    _fields_ = [("stage_params", C.c_void_p), ("state", C.c_void_p), ("main_warm", C.c_void_p),
                ("obst", C.c_void_p), ("obst_meta", C.c_void_p), ("bank", C.c_void_p), ("batch_idx", C.c_void_p),
                ("n_obs", C.c_int), ("n_per", C.c_int), ("n_batches", C.c_int),
                ("seed", C.c_ulonglong), ("draw", C.c_ulonglong),
                ("robot_radius", C.c_double), ("deceleration", C.c_double)]


class MpcgScenarioStepIo(C.Structure):
    """Mirror of `mpcg_scenario_step_io` (include/mpcg_scenario.h)."""
    _fields_ = [("best", C.c_void_p), ("exit_code", C.c_void_p), ("xtraj", C.c_void_p), ("utraj", C.c_void_p),
                ("lam_out", C.c_void_p), ("state_next", C.c_void_p), ("deceleration", C.c_double)]


# the scenario sampler (include/mpcg_scenario.h)
SCENARIO_MAX_SAMPLES, SCENARIO_MAX_OBS, SCENARIO_MAX_N, SCENARIO_MAX_ROWS = 2048, 64, 32, 32
SCENARIO_MIX_C1, SCENARIO_MIX_C2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
SCENARIO_MIX_M1, SCENARIO_MIX_M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


class MpcgTrackSettings(C.Structure):
    """Mirror of `mpcg_track_settings` (include/mpcg_tracks.h)."""
    _fields_ = [("obstacle_radius", C.c_double), ("probabilistic", C.c_int), ("chi_gaussian", C.c_double)]


# the tracked-object layer (include/mpcg_tracks.h)
TRACK_NONE, TRACK_UNSEEN, TRACK_DISC, TRACK_CYLINDER, TRACK_BOX = -1, 0, 1, 2, 3
TRACKS_MAX_N, TRACKS_MAX_OBJECTS, TRACKS_MAX_ROWS, TRACKS_MAX_ELL = 32, 32, 64, 32


def _open_signatures() -> dict:
    i, vp, ptr = C.c_int, C.c_void_p, C.POINTER
    P, SIO = ptr(MpcgProblem), ptr(MpcgScenarioSampleIo)
    TS = ptr(MpcgTrackSettings)
    return {
        "mpcg_scenario.h": {
            "mpcg_scenario_sample_prepare": (i, [P, i, i, SIO, vp, vp, vp, vp]),
            "mpcg_scenario_samples": (i, [P, i, i, SIO, vp, vp]),
            "mpcg_scenario_advance": (i, [P, i, i, ptr(MpcgScenarioStepIo), vp, vp, vp]),
        },
        "mpcg_tracks.h": {
            "mpcg_tracks_rows": (i, [P, i, i, TS] + [vp] * 9),
            "mpcg_obstacle_select": (i, [P, i, i, TS, vp, vp, vp, vp, vp, i, vp, vp, vp, vp]),
        },
    }


# The layers of _build.OPEN_LAYERS, in the form of SIGNATURES: the table a new layer adds its group to
# (tests/test_layer_abi_open.py pins no key set); native._load() applies all three tables in one loop.
OPEN_SIGNATURES = _open_signatures()
SCENARIO_EXPORTS = tuple(OPEN_SIGNATURES["mpcg_scenario.h"])
TRACKS_EXPORTS = tuple(OPEN_SIGNATURES["mpcg_tracks.h"])
