"""ctypes binding of the C ABI (include/mpcg.h) implemented by libmpcg.so.

The product path: no fallback.  If libmpcg.so is missing or cannot be loaded
the import of this module raises, and every solve fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
# Load torch's HIP runtime first: libmpcg.so's libamdhip64.so.7 /
# libhsa-runtime64.so.1 then resolve (by SONAME) to the copies torch already
# mapped, so the process holds exactly one HIP runtime and device pointers
# from torch tensors are valid in our kernels.
import torch

from .native_spec import (ABI_VERSION, ACTIVE_EXPORTS, DECOMP_EXPORTS, DEFAULT_OPTIONS, EXPORTS,  # noqa: F401
                          FLEET_EXPORTS, GUIDANCE_CANDIDATES, LATER_SIGNATURES, MpcgDecompIo, MpcgDecompSettings,
                          GUIDANCE_EXPORTS, INFO_STRIDE, NU, NVAR, NX, PATH_EXPORTS, SIGNATURES, STATS_STRIDE, UNICYCLE_LB,
                          UNICYCLE_UB, MpcgFleetSettings, MpcgFleetState, MpcgGuidanceOut, MpcgGuidanceSettings,
                          MpcgGuidanceState, MpcgIo, MpcgPathSettings, MpcgPathTable, MpcgProblem, MpcgRoadIo,
                          MpcgRoadSettings, MpcgSceneIo, MpcgStepIo, MpcgScenarioIo, ROAD_EXPORTS, problem_from_layout,
                          OPEN_SIGNATURES, SCENARIO_EXPORTS, MpcgScenarioSampleIo, MpcgScenarioStepIo, TRACKS_EXPORTS,
                          MpcgTrackSettings)

PKG = os.path.dirname(os.path.abspath(__file__))
# MPCG_LIB selects a diagnostic build (e.g. libmpcg_stamps.so); default the production library
LIB_PATH = os.environ.get("MPCG_LIB") or os.path.join(PKG, "libmpcg.so")
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for group in list(SIGNATURES.values()) + list(LATER_SIGNATURES.values()) + list(OPEN_SIGNATURES.values()):
        for name, (restype, argtypes) in group.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    # (MPCG_ABI_ACCEPT_OLDER, A/B timing runs of an earlier round's library only: ABI versions whose
    # mpcg_problem is a prefix of this one -- later ABIs only append fields)
    older = {int(v) for v in os.environ.get("MPCG_ABI_ACCEPT_OLDER", "").split(",") if v.strip().isdigit()}
    if lib.mpcg_abi_version() != ABI_VERSION and lib.mpcg_abi_version() not in {v for v in older if 8 <= v < ABI_VERSION}:
        raise ImportError(f"{LIB_PATH}: ABI {lib.mpcg_abi_version()} != {ABI_VERSION}; rebuild")
    return lib


lib = _load()


def load_instances(path: str):
    """Load a library of compiled kernel instances (codegen mpcg_instance.hip, built by
    _build.build_instance or compiled into a drop-in libmpc_planner_solver.so): its static
    initialisers register the instances with libmpcg.so, so mpcg_supported() accepts the
    generated solver's dimensions from then on."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: build it first (oscar_mpc_planner_mr_modification_amd._build.build_instance)")
    before = lib.mpcg_rejected_instances()
    h = C.CDLL(path, mode=C.RTLD_GLOBAL)
    if lib.mpcg_rejected_instances() != before:
        raise ImportError(f"{path}: compiled against another ABI than {LIB_PATH}; rebuild it "
                          "(oscar_mpc_planner_mr_modification_amd._build.build_instance)")
    return h


def supported(pr: MpcgProblem) -> bool:
    return lib.mpcg_supported(C.byref(pr)) == 0


def last_error() -> str:
    return lib.mpcg_last_error().decode()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _addr(t):
    return None if t is None else t.data_ptr()


def _stream(stream, dev):
    """the hipStream_t of `stream` (a torch.cuda stream), or of the current stream of `dev` when it is None"""
    return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(dev)).cuda_stream)


def _dev(name, t, dtype, size=None):
    """assert that `t` is a contiguous device tensor of `dtype`, of the shape `size` (a tuple) or of `size`
    elements (an int)"""
    assert t.dtype == dtype and t.is_cuda and t.is_contiguous(), (name, t.dtype, t.device)
    if size is not None:
        assert (t.numel() == size if isinstance(size, int) else tuple(t.shape) == size), (name, tuple(t.shape), size)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def lam_stride(pr: MpcgProblem) -> int:
    """Doubles per stage of a multiplier block: nx + nh (include/mpcg.h, mpcg_io)."""
    return pr.nx + pr.n_lin + pr.n_ell + pr.n_scen


def qp_mem_size(pr: MpcgProblem) -> int:
    """Doubles of one solve's QP memory (mpcg_io.qp_in / qp_out, opaque)."""
    n = lib.mpcg_qp_mem_size(C.byref(pr))
    if n < 0:
        raise RuntimeError(f"mpcg_qp_mem_size: {last_error() or 'no compiled instance'}")
    return n


def _solve_outputs(pr: MpcgProblem, B: int, dev, out, lam_out, qp_out, stats) -> dict:
    """solve_batch_device's result dict: `out`, or a new one when it is None, with the optional blocks that
    are asked for allocated where it lacks them (a dict that is passed in is not checked)"""
    N, nx = pr.N, pr.nx
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    if out is None:
        out = dict(xtraj=new(F64, B, N + 1, nx), utraj=new(F64, B, N, pr.nu), pobj=new(F64, B), exit=new(I32, B),
                   info=new(I32, B, INFO_STRIDE))
    if lam_out and "lam" not in out:
        out["lam"] = new(F64, B, N, lam_stride(pr))
    if qp_out and "qp" not in out:
        out["qp"] = new(F64, B, qp_mem_size(pr))
    if stats and "stats" not in out:
        out["stats"] = new(F64, B, STATS_STRIDE)
    return out


def _solve_io(pr: MpcgProblem, params, warm, xinit, lam_in, qp_in, out: dict, lam_out, qp_out, stats) -> MpcgIo:
    """The mpcg_io of a solve of params.shape[0] problems: the inputs, checked, and the blocks of `out`
    (_solve_outputs) that the call asks for."""
    B, N, nx = params.shape[0], pr.N, pr.nx
    _dev("params", params, F64, (B, N, pr.npar))
    _dev("warm", warm, F64, (B, N + 1, pr.nu + nx))
    _dev("xinit", xinit, F64, (B, nx))
    if lam_in is not None:
        _dev("lam_in", lam_in, F64, (B, N, lam_stride(pr)))
    if qp_in is not None:
        _dev("qp_in", qp_in, F64, (B, qp_mem_size(pr)))
    return MpcgIo(params.data_ptr(), warm.data_ptr(), xinit.data_ptr(), _addr(lam_in),
                  out["xtraj"].data_ptr(), out["utraj"].data_ptr(), out["pobj"].data_ptr(), out["exit"].data_ptr(),
                  _addr(out.get("info")), out["lam"].data_ptr() if lam_out else None, _addr(qp_in),
                  out["qp"].data_ptr() if qp_out else None, out["stats"].data_ptr() if stats else None)


def solve_batch_device(pr: MpcgProblem, params, warm, xinit, out=None, stream=None, lam_in=None,
                       lam_out=False, qp_in=None, qp_out=False, stats=False):
    """Batched solve on device tensors (torch, float64, on the current HIP device).
    params (B, N, npar), warm (B, N+1, nu+nx), xinit (B, nx), optional lam_in
    (B, N, nx + nh) NLP multipliers and qp_in (B, qp_mem_size) QP memory carried
    over from the previous solve.  Returns a dict of device tensors (+ "lam" if
    lam_out, "qp" if qp_out, "stats" (B, 4) NLP residuals if stats);
    asynchronous on `stream` (torch.cuda stream or None = current)."""
    B, dev = params.shape[0], params.device
    out = _solve_outputs(pr, B, dev, out, lam_out, qp_out, stats)
    io = _solve_io(pr, params, warm, xinit, lam_in, qp_in, out, lam_out, qp_out, stats)
    _check(lib.mpcg_solve(C.byref(pr), B, C.byref(io), _stream(stream, dev)), "mpcg_solve")
    return out


def _host_arrays(pr: MpcgProblem, params, warm, xinit):
    """The inputs of a host-buffer solve as contiguous float64 arrays, their shapes checked, and its zeroed
    result dict: (B, params, warm, xinit, result)."""
    params, warm, xinit = (np.ascontiguousarray(a, np.float64) for a in (params, warm, xinit))
    B, N, nx, nu = params.shape[0], pr.N, pr.nx, pr.nu
    assert params.shape == (B, N, pr.npar) and warm.shape == (B, N + 1, nu + nx) and xinit.shape == (B, nx)
    r = dict(xtraj=np.zeros((B, N + 1, nx)), utraj=np.zeros((B, N, nu)), pobj=np.zeros(B),
             exit=np.zeros(B, np.int32), info=np.zeros((B, INFO_STRIDE), np.int32))
    return B, params, warm, xinit, r


class Context:
    """A persistent host-buffer solve context (mpcg_context_*): what one
    drop-in `MPCPlanner::Solver` holds.  Synchronous `solve`."""

    def __init__(self, pr: MpcgProblem, max_batch: int):
        self.pr = pr
        self.max_batch = max_batch
        self._c = lib.mpcg_context_create(C.byref(pr), max_batch)
        if not self._c:
            raise RuntimeError(f"mpcg_context_create failed: {last_error()}")

    def close(self):
        if self._c:
            lib.mpcg_context_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_iterations(self, sqp_iters: int):
        _check(lib.mpcg_context_set_iterations(self._c, sqp_iters), "mpcg_context_set_iterations")

    def solve(self, params, warm, xinit, lam_in=None, lam_out=False, qp_in=None, qp_out=False, stats=False):
        pr = self.pr
        B, params, warm, xinit, r = _host_arrays(pr, params, warm, xinit)
        N, LS = pr.N, lam_stride(pr)
        if lam_in is not None:
            lam_in = np.ascontiguousarray(lam_in, np.float64)
            assert lam_in.shape == (B, N, LS)
        if lam_out:
            r["lam"] = np.zeros((B, N, LS))
        if qp_in is not None:
            qp_in = np.ascontiguousarray(qp_in, np.float64)
            assert qp_in.shape == (B, qp_mem_size(pr))
        if qp_out:
            r["qp"] = np.zeros((B, qp_mem_size(pr)))
        if stats:
            r["stats"] = np.zeros((B, STATS_STRIDE))
        a = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        io = MpcgIo(a(params), a(warm), a(xinit), a(lam_in), a(r["xtraj"]), a(r["utraj"]), a(r["pobj"]),
                    a(r["exit"]), a(r["info"]), a(r.get("lam")), a(qp_in), a(r.get("qp")), a(r.get("stats")))
        _check(lib.mpcg_context_solve(self._c, B, C.byref(io)), "mpcg_context_solve")
        return r


def solve_batch_host(pr: MpcgProblem, params: np.ndarray, warm: np.ndarray, xinit: np.ndarray):
    """Host-buffer solve through the same kernels (copies in/out, synchronous)."""
    B, params, warm, xinit, r = _host_arrays(pr, params, warm, xinit)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.mpcg_solve_batch_host(C.byref(pr), B, vp(params), vp(warm), vp(xinit), vp(r["xtraj"]), vp(r["utraj"]),
                                   vp(r["pobj"]), vp(r["exit"]), vp(r["info"]))
    _check(rc, "mpcg_solve_batch_host")
    return r


def select_best_device(n_scenes, n_guesses, N, xtraj, pobj, exit_code, prev_traj=None, w_cons=0.0,
                       consistency_enabled=None, previously_selected=None, selection_weight=1.0,
                       disabled=None, stream=None, with_objective: bool = True):
    """mpcg_select_best_device -> (best, objective); with_objective=False passes no objective
    buffer (NULL) and returns (best, None)."""
    dev = pobj.device
    best = torch.empty((n_scenes,), dtype=I32, device=dev)
    objective = torch.empty((n_scenes * n_guesses,), dtype=F64, device=dev) if with_objective else None
    rc = lib.mpcg_select_best_device(n_scenes, n_guesses, N, _ptr(xtraj), _ptr(pobj), _ptr(exit_code),
                                     _ptr(prev_traj), float(w_cons), _ptr(consistency_enabled),
                                     _ptr(previously_selected), float(selection_weight), _ptr(disabled),
                                     _ptr(best), _ptr(objective), _stream(stream, dev))
    _check(rc, "mpcg_select_best_device")
    return best, objective


def winner_records_device(xtraj, utraj, pobj, best, n_guesses, out, stream=None):
    """mpcg_winner_records_device: the selected planner's record per scene (one launch; the device
    form of distributed.winner_records) into `out` [n_scenes][winner_width]."""
    n_scenes = best.shape[0]
    B, N1, nx = xtraj.shape
    nu = utraj.shape[2]
    assert B == n_scenes * n_guesses and out.shape[0] == n_scenes and out.shape[1] == N1 * nx + (N1 - 1) * nu + 2
    for k, t in dict(xtraj=xtraj, utraj=utraj, pobj=pobj, out=out).items():
        _dev(k, t, F64)
    _dev("best", best, I32)
    rc = lib.mpcg_winner_records_device(n_scenes, n_guesses, N1 - 1, nx, nu, _ptr(xtraj), _ptr(utraj), _ptr(pobj),
                                        _ptr(best), _ptr(out), _stream(stream, pobj.device))
    _check(rc, "mpcg_winner_records_device")
    return out


def scenes_to_device(scenes, device):
    """producers.Scenes -> dict of contiguous device tensors (float64 / uint8)."""
    def t(a, dt=F64):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)

    return dict(stage_params=t(scenes.stage_params), state=t(scenes.state), obst=t(scenes.obst),
                obst_meta=t(scenes.obst_meta), guidance=t(scenes.guidance),
                guided=t(scenes.guided.astype(np.uint8), U8), main_warm=t(scenes.main_warm),
                prev_traj=t(scenes.prev_traj), prev_elapsed=t(scenes.prev_elapsed),
                consistency_on=t(scenes.consistency_on.astype(np.uint8), U8),
                previously_selected=t(scenes.previously_selected.astype(np.uint8), U8),
                n_scenes=scenes.n_scenes, n_guesses=scenes.n_guesses)


def prepare_device(pr: MpcgProblem, dsc: dict, robot_radius: float, w_consistency: float, deceleration: float = 3.0,
                   out=None, stream=None, warmstart_with_mpc_solution: bool = False, shift_forward: bool = False):
    """mpcg_prepare: per-planner solver inputs from device-resident scene data
    (`scenes_to_device`).  Returns dict(params, warm, xinit, prev_interp,
    consistency_active) of device tensors; asynchronous on `stream`.
    warmstart_with_mpc_solution: guided planners whose dsc["existing_guidance"] is set start
    from their own previous output dsc["planner_xtraj"] / ["planner_utraj"]
    (guidance_constraints.cpp:335-338)."""
    S, G, N = dsc["n_scenes"], dsc["n_guesses"], pr.N
    dev = dsc["state"].device
    assert tuple(dsc["stage_params"].shape) == (S, pr.npar)
    assert tuple(dsc["obst"].shape) == (S, pr.n_ell, N, 5) and tuple(dsc["guidance"].shape) == (S, G, N + 1, 4)
    if out is None:
        out = dict(params=torch.empty((S * G, N, pr.npar), dtype=F64, device=dev),
                   warm=torch.empty((S * G, N + 1, NVAR), dtype=F64, device=dev),
                   xinit=torch.empty((S * G, NX), dtype=F64, device=dev),
                   prev_interp=torch.empty((S, N, 2), dtype=F64, device=dev),
                   consistency_active=torch.empty((S * G,), dtype=U8, device=dev))
    p = lambda k: _addr(dsc.get(k))  # noqa: E731
    sio = MpcgSceneIo(p("stage_params"), p("state"), p("obst"), p("obst_meta"), p("guidance"), p("guided"),
                      p("main_warm"), p("prev_traj"), p("prev_elapsed"), p("consistency_on"),
                      float(robot_radius), float(w_consistency), float(deceleration),
                      p("planner_xtraj"), p("planner_utraj"), p("existing_guidance"),
                      int(bool(warmstart_with_mpc_solution)), int(bool(shift_forward)))
    rc = lib.mpcg_prepare(C.byref(pr), S, G, C.byref(sio), _ptr(out["params"]), _ptr(out["warm"]), _ptr(out["xinit"]),
                          _ptr(out["prev_interp"]), _ptr(out["consistency_active"]), _stream(stream, dev))
    _check(rc, "mpcg_prepare")
    return out


def advance_device(pr: MpcgProblem, S: int, G: int, best, exit_code, xtraj, utraj, warm, lam_out, state_next, guided,
                   elapsed: float, deceleration: float = 3.0, shift_forward: bool = False,
                   consistency_on_non_guided: bool = True, topology=None, topology_next=None,
                   previously_selected=None, stream=None, out=None):
    """mpcg_advance: the carried state of the next control step (device tensors).
    out: preallocated dict(main_warm, prev_traj, prev_elapsed, consistency_on, previously_selected,
    lam) to write into; its lam may be None (no multipliers carried) or a tensor also when lam_out
    is None (the kernel then writes zeros)."""
    dev = xtraj.device
    N = pr.N
    shapes = dict(main_warm=(S, N + 1, NVAR), prev_traj=(S, N, 2), prev_elapsed=(S,), consistency_on=(S, G),
                  previously_selected=(S, G), lam=(S * G, N, lam_stride(pr)))
    dtypes = dict(consistency_on=U8, previously_selected=U8)
    if out is None:
        out = {k: torch.empty(shp, dtype=dtypes.get(k, F64), device=dev) for k, shp in shapes.items()
               if k != "lam" or lam_out is not None}
        out.setdefault("lam", None)
    else:
        for k, shp in shapes.items():
            if k == "lam" and out[k] is None:
                continue
            _dev(k, out[k], dtypes.get(k, F64), shp)
            assert out[k].device == dev, k
    best32 = best.to(I32).contiguous()
    sio = MpcgStepIo(best32.data_ptr(), exit_code.data_ptr(), xtraj.data_ptr(), utraj.data_ptr(), warm.data_ptr(),
                     _addr(lam_out), state_next.data_ptr(), guided.data_ptr(), _addr(topology), _addr(topology_next),
                     _addr(previously_selected), int(shift_forward), int(consistency_on_non_guided), float(elapsed),
                     float(deceleration))
    rc = lib.mpcg_advance(C.byref(pr), S, G, C.byref(sio), _ptr(out["main_warm"]), _ptr(out["prev_traj"]),
                          _ptr(out["prev_elapsed"]), _ptr(out["consistency_on"]), _ptr(out["previously_selected"]),
                          _ptr(out["lam"]), _stream(stream, dev))
    _check(rc, "mpcg_advance")
    return out


def prepare_scenario_device(pr: MpcgProblem, n_solvers: int, stage_params, state, samples, radius: float,
                            deceleration: float, main_warm=None, out=None, stream=None):
    """SH-MPC solver inputs on the GPU (mpcg_prepare_scenario): stage_params
    (S, npar), state (S, nx), samples (S*P, N, M, 2), optional main_warm
    (S, N+1, nu+nx) -> dict(params, warm, xinit) device tensors."""
    S = stage_params.shape[0]
    N, nx = pr.N, pr.nx
    B = S * n_solvers
    _dev("stage_params", stage_params, F64)
    _dev("state", state, F64, (S, nx))
    _dev("samples", samples, F64)
    if main_warm is not None:
        _dev("main_warm", main_warm, F64)
    assert stage_params.shape[1] == pr.npar
    assert samples.shape[0] == B and samples.shape[1] == N and samples.shape[3] == 2
    dev = stage_params.device
    if out is None:
        out = dict(params=torch.empty((B, N, pr.npar), dtype=F64, device=dev),
                   warm=torch.empty((B, N + 1, NU + nx), dtype=F64, device=dev),
                   xinit=torch.empty((B, nx), dtype=F64, device=dev))
    io = MpcgScenarioIo(stage_params.data_ptr(), state.data_ptr(), _addr(main_warm), samples.data_ptr(),
                        int(samples.shape[2]), float(radius), float(deceleration))
    rc = lib.mpcg_prepare_scenario(C.byref(pr), S, n_solvers, C.byref(io), _ptr(out["params"]), _ptr(out["warm"]),
                                   _ptr(out["xinit"]), _stream(stream, dev))
    _check(rc, "mpcg_prepare_scenario")
    return out


def select_lowest_cost_device(n_scenes, n_solvers, pobj, exit_code, out=None, stream=None):
    dev = pobj.device
    best = out if out is not None else torch.empty((n_scenes,), dtype=I32, device=dev)
    rc = lib.mpcg_select_lowest_cost_device(n_scenes, n_solvers, _ptr(pobj), _ptr(exit_code), _ptr(best),
                                            _stream(stream, dev))
    _check(rc, "mpcg_select_lowest_cost_device")
    return best


def _fleet_state(fstate: dict, S: int, N: int) -> MpcgFleetState:
    sizes = dict(sent_plan=S * N * 3, sent_time=S, last_send_time=S, prev_topology=S)
    for k, n in sizes.items():
        _dev(k, fstate[k], I32 if k == "prev_topology" else F64, n)
    return MpcgFleetState(*(fstate[k].data_ptr() for k in sizes))


def fleet_obstacles_device(pr: MpcgProblem, F: int, R: int, settings: MpcgFleetSettings, fstate: dict, state, now: float,
                           obst, obst_meta, array_obst=None, array_meta=None, array_id=None, stream=None):
    """mpcg_fleet_obstacles (include/mpcg_fleet.h): shift every sender's plan in `fstate`
    (dict sent_plan (F, R, N, 3), sent_time, last_send_time (F, R) float64, prev_topology (F, R)
    int32, device tensors, updated in place) to `now`, then write every robot's obstacle rows into
    obst (S, n_ell, N, 5) / obst_meta (S, n_ell, 2), S = F * R.  array_obst (F, A, N, 5), array_meta
    (F, A, 2), array_id (F, A) int32 or None: the fleets' non-communicating obstacles.
    Asynchronous on `stream`; nothing is allocated."""
    S, N = F * R, pr.N
    A = 0 if array_obst is None else array_obst.shape[1]
    _dev("state", state, F64, (S, pr.nx))
    _dev("obst", obst, F64, (S, pr.n_ell, N, 5))
    _dev("obst_meta", obst_meta, F64, (S, pr.n_ell, 2))
    if A:
        _dev("array_obst", array_obst, F64, (F, A, N, 5))
        _dev("array_meta", array_meta, F64, (F, A, 2))
        if array_id is not None:
            _dev("array_id", array_id, I32, (F, A))
    st = _fleet_state(fstate, S, N)
    rc = lib.mpcg_fleet_obstacles(C.byref(pr), F, R, A, C.byref(settings), C.byref(st), _ptr(state),
                                  _ptr(array_obst) if A else None, _ptr(array_meta) if A else None,
                                  _ptr(array_id) if A else None, float(now), _ptr(obst), _ptr(obst_meta),
                                  _stream(stream, state.device))
    _check(rc, "mpcg_fleet_obstacles")


def fleet_publish_device(pr: MpcgProblem, F: int, R: int, G: int, settings: MpcgFleetSettings, fstate: dict, best, xtraj,
                         state, now: float, reason, published, topology=None, guided=None, stream=None):
    """mpcg_fleet_publish (include/mpcg_fleet.h): after the solves of step `now`, every robot's
    plan, selected topology and communication trigger; publishers' plans replace their entry of
    `fstate` in place.  best (S,) int32, xtraj (S*G, N+1, nx), state (S, nx), topology (S, G) int32
    or None, guided (S, G) uint8 or None; outputs reason (S,) int32, published (S,) uint8.
    Asynchronous on `stream`; nothing is allocated."""
    S, N = F * R, pr.N
    _dev("best", best, I32, S)
    _dev("xtraj", xtraj, F64, (S * G, N + 1, pr.nx))
    _dev("state", state, F64, (S, pr.nx))
    _dev("reason", reason, I32, S)
    _dev("published", published, U8, S)
    if topology is not None:
        _dev("topology", topology, I32, S * G)
    if guided is not None:
        _dev("guided", guided, U8, S * G)
    st = _fleet_state(fstate, S, N)
    rc = lib.mpcg_fleet_publish(C.byref(pr), F, R, G, C.byref(settings), C.byref(st), _ptr(best), _ptr(xtraj),
                                _ptr(state), _ptr(topology), _ptr(guided), float(now), _ptr(reason), _ptr(published),
                                _stream(stream, state.device))
    _check(rc, "mpcg_fleet_publish")


def path_table_device(table, path_of, device) -> dict:
    """paths.PathTable + path_of (S,) -> the device tensors and the mpcg_path_table of
    include/mpcg_path.h (dict coef, knots, n_segments, path_of, path_of_host, native)."""
    coef = torch.from_numpy(np.ascontiguousarray(table.coef, np.float64)).to(device)
    knots = torch.from_numpy(np.ascontiguousarray(table.knots, np.float64)).to(device)
    nseg = torch.from_numpy(np.ascontiguousarray(table.n_segments, np.int32)).to(device)
    po_host = np.ascontiguousarray(path_of, np.int32)
    po = torch.from_numpy(po_host).to(device)
    P, M = coef.shape[0], coef.shape[1]
    assert tuple(coef.shape) == (P, M, 8) and tuple(knots.shape) == (P, M + 1) and tuple(nseg.shape) == (P,)
    nat = MpcgPathTable(coef.data_ptr(), knots.data_ptr(), nseg.data_ptr(), po.data_ptr(), P, M)
    return dict(coef=coef, knots=knots, n_segments=nseg, path_of=po, path_of_host=po_host, native=nat)


def path_update_device(pr: MpcgProblem, dtable: dict, state, closest_segment, closest_s, stage_params, reached,
                       stream=None):
    """mpcg_path_update (include/mpcg_path.h): the closest point of every scene's state (S, nx) on its
    path (`dtable`: path_table_device), closest_segment (S,) int32 in / out (-1: not initialised),
    closest_s (S,) float64, the window of n_seg segments into stage_params (S, npar) and reached (S,)
    uint8.  Asynchronous on `stream`; nothing is allocated."""
    S = state.shape[0]
    _dev("state", state, F64, (S, pr.nx))
    _dev("stage_params", stage_params, F64, (S, pr.npar))
    _dev("closest_s", closest_s, F64, S)
    _dev("closest_segment", closest_segment, I32, S)
    _dev("reached", reached, U8, S)
    assert dtable["path_of"].numel() == S
    rc = lib.mpcg_path_update(C.byref(pr), S, C.byref(dtable["native"]), dtable["path_of_host"].ctypes.data,
                              _ptr(state), _ptr(closest_segment), _ptr(closest_s), _ptr(stage_params), _ptr(reached),
                              _stream(stream, state.device))
    _check(rc, "mpcg_path_update")


def path_command_device(pr: MpcgProblem, G: int, settings: MpcgPathSettings, best, xtraj, utraj, state, cmd,
                        closest_s=None, spline_slot: int = -1, state_next=None, stream=None):
    """mpcg_path_command (include/mpcg_path.h): cmd (S, 2) = (v, w) from best (S,) int32, the winner's
    xtraj (S*G, N+1, nx) / utraj (S*G, N, nu) and state (S, nx); with settings.plant, state_next (S, nx)
    from the kinematic stand-in plant, its entry spline_slot set to closest_s (S,).  Asynchronous on
    `stream`; nothing is allocated."""
    S, N = state.shape[0], pr.N
    _dev("best", best, I32, S)
    _dev("xtraj", xtraj, F64, (S * G, N + 1, pr.nx))
    _dev("utraj", utraj, F64, (S * G, N, pr.nu))
    _dev("state", state, F64, (S, pr.nx))
    _dev("cmd", cmd, F64, (S, 2))
    if state_next is not None:
        _dev("state_next", state_next, F64, (S, pr.nx))
    if closest_s is not None:
        _dev("closest_s", closest_s, F64, S)
    rc = lib.mpcg_path_command(C.byref(pr), S, G, C.byref(settings), _ptr(best), _ptr(xtraj), _ptr(utraj), _ptr(state),
                               _ptr(closest_s), int(spline_slot), _ptr(cmd), _ptr(state_next),
                               _stream(stream, state.device))
    _check(rc, "mpcg_path_command")


def road_bounds_device(left_coef, right_coef, device) -> dict:
    """The bound tables (P, M, 8) of the bounds mode (roads.stack_bounds) as device tensors."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)  # noqa: E731
    return dict(left=t(left_coef), right=t(right_coef))


def road_halfspaces_device(pr: MpcgProblem, G: int, max_obstacles: int, settings: MpcgRoadSettings, dtable: dict,
                           params, state=None, main_warm=None, guided=None, deceleration: float = 3.0, bounds=None,
                           halfspaces=None, stream=None):
    """mpcg_road_halfspaces (include/mpcg_road.h): the two road rows of the stages 1 .. N-1 into
    params (S*G, N, npar) as mpcg_prepare left it -- rows max_obstacles.. of the guided planners
    (guided (S, G) uint8), rows 0, 1 of the others -- at the `spline` entries of main_warm
    (S, N+1, 7), or of the braking plan from state (S, nx) when it is None.  `dtable`:
    path_table_device; `bounds`: road_bounds_device, for the bounds mode; halfspaces (S, N, 2, 3),
    optional, receives the rows per scene.  Asynchronous on `stream`; nothing is allocated."""
    S, N = dtable["path_of"].numel(), pr.N
    _dev("params", params, F64, (S * G, N, pr.npar))
    if state is not None:
        _dev("state", state, F64, (S, pr.nx))
    if main_warm is not None:
        _dev("main_warm", main_warm, F64, (S, N + 1, pr.nu + pr.nx))
    if guided is not None:
        _dev("guided", guided, U8, S * G)
    if halfspaces is not None:
        _dev("halfspaces", halfspaces, F64, (S, N, 2, 3))
    if bounds:
        _dev("bounds left", bounds["left"], F64, tuple(dtable["coef"].shape))
        _dev("bounds right", bounds["right"], F64, tuple(dtable["coef"].shape))
    io = MpcgRoadIo(_addr(state), _addr(main_warm), float(deceleration), _addr(guided),
                    bounds["left"].data_ptr() if bounds else None, bounds["right"].data_ptr() if bounds else None)
    rc = lib.mpcg_road_halfspaces(C.byref(pr), S, G, int(max_obstacles), C.byref(settings), C.byref(dtable["native"]),
                                  dtable["path_of_host"].ctypes.data, C.byref(io), _ptr(params), _ptr(halfspaces),
                                  _stream(stream, params.device))
    _check(rc, "mpcg_road_halfspaces")


def decomp_points_device(occ, n_occ, device) -> dict:
    """The occupied points occ (S, P, 2) and their counts n_occ (S,) (decomp.make_c3_decomp_scenes) as device
    tensors, with the host copy of the counts the entry point checks (dict occ, n_occ, n_occ_host)."""
    occ = np.array(occ, np.float64, order="C")
    assert occ.ndim == 3 and occ.shape[2] == 2, occ.shape
    host = np.array(n_occ, np.int32, order="C")
    assert host.shape == (occ.shape[0],)
    return dict(occ=torch.from_numpy(occ).to(device), n_occ=torch.from_numpy(host).to(device), n_occ_host=host)


def decomp_halfspaces_device(pr: MpcgProblem, G: int, settings: MpcgDecompSettings, dtable: dict, points: dict, params,
                             state, main_warm=None, halfspaces=None, n_found=None, minor_axis=None, stream=None):
    """mpcg_decomp_halfspaces (include/mpcg_decomp.h): the max_constraints = pr.n_scen decomp rows of all N
    stages into params (S*G, N, npar), every planner of a scene alike, from the occupied points `points`
    (decomp_points_device) around the path points at s advanced by the `v` entries of main_warm
    (S, N+1, nu+nx), or of the braking plan from state (S, nx) when it is None.  `dtable`: path_table_device;
    halfspaces (S, N, max_constraints, 3), n_found (S, N) int32 and minor_axis (S, N) are optional outputs.
    Asynchronous on `stream`; nothing is allocated."""
    S, N = dtable["path_of"].numel(), pr.N
    occ, n_occ = points["occ"], points["n_occ"]
    P = occ.shape[1]
    _dev("params", params, F64, (S * G, N, pr.npar))
    _dev("state", state, F64, (S, pr.nx))
    _dev("occ", occ, F64, (S, P, 2))
    _dev("n_occ", n_occ, I32, S)
    assert points["n_occ_host"].shape == (S,) and points["n_occ_host"].dtype == np.int32
    if main_warm is not None:
        _dev("main_warm", main_warm, F64, (S, N + 1, pr.nu + pr.nx))
    if halfspaces is not None:
        _dev("halfspaces", halfspaces, F64, (S, N, pr.n_scen, 3))
    if n_found is not None:
        _dev("n_found", n_found, I32, (S, N))
    if minor_axis is not None:
        _dev("minor_axis", minor_axis, F64, (S, N))
    io = MpcgDecompIo(_addr(state), _addr(main_warm), occ.data_ptr() if P else None, _addr(n_occ), int(P))
    rc = lib.mpcg_decomp_halfspaces(C.byref(pr), S, G, C.byref(settings), C.byref(dtable["native"]),
                                    dtable["path_of_host"].ctypes.data, C.byref(io), points["n_occ_host"].ctypes.data,
                                    _ptr(params), _ptr(halfspaces), _ptr(n_found), _ptr(minor_axis),
                                    _stream(stream, params.device))
    _check(rc, "mpcg_decomp_halfspaces")


def _scenario_sample_io(pr: MpcgProblem, P: int, obst, obst_meta, bank, robot_radius, deceleration, stage_params=None,
                        state=None, main_warm=None, batch_idx=None, seed: int = 0, draw: int = 0):
    """The mpcg_scenario_sample_io of S scenes x P copies, every tensor checked: (io, S, n_obs, n_per)."""
    S, n_obs = obst.shape[0], obst.shape[1]
    n_batches, n_per = bank.shape[0], bank.shape[1]
    _dev("obst", obst, F64, (S, n_obs, pr.N, 5))
    _dev("obst_meta", obst_meta, F64, (S, n_obs, 2))
    _dev("bank", bank, F64, (n_batches, n_per, 2))
    if stage_params is not None:
        _dev("stage_params", stage_params, F64, (S, pr.npar))
    if state is not None:
        _dev("state", state, F64, (S, pr.nx))
    if main_warm is not None:
        _dev("main_warm", main_warm, F64, (S, pr.N + 1, pr.nu + pr.nx))
    if batch_idx is not None:
        _dev("batch_idx", batch_idx, I32, (S * P, n_obs))
    mask = (1 << 64) - 1
    io = MpcgScenarioSampleIo(_addr(stage_params), _addr(state), _addr(main_warm), obst.data_ptr(), obst_meta.data_ptr(),
                              bank.data_ptr(), _addr(batch_idx), int(n_obs), int(n_per), int(n_batches),
                              int(seed) & mask, int(draw) & mask, float(robot_radius), float(deceleration))
    return io, S, n_obs, n_per


def scenario_sample_prepare_device(pr: MpcgProblem, n_solvers: int, stage_params, state, obst, obst_meta, bank,
                                   robot_radius: float, deceleration: float, main_warm=None, batch_idx=None,
                                   seed: int = 0, draw: int = 0, out=None, stream=None):
    """mpcg_scenario_sample_prepare (include/mpcg_scenario.h): the SH-MPC solver inputs of S scenes x P copies
    from the predictions obst (S, n_obs, N, 5) / obst_meta (S, n_obs, 2) and the bank (n_batches, n_per, 2) of
    standard-normal pairs, sampled and reduced in one launch.  The batch of copy sol for obstacle j is
    batch_idx (S*P, n_obs) int32 when given, else derived from (seed, draw).  Returns dict(params, warm,
    xinit) of device tensors (`out` when given: nothing is allocated); asynchronous on `stream`."""
    io, S, _, _ = _scenario_sample_io(pr, n_solvers, obst, obst_meta, bank, robot_radius, deceleration, stage_params,
                                      state, main_warm, batch_idx, seed, draw)
    assert stage_params is not None and state is not None
    B, N, nx, dev = S * n_solvers, pr.N, pr.nx, obst.device
    if out is None:
        out = dict(params=torch.empty((B, N, pr.npar), dtype=F64, device=dev),
                   warm=torch.empty((B, N + 1, pr.nu + nx), dtype=F64, device=dev),
                   xinit=torch.empty((B, nx), dtype=F64, device=dev))
    else:
        _dev("params", out["params"], F64, (B, N, pr.npar))
        _dev("warm", out["warm"], F64, (B, N + 1, pr.nu + nx))
        _dev("xinit", out["xinit"], F64, (B, nx))
    rc = lib.mpcg_scenario_sample_prepare(C.byref(pr), S, n_solvers, C.byref(io), _ptr(out["params"]),
                                          _ptr(out["warm"]), _ptr(out["xinit"]), _stream(stream, dev))
    _check(rc, "mpcg_scenario_sample_prepare")
    return out


def scenario_samples_device(pr: MpcgProblem, n_solvers: int, obst, obst_meta, bank, batch_idx=None, seed: int = 0,
                            draw: int = 0, out=None, stream=None):
    """mpcg_scenario_samples (include/mpcg_scenario.h): the sample tensor (S*P, N, M, 2) of mpcg_scenario_io
    (stage 0: the stage-1 values) the fused launch never stores; for tests, recordings and visualisation."""
    io, S, n_obs, n_per = _scenario_sample_io(pr, n_solvers, obst, obst_meta, bank, 0.0, 0.0, batch_idx=batch_idx,
                                              seed=seed, draw=draw)
    shape = (S * n_solvers, pr.N, n_obs * n_per, 2)
    if out is None:
        out = torch.empty(shape, dtype=F64, device=obst.device)
    _dev("samples", out, F64, shape)
    rc = lib.mpcg_scenario_samples(C.byref(pr), S, n_solvers, C.byref(io), _ptr(out), _stream(stream, obst.device))
    _check(rc, "mpcg_scenario_samples")
    return out


def scenario_advance_device(pr: MpcgProblem, S: int, n_solvers: int, best, exit_code, xtraj, utraj, lam_out, state_next,
                            deceleration: float, main_warm, lam_next=None, stream=None):
    """mpcg_scenario_advance (include/mpcg_scenario.h): main_warm (S, N+1, nu+nx) of the next SH-MPC step -- the
    winner's output shifted forward, or the braking plan from state_next (S, nx) where best (S,) int32 is
    -1 -- and lam_next (S*P, N, nx+nh), each copy's lam_out when its exit code is 1, zero otherwise.
    Asynchronous on `stream`; nothing is allocated."""
    B, N, nx = S * n_solvers, pr.N, pr.nx
    _dev("best", best, I32, S)
    _dev("exit_code", exit_code, I32, B)
    _dev("xtraj", xtraj, F64, (B, N + 1, nx))
    _dev("utraj", utraj, F64, (B, N, pr.nu))
    _dev("state_next", state_next, F64, (S, nx))
    _dev("main_warm", main_warm, F64, (S, N + 1, pr.nu + nx))
    if lam_out is not None:
        _dev("lam_out", lam_out, F64, (B, N, lam_stride(pr)))
    if lam_next is not None:
        _dev("lam_next", lam_next, F64, (B, N, lam_stride(pr)))
    io = MpcgScenarioStepIo(best.data_ptr(), exit_code.data_ptr(), xtraj.data_ptr(), utraj.data_ptr(), _addr(lam_out),
                            state_next.data_ptr(), float(deceleration))
    rc = lib.mpcg_scenario_advance(C.byref(pr), S, n_solvers, C.byref(io), _ptr(main_warm), _ptr(lam_next),
                                   _stream(stream, xtraj.device))
    _check(rc, "mpcg_scenario_advance")


def problem_with_rows(pr: MpcgProblem, n_ell: int) -> MpcgProblem:
    """A copy of `pr` whose n_ell is `n_ell`: what mpcg_obstacle_select takes from a caller whose layout holds no
    ellipsoid rows (SH-MPC: the number of predictions per scene).  The tracked-object layer reads N, dt, nx and
    n_ell only."""
    cp = MpcgProblem.from_buffer_copy(pr)
    cp.n_ell = int(n_ell)
    return cp


def track_table_device(pose, twist, dims, shape, device) -> dict:
    """The table of tracked objects (include/mpcg_tracks.h) as contiguous device tensors: pose (W, A, 3), twist
    (W, A, 2), dims (W, A, 2) float64 and shape (W, A) int32.  Device tensors of the right type are taken as
    they are, so the caller may update them in place between steps."""
    f = lambda a: torch.as_tensor(a, dtype=F64, device=device).contiguous()  # noqa: E731
    shape = torch.as_tensor(shape, dtype=I32, device=device).contiguous()
    W, A = shape.shape
    t = dict(pose=f(pose), twist=f(twist), dims=f(dims), shape=shape)
    for k, n in (("pose", 3), ("twist", 2), ("dims", 2)):
        _dev(k, t[k], F64, (W, A, n))
    return t


def track_rows_buffers(W: int, A: int, N: int, device) -> dict:
    """The candidate rows of W worlds x A object slots, C = 2 A rows per world: what mpcg_tracks_rows writes and
    mpcg_obstacle_select reads."""
    C2 = 2 * A
    return dict(rows=torch.zeros((W, C2, N, 5), dtype=F64, device=device),
                rows_meta=torch.zeros((W, C2, 2), dtype=F64, device=device),
                rows_type=torch.zeros((W, C2), dtype=I32, device=device),
                n_rows=torch.zeros((W,), dtype=I32, device=device))


def tracks_rows_device(pr: MpcgProblem, settings: MpcgTrackSettings, table: dict, out=None, stream=None) -> dict:
    """mpcg_tracks_rows (include/mpcg_tracks.h): the constant-velocity predictions of every world's tracked objects
    (`track_table_device`) as candidate rows.  Returns dict(rows (W, C, N, 5), rows_meta (W, C, 2), rows_type
    (W, C) int32, n_rows (W,) int32), C = 2 A (`out` when given: nothing is allocated); rows past n_rows are not
    written.  Asynchronous on `stream`."""
    W, A = table["shape"].shape
    _dev("shape", table["shape"], I32, (W, A))
    for k, n in (("pose", 3), ("twist", 2), ("dims", 2)):
        _dev(k, table[k], F64, (W, A, n))
    dev = table["shape"].device
    if out is None:
        out = track_rows_buffers(W, A, pr.N, dev)
    _dev("rows", out["rows"], F64, (W, 2 * A, pr.N, 5))
    _dev("rows_meta", out["rows_meta"], F64, (W, 2 * A, 2))
    _dev("rows_type", out["rows_type"], I32, (W, 2 * A))
    _dev("n_rows", out["n_rows"], I32, W)
    rc = lib.mpcg_tracks_rows(C.byref(pr), W, A, C.byref(settings), _ptr(table["pose"]), _ptr(table["twist"]),
                              _ptr(table["dims"]), _ptr(table["shape"]), _ptr(out["rows"]), _ptr(out["rows_meta"]),
                              _ptr(out["rows_type"]), _ptr(out["n_rows"]), _stream(stream, dev))
    _check(rc, "mpcg_tracks_rows")
    return out


def obstacle_select_device(pr: MpcgProblem, settings: MpcgTrackSettings, cand: dict, state, obst, obst_meta,
                           propagate: bool = False, kept=None, stream=None):
    """mpcg_obstacle_select (include/mpcg_tracks.h): keep the n_ell closest of every scene's candidate rows
    (`cand`: dict rows (S, max_rows, N, 5), rows_meta, rows_type, n_rows -- from tracks_rows_device or uploaded
    finished) or pad with dummies, then with `propagate` one more pass of the uncertainty propagation, into obst
    (S, n_ell, N, 5) / obst_meta (S, n_ell, 2); kept (S, n_ell) int32 or None: the candidate index of every
    output row.  Asynchronous on `stream`; nothing is allocated."""
    S, max_rows = cand["rows"].shape[0], cand["rows"].shape[1]
    _dev("rows", cand["rows"], F64, (S, max_rows, pr.N, 5))
    _dev("rows_meta", cand["rows_meta"], F64, (S, max_rows, 2))
    _dev("rows_type", cand["rows_type"], I32, (S, max_rows))
    _dev("n_rows", cand["n_rows"], I32, S)
    _dev("state", state, F64, (S, pr.nx))
    _dev("obst", obst, F64, (S, pr.n_ell, pr.N, 5))
    _dev("obst_meta", obst_meta, F64, (S, pr.n_ell, 2))
    if kept is not None:
        _dev("kept", kept, I32, (S, pr.n_ell))
    rc = lib.mpcg_obstacle_select(C.byref(pr), S, max_rows, C.byref(settings), _ptr(cand["rows"]),
                                  _ptr(cand["rows_meta"]), _ptr(cand["rows_type"]), _ptr(cand["n_rows"]), _ptr(state),
                                  int(bool(propagate)), _ptr(obst), _ptr(obst_meta), _ptr(kept),
                                  _stream(stream, state.device))
    _check(rc, "mpcg_obstacle_select")


class TrackObstacles:
    """tracks_obstacles_device's row scratch: the candidate rows of S scenes x A object slots, allocated once."""

    def __init__(self, pr: MpcgProblem, S: int, A: int, device):
        self.S, self.A = S, A
        self.cand = track_rows_buffers(S, A, pr.N, device)


def tracks_obstacles_device(pr: MpcgProblem, settings: MpcgTrackSettings, table: dict, state, obst, obst_meta,
                            propagate: bool = False, scratch=None, kept=None, stream=None) -> TrackObstacles:
    """mpcg_tracks_rows, then mpcg_obstacle_select: obst (S, n_ell, N, 5) / obst_meta (S, n_ell, 2) of every scene
    from its tracked objects (scene s reads world s of `table`).  `scratch` (a TrackObstacles, returned) holds
    the candidate rows between the two launches; with it nothing is allocated.  Asynchronous on `stream`."""
    S, A = table["shape"].shape
    if scratch is None:
        scratch = TrackObstacles(pr, S, A, state.device)
    assert (scratch.S, scratch.A) == (S, A), ((scratch.S, scratch.A), (S, A))
    tracks_rows_device(pr, settings, table, out=scratch.cand, stream=stream)
    obstacle_select_device(pr, settings, scratch.cand, state, obst, obst_meta, propagate=propagate, kept=kept,
                           stream=stream)
    return scratch


def _guidance_state(gstate: dict, S: int, G: int, N: int) -> MpcgGuidanceState:
    K = 2 * (G - 1)
    fields = dict(class_traj=(F64, S * K * (N + 1) * 2), class_used=(U8, S * K), planner_class=(I32, S * G),
                  selected_topology=(I32, S), prev_was_original=(U8, S))
    for k, (dtype, n) in fields.items():
        _dev(k, gstate[k], dtype, n)
    return MpcgGuidanceState(*(gstate[k].data_ptr() for k in fields))


def guidance_update_device(pr: MpcgProblem, S: int, G: int, settings: MpcgGuidanceSettings, state, stage_params, obst,
                           obst_meta, gstate: dict, guidance, existing_guidance, previously_selected, consistency_on,
                           topology, enabled, n_found, heading, sig_mask, sig_side, clearance, cost, stream=None):
    """mpcg_guidance_update (include/mpcg_guidance.h): this step's guidance trajectories, class ids and
    planner bookkeeping of S scenes x G planners from state (S, nx), stage_params (S, npar), obst
    (S, n_ell, N, 5), obst_meta (S, n_ell, 2) and the layer state `gstate` (dict class_traj
    (S, 2 (G - 1), N+1, 2), class_used (S, 2 (G - 1)) uint8, planner_class (S, G) int32, selected_topology
    (S,) int32, prev_was_original (S,) uint8; class_traj / class_used updated in place).  Outputs:
    guidance (S, G, N+1, 4), existing_guidance / previously_selected / consistency_on / enabled (S, G)
    uint8, topology (S, G) int32, n_found (S,) int32, heading (S, 2), sig_mask / sig_side (S, G) int32,
    clearance / cost (S, 8).  Asynchronous on `stream`; nothing is allocated."""
    N = pr.N
    _dev("state", state, F64, (S, pr.nx))
    _dev("stage_params", stage_params, F64, (S, pr.npar))
    _dev("obst", obst, F64, (S, pr.n_ell, N, 5))
    _dev("obst_meta", obst_meta, F64, (S, pr.n_ell, 2))
    _dev("guidance", guidance, F64, (S, G, N + 1, 4))
    _dev("heading", heading, F64, (S, 2))
    _dev("clearance", clearance, F64, (S, GUIDANCE_CANDIDATES))
    _dev("cost", cost, F64, (S, GUIDANCE_CANDIDATES))
    for k, t in dict(existing_guidance=existing_guidance, previously_selected=previously_selected,
                     consistency_on=consistency_on, enabled=enabled).items():
        _dev(k, t, U8, S * G)
    for k, t in dict(topology=topology, sig_mask=sig_mask, sig_side=sig_side).items():
        _dev(k, t, I32, S * G)
    _dev("n_found", n_found, I32, S)
    st = _guidance_state(gstate, S, G, N)
    out = MpcgGuidanceOut(*(t.data_ptr() for t in (guidance, existing_guidance, previously_selected, consistency_on,
                                                   topology, enabled, n_found, heading, sig_mask, sig_side,
                                                   clearance, cost)))
    rc = lib.mpcg_guidance_update(C.byref(pr), S, G, C.byref(settings), _ptr(state), _ptr(stage_params), _ptr(obst),
                                  _ptr(obst_meta), C.byref(st), C.byref(out), _stream(stream, state.device))
    _check(rc, "mpcg_guidance_update")


def guidance_mask_device(S: int, G: int, enabled, exit_code, stream=None):
    """mpcg_guidance_mask: exit_code (S*G,) int32 of the planners with enabled (S, G) 0 becomes
    MPCG_GUIDANCE_EXIT_DISABLED, in place."""
    _dev("enabled", enabled, U8, S * G)
    _dev("exit_code", exit_code, I32, S * G)
    _check(lib.mpcg_guidance_mask(S, G, _ptr(enabled), _ptr(exit_code), _stream(stream, exit_code.device)),
           "mpcg_guidance_mask")


def guidance_select_device(S: int, G: int, best, guided, topology, enabled, gstate: dict, stream=None):
    """mpcg_guidance_select: selected_topology, prev_was_original and planner_class of `gstate` from
    best (S,) int32, guided / enabled (S, G) uint8 and topology (S, G) int32."""
    _dev("best", best, I32, S)
    _dev("guided", guided, U8, S * G)
    _dev("enabled", enabled, U8, S * G)
    _dev("topology", topology, I32, S * G)
    N = gstate["class_traj"].shape[2] - 1
    st = _guidance_state(gstate, S, G, N)
    _check(lib.mpcg_guidance_select(S, G, _ptr(best), _ptr(guided), _ptr(topology), _ptr(enabled), C.byref(st),
                                    _stream(stream, best.device)), "mpcg_guidance_select")


def active_plan_device(enabled, slot_of=None, solve_of=None, n_active=None, stream=None):
    """mpcg_active_plan (include/mpcg_active.h): the stable compaction of enabled (B,) uint8 (any shape
    of B elements).  Returns slot_of (B,), solve_of (B,) and n_active (1,), int32 device tensors
    (allocated unless given); asynchronous on `stream`."""
    _dev("enabled", enabled, U8)
    B, dev = enabled.numel(), enabled.device
    slot_of = torch.empty((B,), dtype=I32, device=dev) if slot_of is None else slot_of
    solve_of = torch.empty((B,), dtype=I32, device=dev) if solve_of is None else solve_of
    n_active = torch.empty((1,), dtype=I32, device=dev) if n_active is None else n_active
    _dev("slot_of", slot_of, I32, B)
    _dev("solve_of", solve_of, I32, B)
    _dev("n_active", n_active, I32, 1)
    # (an empty tensor's data_ptr is 0: the plan of an empty batch still needs non-null pointers)
    p = lambda t: C.c_void_p(t.data_ptr() or n_active.data_ptr())  # noqa: E731
    _check(lib.mpcg_active_plan(B, p(enabled), p(slot_of), p(solve_of), _ptr(n_active), _stream(stream, dev)),
           "mpcg_active_plan")
    return slot_of, solve_of, n_active


# mpcg_io's fields in order, as the keys of solve_batch_device's arguments and result
_IO_KEYS = ("params", "warm", "xinit", "lam_in", "xtraj", "utraj", "pobj", "exit", "info", "lam", "qp_in", "qp",
            "stats")


def _active_io(pr: MpcgProblem, d: dict, rows: int) -> MpcgIo:
    """An mpcg_io over the tensors of `d` (keys of solve_batch_device's arguments and result: params, warm,
    xinit, lam_in, qp_in, xtraj, utraj, pobj, exit, info, lam, qp, stats; missing or None: NULL), each
    checked to hold at least `rows` blocks of the size include/mpcg.h documents."""
    N, nx, nu = pr.N, pr.nx, pr.nu
    LS = lam_stride(pr)
    Q = qp_mem_size(pr) if (d.get("qp_in") is not None or d.get("qp") is not None) else 0
    block = dict(params=N * pr.npar, warm=(N + 1) * (nu + nx), xinit=nx, lam_in=N * LS, xtraj=(N + 1) * nx,
                 utraj=N * nu, pobj=1, exit=1, info=INFO_STRIDE, lam=N * LS, qp_in=Q, qp=Q, stats=STATS_STRIDE)
    for k in _IO_KEYS:
        t = d.get(k)
        if t is not None:
            _dev(k, t, I32 if k in ("exit", "info") else F64)
            assert t.numel() >= rows * block[k] and (t.shape[0] == 0 or t.numel() == t.shape[0] * block[k]), \
                (k, tuple(t.shape), rows, block[k])
    return MpcgIo(*(_addr(d.get(k)) for k in _IO_KEYS))


def active_gather_device(pr: MpcgProblem, slot_of, full: dict, dense: dict, stream=None):
    """mpcg_active_gather: params, warm, xinit (and lam_in / qp_in where present in both) of every enabled
    solve b of `full` (B rows) into row slot_of[b] of `dense` (at least as many rows as are enabled; the
    caller's responsibility, B rows always suffice).  Dicts of device tensors, keys as in _active_io."""
    B = slot_of.numel()
    _dev("slot_of", slot_of, I32)
    assert full["params"].shape[0] == B
    fio, dio = _active_io(pr, full, B), _active_io(pr, dense, 0)
    _check(lib.mpcg_active_gather(C.byref(pr), B, _ptr(slot_of), C.byref(fio), C.byref(dio),
                                  _stream(stream, slot_of.device)), "mpcg_active_gather")


def active_scatter_device(pr: MpcgProblem, slot_of, dense: dict, full: dict, stream=None):
    """mpcg_active_scatter: every output present in `full` (xtraj, utraj, pobj, exit, info, lam, qp, stats; B
    rows) from row slot_of[b] of `dense`; a disabled solve gets the fill of include/mpcg_active.h, which
    reads full["warm"]."""
    B = slot_of.numel()
    _dev("slot_of", slot_of, I32)
    fio, dio = _active_io(pr, full, B), _active_io(pr, dense, 0)
    _check(lib.mpcg_active_scatter(C.byref(pr), B, _ptr(slot_of), C.byref(dio), C.byref(fio),
                                   _stream(stream, slot_of.device)), "mpcg_active_scatter")


class ActiveWorkspace:
    """mpcg_active_ws: the dense buffers, the plan and the pinned count of mpcg_solve_active for up to
    max_batch solves of `pr`, on the current device."""

    def __init__(self, pr: MpcgProblem, max_batch: int, with_lam: bool = False, with_qp: bool = False,
                 with_stats: bool = False):
        self.pr, self.max_batch = pr, int(max_batch)
        self.with_lam, self.with_qp, self.with_stats = bool(with_lam), bool(with_qp), bool(with_stats)
        self._c = lib.mpcg_active_ws_create(C.byref(pr), self.max_batch, int(self.with_lam), int(self.with_qp),
                                            int(self.with_stats))
        if not self._c:
            raise RuntimeError(f"mpcg_active_ws_create failed: {last_error()}")

    def close(self):
        if self._c:
            lib.mpcg_active_ws_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_active_device(pr: MpcgProblem, params, warm, xinit, enabled, ws=None, stream=None, lam_in=None,
                        lam_out=False, qp_in=None, qp_out=False, stats=False, out=None):
    """mpcg_solve_active (include/mpcg_active.h): solve_batch_device for the solves with enabled (B,) uint8
    non-zero only -- plan, gather, one mpcg_solve of the dense batch, scatter; every other solve holds the
    header's fill (exit ACTIVE_EXIT_SKIPPED).  ws: an ActiveWorkspace (None: one is created for this call).
    Returns solve_batch_device's dict plus n_active (int) and slot_of (B,) int32.  Synchronises `stream`
    once (the count is read on the host; not capturable into a graph) and returns with the solve and the
    scatter in flight on it."""
    B, dev = params.shape[0], params.device
    out = _solve_outputs(pr, B, dev, out, lam_out, qp_out, stats)
    if "slot_of" not in out:
        out["slot_of"] = torch.empty((B,), dtype=I32, device=dev)
    io = _solve_io(pr, params, warm, xinit, lam_in, qp_in, out, lam_out, qp_out, stats)
    _dev("enabled", enabled, U8, B)
    own = ws is None
    if own:
        ws = ActiveWorkspace(pr, max(B, 1), with_lam=lam_in is not None or lam_out,
                             with_qp=qp_in is not None or qp_out, with_stats=stats)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    n = C.c_int(-1)
    try:
        _check(lib.mpcg_solve_active(C.byref(pr), B, C.byref(io), _ptr(enabled), ws._c, C.byref(n),
                                     _stream(s, dev)), "mpcg_solve_active")
        _check(lib.mpcg_active_ws_read_plan(ws._c, B, _ptr(out["slot_of"]), None, _stream(s, dev)),
               "mpcg_active_ws_read_plan")
    finally:
        if own:
            # the workspace's buffers are read by work still in flight
            s.synchronize()
            ws.close()
    out["n_active"] = int(n.value)
    return out
