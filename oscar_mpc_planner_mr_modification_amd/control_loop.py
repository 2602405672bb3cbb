"""Consecutive control steps of many scenes on one GPU: the work
GuidanceConstraints::optimize and Planner::solveMPC do per step, with every
per-step quantity device-resident.

    step():  mpcg_prepare (per-guess inputs) [-> with a road mpcg_road_halfspaces: the two
             road rows into the prepared parameters, before skip_disabled's gather too]
             -> mpcg_solve (all guesses, carried
             multipliers; with skip_disabled mpcg_solve_active: the enabled guesses only)
             -> mpcg_select_best_device (FindBestPlanner with the
             consistency / selection-weight bookkeeping) -> mpcg_advance (warm
             start, previous plan, selection flags, multipliers of the next step)

The scene data of the next step (ego state, obstacle predictions, guidance
trajectories) comes from outside the planner (sensors, guidance_planner), so
`set_scene_data` replaces it between steps.  With `set_tracks` the obstacle predictions
come from a device-resident table of tracked objects instead (include/mpcg_tracks.h):
every step() first fills obst / obst_meta from it.
"""
from __future__ import annotations

from . import native
from .layouts import Layout


class ControlLoop:
    def __init__(self, layout: Layout, scenes, device, robot_radius: float, w_consistency: float,
                 selection_weight: float, deceleration: float = 3.0, shift_forward: bool = False,
                 consistency_on_non_guided: bool = True, elapsed: float | None = None,
                 warmstart_with_mpc_solution: bool = False, guidance_layer=None, skip_disabled: bool = False,
                 road=None):
        import torch

        if skip_disabled and guidance_layer is None:
            raise ValueError("ControlLoop: skip_disabled needs a guidance_layer (the layer is what disables planners)")
        self.lay = layout
        self.pr = native.problem_from_layout(layout)
        self.dev = device
        self.S, self.G = scenes.n_scenes, scenes.n_guesses
        self.rr, self.wc, self.sw, self.dec = robot_radius, w_consistency, selection_weight, deceleration
        self.shift, self.cong = shift_forward, consistency_on_non_guided
        # t-mpc.warmstart_with_mpc_solution (guidance_constraints.cpp:335-338): from the second step on,
        # guided planners (whose guidance then exists) start from their own previous output
        self.own_warm = warmstart_with_mpc_solution
        self.elapsed = layout.dt if elapsed is None else elapsed
        self.dsc = native.scenes_to_device(scenes, device)
        LS = 5 + layout.nh
        self.lam = torch.zeros((self.S * self.G, layout.N, LS), dtype=torch.float64, device=device)
        self.last = None
        self.existing = None
        # guidance.GuidanceLayer or None: with a layer, guidance, existing_guidance and the class-keyed
        # selection flags of every step come from mpcg_guidance_update instead of from outside
        self.guidance_layer = guidance_layer
        # skip_disabled: the planners the layer disables are not solved (mpcg_solve_active)
        # instead of solved and masked afterwards; their outputs then hold the fill of include/mpcg_active.h.
        # One host synchronisation per step (the count of enabled planners); step() adds n_active.
        self.skip_disabled = bool(skip_disabled)
        self.active_ws = native.ActiveWorkspace(self.pr, self.S * self.G, with_lam=True) if self.skip_disabled else None
        # roads.RoadSettings or None: with a road, every step writes the two road-boundary halfspaces
        # (include/mpcg_road.h) into the prepared parameters; the path they follow comes from
        # set_road_path (a PathLoop passes its own).  None: nothing is launched
        self.road = road
        self.road_table = self.road_bounds = self.road_halfspaces = None
        if road is not None:
            if layout.n_lin < layout.max_obstacles + 2:
                raise ValueError(f"ControlLoop: a road needs n_lin >= max_obstacles + 2, the layout has n_lin "
                                 f"{layout.n_lin} for {layout.max_obstacles} obstacles (tmpc_layout(add_halfspaces=2))")
            self._road = road.native()
            self.road_halfspaces = torch.zeros((self.S, layout.N, 2, 3), dtype=torch.float64, device=device)
        # the table of tracked objects (set_tracks) or None: nothing is launched
        self.tracks = None

    def set_tracks(self, pose, twist, dims, shape, settings=None, propagate: bool = False):
        """The tracked objects of every scene (include/mpcg_tracks.h): pose (S, A, 3), twist (S, A, 2), dims
        (S, A, 2), shape (S, A) int32.  From now on every step() first fills obst / obst_meta from them
        (mpcg_tracks_rows, mpcg_obstacle_select; `propagate`: the callback's second pass of
        propagatePredictionUncertainty).  settings: tracks.TrackSettings (None: the defaults).  Device tensors
        are taken as they are -- self.tracks holds them -- so the caller may update them in place between steps."""
        from .tracks import TrackSettings

        if self.lay.n_ell < 1:
            raise ValueError("ControlLoop.set_tracks: the layout has no obstacle rows (n_ell 0)")
        table = native.track_table_device(pose, twist, dims, shape, self.dev)
        W, A = table["shape"].shape
        if W != self.S:
            raise ValueError(f"ControlLoop.set_tracks: {W} worlds for {self.S} scenes")
        self._track_set = (TrackSettings() if settings is None else settings).native()
        self._track_scratch = native.TrackObstacles(self.pr, self.S, A, self.dev)
        self.track_propagate = bool(propagate)
        self.tracks = table

    def set_road_path(self, dtable: dict, bounds: dict | None = None):
        """The path the road follows (native.path_table_device) and, for the bounds mode, the left and
        right bound tables (native.road_bounds_device)."""
        if self.road is None:
            raise ValueError("ControlLoop.set_road_path: the loop has no road")
        if self.road.mode == "bounds" and bounds is None:
            raise ValueError("ControlLoop.set_road_path: the bounds mode needs the bound tables")
        self.road_table, self.road_bounds = dtable, bounds if self.road.mode == "bounds" else None

    def set_scene_data(self, state, obst, guidance, existing_guidance=None):
        """Replace the externally provided scene data (device tensors or arrays).

        existing_guidance (S, G) bool, optional: which guided planners' guidance existed in the
        previous step -- in the reference a planner keeps its guidance only when the homotopy
        class guidance_planner finds this step maps back to the same planner
        (guidance_constraints.cpp:211-257), so it comes from the guidance search, outside the
        planner.  Read by the next step() with warmstart_with_mpc_solution (such a planner
        starts from its own previous output, the others from their guidance); when not given,
        every guided planner's guidance is taken to have existed (each kept its class)."""
        import torch

        t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=self.dev).contiguous()  # noqa: E731
        self.dsc["state"], self.dsc["obst"], self.dsc["guidance"] = t(state), t(obst), t(guidance)
        self.existing = None
        if existing_guidance is not None:
            ex = torch.as_tensor(existing_guidance, device=self.dev).reshape(self.S, self.G)
            self.existing = ex.to(torch.uint8).contiguous()

    def step(self, stream=None):
        """One control step of every scene.  Returns dict(best, exit, xtraj, utraj, pobj, objective, prepared)
        (plus n_active, the number of planners solved, with skip_disabled, and road_halfspaces (S, N, 2, 3) with
        a road)."""
        pr, S, G, N = self.pr, self.S, self.G, self.lay.N
        gl = self.guidance_layer
        if self.tracks is not None:
            native.tracks_obstacles_device(pr, self._track_set, self.tracks, self.dsc["state"], self.dsc["obst"],
                                           self.dsc["obst_meta"], propagate=self.track_propagate,
                                           scratch=self._track_scratch, stream=stream)
        if gl is not None:
            gl.update(self, stream=stream)
        if self.own_warm and self.last is not None:
            self.dsc["planner_xtraj"], self.dsc["planner_utraj"] = self.last["xtraj"], self.last["utraj"]
            self.dsc["existing_guidance"] = self.dsc["guided"] if self.existing is None else self.existing
            if gl is not None:
                self.dsc["existing_guidance"] = gl.existing_guidance
        prep = native.prepare_device(pr, self.dsc, self.rr, self.wc, self.dec, stream=stream,
                                     warmstart_with_mpc_solution=self.own_warm, shift_forward=self.shift)
        if self.road is not None:
            if self.road_table is None:
                raise RuntimeError("ControlLoop.step: the loop has a road but no path (set_road_path)")
            native.road_halfspaces_device(pr, G, self.lay.max_obstacles, self._road, self.road_table, prep["params"],
                                          state=self.dsc["state"], main_warm=self.dsc.get("main_warm"),
                                          guided=self.dsc["guided"], deceleration=self.dec, bounds=self.road_bounds,
                                          halfspaces=self.road_halfspaces, stream=stream)
        if self.skip_disabled:
            out = native.solve_active_device(pr, prep["params"], prep["warm"], prep["xinit"], gl.enabled.reshape(-1),
                                             ws=self.active_ws, stream=stream, lam_in=self.lam, lam_out=True)
        else:
            out = native.solve_batch_device(pr, prep["params"], prep["warm"], prep["xinit"], stream=stream,
                                            lam_in=self.lam, lam_out=True)
            if gl is not None:
                gl.mask(out["exit"], stream=stream)
        best, objective = native.select_best_device(S, G, N, out["xtraj"], out["pobj"], out["exit"],
                                                    prev_traj=prep["prev_interp"], w_cons=self.wc,
                                                    consistency_enabled=prep["consistency_active"],
                                                    previously_selected=self.dsc["previously_selected"],
                                                    selection_weight=self.sw, stream=stream)
        self.last = dict(best=best, exit=out["exit"], xtraj=out["xtraj"], utraj=out["utraj"], pobj=out["pobj"],
                         objective=objective, prepared=prep, lam=out["lam"])
        if self.skip_disabled:
            self.last["n_active"] = out["n_active"]
        if self.road is not None:
            self.last["road_halfspaces"] = self.road_halfspaces
        if gl is not None:
            gl.after_select(self, self.last, stream=stream)
        return self.last

    def advance(self, state_next, stream=None):
        """Carry the planner state into the next step (call after step())."""
        import torch

        L = self.last
        sn = torch.as_tensor(state_next, dtype=torch.float64, device=self.dev).contiguous()
        c = native.advance_device(self.pr, self.S, self.G, L["best"], L["exit"], L["xtraj"], L["utraj"],
                                  L["prepared"]["warm"], L["lam"], sn, self.dsc["guided"], self.elapsed,
                                  self.dec, self.shift, self.cong,
                                  previously_selected=self.dsc["previously_selected"], stream=stream)
        self.dsc["main_warm"] = c["main_warm"]
        self.dsc["prev_traj"] = c["prev_traj"]
        self.dsc["prev_elapsed"] = c["prev_elapsed"]
        self.dsc["consistency_on"] = c["consistency_on"]
        self.dsc["previously_selected"] = c["previously_selected"]
        self.lam = c["lam"]
        self.dsc["state"] = sn
        return c
