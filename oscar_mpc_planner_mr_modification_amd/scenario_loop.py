"""Consecutive SH-MPC control steps of many scenes on one GPU: what ScenarioConstraints::optimize and
Planner::solveMPC do per step on the safe-horizon configuration, with every per-step quantity
device-resident and the obstacle samples drawn on the device (include/mpcg_scenario.h).

    step():     mpcg_scenario_sample_prepare (every copy's samples from the predictions and the bank,
                reduced to its scenario rows) -> mpcg_solve (all copies, carried multipliers)
                -> mpcg_select_lowest_cost_device -> mpcg_winner_records_device
    advance():  mpcg_scenario_advance (warm start and multipliers of the next step)

The scene data of the next step (ego state, obstacle predictions) comes from outside the planner, so
`set_scene_data` replaces it between steps; with `set_tracks` the predictions come from a device-resident table
of tracked objects instead (include/mpcg_tracks.h), filled in first by every step().  Every buffer is allocated in the constructor; step() and
advance() allocate nothing and synchronise nothing when they are given device tensors.  `draw`, the
step counter of the derived batch index, advances by one per step().
"""
from __future__ import annotations

from . import native
from .layouts import Layout


class ScenarioLoop:
    def __init__(self, layout: Layout, scenes, device, bank=None, robot_radius: float | None = None,
                 deceleration: float = 3.0, seed: int | None = None, draw: int = 0):
        """scenes: scenario_sampler.PredictionScenes (stage_params, state, obst, obst_meta, n_solvers, optional
        main_warm: the first step's warm start, else the braking plan); bank (n_batches, n_per, 2): the
        standard-normal pairs (default scenes.bank), uploaded once."""
        import numpy as np
        import torch

        from .synthetic import ROBOT_RADIUS

        if layout.n_scen < 1:
            raise ValueError("ScenarioLoop: the layout has no scenario rows")
        self.lay, self.dev = layout, device
        self.pr = pr = native.problem_from_layout(layout)
        self.S, self.P = scenes.stage_params.shape[0], scenes.n_solvers
        self.rr = ROBOT_RADIUS if robot_radius is None else robot_radius
        self.dec = deceleration
        self.seed = int(scenes.seed if seed is None else seed)
        self.draw = int(draw)
        S, P, N, nx, nu = self.S, self.P, layout.N, layout.nx, layout.nu
        B = S * P
        f64 = dict(dtype=torch.float64, device=device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)  # noqa: E731
        self.stage_params, self.state = t(scenes.stage_params), t(scenes.state)
        self.obst, self.obst_meta = t(scenes.obst), t(scenes.obst_meta)
        self.bank = t(scenes.bank if bank is None else bank)
        self.main_warm = torch.zeros((S, N + 1, nu + nx), **f64)
        self.has_warm = scenes.main_warm is not None
        if self.has_warm:
            self.main_warm.copy_(t(scenes.main_warm))
        self.lam = torch.zeros((B, N, native.lam_stride(pr)), **f64)
        self.prep = dict(params=torch.empty((B, N, pr.npar), **f64), warm=torch.empty((B, N + 1, nu + nx), **f64),
                         xinit=torch.empty((B, nx), **f64))
        self.out = native._solve_outputs(pr, B, device, None, True, False, False)
        self.best = torch.empty((S,), dtype=torch.int32, device=device)
        self.records = torch.empty((S, (N + 1) * nx + N * nu + 2), **f64)
        self.last = None
        # the table of tracked objects (set_tracks) or None: nothing is launched
        self.tracks = None

    def set_tracks(self, pose, twist, dims, shape, settings=None, propagate: bool = False):
        """The tracked objects of every scene (include/mpcg_tracks.h): pose (S, A, 3), twist (S, A, 2), dims
        (S, A, 2), shape (S, A) int32.  From now on every step() first fills the predictions obst / obst_meta --
        what mpcg_scenario_sample_prepare reads -- from them (mpcg_tracks_rows, mpcg_obstacle_select; `propagate`:
        the callback's second pass of propagatePredictionUncertainty).  settings: tracks.TrackSettings (None: the
        defaults with probabilistic on, SH-MPC's GAUSSIAN predictions).  Device tensors are taken as they are --
        self.tracks holds them -- so the caller may update them in place between steps."""
        from .tracks import TrackSettings

        # the SH-MPC layout has no ellipsoid rows: the selection's n_ell is the loop's predictions per scene
        self._track_pr = native.problem_with_rows(self.pr, self.obst.shape[1])
        table = native.track_table_device(pose, twist, dims, shape, self.dev)
        W, A = table["shape"].shape
        if W != self.S:
            raise ValueError(f"ScenarioLoop.set_tracks: {W} worlds for {self.S} scenes")
        self._track_set = (TrackSettings(probabilistic=True) if settings is None else settings).native()
        self._track_scratch = native.TrackObstacles(self._track_pr, self.S, A, self.dev)
        self.track_propagate = bool(propagate)
        self.tracks = table

    def set_scene_data(self, state, obst, obst_meta=None):
        """Replace the externally provided scene data: state (S, nx), obst (S, n_obs, N, 5) and optionally
        obst_meta (S, n_obs, 2), device tensors or arrays, copied into the loop's buffers."""
        import torch

        for dst, src in ((self.state, state), (self.obst, obst), (self.obst_meta, obst_meta)):
            if src is not None:
                dst.copy_(torch.as_tensor(src, dtype=torch.float64).reshape(dst.shape))

    def step(self, stream=None):
        """One control step of every scene.  Returns dict(best, exit, xtraj, utraj, pobj, lam, records, prepared,
        draw): the loop's own buffers, overwritten by the next step."""
        pr, S, P = self.pr, self.S, self.P
        draw = self.draw
        if self.tracks is not None:
            native.tracks_obstacles_device(self._track_pr, self._track_set, self.tracks, self.state, self.obst, self.obst_meta,
                                           propagate=self.track_propagate, scratch=self._track_scratch, stream=stream)
        native.scenario_sample_prepare_device(pr, P, self.stage_params, self.state, self.obst, self.obst_meta,
                                              self.bank, self.rr, self.dec,
                                              main_warm=self.main_warm if self.has_warm else None, seed=self.seed,
                                              draw=draw, out=self.prep, stream=stream)
        self.draw += 1
        out = native.solve_batch_device(pr, self.prep["params"], self.prep["warm"], self.prep["xinit"], out=self.out,
                                        stream=stream, lam_in=self.lam, lam_out=True)
        native.select_lowest_cost_device(S, P, out["pobj"], out["exit"], out=self.best, stream=stream)
        native.winner_records_device(out["xtraj"], out["utraj"], out["pobj"], self.best, P, self.records, stream=stream)
        self.last = dict(best=self.best, exit=out["exit"], xtraj=out["xtraj"], utraj=out["utraj"], pobj=out["pobj"],
                         lam=out["lam"], records=self.records, prepared=self.prep, draw=draw)
        return self.last

    def advance(self, state_next, stream=None):
        """Carry the planner state into the next step (call after step()): the next warm start and the carried
        multipliers, from state_next (S, nx)."""
        import torch

        L = self.last
        self.state.copy_(torch.as_tensor(state_next, dtype=torch.float64).reshape(self.state.shape))
        native.scenario_advance_device(self.pr, self.S, self.P, L["best"], L["exit"], L["xtraj"], L["utraj"], L["lam"],
                                       self.state, self.dec, self.main_warm, lam_next=self.lam, stream=stream)
        self.has_warm = True
        return dict(main_warm=self.main_warm, lam=self.lam)
