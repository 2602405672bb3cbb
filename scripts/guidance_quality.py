#!/usr/bin/env python3
"""What the guidance generator's guesses are worth to the solver, on the CPU oracle: one control step
of default synthetic scenes solved once from synthetic.make_scenes' own guesses and once from the
guesses of guidance.guidance_update_host (the restatement of mpcg_guidance_update; disabled planners
masked).  Recorded in DESIGN 6.5, asserted nowhere.

    python scripts/guidance_quality.py [--config C2] [--scenes 64] [--guesses 8]

Prints one JSON line; needs no GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--guesses", type=int, default=8)
    args = ap.parse_args()
    import oracle_py
    from oscar_mpc_planner_mr_modification_amd import guidance
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.producers import prepare_host
    from oscar_mpc_planner_mr_modification_amd.selection import find_best_planner_host
    from oscar_mpc_planner_mr_modification_amd.synthetic import (DECELERATION, ROBOT_RADIUS, SETTINGS_WEIGHTS,
                                                                 make_scenes)

    oracle_py.build()
    lay = config_layout(args.config)
    S, G, N = args.scenes, args.guesses, lay.N
    w_cons = SETTINGS_WEIGHTS["consistency"]
    orc = oracle_py.Oracle(lay)

    def solve(sc, enabled=None):
        p = prepare_host(lay, sc, ROBOT_RADIUS, w_cons, DECELERATION)
        r = orc.solve_batch(p.params, p.warm, p.xinit)
        status = r["status"] if enabled is None else guidance.mask_host(r["status"], enabled)
        best, _ = find_best_planner_host(S, G, N, r["xtraj"], r["pobj"], status)
        ok = (status == 1).reshape(S, G)
        ran = np.ones((S, G), bool) if enabled is None else enabled > 0
        return dict(scene_success=float((np.asarray(best) >= 0).mean()),
                    guided_planner_success=float(ok[:, :G - 1][ran[:, :G - 1]].mean()) if ran[:, :G - 1].any() else None,
                    guided_planners_solved_per_scene=float(ran[:, :G - 1].sum(1).mean()),
                    guided_successes_per_scene=float((ok & ran)[:, :G - 1].sum(1).mean()))

    sc = make_scenes(lay, S, G)
    sc.consistency_on[:] = False
    sc.previously_selected[:] = False
    own = solve(sc)
    st = guidance.GuidanceSettings(robot_radius=ROBOT_RADIUS, v_ref=SETTINGS_WEIGHTS["reference_velocity"])
    u = guidance.guidance_update_host(lay, sc.state, sc.stage_params, sc.obst, sc.obst_meta,
                                      guidance.initial_state(S, G, N), sc.guidance, G, st)
    sc.guidance = u["guidance"]
    gen = solve(sc, u["enabled"])
    out = {"what": "guidance_quality", "config": args.config, "scenes": S, "guesses": G,
           "make_scenes_guesses": own, "generator_guesses": gen, "mean_classes_found": float(u["n_found"].mean()),
           "classes_found_histogram": np.bincount(u["n_found"], minlength=G).tolist()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
