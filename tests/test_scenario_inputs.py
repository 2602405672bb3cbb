"""The solve batches of tests/test_gpu_scenario_sampler.py have not degenerated: on the oracle alone, with the
host-sampled scenario rows of scenario_sampler.make_shmpc_prediction_scenes (scenario_sampler_cases.solve_inputs),
at the small shape of mpcg_inst_shmpc.hip (N 10, 4 rows; 3 obstacles x 7 samples) and at C5 (N 20, 24 rows;
12 x 100), 8 scenes x 4 copies each: at least 75 % of the solves succeed, at least one successful solve (C5: at
least a quarter of the solves) has a scenario row within 1e-4 of binding, the two oracle builds agree on every
exit code, and on every (solve, stage) consecutive distances among the n_scen + 1 closest samples differ by more
than 1e-9, so that an ulp of cos / sin cannot change a pick and the 1e-12 comparisons of the GPU tests are
meaningful.  No GPU.

Figures of the default oracle build (successful / solves; successful solves with a row within 1e-4; the smallest
distance margin):

    small, seeds 77 .. 84     32/32   4   1.3e-04
    C5,    seeds 123 .. 130   25/32  21   9.5e-08
"""
import numpy as np
import pytest

import scenario_sampler_cases as cases


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_scenario_rows_bind_in_successful_solves(oracle_mod, name):
    c = cases.solve_inputs(name)
    s = cases.SHAPES[name]
    B = s["scenes"] * s["copies"]
    assert c.host.params.shape == (B, c.lay.N, c.lay.npar) and c.samples.shape[2] == s["n_obs"] * s["n_per"]
    r, lit = cases.oracle_run(name), cases.oracle_run(name, literal=True)
    ok = r["status"] == 1
    bind = cases.binding_solves(name, r["xtraj"], ok)
    margin = cases.smallest_margin(name)
    print(f"{name}, seeds {s['seed']} .. {s['seed'] + s['scenes'] - 1}: {ok.sum()}/{B} successful, {bind.sum()} with a "
          f"row within {cases.BINDING_GAP:g}, smallest distance margin {margin:.1e}")
    assert ok.mean() >= 0.75
    assert bind.sum() >= (B / 4 if name == "C5" else 1)
    assert np.array_equal(r["status"], lit["status"])
    assert margin > cases.MARGIN
    # the rows in the solver's parameters are non-trivial on every stage past 0, inactive on stage 0
    rows = cases.scenario_rows(name)
    assert np.all(rows[:, 0] == (0.0, 0.0, 100.0))
    assert np.allclose(np.hypot(rows[:, 1:, :, 0], rows[:, 1:, :, 1]), 1.0, rtol=0, atol=1e-12)
