"""The solve batches of tests/test_gpu_decomp.py have not degenerated: on the oracle alone, with the
host-produced decomp rows of decomp.make_c3_decomp_scenes (decomp_cases.solve_inputs), at the test shape
N 10 / 4 rows and at C3's N 30 / 12 rows, at least 80 % of the solves succeed and at least one successful solve
has a non-dummy decomp row binding: its gap b - a . p at most 1e-4 on some stage, or that stage's slack above
1e-6.  No GPU.

Figures of the default oracle build on the seeds of decomp_cases.SOLVE (successful / solves; solves with a
row within 1e-4; solves with slack above 1e-6; the largest slack; the distance of the two oracle builds):

    N 10, 4 rows,  seed 6100    8/8   gap 2   slack 8   8.7e-05  2.7e-15
    N 30, 12 rows, seed 6300   16/16  gap 11  slack 16  5.8e-04  1.2e-14
"""
import numpy as np
import pytest

import decomp_cases as dc


@pytest.mark.parametrize("N", [10, 30])
def test_decomp_rows_bind_in_successful_solves(oracle_mod, N):
    lay, sc, h, params = dc.solve_inputs(N)
    assert lay.n_scen == dc.SHAPES[N]
    r, lit = dc.oracle_run(N), dc.oracle_run(N, literal=True)
    ok = r["status"] == 1
    rows = h["rows"][:, 1:]
    real = ~((rows[..., 0] == 1.0) & (rows[..., 1] == 0.0) & (rows[..., 2] == (sc.xinit[:, 0] + 100.0)[:, None, None]))
    gap = ((dc.decomp_gaps(N, r["xtraj"]) <= dc.ACTIVE_GAP) & real).any((1, 2)) & ok
    slack = (r["utraj"][:, 1:lay.N, 2] > dc.ACTIVE_SLACK).any(1) & ok
    sp = max(np.abs(r["xtraj"][ok] - lit["xtraj"][ok]).max(), np.abs(r["utraj"][ok] - lit["utraj"][ok]).max())
    print(f"N {N}, {lay.n_scen} rows, seed {dc.SOLVE[N][1]}: {ok.sum()}/{len(ok)} successful, gap {gap.sum()}, "
          f"slack {slack.sum()}, largest slack {r['utraj'][:, :, 2].max():.1e}, builds {sp:.1e}")
    assert real.any()
    assert ok.mean() >= 0.8
    assert dc.binding_solves(N, r, ok).sum() >= 1 and gap.sum() >= 1
    assert np.array_equal(r["status"], lit["status"])
    # the rows in the solver's parameters are the host producer's
    i0 = lay.idx("disc_0_decomp_0_a1")
    assert np.array_equal(params[:, :, i0:i0 + 3 * lay.n_scen].reshape(h["rows"].shape), h["rows"])
