"""scripts/tail_model.py simulate(): the event simulation of the level-ticket schedule on hand-made
instances whose makespans are worked out by hand (the comments), K = 0 and K = all."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from tail_model import simulate  # noqa: E402


def test_whole_solves_and_every_solve_by_levels():
    levels = [[3, 3], [1, 1], [1, 1], [5, 5]]
    # K = 0 on two waves: wave 0 runs solve 0 (until 6); wave 1 runs solves 1, 2 (until 4) and 3 (until 14)
    end, busy, n = simulate(levels, 2, 0)
    assert (end, n) == (14, 0) and busy == pytest.approx(20 / 28)
    # K = 4, tickets level-major.  Wave 0: (s0, l0) until 3, (s0, l1) until 6, (s1, l1) until 7, (s2, l1) until 8.
    # Wave 1: (s1, l0) until 1, (s2, l0) until 2, (s3, l0) until 7, (s3, l1) until 12.  Every second level starts
    # from a carry block
    end, busy, n = simulate(levels, 2, 4)
    assert (end, n) == (12, 4) and busy == pytest.approx(20 / 24)
    # K larger than the batch is the batch; one wave per solve and more: nothing to gain
    assert simulate(levels, 2, 99)[0] == 12
    assert simulate(levels, 8, 0)[0] == simulate(levels, 8, 4)[0] == 10


def test_a_finisher_second_at_the_word_goes_on_in_place():
    levels = [[5, 1], [1, 1]]
    # wave 1 finishes (s1, l0) at 1, draws (s0, l1) while solve 0's first level still runs -- it falls through --
    # and runs (s1, l1) until 2; wave 0 finishes (s0, l0) at 5 and runs (s0, l1) itself until 6
    assert simulate(levels, 2, 2) == (6, pytest.approx(8 / 12), 1)
    # with 2 cycles to load a block and 1 to save one: wave 0 saves until 6 and ends at 7 without a load; wave 1
    # saves until 2, loads until 4 and ends at 5
    assert simulate(levels, 2, 2, load=2, save=1)[::2] == (7, 1)


def test_tickets_of_an_ended_solve_fall_through():
    levels = [[2], [2, 2]]   # solve 0 ends at its first level
    # one wave: (s0, l0) until 2, (s1, l0) until 4, (s0, l1) falls through, (s1, l1) until 6
    assert simulate(levels, 1, 2)[::2] == (6, 1)
    assert simulate(levels, 1, 0)[0] == 6
    assert simulate([], 4, 0)[0] == 0
