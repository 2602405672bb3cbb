"""scripts/tail_model.py with grouped level tickets (simulate(..., group=G), grouped()): hand-made instances whose
makespans are worked out by hand (the comments)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from tail_model import grouped, simulate  # noqa: E402


def test_the_groups_are_level_0_then_g_levels_the_last_one_short():
    c = [[5, 1, 2, 3, 4, 6], [7], [7, 1], [7, 1, 2]]
    assert grouped(c, 1) == c
    assert grouped(c, 2) == [[5, 3, 7, 6], [7], [7, 1], [7, 3]]
    assert grouped(c, 3) == [[5, 6, 10], [7], [7, 1], [7, 3]]
    # a solve that ends in the middle of a group costs the levels it ran


def test_group_1_is_the_schedule_without_groups():
    levels = [[3, 3, 1], [1, 1, 4], [1, 1], [5, 5, 2]]
    for K in (0, 2, 4):
        assert simulate(levels, 2, K, load=2, save=1, group=1) == simulate(levels, 2, K, load=2, save=1)


def test_two_levels_per_ticket_halve_the_hand_overs():
    levels = [[2, 1, 1, 1, 1]] * 2
    # one wave, K = 2, one level per ticket: every level after the first starts from a carry block, 8 hand-overs;
    # 2 x 6 cycles of work + 8 loads of 1 + 8 saves of 1 = 28
    assert simulate(levels, 1, 2, load=1, save=1)[::2] == (28, 8)
    # two levels per ticket: groups {0}, {1, 2}, {3, 4}: 4 hand-overs, 12 + 4 + 4 = 20
    assert simulate(levels, 1, 2, load=1, save=1, group=2)[::2] == (20, 4)
    # four: groups {0}, {1 .. 4}: 2 hand-overs, 12 + 2 + 2 = 16
    assert simulate(levels, 1, 2, load=1, save=1, group=4)[::2] == (16, 2)
    # the busy fraction counts the levels' cycles, whatever the grouping
    assert simulate(levels, 1, 2, load=1, save=1, group=2)[1] == pytest.approx(12 / 20)


def test_a_coarser_ticket_ends_later_on_an_uneven_tail():
    levels = [[1, 4, 4], [1, 1, 1]]
    # two waves, one level per ticket: wave 0 runs (s0, l0) until 1, wave 1 (s1, l0) until 1; then (s0, l1) on one
    # until 5 and (s1, l1), (s1, l2) on the other until 3, which takes (s0, l2)'s ticket while level 1 still runs:
    # it falls through, and solve 0's wave goes on in place until 9
    assert simulate(levels, 2, 2)[0] == 9
    # two levels per ticket: the same 9 -- solve 0's chain is the makespan either way
    assert simulate(levels, 2, 2, group=2)[0] == 9
    # three solves of 1 + 2 + 2 on two waves.  One level per ticket: level 0 of s0, s1 until 1 and of s2 on wave 0
    # until 2; wave 1 runs (s0, l1) until 3, wave 0 (s1, l1) until 4, wave 1 (s2, l1) until 5, wave 0 (s0, l2) until 6,
    # wave 1 (s1, l2) until 7, wave 0 (s2, l2) until 8
    levels = [[1, 2, 2]] * 3
    assert simulate(levels, 2, 3)[0] == 8
    # two levels per ticket: wave 1 runs s0's pair until 5, wave 0 s1's from 2 until 6, wave 1 s2's until 9: the
    # last ticket is twice as long, and so is what the other wave stands idle for
    assert simulate(levels, 2, 3, group=2)[0] == 9
