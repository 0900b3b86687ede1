"""A numpy model of k_meet3's static schedule (Meet3Schedule, csrc/pgq_meet.hip): the first max(0, n - T) rows, rounded down
to a multiple of R, go R consecutive rows to a group, every row behind them is a group of its own; a grid of G workgroups
takes the groups at the stride G.  Over a sweep of (n, R, T, G) every row in 0 .. n-1 is taken exactly once, groups never
straddle the head's end, and R = 1 is one row per group in row order."""
import numpy as np
import pytest


def schedule(n, R, T):
    """(first row, number of rows) per group, in group order: the struct's first() and rows()."""
    shift = {1: 0, 2: 1, 4: 2, 8: 3}[R]
    head = max(0, n - T)
    head_groups = head >> shift
    groups = head_groups + (n - (head_groups << shift))
    g = np.arange(groups, dtype=np.int64)
    first = np.where(g < head_groups, g << shift, (head_groups << shift) + (g - head_groups))
    rows = np.where(g < head_groups, 1 << shift, 1)
    return first, rows, head_groups


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_every_row_is_taken_exactly_once(R):
    for T in (0, 1, 3, 7, 8, 64, 1000, 14336):
        for n in sorted({1, 2, R - 1, R, R + 1, T, T + 1, T + R - 1, T + R, T + R + 1, 257, 4099, 70001} - {0, -1}):
            first, rows, head_groups = schedule(n, R, T)
            taken = np.zeros(n, dtype=np.int64)
            for f, c in zip(first[:head_groups], rows[:head_groups]):
                taken[f:f + c] += 1
            np.add.at(taken, first[head_groups:], 1)
            assert (taken == 1).all(), (n, R, T)
            assert (np.diff(first) == rows[:-1]).all(), "groups follow each other in row order"
            assert n - head_groups * R >= min(n, T) and n - head_groups * R < min(n, T) + R, "the tail is T rows and what rounding leaves"
            for G in (1, 7, 8192):  # a capped grid: workgroup b takes groups b, b + G, ...
                seen = np.concatenate([np.arange(b, len(first), G) for b in range(min(G, len(first)))])
                assert len(seen) == len(first) and len(np.unique(seen)) == len(first)
            if R == 1:
                assert (first == np.arange(n)).all() and (rows == 1).all()
