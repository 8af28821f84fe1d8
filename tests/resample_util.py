"""Shared by tests/test_resample*.py: the two resampling maps the tests use and numpy models of the rule (megaverse_amd/csrc/mv_fork.h: resample_resolve)."""
import numpy as np

from fork_util import N, columns

# a swap 0 <-> 1, a 3-cycle 2 <- 3 <- 4 <- 2, a chain 5 <- 7 <- 6, a pure source 6
PERM = [1, 0, 3, 4, 2, 7, -1, 6]
PERM_COLS = [1, 0, 3, 4, 2, 7, 6, 6]
PERM_STAGED = {0, 1, 2, 3, 4, 7}
# a multinomial draw: env 3 serves three envs and is overwritten by env 0, env 0 serves three envs and is overwritten by env 3; two entries name themselves
DRAW = [3, 3, 3, 0, 4, 0, 6, 0]
DRAW_COLS = [3, 3, 3, 0, 4, 0, 6, 0]
DRAW_STAGED = {0, 3}
assert len(PERM) == len(DRAW) == N and columns(PERM) == PERM_COLS and columns(DRAW) == DRAW_COLS


def model(m):
    """-> (resolved, staged, invalid) as lists: entry d is left alone where m[d] is -1 or d, invalid where it is out of range and valid otherwise; env d is
    staged where its entry is valid and another valid entry names it"""
    n = len(m)
    valid = [m[d] != -1 and m[d] != d and 0 <= m[d] < n for d in range(n)]
    invalid = [int(m[d] != -1 and m[d] != d and not 0 <= m[d] < n) for d in range(n)]
    resolved = [int(m[d]) if valid[d] else -1 for d in range(n)]
    staged = [int(valid[d] and any(valid[i] and m[i] == d for i in range(n) if i != d)) for d in range(n)]
    return resolved, staged, invalid


def compose(first, second):
    """the columns after resampling with `first` and then with `second`: env e holds what env first_cols[second_cols[e]] held at the start"""
    a, b = columns(first), columns(second)
    return [a[b[e]] for e in range(len(a))]
