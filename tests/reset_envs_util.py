"""Shared by tests/test_reset_envs*.py: the shapes and masks of the GPU tests, and the episode log with masked resets in numpy."""
import numpy as np

import episode_log_util

N = 8
W, H = 32, 32
FLAGGED = [0, 3, N - 1]


def mask_of(envs, n=N):
    m = np.zeros(n, np.bool_)
    m[list(envs)] = True
    return m


MASK = mask_of(FLAGGED)
COMPLEMENT = ~MASK
MASKS = {"flagged_0_3_last": MASK, "complement": COMPLEMENT}


class CutModel(episode_log_util.Model):
    """episode_log_util's model plus mv_reset_envs: a flagged env's accumulators go to zero and it writes no record; records, counts and the tick
    counter stay"""

    def cut(self, mask):
        mask = np.asarray(mask).astype(bool)
        assert mask.shape == (self.N,)
        self.ret[np.repeat(mask, self.A)] = 0.0
        self.len[mask] = 0
