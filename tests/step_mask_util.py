"""Shared by tests/test_step_mask*.py: the shapes and masks of the GPU tests (tests/reset_envs_util.py's: {0, 3, 7} stepping and its complement), and the
episode log with step masks in numpy."""
import numpy as np

import episode_log_util
from reset_envs_util import COMPLEMENT, H, MASK, N, W, mask_of  # noqa: F401  (re-exported)

STEPPING = {"step_0_3_last": MASK, "step_complement": COMPLEMENT}


class MaskedModel(episode_log_util.Model):
    """episode_log_util's model plus mv_set_step_mask: a tick of a frozen env adds nothing to its running returns or its running length and writes no
    record; the tick counter is the gym's and runs on for everybody"""

    def feed(self, rewards, dones, tobj, step_mask=None):
        if step_mask is None:
            return super().feed(rewards, dones, tobj)
        steps = np.asarray(step_mask) != 0
        assert steps.shape == (self.N,)
        per_agent = np.repeat(steps, self.A)
        for r, d, o in zip(rewards, dones, tobj):
            ret, length = self.ret.copy(), self.len.copy()
            # (whatever the frozen envs' inputs hold -- the gym stages zeros for them, the synthetic tests hand over noise -- none of it may count)
            super().feed(r[None], (np.asarray(d) != 0)[None] & steps[None], o[None])
            self.ret[~per_agent] = ret[~per_agent]
            self.len[~steps] = length[~steps]
