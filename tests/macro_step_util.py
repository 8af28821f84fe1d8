"""Shared by tests/test_macro_step*.py: the rule and the fold of macro steps (include/megaverse_hip.h: mv_macro_step) restated in numpy, the episode log
with macro steps, and the wrapper loop a macro step replaces -- independent of the library under test."""
import numpy as np

import episode_budget_util as B
import step_mask_util  # noqa: F401  (the masks and shapes of the GPU tests)
from episode_budget_util import H, N, W  # noqa: F401  (re-exported)


def rule(dones, mask, left, ticks, k=None):
    """one macro step.  dones [k][N]: what tick t stages for env e IF it steps; mask [N] or None; left [N] or None (no budget); ticks [N] or None (every
    env: k) -> (steps bool [k][N], left behind the last tick, ticks left behind the last tick).
    An env steps when mask and budget let it (episode_budget_util.rule) and it has ticks left; a stepped tick takes one tick off, all of them if it
    staged done, and spends the budget as always."""
    dones = np.asarray(dones) != 0
    k, n = dones.shape
    left = np.full(n, -1, np.int64) if left is None else np.array(left, np.int64).copy()
    tl = np.full(n, k, np.int64) if ticks is None else np.clip(np.array(ticks, np.int64), 0, k)
    on = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    steps = np.zeros((k, n), bool)
    for t in range(k):
        steps[t] = on & (left != 0) & (tl > 0)
        left -= (steps[t] & dones[t] & (left > 0)).astype(np.int64)
        tl = np.where(steps[t], np.where(dones[t], 0, tl - 1), tl)
    return steps, left.astype(np.int32), tl.astype(np.int32)


def fold(values):
    """values [k][n] float32 -> [n]: s = v_0; s = s + v_t, one float32 addition per tick, in tick order"""
    v = np.asarray(values, np.float32)
    s = v[0].copy()
    for t in range(1, v.shape[0]):
        s = (s + v[t]).astype(np.float32)
    return s


class MacroModel(B.BudgetModel):
    """episode_budget_util's model plus mv_macro_step: feed_macro takes the k ticks of one call as the gym staged them (or as an env that steps would have)
    and counts only the ticks the rule lets each env step in -- a tick the env did not step in adds nothing to returns or length and writes no record; the
    tick counter is the gym's and runs on by k"""

    def feed_macro(self, rewards, dones, tobj, ticks=None, step_mask=None):
        rewards, dones, tobj = np.asarray(rewards, np.float32), np.asarray(dones), np.asarray(tobj, np.float32)
        steps, left, _ = rule(dones, step_mask, self.left, ticks)
        for t in range(dones.shape[0]):
            step_mask_util.MaskedModel.feed(self, rewards[t][None], dones[t][None], tobj[t][None], steps[t].astype(np.uint8))
        if self.left is not None:
            self.left = left
        return steps
