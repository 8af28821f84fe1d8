"""Shared by tests/test_episode_log.py and tests/test_episode_log_gpu.py: the CPU oracle's outputs for the episode-log rollouts, and the log those outputs
imply -- the bookkeeping of include/megaverse_hip.h (mv_set_episode_log) done in numpy float64, independent of the library under test."""
import functools
import os

import numpy as np

import oracle_lib
from megaverse_amd.rollout import action_masks, sample_actions

ENV_SEED, POLICY_SEED = 42, 7
W, H = 64, 36     # (the log does not depend on the frame size)

RECORD = np.dtype([("agent", "<i4"), ("length", "<i4"), ("end_tick", "<u4"), ("true_objective", "<f4"), ("ret", "<f8")])

# name -> (scenario, envs, agents per env, params, ticks, floor on records, floor on records with ret != 0, floor on "finished twice within 16 ticks")
ROLLOUTS = {
    "collect_long": ("Collect", 128, 2, {"episodeLengthSec": 4.5}, 480, 150, 100, 0),
    "collect_short": ("Collect", 32, 2, {"episodeLengthSec": -60.0}, 400, 800, 30, 40),
    "sokoban": ("Sokoban", 64, 1, {"episodeLengthSec": 4.5}, 480, 400, 0, 0),
    "tower_short": ("TowerBuilding", 32, 4, {"episodeLengthSec": -200.0}, 400, 1500, 30, 0),
    "boxagone": ("BoxAGone", 16, 1, {}, 320, 30, 30, 0),
}


# More than 1024 agents: the kernel's threads take several agents each (chunks of 1024), with agents per env that do not divide a wave (3) and that do (4);
# 4160 agents x 16 ticks: more cells than threads in the kernel's scan.  GPU tests only (same fields; floors: about four fifths of what the oracle alone gives,
# checked on the CPU: 15387 / 13976 / 34720 records, 117 / 107 / 31 of them with ret != 0).
LARGE_ROLLOUTS = {
    "tower_512x3": ("TowerBuilding", 512, 3, {"episodeLengthSec": -200.0}, 160, 12000, 80, 0),
    "tower_320x4": ("TowerBuilding", 320, 4, {"episodeLengthSec": -200.0}, 160, 11000, 80, 0),
    "tower_1040x4": ("TowerBuilding", 1040, 4, {"episodeLengthSec": -200.0}, 64, 28000, 20, 0),
}
ALL_ROLLOUTS = {**ROLLOUTS, **LARGE_ROLLOUTS}


def boxoban_env():
    os.environ.setdefault("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))


@functools.lru_cache(maxsize=None)
def oracle_outputs(scenario, N, A, params_items, ticks, env_seed=ENV_SEED, policy_seed=POLICY_SEED):
    """the oracle stepped `ticks` times without rendering, tick index as step index -> rewards [ticks][N*A] f32, dones [ticks][N] u8,
    true objectives [ticks][N*A] f32 (read where done, 0 elsewhere)"""
    boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, dict(params_items))
    og.seed(env_seed)
    og.reset()
    rewards = np.zeros((ticks, N * A), np.float32)
    dones = np.zeros((ticks, N), np.uint8)
    tobj = np.zeros((ticks, N * A), np.float32)
    for t in range(ticks):
        og.set_action_masks(action_masks(sample_actions(policy_seed, t, N * A)))
        og.step_norender()
        rewards[t] = og.get_last_rewards()
        dones[t] = og.get_dones()
        for e in np.flatnonzero(dones[t]).tolist():
            for a in range(A):
                tobj[t, e * A + a] = og.true_objective(e, a)
    og.close()
    return rewards, dones, tobj


def rollout(name):
    scenario, N, A, params, ticks, *_ = ALL_ROLLOUTS[name]
    return oracle_outputs(scenario, N, A, tuple(sorted(params.items())), ticks)


class Model:
    """the episode log in numpy: feed(rewards [k][N*A], dones [k][N], true objectives [k][N*A]) in tick order"""

    def __init__(self, N, A, capacity=None):
        self.N, self.A, self.capacity = N, A, capacity
        self.reset()
        self.records, self.dropped = [], 0

    def reset(self):
        """mv_reset: accumulators and the tick counter go to zero, the records stay"""
        self.ret = np.zeros(self.N * self.A, np.float64)
        self.len = np.zeros(self.N, np.int32)
        self.tick = 0

    def restart(self):
        """the log switched off and on again: empty, zero accumulators; the tick counter runs on"""
        tick = self.tick
        self.reset()
        self.tick = tick
        self.records, self.dropped = [], 0

    def feed(self, rewards, dones, tobj):
        for r, d, o in zip(rewards, dones, tobj):
            self.ret += r.astype(np.float64)
            self.len += 1
            for e in np.flatnonzero(d).tolist():
                for a in range(self.A):
                    i = e * self.A + a
                    if self.capacity is None or len(self.records) < self.capacity:
                        self.records.append((i, int(self.len[e]), self.tick, o[i], self.ret[i]))
                    else:
                        self.dropped += 1
                    self.ret[i] = 0.0
                self.len[e] = 0
            self.tick += 1

    def drain(self, n=None):
        n = len(self.records) if n is None else min(n, len(self.records))
        out = np.array(self.records[:n], RECORD) if n else np.zeros(0, RECORD)
        del self.records[:n]
        return out


def expected_log(name, capacity=None):
    scenario, N, A, params, ticks, *_ = ALL_ROLLOUTS[name]
    m = Model(N, A, capacity)
    m.feed(*rollout(name))
    return m


def assert_floors(name, records):
    """a rollout that sees few episodes proves nothing: the floors on the EXPECTED log"""
    *_, min_records, min_nonzero, min_twice = ALL_ROLLOUTS[name]
    assert len(records) >= min_records, (name, len(records))
    assert int((records["ret"] != 0).sum()) >= min_nonzero, (name, int((records["ret"] != 0).sum()))
    if min_twice:   # an env finishing twice inside one aligned window of 16 ticks (a stepping call's worth), counted per env and window
        first = records[records["agent"] % ALL_ROLLOUTS[name][2] == 0]
        twice = 0
        for e in np.unique(first["agent"]):
            _, per_window = np.unique(first["end_tick"][first["agent"] == e] // 16, return_counts=True)
            twice += int((per_window >= 2).sum())
        assert twice >= min_twice, (name, twice)
