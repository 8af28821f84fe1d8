"""Shared by tests/test_action_ring*.py: the biased action scripts the action-ring tests replay, and their cases."""
import numpy as np

TICKS = 96
# the shortest episodes mv_recommended_ticks_per_call still answers >= 8 for (statusPeriod 16: episodeLengthSec * 15 >= 64 ticks): an auto-reset falls inside a call
EPISODE_SEC = 4.27
# name -> (scenario, envs, agents per env)
CASES = {
    "tower": ("TowerBuilding", 7, 1), "obstacles_hard": ("ObstaclesHard", 6, 1), "collect": ("Collect", 5, 1), "rearrange": ("Rearrange", 6, 1),
    "hex_memory": ("HexMemory", 4, 1), "tower_a3": ("TowerBuilding", 5, 3), "obstacles_easy_a2": ("ObstaclesEasy", 6, 2),
}
# the calls the 96 ticks are played in: short and full ones, a 16-tick call is two step launches of 8
CALLS = [8, 16, 5, 16, 3, 16, 16, 16]
assert sum(CALLS) == TICKS
# name -> (idle ticks before the script's window, script seed).  Most scenarios add their own time to episodeLengthSec (TowerBuilding 4 s per object, the
# Obstacles family never goes below 35 s per platform), so their first episodes end after hundreds of ticks: the window starts ~40 ticks before the first env
# of an idle run finishes.  Chosen on the CPU oracle so that the window holds at least one non-zero reward and at least one done; the oracle test asserts it.
WARMUP = {"tower": (1464, 1), "obstacles_hard": (1728, 2), "collect": (80, 1), "rearrange": (24, 24), "hex_memory": (112, 1), "tower_a3": (1464, 1),
          "obstacles_easy_a2": (496, 1)}


def make_script(seed, ticks, agents):
    """[ticks, agents, 6] int32 multi-discrete actions (heads: strafe, walk, turn, jump, interact, look up / down), numpy from a fixed seed.  Biased, not
    uniform: runs of 3..16 ticks per agent in which walking forward (often with interact) dominates, with long turn and look runs between them -- an agent
    that gets somewhere, picks things up and puts them down, where the uniform policy dithers on the spot."""
    rng = np.random.default_rng(seed)
    out = np.zeros((ticks, agents, 6), np.int32)
    for a in range(agents):
        t = 0
        while t < ticks:
            run = int(rng.integers(3, 17))
            kind = int(rng.choice(6, p=[0.35, 0.25, 0.15, 0.10, 0.10, 0.05]))
            seg = out[t:t + run, a]
            n = seg.shape[0]
            if kind == 0:     # forward, interact now and then
                seg[:, 1] = 1
                seg[:, 4] = rng.random(n) < 0.25
            elif kind == 1:   # forward with interact held, a jump now and then
                seg[:, 1] = 1
                seg[:, 4] = 1
                seg[:, 3] = rng.random(n) < 0.15
            elif kind == 2:   # a long turn
                seg[:, 2] = 1 + int(rng.integers(0, 2))
            elif kind == 3:   # a long look up or down, interact at its end
                seg[:, 5] = 1 + int(rng.integers(0, 2))
                seg[-1, 4] = 1
            elif kind == 4:   # forward while turning
                seg[:, 1] = 1
                seg[:, 2] = 1 + int(rng.integers(0, 2))
            else:             # strafe or back off, jumping
                seg[:, int(rng.integers(0, 2))] = 1 + int(rng.integers(0, 2))
                seg[:, 3] = rng.random(n) < 0.5
            t += run
    return out
