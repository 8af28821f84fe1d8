"""HexMemory's and HexExplore's generator that runs on the device (megaverse_amd/csrc/mv_hex_draw.h), compiled for the CPU (mv_debug_draw_host: no GPU
involved, the parallel phases in their serial form), against the product's host generator (mv_gen_hex.cpp through mv_debug_generate_episode, which
test_host_generators.py holds against the oracle): the same env seed -> the same record, field for field -- the header, the first num_agents spawn points and
rotations, objs[:num_objs], boxes[:num_boxes] -- over consecutive episodes of one env's stream."""
import numpy as np
import pytest

from draw_util import draw_host
from test_host_generators import generate

NAMES = ["HexMemory", "HexExplore"]
# 0, 1, 42, the largest seed, and 196 drawn once from np.random.default_rng(20261)
SEEDS = [0, 1, 42, (1 << 30) - 1] + [int(s) for s in np.random.default_rng(20261).integers(0, 1 << 30, 196)]
HEADER = ("num_boxes", "num_colliders", "num_objs", "num_good", "episode_len", "target")


def assert_same_episode(got, want, agents, what):
    for f in HEADER:
        assert got[f].tobytes() == want[f].tobytes(), (what, f, got[f], want[f])
    assert got["spawn"][:agents].tobytes() == want["spawn"][:agents].tobytes(), (what, got["spawn"][:agents], want["spawn"][:agents])
    assert got["yaw"][:agents].tobytes() == want["yaw"][:agents].tobytes(), what
    for name, count in (("objs", "num_objs"), ("boxes", "num_boxes")):
        n = int(want[count])
        same = [got[name][i].tobytes() == want[name][i].tobytes() for i in range(n)]
        assert all(same), (what, name, same.index(False), got[name][same.index(False)], want[name][same.index(False)])
    assert not got["boxes"][int(want["num_boxes"]):].tobytes().strip(b"\0"), what   # (the device code leaves the rest zero)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("agents", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_device_code_on_the_host_draws_the_host_generators_episodes(name, agents, n):
    """... and what the seed set covers, judged on the HOST generator's records alone: every maze size, landmarks, and HexMemory's bad_count.

    bad_count has ONE outcome, not two.  It is good_count unless places < 2 good_count, with good_count = ceil(fraction x places), fraction = frand x 0.25 +
    0.2 < 0.45 and places = 3 size (size - 1) = 6, 18, 36, 60, 90 or 126: ceil(0.45 x places) is 3, 9, 17, 27, 41 and 57, never above places / 2 -- at size 2
    it reaches exactly half.  No env seed in 0 .. 5999 gives a HexMemory episode without bad objects on the host generator (1018 of them are mazes of size 2).
    So the zero branch cannot be covered by any seed list; what is asserted is that every episode of the set has its bad objects, sizes 2 included."""
    sizes, landmarks, bad = set(), 0, set()
    for s in SEEDS:
        got, want = draw_host(name, agents, s, n), generate(name, agents, s, n)
        assert got["seq"] == n
        assert_same_episode(got, want, agents, (name, s, n))
        # what this seed exercises, read from the HOST generator's record alone: the floor spans 2 sqrt(3) (size - 0.5) x 3.5 each way from the centre
        floor = want["boxes"][0]
        sizes.add(int(round((floor["b"][0] - floor["a"][0]) / (4 * np.sqrt(3.0) * 3.5) + 0.5)))
        walls = int(want["num_colliders"]) - 1
        landmarks += int(want["num_boxes"]) - 1 - 2 * walls
        bad.add(int(want["num_objs"]) - 1 - int(want["num_good"]) > 0)
    assert sizes == {2, 3, 4, 5, 6, 7}, sizes
    assert landmarks > 0
    if name == "HexMemory":
        assert bad == {True}, bad
