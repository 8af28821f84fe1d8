"""The Obstacles family's and Empty's generator that runs on the device (megaverse_amd/csrc/mv_obstacles_draw.h), compiled for the CPU
(mv_debug_obstacles_draw_host: no GPU involved), against the product's host generator (mv_gen_obstacles.cpp through mv_debug_generate_episode, which
test_host_generators.py holds against the oracle): the same env seed -> byte-identical episodes -- merged slabs, terrain, movable boxes, reward objects, spawn
cells and rotations, colours, episode length -- over consecutive episodes of one env's stream.  The host generator keeps its chain in std::vector / std::map /
std::set and draws through libstdc++; the device code keeps it in fixed arrays and two bit planes, so this is where the restatement is pinned."""
import numpy as np
import pytest

from megaverse_amd import extension as ext
from test_host_generators import EPISODE_BLOB, generate

NAMES = ["ObstaclesEasy", "ObstaclesMedium", "ObstaclesHard", "ObstaclesWalls", "ObstaclesSteps", "ObstaclesLava", "Empty"]
# The committed seed set: the four corner values, 40 drawn once from np.random.default_rng(20260) and two added by a search over the host generator
# (mv_debug_obstacles_draw_stats_host) so that the set reaches the retry loop: as ObstaclesHard's first episode, env seed 28 takes four chain attempts
# (three hull clashes) and 67 takes three.
CLASH_SEEDS = [28, 67]
SEEDS = [0, 1, 42, (1 << 30) - 1] + [int(s) for s in np.random.default_rng(20260).integers(0, 1 << 30, 40)] + CLASH_SEEDS
GEN_FLAG_NAMES = {1: "GEN_SLABS", 2: "GEN_TERRAIN", 4: "GEN_OBJECTS", 8: "GEN_REWARDS", 16: "GEN_COORDS"}


def draw_host(name, agents, env_seed, n, base_len=60.0):
    lib = ext.load_library()
    size = lib.mv_debug_obstacles_draw_host(name.encode(), agents, env_seed, n, base_len, None, 0)
    assert size == EPISODE_BLOB.itemsize, (size, ext.last_error() if hasattr(ext, "last_error") else "")
    buf = np.zeros(1, EPISODE_BLOB)
    assert lib.mv_debug_obstacles_draw_host(name.encode(), agents, env_seed, n, base_len, buf.ctypes.data, size) == size
    return buf[0]


def draw_stats(name, agents, env_seed, n, base_len=60.0):
    """-> (host generator: attempts, left turns, right turns, GEN_* flags), (the device code on the CPU: the same four)"""
    out = np.zeros(8, np.int32)
    assert ext.load_library().mv_debug_obstacles_draw_stats_host(name.encode(), agents, env_seed, n, base_len, out.ctypes.data) == 0
    return tuple(int(v) for v in out[:4]), tuple(int(v) for v in out[4:])


def assert_same_episode(got, want, agents, what):
    for f in ("num_boxes", "num_terrain", "num_objects", "num_rewards", "num_platforms", "layout_color", "wall_color", "draw_walls"):
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert np.float32(got["episode_len"]).tobytes() == np.float32(want["episode_len"]).tobytes(), (what, got["episode_len"], want["episode_len"])
    assert (got["dim"] == want["dim"]).all() and (got["org"] == want["org"]).all(), (what, got["dim"], want["dim"], got["org"], want["org"])
    assert (got["spawn"] == want["spawn"]).all(), what
    assert (got["yaw_frand"][:agents].view(np.uint32) == want["yaw_frand"][:agents].view(np.uint32)).all(), what
    for name, count in (("boxes", "num_boxes"), ("terrain", "num_terrain"), ("objects", "num_objects"), ("rewards", "num_rewards")):
        n = int(want[count])
        assert got[name][:n].tobytes() == want[name][:n].tobytes(), (what, name)


@pytest.mark.parametrize("agents", [1, 4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_device_code_on_the_host_draws_the_host_generators_episodes(name, agents):
    for s in SEEDS:
        for n in (1, 2, 3):
            got, want = draw_host(name, agents, s, n), generate(name, agents, s, n)
            assert got["seq"] == n
            assert_same_episode(got, want, agents, (name, s, n))


def test_long_env_stream_and_episode_length_parameter():
    # one env's stream far down (every episode re-seeds from the one before), and the base episode length
    for n in (10, 57):
        assert_same_episode(draw_host("ObstaclesHard", 3, 777, n), generate("ObstaclesHard", 3, 777, n), 3, n)
        assert draw_host("ObstaclesHard", 3, 777, n)["seq"] == n
    assert_same_episode(draw_host("Empty", 2, 777, 57), generate("Empty", 2, 777, 57), 2, 57)
    for name in ("ObstaclesEasy", "Empty"):
        got, want = draw_host(name, 1, 5, 1, 10.0), generate(name, 1, 5, 1, 10.0)
        assert_same_episode(got, want, 1, (name, "base_len"))
    assert draw_host("Empty", 1, 5, 1, 10.0)["episode_len"] == np.float32(10.0)
    assert draw_host("ObstaclesEasy", 1, 5, 1, 10.0)["episode_len"] >= 35.0   # (35 s per platform: the parameter is a floor)


def test_the_seed_set_reaches_the_retry_loop_both_turns_and_no_capacity():
    """What the committed seed set exercises, judged on the HOST generator alone (and the device code agrees on how each episode came about)."""
    clashes, both_turns = 0, 0
    for s in SEEDS:
        for n in (1, 2, 3):
            host, dev = draw_stats("ObstaclesHard", 1, s, n)
            assert host == dev, (s, n, host, dev)
            assert host[3] == 0, (s, n, GEN_FLAG_NAMES.get(host[3], host[3]))
            clashes += host[0] > 1
            both_turns += host[1] > 0 and host[2] > 0
    assert clashes >= 1 and both_turns >= 1, (clashes, both_turns)
    for s in CLASH_SEEDS:
        assert draw_stats("ObstaclesHard", 1, s, 1)[0][0] >= 3, s
    for name in NAMES:
        for s in SEEDS:
            host, dev = draw_stats(name, 8, s, 2)
            assert host == dev and host[3] == 0, (name, s, host, dev)


def test_no_seed_of_the_first_ten_thousand_exceeds_a_capacity():
    """The issue asks for one level forced over MAX_OBJECTS or MAX_BOXES if some env seed among the first 10 000 does that on the host.  None does: for
    ObstaclesHard (one agent, first episode) and for the five other Obstacles names (eight agents, first episode) the host generator raises no capacity flag
    for any seed in 0 .. 9999, and neither for ObstaclesHard's second and third episodes of seeds 0 .. 2999 -- searched with mv_debug_obstacles_draw_stats_host
    when this test was written; what is left of that search here is a sample of it that runs in a second: every 7th seed of ObstaclesHard, with the device
    code's flags, attempts and turns held against the host's."""
    worst = 0
    for s in range(0, 10000, 7):
        host, dev = draw_stats("ObstaclesHard", 1, s, 1)
        assert host == dev and host[3] == 0, (s, host, dev)
        worst = max(worst, host[0])
    assert 2 <= worst <= 20, worst
