"""Scene observations without a device: the record's host twin (mv_debug_scene_obs_host) against a numpy restatement of its table (scene_obs_util), the
column tables, the refusals that need no gym.  Every comparison is equality of uint32 views."""
import itertools
import os
import re

import numpy as np
import pytest

import football_model
import scene_obs_util as S
from megaverse_amd import extension

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 32-bit patterns a float conversion would change: -0.0f, NaNs with payloads, denormals, infinities
SPECIALS = np.array([0x80000000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x00000000, 0x3f800000, 0xdeadbeef,
                     0x7fffffff, 0x00400000, 0xcafef00d, 0x12345678, 0xffffffff, 0x00000002, 0xffc00000, 0x7fa00000], np.uint32)


def same(got, want, what):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want, np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: columns {bad.tolist()}: {[hex(int(x)) for x in got[bad]]} vs {[hex(int(x)) for x in want[bad]]}"


def test_symbols_are_declared_exported_and_bound():
    """the four calls: declared in the header, exported by the library, bound with the declared arity; MV_SCENE_OBS_FLOATS == 32; the ABI version stays 2"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_set_scene_obs", 2), ("mv_get_scene_obs", 1), ("mv_get_scene_observation", 3), ("mv_debug_scene_obs_host", 7)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == arity
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert re.search(r"MV_SCENE_OBS_FLOATS\s*=\s*32\b", text)
    assert extension.MV_SCENE_OBS_FLOATS == 32
    assert lib.mv_abi_version() == 2


def common_header(rng, words=None):
    """a header whose int columns hold values a level can have and whose copied columns hold `words` (3 uint32) or random bits; everything the record does
    not read is filled with a pattern that must not leak"""
    h = np.zeros(1, S.ENV_HEADER)
    h.view(np.uint32)[:] = 0x5a5a5a5a
    h = h[0]
    for name, hi in (("L", 64), ("H", 16), ("W", 64), ("num_frames", 100000), ("solved", 2), ("highest_tower", 96), ("num_objects", 81), ("num_platforms", 973),
                     ("episodes_consumed", 1 << 20)):
        h[name] = rng.randint(0, hi)
    h["bz"] = rng.randint(0, 64, 4)
    h["num_terrain"], h["num_rewards"] = 0, 0
    w = rng.randint(0, 1 << 32, 3, dtype=np.uint64).astype(np.uint32) if words is None else np.asarray(words, np.uint32)
    for name, x in zip(("episode_sec", "episode_len", "bz_reward"), w):
        h[name] = np.array([x], np.uint32).view(np.float32)[0]
    return h


def host(scn, h, terrain=None, rewards=None, ball=None):
    return extension.debug_scene_obs_host(scn, h.tobytes(), None if terrain is None else terrain.tobytes(), None if rewards is None else rewards.tobytes(),
                                          None if ball is None else ball.tobytes())


def test_common_block_and_unlisted_scenarios():
    """columns 0..15 for every scenario family, the copied ones fed -0.0f, NaNs with payloads and denormals; the scenarios without columns of their own give
    an all-zero block 16..31 whatever the lists hold"""
    rng = np.random.RandomState(1)
    terrain = np.zeros(16, S.TERRAIN_BOX); terrain.view(np.uint32)[:] = 0x01010101   # (exit bits everywhere: must not show outside SCN_OBSTACLES)
    rewards = np.ones(96, S.MOVABLE)
    ball = np.zeros(1, football_model.STATE); ball.view(np.uint32)[:] = 0x3f800000
    for shift in range(len(SPECIALS)):
        words = np.roll(SPECIALS, shift)[:3]
        for name in ("Collect", "Rearrange", "Sokoban", "HexMemory", "BoxAGone", "Empty"):
            h = common_header(rng, words)
            got = host(S.SCN[name], h, terrain, rewards, ball[0])
            same(got, S.row(S.SCN[name], h, h["episodes_consumed"]), f"{name}, shift {shift}")
            assert (got.view(np.uint32)[15:] == 0).all()
            same(host(S.SCN[name], h), got.view(np.uint32), f"{name}: unused inputs are NULL")
    assert len(set(S.SCN.values())) == 10


def test_tower_and_hex_explore():
    """TowerBuilding: bz[0..3] as ints; HexExplore: hex_target copied, bit for bit"""
    rng = np.random.RandomState(2)
    for shift in range(len(SPECIALS)):
        h = common_header(rng, np.roll(SPECIALS, shift + 5)[:3])
        same(host(S.SCN_TOWER, h), S.row(S.SCN_TOWER, h, h["episodes_consumed"]), f"tower {shift}")
        t = np.roll(SPECIALS, shift)[:2].view(np.float32)
        h["hex_target"] = t
        want = S.row(S.SCN_HEX_EXPLORE, h, h["episodes_consumed"], hex_target=t)
        same(host(S.SCN_HEX_EXPLORE, h), want, f"hex explore {shift}")
        assert want[16:18].tolist() == np.roll(SPECIALS, shift)[:2].tolist() and (want[18:] == 0).all()


def exit_cases():
    """(num_terrain, indices of exit boxes): 0, 1 and 3 exits at first, middle and last index, and beyond num_terrain (ignored there)"""
    return [(0, []), (5, []), (5, [0]), (5, [2]), (5, [4]), (16, [15]), (16, [0, 7, 15]), (9, [3, 4, 8]), (4, [6]), (4, [1, 9, 12]), (1, [0]), (16, list(range(16)))]


@pytest.mark.parametrize("num_terrain,exits", exit_cases())
def test_obstacles_exits(num_terrain, exits):
    """column 16: the exit boxes below num_terrain; 17..22: min and max of the first of them, zeros when there is none.  Non-exit boxes carry other type bits"""
    rng = np.random.RandomState(3 + num_terrain + len(exits))
    h = common_header(rng)
    h["num_terrain"] = num_terrain
    terrain = np.zeros(16, S.TERRAIN_BOX)
    terrain["min"], terrain["max"] = rng.randint(0, 60, (16, 3)), rng.randint(1, 64, (16, 3))
    terrain["type"] = rng.choice([0, S.TERRAIN_LAVA, 4, 6], 16)
    terrain["pad"] = 0x7fffffff
    for i in exits:
        terrain["type"][i] |= S.TERRAIN_EXIT
    want = S.row(S.SCN_OBSTACLES, h, h["episodes_consumed"], terrain=terrain.view(np.int32).reshape(16, 8), rewards=np.zeros((0, 4), np.int8))
    same(host(S.SCN_OBSTACLES, h, terrain), want, f"{num_terrain}, {exits}")
    live = [i for i in exits if i < num_terrain]
    assert want[16] == S.of_int(len(live))[0]
    if live:
        assert want[17:20].tolist() == S.of_int(terrain["min"][live[0]]).tolist() and want[20:23].tolist() == S.of_int(terrain["max"][live[0]]).tolist()
    else:
        assert (want[17:23] == 0).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 96])
def test_obstacles_diamonds(n):
    """column 23 over reward lists of length 0, 1, 63, 64, 65 (the wave-round boundary of the device path) and 96: all there, none, alternating, only the
    first, only the last, random mixes with every state value a slot can hold, and slots beyond num_rewards that must not count"""
    rng = np.random.RandomState(n)
    mixes = [np.ones(n, np.int8), np.zeros(n, np.int8), (np.arange(n) % 2).astype(np.int8), (np.arange(n) == 0).astype(np.int8),
             (np.arange(n) == n - 1).astype(np.int8)] + [rng.choice(np.array([0, 1, 2, -1, 127, -128], np.int8), n) for _ in range(12)]
    if n <= 4:
        mixes += [np.array(m, np.int8) for m in itertools.product([0, 1], repeat=n)]
    for k, states in enumerate(mixes):
        h = common_header(rng)
        h["num_rewards"] = n
        rewards = np.zeros(96, S.MOVABLE)
        rewards["x"], rewards["y"], rewards["z"] = rng.randint(0, 64, 96), rng.randint(0, 16, 96), rng.randint(0, 64, 96)
        rewards["state"] = 1   # (beyond num_rewards: ignored)
        rewards["state"][:n] = states
        want = S.row(S.SCN_OBSTACLES, h, h["episodes_consumed"], terrain=np.zeros((16, 8), np.int32), rewards=rewards.view(np.int8).reshape(96, 4))
        assert want[23] == S.of_int(int((states != 0).sum()))[0]
        same(host(S.SCN_OBSTACLES, h, np.zeros(16, S.TERRAIN_BOX), rewards), want, f"length {n}, mix {k}")
        same(host(S.SCN_OBSTACLES, h, np.zeros(16, S.TERRAIN_BOX), rewards[:n]), want, f"length {n}, mix {k}: a list of exactly num_rewards")


def test_obstacles_random_levels():
    """random terrain and reward lists together"""
    rng = np.random.RandomState(11)
    for k in range(200):
        h = common_header(rng)
        h["num_terrain"], h["num_rewards"] = rng.randint(0, 17), rng.randint(0, 97)
        terrain = np.zeros(16, S.TERRAIN_BOX)
        terrain.view(np.int32)[:] = rng.randint(0, 64, 16 * 8)
        terrain["type"] = rng.randint(0, 8, 16)
        rewards = np.zeros(96, S.MOVABLE)
        rewards.view(np.int8)[:] = rng.randint(-128, 128, 96 * 4)
        rewards["state"] = rng.choice([0, 0, 1, 2], 96)
        want = S.row(S.SCN_OBSTACLES, h, h["episodes_consumed"], terrain=terrain.view(np.int32).reshape(16, 8), rewards=rewards.view(np.int8).reshape(96, 4))
        same(host(S.SCN_OBSTACLES, h, terrain, rewards), want, f"level {k}")


def test_football():
    """columns 16..30: FootballState's first 15 words, kicks and contacts as ints, everything else bit for bit; the pad word does not leak"""
    rng = np.random.RandomState(5)
    for shift in range(len(SPECIALS)):
        h = common_header(rng)
        ball = np.zeros(1, football_model.STATE)
        w = ball.view(np.uint32)
        w[:] = np.roll(SPECIALS, shift)[:16]
        ball["kicks"], ball["contacts"] = rng.randint(0, 9), rng.randint(0, 1 << 16)
        ball["pad"] = -1
        want = S.row(S.SCN_FOOTBALL, h, h["episodes_consumed"], ball=ball[0])
        same(host(S.SCN_FOOTBALL, h, ball=ball[0]), want, f"shift {shift}")
        assert want[31] == 0 and want[16:23].tolist() == w[0:7].tolist() and want[24:27].tolist() == w[8:11].tolist() and want[28:31].tolist() == w[12:15].tolist()


def test_field_tables():
    """SCENE_OBS_FIELDS: 16 distinct names in order; the per-scenario tables: distinct indices in 16..31, one table for every Obstacles variant, {} for the
    scenarios without columns; MegaverseEnv re-exports the same objects"""
    from megaverse_amd.megaverse_env import SUPPORTED_SCENARIOS, MegaverseEnv
    names = list(extension.SCENE_OBS_FIELDS)
    assert len(names) == 16 and len(set(names)) == 16 and [extension.SCENE_OBS_FIELDS[n] for n in names] == list(range(16))
    assert S.F == extension.SCENE_OBS_FIELDS   # (the tests' restatement indexes the same columns)
    tables = extension.SCENE_OBS_SCENARIO_FIELDS
    assert sorted(tables) == sorted(SUPPORTED_SCENARIOS) == sorted(S.SCN)
    for scenario, t in tables.items():
        idx = list(t.values())
        assert all(16 <= i <= 31 for i in idx) and len(set(idx)) == len(idx), scenario
        assert not (set(t) & set(names)), scenario
    obst = [n for n in tables if n.startswith("Obstacles")]
    assert len(obst) == 6 and all(tables[n] is tables["ObstaclesEasy"] for n in obst)
    for n in ("Collect", "Rearrange", "Sokoban", "HexMemory", "BoxAGone", "Empty"):
        assert tables[n] == {}
    assert sorted(tables["TowerBuilding"].values()) == [16, 17, 18, 19] and sorted(tables["HexExplore"].values()) == [16, 17]
    assert sorted(tables["ObstaclesHard"].values()) == list(range(16, 24)) and sorted(tables["Football"].values()) == list(range(16, 31))
    assert (tables["ObstaclesHard"]["num_exits"], tables["ObstaclesHard"]["diamonds_left"]) == (S.NUM_EXITS, S.DIAMONDS)
    assert (tables["Football"]["ball_x"], tables["Football"]["ball_radius"], tables["Football"]["kicks"], tables["Football"]["contacts"]) \
        == (S.BALL_POS, S.BALL_RADIUS, S.KICKS, S.CONTACTS)
    assert MegaverseEnv.SCENE_OBS_FIELDS is extension.SCENE_OBS_FIELDS and MegaverseEnv.SCENE_OBS_SCENARIO_FIELDS is tables
    assert hasattr(MegaverseEnv, "scene_obs")
    assert all(hasattr(extension.MegaverseGym, n) for n in ("set_scene_obs", "scene_obs", "scene_obs_ring", "get_scene_observation"))


def test_multitask_refuses_with_text():
    """MultiTaskGym.set_scene_obs raises before it touches a device"""
    from megaverse_amd.multitask import MultiTaskGym
    for arg in (True, None):
        with pytest.raises(RuntimeError, match="mv_set_scene_obs"):
            MultiTaskGym.set_scene_obs(type("G", (), {"_group": None})(), arg)


def test_no_gym_is_an_error_with_text():
    """a null gym: -1 with text from the three calls that take one; the host hook refuses what it cannot pack"""
    lib = extension.load_library()
    out = np.zeros(32, np.float32)
    for fn, args in ((lib.mv_set_scene_obs, (None,)), (lib.mv_get_scene_obs, ()), (lib.mv_get_scene_observation, (0, out.ctypes.data))):
        assert fn(None, *args) == -1
        assert b"null gym" in lib.mv_last_error() and b"scene_obs" in lib.mv_last_error()
    assert lib.mv_debug_scene_obs_host(0, None, None, None, 0, None, out.ctypes.data) == -1 and b"mv_debug_scene_obs_host" in lib.mv_last_error()
    h = S.header_record(num_rewards=3)
    with pytest.raises(RuntimeError, match="num_rewards"):
        host(S.SCN_OBSTACLES, h, np.zeros(16, S.TERRAIN_BOX), np.zeros(2, S.MOVABLE))
    with pytest.raises(RuntimeError, match="FootballState"):
        host(S.SCN_FOOTBALL, h)


class FakeTensor:
    """what check_scene_obs asks of a tensor, with no device behind it"""

    def __init__(self, shape, dtype="torch.float32", is_cuda=True, contiguous=True, index=0):
        self.shape, self.dtype, self.is_cuda, self._contiguous, self.asked = shape, dtype, is_cuda, contiguous, 0
        self.device = type("D", (), {"index": index, "__str__": lambda s: f"cuda:{index}"})()

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        self.asked += 1
        return 0


class RaisingLib:
    """a library that answers the ring count (none) and fails the test on every other call"""

    def mv_get_output_ring(self, g):
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


@pytest.mark.parametrize("bad", [FakeTensor((1, 3, 16)), FakeTensor((2, 3, 32)), FakeTensor((3, 32)), FakeTensor((1, 3, 32), dtype="torch.float64"),
                                 FakeTensor((1, 3, 32), is_cuda=False), FakeTensor((1, 3, 32), contiguous=False), FakeTensor((1, 6, 32)),
                                 np.zeros((1, 3, 32), np.float32)],
                         ids=["columns", "entries", "rank", "float64", "cpu", "strided", "rows-per-agent", "numpy"])
def test_tensor_is_checked_before_any_device_call(bad):
    """a wrong shape (one row per ENV, not per agent), dtype or device, a strided tensor, a host array: ValueError from set_scene_obs, nothing attached"""
    gym = extension.MegaverseGym.__new__(extension.MegaverseGym)
    gym._lib, gym._g, gym.num_envs, gym.num_agents_per_env, gym.device, gym._scene_obs = RaisingLib(), None, 3, 2, 0, "before"
    with pytest.raises(ValueError, match="set_scene_obs"):
        gym.set_scene_obs(bad)
    assert getattr(bad, "asked", 0) == 0 and gym._scene_obs == "before"
    good = FakeTensor((4, 3, 32))
    assert extension.check_scene_obs(good, 4, 3, 0) is good
