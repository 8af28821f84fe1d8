"""Entity observations without a device: the record's host twin (mv_debug_entity_obs_host) against an independent numpy model of its table (entity_obs_util)
on every tick of oracle rollouts of every scenario family, the layout tables, the row arithmetic of the label words, the refusals that need no gym.  Every
comparison is equality of uint32 views.  Every rollout asserts a counter of what it contained: none of the comparisons can pass on an empty scene."""
import os
import re

import numpy as np
import pytest

import entity_obs_util as EU
import episode_log_util as U
import football_model
import state_obs_util as SO
from megaverse_amd import extension
from megaverse_amd.rollout import action_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TICKS, POLICY_SEED = 3, 200, 7

# (scenario, agents) -> (env seed, float params, the events the rollout must contain).  The seeds were chosen by running the oracle on the CPU under
# EU.scripted_actions(POLICY_SEED, tick, ...): each rollout provably holds what its row lists (the counters are asserted below).
# episodeLengthSec: TowerBuilding adds 4 s per object to it, so -300 ends every episode on its first tick -- a new level, with another object count, per tick;
# HexExplore, Football and Empty take it as it is.
ROLLOUTS = {
    ("TowerBuilding", 1): (42, None, ("carried", "put_down")),
    ("TowerBuilding", 2): (43, None, ("carried", "put_down")),
    ("TowerBuilding", 4): (42, {"episodeLengthSec": -300.0}, ("reset",)),
    ("ObstaclesEasy", 1): (43, None, ("carried",)),
    ("ObstaclesEasy", 2): (42, None, ("carried", "put_down")),
    ("ObstaclesHard", 1): (42, None, ("picked_diamond",)),
    ("ObstaclesHard", 2): (43, None, ("picked_diamond", "put_down")),
    ("Collect", 1): (42, None, ("red_diamond", "carried", "put_down")),
    ("Collect", 2): (42, None, ("red_diamond", "picked_diamond")),
    ("Rearrange", 1): (42, None, ("carried",)),
    ("Rearrange", 2): (43, None, ("carried",)),
    ("Sokoban", 1): (42, None, ("pushed",)),
    ("Sokoban", 2): (43, None, ("pushed",)),
    ("HexMemory", 1): (42, None, ("dead_hex",)),
    ("HexMemory", 2): (43, None, ("dead_hex",)),
    ("HexExplore", 1): (42, {"episodeLengthSec": 1.5}, ("reset",)),
    ("HexExplore", 2): (43, {"episodeLengthSec": 1.5}, ("reset",)),
    ("BoxAGone", 1): (42, None, ("reset",)),
    ("BoxAGone", 2): (43, None, ("reset",)),
    ("Football", 1): (42, {"episodeLengthSec": 1.5}, ("kick", "reset")),
    ("Football", 2): (43, {"episodeLengthSec": 1.5}, ("kick", "reset")),
    ("Empty", 1): (42, {"episodeLengthSec": 2.0}, ("reset",)),
    ("Empty", 2): (43, {"episodeLengthSec": 2.0}, ("reset",)),
}


def same(got, want, what):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want, np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at (row, column) {bad[0].tolist()}: {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x}"


def host(name, A, snap, ball=None):
    return extension.debug_entity_obs_host(name, A, **EU.struct_images(name, A, snap, ball))


def counts_of(name, snap):
    """how many records of each group exist in a snapshot (the rows behind them must be all zero)"""
    fam = EU.SCN[name]
    terrain = {0: 1, 1: int(snap["num_terrain"]), 3: int(snap["num_items"]), 4: min(int((np.asarray(snap["soko"]) == EU.SOKO_GOAL).sum()), EU.MAX_OBJECTS)}.get(fam, 0)
    rewards = int(snap["hex_num_objs"]) if fam in (6, 7) else 1 if fam == 9 else int(snap["num_rewards"])
    return {"terrain": terrain, "objects": int(snap["num_objects"]), "rewards": rewards}


@pytest.mark.parametrize("scenario,A", sorted(ROLLOUTS))
def test_host_twin_against_the_model_on_oracle_rollouts(oracle, scenario, A):
    """3 envs, 200 ticks of the oracle under the interact-heavy action script: behind mv_reset and behind every tick the host pack function, fed the raw record
    bytes of every env, gives the model's rows bit for bit; rows past a group's count are all zero, on reset ticks too; the rollout contains its events"""
    seed, params, must = ROLLOUTS[(scenario, A)]
    U.boxoban_env()
    og = oracle.OracleGym(scenario, 32, 32, N, A, 1, False, params)
    og.seed(seed)
    og.reset()
    lay, E = EU.layout(scenario, A)
    ev = EU.Events()
    ball_of = (lambda e: og.football_state(e)) if scenario == "Football" else (lambda e: None)
    before = [og.snapshot(e) for e in range(N)]
    distinct = set()
    for tick in range(-1, TICKS):
        if tick >= 0:
            masks = action_masks(EU.scripted_actions(POLICY_SEED, tick, N * A))
            for e in range(N):
                for a in range(A):
                    og.set_action_mask(e, a, int(masks[e * A + a]))
            og.step_norender()
        dones = og.get_dones() if tick >= 0 else np.zeros(N, np.uint8)
        for e in range(N):
            snap, ball = og.snapshot(e), ball_of(e)
            got = host(scenario, A, snap, ball)
            assert got.shape == (E, 8)
            same(got, EU.rows(scenario, A, snap, ball), f"{scenario}, {A} agents, tick {tick}, env {e}")
            bits = got.view(np.uint32)
            for group, n in counts_of(scenario, snap).items():
                base, rows, _ = lay[group]
                assert (bits[base + min(n, rows):base + rows] == 0).all(), f"tick {tick}, env {e}: rows past the {n} {group} records are not zero"
                assert (bits[base:base + min(n, rows), 0] != 0).all(), f"tick {tick}, env {e}: a {group} record without its word"
            if tick >= 0:
                ev.see(scenario, e, before[e], snap, dones[e], ball)
            before[e] = snap
            distinct.add(got.tobytes())
    og.close()
    missing = [k for k in must if ev.c[k] == 0]
    assert not missing, f"{scenario}, {A} agents: the rollout holds no {missing}: {ev.c}"
    assert len(distinct) > TICKS // 2, "the rows barely changed: the comparison would prove less than it says"


def test_symbols_are_declared_exported_and_bound():
    """the six calls: declared in the header, exported by the library, bound with the declared arity; MV_ENTITY_OBS_FLOATS == 8; the ABI version stays 2"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_entity_obs_rows", 1), ("mv_entity_obs_layout", 2), ("mv_set_entity_obs", 2), ("mv_get_entity_obs", 1),
                        ("mv_get_entity_observation", 3), ("mv_debug_entity_obs_host", 13)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == arity
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert re.search(r"MV_ENTITY_OBS_FLOATS\s*=\s*8\b", text)
    assert extension.MV_ENTITY_OBS_FLOATS == 8 and list(extension.ENTITY_OBS_FIELDS) == list(EU.F) and extension.ENTITY_OBS_FIELDS == EU.F
    assert lib.mv_abi_version() == 2


def hex_header(n):
    h = np.zeros(1, SO.ENV_HEADER)
    h["num_rewards"] = n
    return h


def test_hex_memory_good_is_hidden():
    """two HexMemory records that differ only in the `good` bit of meta (bit 4) give identical rows, alive or dead, for every shape"""
    agents = np.zeros(1, SO.AGENT_STATE)
    rng = np.random.RandomState(5)
    for alive in (0, 1):
        for shape in (0, 1, 2):
            objs = np.zeros((2, 128), EU_HEX())
            for k in range(2):
                objs[k]["a"], objs[k]["b"] = rng.rand(128, 3), rng.rand(128, 3)
            objs[1] = objs[0]
            cell_bits = rng.randint(0, 1 << 16, 128) << 12
            objs[0]["meta"] = shape | (0 << 4) | (alive << 8) | cell_bits
            objs[1]["meta"] = shape | (1 << 4) | (alive << 8) | cell_bits
            objs[0]["color"], objs[1]["color"] = 0x112233, 0x112233
            rows = [extension.debug_entity_obs_host("HexMemory", 1, hex_header(128).tobytes(), agents.tobytes(), hex_objs=o.tobytes()).view(np.uint32) for o in objs]
            assert (objs[0]["meta"] != objs[1]["meta"]).all()
            same(rows[0], rows[1], f"alive {alive}, shape {shape}")
            want = EU.of_int(1 + shape if alive else 0)[0]
            assert (rows[0][:128, 7] == want).all() and (rows[0][:128, 0] == EU.of_int((EU.K["COLLECTABLE"] << 12) + np.arange(128))).all()


def EU_HEX():
    import oracle_lib
    return oracle_lib.HEX_REC


@pytest.mark.parametrize("goals", [0, 1, 4, 63, 64, 65, 80, 81, 200, 1024])
def test_sokoban_goal_rows(goals):
    """the compacted group: row k is the k-th SOKO_GOAL cell of np.flatnonzero(cells == SOKO_GOAL), its word carries x * W + z, its cell is (x, 1, z) at voxel
    size 2; the rows behind the last goal are zero; goals beyond the 80th get no row.  Counts at the rounds' boundaries of the device path (64 cells)"""
    rng = np.random.RandomState(goals)
    cells = rng.choice(np.array([0, 1], np.uint8), 1024)   # (floor and walls)
    where = np.sort(rng.choice(1024, goals, replace=False))
    cells[where] = EU.SOKO_GOAL
    h = np.zeros(1, SO.ENV_HEADER)
    h["W"], h["L"] = 32, 32
    agents = np.zeros(2, SO.AGENT_STATE)
    got = extension.debug_entity_obs_host("Sokoban", 2, h.tobytes(), agents.tobytes(), soko=cells.tobytes(), objects=np.zeros(320, np.uint8).tobytes()).view(np.uint32)
    idx = np.flatnonzero(cells == EU.SOKO_GOAL)
    assert idx.tolist() == where.tolist()
    listed = idx[:80]
    assert (got[:len(listed), 0] == EU.of_int((EU.K["EXIT"] << 12) + (listed // 32) * 32 + listed % 32)).all()
    assert (got[:len(listed), 1].view(np.float32) == 2.0 * (listed // 32) + 1.0).all() and (got[:len(listed), 3].view(np.float32) == 2.0 * (listed % 32) + 1.0).all()
    assert (got[:len(listed), 2].view(np.float32) == 3.0).all() and (got[:len(listed), 4:7].view(np.float32) == 1.0).all() and (got[:len(listed), 7].view(np.float32) == 1.0).all()
    assert (got[len(listed):160] == 0).all()
    snap = {"soko": cells, "W": 32, "num_objects": 0, "objects": np.zeros((80, 4), np.int8), "agents": np.zeros(2, [("pos", "<f4", 3), ("carrying", "<i4")])}
    same(got, EU.rows("Sokoban", 2, snap), f"{goals} goals")


def test_layout_against_the_table():
    """entity_layout / entity_rows / the model's table agree for every scenario and agent count; E <= 192 (three rounds of a wave); HexMemory has the most"""
    from megaverse_amd import ENTITY_OBS_FIELDS, entity_layout, entity_rows
    from megaverse_amd.megaverse_env import SUPPORTED_SCENARIOS
    assert ENTITY_OBS_FIELDS is extension.ENTITY_OBS_FIELDS
    want = {"TowerBuilding": (1, 80, 0), "ObstaclesEasy": (16, 80, 16), "ObstaclesHard": (16, 80, 16), "Collect": (0, 80, 96), "Rearrange": (8, 80, 0),
            "Sokoban": (80, 80, 0), "HexMemory": (0, 0, 128), "HexExplore": (0, 0, 128), "BoxAGone": (0, 0, 0), "Football": (0, 0, 1), "Empty": (0, 0, 0)}
    assert set(want) <= set(SUPPORTED_SCENARIOS) and set(want) == set(EU.SCENARIOS)
    for name in SUPPORTED_SCENARIOS:
        for A in range(1, 9):
            lay = entity_layout(name, A)
            assert list(lay) == ["terrain", "objects", "rewards", "agents"]
            at = 0
            for s in lay.values():
                assert s.start == at and s.step is None
                at = s.stop
            assert at == entity_rows(name, A) <= 192
            if name in want:
                assert tuple(s.stop - s.start for s in lay.values()) == want[name] + (A,), (name, A)
                model, E = EU.layout(name, A)
                assert E == at and [(b, b + n) for b, n, _ in model.values()] == [(s.start, s.stop) for s in lay.values()]
    with pytest.raises(ValueError):
        entity_layout("NoSuchScenario", 1)
    with pytest.raises(ValueError):
        entity_layout("Collect", 9)


def test_row_of_words():
    """entity_row_of: the row of a label word is its group's base + its instance; -1 for the classes without rows, for instances beyond the group, for classes
    of another scenario and for Sokoban's EXIT; numpy int16 planes are read as unsigned words"""
    from megaverse_amd import entity_row_of
    K = EU.K
    w = lambda c, i: (K[c] << 12) | i   # noqa: E731
    for name, A in (("ObstaclesHard", 2), ("Collect", 4), ("TowerBuilding", 1), ("Rearrange", 2), ("Sokoban", 2), ("HexMemory", 8), ("Football", 2), ("BoxAGone", 3)):
        lay, E = EU.layout(name, A)
        cases = {0: -1, w("FLOOR", 3): -1, w("STRUCTURE", 100): -1, w("FURNITURE", 2): -1, w("HUD", 0): -1, w("AGENT", A - 1): lay["agents"][0] + A - 1,
                 w("AGENT", A): -1}
        if lay["objects"][1]:
            cases.update({w("MOVABLE", 79): lay["objects"][0] + 79, w("CARRIED", 5): lay["objects"][0] + 5, w("MOVABLE", 80): -1})
        else:
            cases[w("MOVABLE", 0)] = -1
        fam = EU.SCN[name]
        if fam == 1:
            cases.update({w("EXIT", 0): 0, w("LAVA", 15): 15, w("LAVA", 16): -1, w("COLLECTABLE", 15): lay["rewards"][0] + 15, w("COLLECTABLE", 16): -1, w("HAZARD", 0): -1})
        if fam == 2:
            cases.update({w("COLLECTABLE", 95): lay["rewards"][0] + 95, w("HAZARD", 7): lay["rewards"][0] + 7, w("COLLECTABLE", 96): -1, w("EXIT", 0): -1})
        if fam == 0:
            cases.update({w("BUILDING_ZONE", 0): 0, w("BUILDING_ZONE", 1): -1, w("COLLECTABLE", 0): -1})
        if fam == 3:
            cases.update({w("TARGET", 7): 7, w("TARGET", 8): -1})
        if fam == 4:
            cases.update({w("EXIT", 0): -1, w("EXIT", 33): -1})
        if fam == 6:
            cases.update({w("COLLECTABLE", 127): 127, w("COLLECTABLE", 128): -1, w("BALL", 0): -1})
        if fam == 9:
            cases.update({w("BALL", 0): 0, w("BALL", 1): -1, w("COLLECTABLE", 0): -1})
        words = np.array(list(cases), np.uint16)
        got = entity_row_of(words.view(np.int16).reshape(1, -1), name, A)
        assert got.shape == (1, len(words)) and got[0].tolist() == list(cases.values()), (name, dict(zip(cases, got[0].tolist())))
        assert entity_row_of(words.astype(np.int32), name, A).tolist() == list(cases.values())
        import torch
        for t in (torch.as_tensor(words.view(np.int16).copy()), torch.as_tensor(words.astype(np.int32))):   # (the tensors a label plane comes as)
            assert entity_row_of(t, name, A).tolist() == list(cases.values())
        assert ((got >= -1) & (got < E)).all()


def test_multitask_refuses_with_text():
    """MultiTaskGym.set_entity_obs raises before it touches a device, with the group refusal's text"""
    from megaverse_amd.multitask import MultiTaskGym
    for arg in (True, None):
        with pytest.raises(RuntimeError, match="mv_set_entity_obs"):
            MultiTaskGym.set_entity_obs(type("G", (), {"_group": None})(), arg)


def test_no_gym_is_an_error_with_text():
    """a null gym: -1 with text from the five calls that take one; the host hook refuses what it cannot pack"""
    lib = extension.load_library()
    out = np.zeros(192 * 8, np.float32)
    lay = np.zeros((4, 3), np.int32)
    for fn, args in ((lib.mv_set_entity_obs, (None,)), (lib.mv_get_entity_obs, ()), (lib.mv_get_entity_observation, (0, out.ctypes.data)),
                     (lib.mv_entity_obs_rows, ()), (lib.mv_entity_obs_layout, (lay.ctypes.data,))):
        assert fn(None, *args) == -1
        assert b"null gym" in lib.mv_last_error() and b"entity_obs" in lib.mv_last_error()
    assert (out == 0).all() and (lay == 0).all()
    assert lib.mv_debug_entity_obs_host(0, 1, None, None, None, None, None, None, 0, None, None, None, out.ctypes.data) == -1
    assert b"mv_debug_entity_obs_host" in lib.mv_last_error()
    h, a = np.zeros(1, SO.ENV_HEADER), np.zeros(1, SO.AGENT_STATE)
    h["num_rewards"] = 3
    with pytest.raises(RuntimeError, match="num_rewards"):
        extension.debug_entity_obs_host("ObstaclesHard", 1, h.tobytes(), a.tobytes(), terrain=bytes(512), objects=bytes(320), rewards=bytes(8))
    with pytest.raises(RuntimeError, match="FootballState"):
        extension.debug_entity_obs_host("Football", 1, h.tobytes(), a.tobytes())
    with pytest.raises(RuntimeError, match="1024 level cells"):
        extension.debug_entity_obs_host("Sokoban", 1, h.tobytes(), a.tobytes(), objects=bytes(320))
    with pytest.raises(ValueError):
        extension.debug_entity_obs_host("Football", 1, h.tobytes(), bytes(64), football_state=np.zeros(1, football_model.STATE).tobytes())
    assert (out == 0).all()


class FakeTensor:
    """what check_entity_obs asks of a tensor, with no device behind it"""

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


@pytest.mark.parametrize("bad", [FakeTensor((1, 3, 178, 4)), FakeTensor((2, 3, 178, 8)), FakeTensor((3, 178, 8)), FakeTensor((1, 3, 178, 8), dtype="torch.float64"),
                                 FakeTensor((1, 3, 178, 8), is_cuda=False), FakeTensor((1, 3, 178, 8), contiguous=False), FakeTensor((1, 3, 177, 8)),
                                 np.zeros((1, 3, 178, 8), np.float32)],
                         ids=["columns", "entries", "rank", "float64", "cpu", "strided", "rows", "numpy"])
def test_tensor_is_checked_before_any_device_call(bad):
    """a wrong shape (E rows per env: Collect with two agents has 178), dtype or device, a strided tensor, a host array: ValueError from set_entity_obs,
    nothing attached"""
    gym = extension.MegaverseGym.__new__(extension.MegaverseGym)
    gym._lib, gym._g, gym.num_envs, gym.num_agents_per_env, gym.device, gym._entity_obs, gym.scenario = RaisingLib(), None, 3, 2, 0, "before", "Collect"
    with pytest.raises(ValueError, match="set_entity_obs"):
        gym.set_entity_obs(bad)
    assert getattr(bad, "asked", 0) == 0 and gym._entity_obs == "before"
    good = FakeTensor((4, 3, 178, 8))
    assert extension.check_entity_obs(good, 4, 3, 178, 0) is good
