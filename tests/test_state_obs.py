"""State observations without a device: the record against a numpy restatement of its table, the column names, the refusals that need no gym."""
import os
import re

import numpy as np
import pytest

import state_obs_util as S
from megaverse_amd import extension
from megaverse_amd.rollout import action_masks, sample_actions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    """the calls: declared in the header, exported by the library, bound with the declared arity; MV_STATE_OBS_FLOATS == 16; the ABI version stays 2"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_set_state_obs", 2), ("mv_get_state_obs", 1), ("mv_get_state_observation", 4), ("mv_debug_state_obs_host", 3),
                        ("mv_get_output_ring", 1)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == arity
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert re.search(r"MV_STATE_OBS_FLOATS\s*=\s*16\b", text)
    assert extension.MV_STATE_OBS_FLOATS == 16
    assert lib.mv_abi_version() == 2


def interact_heavy_masks(seed, step, n):
    """random actions with the interact bit set for half of the agents: objects are picked up and put down, `carrying` flips"""
    masks = np.array(action_masks(sample_actions(seed, step, n)), np.int64)
    rng = np.random.RandomState(seed * 1000 + step)
    return masks | np.where(rng.rand(n) < 0.5, 1 << 8, 0)   # (ACT_INTERACT)


@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 2), ("ObstaclesEasy", 1), ("Collect", 1)])
def test_pack_against_numpy_on_oracle_states(oracle, scenario, A):
    """1. the oracle rolled for 40 ticks, 4 envs: after every tick the host pack function, fed the struct images of every agent, gives the table's row, bit
    for bit; over the run `carrying` takes both values where the scenario has objects to carry"""
    N = 4
    og = oracle.OracleGym(scenario, 32, 32, N, A, 1, False, None)
    og.seed(42)
    og.reset()
    carried = set()
    for tick in range(41):
        for e in range(N):
            snap = og.snapshot(e)
            want = S.rows_of_snapshot(snap, A)
            for a in range(A):
                agent, header = S.struct_images(snap, a)
                got = extension.debug_state_obs_host(agent.tobytes(), header.tobytes())
                assert got.view(np.uint32).tolist() == want[a].tolist(), f"{scenario}, tick {tick}, env {e}, agent {a}: {got} vs {want[a].view(np.float32)}"
                carried.add(int(want[a][S.F["carrying"]]))
        masks = interact_heavy_masks(7, tick, N * A)
        for e in range(N):
            for a in range(A):
                og.set_action_mask(e, a, int(masks[e * A + a]))
        og.step_norender()
    og.close()
    if scenario == "TowerBuilding":
        assert carried == {0, 0x3f800000}, "carrying never flipped: the run does not exercise column 11"


def test_pack_moves_bits():
    """1. hand-made records: -0.0, NaNs with payloads, denormals and infinities pass through every copied column unchanged; column 11 is 1.0f / +0.0f by the
    sign of `carrying` alone; column 15 is +0.0f whatever the records hold"""
    specials = np.array([0x80000000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x00000000, 0x3f800000,
                         0xdeadbeef, 0x7fffffff, 0x00400000, 0xcafef00d, 0x12345678, 0xffffffff], np.uint32)
    for shift in range(16):
        words = np.roll(specials, shift)
        agent, header = np.zeros(1, S.AGENT_STATE), np.zeros(1, S.ENV_HEADER)
        agent.view(np.uint32)[:] = 0xa5a5a5a5   # (what the record does not copy must not leak into it)
        header.view(np.uint32)[:] = 0x5a5a5a5a
        au, hu = agent.view(np.uint32), header.view(np.uint32)
        au[0:11] = words[0:11]
        hu[S.ENV_HEADER.fields["episode_sec"][1] // 4] = words[12]
        hu[S.ENV_HEADER.fields["episode_len"][1] // 4] = words[13]
        au[S.AGENT_STATE.fields["total_reward"][1] // 4] = words[14]
        for carrying in (-1, 0, 3, -2 ** 31, 2 ** 31 - 1):
            agent["carrying"] = carrying
            got = extension.debug_state_obs_host(agent.tobytes(), header.tobytes()).view(np.uint32)
            want = words.copy()
            want[11] = 0x3f800000 if carrying >= 0 else 0
            want[15] = 0
            assert got.tolist() == want.tolist(), (shift, carrying)


def test_field_names():
    """2. STATE_OBS_FIELDS: 16 distinct names in the table's order, shared by MegaverseGym's module and MegaverseEnv"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    names = ["pos_x", "pos_y", "pos_z", "m00", "m02", "m20", "m22", "pitch", "hvx", "hvz", "vvel", "carrying", "episode_sec", "episode_len", "total_reward",
             "reserved"]
    assert list(extension.STATE_OBS_FIELDS) == names and len(set(names)) == 16
    assert [extension.STATE_OBS_FIELDS[n] for n in names] == list(range(16))
    assert MegaverseEnv.STATE_OBS_FIELDS is extension.STATE_OBS_FIELDS
    assert S.F == extension.STATE_OBS_FIELDS   # (the tests' restatement indexes the same columns)
    assert all(hasattr(MegaverseEnv, n) for n in ("state_obs",)) and all(hasattr(extension.MegaverseGym, n) for n in
                                                                          ("set_state_obs", "state_obs", "get_state_observation"))


def test_multitask_refuses_with_text():
    """3. MultiTaskGym.set_state_obs raises before it touches a device"""
    from megaverse_amd.multitask import MultiTaskGym
    for arg in (True, None):
        with pytest.raises(RuntimeError, match="mv_set_state_obs"):
            MultiTaskGym.set_state_obs(type("G", (), {"_group": None})(), arg)


def test_no_gym_is_an_error_with_text():
    """a null gym: -1 with text from the three calls that take one; null pointers to the host hook likewise"""
    lib = extension.load_library()
    out = np.zeros(16, np.float32)
    for fn, args in ((lib.mv_set_state_obs, (None,)), (lib.mv_get_state_obs, ()), (lib.mv_get_state_observation, (0, 0, out.ctypes.data))):
        assert fn(None, *args) == -1
        assert b"null gym" in lib.mv_last_error() and b"state_obs" in lib.mv_last_error()
    assert lib.mv_debug_state_obs_host(None, None, out.ctypes.data) == -1 and b"mv_debug_state_obs_host" in lib.mv_last_error()


class FakeTensor:
    """what check_state_obs asks of a tensor, with no device behind it"""

    def __init__(self, shape, dtype="torch.float32", is_cuda=True, contiguous=True, index=0):
        self.shape, self.dtype, self.is_cuda, self._contiguous, self.asked = shape, dtype, is_cuda, contiguous, 0
        self.device = type("D", (), {"index": index, "__str__": lambda s: f"cuda:{index}"})()

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        self.asked += 1
        return 0


class RaisingLib:
    """a library that answers the one question a well-formed tensor leads to (the ring count: none) and fails the test on every other call"""

    def __init__(self):
        self.asked = 0

    def mv_get_output_ring(self, g):
        self.asked += 1
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


@pytest.mark.parametrize("bad", [FakeTensor((1, 6, 15)), FakeTensor((2, 6, 16)), FakeTensor((6, 16)), FakeTensor((1, 6, 16), dtype="torch.float64"),
                                 FakeTensor((1, 6, 16), is_cuda=False), FakeTensor((1, 6, 16), contiguous=False), FakeTensor((1, 6, 16), index=1),
                                 np.zeros((1, 6, 16), np.float32)],
                         ids=["columns", "entries", "rank", "float64", "cpu", "strided", "other-device", "numpy"])
def test_tensor_is_checked_before_any_device_call(bad):
    """a wrong shape, dtype or device, a strided tensor, a host array: ValueError from MegaverseGym.set_state_obs itself, the library untouched"""
    gym = extension.MegaverseGym.__new__(extension.MegaverseGym)
    gym._lib, gym._g, gym.num_envs, gym.num_agents_per_env, gym.device, gym._state_obs = RaisingLib(), None, 3, 2, 0, "before"
    with pytest.raises(ValueError, match="set_state_obs"):
        gym.set_state_obs(bad)
    assert getattr(bad, "asked", 0) == 0 and gym._state_obs == "before"
    assert gym._lib.asked == (1 if getattr(bad, "shape", None) == (2, 6, 16) else 0)   # (only the entry count needs the gym's ring count)
    good = FakeTensor((4, 6, 16))
    assert extension.check_state_obs(good, 4, 6, 0) is good
