"""Action rings without a device: the ABI, the policy table, the Python argument checks, the split of a batch's actions over its sub-gyms, the index rule."""
import os
import re

import numpy as np
import pytest

from action_ring_util import CALLS, TICKS, make_script
from megaverse_amd import extension
from megaverse_amd.megaverse_env import MegaverseEnv, check_sequence_actions
from megaverse_amd.multitask import MultiTaskGym, check_action_ring, split_action_ring
from megaverse_amd.rollout import action_ring_entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name in ("mv_set_action_ring", "mv_debug_launch_counts"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == (3 if name == "mv_set_action_ring" else 2)
    assert re.search(r"\bMV_POLICY_SEQUENCE\s*=\s*3\b", text)
    assert lib.mv_abi_version() == 2


def test_policy_table():
    assert extension.MegaverseGym.POLICIES["sequence"] == 3
    assert {k: v for k, v in extension.MegaverseGym.POLICIES.items() if k != "sequence"} == {"none": 0, "multidiscrete": 1, "single-bit": 2}


def test_null_gym_is_an_error_not_a_crash():
    lib = extension.load_library()
    assert lib.mv_set_action_ring(None, 1, None) < 0 and lib.mv_last_error()
    assert lib.mv_debug_launch_counts(None, None) < 0


def test_index_rule_in_uint32():
    """(first + j) % count with the sum taken in uint32: against numpy's wrapping arithmetic, across the wrap and for counts that do not divide 2^32"""
    rng = np.random.default_rng(0)
    firsts = np.concatenate([np.array([0, 3, 2 ** 32 - 4, 2 ** 32 - 1, 2 ** 31 - 1, 2 ** 31], np.uint64), rng.integers(0, 2 ** 32, 64, dtype=np.uint64)])
    for count in (1, 2, 5, 7, 16, 96, 1000003):
        for first in firsts:
            j = np.arange(20, dtype=np.uint32)
            want = (np.uint32(first) + j) % np.uint32(count)   # (array arithmetic wraps)
            got = [action_ring_entry(int(first), int(q), count) for q in j]
            assert got == want.tolist(), (first, count)
    assert [action_ring_entry(2 ** 32 - 4, q, 5) for q in range(8)] == [2, 3, 4, 0, 0, 1, 2, 3]   # 2^32 - 4 = 2 (mod 5); the sum wraps to 0 at j = 4
    assert [action_ring_entry(3, q, 5) for q in range(8)] == [3, 4, 0, 1, 2, 3, 4, 0]
    assert all(action_ring_entry(f, q, 1) == 0 for f in (0, 77, 2 ** 32 - 1) for q in range(4))


def test_split_follows_locate():
    """MultiTaskGym.set_action_ring's split == a numpy model of locate: global env i is local env i // S of sub-gym i % S"""
    for S, per_task, A, count in ((3, 4, 1, 8), (2, 5, 3, 4), (8, 2, 2, 3)):
        NE = S * per_task
        acts = np.arange(count * NE * A * 6, dtype=np.int32).reshape(count, NE * A, 6)
        parts = split_action_ring(acts, S, A)
        mt = object.__new__(MultiTaskGym)   # (locate needs the list of sub-gyms only)
        mt.gyms = list(range(S))
        assert len(parts) == S
        for k, p in enumerate(parts):
            assert p.shape == (count, per_task * A, 6)
        for i in range(NE):
            k, j = mt.locate(i)
            for a in range(A):
                assert np.array_equal(parts[k][:, j * A + a], acts[:, i * A + a]), (S, A, i, a)


def test_multitask_argument_checks():
    ok = np.zeros((4, 12, 6), np.int32)
    assert check_action_ring(ok, 12, 1) == 4 and check_action_ring(ok, 6, 2) == 4
    for bad in (np.zeros((4, 12), np.int32), np.zeros((4, 11, 6), np.int32), np.zeros((4, 12, 5), np.int32), np.zeros((0, 12, 6), np.int32)):
        with pytest.raises(ValueError, match="count >= 1"):
            check_action_ring(bad, 12, 1)
    for dt in (np.int64, np.float32, np.uint8):
        with pytest.raises(ValueError, match="int32"):
            check_action_ring(ok.astype(dt), 12, 1)
    mt = object.__new__(MultiTaskGym)   # (the check comes before anything touches a gym)
    mt.num_envs, mt.num_agents_per_env, mt.gyms = 12, 1, []
    with pytest.raises(ValueError):
        mt.set_action_ring(np.zeros((4, 13, 6), np.int32))


def test_step_sequence_argument_checks():
    assert check_sequence_actions(np.zeros((20, 8, 6), np.int32), 8) == 20
    assert check_sequence_actions(np.zeros((1, 8, 6), np.int64), 8) == 1
    assert check_sequence_actions([[[0] * 6] * 2] * 3, 2) == 3
    for bad in (np.zeros((20, 8), np.int32), np.zeros((20, 7, 6), np.int32), np.zeros((0, 8, 6), np.int32), np.zeros((20, 8, 7), np.int32)):
        with pytest.raises(ValueError, match="num_agents = 8"):
            check_sequence_actions(bad, 8)
    with pytest.raises(ValueError, match="integers"):
        check_sequence_actions(np.zeros((2, 8, 6), np.float32), 8)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="int32 and on the device"):
        check_sequence_actions(torch.zeros((2, 8, 6), dtype=torch.int32), 8)   # a host tensor
    with pytest.raises(ValueError, match="num_agents = 8"):
        check_sequence_actions(torch.zeros((2, 9, 6), dtype=torch.int32), 8)
    env = object.__new__(MegaverseEnv)   # (the check comes before anything touches the gym)
    env.num_agents = 8
    with pytest.raises(ValueError):
        env.step_sequence(np.zeros((2, 8, 5), np.int32))


def test_scripts_are_biased_and_reproducible():
    """the scripts the GPU tests replay: fixed by their seed, within the action space, forward and interact dominating -- not a uniform draw"""
    a, b = make_script(3, TICKS, 12), make_script(3, TICKS, 12)
    assert np.array_equal(a, b) and a.dtype == np.int32 and a.shape == (TICKS, 12, 6) and sum(CALLS) == TICKS
    assert (a >= 0).all() and (a < np.array([3, 3, 3, 2, 2, 3])).all()
    assert (a[..., 1] == 1).mean() > 0.5 and (a[..., 1] == 2).mean() < 0.1    # a uniform draw walks forward a third of the time
    assert (a[..., 4] == 1).mean() > 0.2
    turn = a[:, 0, 2]
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[-1], turn, [-1]])) != 0))
    assert runs.max() >= 6   # long turn or straight runs
