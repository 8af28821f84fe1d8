"""Env forks without a device: the ABI, the rule of a fork map (megaverse_amd/csrc/mv_fork.h through mv_debug_fork_plan_host), the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fork_util import MAP
from megaverse_amd import extension
from megaverse_amd.extension import check_fork_map, debug_fork_plan_host
from megaverse_amd.megaverse_env import MegaverseEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_fork_envs", 2), ("mv_fork_envs_host", 2), ("mv_debug_fork_plan_host", 4)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert lib.mv_abi_version() == 2   # (additive)


def plan(m):
    resolved, invalid = debug_fork_plan_host(m)
    return resolved.tolist(), invalid.tolist()


def test_identity_and_minus_one_leave_alone():
    assert plan([-1, 1, -1, 3]) == ([-1, -1, -1, -1], [0, 0, 0, 0])
    assert plan([0]) == ([-1], [0]) and plan([-1]) == ([-1], [0])


def test_shared_sources_resolve():
    """the map of the GPU tests: env 0 and the last env each serve two destinations, one entry points at itself"""
    assert MAP == [-1, 0, 0, 7, 4, 7, -1, -1]
    assert plan(MAP) == ([-1, 0, 0, 7, -1, 7, -1, -1], [0] * 8)
    # every env from env 0, and a source that names itself
    assert plan([0, 0, 0, 0, 0]) == ([-1, 0, 0, 0, 0], [0] * 5)
    assert plan([-1] + [0] * 1023)[0] == [-1] + [0] * 1023
    # odd envs from their even neighbour
    m = [-1 if d % 2 == 0 else d - 1 for d in range(64)]
    assert plan(m) == (m, [0] * 64)


def test_a_chain_of_two_is_invalid_in_every_entry_it_involves():
    # 2 <- 1 <- 0: env 1 would be written and read in the same launch
    assert plan([-1, 0, 1, -1]) == ([-1, -1, -1, -1], [0, 1, 1, 0])
    # ... wherever the chain's entries stand, and the valid entries beside it stay valid
    assert plan([-1, 2, 3, -1, 3, -1]) == ([-1, -1, -1, -1, 3, -1], [0, 1, 1, 0, 0, 0])
    assert plan([-1, 0, 1, -1, 8, 7, -1, -1]) == ([-1, -1, -1, -1, -1, 7, -1, -1], [0, 1, 1, 0, 1, 0, 0, 0])


def test_a_cycle_of_two_is_invalid_in_both_entries():
    assert plan([1, 0]) == ([-1, -1], [1, 1])
    assert plan([-1, 2, 1, 0]) == ([-1, -1, -1, 0], [0, 1, 1, 0])
    assert plan([1, 2, 0]) == ([-1, -1, -1], [1, 1, 1])


def test_indices_out_of_range_are_invalid():
    assert plan([4, -2, -1, 2 ** 31 - 1]) == ([-1, -1, -1, -1], [1, 1, 0, 1])
    assert plan([-(2 ** 31), 0]) == ([-1, -1], [1, 1])   # (entry 1's source is not left alone: what an invalid entry names stays untouched)
    assert plan([-1, 0, 3]) == ([-1, 0, -1], [0, 0, 1])


def test_plan_against_a_numpy_model():
    """random maps: valid <=> the source is in range and left alone itself, and nobody names the destination as a source"""
    rng = np.random.default_rng(5)
    for N in (1, 2, 3, 8, 33):
        for _ in range(40):
            m = rng.integers(-2, N + 1, N).astype(np.int32)
            resolved, invalid = debug_fork_plan_host(m)
            for d in range(N):
                s = int(m[d])
                if s == -1 or s == d:
                    want = (-1, 0)
                elif s < 0 or s >= N or not (m[s] == -1 or m[s] == s) or any(m[i] == d and i != d for i in range(N)):
                    want = (-1, 1)
                else:
                    want = (s, 0)
                assert (int(resolved[d]), int(invalid[d])) == want, (m.tolist(), d)
            # what the rule promises the kernel: no env is both read and written
            dst = {d for d in range(N) if resolved[d] >= 0}
            assert dst.isdisjoint({int(resolved[d]) for d in dst})


def test_null_gym_and_null_map_are_errors_not_crashes():
    lib = extension.load_library()
    m = (C.c_int32 * 4)(-1, 0, -1, -1)
    for fn in (lib.mv_fork_envs, lib.mv_fork_envs_host):
        assert fn(None, m) < 0 and b"null gym" in lib.mv_last_error()
        assert fn(None, None) < 0 and lib.mv_last_error()
    out = (C.c_int32 * 4)()
    assert lib.mv_debug_fork_plan_host(None, 4, out, out) < 0 and b"null" in lib.mv_last_error()
    assert lib.mv_debug_fork_plan_host(m, 4, None, out) < 0 and lib.mv_debug_fork_plan_host(m, 4, out, None) < 0
    assert lib.mv_debug_fork_plan_host(m, -1, out, out) < 0


def test_python_argument_checks():
    assert check_fork_map(MAP, 8).dtype == np.int32 and check_fork_map(np.array(MAP, np.int64), 8).tolist() == MAP
    for bad in (MAP[:7], [MAP], np.zeros((8, 1), np.int32)):
        with pytest.raises(ValueError, match="8 integers"):
            check_fork_map(bad, 8)
    with pytest.raises(ValueError, match="integers"):
        check_fork_map(np.zeros(8, np.float32), 8)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="int32 CUDA tensor"):
        check_fork_map(torch.zeros(8, dtype=torch.int32), 8)   # a host tensor
    with pytest.raises(ValueError, match="int32 CUDA tensor"):
        check_fork_map(torch.zeros(8, dtype=torch.int64), 8)


class _Recorder:
    def __init__(self):
        self.maps = []

    def fork_envs(self, m):
        self.maps.append(np.asarray(m).tolist())


def test_env_fork_builds_the_map():
    env = object.__new__(MegaverseEnv)   # (the map is built before anything touches the gym)
    env.num_envs, env.env = 6, _Recorder()
    env.fork(2)
    env.fork(0, [1, 5])
    env.fork(3, [3, 4])   # the source among its destinations: left alone
    env.fork(1, [])
    assert env.env.maps == [[2, 2, -1, 2, 2, 2], [-1, 0, -1, -1, -1, 0], [-1, -1, -1, -1, 3, -1], [-1] * 6]
    for src, dst in ((6, None), (-1, None), (0, [6]), (0, [-1])):
        with pytest.raises(ValueError):
            env.fork(src, dst)
