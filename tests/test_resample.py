"""Env resampling without a device: the ABI, the rule of a resampling map and its two phases (megaverse_amd/csrc/mv_fork.h through
mv_debug_resample_plan_host and mv_debug_resample_apply_host), the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fork_util import MAP, columns
from megaverse_amd import extension
from megaverse_amd.extension import check_fork_map, debug_resample_apply_host, debug_resample_plan_host
from megaverse_amd.megaverse_env import MegaverseEnv
from resample_util import DRAW, DRAW_COLS, DRAW_STAGED, PERM, PERM_COLS, PERM_STAGED, compose, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity, res in (("mv_resample_envs", 2, "int"), ("mv_resample_envs_host", 2, "int"), ("mv_resample_staging_bytes", 1, "int64_t"),
                             ("mv_debug_resample_plan_host", 5, "int"), ("mv_debug_resample_apply_host", 5, "int")):
        assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert bound["mv_resample_staging_bytes"][0] is C.c_int64
    assert lib.mv_abi_version() == 2   # (additive)


def plan(m):
    return tuple(x.tolist() for x in debug_resample_plan_host(m))


def flags(envs, n=8):
    return [int(e in envs) for e in range(n)]


def test_the_plans_of_the_test_maps_by_hand():
    assert plan(PERM) == ([1, 0, 3, 4, 2, 7, -1, 6], flags(PERM_STAGED), [0] * 8)
    assert [s if s >= 0 else e for e, s in enumerate(plan(PERM)[0])] == PERM_COLS
    # the two entries that name themselves are left alone
    assert plan(DRAW) == ([3, 3, 3, 0, -1, 0, -1, 0], flags(DRAW_STAGED), [0] * 8)
    assert [s if s >= 0 else e for e, s in enumerate(plan(DRAW)[0])] == DRAW_COLS
    # a fork map stages nobody: no source is a destination
    assert plan(MAP) == ([-1, 0, 0, 7, -1, 7, -1, -1], [0] * 8, [0] * 8)
    assert compose(PERM, DRAW) == [4, 4, 4, 1, 2, 1, 6, 1]


def test_chains_swaps_and_cycles_are_valid():
    assert plan([1, 0]) == ([1, 0], [1, 1], [0, 0])
    assert plan([1, 2, 0]) == ([1, 2, 0], [1, 1, 1], [0, 0, 0])
    # 2 <- 1 <- 0: env 1 is read and written, so it is staged; env 2 is written only, env 0 read only
    assert plan([-1, 0, 1, -1]) == ([-1, 0, 1, -1], [0, 1, 0, 0], [0] * 4)
    assert plan([-1, 1, -1, 3]) == ([-1] * 4, [0] * 4, [0] * 4) and plan([0]) == ([-1], [0], [0]) and plan([-1]) == ([-1], [0], [0])
    # a full rotation stages everybody
    n = 64
    assert plan([(d + 1) % n for d in range(n)]) == ([(d + 1) % n for d in range(n)], [1] * n, [0] * n)


def test_indices_out_of_range_are_invalid_and_name_nobody():
    assert plan([4, -2, -1, 2 ** 31 - 1]) == ([-1] * 4, [0] * 4, [1, 1, 0, 1])
    # entry 0 is skipped; entry 1 names the skipped env 0 and stays valid; env 0 is not staged (it is not written)
    assert plan([-(2 ** 31), 0]) == ([-1, 0], [0, 0], [1, 0])
    # the GPU test's map: 3 <- 2 and 6 <- 5 stay valid although entries 2 and 5 are skipped, and the swap is staged
    assert plan([1, 0, 8, 2, -1, -5, 5, -1]) == ([1, 0, -1, 2, -1, -1, 5, -1], [1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 1, 0, 0])
    # an invalid entry's value equals nobody's index, so nobody is staged because of it: env 1 is named by the invalid entry 0 only if N were larger
    assert plan([3, 2, -1]) == ([-1, 2, -1], [0, 0, 0], [1, 0, 0])


RANDOM_SIZES = (1, 2, 3, 8, 33, 257)


def test_plan_against_a_numpy_model():
    rng = np.random.default_rng(5)
    for N in RANDOM_SIZES:
        for _ in range(20):
            m = rng.integers(-2, N + 1, N).astype(np.int32)
            assert plan(m) == model(m.tolist()), m.tolist()


def test_apply_equals_a_gather_of_the_old_state_in_every_order():
    rng = np.random.default_rng(6)
    maps = [np.array(PERM, np.int32), np.array(DRAW, np.int32), np.array(MAP, np.int32)]
    for N in RANDOM_SIZES:
        maps += [rng.integers(-2, N + 1, N).astype(np.int32) for _ in range(10)]
        maps.append(rng.permutation(N).astype(np.int32))
    for m in maps:
        N = m.size
        old = rng.integers(0, 256, (N, 48)).astype(np.uint8)
        resolved, staged, invalid = model(m.tolist())
        cols = np.array([s if s >= 0 else e for e, s in enumerate(resolved)])
        want = old[cols]
        for order in (0, 1, 2):
            got = debug_resample_apply_host(m, old, order)
            assert got.tobytes() == want.tobytes(), (m.tolist(), order)
        skipped = np.flatnonzero(invalid)
        assert want[skipped].tobytes() == old[skipped].tobytes()
    assert debug_resample_apply_host(PERM, np.arange(8, dtype=np.uint8).reshape(8, 1)).reshape(-1).tolist() == PERM_COLS


def test_null_arguments_are_errors_not_crashes():
    lib = extension.load_library()
    m = (C.c_int32 * 4)(1, 0, -1, -1)
    for fn in (lib.mv_resample_envs, lib.mv_resample_envs_host):
        assert fn(None, m) < 0 and b"null gym" in lib.mv_last_error()
        assert fn(None, None) < 0 and lib.mv_last_error()
    assert lib.mv_resample_staging_bytes(None) == -1
    out = (C.c_int32 * 4)()
    assert lib.mv_debug_resample_plan_host(None, 4, out, out, out) < 0 and b"null" in lib.mv_last_error()
    assert lib.mv_debug_resample_plan_host(m, 4, None, out, out) < 0 and lib.mv_debug_resample_plan_host(m, 4, out, None, out) < 0
    assert lib.mv_debug_resample_plan_host(m, 4, out, out, None) < 0 and lib.mv_debug_resample_plan_host(m, -1, out, out, out) < 0
    state = (C.c_uint8 * 16)()
    assert lib.mv_debug_resample_apply_host(None, 4, 4, state, 0) < 0 and b"null" in lib.mv_last_error()
    assert lib.mv_debug_resample_apply_host(m, 4, 4, None, 0) < 0 and lib.mv_debug_resample_apply_host(m, -1, 4, state, 0) < 0
    assert lib.mv_debug_resample_apply_host(m, 4, -1, state, 0) < 0
    assert lib.mv_debug_resample_apply_host(m, 4, 4, state, 3) < 0 and b"order" in lib.mv_last_error()
    assert lib.mv_debug_resample_apply_host(m, 4, 4, state, 0) == 0


def test_python_argument_checks():
    """resample_envs takes its argument through fork_envs' check"""
    assert check_fork_map(PERM, 8).dtype == np.int32 and check_fork_map(np.array(DRAW, np.int64), 8).tolist() == DRAW
    for bad in (PERM[:7], [PERM], np.zeros((8, 1), np.int32)):
        with pytest.raises(ValueError, match="8 integers"):
            check_fork_map(bad, 8)
    with pytest.raises(ValueError, match="uint8"):
        debug_resample_apply_host(PERM, np.zeros((8, 4), np.int32))
    with pytest.raises(ValueError, match="uint8"):
        debug_resample_apply_host(PERM, np.zeros((7, 4), np.uint8))

    class Gym:   # MegaverseGym.resample_envs on an object that records what reaches the library
        num_envs, calls = 8, []
        _fork_held = None
        resample_envs = extension.MegaverseGym.resample_envs

        class _lib:
            mv_resample_envs_host = staticmethod(lambda g, p: Gym.calls.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (8,)).tolist()) or 0)
        _g = None
        _ck = staticmethod(lambda rc: rc)
    g = Gym()
    g.resample_envs(PERM)
    g.resample_envs(np.array(DRAW, np.int64))
    assert Gym.calls == [PERM, DRAW]
    for bad in (PERM[:7], np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            g.resample_envs(bad)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="int32 CUDA tensor"):
        g.resample_envs(torch.zeros(8, dtype=torch.int32))   # a host tensor


class _Recorder:
    def __init__(self):
        self.maps = []

    def resample_envs(self, m):
        self.maps.append(np.asarray(m).tolist())


def test_env_resample_and_swap_build_the_map():
    env = object.__new__(MegaverseEnv)   # (the map is built before anything touches the gym)
    env.num_envs, env.env = 6, _Recorder()
    env.resample([1, 0, 3, 4, 2, -1])
    env.swap(0, 5)
    env.swap(4, 2)
    env.swap(3, 3)
    assert env.env.maps == [[1, 0, 3, 4, 2, -1], [5, -1, -1, -1, -1, 0], [-1, -1, 4, -1, 2, -1], [-1, -1, -1, 3, -1, -1]]
    assert columns(env.env.maps[3]) == list(range(6))   # an env swapped with itself is left alone
    for a, b in ((6, 0), (0, 6), (-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            env.swap(a, b)
