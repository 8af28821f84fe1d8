"""Step masks without a device: the ABI, the episode log's masked host twin (megaverse_amd/csrc/mv_episode_log.h: episode_log_steps, through
mv_debug_episode_log_masked_host) against numpy, the Python argument checks."""
import os
import re

import numpy as np
import pytest

import episode_log_util as U
from megaverse_amd import extension
from megaverse_amd.extension import check_step_mask, debug_episode_log_host, debug_episode_log_masked_host
from step_mask_util import MaskedModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    """3. the three calls and the masked log hook: declared in the header, exported by the library, bound with the declared arity"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_set_step_mask", 2), ("mv_set_step_mask_host", 2), ("mv_get_step_mask", 1), ("mv_debug_episode_log_masked_host", 14)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert len(bound["mv_debug_episode_log_host"][1]) == 13   # (the old hook's signature is what it was)
    assert lib.mv_abi_version() == 2   # (additive)


def test_no_gym_is_an_error_with_text():
    """3. a null gym: -1 with text, from all three"""
    lib = extension.load_library()
    mask = np.ones(4, np.uint8)
    for fn, args in ((lib.mv_set_step_mask, (mask.ctypes.data,)), (lib.mv_set_step_mask_host, (mask.ctypes.data,)), (lib.mv_set_step_mask, (None,)),
                     (lib.mv_set_step_mask_host, (None,)), (lib.mv_get_step_mask, ())):
        assert fn(None, *args) == -1
        assert b"null gym" in lib.mv_last_error() and b"mv_" in lib.mv_last_error()


def synthetic(seed, k, N, A):
    rng = np.random.default_rng(seed)
    rewards = (rng.standard_normal((k, N * A)) * (rng.random((k, N * A)) < 0.4)).astype(np.float32)
    dones = (rng.random((k, N)) < 0.15).astype(np.uint8)
    tobj = rng.standard_normal((k, N * A)).astype(np.float32)
    return rewards, dones, tobj


# (ticks of the call, its mask; None: no mask attached).  Env 1 is frozen in the second and third call after five ticks of an episode -- mid-episode, asserted
# below -- and thaws with another mask; the all-zero call freezes everybody; 255 and 7 are "any non-zero byte".
LEGS = [(5, None), (7, [1, 0, 1, 1, 0]), (4, [0, 0, 1, 0, 1]), (16, [0, 0, 0, 0, 0]), (9, [255, 7, 0, 1, 1]), (6, None), (11, [1, 1, 1, 1, 1])]


@pytest.mark.parametrize("A", [1, 3])
def test_masked_log_twin_against_numpy(A):
    """1. mv_debug_episode_log_masked_host over calls whose masks change from call to call (N = 5, A = 1 and 3: odd): random rewards and dones -- the frozen
    envs' too: none of them may count -- against the numpy model: records, count, ret and len byte for byte after every call"""
    N, cap = 5, 4096
    model, state, tick = MaskedModel(N, A), None, 0
    saw_mid_episode = False
    for j, (k, mask) in enumerate(LEGS):
        r, d, o = synthetic(50 + j, k, N, A)
        if j == 0:
            d[:, 1] = 0   # (env 1 is in the middle of an episode -- five ticks long -- when the next call freezes it)
        before = (model.ret.copy(), model.len.copy())
        model.feed(r, d, o, mask)
        state = debug_episode_log_masked_host(mask, r, d, o, A, cap, tick, state)
        tick += k
        assert state["ret"].tobytes() == model.ret.tobytes() and state["len"].tobytes() == model.len.tobytes(), f"call {j}"
        assert state["count"] == len(model.records), f"call {j}"
        if mask is not None:
            frozen = np.array(mask) == 0
            assert state["len"][frozen].tobytes() == before[1][frozen].tobytes()
            assert state["ret"].reshape(N, A)[frozen].tobytes() == before[0].reshape(N, A)[frozen].tobytes()
            saw_mid_episode = saw_mid_episode or bool((before[1][frozen] > 0).any() and before[0].reshape(N, A)[frozen].any())
    assert saw_mid_episode, "no env was frozen in the middle of an episode"
    assert model.tick == tick == sum(k for k, _ in LEGS)
    want = np.array(model.records, U.RECORD)
    assert state["count"] == len(want) > 10 and state["dropped"] == 0
    assert state["records"][:state["count"]].tobytes() == want.tobytes()
    # a record's length counts the ticks its env stepped, its end_tick the gym's ticks: env 1's first record spans the calls that froze it
    first = want[want["agent"] // A == 1][0]
    assert int(first["length"]) < int(first["end_tick"]) + 1
    # ... and the masks mattered: the same ticks without them leave another log
    plain = U.Model(N, A)
    for j, (k, _) in enumerate(LEGS):
        plain.feed(*synthetic(50 + j, k, N, A))
    assert np.array(plain.records, U.RECORD).tobytes() != want.tobytes()


@pytest.mark.parametrize("A", [1, 3])
def test_capacity_overflow_with_a_mask(A):
    """1. a log of 6 records: what does not fit is dropped and counted, with masks as without"""
    N, cap = 5, 6
    model, state, tick = MaskedModel(N, A, cap), None, 0
    for j, (k, mask) in enumerate(LEGS):
        r, d, o = synthetic(80 + j, k, N, A)
        model.feed(r, d, o, mask)
        state = debug_episode_log_masked_host(mask, r, d, o, A, cap, tick, state)
        tick += k
    assert state["count"] == cap == len(model.records) and state["dropped"] == model.dropped > 0
    assert state["records"].tobytes() == np.array(model.records, U.RECORD).tobytes()
    assert state["ret"].tobytes() == model.ret.tobytes() and state["len"].tobytes() == model.len.tobytes()


@pytest.mark.parametrize("A", [1, 3])
def test_null_mask_is_the_old_hook(A):
    """1. step_mask = NULL against mv_debug_episode_log_host: every output byte for byte, call after call; an all-ones mask too"""
    N, cap = 5, 12
    old = new = ones = None
    tick = 0
    for j in range(4):
        k = 7 + j
        r, d, o = synthetic(120 + j, k, N, A)
        old = debug_episode_log_host(r, d, o, A, cap, tick, old)
        new = debug_episode_log_masked_host(None, r, d, o, A, cap, tick, new)
        ones = debug_episode_log_masked_host(np.ones(N, np.uint8), r, d, o, A, cap, tick, ones)
        tick += k
        for other in (new, ones):
            for key in ("ret", "len", "records"):
                assert old[key].tobytes() == other[key].tobytes(), (j, key)
            assert (old["count"], old["dropped"]) == (other["count"], other["dropped"])
    assert old["dropped"] > 0 and old["count"] == cap


def test_mask_argument_check():
    """2. check_reset_mask's rules, and None"""
    assert check_step_mask(None, 3) is None
    m = check_step_mask([True, False, True], 3)
    assert m.dtype == np.uint8 and m.tolist() == [1, 0, 1] and m.flags.c_contiguous
    assert check_step_mask(np.array([0, 2, 255], np.uint8), 3).tolist() == [0, 1, 1]
    assert check_step_mask(np.zeros(3, np.bool_), 3).tolist() == [0, 0, 0]
    for bad in ([True, False], np.zeros((3, 1), np.bool_), np.zeros(3, np.int32), np.zeros(3, np.float32), [0.5, 0.0, 1.0], np.zeros(3, np.uint16)):
        with pytest.raises(ValueError, match="set_step_mask"):
            check_step_mask(bad, 3)


def test_an_object_with_only_a_data_ptr_is_a_value_error():
    """2. anything with data_ptr() takes the device branch: what is not a contiguous bool / uint8 CUDA tensor of the right shape is a ValueError"""
    class Bare:
        shape, dtype = (3,), "torch.bool"

        def data_ptr(self):
            return 0

    class NoShape:
        def data_ptr(self):
            return 0

    for bad in (Bare(), NoShape()):
        with pytest.raises(ValueError, match="set_step_mask"):
            check_step_mask(bad, 3)
