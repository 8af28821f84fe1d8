"""Masked env resets without a device: the ABI, the episode log's masked clear (megaverse_amd/csrc/mv_episode_log.h: episode_log_cut, through
mv_debug_episode_log_cut_host) against numpy, the Python argument checks."""
import os
import re

import numpy as np
import pytest

import episode_log_util as U
from megaverse_amd import extension
from megaverse_amd.extension import check_reset_mask, debug_episode_log_cut_host, debug_episode_log_host
from reset_envs_util import CutModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_reset_envs", 3), ("mv_reset_envs_host", 3), ("mv_debug_episode_log_cut_host", 5)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert lib.mv_abi_version() == 2   # (additive)


def test_no_gym_is_an_error_with_text():
    lib = extension.load_library()
    mask = np.ones(4, np.uint8)
    for fn in (lib.mv_reset_envs, lib.mv_reset_envs_host):
        assert fn(None, mask.ctypes.data, 1) == -1
        assert b"null gym" in lib.mv_last_error()
    ret, length = np.ones(4), np.ones(4, np.int32)
    assert lib.mv_debug_episode_log_cut_host(None, 4, 1, ret.ctypes.data, length.ctypes.data) == -1
    assert b"mv_debug_episode_log_cut_host" in lib.mv_last_error()
    assert ret.tolist() == [1.0] * 4 and length.tolist() == [1] * 4


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("mask", [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 1, 0, 0, 1], [7, 0, 0, 255, 0]], ids=["zeros", "ones", "mixed", "any_non_zero_byte"])
def test_cut_against_numpy(A, mask):
    """N = 5 (odd), A = 1 and 3 (odd): a flagged env's A returns and its length read zero, every other value keeps its bits"""
    N = 5
    rng = np.random.default_rng(100 + A)
    ret = rng.standard_normal(N * A) * 10.0
    length = rng.integers(1, 500, N).astype(np.int32)
    want_ret, want_len = ret.copy(), length.copy()
    m = np.array(mask, np.uint8) != 0
    want_ret[np.repeat(m, A)] = 0.0
    want_len[m] = 0
    lib = extension.load_library()
    raw = np.array(mask, np.uint8)
    assert lib.mv_debug_episode_log_cut_host(raw.ctypes.data, N, A, ret.ctypes.data, length.ctypes.data) == 0
    assert ret.tobytes() == want_ret.tobytes() and length.tobytes() == want_len.tobytes()
    if m.all():
        assert not ret.any() and not length.any()


def synthetic(seed, k, N, A):
    rng = np.random.default_rng(seed)
    rewards = (rng.standard_normal((k, N * A)) * (rng.random((k, N * A)) < 0.4)).astype(np.float32)
    dones = (rng.random((k, N)) < 0.15).astype(np.uint8)
    tobj = rng.standard_normal((k, N * A)).astype(np.float32)
    return rewards, dones, tobj


@pytest.mark.parametrize("A", [1, 3])
def test_tick_body_cut_tick_body(A):
    """mv_debug_episode_log_host over 9 ticks, the cut, 11 more ticks, a second cut with another mask, 6 more: records, count, ret and len against the
    numpy model (episode_log_util.Model + 'a flagged env's accumulators go to zero and it writes no record'), byte for byte"""
    N, cap = 5, 4096
    legs = [(9, [1, 0, 0, 1, 0]), (11, [0, 1, 1, 1, 0]), (6, None)]
    model, state, tick = CutModel(N, A), None, 0
    for j, (k, mask) in enumerate(legs):
        r, d, o = synthetic(7 + j, k, N, A)
        assert d.any()
        model.feed(r, d, o)
        state = debug_episode_log_host(r, d, o, A, cap, tick, state)
        tick += k
        if mask is not None:
            count = state["count"]
            running = state["ret"].copy()
            assert running[np.repeat(np.array(mask, bool), A)].any(), "the cut would clear nothing"
            model.cut(mask)
            debug_episode_log_cut_host(mask, A, state["ret"], state["len"])
            assert state["count"] == count   # (a cut writes no record: nothing of the log but the accumulators is handed to it)
        assert state["ret"].tobytes() == model.ret.tobytes() and state["len"].tobytes() == model.len.tobytes(), f"leg {j}"
    want = np.array(model.records, U.RECORD)
    assert state["count"] == len(want) > 10 and state["dropped"] == 0
    assert state["records"][:state["count"]].tobytes() == want.tobytes()
    # ... and the cuts mattered: the same ticks without them leave another log
    plain = U.Model(N, A)
    for j, (k, _) in enumerate(legs):
        plain.feed(*synthetic(7 + j, k, N, A))
    assert np.array(plain.records, U.RECORD).tobytes() != want.tobytes()


def test_mask_argument_check():
    m = check_reset_mask([True, False, True], 3)
    assert m.dtype == np.uint8 and m.tolist() == [1, 0, 1] and m.flags.c_contiguous
    assert check_reset_mask(np.array([0, 2, 255], np.uint8), 3).tolist() == [0, 1, 1]
    assert check_reset_mask(np.zeros(3, np.bool_), 3).tolist() == [0, 0, 0]
    for bad in ([True, False], np.zeros((3, 1), np.bool_), np.zeros(3, np.int32), np.zeros(3, np.float32), [0.5, 0.0, 1.0]):
        with pytest.raises(ValueError, match="reset_envs"):
            check_reset_mask(bad, 3)


def test_an_object_with_only_a_data_ptr_is_a_value_error():
    """anything with data_ptr() takes the device branch: what is not a contiguous bool / uint8 CUDA tensor of the right shape is a ValueError, whatever
    attributes it lacks"""
    class Bare:
        shape, dtype = (3,), "torch.bool"

        def data_ptr(self):
            return 0

    class NoShape:
        def data_ptr(self):
            return 0

    for bad in (Bare(), NoShape()):
        with pytest.raises(ValueError, match="reset_envs"):
            check_reset_mask(bad, 3)

