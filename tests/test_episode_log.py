"""CPU: the episode log's per-tick body (megaverse_amd/csrc/mv_episode_log.h -- the source the kernel runs, compiled for the host behind
mv_debug_episode_log_host) against the bookkeeping done in numpy float64 (tests/episode_log_util.py: Model) on the CPU oracle's outputs; the record's
layout; the new symbols; argument errors.  No GPU involved."""
import ctypes as C

import numpy as np
import pytest

import episode_log_util as U


def host_log(name, chunk, capacity=1 << 16):
    import megaverse_amd.extension as ext
    _, N, A, _, ticks, *_ = U.ROLLOUTS[name]
    rewards, dones, tobj = U.rollout(name)
    state = None
    for t0 in range(0, ticks, chunk):
        state = ext.debug_episode_log_host(rewards[t0:t0 + chunk], dones[t0:t0 + chunk], tobj[t0:t0 + chunk], A, capacity, first_tick=t0, state=state)
    return state


@pytest.mark.parametrize("chunk", [1, 7, 16])
@pytest.mark.parametrize("name", sorted(U.ROLLOUTS))
def test_host_twin_equals_the_numpy_model(name, chunk):
    want = U.expected_log(name)
    records = want.drain()
    U.assert_floors(name, records)
    got = host_log(name, chunk)
    assert got["count"] == len(records) and got["dropped"] == 0
    assert got["records"][:got["count"]].tobytes() == records.tobytes()
    assert got["ret"].tobytes() == want.ret.tobytes() and got["len"].tobytes() == want.len.tobytes()


def test_records_are_in_end_tick_agent_order():
    got = host_log("tower_short", 7)
    records = got["records"][:got["count"]]
    assert len(records) >= 1500
    key = records["end_tick"].astype(np.int64) * (1 << 20) + records["agent"]
    assert (np.diff(key) > 0).all()


@pytest.mark.parametrize("chunk", [1, 16])
def test_capacity_keeps_the_first_records_and_counts_the_rest(chunk):
    full = U.expected_log("tower_short")
    records = full.drain()
    U.assert_floors("tower_short", records)
    got = host_log("tower_short", chunk, capacity=64)
    assert got["count"] == 64 and got["dropped"] == len(records) - 64
    assert got["records"].tobytes() == records[:64].tobytes()
    assert got["ret"].tobytes() == full.ret.tobytes() and got["len"].tobytes() == full.len.tobytes()   # accumulators are reset all the same
    bounded = U.expected_log("tower_short", capacity=64)
    assert bounded.dropped == got["dropped"] and bounded.drain().tobytes() == records[:64].tobytes()


def test_record_dtype():
    import megaverse_amd.extension as ext
    dt = ext.EPISODE_RECORD_DTYPE
    assert dt.itemsize == 24
    assert [(n, dt.fields[n][1], dt.fields[n][0]) for n in dt.names] == [
        ("agent", 0, np.dtype("<i4")), ("length", 4, np.dtype("<i4")), ("end_tick", 8, np.dtype("<u4")), ("true_objective", 12, np.dtype("<f4")),
        ("ret", 16, np.dtype("<f8"))]
    assert U.RECORD.itemsize == 24 and [U.RECORD.fields[n][1] for n in U.RECORD.names] == [0, 4, 8, 12, 16]


def test_symbols_resolve():
    import megaverse_amd.extension as ext
    lib = ext.load_library()
    bound = {n for n, _, _ in ext.SYMBOLS}
    for n in ("mv_set_episode_log", "mv_get_episode_log_capacity", "mv_flush_episode_log", "mv_episode_log_count", "mv_drain_episode_log",
              "mv_episode_log_records_device_ptr", "mv_episode_log_count_device_ptr", "mv_episode_returns_device_ptr", "mv_episode_lengths_device_ptr",
              "mv_ticks_since_reset", "mv_debug_episode_log_host"):
        assert hasattr(lib, n) and n in bound, n


def test_argument_errors():
    import megaverse_amd.extension as ext
    lib = ext.load_library()
    count, dropped = C.c_uint32(), C.c_uint32()
    assert lib.mv_set_episode_log(None, 16) < 0 and b"null gym" in lib.mv_last_error()
    assert lib.mv_set_episode_log(None, -1) < 0 and b"capacity >= 0" in lib.mv_last_error()
    assert lib.mv_flush_episode_log(None) < 0
    assert lib.mv_episode_log_count(None, C.byref(count), C.byref(dropped)) < 0
    assert lib.mv_drain_episode_log(None, None, 0, C.byref(dropped)) < 0
    assert lib.mv_drain_episode_log(None, None, -1, C.byref(dropped)) < 0 and b"max_records" in lib.mv_last_error()
    assert lib.mv_get_episode_log_capacity(None) == -1 and lib.mv_ticks_since_reset(None) == -1
    assert lib.mv_episode_returns_device_ptr(None) is None and lib.mv_episode_log_records_device_ptr(None) is None
    one = np.zeros((1, 1), np.float32)
    with pytest.raises(RuntimeError, match="bad arguments"):
        ext.debug_episode_log_host(one, np.zeros((1, 1), np.uint8), one, 1, 0)
    with pytest.raises(ValueError):
        ext.debug_episode_log_host(np.zeros((1, 3), np.float32), np.zeros((1, 1), np.uint8), one, 1, 4)
