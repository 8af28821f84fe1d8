"""Macro steps on the CPU (include/megaverse_hip.h: mv_macro_step): the header and the bindings, the rule's and the fold's host twins against their numpy
restatements (tests/macro_step_util.py), the episode log's update with the mirror of the ticks left against the numpy model, and the Python defaults."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import macro_step_util as M
from megaverse_amd import extension as ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)


def test_header_binding_and_abi_version():
    text = header()
    for name, args in (("mv_macro_step", 5), ("mv_macro_step_host", 5), ("mv_debug_macro_rule_host", 9), ("mv_debug_macro_fold_host", 4)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == args, f"{name}: {m.group(1)}"
        bound = [s for s in ext.SYMBOLS if s[0] == name]
        assert len(bound) == 1 and len(bound[0][2]) == args and bound[0][1] is C.c_int, name
    lib = ext.load_library()
    assert lib.mv_abi_version() == 2
    rule_h = open(os.path.join(ROOT, "megaverse_amd", "csrc", "mv_macro_step.h")).read()
    assert "__host__ __device__" in rule_h and "macro_steps" in rule_h and "macro_after_tick" in rule_h and "macro_fold" in rule_h
    # no gym: -1 with a text that names the call, no crash
    a = np.zeros((1, 6), np.int32)
    assert lib.mv_macro_step(None, 4, a.ctypes.data, None, 1) == -1 and b"mv_macro_step" in lib.mv_last_error()
    assert lib.mv_macro_step_host(None, 4, a.ctypes.data, None, 1) == -1 and b"mv_macro_step_host" in lib.mv_last_error()
    pyb = open(os.path.join(ROOT, "megaverse_amd", "pybind", "megaverse_module.cpp")).read()
    assert '.def("macro_step"' in pyb and "mv_macro_step_host" in pyb


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------------
def check_rule(dones, mask, left, ticks):
    steps, left_out, tl_out = ext.debug_macro_rule_host(dones, mask, left, ticks)
    want_steps, want_left, want_tl = M.rule(dones, mask, left, ticks)
    assert steps.astype(bool).tolist() == want_steps.tolist()
    assert left_out.tolist() == want_left.tolist() and tl_out.tolist() == want_tl.tolist()
    return want_steps, want_left, want_tl


def test_rule_hand_written_cases():
    k = 5
    # env:          0      1      2        3         4          5            6           7          8          9
    # done on:      first  last   middle   never     never      middle       first       first      first      middle
    # ticks:        k      k      k        0         k + 7      2 (< done)   k           k          k          k
    # mask:         1      1      1        1         1          1            0 (frozen)  1          1          1
    # budget:       -1     -1     -1       -1        -1         -1           -1          0          1          2
    dones = np.zeros((k, 10), np.uint8)
    dones[0, [0, 6, 7, 8]] = 1
    dones[k - 1, 1] = 1
    dones[2, [2, 5, 9]] = 1
    ticks = np.array([k, k, k, 0, k + 7, 2, k, k, k, k], np.int32)
    mask = np.ones(10, np.uint8)
    mask[6] = 0
    left = np.array([-1, -1, -1, -1, -1, -1, -1, 0, 1, 2], np.int32)
    steps, left_out, tl = check_rule(dones, mask, left, ticks)
    assert steps.sum(axis=0).tolist() == [1, k, 3, 0, k, 2, 0, 0, 1, 3]
    assert tl.tolist() == [0, 0, 0, 0, 0, 0, k, k, 0, 0]          # (a frozen or halted env keeps its ticks; a clamped one had k)
    assert left_out.tolist() == [-1, -1, -1, -1, -1, -1, -1, 0, 0, 1]
    # no ticks given: every env gets k; no mask
    check_rule(dones, None, left, None)
    # negative ticks clamp to 0; a budget of 2 spent over two calls' worth of dones in one call cannot happen: the first done ends the macro step
    d2 = np.ones((4, 3), np.uint8)
    steps, left_out, tl = check_rule(d2, None, [2, 2, -1], [-3, 4, 9])
    assert steps.sum(axis=0).tolist() == [0, 1, 1] and left_out.tolist() == [2, 1, -1] and tl.tolist() == [0, 0, 0]


@pytest.mark.parametrize("seed", range(6))
def test_rule_random_cases(seed):
    rng = np.random.default_rng(seed)
    k, n = int(rng.integers(1, 18)), int(rng.integers(1, 40))
    dones = (rng.random((k, n)) < 0.15).astype(np.uint8) * rng.integers(1, 255, (k, n)).astype(np.uint8)   # (any non-zero byte is a done)
    mask = None if seed % 3 == 0 else (rng.random(n) < 0.8).astype(np.uint8) * 7
    left = None if seed % 2 == 0 else rng.integers(-1, 3, n).astype(np.int32)
    ticks = None if seed == 1 else rng.integers(-2, k + 6, n).astype(np.int32)
    check_rule(dones, mask, left, ticks)


# ---- the fold ----------------------------------------------------------------------------------------------------------------------------------------
def test_fold_is_the_left_fold_bit_for_bit():
    cols = np.array([[1e8, 1.0, -1e8, 1.0],            # left fold: 1.0; pairwise: 0.0; reversed: 0.0
                     [-0.0, -0.0, -0.0, -0.0],         # stays -0.0: the first value is taken, not added to zero
                     [-0.0, 0.0, -0.0, -0.0],          # +0.0
                     [1.0, 2 ** -24, 2 ** -24, 2 ** -24],   # 1.0: each addend is half an ulp and rounds to even; summed first they would count
                     [0.1, 0.2, 0.3, 0.4],
                     [3.0, -3.0, 1e-30, 0.0]], np.float32).T.copy()
    got = ext.debug_macro_fold_host(cols)
    want = M.fold(cols)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert got[0] == 1.0 and np.signbit(got[1]) and got[1] == 0 and not np.signbit(got[2]) and got[3] == 1.0
    pairwise = (cols[0] + cols[1]).astype(np.float32) + (cols[2] + cols[3]).astype(np.float32)
    assert pairwise[0] != got[0] and pairwise[3] != got[3], "the cases do not tell the orders apart"
    # k = 1: the value itself, its bits
    one = np.array([[-0.0, np.float32(1e-45), 7.5]], np.float32)
    assert ext.debug_macro_fold_host(one).view(np.uint32).tolist() == one[0].view(np.uint32).tolist()
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((11, 257)) * 10.0 ** rng.integers(-6, 7, (11, 257))).astype(np.float32)
    assert ext.debug_macro_fold_host(v).view(np.uint32).tolist() == M.fold(v).view(np.uint32).tolist()


# ---- the episode log with the mirror of the ticks left -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_episode_log_update_with_the_mirror(seed):
    """several macro steps in a row through the log's host twin -- the per-tick body the kernel runs, with the rule of mv_macro_step.h walked over the mirror
    -- against the numpy model: records, running returns and lengths, the mirrors of budget and ticks left behind every call"""
    rng = np.random.default_rng(100 + seed)
    N, A, k, calls = 9, (1, 2, 3, 1)[seed], (4, 11, 1, 16)[seed], 7
    model = M.MacroModel(N, A, capacity=64)
    budget = None if seed % 2 == 0 else rng.integers(-1, 4, N).astype(np.int32)
    model.attach(budget)
    left = None if budget is None else budget.copy()
    mask = None if seed < 2 else (np.arange(N) % 4 != 1).astype(np.uint8)
    state, tick = None, 0
    for c in range(calls):
        rewards = rng.standard_normal((k, N * A)).astype(np.float32)
        dones = (rng.random((k, N)) < 0.2).astype(np.uint8)
        tobj = rng.standard_normal((k, N * A)).astype(np.float32)
        ticks = None if c % 3 == 0 else rng.integers(-1, k + 3, N).astype(np.int32)
        tl = np.full(N, k, np.int32) if ticks is None else np.clip(ticks, 0, k).astype(np.int32)
        steps = model.feed_macro(rewards, dones, tobj, ticks, mask)
        state = ext.debug_episode_log_macro_host(mask, left, tl, rewards, dones, tobj, A, 64, first_tick=tick, state=state)
        tick += k
        want_tl = M.rule(dones, mask, None if budget is None else budget, ticks)[2]
        assert tl.tolist() == want_tl.tolist(), f"call {c}: the mirror of the ticks left"
        if left is not None:
            assert left.tolist() == model.left.tolist(), f"call {c}: the mirror of the budgets"
            budget = model.left.copy()
        assert state["ret"].tobytes() == model.ret.tobytes() and state["len"].tolist() == model.len.tolist(), f"call {c}"
        assert steps.any() or c > 0
    want = model.drain()
    assert state["count"] == len(want) and state["dropped"] == model.dropped
    assert state["records"][:state["count"]].tobytes() == want.astype(ext.EPISODE_RECORD_DTYPE).tobytes()
    assert len(want) > 0, "no episode finished: the case shows nothing"
    # tl = None: the budget twin, byte for byte
    r, d, o = rng.standard_normal((3, N * A)).astype(np.float32), (rng.random((3, N)) < 0.3).astype(np.uint8), np.zeros((3, N * A), np.float32)
    a = ext.debug_episode_log_macro_host(mask, None, None, r, d, o, A, 16)
    b = ext.debug_episode_log_budget_host(mask, None, r, d, o, A, 16)
    assert a["records"].tobytes() == b["records"].tobytes() and a["ret"].tobytes() == b["ret"].tobytes() and a["count"] == b["count"]


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------------
def test_default_signatures():
    from megaverse_amd.extension import MegaverseGym
    from megaverse_amd.megaverse_env import MegaverseEnv
    from megaverse_amd.multitask import MultiTaskGym
    from megaverse_amd import rl
    p = inspect.signature(MegaverseGym.macro_step).parameters
    assert list(p) == ["self", "k", "actions", "ticks", "render"] and p["ticks"].default is None and p["render"].default == "last"
    p = inspect.signature(MegaverseEnv.macro_step).parameters
    assert list(p) == ["self", "actions", "k", "ticks", "render"] and p["k"].default is None and p["ticks"].default is None and p["render"].default == "last"
    assert inspect.signature(MegaverseEnv.__init__).parameters["frame_skip"].default == 1
    with pytest.raises(RuntimeError, match="not provided"):
        MultiTaskGym.macro_step(None, 4, None)
    assert "frame_skip" in inspect.getsource(rl.Wrapper.__init__)


def test_argument_checks_need_no_device():
    a = np.zeros((6, 6), np.int32)
    got, t = ext.check_macro_step_args(a.tolist(), None, 3, 2)
    assert got.dtype == np.int32 and got.shape == (6, 6) and t is None
    got, t = ext.check_macro_step_args(a, [0, 1, 9], 3, 2)
    assert t.dtype == np.int32 and t.tolist() == [0, 1, 9]
    for bad_a, bad_t in ((np.zeros((5, 6), np.int32), None), (np.zeros((6, 6), np.float32), None), (a, [1, 2]), (a, [0.5, 1, 2]), (None, None)):
        with pytest.raises(ValueError):
            ext.check_macro_step_args(bad_a, bad_t, 3, 2)
    with pytest.raises(ValueError, match="render"):
        ext.render_mode_of("sometimes")
    from megaverse_amd.megaverse_env import MegaverseEnv
    for bad in (0, -1, 2.0, True, "4"):
        with pytest.raises(ValueError, match="frame_skip"):
            MegaverseEnv("TowerBuilding", 2, 1, frame_skip=bad)
