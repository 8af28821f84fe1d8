"""Episode budgets without a device: the rule's host twin (megaverse_amd/csrc/mv_episode_budget.h through mv_debug_episode_budget_host) against a numpy
restatement, the episode log's budgeted host twin against the numpy model, the ABI, the refusals and argument checks that need no device."""
import os
import re

import numpy as np
import pytest

import episode_log_util as U
from episode_budget_util import BudgetModel, rule
from megaverse_amd import extension
from megaverse_amd.extension import (check_episode_budget, debug_episode_budget_host, debug_episode_log_budget_host,
                                     debug_episode_log_masked_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dones_at(k, n, where):
    d = np.zeros((k, n), np.uint8)
    for t, e in where:
        d[t, e] = 1
    return d


def test_rule_by_hand():
    """1. one call of 8 ticks, 8 envs -- budget 0 at attach (env 0); 1 with a done on the call's first, a middle and the last tick (envs 1, 2, 3); 2 with
    two dones inside the call and a third that must not happen (env 4); -1 with three dones (env 5); a mask-frozen env that never spends (env 6); 1 and no
    done (env 7)"""
    k, n = 8, 8
    d = dones_at(k, n, [(0, 0), (3, 0), (0, 1), (4, 1), (3, 2), (7, 3), (1, 4), (4, 4), (6, 4), (0, 5), (2, 5), (7, 5), (2, 6), (5, 6)])
    mask = np.array([1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    left = np.array([0, 1, 1, 1, 2, -1, 1, 1], np.int32)
    steps, out = debug_episode_budget_host(d, mask, left)
    want = np.ones((k, n), np.uint8)
    want[:, 0] = 0          # halted from the attach on
    want[1:, 1] = 0         # finished on tick 0: the finishing tick itself steps
    want[4:, 2] = 0         # ... on tick 3
    #                         env 3 finishes on the last tick: every tick of the call steps
    want[5:, 4] = 0         # two episodes: ticks 1 and 4
    #                         env 5 is unlimited
    want[:, 6] = 0          # frozen by the mask
    assert steps.tolist() == want.tolist()
    assert out.tolist() == [0, 0, 0, 0, 0, -1, 1, 1]
    # the same without the mask: env 6 steps and finishes on tick 2
    steps, out = debug_episode_budget_host(d, None, left)
    want[:, 6] = [1, 1, 1, 0, 0, 0, 0, 0]
    assert steps.tolist() == want.tolist() and out.tolist() == [0, 0, 0, 0, 0, -1, 0, 1]
    # carried over a second call: who halted stays halted whatever the dones say; env 7 spends now
    steps2, out2 = debug_episode_budget_host(dones_at(3, n, [(0, 1), (1, 7), (2, 7)]), None, out)
    assert steps2.tolist() == [[0, 0, 0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 1, 0, 0]]
    assert out2.tolist() == [0, 0, 0, 0, 0, -1, 0, 0]


@pytest.mark.parametrize("seed", range(6))
def test_rule_against_numpy(seed):
    """1. random dones / masks / budgets (odd sizes; INT32_MIN and a large budget among them): steps and left, value for value"""
    rng = np.random.default_rng(seed)
    k, n = int(rng.integers(1, 40)), int(rng.integers(1, 70))
    d = (rng.random((k, n)) < 0.2).astype(np.uint8) * rng.integers(1, 256, (k, n)).astype(np.uint8)   # (any non-zero byte is a done)
    mask = None if seed % 3 == 0 else (rng.random(n) < 0.7).astype(np.uint8) * 255
    left = rng.integers(-2, 5, n).astype(np.int32)
    left[rng.random(n) < 0.05] = np.iinfo(np.int32).min
    left[rng.random(n) < 0.05] = np.iinfo(np.int32).max
    steps, out = debug_episode_budget_host(d, mask, left)
    want_steps, want_left = rule(d, mask, left)
    assert steps.tolist() == want_steps.astype(np.uint8).tolist()
    assert out.tolist() == want_left.tolist()
    assert (out[left < 0] == left[left < 0]).all() and (out >= 0)[left >= 0].all()
    # an env finishes exactly as many episodes as it spends
    spent = (want_steps & (d != 0) & (left[None] > 0)).sum(axis=0)
    assert ((left - out)[left > 0] == spent[left > 0]).all()


def synthetic(seed, k, N, A):
    rng = np.random.default_rng(seed)
    rewards = (rng.standard_normal((k, N * A)) * (rng.random((k, N * A)) < 0.4)).astype(np.float32)
    dones = (rng.random((k, N)) < 0.15).astype(np.uint8)
    tobj = rng.standard_normal((k, N * A)).astype(np.float32)
    return rewards, dones, tobj


# (ticks of the call, its mask or None, a budget attached in front of the call: a list, None = detach, "keep" = nothing happens)
LEGS = [(5, None, "keep"), (16, None, [1, 2, 0, -1, 1]), (16, [1, 1, 1, 1, 0], "keep"), (9, None, "keep"), (16, None, [1, 1, 1, 1, 1]), (7, [1, 0, 1, 1, 1], "keep"),
        (11, None, [2, 2, 2, -1, 0]), (6, None, None), (8, None, [0, 0, 3, 3, 3])]


@pytest.mark.parametrize("A", [1, 4])
def test_budgeted_log_twin_against_numpy(A):
    """2. mv_debug_episode_log_budget_host over calls with budgets, masks, re-attaches and a detach (N = 5): random rewards and dones -- the halted envs' too:
    none of them may count -- against the numpy model: records, count, ret, len and the mirror byte for byte after every call"""
    N, cap = 5, 4096
    model, state, tick, left = BudgetModel(N, A), None, 0, None
    halted_mid_call = resumed = False
    for j, (k, mask, budget) in enumerate(LEGS):
        r, d, o = synthetic(300 + j, k, N, A)
        if budget != "keep":
            was = None if left is None else left.copy()
            left = None if budget is None else np.array(budget, np.int32)
            model.attach(budget)
            resumed = resumed or (was is not None and left is not None and bool(((was == 0) & (left != 0)).any()))
        before = None if left is None else left.copy()
        model.feed(r, d, o, mask)
        state = debug_episode_log_budget_host(mask, left, r, d, o, A, cap, tick, state)
        tick += k
        assert state["ret"].tobytes() == model.ret.tobytes() and state["len"].tobytes() == model.len.tobytes(), f"call {j}"
        assert state["count"] == len(model.records), f"call {j}"
        if left is not None:
            assert left.tobytes() == model.left.tobytes(), f"call {j}"
            want_steps, want_left = rule(d, mask, before)
            assert left.tolist() == want_left.tolist()
            halted_mid_call = halted_mid_call or bool((want_steps.any(axis=0) & ~want_steps.all(axis=0)).any())
    assert halted_mid_call and resumed
    want = np.array(model.records, U.RECORD)
    assert state["count"] == len(want) > 10 and state["dropped"] == 0
    assert state["records"][:state["count"]].tobytes() == want.tobytes()
    # the budgets mattered: the same ticks without them leave another log
    plain = U.Model(N, A)
    for j, (k, _, _) in enumerate(LEGS):
        plain.feed(*synthetic(300 + j, k, N, A))
    assert len(plain.records) > len(want)


@pytest.mark.parametrize("A", [1, 4])
def test_length_after_a_reattach_counts_from_the_first_stepped_tick(A):
    """2. env 0 finishes on tick 2 of a call of 16 and halts; re-attached, it finishes 5 ticks into the next call: length 5, whatever the 13 halted ticks held"""
    N = 2
    r = np.ones((16, N * A), np.float32)
    d = dones_at(16, N, [(2, 0)])
    o = np.zeros((16, N * A), np.float32)
    left = np.array([1, -1], np.int32)
    state = debug_episode_log_budget_host(None, left, r, d, o, A, 64)
    assert left.tolist() == [0, -1] and state["count"] == A and state["len"].tolist() == [0, 16]
    assert state["records"][:A]["length"].tolist() == [3] * A and state["records"][:A]["ret"].tolist() == [3.0] * A
    left[:] = [1, -1]   # the re-attach
    state = debug_episode_log_budget_host(None, left, r, dones_at(16, N, [(4, 0), (9, 0)]), o, A, 64, 16, state)
    assert left.tolist() == [0, -1] and state["count"] == 2 * A
    rec = state["records"][A:2 * A]
    assert rec["length"].tolist() == [5] * A and rec["ret"].tolist() == [5.0] * A and rec["end_tick"].tolist() == [20] * A
    assert state["len"].tolist() == [0, 32] and state["ret"].reshape(N, A)[0].tolist() == [0.0] * A


@pytest.mark.parametrize("A", [1, 3])
def test_null_budget_is_the_masked_hook(A):
    """2. left = NULL against mv_debug_episode_log_masked_host, and an all -1 budget: every output byte for byte"""
    N, cap = 5, 12
    old = new = unlimited = None
    tick = 0
    left = np.full(N, -1, np.int32)
    for j in range(4):
        k = 7 + j
        r, d, o = synthetic(520 + j, k, N, A)
        mask = None if j % 2 else [1, 0, 1, 1, 1]
        old = debug_episode_log_masked_host(mask, r, d, o, A, cap, tick, old)
        new = debug_episode_log_budget_host(mask, None, r, d, o, A, cap, tick, new)
        unlimited = debug_episode_log_budget_host(mask, left, r, d, o, A, cap, tick, unlimited)
        tick += k
        for other in (new, unlimited):
            for key in ("ret", "len", "records"):
                assert old[key].tobytes() == other[key].tobytes(), (j, key)
            assert (old["count"], old["dropped"]) == (other["count"], other["dropped"])
    assert left.tolist() == [-1] * N and old["dropped"] > 0


def test_symbols_are_declared_exported_and_bound():
    """3. the new calls: declared in the header with the bound arity, exported by the library, in the ctypes table; the pybind module binds the Python surface"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, ret, arity in (("mv_set_episode_budget", "int", 2), ("mv_set_episode_budget_host", "int", 2), ("mv_get_episode_budget", "int", 1),
                             ("mv_episode_budget_device_ptr", r"void\s*\*", 1), ("mv_halted_count_device_ptr", r"void\s*\*", 1), ("mv_halted_count", "int", 2),
                             ("mv_debug_episode_log_budget_host", "int", 15), ("mv_debug_episode_budget_host", "int", 7)):
        m = re.search(r"\b" + ret + r"\s*" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == arity, name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert len(bound["mv_debug_episode_log_masked_host"][1]) == 14   # (the old hooks' signatures are what they were)
    assert lib.mv_abi_version() == 2   # (additive)
    module = open(os.path.join(ROOT, "megaverse_amd", "pybind", "megaverse_module.cpp")).read()
    for name in ("set_episode_budget", "has_episode_budget", "halted_count", "episode_budget_device_ptr", "halted_count_device_ptr"):
        assert re.search(r'\.def\("' + name + r'",\s*&Gym::' + name + r"\)", module), name
    for call in ("mv_set_episode_budget_host", "mv_get_episode_budget", "mv_halted_count", "mv_episode_budget_device_ptr", "mv_halted_count_device_ptr"):
        assert call + "(gym_" in module, call


def test_no_gym_is_an_error_with_text():
    """4. a null gym: -1 (NULL from the pointer getters) with text"""
    lib = extension.load_library()
    b = np.ones(4, np.int32)
    out = extension._I()
    import ctypes
    for fn, args in ((lib.mv_set_episode_budget, (b.ctypes.data,)), (lib.mv_set_episode_budget_host, (b.ctypes.data,)), (lib.mv_set_episode_budget, (None,)),
                     (lib.mv_set_episode_budget_host, (None,)), (lib.mv_get_episode_budget, ()), (lib.mv_halted_count, (ctypes.byref(out),))):
        assert fn(None, *args) == -1
        assert b"null gym" in lib.mv_last_error() and b"mv_" in lib.mv_last_error()
    assert not lib.mv_episode_budget_device_ptr(None) and not lib.mv_halted_count_device_ptr(None)


def test_host_twin_refuses_bad_arguments():
    lib = extension.load_library()
    d, left, steps = np.zeros((2, 3), np.uint8), np.zeros(3, np.int32), np.zeros((2, 3), np.uint8)
    assert lib.mv_debug_episode_budget_host(None, None, left.ctypes.data, 2, 3, steps.ctypes.data, left.ctypes.data) == -1
    assert lib.mv_debug_episode_budget_host(d.ctypes.data, None, left.ctypes.data, 2, 0, steps.ctypes.data, left.ctypes.data) == -1
    assert b"mv_debug_episode_budget_host" in lib.mv_last_error()
    with pytest.raises(ValueError):
        debug_episode_budget_host(d, None, np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        debug_episode_log_budget_host(None, [1, 2, 3], *synthetic(1, 2, 3, 1), 1, 8)   # (left is advanced in place: a numpy int32 array)


def test_budget_argument_check():
    """4. None, an int, a sequence, numpy; what is not N int32 values is a ValueError"""
    assert check_episode_budget(None, 3) is None
    b = check_episode_budget(2, 3)
    assert b.dtype == np.int32 and b.tolist() == [2, 2, 2] and b.flags.c_contiguous
    assert check_episode_budget(-1, 2).tolist() == [-1, -1]
    assert check_episode_budget([0, 1, -1], 3).tolist() == [0, 1, -1]
    assert check_episode_budget(np.array([5, 0, 7], np.int64), 3).dtype == np.int32
    for bad in ([1, 2], np.zeros((3, 1), np.int32), np.zeros(3, np.float32), [0.5, 0.0, 1.0], [True, False, True], True, 2 ** 31, [0, 0, 2 ** 31], "1"):
        with pytest.raises(ValueError, match="set_episode_budget"):
            check_episode_budget(bad, 3)

    class Bare:
        shape, dtype = (3,), "torch.int32"

        def data_ptr(self):
            return 0

    with pytest.raises(ValueError, match="set_episode_budget"):
        check_episode_budget(Bare(), 3)


def test_multitask_refuses_with_text():
    """4. MultiTaskGym.set_episode_budget raises before it touches a device"""
    from megaverse_amd.multitask import MultiTaskGym
    with pytest.raises(RuntimeError, match="mv_set_episode_budget"):
        MultiTaskGym.set_episode_budget(type("G", (), {"_group": None})(), 1)


@pytest.mark.parametrize("family", ["empty", "football", "rearrange", "sokoban"])
def test_gpu_schedule_condition_on_the_oracle(family):
    """what tests/test_episode_budget_gpu.py relies on, checked on the CPU oracle (the families whose schedule takes a fraction of a second here; the GPU
    tests assert the same of every family before they use it): with budget 1 the eight envs halt on eight different ticks behind the attach, one on
    tick 7 and one on tick 8 of a 16-tick call, the others inside a launch; a halted env's walk stands still"""
    import episode_budget_util as B
    scenario, params, seed, TA, delays, walks, halts = B.schedule(family)
    B.assert_condition(halts, family)
    assert sorted(halts) == sorted(B.TARGETS) and all(0 <= d < TA for d in delays)
    for e, w in enumerate(walks):
        last = max(w)
        cap, stepped, left = w[last]
        assert stepped and left == 0 and cap["dones"][e] == 1 and all(w[t][2] == 1 for t in range(TA, last))
        after, stepped, left = B.at(w, last + 3)
        assert not stepped and left == 0 and not after["rewards"].any() and not after["dones"].any()
        assert after["snap"][e].tobytes() == cap["snap"][e].tobytes() if hasattr(cap["snap"][e], "tobytes") else after["snap"][e] is cap["snap"][e]
