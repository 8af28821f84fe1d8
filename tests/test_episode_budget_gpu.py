"""Episode budgets on the GPU (include/megaverse_hip.h: mv_set_episode_budget): envs halt on the device after n finished episodes.

Every test but the launch-shape one uses 8 envs and 32 x 32 frames (tests/reset_envs_util.py).  Envs are independent, so expected values come from the CPU
oracle as it is (tests/episode_budget_util.py): env e of the gym is env e of an oracle that stepped on exactly the gym ticks env e stepped on -- every tick
up to and including its halting tick, none from then on, and after a re-attach the ticks behind it, with the actions of those tick indices.  Before the budget
is attached the envs' clocks are staggered (env e is frozen for delays[e] ticks by step masks), so that with budget 1 the envs halt on different ticks of
the calls that follow: one on tick 7 and one on tick 8 of a 16-tick call (the boundary between its two launches), the others inside a launch.  Where a test
compares two paths of the library instead, one of them is the tick-by-tick mv_step path the oracle tests pin.  Every comparison is equality of bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_budget_util as B
import episode_log_util as U
import oracle_lib
from episode_budget_util import H, N, W, BudgetModel, rule
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.megaverse_env import MegaverseEnv
from megaverse_amd.rollout import action_masks, sample_actions
from test_reset_envs_gpu import all_raw, check_env, make_gym, raw
from test_step_mask_gpu import SENTINEL, TICKS, run_entry, step_ok

pytestmark = pytest.mark.gpu


def make(family, A, mode, log=0):
    scenario, params, _, seed = B.FAMILIES[family]
    return make_gym(scenario, A, mode, params, seed=seed, log=log)


# BoxAGone's episodes end by what the agents do, 30 - 60 ticks in: the tests that go on with other actions than the oracle schedule's (the entry matrix) step it 16
# ticks further first -- on the CPU oracle three envs then end an episode within the next 16 ticks, on ticks 5, 7 and 8
EXTRA = {"boxagone": 16}


def stagger(g, family, A, extra=0):
    """the gym ticks 0 .. TA - 1 of the family's schedule: env e is frozen for its first delays[e] ticks (host step masks), nothing is drawn but the last
    tick; the mask is detached again; `extra` more ticks of every env -> the ticks stepped"""
    TA, delays = B.stagger_plan(family, A)
    delays = np.array(delays)
    for t in range(TA + extra):
        if t == 0 or (t in delays and t < TA):
            g.set_step_mask(delays <= t)
        if t == TA:
            g.set_step_mask(None)
        g.set_actions_batched(B.actions(t, A))
        rc = g._lib.mv_step(g._g) if t == TA + extra - 1 else g._lib.mv_step_no_render(g._g)
        assert rc == 0, g._lib.mv_last_error()
    g.set_step_mask(None)
    return TA + extra


def budget_of(g):
    return g.episode_budget().cpu().numpy()


def check_budget(g, left, what):
    """the gym-owned array, the halted count on the host and through its device pointer, against the rule"""
    assert budget_of(g).tolist() == list(left), f"{what}: budgets"
    halted = sum(1 for v in left if v == 0)
    assert g.halted_count() == halted and int(g.halted_count_tensor().cpu()[0]) == halted, f"{what}: halted count"


# ---- 1. against the oracle, every scenario family; 5. several agents ----------------------------------------------------------------------------------
def against_the_oracle(family, A):
    scenario, _, _, TA, _, walks, halts = B.schedule(family, A)
    B.assert_condition(halts, family)
    g = make(family, A, "exact")
    assert stagger(g, family, A) == TA
    for e in range(N):
        check_env(g, B.at(walks[e], TA - 1)[0], scenario, A, e, f"{family}, tick {TA - 1} (before the attach)")
    g.set_episode_budget(1)
    assert g.has_episode_budget()
    check_budget(g, [1] * N, "behind the attach")
    consumed = {}
    for t in range(TA, TA + max(halts) + B.PAST + 1):
        g.set_actions_batched(B.actions(t, A))
        step_ok(g)
        now = g.debug_episodes_consumed().tolist()
        for e in range(N):
            cap, stepped, _ = B.at(walks[e], t)
            check_env(g, cap, scenario, A, e, f"{family}, tick {t} = attach + {t - TA}{'' if stepped else ' (halted)'}")
            if stepped:
                consumed[e] = now[e]
            else:
                assert now[e] == consumed[e], f"{family}, tick {t}: halted env {e} took an episode"
        check_budget(g, [B.at(walks[e], t)[2] for e in range(N)], f"{family}, tick {t}")
    assert g.halted_count() == N
    g.close()


@pytest.mark.parametrize("family", B.ORACLE_FAMILIES)
def test_budget_one_against_the_oracle(hip, family):
    """1. the clocks staggered, budget 1 for every env, mv_step tick by tick until 10 ticks past the last halt: snapshot, scenario state, reward bits,
    dones, true objectives and exact-mode frames of every env behind every tick; the budgets and the halted count behind every call; a halted env takes
    no episode"""
    against_the_oracle(family, 1)


@pytest.mark.parametrize("family,A", [("tower", 4), ("obstacles_easy", 2)])
def test_several_agents_against_the_oracle(hip, family, A):
    """5. TowerBuilding x 4 (every wave ticks) and ObstaclesEasy x 2 on test 1's schedule; the finishing tick's rewards of every agent are the oracle's"""
    against_the_oracle(family, A)


# ---- 2. budgets 0 / 1 / 2 / -1 in one gym, then a re-attach ---------------------------------------------------------------------------------------------
FIRST, SECOND = (0, 1, 2, -1, 1, 2, 0, -1), (1, 1, 0, -1, 2, 0, 1, 3)


@pytest.mark.parametrize("family", ["rearrange", "football"])
def test_mixed_budgets_then_a_reattach(hip, family):
    """2. episodes of 65 ticks.  Budgets 0 / 1 / 2 / -1 mixed; 80 ticks later every finite env has halted and every value is replaced: halted envs resume
    (against oracles that skipped their halted windows), a running env is halted by a 0, the unlimited env is oracle P throughout"""
    A = 2 if family == "football" else 1
    scenario, _, _, TA, delays, _, _ = B.schedule(family, A)
    TR, T = TA + 80, TA + 80 + 80
    walks = [B.walk(family, A, e, delays[e], ((TA, FIRST[e]), (TR, SECOND[e])), TA - 1, T) for e in range(N)]
    assert all(walks[e][TR - 1][2] == (0 if FIRST[e] >= 0 else -1) for e in range(N)), "a finite env has not halted before the re-attach"
    assert [walks[e][T - 1][2] for e in range(N)] == [0, 0, 0, -1, 1, 0, 0, 2]   # (halted again; halted by the 0; one and two episodes into a larger budget)
    resumed = [e for e in range(N) if FIRST[e] >= 0 and SECOND[e] > 0]
    assert all(walks[e][TR][1] and not walks[e][TR - 1][1] for e in resumed)
    g = make(family, A, "exact")
    stagger(g, family, A)
    for t in range(TA, T):
        if t == TA:
            g.set_episode_budget(np.array(FIRST, np.int32))
        if t == TR:
            g.set_episode_budget(list(SECOND))
        g.set_actions_batched(B.actions(t, A))
        step_ok(g)
        for e in range(N):
            cap, stepped, _ = walks[e][t]
            check_env(g, cap, scenario, A, e, f"{family}, tick {t}{'' if stepped else ' (halted)'}")
        check_budget(g, [walks[e][t][2] for e in range(N)], f"{family}, tick {t}")
    g.close()


# ---- 3. every stepping entry and policy; 4. batched entries of every family; 5. several agents -------------------------------------------------------------
ENTRIES = ("step", "step_no_render", "step_n_8", "step_n_16", "render_none", "render_last")


@functools.lru_cache(maxsize=None)
def twin_reference(family, A, policy):
    """the budgeted twin, tick by tick through mv_step (the entry test 1 pins to the oracle), not pipelined"""
    g = make(family, A, "fast")
    g.set_pipelining(False)
    stagger(g, family, A, EXTRA.get(family, 0))
    g.set_episode_budget(1)
    out = run_entry(g, "step", policy, A)
    out["left"] = budget_of(g).tolist()
    g.close()
    return out


def check_entry(monkeypatch, family, A, entry, policy, variants):
    ref = twin_reference(family, A, policy)
    steps, left = rule(ref["done"], None, [1] * N)
    assert ref["left"] == left.tolist()
    per = np.repeat(steps, A, axis=1)
    assert not ref["rew"][~per].any() and not ref["done"][~steps].any()
    halts = [int(np.flatnonzero(ref["done"][:, e])[0]) if ref["done"][:, e].any() else None for e in range(N)]
    if family != "boxagone":
        B.assert_condition(halts, f"{family} x {A}, {policy}")
    else:   # (its endings follow the actions: some envs halt inside these 16 ticks -- on both sides of the boundary between two launches -- and some do not)
        assert {7, 8} < {h for h in halts if h is not None} and None in halts and any(h is not None and h % 8 not in (0, 7) for h in halts), halts
    for variant in variants:
        what = f"{family} x {A}, {entry}, {policy}, {variant}"
        monkeypatch.delenv("MV_STEP_PIPE", raising=False)
        if variant in ("pipe0", "pipe1"):
            monkeypatch.setenv("MV_STEP_PIPE", variant[-1])
        outs = []
        for budgeted in (True, False):
            g = make(family, A, "fast")
            if variant == "unpipelined":
                g.set_pipelining(False)
            stagger(g, family, A, EXTRA.get(family, 0))
            if budgeted:
                g.set_episode_budget(1)
            outs.append(run_entry(g, entry, policy, A))
            if budgeted:
                check_budget(g, left.tolist(), what)
            g.close()
        got, plain = outs
        assert got["launches"] == plain["launches"], f"{what}: {got['launches']} launches with a budget, {plain['launches']} without"
        if family != "boxagone" and entry not in ("step", "step_no_render"):   # (BoxAGone is stepped tick by tick: its episodes can end within a few ticks)
            assert got["launches"][0] == 2, f"{what}: {got['launches'][0]} step launches for 16 ticks: these are not the resident multi-tick kernels"
        assert got["rew"].tobytes() == ref["rew"].tobytes(), f"{what}: rewards"
        assert got["done"].tobytes() == ref["done"].tobytes(), f"{what}: dones"
        assert got["snaps"] == ref["snaps"], f"{what}: final state of envs {[e for e in range(N) if got['snaps'][e] != ref['snaps'][e]]}"
        assert got["tobj"].tobytes() == ref["tobj"].tobytes() and got["consumed"] == ref["consumed"], what
        assert got["snaps"] != plain["snaps"], f"{what}: the budget changed nothing"
        drawn = {"step": range(TICKS), "step_n_8": range(TICKS), "step_n_16": range(TICKS), "render_last": [TICKS - 1]}.get(entry, [])
        assert sorted(got["frames"]) == list(drawn)
        for t in drawn:
            assert got["frames"][t].tobytes() == ref["frames"][t].tobytes(), f"{what}: frames of tick {t}"
        if entry in ("step_no_render", "render_none", "step_n_8", "step_n_16"):   # (the ring entries took the frames, or nothing was drawn)
            assert (got["slab"] == SENTINEL).all(), f"{what}: {int((got['slab'] != SENTINEL).sum())} bytes of the slab were written"


TOWER_MATRIX = [(e, p) for e in ENTRIES for p in ("multidiscrete", "single-bit", "sequence")]


@pytest.mark.parametrize("entry,policy", TOWER_MATRIX, ids=[f"{e}-{p}" for e, p in TOWER_MATRIX])
def test_every_entry_and_policy(hip, monkeypatch, entry, policy):
    """3. TowerBuilding with episodes long enough for resident multi-tick launches, fast pixels, the clocks staggered, budget 1, 16 ticks through each entry
    and policy: rewards and dones of every tick, every drawn
    frame, final snapshots, true objectives, consumed counts, budgets and halted count equal the tick-by-tick twin's; the launches equal the same calls'
    without a budget; MV_RENDER_NONE, mv_step_no_render and calls into rings write not one byte of the slab.  Pipelined (the default), not pipelined, and
    with the software-pipelined kernel forced off and on."""
    variants = ("default", "unpipelined") if entry in ("step", "step_no_render") else ("default", "pipe0", "pipe1")
    check_entry(monkeypatch, "tower_long", 1, entry, policy, variants)


@pytest.mark.parametrize("entry", ["step_n_8", "render_none", "render_last"])
@pytest.mark.parametrize("family", ["boxagone", "collect_long", "empty", "football", "hex_memory_long", "obstacles_easy", "rearrange", "sokoban"])
def test_batched_entries_every_family(hip, monkeypatch, family, entry):
    """4. the multi-tick kernels of every other scenario family (each has its own instantiations of the shared bodies)"""
    check_entry(monkeypatch, family, 1, entry, "multidiscrete", ("default", "pipe0") if family in ("obstacles_easy", "empty") else ("default",))


@pytest.mark.parametrize("entry", ["step", "step_n_8", "step_n_16", "render_none", "render_last"])
def test_several_agents_tower_entries(hip, monkeypatch, entry):
    """5. TowerBuilding with four agents per env: every wave of the workgroup keeps the env's budget and takes the same side of the per-tick choice"""
    check_entry(monkeypatch, "tower_long", 4, entry, "multidiscrete", ("default",))


# ---- 6. mask and budget together --------------------------------------------------------------------------------------------------------------------------
def test_mask_and_budget_together(hip):
    """6. Sokoban (65-tick episodes), budget 1, envs 1 and 4 frozen by a step mask for the first 32 ticks, batched calls of 8 into rings; the device forms
    (budget and mask written by kernels on the gym's stream, nothing synchronising) against the host forms.  A mask-frozen env spends nothing and keeps
    its state; thawed, it runs its budget and halts; budgets and dones follow the rule call by call"""
    import torch
    A, K, family = 1, 8, "sokoban"
    mask = np.ones(N, bool)
    mask[[1, 4]] = False
    out = []
    for form in ("device", "host"):
        g = make(family, A, "fast")
        stagger(g, family, A)
        before = all_raw(g)
        rings = [torch.full((K, N * A), -7.0, dtype=torch.float32, device="cuda:0"), torch.full((K, N), 9, dtype=torch.uint8, device="cuda:0")]
        keep = [torch.zeros(N, dtype=torch.int32, device="cuda:0"), torch.ones(N, dtype=torch.bool, device="cuda:0"), torch.as_tensor(mask).to("cuda:0")]
        torch.cuda.synchronize()
        g.set_output_ring(K, 0, rings[0].data_ptr(), rings[1].data_ptr())
        if form == "device":
            keep[0].add_(1)   # (0 everywhere, were it read before this kernel has run)
            g.set_episode_budget(keep[0])
            torch.logical_and(keep[2], keep[2], out=keep[1])
            g.set_step_mask(keep[1])
        else:
            g.set_episode_budget(1)
            g.set_step_mask(mask)
        left, dones, lefts = np.ones(N, np.int32), [], []
        for c in range(14):
            if c == 4:
                g.set_step_mask(None)
            g.step_n(K, "multidiscrete", B.POLICY_SEED, c * K, render="none")
            g.synchronize()
            d = rings[1].cpu().numpy()
            steps, left = rule(d, mask if c < 4 else None, left)
            assert not d[~steps].any() and budget_of(g).tolist() == left.tolist(), f"{form}, call {c}"
            if c == 3:
                assert left[[1, 4]].tolist() == [1, 1] and [raw(g, e) for e in (1, 4)] == [before[e] for e in (1, 4)], "a frozen env spent or moved"
                assert g.halted_count() == N - 2
            dones.append(d)
            lefts.append(left.tolist())
        assert g.halted_count() == N and np.concatenate(dones)[:, [1, 4]].sum(axis=0).tolist() == [1, 1]
        out.append((np.concatenate(dones).tobytes(), lefts, all_raw(g)))
        g.close()
        del keep
    assert out[0] == out[1], "the device forms and the host forms differ"


# ---- 7. the episode log -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_episode_log_every_entry(hip, entry):
    """7. Sokoban (65-tick episodes), the clocks staggered, the log switched on, budget 1, legs of 16 ticks through one entry.  The model (BudgetModel) is fed
    the gym's own per-tick outputs: records, running returns and lengths byte for byte behind every leg; exactly sum(budget) records once everybody has
    halted, and nothing moves on a further leg; after a re-attach an episode's length counts from its own first stepped tick (65, not 65 + the halted
    ticks); with the log switched off and on again while the budget is attached, the log's mirror is the live array: halted ticks add no length"""
    import torch
    A, K, family = 1, 16, "sokoban"
    g = make(family, A, "fast")
    TA = stagger(g, family, A)
    g.set_episode_log(4096)
    model = BudgetModel(N, A)
    model.tick = TA
    batched = entry not in ("step", "step_no_render")
    if batched:
        k = 8 if entry == "step_n_8" else K
        mode = {"render_none": "none", "render_last": "last"}.get(entry, "every")
        rings = [torch.zeros((K, N * A), dtype=torch.float32, device="cuda:0"), torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")]
        obs = torch.zeros((K, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0") if mode == "every" else None
        torch.cuda.synchronize()
        g.set_output_ring(K, obs.data_ptr() if obs is not None else 0, rings[0].data_ptr(), rings[1].data_ptr())
    legs = [0]

    def leg(what):
        first = legs[0] * K
        legs[0] += 1
        if batched:
            for j in range(0, K, k):
                g.step_n(k, "multidiscrete", B.POLICY_SEED, first + j, render=mode)
            g.synchronize()
            model.feed(rings[0].cpu().numpy(), rings[1].cpu().numpy(), np.repeat(g.get_true_objectives()[None], K, axis=0))
        else:
            for t in range(K):
                g.sample_random_actions(B.POLICY_SEED, first + t)
                rc = g._lib.mv_step(g._g) if entry == "step" else g._lib.mv_step_no_render(g._g)
                assert rc == 0, g._lib.mv_last_error()
                model.feed(g.get_rewards_array()[None], g.get_dones()[None], g.get_true_objectives()[None])
        if g.episode_log_capacity() > 0:
            assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes(), f"running returns, {what}"
            assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes(), f"running lengths, {what}"
        assert budget_of(g).tolist() == model.left.tolist(), what

    def drained(what):
        want = model.drain()
        got = g.drain_episode_log()
        assert g.episode_log_dropped == 0 and got.tobytes() == want.tobytes(), what
        return want

    g.set_episode_budget(1)
    model.attach([1] * N)
    leg("budget 1")
    assert g.halted_count() == N
    leg("everybody halted")
    first = drained("budget 1")
    assert len(first) == N == sum([1] * N) and sorted(first["length"].tolist()) == sorted(h + 1 for h in B.TARGETS)
    assert model.len.tolist() == [0] * N
    g.set_episode_budget(1)   # the re-attach
    model.attach([1] * N)
    for i in range(5):
        leg(f"re-attached, leg {i}")
    second = drained("re-attached")
    assert len(second) == N and second["length"].tolist() == [65] * N and g.halted_count() == N
    g.set_episode_budget(2)
    model.attach([2] * N)
    g.set_episode_log(0)
    for i in range(5):   # (the log is off: the first of the two episodes ends unrecorded, the budgets go to 1)
        leg(f"log off, leg {i}")
    assert budget_of(g).tolist() == [1] * N
    model.records.clear()
    model.restart()
    g.set_episode_log(4096)
    for i in range(6):
        leg(f"log on again, leg {i}")
    third = drained("log on again")
    assert len(third) == N and g.halted_count() == N and model.len.tolist() == [0] * N
    g.close()


@pytest.mark.parametrize("n,A", [(8, 4), (264, 4), (1040, 1)], ids=["8x4", "264x4", "1040x1"])
def test_episode_log_several_agents_and_more_than_1024_agents(hip, n, A):
    """7. Empty with 65-tick episodes, A agents per env, up to 1056 agents: the log's kernel takes several agents per thread (chunks of 1024) and finds an
    agent's env by division.  Five ticks, the log on, budgets 0 / 1 / 2 / -1 by env index, nine calls of 16 ticks without drawing: the envs halt on tick 11 of
    the fourth call and on tick 12 of the eighth.  Records, running returns, lengths and budgets against the numpy model fed the gym's own per-tick outputs"""
    import torch
    K = 16
    g = MegaverseGym("Empty", W, H, n, A, 1, False, {"episodeLengthSec": 4.3})
    g.set_pixel_mode("fast")
    g.seed(11)
    g.reset()
    for t in range(5):
        g.sample_random_actions(B.POLICY_SEED, t)
        assert g._lib.mv_step_no_render(g._g) == 0, g._lib.mv_last_error()
    g.set_episode_log(4 * n * A)
    budget = np.array([0, 1, 2, -1], np.int32)[np.arange(n) % 4]
    g.set_episode_budget(budget)
    model = BudgetModel(n, A)
    model.tick = 5
    model.attach(budget)
    rings = [torch.zeros((K, n * A), dtype=torch.float32, device="cuda:0"), torch.zeros((K, n), dtype=torch.uint8, device="cuda:0")]
    torch.cuda.synchronize()
    g.set_output_ring(K, 0, rings[0].data_ptr(), rings[1].data_ptr())
    for c in range(9):
        g.step_n(K, "multidiscrete", B.POLICY_SEED, 5 + c * K, render="none")
        g.synchronize()
        done = rings[1].cpu().numpy()
        model.feed(rings[0].cpu().numpy(), done, np.repeat(g.get_true_objectives()[None], K, axis=0))
        assert budget_of(g).tolist() == model.left.tolist(), f"call {c}"
        assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes(), f"running returns, call {c}"
        assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes(), f"running lengths, call {c}"
        if c in (3, 7):   # (gym ticks 64 and 129: entries 11 and 12 of these calls)
            j = 11 if c == 3 else 12
            assert done[j].any() and not done[:j].any(), "nobody halts inside this call: the test would prove less"
    want = model.drain()
    got = g.drain_episode_log()
    finite = int((budget == 1).sum() + 2 * (budget == 2).sum())
    unlimited = int((budget < 0).sum())
    assert len(want) == (finite + 2 * unlimited) * A and g.episode_log_dropped == 0
    assert got.tobytes() == want.tobytes()
    assert model.left.tolist() == np.where(budget < 0, -1, 0).tolist() and g.halted_count() == n - unlimited
    g.close()


def test_pybind_module_calls(hip):
    """the pybind11 flavour of the binding, built and called: an int, a list and None through set_episode_budget, the halted count, the two device
    pointers; a bool is refused (to Python a bool is an int)"""
    import torch
    from megaverse_amd import build
    from megaverse_amd.extension import _DeviceArray
    build.build_pybind()
    from megaverse_amd.pybind import megaverse as m
    g = m.MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    g.seed(11)
    g.reset()
    assert not g.has_episode_budget() and g.episode_budget_device_ptr() == 0 and g.halted_count_device_ptr() == 0
    with pytest.raises(RuntimeError, match="no episode budget"):
        g.halted_count()
    g.set_episode_budget(3)
    assert g.has_episode_budget() and g.halted_count() == 0
    values = [0, 1, -1, 0, 2, 0, 5, -7]
    g.set_episode_budget(values)
    assert g.halted_count() == 3
    left = torch.as_tensor(_DeviceArray(g.episode_budget_device_ptr(), (N,), "<i4"), device="cuda:0")
    count = torch.as_tensor(_DeviceArray(g.halted_count_device_ptr(), (1,), "<i4"), device="cuda:0")
    assert left.cpu().tolist() == values and int(count.cpu()[0]) == 3
    g.step()
    assert left.cpu().tolist() == values and g.halted_count() == 3
    for bad in (True, [1, 2], "1", 1.5):
        with pytest.raises((RuntimeError, TypeError)):
            g.set_episode_budget(bad)
    assert g.halted_count() == 3
    g.set_episode_budget(None)
    assert not g.has_episode_budget() and g.episode_budget_device_ptr() == 0
    g.close()


def test_run_episodes_sequence_policy(hip):
    """11. run_episodes(1, policy='sequence') replays a ring of 24 action entries modulo its length, over episodes of 65 ticks: the records of a twin gym
    stepped tick by tick on entry t % 24; with the log already on, its running lengths carry over into the call; without actions: ValueError"""
    import torch
    U.boxoban_env()
    A, seed, count = 1, 11, 24
    params = {"episodeLengthSec": 4.3}
    actions = np.stack([sample_actions(B.POLICY_SEED + 3, t, N * A) for t in range(count)]).astype(np.int32)
    env = MegaverseEnv("Sokoban", N, A, params=params, img_w=W, img_h=H, episode_log=64)
    env.seed(seed)
    env.reset()
    records = env.run_episodes(1, policy="sequence", actions=actions)
    assert env.env.halted_count() == N
    tw = make_gym("Sokoban", A, "fast", params, seed=seed)
    tw.set_episode_budget(1)
    model = BudgetModel(N, A)
    model.attach([1] * N)
    for t in range(65):
        tw.set_actions_batched(actions[t % count])
        assert tw._lib.mv_step_no_render(tw._g) == 0
        model.feed(tw.get_rewards_array()[None], tw.get_dones()[None], tw.get_true_objectives()[None])
    want = model.drain()
    assert len(records) == N * A == len(want) and records.tobytes() == want.tobytes() and records["length"].tolist() == [65] * N
    assert all_raw(env.env)[0] == raw(tw, 0)
    # a second evaluation with the log still on, 8 ticks into an episode
    env.set_episode_budget(None)
    dev = torch.as_tensor(actions).to("cuda:0")
    env.env.set_episode_budget(1)
    env.env.set_action_ring(count, dev.data_ptr())
    env.env.step_n(8, "sequence", 0, 0, render="none")   # (nothing ends: 8 of 65 ticks)
    env.env.set_episode_budget([0] * N)
    again = env.run_episodes(1, policy="sequence", actions=dev)
    assert len(again) == N and again["length"].tolist() == [65] * N, "the running lengths of the log count the 8 ticks before the call"
    with pytest.raises(ValueError, match="sequence"):
        env.run_episodes(1, policy="sequence")
    tw.close()
    env.close()


# ---- 8. other operations act regardless -------------------------------------------------------------------------------------------------------------------
def test_other_operations_move_state_not_budgets(hip):
    """8. Rearrange, budgets -1 for env 0 and 1 for the others, 16 ticks: envs 1 .. 7 are halted.  A fork into a halted env, a load into a halted env,
    mv_reset_envs of a halted env, mv_reset: the state moves, the budgets do not, and the halted envs stay frozen on their new state while env 0 steps"""
    A, family = 1, "rearrange"
    g = make(family, A, "exact")
    t = stagger(g, family, A)
    want = [-1] + [0] * (N - 1)
    g.set_episode_budget([-1] + [1] * (N - 1))

    def ticks(n, t):
        for _ in range(n):
            g.set_actions_batched(B.actions(t, A))
            step_ok(g)
            t += 1
        return t

    t = ticks(16, t)
    check_budget(g, want, "16 ticks")
    store = g.new_env_store(1)
    g.save_envs([0] + [-1] * (N - 1), store)
    t = ticks(2, t)
    before = all_raw(g)
    g.fork_envs([-1, -1, -1, 0] + [-1] * (N - 4))                     # env 0 -> halted env 3
    g.load_envs([-1, -1, -1, -1, -1, 0, -1, -1], store)              # the record -> halted env 5
    g.reset_envs(np.arange(N) == 2)                                  # halted env 2 takes its next episode
    moved = all_raw(g)
    assert moved[3] == moved[0] and [moved[e] != before[e] for e in range(N)] == [e in (2, 3, 5) for e in range(N)]
    check_budget(g, want, "fork, load, reset_envs")
    consumed = g.debug_episodes_consumed().tolist()
    t = ticks(3, t)
    after = all_raw(g)
    assert after[0] != moved[0] and after[1:] == moved[1:], "a halted env moved, or the unlimited one did not"
    assert g.get_dones()[1:].tolist() == [0] * (N - 1) and not g.get_rewards_array()[1:].any()
    assert g.debug_episodes_consumed().tolist()[1:] == consumed[1:]
    g.reset()
    fresh = all_raw(g)
    assert all(fresh[e] != after[e] for e in range(N)) and g.has_episode_budget()
    check_budget(g, want, "mv_reset")
    ticks(2, 0)
    assert all_raw(g)[1:] == fresh[1:] and raw(g, 0) != fresh[0]
    check_budget(g, want, "behind mv_reset")
    g.close()


# ---- 9. detach ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step", "step_n_16", "render_none"])
def test_detached_and_unlimited_equal_no_budget(hip, entry):
    """9. three gyms: one never had a budget, one had budget 1 attached and detached again, one carries -1 for every env.  16 ticks across an episode end
    of every env: the same rewards, dones, frames, slab, snapshots; the detached gym takes the launches of the gym that never had one"""
    family, A = "rearrange", 1
    outs = []
    for kind in ("never", "detached", "unlimited"):
        g = make(family, A, "fast")
        stagger(g, family, A)
        if kind == "detached":
            g.set_episode_budget(1)
            g.set_episode_budget(None)
            assert not g.has_episode_budget()
            with pytest.raises(RuntimeError, match="no episode budget"):
                g.episode_budget()
        if kind == "unlimited":
            g.set_episode_budget(-1)
        outs.append(run_entry(g, entry, "multidiscrete", A))
        if kind == "unlimited":
            check_budget(g, [-1] * N, "unlimited")
        g.close()
    never = outs[0]
    assert never["done"].sum(axis=0).tolist() == [1] * N
    for kind, out in zip(("detached", "unlimited"), outs[1:]):
        for key in ("rew", "done", "slab", "tobj"):
            assert out[key].tobytes() == never[key].tobytes(), (kind, key)
        assert out["snaps"] == never["snaps"] and out["consumed"] == never["consumed"], kind
        assert sorted(out["frames"]) == sorted(never["frames"]) and all(out["frames"][t].tobytes() == never["frames"][t].tobytes() for t in never["frames"]), kind
    assert outs[1]["launches"] == never["launches"]


# ---- 10. launch shape -------------------------------------------------------------------------------------------------------------------------------------
def test_launch_shape_1024_envs(hip):
    """10. TowerBuilding, 1024 envs x 32 x 32, one 16-tick render='none' call, every odd env with budget 0 and every even one unlimited.  Oracle E steps
    ticks 0..15; an even env is E's, an odd env the reset state of a fresh oracle.  Rewards and dones of every tick, every env's snapshot at the end"""
    import torch
    n, A, K, seed = 1024, 1, 16, 42
    even = np.arange(n) % 2 == 0
    g = MegaverseGym("TowerBuilding", W, H, n, A, 1, False, {})
    g.seed(seed)
    g.reset()
    rings = (torch.zeros((K, n * A), dtype=torch.float32, device="cuda:0"), torch.zeros((K, n), dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    g.set_output_ring(K, 0, rings[0].data_ptr(), rings[1].data_ptr())
    oracles = []
    for _ in range(2):
        og = oracle_lib.OracleGym("TowerBuilding", W, H, n, A, 1, False, {})
        og.seed(seed)
        og.reset()
        oracles.append(og)
    rew, done = np.zeros((K, n * A), np.float32), np.zeros((K, n), np.uint8)
    for j in range(K):
        oracles[0].set_action_masks(action_masks(sample_actions(B.POLICY_SEED, j, n * A)))
        oracles[0].step_norender()
        rew[j], done[j] = oracles[0].get_last_rewards(), oracles[0].get_dones()
    g.set_episode_budget(np.where(even, -1, 0).astype(np.int32))
    c0 = g.debug_launch_counts()
    g.step_n(K, "multidiscrete", B.POLICY_SEED, 0, render="none")
    assert g.debug_launch_counts()[0] - c0[0] == 2, "16 ticks are two step launches of 8"
    g.synchronize()
    assert rings[0].cpu().numpy().tobytes() == np.where(even[None], rew, np.float32(0.0)).astype(np.float32).tobytes(), "rewards"
    assert rings[1].cpu().numpy().tobytes() == np.where(even[None], done, np.uint8(0)).astype(np.uint8).tobytes(), "dones"
    for e in range(n):
        assert diff_snapshots(oracles[0 if even[e] else 1].snapshot(e), hip_snapshot(g, e), A) == [], f"env {e}"
    assert g.halted_count() == n // 2 and budget_of(g).tolist() == np.where(even, -1, 0).tolist()
    for og in oracles:
        og.close()
    g.close()


# ---- 11. refusals, before the first reset, arena bytes, the host form in a row, run_episodes ---------------------------------------------------------------
def test_refusals(hip):
    """11. a gym in a group; mv_group_create and mv_step_many with a budgeted member; a closed gym; wrong tensors (ValueError)"""
    import torch
    a, b = make_gym("TowerBuilding", 1, "fast"), make_gym("ObstaclesEasy", 1, "fast")
    lib = a._lib
    data = np.ones(N, np.int32)
    handles = (C.c_void_p * 2)(a._g, b._g)
    a.set_episode_budget(1)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == -1 and b"episode budget" in lib.mv_last_error()
    before = all_raw(a), all_raw(b)
    assert lib.mv_step_many(handles, 2, 1, 1, B.POLICY_SEED, 0) == -1 and b"episode budget" in lib.mv_last_error()
    assert (all_raw(a), all_raw(b)) == before, "mv_step_many stepped a gym before it refused"
    a.set_episode_budget(None)
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    out = C.c_int32()
    for g in (a, b):
        for fn in (lib.mv_set_episode_budget_host, lib.mv_set_episode_budget):
            assert fn(g._g, data.ctypes.data) == -1 and b"mv_group" in lib.mv_last_error()
        assert lib.mv_get_episode_budget(g._g) == 0 and not lib.mv_episode_budget_device_ptr(g._g) and not lib.mv_halted_count_device_ptr(g._g)
        with pytest.raises(RuntimeError, match="mv_group"):
            g.set_episode_budget(1)
    assert lib.mv_group_destroy(grp) == 0
    assert lib.mv_halted_count(a._g, C.byref(out)) == -1 and b"no episode budget" in lib.mv_last_error()
    for bad in (torch.zeros(N + 1, dtype=torch.int32, device="cuda:0"), torch.zeros(N, dtype=torch.int64, device="cuda:0"), torch.zeros(N, dtype=torch.int32),
                np.zeros(N - 1, np.int32), np.zeros(N, np.float32)):
        with pytest.raises(ValueError, match="set_episode_budget"):
            a.set_episode_budget(bad)
    assert not a.has_episode_budget()
    a.set_episode_budget(2)   # (valid again once the group is gone)
    handle = a._g
    lib.mv_close(handle)
    for fn in (lib.mv_set_episode_budget_host, lib.mv_set_episode_budget):
        assert fn(handle, data.ctypes.data) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_episode_budget(handle) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_halted_count(handle, C.byref(out)) == -1 and not lib.mv_episode_budget_device_ptr(handle)
    a.close(); b.close()


def test_before_the_first_reset_and_arena_bytes(hip):
    """11. the budget may be attached before the first mv_reset; its one allocation -- budgets, halted count, the log's mirror -- is counted in
    mv_arena_bytes from its first use and does not grow"""
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    bytes0 = g.arena_bytes()
    g.set_episode_budget([0, 1] * (N // 2))
    assert g.arena_bytes() == bytes0 + (2 * N + 1) * 4 and g.has_episode_budget()
    g.set_episode_budget(None)
    g.set_episode_budget([1, 0] * (N // 2))
    assert g.arena_bytes() == bytes0 + (2 * N + 1) * 4
    g.seed(11)
    g.reset()
    fresh = all_raw(g)
    g.set_actions_batched(B.actions(0, 1))
    step_ok(g)
    assert [raw(g, e) != fresh[e] for e in range(N)] == [True, False] * (N // 2)
    check_budget(g, [1, 0] * (N // 2), "one tick")
    g.close()


def test_host_form_many_times_without_a_synchronisation(hip):
    """11. the host form six times in a row with steps in flight and nothing synchronising (its pinned staging buffers are reused as their copies complete,
    asked for, never waited for): the last budget holds, every stepping call returns 0"""
    A = 1
    last = [0, -1, 3, 0, 0, -1, 1, 0]
    g, tw = make_gym("TowerBuilding", A, "fast"), make_gym("TowerBuilding", A, "fast")
    tw.set_episode_budget(last)
    for i in range(6):
        g.set_episode_budget([0, 1, -1][i % 3] if i < 5 else last)
    for t in range(4):
        for x in (g, tw):
            x.sample_random_actions(B.POLICY_SEED, t)
            step_ok(x)
        g.set_episode_budget(last)   # (again, between steps in flight)
    assert all_raw(g) == all_raw(tw)
    check_budget(g, last, "the last budget")
    g.close(); tw.close()


def test_run_episodes(hip):
    """11. MegaverseEnv.run_episodes(2), Sokoban with 65-tick episodes x 2 agents... one agent: exactly 2 N A records with the contents of the numpy model fed
    by a twin gym stepped tick by tick on the same policy, every env halted, the halted count read once per call"""
    U.boxoban_env()
    A, seed = 1, 11
    params = {"episodeLengthSec": 4.3}
    env = MegaverseEnv("Sokoban", N, A, params=params, img_w=W, img_h=H)
    env.seed(seed)
    env.reset()
    reads = []
    count = env.env.halted_count
    env.env.halted_count = lambda: reads.append(1) or count()
    records = env.run_episodes(2, seed=B.POLICY_SEED)
    assert env.halted().cpu().tolist() == [True] * N and env.env.halted_count() == N
    calls = -(-130 // env.env.recommended_ticks_per_call())
    assert len(reads) == calls + 1, f"{len(reads) - 1} reads of the halted count in {calls} calls"
    tw = make_gym("Sokoban", A, "fast", params, seed=seed)
    tw.set_episode_budget(2)
    model = BudgetModel(N, A)
    model.attach([2] * N)
    for t in range(130):
        tw.sample_random_actions(B.POLICY_SEED, t)
        assert tw._lib.mv_step_no_render(tw._g) == 0
        model.feed(tw.get_rewards_array()[None], tw.get_dones()[None], tw.get_true_objectives()[None])
    assert model.left.tolist() == [0] * N
    want = model.drain()
    assert len(records) == 2 * N * A == len(want) and records.tobytes() == want.tobytes()
    assert records["length"].tolist() == [65] * (2 * N)
    tw.close()
    env.close()
