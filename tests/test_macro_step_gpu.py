"""Macro steps on the GPU (include/megaverse_hip.h: mv_macro_step): one decision held for up to k ticks, every env stops at its own first done, one summed
reward, one done and one frame per call.

8 envs, 32 x 32 frames (tests/reset_envs_util.py).  Expected values come from the CPU oracle as it is -- env e of the gym is env e of an oracle that stepped
on exactly the gym ticks env e stepped in, holding the decision's action and summing in float32 (the wrapper loop a macro step replaces) -- or from twin gyms
that take a path of the library earlier tests pin: the composition of budget 1, an action ring of one entry and an MV_RENDER_LAST call, or mv_step tick by
tick under a step mask the host rewrites.  The envs' clocks are staggered first (tests/episode_budget_util.py), so that their episodes end on different ticks
of the calls that follow.  Every comparison is equality of bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_budget_util as B
import episode_log_util as U
import macro_step_util as M
import state_obs_util as S
from hip_util import hip_snapshot
from macro_step_util import H, N, W
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.megaverse_env import MegaverseEnv
from megaverse_amd.rollout import action_masks
from test_episode_budget_gpu import EXTRA, stagger
from test_reset_envs_gpu import all_raw, check_env, slab

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
CLOCK_FAMILIES = ("rearrange", "sokoban", "football", "empty")   # episodes exactly as long as episodeLengthSec says (65 ticks): where dones fall is known


def make(family, A, mode="fast", log=0, layout="rgba"):
    scenario, params, _, seed = B.FAMILIES[family]
    U.boxoban_env()
    g = MegaverseGym(scenario, W, H, N, A, 1, False, dict(params))
    g.set_pixel_mode(mode)
    if layout != "rgba":
        g.set_obs_layout(layout)
    g.seed(seed)
    if log:
        g.set_episode_log(log)
    g.reset()
    return g


def held(c, A):
    """the action decision c holds: int32 [N*A][6]"""
    return np.ascontiguousarray(B.actions(100000 + c, A), np.int32).reshape(N * A, 6)


def outputs(g):
    return g.get_rewards_array().copy(), g.get_dones().copy(), g.get_true_objectives().copy()


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------------------------
# the calls behind the stagger.  With budget-1 halting ticks (7, 8, 2, 3, 4, 5, 6, 9) relative to the stagger's end, the first call (k = 11: more than a
# launch of 8 ticks) sees dones on its ticks 7 and 8 and inside both launches; the envs then wait for the call's end and go on in step, 65-tick episodes ending
# 64 ticks later: on the LAST tick of the third call and on the FIRST tick of the sixth (the clock families; checked on the oracle's walk, not assumed)
DECISIONS = (11, 4, 61, 4, 60, 4)


@functools.lru_cache(maxsize=None)
def oracle_decisions(family, A, e, delay, TA):
    """env e: an oracle steps the stagger's ticks (frozen for the first `delay`), then runs the wrapper loop per decision -- hold the action, sum in float32,
    break at done -> [(capture behind the decision with the summed rewards and the done, the call's tick that finished the episode or None)]"""
    scenario = B.FAMILIES[family][0]
    og = B.new_oracle(family, A)
    for t in range(delay, TA):
        og.set_action_masks(action_masks(B.actions(t, A)))
        og.step_norender()
    out = []
    for c, k in enumerate(DECISIONS):
        masks = action_masks(held(c, A))
        total, done_at = None, None
        for j in range(k):
            og.set_action_masks(masks)
            og.step_norender()
            r = og.get_last_rewards().astype(np.float32)
            total = r.copy() if total is None else (total + r).astype(np.float32)
            if og.get_dones()[e]:
                done_at = j
                break
        og.render_env(e)
        cap = B.capture(og, scenario, A, e)
        cap["rewards"] = total
        cap["dones"] = np.full(N, 1 if done_at is not None else 0, np.uint8)
        out.append((cap, done_at))
    og.close()
    return out


@pytest.mark.parametrize("family", B.ORACLE_FAMILIES)
def test_against_the_oracle(hip, family):
    """1. decision for decision: summed rewards and dones bit for bit, mv_debug_snapshot state, the scenario's own state, true objectives and the
    MV_RENDER_LAST frames in exact mode, for every env -- none is left out"""
    A = 1
    scenario = B.FAMILIES[family][0]
    TA, delays = B.stagger_plan(family, A)
    walks = [oracle_decisions(family, A, e, delays[e], TA) for e in range(N)]
    finished = [[w[c][1] for w in walks] for c in range(len(DECISIONS))]
    # (where the endings follow the actions -- BoxAGone -- the held actions move them: some call, not necessarily the first)
    assert any(d is not None and 0 < d < k - 1 for row, k in zip(finished, DECISIONS) for d in row), f"{family}: no env finishes inside a call: {finished}"
    if family in CLOCK_FAMILIES:
        assert {7, 8} <= set(finished[0]) and any(d is not None and 0 < d < 7 for d in finished[0]), finished[0]
        assert set(finished[2]) == {DECISIONS[2] - 1} and set(finished[5]) == {0}, (finished[2], finished[5])
    g = make(family, A, "exact")
    assert stagger(g, family, A) == TA
    ticks0 = g.ticks_since_reset() if hasattr(g, "ticks_since_reset") else None
    for c, k in enumerate(DECISIONS):
        g.macro_step(k, held(c, A), render="last")
        for e in range(N):
            check_env(g, walks[e][c][0], scenario, A, e, f"{family}, decision {c} (k = {k}; the env finished on tick {walks[e][c][1]})")
    if ticks0 is not None:
        assert g.ticks_since_reset() == ticks0 + sum(DECISIONS)
    g.close()


# ---- 2. against the existing composition --------------------------------------------------------------------------------------------------------------------
def composition_decision(g, k, acts, A):
    """budget 1 re-attached, an action ring of one entry, k ticks into rings of k with the last one drawn, a numpy fold -> (rewards, dones)"""
    import torch
    a = torch.as_tensor(acts).to("cuda:0")
    rew = torch.zeros((k, N * A), dtype=torch.float32, device="cuda:0")
    done = torch.zeros((k, N), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.set_episode_budget(1)
    g.set_action_ring(1, a.data_ptr())
    g.set_output_ring(k, 0, rew.data_ptr(), done.data_ptr())
    g.step_n(k, "sequence", 0, 0, render="last")
    g.synchronize(); torch.cuda.synchronize()
    g.set_output_ring(0)
    g.set_action_ring(0)
    return M.fold(rew.cpu().numpy()), done.cpu().numpy().any(axis=0).astype(np.uint8)


@pytest.mark.parametrize("layout", ["rgba", "chw"])
@pytest.mark.parametrize("family", sorted(B.FAMILIES))
def test_against_the_composition(hip, family, layout):
    """2. a twin of the same seed runs what a caller composes today; reward, done, true objectives, last frame, snapshots and the drained episode log are the
    twin's byte for byte, for k = 11 (over the staggered episode ends), 4 and 1, in the default (fast) pixel mode"""
    A = 1
    gm, gc = make(family, A, log=256, layout=layout), make(family, A, log=256, layout=layout)
    for g in (gm, gc):
        stagger(g, family, A, EXTRA.get(family, 0))
    any_done = False
    for c, k in enumerate((11, 4, 1, 4, 11, 1)):
        acts = held(c, A)
        gm.macro_step(k, acts, render="last")
        rew, done = composition_decision(gc, k, acts, A)
        what = f"{family}, {layout}, decision {c} (k = {k})"
        got = outputs(gm)
        assert got[0].tobytes() == rew.tobytes(), f"{what}: rewards"
        assert got[1].tobytes() == done.tobytes(), f"{what}: dones"
        assert got[2].tobytes() == gc.get_true_objectives().tobytes(), f"{what}: true objectives"
        assert slab(gm, A).tobytes() == slab(gc, A).tobytes(), f"{what}: the last frame"
        assert all_raw(gm) == all_raw(gc), f"{what}: snapshots"
        any_done = any_done or bool(done.any())
    assert any_done, f"{family}: no env finished inside a call"
    a, b = gm.drain_episode_log(), gc.drain_episode_log()
    assert len(a) > 0 and a.tobytes() == b.tobytes(), f"{family}: the episode logs"
    assert not gm.has_episode_budget()
    gm.close(); gc.close()


# ---- 3. per-env durations; 4. composition: the tick-by-tick emulation ------------------------------------------------------------------------------------------
def emulated_decision(g, k, acts, ticks, mask):
    """mv_step tick by tick under a step mask the host rewrites from the dones it reads back: the rule, applied by the caller
    -> (summed rewards, dones, per-tick (rewards, dones, true objectives))"""
    tl = np.full(N, k, np.int64) if ticks is None else np.clip(np.asarray(ticks, np.int64), 0, k)
    on = np.ones(N, bool) if mask is None else np.asarray(mask) != 0
    total, dones, per_tick = None, np.zeros(N, np.uint8), []
    for j in range(k):
        steps = on & (tl > 0)
        g.set_step_mask(steps)
        g.set_actions_batched(acts)
        rc = g._lib.mv_step(g._g) if j == k - 1 else g._lib.mv_step_no_render(g._g)
        assert rc == 0, g._lib.mv_last_error()
        r, d, o = outputs(g)
        per_tick.append((r, d, o))
        total = r.copy() if total is None else (total + r).astype(np.float32)
        dones |= (d != 0).astype(np.uint8)
        tl = np.where(steps, np.where(d != 0, 0, tl - 1), tl)
    g.set_step_mask(mask)
    return total, dones, per_tick


def against_the_emulation(family, A, decisions, mask=None, budget=None, draw=None, log=0, state=False, extra_check=None):
    """decisions: [(k, ticks or None)].  The macro gym and the emulating twin share seed, stagger, step mask, budget and draw mask."""
    gm, ge = make(family, A, log=log), make(family, A, log=log)
    buf = None
    for g in (gm, ge):
        stagger(g, family, A, EXTRA.get(family, 0))
        if budget is not None:
            g.set_episode_budget(np.asarray(budget, np.int32))
        if draw is not None:
            g.set_draw_mask(np.asarray(draw, bool))
    if mask is not None:
        gm.set_step_mask(np.asarray(mask, bool))
    if state:
        buf = gm.set_state_obs(True)
    finished = 0
    for c, (k, ticks) in enumerate(decisions):
        acts = held(c, A)
        before = all_raw(gm)
        gm.macro_step(k, acts, ticks=None if ticks is None else np.asarray(ticks, np.int32), render="last")
        rew, done, _ = emulated_decision(ge, k, acts, ticks, mask)
        what = f"{family} x {A}, decision {c} (k = {k}, ticks = {ticks})"
        got = outputs(gm)
        assert got[0].tobytes() == rew.tobytes(), f"{what}: rewards"
        assert got[1].tobytes() == done.tobytes(), f"{what}: dones"
        assert got[2].tobytes() == ge.get_true_objectives().tobytes(), f"{what}: true objectives"
        assert slab(gm, A).tobytes() == slab(ge, A).tobytes(), f"{what}: the last frame"
        after = all_raw(gm)
        assert after == all_raw(ge), f"{what}: snapshots"
        still = [e for e in range(N) if (ticks is not None and ticks[e] <= 0) or (mask is not None and not mask[e])]
        for e in still:
            assert after[e] == before[e], f"{what}: env {e} does not step and changed"
            assert not got[0][e * A:(e + 1) * A].any() and not got[1][e], f"{what}: env {e} does not step and reports"
        if budget is not None:
            assert gm.episode_budget().cpu().numpy().tolist() == ge.episode_budget().cpu().numpy().tolist(), f"{what}: budgets"
            assert gm.halted_count() == ge.halted_count(), f"{what}: halted count"
        if state:
            import torch
            gm.synchronize(); torch.cuda.synchronize()
            rows = buf.cpu().numpy().reshape(-1, N * A, 16)[0]
            want = S.rows_of_gym_snapshots(lambda e: hip_snapshot(gm, e), N, A)
            assert rows.view(np.uint32).tolist() == np.asarray(want).view(np.uint32).reshape(N * A, 16).tolist(), f"{what}: state observations"
        finished += int(done.sum())
        if extra_check:
            extra_check(gm, ge, c)
    assert finished > 0, f"{family}: no env finished inside a call"
    if log:
        a, b = gm.drain_episode_log(), ge.drain_episode_log()
        assert len(a) > 0 and a.tobytes() == b.tobytes(), f"{family}: the episode logs"
    assert gm.ticks_since_reset() == ge.ticks_since_reset()
    gm.close(); ge.close()


K3 = 6
TICKS3 = [0, 1, K3, K3 + 5, 2, 3, 0, K3]


@pytest.mark.parametrize("family", ["sokoban", "tower_long"])
def test_per_env_durations(hip, family):
    """3. ticks = [0, 1, k, k + 5, ...]: every env holds its action for its own number of ticks; an env with ticks = 0 keeps every byte of its snapshot"""
    against_the_emulation(family, 1, [(K3, TICKS3), (11, [11, 0, 3, 12, 8, 9, 1, -4]), (K3, None), (K3, TICKS3[::-1])])


def test_with_a_step_mask(hip):
    """4. envs 1 and 4 frozen by a step mask: they do not step in any call and keep their ticks; the others follow the rule"""
    mask = np.ones(N, bool)
    mask[[1, 4]] = False
    against_the_emulation("rearrange", 1, [(11, None), (4, TICKS3), (4, None)], mask=mask)


def test_with_a_user_budget_of_two(hip):
    """4. a budget of 2 is spent ACROSS macro steps: each env's two episodes end in different calls, then it halts for good"""
    decisions = [(11, None)] + [(16, None)] * 9
    against_the_emulation("football", 2, decisions, budget=[2] * N)
    g = make("football", 2)
    stagger(g, "football", 2)
    g.set_episode_budget(2)
    lefts = []
    for c, (k, _) in enumerate(decisions):
        g.macro_step(k, held(c, 2), render="none")
        lefts.append(g.episode_budget().cpu().numpy().tolist())
    assert lefts[0] == [1] * N and lefts[-1] == [0] * N and g.halted_count() == N, lefts
    assert any(1 in l and 0 in l for l in lefts) or lefts.index([0] * N) > 1
    before = all_raw(g)
    g.macro_step(4, held(99, 2), render="last")
    r, d, _ = outputs(g)
    assert all_raw(g) == before and not r.any() and not d.any(), "a halted env stepped"
    g.close()


def test_with_a_draw_mask(hip):
    """4. undrawn envs' rows keep what they held; everything else about the call is unchanged"""
    draw = np.ones(N, bool)
    draw[[0, 5]] = False
    against_the_emulation("sokoban", 1, [(11, None), (4, None)], draw=draw)


def test_with_state_observations(hip):
    """4. the call's one entry holds every agent's row behind the call's last tick: the pack of the snapshot after the call"""
    against_the_emulation("rearrange", 1, [(11, None), (4, TICKS3), (1, None)], state=True)


def test_with_the_episode_log(hip):
    """4. the log with the mirror of the ticks left: the twin's log (every tick a call of its own under a step mask), and the numpy model fed with the twin's
    per-tick outputs, record for record"""
    family, A = "rearrange", 1
    decisions = [(11, None), (4, TICKS3), (61, None), (4, None)]
    against_the_emulation(family, A, decisions, log=256)
    gm, ge = make(family, A), make(family, A)
    for g in (gm, ge):
        stagger(g, family, A)
    gm.set_episode_log(256)   # (switched on behind the stagger: returns and lengths count from here, as the model's do)
    model = M.MacroModel(N, A, capacity=256)
    model.tick = gm.ticks_since_reset()
    for c, (k, ticks) in enumerate(decisions):
        gm.macro_step(k, held(c, A), ticks=None if ticks is None else np.asarray(ticks, np.int32), render="none")
        _, _, per_tick = emulated_decision(ge, k, held(c, A), ticks, None)
        r, d, o = (np.stack([p[i] for p in per_tick]) for i in range(3))
        model.feed_macro(r, d, o, ticks)
    got, want = gm.drain_episode_log(), model.drain()
    assert len(got) == len(want) > 0 and got.tobytes() == want.astype(got.dtype).tobytes(), "the log against the numpy model"
    gm.close(); ge.close()


def test_tower_with_four_agents(hip):
    """4. TowerBuilding at four agents per env: every wave of the workgroup keeps the env's ticks left and takes the same side of the per-tick choice"""
    against_the_emulation("tower_long", 4, [(11, None), (K3, TICKS3), (4, None)])


# ---- 5. output ring ---------------------------------------------------------------------------------------------------------------------------------------------
def test_output_ring(hip):
    """5. sixteen macro steps into a ring of 16 fill entries 0 .. 15 in order -- a step_n(3) in between advances the position by 3 -- and render='none' writes
    no byte of the slab or of the ring's frames"""
    import torch
    family, A, R = "sokoban", 1, 16
    ga, gb = make(family, A), make(family, A)
    for g in (ga, gb):
        stagger(g, family, A)
    obs = torch.full((R, N * A, H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda:0")
    rew = torch.full((R, N * A), -7.0, dtype=torch.float32, device="cuda:0")
    done = torch.full((R, N), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ga.set_output_ring(R, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
    want, entry = {}, 0
    for c in range(13):
        if c == 5:
            for g in (ga, gb):
                g.step_n(3, "multidiscrete", B.POLICY_SEED, 0)
            entry += 3
            want[entry - 1] = outputs(gb)[:2] + (slab(gb, A),)
        k = (11, 4, 1)[c % 3]
        for g in (ga, gb):
            g.macro_step(k, held(c, A), render="last")
        want[entry] = outputs(gb)[:2] + (slab(gb, A),)
        entry += 1
    assert entry == R
    ga.synchronize(); torch.cuda.synchronize()
    o, r, d = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    assert sorted(want) == [0, 1, 2, 3, 4] + list(range(7, 16))
    for i, (wr, wd, wo) in want.items():
        assert r[i].tobytes() == wr.tobytes() and d[i].tobytes() == wd.tobytes(), f"ring entry {i}: rewards / dones"
        assert o[i].tobytes() == wo.tobytes(), f"ring entry {i}: frames"
    assert all_raw(ga) == all_raw(gb)
    # render = 'none': the next two entries' frames (0 and 1 again) and the slab keep every byte
    obs.fill_(SENTINEL)
    torch.cuda.synchronize()
    for c in range(2):
        ga.macro_step(4, held(50 + c, A), render="none")
        gb.macro_step(4, held(50 + c, A), render="none")
    ga.synchronize(); torch.cuda.synchronize()
    assert (obs.cpu().numpy() == SENTINEL).all(), "render='none' wrote into the ring's frames"
    assert rew.cpu().numpy()[1].tobytes() == gb.get_rewards_array().tobytes()
    ga.close(); gb.close()
    g = make(family, A)
    sl = torch.full((N * A, H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.set_obs_buffer(sl.data_ptr())
    g.macro_step(11, held(0, A), render="none")
    g.synchronize(); torch.cuda.synchronize()
    assert (sl.cpu().numpy() == SENTINEL).all(), "render='none' wrote into the slab"
    g.close()


# ---- 6. MegaverseEnv(frame_skip = 4) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,length", [("step", 1.0), ("step_batched", 1.0), ("step_device", 4.3)])
def test_env_frame_skip(hip, method, length):
    """6. step / step_batched / step_device of MegaverseEnv(frame_skip=4) against frame_skip=1 stepped in a Python loop with the per-env break (the envs that
    finished wait under a step mask).  Episodes of 1 s are stepped tick by tick by the library, those of 4.3 s in resident launches."""
    import torch
    from megaverse_amd import rl
    K, n, A = 4, 4, 2
    envs = [MegaverseEnv("Rearrange", n, A, params={"episodeLengthSec": length}, img_w=W, img_h=H, frame_skip=fs) for fs in (K, 1)]
    for env in envs:
        env.seed(11)
        env.reset()
    e4, e1 = envs
    finished = 0
    for c in range(20 if length > 2 else 8):
        acts = np.ascontiguousarray(B.actions(7000 + c, A)[:n * A], np.int32).reshape(n * A, 6)
        if method == "step":
            obs, rew, dones, infos = e4.step(acts.tolist())
            got = (np.stack(obs), np.asarray(rew, np.float32), np.asarray(dones, bool)[::A])
        elif method == "step_batched":
            obs, rew, dones = e4.step_batched(acts)
            got = (obs.cpu().numpy(), rew.copy(), dones.copy())
        else:
            obs, rew, dones = e4.step_device(torch.as_tensor(acts).to("cuda:0"))
            e4.env.synchronize(); torch.cuda.synchronize()
            got = (obs.cpu().numpy(), rew.cpu().numpy(), dones.cpu().numpy() != 0)
        active, total, done = np.ones(n, bool), None, np.zeros(n, bool)
        for j in range(K):
            e1.set_step_mask(active)
            o, r, d = e1.step_batched(acts)
            total = r.copy() if total is None else (total + r).astype(np.float32)
            done |= d
            active &= ~d
        e1.set_step_mask(None)
        what = f"{method}, decision {c}"
        assert got[1].tobytes() == total.tobytes(), f"{what}: rewards"
        assert got[2].tolist() == done.tolist(), f"{what}: dones"
        assert got[0].tobytes() == o.cpu().numpy().tobytes(), f"{what}: observations"
        finished += int(done.sum())
    assert finished > 0
    for env in envs:
        env.close()
    w = rl.make_megaverse("Rearrange", img_w=W, img_h=H, frame_skip=K)
    assert w.frame_skip == K and w.env.frame_skip == K
    w.close()
    w = rl.make_megaverse("Rearrange", img_w=W, img_h=H)
    assert w.frame_skip == 1
    w.close()


# ---- 7. the device form behind a kernel ---------------------------------------------------------------------------------------------------------------------------
def test_device_form_behind_a_kernel(hip):
    """7. actions and ticks written by kernels on the gym's stream into ONE buffer each, rewritten in front of every call, 20 calls, nothing synchronising in
    between: the results in a ring of 20 equal the host form's"""
    import torch
    family, A, CALLS, K = "sokoban", 1, 20, 4
    gd, gh = make(family, A), make(family, A)
    for g in (gd, gh):
        stagger(g, family, A)
    acts = np.stack([held(c, A) for c in range(CALLS)])
    ticks = np.stack([np.roll(np.array(TICKS3, np.int32), c) for c in range(CALLS)])
    src_a, src_t = torch.as_tensor(acts).to("cuda:0"), torch.as_tensor(ticks).to("cuda:0")
    a, t = torch.zeros((N * A, 6), dtype=torch.int32, device="cuda:0"), torch.zeros(N, dtype=torch.int32, device="cuda:0")
    rew = torch.full((CALLS, N * A), -7.0, dtype=torch.float32, device="cuda:0")
    done = torch.full((CALLS, N), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gd.set_output_ring(CALLS, 0, rew.data_ptr(), done.data_ptr())
    for c in range(CALLS):
        torch.add(src_a[c], 0, out=a)   # (were the buffers read before these kernels have run, call c would act on call c - 1's values)
        torch.add(src_t[c], 0, out=t)
        gd.macro_step(K, a, ticks=t, render="last" if c == CALLS - 1 else "none")
    want = []
    for c in range(CALLS):
        gh.macro_step(K, acts[c], ticks=ticks[c], render="last" if c == CALLS - 1 else "none")
        want.append(outputs(gh)[:2])
    gd.synchronize(); torch.cuda.synchronize()
    assert rew.cpu().numpy().tobytes() == np.stack([w[0] for w in want]).tobytes(), "rewards of the 20 calls"
    assert done.cpu().numpy().tobytes() == np.stack([w[1] for w in want]).tobytes(), "dones of the 20 calls"
    assert all_raw(gd) == all_raw(gh) and slab(gd, A).tobytes() == slab(gh, A).tobytes()
    assert np.stack([w[1] for w in want]).any(), "no env finished"
    gd.close(); gh.close()


# ---- 8. a gym that never calls it -----------------------------------------------------------------------------------------------------------------------------------
def test_a_gym_that_never_calls_it(hip):
    """8. (a guard: passes without the feature too) launch counts and a 32-tick step_n rollout of a gym that never makes a macro step are a fresh gym's --
    also beside a gym that does"""
    import torch
    family, A = "tower_long", 1
    outs = []
    for other in (False, True):
        g = make(family, A)
        if other:
            busy = make(family, A)
            busy.macro_step(11, held(0, A))
        obs = torch.zeros((32, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0")
        rew = torch.zeros((32, N * A), dtype=torch.float32, device="cuda:0")
        done = torch.zeros((32, N), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        g.set_output_ring(32, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
        c0 = g.debug_launch_counts()
        for q in range(2):
            g.step_n(16, "multidiscrete", B.POLICY_SEED, 16 * q)
        g.synchronize(); torch.cuda.synchronize()
        c1 = g.debug_launch_counts()
        outs.append(((c1[0] - c0[0], c1[1] - c0[1]), obs.cpu().numpy().tobytes(), rew.cpu().numpy().tobytes(), done.cpu().numpy().tobytes(), all_raw(g),
                     g.arena_bytes() if hasattr(g, "arena_bytes") else 0))
        g.close()
        if other:
            busy.close()
    assert outs[0] == outs[1]


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import torch
    A = 1
    lib = None
    U.boxoban_env()
    fresh = MegaverseGym("Sokoban", W, H, N, A, 1, False, {})
    lib = fresh._lib
    acts = held(0, A)
    with pytest.raises(RuntimeError, match="mv_reset first"):
        fresh.macro_step(4, acts)
    fresh.close()
    g = make("sokoban", A)
    before = all_raw(g)
    with pytest.raises(RuntimeError, match="MV_RENDER_EVERY"):
        g.macro_step(4, acts, render="every")
    assert lib.mv_macro_step_host(g._g, 4, acts.ctypes.data, None, 0) == -1 and b"MV_RENDER_EVERY" in lib.mv_last_error()
    assert lib.mv_macro_step_host(g._g, 4, acts.ctypes.data, None, 7) == -1 and b"render mode" in lib.mv_last_error()
    for k in (0, -3):
        with pytest.raises(RuntimeError, match="k >= 1"):
            g.macro_step(k, acts)
    assert lib.mv_macro_step_host(g._g, 4, None, None, 1) == -1 and b"null actions" in lib.mv_last_error()
    assert lib.mv_macro_step(g._g, 4, None, None, 1) == -1 and b"null actions" in lib.mv_last_error()
    for bad in (np.zeros((N * A, 5), np.int32), np.zeros((N * A + 1, 6), np.int32), torch.zeros((N * A, 6), dtype=torch.int64, device="cuda:0"),
                torch.zeros((N * A, 6), dtype=torch.int32)):
        with pytest.raises(ValueError):
            g.macro_step(4, bad)
    with pytest.raises(ValueError):
        g.macro_step(4, acts, ticks=np.zeros(N + 1, np.int32))
    with pytest.raises(ValueError):
        g.macro_step(4, acts, ticks=torch.zeros(N, dtype=torch.int32, device="cuda:0"))   # (host actions, device ticks)
    assert all_raw(g) == before, "a refused call changed the gym"
    other = make("sokoban", A)
    handles = (C.c_void_p * 2)(g._g, other._g)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    with pytest.raises(RuntimeError, match="mv_group"):
        g.macro_step(4, acts)
    assert lib.mv_group_destroy(grp) == 0
    g.macro_step(4, acts)   # (valid again once the group is gone)
    g.synchronize()
    handle = g._g
    lib.mv_close(handle)
    assert lib.mv_macro_step_host(handle, 4, acts.ctypes.data, None, 1) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_macro_step(handle, 4, acts.ctypes.data, None, 1) == -1 and b"closed" in lib.mv_last_error()
    g.close(); other.close()
