"""Masked env resets on the GPU (include/megaverse_hip.h: mv_reset_envs): the envs a mask flags leave their episode and take the next one of their own sequence.

Every test uses 8 envs and 32 x 32 frames (tests/reset_envs_util.py) and the masks {env 0, env 3, env 7} and its complement unless it says otherwise.  Expected
values come from the CPU oracle -- an env's episode sequence depends on its own seed chain only, so a flagged env must be the env of an oracle gym that was
reset as a whole at that tick, and an unflagged env the env of one that was not -- or from twin gyms that take another path to the same state.  No env, tick
or byte is left out of a comparison."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_log_util as U
import oracle_lib
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions
from reset_envs_util import COMPLEMENT, H, MASK, MASKS, N, W, CutModel, mask_of

pytestmark = pytest.mark.gpu

ENV_SEED, POLICY_SEED = 42, 1234
T0, T_AFTER = 7, 12


def make_gym(scenario, A, mode, params=None, seed=ENV_SEED, log=0, threads=1):
    U.boxoban_env()
    g = MegaverseGym(scenario, W, H, N, A, threads, False, params or {})
    g.set_pixel_mode(mode)
    g.seed(seed)
    if log:
        g.set_episode_log(log)
    g.reset()
    return g


def act(g, A, t):
    g.set_actions_batched(sample_actions(POLICY_SEED, t, N * A))


def raw(g, e):
    return g.debug_snapshot_bytes(e).tobytes()


def all_raw(g):
    return [raw(g, e) for e in range(N)]


def slab(g, A):
    return np.stack([g.get_observation(e, a) for e in range(N) for a in range(A)])


def device_mask(mask):
    """the mask as a torch.bool CUDA tensor, written by a kernel on the gym's stream (torch's current one: the null stream)"""
    import torch
    src = torch.as_tensor(np.asarray(mask, np.bool_)).to("cuda:0")
    out = torch.zeros(N, dtype=torch.bool, device="cuda:0")
    torch.cuda.synchronize()
    torch.logical_or(src, src, out=out)
    return out


# ---- 1. against the oracle, every scenario family ------------------------------------------------------------------------------------------------------
ORACLE_CASES = {"tower_a1": ("TowerBuilding", 1), "tower_a2": ("TowerBuilding", 2), "obstacles_easy": ("ObstaclesEasy", 1), "collect": ("Collect", 1),
                "rearrange": ("Rearrange", 1), "sokoban": ("Sokoban", 1), "hex_memory": ("HexMemory", 1), "boxagone": ("BoxAGone", 1),
                "empty": ("Empty", 1), "football": ("Football", 2)}   # (Football against its generator's episodes and twin gyms too: test_masked_reset_football below)


def capture(og, scenario, A):
    out = {"snap": [og.snapshot(e) for e in range(N)], "rewards": og.get_last_rewards().copy(), "dones": og.get_dones().copy(),
           "tobj": np.array([og.true_objective(e, a) for e in range(N) for a in range(A)], np.float32),
           "frames": np.stack([og.get_observation(e, a).copy() for e in range(N) for a in range(A)])}
    if scenario == "BoxAGone":
        out["bag"] = [og.boxagone_state(e) for e in range(N)]
    if scenario == "Football":
        out["ball"] = [og.football_state(e) for e in range(N)]
    return out


@functools.lru_cache(maxsize=None)
def oracle_reference(scenario, A, resets=1, ticks_after=T_AFTER):
    """oracle P steps T0 ticks and goes on; oracle Q steps T0 ticks, calls reset() `resets` times, and goes on: [(P, Q) right behind the reset, then behind
    each of ticks_after more ticks] -- with resets > 1 preceded by (None, Q) behind each earlier reset -- computed once per scenario and shared by the masks"""
    U.boxoban_env()
    pq = []
    for _ in range(2):
        og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, {})
        og.seed(ENV_SEED)
        og.reset()
        pq.append(og)
    P, Q = pq
    for t in range(T0):
        m = action_masks(sample_actions(POLICY_SEED, t, N * A))
        for og in pq:
            og.set_action_masks(m)
            og.step_norender()
    P.render()
    out = []
    for r in range(resets):
        Q.reset()
        if r < resets - 1:
            out.append((None, capture(Q, scenario, A)))
    out.append((capture(P, scenario, A), capture(Q, scenario, A)))
    for t in range(T0, T0 + ticks_after):
        m = action_masks(sample_actions(POLICY_SEED, t, N * A))
        for og in pq:
            og.set_action_masks(m)
            og.step()
        out.append((capture(P, scenario, A), capture(Q, scenario, A)))
    P.close(); Q.close()
    return out


def check_env(hg, ref, scenario, A, e, what):
    """env e of the gym == env e of an oracle capture: state, reward bit patterns, done, true objectives, exact pixels"""
    assert diff_snapshots(ref["snap"][e], hip_snapshot(hg, e), A) == [], f"{what}: state of env {e}"
    if scenario == "BoxAGone":
        import boxagone_model as M
        so, sh = ref["bag"][e], hg.debug_boxagone_state(e).view(M.STATE)[0]
        bad = [n for n in M.STATE.names if so[n].tobytes() != sh[n].tobytes()]
        assert not bad, f"{what}: BoxAGone state of env {e}: {bad}"
    if scenario == "Football":
        from football_cases import record
        so, sh = ref["ball"][e], record(hg.debug_football_state(e))
        assert so.tobytes() == sh.tobytes(), f"{what}: Football's ball of env {e}: {so} vs {sh}"
    rew, done, tobj = hg.get_rewards_array(), hg.get_dones(), hg.get_true_objectives()
    s = slice(e * A, (e + 1) * A)
    assert rew[s].view(np.uint32).tolist() == ref["rewards"][s].view(np.uint32).tolist(), f"{what}: rewards of env {e}"
    assert int(done[e]) == int(ref["dones"][e]), f"{what}: done of env {e}"
    assert tobj[s].view(np.uint32).tolist() == ref["tobj"][s].view(np.uint32).tolist(), f"{what}: true objectives of env {e}"
    for a in range(A):
        assert np.array_equal(hg.get_observation(e, a), ref["frames"][e * A + a]), f"{what}: frame of env {e}, agent {a}"


@pytest.mark.parametrize("mask_name", sorted(MASKS))
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_masked_reset_against_the_oracle(hip, case, mask_name):
    """1. T0 = 7 ticks, reset_envs(mask) in the host form with render, 12 more ticks; right behind the reset and behind every later tick a flagged env is
    the env of the oracle that was reset at tick 7 and an unflagged env the env of the oracle that was not: snapshot, rewards, dones, true objectives,
    exact-mode pixels -- every env, every tick"""
    scenario, A = ORACLE_CASES[case]
    mask = MASKS[mask_name]
    ref = oracle_reference(scenario, A)
    assert ref[0][0]["snap"][0].tobytes() != ref[0][1]["snap"][0].tobytes(), "the oracle's reset changed nothing: the test would prove nothing"
    hg = make_gym(scenario, A, "exact")
    for t in range(T0):
        act(hg, A, t)
        hg.step()
    hg.reset_envs(mask, render=True)
    for j in range(T_AFTER + 1):
        if j > 0:
            act(hg, A, T0 + j - 1)
            hg.step()
        P, Q = ref[j]
        for e in range(N):
            check_env(hg, Q if mask[e] else P, scenario, A, e, f"{case}, {mask_name}, {'the reset' if j == 0 else f'tick {T0 + j - 1}'}")
    assert hg.ticks_since_reset() == T0 + T_AFTER
    hg.close()


def football_state(g, e):
    st = g.debug_football_state(e)
    return b"".join(np.asarray(st[k]).tobytes() for k in ("pos", "radius", "vel", "kicks", "ang", "contacts", "force"))


@pytest.mark.parametrize("mask_name", sorted(MASKS))
def test_masked_reset_football(hip, mask_name):
    """1, Football, beside its oracle case above: the references from before the oracle knew the scenario -- right behind the reset a flagged env is
    the SECOND episode tests/football_model.py generates from that env's seed stream, ball
    at rest in its reset state (the check test_football_gpu.py makes of a fresh episode); and behind the reset and every one of the 12 later ticks a flagged
    env is, byte for byte, the env of a twin gym that was reset as a whole at tick 7 and an unflagged env the env of a twin that was left alone: snapshot,
    ball state, rewards, dones, true objectives, exact-mode pixels"""
    import football_model as M
    from test_football_gpu import check_fresh, env_streams, state
    A, mask = 1, MASKS[mask_name]
    gM, gR, gU = (make_gym("Football", A, "exact") for _ in range(3))
    for t in range(T0):
        for g in (gM, gR, gU):
            act(g, A, t)
            g.step()
    gM.reset_envs(mask, render=True)
    gR.reset()
    streams = env_streams(ENV_SEED, N)
    for e in range(N):
        second = [M.generate(streams[e], A, 60.0) for _ in range(2)][1]
        if mask[e]:
            check_fresh(state(gM, e), hip_snapshot(gM, e), second, A)
    for j in range(T_AFTER + 1):
        if j > 0:
            for g in (gM, gR, gU):
                act(g, A, T0 + j - 1)
                g.step()
        out = {g: (g.get_rewards_array(), g.get_dones(), g.get_true_objectives()) for g in (gM, gR, gU)}
        for e in range(N):
            ref, what = (gR if mask[e] else gU), f"football, {mask_name}, {j} ticks behind the reset, env {e}"
            assert raw(gM, e) == raw(ref, e), f"{what}: snapshot"
            assert football_state(gM, e) == football_state(ref, e), f"{what}: ball"
            for x, y in zip(out[gM], out[ref]):
                n = x.size // N
                assert x[e * n:(e + 1) * n].tobytes() == y[e * n:(e + 1) * n].tobytes(), f"{what}: outputs"
            assert np.array_equal(gM.get_observation(e, 0), ref.get_observation(e, 0)), f"{what}: frame"
    assert all_raw(gR) != all_raw(gU)
    for g in (gM, gR, gU):
        g.close()


# ---- 2. the device form equals the host form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_device_form_equals_host_form(hip, scenario, mode):
    """2. twin gyms, the same mask as a torch.bool CUDA tensor and as numpy: every env's snapshot and the observation slab, byte for byte, right behind the
    reset and after five more ticks; exact pixels and the product's default (fast pixels, pipelined)"""
    A = 1
    dev, host = make_gym(scenario, A, mode), make_gym(scenario, A, mode)
    for t in range(T0):
        for g in (dev, host):
            act(g, A, t)
            g.step()
    before = all_raw(dev)
    keep = device_mask(MASK)
    dev.reset_envs(keep)
    host.reset_envs(MASK)
    for j in range(6):
        if j > 0:
            for g in (dev, host):
                act(g, A, T0 + j)
                assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()
        assert all_raw(dev) == all_raw(host), f"{scenario}, {mode}: snapshots, {j} ticks behind the reset"
        assert slab(dev, A).tobytes() == slab(host, A).tobytes(), f"{scenario}, {mode}: observation slab, {j} ticks behind the reset"
        if j == 0:
            after = all_raw(dev)
            assert [after[e] != before[e] for e in range(N)] == MASK.tolist(), "flagged envs changed, the others did not"
    dev.close(); host.close()
    del keep


# ---- 3. extremes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_all_zero_and_all_ones_masks(hip, scenario):
    """3. three twins: U is left alone, M gets the masked resets, R gets mv_reset.  An all-zero mask (both forms) leaves M what U is: snapshots, slab,
    rewards, dones, episodes_consumed.  An all-ones mask leaves M what R is after mv_reset: snapshots and slab.  mv_ticks_since_reset of M stays U's."""
    A = 1
    gU, gM, gR = (make_gym(scenario, A, "exact") for _ in range(3))
    for t in range(T0):
        for g in (gU, gM, gR):
            act(g, A, t)
            g.step()
    zeros = device_mask(np.zeros(N, bool))
    for form in (zeros, np.zeros(N, bool)):
        gM.reset_envs(form)
        assert all_raw(gM) == all_raw(gU)
        assert slab(gM, A).tobytes() == slab(gU, A).tobytes()
        assert gM.get_rewards_array().tobytes() == gU.get_rewards_array().tobytes() and gM.get_dones().tobytes() == gU.get_dones().tobytes()
        assert gM.get_true_objectives().tobytes() == gU.get_true_objectives().tobytes()
        assert gM.debug_episodes_consumed().tolist() == gU.debug_episodes_consumed().tolist() == [1] * N
    gM.reset_envs(np.ones(N, bool))
    gR.reset()
    assert all_raw(gM) == all_raw(gR) and all_raw(gM) != all_raw(gU)
    assert slab(gM, A).tobytes() == slab(gR, A).tobytes()
    assert gM.get_rewards_array().tobytes() == gR.get_rewards_array().tobytes() and gM.get_dones().tobytes() == gR.get_dones().tobytes()
    assert gM.debug_episodes_consumed().tolist() == gR.debug_episodes_consumed().tolist() == [2] * N
    assert gM.ticks_since_reset() == gU.ticks_since_reset() == T0 and gR.ticks_since_reset() == 0
    for g in (gM, gR):   # ... and both go on alike
        act(g, A, T0)
        g.step()
    assert all_raw(gM) == all_raw(gR) and slab(gM, A).tobytes() == slab(gR, A).tobytes()
    for g in (gU, gM, gR):
        g.close()
    del zeros


# ---- 4. between batched calls, without a host wait -----------------------------------------------------------------------------------------------------
def test_between_batched_calls_without_host_sync(hip):
    """4. TowerBuilding, output rings, step_n(8), the mask written by a torch kernel on the gym's stream, reset_envs(tensor), step_n(8) -- nothing
    synchronises in between: all 16 ring entries (the rings are 16 deep so that both calls' entries can be compared) and the final state equal a
    reference that synchronises on both sides of the reset and uses the host form; the second call still is ONE step launch"""
    import torch
    A, K = 1, 8
    out = []
    for sync in (False, True):
        g = make_gym("TowerBuilding", A, "fast")
        rings = (torch.zeros((2 * K, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0"), torch.full((2 * K, N * A), -7.0, dtype=torch.float32, device="cuda:0"),
                 torch.full((2 * K, N), 9, dtype=torch.uint8, device="cuda:0"))
        src = torch.as_tensor(MASK).to("cuda:0")
        dev_mask = torch.zeros(N, dtype=torch.bool, device="cuda:0")   # (would reset nothing, were it read before the kernel below has run)
        torch.cuda.synchronize()
        g.set_output_ring(2 * K, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
        g.step_n(K, "multidiscrete", POLICY_SEED, 0)
        if sync:
            g.synchronize()
            g.reset_envs(MASK)
            g.synchronize()
        else:
            torch.logical_or(src, src, out=dev_mask)
            g.reset_envs(dev_mask)
        c0 = g.debug_launch_counts()
        g.step_n(K, "multidiscrete", POLICY_SEED, K)
        c1 = g.debug_launch_counts()
        assert c1[0] - c0[0] == 1, f"the call behind the reset took {c1[0] - c0[0]} step launches"
        g.synchronize()
        out.append(([r.cpu().numpy() for r in rings], all_raw(g), g.debug_episodes_consumed().tolist()))
        g.close()
    (ra, sa, ca), (rb, sb, cb) = out
    for x, y, name in zip(ra, rb, ("observations", "rewards", "dones")):
        assert x.tobytes() == y.tobytes(), f"{name} rings differ from the synchronised reference's"
    assert sa == sb and ca == cb
    assert not ra[2].any(), "an env finished inside the window"
    assert ca == [2 if MASK[e] else 1 for e in range(N)]
    assert not ra[1][K - 1].reshape(N, A)[MASK].any() and not ra[2][K - 1][MASK].any()   # (the current ring entry's rewards / dones of the flagged envs)


# ---- 5. forks ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_fork_destination_takes_its_own_next_episode(hip):
    """5. env 1 forks from env 0, three ticks, reset_envs of env 1 alone: env 1 is what env 1 of a twin is that forked nothing and was reset at the same
    tick; its episodes_consumed went up by exactly one, env 0's did not move"""
    A = 1
    only1 = mask_of([1])
    fg, tw = make_gym("TowerBuilding", A, "exact"), make_gym("TowerBuilding", A, "exact")
    for t in range(T0 + 3):
        if t == T0:
            assert raw(fg, 1) != raw(fg, 0)
            fg.fork_envs([-1, 0] + [-1] * (N - 2))
            assert raw(fg, 1) == raw(fg, 0)
        for g in (fg, tw):
            act(g, A, t)
            g.step()
    assert raw(fg, 1) != raw(tw, 1)
    before = fg.debug_episodes_consumed().tolist()
    fg.reset_envs(only1)
    tw.reset_envs(only1)
    assert raw(fg, 1) == raw(tw, 1)
    after = fg.debug_episodes_consumed().tolist()
    assert after[1] == before[1] + 1 and after[0] == before[0] and after == tw.debug_episodes_consumed().tolist()
    assert np.array_equal(fg.get_observation(1, 0), tw.get_observation(1, 0))
    for g in (fg, tw):
        act(g, A, T0 + 3)
        g.step()
    assert raw(fg, 1) == raw(tw, 1)
    fg.close(); tw.close()


# ---- 6. the episode log --------------------------------------------------------------------------------------------------------------------------------
LOG_CASES = {
    # scenario, agents per env, params, ticks per leg, "a flagged env is in the middle of an episode at the first cut"
    # BoxAGone: an episode ends once every agent is on the floor, for a random agent after 30 - 60 ticks and never under 20 (mv_api.hip, the status period):
    # at tick 18 every env is inside its first episode, and in the 62 ticks behind the first cut the envs it left alone finish theirs
    "boxagone_a1": ("BoxAGone", 1, {}, (18, 25, 37), True),
    # TowerBuilding with tests/episode_log_util.py's short episodes (episodeLengthSec -200: an env whose room holds up to 50 objects finishes EVERY tick, so
    # its accumulators are zero between ticks whatever is cut): two agents per env, records every tick, around the cuts
    "tower_short_a2": ("TowerBuilding", 2, {"episodeLengthSec": -200.0}, (9, 12, 9), False),
}


@pytest.mark.parametrize("case", sorted(LOG_CASES))
def test_episode_log_with_masked_resets(hip, case):
    """6. episodes that end naturally inside the run, masked resets at two ticks -- the host form behind a leg of mv_step, the device form behind a leg of
    mv_step_n -- and a last leg of mv_step_many: the drained records, the running returns and lengths equal the numpy model's byte for byte (fed with the
    gym's own per-tick outputs), and a flagged env's running return and length read zero right behind the call.  Both gyms have episodes that can be a
    few ticks long, which the library steps one tick per call whatever k is; the mv_step_n leg asks for one tick per call, since the model needs every
    tick's true objectives."""
    scenario, A, params, legs, running = LOG_CASES[case]
    g = make_gym(scenario, A, "fast", params, log=4096)
    model = CutModel(N, A)
    handles = (C.c_void_p * 1)(g._g)
    tick = 0

    def fed():
        model.feed(g.get_rewards_array()[None], g.get_dones()[None], g.get_true_objectives()[None])

    def check_cut(mask):
        model.cut(mask)
        ret, length = g.episode_returns_tensor().cpu().numpy(), g.episode_lengths_tensor().cpu().numpy()
        assert not ret.reshape(N, A)[mask].any() and not length[mask].any(), "a flagged env's running return / length is not zero"
        assert ret.tobytes() == model.ret.tobytes() and length.tobytes() == model.len.tobytes()
        assert g.episode_log_count() == (len(model.records), 0)

    for _ in range(legs[0]):
        g.sample_random_actions(POLICY_SEED, tick)
        assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()
        fed(); tick += 1
    if running:
        assert (model.len == legs[0]).all(), "an env finished before the first cut, or the cut would clear nothing"
    g.reset_envs(MASK)
    check_cut(MASK)
    for _ in range(legs[1]):
        assert g._lib.mv_step_n(g._g, 1, 1, POLICY_SEED, tick) == 0, g._lib.mv_last_error()
        fed(); tick += 1
    if running:
        assert model.len[COMPLEMENT].any(), "the second cut would clear nothing"
    keep = device_mask(COMPLEMENT)
    g.reset_envs(keep)
    check_cut(COMPLEMENT)
    for _ in range(legs[2]):
        assert g._lib.mv_step_many(handles, 1, 1, 1, POLICY_SEED, tick) == 0, g._lib.mv_last_error()
        fed(); tick += 1
    want = np.array(model.records, U.RECORD)
    assert len(want) > 0, "no episode ended inside the run"
    got = g.drain_episode_log()
    assert g.episode_log_dropped == 0
    assert got.tobytes() == want.tobytes()
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes()
    assert g.ticks_since_reset() == sum(legs) == model.tick
    g.close()
    del keep


def test_episode_log_with_a_masked_reset_between_batched_calls(hip):
    """6, batched.  Sokoban with episodes of 4.5 s (every episode ends at its 68th tick -- checked on the CPU oracle; the status words travel every 16th
    tick, so mv_step_n takes its one-launch path), output rings 8 deep, calls of mv_step_n(8): two calls, reset_envs(MASK) in the device form, twelve more
    calls -- the unflagged envs finish their first episode in tick 67, the flagged ones theirs in tick 16 + 67, all inside the run.  The model is fed from the rings (rewards, dones of every tick) and,
    no env finishing twice inside one call (asserted), the true objectives read behind the call.  Records, running returns and lengths byte for byte;
    every call ONE step launch."""
    import torch
    A, K, calls, cut_after = 1, 8, 14, 2
    g = make_gym("Sokoban", A, "fast", {"episodeLengthSec": 4.5}, log=4096)
    rings = (torch.zeros((K, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((K, N * A), dtype=torch.float32, device="cuda:0"),
             torch.zeros((K, N), dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    g.set_output_ring(K, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
    model = CutModel(N, A)
    keep = device_mask(MASK)
    for c in range(calls):
        c0 = g.debug_launch_counts()
        assert g._lib.mv_step_n(g._g, K, 1, POLICY_SEED, c * K) == 0, g._lib.mv_last_error()
        assert g.debug_launch_counts()[0] - c0[0] == 1, "the call did not take the one-launch step path"
        g.synchronize()
        rew, done = rings[1].cpu().numpy(), rings[2].cpu().numpy()
        assert (done.sum(axis=0) <= 1).all(), "an env finished twice inside one call: the true objectives read behind it are not every tick's"
        model.feed(rew, done, np.repeat(g.get_true_objectives()[None], K, axis=0))
        if c + 1 == cut_after:
            assert (model.len == cut_after * K).all(), "an env finished before the cut"
            g.reset_envs(keep, render=False)
            model.cut(MASK)
            assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes()
            assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes()
    want = np.array(model.records, U.RECORD)
    finished = set((want["agent"] // A).tolist())
    assert finished == set(range(N)), f"only envs {sorted(finished)} finished an episode inside the run"
    for e in np.flatnonzero(MASK):   # (the expected log itself: a flagged env's first record counts from the cut, not from tick 0)
        r = want[want["agent"] // A == e][0]
        assert int(r["length"]) == int(r["end_tick"]) + 1 - cut_after * K
    got = g.drain_episode_log()
    assert g.episode_log_dropped == 0
    assert got.tobytes() == want.tobytes()
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes()
    assert g.ticks_since_reset() == calls * K == model.tick
    g.close()
    del keep, rings


# ---- 7. host-fed supply --------------------------------------------------------------------------------------------------------------------------------
def test_device_form_on_a_host_fed_gym_does_not_starve(hip):
    """7a. ObstaclesEasy (the host's feeder, three resident episodes per env), the device form on half of the envs after 5 ticks, then 40 ticks of mv_step:
    every stepping call returns 0 -- no starvation warning -- and the flagged envs took exactly one episode"""
    A = 1
    half = mask_of(range(0, N, 2))
    g = make_gym("ObstaclesEasy", A, "fast")
    for t in range(5):
        g.sample_random_actions(POLICY_SEED, t)
        assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()
    keep = device_mask(half)
    assert g._lib.mv_reset_envs(g._g, C.c_void_p(keep.data_ptr()), 1) == 0, g._lib.mv_last_error()
    for t in range(5, 45):
        g.sample_random_actions(POLICY_SEED, t)
        assert g._lib.mv_step(g._g) == 0, (t, g._lib.mv_last_error())
    assert not g.get_dones().any()
    assert g.debug_episodes_consumed().tolist() == [2 if half[e] else 1 for e in range(N)]
    g.close()
    del keep


def test_host_form_three_times_in_a_row(hip):
    """7b. Empty (host-fed, TWO resident episodes per env), the host form three times on env 3 with no step in between: every call returns 0, env 3's
    episodes_consumed advances by one each time and its snapshot is the oracle's env 3 after as many reset()s; every other env stays the oracle's that
    was never reset"""
    scenario, A, e = "Empty", 1, 3
    ref = oracle_reference(scenario, A, resets=3, ticks_after=0)
    g = make_gym(scenario, A, "exact")
    for t in range(T0):
        act(g, A, t)
        g.step()
    m = mask_of([e])
    data = np.ascontiguousarray(m, np.uint8)
    snaps = []
    for r in range(3):
        assert g._lib.mv_reset_envs_host(g._g, data.ctypes.data, 1) == 0, g._lib.mv_last_error()
        assert g.debug_episodes_consumed().tolist() == [2 + r if i == e else 1 for i in range(N)]
        Q = ref[r][1]
        assert diff_snapshots(Q["snap"][e], hip_snapshot(g, e), A) == [], f"env {e} after {r + 1} resets"
        assert np.array_equal(g.get_observation(e, 0), Q["frames"][e])
        snaps.append(raw(g, e))
    assert len(set(snaps)) == 3, "three resets, fewer than three different episodes"
    P = ref[2][0]
    for i in range(N):
        if i != e:
            check_env(g, P, scenario, A, i, f"env {i}, never reset")
    g.step()
    g.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_errors(hip):
    """8. before the first mv_reset, a null mask, a closed gym: -1 with text, nothing changes"""
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    lib = g._lib
    data = np.ones(N, np.uint8)
    for fn in (lib.mv_reset_envs_host, lib.mv_reset_envs):
        assert fn(g._g, data.ctypes.data, 1) == -1 and b"mv_reset first" in lib.mv_last_error()
    with pytest.raises(RuntimeError, match="mv_reset first"):
        g.reset_envs(MASK)
    g.seed(ENV_SEED); g.reset()
    act(g, 1, 0); g.step()
    before, frames, consumed = all_raw(g), slab(g, 1).tobytes(), g.debug_episodes_consumed().tolist()
    for fn in (lib.mv_reset_envs_host, lib.mv_reset_envs):
        assert fn(g._g, None, 1) == -1 and b"null mask" in lib.mv_last_error()
    with pytest.raises(ValueError, match="reset_envs"):
        g.reset_envs(np.ones(N + 1, bool))
    assert all_raw(g) == before and slab(g, 1).tobytes() == frames and g.debug_episodes_consumed().tolist() == consumed
    handle = g._g
    lib.mv_close(handle)
    for fn in (lib.mv_reset_envs_host, lib.mv_reset_envs):
        assert fn(handle, data.ctypes.data, 1) == -1 and b"closed" in lib.mv_last_error()
    g.close()


# ---- 9. the Python surface -----------------------------------------------------------------------------------------------------------------------------
def test_env_reset_envs(hip):
    """9. MegaverseEnv.reset_envs([0, 3]) on an 8-env env: the observations step_device hands out change for envs 0 and 3 and for no other env, exactly;
    their rewards and dones read zero; a wrong index or a wrong mask length is a ValueError"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("TowerBuilding", N, 1, 1, False, None, img_w=W, img_h=H)
    env.env.set_pixel_mode("fast")
    env.seed(3)
    env.reset()
    for t in range(4):
        obs, rew, done = env.step_device(sample_actions(POLICY_SEED, t, N))
    env.env.synchronize()
    before, states = obs.cpu().numpy().copy(), all_raw(env.env)
    assert env.reset_envs([0, 3]) is None
    env.env.synchronize()
    after, now = obs.cpu().numpy(), all_raw(env.env)
    changed = [not np.array_equal(before[e], after[e]) for e in range(N)]
    assert changed == mask_of([0, 3]).tolist()
    assert [now[e] != states[e] for e in range(N)] == mask_of([0, 3]).tolist()
    assert not rew.cpu().numpy()[[0, 3]].any() and not done.cpu().numpy()[[0, 3]].any()
    with pytest.raises(ValueError, match="reset_envs"):
        env.reset_envs([N])
    with pytest.raises(ValueError, match="reset_envs"):
        env.env.reset_envs(np.zeros(N - 1, bool))
    with pytest.raises(ValueError, match="reset_envs"):
        env.env.reset_envs(np.zeros(N, np.int32))
    env.step_device(sample_actions(POLICY_SEED, 4, N))
    env.close()


# ---- 10. members of a group ----------------------------------------------------------------------------------------------------------------------------
def test_multitask_reset_envs(hip):
    """10. MultiTaskGym (TowerBuilding + ObstaclesEasy, one mv_group): three twins -- M gets reset_envs(mask) in the batch's numbering, R a full reset(),
    U nothing; flagged envs of M are R's, the others U's, right behind the reset and after a batched group call; both forms"""
    import torch
    from megaverse_amd.multitask import MultiTaskGym
    mask = mask_of([0, 3, 5])   # tasks 0, 1, 1: local envs 0 / 1, 2
    for form in ("host", "device"):
        gyms = []
        for _ in range(3):
            m = MultiTaskGym(["TowerBuilding", "ObstaclesEasy"], W, H, N, 1, 1)
            m.set_pixel_mode("fast")
            m.attach(torch.device("cuda:0"))
            m.seed(ENV_SEED)
            m.reset()
            # (a host-fed member's rings get their second episodes from the stepping calls behind mv_reset, once its status words have travelled back: two
            # calls with the device caught up in between, so that the device form below finds an episode resident -- it uses only what is)
            m.step_n(2, "multidiscrete", POLICY_SEED, 0)
            m.synchronize()
            m.step_n(2, "multidiscrete", POLICY_SEED, 2)
            gyms.append(m)
        gM, gR, gU = gyms
        assert gM.union

        def states(m):
            out = []
            for i in range(N):
                sub, j = m.locate(i)
                out.append(raw(sub, j))
            return out

        keep = device_mask(mask) if form == "device" else None
        gM.reset_envs(keep if form == "device" else mask)
        gR.reset()
        for k in range(2):
            if k:
                for m in gyms:
                    m.step_n(4, "multidiscrete", POLICY_SEED, 4)
            sM, sR, sU = states(gM), states(gR), states(gU)
            assert [sM[i] == (sR[i] if mask[i] else sU[i]) for i in range(N)] == [True] * N, f"{form} form, {'behind the reset' if k == 0 else 'a call later'}"
            assert [sM[i] != sU[i] for i in range(N)] == mask.tolist()
            for i in range(N):
                want = gR if mask[i] else gU
                assert np.array_equal(gM.get_observation(i, 0), want.get_observation(i, 0)), f"{form} form: frame of env {i}"
        for m in gyms:
            m.close()
        del keep
