"""Env forks on the GPU (include/megaverse_hip.h: mv_fork_envs): env d leaves its episode and continues env s's, inside one gym.

Every test uses 8 envs, 64 x 36 frames and the one map of tests/fork_util.py.  Before the fork every env is driven by its own column of a scripted action
stream (tests/action_ring_util.py: make_script), so all eight states differ -- asserted.  T1 ticks run before the fork and T2 after it; no env may finish
inside them -- asserted on every tick -- so that a destination really continues its source's episode.  Expected values come from the CPU oracle (which is
never forked: it just runs the script) or from a twin gym that does not fork."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
from action_ring_util import make_script
from fork_util import H, MAP, N, W, columns, log_model, remap
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import GymGroup, MegaverseGym

pytestmark = pytest.mark.gpu

BOXOBAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban")
COLS = columns(MAP)
DESTINATIONS = [e for e in range(N) if COLS[e] != e]
assert DESTINATIONS == [1, 2, 3, 5] and COLS == [0, 0, 0, 7, 4, 7, 6, 7]


def window(scenario):
    """T1 = T2: 12 ticks where episodes last hundreds of ticks, 6 for BoxAGone (its episodes never end under 20 ticks: mv_api.hip, the status period)"""
    return 6 if scenario == "BoxAGone" else 12


def make_gym(scenario, A, mode, params=None, seed=42, log=0):
    g = MegaverseGym(scenario, W, H, N, A, 1, False, params or {})
    g.set_pixel_mode(mode)
    g.seed(seed)
    if log:
        g.set_episode_log(log)
    g.reset()
    return g


def make_oracle(scenario, A, params=None, seed=42):
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, params or {})
    og.seed(seed)
    og.reset()
    return og


def oracle_act(og, A, actions):
    for e in range(N):
        for a in range(A):
            og.set_actions(e, a, actions[e * A + a].tolist())


def raw(g, e):
    return g.debug_snapshot_bytes(e).tobytes()


def assert_all_states_differ(g, what):
    snaps = [raw(g, e) for e in range(N)]
    assert len(set(snaps)) == N, f"{what}: two envs are in the same state before the fork: the test would prove nothing"
    return snaps


def frames_of(g, A, e):
    return np.stack([g.get_observation(e, a) for a in range(A)])


# ---- 1. against the oracle, exact pixels ---------------------------------------------------------------------------------------------------------------
ORACLE_CASES = {"tower_a1": ("TowerBuilding", 1), "tower_a3": ("TowerBuilding", 3), "obstacles_easy_a2": ("ObstaclesEasy", 2), "collect": ("Collect", 1),
                "rearrange": ("Rearrange", 1), "sokoban": ("Sokoban", 1), "hex_memory": ("HexMemory", 1), "boxagone": ("BoxAGone", 1), "football": ("Football", 2)}


def check_against_oracle(hg, og, A, e, src, what, boxagone=False, football=False):
    """env e of the gym == env src of the oracle: state, rewards, dones, true objectives, frames"""
    assert diff_snapshots(og.snapshot(src), hip_snapshot(hg, e), A) == [], f"{what}: state of env {e} against the oracle's env {src}"
    if boxagone:
        import boxagone_model as M
        so, sh = og.boxagone_state(src), hg.debug_boxagone_state(e).view(M.STATE)[0]
        bad = [n for n in M.STATE.names if so[n].tobytes() != sh[n].tobytes()]
        assert not bad, f"{what}: BoxAGone state of env {e}: {bad}"
    if football:
        from football_cases import record
        so, sh = og.football_state(src), record(hg.debug_football_state(e))
        assert so.tobytes() == sh.tobytes(), f"{what}: Football's ball of env {e}: {so} vs {sh}"
    rew, done, tobj = hg.get_rewards_array(), hg.get_dones(), hg.get_true_objectives()
    assert rew[e * A:(e + 1) * A].tobytes() == og.get_last_rewards()[src * A:(src + 1) * A].tobytes(), f"{what}: rewards of env {e}"
    assert int(done[e]) == int(og.get_dones()[src]), f"{what}: done of env {e}"
    for a in range(A):
        assert np.float32(tobj[e * A + a]).tobytes() == np.float32(og.true_objective(src, a)).tobytes(), f"{what}: true objective of env {e}"
        assert np.array_equal(hg.get_observation(e, a), og.get_observation(src, a)), f"{what}: frame of env {e}, agent {a}"


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_fork_against_the_oracle(hip, case, monkeypatch):
    """1. T1 ticks on the per-env script, the fork, T2 ticks in which every destination acts on its source's column: after every post-fork tick env d is
    the oracle's env s -- snapshot, rewards, dones, true objectives, exact-mode frames -- and byte for byte the gym's own env s; every env that was left
    alone is its own oracle env."""
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)
    scenario, A = ORACLE_CASES[case]
    T = window(scenario)
    script = make_script(11, 2 * T, N * A)
    forked = remap(script, COLS, A, T)
    hg, og = make_gym(scenario, A, "exact"), make_oracle(scenario, A)
    for t in range(T):
        hg.set_actions_batched(script[t]); hg.step()
        oracle_act(og, A, script[t]); og.step_norender()
        assert not hg.get_dones().any() and not og.get_dones().any(), f"an env finished before the fork (tick {t})"
    before = assert_all_states_differ(hg, case)
    hg.fork_envs(MAP)
    # the fork itself: destinations are their sources, everyone else is untouched; the public outputs still describe the last stepped tick
    for e in range(N):
        assert raw(hg, e) == before[COLS[e]], f"{case}: env {e} right after the fork"
    for t in range(T, 2 * T):
        hg.set_actions_batched(forked[t]); hg.step()
        oracle_act(og, A, script[t]); og.step()
        assert not hg.get_dones().any() and not og.get_dones().any(), f"an env finished inside the window (tick {t})"
        for e in range(N):
            check_against_oracle(hg, og, A, e, COLS[e], f"{case}, tick {t}", boxagone=scenario == "BoxAGone", football=scenario == "Football")
        for d in DESTINATIONS:
            assert raw(hg, d) == raw(hg, COLS[d]), f"{case}, tick {t}: env {d} is not byte for byte its source {COLS[d]}"
    hg.close(); og.close()


# ---- 2. branches diverge correctly ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "Collect"])
def test_branches_diverge(hip, scenario):
    """2. after the fork the two destinations of env 0 act on two DIFFERENT fresh columns: each is the env 0 of an oracle gym of its own, seeded and
    scripted alike, whose env 0 switches to that column at tick T1"""
    A, T = 1, window(scenario)
    script = make_script(11, 2 * T, N * A)
    fresh = make_script(23, 2 * T, 2)   # two columns nobody has acted on
    assert not np.array_equal(fresh[T:, 0], fresh[T:, 1]) and not np.array_equal(fresh[T:, 0], script[T:, 0])
    forked = remap(script, COLS, A, T)
    forked[T:, 1], forked[T:, 2] = fresh[T:, 0], fresh[T:, 1]
    oracles = []
    for k in range(2):
        s = script.copy()
        s[T:, 0] = fresh[T:, k]
        oracles.append((make_oracle(scenario, A), s))
    hg = make_gym(scenario, A, "exact")
    for t in range(2 * T):
        if t == T:
            assert_all_states_differ(hg, scenario)
            hg.fork_envs(MAP)
        hg.set_actions_batched((script if t < T else forked)[t]); hg.step()
        assert not hg.get_dones().any(), f"an env finished inside the window (tick {t})"
        for og, s in oracles:
            oracle_act(og, A, s[t])
            og.step() if t >= T else og.step_norender()
            assert not og.get_dones().any()
        if t >= T:
            for k, (og, _) in enumerate(oracles):
                check_against_oracle(hg, og, A, 1 + k, 0, f"{scenario}, branch {k}, tick {t}")
    assert raw(hg, 1) != raw(hg, 2) and raw(hg, 1) != raw(hg, 0), "the branches did not diverge: the fresh columns changed nothing"
    hg.close()
    for og, _ in oracles:
        og.close()


# ---- 3. every scenario in the product's default mode ---------------------------------------------------------------------------------------------------
DEFAULT_MODE = ["TowerBuilding", "ObstaclesHard", "Collect", "Rearrange", "Sokoban", "Empty", "HexMemory", "HexExplore", "BoxAGone", "Football"]


def extra_state(g, scenario, e):
    if scenario == "BoxAGone":
        return g.debug_boxagone_state(e).tobytes()
    if scenario == "Football":
        st = g.debug_football_state(e)
        return b"".join(np.asarray(st[k]).tobytes() for k in ("pos", "radius", "vel", "kicks", "ang", "contacts", "force"))
    return b""


@pytest.mark.parametrize("scenario", DEFAULT_MODE)
def test_fork_equals_an_unforked_twin_in_default_mode(hip, scenario, monkeypatch):
    """3. fast pixels, pipelined single-tick calls out of an action ring: the gym that forks against a twin that does not, whose env s is fed what the
    fork's env d is fed -- snapshots, BoxAGone / Football state, rewards, dones and frames byte for byte after every post-fork tick"""
    import torch
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)
    A, T = 1, window(scenario)
    script = make_script(13, 2 * T, N * A)
    rings = [torch.as_tensor(remap(script, COLS, A, T)).to("cuda:0"), torch.as_tensor(script).to("cuda:0")]
    gyms = [make_gym(scenario, A, "fast"), make_gym(scenario, A, "fast")]
    for g, ring in zip(gyms, rings):
        assert g.pipelining() and g.pixel_mode() == "fast"
        g.set_action_ring(2 * T, ring.data_ptr())
    fg, tw = gyms
    for t in range(2 * T):
        if t == T:
            before = assert_all_states_differ(fg, scenario)
            fg.fork_envs(MAP)
            for e in range(N):
                assert raw(fg, e) == before[COLS[e]] == raw(tw, COLS[e]), f"{scenario}: env {e} right after the fork"
        for g in gyms:
            g.step_n(1, "sequence", 0, t)
        rf, rt, df, dt = fg.get_rewards_array(), tw.get_rewards_array(), fg.get_dones(), tw.get_dones()
        assert not df.any() and not dt.any(), f"an env finished inside the window (tick {t})"
        if t < T:
            continue
        for e in range(N):
            s = COLS[e]
            assert raw(fg, e) == raw(tw, s), f"{scenario}, tick {t}: state of env {e} against the twin's env {s}"
            assert extra_state(fg, scenario, e) == extra_state(tw, scenario, s), f"{scenario}, tick {t}: scenario state of env {e}"
            assert rf[e * A:(e + 1) * A].tobytes() == rt[s * A:(s + 1) * A].tobytes() and df[e] == dt[s], f"{scenario}, tick {t}: outputs of env {e}"
            assert np.array_equal(frames_of(fg, A, e), frames_of(tw, A, s)), f"{scenario}, tick {t}: frames of env {e}"
    for g in gyms:
        g.close()


# ---- 4. between batched calls, without a host synchronisation ------------------------------------------------------------------------------------------
def rings_of(torch, count, A):
    t = (torch.zeros((count, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0"), torch.full((count, N * A), -7.0, dtype=torch.float32, device="cuda:0"),
         torch.full((count, N), 9, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("form", ["device_map", "host_map"])
@pytest.mark.parametrize("scenario,overlap,depth", [("TowerBuilding", False, 16), ("ObstaclesEasy", True, 32)])
def test_fork_between_batched_calls_without_host_sync(hip, scenario, overlap, depth, form):
    """4. step_n(8, 'sequence'), the map written by a torch kernel on the gym's stream, fork_envs(tensor), step_n(8, 'sequence') -- nothing synchronises in
    between: every ring entry and the final state equal a twin that synchronises around each of the three.  host_map: the same with the map as a list
    (the host form goes to the simulation stream between the two calls' step launches)."""
    import torch
    A, K = 1, 8
    script = remap(make_script(17, 2 * K, N * A), COLS, A, K)
    dev_script = torch.as_tensor(script).to("cuda:0")
    map_src = torch.as_tensor(np.array(MAP, np.int32)).to("cuda:0")
    out = []
    for sync in (False, True):
        g = make_gym(scenario, A, "fast")
        rings = rings_of(torch, depth, A)
        g.set_output_ring(depth, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
        if overlap:
            g.set_pass_overlap(True)
        g.set_action_ring(2 * K, dev_script.data_ptr())
        dev_map = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")   # (would fork nothing, were it read before the kernel below has run)
        torch.cuda.synchronize()
        g.step_n(K, "sequence", 0, 0)
        if sync:
            g.synchronize()
        torch.add(map_src, 0, out=dev_map)   # (the gym's stream is torch's current one: the null stream)
        g.fork_envs(dev_map if form == "device_map" else MAP)
        if sync:
            g.synchronize()
        g.step_n(K, "sequence", 0, K)
        g.synchronize()
        out.append(([r.cpu().numpy() for r in rings], [raw(g, e) for e in range(N)]))
        assert not out[-1][0][2][:2 * K].any(), "an env finished inside the window"
        g.close()
    (ra, sa), (rb, sb) = out
    for x, y, name in zip(ra, rb, ("observations", "rewards", "dones")):
        assert x.tobytes() == y.tobytes(), f"{scenario}: {name} rings differ from the synchronised twin's"
    assert sa == sb, f"{scenario}: final state differs from the synchronised twin's"
    for d in DESTINATIONS:   # ... and the fork happened: the destinations ran their sources' episodes on their sources' actions
        assert sa[d] == sa[COLS[d]]
    assert len({sa[e] for e in range(N)}) == N - len(DESTINATIONS)


# ---- 5. / 6. identity is kept; the episode log -------------------------------------------------------------------------------------------------------
SHORT = {"episodeLengthSec": 2.0}
FORK_TICK = 5
MAX_TICKS = 6000   # (TowerBuilding adds 4 s per object to episodeLengthSec: up to ~300 s of 15 ticks)


def run_until_everyone_finished(g, A, fork_at=None):
    """idle ticks until every env has finished once, and one tick more -> per-tick rewards / dones / true objectives, and each env's snapshot and
    episodes_consumed right behind the tick that finished its first episode (the first state of the next episode of its own sequence)"""
    rewards, dones, tobj, first = [], [], [], {}
    extra = 0
    for t in range(MAX_TICKS):
        if fork_at is not None and t == fork_at:
            g.fork_envs(MAP)
        rc = g._lib.mv_step_no_render(g._g)
        assert rc == 0, (t, rc, g._lib.mv_last_error())
        d = g.get_dones()
        rewards.append(g.get_rewards_array()); dones.append(d); tobj.append(g.get_true_objectives())
        for e in np.flatnonzero(d):
            if int(e) not in first:
                first[int(e)] = (t, raw(g, int(e)), int(g.debug_episodes_consumed()[e]))
        if len(first) == N:
            extra += 1
            if extra == 2:
                break
    assert len(first) == N, "not every env finished"
    return np.stack(rewards), np.stack(dones), np.stack(tobj), first


@functools.lru_cache(maxsize=None)
def unforked_twin(scenario):
    g = make_gym(scenario, 1, "fast", SHORT)
    out = run_until_everyone_finished(g, 1)
    assert g._lib.mv_step_no_render(g._g) == 0
    g.close()
    return out


@pytest.mark.parametrize("log", [0, 4096], ids=["no_log", "episode_log"])
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_identity_is_kept(hip, scenario, log):
    """5. episodeLengthSec 2.0, idle actions, the fork at tick 5, until every env has finished once and one tick more: every env then took the next episode
    of its OWN sequence -- its snapshot right behind its finishing tick and its episodes_consumed are the unforked twin's right behind that env's finishing
    tick -- and nothing starved (TowerBuilding: device-drawn episodes, ObstaclesEasy: the host feeder).
    6. with the episode log on: the forked envs' records carry the length and return of the whole episode from the SOURCE's start, the destinations' cut
    episodes wrote none; expected records: a numpy model over the per-tick outputs the twin's episodes imply."""
    A = 1
    tw_rew, tw_done, tw_tobj, tw_first = unforked_twin(scenario)
    g = make_gym(scenario, A, "fast", SHORT, log=log)
    assert not tw_done[:FORK_TICK + 1].any(), "an env finished before the fork"
    rew, done, tobj, first = run_until_everyone_finished(g, A, fork_at=FORK_TICK)
    for e in range(N):
        t, snap, consumed = first[e]
        assert t == tw_first[COLS[e]][0], f"env {e} finished at tick {t}, its source's episode ends at {tw_first[COLS[e]][0]}"
        assert snap == tw_first[e][1], f"env {e}: the episode after the fork's is not the next one of its own sequence"
        assert consumed == tw_first[e][2] == 2
    # what the forked gym's outputs must have been: env e played its source's first episode from tick 0 (the public outputs are per tick: before the fork
    # they were env e's own), then the episodes of its own sequence, which the twin played from another tick on -- idle actions: the same ticks, shifted
    T = done.shape[0]
    want_rew, want_done = np.zeros_like(rew), np.zeros_like(done)
    for e in range(N):
        s, end_s, end_e = COLS[e], tw_first[COLS[e]][0], tw_first[e][0]
        own = (tw_rew[end_e + 1:, e], tw_done[end_e + 1:, e])
        head = [tw_rew[:end_s + 1, s].copy(), tw_done[:end_s + 1, s].copy()]
        head[0][:FORK_TICK], head[1][:FORK_TICK] = tw_rew[:FORK_TICK, e], tw_done[:FORK_TICK, e]
        n = min(T - (end_s + 1), own[0].shape[0])
        want_rew[:end_s + 1 + n, e] = np.concatenate([head[0], own[0][:n]])
        want_done[:end_s + 1 + n, e] = np.concatenate([head[1], own[1][:n]])
        known = end_s + 1 + n
        assert rew[:known, e].tobytes() == want_rew[:known, e].tobytes() and np.array_equal(done[:known, e], want_done[:known, e]), f"outputs of env {e}"
    if not log:
        assert g._lib.mv_step_no_render(g._g) == 0, g._lib.mv_last_error()   # nothing starved
        g.close()
        return
    # the log: the running return restarts from the source's at the fork -- model: env d's rewards before the fork are its source's
    model_rew = rew.copy()
    for d in DESTINATIONS:
        model_rew[:FORK_TICK, d] = tw_rew[:FORK_TICK, COLS[d]]
    records, ret, length = log_model(model_rew, done, tobj, A)
    got = g.drain_episode_log()
    assert g.episode_log_dropped == 0 and len(got) == len(records) >= N
    for r, w in zip(got, records):
        assert (int(r["agent"]), int(r["length"]), int(r["end_tick"])) == w[:3], (r, w)
        assert np.float32(r["true_objective"]).tobytes() == np.float32(w[3]).tobytes() and np.float64(r["ret"]).tobytes() == np.float64(w[4]).tobytes(), (r, w)
    for d in DESTINATIONS:   # the whole episode from the source's start, and no record of the cut one
        mine = [r for r in got if int(r["agent"]) == d]
        assert int(mine[0]["length"]) == tw_first[COLS[d]][0] + 1 == int(mine[0]["end_tick"]) + 1
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == length.tobytes()
    assert g._lib.mv_step_no_render(g._g) == 0, g._lib.mv_last_error()   # nothing starved
    g.close()


# ---- 7. invalid entries on the device path -------------------------------------------------------------------------------------------------------------
def test_invalid_entries_are_skipped_and_reported_once(hip):
    """7. a device map with a chain (2 <- 1 <- 0) and an index of N: the envs concerned stay byte for byte what they were, the valid entry of the same
    map is applied, the next step returns 1 once with a text that names forks, the call after it 0"""
    import torch
    bad = [-1, 0, 1, -1, N, 7, -1, -1]
    g = make_gym("TowerBuilding", 1, "fast")
    script = make_script(19, 8, N)
    for t in range(8):
        g.set_actions_batched(script[t]); g.step()
    before = assert_all_states_differ(g, "invalid entries")
    dev_map = torch.as_tensor(np.array(bad, np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    g.fork_envs(dev_map)
    after = [raw(g, e) for e in range(N)]
    for e in (0, 1, 2, 3, 4, 6, 7):
        assert after[e] == before[e], f"env {e} changed"
    assert after[5] == before[7], "the valid entry was not applied"
    lib = g._lib
    assert lib.mv_step(g._g) == 1
    text = lib.mv_last_error().decode()
    assert "mv_fork_envs" in text and "chain" in text, text
    assert lib.mv_step(g._g) == 0
    # a valid device map reports nothing
    g.fork_envs(torch.as_tensor(np.array(MAP, np.int32)).to("cuda:0"))
    assert lib.mv_step(g._g) == 0 and lib.mv_step(g._g) == 0
    g.synchronize()
    g.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """8. before the first reset; on a gym in a group; the host form on a chain or an index out of range: -1 with text, the state unchanged"""
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    with pytest.raises(RuntimeError, match="mv_reset"):
        g.fork_envs(MAP)
    g.seed(42); g.reset()
    before = [raw(g, e) for e in range(N)]
    with pytest.raises(RuntimeError, match="chain"):
        g.fork_envs([-1, 0, 1, -1, -1, 7, -1, -1])
    with pytest.raises(RuntimeError, match="out of range"):
        g.fork_envs([-1, 0, 0, N, -1, 7, -1, -1])
    assert g._lib.mv_fork_envs(g._g, None) < 0 and b"null map" in g._lib.mv_last_error()
    assert [raw(g, e) for e in range(N)] == before
    g.step()
    other = make_gym("ObstaclesEasy", 1, "fast")
    grp = GymGroup([g, other])
    with pytest.raises(RuntimeError, match="mv_group"):
        g.fork_envs(MAP)
    grp.close()
    g.fork_envs(MAP)   # on its own again
    g.step()
    g.synchronize()
    g.close(); other.close()
    with pytest.raises(RuntimeError, match="closed"):
        g_closed = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
        handle = g_closed._g
        g_closed._lib.mv_close(handle)
        try:
            g_closed.fork_envs(MAP)
        finally:
            g_closed.close()


def test_env_fork(hip):
    """MegaverseEnv.fork: one env into all others, then into two of them"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("TowerBuilding", N, 1, 1, False, None, img_w=W, img_h=H)
    env.env.set_pixel_mode("fast")
    env.seed(3)
    env.reset()
    script = make_script(29, 4, N)
    for t in range(4):
        env.step_device(script[t])
    before = assert_all_states_differ(env.env, "MegaverseEnv.fork")
    env.fork(6, [0, 3])
    assert [raw(env.env, e) for e in range(N)] == [before[6] if e in (0, 3) else before[e] for e in range(N)]
    env.fork(2)
    assert all(raw(env.env, e) == before[2] for e in range(N))
    env.close()
