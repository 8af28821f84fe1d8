"""Env resampling on the GPU (include/megaverse_hip.h: mv_resample_envs): env d takes the state env src_of[d] had before the call, for any map.

The structure is tests/test_fork_gpu.py's: 8 envs (but test 6), 64 x 36 frames, the two maps of tests/resample_util.py.  Before the call every env is driven by
its own column of a scripted action stream, so all eight states differ -- asserted; T1 ticks run before the call and T2 after it, and no env may finish
inside them -- asserted on every tick.  Expected values come from the CPU oracle (which is never resampled: it just runs the script) or from a twin gym."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
from action_ring_util import make_script
from fork_util import H, MAP, N, W, columns, log_model, remap
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import GymGroup, MegaverseGym
from resample_util import DRAW, DRAW_COLS, PERM, PERM_COLS, compose

pytestmark = pytest.mark.gpu

BOXOBAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban")
MAPS = {"perm": (PERM, PERM_COLS), "draw": (DRAW, DRAW_COLS)}


def window(scenario):
    """T1 = T2: 12 ticks where episodes last hundreds of ticks, 6 for BoxAGone (its episodes never end under 20 ticks)"""
    return 6 if scenario == "BoxAGone" else 12


def make_gym(scenario, A, mode, params=None, seed=42, log=0, n=N):
    g = MegaverseGym(scenario, W, H, n, A, 1, False, params or {})
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


def assert_all_states_differ(g, what, n=N):
    snaps = [raw(g, e) for e in range(n)]
    assert len(set(snaps)) == n, f"{what}: two envs are in the same state before the call: the test would prove nothing"
    return snaps


def frames_of(g, A, e):
    return np.stack([g.get_observation(e, a) for a in range(A)])


def device_map(m):
    import torch
    t = torch.as_tensor(np.array(m, np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return t


# ---- 1. against the oracle, exact pixels ---------------------------------------------------------------------------------------------------------------
ORACLE_CASES = {"tower_a1": ("TowerBuilding", 1, "perm"), "tower_a3": ("TowerBuilding", 3, "perm"), "obstacles_easy_a2": ("ObstaclesEasy", 2, "perm"),
                "sokoban": ("Sokoban", 1, "perm"), "hex_memory": ("HexMemory", 1, "perm"), "boxagone": ("BoxAGone", 1, "perm"), "football": ("Football", 2, "perm"),
                "tower_a1_draw": ("TowerBuilding", 1, "draw")}


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
def test_resample_against_the_oracle(hip, case, monkeypatch):
    """1. T1 ticks on the per-env script, the call, T2 ticks in which env e acts on column cols[e]: right after the call env e is byte for byte what env
    cols[e] was, and after every later tick it is the oracle's env cols[e] -- snapshot, rewards, dones, true objectives, exact-mode frames"""
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)
    scenario, A, which = ORACLE_CASES[case]
    m, cols = MAPS[which]
    T = window(scenario)
    script = make_script(11, 2 * T, N * A)
    resampled = remap(script, cols, A, T)
    hg, og = make_gym(scenario, A, "exact"), make_oracle(scenario, A)
    for t in range(T):
        hg.set_actions_batched(script[t]); hg.step()
        oracle_act(og, A, script[t]); og.step_norender()
        assert not hg.get_dones().any() and not og.get_dones().any(), f"an env finished before the call (tick {t})"
    before = assert_all_states_differ(hg, case)
    hg.resample_envs(m)
    for e in range(N):
        assert raw(hg, e) == before[cols[e]], f"{case}: env {e} right after the call"
    for t in range(T, 2 * T):
        hg.set_actions_batched(resampled[t]); hg.step()
        oracle_act(og, A, script[t]); og.step()
        assert not hg.get_dones().any() and not og.get_dones().any(), f"an env finished inside the window (tick {t})"
        for e in range(N):
            check_against_oracle(hg, og, A, e, cols[e], f"{case}, tick {t}", boxagone=scenario == "BoxAGone", football=scenario == "Football")
    for e in range(N):   # envs that drew the same source run one episode, byte for byte
        for f in range(e):
            assert (raw(hg, e) == raw(hg, f)) == (cols[e] == cols[f]), f"{case}: envs {f} and {e}"
    hg.close(); og.close()


# ---- 2. every scenario in the product's default mode ---------------------------------------------------------------------------------------------------
DEFAULT_MODE = ["TowerBuilding", "ObstaclesHard", "Collect", "Rearrange", "Sokoban", "Empty", "HexMemory", "HexExplore", "BoxAGone", "Football"]


def extra_state(g, scenario, e):
    if scenario == "BoxAGone":
        return g.debug_boxagone_state(e).tobytes()
    if scenario == "Football":
        st = g.debug_football_state(e)
        return b"".join(np.asarray(st[k]).tobytes() for k in ("pos", "radius", "vel", "kicks", "ang", "contacts", "force"))
    return b""


@pytest.mark.parametrize("scenario", DEFAULT_MODE)
def test_resample_equals_an_unresampled_twin_in_default_mode(hip, scenario, monkeypatch):
    """2. fast pixels, pipelined single-tick calls out of an action ring, the map PERM: the gym that resamples against a twin that never does, whose env
    cols[e] is fed what env e is fed -- snapshots, BoxAGone / Football state, rewards, dones and frames byte for byte after every later tick"""
    import torch
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)
    A, T, cols = 1, window(scenario), PERM_COLS
    script = make_script(13, 2 * T, N * A)
    rings = [torch.as_tensor(remap(script, cols, A, T)).to("cuda:0"), torch.as_tensor(script).to("cuda:0")]
    gyms = [make_gym(scenario, A, "fast"), make_gym(scenario, A, "fast")]
    for g, ring in zip(gyms, rings):
        assert g.pipelining() and g.pixel_mode() == "fast"
        g.set_action_ring(2 * T, ring.data_ptr())
    rg, tw = gyms
    for t in range(2 * T):
        if t == T:
            before = assert_all_states_differ(rg, scenario)
            extra = [extra_state(rg, scenario, e) for e in range(N)]
            rg.resample_envs(PERM)
            for e in range(N):
                assert raw(rg, e) == before[cols[e]] == raw(tw, cols[e]), f"{scenario}: env {e} right after the call"
                assert extra_state(rg, scenario, e) == extra[cols[e]], f"{scenario}: scenario state of env {e} right after the call"
        for g in gyms:
            g.step_n(1, "sequence", 0, t)
        rf, rt, df, dt = rg.get_rewards_array(), tw.get_rewards_array(), rg.get_dones(), tw.get_dones()
        assert not df.any() and not dt.any(), f"an env finished inside the window (tick {t})"
        if t < T:
            continue
        for e in range(N):
            s = cols[e]
            assert raw(rg, e) == raw(tw, s), f"{scenario}, tick {t}: state of env {e} against the twin's env {s}"
            assert extra_state(rg, scenario, e) == extra_state(tw, scenario, s), f"{scenario}, tick {t}: scenario state of env {e}"
            assert rf[e * A:(e + 1) * A].tobytes() == rt[s * A:(s + 1) * A].tobytes() and df[e] == dt[s], f"{scenario}, tick {t}: outputs of env {e}"
            assert np.array_equal(frames_of(rg, A, e), frames_of(tw, A, s)), f"{scenario}, tick {t}: frames of env {e}"
    for g in gyms:
        g.close()


# ---- 3. a fork map gives a fork --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device_map", "host_map"])
@pytest.mark.parametrize("scenario", ["TowerBuilding", "HexMemory"])
def test_a_fork_map_gives_a_fork(hip, scenario, form):
    """3. resample_envs(MAP) on one gym, fork_envs(MAP) on its twin: all eight snapshots are identical, and so are the identities"""
    A, T = 1, 8
    script = make_script(31, T, N * A)
    gyms = [make_gym(scenario, A, "fast"), make_gym(scenario, A, "fast")]
    for t in range(T):
        for g in gyms:
            g.set_actions_batched(script[t]); g.step()
    rg, fg = gyms
    before = assert_all_states_differ(rg, scenario)
    rg.resample_envs(device_map(MAP) if form == "device_map" else MAP)
    fg.fork_envs(MAP)
    cols = columns(MAP)
    for e in range(N):
        assert raw(rg, e) == raw(fg, e) == before[cols[e]], f"{scenario}: env {e}"
    assert rg.debug_episodes_consumed().tolist() == fg.debug_episodes_consumed().tolist()
    for g in gyms:
        assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()
    for e in range(N):
        assert raw(rg, e) == raw(fg, e), f"{scenario}: env {e} a tick later"
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
def test_resample_between_batched_calls_without_host_sync(hip, scenario, overlap, depth, form):
    """4. step_n(8, 'sequence'), the map written by a torch kernel on the gym's stream, resample_envs(tensor), step_n(8, 'sequence') -- nothing synchronises
    in between: every ring entry and the final state equal a twin that synchronises around each of the three.  host_map: the same with the map as a list."""
    import torch
    A, K, cols = 1, 8, PERM_COLS
    script = remap(make_script(17, 2 * K, N * A), cols, A, K)
    dev_script = torch.as_tensor(script).to("cuda:0")
    map_src = torch.as_tensor(np.array(PERM, np.int32)).to("cuda:0")
    out = []
    for sync in (False, True):
        g = make_gym(scenario, A, "fast")
        rings = rings_of(torch, depth, A)
        g.set_output_ring(depth, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
        if overlap:
            g.set_pass_overlap(True)
        g.set_action_ring(2 * K, dev_script.data_ptr())
        dev_map = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")   # (would move nothing, were it read before the kernel below has run)
        torch.cuda.synchronize()
        g.step_n(K, "sequence", 0, 0)
        if sync:
            g.synchronize()
        torch.add(map_src, 0, out=dev_map)   # (the gym's stream is torch's current one: the null stream)
        g.resample_envs(dev_map if form == "device_map" else PERM)
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
    # ... and the resampling happened: the two envs that drew env 6 ran one episode on one column of actions, everybody else differs
    assert sa[6] == sa[7] and len(set(sa)) == len(set(cols)) == N - 1


# ---- 5. two calls back to back -------------------------------------------------------------------------------------------------------------------------
def test_two_calls_back_to_back(hip):
    """5. resample_envs(PERM), then resample_envs(DRAW) with no step between them, both from device maps: the result is the composition -- the second call
    reads what the first one committed, and the staging arena serves both"""
    A, T = 1, 8
    g = make_gym("TowerBuilding", A, "fast")
    script = make_script(37, T, N * A)
    for t in range(T):
        g.set_actions_batched(script[t]); g.step()
    before = assert_all_states_differ(g, "two calls")
    first, second = device_map(PERM), device_map(DRAW)
    g.resample_envs(first)
    bytes_after_first = g.resample_staging_bytes()
    g.resample_envs(second)
    assert g.resample_staging_bytes() == bytes_after_first > 0
    cols = compose(PERM, DRAW)
    for e in range(N):
        assert raw(g, e) == before[cols[e]], f"env {e}: expected the state of env {cols[e]}"
    assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()
    g.synchronize()
    g.close()


# ---- 6. 1024 envs --------------------------------------------------------------------------------------------------------------------------------------
def test_a_full_random_map_over_1024_envs(hip):
    """6. TowerBuilding, 1024 envs, every env draws its source uniformly: 4096 workgroups per phase, more than one round on the device.  Every env's
    snapshot is the pre-call snapshot of the env it drew."""
    n, A, T = 1024, 1, 8
    m = np.random.default_rng(7).integers(0, n, n).astype(np.int32)
    g = make_gym("TowerBuilding", A, "fast", n=n)
    script = make_script(41, T, n * A)
    for t in range(T):
        g.set_actions_batched(script[t]); g.step()
    before = assert_all_states_differ(g, "1024 envs", n)
    import torch
    dev = torch.as_tensor(m).to("cuda:0")
    torch.cuda.synchronize()
    g.resample_envs(dev)
    wrong = [e for e in range(n) if raw(g, e) != before[int(m[e])]]
    assert not wrong, f"{len(wrong)} envs do not hold the state of the env they drew, the first: {wrong[:8]}"
    assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()
    g.synchronize()
    g.close()


# ---- 7. identity is kept; the episode log --------------------------------------------------------------------------------------------------------------
SHORT = {"episodeLengthSec": 2.0}
CALL_TICK = 5
MAX_TICKS = 6000   # (TowerBuilding adds 4 s per object to episodeLengthSec: up to ~300 s of 15 ticks)
LOG_A = 3          # an odd agent count: the log's accumulators are no 16-byte rows and take the dword path


def run_until_everyone_finished(g, A, at_tick=None, call=None):
    """idle ticks until every env has finished once, and one tick more -> per-tick rewards / dones / true objectives, and each env's snapshot and
    episodes_consumed right behind the tick that finished its first episode (the first state of the next episode of its own sequence)"""
    rewards, dones, tobj, first = [], [], [], {}
    extra = 0
    for t in range(MAX_TICKS):
        if at_tick is not None and t == at_tick:
            call(g)
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
def unresampled_twin(scenario, A):
    g = make_gym(scenario, A, "fast", SHORT)
    out = run_until_everyone_finished(g, A)
    assert g._lib.mv_step_no_render(g._g) == 0
    g.close()
    return out


def test_identity_is_kept_and_the_log_follows(hip):
    """7. the episode log on, three agents per env, episodeLengthSec 2.0, idle actions, resample_envs(PERM) at tick 5.  Right after the call the running
    returns and lengths are the pre-call ones permuted, episodes_consumed is unchanged.  Then until every env has finished once and one tick more: every env
    took the next episode of its OWN sequence -- its snapshot right behind its finishing tick and its episodes_consumed are the unresampled twin's right
    behind that env's finishing tick -- the drained records equal a numpy model over the per-tick outputs the twin's episodes imply, and nothing starved."""
    scenario, A, cols = "TowerBuilding", LOG_A, PERM_COLS
    tw_rew, tw_done, tw_tobj, tw_first = unresampled_twin(scenario, A)
    assert not tw_done[:CALL_TICK + 1].any(), "an env finished before the call"
    g = make_gym(scenario, A, "fast", SHORT, log=4096)
    seen = {}

    def call(g):
        """the call, with recognisable values in the accumulators around it (five idle ticks leave every return at zero and every length at 5: permuting those
        would show nothing); afterwards the accumulators hold what the call makes of their real values"""
        import torch
        rt, lt = g.episode_returns_tensor(), g.episode_lengths_tensor()
        ret0, len0, consumed = rt.cpu().numpy(), lt.cpu().numpy(), g.debug_episodes_consumed()
        assert (len0 == CALL_TICK).all()
        marks_r, marks_l = np.arange(N * A, dtype=np.float64) + 0.25, 100 + np.arange(N, dtype=np.int32)
        rt.copy_(torch.as_tensor(marks_r)); lt.copy_(torch.as_tensor(marks_l))
        torch.cuda.synchronize()
        g.resample_envs(PERM)
        g.synchronize()
        seen["ret"], seen["len"] = (marks_r, rt.cpu().numpy()), (marks_l, lt.cpu().numpy())
        seen["consumed"] = (consumed, g.debug_episodes_consumed())
        rt.copy_(torch.as_tensor(ret0.reshape(N, A)[cols].reshape(-1).copy())); lt.copy_(torch.as_tensor(len0[cols].copy()))
        torch.cuda.synchronize()

    rew, done, tobj, first = run_until_everyone_finished(g, A, at_tick=CALL_TICK, call=call)
    assert seen["ret"][1].tobytes() == seen["ret"][0].reshape(N, A)[cols].tobytes(), "running returns right after the call"
    assert seen["len"][1].tobytes() == seen["len"][0][cols].tobytes(), "running lengths right after the call"
    assert seen["consumed"][0].tolist() == seen["consumed"][1].tolist() == [1] * N
    for e in range(N):
        t, snap, consumed = first[e]
        assert t == tw_first[cols[e]][0], f"env {e} finished at tick {t}, the episode it drew ends at {tw_first[cols[e]][0]}"
        assert snap == tw_first[e][1], f"env {e}: the episode after the resampled one is not the next one of its own sequence"
        assert consumed == tw_first[e][2] == 2
    # what the gym's outputs must have been: env e played the first episode of env cols[e] (the public outputs are per tick: before the call they were env e's
    # own), then the episodes of its own sequence, which the twin played from another tick on -- idle actions: the same ticks, shifted
    T = done.shape[0]
    for e in range(N):
        s, end_s, end_e = cols[e], tw_first[cols[e]][0], tw_first[e][0]
        ea, sa = slice(e * A, (e + 1) * A), slice(s * A, (s + 1) * A)
        own = (tw_rew[end_e + 1:, ea], tw_done[end_e + 1:, e])
        head = [tw_rew[:end_s + 1, sa].copy(), tw_done[:end_s + 1, s].copy()]
        head[0][:CALL_TICK], head[1][:CALL_TICK] = tw_rew[:CALL_TICK, ea], tw_done[:CALL_TICK, e]
        n = min(T - (end_s + 1), own[0].shape[0])
        want_rew, want_done = np.concatenate([head[0], own[0][:n]]), np.concatenate([head[1], own[1][:n]])
        known = end_s + 1 + n
        assert rew[:known, ea].tobytes() == want_rew.tobytes() and np.array_equal(done[:known, e], want_done), f"outputs of env {e}"
    # the log: the running return continues from the source's at the call -- model: env e's rewards before the call are those of the env it drew
    model_rew = rew.copy()
    for e in range(N):
        model_rew[:CALL_TICK, e * A:(e + 1) * A] = tw_rew[:CALL_TICK, cols[e] * A:(cols[e] + 1) * A]
    records, ret, length = log_model(model_rew, done, tobj, A)
    got = g.drain_episode_log()
    assert g.episode_log_dropped == 0 and len(got) == len(records) >= N * A
    for r, w in zip(got, records):
        assert (int(r["agent"]), int(r["length"]), int(r["end_tick"])) == w[:3], (r, w)
        assert np.float32(r["true_objective"]).tobytes() == np.float32(w[3]).tobytes() and np.float64(r["ret"]).tobytes() == np.float64(w[4]).tobytes(), (r, w)
    for e in range(N):   # the whole episode from its start in the env it was drawn from
        mine = [r for r in got if int(r["agent"]) == e * A]
        assert int(mine[0]["length"]) == tw_first[cols[e]][0] + 1 == int(mine[0]["end_tick"]) + 1
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == length.tobytes()
    assert g._lib.mv_step_no_render(g._g) == 0, g._lib.mv_last_error()   # nothing starved
    g.close()


# ---- 8. invalid entries on the device path -------------------------------------------------------------------------------------------------------------
def test_invalid_entries_are_skipped_and_reported_once(hip):
    """8. a device map with an index of N and one of -5: those two envs stay byte for byte what they were, the entries that name them still receive their
    pre-call state, the swap in the same map is applied, the next step returns 1 once with a text that names mv_resample_envs, the call after it 0"""
    bad = [1, 0, N, 2, -1, -5, 5, -1]
    g = make_gym("TowerBuilding", 1, "fast")
    script = make_script(19, 8, N)
    for t in range(8):
        g.set_actions_batched(script[t]); g.step()
    before = assert_all_states_differ(g, "invalid entries")
    g.resample_envs(device_map(bad))
    after = [raw(g, e) for e in range(N)]
    for e in (2, 5, 4, 7):
        assert after[e] == before[e], f"env {e} changed"
    assert after[3] == before[2] and after[6] == before[5], "an entry that names a skipped env did not receive that env's state"
    assert after[0] == before[1] and after[1] == before[0], "the swap was not applied"
    lib = g._lib
    assert lib.mv_step(g._g) == 1
    text = lib.mv_last_error().decode()
    assert "mv_resample_envs" in text and "out of range" in text and "mv_fork_envs" not in text, text
    assert lib.mv_step(g._g) == 0
    # a valid device map reports nothing
    g.resample_envs(device_map(PERM))
    assert lib.mv_step(g._g) == 0 and lib.mv_step(g._g) == 0
    g.synchronize()
    g.close()


# ---- 9. refusals; the staging arena --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_staging_memory(hip):
    """9. before the first reset; on a gym in a group; the host form on an index out of range: -1 with text, the state unchanged; a null map; a closed gym.
    The staging arena: nothing before the first call, N x bytes per env or more after it, counted in mv_arena_bytes."""
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    with pytest.raises(RuntimeError, match="mv_reset"):
        g.resample_envs(PERM)
    g.seed(42); g.reset()
    before = [raw(g, e) for e in range(N)]
    arena = g.arena_bytes()
    assert g.resample_staging_bytes() == 0
    with pytest.raises(RuntimeError, match="out of range"):
        g.resample_envs([1, 0, 3, N, 2, 7, -1, 6])
    with pytest.raises(RuntimeError, match="out of range"):
        g.resample_envs([1, 0, 3, -2, 2, 7, -1, 6])
    assert g._lib.mv_resample_envs(g._g, None) < 0 and b"null map" in g._lib.mv_last_error()
    assert g._lib.mv_resample_envs_host(g._g, None) < 0 and b"null map" in g._lib.mv_last_error()
    assert [raw(g, e) for e in range(N)] == before
    g.resample_envs([-1] * N)   # leaves everyone alone: nothing is launched
    assert [raw(g, e) for e in range(N)] == before
    g.step()
    other = make_gym("ObstaclesEasy", 1, "fast")
    grp = GymGroup([g, other])
    with pytest.raises(RuntimeError, match="mv_group"):
        g.resample_envs(PERM)
    grp.close()
    before = [raw(g, e) for e in range(N)]
    g.resample_envs(PERM)   # on its own again
    assert [raw(g, e) for e in range(N)] == [before[c] for c in PERM_COLS]
    staging = g.resample_staging_bytes()
    assert staging >= N * g.fork_bytes_per_env() and g.arena_bytes() == arena + staging
    g.set_episode_log(64)   # the arena was sized for the log's accumulators: switching it on later moves them through it as well
    grown = g.arena_bytes()
    g.resample_envs(DRAW)
    assert g.resample_staging_bytes() == staging and g.arena_bytes() == grown
    g.step()
    g.synchronize()
    g.close(); other.close()
    with pytest.raises(RuntimeError, match="closed"):
        g_closed = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
        handle = g_closed._g
        g_closed._lib.mv_close(handle)
        try:
            g_closed.resample_envs(PERM)
        finally:
            g_closed.close()


def test_env_resample_and_swap(hip):
    """MegaverseEnv.swap and MegaverseEnv.resample"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("TowerBuilding", N, 1, 1, False, None, img_w=W, img_h=H)
    env.env.set_pixel_mode("fast")
    env.seed(3)
    env.reset()
    script = make_script(29, 4, N)
    for t in range(4):
        env.step_device(script[t])
    before = assert_all_states_differ(env.env, "MegaverseEnv.swap")
    env.swap(2, 6)
    assert [raw(env.env, e) for e in range(N)] == [before[{2: 6, 6: 2}.get(e, e)] for e in range(N)]
    env.swap(6, 2)
    assert [raw(env.env, e) for e in range(N)] == before
    env.resample(DRAW)
    assert [raw(env.env, e) for e in range(N)] == [before[c] for c in DRAW_COLS]
    env.close()
