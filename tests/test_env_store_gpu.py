"""Env stores on the GPU (include/megaverse_hip.h: mv_save_envs / mv_load_envs): an env's episode state saved into a record of a caller-owned store and
loaded back -- into the same env later, into other envs, into another gym.

Every test uses 8 envs, 64 x 36 frames and the helpers of tests/test_fork_gpu.py: envs are driven by their own columns of a scripted action stream, so all
eight states differ (asserted); no env may finish inside a window (asserted).  Expected values come from the CPU oracle, which is never saved or loaded: it
just runs the script.  The only "bad" records are zeroed slots and genuine records of gyms of another configuration."""
import numpy as np
import pytest

import test_fork_gpu as F
from action_ring_util import make_script
from fork_util import H, MAP, N, W, columns, log_model, remap  # noqa: F401
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import GymGroup, MegaverseGym

pytestmark = pytest.mark.gpu

COLS = columns(MAP)
LOAD_MAP = [s if s >= 0 else -1 for s in MAP]   # env d continues record MAP[d], where env MAP[d] was saved; entry 4 loads its own record
LOADED = [e for e in range(N) if LOAD_MAP[e] >= 0]
OWN_SLOTS = list(range(N))
assert LOAD_MAP == [-1, 0, 0, 7, 4, 7, -1, -1] and LOADED == [1, 2, 3, 4, 5]


def gym_bytes(g, scenario=""):
    """everything of a gym a test can see: every env's snapshot and scenario state, the public outputs, the identity's counts"""
    g.synchronize()
    return ([F.raw(g, e) for e in range(g.num_envs)], [F.extra_state(g, scenario, e) for e in range(g.num_envs)], g.get_rewards_array().tobytes(),
            g.get_dones().tobytes(), g.get_true_objectives().tobytes(), g.debug_episodes_consumed().tobytes())


def store_bytes(g, store):
    g.synchronize()
    return store.cpu().numpy().copy()


# ---- 1. a load is a fork from a record: against the oracle, exact pixels -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(F.ORACLE_CASES))
def test_load_is_a_fork_from_a_record(hip, case, monkeypatch):
    """1. T1 scripted ticks, every env saved to its own slot of a 16-slot store (the gym does not change), the load of the slots MAP implies: right behind it
    env d is what env COLS[d] was at the save, and for T2 ticks env e is the oracle's env COLS[e] -- snapshot, rewards, dones, true objectives, frames"""
    monkeypatch.setenv("BOXOBAN_LEVELS", F.BOXOBAN)
    scenario, A = F.ORACLE_CASES[case]
    T = F.window(scenario)
    script = make_script(11, 2 * T, N * A)
    forked = remap(script, COLS, A, T)
    hg, og = F.make_gym(scenario, A, "exact"), F.make_oracle(scenario, A)
    for t in range(T):
        hg.set_actions_batched(script[t]); hg.step()
        F.oracle_act(og, A, script[t]); og.step_norender()
        assert not hg.get_dones().any() and not og.get_dones().any(), f"an env finished before the save (tick {t})"
    before = F.assert_all_states_differ(hg, case)
    store = hg.new_env_store(16)
    assert tuple(store.shape) == (16, hg.env_record_bytes()) and hg.env_record_bytes() % 16 == 0 and hg.env_record_layout() != 0
    whole = gym_bytes(hg, scenario)
    hg.save_envs(OWN_SLOTS, store)
    assert gym_bytes(hg, scenario) == whole, f"{case}: the save changed the gym"
    hg.load_envs(LOAD_MAP, store)
    for e in range(N):
        assert F.raw(hg, e) == before[COLS[e]], f"{case}: env {e} right after the load"
    for t in range(T, 2 * T):
        hg.set_actions_batched(forked[t]); hg.step()
        F.oracle_act(og, A, script[t]); og.step()
        assert not hg.get_dones().any() and not og.get_dones().any(), f"an env finished inside the window (tick {t})"
        for e in range(N):
            F.check_against_oracle(hg, og, A, e, COLS[e], f"{case}, tick {t}", boxagone=scenario == "BoxAGone", football=scenario == "Football")
    hg.close(); og.close()


# ---- 2. time travel: every source was overwritten long ago ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 1), ("Collect", 1), ("HexMemory", 1), ("Football", 2)])
def test_time_travel(hip, scenario, A):
    """2. all envs saved at tick T1, T2 scripted ticks recorded (the oracle checked on the way), all envs loaded back, ticks T1 .. T1 + T2 replayed: every
    recorded byte repeats"""
    T = F.window(scenario)
    script = make_script(11, 2 * T, N * A)
    hg, og = F.make_gym(scenario, A, "exact"), F.make_oracle(scenario, A)
    for t in range(T):
        hg.set_actions_batched(script[t]); hg.step()
        F.oracle_act(og, A, script[t]); og.step_norender()
    F.assert_all_states_differ(hg, scenario)
    store = hg.new_env_store(N)
    hg.save_envs(OWN_SLOTS, store)

    def play(with_oracle):
        seen = []
        for t in range(T, 2 * T):
            hg.set_actions_batched(script[t]); hg.step()
            assert not hg.get_dones().any(), f"an env finished inside the window (tick {t})"
            if with_oracle:
                F.oracle_act(og, A, script[t]); og.step()
                for e in range(N):
                    F.check_against_oracle(hg, og, A, e, e, f"{scenario}, tick {t}", football=scenario == "Football")
            seen.append(([F.raw(hg, e) for e in range(N)], [F.extra_state(hg, scenario, e) for e in range(N)], hg.get_rewards_array().tobytes(),
                         hg.get_dones().tobytes(), [F.frames_of(hg, A, e).tobytes() for e in range(N)]))
        return seen

    first = play(True)
    hg.load_envs(OWN_SLOTS, store)
    again = play(False)
    for t, (x, y) in enumerate(zip(first, again)):
        assert x == y, f"{scenario}: tick {T + t} did not repeat after the load"
    hg.close(); og.close()


# ---- 3. more states than envs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 1), ("ObstaclesEasy", 2)])
def test_more_states_than_envs(hip, scenario, A):
    """3. a 24-slot store holds all envs at three ticks; then env e takes tick t[e % 3]'s record of env (e + 3) % 8: it is the matching env of an oracle gym
    stopped at that tick, right away and through 4 more ticks"""
    ticks, more = [3, 6, 9], 4
    script = make_script(31, ticks[-1] + more, N * A)
    hg = F.make_gym(scenario, A, "exact")
    store = hg.new_env_store(3 * N)
    oracles = []
    for t in range(ticks[-1]):
        hg.set_actions_batched(script[t]); hg.step()
        assert not hg.get_dones().any()
        if t + 1 in ticks:
            k = ticks.index(t + 1)
            hg.save_envs([k * N + e for e in range(N)], store)
            og = F.make_oracle(scenario, A)
            for u in range(t + 1):
                F.oracle_act(og, A, script[u]); og.step_norender()
                assert not og.get_dones().any()
            oracles.append(og)
    src = [(e + 3) % N for e in range(N)]
    which = [e % 3 for e in range(N)]
    hg.load_envs([which[e] * N + src[e] for e in range(N)], store)
    for e in range(N):
        assert diff_snapshots(oracles[which[e]].snapshot(src[e]), hip_snapshot(hg, e), A) == [], f"{scenario}: env {e} right after the load"
    for j in range(more):
        actions = np.zeros((N * A, 6), np.int32)
        for e in range(N):
            actions[e * A:(e + 1) * A] = script[ticks[which[e]] + j][src[e] * A:(src[e] + 1) * A]
        hg.set_actions_batched(actions); hg.step()
        assert not hg.get_dones().any()
        for k, og in enumerate(oracles):
            F.oracle_act(og, A, script[ticks[k] + j]); og.step()
        for e in range(N):
            F.check_against_oracle(hg, oracles[which[e]], A, e, src[e], f"{scenario}, {j + 1} ticks after the load")
    hg.close()
    for og in oracles:
        og.close()


# ---- 4. through host memory into another gym -----------------------------------------------------------------------------------------------------------
def test_through_host_memory_into_another_gym(hip):
    """4. saved in gym X (8 envs, seed 42), the store moved through host memory, loaded into gym Y (4 envs, seed 7): Y's envs follow X's oracle envs tick for
    tick in exact pixels.  Gyms of another scenario and of another episodeLengthSec have other layout words; their loads are skipped and reported once."""
    import torch
    scenario, A, T = "TowerBuilding", 1, 12
    script = make_script(11, 2 * T, N * A)
    xg, og = F.make_gym(scenario, A, "exact"), F.make_oracle(scenario, A)
    for t in range(T):
        xg.set_actions_batched(script[t]); xg.step()
        F.oracle_act(og, A, script[t]); og.step_norender()
    store = xg.new_env_store(N)
    xg.save_envs(OWN_SLOTS, store)
    xg.synchronize()
    moved = store.cpu().to("cuda:0")
    assert moved.data_ptr() != store.data_ptr()
    yg = MegaverseGym(scenario, W, H, 4, A, 1, False, {})
    yg.set_pixel_mode("exact"); yg.seed(7); yg.reset()
    assert yg.env_record_layout() == xg.env_record_layout() and yg.env_record_bytes() == xg.env_record_bytes()
    takes = [5, 0, 7, 2]
    consumed = yg.debug_episodes_consumed().copy()
    yg.load_envs(takes, moved)
    for t in range(T, 2 * T):
        yg.set_actions_batched(np.concatenate([script[t][s * A:(s + 1) * A] for s in takes])); yg.step()
        F.oracle_act(og, A, script[t]); og.step()
        assert not yg.get_dones().any() and not og.get_dones().any()
        for d, s in enumerate(takes):
            F.check_against_oracle(yg, og, A, d, s, f"gym Y, tick {t}")
    assert np.array_equal(yg.debug_episodes_consumed(), consumed)
    # gyms of another configuration: the header keeps X's records out
    others = [MegaverseGym("ObstaclesEasy", W, H, 4, A, 1, False, {}), MegaverseGym(scenario, W, H, 4, A, 1, False, {"episodeLengthSec": 30.0}),
              MegaverseGym("ObstaclesHard", W, H, 4, A, 1, False, {})]
    words = {xg.env_record_layout()}
    for g in others:
        g.seed(7); g.reset(); g.step()
        assert g.env_record_layout() not in words, "two configurations share a layout word"
        words.add(g.env_record_layout())
        before = gym_bytes(g)
        slots = (moved.numel() // g.env_record_bytes())
        assert slots >= 2
        # (through the C ABI: the Python surface refuses a store whose second dimension is another gym's record size)
        m = np.array([0, -1, 1, -1], np.int32)
        assert g._lib.mv_load_envs_host(g._g, m.ctypes.data, moved.data_ptr(), slots) == 0, g._lib.mv_last_error()
        assert gym_bytes(g) == before, "a record of another configuration was loaded"
        assert g._lib.mv_step(g._g) == 1
        assert "mv_load_envs" in g._lib.mv_last_error().decode()
        assert g._lib.mv_step(g._g) == 0
    # ... and Obstacles records do not cross between variants either (same record size: the Python surface)
    easy, _, hard = others
    st = easy.new_env_store(4)
    easy.save_envs([0, 1, 2, 3], st)
    before = gym_bytes(hard)
    hard.load_envs([0, 1, 2, 3], st)
    assert gym_bytes(hard) == before
    with pytest.warns(RuntimeWarning, match="mv_load_envs"):
        hard.step()
    for g in others + [xg, yg]:
        g.synchronize(); g.close()
    og.close()


# ---- 5. identity is kept; the episode log ----------------------------------------------------------------------------------------------------------------
SAVE_TICK, LOAD_TICK = 3, 5
DELAY = LOAD_TICK - SAVE_TICK   # a loaded env replays the ticks between save and load: its episode ends that much later than its source's did


def run_until_everyone_finished(g, store, save_from=None):
    """F.run_until_everyone_finished with the save at tick 3 (from g, or from save_from, a gym stepped alongside until then) and the load at tick 5"""
    rewards, dones, tobj, first = [], [], [], {}
    extra = 0
    for t in range(F.MAX_TICKS):
        if t == SAVE_TICK:
            (save_from or g).save_envs(OWN_SLOTS, store)
        if t == LOAD_TICK:
            g.load_envs(LOAD_MAP, store)
        for x in [g] + ([save_from] if save_from is not None and t < SAVE_TICK else []):
            rc = x._lib.mv_step_no_render(x._g)
            assert rc == 0, (t, rc, x._lib.mv_last_error())
        d = g.get_dones()
        rewards.append(g.get_rewards_array()); dones.append(d); tobj.append(g.get_true_objectives())
        for e in np.flatnonzero(d):
            if int(e) not in first:
                first[int(e)] = (t, F.raw(g, int(e)), int(g.debug_episodes_consumed()[e]))
        if len(first) == N:
            extra += 1
            if extra == 2:
                break
    assert len(first) == N, "not every env finished"
    return np.stack(rewards), np.stack(dones), np.stack(tobj), first


@pytest.mark.parametrize("log", ["no_log", "episode_log", "saved_without_log"])
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_identity_is_kept(hip, scenario, log):
    """5. episodeLengthSec 2.0, idle actions, saved at tick 3, loaded at tick 5, until every env has finished once and one tick more: every env then took the
    next episode of its OWN sequence -- its snapshot right behind its finishing tick and its episodes_consumed are the unloaded twin's -- and nothing
    starved.  With the episode log: a loaded episode is logged from its record's start, the cut episode writes no record; a record saved with the log off
    counts from the load."""
    A = 1
    tw_rew, tw_done, tw_tobj, tw_first = F.unforked_twin(scenario)
    assert not tw_done[:LOAD_TICK + 1].any(), "an env finished before the load"
    g = F.make_gym(scenario, A, "fast", F.SHORT, log=0 if log == "no_log" else 4096)
    saver = F.make_gym(scenario, A, "fast", F.SHORT) if log == "saved_without_log" else None
    store = g.new_env_store(N)
    rew, done, tobj, first = run_until_everyone_finished(g, store, saver)
    if saver is not None:
        saver.synchronize(); saver.close()
    for e in range(N):
        t, snap, consumed = first[e]
        want = tw_first[COLS[e]][0] + (DELAY if e in LOADED else 0)
        assert t == want, f"env {e} finished at tick {t}, its record's episode ends at {want}"
        assert snap == tw_first[e][1], f"env {e}: the episode after the loaded one is not the next one of its own sequence"
        assert consumed == tw_first[e][2] == 2
    if log == "no_log":
        assert g._lib.mv_step_no_render(g._g) == 0, g._lib.mv_last_error()   # nothing starved
        g.close()
        return
    # The log's model: at the load env e's running return and length become its record's -- the source's first 3 ticks -- or, saved without the log, zero.
    # As per-tick rewards: the source's (or zero) in ticks 0 .. 2, zero in ticks 3 .. 4, and a first record that is shorter by the ticks not counted.
    model_rew = rew.copy()
    for e in LOADED:
        model_rew[:LOAD_TICK, e] = 0.0
        if saver is None:
            model_rew[:SAVE_TICK, e] = tw_rew[:SAVE_TICK, COLS[e]]
    records, ret, length = log_model(model_rew, done, tobj, A)
    uncounted = DELAY if saver is None else LOAD_TICK
    seen = set()
    for i, r in enumerate(records):
        if r[0] in LOADED and r[0] not in seen:
            seen.add(r[0])
            records[i] = (r[0], r[1] - uncounted) + r[2:]
    got = g.drain_episode_log()
    assert g.episode_log_dropped == 0 and len(got) == len(records) >= N
    for r, w in zip(got, records):
        assert (int(r["agent"]), int(r["length"]), int(r["end_tick"])) == w[:3], (r, w)
        assert np.float32(r["true_objective"]).tobytes() == np.float32(w[3]).tobytes() and np.float64(r["ret"]).tobytes() == np.float64(w[4]).tobytes(), (r, w)
    for e in LOADED:   # the whole episode from the record's start (or from the load), and no record of the cut one
        mine = [r for r in got if int(r["agent"]) == e]
        assert int(mine[0]["length"]) == tw_first[COLS[e]][0] + 1 - (0 if saver is None else SAVE_TICK)
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == length.tobytes()
    assert g._lib.mv_step_no_render(g._g) == 0, g._lib.mv_last_error()   # nothing starved
    g.close()


# ---- 6. between batched calls, without a host synchronisation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,overlap,form,render", [("TowerBuilding", False, "device_map", "every"), ("TowerBuilding", False, "host_map", "every"),
                                                          ("ObstaclesEasy", True, "device_map", "every"), ("ObstaclesEasy", True, "host_map", "every"),
                                                          ("TowerBuilding", False, "device_map", "none")])
def test_save_and_load_between_batched_calls_without_host_sync(hip, scenario, overlap, form, render):
    """6. step_n(8), the save map written by a torch kernel on the gym's stream, save_envs, step_n(8), the load map likewise, load_envs, step_n(8) --
    nothing synchronises in between: every ring entry, the store and the final state equal a twin that synchronises around each call, launch for launch"""
    import torch
    A, K, depth = 1, 8, 32
    script = remap(make_script(17, 3 * K, N * A), COLS, A, 2 * K)
    dev_script = torch.as_tensor(script).to("cuda:0")
    save_src = torch.as_tensor(np.array(OWN_SLOTS, np.int32)).to("cuda:0")
    load_src = torch.as_tensor(np.array(LOAD_MAP, np.int32)).to("cuda:0")
    out = []
    for sync in (False, True):
        g = F.make_gym(scenario, A, "fast")
        rings = F.rings_of(torch, depth, A)
        g.set_output_ring(depth, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
        if overlap:
            g.set_pass_overlap(True)
        g.set_action_ring(3 * K, dev_script.data_ptr())
        store = g.new_env_store(N)
        save_map = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")   # (would do nothing, were they read before the kernels below have run)
        load_map = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        counts = g.debug_launch_counts()

        def pause():
            if sync:
                g.synchronize()

        g.step_n(K, "sequence", 0, 0, render=render); pause()
        torch.add(save_src, 0, out=save_map)   # (the gym's stream is torch's current one: the null stream)
        g.save_envs(save_map if form == "device_map" else OWN_SLOTS, store); pause()
        g.step_n(K, "sequence", 0, K, render=render); pause()
        torch.add(load_src, 0, out=load_map)
        g.load_envs(load_map if form == "device_map" else LOAD_MAP, store); pause()
        g.step_n(K, "sequence", 0, 2 * K, render=render)
        g.synchronize()
        after = g.debug_launch_counts()
        out.append(([r.cpu().numpy() for r in rings], [F.raw(g, e) for e in range(N)], store.cpu().numpy(), (after[0] - counts[0], after[1] - counts[1])))
        assert not out[-1][0][2][:3 * K].any(), "an env finished inside the window"
        g.close()
    (ra, sa, ta, ca), (rb, sb, tb, cb) = out
    for x, y, name in zip(ra, rb, ("observations", "rewards", "dones")):
        assert x.tobytes() == y.tobytes(), f"{scenario}: {name} rings differ from the synchronised twin's"
    assert sa == sb, f"{scenario}: final state differs from the synchronised twin's"
    for t in (ta, tb):   # (the identity's dwords of the EnvHeader travel in a record and are ignored by a load: an unseeded header seed differs per gym)
        t.view(np.uint32)[:, [16 + i for i in (19, 20, 28, 29)]] = 0
    assert ta.tobytes() == tb.tobytes() and ta.any(), f"{scenario}: the store differs from the synchronised twin's"
    assert ca == cb, f"{scenario}: launches {ca}, the synchronised twin's {cb}: a batched path was left"
    # ... and the load happened: envs that took one record ran it on the same actions, eight ticks behind the env that was saved
    assert sa[1] == sa[2] and sa[3] == sa[5] and sa[1] != sa[0] and sa[3] != sa[7]


# ---- 7. invalid entries on the device path -------------------------------------------------------------------------------------------------------------
def stepped_gym(ticks=8):
    g = F.make_gym("TowerBuilding", 1, "fast")
    script = make_script(19, ticks, N)
    for t in range(ticks):
        g.set_actions_batched(script[t]); g.step()
    return g, F.assert_all_states_differ(g, "invalid entries")


def reports_once(g, name):
    lib = g._lib
    assert lib.mv_step(g._g) == 1
    text = lib.mv_last_error().decode()
    assert name in text, text
    assert lib.mv_step(g._g) == 0


def test_invalid_save_entries_are_skipped_and_reported_once(hip):
    """7a. a device save map with an index of `slots` and two envs on one slot: those slots keep their bytes, the valid entries are written, the gym does not
    change, the next step returns 1 once with a text naming the call"""
    import torch
    g, before = stepped_gym()
    store = g.new_env_store(16)
    store.fill_(0xAB)
    whole = gym_bytes(g)
    dev_map = torch.as_tensor(np.array([0, 16, 5, 5, -1, 2, -1, -1], np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    g.save_envs(dev_map, store)
    assert gym_bytes(g) == whole
    got = store_bytes(g, store)
    for m in range(16):
        if m not in (0, 2):
            assert (got[m] == 0xAB).all(), f"slot {m} was written"
    assert got[0][:4].view(np.uint32)[0] == 0x5652454D and got[2][:4].view(np.uint32)[0] == 0x5652454D
    reports_once(g, "mv_save_envs")
    # the two records are whole: loaded into envs 6 and 7 of a gym brought to the same tick they are envs 0 and 5
    g2, before2 = stepped_gym()
    g2.load_envs([-1, -1, -1, -1, -1, -1, 0, 2], store)
    assert F.raw(g2, 6) == before2[0] == before[0] and F.raw(g2, 7) == before2[5]
    assert g2._lib.mv_step(g2._g) == 0
    for x in (g, g2):
        x.synchronize(); x.close()


@pytest.mark.parametrize("form", ["device_map", "host_map"])
def test_invalid_load_entries_are_skipped_and_reported_once(hip, form):
    """7b. a load map that names a never-written (zeroed) slot -- and, on the device path, an index of -2: those envs stay byte for byte, the valid entry
    is applied, the next step returns 1 once with a text naming the call.  The host form relies on the kernel's header check in the same way."""
    import torch
    g, before = stepped_gym()
    store = g.new_env_store(16)
    g.save_envs([0, -1, -1, -1, -1, -1, -1, -1], store)
    bad = [-2 if form == "device_map" else -1, 9, 0, -1, -1, -1, -1, -1]
    if form == "device_map":
        dev_map = torch.as_tensor(np.array(bad, np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        g.load_envs(dev_map, store)
    else:
        g.load_envs(bad, store)
    after = [F.raw(g, e) for e in range(N)]
    for e in (0, 1, 3, 4, 5, 6, 7):
        assert after[e] == before[e], f"env {e} changed"
    assert after[2] == before[0], "the valid entry was not applied"
    reports_once(g, "mv_load_envs")
    # a valid map reports nothing
    g.save_envs(OWN_SLOTS, store)
    g.load_envs(torch.as_tensor(np.array(LOAD_MAP, np.int32)).to("cuda:0") if form == "device_map" else LOAD_MAP, store)
    assert g._lib.mv_step(g._g) == 0 and g._lib.mv_step(g._g) == 0
    g.synchronize(); g.close()


# ---- 8. refusals and host validation ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_host_validation(hip):
    """8. every refusal returns -1 with text and leaves the gym as it was; bad host maps raise and copy nothing; a host map of -1s launches nothing"""
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    lib = g._lib
    store = g.new_env_store(16)
    own = np.array(OWN_SLOTS, np.int32)
    forms = [lib.mv_save_envs_host, lib.mv_load_envs_host, lib.mv_save_envs, lib.mv_load_envs]

    def refused(fn, args, text):
        assert fn(*args) == -1 and text in lib.mv_last_error().decode(), (text, lib.mv_last_error())

    for fn in forms:
        refused(fn, (None, own.ctypes.data, store.data_ptr(), 16), "null gym")
        refused(fn, (g._g, own.ctypes.data, store.data_ptr(), 16), "mv_reset")   # before the first reset
    assert lib.mv_env_record_bytes(None) == -1 and lib.mv_env_record_layout(None) == 0
    g.seed(42); g.reset()
    before, zeros = gym_bytes(g), store_bytes(g, store)
    for fn in forms:
        refused(fn, (g._g, None, store.data_ptr(), 16), "null map")
        refused(fn, (g._g, own.ctypes.data, None, 16), "null store")
        refused(fn, (g._g, own.ctypes.data, store.data_ptr(), 0), "slots")
        refused(fn, (g._g, own.ctypes.data, store.data_ptr(), -3), "slots")
        refused(fn, (g._g, own.ctypes.data, store.data_ptr() + 8, 15), "16-byte aligned")
    # host validation
    with pytest.raises(RuntimeError, match="out of range"):
        g.save_envs([0, 1, 2, 16, -1, -1, -1, -1], store)
    with pytest.raises(RuntimeError, match="out of range"):
        g.save_envs([0, 1, 2, -2, -1, -1, -1, -1], store)
    with pytest.raises(RuntimeError, match="another env names too"):
        g.save_envs([0, 1, 2, 1, -1, -1, -1, -1], store)
    with pytest.raises(RuntimeError, match="out of range"):
        g.load_envs([0, 0, 0, 16, -1, -1, -1, -1], store)
    counts = g.debug_launch_counts()
    g.save_envs([-1] * N, store)
    g.load_envs([-1] * N, store)
    assert g.debug_launch_counts() == counts
    assert gym_bytes(g) == before and np.array_equal(store_bytes(g, store), zeros)
    g.step()
    # a gym in a group
    other = F.make_gym("ObstaclesEasy", 1, "fast")
    grp = GymGroup([g, other])
    for fn, name in zip((g.save_envs, g.load_envs), ("mv_save_envs_host", "mv_load_envs_host")):
        with pytest.raises(RuntimeError, match="mv_group"):
            fn(OWN_SLOTS, store)
    grp.close()
    g.save_envs(OWN_SLOTS, store)   # on its own again
    g.load_envs(LOAD_MAP, store)
    g.step()
    g.synchronize()
    # a closed gym
    handle = g._g
    lib.mv_close(handle)
    for fn in forms:
        refused(fn, (handle, own.ctypes.data, store.data_ptr(), 16), "closed")
    assert lib.mv_env_record_bytes(handle) == -1 and lib.mv_env_record_layout(handle) == 0
    g.close(); other.close()


# ---- 9. with a step mask -----------------------------------------------------------------------------------------------------------------------------------
def test_with_a_step_mask(hip):
    """9. env 0 frozen: a record loaded into it becomes its state, and it stays frozen; saving a frozen env yields the same record tick after tick"""
    g, before = stepped_gym()
    store = g.new_env_store(4)
    g.save_envs([-1, -1, -1, 0, -1, -1, -1, -1], store)   # env 3 -> record 0
    mask = np.ones(N, np.bool_); mask[0] = False
    g.set_step_mask(mask)
    g.load_envs([0, -1, -1, -1, -1, -1, -1, -1], store)
    assert F.raw(g, 0) == before[3]
    script = make_script(23, 4, N)
    for t in range(4):
        g.set_actions_batched(script[t]); g.step()
        assert F.raw(g, 0) == before[3], f"the frozen env moved (tick {t})"
        g.save_envs([1 + t % 2, -1, -1, -1, -1, -1, -1, -1], store)   # records 1 and 2 in turn
    got = store_bytes(g, store)
    assert got[1].tobytes() == got[2].tobytes() and got[1].any()
    assert F.raw(g, 3) != before[3], "the other envs did not step"
    # thawed, env 0 continues the record: it is env 3's twin one tick behind... it simply moves
    g.set_step_mask(None)
    g.set_actions_batched(script[0]); g.step()
    assert F.raw(g, 0) != before[3]
    g.synchronize(); g.close()


# ---- 10. the env surface -------------------------------------------------------------------------------------------------------------------------------------
def test_env_save_and_load(hip):
    """10. MegaverseEnv.save / load: a round trip with default and with explicit slots"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("TowerBuilding", N, 1, 1, False, None, img_w=W, img_h=H)
    env.env.set_pixel_mode("fast")
    env.seed(3)
    env.reset()
    script = make_script(29, 8, N)
    for t in range(4):
        env.step_device(script[t])
    before = F.assert_all_states_differ(env.env, "MegaverseEnv.save")
    store = env.new_store(12)
    env.save(range(N), store)                  # record e <- env e
    env.save([6, 2], store, slots=[8, 11])
    for t in range(4, 8):
        env.step_device(script[t])
    assert all(F.raw(env.env, e) != before[e] for e in range(N))
    env.load([1, 3], store)                    # default slots: their own records
    env.load([0, 5, 7], store, slots=[8, 11, 8])
    want = {1: 1, 3: 3, 0: 6, 5: 2, 7: 6}
    for e in range(N):
        if e in want:
            assert F.raw(env.env, e) == before[want[e]], f"env {e}"
        else:
            assert F.raw(env.env, e) != before[e]
    env.close()
