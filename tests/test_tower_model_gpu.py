"""TowerBuilding's stacking rules on the device: the HIP gym through the scripted cases of tests/tower_cases.py under the float64 model (tests/tower_model.py:
rules (E), (R), (U)) tick by tick -- step_kernel<1> and step_kernel<MAX_AGENTS> -- and bit-equal to the CPU oracle as well; then the launch shapes: the
same scripts out of a device action ring, one batched call per segment, and with the Tower gym as one member of a MultiTaskGym beside an Empty gym: the
rewards of every tick and the final state equal the tick-by-tick run the model judged.  Which kernel a replay reaches (mv_step.hip: launch_step_ticks,
mv_api_step.hip: the call's plan):
    one agent per env, MV_STEP_PIPE=0     step_ticks_kernel, the one-wave kernel a Tower gym of more than 512 envs takes     sweep, tower_a1, stress_a1
    one agent per env, MV_STEP_PIPE=1     step_ticks_pipe_kernel, the two-wave kernel gyms of up to 512 envs take            sweep, tower_a1, stress_a1
    several agents per env                step_ticks_agents_kernel                                                          tower_a4, order, stress_a4
    (mv_set_pipelining only chooses the stream the step launch goes to; every variant is also replayed with it off)
    a group, one agent per env, fast pixels, rings k deep: step_union_ticks_kernel, one step launch per call                sweep, tower_a1, stress_a1
    a group otherwise: step_union_kernel, one step launch per tick             tower_a4, order, stress_a4; tick by tick: order, tower_a1, tower_a4
Every replay asserts the step launches it took (mv_debug_launch_counts).  And the two debug setters against their oracle twins."""
import functools

import numpy as np
import pytest

import oracle_lib
import tower_cases as TC
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MegaverseGym

pytestmark = pytest.mark.gpu

REPLAY = [n for n, c in TC.CASES.items() if c.replay]
GROUP = dict(env_offset=0, env_stride=2)   # how a MultiTaskGym of two scenarios creates its first member


def final_state(g, N):
    return [g.debug_snapshot_bytes(e).tobytes() for e in range(N)]


@functools.lru_cache(maxsize=None)
def hip_run(name, group=False):
    """the HIP gym through a case tick by tick under the model, once -> (judge, [ticks] rewards, the final snapshots' bytes)"""
    case = TC.CASES[name]
    g = case.make(MegaverseGym, **(dict(GROUP, total_envs=2 * case.N) if group else {}))
    judge, rewards = TC.run_judged(case, g)
    out = judge, rewards, final_state(g, case.N)
    g.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    case = TC.CASES[name]
    g = case.make(oracle_lib.OracleGym)
    rewards = []
    for what, _ in TC.play(case, g):
        if what == "tick":
            rewards.append(g.get_last_rewards().copy())
    snaps = [g.snapshot(e).copy() for e in range(case.N)]
    g.close()
    return rewards, snaps


def test_setters_match_their_oracle_twins(hip):
    """identical setter calls on a HIP gym and an oracle gym: no snapshot difference, one exact-mode frame byte-equal; bz_reward is the kernel's own sum;
    inconsistent input is refused with a text that names the call, and changes nothing"""
    N, A = 2, 2
    og = oracle_lib.OracleGym("TowerBuilding", 64, 36, N, A, 1, False, {})
    hg = MegaverseGym("TowerBuilding", 64, 36, N, A, 1, False, {})
    hg.set_pixel_mode("exact")
    for g in (og, hg):
        g.seed(42)
        g.reset()
    rooms = [TC.Room(og.snapshot(e)) for e in range(N)]
    for e, r in enumerate(rooms):
        zc = r.zone_cells()
        objs = [[c[0], 1 + k % 3, c[1], 0] for k, c in enumerate(zc[:9])] + [[0, 0, 0, 2]] + TC.fillers(r, 60, avoid=zc) + [[zc[0][0], 12, zc[0][1], 0]]
        for g in (og, hg):
            g.debug_set_objects(e, objs)
            g.debug_set_agent_pitch(e, 0, 0.35)
            g.debug_set_agent_pitch(e, 1, -0.5)
    for g in (og, hg):
        g.step()
    for e in range(N):
        s = hip_snapshot(hg, e)
        assert diff_snapshots(og.snapshot(e), s, A) == [], e
        assert int(s["num_objects"]) == 71 and int(s["agents"][1]["carrying"]) == 9 and int(s["agents"][0]["carrying"]) == -1
        assert float(s["bz_reward"]) > 20.0   # (the box at y = 12 is in the sum, index 70: the second register slot)
        for a in range(A):
            assert np.array_equal(og.get_observation(e, a), hg.get_observation(e, a)), (e, a)
    before = hg.debug_snapshot_bytes(0).tobytes()
    for bad, text in (([[0, 0, 0, 1], [0, 0, 0, 1]], "two objects are carried"), ([[0, 0, 0, 3]], "does not have"),
                      ([[3, 1, 3, 0], [3, 1, 3, 0]], "share a voxel"), ([[0, 1, 3, 0]], "solid voxel"), ([[2, 4, 2, 0]] * 81, "bad arguments")):
        with pytest.raises(RuntimeError, match="mv_debug_set_objects: .*" + text):
            hg.debug_set_objects(0, bad)
        with pytest.raises(RuntimeError):
            og.debug_set_objects(0, bad)
    with pytest.raises(RuntimeError, match="mv_debug_set_agent_pitch"):
        hg.debug_set_agent_pitch(0, A, 0.0)
    assert hg.debug_snapshot_bytes(0).tobytes() == before
    hg.debug_set_objects(1, [])
    og.debug_set_objects(1, [])
    assert diff_snapshots(og.snapshot(1), hip_snapshot(hg, 1), A) == []
    og.close(); hg.close()
    other = MegaverseGym("ObstaclesEasy", 32, 32, 1, 1, 1, False, {})
    other.seed(1); other.reset()
    with pytest.raises(RuntimeError, match="mv_debug_set_objects: not a TowerBuilding gym"):
        other.debug_set_objects(0, [])
    other.close()


def judged(name, judge):
    c = judge.counts()
    print(f"\n[tower model, HIP] {name}: interact ticks {judge.interact_ticks}, judged {judge.judged}, fragile {judge.fragile}, finished {judge.finished}, rewards "
          f"unjudged {judge.reward_unjudged}, respawns {judge.respawns}, largest reward error / bound {judge.worst_ratio:.3f}, {c}")
    assert judge.failures == [], judge.failures[:10]
    assert judge.respawns == 0 and judge.interact_ticks > 0
    return c


@pytest.mark.parametrize("name", list(TC.CASES))
def test_hip_through_case(hip, name):
    """the HIP gym, stepped tick by tick, through a case under (E), (R), (U) -- the same assertions the oracle meets in test_tower_model.py -- and bit-equal to
    the oracle: the rewards of every tick, every env's state at the end"""
    case = TC.CASES[name]
    judge, rewards, state = hip_run(name)
    c = judged(name, judge)
    if case.scripted:
        assert judge.fragile == 0 and judge.min_margin >= TC.MARGIN
    else:
        assert judge.fragile <= 0.02 * judge.interact_ticks
        assert c["picks"] >= 100 and c["placements"] >= 50 and c["picks_48"] >= 10 and c["placements_48"] >= 10 and c["placements_y3"] >= 5, c
    if name == "sweep":
        assert sorted(ev[3] for ev in judge.events if ev[1] == "pick") == list(range(80)) == sorted(ev[3] for ev in judge.events if ev[1] == "place")
    if name.startswith("tower"):
        assert [ev[4][1] for ev in judge.events if ev[0] == 0 and ev[1] == "place"] == list(range(1, TC.TOWER_TOP + 1)) + [2]
    if name == "end":
        assert judge.finished >= 1 and all(o[1] == o[2] for o in judge.objectives) and judge.objectives[0][1] == 3.0
    want_rewards, want_snaps = oracle_run(name)
    assert len(rewards) == len(want_rewards)
    for t, (r, w) in enumerate(zip(rewards, want_rewards)):
        assert r.tobytes() == w.tobytes(), f"rewards of tick {t}: {r} vs the oracle's {w}"
    for e in range(case.N):
        assert diff_snapshots(want_snaps[e], np.frombuffer(state[e], oracle_lib.SNAP)[0], case.A) == [], f"state of env {e}"


def test_order_with_the_sequential_redo(hip, monkeypatch):
    """case f once more with MV_DEBUG_FORCE_REDO: the shared-out controllers are thrown away and run in a row before interact -- same judgement, same bits"""
    monkeypatch.setenv("MV_DEBUG_FORCE_REDO", "1")
    case = TC.CASES["order"]
    g = case.make(MegaverseGym)
    judge, rewards = TC.run_judged(case, g)
    state = final_state(g, case.N)
    g.close()
    monkeypatch.delenv("MV_DEBUG_FORCE_REDO")
    judged("order, redo", judge)
    _, want_rewards, want_state = hip_run("order")
    assert all(r.tobytes() == w.tobytes() for r, w in zip(rewards, want_rewards)) and state == want_state


def replay_single(case, pipelining):
    """the case out of a device action ring, one step_n call per segment -> ([ticks] rewards, final state, (step launches, calls, ticks))"""
    import torch
    g = case.make(MegaverseGym)
    g.set_pipelining(pipelining)
    depth = 16
    ring = torch.full((depth, case.N * case.A), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g.set_output_ring(depth, 0, ring.data_ptr(), 0)
    rewards, t, launches, calls, keep = [], 0, 0, 0, []
    for cmds, actions in case.segments(g):
        TC.apply(g, cmds)
        dev = torch.as_tensor(np.ascontiguousarray(actions)).to("cuda:0")
        keep.append(dev)
        k = len(actions)
        g.set_action_ring(k, dev.data_ptr())
        before = g.debug_launch_counts()[0]
        g.step_n(k, "sequence", 0, 0)
        launches += g.debug_launch_counts()[0] - before
        calls += 1
        g.synchronize()
        host = ring.cpu().numpy()
        rewards += [host[(t + j) % depth].copy() for j in range(k)]
        t += k
    out = rewards, final_state(g, case.N), (launches, calls, t)
    g.close()
    return out


# (case, MV_STEP_PIPE or None, pipelining): the one-wave and the two-wave kernel for the one-agent cases, the agents kernel for the others
RING_REPLAYS = [(n, pipe, on) for n in REPLAY for pipe in (("0", "1") if TC.CASES[n].A == 1 else (None,)) for on in (True, False)]


@pytest.mark.parametrize("name,pipe,pipelining", RING_REPLAYS)
def test_replay_through_an_action_ring(hip, monkeypatch, name, pipe, pipelining):
    """cases a, d, f, g replayed in batched calls (8 ticks each; the tower in calls of 2): the rewards of every tick and the final state are those of the
    tick-by-tick run the model judged.  Every call is ONE step launch of all its ticks; which kernel: the module's table (MV_STEP_PIPE is read at every
    launch)"""
    monkeypatch.delenv("MV_STEP_PIPE", raising=False)
    if pipe is not None:
        monkeypatch.setenv("MV_STEP_PIPE", pipe)
    case = TC.CASES[name]
    _, want_rewards, want_state = hip_run(name)
    rewards, state, (launches, calls, ticks) = replay_single(case, pipelining)
    assert ticks == len(want_rewards) and launches == calls < ticks, (launches, calls, ticks)
    for t, (r, w) in enumerate(zip(rewards, want_rewards)):
        assert r.tobytes() == w.tobytes(), f"rewards of tick {t}: {r} vs {w}"
    assert state == want_state


def replay_in_group(name, batched):
    from megaverse_amd.multitask import MultiTaskGym
    case = TC.CASES[name]
    judge, want_rewards, want_state = hip_run(name, True)
    assert judge.failures == [], judge.failures[:10]
    N, A = case.N, case.A
    mt = MultiTaskGym(["TowerBuilding", "Empty"], TC.W, TC.H, 2 * N, A, 1, case.params)
    mt.set_pixel_mode("fast")   # (a group's one-launch calls need the fast pixels; the state does not depend on the pixel mode)
    mt.seed(case.seed)
    mt.reset()
    tower = mt.gyms[0]
    depth = 16
    _, ring_rewards, _ = mt.set_output_ring(depth)
    rewards, t, launches, calls = [], 0, 0, 0
    for cmds, actions in case.segments(tower):
        TC.apply(tower, cmds)
        k = len(actions)
        both = np.zeros((k, N, 2, A, 6), np.int32)   # global env i is local env i // 2 of member i % 2
        both[:, :, 0] = actions.reshape(k, N, A, 6)
        both = both.reshape(k, 2 * N * A, 6)
        before = tower.debug_launch_counts()[0]   # (a member reports the group's launches)
        if batched:
            mt.set_action_ring(both)
            mt.step_n(k, "sequence", 0, 0)
            mt.synchronize()
            host = ring_rewards[0].cpu().numpy()
            rewards += [host[(t + j) % depth].copy() for j in range(k)]
        else:
            for j in range(k):
                for i in np.argwhere(both[j].any(axis=1)).ravel():
                    mt.set_actions(int(i) // A, int(i) % A, both[j, i].tolist())
                mt.step()
                mt.synchronize()
                rewards.append(ring_rewards[0].cpu().numpy()[(t + j) % depth].copy())
                for i in np.argwhere(both[j].any(axis=1)).ravel():
                    mt.set_actions(int(i) // A, int(i) % A, [0] * 6)
        launches += tower.debug_launch_counts()[0] - before
        calls += 1
        t += k
    assert t == len(want_rewards)
    # one union step launch per call where the group can batch (one agent per env: step_union_ticks_kernel), else one per tick (step_union_kernel)
    assert launches == (calls if batched and A == 1 else t), (launches, calls, t)
    for j, (r, w) in enumerate(zip(rewards, want_rewards)):
        assert r.tobytes() == w.tobytes(), f"rewards of tick {j}: {r} vs {w}"
    assert final_state(tower, N) == want_state
    mt.close()


@pytest.mark.parametrize("name", REPLAY)
def test_replay_as_a_group_member(hip, name):
    """the same with the Tower gym as the first member of a MultiTaskGym beside an Empty gym, one call per segment -- against a judged tick-by-tick run of a
    gym of its own created the way the group creates its member.  One agent per env (sweep, tower_a1, stress_a1): one union launch of k ticks per call,
    step_union_ticks_kernel, asserted by the launch count; several agents (tower_a4, order, stress_a4): a group has no k-tick launch for them, the call is
    k launches of step_union_kernel"""
    replay_in_group(name, True)


@pytest.mark.parametrize("name", ["order", "tower_a1", "tower_a4"])
def test_replay_as_a_group_member_tick_by_tick(hip, name):
    """... and one union launch per tick (step_union_kernel, MultiTaskGym.step): the short cases"""
    replay_in_group(name, False)
