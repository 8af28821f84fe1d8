"""What tests/test_rearrange_model_gpu.py and tests/test_sokoban_model_gpu.py share: the HIP gym through a case of tests/rearrange_cases.py or
tests/sokoban_cases.py under its model (tests/rule_judge.py), the CPU oracle through the same case, and the two replays -- out of a device action ring,
one batched call per segment, and as the first member of a MultiTaskGym beside an Empty gym.  TEST INFRASTRUCTURE ONLY (the counterpart of what
tests/test_tower_model_gpu.py holds for TowerBuilding)."""
import numpy as np

import oracle_lib
import rule_judge
import tower_cases as TC
from hip_util import diff_snapshots
from megaverse_amd.extension import MegaverseGym

GROUP = dict(env_offset=0, env_stride=2)   # how a MultiTaskGym of two scenarios creates its first member
DEPTH = 16


def final_state(g, N):
    return [g.debug_snapshot_bytes(e).tobytes() for e in range(N)]


def hip_run(case, model, group=False, **state_kw):
    """the HIP gym through a case tick by tick under the model -> (judge, [ticks] rewards, [ticks] dones, [ticks] objectives, the final snapshots' bytes)"""
    g = case.make(MegaverseGym, **(dict(GROUP, total_envs=2 * case.N) if group else {}))
    judge, rewards, dones, objectives = rule_judge.run_judged(case, g, model, min_margin=TC.MARGIN if case.scripted else None, **state_kw)
    out = judge, rewards, dones, objectives, final_state(g, case.N)
    g.close()
    return out


def oracle_run(case):
    g = case.make(oracle_lib.OracleGym)
    rewards, dones, objectives = [], [], []
    for what, _ in TC.play(case, g):
        if what == "tick":
            rewards.append(g.get_last_rewards().copy())
            dones.append(g.get_dones().astype(bool))
            objectives.append({int(e): g.true_objective(int(e), 0) for e in np.nonzero(dones[-1])[0]})
    snaps = [g.snapshot(e).copy() for e in range(case.N)]
    g.close()
    return rewards, dones, objectives, snaps


def assert_equal_to_oracle(case, hip, oracle):
    """bit-equal: the rewards and dones of every tick, the true objective of every finished episode, every env's state at the end"""
    _, rewards, dones, objectives, state = hip
    want_rewards, want_dones, want_objectives, want_snaps = oracle
    assert len(rewards) == len(want_rewards)
    for t in range(len(rewards)):
        assert rewards[t].tobytes() == np.asarray(want_rewards[t], np.float32).tobytes(), f"rewards of tick {t}: {rewards[t]} vs the oracle's {want_rewards[t]}"
        assert dones[t].tolist() == want_dones[t].tolist(), f"dones of tick {t}"
        assert objectives[t] == want_objectives[t], f"true objectives of tick {t}: {objectives[t]} vs the oracle's {want_objectives[t]}"
    for e in range(case.N):
        assert diff_snapshots(want_snaps[e], np.frombuffer(state[e], oracle_lib.SNAP)[0], case.A) == [], f"state of env {e}"


def replay_single(case, pipelining):
    """the case out of a device action ring, one step_n call per segment -> ([ticks] rewards, [ticks] dones, (the last call's ticks, {env: true objective}
    of the envs that finished during it, read behind it), final state, (step launches, the launches the call plan states, calls, ticks))"""
    import torch
    g = case.make(MegaverseGym)
    g.set_pipelining(pipelining)
    ring = torch.full((DEPTH, case.N * case.A), -7.0, dtype=torch.float32, device="cuda:0")
    ring_dones = torch.full((DEPTH, case.N), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.set_output_ring(DEPTH, 0, ring.data_ptr(), ring_dones.data_ptr())
    rewards, dones, t, launches, calls, keep = [], [], 0, 0, 0, []
    expected = 0
    for cmds, actions in case.segments(g):
        TC.apply(g, cmds)
        dev = torch.as_tensor(np.ascontiguousarray(actions)).to("cuda:0")
        keep.append(dev)
        k = len(actions)
        assert k <= DEPTH
        g.set_action_ring(k, dev.data_ptr())
        before = g.debug_launch_counts()[0]
        g.step_n(k, "sequence", 0, 0)
        launches += g.debug_launch_counts()[0] - before
        calls += 1
        expected += 1 if case.A == 1 else k   # (mv_api_step.hip: one step launch for a call's k ticks with one agent per env; with several, TowerBuilding only)
        g.synchronize()
        host, host_dones = ring.cpu().numpy(), ring_dones.cpu().numpy()
        rewards += [host[(t + j) % DEPTH].copy() for j in range(k)]
        dones += [host_dones[(t + j) % DEPTH].astype(bool) for j in range(k)]
        t += k
    finished = np.nonzero(np.stack(dones[-k:]).any(axis=0))[0]
    objectives = {int(e): g.true_objective(int(e), 0) for e in finished}
    out = rewards, dones, (k, objectives), final_state(g, case.N), (launches, expected, calls, t)
    g.close()
    return out


def assert_replay_equals(case, hip, replay):
    """a replay's rewards and dones of every tick and its final state are those of the tick-by-tick run the model judged, and so are the true objectives
    of the envs that finished during its last call (the setter-free tail of a `solve` case -- the solving tick through the tick that ends the episode and
    swaps the next one in -- is ONE batched call).  With one agent per env every call is ONE step launch of all its ticks; with several it is one per tick."""
    _, want_rewards, want_dones, want_objectives, want_state = hip
    rewards, dones, (k, objectives), state, (launches, expected, calls, ticks) = replay
    assert ticks == len(want_rewards) and launches == expected and calls <= ticks, (launches, expected, calls, ticks)
    for t in range(ticks):
        assert rewards[t].tobytes() == want_rewards[t].tobytes(), f"rewards of tick {t}: {rewards[t]} vs {want_rewards[t]}"
        assert dones[t].tolist() == want_dones[t].tolist(), f"dones of tick {t}"
    want = {}
    for o in want_objectives[ticks - k:]:
        want.update(o)
    assert objectives == want, (objectives, want)
    assert state == want_state


def replay_in_group(case, hip_group, batched=True):
    """the case with its gym as the first member of a MultiTaskGym beside an Empty gym, one call per segment (batched) or one per tick -- against a judged
    tick-by-tick run of a gym of its own created the way the group creates its member.  One agent per env: one union launch of k ticks per call
    (step_union_ticks_kernel); several agents: a group has no k-tick launch for them, the call is k launches of step_union_kernel"""
    from megaverse_amd.multitask import MultiTaskGym
    judge, want_rewards, want_dones, _, want_state = hip_group
    assert judge.failures == [], judge.failures[:10]
    N, A = case.N, case.A
    mt = MultiTaskGym([case.scenario, "Empty"], TC.W, TC.H, 2 * N, A, 1, case.params)
    mt.set_pixel_mode("fast")   # (a group's one-launch calls need the fast pixels; the state does not depend on the pixel mode)
    mt.seed(case.seed)
    mt.reset()
    member = mt.gyms[0]
    _, ring_rewards, ring_dones = mt.set_output_ring(DEPTH)
    rewards, dones, t, launches, expected = [], [], 0, 0, 0
    for cmds, actions in case.segments(member):
        TC.apply(member, cmds)
        k = len(actions)
        both = np.zeros((k, N, 2, A, 6), np.int32)   # global env i is local env i // 2 of member i % 2
        both[:, :, 0] = actions.reshape(k, N, A, 6)
        both = both.reshape(k, 2 * N * A, 6)
        before = member.debug_launch_counts()[0]   # (a member reports the group's launches)
        if batched:
            mt.set_action_ring(both)
            mt.step_n(k, "sequence", 0, 0)
            mt.synchronize()
            host, host_dones = ring_rewards[0].cpu().numpy(), ring_dones[0].cpu().numpy()
            rewards += [host[(t + j) % DEPTH].copy() for j in range(k)]
            dones += [host_dones[(t + j) % DEPTH].astype(bool) for j in range(k)]
        else:
            for j in range(k):
                for i in np.argwhere(both[j].any(axis=1)).ravel():
                    mt.set_actions(int(i) // A, int(i) % A, both[j, i].tolist())
                mt.step()
                mt.synchronize()
                rewards.append(ring_rewards[0].cpu().numpy()[(t + j) % DEPTH].copy())
                dones.append(ring_dones[0].cpu().numpy()[(t + j) % DEPTH].astype(bool))
                for i in np.argwhere(both[j].any(axis=1)).ravel():
                    mt.set_actions(int(i) // A, int(i) % A, [0] * 6)
        launches += member.debug_launch_counts()[0] - before
        expected += 1 if batched and A == 1 else k
        t += k
    assert t == len(want_rewards)
    assert launches == expected, (launches, expected, t)
    for j, (r, w) in enumerate(zip(rewards, want_rewards)):
        assert r.tobytes() == w.tobytes(), f"rewards of tick {j}: {r} vs {w}"
        assert dones[j].tolist() == want_dones[j].tolist(), f"dones of tick {j}"
    assert final_state(member, N) == want_state
    mt.close()
