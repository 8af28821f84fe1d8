"""BoxAGone in the CPU oracle (oracle/mv_oracle.cpp, restated from scenario_box_a_gone.{hpp,cpp}): its episodes against the host generator
(mv_gen_boxagone.cpp through mv_debug_generate_episode, no GPU), its scenario logic against the Python restatement (boxagone_model.step)
replayed on the oracle's own post-physics agents, and properties of its rollouts (support under every agent on the ground, the room's walls)."""
import numpy as np
import pytest

import boxagone_model as M
import oracle_lib
from megaverse_amd import extension as ext
from megaverse_amd.rollout import action_masks, sample_actions

F32 = np.float32
CAP_HH, CAP_R = F32(F32(1.05) * F32(0.5)), F32(0.33)


def env_seeds(master, n):
    r = M.MT19937(master)
    return [M.rand_range(0, 1 << 30, r) for _ in range(n)]


def generated(agents, env_seed, n, base_len):
    lib = ext.load_library()
    buf = np.zeros(M.BLOB.itemsize, np.uint8)
    assert lib.mv_debug_generate_episode(b"BoxAGone", agents, env_seed, n, base_len, buf.ctypes.data, buf.size) == buf.size
    return buf.view(M.BLOB)[0]


def yaw_basis(frand):
    """spawn_agents' yaw basis for randomRotation = frand * pi * 2 (Bullet's quaternion -> matrix for the Y axis, mv_sincos of the half angle)"""
    L = oracle_lib.lib()
    import ctypes as C
    angle = F32(F32(F32(frand) * F32(3.14159274)) * F32(2))
    sh, ch = C.c_float(), C.c_float()
    L.mvo_sincos(F32(angle * F32(0.5)), C.byref(sh), C.byref(ch))
    qy, w = F32(sh.value), F32(ch.value)
    s = F32(F32(2.0) / F32(F32(qy * qy) + F32(w * w)))
    ys = F32(qy * s)
    c, sn = F32(F32(1.0) - F32(qy * ys)), F32(w * ys)
    return np.array([c, sn, -sn, c], F32)


def check_episode(snap, st, blob, A):
    np_ = int(blob["num_platforms"])
    assert int(st["num_platforms"]) == np_ == int(snap["num_platforms"]) and int(st["num_levels"]) == int(blob["num_levels"])
    assert st["level_y"].tolist() == blob["level_y"].tolist()
    plat = st["plat"][:np_]
    want = blob["platforms"][:np_]
    assert np.array_equal(plat["x"], want["x"]) and np.array_equal(plat["y"], want["y"]) and np.array_equal(plat["z"], want["z"])
    assert np.array_equal(plat["state"], want["state"])           # level, every platform on its cell
    assert not st["plat"][np_:].view(np.uint32).any() and not st["ticks"].any() and int(st["takes"]) == 0
    assert int(snap["hex_num_boxes"]) == 5 + np_ + 3 * A and int(snap["hex_num_objs"]) == 0 and int(snap["scenario"]) == 8
    assert (snap["hex_boxes"]["meta"][: int(snap["hex_num_boxes"])] == 1 << 4).all()
    for i in range(A):
        ag = snap["agents"][i]
        sp = blob["spawn"][i]
        assert ag["spawn"].tolist() == [int(np.floor(v)) for v in sp]
        assert ag["pos"].tobytes() == np.array([sp[0] + F32(0.5), sp[1] + F32(1.75), sp[2] + F32(0.5)], F32).tobytes()
        assert ag["basis"].tobytes() == yaw_basis(blob["yaw_frand"][i]).tobytes(), i
    assert float(snap["episode_len"]) == float(blob["episode_len"])


@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_episodes_equal_host_generator(A):
    """first and later episodes of every env: platforms, levels, spawns and yaw draws are the host generator's (episodes end after one tick)"""
    N, length = 3, 0.05
    for master in (7 + A, 1000 + A):
        g = oracle_lib.OracleGym("BoxAGone", 16, 16, N, A, 1, False, {"episodeLengthSec": length})
        g.seed(master); g.reset()
        seeds = env_seeds(master, N)
        for n in range(1, 5):
            for e in range(N):
                check_episode(g.snapshot(e), g.boxagone_state(e), generated(A, seeds[e], n, length), A)
            g.step_norender()
            assert g.get_dones().all()
        g.close()


def test_defaults_and_shaping_keys():
    g = oracle_lib.OracleGym("BoxAGone", 16, 16, 1, 2, 1, False, {})
    g.seed(1); g.reset()
    assert g.get_reward_shaping(0, 1) == {"teamSpirit": 0.0, "boxagoneTouchedFloor": pytest.approx(-0.1), "boxagonePerStepReward": pytest.approx(0.01)}
    s = g.snapshot(0)
    assert float(s["episode_len"]) == 300.0 and (int(s["L"]), int(s["H"]), int(s["W"])) == (24, 8, 24)
    for _ in range(12):   # look up for longer than the limit allows: the pitch stops at 0.75 (scenario_box_a_gone.hpp:78)
        g.set_action_mask(0, 0, 1 << 10)
        g.step_norender()
    assert g.snapshot(0)["agents"][0]["pitch"] == F32(0.75)
    g.close()


def floor_agents(agents):
    """the agents of an episode's last tick: every one is on the floor (once there, nothing reaches a platform level again), at rest"""
    a = agents.copy()
    for i in range(len(a)):
        a[i]["pos"][1] = F32(2.9)
        a[i]["vvel"] = F32(0.0); a[i]["voffset"] = F32(0.0)
    return a


def policy(kind, seed, step, n):
    if kind == "random":
        return action_masks(sample_actions(seed, step, n))
    if kind == "forward":
        return action_masks(M.forward_actions(seed, step, n))
    return np.zeros(n, np.int32)


def under_ceiling(agent, boxes, others, reach):
    """was the capsule's upper hemisphere, on its way up by at most `reach`, stopped by the underside of a box or another capsule?  (stepUp
    hitting a ceiling zeroes the vertical velocity and offset, kinematic_character_controller.cpp: the agent counts as on the ground then)"""
    c = agent["pos"].astype(np.float64) + np.array([0.0, float(CAP_HH), 0.0])
    for b in boxes:
        lo, hi = b["a"].astype(np.float64), b["b"].astype(np.float64)
        d = np.linalg.norm(np.maximum(np.maximum(lo - c, 0.0), c - hi))
        if d <= float(CAP_R) + reach and c[1] <= lo[1] + 0.06:
            return True
    for o in others:
        q = o["pos"].astype(np.float64)
        d = np.linalg.norm(c - np.array([q[0], min(max(c[1], q[1] - float(CAP_HH)), q[1] + float(CAP_HH)), q[2]]))
        if d <= 2 * float(CAP_R) + reach and c[1] <= q[1]:
            return True
    return False


def supported(agent, boxes, others):
    """is there a platform, temporary platform, floor or another agent's capsule right under this agent's capsule?  Its lower hemisphere
    (centre pos - CAP_HH) touches it -- within the controller's penetration / step slack -- from above"""
    c = agent["pos"].astype(np.float64) - np.array([0.0, float(CAP_HH), 0.0])
    r, slack = float(CAP_R), 0.06
    for b in boxes:
        lo, hi = b["a"].astype(np.float64), b["b"].astype(np.float64)
        d = np.linalg.norm(np.maximum(np.maximum(lo - c, 0.0), c - hi))
        if d <= r + slack and c[1] >= hi[1] - slack:
            return True
    for o in others:   # the other capsule's segment
        q = o["pos"].astype(np.float64)
        top = q[1] + float(CAP_HH)
        d = np.linalg.norm(c - np.array([q[0], min(max(c[1], q[1] - float(CAP_HH)), top), q[2]]))
        if d <= 2 * r + slack and c[1] >= q[1]:
            return True
    return False


@pytest.mark.parametrize("A,kind,seed", [(1, "forward", 3), (1, "random", 4), (2, "forward", 5), (2, "random", 6), (4, "forward", 7),
                                         (4, "random", 8), (2, "idle", 9)])
def test_logic_matches_model_on_oracle_rollouts(A, kind, seed):
    """boxagone_model.step replayed on the oracle's post-physics agents: rewards, the BoxAGoneState record, episode_sec and dones bit for
    bit, the true objective on the ending tick; and on every tick every agent on the ground stands on something, inside the room"""
    N, T = 4, 300
    g = oracle_lib.OracleGym("BoxAGone", 16, 16, N, A, 2, False, {})
    g.seed(seed); g.reset()
    snaps = [g.snapshot(e) for e in range(N)]
    sts = [g.boxagone_state(e) for e in range(N)]
    wraps = finished = resets = grown = expired = 0
    for t in range(T):
        g.set_action_masks(policy(kind, seed, t, N * A))
        g.step_norender()
        rewards = g.get_last_rewards().reshape(N, A)
        dones = g.get_dones()
        for e in range(N):
            prev, st0 = snaps[e], sts[e]
            shaping = prev["agents"]["shaping"][:A]
            snap, st = g.snapshot(e), g.boxagone_state(e)
            agents = floor_agents(prev["agents"][:A]) if dones[e] else snap["agents"][:A]
            want, r, touching, sec, done = M.step(st0, agents, shaping, F32(prev["episode_sec"]), F32(prev["episode_len"]), A)
            assert done == bool(dones[e]), (t, e)
            if dones[e]:   # (the rewards are read after the auto-reset zero-filled them: megaverse.cpp:128-137)
                assert not rewards[e].any() and (r == F32(-0.1)).all(), (t, e, rewards[e], r)
                resets += 1
                obj = np.array([g.true_objective(e, a) for a in range(A)], F32)
                assert obj.tobytes() == M.true_objective(want, A, F32(300.0)).tobytes(), (t, e, obj)
                assert int(snap["num_frames"]) == 0 and int(st["takes"]) == 0
            else:
                assert rewards[e].tobytes() == r.tobytes(), (t, e, rewards[e], r)
                assert st.tobytes() == want.tobytes(), (t, e, [n for n in M.STATE.names if st[n].tobytes() != want[n].tobytes()])
                assert F32(snap["episode_sec"]) == sec, (t, e)
                finished += int(want["finished"]) and not int(st0["finished"])
                wraps += int(st["takes"]) > 3 * A and int(st0["takes"]) == 3 * A
                grown += int(((st["ticks"] > 0) & (st["ticks"] <= 5)).sum())
                expired += int(((st0["ticks"] == 1)).sum())
                boxes = prev["hex_boxes"][: int(prev["hex_num_boxes"])]   # what the tick's physics saw
                for i in range(A):
                    ag = snap["agents"][i]
                    x, y, z = (float(v) for v in ag["pos"])
                    inner = (2.0 + 0.33 / 2, 46.0 - 0.33 / 2)   # the walls' inner faces (agents in a crowd may press each other in a bit)
                    assert inner[0] < x < inner[1] and inner[0] < z < inner[1] and y > 2.0, (t, e, i, ag["pos"])
                    if M.on_ground(ag):   # the others as agent i's controller saw them: the ones before it have moved already
                        others = [snap["agents"][j] for j in range(i)] + [prev["agents"][j] for j in range(i + 1, A)]
                        reach = max(float(prev["agents"][i]["vvel"]), 0.0) * float(M.DT) + 0.06
                        assert supported(ag, boxes, others) or under_ceiling(ag, boxes, others, reach), (t, e, i, ag["pos"])
            snaps[e], sts[e] = snap, st
    if kind != "idle":
        assert wraps > 0 and grown > 0 and expired > 0, (wraps, grown, expired)
        assert finished > 0 and resets > 0, (finished, resets)
    g.close()
