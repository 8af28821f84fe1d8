"""Football in the CPU oracle (oracle/mv_oracle.cpp), without a GPU.  Its episodes against the host generator (mv_gen_football.cpp) and the Python
restatement (football_model.generate) byte for byte, across auto-resets; its ball against football_model.step on every tick of rollouts that kick,
hit walls and capsules, get stopped by the ball and reset (all asserted, on the oracle's own records); properties of the controllers against the sphere
collider; and the scripted contact cases of football_cases.py, each with what it must have exercised.  The GPU tests (test_football_parity_gpu.py) then
hold the device to this oracle bit for bit, with the same rollouts and cases."""
import ctypes as C
import functools

import numpy as np
import pytest

import football_cases as FC
import football_model as M
import oracle_lib
from megaverse_amd import extension as ext
from megaverse_amd.rollout import action_masks

F32 = np.float32
ORANGE, WHITE = 0xFFB400, 0xFFFFFF
CAP_BOTTOM = FC.CAP_HH + FC.CAP_R
ROLLOUT_PARAMS = {"episodeLengthSec": 10.0}   # 150 ticks: two auto-resets per env inside the 400 ticks below
ROLLOUT_SEEDS = {1: 21, 2: 22, 3: 23, 4: 24, 8: 28}
ROLLOUT_TICKS = 400


def env_seeds(master, n):
    r = M.MT19937(master)
    return [M.rand_range(0, 1 << 30, r) for _ in range(n)]   # mvo_seed / mv_seed: megaverse.cpp:60-69


def host_generated(A, env_seed, n, base_len):
    lib = ext.load_library()
    buf = np.zeros(n * M.BLOB.itemsize, np.uint8)
    assert lib.mv_debug_generate_football(A, env_seed, n, base_len, buf.ctypes.data, buf.size) == n
    return buf.view(M.BLOB)


def yaw_basis(fr):
    """spawnAgents' rotation of frand() * pi * 2 as the yaw basis (m00, m02, m20, m22): btQuaternion(axis y, angle) -> btMatrix3x3, on the
    polynomial sincos both sides use (mvo_sincos)"""
    ang = F32(F32(F32(fr) * F32(3.14159274)) * F32(2))
    s, c = C.c_float(), C.c_float()
    oracle_lib.lib().mvo_sincos(C.c_float(float(F32(ang * F32(0.5)))), C.byref(s), C.byref(c))
    sh, ch = F32(s.value), F32(c.value)
    k = F32(F32(2.0) / F32(F32(sh * sh) + F32(ch * ch)))
    ys = F32(sh * k)
    cs, sn = F32(F32(1.0) - F32(sh * ys)), F32(ch * ys)
    return np.array([cs, sn, -sn, cs], np.float32)


def check_fresh(og, e, blob, A):
    """env e of the oracle right after a reset against one FootballBlob"""
    s, b = og.snapshot(e), og.football_state(e)
    assert b.tobytes() == M.reset_state().tobytes(), b
    assert int(s["scenario"]) == 9 and (int(s["L"]), int(s["H"]), int(s["W"])) == (int(blob["length"]), int(blob["height"]), int(blob["width"]))
    nb = int(blob["num_boxes"])
    assert nb == 5 and int(s["hex_num_boxes"]) == nb and int(s["hex_num_objs"]) == 1
    for k, (lo, hi) in enumerate(M.room_boxes(blob)):
        r = s["hex_boxes"][k]
        assert tuple(r["a"]) == lo and tuple(r["b"]) == hi and int(r["meta"]) == 1 << 4 and int(r["color"]) == WHITE, (k, r)
    ball = s["hex_objs"][0]
    assert tuple(ball["a"]) == (5.0, 5.0, 5.0) and tuple(ball["b"]) == (0.5, 0.5, 0.5) and int(ball["meta"]) == 2 and int(ball["color"]) == ORANGE
    assert float(s["episode_sec"]) == 0.0 and float(s["episode_len"]) == float(blob["episode_len"]) and float(s["bar_half_width"]) == float(F32(0.24))
    assert int(s["done"]) == 0 and int(s["num_frames"]) == 0
    for k in range(A):
        sp, a = blob["spawn"][k], s["agents"][k]
        assert np.array_equal(a["pos"], np.array([sp[0] + F32(0.5), sp[1] + F32(1.75), sp[2] + F32(0.5)], np.float32)), (k, a["pos"], sp)
        assert a["basis"].tobytes() == yaw_basis(blob["yaw_frand"][k]).tobytes(), (k, a["basis"])
        assert a["spawn"].tolist() == [int(v) for v in sp]
        assert not any(float(a[f]) for f in ("pitch", "vvel", "voffset", "step_offset", "last_reward", "total_reward")) and not a["hv"].any()


@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_episodes_match_the_generator_across_resets(A):
    N, length = 4, 0.2   # the episode clock reaches 0.2 on the third tick
    ticks = 3
    for master in (7, 42, 1001):
        og = oracle_lib.OracleGym("Football", 16, 16, N, A, 1, False, {"episodeLengthSec": length})
        og.seed(master); og.reset()
        blobs = []
        for e, es in enumerate(env_seeds(master, N)):
            host, model = host_generated(A, es, 3, length), M.episodes(A, es, 3, length)
            assert all(host[n].tobytes() == model[n].tobytes() for n in range(3))
            blobs.append(model)
        for episode in range(3):
            for e in range(N):
                check_fresh(og, e, blobs[e][episode], A)
            for t in range(ticks):
                og.step_norender()
                assert og.get_dones().tolist() == [int(t == ticks - 1)] * N, (episode, t)
                assert not og.get_last_rewards().any()
            assert all(og.true_objective(e, a) == 0.0 for e in range(N) for a in range(A))
        og.close()


def test_name_and_shaping():
    og = oracle_lib.OracleGym("football", 16, 16, 1, 2, 1, False, {})
    og.seed(1); og.reset()
    assert og.get_reward_shaping(0, 1) == {"teamSpirit": 0.0}
    assert float(og.snapshot(0)["episode_len"]) == 60.0
    og.close()


# ---- rollouts ---------------------------------------------------------------------------------------------------------------------------------

def boxes_of(snap):
    return [(tuple(F32(v) for v in r["a"]), tuple(F32(v) for v in r["b"])) for r in snap["hex_boxes"][: int(snap["hex_num_boxes"])]]


def caps(snap, A):
    return [tuple(F32(v) for v in snap["agents"][k]["pos"]) for k in range(A)]


@functools.lru_cache(maxsize=None)
def rollout(A):
    """N = 8 envs, even ones chase and kick, odd ones act at random: per tick and env (masks, snapshot before, snapshot after, ball before, ball
    after, done), and the events of the run"""
    N, seed = 8, ROLLOUT_SEEDS[A]
    og = oracle_lib.OracleGym("Football", 16, 16, N, A, 1, False, ROLLOUT_PARAMS)
    og.seed(seed); og.reset()
    snaps, balls = [og.snapshot(e) for e in range(N)], [og.football_state(e) for e in range(N)]
    events, ticks = FC.Events(), []
    for t in range(ROLLOUT_TICKS):
        masks = action_masks(FC.policy_actions("chaser", og, N, A, seed, t)).reshape(N, A)
        og.set_action_masks(masks)
        og.step_norender()
        dones = og.get_dones()
        assert not og.get_last_rewards().any()
        row = []
        for e in range(N):
            snap, ball = og.snapshot(e), og.football_state(e)
            events.tick(A, masks[e], snaps[e], snap, ball, bool(dones[e]))
            row.append((masks[e], snaps[e], snap, balls[e], ball, bool(dones[e])))
            snaps[e], balls[e] = snap, ball
        ticks.append(row)
    og.close()
    return ticks, events


@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_ball_is_the_stated_model_on_every_tick(A):
    """football_model.step, fed the oracle's previous ball and its capsules before and after the tick, gives the oracle's FootballState bit for
    bit -- kicks and contact bits included; after a reset the ball is the reset record"""
    ticks, events = rollout(A)
    for t, row in enumerate(ticks):
        for e, (masks, before, after, ball0, ball1, done) in enumerate(row):
            if done:
                assert ball1.tobytes() == M.reset_state().tobytes(), (t, e)
                continue
            want = M.step(ball0, boxes_of(before), caps(before, A), caps(after, A), [int(m) for m in masks])
            assert ball1.tobytes() == want.tobytes(), (t, e, ball1, want)
            drawn = after["hex_objs"][0]
            assert drawn["a"].tobytes() == ball1["pos"].tobytes() and tuple(drawn["b"]) == (1.0, 1.0, 1.0), (t, e)
    assert events.all_seen(), events
    assert events.resets == 8 * 2, events   # episodes end on tick 150 and 300


def contacts_of(p, boxes, others, ball):
    """the capsule with its centre at p against every collider, in float64: [(gap, upward part of the contact normal)] -- boxes grown by the
    capsule's half height, other capsules (summed half lengths and radii), the ball (its segment of half-length CAP_HH, summed radii)"""
    p = np.array(p, np.float64)
    out = []

    def add(v, r):
        d = float(np.linalg.norm(v))
        out.append((d - r, v[1] / d) if d > 0.0 else (-r, 0.0))

    for lo, hi in boxes:
        lo, hi = np.array(lo, np.float64) - [0, FC.CAP_HH, 0], np.array(hi, np.float64) + [0, FC.CAP_HH, 0]
        v = p - np.clip(p, lo, hi)
        if v.any():
            add(v, FC.CAP_R)
        else:   # the centre inside the grown box: out through the nearest face
            depth, up = min((p[0] - lo[0], 0.0), (hi[0] - p[0], 0.0), (p[1] - lo[1], -1.0), (hi[1] - p[1], 1.0), (p[2] - lo[2], 0.0), (hi[2] - p[2], 0.0))
            out.append((-depth - FC.CAP_R, up))
    for c, half, r in [(o, 2 * FC.CAP_HH, 2 * FC.CAP_R) for o in others] + [(ball, FC.CAP_HH, FC.SUM_R)]:
        c = np.array(c, np.float64)
        add(p - np.array([c[0], min(max(p[1], c[1] - half), c[1] + half), c[2]]), r)
    return out


@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_controllers_against_the_ball_keep_their_properties(A):
    """every tick of the rollouts, with each agent's capsule measured against every collider its controller has -- the ball at its NEW pose, the
    room's boxes, the other capsules (where each was before or after its own controller ran, whichever is nearer):
    (1) where no agent started the tick deeper than MAX_PEN_DEPTH in any of them, none ends it deeper in the ball than MAX_PEN_DEPTH + 0.045 (the
    walk-in test's margin).  (An agent that starts deep in a wall -- the ball pressed it there -- is pushed out of the wall into the ball.)
    (2) an agent on the ground stands on something: a collider within 0.1 (the sweep's 0.04 + the recovery's 0.041, test_oracle_properties.py's
    bound) whose contact normal points up at least as much as the slope limit, 0.7071, less rounding.  Not asked of an agent that was moving up
    this tick (it jumped, or its vertical velocity was positive): stepUp's ceiling branch zeroes the vertical velocity of an agent that bumps its
    head -- here on the ball -- and onGround() is true in mid-air for one tick, as in the reference's controller.
    (3) agents stay inside the room: always inside its outer box and above the floor slab's underside; and within the walls and on the floor to
    0.1 (the same bound) where the agent did not start the tick deeper than MAX_PEN_DEPTH in anything and overlaps neither the ball nor another
    capsule at its end: the ball and the capsules come before the boxes in the recovery's order (five pushes, first object first), so an agent
    between one of them and a wall is left in the wall until they have gone.  (Asked of an agent until its capsule's lowest point has been above the walls' tops in
    this episode: an agent spawns 0.9 above the floor with onGround() true and can jump there, which takes it onto and over a wall 3 high, as in
    the reference.)"""
    ticks, _ = rollout(A)
    checked = grounded = free = 0
    over = np.zeros((8, A), bool)
    for t, row in enumerate(ticks):
        for e, (masks, before, after, ball0, ball1, done) in enumerate(row):
            if done:
                over[e] = False
                continue
            c = ball1["pos"]
            boxes = boxes_of(after)
            others = [[s["agents"][j]["pos"] for s in (before, after) for j in range(A) if j != i] for i in range(A)]
            start = [contacts_of(before["agents"][i]["pos"], boxes, others[i], c) for i in range(A)]
            end = [contacts_of(after["agents"][i]["pos"], boxes, others[i], c) for i in range(A)]
            start_ok = [min(g for g, _ in start[i]) >= -FC.MAX_PEN_DEPTH for i in range(A)]
            if all(start_ok):
                checked += 1
                assert min(end[i][-1][0] for i in range(A)) >= -(FC.MAX_PEN_DEPTH + 0.045), (t, e, [x[-1] for x in start], [x[-1] for x in end])
            L, W = int(after["L"]), int(after["W"])
            for i in range(A):
                a = after["agents"][i]
                x, y, z = (float(v) for v in a["pos"])
                over[e, i] |= y - CAP_BOTTOM >= int(after["H"]) - 0.1
                if not over[e, i]:
                    assert 0.0 <= x <= L and 0.0 <= z <= W and y - CAP_BOTTOM >= 0.0, (t, e, i, x, y, z)
                    if start_ok[i] and min(g for g, _ in end[i][len(boxes):]) >= 0.0:
                        free += 1
                        assert 1.0 + 0.33 - 0.1 <= x <= L - 1 - 0.33 + 0.1 and 1.0 + 0.33 - 0.1 <= z <= W - 1 - 0.33 + 0.1, (t, e, i, x, z)
                        assert y - CAP_BOTTOM >= 1.0 - 0.1, (t, e, i, y)
                moving_up = bool(int(masks[i]) & (1 << 7)) or float(before["agents"][i]["vvel"]) > 0.0
                if abs(float(a["vvel"])) < 1.2e-7 and abs(float(a["voffset"])) < 1.2e-7 and not moving_up:   # onGround()
                    grounded += 1
                    assert any(g <= 0.1 and up >= 0.70 for g, up in end[i]), (t, e, i, a["pos"], c)
    assert checked > ROLLOUT_TICKS * 8 // 2 and min(grounded, free) > ROLLOUT_TICKS * 8 * A // 2, (checked, grounded, free)


# ---- the scripted contact cases on the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("A", [1, 2])
def test_scripted_contact_cases_exercise_what_they_name(A):
    cases = [c for c in FC.scripted_cases() if len(c.agents) == A]
    og = oracle_lib.OracleGym("Football", 16, 16, len(cases), A, 1, False, {})
    og.seed(5); og.reset()
    for c, trace in zip(cases, FC.run_on_oracle(og, cases, 45)):
        try:
            c.expect(trace)
        except AssertionError as ex:
            raise AssertionError(f"case {c.name}: {ex}") from ex
    og.close()
