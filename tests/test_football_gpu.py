"""Football on the GPU (mv_tick_football.h, mv_step_football.hip): the reset against the host generator's episodes, the ball replayed in Python
(football_model.step) from the device's own records, tick after tick and bit for bit, known answers of the ball model and of the kicks, the
ball's pixels, the launch shapes against each other, and the Python surface."""
import numpy as np
import pytest

import football_model as M
from hip_util import hip_snapshot
from megaverse_amd.extension import MegaverseGym

pytestmark = pytest.mark.gpu

F32 = np.float32
ORANGE = 0xFFB400


def make(N, A, seed=42, params=None, w=64, h=64):
    g = MegaverseGym("Football", w, h, N, A, 1, False, params or {})
    g.seed(seed)
    g.reset()
    return g


def env_streams(master, N):
    r = M.MT19937(master)
    return [M.MT19937(M.rand_range(0, 1 << 30, r)) for _ in range(N)]


def state(g, e):
    d = g.debug_football_state(e)
    s = np.zeros((), M.STATE)
    for k in ("pos", "radius", "vel", "kicks", "ang", "contacts", "force"):
        s[k] = d[k]
    return s


def same(a, b):
    return a.tobytes() == b.tobytes()


def caps(snap, A):
    return [tuple(F32(v) for v in snap["agents"][k]["pos"]) for k in range(A)]


def check_fresh(st, snap, blob, A):
    assert same(st, M.reset_state())
    assert snap["L"] == blob["length"] and snap["H"] == blob["height"] and snap["W"] == blob["width"]
    nb = int(blob["num_boxes"])
    assert snap["hex_num_boxes"] == nb and snap["hex_num_objs"] == 1 and snap["episode_sec"] == 0.0
    for k, (lo, hi) in enumerate(M.room_boxes(blob)):
        assert tuple(snap["hex_boxes"][k]["a"]) == lo and tuple(snap["hex_boxes"][k]["b"]) == hi and snap["hex_boxes"][k]["color"] == 0xFFFFFF
    ball = snap["hex_objs"][0]
    assert tuple(ball["a"]) == (5.0, 5.0, 5.0) and tuple(ball["b"]) == (0.5, 0.5, 0.5) and ball["color"] == ORANGE
    for k in range(A):
        s = blob["spawn"][k]
        assert np.array_equal(snap["agents"][k]["pos"], np.array([s[0] + F32(0.5), s[1] + F32(1.75), s[2] + F32(0.5)], np.float32))
        c, sn = (float(v) for v in snap["agents"][k]["basis"][:2])
        ang = float(blob["yaw_frand"][k]) * np.pi * 2
        assert abs(c - np.cos(ang)) < 1e-5 and abs(sn - np.sin(ang)) < 1e-5, (k, c, sn, ang)


@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_reset_matches_generator(A):
    N = 16
    g = make(N, A, seed=7)
    streams = env_streams(7, N)
    for e in range(N):
        check_fresh(state(g, e), hip_snapshot(g, e), M.generate(streams[e], A, 60.0), A)
    g.close()


def chaser(snap, ball, A):
    """turn towards the ball, walk, kick: multi-discrete actions of one env's agents"""
    acts = np.zeros((A, 6), np.int32)
    for k in range(A):
        p, b = snap["agents"][k]["pos"], snap["agents"][k]["basis"]
        d = np.array([ball[0] - p[0], ball[2] - p[2]], np.float64)
        left = np.array([-b[0], b[1]], np.float64)
        side = float(d @ left) / (np.linalg.norm(d) + 1e-9)
        acts[k, 1] = 1
        acts[k, 2] = 1 if side > 0.15 else 2 if side < -0.15 else 0
        acts[k, 4] = 1
    return acts


def mask_of(a):
    m, idx = 0, 0
    for i, s in enumerate([3, 3, 3, 2, 2, 3]):
        if a[i] > 0:
            m |= 1 << (idx + int(a[i]))
        idx += s - 1
    return m


def inside(st, blob, margin):
    """the centre in the room's interior shrunk by the radius, less the margin"""
    x, y, z = (float(v) for v in st["pos"])
    L, W = int(blob["length"]), int(blob["width"])
    return 2.0 - margin <= x <= L - 2.0 + margin and 2.0 - margin <= z <= W - 2.0 + margin and y >= 2.0 - margin


def margin(prev):
    """a contact is found at the start pose only: in its last tick before one a ball can travel its integrated velocity times dt into a wall or
    the floor (a chaser kicking on consecutive ticks adds 70 N each: 10 units / s and more)"""
    v = float(np.linalg.norm(prev["vel"])) + float(M.DT) * (float(np.linalg.norm(prev["force"])) + 10.0)
    return 0.05 + float(M.DT) * v


def ticks_to(length):
    """the tick on which the float32 episode clock reaches `length` (60 s: tick 901)"""
    sec, n = F32(0), 0
    while sec < F32(length):
        sec, n = F32(sec + M.DT), n + 1
    return n


@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_ball_replay(A):
    """N = 64 envs, 1000 ticks (an auto-reset at 900): even envs chase the ball, odd ones act at random.  Every tick the model, fed the device's
    previous ball and the agents' capsules before and after the tick, must give the device's ball bit for bit."""
    N, T = 64, 1000   # (episodes end on tick 901)
    g = make(N, A, seed=11)
    streams = env_streams(11, N)
    blobs = [M.generate(streams[e], A, 60.0) for e in range(N)]
    rng = np.random.default_rng(3)
    sts = [state(g, e) for e in range(N)]
    snaps = [hip_snapshot(g, e) for e in range(N)]
    kicked, walls, capsules, resets = set(), set(), set(), 0
    over = [False] * N   # (a ball kicked on several ticks in a row can fly over a low wall -- 3..6 high -- and leave the room, as in the reference)
    for t in range(T):
        acts = np.zeros((N, A, 6), np.int32)
        for e in range(N):
            if e % 2 == 0:
                acts[e] = chaser(snaps[e], sts[e]["pos"], A)
            else:
                acts[e] = np.stack([rng.integers(0, s, A) for s in [3, 3, 3, 2, 2, 3]], 1)
        g.set_actions_batched(acts.reshape(N * A, 6))
        g.step()
        dones = g.get_dones()
        rewards = g.get_rewards_array()
        assert not rewards.any()
        for e in range(N):
            snap, st = hip_snapshot(g, e), state(g, e)
            if dones[e]:
                assert t == ticks_to(60.0) - 1, (e, t)
                resets += 1
                assert all(g.true_objective(e, i) == 0.0 for i in range(A))
                blobs[e] = M.generate(streams[e], A, 60.0)
                check_fresh(st, snap, blobs[e], A)
                over[e] = False
            else:
                want = M.step(sts[e], M.room_boxes(blobs[e]), caps(snaps[e], A), caps(snap, A), [mask_of(a) for a in acts[e]])
                assert same(st, want), (e, t, st, want)
                # (several agents kicking on one tick add their forces -- up to 8 x 70 -- and a ball that fast can tunnel: the bound is one or two agents')
                over[e] |= float(st["pos"][1]) >= float(blobs[e]["height"])
                assert A > 2 or over[e] or inside(st, blobs[e], margin(sts[e])), (e, t, st)
                if st["kicks"]:
                    kicked.add(e)
                if st["contacts"] & (0xF << 9):   # boxes 1..4: the walls
                    walls.add(e)
                if st["contacts"] & 0xFF:
                    capsules.add(e)
            sts[e], snaps[e] = st, snap
    assert resets == N
    chasers = N // 2
    assert len([e for e in kicked if e % 2 == 0]) >= chasers * 3 // 4, sorted(kicked)
    assert len(walls) >= N // 8, sorted(walls)
    assert len(capsules) >= N // 8, sorted(capsules)
    g.close()


# ---- known answers -------------------------------------------------------------------------------------------------------------------------

def rest_y():
    from canonical_frames import REST_Y
    return REST_Y


def park_agents(g, e, A, x=100.0):
    """agents far outside the room (they fall forever, nowhere near the ball)"""
    for k in range(A):
        g.debug_set_agent_pos(e, k, x + 3 * k, 50.0, x)


def test_ball_settles_on_the_floor():
    N = 8
    g = make(N, 1, seed=3)
    for e in range(N):
        park_agents(g, e, 1)
        g.debug_set_football_state(e, (5.0 + 0.5 * e, 3.5, 6.0), vel=(0.0, -3.0, 0.0))
    g.set_actions_batched(np.zeros((N, 6), np.int32))
    for _ in range(30):
        g.step()
    for e in range(N):
        st = state(g, e)
        assert abs(float(st["pos"][1]) - 2.0) <= 0.04 and float(np.linalg.norm(st["vel"])) < 1e-3, (e, st)
    g.close()


def kick_setup(dx):
    """a ball resting at (8, 2, 8), one agent on the floor at horizontal distance dx along -x of it, Interact"""
    g = make(4, 1, seed=5)
    for e in range(4):
        g.debug_set_football_state(e, (8.0, 2.0, 8.0))
        g.debug_set_agent_pos(e, 0, 8.0 - dx, rest_y(), 8.0)
        g.debug_set_agent_velocity(e, 0, 0.0, 0.0, 0.0)
    acts = np.zeros((4, 6), np.int32)
    acts[:, 4] = 1
    g.set_actions_batched(acts)
    g.step()
    return g


def test_kick_in_range_and_out_of_range():
    g = kick_setup(1.5)
    st = state(g, 0)
    assert st["kicks"] == 1 and st["force"][1] == F32(35.0) and st["force"][0] > 60.0
    snap = hip_snapshot(g, 0)
    v0 = st["vel"].copy()
    g.set_actions_batched(np.zeros((4, 6), np.int32))
    g.step()
    st1, snap1 = state(g, 0), hip_snapshot(g, 0)
    boxes = [(tuple(F32(v) for v in r["a"]), tuple(F32(v) for v in r["b"])) for r in snap["hex_boxes"][: int(snap["hex_num_boxes"])]]
    assert same(st1, M.step(st, boxes, caps(snap, 1), caps(snap1, 1), [0]))
    assert float(st1["vel"][0] - v0[0]) > 3.0 and float(st1["vel"][1]) > 0.0   # the force, 70 x n dt, on top of the floor's response
    g.close()
    g = kick_setup(1.85)
    assert state(g, 0)["kicks"] == 0 and not state(g, 0)["force"].any()
    g.close()


def test_two_kicks_add():
    g = make(4, 2, seed=5)
    ry = rest_y()
    g.debug_set_football_state(0, (8.0, 2.0, 8.0))
    g.debug_set_agent_pos(0, 0, 6.6, ry, 8.0)   # -x side
    g.debug_set_agent_pos(0, 1, 8.0, ry, 6.6)   # -z side
    acts = np.zeros((8, 6), np.int32)
    acts[0:2, 4] = 1
    g.set_actions_batched(acts)
    g.step()
    snap, st = hip_snapshot(g, 0), state(g, 0)
    assert st["kicks"] == 2
    one = [M.kicks(_zero_force(st), [c], [M.ACT_INTERACT])["force"] for c in caps(snap, 2)]
    assert st["force"][1] == F32(70.0) and np.allclose(st["force"], one[0] + one[1], atol=1e-5)
    g.close()


def _zero_force(st):
    s = st.copy()
    s["force"] = 0.0
    return s


def test_agent_walks_into_a_resting_ball_and_stops():
    N = 4
    g = make(N, 1, seed=9)
    ry = rest_y()
    c, sn = float(F32(np.cos(np.pi / 2))), float(F32(np.sin(np.pi / 2)))
    for e in range(N):
        g.debug_set_football_state(e, (6.0, 2.0, 6.0))
        g.debug_set_agent_pos(e, 0, 10.0, ry, 6.0)   # looking along -x at the ball
        g.debug_set_agent_yaw(e, 0, c, sn)
        g.debug_set_agent_velocity(e, 0, 0.0, 0.0, 0.0)
    fwd = np.zeros((N, 6), np.int32)
    fwd[:, 1] = 1
    touched = False
    for _ in range(45):
        g.set_actions_batched(fwd)
        g.step()
        for e in range(N):
            p, st = hip_snapshot(g, e)["agents"][0]["pos"], state(g, e)
            # the controller's sweep stops within ALLOWED_CCD_PEN (0.04) of the ball, its recovery leaves at most MAX_PEN_DEPTH (0.041)
            assert float(np.hypot(p[0] - st["pos"][0], p[2] - st["pos"][2])) >= 1.33 - 0.045, (e, _, p, st)
            # no kick: the ball only answers the ~0.04 of overlap the sweep leaves (~0.3 units / s against a walk of 4.5)
            assert abs(float(st["pos"][0]) - 6.0) < 1.2 and abs(float(st["pos"][2]) - 6.0) < 1e-3 and abs(float(st["pos"][1]) - 2.0) < 1e-3, (e, st)
            touched |= bool(st["contacts"] & 1)
    p = hip_snapshot(g, 0)["agents"][0]["pos"]
    assert float(p[0]) < 7.5 and touched   # it did walk up to the ball
    g.close()


# ---- pixels ----------------------------------------------------------------------------------------------------------------------------------

def is_orange(px):
    r, gr, b = int(px[0]), int(px[1]), int(px[2])
    return r >= gr >= b and r - b > 60 and r > 60


def check_disc(g, e, centre, radius, D):
    """the agent's eye at the ball's height, D along +x of it, looking along -x: the ball's silhouette is a disc about the image's centre of
    angular radius asin(r / D); every pixel whose ray passes clearly inside it is orange, every one clearly outside is not"""
    from canonical_frames import EYE_ABOVE_CENTRE, ray
    W = H = 128
    c, sn = float(F32(np.cos(np.pi / 2))), float(F32(np.sin(np.pi / 2)))
    g.debug_set_agent_pos(e, 0, float(centre[0]) + D, float(centre[1]) - EYE_ABOVE_CENTRE, float(centre[2]))
    g.debug_set_agent_yaw(e, 0, c, sn)
    out = {}
    for mode in ("exact", "fast"):
        g.set_pixel_mode(mode)
        g.render()
        out[mode] = g.get_observation(e, 0).copy()
    d = np.abs(out["exact"].astype(np.int16) - out["fast"].astype(np.int16)).max(axis=-1)   # test_fast_pixels_gpu.py's tolerance
    assert (d > 1).sum() <= max(2, 1e-4 * d.size) and (d > 0).sum() <= max(4, 5e-4 * d.size)
    img = out["exact"]
    px_ang = 2 * np.arctan(np.tan(np.deg2rad(50.0))) / W   # (about one pixel's angle at the centre)
    inside = outside = 0
    for j in range(H):
        for i in range(W):
            r = ray(i, j, W, H)
            ang = np.arccos(-r[2] / np.linalg.norm(r))
            lim = np.arcsin(radius / D)
            row = H - 1 - j   # (observations are stored top row first)
            if ang < lim - 1.0 * px_ang:
                assert is_orange(img[row, i]), (i, j, img[row, i].tolist())
                inside += 1
            elif ang > lim + 1.0 * px_ang:
                assert not is_orange(img[row, i]), (i, j, img[row, i].tolist())
                outside += 1
    return inside


def test_ball_pixels_reset_frame_then_first_tick():
    g = make(2, 1, seed=13, w=128, h=128)
    n_half = check_disc(g, 0, (5.0, 5.0, 5.0), 0.5, 4.0)
    g.set_actions_batched(np.zeros((2, 6), np.int32))
    g.step()
    st = state(g, 0)
    assert st["radius"] == 1.0
    n_one = check_disc(g, 0, st["pos"], 1.0, 4.0)
    assert 3.0 < n_one / n_half < 5.0   # (the disc's area: four times)
    g.close()


# ---- launch shapes, the benchmark's shape ---------------------------------------------------------------------------------------------------

def run_shape(shape, N=32, calls=4, seed=77):
    """N envs, 16 x calls ticks of the device's random policy: every tick's observations (exact pixels), rewards and dones, and the state at the
    end of every call.  step_n: one call of 16 ticks into an output ring of 16."""
    import torch
    g = make(N, 1, seed=5)
    g.set_pixel_mode("exact")
    if shape == "unpipelined":
        g.set_pipelining(False)
    ring = None
    if shape == "step_n":
        ring = (torch.zeros((16, N, 64, 64, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((16, N), dtype=torch.float32, device="cuda:0"),
                torch.zeros((16, N), dtype=torch.uint8, device="cuda:0"))
        torch.cuda.synchronize()
        g.set_output_ring(16, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    ticks, states = [], []
    for c in range(calls):
        if shape == "step_n":
            g.step_n(16, "multidiscrete", seed, 16 * c)
            g.synchronize(); torch.cuda.synchronize()
            o, r, d = ring[0].cpu().numpy(), ring[1].cpu().numpy(), ring[2].cpu().numpy()
            ticks += [(o[j].copy(), r[j].copy(), d[j].copy()) for j in range(16)]
        else:
            for j in range(16):
                g.sample_random_actions(seed, 16 * c + j)
                g.step()
                ticks.append((np.stack([g.get_observation(e, 0) for e in range(N)]), g.get_rewards_array().copy(), g.get_dones().copy()))
        g.synchronize()
        states.append([(state(g, e).tobytes(), g.debug_snapshot_bytes(e).copy()) for e in range(N)])
    g.close()
    return ticks, states


def test_launch_shapes_agree():
    (ta, sa), (tb, sb), (tc, sc) = run_shape("step"), run_shape("step_n"), run_shape("unpipelined")
    for (tx, sx), what in (((tb, sb), "step_n"), ((tc, sc), "unpipelined")):
        for k, ((o1, r1, d1), (o2, r2, d2)) in enumerate(zip(ta, tx)):
            assert np.array_equal(o1, o2), (what, k)
            assert not r1.any() and np.array_equal(r1.view(np.uint32), r2.view(np.uint32)) and np.array_equal(d1, d2), (what, k)
        for c, (x, y) in enumerate(zip(sa, sx)):
            assert all(p[0] == q[0] and np.array_equal(p[1], q[1]) for p, q in zip(x, y)), (what, c)


def test_no_starvation_at_the_benchmark_shape():
    """1024 envs, 128 x 128, the device's random policy, 16 ticks per call into an output ring, overlapped passes (bench.py's shape), 1000 ticks:
    every env crosses its 900-tick episode end, and none may find its next episode missing"""
    import warnings
    import torch
    N, K = 1024, 16
    g = make(N, 1, seed=42, w=128, h=128)
    obs = torch.zeros((K, N, 128, 128, 4), dtype=torch.uint8, device="cuda:0")
    don = torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.set_output_ring(K, obs.data_ptr(), 0, don.data_ptr())
    g.set_pass_overlap(True)
    ends = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # a starved env is reported as a RuntimeWarning by the stepping call
        for c in range(63):
            g.step_n(K, "multidiscrete", 1234, K * c)
            if c == 56:   # ticks 897..912: the episode ends
                g.synchronize(); torch.cuda.synchronize()
                ends += int(don.sum().item())
    g.synchronize()
    assert ends == N, ends
    g.close()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------

def test_env_surface():
    from megaverse_amd.megaverse_env import SUPPORTED_SCENARIOS, MegaverseEnv
    assert "Football" in SUPPORTED_SCENARIOS
    env = MegaverseEnv("Football", 2, 2, 1, False, None, img_w=64, img_h=36)
    obs = env.reset()
    assert len(obs) == 4 and obs[0].shape == (3, 36, 64)
    assert env.get_default_reward_shaping() == {"teamSpirit": 0.0}
    n = ticks_to(60.0)
    for t in range(n):
        obs, rew, dones, infos = env.step([[0, 1, 1, 0, 1, 0]] * 4)
        assert len(rew) == 4 and all(r == 0.0 for r in rew)
        assert list(dones) == [t == n - 1] * 4, (t, dones)
    assert all(inf["true_reward"] == 0.0 for inf in infos)
    env.close()


def test_multitask_union_refuses_football():
    from megaverse_amd.multitask import MultiTaskGym
    with pytest.raises(Exception, match="Football"):
        MultiTaskGym(["TowerBuilding", "Football"], 4, 1, 64, 36)
