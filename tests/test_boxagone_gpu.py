"""BoxAGone on the GPU (mv_tick_boxagone.h, mv_step_boxagone.hip): the reset against the host generator's episodes, the scenario logic
replayed in Python (boxagone_model.step) from the device's own post-physics agents, tick after tick, the physical consequences of vanishing
platforms, the launch shapes against each other, and the Python surface."""
import numpy as np
import pytest

import boxagone_model as M
from hip_util import hip_snapshot
from megaverse_amd.extension import MegaverseGym

pytestmark = pytest.mark.gpu

F32 = np.float32


def make(N, A, seed=42, params=None, w=64, h=64):
    g = MegaverseGym("BoxAGone", w, h, N, A, 1, False, params or {})
    g.seed(seed)
    g.reset()
    return g


def env_streams(master, N):
    r = M.MT19937(master)
    return [M.MT19937(M.rand_range(0, 1 << 30, r)) for _ in range(N)]


def state(g, e):
    return g.debug_boxagone_state(e).view(M.STATE)[0].copy()


def check_fresh(st, snap, blob, A):
    """the device's records of an env that has just taken episode `blob`"""
    n = int(blob["num_platforms"])
    assert st["num_platforms"] == n and st["num_levels"] == blob["num_levels"] and st["takes"] == 0 and st["finished"] == 0
    assert np.array_equal(st["level_y"], blob["level_y"])
    assert np.array_equal(st["plat"][:n].view(np.uint32), blob["platforms"][:n].view(np.uint32))   # level | PRESENT << 4
    assert not st["ticks"].any() and (st["last_platform"][:A] == -1).all() and not st["sec_before"].any()
    assert (st["temps"]["plat"][: 3 * A] == -1).all() and (st["temps"]["sxz"][: 3 * A] == M.PLAT_HXZ).all()
    cells = st["cell"]
    assert (cells >= 0).sum() == n
    for i, p in enumerate(blob["platforms"][:n]):
        assert cells[p["state"], p["x"], p["z"]] == i
    assert snap["num_platforms"] == n and snap["hex_num_boxes"] == 5 + n + 3 * A and snap["episode_sec"] == 0.0 and snap["hex_num_objs"] == 0
    for k in range(A):
        s = blob["spawn"][k]
        assert np.array_equal(snap["agents"][k]["pos"], np.array([s[0] + F32(0.5), s[1] + F32(1.75), s[2] + F32(0.5)], np.float32))
    recs = snap["hex_boxes"]
    colors = [0xFFB400, 0x2EB5D0, 0xD468EE]
    for i, p in enumerate(blob["platforms"][:n]):
        r = recs[5 + i]
        c = np.array([(F32(p["x"]) + F32(0.5)) * F32(2), (F32(p["y"]) + F32(0.5)) * F32(2), (F32(p["z"]) + F32(0.5)) * F32(2)], np.float32)
        assert np.array_equal(r["a"], c - np.array([M.PLAT_HXZ, M.PLAT_HY, M.PLAT_HXZ], np.float32)) and r["color"] == colors[p["state"]]


@pytest.mark.parametrize("A", [1, 2, 4])
def test_reset_matches_generator(A):
    N = 16
    g = make(N, A, seed=7)
    streams = env_streams(7, N)
    for e in range(N):
        check_fresh(state(g, e), hip_snapshot(g, e), M.generate(streams[e], A), A)
    g.close()


def actions_for(policy, N, A, t, rng):
    if policy == "random":
        sizes = [3, 3, 3, 2, 2, 3]
        return np.stack([rng.integers(0, s, N * A) for s in sizes], 1).astype(np.int32)
    acts = np.zeros((N * A, 6), np.int32)
    if policy == "forward":
        acts[:, 1] = 1
    return acts


def same_state(got, want, what):
    for f in ("takes", "finished", "last_platform", "plat", "ticks", "tslot", "cell"):
        assert np.array_equal(got[f], want[f]), (what, f)
    assert np.array_equal(got["sec_before"].view(np.uint32), want["sec_before"].view(np.uint32)), (what, "sec_before")
    assert np.array_equal(got["temps"].view(np.uint32), want["temps"].view(np.uint32)), (what, "temps")


@pytest.mark.parametrize("policy", ["idle", "forward", "random"])
@pytest.mark.parametrize("A", [1, 2, 4])
def test_logic_replay(A, policy):
    N, T = 64, 400
    g = make(N, A, seed=11)
    streams = env_streams(11, N)
    rng = np.random.default_rng(5)
    sts = [state(g, e) for e in range(N)]
    snaps = [hip_snapshot(g, e) for e in range(N)]
    for e in range(N):   # every env's first episode, then its stream stands where the next reset will continue it
        M.generate(streams[e], A)
    shaping = [[snaps[e]["agents"][i]["shaping"].copy() for i in range(A)] for e in range(N)]
    ends = wraps = finishes = 0
    for t in range(T):
        g.set_actions_batched(actions_for(policy, N, A, t, rng))
        g.step()
        rewards, dones = g.get_rewards_array().reshape(N, A), g.get_dones()
        for e in range(N):
            snap, st = hip_snapshot(g, e), state(g, e)
            prev, psnap = sts[e], snaps[e]
            if not dones[e]:
                want, rew, touching, sec, done = M.step(prev, snap["agents"], shaping[e], psnap["episode_sec"], psnap["episode_len"], A)
                assert not done, (e, t)
                assert np.array_equal(rewards[e].view(np.uint32), rew.view(np.uint32)), (e, t, rewards[e], rew)
                same_state(st, want, (e, t))
                assert snap["episode_sec"] == sec and snap["solved"] == want["finished"], (e, t)
                wraps += int(st["takes"] > 3 * A)
                finishes += int(want["finished"] and not prev["finished"])
            else:
                ends += 1
                # the finishing tick: every agent on the floor 0.3 s ago (doneWithTimer) or the episode's length; the env took its next episode
                sec = F32(psnap["episode_sec"] + M.DT)
                assert prev["finished"] and sec >= psnap["episode_len"], (e, t)
                assert not rewards[e].any()
                # the objective of the finished episode: its last scenario step ran on positions the swap-in has replaced.  Every agent was on the
                # floor when doneWithTimer ran; on the last tick an agent is still there (secondsBeforeTouchedFloor unchanged) or -- a jump from the
                # floor takes the capsule's origin 3.3 units up, to y + 0.05 = 6.2: coords.y = 3 -- above it (set to the episode time).  The device's
                # value must be the model's for one of these 2^A cases; idle and forward agents never jump: exactly the first.
                obj = np.array([g.true_objective(e, i) for i in range(A)], np.float32)
                cands = []
                for mask in range(1 << A) if policy == "random" else [0]:
                    last = prev.copy()
                    for i in range(A):
                        if mask >> i & 1:
                            last["sec_before"][i] = psnap["episode_sec"]
                    cands.append(M.true_objective(last, A, psnap["episode_len"]))
                assert any(np.array_equal(obj.view(np.uint32), c.view(np.uint32)) for c in cands), (e, t, obj, cands)
                check_fresh(st, snap, M.generate(streams[e], A), A)
            sts[e], snaps[e] = st, snap
    if policy == "idle":   # (an idle agent visits one platform per level: the ring never wraps)
        assert ends > 0 and finishes > 0
    else:
        assert wraps > 0, "no run took more temporary platforms than the ring holds"
    g.close()


def test_idle_agent_rides_its_temporary_platform_then_falls():
    N, A = 16, 1
    g = make(N, A, seed=3)
    g.set_actions_batched(np.zeros((N, 6), np.int32))
    hist = {e: [] for e in range(N)}
    for t in range(60):
        g.step()
        for e in range(N):
            s, st = hip_snapshot(g, e), state(g, e)
            hist[e].append((s["agents"][0].copy(), st, int(g.get_dones()[e])))
    for e in range(N):
        first = None
        for t, (ag, st, d) in enumerate(hist[e]):
            cx, cy, cz = M.agent_cell(ag["pos"])
            if M.on_ground(ag) and cy in st["level_y"][: st["num_levels"]].tolist():
                lv = st["level_y"][: st["num_levels"]].tolist().index(cy)
                p = int(st["cell"][lv][cx][cz])
                if p >= 0:
                    first = (t, p, cy)
                    break
        assert first is not None, e
        t0, p, cy = first
        st0 = hist[e][t0][1]
        assert M.platform_status(st0, p) == M.VISITED and st0["ticks"][p] == 14   # gone on the first grounded tick
        for t in range(t0, t0 + 14):   # on the temporary platform for its lifetime
            ag, st, d = hist[e][t]
            assert M.agent_cell(ag["pos"])[1] == cy and M.platform_status(st, p) == M.VISITED, (e, t)
        assert M.platform_status(hist[e][t0 + 14][1], p) == M.REMOVED
        # then it falls, strictly, until it stands again (a lower level or the floor)
        y = [h[0]["pos"][1] for h in hist[e][t0 + 14:]]
        k = 1
        while k < len(y) and not M.on_ground(hist[e][t0 + 14 + k][0]):
            assert y[k] < y[k - 1], (e, t0 + 14 + k)
            k += 1
        assert k < len(y) and y[k] < y[0] - 1.0, e
    g.close()


@pytest.mark.parametrize("A", [1, 4])
def test_never_grounded_over_nothing(A):
    N = 32
    g = make(N, A, seed=9)
    rng = np.random.default_rng(1)
    for t in range(150):
        g.set_actions_batched(actions_for("random", N, A, t, rng))
        g.step()
        for e in range(N):
            s, st = hip_snapshot(g, e), state(g, e)
            levels = st["level_y"][: st["num_levels"]].tolist()
            for i in range(A):
                ag = s["agents"][i]
                cx, cy, cz = M.agent_cell(ag["pos"])
                if not (M.on_ground(ag) and cy in levels and F32(ag["pos"][1]) < F32(2 * cy + 1.04 + 0.855 + 0.05)):
                    continue
                lv = levels.index(cy)
                support = False   # a platform or a placed temporary one in the agent's cell or next to it (a capsule can rest on a neighbour's edge)
                for dx in (-1, 0, 1):
                    for dz in (-1, 0, 1):
                        x, z = cx + dx, cz + dz
                        if 0 <= x < 24 and 0 <= z < 24 and st["cell"][lv][x][z] >= 0:
                            p = int(st["cell"][lv][x][z])
                            tp = st["temps"][: 3 * A]
                            support |= M.platform_status(st, p) == M.PRESENT or bool(((tp["plat"] == p) & (tp["away"] == 0)).any())
                assert support, (e, t, i)
    g.close()


def run_shape(shape, N=32, calls=8, seed=77):
    """N envs, 16 x calls ticks of the device's random policy: every tick's observations (exact pixels), rewards and dones, and the state at the end
    of every call.  step_n: one call of 16 ticks into an output ring of 16 (the multi-tick step kernel, the batched observation launch)."""
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
        states.append([(g.debug_boxagone_state(e).copy(), g.debug_snapshot_bytes(e).copy()) for e in range(N)])
    g.close()
    return ticks, states


def test_launch_shapes_agree():
    (ta, sa), (tb, sb), (tc, sc) = run_shape("step"), run_shape("step_n"), run_shape("unpipelined")
    assert sum(int(d.sum()) for _, _, d in ta) >= 8, "the run must cross episode ends"
    for (tx, sx), what in (((tb, sb), "step_n"), ((tc, sc), "unpipelined")):
        for k, ((o1, r1, d1), (o2, r2, d2)) in enumerate(zip(ta, tx)):
            assert np.array_equal(o1, o2), (what, k)
            assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32)) and np.array_equal(d1, d2), (what, k)
        for c, (x, y) in enumerate(zip(sa, sx)):
            assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(x, y)), (what, c)


def test_no_starvation_at_the_benchmark_shape():
    """1024 envs, 128 x 128, the device's random policy, 16 ticks per call into an output ring, overlapped passes (bench.py's shape): episodes end
    every 30-60 ticks, and no env may ever find its next episode missing (it would repeat its done step)."""
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
        for c in range(40):
            g.step_n(K, "multidiscrete", 1234, K * c)
            if c % 8 == 7:   # (a sample: the host otherwise runs ahead of the device as bench.py's loop does)
                g.synchronize(); torch.cuda.synchronize()
                ends += int(don.sum().item())
    assert ends >= N // 2, ends   # (5 x 16 sampled ticks: ~2000 episode ends)
    g.close()


def test_env_surface():
    from megaverse_amd.megaverse_env import SUPPORTED_SCENARIOS, MegaverseEnv
    assert "BoxAGone" in SUPPORTED_SCENARIOS
    env = MegaverseEnv("BoxAGone", 2, 2, 1, False, None, img_w=64, img_h=36)
    obs = env.reset()
    assert len(obs) == 4 and obs[0].shape == (3, 36, 64)
    shaping = env.get_default_reward_shaping()
    assert shaping == {"teamSpirit": 0.0, "boxagoneTouchedFloor": pytest.approx(-0.1), "boxagonePerStepReward": pytest.approx(0.01)}
    obs, rew, dones, infos = env.step([[0] * 6] * 4)
    assert len(rew) == 4 and len(dones) == 4 and not any(dones) and all(inf == {} for inf in infos)
    assert all(r == pytest.approx(0.01) for r in rew)   # on a platform, above the floor
    env.set_reward_shaping({"teamSpirit": 0.0, "boxagoneTouchedFloor": -0.1, "boxagonePerStepReward": 0.5}, 0)
    obs, rew, dones, infos = env.step([[0] * 6] * 4)
    assert rew[0] == pytest.approx(0.5) and rew[2] == pytest.approx(0.01)
    env.close()
    env = MegaverseEnv("BoxAGone", 2, 1, 1, False, {"episodeLengthSec": 1.0}, img_w=64, img_h=36)
    env.reset()
    n = ticks_to(1.0)
    for t in range(n):
        obs, rew, dones, infos = env.step([[0] * 6] * 2)
        assert all(dones) == (t == n - 1)
    assert all(0.0 < inf["true_reward"] <= 1.0 for inf in infos)   # one agent: the fraction of the episode above the floor
    env.close()


def ticks_to(length):
    sec, n = F32(0), 0
    while sec < F32(length):
        sec, n = F32(sec + M.DT), n + 1
    return n


def test_episode_length_param():
    g = make(4, 1, params={"episodeLengthSec": 2.0})
    g.set_actions_batched(np.zeros((4, 6), np.int32))
    done_at = None
    for t in range(40):
        g.step()
        if g.get_dones().all():
            done_at = t + 1
            break
    assert done_at == ticks_to(2.0)
    g.close()


def test_multitask_union_refuses_boxagone():
    from megaverse_amd.multitask import MultiTaskGym
    with pytest.raises(Exception, match="BoxAGone"):
        MultiTaskGym(["TowerBuilding", "BoxAGone"], 4, 1, 64, 36)


# ---- canonical frame (tests/canonical_frames.py): an agent on the floor, pitch 0, looking along -x under a level-0 platform; what every pixel of
# the floor rows and of the platform's underside block shows, derived from the scene as the generator built it -- not from the device's records


def world_ray(i, j, W, H):
    """looking along -x (yaw pi / 2): camera z = world +x, camera y = world y, camera x = world -z"""
    from canonical_frames import ray
    dc = ray(i, j, W, H)
    return np.array([dc[2], dc[1], -dc[0]]), dc


def hand_scene(blob, visited, temps):
    """(lo, hi, colour) of every box in view: the room (white, voxel size 2), the platforms not yet visited (level colour), the temporary ones that
    stand (green, 1.05 x and grown)"""
    boxes = [(np.array(lo, float) * 2, np.array(hi, float) * 2, 0xFFFFFF) for lo, hi in M.ROOM_BOXES]
    colors = [0xFFB400, 0x2EB5D0, 0xD468EE]
    hxz, hy = 0.42 * 2, 0.42 * 2 * 0.045
    for k, p in enumerate(blob["platforms"][: int(blob["num_platforms"])]):
        c = np.array([p["x"] + 0.5, p["y"] + 0.5, p["z"] + 0.5]) * 2
        if k in temps:
            s = 1.05 * 1.03 ** temps[k]
            boxes.append((c - [hxz * s, hy * s, hxz * s], c + [hxz * s, hy * s, hxz * s], 0x3BB372))
        elif k not in visited:
            boxes.append((c - [hxz, hy, hxz], c + [hxz, hy, hxz], colors[int(p["state"])]))
    return boxes


def hand_pixel(eye, i, j, W, H, boxes):
    """float64 ray cast: the nearest face and its Phong shade (canonical_frames.phong), or None near an edge / a tie (silhouettes are not derived)"""
    from canonical_frames import phong
    d, dc = world_ray(i, j, W, H)
    hits = []
    for lo, hi, col in boxes:
        t0, t1, ax = -np.inf, np.inf, -1
        for a in range(3):
            if abs(d[a]) < 1e-12:
                if not (lo[a] <= eye[a] <= hi[a]):
                    break
                continue
            ta, tb = (lo[a] - eye[a]) / d[a], (hi[a] - eye[a]) / d[a]
            if ta > tb:
                ta, tb = tb, ta
            if ta > t0:
                t0, ax = ta, a
            t1 = min(t1, tb)
        else:
            if ax >= 0 and 0.01 <= t0 <= t1 and t0 <= 120.0:
                hits.append((t0, ax, lo, hi, col))
    if not hits:
        return [0, 0, 0, 255]
    hits.sort(key=lambda h: h[0])
    t, ax, lo, hi, col = hits[0]
    if len(hits) > 1 and hits[1][0] - t < 1e-3:
        return None
    P = eye + t * d
    for a in range(3):
        if a != ax and min(P[a] - lo[a], hi[a] - P[a]) < 0.03:
            return None
    Nw = np.zeros(3)
    Nw[ax] = -np.sign(d[ax])
    Nc = np.array([-Nw[2], Nw[1], Nw[0]])
    return phong(dc * t, Nc, col)


def check_view(g, e, eye_xz, rest_y, boxes, rows, cols, what):
    from canonical_frames import EYE_ABOVE_CENTRE
    W = H = 128
    c, sn = float(np.float32(np.cos(np.pi / 2))), float(np.float32(np.sin(np.pi / 2)))
    g.debug_set_agent_pos(e, 0, eye_xz[0], rest_y, eye_xz[1])
    g.debug_set_agent_yaw(e, 0, c, sn)
    g.debug_set_agent_velocity(e, 0, 0.0, 0.0, 0.0)
    eye = np.array([eye_xz[0], float(np.float32(rest_y)) + 0.05 + 0.41, eye_xz[1]])
    assert abs(eye[1] - (rest_y + EYE_ABOVE_CENTRE)) < 1e-6
    out = {}
    for mode in ("exact", "fast"):
        g.set_pixel_mode(mode); g.render()
        out[mode] = g.get_observation(e, 0).copy()
    d = np.abs(out["exact"].astype(np.int16) - out["fast"].astype(np.int16)).max(axis=-1)   # test_fast_pixels_gpu.py's tolerance
    assert (d > 1).sum() <= max(2, 1e-4 * d.size) and (d > 0).sum() <= max(4, 5e-4 * d.size), what
    checked = 0
    for j in rows:
        for i in cols:
            want = hand_pixel(eye, i, j, W, H, boxes)
            if want is None:
                continue
            checked += 1
            for mode in ("exact", "fast"):
                px = out[mode][j, i]
                assert px[3] == 255 and all(abs(int(a) - int(b)) <= 1 for a, b in zip(px[:3], want[:3])), (what, mode, i, j, px.tolist(), want)
    return checked


def test_canonical_frame_platform_underside():
    N = 16
    g = make(N, 1, seed=21, w=128, h=128)
    streams = env_streams(21, N)
    blobs = [M.generate(streams[e], 1) for e in range(N)]
    rest_y = 2.0 + 0.525 + 0.33 - 0.04   # on the floor (top at y = 2)
    eye_y = rest_y + 0.46
    pick = None
    for e, b in enumerate(blobs):
        for k, p in enumerate(b["platforms"][: int(b["num_platforms"])]):
            if p["state"] != 0 or p["y"] != 3 or not (4 <= p["z"] <= 19) or p["x"] < 5:   # (below the light: the underside is ambient only)
                continue
            yu = (p["y"] + 0.5) * 2 - 0.42 * 2 * 0.045
            dist = max(7.0, 1.8 * (yu - eye_y))
            xa = (p["x"] + 0.5) * 2 + dist
            if xa <= 42.0:
                pick = (e, k, p, xa, dist, yu)
                break
        if pick:
            break
    assert pick
    e, k, p, xa, dist, yu = pick
    b = blobs[e]
    zc = (p["z"] + 0.5) * 2
    from canonical_frames import row_of
    jc = int(row_of(yu - eye_y, dist, 128))
    block_rows, block_cols = range(jc - 3, jc + 4), range(58, 70)
    floor_rows, floor_cols = (6, 12, 20, 28, 36), range(4, 124, 8)
    # 1. the platform is there: its underside, ambient only (N.L < 0), in its level's colour
    n = check_view(g, e, (xa, zc), rest_y, hand_scene(b, set(), {}), floor_rows, floor_cols, "floor")
    assert n >= 60
    n = check_view(g, e, (xa, zc), rest_y, hand_scene(b, set(), {}), block_rows, block_cols, "underside")
    assert n >= 30
    from canonical_frames import phong
    assert hand_pixel(np.array([xa, eye_y, zc]), 63, jc, 128, 128, hand_scene(b, set(), {})) == phong(np.array([0.0, 0.0, -1.0]), np.array([0.0, -1.0, 0.0]), 0xFFB400)
    # 2. an agent stands on it: the platform goes, a green one 1.05 x its size takes its place
    top = (p["y"] + 0.5) * 2 + 0.42 * 2 * 0.045 + 0.525 + 0.33
    on_top = ((p["x"] + 0.5) * 2, top, zc)
    g.set_actions_batched(np.zeros((N, 6), np.int32))
    for t in range(6):
        g.debug_set_agent_pos(e, 0, *on_top)
        g.debug_set_agent_velocity(e, 0, 0.0, 0.0, 0.0)
        g.step()
        st = state(g, e)
        if M.platform_status(st, k) == M.VISITED:
            break
    assert M.platform_status(st, k) == M.VISITED and st["ticks"][k] == 14
    pos = hip_snapshot(g, e)["agents"][0]["pos"].copy()   # standing on the temporary platform
    assert check_view(g, e, (xa, zc), rest_y, hand_scene(b, {k}, {k: 0}), block_rows, block_cols, "temporary") >= 30
    # 3. it lives out its 15 ticks (growing 1.03 x per tick in the last five) with the agent on it, then what lay behind shows
    while st["ticks"][k] > 0:
        g.debug_set_agent_pos(e, 0, *[float(v) for v in pos])
        g.debug_set_agent_velocity(e, 0, 0.0, 0.0, 0.0)
        g.step()
        st = state(g, e)
        if st["ticks"][k] == 3:   # grown at 5, 4 and 3 ticks left
            assert check_view(g, e, (xa, zc), rest_y, hand_scene(b, {k}, {k: 3}), block_rows, block_cols, "temporary, grown") >= 30
    assert M.platform_status(st, k) == M.REMOVED and not g.get_dones()[e]
    assert check_view(g, e, (xa, zc), rest_y, hand_scene(b, {k}, {}), block_rows, block_cols, "behind") >= 30
    g.close()
