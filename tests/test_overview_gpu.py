"""GPU: overview cameras (mv_set_overview / mv_draw_overview).
1. Identity: an AGENT camera with a zero offset under the first-person rule is the agent's own observation -- byte for byte the exact pass's frame and the
   oracle's, for every scenario of the matrix (every list tier of the overview's kernels), every agent, after reset and after 40 scripted ticks, at sizes with
   partial tiles; once at the hires size against draw_hires.
2. Free and chase cameras against the float64 model of tests/overview_reference.py (never a kernel's output), own-body drawing provably covered.
3. Non-interference: a pipelined fast-mode gym that draws an overview after every stepping call equals a twin that never attached, byte for byte.
4. Surface: caller-owned buffers, detach / re-attach, default pose, device and host camera forms, clamping, refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import depth_reference as dr
import oracle_lib
import overview_reference as ovr
import pixel_reference as pr
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd import follow, look_at, overview_default_camera
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.multitask import MultiTaskGym

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MATRIX = pr.MATRIX + [("Empty", 1)]


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def advance(gyms, og, n_envs, A, ticks, first=0):
    for tick in range(first, first + ticks):
        acts, masks = pr.scripted(n_envs, A, tick)
        if og is not None:
            og.set_action_masks(masks); og.step_norender()
        for g in gyms:
            g.set_actions_batched(acts); g.step_no_render()


def frames(g):
    return np.stack([g.get_observation(e, a) for e in range(g.num_envs) for a in range(g.num_agents_per_env)])


# ---- 1. identity -----------------------------------------------------------------------------------------------------------------------------------
def check_identity(og, hg, ov, N, A, what):
    hg.render()
    for e in range(N):
        og.render_env(e)
    own = frames(hg).reshape(N, A, *ov.shape[1:])
    for k in range(A):
        hg.set_overview_cameras(follow(k, first_person=True))
        hg.draw_overview()
        got = host(ov)
        for e in range(N):
            assert np.array_equal(got[e], own[e, k]), f"{what}: env {e} from agent {k}'s eye differs from the agent's own observation"
            assert np.array_equal(got[e], og.get_observation(e, k)), f"{what}: env {e} from agent {k}'s eye differs from the oracle's frame"
            assert np.array_equal(got[e], hg.get_overview_observation(e))
    assert hg.overview_dropped() == (0, 0), what


@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", MATRIX)
def test_agent_camera_is_the_agents_observation(hip, scenario, A, W, H):
    N = pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    hg = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    hg.set_pixel_mode("exact")
    for g in (og, hg):
        g.seed(pr.SEED); g.reset()
    ov = hg.set_overview(W, H)
    assert tuple(ov.shape) == (N, H, W, 4) and ov.dtype == torch.uint8
    check_identity(og, hg, ov, N, A, f"{scenario} {W}x{H} after reset")
    advance([hg], og, N, A, 40)
    for e in range(N):
        assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
    check_identity(og, hg, ov, N, A, f"{scenario} {W}x{H} after 40 ticks")
    og.close(); hg.close()


def test_agent_camera_at_the_hires_size(hip):
    """overview 128 x 72 against draw_hires in exact mode: another size, the same frames"""
    N, A = pr.N_ENVS, 2
    hg = MegaverseGym("TowerBuilding", 64, 64, N, A, 1, False, {})
    hg.set_pixel_mode("exact"); hg.seed(pr.SEED); hg.reset()
    advance([hg], None, N, A, 40)
    hg.set_render_resolution(128, 72)
    hg.draw_overview()   # (not attached: nothing)
    hg.draw_hires()
    ov = hg.set_overview(128, 72)
    for k in range(A):
        hg.set_overview_cameras([follow(k, first_person=True)] * N)
        hg.draw_overview()
        got = host(ov)
        for e in range(N):
            assert np.array_equal(got[e], hg.get_hires_observation(e, k)), f"env {e} agent {k}"
    assert hg.overview_dropped() == (0, 0)
    hg.close()


# ---- 2. free cameras against the float64 model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ovr.POSES)
@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", ovr.SCENARIOS)
def test_free_and_chase_cameras_against_float64(hip, scenario, A, W, H, name):
    """the default pose, a look_at beside agent 0 and a chase camera behind it, at the seed and tick overview_reference.CASES picked on the model alone: the
    rule of overview_reference.judge on the device's own snapshot, once it equals the oracle's"""
    N = ovr.N_ENVS
    seed, ticks = ovr.CASES[scenario, (W, H)][name]
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    hg = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    for g in (og, hg):
        g.seed(seed); g.reset()
    advance([hg], og, N, A, ticks)
    ov = hg.set_overview(W, H)
    snaps = []
    for e in range(N):
        assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
        snaps.append(hip_snapshot(hg, e))
    cams = np.stack([ovr.pose(s, name) for s in snaps])
    hg.set_overview_cameras(cams)
    hg.draw_overview()
    got = host(ov)
    interior = excused = 0
    for e in range(N):
        model = ovr.render(snaps[e], cams[e], W, H, A)
        if name != "default":
            own = int((model.winner == ovr.capsule_id(snaps[e], 0, A)).sum())
            assert own >= ovr.OWN_PIXELS, f"{scenario} {name} env {e}: agent 0's own capsule wins {own} pixels in the model"
        r = ovr.judge(got[e], model)
        assert not r.failures, f"{scenario} {W}x{H} {name} env {e}: {len(r.failures)} pixels outside the rule, first (x, y, got, model) {r.failures[:4]}"
        interior += r.interior; excused += r.excused
    share = interior / (N * W * H)
    print(f"{scenario} {W}x{H} {name}: interior share {share:.3f}, curved pixels excused {excused} (cap {pr.CAP:.0e} of {N * W * H})")
    assert share >= dr.INTERIOR_SHARE
    assert excused <= pr.CAP * N * W * H
    assert hg.overview_dropped() == (0, 0)
    og.close(); hg.close()


# ---- 3. non-interference -------------------------------------------------------------------------------------------------------------------------------
def test_drawing_between_pipelined_calls_changes_nothing(hip):
    N, A, W, H, RING = 4, 2, 48, 20, 8
    gyms, rings = [], []
    for _ in range(2):
        g = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
        g.set_pixel_mode("fast")
        assert g.pixel_mode() == "fast" and g.pipelining()
        g.seed(13); g.reset()
        obs = torch.zeros((RING, N * A, H, W, 4), dtype=torch.uint8, device="cuda")
        rew = torch.zeros((RING, N * A), dtype=torch.float32, device="cuda")
        done = torch.zeros((RING, N), dtype=torch.uint8, device="cuda")
        g.set_output_ring(RING, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
        gyms.append(g); rings.append((obs, rew, done))
    a, twin = gyms
    before = a.arena_bytes()
    assert before == twin.arena_bytes()
    ov = a.set_overview(W, H)
    cap = a.overview_capacity()
    assert cap == 256

    def up(b):
        return (b + 255) // 256 * 256
    arrays = up(N * cap * 32) + up(N * cap * 8) + up(N * 1024) + 3 * up(N * 4) + 2 * up(N * 64) + up(8)   # mv_overview.h: overview_layout
    assert a.arena_bytes() - before == arrays + N * W * H * 4
    a.set_overview_cameras([follow(e % A, back=1.5, up=0.5) for e in range(N)])
    tick, seen = 0, []
    for call in range(10):   # 5 single ticks and 5 calls of 8 ticks in turn; with the 3 ticks below 48 in all
        if call % 2 == 0:
            acts, _ = pr.scripted(N, A, tick)
            for g in gyms:
                g.set_actions_batched(acts); g.step()
            tick += 1
        else:
            for g in gyms:
                g.step_n(8, "multidiscrete", 21, tick)
            tick += 8
        a.draw_overview()
        twin.draw_overview()   # (not attached: returns, draws nothing)
        seen.append(host(ov).copy())
        for (x, y) in zip(rings[0], rings[1]):
            assert np.array_equal(host(x), host(y)), f"call {call}: a ring differs"
        assert np.array_equal(a.get_true_objectives().view(np.uint32), twin.get_true_objectives().view(np.uint32))
    for g in gyms:
        g.step_n(3, "multidiscrete", 21, tick)
    tick += 3
    assert tick == 48
    for (x, y) in zip(rings[0], rings[1]):
        assert np.array_equal(host(x), host(y))
    for e in range(N):
        assert not diff_snapshots(hip_snapshot(a, e), hip_snapshot(twin, e), A)
    assert twin.overview_obs() is None and twin.arena_bytes() == before and twin.overview_dropped() == (0, 0)
    assert any(not np.array_equal(seen[0], s) for s in seen[1:]), "the overview never changed while the envs moved"
    assert a.overview_dropped() == (0, 0)
    a.set_overview(0, 0)
    assert a.arena_bytes() - before == arrays   # (the arrays stay until mv_close; the gym's own frames went)
    for g in gyms:
        g.close()


# ---- 4. surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_surface(hip):
    N, A, W, H = 4, 2, 48, 20
    g = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
    g.seed(3); g.reset()
    advance([g], None, N, A, 12)
    lib = g._lib
    # a caller-owned tensor is written in place; a sentinel around it survives
    big = torch.full((N + 2, H, W, 4), 0x5A, dtype=torch.uint8, device="cuda")
    mine = big[1:N + 1]
    assert g.set_overview(W, H, mine) is mine and g.overview_obs() is mine
    g.draw_overview()
    got = host(big)
    assert (got[0] == 0x5A).all() and (got[-1] == 0x5A).all()
    default = got[1:N + 1]
    assert (default[..., 3] == 255).all() and (default[..., :3] != 0).any()
    # the default pose is the record overview_default_camera returns
    g.set_overview_cameras(overview_default_camera()); g.draw_overview()
    assert np.array_equal(host(mine), default)
    # device and host camera forms give equal frames; None restores the default
    cams = np.stack([follow(e % A, back=2.0, up=1.0) if e % 2 else look_at((3.0 + e, 6.0, 2.5), (8.0, 1.0, 8.0)) for e in range(N)])
    g.set_overview_cameras(cams); g.draw_overview()
    from_host = host(mine)
    assert not np.array_equal(from_host, default)
    dev = torch.from_numpy(cams.view(np.int32).reshape(N, 16).copy()).cuda()
    g.set_overview_cameras(None); g.draw_overview()
    assert np.array_equal(host(mine), default)
    g.set_overview_cameras(dev); g.draw_overview()
    assert np.array_equal(host(mine), from_host)
    assert g.overview_dropped() == (0, 0)
    # a device record with agent = A is taken as FREE with the record's pose, and counted
    bad = cams.copy()
    bad[0] = look_at((3.0, 6.0, 2.5), (8.0, 1.0, 8.0)); bad["agent"][0] = A
    free = bad.copy(); free["agent"][0] = -1
    g.set_overview_cameras(free); g.draw_overview()
    want = host(mine)
    g.set_overview_cameras(torch.from_numpy(bad.view(np.int32).reshape(N, 16).copy()).cuda()); g.draw_overview()
    assert np.array_equal(host(mine), want)
    assert g.overview_dropped() == (0, 1)
    # detaching and re-attaching at another size, gym-owned
    g.set_overview(0, 0)
    assert g.overview_obs() is None
    g.draw_overview()   # (detached: nothing)
    assert np.array_equal(host(mine), want)
    own = g.set_overview(64, 64)
    assert tuple(own.shape) == (N, 64, 64, 4)
    g.set_overview_cameras(None); g.draw_overview()
    assert (host(own)[..., 3] == 255).all() and g.get_overview_observation(N - 1).shape == (64, 64, 4)
    # refusals carry text
    with pytest.raises(RuntimeError, match="mv_set_overview.*1025"):
        g.set_overview(1025, 64)
    with pytest.raises(ValueError, match="set_overview_cameras.*agent"):
        g.set_overview_cameras(follow(A))
    rec = np.repeat(follow(A).reshape(1), N)
    assert lib.mv_set_overview_cameras_host(g._g, rec.ctypes.data) == -1 and b"agent 2 is outside -1 .. 1" in lib.mv_last_error()
    rec = np.repeat(follow(0).reshape(1), N); rec["pad"][2, 1] = 7
    assert lib.mv_set_overview_cameras_host(g._g, rec.ctypes.data) == -1 and b"pad" in lib.mv_last_error()
    with pytest.raises(ValueError, match="set_overview"):
        g.set_overview(64, 64, torch.zeros((N, 64, 63, 4), dtype=torch.uint8, device="cuda"))
    other = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
    other.seed(1); other.reset()
    handles = (C.c_void_p * 2)(g._g.value, other._g.value)
    out = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1
    assert b"an overview attached" in lib.mv_last_error() and b"mv_set_overview" in lib.mv_last_error()
    assert lib.mv_step_many(handles, 2, 1, 1, 0, 0) == -1 and b"mv_set_overview" in lib.mv_last_error()
    g.set_overview(0, 0)
    assert lib.mv_group_create(handles, 2, C.byref(out)) == 0
    with pytest.raises(RuntimeError, match="mv_set_overview.*mv_group"):
        g.set_overview(64, 64)
    lib.mv_group_destroy(out)
    with pytest.raises(RuntimeError, match="mv_set_overview"):
        MultiTaskGym.set_overview(None, 64, 64)
    g.close(); other.close()


def test_env_render_overview(hip):
    """MegaverseEnv(overview=(w, h)): render_overview tiles the envs' frames as BGR, top row first; render() is what it is without the option"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    N, A = 3, 2
    env = MegaverseEnv("TowerBuilding", N, A, img_w=64, img_h=36, overview=(48, 20))
    plain = MegaverseEnv("TowerBuilding", N, A, img_w=64, img_h=36)
    for e in (env, plain):
        e.seed(5); e.reset()
        e.env.set_render_resolution(64, 36)
    assert plain.overview_obs() is None
    with pytest.raises(RuntimeError, match="overview="):
        plain.render_overview()
    img = env.render_overview()
    assert img.shape == (20, N * 48, 3) and img.dtype == np.uint8 and img.any()
    ov = host(env.overview_obs())
    for e in range(N):
        assert np.array_equal(img[:, e * 48:(e + 1) * 48], ov[e, ::-1][:, :, [2, 1, 0]])
    env.set_overview_cameras([follow(e % A, back=2.0, up=1.0) for e in range(N)])
    assert not np.array_equal(env.render_overview(), img)
    assert np.array_equal(env.render(mode='rgb_array'), plain.render(mode='rgb_array'))
    env.close(); plain.close()


def test_env_order_draws_the_same_bytes(hip, monkeypatch):
    """MV_OVERVIEW_ORDER=0 (read at the first attach): no frame-order launch, the envs drawn in env order -- the order only schedules"""
    N, A, W, H = 6, 2, 48, 20
    got = []
    for order in ("1", "0"):
        monkeypatch.setenv("MV_OVERVIEW_ORDER", order)
        g = MegaverseGym("ObstaclesHard", W, H, N, A, 1, False, {})
        g.seed(9); g.reset()
        advance([g], None, N, A, 12)
        ov = g.set_overview(W, H)
        frames_ = []
        for cam in (overview_default_camera(), follow(1, back=2.0, up=1.0), follow(0, first_person=True)):
            g.set_overview_cameras(cam); g.draw_overview()
            frames_.append(host(ov))
        assert g.overview_dropped() == (0, 0)
        got.append(np.stack(frames_))
        g.close()
    assert np.array_equal(got[0], got[1]) and got[0].any()
