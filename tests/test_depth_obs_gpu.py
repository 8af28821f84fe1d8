"""GPU: depth observations (mv_set_depth_obs).  Known answers against the float64 closed forms of tests/depth_reference.py (never a kernel's output) in both
pixel modes and at sizes with edge tiles and an odd width; one trace / two outputs in exact mode; the follower behind a fast pass against it, bit for bit; hit /
no-hit against the float64 reference under the project's pixel rule; the half-precision format; which entries are written by which calls; refusals."""
import os

import numpy as np
import pytest
import torch

import depth_reference as dr
import oracle_lib
import pixel_reference as pr
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MV_DEPTH_F16, MegaverseGym
from megaverse_amd.multitask import MultiTaskGym

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MATRIX = pr.MATRIX + [("Empty", 1)]
BG = np.array([0, 0, 0, 255], np.uint8)


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels


def planes(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def frames(g):
    return np.stack([g.get_observation(e, a) for e in range(g.num_envs) for a in range(g.num_agents_per_env)])


def sentinel(t):
    t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).fill_(0x7FC1 if t.dtype == torch.float16 else 0x7FC12345)   # a NaN pattern


def is_sentinel(a):
    return a.view(np.uint16) == 0x7FC1 if a.dtype == np.float16 else a.view(np.uint32) == 0x7FC12345


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------------------
def judge_known(og, hg, env, W, H, what):
    """both pixel modes' plane of (env, agent 0) against the float64 caster at the interior world-box pixels, 0 at the interior background pixels"""
    assert not diff_snapshots(og.snapshot(env), hip_snapshot(hg, env), 1), f"{what}: the twin's state differs"
    snap = hip_snapshot(hg, env)   # (the pose of the state-observation row: the same bits)
    _, prim = og.render_f64(env, 0)
    m, bg = dr.interior_mask(prim, og.prim_table(env, 0), dr.is_world_box), dr.background_mask(prim)
    t, box, axis, dwk, lo, hi = dr.expected_boxes(snap, 0, W, H)
    assert m.sum() > 0 and np.isfinite(t[m]).all()
    d = hg.depth_obs_ring()
    for mode in ("exact", "fast"):
        sentinel(d)
        hg.set_pixel_mode(mode); hg.render()
        got = planes(d)[0, env].astype(np.float64)
        err = np.abs(got[m] - t[m]) / dr.slab_bound(t[m], dwk[m])
        print(f"{what} {mode}: {int(m.sum())} hit pixels, largest error {err.max():.3f} of the bound; {int(bg.sum())} background pixels")
        assert (err <= 1.0).all(), f"{what} {mode}: {int((err > 1).sum())} pixels outside the bound, worst {err.max():.1f} x at {np.argwhere(m)[err.argmax()].tolist()}"
        assert (got[bg] == 0).all(), f"{what} {mode}: depth at background pixels"
        assert np.array_equal(got, hg.get_depth_observation(env, 0).astype(np.float64))   # (the read-back of one plane)


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_known_answers_tower(hip, W, H):
    """(a) the wall square-on, (b) the floor under the agent, (c) a movable box's front face -- through the caster the CPU test ties to the closed forms"""
    og = oracle_lib.OracleGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1)
    hg = MegaverseGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1, False, {})
    for g in (og, hg):
        g.seed(dr.TOWER_SEED); g.reset()
    hg.set_depth_obs(True)
    e = dr.pose_tower_wall(og, [og, hg])
    judge_known(og, hg, e, W, H, f"TowerBuilding wall {W}x{H}")
    e, _ = dr.pose_tower_box(og, [og, hg])
    judge_known(og, hg, e, W, H, f"TowerBuilding box {W}x{H}")
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
@pytest.mark.parametrize("pose", list(dr.EMPTY_POSES))
def test_known_answers_empty(hip, pose, W, H):
    """(d) the float64 ray / AABB caster over the snapshot's boxes, at pitch 0 and at two pitched cameras"""
    og = oracle_lib.OracleGym("Empty", W, H, dr.EMPTY_ENVS, 1, 1)
    hg = MegaverseGym("Empty", W, H, dr.EMPTY_ENVS, 1, 1, False, {})
    for g in (og, hg):
        g.seed(dr.EMPTY_SEED); g.reset()
    hg.set_depth_obs(True)
    e = dr.pose_empty([og, hg], pose)
    judge_known(og, hg, e, W, H, f"Empty {pose} {W}x{H}")
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_known_answers_football(hip, W, H):
    """(e) the float64 ray / sphere on Football's ball, placed BALL_DIST in front of a pitch-0 agent, inside 0.8 of its projected radius"""
    og = oracle_lib.OracleGym("Football", W, H, 4, 2, 1)
    hg = MegaverseGym("Football", W, H, 4, 2, 1, False, {})
    for g in (og, hg):
        g.seed(dr.EMPTY_SEED); g.reset()
    d = hg.set_depth_obs(True)
    e, centre, radius = dr.pose_football([og, hg])
    assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), 2)
    a = hip_snapshot(hg, e)["agents"][0]
    eye, C = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, share = dr.cast_sphere(eye, C, W, H, centre, radius)
    inside = np.isfinite(t) & (share <= 0.8)
    assert inside.sum() >= 4
    for mode in ("exact", "fast"):
        sentinel(d); hg.set_pixel_mode(mode); hg.render()
        got = planes(d)[0].reshape(4, 2, H, W)[e, 0].astype(np.float64)
        rel = np.abs(got[inside] - t[inside]) / t[inside]
        print(f"Football {W}x{H} {mode}: {int(inside.sum())} ball pixels, largest relative error {rel.max():.2e} (bound {dr.SPHERE_REL:.1e})")
        assert (rel <= dr.SPHERE_REL).all()
    og.close(); hg.close()


# ---- 2., 3., 5., 7. one trace / two outputs; the follower; half precision; planes per agent -------------------------------------------------------------
def advance(gyms, og, n_envs, A, ticks):
    for tick in range(ticks):
        acts, masks = pr.scripted(n_envs, A, tick)
        if og is not None:
            og.set_action_masks(masks); og.step_norender()
        for g in gyms:
            g.set_actions_batched(acts); g.step_no_render()


@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", MATRIX)
def test_two_outputs_follower_and_half(hip, scenario, A, W, H):
    N = pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    hg, twin = (MegaverseGym(scenario, W, H, N, A, 1, False, {}) for _ in range(2))
    for g in (og, hg, twin):
        g.seed(pr.SEED); g.reset()
    d = hg.set_depth_obs(True)
    advance([hg, twin], og, N, A, 12)
    # exact mode: one trace, two outputs -- the colours are the oracle's and the twin's, byte for byte
    sentinel(d)
    for g in (hg, twin):
        g.set_pixel_mode("exact"); g.render()
    for e in range(N):
        og.render_env(e)
    want = np.stack([og.get_observation(e, a) for e in range(N) for a in range(A)])
    rgb, exact = frames(hg), planes(d)[0]
    assert np.array_equal(rgb, want), f"{scenario}: exact mode with depth attached differs from the oracle"
    assert np.array_equal(rgb, frames(twin)), f"{scenario}: exact mode with depth attached differs from a gym without"
    assert not is_sentinel(exact).any() and np.isfinite(exact).all() and (exact >= 0).all() and (exact <= 120.0).all()
    drawn = (rgb != BG).any(-1)
    assert (exact[drawn] > 0).all(), f"{scenario}: {int((exact[drawn] == 0).sum())} coloured pixels without a depth"
    assert (exact[exact > 0] >= np.float32(0.01)).all()
    # fast mode: the follower's planes are the one-trace form's bits; the colours are the twin's bytes
    sentinel(d)
    for g in (hg, twin):
        g.set_pixel_mode("fast"); g.render()
    assert np.array_equal(planes(d)[0].view(np.uint32), exact.view(np.uint32)), f"{scenario}: the follower's depth differs from the exact pass's"
    assert np.array_equal(frames(hg), frames(twin)), f"{scenario}: fast mode with depth attached differs from a gym without"
    if A > 1:   # the planes are per agent
        per = exact.reshape(N, A, H, W)
        assert any(not np.array_equal(per[e, 0], per[e, 1]) for e in range(N))
    # half precision: float16(float32), bit for bit, in both forms
    hg.set_depth_obs(None)
    h = hg.set_depth_obs(True, "float16")
    assert hg._lib.mv_get_depth_format(hg._g) == MV_DEPTH_F16 and h.dtype == torch.float16
    for mode in ("fast", "exact"):
        sentinel(h)
        hg.set_pixel_mode(mode); hg.render()
        assert np.array_equal(planes(h)[0].view(np.uint16), exact.astype(np.float16).view(np.uint16)), f"{scenario} {mode}: float16 planes are not float16(float32)"
    assert np.array_equal(hg.get_depth_observation(N - 1, A - 1), exact.reshape(N, A, H, W)[N - 1, A - 1].astype(np.float16).astype(np.float32))
    for g in (og, hg, twin):
        g.close()


@pytest.mark.parametrize("W,H", [(40, 24), (128, 128)])
@pytest.mark.parametrize("scenario,A", MATRIX)
def test_half_precision_edge_and_large(hip, scenario, A, W, H):
    """float16 = float16(float32), bit for bit, on every scenario of the matrix -- every list size's instantiation, depth only and colours + depth -- at a
    size with edge tiles (40 x 24) and at 128 x 128, on the state a dozen scripted ticks leave"""
    N = pr.N_ENVS
    g = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    g.seed(pr.SEED); g.reset()
    advance([g], None, N, A, 12)
    d = g.set_depth_obs(True); g.render(); f32 = planes(d)[0]
    assert (f32 > 0).any() and not is_sentinel(f32).any()
    g.set_depth_obs(None)
    h = g.set_depth_obs(True, torch.float16)
    for mode in ("fast", "exact"):
        sentinel(h); g.set_pixel_mode(mode); g.render()
        assert np.array_equal(planes(h)[0].view(np.uint16), f32.astype(np.float16).view(np.uint16)), f"{scenario} {W}x{H} {mode}: float16 planes are not float16(float32)"
    g.close()


# ---- 4. hit / no-hit against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", MATRIX)
def test_hit_or_miss_against_float64(hip, scenario, A, W, H):
    """(depth == 0) against (prim < 0) of the float64 reference; every disagreement explained by explain_f64 under the oracle's parameters, within the cap"""
    N = pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    hg = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    for g in (og, hg):
        g.seed(pr.SEED); g.reset()
    d = hg.set_depth_obs(True)
    advance([hg], og, N, A, 40)
    hg.render()
    got = planes(d)[0].reshape(N, A, H, W)
    pixels, explained = 0, 0
    for e in range(N):
        assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
        for a in range(A):
            _, prim, _ = pr.reference(og, e, a)
            pixels += W * H
            ys, xs = np.nonzero((got[e, a] == 0) != (prim < 0))
            if not len(ys):
                continue
            colors, counts = og.explain_f64(e, a, np.stack([xs, ys], 1), pr.DELTA_ORACLE, pr.EPS_4ULP)
            for k, (x, y) in enumerate(zip(xs, ys)):
                cand = colors[k, : counts[k]]
                is_bg = (cand[:, :3] == 0).all(-1)
                ok = is_bg.any() if got[e, a, y, x] == 0 else (~is_bg).any()
                assert ok, f"{scenario} env {e} agent {a} ({x}, {y}): depth {got[e, a, y, x]} against prim {prim[y, x]} is not explained"
                explained += 1
    print(f"{scenario} {W}x{H}: {explained} explained disagreements of {pixels} pixels (cap {pr.CAP:.0e})")
    assert explained <= pr.CAP * pixels
    og.close(); hg.close()


# ---- 6. where it is written ------------------------------------------------------------------------------------------------------------------------
def ring_gym(scenario="TowerBuilding", N=4, A=1, W=40, H=24, count=4, dtype="float32", mode="fast"):
    g = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    g.set_pixel_mode(mode); g.seed(7); g.reset()
    obs = torch.zeros((count, N * A, H, W, 4), dtype=torch.uint8, device="cuda")
    g.set_output_ring(count, obs.data_ptr())
    d = g.set_depth_obs(True, dtype)
    assert tuple(d.shape) == (count, N * A, H, W) and g._lib.mv_get_depth_obs(g._g) == count
    return g, obs, d


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_step_n_fills_the_ring(hip, mode):
    """step_n(4) into a ring of 4: every entry is mv_render's plane of a twin stepped tick by tick; one extra pass-side launch per drawn tick in fast mode"""
    g, obs, d = ring_gym(mode=mode)
    twin = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    twin.set_pixel_mode(mode); twin.seed(7); twin.reset()
    td = twin.set_depth_obs(True)
    plain = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})   # no depth: the launch counts to compare with
    plain.set_pixel_mode(mode); plain.seed(7); plain.reset()
    pobs = torch.zeros_like(obs); plain.set_output_ring(4, pobs.data_ptr())
    sentinel(d)
    c0, p0 = g.debug_launch_counts(), plain.debug_launch_counts()
    g.step_n(4, "multidiscrete", 9, 0); plain.step_n(4, "multidiscrete", 9, 0)
    c1, p1 = g.debug_launch_counts(), plain.debug_launch_counts()
    assert c1[0] - c0[0] == p1[0] - p0[0]
    assert (c1[1] - c0[1]) - (p1[1] - p0[1]) == (4 if mode == "fast" else 0)
    got = planes(d)
    assert not is_sentinel(got).any()
    assert np.array_equal(planes(obs), planes(pobs)), "the colours differ from those of a gym without depth"
    for j in range(4):
        twin.step_n(1, "multidiscrete", 9, j, render="none")
        twin.render()
        assert np.array_equal(got[j].view(np.uint32), planes(td)[0].view(np.uint32)), f"entry {j} is not the plane of tick {j}"
    # render = 'none' leaves every byte; 'last' and a macro step write the one entry
    sentinel(d); g.step_n(4, "multidiscrete", 9, 4, render="none")
    assert is_sentinel(planes(d)).all()
    g.step_n(4, "multidiscrete", 9, 8, render="last")
    got = planes(d)
    assert is_sentinel(got[:3]).all() and not is_sentinel(got[3]).any()
    sentinel(d); g.macro_step(3, np.zeros((4, 6), np.int32), render="last")
    got = planes(d)
    assert not is_sentinel(got[0]).any() and is_sentinel(got[1:]).all()
    sentinel(d); g.macro_step(3, np.zeros((4, 6), np.int32), render="none"); g.step_no_render()
    assert is_sentinel(planes(d)).all()
    for x in (g, twin, plain):
        x.close()


def test_masks_resets_and_single_steps(hip):
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(7); g.reset()
    d = g.set_depth_obs(True)
    assert tuple(d.shape) == (1, 4, 24, 40)
    sentinel(d); g.step()
    assert not is_sentinel(planes(d)).any()
    assert tuple(g.depth_obs().shape) == (4, 24, 40)
    # a draw mask leaves the undrawn envs' planes alone
    sentinel(d); g.set_draw_mask(np.array([1, 0, 1, 0], np.uint8)); g.step()
    got = planes(d)[0]
    assert not is_sentinel(got[[0, 2]]).any() and is_sentinel(got[[1, 3]]).all()
    g.step_n(3, "multidiscrete", 1, 0)
    got = planes(d)[0]
    assert not is_sentinel(got[[0, 2]]).any() and is_sentinel(got[[1, 3]]).all()
    g.set_draw_mask(None)
    # mv_reset and reset_envs(render = True) refresh the planes
    sentinel(d); g.reset()
    assert not is_sentinel(planes(d)).any()
    sentinel(d); g.reset_envs(np.array([0, 1, 0, 0], np.uint8), render=True)
    assert not is_sentinel(planes(d)).any()
    sentinel(d); g.reset_envs(np.array([0, 1, 0, 0], np.uint8), render=False)
    assert is_sentinel(planes(d)).all()
    # not pipelined: the same planes
    g.render(); want = planes(d)
    g.set_pipelining(False); sentinel(d); g.render()
    assert np.array_equal(planes(d).view(np.uint32), want.view(np.uint32))
    g.close()


def test_two_agents_see_each_other(hip):
    """two agents per env, face to face: the other agent's capsule is the nearest surface at the frame's centre, nearer than the room behind it"""
    W, H = 64, 64
    for scenario in ("TowerBuilding", "Football"):
        g = MegaverseGym(scenario, W, H, 4, 2, 1, False, {})
        g.seed(3); g.reset()
        d = g.set_depth_obs(True)
        s = hip_snapshot(g, 0)
        x, y, z = (float(v) for v in s["agents"][0]["pos"])
        c, sn = float(np.float32(np.cos(np.pi / 2))), float(np.float32(np.sin(np.pi / 2)))
        g.debug_set_agent_pos(0, 1, x - 2.0, y, z)       # agent 1 two units in front of agent 0, which looks along -x
        g.debug_set_agent_yaw(0, 0, c, sn)
        g.debug_set_agent_yaw(0, 1, -c, -sn)
        for mode in ("fast", "exact"):
            g.set_pixel_mode(mode); g.render()
            p = planes(d)[0].reshape(4, 2, H, W)
            centre = p[0, :, H // 2 - 6, W // 2]   # (a little below the eyes: the capsule's cylinder)
            assert (np.abs(centre - (2.0 - 0.33)) < 0.02).all(), f"{scenario} {mode}: the capsule's depth at the centre is {centre}, expected 2 - 0.33"
        g.close()


# ---- 8. refusals and detach ------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(1); g.reset()
    lib = g._lib
    buf = torch.zeros((1, 4, 24, 40), device="cuda")
    assert lib.mv_set_depth_obs(g._g, buf.data_ptr(), 5) == -1 and b"unknown format" in lib.mv_last_error()
    assert lib.mv_get_depth_obs(g._g) == 0 and lib.mv_get_depth_format(g._g) == -1
    with pytest.raises(RuntimeError, match="mv_set_depth_obs"):
        g.get_depth_observation(0, 0)
    with pytest.raises(ValueError, match="set_depth_obs"):
        g.set_depth_obs(torch.zeros((1, 4, 24, 41), device="cuda"))
    with pytest.raises(ValueError, match="set_depth_obs"):
        g.set_depth_obs(torch.zeros((1, 4, 24, 40), device="cuda", dtype=torch.float64))
    g.set_still_frames(True)
    with pytest.raises(RuntimeError, match="mv_set_depth_obs.*mv_set_still_frames"):
        g.set_depth_obs(True)
    g.set_still_frames(False)
    g.set_depth_obs(buf)
    assert lib.mv_get_depth_obs(g._g) == 1 and lib.mv_get_depth_format(g._g) == 0
    with pytest.raises(RuntimeError, match="mv_set_still_frames.*mv_set_depth_obs"):
        g.set_still_frames(True)
    ring = torch.zeros((2, 4, 24, 40, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="mv_set_output_ring.*mv_set_depth_obs"):
        g.set_output_ring(2, ring.data_ptr())
    with pytest.raises(RuntimeError, match="mv_set_render_resolution.*mv_set_depth_obs"):
        g.set_render_resolution(64, 36)
    other = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    other.seed(1); other.reset()
    import ctypes as C
    handles = (C.c_void_p * 2)(g._g.value, other._g.value)
    out = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1
    assert b"depth observations attached" in lib.mv_last_error() and b"mv_set_depth_obs" in lib.mv_last_error()
    assert lib.mv_step_many(handles, 2, 1, 1, 0, 0) == -1 and b"mv_set_depth_obs" in lib.mv_last_error()
    g.draw_hires()   # ignores the option
    g.set_depth_obs(None)
    assert lib.mv_get_depth_obs(g._g) == 0
    g.set_output_ring(2, ring.data_ptr()); g.set_output_ring(0)
    g.set_render_resolution(64, 36)
    assert lib.mv_group_create(handles, 2, C.byref(out)) == 0
    assert lib.mv_set_depth_obs(g._g, buf.data_ptr(), 0) == -1 and b"mv_group" in lib.mv_last_error()
    lib.mv_group_destroy(out)
    with pytest.raises(RuntimeError, match="mv_set_depth_obs"):
        MultiTaskGym.set_depth_obs(None)
    g.close(); other.close()


def test_detach_is_as_never_attached(hip):
    """after a detach the gym's launches and bytes are those of a gym that never attached; mv_close leaves the caller's buffer alone"""
    a, b = (MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {}) for _ in range(2))
    for g in (a, b):
        g.seed(2); g.reset()
    d = a.set_depth_obs(True)
    a.step_n(2, "multidiscrete", 4, 0); b.step_n(2, "multidiscrete", 4, 0)
    a.set_depth_obs(None)
    sentinel(d)
    ca, cb = a.debug_launch_counts(), b.debug_launch_counts()
    for g in (a, b):
        g.step_n(4, "multidiscrete", 4, 2); g.step(); g.render()
    ca2, cb2 = a.debug_launch_counts(), b.debug_launch_counts()
    assert (ca2[0] - ca[0], ca2[1] - ca[1]) == (cb2[0] - cb[0], cb2[1] - cb[1])
    assert np.array_equal(frames(a), frames(b)) and is_sentinel(planes(d)).all()
    d = a.set_depth_obs(True); a.render(); want = planes(d)
    a.close(); b.close()
    assert np.array_equal(planes(d).view(np.uint32), want.view(np.uint32))


def test_megaverse_env_surface(hip):
    """MegaverseEnv(..., depth_obs=...): planes per env and agent, the RGB observation space unchanged, the buffer re-attached around ring changes"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    with pytest.raises(ValueError, match="depth_obs"):
        MegaverseEnv("TowerBuilding", 4, 2, img_w=40, img_h=24, depth_obs="int8")
    env = MegaverseEnv("TowerBuilding", 4, 2, img_w=40, img_h=24, depth_obs="float16")
    env.reset()
    d = env.depth_obs()
    assert tuple(d.shape) == (4, 2, 24, 40) and d.dtype == torch.float16 and (planes(d) > 0).any()
    assert env.observation_space.shape == (3, 24, 40)
    env._set_output_ring(0)   # (what step_device / step_sequence do around their rings)
    assert env.env._lib.mv_get_depth_obs(env.env._g) == 1 and env.depth_obs().dtype == torch.float16
    env.close()
    plain = MegaverseEnv("TowerBuilding", 4, 1, img_w=40, img_h=24)
    with pytest.raises(RuntimeError, match="depth_obs=True"):
        plain.depth_obs()
    plain.close()
