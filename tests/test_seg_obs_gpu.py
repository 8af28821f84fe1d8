"""GPU: segmentation observations (mv_set_seg_obs).  The label planes against tests/seg_reference.py (float64 geometry and the snapshot's records, never a
kernel's output) in both formats, both pixel modes and both colour layouts, at sizes with edge tiles and an odd width; the follower behind a fast pass
against the one-trace form, byte for byte; labels beside depth; a gym with labels against a twin without; which entries are written by which calls; launch
counts -- one follower for depth + labels; refusals."""
import os

import numpy as np
import pytest
import torch

import depth_reference as dr
import oracle_lib
import pixel_reference as pr
import seg_reference as sr
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16, MegaverseGym, seg_split
from megaverse_amd.multitask import MultiTaskGym

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

K = sr.CLASSES
MATRIX = pr.MATRIX + [("Empty", 1)]
SENT8, SENT16 = 0xEE, 0xFEED   # no class is 14 < c: neither is a label


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels


def planes(t):
    """a label or depth tensor -> numpy; an int16 tensor as the uint16 words it holds"""
    torch.cuda.synchronize()
    a = t.detach().cpu().numpy().copy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def frames(g):
    return np.stack([g.get_observation(e, a) for e in range(g.num_envs) for a in range(g.num_agents_per_env)])


def sentinel(t):
    if t.dtype == torch.uint8:
        t.fill_(SENT8)
    elif t.dtype == torch.int16:
        t.fill_(int(np.uint16(SENT16).view(np.int16)))
    else:
        t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).fill_(0x7FC1 if t.dtype == torch.float16 else 0x7FC12345)


def is_sentinel(a):
    if a.dtype == np.uint8:
        return a == SENT8
    if a.dtype == np.uint16:
        return a == SENT16
    return a.view(np.uint16) == 0x7FC1 if a.dtype == np.float16 else a.view(np.uint32) == 0x7FC12345


def advance(gyms, og, n_envs, A, ticks):
    for tick in range(ticks):
        acts, masks = pr.scripted(n_envs, A, tick)
        if og is not None:
            og.set_action_masks(masks); og.step_norender()
        for g in gyms:
            g.set_actions_batched(acts); g.step_no_render()


# ---- 1. box scenes: the float64 caster and the restated draw list -------------------------------------------------------------------------------------
def judge_scene(og, gyms, env, W, H, what, n_agents=1, box=True):
    """every gym of `gyms` (one per colour layout): both formats x both pixel modes of (env, agent 0) -- equality with the float64 caster's word at the
    compared pixels (box scenes), and seg_reference.judge against the restated draw list on the whole frame"""
    snap = hip_snapshot(gyms[0], env)
    assert not diff_snapshots(og.snapshot(env), snap, n_agents), f"{what}: the twin's state differs"
    listed, interior = sr.expected(og, snap, env, 0)
    assert interior.mean() >= sr.INTERIOR_SHARE
    if box:
        m, _ = sr.world_box_interior(og, env, 0)
        want, margin, hit = sr.box_scene(snap, 0, W, H)
        assert m.any() and not (m & hit & (margin <= pr.EPS_4ULP)).any()
    for hg in gyms:
        for fmt in ("instance", "class"):
            d = hg.set_seg_obs(True, fmt)
            for mode in ("exact", "fast"):
                sentinel(d)
                hg.set_pixel_mode(mode); hg.render()
                got = planes(d)[0].reshape(hg.num_envs, n_agents, H, W)[env, 0]
                tag = f"{what} {fmt} {mode} layout {hg._seg_layout}"
                assert not is_sentinel(got).any(), f"{tag}: pixels left unwritten"
                if box:
                    w = want if fmt == "instance" else want >> 12
                    bad = m & (got != w)
                    assert not bad.any(), f"{tag}: {int(bad.sum())} compared pixels differ from the float64 caster, first at {np.argwhere(bad)[0].tolist()}"
                sr.judge(got, listed, interior, tag, class_only=fmt == "class")
                assert np.array_equal(got.astype(np.uint16), hg.get_seg_observation(env, 0)), f"{tag}: the read-back of one plane differs"
            hg.set_seg_obs(None)
    return listed


def scene_gyms(scenario, W, H, n_envs, n_agents, seed):
    og = oracle_lib.OracleGym(scenario, W, H, n_envs, n_agents, 1)
    gyms = []
    for layout in ("rgba", "chw"):
        g = MegaverseGym(scenario, W, H, n_envs, n_agents, 1, False, {})
        g.set_obs_layout(layout); g._seg_layout = layout
        gyms.append(g)
    for g in [og] + gyms:
        g.seed(seed); g.reset()
    return og, gyms


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_box_scenes_tower(hip, W, H):
    og, gyms = scene_gyms("TowerBuilding", W, H, dr.TOWER_ENVS, 1, dr.TOWER_SEED)
    e = dr.pose_tower_wall(og, [og] + gyms)
    listed = judge_scene(og, gyms, e, W, H, f"TowerBuilding wall {W}x{H}")
    assert {K["FLOOR"], K["STRUCTURE"]} <= set((listed >> 12).ravel().tolist())
    e, _ = dr.pose_tower_box(og, [og] + gyms)
    listed = judge_scene(og, gyms, e, W, H, f"TowerBuilding box {W}x{H}")
    assert K["MOVABLE"] in set((listed >> 12).ravel().tolist())
    for g in [og] + gyms:
        g.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
@pytest.mark.parametrize("pose", list(dr.EMPTY_POSES))
def test_box_scenes_empty(hip, pose, W, H):
    og, gyms = scene_gyms("Empty", W, H, dr.EMPTY_ENVS, 1, dr.EMPTY_SEED)
    e = dr.pose_empty([og] + gyms, pose)
    judge_scene(og, gyms, e, W, H, f"Empty {pose} {W}x{H}")
    for g in [og] + gyms:
        g.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_box_scenes_obstacles(hip, W, H):
    """ObstaclesHard with a lava slab and the exit pad in view"""
    og, gyms = scene_gyms("ObstaclesHard", W, H, sr.OBST_ENVS, 1, sr.OBST_SEED)
    e = sr.pose_obstacles(og, [og] + gyms)
    listed = judge_scene(og, gyms, e, W, H, f"ObstaclesHard {W}x{H}")
    assert {K["EXIT"], K["LAVA"]} <= set((listed >> 12).ravel().tolist())
    for g in [og] + gyms:
        g.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_ball_football(hip, W, H):
    """(ii) BALL, instance 0, wherever the float64 sphere is hit inside 0.8 of its projected radius -- and the whole frame against the draw list"""
    og, gyms = scene_gyms("Football", W, H, 4, 2, dr.EMPTY_SEED)
    e, centre, radius = dr.pose_football([og] + gyms)
    a = hip_snapshot(gyms[0], e)["agents"][0]
    eye, C = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, share = dr.cast_sphere(eye, C, W, H, centre, radius)
    inside = np.isfinite(t) & (share <= 0.8)
    assert inside.sum() >= 4
    judge_scene(og, gyms, e, W, H, f"Football {W}x{H}", n_agents=2, box=False)
    for hg in gyms:
        d = hg.set_seg_obs(True, "instance")
        for mode in ("exact", "fast"):
            hg.set_pixel_mode(mode); hg.render()
            got = planes(d)[0].reshape(4, 2, H, W)[e, 0]
            assert (got[inside] == sr.word(K["BALL"], 0)).all(), f"Football {W}x{H} {mode}: the ball's pixels are not BALL / 0"
    for g in [og] + gyms:
        g.close()


# ---- 2. every scenario: the restated draw list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,A", pr.MATRIX)
def test_other_scenarios_against_the_draw_list(hip, scenario, A):
    """one seeded, scripted state per scenario at 128 x 128: every frame of which 80 % is interior (chosen on the oracle) against the restated draw list,
    in both pixel modes"""
    W, H, N = 128, 128, pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    hg = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    for g in (og, hg):
        g.seed(pr.SEED); g.reset()
    advance([hg], og, N, A, 12)
    for e in range(N):
        assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
    chosen = sr.compared_frames(og, N, A)
    assert len(chosen) >= N * A // 2
    assert sr.MATRIX_CLASSES[scenario] <= sr.classes_in(chosen), f"{scenario}: the compared frames no longer show {sorted(sr.MATRIX_CLASSES[scenario] - sr.classes_in(chosen))}"
    d = hg.set_seg_obs(True, "instance")
    for mode in ("exact", "fast"):
        sentinel(d); hg.set_pixel_mode(mode); hg.render()
        got = planes(d)[0].reshape(N, A, H, W)
        assert not is_sentinel(got).any()
        for e, a, want, interior in chosen:
            sr.judge(got[e, a], want, interior, f"{scenario} env {e} agent {a} {mode}")
    og.close(); hg.close()


def test_two_agents_face_to_face_with_a_carried_box(hip):
    """TowerBuilding, two agents facing each other, a box in agent 1's hands: from agent 0 AGENT / 1, CARRIED / 0 and a HUD row; from agent 1 AGENT / 0"""
    W, H = 128, 128
    og = oracle_lib.OracleGym("TowerBuilding", W, H, 4, 2, 1)
    hg = MegaverseGym("TowerBuilding", W, H, 4, 2, 1, False, {})
    for g in (og, hg):
        g.seed(3); g.reset()
    sr.pose_face_to_face([og, hg], og.snapshot(0), carried=0)
    snap = hip_snapshot(hg, 0)
    assert not diff_snapshots(og.snapshot(0), snap, 2)
    d = hg.set_seg_obs(True, "instance")
    for mode in ("exact", "fast"):
        hg.set_pixel_mode(mode); hg.render()
        got = planes(d)[0].reshape(4, 2, H, W)[0]
        for a in (0, 1):
            want, interior = sr.expected(og, snap, 0, a)
            assert interior.mean() >= sr.INTERIOR_SHARE
            sr.judge(got[a], want, interior, f"face to face, agent {a}, {mode}")
        seen0, seen1 = set(got[0].ravel().tolist()), set(got[1].ravel().tolist())
        assert {sr.word(K["AGENT"], 1), sr.word(K["CARRIED"], 0), sr.word(K["HUD"], 0)} <= seen0 and sr.word(K["AGENT"], 0) not in seen0
        assert sr.word(K["AGENT"], 0) in seen1 and sr.word(K["AGENT"], 1) not in seen1
        assert got[0][H // 2 - 12, W // 2] == sr.word(K["AGENT"], 1)   # (a little below the eyes: the capsule's cylinder)
        cls, inst = seg_split(got[0])
        assert cls[H // 2 - 12, W // 2] == K["AGENT"] and inst[H // 2 - 12, W // 2] == 1
    og.close(); hg.close()


def test_rearrange_carried_item_targets_and_movables(hip):
    """Rearrange, three agents: agent 1 picks item 0 (a capsule) up through INTERACT ticks stepped on both gyms.  From agent 0: CARRIED / 0 -- a scaled shape
    in agent 1's camera frame -- AGENT / 1 and the MOVABLE items left on the right pedestal; from agent 2: the TARGET items of the left pedestal.  Both pixel
    modes, both formats, against the restated draw list"""
    W, H, N, A = 128, 128, sr.REARRANGE_ENVS, sr.REARRANGE_AGENTS
    og = oracle_lib.OracleGym("Rearrange", W, H, N, A, 1)
    hg = MegaverseGym("Rearrange", W, H, N, A, 1, False, {})
    for g in (og, hg):
        g.seed(sr.REARRANGE_SEED); g.reset()
    e = sr.pose_rearrange_carried(og, [og, hg])
    snap = hip_snapshot(hg, e)
    assert not diff_snapshots(og.snapshot(e), snap, A), "the twin's state differs"
    want = sr.rearrange_scene_expected(og, snap, e)
    for fmt in ("instance", "class"):
        d = hg.set_seg_obs(True, fmt)
        for mode in ("exact", "fast"):
            sentinel(d); hg.set_pixel_mode(mode); hg.render()
            got = planes(d)[0].reshape(N, A, H, W)[e]
            assert not is_sentinel(got).any()
            for a in range(A):
                sr.judge(got[a], want[a][0], want[a][1], f"Rearrange scene, agent {a}, {fmt} {mode}", class_only=fmt == "class")
            if fmt == "instance":
                seen0, seen2 = set(got[0][want[0][1]].tolist()), set(got[2][want[2][1]].tolist())
                assert {sr.word(K["CARRIED"], 0), sr.word(K["AGENT"], 1), sr.word(K["MOVABLE"], 1), sr.word(K["MOVABLE"], 2)} <= seen0
                assert {sr.word(K["TARGET"], 0), sr.word(K["TARGET"], 1), sr.word(K["TARGET"], 2)} <= seen2
        hg.set_seg_obs(None)
    og.close(); hg.close()


@pytest.mark.parametrize("fmt", ["class", "instance"])
def test_buffers_that_do_not_start_at_a_dword(hip, fmt):
    """40 x 24 (W a multiple of 4): a class buffer that starts one byte, an instance buffer that starts two bytes behind a dword boundary takes the
    byte / two-byte stores instead of the combined dwords -- the same planes as an aligned buffer's, in both pixel modes, with nothing written outside"""
    W, H, N = 40, 24, 4
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    g.seed(7); g.reset()
    want = {}
    d = g.set_seg_obs(True, fmt)
    for mode in ("exact", "fast"):
        g.set_pixel_mode(mode); g.render(); want[mode] = planes(d)[0]
    g.set_seg_obs(None)
    n = N * H * W
    raw = torch.zeros(n + 8, dtype=d.dtype, device="cuda")
    view = raw[1:1 + n].view(1, N, H, W)
    assert view.data_ptr() % 4 == (1 if fmt == "class" else 2) and view.is_contiguous()
    g.set_seg_obs(view, fmt)
    for mode in ("exact", "fast"):
        sentinel(raw); g.set_pixel_mode(mode); g.render()
        got = planes(raw)
        assert np.array_equal(got[1:1 + n].reshape(N, H, W), want[mode]), f"{fmt} {mode}: the planes of a buffer off a dword boundary differ"
        assert is_sentinel(got[:1]).all() and is_sentinel(got[1 + n:]).all(), f"{fmt} {mode}: bytes outside the buffer were written"
    g.close()


def test_hud_row_at_the_hand_derived_columns(hip):
    """the viewer's own time bar at 128 x 128: HUD / 0 at the pixels derived by hand from the bar's box (seg_reference.hud_pixels), in neither format and
    neither pixel mode anywhere that is surely outside them"""
    W, H = 128, 128
    hg = MegaverseGym("TowerBuilding", W, H, 4, 1, 1, False, {})
    hg.seed(3); hg.reset()
    for fmt in ("instance", "class"):
        d = hg.set_seg_obs(True, fmt)
        for mode in ("exact", "fast"):
            sentinel(d); hg.set_pixel_mode(mode); hg.render()
            got = planes(d)[0]
            for e in range(4):
                inside, outside = sr.hud_pixels(float(hip_snapshot(hg, e)["bar_half_width"]), W, H)
                assert inside.sum() >= 8
                hud = got[e] == (sr.word(K["HUD"], 0) if fmt == "instance" else K["HUD"])
                assert hud[inside].all() and not hud[outside].any(), f"env {e} {fmt} {mode}: the time bar is not where its box puts it"
        hg.set_seg_obs(None)
    hg.close()


# ---- 3. bit-equality properties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", pr.SIZES + [(41, 23)])
@pytest.mark.parametrize("scenario,A", MATRIX)
def test_bit_equalities(hip, scenario, A, W, H):
    N = pr.N_ENVS
    hg, twin = (MegaverseGym(scenario, W, H, N, A, 1, False, {}) for _ in range(2))
    for g in (hg, twin):
        g.seed(pr.SEED); g.reset()
    advance([hg, twin], None, N, A, 12)
    s16 = hg.set_seg_obs(True, "instance")
    td = twin.set_depth_obs(True)
    # exact mode: one trace; the colours are the twin's
    sentinel(s16)
    for g in (hg, twin):
        g.set_pixel_mode("exact"); g.render()
    exact, depth_alone = planes(s16)[0], planes(td)[0]
    assert not is_sentinel(exact).any() and ((exact >> 12) < 15).all()
    assert np.array_equal(frames(hg), frames(twin)), f"{scenario}: exact mode with labels attached differs from a gym without"
    assert np.array_equal(exact == 0, depth_alone == 0), f"{scenario}: the label is not 0 exactly where the depth is 0"
    # fast mode: the follower's planes are the one-trace form's bytes
    sentinel(s16)
    for g in (hg, twin):
        g.set_pixel_mode("fast"); g.render()
    assert np.array_equal(planes(s16)[0], exact), f"{scenario}: the follower's labels differ from the exact pass's"
    assert np.array_equal(frames(hg), frames(twin)), f"{scenario}: fast mode with labels attached differs from a gym without"
    assert np.array_equal(planes(td)[0].view(np.uint32), depth_alone.view(np.uint32))
    # labels with depth attached, depth with labels attached: both modes, the same bytes as alone
    hd = hg.set_depth_obs(True)
    for mode in ("fast", "exact"):
        sentinel(s16); sentinel(hd)
        for g in (hg, twin):
            g.set_pixel_mode(mode); g.render()
        assert np.array_equal(planes(s16)[0], exact), f"{scenario} {mode}: labels with depth attached differ from labels alone"
        assert np.array_equal(planes(hd)[0].view(np.uint32), depth_alone.view(np.uint32)), f"{scenario} {mode}: depth with labels attached differs from depth alone"
        assert np.array_equal(frames(hg), frames(twin)), f"{scenario} {mode}: the colours with both attached differ from a gym with depth alone"
    # the U8 plane is the U16's class nibble, with depth attached and without, in both modes
    hg.set_seg_obs(None)
    s8 = hg.set_seg_obs(True, "class")
    assert hg._lib.mv_get_seg_format(hg._g) == MV_SEG_CLASS_U8 and s8.dtype == torch.uint8
    for with_depth in (True, False):
        if not with_depth:
            hg.set_depth_obs(None)
        for mode in ("fast", "exact"):
            sentinel(s8); hg.set_pixel_mode(mode); hg.render()
            assert np.array_equal(planes(s8)[0], (exact >> 12).astype(np.uint8)), f"{scenario} {mode}: the class plane is not the instance plane's nibble"
    assert np.array_equal(hg.get_seg_observation(N - 1, A - 1), (exact >> 12).reshape(N, A, H, W)[N - 1, A - 1])
    for g in (hg, twin):
        g.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_a_twin_without_labels_steps_alike(hip, mode):
    """RGB frames, rewards, dones and state of a gym with labels (and depth) attached against a twin without, over stepped ticks"""
    N, A, W, H = 4, 2, 40, 24
    hg, twin = (MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {}) for _ in range(2))
    for g in (hg, twin):
        g.set_pixel_mode(mode); g.seed(11); g.reset()
    hg.set_seg_obs(True, "instance"); hg.set_depth_obs(True, "float16")
    for tick in range(6):
        acts, _ = pr.scripted(N, A, tick)
        for g in (hg, twin):
            g.set_actions_batched(acts); g.step()
        assert np.array_equal(frames(hg), frames(twin))
        assert np.array_equal(hg.get_rewards_array().view(np.uint32), twin.get_rewards_array().view(np.uint32)) and np.array_equal(hg.get_dones(), twin.get_dones())
    for g in (hg, twin):
        g.step_n(5, "multidiscrete", 4, 6)
    assert np.array_equal(frames(hg), frames(twin))
    for e in range(N):
        assert not diff_snapshots(hip_snapshot(hg, e), hip_snapshot(twin, e), A)
    hg.close(); twin.close()


# ---- 4. where it is written, what it launches ------------------------------------------------------------------------------------------------------------
def ring_gym(fmt="instance", mode="fast", with_depth=False, N=4, A=1, W=40, H=24, count=4):
    g = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
    g.set_pixel_mode(mode); g.seed(7); g.reset()
    obs = torch.zeros((count, N * A, H, W, 4), dtype=torch.uint8, device="cuda")
    g.set_output_ring(count, obs.data_ptr())
    d = g.set_seg_obs(True, fmt)
    dd = g.set_depth_obs(True) if with_depth else None
    assert tuple(d.shape) == (count, N * A, H, W) and g._lib.mv_get_seg_obs(g._g) == count
    return g, obs, d, dd


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_step_n_fills_the_ring(hip, mode, with_depth):
    """step_n(4) into a ring of 4: every entry is mv_render's plane of a twin stepped tick by tick; ONE extra pass-side launch per drawn tick in fast mode --
    with labels alone and with depth + labels alike"""
    g, obs, d, dd = ring_gym(mode=mode, with_depth=with_depth)
    twin = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    twin.set_pixel_mode(mode); twin.seed(7); twin.reset()
    td = twin.set_seg_obs(True, "instance")
    plain = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})   # nothing attached: the launch counts to compare with
    plain.set_pixel_mode(mode); plain.seed(7); plain.reset()
    pobs = torch.zeros_like(obs); plain.set_output_ring(4, pobs.data_ptr())
    sentinel(d)
    if dd is not None:
        sentinel(dd)
    c0, p0 = g.debug_launch_counts(), plain.debug_launch_counts()
    g.step_n(4, "multidiscrete", 9, 0); plain.step_n(4, "multidiscrete", 9, 0)
    c1, p1 = g.debug_launch_counts(), plain.debug_launch_counts()
    assert c1[0] - c0[0] == p1[0] - p0[0]
    assert (c1[1] - c0[1]) - (p1[1] - p0[1]) == (4 if mode == "fast" else 0), "one follower per drawn tick, whatever is attached"
    got = planes(d)
    assert not is_sentinel(got).any() and (dd is None or not is_sentinel(planes(dd)).any())
    assert np.array_equal(planes(obs), planes(pobs)), "the colours differ from those of a gym without labels"
    for j in range(4):
        twin.step_n(1, "multidiscrete", 9, j, render="none")
        twin.render()
        assert np.array_equal(got[j], planes(td)[0]), f"entry {j} is not the plane of tick {j}"
    # one drawn tick: one launch more than the plain gym's
    c0, p0 = g.debug_launch_counts(), plain.debug_launch_counts()
    g.step(); plain.step()
    c1, p1 = g.debug_launch_counts(), plain.debug_launch_counts()
    assert (c1[1] - c0[1]) - (p1[1] - p0[1]) == (1 if mode == "fast" else 0)
    # render = 'none' leaves every byte; 'last' and a macro step write the one entry
    sentinel(d); g.step_n(4, "multidiscrete", 9, 5, render="none")
    assert is_sentinel(planes(d)).all()
    g.step_n(3, "multidiscrete", 9, 9, render="last")    # ticks 9, 10, 11 of the ring: entry 11 % 4 == 3
    got = planes(d)
    assert is_sentinel(got[:3]).all() and not is_sentinel(got[3]).any()
    sentinel(d); g.macro_step(3, np.zeros((4, 6), np.int32), render="last")
    got = planes(d)
    assert not is_sentinel(got[0]).any() and is_sentinel(got[1:]).all()
    sentinel(d); g.macro_step(3, np.zeros((4, 6), np.int32), render="none"); g.step_no_render()
    assert is_sentinel(planes(d)).all()
    for x in (g, twin, plain):
        x.close()


@pytest.mark.parametrize("fmt", ["class", "instance"])
def test_masks_resets_and_single_steps(hip, fmt):
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(7); g.reset()
    d = g.set_seg_obs(True, fmt)
    assert tuple(d.shape) == (1, 4, 24, 40)
    sentinel(d); g.step()
    assert not is_sentinel(planes(d)).any()
    assert tuple(g.seg_obs().shape) == (4, 24, 40) and g.seg_obs_ring() is d
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
    assert np.array_equal(planes(d), want)
    g.close()


# ---- 5. refusals and detach ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(1); g.reset()
    lib = g._lib
    buf = torch.zeros((1, 4, 24, 40), device="cuda", dtype=torch.int16)
    assert lib.mv_set_seg_obs(g._g, buf.data_ptr(), 5) == -1 and b"unknown format" in lib.mv_last_error()
    assert lib.mv_set_seg_obs(g._g, buf.data_ptr() + 1, MV_SEG_INSTANCE_U16) == -1 and b"2-byte aligned" in lib.mv_last_error()
    assert lib.mv_get_seg_obs(g._g) == 0 and lib.mv_get_seg_format(g._g) == -1
    with pytest.raises(RuntimeError, match="mv_set_seg_obs"):
        g.get_seg_observation(0, 0)
    with pytest.raises(ValueError, match="set_seg_obs"):
        g.set_seg_obs(torch.zeros((1, 4, 24, 41), device="cuda", dtype=torch.uint8))
    with pytest.raises(ValueError, match="set_seg_obs"):
        g.set_seg_obs(buf, "class")            # an int16 tensor is no class plane
    with pytest.raises(ValueError, match="set_seg_obs"):
        g.set_seg_obs(True, "depth")
    g.set_still_frames(True)
    with pytest.raises(RuntimeError, match="mv_set_seg_obs.*mv_set_still_frames"):
        g.set_seg_obs(True)
    g.set_still_frames(False)
    g.set_seg_obs(buf, "instance")
    assert lib.mv_get_seg_obs(g._g) == 1 and lib.mv_get_seg_format(g._g) == MV_SEG_INSTANCE_U16
    with pytest.raises(RuntimeError, match="mv_set_still_frames.*mv_set_seg_obs"):
        g.set_still_frames(True)
    ring = torch.zeros((2, 4, 24, 40, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="mv_set_output_ring.*mv_set_seg_obs"):
        g.set_output_ring(2, ring.data_ptr())
    with pytest.raises(RuntimeError, match="mv_set_render_resolution.*mv_set_seg_obs"):
        g.set_render_resolution(64, 36)
    other = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    other.seed(1); other.reset()
    import ctypes as C
    handles = (C.c_void_p * 2)(g._g.value, other._g.value)
    out = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1
    assert b"segmentation observations attached" in lib.mv_last_error() and b"mv_set_seg_obs" in lib.mv_last_error()
    assert lib.mv_step_many(handles, 2, 1, 1, 0, 0) == -1 and b"mv_set_seg_obs" in lib.mv_last_error()
    g.draw_hires()   # ignores the option
    # depth and labels attach and detach independently, in either order
    dd = g.set_depth_obs(True); g.set_seg_obs(None)
    assert lib.mv_get_seg_obs(g._g) == 0 and lib.mv_get_depth_obs(g._g) == 1
    sentinel(dd); sentinel(buf); g.render()
    assert not is_sentinel(planes(dd)).any() and is_sentinel(planes(buf)).all()
    g.set_seg_obs(buf, "instance"); g.set_depth_obs(None)
    sentinel(dd); sentinel(buf); g.render()
    assert is_sentinel(planes(dd)).all() and not is_sentinel(planes(buf)).any()
    g.set_seg_obs(None)
    g.set_output_ring(2, ring.data_ptr()); g.set_output_ring(0)
    g.set_render_resolution(64, 36)
    assert lib.mv_group_create(handles, 2, C.byref(out)) == 0
    assert lib.mv_set_seg_obs(g._g, buf.data_ptr(), 0) == -1 and b"mv_group" in lib.mv_last_error()
    lib.mv_group_destroy(out)
    with pytest.raises(RuntimeError, match="mv_set_seg_obs"):
        MultiTaskGym.set_seg_obs(None)
    g.close(); other.close()


def test_detach_is_as_never_attached(hip):
    """after a detach the gym's launches and bytes are those of a gym that never attached; mv_close leaves the caller's buffer alone"""
    a, b = (MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {}) for _ in range(2))
    for g in (a, b):
        g.seed(2); g.reset()
    d = a.set_seg_obs(True, "class")
    a.step_n(2, "multidiscrete", 4, 0); b.step_n(2, "multidiscrete", 4, 0)
    a.set_seg_obs(None)
    sentinel(d)
    ca, cb = a.debug_launch_counts(), b.debug_launch_counts()
    for g in (a, b):
        g.step_n(4, "multidiscrete", 4, 2); g.step(); g.render()
    ca2, cb2 = a.debug_launch_counts(), b.debug_launch_counts()
    assert (ca2[0] - ca[0], ca2[1] - ca[1]) == (cb2[0] - cb[0], cb2[1] - cb[1])
    assert np.array_equal(frames(a), frames(b)) and is_sentinel(planes(d)).all()
    d = a.set_seg_obs(True, "class"); a.render(); want = planes(d)
    a.close(); b.close()
    assert np.array_equal(planes(d), want)


def test_megaverse_env_surface(hip):
    """MegaverseEnv(..., seg_obs=...): planes per env and agent, the RGB observation space unchanged, the buffer re-attached around ring changes"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    with pytest.raises(ValueError, match="seg_obs"):
        MegaverseEnv("TowerBuilding", 4, 2, img_w=40, img_h=24, seg_obs="depth")
    env = MegaverseEnv("TowerBuilding", 4, 2, img_w=40, img_h=24, seg_obs="instance", depth_obs=True)
    env.reset()
    d = env.seg_obs()
    assert tuple(d.shape) == (4, 2, 24, 40) and d.dtype == torch.int16
    cls, inst = seg_split(d)
    assert cls.dtype == torch.uint8 and int(cls.max()) <= 14 and (cls == K["FLOOR"]).any()
    assert ((cls == 0) == (env.depth_obs() == 0)).all()
    assert env.observation_space.shape == (3, 24, 40)
    env._set_output_ring(0)   # (what step_device / step_sequence do around their rings)
    assert env.env._lib.mv_get_seg_obs(env.env._g) == 1 and env.env._lib.mv_get_seg_format(env.env._g) == MV_SEG_INSTANCE_U16
    env.close()
    env = MegaverseEnv("TowerBuilding", 4, 1, img_w=40, img_h=24, seg_obs=True)
    env.reset()
    assert env.seg_obs().dtype == torch.uint8 and (env.seg_obs() == K["FLOOR"]).any()
    env.close()
    plain = MegaverseEnv("TowerBuilding", 4, 1, img_w=40, img_h=24)
    with pytest.raises(RuntimeError, match="seg_obs=True"):
        plain.seg_obs()
    plain.close()
