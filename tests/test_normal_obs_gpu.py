"""GPU: normal observations (mv_set_normal_obs).  Known answers against the float64 closed forms of tests/normal_reference.py (never a kernel's output) in both
formats and pixel modes at sizes with edge tiles and an odd width; over the scenario matrix the zero sets, unit length, orientation, the follower against the
one-trace planes and every attach subset against the planes attached alone, byte for byte; planar consistency with the depth plane; the two formats against
each other; which entries are written by which calls and what they cost in launches; resets inside a batched call; refusals and the Python surface."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import depth_reference as dr
import normal_reference as nr
import oracle_lib
import pixel_reference as pr
import seg_reference as sr
from canonical_frames import TAN, TAN_Y
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MV_NORMAL_F16, MV_NORMAL_SNORM8, MegaverseGym
from megaverse_amd.multitask import MultiTaskGym

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MATRIX = pr.MATRIX + [("Empty", 1)]
FORMATS = ["float16", "int8"]
STREAMS = ("depth", "seg", "normal")
SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(STREAMS, r)]   # the seven non-empty sets
# | |n| - 1 | and n . dc, derived.  Each stored component is off by at most the format term, so the length by at most sqrt(3) of it; the fp32 vector itself is
# unit within NORM_FP32 = 2^-16: a box's is a row of the camera matrix (a few 2^-24), a curved hit's is (P - c) / r with P = o + t d, whose length moves by
# (d . n) dt / r to first order -- the measured normal_reference.SPHERE_ABS = 1.35e-5 is that very quantity -- and, at grazing pixels where d . n vanishes and
# dt grows to ~sqrt(2^-24) |B|, by (dt |d|)^2 / (2 r^2) < 4e-6.  A ray direction is at most sqrt(1 + tan^2 + tan_y^2) long.
NORM_FP32 = 2.0 ** -16
DC_MAX = float(np.sqrt(1 + TAN ** 2 + TAN_Y ** 2))


def norm_bound(fmt):
    return np.sqrt(3.0) * nr.FORMAT_ABS[fmt] + NORM_FP32


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels


def planes(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def raw(t):
    """a tensor's bytes"""
    return planes(t.view(torch.uint8) if t.dtype != torch.uint8 else t)


def frames(g):
    return np.stack([g.get_observation(e, a) for e in range(g.num_envs) for a in range(g.num_agents_per_env)])


def sentinel(t):
    t.view(torch.uint8).fill_(0xA5)   # (no format stores this byte everywhere: w is 0, 1.0 or 127)


def is_sentinel(a):
    return a.view(np.uint8) == 0xA5


def attach(g, name, fmt=None):
    if name == "depth":
        return g.set_depth_obs(True)
    if name == "seg":
        return g.set_seg_obs(True, "instance")
    return g.set_normal_obs(True, fmt or "float16")


def detach_all(g):
    g.set_depth_obs(None); g.set_seg_obs(None); g.set_normal_obs(None)


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------------------
def judge_known(hg, env, agent, A, want, mask, fp_abs, background, what):
    """both formats and both pixel modes of (env, agent)'s plane against float64 normals at mask; four zeros at background"""
    for fmt in FORMATS:
        hg.set_normal_obs(None)
        t = hg.set_normal_obs(True, fmt)
        for mode in ("exact", "fast"):
            sentinel(t)
            hg.set_pixel_mode(mode); hg.render()
            got = planes(t)[0, env * A + agent]
            ok, share = nr.judge(got, want, mask, fp_abs, background)
            print(f"{what} {fmt} {mode}: {int(mask.sum())} pixels, largest error {share:.3f} of the bound; {0 if background is None else int(background.sum())} background pixels")
            assert ok, f"{what} {fmt} {mode}: outside the bound ({share:.2f} of it), w != 1 or background not zero"
            wide = got.astype(np.float32) / np.float32(127) if fmt == "int8" else got.astype(np.float32)
            assert np.array_equal(wide, hg.get_normal_observation(env, agent))   # (the read-back of one plane: b / 127.0f, or the half widened)
    hg.set_normal_obs(None)


def box_known(og, hg, env, W, H, what):
    assert not diff_snapshots(og.snapshot(env), hip_snapshot(hg, env), 1), f"{what}: the twin's state differs"
    snap = hip_snapshot(hg, env)
    _, prim = og.render_f64(env, 0)
    m, bg = dr.interior_mask(prim, og.prim_table(env, 0), dr.is_world_box), dr.background_mask(prim)
    t, box, axis, dwk, lo, hi = dr.expected_boxes(snap, 0, W, H)
    a = snap["agents"][0]
    _, Cm = dr.camera64(a["pos"], a["basis"], a["pitch"])
    judge_known(hg, env, 0, 1, nr.box_normals(Cm, axis, dwk), m, nr.BOX_ABS, bg, what)


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_known_answers_tower(hip, W, H):
    """(a) on the wall seen square-on, the floor, and a movable box's faces"""
    og = oracle_lib.OracleGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1)
    hg = MegaverseGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1, False, {})
    for g in (og, hg):
        g.seed(dr.TOWER_SEED); g.reset()
    e = dr.pose_tower_wall(og, [og, hg])
    box_known(og, hg, e, W, H, f"TowerBuilding wall {W}x{H}")
    e, _ = dr.pose_tower_box(og, [og, hg])
    box_known(og, hg, e, W, H, f"TowerBuilding box {W}x{H}")
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
@pytest.mark.parametrize("pose", list(dr.EMPTY_POSES))
def test_known_answers_empty(hip, pose, W, H):
    """(a) at pitch 0 and at two pitched cameras: the rows of a camera matrix that is no permutation"""
    og = oracle_lib.OracleGym("Empty", W, H, dr.EMPTY_ENVS, 1, 1)
    hg = MegaverseGym("Empty", W, H, dr.EMPTY_ENVS, 1, 1, False, {})
    for g in (og, hg):
        g.seed(dr.EMPTY_SEED); g.reset()
    e = dr.pose_empty([og, hg], pose)
    box_known(og, hg, e, W, H, f"Empty {pose} {W}x{H}")
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_known_answers_football(hip, W, H):
    """(b) the ball, a scaled sphere, inside 0.8 of its projected radius"""
    og = oracle_lib.OracleGym("Football", W, H, 4, 2, 1)
    hg = MegaverseGym("Football", W, H, 4, 2, 1, False, {})
    for g in (og, hg):
        g.seed(dr.EMPTY_SEED); g.reset()
    e, centre, radius = dr.pose_football([og, hg])
    assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), 2)
    a = hip_snapshot(hg, e)["agents"][0]
    eye, Cm = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, share = dr.cast_sphere(eye, Cm, W, H, centre, radius)
    inside = np.isfinite(t) & (share <= 0.8)
    assert inside.sum() >= 4
    _, prim = og.render_f64(e, 0)
    judge_known(hg, e, 0, 2, nr.sphere_normals(eye, Cm, W, H, centre, radius, t), inside, nr.SPHERE_ABS, dr.background_mask(prim), f"Football {W}x{H}")
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_known_answers_capsule(hip, W, H):
    """(c) the other agent's capsule face to face, on its cylinder part"""
    og = oracle_lib.OracleGym("TowerBuilding", W, H, 4, 2, 1)
    hg = MegaverseGym("TowerBuilding", W, H, 4, 2, 1, False, {})
    for g in (og, hg):
        g.seed(3); g.reset()
    sr.pose_face_to_face([og, hg], og.snapshot(0))
    assert not diff_snapshots(og.snapshot(0), hip_snapshot(hg, 0), 2)
    snap = hip_snapshot(hg, 0)
    _, prim = og.render_f64(0, 0)
    a = snap["agents"][0]
    eye, Cm = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, want = nr.cast_capsule_cylinder(eye, Cm, W, H, nr.capsule_centre(snap["agents"][1]["pos"]))
    m = dr.interior_mask(prim, og.prim_table(0, 0), lambda kind, frame: kind == nr.PRIM_CAPSULE) & np.isfinite(t)
    assert m.mean() >= 0.02   # (tests/test_normal_obs.py: CAPSULE_SHARE, found on the reference alone)
    judge_known(hg, 0, 0, 2, want, m, nr.CAPSULE_ABS, dr.background_mask(prim), f"capsule {W}x{H}")
    og.close(); hg.close()


# ---- 2., 3., 4. the matrix ---------------------------------------------------------------------------------------------------------------------------
def advance(gyms, og, n_envs, A, ticks):
    for tick in range(ticks):
        acts, masks = pr.scripted(n_envs, A, tick)
        if og is not None:
            og.set_action_masks(masks); og.step_norender()
        for g in gyms:
            g.set_actions_batched(acts); g.step_no_render()


def alone(g, name, fmt=None):
    """the bytes of one stream's planes attached alone, drawn in exact pixel mode (the one-trace form)"""
    detach_all(g)
    t = attach(g, name, fmt)
    sentinel(t); g.set_pixel_mode("exact"); g.render()
    out = raw(t)[0]
    assert not is_sentinel(out).all()
    return out


@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", MATRIX)
def test_matrix(hip, scenario, A, W, H):
    N = pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    hg, twin = (MegaverseGym(scenario, W, H, N, A, 1, False, {}) for _ in range(2))
    for g in (og, hg, twin):
        g.seed(pr.SEED); g.reset()
    advance([hg, twin], og, N, A, 12)
    want = {name: alone(hg, name) for name in STREAMS}
    s8 = alone(hg, "normal", "int8")
    depth = want["depth"].view(np.float32).reshape(N * A, H, W)
    label = want["seg"].view(np.uint16).reshape(N * A, H, W)
    f16 = want["normal"].view(np.float16).reshape(N * A, H, W, 4)
    s8 = s8.view(np.int8).reshape(N * A, H, W, 4)
    dc = dr.rays64(W, H)
    # the zero set is the depth's and the labels', exactly; w elsewhere; unit length; facing the viewer
    for got, fmt in ((f16, MV_NORMAL_F16), (s8, MV_NORMAL_SNORM8)):
        zero = ~got.view(np.uint8).reshape(N * A, H, W, -1).any(-1)
        assert np.array_equal(zero, depth == 0) and np.array_equal(zero, label == 0), f"{scenario}: the all-zero set is not the depth's and the labels' zero set"
        xyz, w = nr.widen(got)
        assert (w[~zero] == 1.0).all() and (~zero).any()
        length = np.abs(np.linalg.norm(xyz[~zero], axis=-1) - 1)
        facing = (xyz * dc[None]).sum(-1)[~zero]
        print(f"{scenario} {W}x{H} format {fmt}: | |n| - 1 | up to {length.max():.2e} (bound {norm_bound(fmt):.2e}); n . dc up to {facing.max():.2e} (slack {DC_MAX * norm_bound(fmt):.2e})")
        assert (length <= norm_bound(fmt)).all(), f"{scenario}: a normal is not unit"
        assert (facing <= DC_MAX * norm_bound(fmt)).all(), f"{scenario}: a normal faces away from the viewer"
    # 4. the two formats against each other
    gap = np.abs(127.0 * f16[..., :3].astype(np.float64) - s8[..., :3].astype(np.float64))
    assert (gap <= 0.5 + 127 * 2.0 ** -12).all(), f"{scenario}: SNORM8 against F16 off by {gap.max():.3f}"
    # every attach subset, in both pixel modes: each plane it includes holds the bytes it has when attached alone (fast: the follower's; exact: one trace)
    for subset in SUBSETS:
        detach_all(hg)
        t = {name: attach(hg, name) for name in subset}
        for mode in ("fast", "exact"):
            for name in subset:
                sentinel(t[name])
            hg.set_pixel_mode(mode); twin.set_pixel_mode(mode)
            hg.render(); twin.render()
            for name in subset:
                assert np.array_equal(raw(t[name])[0], want[name]), f"{scenario} {mode} {subset}: the {name} planes differ from those attached alone"
            assert np.array_equal(frames(hg), frames(twin)), f"{scenario} {mode} {subset}: the colours differ from a gym with nothing attached"
    # 3. planar consistency on interior box pixels: the normal against the cross product of the neighbours' positions from the float32 depth plane
    judged = total = 0
    for e in range(N):
        assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A), f"{scenario}: the oracle's state differs"
        for a in range(A):
            _, prim = og.render_f64(e, a)
            m = nr.box_interior(prim, og.prim_table(e, a))
            n, bound = nr.plane_normals(depth[e * A + a], W, H)
            ok = m & (bound < nr.PLANE_MAX_ANGLE)
            total += int(m.sum()); judged += int(ok.sum())
            for got, fmt in ((f16, MV_NORMAL_F16), (s8, MV_NORMAL_SNORM8)):
                xyz, _ = nr.widen(got[e * A + a])
                err = np.abs(xyz[ok] - n[ok]).max(-1) if ok.any() else np.zeros(0)
                bad = err > bound[ok] + nr.FORMAT_ABS[fmt]
                assert not bad.any(), (f"{scenario} env {e} agent {a} format {fmt}: {int(bad.sum())} box pixels whose normal is not the depth plane's, worst "
                                       f"{float((err / (bound[ok] + nr.FORMAT_ABS[fmt])).max()):.1f} x the bound at {np.argwhere(ok)[err.argmax()].tolist()}")
    print(f"{scenario} {W}x{H}: planar consistency judged {judged} of {total} interior box pixels")
    # (one half: the share the check must reach on every frame set used; tests/test_normal_obs.py states what the reference alone reaches of the same frames)
    assert total > 0 and judged >= 0.5 * total, f"{scenario} {W}x{H}: the planar check judged only {judged} of {total} interior box pixels"
    # stepping with all three attached: colours, rewards, dones and state are the plain twin's
    for mode in ("fast", "exact"):
        hg.set_pixel_mode(mode); twin.set_pixel_mode(mode)
        for g in (hg, twin):
            g.step_n(2, "multidiscrete", 9, 0)
        assert np.array_equal(frames(hg), frames(twin))
        assert np.array_equal(hg.get_rewards_array().view(np.uint32), twin.get_rewards_array().view(np.uint32)) and np.array_equal(hg.get_dones(), twin.get_dones())
        for e in range(N):
            assert not diff_snapshots(hip_snapshot(hg, e), hip_snapshot(twin, e), A)
    for g in (og, hg, twin):
        g.close()


@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 2), ("Rearrange", 3), ("Collect", 2), ("HexMemory", 2)])
def test_planar_colour_layout(hip, scenario, A):
    """the channel-first colour layout (every list size's kernel): the planes are the RGBA gym's bytes, the colours a plain twin's, in both pixel modes"""
    N, (W, H) = pr.N_ENVS, pr.SIZES[0]
    rgba, chw, twin = (MegaverseGym(scenario, W, H, N, A, 1, False, {}) for _ in range(3))
    for g in (chw, twin):
        g.set_obs_layout("chw")
    for g in (rgba, chw, twin):
        g.seed(pr.SEED); g.reset()
    advance([rgba, chw, twin], None, N, A, 12)
    tr, tc = ({name: attach(g, name) for name in STREAMS} for g in (rgba, chw))
    for mode in ("fast", "exact"):
        for g in (rgba, chw, twin):
            g.set_pixel_mode(mode); g.render()
        for name in STREAMS:
            assert np.array_equal(raw(tc[name]), raw(tr[name])), f"{scenario} {mode}: the {name} planes depend on the colour layout"
        assert np.array_equal(frames(chw), frames(twin)), f"{scenario} {mode}: channel-first colours differ from a plain twin's"
        for g in (chw, twin):   # stepping with all three attached: colours, rewards, dones and state are the plain twin's in this layout too
            g.step_n(2, "multidiscrete", 9, 0)
        assert np.array_equal(frames(chw), frames(twin))
        assert np.array_equal(chw.get_rewards_array().view(np.uint32), twin.get_rewards_array().view(np.uint32)) and np.array_equal(chw.get_dones(), twin.get_dones())
        for e in range(N):
            assert not diff_snapshots(hip_snapshot(chw, e), hip_snapshot(twin, e), A)
        rgba.step_n(2, "multidiscrete", 9, 0)   # (the RGBA gym keeps pace: the next mode compares planes again)
    for g in (rgba, chw, twin):
        g.close()


# ---- 5. where it is written ------------------------------------------------------------------------------------------------------------------------
def ring_gym(subset=("normal",), count=4, fmt="float16", mode="fast", scenario="TowerBuilding", params=None, attach_planes=True):
    g = MegaverseGym(scenario, 40, 24, 4, 1, 1, False, params or {})
    g.set_pixel_mode(mode); g.seed(7); g.reset()
    obs = torch.zeros((count, 4, 24, 40, 4), dtype=torch.uint8, device="cuda")
    g.set_output_ring(count, obs.data_ptr())
    t = {name: attach(g, name, fmt) for name in subset} if attach_planes else {}
    return g, obs, t


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_step_n_fills_the_ring(hip, mode, fmt):
    """step_n(4) into a ring of 4: every entry is mv_render's plane of a twin stepped tick by tick; render = 'last' writes one entry, 'none' none"""
    g, obs, t = ring_gym(mode=mode, fmt=fmt)
    d = t["normal"]
    assert tuple(d.shape) == (4, 4, 24, 40, 4) and g._lib.mv_get_normal_obs(g._g) == 4
    assert g._lib.mv_get_normal_format(g._g) == (MV_NORMAL_SNORM8 if fmt == "int8" else MV_NORMAL_F16)
    twin = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    twin.set_pixel_mode(mode); twin.seed(7); twin.reset()
    td = twin.set_normal_obs(True, fmt)
    sentinel(d)
    g.step_n(4, "multidiscrete", 9, 0)
    got = raw(d)
    assert not is_sentinel(got).all(-1).any()
    for j in range(4):
        twin.step_n(1, "multidiscrete", 9, j, render="none")
        twin.render()
        assert np.array_equal(got[j], raw(td)[0]), f"entry {j} is not the plane of tick {j}"
    sentinel(d); g.step_n(4, "multidiscrete", 9, 4, render="none")
    assert is_sentinel(raw(d)).all()
    g.step_n(4, "multidiscrete", 9, 8, render="last")
    got = raw(d)
    assert is_sentinel(got[:3]).all() and not is_sentinel(got[3]).all(-1).any()
    sentinel(d); g.macro_step(3, np.zeros((4, 6), np.int32), render="last")
    got = raw(d)
    assert not is_sentinel(got[0]).all(-1).any() and is_sentinel(got[1:]).all()
    sentinel(d); g.macro_step(3, np.zeros((4, 6), np.int32), render="none"); g.step_no_render()
    assert is_sentinel(raw(d)).all()
    g.close(); twin.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_launch_counts_of_every_subset(hip, mode):
    """fast mode: exactly ONE launch more per drawn tick than a plain gym, whichever subset is attached; exact mode: none more"""
    plain, pobs, _ = ring_gym(mode=mode, attach_planes=False)
    p0 = plain.debug_launch_counts(); plain.step_n(4, "multidiscrete", 9, 0); plain.step(); p1 = plain.debug_launch_counts()
    for subset in SUBSETS:
        g, obs, t = ring_gym(subset=subset, mode=mode)
        c0 = g.debug_launch_counts(); g.step_n(4, "multidiscrete", 9, 0); g.step(); c1 = g.debug_launch_counts()
        assert c1[0] - c0[0] == p1[0] - p0[0], subset
        assert (c1[1] - c0[1]) - (p1[1] - p0[1]) == (5 if mode == "fast" else 0), f"{subset}: {(c1[1] - c0[1]) - (p1[1] - p0[1])} launches more than a plain gym in 5 drawn ticks"
        assert np.array_equal(planes(obs), planes(pobs)), f"{subset}: the colours differ from those of a gym without planes"
        g.close()
    plain.close()


def test_masks_resets_and_single_steps(hip):
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(7); g.reset()
    d = g.set_normal_obs(True)
    assert tuple(d.shape) == (1, 4, 24, 40, 4) and d.dtype == torch.float16
    written = lambda x: not is_sentinel(x).all(-1).any()   # noqa: E731  (every pixel's value was stored)
    sentinel(d); g.step()
    assert written(raw(d)) and tuple(g.normal_obs().shape) == (4, 24, 40, 4)
    sentinel(d); g.set_draw_mask(np.array([1, 0, 1, 0], np.uint8)); g.step()
    got = raw(d)[0]
    assert written(got[[0, 2]]) and is_sentinel(got[[1, 3]]).all()
    g.step_n(3, "multidiscrete", 1, 0)
    got = raw(d)[0]
    assert written(got[[0, 2]]) and is_sentinel(got[[1, 3]]).all()
    g.set_draw_mask(None)
    sentinel(d); g.reset()
    assert written(raw(d))
    sentinel(d); g.reset_envs(np.array([0, 1, 0, 0], np.uint8), render=True)
    assert written(raw(d))
    sentinel(d); g.reset_envs(np.array([0, 1, 0, 0], np.uint8), render=False)
    assert is_sentinel(raw(d)).all()
    sentinel(d); g.step_no_render()
    assert is_sentinel(raw(d)).all()
    g.render(); want = raw(d)
    g.set_pipelining(False); sentinel(d); g.render()
    assert np.array_equal(raw(d), want)
    g.close()


# ---- 6. resets inside a batched call ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_resets_inside_a_batched_call(hip, mode):
    """Empty with episodes of 0.2 s, three ticks: envs reset inside every 4-tick call, and every ring entry's normals are the tick-by-tick twin's, byte for byte -- the
    normals read nothing outside the frame's own list and header (the labels' batched-call limit does not apply)"""
    params = {"episodeLengthSec": 0.2}
    g, obs, t = ring_gym(mode=mode, params=params, scenario="Empty")
    twin = MegaverseGym("Empty", 40, 24, 4, 1, 1, False, params)
    twin.set_pixel_mode(mode); twin.seed(7); twin.reset()
    td = twin.set_normal_obs(True)
    dones = 0
    for call in range(2):
        sentinel(t["normal"])
        g.step_n(4, "multidiscrete", 9, 4 * call)
        got = raw(t["normal"])
        for j in range(4):
            twin.step_n(1, "multidiscrete", 9, 4 * call + j)
            dones += int(np.asarray(twin.get_dones()).sum())
            assert np.array_equal(got[j], raw(td)[0]), f"call {call}: entry {j} differs from the tick-by-tick twin's"
    assert dones > 0, "no env finished an episode inside the calls: the test shows nothing"
    g.close(); twin.close()


# ---- 7. refusals and surface -----------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(1); g.reset()
    lib = g._lib
    err = lambda: lib.mv_last_error().decode()   # noqa: E731
    buf = torch.zeros((1, 4, 24, 40, 4), device="cuda", dtype=torch.float16)
    assert lib.mv_set_normal_obs(g._g, buf.data_ptr(), 5) == -1 and err() == "mv_set_normal_obs: unknown format (MV_NORMAL_F16, MV_NORMAL_SNORM8)"
    assert lib.mv_get_normal_obs(g._g) == 0 and lib.mv_get_normal_format(g._g) == -1
    assert lib.mv_set_normal_obs(g._g, buf.data_ptr() + 4, MV_NORMAL_F16) == -1
    assert err() == "mv_set_normal_obs: the buffer must be 8-byte aligned (MV_NORMAL_F16) or 4-byte aligned (MV_NORMAL_SNORM8)"
    assert lib.mv_set_normal_obs(g._g, buf.data_ptr() + 2, MV_NORMAL_SNORM8) == -1 and "4-byte aligned" in err()
    assert lib.mv_set_normal_obs(g._g, buf.data_ptr() + 4, MV_NORMAL_SNORM8) == 0 and lib.mv_set_normal_obs(g._g, None, 0) == 0
    with pytest.raises(RuntimeError, match=r"mv_get_normal_observation: no normal observations attached \(mv_set_normal_obs\)"):
        g.get_normal_observation(0, 0)
    with pytest.raises(ValueError, match="set_normal_obs"):
        g.set_normal_obs(torch.zeros((1, 4, 24, 40), device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError, match="set_normal_obs"):
        g.set_normal_obs(torch.zeros((1, 4, 24, 40, 4), device="cuda", dtype=torch.float32))
    g.set_still_frames(True)
    with pytest.raises(RuntimeError) as ei:
        g.set_normal_obs(True)
    assert str(ei.value) == ("mv_set_normal_obs: still frames are switched on (mv_set_still_frames), and a still frame's normal plane would not be carried: "
                             "switch them off first")
    g.set_still_frames(False)
    g.set_normal_obs(buf)
    assert lib.mv_get_normal_obs(g._g) == 1 and lib.mv_get_normal_format(g._g) == MV_NORMAL_F16
    with pytest.raises(RuntimeError) as ei:
        g.set_still_frames(True)
    assert str(ei.value) == ("mv_set_still_frames: normal observations are attached (mv_set_normal_obs), and a still frame's normal plane would not be carried: "
                             "detach the normal observations first")
    ring = torch.zeros((2, 4, 24, 40, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError) as ei:
        g.set_output_ring(2, ring.data_ptr())
    assert str(ei.value) == ("mv_set_output_ring: normal observations are attached (mv_set_normal_obs), sized by the ring count they were attached under: "
                             "detach the normal observations first")
    with pytest.raises(RuntimeError) as ei:
        g.set_render_resolution(64, 36)
    assert str(ei.value) == ("mv_set_render_resolution: normal observations are attached (mv_set_normal_obs), whose planes are of the observation size: "
                             "detach the normal observations first")
    other = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    other.seed(1); other.reset()
    handles = (C.c_void_p * 2)(g._g.value, other._g.value)
    out = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1
    assert err() == "mv_group_create: a gym has normal observations attached (mv_set_normal_obs): the union launches write none; detach them first"
    assert lib.mv_step_many(handles, 2, 1, 1, 0, 0) == -1
    assert err() == "mv_step_many: gym 0 has normal observations attached (mv_set_normal_obs): step it on its own, or detach them first"
    g.draw_hires()   # ignores the option
    g.set_normal_obs(None)
    assert lib.mv_get_normal_obs(g._g) == 0
    g.set_output_ring(2, ring.data_ptr()); g.set_output_ring(0)
    g.set_render_resolution(64, 36)
    assert lib.mv_group_create(handles, 2, C.byref(out)) == 0
    assert lib.mv_set_normal_obs(g._g, buf.data_ptr(), 0) == -1
    assert err() == "mv_set_normal_obs: this gym belongs to an mv_group, whose union launches write no normal observations"
    lib.mv_group_destroy(out)
    mt = MultiTaskGym(["TowerBuilding", "ObstaclesHard"], 40, 24, 4, 1, 2)
    with pytest.raises(RuntimeError) as ei:
        mt.set_normal_obs(True)
    assert str(ei.value) == ("MultiTaskGym.set_normal_obs: mv_group_create and mv_step_many refuse a gym with normal observations attached "
                             "(mv_set_normal_obs): the union launches write none; step such a gym on its own")
    mt.close()
    g.close(); other.close()


def test_detach_is_as_never_attached(hip):
    """after a detach the gym's launches and bytes are those of a gym that never attached; mv_close leaves the caller's buffer alone"""
    a, b = (MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {}) for _ in range(2))
    for g in (a, b):
        g.seed(2); g.reset()
    d = a.set_normal_obs(True, "int8")
    a.step_n(2, "multidiscrete", 4, 0); b.step_n(2, "multidiscrete", 4, 0)
    a.set_normal_obs(None)
    sentinel(d)
    ca, cb = a.debug_launch_counts(), b.debug_launch_counts()
    for g in (a, b):
        g.step_n(4, "multidiscrete", 4, 2); g.step(); g.render()
    ca2, cb2 = a.debug_launch_counts(), b.debug_launch_counts()
    assert (ca2[0] - ca[0], ca2[1] - ca[1]) == (cb2[0] - cb[0], cb2[1] - cb[1])
    assert np.array_equal(frames(a), frames(b)) and is_sentinel(raw(d)).all()
    d = a.set_normal_obs(True); a.render(); want = raw(d)
    a.close(); b.close()
    assert np.array_equal(raw(d), want)


def test_megaverse_env_surface(hip):
    """MegaverseEnv(..., normal_obs=...): planes per env and agent, the RGB observation space unchanged, the buffer re-attached around ring changes"""
    import megaverse_amd
    from megaverse_amd.megaverse_env import MegaverseEnv
    with pytest.raises(ValueError, match="normal_obs"):
        MegaverseEnv("TowerBuilding", 4, 2, img_w=40, img_h=24, normal_obs="float32")
    env = MegaverseEnv("TowerBuilding", 4, 2, img_w=40, img_h=24, normal_obs="int8", depth_obs=True)
    env.reset()
    d = env.normal_obs()
    assert tuple(d.shape) == (4, 2, 24, 40, 4) and d.dtype == torch.int8
    xyz, valid = megaverse_amd.normals_to_float(d)
    torch.cuda.synchronize()
    assert tuple(xyz.shape) == (4, 2, 24, 40, 3) and xyz.dtype == torch.float32 and bool(valid.any())
    assert bool((valid == (env.depth_obs() > 0)).all())
    assert float((xyz[valid].norm(dim=-1) - 1).abs().max()) <= norm_bound(MV_NORMAL_SNORM8)
    assert env.observation_space.shape == (3, 24, 40)
    env._set_output_ring(0)   # (what step_device / step_sequence do around their rings)
    assert env.env._lib.mv_get_normal_obs(env.env._g) == 1 and env.normal_obs().dtype == torch.int8
    env.close()
    env = MegaverseEnv("TowerBuilding", 4, 1, img_w=40, img_h=24, normal_obs=True)
    env.reset()
    assert env.normal_obs().dtype == torch.float16
    env.close()
    plain = MegaverseEnv("TowerBuilding", 4, 1, img_w=40, img_h=24)
    with pytest.raises(RuntimeError, match="normal_obs=True"):
        plain.normal_obs()
    plain.close()
