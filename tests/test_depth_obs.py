"""CPU: depth observations (mv_set_depth_obs) without a device -- the pack rule's host twin against numpy, the exported symbols, and what the GPU tests'
reference (tests/depth_reference.py) rests on, asserted on the oracle alone: the closed forms agree with the float64 caster, every pose keeps at least 80 % of
the frame interior, and a numpy float32 restatement of the kernel's slab formula stays inside the derived bound at every compared pixel."""
import os

import numpy as np
import pytest

import depth_reference as dr
import oracle_lib
from canonical_frames import EYE_Y
from megaverse_amd import extension as ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the pack rule ---------------------------------------------------------------------------------------------------------------------------------
def test_pack_f32_is_the_bits_of_t():
    rng = np.random.default_rng(1)
    t = rng.uniform(0.01, 120.0, 4096).astype(np.float32)
    hit = (rng.random(t.size) < 0.8).astype(np.uint8)
    got = ext.debug_depth_pack_host(t, hit, ext.MV_DEPTH_F32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.where(hit != 0, t, np.float32(0)).view(np.uint32))


def test_pack_f16_rounds_to_nearest_even():
    rng = np.random.default_rng(2)
    t = rng.uniform(0.01, 120.0, 1 << 16).astype(np.float32)
    got = ext.debug_depth_pack_host(t, np.ones(t.size, np.uint8), ext.MV_DEPTH_F16)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), t.astype(np.float16).view(np.uint16))
    # exactly halfway between two neighbouring halves: the tie goes to the even one
    h = np.arange(np.float16(0.01).view(np.uint16), np.float16(120.0).view(np.uint16), dtype=np.uint16)
    lo, hi = h.view(np.float16).astype(np.float32), (h + 1).view(np.float16).astype(np.float32)
    mid = (lo + hi) * np.float32(0.5)   # exact: 12 significant bits
    assert np.array_equal(mid.astype(np.float64), (lo.astype(np.float64) + hi.astype(np.float64)) / 2)
    got = ext.debug_depth_pack_host(mid, np.ones(mid.size, np.uint8), ext.MV_DEPTH_F16)
    want = np.where(h % 2 == 0, h, h + 1).astype(np.uint16)
    assert np.array_equal(got.view(np.uint16), want) and np.array_equal(want, mid.astype(np.float16).view(np.uint16))


def test_pack_no_hit_is_zero_in_both_formats():
    t = np.array([0.01, 5.0, 120.0, np.inf], np.float32)
    for fmt in (ext.MV_DEPTH_F32, ext.MV_DEPTH_F16):
        got = ext.debug_depth_pack_host(t, np.zeros(4, np.uint8), fmt)
        assert not got.view(np.uint16 if fmt else np.uint32).any()


def test_pack_refuses_an_unknown_format():
    with pytest.raises(RuntimeError, match="unknown format"):
        ext.debug_depth_pack_host(np.ones(2, np.float32), np.ones(2, np.uint8), 7)


def test_symbols_are_exported_and_bound():
    lib = ext.load_library()
    names = ["mv_set_depth_obs", "mv_get_depth_obs", "mv_get_depth_format", "mv_get_depth_observation", "mv_debug_depth_pack_host"]
    bound = {s[0] for s in ext.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "megaverse_hip.h")).read()
    for n in names:
        assert n in bound and hasattr(lib, n) and f" {n}(" in header, n
    assert lib.mv_get_depth_obs(None) == -1 and lib.mv_get_depth_format(None) == -1
    assert lib.mv_set_depth_obs(None, None, 0) == -1 and b"mv_set_depth_obs" in lib.mv_last_error()


def test_python_argument_checks():
    assert ext.depth_format_of("float16") == ext.MV_DEPTH_F16 and ext.depth_format_of(np.float32) == ext.MV_DEPTH_F32
    with pytest.raises(ValueError):
        ext.depth_format_of("int8")
    with pytest.raises(ValueError, match="set_depth_obs"):
        ext.check_depth_obs(np.zeros((1, 4, 8, 8), np.float32), 1, 4, 8, 8, ext.MV_DEPTH_F32, 0)   # not a CUDA tensor


# ---- the reference, on the oracle alone ------------------------------------------------------------------------------------------------------------
RATIOS = {}


def check_pose(og, env, W, H, what):
    """the 80 % condition and the float32 model's bound for one pose -> (t64, box, axis, masks ...) for the closed-form checks"""
    snap = og.snapshot(env)
    _, prim = og.render_f64(env, 0)
    table = og.prim_table(env, 0)
    share = dr.interior_share(prim)
    assert share >= dr.INTERIOR_SHARE, f"{what}: only {share:.3f} of the frame is interior"
    t, box, axis, dwk, lo, hi = dr.expected_boxes(snap, 0, W, H)
    m = dr.interior_mask(prim, table, dr.is_world_box)
    assert m.any() and np.isfinite(t[m]).all(), f"{what}: the caster misses where the oracle's float64 frame shows a world box"
    assert np.isinf(t[dr.background_mask(prim)]).all(), f"{what}: the caster hits a world box where the oracle's float64 frame shows background"
    a = snap["agents"][0]
    model = dr.slab_model_f32(a["pos"], a["basis"], a["pitch"], W, H, lo, hi, box, axis)
    ratio = float((np.abs(model[m].astype(np.float64) - t[m]) / dr.slab_bound(t[m], dwk[m])).max())
    RATIOS[what] = ratio
    print(f"{what}: interior {share:.3f}, compared hits {int(m.sum())}, float32 model / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: the float32 restatement leaves the derived bound ({ratio:.2f} of it)"
    return t, box, axis, m, lo, hi


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_tower_poses_closed_forms(W, H):
    og = oracle_lib.OracleGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1)
    og.seed(dr.TOWER_SEED); og.reset()
    e = dr.pose_tower_wall(og, [og])
    t, box, axis, m, lo, hi = check_pose(og, e, W, H, f"TowerBuilding wall {W}x{H}")
    wall = m & (axis == 0) & (hi[np.maximum(box, 0), 0] == 1.0)
    assert wall.sum() > 0.2 * W * H and np.abs(t[wall] - dr.WALL_DIST).max() < 1e-12          # (a): the face's distance, for EVERY pixel of the face
    floor = m & (axis == 1) & (hi[np.maximum(box, 0), 1] == 1.0)
    dcy = dr.rays64(W, H)[..., 1]
    assert floor.sum() > 0.05 * W * H and (dcy[floor] < 0).all() and (np.abs(t[floor] - (EYE_Y - 1.0) / -dcy[floor]) < 2.0 ** -23 * t[floor]).all()   # (b); the pose's fp32 height is within half an ulp of REST_Y
    e, _ = dr.pose_tower_box(og, [og])
    t, box, axis, m, lo, hi = check_pose(og, e, W, H, f"TowerBuilding box {W}x{H}")
    cube = (hi[:, 0] - lo[:, 0] < 0.8)[np.maximum(box, 0)]   # (a movable box: a cube of edge 0.78)
    face = m & (axis == 0) & cube & (np.abs(t - dr.BOX_DIST) < 1e-6)
    half_ulp = float(np.spacing(np.float32(og.snapshot(e)["agents"][0]["pos"][0]))) / 2   # (the pose's x is the nearest fp32 to face + BOX_DIST)
    assert face.sum() >= 4 and np.abs(t[face] - dr.BOX_DIST).max() <= half_ulp                # (c)
    og.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
@pytest.mark.parametrize("pose", list(dr.EMPTY_POSES))
def test_empty_poses(pose, W, H):
    og = oracle_lib.OracleGym("Empty", W, H, dr.EMPTY_ENVS, 1, 1)
    og.seed(dr.EMPTY_SEED); og.reset()
    e = dr.pose_empty([og], pose)
    pitch = float(og.snapshot(e)["agents"][0]["pitch"])
    assert (pitch == 0.0) == (pose == "pitch 0") and abs(pitch) < 0.5
    check_pose(og, e, W, H, f"Empty {pose} {W}x{H}")
    og.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_football_pose(W, H):
    """(e): the ball in front of a pitch-0 agent -- the 80 % condition, the ball alone inside 0.8 of its projected radius, and the measured float32 bound"""
    og = oracle_lib.OracleGym("Football", W, H, 4, 2, 1)
    og.seed(dr.EMPTY_SEED); og.reset()
    e, centre, radius = dr.pose_football([og])
    snap = og.snapshot(e); a = snap["agents"][0]
    _, prim = og.render_f64(e, 0)
    table = og.prim_table(e, 0)
    assert dr.interior_share(prim) >= dr.INTERIOR_SHARE
    eye, C = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, share = dr.cast_sphere(eye, C, W, H, centre, radius)
    inside = np.isfinite(t) & (share <= 0.8)
    assert inside.sum() >= 4 and (table[prim[inside], 0] == 4).all(), "something else than the ball inside 0.8 of its projected radius"
    assert 0.0 <= t[inside].min() - (dr.BALL_DIST - dr.BALL_RADIUS) < 0.05   # the nearest point: the centre's distance less the radius (pixel centres miss it by a little)
    model = dr.sphere_model_f32(a["pos"], a["basis"], a["pitch"], W, H, centre, radius)
    rel = float((np.abs(model[inside].astype(np.float64) - t[inside]) / t[inside]).max())
    print(f"Football {W}x{H}: {int(inside.sum())} compared pixels, float32 model relative error {rel:.2e} (bound {dr.SPHERE_REL:.1e} = 4 x the largest measured)")
    assert 4 * rel <= dr.SPHERE_REL * 1.0001
    og.close()


def test_wrong_conventions_miss_by_orders_of_magnitude():
    """Euclidean depth and a flipped row order against the planar, bottom-up closed forms: far outside the bound"""
    W, H = 40, 24
    og = oracle_lib.OracleGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1)
    og.seed(dr.TOWER_SEED); og.reset()
    e = dr.pose_tower_wall(og, [og])
    t, box, axis, dwk, lo, hi = dr.expected_boxes(og.snapshot(e), 0, W, H)
    hit = np.isfinite(t)
    bound = dr.slab_bound(np.where(hit, t, 1.0), np.where(hit, dwk, 1.0))
    euclid = t * np.linalg.norm(dr.rays64(W, H), axis=-1)
    assert ((np.abs(euclid - t) > 1000 * bound) & hit).mean() > 0.5
    flipped = t[::-1]
    both = hit & np.isfinite(flipped)
    assert ((np.abs(flipped - t) > 1000 * bound) & both).sum() > 0.2 * W * H
    og.close()
