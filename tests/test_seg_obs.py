"""CPU: segmentation observations (mv_set_seg_obs) without a device -- the label rule's host twin against a Python restatement of the table for every
scenario, the pack rule against numpy, seg_split, the exported symbols, and what the GPU tests' reference (tests/seg_reference.py) rests on, asserted on the
oracle alone: the restated draw list agrees with the oracle's, every pose keeps at least 80 % of the frame interior, no interior pixel of a box scene has a
runner-up within pixel_reference's EPS_4ULP of its winner, and planted mistakes are rejected."""
import os

import numpy as np
import pytest

import depth_reference as dr
import oracle_lib
import pixel_reference as pr
import seg_reference as sr
from megaverse_amd import extension as ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = sr.CLASSES
SCENARIOS = sorted(sr.SCN.values())


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(ROOT, "tests", "golden", "boxoban"))


# ---- the table, restated -----------------------------------------------------------------------------------------------------------------------------
def bounds_py(scen, L, Wr, boxes, terrain, objects, rewards, agents):
    hexlike = scen in sr.HEX_LIKE
    n_terrain = 1 if scen == 0 else sr.NUM_STATIC + terrain if scen == 3 else L * max(Wr, 1) if scen == 4 else 0 if hexlike else terrain
    n_rewards = 0 if scen == 0 else 3 * rewards if hexlike else 2 * rewards
    t = boxes; o = t + n_terrain; r = o + objects; a = r + n_rewards
    return (t, o, r, a, a + 3 * agents)


def rule_py(scen, slot, b, subtype):
    """the table of mv_seg_obs.h, from the issue's text: -> (class, instance)"""
    t, o, r, a, end = b
    hexlike = scen in sr.HEX_LIKE
    if slot < 0 or slot >= end:
        return 0, 0
    if slot < t:
        return (K["STRUCTURE"] if hexlike or subtype != 0 else K["FLOOR"]), slot
    if slot < o:
        j = slot - t
        if scen == 0:
            return K["BUILDING_ZONE"], 0
        if scen == 3:
            return (K["FURNITURE"], j) if j < sr.NUM_STATIC else (K["TARGET"], j - sr.NUM_STATIC)
        if scen == 4:
            return (K["FURNITURE"], j) if subtype == sr.SOKO_WALL else (K["EXIT"], j) if subtype == sr.SOKO_GOAL else (0, 0)
        return (K["EXIT"] if subtype == sr.TERRAIN_EXIT else K["LAVA"]), j
    if slot < r:
        return (K["CARRIED"] if subtype > 0 else K["MOVABLE"]), slot - o
    if slot < a:
        q = slot - r
        if hexlike:
            return (K["BALL"] if scen == 9 else K["COLLECTABLE"]), q // 3
        return (K["HAZARD"] if scen == 2 and subtype == 2 else K["COLLECTABLE"]), q // 2
    q = slot - a
    return (K["HUD"] if q % 3 == 2 else K["AGENT"]), q // 3


COUNTS = [  # (L, W, boxes, terrain, objects, rewards, agents): full groups, then empty ones
    (8, 6, 7, 3, 5, 4, 3), (8, 6, 7, 0, 0, 0, 1), (5, 5, 0, 0, 0, 0, 2), (12, 9, 60, 16, 80, 16, 8),
]


@pytest.mark.parametrize("scen", SCENARIOS)
def test_rule_host_against_the_table(scen):
    for counts in COUNTS:
        b = bounds_py(scen, *counts)
        assert ext.debug_seg_bounds_host(scen, *counts) == b, (scen, counts)
        slots = {-1, b[4], b[4] - 1}
        for edge in b:
            slots |= {edge - 1, edge, edge + 1}
        A = counts[6]
        slots |= {b[3] + p for p in (0, 1, 2)} | {b[3] + 3 * (A - 1) + p for p in (0, 1, 2)}   # parts 0 / 1 / 2 of the first and the last agent
        for slot in sorted(slots):
            for subtype in (-1, 0, 1, 2, 3, 4):
                cls, inst = rule_py(scen, slot, b, subtype)
                want = sr.word(cls, inst)
                assert ext.debug_seg_rule_host(scen, slot, b, subtype, "instance") == want, (scen, counts, slot, subtype)
                assert ext.debug_seg_rule_host(scen, slot, b, subtype, "class") == want >> 12, (scen, counts, slot, subtype)


def test_rule_named_cases():
    full = (8, 6, 7, 3, 5, 4, 3)
    tower, collect, rearr, hexm, foot, obst, soko = (sr.SCN[n] for n in ("TowerBuilding", "Collect", "Rearrange", "HexMemory", "Football", "Obstacles", "Sokoban"))
    b = bounds_py(tower, *full)
    assert b == (7, 8, 13, 13, 22)   # (no diamonds in TowerBuilding: the reward group is empty)
    rule = lambda s, slot, bb, sub: sr.split([ext.debug_seg_rule_host(s, slot, bb, sub, "instance")])
    assert rule(tower, 7, b, 0) == (K["BUILDING_ZONE"], 0)
    assert rule(tower, 9, b, 0) == (K["MOVABLE"], 1) and rule(tower, 9, b, 2) == (K["CARRIED"], 1)          # a resting and a carried object
    assert rule(tower, 13, b, 0) == (K["AGENT"], 0) and rule(tower, 14, b, 0) == (K["AGENT"], 0) and rule(tower, 15, b, 0) == (K["HUD"], 0)
    assert rule(tower, 19, b, 0) == (K["AGENT"], 2) and rule(tower, 21, b, 0) == (K["HUD"], 2)
    assert rule(tower, 3, b, 0) == (K["FLOOR"], 3) and rule(tower, 3, b, 1) == (K["STRUCTURE"], 3)
    b = bounds_py(collect, *full)
    assert rule(collect, b[2] + 5, b, 1) == (K["COLLECTABLE"], 2) and rule(collect, b[2] + 5, b, 2) == (K["HAZARD"], 2)   # green and red diamonds
    b = bounds_py(obst, *full)
    assert rule(obst, b[2] + 5, b, 2) == (K["COLLECTABLE"], 2)    # (polarity is Collect's)
    assert rule(obst, b[0] + 1, b, sr.TERRAIN_EXIT) == (K["EXIT"], 1) and rule(obst, b[0] + 1, b, 2) == (K["LAVA"], 1)
    b = bounds_py(hexm, *full)
    # HexMemory's good / bad bit (HexRec.meta >> 4 & 1) is no input of the rule: a good and a bad object map to the same word, and no sub-type value moves it
    good_meta, bad_meta = sr.HEX_DIAMOND | 1 << 4 | 1 << 8, sr.HEX_DIAMOND | 0 << 4 | 1 << 8
    assert ext.debug_seg_rule_host(hexm, b[2] + 4, b, good_meta, "instance") == ext.debug_seg_rule_host(hexm, b[2] + 4, b, bad_meta, "instance") == sr.word(K["COLLECTABLE"], 1)
    for sub in range(-1, 5):
        assert ext.debug_seg_rule_host(hexm, b[2] + 4, b, sub, "instance") == sr.word(K["COLLECTABLE"], 1)
        assert ext.debug_seg_rule_host(hexm, 3, b, sub, "instance") == sr.word(K["STRUCTURE"], 3)
    b = bounds_py(foot, 8, 6, 7, 0, 0, 1, 2)
    assert rule(foot, b[2], b, 0) == (K["BALL"], 0)
    b = bounds_py(rearr, *full)
    assert b[1] - b[0] == sr.NUM_STATIC + 3
    assert rule(rearr, b[0] + 8, b, 0) == (K["FURNITURE"], 8) and rule(rearr, b[0] + 9, b, 0) == (K["TARGET"], 0)
    b = bounds_py(soko, *full)
    assert b[1] - b[0] == 8 * 6
    assert rule(soko, b[0] + 13, b, sr.SOKO_WALL) == (K["FURNITURE"], 13) and rule(soko, b[0] + 13, b, sr.SOKO_GOAL) == (K["EXIT"], 13)
    assert ext.debug_seg_rule_host(soko, b[0] + 13, b, 0, "instance") == 0


def test_class_names_and_the_exported_table():
    assert ext.SEG_CLASSES == K and len(K) == 15 and max(K.values()) == 14
    for name, value in K.items():
        assert ext.seg_class_name(value) == name
    assert ext.seg_class_name(15) is None and ext.seg_class_name(-1) is None
    import megaverse_amd
    assert megaverse_amd.SEG_CLASSES is ext.SEG_CLASSES and megaverse_amd.seg_split is ext.seg_split


# ---- the pack rule, seg_split --------------------------------------------------------------------------------------------------------------------------
def test_pack_host_against_numpy():
    rng = np.random.default_rng(3)
    cls = rng.integers(0, 15, 4096).astype(np.int32)
    inst = rng.integers(0, 4096, 4096).astype(np.int32)
    cls[:4], inst[:4] = [0, 0, 14, 1], [0, 4095, 4095, 4095]
    u16 = ext.debug_seg_pack_host(cls, inst, "instance")
    u8 = ext.debug_seg_pack_host(cls, inst, "class")
    assert u16.dtype == np.uint16 and u8.dtype == np.uint8
    assert np.array_equal(u16, np.where(cls == 0, 0, (cls << 12) | inst).astype(np.uint16))
    assert np.array_equal(u16 >> 12, u8) and np.array_equal(u8, cls)                    # the class nibble is the U8 byte, bit for bit
    assert u16[0] == 0 and u16[1] == 0 and u8[1] == 0                                   # class 0: the whole word is 0, whatever the instance
    assert u16[2] == (14 << 12) | 4095 and (u16[2] & 4095) == 4095 and u16[3] == (1 << 12) | 4095   # instance 4095 round-trips
    with pytest.raises(RuntimeError, match="unknown format"):
        load = ext.load_library()
        out = np.zeros(2, np.uint16)
        if load.mv_debug_seg_pack_host(cls.ctypes.data, inst.ctypes.data, 2, 7, out.ctypes.data) != 0:
            raise RuntimeError(load.mv_last_error().decode())
    with pytest.raises(RuntimeError, match="instance outside"):
        ext.debug_seg_pack_host([1], [4096], "instance")


def test_seg_split_numpy_and_torch():
    import torch
    words = np.array([0, (1 << 12) | 5, (14 << 12) | 4095, (8 << 12) | 79, (13 << 12) | 7], np.uint16)
    cls, inst = ext.seg_split(words)
    assert cls.tolist() == [0, 1, 14, 8, 13] and inst.tolist() == [0, 5, 4095, 79, 7]
    cls, inst = ext.seg_split(words.view(np.int16))       # the bits of an int16 tensor's numpy copy
    assert cls.tolist() == [0, 1, 14, 8, 13] and inst.tolist() == [0, 5, 4095, 79, 7]
    tc, ti = ext.seg_split(torch.from_numpy(words.view(np.int16).copy()).reshape(5, 1))
    assert tc.dtype == torch.uint8 and tuple(tc.shape) == (5, 1) and tc.flatten().tolist() == [0, 1, 14, 8, 13] and ti.flatten().tolist() == [0, 5, 4095, 79, 7]
    assert sr.split(words)[0].tolist() == cls.tolist()


def test_symbols_are_exported_and_bound():
    lib = ext.load_library()
    names = ["mv_set_seg_obs", "mv_get_seg_obs", "mv_get_seg_format", "mv_get_seg_observation", "mv_seg_class_name", "mv_debug_seg_rule_host",
             "mv_debug_seg_pack_host", "mv_debug_seg_bounds_host"]
    bound = {s[0] for s in ext.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "megaverse_hip.h")).read()
    for n in names:
        assert n in bound and hasattr(lib, n) and f"{n}(" in header, n
    assert lib.mv_get_seg_obs(None) == -1 and lib.mv_get_seg_format(None) == -1
    assert lib.mv_set_seg_obs(None, None, 0) == -1 and b"mv_set_seg_obs" in lib.mv_last_error()


def test_python_argument_checks():
    assert ext.seg_format_of("class") == ext.MV_SEG_CLASS_U8 and ext.seg_format_of("instance") == ext.MV_SEG_INSTANCE_U16 and ext.seg_format_of(1) == 1
    for bad in ("depth", 2, True, None):
        with pytest.raises(ValueError, match="set_seg_obs"):
            ext.seg_format_of(bad)
    with pytest.raises(ValueError, match="set_seg_obs"):
        ext.check_seg_obs(np.zeros((1, 4, 8, 8), np.uint8), 1, 4, 8, 8, ext.MV_SEG_CLASS_U8, 0)   # not a CUDA tensor
    from megaverse_amd.multitask import MultiTaskGym
    with pytest.raises(RuntimeError, match="mv_set_seg_obs"):
        MultiTaskGym.set_seg_obs(None)


# ---- the reference, on the oracle alone ----------------------------------------------------------------------------------------------------------------
def check_box_pose(og, env, W, H, what):
    """the conditions of a box scene: 80 % interior, the caster's hit / miss and labels agree with the restated draw list at the compared pixels, and no
    compared hit pixel has a runner-up within EPS_4ULP -> (want, interior, prim)"""
    snap = og.snapshot(env)
    m, prim = sr.world_box_interior(og, env, 0)
    share = dr.interior_share(prim)
    assert share >= sr.INTERIOR_SHARE, f"{what}: only {share:.3f} of the frame is interior"
    want, margin, hit = sr.box_scene(snap, 0, W, H)
    listed, interior = sr.expected(og, snap, env, 0)
    assert m.any() and np.array_equal(want[m], listed[m]), f"{what}: the caster's labels differ from the restated draw list's at compared pixels"
    fragile = m & hit & (margin <= pr.EPS_4ULP)
    print(f"{what}: interior {share:.3f}, compared {int(m.sum())}, smallest runner-up margin {float(margin[m & hit].min()):.2e}, classes {sorted(set((want[m] >> 12).tolist()))}")
    assert not fragile.any(), f"{what}: {int(fragile.sum())} compared pixels have a runner-up within EPS_4ULP: choose another pose"
    return want, m, prim


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_box_scene_conditions_tower(W, H):
    og = oracle_lib.OracleGym("TowerBuilding", W, H, dr.TOWER_ENVS, 1, 1)
    og.seed(dr.TOWER_SEED); og.reset()
    e = dr.pose_tower_wall(og, [og])
    want, m, _ = check_box_pose(og, e, W, H, f"TowerBuilding wall {W}x{H}")
    assert {K["FLOOR"], K["STRUCTURE"]} <= set((want[m] >> 12).tolist())
    e, _ = dr.pose_tower_box(og, [og])
    want, m, prim = check_box_pose(og, e, W, H, f"TowerBuilding box {W}x{H}")
    assert K["MOVABLE"] in set((want[m] >> 12).tolist())
    # planted mistakes on the model: each is rejected
    listed, interior = sr.expected(og, og.snapshot(e), e, 0)
    sr.judge(listed, listed, interior)
    sr.judge(listed >> 12, listed, interior, class_only=True)
    for name, wrong in (("rows flipped", sr.planted_rows_flipped(listed)), ("shifted by a tile", sr.planted_tile_shift(listed)),
                        ("slot for instance", sr.planted_slot_for_instance(listed, prim))):
        with pytest.raises(AssertionError):
            sr.judge(wrong, listed, interior, name)
    og.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
@pytest.mark.parametrize("pose", list(dr.EMPTY_POSES))
def test_box_scene_conditions_empty(pose, W, H):
    og = oracle_lib.OracleGym("Empty", W, H, dr.EMPTY_ENVS, 1, 1)
    og.seed(dr.EMPTY_SEED); og.reset()
    e = dr.pose_empty([og], pose)
    check_box_pose(og, e, W, H, f"Empty {pose} {W}x{H}")
    og.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_box_scene_conditions_obstacles(W, H):
    """ObstaclesHard with a lava slab and the exit pad in view: both classes among the compared pixels, at every size"""
    og = oracle_lib.OracleGym("ObstaclesHard", W, H, sr.OBST_ENVS, 1, 1)
    og.seed(sr.OBST_SEED); og.reset()
    e = sr.pose_obstacles(og, [og])
    want, m, _ = check_box_pose(og, e, W, H, f"ObstaclesHard {W}x{H}")
    seen = set((want[m] >> 12).tolist())
    assert {K["EXIT"], K["LAVA"]} <= seen, f"classes among the compared pixels: {sorted(seen)}"
    og.close()


@pytest.mark.parametrize("W,H", dr.SIZES)
def test_box_scene_conditions_football(W, H):
    """(ii) Football's ball in front of the agent: the restated draw list says BALL wherever the float64 sphere is hit inside 0.8 of its projected radius"""
    og = oracle_lib.OracleGym("Football", W, H, 4, 2, 1)
    og.seed(dr.EMPTY_SEED); og.reset()
    e, centre, radius = dr.pose_football([og])
    snap = og.snapshot(e)
    a = snap["agents"][0]
    eye, C = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, share = dr.cast_sphere(eye, C, W, H, centre, radius)
    inside = np.isfinite(t) & (share <= 0.8)
    want, interior = sr.expected(og, snap, e, 0)
    assert inside.sum() >= 4 and (want[inside] == sr.word(K["BALL"], 0)).all()
    assert interior.mean() >= sr.INTERIOR_SHARE
    og.close()


def test_face_to_face_scene_conditions():
    """TowerBuilding, two agents face to face, a box in the other's hands: AGENT and HUD of agent 1 and CARRIED are in agent 0's view, MOVABLE elsewhere"""
    W, H = 128, 128
    og = oracle_lib.OracleGym("TowerBuilding", W, H, 4, 2, 1)
    og.seed(3); og.reset()
    sr.pose_face_to_face([og], og.snapshot(0), carried=0)
    snap = og.snapshot(0)
    assert int(snap["objects"][0][3]) == 2
    want, interior = sr.expected(og, snap, 0, 0)
    assert interior.mean() >= sr.INTERIOR_SHARE
    seen = set(want[interior].tolist())
    assert {sr.word(K["AGENT"], 1), sr.word(K["CARRIED"], 0)} <= seen, sorted(seen)
    assert sr.word(K["HUD"], 0) in set(want.ravel().tolist())     # the viewer's own time bar: a row three thousandths high, seldom interior
    assert sr.word(K["AGENT"], 0) not in set(want.ravel().tolist())   # no agent sees itself
    og.close()


def test_hud_row_hand_derived_on_the_model():
    """the viewer's own time bar at 128 x 128: the restated draw list says HUD / 0 at the hand-derived pixels and nowhere that is surely outside them"""
    W, H = 128, 128
    og = oracle_lib.OracleGym("TowerBuilding", W, H, 4, 1, 1)
    og.seed(3); og.reset()
    for e in range(4):
        snap = og.snapshot(e)
        inside, outside = sr.hud_pixels(float(snap["bar_half_width"]), W, H)
        assert inside.sum() >= 8, "the bar covers too few pixels to test"
        want, _ = sr.expected(og, snap, e, 0)
        hud = want == sr.word(K["HUD"], 0)
        assert hud[inside].all() and not hud[outside].any()
    og.close()


@pytest.mark.parametrize("scenario,A", pr.MATRIX)
def test_draw_list_restated_and_interior_share(scenario, A):
    """(iii) on the oracle alone, on the state the GPU test uses (pixel_reference's seed and script): prim_words' list has the oracle's entries, every class
    is admitted by its entry's (kind, frame); the frames compared are those of which 80 % is interior, at least half of them"""
    W, H = 128, 128
    N = pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    og.seed(pr.SEED); og.reset()
    for tick in range(12):
        pr.step_oracle(og, N, A, tick)
    chosen = sr.compared_frames(og, N, A)
    assert len(chosen) >= N * A // 2, f"{scenario}: only {len(chosen)} of {N * A} frames are 80 % interior"
    seen = sr.classes_in(chosen)
    print(f"{scenario}: {len(chosen)} of {N * A} frames compared, classes in view {sorted(seen)}")
    assert sr.MATRIX_CLASSES[scenario] <= seen, f"{scenario}: the compared frames no longer show {sorted(sr.MATRIX_CLASSES[scenario] - seen)}"
    og.close()


def test_every_class_is_compared_somewhere():
    """the scenes of the GPU tests, taken together, name every class of the table"""
    named = set().union(*sr.MATRIX_CLASSES.values()) | {"TARGET", "CARRIED"}   # (the Rearrange scene below and the face-to-face scene)
    assert named == set(K) - {"NONE"}


def test_rearrange_carried_scene_conditions():
    """Rearrange: a capsule item picked up by agent 1 through INTERACT -- CARRIED / 0 as a scaled shape in agent 1's camera frame from agent 0's view, MOVABLE
    instances on the right pedestal, TARGET instances on the left one from agent 2's view"""
    og = oracle_lib.OracleGym("Rearrange", 128, 128, sr.REARRANGE_ENVS, sr.REARRANGE_AGENTS, 1)
    og.seed(sr.REARRANGE_SEED); og.reset()
    e = sr.pose_rearrange_carried(og, [og])
    sr.rearrange_scene_expected(og, og.snapshot(e), e)
    og.close()
