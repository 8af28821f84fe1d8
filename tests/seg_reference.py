"""What a label plane (mv_set_seg_obs) must hold, from float64 geometry and the snapshot's records -- never read off a kernel.

The label of a pixel names the drawable of its nearest hit: class << 12 | instance (megaverse_amd/csrc/mv_seg_obs.h has the table; restated here as CLASSES
and in the functions below, independently of the header's code).  Three models:
  (i)  box_scene: depth_reference's float64 ray / AABB caster over the world boxes of a snapshot.  seg_world_boxes lists them WITH the word each must carry:
       an opaque layout box's original index and its `slot` field give FLOOR / STRUCTURE, then TowerBuilding's building zone, then Obstacles' terrain slabs
       (EXIT / LAVA by their type), then the objects resting in the world by object index.  runner_up_margin gives, per pixel, how far (relative) the second
       nearest box lies behind the winner: the CPU test asserts that no interior pixel of a pose used has a runner-up within pixel_reference's EPS_4ULP, which
       is what lets the GPU test demand equality there.
  (ii) Football's ball: depth_reference.cast_sphere, BALL inside 0.8 of the projected radius.
  (iii) every scenario: the float64 oracle's `prim` map (OracleGym.render_f64) indexes the frame's draw list, which the oracle emits in the order the reference
       emits drawables and skipping what is not drawn.  prim_words walks the snapshot's records in that order and gives every list entry its word; the list's
       (kind, frame) rows (prim_table) must admit each word's class (ADMITS: a world capsule is AGENT, a cone is COLLECTABLE or HAZARD, a box in camera frame k
       is AGENT, HUD or CARRIED, a scaled shape is TARGET, MOVABLE, CARRIED, COLLECTABLE or BALL, a world box is any of the box classes), and the entry counts
       must agree -- check_against_table.

Compared pixels (judge): INTERIOR pixels -- depth_reference.uniform3x3 on the float64 prim map -- must hold the expected word exactly; every other pixel must
hold a word that occurs in its 3 x 3 neighbourhood of the expected map (a silhouette may fall on either side of a pixel centre in float32).  Condition, asserted
on the CPU on the oracle alone for every pose used: at least INTERIOR_SHARE of every compared frame is interior."""
import numpy as np

import depth_reference as dr
from canonical_frames import BOX_HALF

INTERIOR_SHARE = dr.INTERIOR_SHARE
CLASSES = {"NONE": 0, "FLOOR": 1, "STRUCTURE": 2, "EXIT": 3, "LAVA": 4, "BUILDING_ZONE": 5, "FURNITURE": 6, "TARGET": 7, "MOVABLE": 8, "CARRIED": 9,
           "COLLECTABLE": 10, "HAZARD": 11, "BALL": 12, "AGENT": 13, "HUD": 14}
K = CLASSES
SCN = {"TowerBuilding": 0, "Obstacles": 1, "Collect": 2, "Rearrange": 3, "Sokoban": 4, "Empty": 5, "HexMemory": 6, "HexExplore": 7, "BoxAGone": 8, "Football": 9}
HEX_LIKE = (6, 7, 8, 9)
NUM_STATIC = 9
VX_OPAQUE, TERRAIN_EXIT, SOKO_WALL, SOKO_GOAL, SOKO_DIM = 2, 1, 1, 2, 32
HEX_PILLAR, HEX_DIAMOND, HEX_SPHERE = 0, 1, 2
MAX_AGENTS = 8
# oracle prim_table kinds (oracle/mv_oracle.cpp build_prims): 1 box, 2 capsule, 3 cone, 4 / 5 / 6 scaled sphere / capsule / cylinder
BOX_CLASSES = {K["FLOOR"], K["STRUCTURE"], K["EXIT"], K["LAVA"], K["BUILDING_ZONE"], K["FURNITURE"], K["TARGET"], K["MOVABLE"]}


def word(cls, instance):
    return 0 if cls == 0 else (cls << 12) | instance


def split(words):
    w = np.asarray(words).astype(np.uint16)
    return (w >> 12).astype(np.uint8), (w & 4095).astype(np.int32)


def admits(kind, frame, viewer):
    """the classes a draw-list entry of (kind, frame) may carry; frame < 0: the world, 0 .. 7: agent k's camera, 8 ..: a Hex wall orientation"""
    if kind == 2:
        return {K["AGENT"]}
    if kind == 3:
        return {K["COLLECTABLE"], K["HAZARD"]}
    if kind == 1 and 0 <= frame < MAX_AGENTS:
        return {K["AGENT"], K["HUD"], K["CARRIED"]}
    if kind == 1 and frame >= MAX_AGENTS:
        return {K["STRUCTURE"]}
    if kind == 1:
        return BOX_CLASSES
    if 0 <= frame < MAX_AGENTS:
        return {K["CARRIED"]}
    return {K["TARGET"], K["MOVABLE"], K["COLLECTABLE"], K["BALL"]}


def prim_words(snap, viewer):
    """(iii) the word of every entry of the oracle's draw list for `viewer`, in the list's order, from the snapshot's records"""
    scen = int(snap["scenario"])
    A = int(snap["num_agents"])
    out = []
    if scen not in HEX_LIKE:
        for i in range(int(snap["num_boxes"])):
            b = snap["boxes"][i]
            if int(b[6]) & VX_OPAQUE:
                out.append(word(K["FLOOR"] if int(b[7]) == 0 else K["STRUCTURE"], i))
    if scen == SCN["Sokoban"]:
        L, Wr = int(snap["L"]), max(int(snap["W"]), 1)
        for x in range(L):
            for z in range(Wr):
                t = int(snap["soko"][x * SOKO_DIM + z])
                if t:
                    out.append(word(K["FURNITURE"] if t == SOKO_WALL else K["EXIT"], x * Wr + z))
        out += [word(K["MOVABLE"], i) for i in range(int(snap["num_objects"]))]
    if scen in HEX_LIKE:
        out += [word(K["STRUCTURE"], i) for i in range(int(snap["hex_num_boxes"]))]
        for j in range(int(snap["hex_num_objs"])):
            shape = int(snap["hex_objs"][j]["meta"]) & 15
            parts = 1 if shape == HEX_SPHERE else 3 if shape == HEX_PILLAR else 2
            out += [word(K["BALL"] if scen == SCN["Football"] else K["COLLECTABLE"], j)] * parts
    if scen == SCN["TowerBuilding"]:
        out.append(word(K["BUILDING_ZONE"], 0))
    if scen not in HEX_LIKE and scen not in (SCN["Rearrange"], SCN["Sokoban"], SCN["TowerBuilding"]):
        for i in range(int(snap["num_terrain"])):
            out.append(word(K["EXIT"] if int(snap["terrain"][i][6]) == TERRAIN_EXIT else K["LAVA"], i))
    if scen == SCN["Rearrange"]:
        out += [word(K["FURNITURE"], i) for i in range(NUM_STATIC)]
        out += [word(K["TARGET"], i) for i in range(int(snap["num_items"]))]
        out += [word(K["CARRIED"] if int(snap["objects"][i][3]) > 0 else K["MOVABLE"], i) for i in range(int(snap["num_items"]))]
    if scen not in (SCN["Rearrange"], SCN["Sokoban"]):
        out += [word(K["CARRIED"] if int(snap["objects"][i][3]) > 0 else K["MOVABLE"], i) for i in range(int(snap["num_objects"]))]
    if scen not in HEX_LIKE:
        for i in range(int(snap["num_rewards"])):
            active = int(snap["rewards"][i][3])
            if active:
                out += [word(K["HAZARD"] if scen == SCN["Collect"] and active == 2 else K["COLLECTABLE"], i)] * 2
    for k in range(A):
        if k != viewer:
            out += [word(K["AGENT"], k)] * 2
        out.append(word(K["HUD"], k))
    return np.asarray(out, np.uint16)


def check_against_table(words, table, viewer):
    """the restated list against the oracle's own: the same number of entries, every entry's class admitted by its (kind, frame)"""
    assert len(words) == len(table), f"the restated draw list has {len(words)} entries, the oracle's {len(table)}"
    for p in range(len(table)):
        cls = int(words[p]) >> 12
        assert cls in admits(int(table[p, 0]), int(table[p, 1]), viewer), f"entry {p}: class {cls} on kind {int(table[p, 0])} frame {int(table[p, 1])}"


def label_map(prim, words):
    """the expected plane of words: words[prim], 0 where the float64 ray hits nothing"""
    w = np.concatenate([np.asarray(words, np.uint16), np.zeros(1, np.uint16)])
    return w[np.where(prim >= 0, prim, len(words))]


def expected(og, snap, env, viewer):
    """(iii) -> (want [H, W] uint16, interior [H, W] bool) of the oracle gym's present state"""
    _, prim = og.render_f64(env, viewer)
    words = prim_words(snap, viewer)
    check_against_table(words, og.prim_table(env, viewer), viewer)
    return label_map(prim, words), dr.uniform3x3(prim)


def neighbourhood_has(want, got):
    """per pixel: got occurs in the 3 x 3 neighbourhood (clipped to the frame) of want"""
    H, W = want.shape
    p = np.pad(want, 1, mode="edge")
    ok = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            ok |= p[dy:H + dy, dx:W + dx] == got
    return ok


def judge(got, want, interior, what="", class_only=False):
    """the comparison: equality at interior pixels, membership of the neighbourhood elsewhere; class_only: got is a plane of class bytes"""
    got = np.asarray(got).astype(np.uint16)
    if class_only:
        want = (want >> 12).astype(np.uint16)
    bad = interior & (got != want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} interior pixels hold another label, first at (row, col) {np.argwhere(bad)[0].tolist()}: "
                           f"got {int(got[tuple(np.argwhere(bad)[0])])}, expected {int(want[tuple(np.argwhere(bad)[0])])}")
    edge = ~interior & ~neighbourhood_has(want, got)
    assert not edge.any(), f"{what}: {int(edge.sum())} silhouette pixels hold a label no neighbour shows, first at {np.argwhere(edge)[0].tolist()}"


# ---- (i) the box scenes ------------------------------------------------------------------------------------------------------------------------------
def seg_world_boxes(snap):
    """depth_reference.world_boxes' list (opaque layout boxes, TowerBuilding's zone, resting objects) with Obstacles' terrain slabs appended
    -> (lo [n, 3], hi [n, 3], words [n])"""
    scen = int(snap["scenario"])
    lo, hi = dr.world_boxes(snap)
    words = []
    for i in range(int(snap["num_boxes"])):
        b = snap["boxes"][i]
        if int(b[6]) & VX_OPAQUE:
            words.append(word(K["FLOOR"] if int(b[7]) == 0 else K["STRUCTURE"], i))
    if scen == SCN["TowerBuilding"]:
        words.append(word(K["BUILDING_ZONE"], 0))
    words += [word(K["MOVABLE"], i) for i in range(int(snap["num_objects"])) if int(snap["objects"][i][3]) == 0]
    assert len(words) == len(lo)
    if scen in (SCN["Obstacles"], SCN["Empty"]):
        t = np.asarray(snap["terrain"][: int(snap["num_terrain"])]).astype(np.float64).reshape(-1, 8)
        if len(t):
            tlo, thi = t[:, 0:3].copy(), t[:, 3:6].copy()
            thi[:, 1] = tlo[:, 1] + 0.05   # a 0.05-thick slab on the terrain box's floor (layout_utils.cpp:53-68)
            lo, hi = np.concatenate([lo, tlo]), np.concatenate([hi, thi])
            words += [word(K["EXIT"] if int(r[6]) == TERRAIN_EXIT else K["LAVA"], i) for i, r in enumerate(t)]
    return lo, hi, np.asarray(words, np.uint16)


def box_scene(snap, agent, W, H):
    """(i) -> (want [H, W] uint16: the word of the nearest world box, 0 for a miss; margin [H, W]: the runner-up's relative distance behind the winner, inf
    with none; hit [H, W])"""
    a = snap["agents"][agent]
    lo, hi, words = seg_world_boxes(snap)
    eye, C = dr.camera64(a["pos"], a["basis"], a["pitch"])
    t, box, _, _ = dr.cast_boxes(eye, C, W, H, lo, hi)
    want = np.where(box >= 0, words[np.maximum(box, 0)], 0).astype(np.uint16)
    # the runner-up: the nearest entry among the OTHER boxes
    dw = dr.rays64(W, H) @ C.T
    second = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dw
        for i in range(len(lo)):
            t1, t2 = (lo[i] - eye) * inv, (hi[i] - eye) * inv
            te, tx = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
            ok = (te <= tx) & (te >= dr.NEAR_Z) & (te <= dr.FAR_Z) & (box != i)
            second = np.where(ok & (te < second), te, second)
        margin = np.where(np.isfinite(t), (second - t) / t, np.inf)
    return want, margin, np.isfinite(t)


def world_box_interior(og, env, agent):
    """the compared pixels of (i): interior, and showing a world box or background alone"""
    _, prim = og.render_f64(env, agent)
    table = og.prim_table(env, agent)
    return dr.interior_mask(prim, table, dr.is_world_box) | dr.background_mask(prim), prim


OBST_ENVS, OBST_SEED, OBST_ENV, OBST_YAW, OBST_PITCH = 8, 3, 3, 5 * np.pi / 4, -0.4


def pose_obstacles(og, gyms):
    """ObstaclesHard, seed OBST_SEED, env OBST_ENV: the agent stands on the middle of the exit pad, turned by OBST_YAW and pitched down by OBST_PITCH, from
    where the pad under it and a lava slab further on are both in view (found by a search over the terrain boxes, eight yaws and three pitches on the oracle
    alone; tests/test_seg_obs.py asserts the conditions for it) -> env"""
    from canonical_frames import REST_Y
    snap = og.snapshot(OBST_ENV)
    pads = [snap["terrain"][i] for i in range(int(snap["num_terrain"])) if int(snap["terrain"][i][6]) == TERRAIN_EXIT]
    assert pads, "the env has no exit pad"
    t = pads[0]
    x, y, z = (int(t[0]) + int(t[3])) / 2.0, float(t[1]) + (REST_Y - 1.0), (int(t[2]) + int(t[5])) / 2.0
    c, s = float(np.float32(np.cos(OBST_YAW))), float(np.float32(np.sin(OBST_YAW)))
    for g in gyms:
        g.debug_set_agent_pos(OBST_ENV, 0, x, y, z)
        g.debug_set_agent_yaw(OBST_ENV, 0, c, s)
        g.debug_set_agent_velocity(OBST_ENV, 0, 0.0, 0.0, 0.0)
        g.debug_set_agent_pitch(OBST_ENV, 0, OBST_PITCH)
    return OBST_ENV


# The classes that the compared frames of the seeded, scripted state of every scenario of pixel_reference.MATRIX must show (128 x 128, pixel_reference's seed,
# twelve scripted ticks): stated here so that a changed seed or script cannot silently empty the per-scenario tests.  Found on the oracle alone.
MATRIX_CLASSES = {
    "TowerBuilding": {"FLOOR", "STRUCTURE", "BUILDING_ZONE", "MOVABLE", "AGENT", "HUD"},
    "ObstaclesHard": {"FLOOR", "STRUCTURE", "EXIT", "LAVA", "MOVABLE", "COLLECTABLE", "AGENT", "HUD"},
    "Collect": {"FLOOR", "STRUCTURE", "MOVABLE", "COLLECTABLE", "HAZARD", "AGENT", "HUD"},
    "Rearrange": {"FLOOR", "FURNITURE", "MOVABLE", "AGENT", "HUD"},
    "HexMemory": {"STRUCTURE", "COLLECTABLE", "AGENT", "HUD"},
    "Sokoban": {"FLOOR", "EXIT", "FURNITURE", "MOVABLE", "HUD"},
    "BoxAGone": {"STRUCTURE", "HUD"},
    "Football": {"STRUCTURE", "BALL", "AGENT", "HUD"},
}


def classes_in(frames_):
    """the class names among the words of compared_frames' frames"""
    names = {v: k for k, v in CLASSES.items()}
    return {names[int(c)] for _, _, want, _ in frames_ for c in np.unique(want >> 12)} - {"NONE"}


def compared_frames(og, n_envs, n_agents):
    """(iii) the frames of the oracle gym's present state that meet the 80 % condition -> [(env, agent, want, interior)]: chosen on the oracle alone"""
    out = []
    for e in range(n_envs):
        snap = og.snapshot(e)
        for a in range(n_agents):
            want, interior = expected(og, snap, e, a)
            if interior.mean() >= INTERIOR_SHARE:
                out.append((e, a, want, interior))
    return out


def pose_face_to_face(gyms, snap0, carried=None):
    """env 0 of a gym with two agents: agent 1 two units in front of agent 0, each turned towards the other; carried: the index of a movable box put into
    agent 1's hands (TowerBuilding: debug_set_objects) -> from agent 0 the other's capsule, eye box and time bar -- and the carried box -- are in view"""
    x, y, z = (float(v) for v in snap0["agents"][0]["pos"])
    c, sn = float(np.float32(np.cos(np.pi / 2))), float(np.float32(np.sin(np.pi / 2)))
    for g in gyms:
        g.debug_set_agent_pos(0, 1, x - 2.0, y, z)
        g.debug_set_agent_yaw(0, 0, c, sn)
        g.debug_set_agent_yaw(0, 1, -c, -sn)
        for k in (0, 1):
            g.debug_set_agent_velocity(0, k, 0.0, 0.0, 0.0)
        if carried is not None:
            objs = np.array(snap0["objects"][: int(snap0["num_objects"])], np.int8).reshape(-1, 4).copy()
            objs[carried, 3] = 2   # 1 + k: in agent 1's hands
            g.debug_set_objects(0, objs)


REARRANGE_ENVS, REARRANGE_AGENTS, REARRANGE_SEED, REARRANGE_ENV = 4, 3, 3, 1   # (env 1: item 0 is a capsule, items 1 and 2 cylinders)
ACT_INTERACT = 1 << 8          # action mask bit (env.hpp:22-42); multi-discrete: the fifth action


def pose_rearrange_carried(og, gyms):
    """Rearrange, three agents, env REARRANGE_ENV: agent 1 is put one unit beside item 0 on the right pedestal, turned towards it and pitched down, and
    INTERACTS for three ticks, after which it carries the item (found by a search over sides, distances and pitches on the oracle alone; the callers assert
    objects[0].state == 2).  Then agent 0 is put three units to the side of the pedestal looking across it -- the carrier, the item hanging in front of the
    carrier's camera and the items left on the pedestal are in its view -- and agent 2 likewise beside the LEFT pedestal, where the target arrangement
    stands.  Every gym gets the same setter calls and the same ticks -> env"""
    e, A, N = REARRANGE_ENV, REARRANGE_AGENTS, REARRANGE_ENVS
    snap = og.snapshot(e)
    o = snap["objects"][0]
    ox, oz = int(o[0]) + 0.5, int(o[2]) + 0.5
    ay = float(snap["agents"][1]["pos"][1])
    masks = np.zeros(N * A, np.int32); masks[e * A + 1] = ACT_INTERACT
    acts = np.zeros((N * A, 6), np.int32); acts[e * A + 1, 4] = 1
    for g in gyms:
        g.debug_set_agent_pos(e, 1, ox - 1.0, ay, oz)
        g.debug_set_agent_yaw(e, 1, 0.0, -1.0)         # looking along +x, at the item
        g.debug_set_agent_velocity(e, 1, 0.0, 0.0, 0.0)
        g.debug_set_agent_pitch(e, 1, -0.5)
        for _ in range(3):
            if hasattr(g, "set_action_masks"):
                g.set_action_masks(masks); g.step_norender()
            else:
                g.set_actions_batched(acts); g.step_no_render()
    ay = float(og.snapshot(e)["agents"][1]["pos"][1])
    for g in gyms:
        for k, x in ((0, ox - 0.5), (2, ox - 0.5 - 8.0)):   # (the pedestals' centres are 8 apart in x: mv_rearrange.h RE_LEFT_X, RE_RIGHT_X)
            g.debug_set_agent_pos(e, k, x, ay, oz + 3.0)
            g.debug_set_agent_yaw(e, k, 1.0, 0.0)      # looking along -z, across the pedestal
            g.debug_set_agent_velocity(e, k, 0.0, 0.0, 0.0)
            g.debug_set_agent_pitch(e, k, -0.3)
    return e


def rearrange_scene_expected(og, snap, env):
    """the Rearrange scene's conditions on the oracle alone -> [(want, interior)] per agent: item 0 is in agent 1's hands and is drawn as a scaled shape or a
    box in agent 1's camera frame; agent 0's interior pixels show CARRIED / 0, AGENT / 1 and at least two MOVABLE instances other than 0; agent 2's show at
    least three TARGET instances; 80 % of each frame is interior"""
    n = int(snap["num_items"])
    assert int(snap["objects"][0][3]) == 2 and n >= 3, "item 0 is not in agent 1's hands"
    out = [expected(og, snap, env, a) for a in range(REARRANGE_AGENTS)]
    for a, (want, interior) in enumerate(out):
        assert interior.mean() >= INTERIOR_SHARE, f"agent {a}: only {interior.mean():.3f} of the frame is interior"
    table = og.prim_table(env, 0)
    words = prim_words(snap, 0)
    carried = [p for p in range(len(words)) if int(words[p]) == word(K["CARRIED"], 0)]
    assert len(carried) == 1 and int(table[carried[0], 1]) == 1 and int(table[carried[0], 0]) >= 4, "the carried item is no scaled shape in agent 1's camera frame"
    seen0 = set(out[0][0][out[0][1]].tolist())
    assert {word(K["CARRIED"], 0), word(K["AGENT"], 1)} <= seen0 and word(K["MOVABLE"], 0) not in seen0, sorted(seen0)
    assert len({w for w in seen0 if w >> 12 == K["MOVABLE"]}) >= 2, sorted(seen0)
    seen2 = set(out[2][0][out[2][1]].tolist())
    assert len({w for w in seen2 if w >> 12 == K["TARGET"]}) >= 3 and all((w & 4095) < n for w in seen2 if w >> 12 == K["TARGET"]), sorted(seen2)
    return out


def hud_pixels(bar_half_width, W, H, slack=1e-3):
    """the viewer's own time bar, derived by hand from its box in the viewer's camera frame (scenario_default.hpp:99-170: x in [-bw, bw], y in -0.131 -+ 0.0015,
    z in -0.2 -+ 0.001) and the ray dc = (x, y, -1) of canonical_frames.ray: the front face z = -0.199 is met at t = 0.199, so a pixel shows the bar where
    0.199 dc_y lies in the bar's y range and 0.199 |dc_x| <= bw -> (inside [H, W]: surely the bar, outside [H, W]: surely not), `slack` away from the edges"""
    from canonical_frames import TAN, TAN_Y
    dcx = (((np.arange(W) + 0.5) / W) * 2 - 1) * TAN
    dcy = (((np.arange(H) + 0.5) / H) * 2 - 1) * TAN_Y
    y = 0.199 * dcy
    rows_in = (y >= -0.1325 + slack * 0.1) & (y <= -0.1295 - slack * 0.1)
    rows_out = (0.199 * dcy < -0.1325 - slack) | (0.201 * dcy > -0.1295 + slack)   # (t dc_y over t in [0.199, 0.201] stays below / above the bar)
    cols_in = 0.199 * np.abs(dcx) <= bar_half_width - slack
    cols_out = 0.199 * np.abs(dcx) >= bar_half_width + slack
    inside = rows_in[:, None] & cols_in[None, :]
    outside = rows_out[:, None] | cols_out[None, :]
    return inside, outside


# ---- planted mistakes (tests/test_seg_obs.py shows that judge rejects each) ---------------------------------------------------------------------------
def planted_rows_flipped(want):
    return want[::-1].copy()


def planted_tile_shift(want, tile=16):
    return np.roll(want, tile, axis=1)


def planted_slot_for_instance(want, prim):
    """the drawable's place in the whole draw list (its slot, where every slot is drawn) in the instance field instead of the index within its class's
    records: right for the layout boxes, which come first, wrong for everything behind them"""
    cls = want >> 12
    return np.where(prim >= 0, (cls << 12) | (prim.astype(np.int64) & 4095), 0).astype(np.uint16)
