"""A float64 numpy model of a frame from ANY camera -- what an overview frame (mv_set_overview / mv_draw_overview) must show -- built on the closed forms the
other references already state and never on a kernel's output: depth_reference.camera64 / rays64 / cast_boxes / cast_sphere for the geometry,
canonical_frames.phong / TAN / LIGHT for the shading.

Camera (include/megaverse_hip.h: mv_camera).  FREE: eye and basis from the record.  AGENT k: camera64 of agent k's pose -- eye 0.05 + 0.41 above the capsule
centre, columns right / up / back, pitch about the local x axis --, the record's offset added as C . offset.  Projection and clip range are the agents':
rays through the pixel centres with tan 50 deg horizontally at aspect 128 / 72 whatever the frame size, hits kept in [0.01, 120]; the light is (0, 4, 2) in
the camera's own space.

Drawables come from a snapshot record (oracle_lib.SNAP), for the scenarios whose drawables are boxes, capsules and the ball, in the order the reference
emits them (magnum_env_renderer.cpp:158-340), which is also the tie order -- nearest t, then the earlier drawable:
  Empty          the layout's opaque boxes (floor colour for slot 0, wall colour otherwise) | 3 per agent
  TowerBuilding  ... | the building zone's slab, 0.05 thick on the floor, 0x555555 | the movable objects: resting, cubes of half extent 0.39 around their
                 voxel's centre; carried, cubes of 0.39 x 0.78 at (0, -0.74, -1) in the carrying agent's camera frame; 0xadd8e6 | 3 per agent
  Football       the room's world boxes (HexRec records) | the ball, a sphere | 3 per agent
Per agent: the capsule (radius 0.35, half length 0.36, centre 0.05 + 0.09 above the state's position, the agent's colour), the eyes box (0.5 x 0.24 x 0.4 at
z = -0.19 of the agent's camera frame, 0x2c3e50) and the time bar (2 bar_half_width x 0.003 x 0.002 at (0, -0.131, -0.2) of that frame, 0x2eb5d0).  `hide`: the
agent whose capsule and eyes box are left out -- the first-person rule.  Only front faces are hit, as with back-face culling: a capsule's or a sphere's nearer
root, a box's entry face.

judge() is the acceptance rule.  A pixel whose 3 x 3 neighbourhood (clipped to the frame) has ONE winner in the model is interior and must be within 1 of 255
per channel; any other pixel must be within 1 of the background or of the colour of some winner of its neighbourhood -- evaluated at this pixel where that
drawable is hit by this pixel's ray, and at the neighbouring pixel where it wins.  Pixels of curved drawables (capsule, ball) that miss -- interior ones whose
winner is curved, and edge pixels with a curved winner in their neighbourhood -- are counted as `excused`, for the caller to hold under pixel_reference.CAP:
the fp32 arithmetic under test is ill-conditioned there and there alone (pixel_reference's header: the discriminant B B - A C cancels, x^300 multiplies the
normal's error; seen on the CPU oracle: one capsule-highlight pixel of 32768, TowerBuilding 64 x 64 after reset, blue 223 against 234).  Boxes get no excuse.

CASES: the interior share of a frame set (all envs, and all agents for the first-person views) must be at least depth_reference.INTERIOR_SHARE, and in the
look_at and chase poses agent 0's own capsule must win at least OWN_PIXELS pixels in EVERY env.  Both are conditions on the MODEL alone, so the seeds and
ticks (after reset: 0; after 40 scripted ticks: 40) were picked with it, on snapshots of the CPU oracle: per scenario, size and pose the first seed of
pixel_reference.SEED, 1, 2, ... that meets them (small frames leave few interior pixels: at 48 x 20 most seeds fall short of 0.8).
tests/test_overview_reference.py asserts the conditions for every entry; tests/test_overview_gpu.py draws exactly these."""
import numpy as np

import depth_reference as dr
from canonical_frames import phong

SCENARIOS = [("Empty", 1), ("TowerBuilding", 2), ("Football", 2)]
SCN_TOWER, SCN_EMPTY, SCN_FOOTBALL = 0, 5, 9
AGENT_COLORS = (0xffdd3c, 0x3bb372, 0x2eb5d0, 0xffb400, 0xd468ee, 0x222222, 0xff0000)
OBJ_HALF, CARRY_SCALE, CARRY_AT = 0.39, 0.78, (0.0, -0.44 + -0.3, -1.0)
CAPSULE_R, CAPSULE_HL, CAPSULE_UP = 0.35, 0.36, 0.09
EYES_LO, EYES_HI, EYES_COLOR = (-0.25, -0.12, -0.19 - 0.2), (0.25, 0.12, -0.19 + 0.2), 0x2c3e50
BAR_COLOR = 0x2eb5d0
HEX_SPHERE = 2
BOX, CAPSULE, SPHERE = "box", "capsule", "sphere"
OWN_PIXELS = 20
N_ENVS = 4
POSES = ("default", "look_at", "chase")
# (scenario, (W, H)) -> {"first_person": seed (both ticks), pose: (seed, ticks)}
CASES = {
    ("Empty", (64, 64)): {"first_person": 11, "default": (11, 0), "look_at": (11, 0), "chase": (11, 0)},
    ("TowerBuilding", (64, 64)): {"first_person": 11, "default": (11, 0), "look_at": (11, 0), "chase": (11, 40)},
    ("Football", (64, 64)): {"first_person": 11, "default": (11, 0), "look_at": (11, 0), "chase": (11, 0)},
    ("Empty", (48, 20)): {"first_person": 11, "default": (11, 0), "look_at": (2, 0), "chase": (11, 0)},
    ("TowerBuilding", (48, 20)): {"first_person": 1, "default": (1, 0), "look_at": (71, 40), "chase": (1, 0)},
    ("Football", (48, 20)): {"first_person": 1, "default": (3, 0), "look_at": (21, 40), "chase": (13, 40)},
}


def pose(snap, name):
    """the three poses of the free-camera tests as camera records: the default pose; a look_at from agent 0's position + (-2, 2, -2) at agent 0; a chase
    camera 2 behind and 1 above agent 0"""
    from megaverse_amd import follow, look_at, overview_default_camera
    p0 = np.asarray(snap["agents"][0]["pos"], np.float32)
    return {"default": lambda: overview_default_camera(), "look_at": lambda: look_at(p0 + np.array([-2, 2, -2], np.float32), p0),
            "chase": lambda: follow(0, back=2.0, up=1.0)}[name]()


def camera_of(snap, cam):
    """one CAMERA_DTYPE record -> (eye [3], C [3, 3] float64, hide: the agent whose body is not drawn or -1)"""
    agent, off = int(cam["agent"]), np.asarray(cam["eye"], np.float64)
    if agent < 0:
        return off.copy(), np.asarray(cam["c"], np.float64).reshape(3, 3), -1
    a = snap["agents"][agent]
    eye, C = dr.camera64(a["pos"], a["basis"], a["pitch"])
    if off.any():
        eye = eye + C @ off
    return eye, C, agent if int(cam["flags"]) & 1 else -1


def drawables(snap, num_agents, hide=-1):
    """-> list of (kind, frame, colour, geometry) in draw order; frame -1: the world, k: agent k's camera frame; geometry: (lo, hi), (centre, r, hl), (centre, r)"""
    scn = int(snap["scenario"])
    out = []
    if scn == SCN_FOOTBALL:
        for b in snap["hex_boxes"][: int(snap["hex_num_boxes"])]:
            assert int(b["meta"]) & 15 == 0, "Football's boxes live in the world frame"
            out.append((BOX, -1, int(b["color"]) & 0xffffff, (np.asarray(b["a"], np.float64), np.asarray(b["b"], np.float64))))
    else:
        assert scn in (SCN_TOWER, SCN_EMPTY), "overview_reference models Empty, TowerBuilding and Football"
        for b in np.asarray(snap["boxes"][: int(snap["num_boxes"])]):
            if int(b[6]) & 2:
                out.append((BOX, -1, int(snap["layout_color"] if int(b[7]) == 0 else snap["wall_color"]) & 0xffffff, (b[0:3].astype(np.float64), b[3:6].astype(np.float64))))
    if scn == SCN_TOWER:
        bz = [float(v) for v in snap["bz"]]
        out.append((BOX, -1, 0x555555, (np.array([bz[0], 1.0, bz[2]]), np.array([bz[1], 1.0 + 0.05, bz[3]]))))
    else:
        assert int(snap["num_terrain"]) == 0 or scn == SCN_FOOTBALL, "no terrain slabs in the modelled scenarios"
    if scn == SCN_TOWER:
        for o in snap["objects"][: int(snap["num_objects"])]:
            state = int(o[3])
            if state <= 0:
                c = np.array([int(o[0]) + 0.5, int(o[1]) + 0.5, int(o[2]) + 0.5])
                out.append((BOX, -1, 0xadd8e6, (c - OBJ_HALF, c + OBJ_HALF)))
            else:
                c, hh = np.array(CARRY_AT), OBJ_HALF * CARRY_SCALE
                out.append((BOX, state - 1, 0xadd8e6, (c - hh, c + hh)))
    else:
        assert int(snap["num_objects"]) == 0, "no movable objects in Empty and Football"
    if scn == SCN_FOOTBALL:
        for o in snap["hex_objs"][: int(snap["hex_num_objs"])]:
            assert int(o["meta"]) & 15 == HEX_SPHERE and float(o["b"][0]) == float(o["b"][1]) == float(o["b"][2]), "Football's one collectable record is the ball"
            out.append((SPHERE, -1, int(o["color"]) & 0xffffff, (np.asarray(o["a"], np.float64), float(o["b"][0]))))
    else:
        assert int(snap["num_rewards"]) == 0, "no diamonds in Empty and TowerBuilding"
    bw = float(snap["bar_half_width"])
    for k in range(num_agents):
        a = snap["agents"][k]
        x, y, z = (float(v) for v in a["pos"])
        if k != hide:
            out.append((CAPSULE, -1, AGENT_COLORS[k % 7], (np.array([x, (y + 0.05) + CAPSULE_UP, z]), CAPSULE_R, CAPSULE_HL)))
            out.append((BOX, k, EYES_COLOR, (np.array(EYES_LO), np.array(EYES_HI))))
        out.append((BOX, k, BAR_COLOR, (np.array([-bw, -0.131 - 0.0015, -0.2 - 0.001]), np.array([bw, -0.131 + 0.0015, -0.2 + 0.001]))))
    return out


def capsule_id(snap, agent, num_agents, hide=-1):
    """the index of agent `agent`'s capsule in drawables(snap, num_agents, hide)"""
    caps = [i for i, d in enumerate(drawables(snap, num_agents, hide)) if d[0] == CAPSULE]
    return caps[[k for k in range(num_agents) if k != hide].index(agent)]


def cast_capsule(eye, C, W, H, centre, r, hl):
    """front faces of an upright capsule: the cylinder's nearer root where it lands between the end planes, each end sphere's nearer root where it lands on
    the outer hemisphere; the nearest of those inside the clip range -> (t [H, W], inf: miss; n [H, W, 3] world-space unit normal)"""
    dw = dr.rays64(W, H) @ C.T
    o = eye - centre
    t = np.full((H, W), np.inf); n = np.zeros((H, W, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        A = dw[..., 0] ** 2 + dw[..., 2] ** 2
        B = o[0] * dw[..., 0] + o[2] * dw[..., 2]
        Cc = o[0] ** 2 + o[2] ** 2 - r * r
        disc = B * B - A * Cc
        tc = np.where((disc >= 0) & (A > 0), (-B - np.sqrt(np.maximum(disc, 0))) / A, np.inf)
        y = o[1] + tc * dw[..., 1]
        ok = (tc >= dr.NEAR_Z) & (tc <= dr.FAR_Z) & (y >= -hl) & (y <= hl)
        t[ok] = tc[ok]
        p = o + tc[..., None] * dw
        n[ok] = (p * np.array([1.0, 0.0, 1.0]) / r)[ok]
        for s in (-1.0, 1.0):
            os_ = o - np.array([0.0, s * hl, 0.0])
            A3 = (dw * dw).sum(-1); B3 = dw @ os_; C3 = os_ @ os_ - r * r
            disc = B3 * B3 - A3 * C3
            ts = np.where(disc >= 0, (-B3 - np.sqrt(np.maximum(disc, 0))) / A3, np.inf)
            p = os_ + ts[..., None] * dw
            ok = (ts >= dr.NEAR_Z) & (ts <= dr.FAR_Z) & (s * p[..., 1] >= 0) & (ts < t)
            t[ok] = ts[ok]; n[ok] = (p / r)[ok]
    return t, n


class Frame:
    """what render() returns: rgba [H, W, 4] uint8, winner [H, W] (index into `table`, -1: background), and per drawable its own depth and camera-space
    normal maps (T [n, H, W], inf: not hit; N [n, H, W, 3]) with which judge() evaluates a neighbour's drawable at this pixel"""

    def __init__(self, table, T, N, dc):
        self.table, self.T, self.N, self.dc = table, T, N, dc
        n, H, W = T.shape
        best = T.argmin(0) if n else np.zeros((H, W), int)   # (the first minimum: the earlier drawable on a tie)
        hit = np.isfinite(T.min(0)) if n else np.zeros((H, W), bool)
        self.winner = np.where(hit, best, -1)
        self.rgba = np.zeros((H, W, 4), np.uint8); self.rgba[..., 3] = 255
        for y, x in zip(*np.nonzero(hit)):
            self.rgba[y, x] = self.colour(int(self.winner[y, x]), y, x)

    def colour(self, d, y, x):
        """drawable d's shaded colour at pixel (x, y), where this pixel's ray hits it"""
        return phong(self.dc[y, x] * self.T[d, y, x], self.N[d, y, x], self.table[d][2])

    def curved(self, d):
        return self.table[d][0] != BOX


def render(snap, cam, W, H, num_agents):
    """the frame of one env from one camera record -> Frame"""
    eye, C, hide = camera_of(snap, cam)
    table = drawables(snap, num_agents, hide)
    dc = dr.rays64(W, H)
    T = np.full((len(table), H, W), np.inf); N = np.zeros((len(table), H, W, 3))
    frames = {}
    for k in range(num_agents):
        a = snap["agents"][k]
        frames[k] = dr.camera64(a["pos"], a["basis"], a["pitch"])
    for i, (kind, fr, _, geo) in enumerate(table):
        if kind == BOX:
            if fr < 0:
                e, Cf = eye, C
            else:   # the camera expressed in agent fr's camera frame
                ek, Ck = frames[fr]
                e, Cf = Ck.T @ (eye - ek), Ck.T @ C
            t, box, axis, dwk = dr.cast_boxes(e, Cf, W, H, geo[0][None], geo[1][None])
            n = np.zeros((H, W, 3))
            n[np.arange(H)[:, None], np.arange(W)[None, :], axis] = np.where(dwk > 0, -1.0, 1.0)
            T[i] = np.where(box >= 0, t, np.inf); N[i] = n @ Cf   # (row vectors: n Cf = (Cf^T n)^T, the normal in the viewing camera's axes)
        elif kind == CAPSULE:
            t, n = cast_capsule(eye, C, W, H, *geo)
            T[i] = t; N[i] = n @ C
        else:
            centre, r = geo
            t, _ = dr.cast_sphere(eye, C, W, H, centre, r)
            dw = dc @ C.T
            with np.errstate(invalid="ignore"):
                p = eye + np.where(np.isfinite(t), t, 0.0)[..., None] * dw
            T[i] = t; N[i] = ((p - centre) / r) @ C
    return Frame(table, T, N, dc)


class Judgement:
    def __init__(self):
        self.interior, self.excused, self.failures = 0, 0, []


def judge(got, model):
    """got [H, W, 4] uint8 against the model's frame under the rule of the module's header -> Judgement (interior: pixels with one winner in their 3 x 3;
    excused: curved interior pixels outside 1 / 255; failures: (x, y, got, want) of every pixel that breaks the rule)"""
    H, W = model.winner.shape
    assert got.shape == (H, W, 4) and got.dtype == np.uint8
    out = Judgement()
    assert (got[..., 3] == 255).all(), "alpha"
    interior = dr.uniform3x3(model.winner)
    out.interior = int(interior.sum())
    d = np.abs(got[..., :3].astype(np.int16) - model.rgba[..., :3].astype(np.int16)).max(-1)
    for y, x in zip(*np.nonzero(d > 1)):
        px = got[y, x, :3].astype(np.int16)
        w = int(model.winner[y, x])
        if interior[y, x]:
            if w >= 0 and model.curved(w):
                out.excused += 1
            else:
                out.failures.append((int(x), int(y), px.tolist(), model.rgba[y, x, :3].tolist()))
            continue
        cands, curved = [[0, 0, 0]], False
        for yy in range(max(0, y - 1), min(H, y + 2)):
            for xx in range(max(0, x - 1), min(W, x + 2)):
                s = int(model.winner[yy, xx])
                if s < 0:
                    continue
                curved = curved or model.curved(s)
                cands.append(model.rgba[yy, xx, :3].tolist())
                if np.isfinite(model.T[s, y, x]):
                    cands.append(model.colour(s, y, x)[:3])
        if (np.abs(np.asarray(cands, np.int16) - px).max(-1) <= 1).any():
            continue
        if curved:
            out.excused += 1
        else:
            out.failures.append((int(x), int(y), px.tolist(), model.rgba[y, x, :3].tolist()))
    return out
