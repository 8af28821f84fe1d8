"""Scripted TowerBuilding cases for the stacking rules (tests/tower_model.py judges them), shared by the CPU test of the oracle (test_tower_model.py) and
the GPU tests (test_tower_model_gpu.py).  TEST INFRASTRUCTURE ONLY.

A case drives ONE gym-like object -- OracleGym or MegaverseGym, they share the debug hooks.  It is a list of segments: setter commands, then k ticks of
multi-discrete actions [k, N * A, 6].  The commands are data, not calls, so that the same case can be played tick by tick (`play`, a generator that yields
after every setter block and every tick) or replayed through a device action ring one segment per call (test_tower_model_gpu.py).  Everything is built
from the debug setters (objects, pitch, position, yaw, velocity) and set_reward_shaping on the rooms a seeded reset generated; every scripted case is laid
out so that no floored point comes within 0.05 of a voxel boundary -- the judge asserts that on the model's own numbers.

Geometry (tests/canonical.py): a capsule rests with its centre 0.815 above the surface it stands on; a movable box at voxel y collides up to y + 0.8985;
forward = (-sin yaw, 0, -cos yaw); dt = 1 / 15, so an agent left in the air falls 0.06 in its first tick.  With the eye 0.46 above the centre, an agent on
the floor (surface 1.0) at pitch 0 picks at y = 1.835 and places at y = 1.535, one voxel ahead; at pitch +0.6 it places at y = 2.23, still one voxel ahead."""
import numpy as np

MARGIN = 0.05
W = H = 32
FLOOR = 1.0
INTERACT = [0, 0, 0, 0, 1, 0]
DIRS = {"+x": (1, 0), "-x": (-1, 0), "+z": (0, 1), "-z": (0, -1)}


def stand(surface):
    return surface + 0.525 + 0.33 - 0.04


def box_top(y):
    return y + 0.5 - 0.05 + 0.39 * 1.15


def pose(e, a, cell, face="+x", pitch=0.0, y=None):
    """agent a of env e over the centre of cell (x, z), standing on the floor unless y is given, facing `face`"""
    dx, dz = DIRS[face]
    return ("pose", e, a, (cell[0] + 0.5, stand(FLOOR) if y is None else y, cell[1] + 0.5), (float(-dz), float(-dx)), float(pitch))


def apply(g, cmds):
    for c in cmds:
        if c[0] == "objects":
            g.debug_set_objects(c[1], np.asarray(c[2], np.int8).reshape(-1, 4))
        elif c[0] == "pose":
            _, e, a, p, cs, pitch = c
            g.debug_set_agent_pos(e, a, *[float(np.float32(v)) for v in p])
            g.debug_set_agent_yaw(e, a, *cs)
            g.debug_set_agent_velocity(e, a, 0.0, 0.0, 0.0)
            g.debug_set_agent_pitch(e, a, float(np.float32(pitch)))
        elif c[0] == "shaping":
            cur = g.get_reward_shaping(c[1], c[2])
            cur.update(c[3])
            g.set_reward_shaping(c[1], c[2], cur)
        else:
            raise ValueError(c[0])


def snapshot(g, e):
    if hasattr(g, "snapshot"):
        return g.snapshot(e)
    import oracle_lib
    return g.debug_snapshot_bytes(e).view(oracle_lib.SNAP)[0]


def tick(g):
    g.step_norender() if hasattr(g, "step_norender") else g.step_no_render()


def dones_of(g, N):
    return np.asarray(g.get_dones()) if hasattr(g, "get_dones") else np.asarray([g.is_done(e) for e in range(N)])


class Case:
    scenario = "TowerBuilding"   # (tests/rearrange_cases.py and tests/sokoban_cases.py state theirs)

    def __init__(self, name, N, A, build, params=None, seed=42, scripted=True, replay=0):
        """replay = k > 0: the GPU tests also replay the case through an action ring, one call per segment; its segments are padded to k ticks with idle ones"""
        self.name, self.N, self.A, self.build, self.params, self.seed = name, N, A, build, dict(params or {}), seed
        self.scripted, self.replay = scripted, replay

    def make(self, cls, **kw):
        g = cls(self.scenario, W, H, self.N, self.A, 1, False, self.params, **kw)
        g.seed(self.seed)
        g.reset()
        return g

    def segments(self, g):
        segs = self.build(self, [snapshot(g, e) for e in range(self.N)])
        out = []
        for cmds, act in segs:
            if len(act) < self.replay:
                act = np.concatenate([act, np.zeros((self.replay - len(act),) + act.shape[1:], np.int32)])
            out.append((cmds, act))
        return out


def play(case, g):
    """generator: yields ("setup", the commands) after a segment's setters and ("tick", actions [N * A, 6]) after every tick"""
    for cmds, actions in case.segments(g):
        apply(g, cmds)
        yield "setup", cmds
        for row in actions:
            for i in range(case.N * case.A):
                g.set_actions(i // case.A, i % case.A, row[i].tolist())
            tick(g)
            yield "tick", row


# ---- rooms -------------------------------------------------------------------------------------------------------------------------------------

class Room:
    """what a case needs of a generated room: interior cells x in [1, L - 2], z in [1, W - 2], the zone, free floor cells handed out once each"""

    def __init__(self, snap):
        self.L, self.W = int(snap["L"]), int(snap["W"])
        self.bz = tuple(int(v) for v in snap["bz"])
        self.taken = set()

    def zone_cells(self):
        return [(x, z) for x in range(self.bz[0], self.bz[1]) for z in range(self.bz[2], self.bz[3])]

    def in_zone(self, c):
        return self.bz[0] <= c[0] < self.bz[1] and self.bz[2] <= c[1] < self.bz[3]

    def interior(self):
        return [(x, z) for x in range(1, self.L - 1) for z in range(1, self.W - 1)]

    def take(self, *cells):
        self.taken.update(cells)

    def free(self, n, zone=False):
        """n interior cells nobody took, outside the zone (or inside), at least 3 cells (Chebyshev) from every taken one and from each other"""
        out = []
        if n == 0:
            return out
        for c in self.interior():
            if self.in_zone(c) != zone:
                continue
            if all(max(abs(c[0] - t[0]), abs(c[1] - t[1])) >= 3 for t in list(self.taken) + out):
                out.append(c)
                if len(out) == n:
                    self.taken.update(out)
                    return out
        raise AssertionError("no free cells left in this room")


def fillers(room, n, avoid=()):
    """n boxes hanging at voxels y = 4 and y = 6 (clear of a standing agent's head) over interior columns nobody uses: they only occupy indices"""
    cells = [c for c in room.interior() if c not in room.taken and c not in avoid]
    out = [[c[0], y, c[1], 0] for y in (4, 6) for c in cells][:n]
    assert len(out) == n
    return out


# ---- a. index sweep ----------------------------------------------------------------------------------------------------------------------------

def sweep_layout():
    """the same 80 boxes in every room: a sheet at voxel y = 3 over x in [1, 8], z in [1, 10] (every room's interior holds it); index i at (1 + i % 8, 3, 1 + i // 8)"""
    return [[1 + i % 8, 3, 1 + i // 8, 0] for i in range(80)]


def build_sweep(case, snaps):
    """env e stands on the floor beside box e's column, looks up and takes it (the voxel at y = 2 is empty, the one above holds the box); then it stands in
    its zone and puts it down there"""
    boxes = sweep_layout()
    cmds0, cmds1 = [], []
    for e in range(case.N):
        room = Room(snaps[e])
        x, _, z, _ = boxes[e]
        cmds0 += [("objects", e, boxes), pose(e, 0, (x + 1, z), "-x", 0.5)]
        cmds1.append(pose(e, 0, (room.bz[0], room.bz[2]), "+x"))
    act = np.zeros((1, case.N, 6), np.int32)
    act[:, :, 4] = 1
    return [(cmds0, act), (cmds1, act.copy())]


# ---- b. pick rules -----------------------------------------------------------------------------------------------------------------------------

def build_pick(case, snaps):
    """A = 2 (agent 1 stands aside and never acts); one env per rule, agent 0 at cell c facing +x, the tried column is c + (1, 0)"""
    assert case.A == 2
    cmds, later = [], []
    act = np.zeros((3, case.N * 2, 6), np.int32)
    for e in range(case.N):
        room = Room(snaps[e])
        c, park = room.free(2)
        t = (c[0] + 1, c[1])
        objs, pitch, y, ticks = [], 0.0, None, (0,)
        if e == 0:     # box under box: the upper one goes
            objs = [[t[0], 1, t[1], 0], [t[0], 2, t[1], 0]]
        elif e == 1:   # a box above an empty voxel: taken through "then the one above"
            objs = [[t[0], 2, t[1], 0]]
        elif e == 2:   # three high: the first is covered, the second is covered, nothing is taken
            objs = [[t[0], 1, t[1], 0], [t[0], 2, t[1], 0], [t[0], 3, t[1], 0]]
        elif e == 3:   # a box agent 1 carries, recorded at the voxel above, covers nothing: the box at y = 1 goes
            objs = [[t[0], 2, t[1], 2], [t[0], 1, t[1], 0]]
        elif e == 4:   # level pitch does not reach a box at y = 3 (tries 1 and 2) ...
            objs = [[t[0], 3, t[1], 0]]
        elif e == 5:   # ... looking up does (tries 2 and 3)
            objs, pitch = [[t[0], 3, t[1], 0]], 0.5
        elif e == 6:   # in the air at 2.2 a level look tries 2 and 3: a box at y = 1 stays ...
            objs, y = [[t[0], 1, t[1], 0]], 2.2
        elif e == 7:   # ... looking down tries 1 and 2: it goes
            objs, pitch, y = [[t[0], 1, t[1], 0]], -0.5, 2.2
        elif e == 8:   # pick, put down, pick again inside the zone: the second pick pays no first-pick reward
            zc = room.zone_cells()[0]
            c, t = zc, (zc[0] + 1, zc[1])
            objs, ticks = [[t[0], 1, t[1], 0]], (0, 1, 2)
        cmds += [("objects", e, objs), pose(e, 0, c, "+x", pitch, y), pose(e, 1, park)]
        for k in ticks:
            act[k, e * 2] = INTERACT
    return [(cmds, act)]


# ---- c. place rules ----------------------------------------------------------------------------------------------------------------------------

def build_place(case, snaps, expect=None):
    """A = 2; agent 0 carries box 0 in every env.  Envs are handed to the rules in order, each rule takes the first room that allows it."""
    assert case.A == 2
    rooms = [Room(s) for s in snaps]
    used, cmds = set(), []
    act = np.zeros((1, case.N * 2, 6), np.int32)
    expect = {} if expect is None else expect   # rule -> the env that plays it (place_expect)

    def env_for(ok):
        for e, r in enumerate(rooms):
            if e not in used and ok(r):
                used.add(e)
                return e, r
        raise AssertionError("no room for a place rule")

    def put(e, r, name, objs, c, face, pitch=0.0, y=None, other=None):
        r.take(c)
        cmds.extend([("objects", e, [[0, 0, 0, 1]] + objs), pose(e, 0, c, face, pitch, y), pose(e, 1, other if other else r.free(1)[0])])
        act[0, e * 2] = INTERACT
        expect[name] = e

    # The target is a wall voxel beside a zone that touches the wall.  The rooms have no solid voxel inside a zone but the floor, which no place point
    # reaches, so the zone rule refuses this target as well: "a solid target is refused" on its own stays UNJUDGED (DESIGN.md "Stacking model"); the case
    # shows only that a wall target is refused and changes nothing.
    def wall_side(r):
        return ("-x" if r.bz[0] == 1 else "-z" if r.bz[2] == 1 else "+x" if r.bz[1] == r.L - 1 else "+z" if r.bz[3] == r.W - 1 else None)
    e, r = env_for(lambda r: wall_side(r) is not None)
    side = wall_side(r)
    put(e, r, "wall beside the zone", [], (r.bz[1] - 1 if side == "+x" else r.bz[0], r.bz[3] - 1 if side == "+z" else r.bz[2]), side)
    # the zone's edges: the last voxel inside, the first one outside (where that one is not a wall, so that only the zone refuses it)
    for name, ok, cell, face in (
            ("x < bz1 inside", lambda r: True, lambda r: (r.bz[1] - 2, r.bz[2]), "+x"),
            ("x = bz1 outside", lambda r: r.bz[1] <= r.L - 2, lambda r: (r.bz[1] - 1, r.bz[2]), "+x"),
            ("x = bz0 inside", lambda r: True, lambda r: (r.bz[0] + 1, r.bz[2]), "-x"),
            ("x = bz0 - 1 outside", lambda r: r.bz[0] >= 2, lambda r: (r.bz[0], r.bz[2]), "-x"),
            ("z < bz3 inside", lambda r: True, lambda r: (r.bz[0], r.bz[3] - 2), "+z"),
            ("z = bz3 outside", lambda r: r.bz[3] <= r.W - 2, lambda r: (r.bz[0], r.bz[3] - 1), "+z"),
            ("z = bz2 inside", lambda r: True, lambda r: (r.bz[0], r.bz[2] + 1), "-z"),
            ("z = bz2 - 1 outside", lambda r: r.bz[2] >= 2, lambda r: (r.bz[0], r.bz[2]), "-z")):
        e, r = env_for(ok)
        put(e, r, name, [], cell(r), face)
    zc = lambda r: (r.bz[0], r.bz[2])
    tc = lambda r: (r.bz[0] + 1, r.bz[2])
    e, r = env_for(lambda r: True)    # the target holds a box
    put(e, r, "target holds a box", [[tc(r)[0], 1, tc(r)[1], 0]], zc(r), "+x")
    e, r = env_for(lambda r: True)    # agent 1 stands in the target voxel
    r.take(tc(r))
    put(e, r, "another agent's voxel", [], zc(r), "+x", other=tc(r))
    e, r = env_for(lambda r: True)    # in the air, looking steeply down: the target is the agent's own voxel, which does not count
    put(e, r, "own voxel", [], zc(r), "+x", -1.2, 2.93)
    e, r = env_for(lambda r: True)    # from a column of four: the box falls four voxels to the floor
    put(e, r, "drop to the floor", [[zc(r)[0], y, zc(r)[1], 0] for y in (1, 2, 3, 4)], zc(r), "+x", 0.0, stand(box_top(4)))
    e, r = env_for(lambda r: True)    # ... onto a stack of two
    put(e, r, "drop onto a stack", [[zc(r)[0], y, zc(r)[1], 0] for y in (1, 2, 3, 4)] + [[tc(r)[0], y, tc(r)[1], 0] for y in (1, 2)], zc(r), "+x", 0.0,
        stand(box_top(4)))
    e, r = env_for(lambda r: True)    # from a column of two onto a column of three: level, the target holds a box; looking up, it lands on top
    put(e, r, "onto a column one higher", [[zc(r)[0], y, zc(r)[1], 0] for y in (1, 2)] + [[tc(r)[0], y, tc(r)[1], 0] for y in (1, 2, 3)], zc(r), "+x", 0.6,
        stand(box_top(2)))
    for e in range(case.N):
        if e not in used:
            cmds += [("objects", e, [])]
    return [(cmds, act)]


def place_expect(snaps):
    """rule -> the env of case c that plays it, for these rooms"""
    expect = {}
    build_place(CASES["place"], snaps, expect)
    return expect


# ---- d. heights and rewards --------------------------------------------------------------------------------------------------------------------

TOWER_TOP = 12
SPIRITS = (0.0, 0.5, 1.0)


def build_tower(case, snaps):
    """Env e has team spirit SPIRITS[e].  48 fillers hold indices 0 .. 47, so that every box that counts has an index >= 48: four boxes on the zone's floor,
    a support column of 13 beside the tower's column, 12 spares.  Agent 0 stands on the support column; before every tick one spare is handed to it
    (set_objects states the same scene with that spare carried), it puts it on the tower: y = 1 .. 12, the cap binds from y = 9.  Then it goes down, takes
    one of the zone's floor boxes and puts it on another one: the delta carries the removal.  The other agents stand aside and get their share."""
    segs = []
    rooms = [Room(s) for s in snaps]
    scene = []
    for e, r in enumerate(rooms):
        zone = r.zone_cells()
        tower, support = (r.bz[0] + 1, r.bz[2]), (r.bz[0], r.bz[2])
        floor = [c for c in zone if c[0] >= r.bz[0] + 1 and c[1] >= r.bz[2] + 1][:4]   # (zones are at least 3 x 3)
        assert len(floor) == 4
        r.take(tower, support, *floor)
        parks = r.free(case.A - 1)
        hang = fillers(r, 60, avoid=zone)
        objs = hang[:48] + [[c[0], 1, c[1], 0] for c in floor] + [[support[0], y, support[1], 0] for y in range(1, 14)] + hang[48:]
        assert len(objs) == 77
        scene.append((r, tower, support, floor, parks, objs))
    cmds = []
    for e, (r, tower, support, floor, parks, objs) in enumerate(scene):
        cmds += [("shaping", e, a, {"teamSpirit": SPIRITS[e]}) for a in range(case.A)]
        cmds += [pose(e, a + 1, parks[a]) for a in range(case.A - 1)]
    for k in range(TOWER_TOP):
        for e, (r, tower, support, floor, parks, objs) in enumerate(scene):
            objs = [list(o) for o in objs]
            for j in range(k):
                objs[65 + j] = [tower[0], 1 + j, tower[1], 0]
            objs[65 + k] = [0, 0, 0, 1]
            cmds += [("objects", e, objs), pose(e, 0, support, "+x", 0.0, stand(box_top(13)))]
        act = np.zeros((1, case.N * case.A, 6), np.int32)
        act[0, ::case.A] = INTERACT
        segs.append((cmds, act))
        cmds = []
    # the box on floor[0] goes onto floor[1] -- from the cell west of it (inside the zone or not, free either way), first level, then looking up
    for step, (cell, pitch) in enumerate(((0, 0.0), (1, 0.6))):
        for e, (r, tower, support, floor, parks, objs) in enumerate(scene):
            c = floor[cell]
            cmds.append(pose(e, 0, (c[0] - 1, c[1]), "+x", pitch))
        act = np.zeros((1, case.N * case.A, 6), np.int32)
        act[0, ::case.A] = INTERACT
        segs.append((cmds, act))
        cmds = []
    return segs


def build_end(case, snaps):
    """short episodes (seed 8: the shortest of the three lasts 20.2 s): agent 0 puts one box on a stack of two in the zone (highest_tower 3), then nothing
    happens until the first env's episode ends by itself"""
    cmds = []
    shortest = 1 << 30
    for e, s in enumerate(snaps):
        r = Room(s)
        zc, tc = (r.bz[0], r.bz[2]), (r.bz[0] + 1, r.bz[2])
        cmds += [("objects", e, [[0, 0, 0, 1]] + [[zc[0], y, zc[1], 0] for y in (1, 2)] + [[tc[0], y, tc[1], 0] for y in (1, 2)]),
                 pose(e, 0, zc, "+x", 0.0, stand(box_top(2)))]
        shortest = min(shortest, int(np.ceil(float(s["episode_len"]) * 15.0)) + 2)
    assert shortest <= 320
    act = np.zeros((shortest, case.N, 6), np.int32)
    act[0, :, 4] = 1
    return [(cmds, act)]


# ---- e. zone visit -----------------------------------------------------------------------------------------------------------------------------

def build_visit(case, snaps):
    """env 0: carrying, outside (nothing), inside (the team reward), outside and inside again (not twice); env 1: takes a box while inside (both rewards in
    one tick); env 2: inside without a box for three ticks (nothing)"""
    rooms = [Room(s) for s in snaps]
    for r in rooms:
        r.take(*r.zone_cells())
    inside = [(r.bz[0] + 1, r.bz[2] + 1) for r in rooms]
    outside = [r.free(1)[0] for r in rooms]
    segs = []
    none = np.zeros((1, case.N, 6), np.int32)
    first = [("objects", 0, [[0, 0, 0, 1]]), pose(0, 0, outside[0]),
             ("objects", 1, [[inside[1][0] + 1, 1, inside[1][1], 0]]), pose(1, 0, inside[1], "+x"),
             ("objects", 2, [[inside[2][0] + 1, 1, inside[2][1], 0]]), pose(2, 0, inside[2], "-x")]
    act = none.copy()
    act[0, 1] = INTERACT
    segs.append((first, act))
    segs.append(([pose(0, 0, inside[0], "-z")], none.copy()))
    segs.append(([pose(0, 0, outside[0])], none.copy()))
    segs.append(([pose(0, 0, inside[0], "-z")], none.copy()))
    return segs


# ---- f. order ----------------------------------------------------------------------------------------------------------------------------------

def build_order(case, snaps):
    """A = 4 (the controllers are shared out before interact); agents 2 and 3 stand aside.  env 0: agents 0 and 1 face one box from both sides, the lower
    index gets it; env 1: agent 0 puts a box into a zone voxel and agent 1 takes it out of it in the same tick; env 2: the other way round -- agent 0 finds
    nothing, agent 1's box stays"""
    assert case.A == 4
    cmds = []
    act = np.zeros((1, case.N * 4, 6), np.int32)
    for e, s in enumerate(snaps):
        r = Room(s)
        mid = (r.bz[0] + 1, r.bz[2])
        west, east = (mid[0] - 1, mid[1]), (mid[0] + 1, mid[1])
        r.take(mid, west, east)
        parks = r.free(2)
        objs = {0: [[mid[0], 1, mid[1], 0]], 1: [[0, 0, 0, 1]], 2: [[0, 0, 0, 2]]}[e]
        cmds += [("objects", e, objs), pose(e, 0, west, "+x"), pose(e, 1, east, "-x"), pose(e, 2, parks[0]), pose(e, 3, parks[1])]
        act[0, e * 4] = act[0, e * 4 + 1] = INTERACT
    return [(cmds, act)]


# ---- g. stress ---------------------------------------------------------------------------------------------------------------------------------

STRESS_TICKS = 320
STRESS_PARAMS = {"verticalLookLimitRad": 0.6}


def stress_script(seed, ticks, agents):
    """interact-biased (tests/action_ring_util.py: make_script dithers less, but earns few placements): runs of 2 .. 8 ticks per agent -- interact held or
    pulsed on the spot, turns, looks, short walks and jumps"""
    rng = np.random.default_rng(seed)
    out = np.zeros((ticks, agents, 6), np.int32)
    for a in range(agents):
        t = 0
        while t < ticks:
            run = int(rng.integers(2, 9))
            kind = int(rng.choice(6, p=[0.50, 0.18, 0.14, 0.08, 0.06, 0.04]))
            seg = out[t:t + run, a]
            n = seg.shape[0]
            if kind == 0:      # interact on the spot, every tick
                seg[:, 4] = 1
            elif kind == 1:    # turn, interact at the end
                seg[:, 2] = 1 + int(rng.integers(0, 2))
                seg[-1, 4] = 1
            elif kind == 2:    # turn while interacting
                seg[:, 2] = 1 + int(rng.integers(0, 2))
                seg[:, 4] = rng.random(n) < 0.5
            elif kind == 3:    # look up or down, interact at the end
                seg[:, 5] = 1 + int(rng.integers(0, 2))
                seg[-1, 4] = 1
            elif kind == 4:    # walk, interact now and then
                seg[:, 1] = 1
                seg[:, 4] = rng.random(n) < 0.4
            else:              # walk and jump
                seg[:, 1] = 1
                seg[:, 3] = 1
            t += run
    return out


def stress_layout(room, rng, A, e):
    """60 .. 80 boxes around the zone's low corner, indices shuffled.  Relative to that corner: the block x in [-1, 3], z in [-1, 1] stands three high, but
    the start cells (0, 0) and (2, 0) two high -- an agent there takes and puts back boxes at y = 3; the rows z = 2, 3 stand one high around the start cells
    (0, 2) and (2, 2), which are empty -- an agent there works on the floor; the rest lies scattered on the floor.  Only what is inside the room counts, so
    a zone in a corner of its room is part-filled differently from one in the middle.  A = 1: even envs start on the stack, odd ones on the floor."""
    ox, oz = room.bz[0], room.bz[2]
    inside = set(room.interior())
    starts = [(ox, oz), (ox + 2, oz), (ox, oz + 2), (ox + 2, oz + 2)]
    boxes, used = [], set()
    for dx in range(-1, 4):
        for dz in range(-1, 4):
            c = (ox + dx, oz + dz)
            if c not in inside:
                continue
            h = (2 if c in starts else 3) if dz <= 1 else (0 if c in starts else 1)
            boxes += [[c[0], y, c[1], 0] for y in range(1, 1 + h)]
            used.add(c)
    rest = [c for c in room.interior() if c not in used]
    rng.shuffle(rest)
    want = int(rng.integers(max(60, len(boxes)), 81))
    boxes += [[c[0], 1, c[1], 0] for c in rest[:want - len(boxes)]]
    assert 60 <= len(boxes) <= 80, len(boxes)
    order = rng.permutation(len(boxes))
    if A == 1:
        starts = [starts[2 * (e % 2)]]
    return [boxes[i] for i in order], [(c, stand(box_top(2)) if c[1] == oz else stand(FLOOR)) for c in starts[:A]]


def make_stress(A, seed):
    def build(case, snaps):
        rng = np.random.default_rng(seed)
        cmds = []
        for e, s in enumerate(snaps):
            boxes, starts = stress_layout(Room(s), rng, A, e)
            cmds.append(("objects", e, boxes))
            cmds += [pose(e, a, starts[a][0], ("+x", "-x", "+z", "-z")[(e + a) % 4], 0.0, starts[a][1]) for a in range(A)]
        script = stress_script(seed, STRESS_TICKS, case.N * A)
        return [(cmds if k == 0 else [], script[k:k + 8]) for k in range(0, STRESS_TICKS, 8)]
    return build


STRESS_SEEDS = {1: 7, 4: 5}   # chosen on the CPU with the oracle (test_tower_model.py asserts the counts they give)

CASES = {c.name: c for c in (
    Case("sweep", 80, 1, build_sweep, replay=8),
    Case("pick", 9, 2, build_pick),
    Case("place", 24, 2, build_place),
    Case("tower_a1", 3, 1, build_tower, replay=2),
    Case("tower_a2", 3, 2, build_tower),
    Case("tower_a4", 3, 4, build_tower, replay=2),
    Case("end", 3, 1, build_end, params={"episodeLengthSec": 0.2}, seed=8),
    Case("visit", 3, 1, build_visit),
    Case("order", 3, 4, build_order, replay=8),
    Case("stress_a1", 8, 1, make_stress(1, STRESS_SEEDS[1]), params=STRESS_PARAMS, scripted=False, replay=8),
    Case("stress_a4", 8, 4, make_stress(4, STRESS_SEEDS[4]), params=STRESS_PARAMS, scripted=False, replay=8),
)}


def run_judged(case, g, rules=None, on_tick=None):
    """plays the case on g under the model's eyes -> (Judge, [ticks] rewards [N * A] fp32 of every tick); on_tick(t, g): the caller's own look at every tick"""
    import tower_model
    judge = tower_model.Judge(lambda e: snapshot(g, e), case.N, case.A, rules)
    rewards, t = [], 0
    for what, row in play(case, g):
        if what == "setup":   # restated objects: the whole record; poses and shaping: the reward's history stays the model's
            fresh = {c[1] for c in row if c[0] == "objects"} if rewards else set(range(case.N))
            judge.sync(sorted(fresh))
            judge.sync([e for e in range(case.N) if e not in fresh], keep=True)
            continue
        r = np.asarray(g.get_last_rewards(), np.float32)
        rewards.append(r)
        judge.tick(row[:, 4].reshape(case.N, case.A) << 8, r, dones_of(g, case.N), g.true_objective, MARGIN if case.scripted else None)
        if on_tick:
            on_tick(t, g)
        t += 1
    return judge, rewards
