"""Seeded, deterministic query classes for the controller's sweeps, push-outs and steps (tests/physics_reference.py states what they are judged
by).  Every input is fp32-representable.  A Batch is one collider array with the records that run against it -- one launch on the device; its
`variants` are the mv_debug_* variants whose kernels can hold it (kinds, and at most 64 NC slots).  Collider sets come in the sizes at which the
wave logic can go wrong: 1, 63, 64, 65, 128 and 64 NC slots, the live colliders at chosen slots, the rest far-away filler boxes.

Classes (CLASSES below): boxes (face-on, edge and corner approaches at voxel scale and at Collect's heights: walks, falls, jumps), grazing (a path
passing 0.0385 .. 0.2 under a rounded edge, a capsule, the ball), threshold (queries that sit ON the code's thresholds: exempt from the fragile cap),
ties (bit-equal fractions with different normals at every slot relation, and the same with the slots swapped), slope (the slope filter on both
sides of MAX_SLOPE_COS, a nearer rejected hit in front of a farther accepted one), hex (boxes in wall frames 0, 1, 2 beside axis-aligned ones),
ball (football_cases' geometries as single casts), pushout, and steps (player_step scenes)."""
import numpy as np

import physics_reference as R

F32 = np.float32
NC_OF = {0: 1, 1: 2, 2: 4, 3: 1, 4: 1}                     # MV_PHYS_NC1, NC2, NC4, HEX, BALL
KINDS_OF = {0: {0, 1, 2}, 1: {0, 1, 2}, 2: {0, 1, 2}, 3: {0, 1, 2, 3, 4, 5}, 4: {0, 1, 2, 7}}
HH, CR = F32(R.CAP_HH), F32(R.CAP_R)
UP, DOWN = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
REST = float(R.CAP_HH + R.CAP_R - R.ALLOWED_CCD_PEN)     # capsule centre above the surface it stands on


class Batch:
    def __init__(self, cls, name, cols, queries=None, positions=None, agents=None, meta=None):
        self.cls, self.name, self.cols = cls, name, np.ascontiguousarray(cols, R.COL)
        self.queries = None if queries is None else np.ascontiguousarray(queries, R.QUERY)
        self.positions = None if positions is None else np.ascontiguousarray(positions, F32).reshape(-1, 3)
        self.agents = None if agents is None else np.ascontiguousarray(agents, R.AGENT)
        self.meta = meta or {}
        kinds = set(int(k) for k in self.cols["kind"])
        self.variants = [v for v in range(5) if kinds <= KINDS_OF[v] and len(self.cols) <= 64 * NC_OF[v]]
        assert self.variants, (cls, name)
        for a in (self.cols["lo"], self.cols["hi"], self.positions) + (() if self.queries is None else (self.queries["from"], self.queries["to"])):
            assert a is None or np.isfinite(a).all()

    def __repr__(self):
        return f"{self.cls}/{self.name}"


def box(lo, hi, frame=None):
    """a box with RAW bounds (in its frame): the record holds them grown by CAP_HH in y, as the tick headers grow them"""
    c = np.zeros((), R.COL)
    c["kind"] = 1 if frame is None else 3 + frame
    c["lo"] = (F32(lo[0]), F32(lo[1]) - HH, F32(lo[2]))
    c["hi"] = (F32(hi[0]), F32(hi[1]) + HH, F32(hi[2]))
    return c


def capsule(centre):
    c = np.zeros((), R.COL)
    c["kind"], c["lo"], c["hi"] = 2, centre, (F32(2) * HH, 0, 0)
    return c


def ball(centre, radius=1.0):
    c = np.zeros((), R.COL)
    c["kind"], c["lo"], c["hi"] = 7, centre, (HH, CR + F32(radius), 0)
    return c


def place(live, n_cols, slots=None):
    """n_cols slots: the live colliders at `slots` (default: the first ones), far-away filler boxes everywhere else"""
    slots = list(range(len(live))) if slots is None else list(slots)
    assert len(slots) == len(live) and len(set(slots)) == len(slots) and max(slots, default=0) < n_cols
    out = np.zeros(n_cols, R.COL)
    for i in range(n_cols):
        out[i] = box((50.0 + (i % 16), -30.0, 50.0 + (i // 16)), (50.5 + (i % 16), -29.0, 50.5 + (i // 16)))
    for s, c in zip(slots, live):
        out[s] = c
    return out


def queries(frm, to, up=(0.0, 0.0, 0.0), msd=0.0, forward=False):
    """QUERY records; forward: the forward sweep's filter (up = from - to, minSlopeDot 0)"""
    frm, to = np.asarray(frm, F32).reshape(-1, 3), np.asarray(to, F32).reshape(-1, 3)
    q = np.zeros(len(frm), R.QUERY)
    q["from"], q["to"] = frm, to
    q["up"] = (frm - to) if forward else np.broadcast_to(np.asarray(up, F32), frm.shape)
    q["min_slope_dot"] = 0.0 if forward else msd
    return q


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _to_world(col, v):
    c, s = R._frame(np.asarray(col["kind"]))
    return R._to_world(c, s, np.asarray(v, np.float64))


def approach(rng, col, mode, n):
    """n sweeps towards a box-like collider (bounds as in its record, its own frame): face-on, edge and corner contact points; the path passes the
    contact position at t in (0.1, 1.3) of its length (past 1: it ends short).  mode: walk (horizontal, |d| <= 0.3), fall (down, up to 55 / 15), jump"""
    lo, hi = col["lo"].astype(np.float64), col["hi"].astype(np.float64)
    frm, to = [], []
    while len(frm) < n:
        st = rng.integers(-1, 2, 3)
        if mode == "walk":
            if st[0] == 0 and st[2] == 0:
                continue
            st[1] = rng.choice([0, 0, 1])
        elif mode == "fall":
            st[1] = 1
        else:
            st[1] = -1
        cpt = np.where(st < 0, lo, np.where(st > 0, hi, lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)))
        if mode == "walk" and st[1] == 0:
            cpt[1] = hi[1] - rng.uniform(0.0, 0.7)        # a walker's centre: well above the floor the box stands on
        nrm = _unit(np.where(st != 0, st * rng.uniform(0.1, 1.0, 3), 0.0))
        if mode == "walk":
            nh = _unit(np.array([nrm[0], 0.0, nrm[2]]))
            ang = rng.uniform(-1.4, 1.4)
            d = -np.array([nh[0] * np.cos(ang) - nh[2] * np.sin(ang), 0.0, nh[0] * np.sin(ang) + nh[2] * np.cos(ang)]) * rng.uniform(0.05, 0.3)
        elif mode == "fall":
            d = np.array([0.0, -rng.uniform(0.2, 55.0 / 15.0), 0.0])
        else:
            d = np.array([0.0, rng.uniform(0.05, 6.2 / 15.0), 0.0])
        contact = cpt + nrm * (R.CAP_R - R.ALLOWED_CCD_PEN)
        start = contact - d * rng.uniform(0.1, 1.3)
        frm.append(_to_world(col, start))
        to.append(_to_world(col, start + d))
    return np.array(frm), np.array(to)


def _mode_queries(rng, col, n_each):
    qs = []
    f, t = approach(rng, col, "walk", n_each)
    qs.append(queries(f, t, forward=True))
    f, t = approach(rng, col, "fall", n_each)
    qs.append(queries(f, t, UP, R.MAX_SLOPE_COS))
    f, t = approach(rng, col, "jump", n_each)
    qs.append(queries(f, t, DOWN, R.MAX_SLOPE_COS))
    return np.concatenate(qs)


def class_boxes():
    rng = np.random.default_rng(101)
    voxel = [box((0, 0, 0), (40, 1, 40)), box((20, 1, 20), (21, 2, 21)), box((22, 1, 20), (23, 3, 21)), box((0, 1, 0), (1, 6, 40)),
             box((37.25, 1, 3.5), (38.5, 1.9, 39.75))]
    collect = [box((30, 1, 30), (31, 12, 31)), box((28, 8, 28), (30, 9, 30)), box((0, 0, 0), (40, 1, 40))]
    out = []
    for name, live, targets, n_cols, slots in (("voxel_5", voxel, (1, 2, 3, 4), 5, None), ("voxel_63", voxel, (1, 2, 4), 63, (62, 0, 31, 7, 40)),
                                               ("voxel_64", voxel, (1, 3), 64, (0, 63, 1, 62, 33)), ("voxel_65", voxel, (2, 4), 65, (64, 0, 5, 6, 63)),
                                               ("voxel_128", voxel, (1, 2), 128, (127, 64, 63, 0, 100)), ("voxel_256", voxel, (2, 3), 256, (255, 192, 128, 64, 1)),
                                               ("collect_3", collect, (0, 1), 3, None), ("collect_1", collect[:1], (0,), 1, None)):
        cols = place(live, n_cols, slots)
        idx = list(range(len(live))) if slots is None else list(slots)
        q = np.concatenate([_mode_queries(rng, cols[idx[t]], 40 if n_cols > 5 else 70) for t in targets])
        out.append(Batch("boxes", name, cols, q))
    return out


def _graze(rng, n, centre_of, axis_dir, radius):
    """paths whose closest approach to a rounded edge / axis lies `radius - depth` from it, depth in 0.0385 .. 0.2 under the surface"""
    frm, to = [], []
    for _ in range(n):
        depth = rng.uniform(0.0385, 0.2)
        u, t = axis_dir(rng)
        pc = centre_of(rng) + u * (radius - depth)
        a = rng.uniform(0.05, 0.25)
        b = rng.uniform(0.02, 0.3 - a)
        frm.append(pc - t * a)
        to.append(pc + t * b)
    return np.array(frm), np.array(to)


def class_grazing():
    rng = np.random.default_rng(202)
    bx = box((10, 1, 10), (11, 2, 11))
    cp = capsule((14.0, 1.815, 10.5))
    bl = ball((18.0, 2.0, 10.5))

    def vertical_edge(rng):   # the edge x = 11, z = 11: outward directions in its quadrant, the path horizontal and across them
        ang = rng.uniform(0.1, np.pi / 2 - 0.1)
        u = np.array([np.cos(ang), 0.0, np.sin(ang)])
        return u, np.array([-u[2], 0.0, u[0]]) * rng.choice([-1.0, 1.0])

    def top_edge(rng):        # the (grown) top edge x = 11: a fall past it
        return np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0])

    def around_axis(rng):
        ang = rng.uniform(0.0, 2 * np.pi)
        u = np.array([np.cos(ang), 0.0, np.sin(ang)])
        return u, np.array([-u[2], 0.0, u[0]])

    out = []
    f1, t1 = _graze(rng, 500, lambda r: np.array([11.0, r.uniform(1.9, 2.4), 11.0]), vertical_edge, R.CAP_R)
    f2, t2 = _graze(rng, 300, lambda r: np.array([11.0, float(bx["hi"][1]), r.uniform(10.1, 10.9)]), top_edge, R.CAP_R)
    q = np.concatenate([queries(f1, t1, forward=True), queries(f2, t2, UP, R.MAX_SLOPE_COS)])
    out.append(Batch("grazing", "box_edge_1", bx.reshape(1), q))
    out.append(Batch("grazing", "box_edge_65", place([bx], 65, [64]), q[::4]))
    f3, t3 = _graze(rng, 400, lambda r: np.array([14.0, r.uniform(1.0, 2.6), 10.5]), around_axis, 2 * R.CAP_R)
    out.append(Batch("grazing", "capsule", place([cp, bx], 2), queries(f3, t3, forward=True)))
    f4, t4 = _graze(rng, 400, lambda r: np.array([18.0, r.uniform(1.6, 2.4), 10.5]), around_axis, R.CAP_R + 1.0)
    out.append(Batch("grazing", "ball", place([bl, bx], 2), queries(f4, t4, forward=True)))
    return out


def _ulps(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return x


def class_threshold():
    """queries that sit on the thresholds, against the box [10, 11]^3 (raw), a capsule and the ball"""
    bx = box((10, 10, 10), (11, 11, 11))
    cp = capsule((14.0, 10.5, 10.5))
    bl = ball((18.0, 10.5, 10.5))
    hix, hiy = F32(bx["hi"][0]), F32(bx["hi"][1])
    frm, to, tags = [], [], []

    def add(tag, f, t):
        frm.append(np.asarray(f, F32)); to.append(np.asarray(t, F32)); tags.append(tag)

    on = hix + CR + (F32(R.CAST_RADIUS) - F32(R.ALLOWED_CCD_PEN))        # a start exactly CAST_RADIUS - 0.04 from the face
    for k in (-2, -1, 0, 1, 2):
        add("start_on_radius", (_ulps(on, k), 10.5, 10.5), (_ulps(on, k) - F32(0.2), 10.5, 10.5))
    reach = hix + (CR - F32(R.ALLOWED_CCD_PEN)) + F32(0.25)                # lambda lands on 1.0: gap + 0.04 == |d|
    for k in (-2, -1, 0, 1, 2):
        add("lambda_one", (_ulps(reach, k), 10.5, 10.5), (_ulps(reach, k) - F32(0.25), 10.5, 10.5))
    add("zero_length", (11.5, 10.5, 10.5), (11.5, 10.5, 10.5))
    add("zero_length_inside", (11.2, 10.5, 10.5), (11.2, 10.5, 10.5))
    add("one_ulp", (11.5, 10.5, 10.5), (_ulps(11.5, -1), 10.5, 10.5))
    add("one_ulp_inside", (11.2, 10.5, 10.5), (_ulps(11.2, -1), 10.5, 10.5))
    for depth in (0.0395, 0.05, 0.2, 0.32):                               # start inside: fraction 0
        add("start_inside", (hix + CR - F32(depth), 10.5, 10.5), (hix + CR - F32(depth) - F32(0.2), 10.5, 10.5))
        add("start_inside_leaving", (hix + CR - F32(depth), 10.5, 10.5), (hix + CR - F32(depth) + F32(0.2), 10.5, 10.5))
    for p in ((10.9, 10.5, 10.5), (10.5, 10.5, 10.1), (10.5, hiy - F32(0.05), 10.5), (10.5, 10.5, 10.5), (10.25, 10.5, 10.25)):   # d2 == 0
        for d in ((0.2, 0, 0), (-0.2, 0, 0), (0, 0.2, 0), (0, -0.2, 0), (0, 0, 0.2), (0, 0, -0.2)):
            add("centre_inside", p, tuple(F32(a) + F32(b) for a, b in zip(p, d)))
    for dy in (0.0, 0.4, 1.2):                                            # the centre on a capsule's axis / the ball's
        for cx in (14.0, 18.0):
            for d in ((0.2, 0, 0), (-0.2, 0, 0), (0, 0, 0.2), (0, -0.2, 0)):
                add("on_axis", (cx, 10.5 + dy, 10.5), (cx + d[0], 10.5 + dy + d[1], 10.5 + d[2]))
            add("near_axis", (cx + 5e-7, 10.5 + dy, 10.5), (cx + 0.2, 10.5 + dy, 10.5))
            add("near_axis", (cx + 2e-6, 10.5 + dy, 10.5), (cx - 0.2, 10.5 + dy, 10.5))
    n_plain = len(frm)
    # the cull: the path's bounding box exactly CAP_R from the box, one ulp inside, one ulp outside, on every side, moving along the face and away
    for axis in range(3):
        for side in (0, 1):
            edge = F32(bx["hi"][axis]) + CR if side else F32(bx["lo"][axis]) - CR
            for k in (-1, 0, 1):
                for d in ((0.13, 0.07), (-0.2, 0.0), (0.0, 0.0)):
                    p = np.array([10.5, 10.5, 10.5], F32)
                    p[axis] = _ulps(edge, k)
                    q = p.copy()
                    q[(axis + 1) % 3] += F32(d[0]); q[(axis + 2) % 3] += F32(d[1])
                    add("cull", p, q)
                    far = p.copy()
                    far[axis] = edge + (F32(0.25) if side else F32(-0.25))
                    add("cull", far, p)                                    # ends there, coming from outside
                    add("cull", p, far)
    rng = np.random.default_rng(303)
    for _ in range(300):                                                   # random paths whose bounding box lies within 1e-3 of the cull's border
        axis, side = rng.integers(0, 3), rng.integers(0, 2)
        edge = float(bx["hi"][axis]) + R.CAP_R if side else float(bx["lo"][axis]) - R.CAP_R
        p = rng.uniform(9.8, 11.2, 3)
        q = p + rng.uniform(-0.2, 0.2, 3)
        off = rng.uniform(-1e-3, 1e-3)
        shift = (edge + off) - (min(p[axis], q[axis]) if side else max(p[axis], q[axis]))
        p[axis] += shift; q[axis] += shift
        add("cull", p, q)
    q = queries(np.array(frm), np.array(to), forward=True)
    q2 = queries(np.array(frm), np.array(to), UP, R.MAX_SLOPE_COS)
    cols = place([bx, cp, bl], 3)
    cols_nb = place([bx, cp], 2)
    meta = {"tags": tags + tags, "cull": np.array([t == "cull" for t in tags + tags])}
    return [Batch("threshold", "box_capsule_ball", cols, np.concatenate([q, q2]), meta=meta),
            Batch("threshold", "box_capsule", cols_nb, np.concatenate([q, q2]), meta=meta),
            Batch("threshold", "box_capsule_256", place([bx, cp], 256, [200, 77]), np.concatenate([q, q2])[::3],
                  meta={"tags": (tags + tags)[::3], "cull": meta["cull"][::3]})]


def class_ties():
    """Symmetric inner corners met along the diagonal: the walls' fractions are bit-equal (the same operations on the same values), their normals differ.
    Every corner of one array sits at its own place in the world with its walls at one slot relation; `swapped` holds the same walls with each
    corner's slots exchanged.  meta["first"]: [Q] which wall (0: the x wall, 1: the z wall, 2: the floor) holds the lowest slot."""
    rng = np.random.default_rng(404)
    out = []
    relations = {4: [(5, 69), (6, 134), (8, 199), (72, 136), (10, 14), (80, 90), (20, 85), (30, 223), (150, 40)],
                 2: [(5, 69), (10, 14), (80, 90), (20, 85), (100, 40)], 1: [(5, 9), (0, 63), (30, 31)]}
    for nc, rel in relations.items():
        for swapped in (False, True):
            rng = np.random.default_rng(404 + nc)                         # the same queries for both slot orders
            live, slots, frm, to, first, roles = [], [], [], [], [], ([], [], [])
            for j, (s0, s1) in enumerate(rel):
                ox = 8.0 * j                                              # corner j: walls x in [ox, ox + 1] and z in [0, 1], a floor below
                three = j % 3 == 2
                wx, wz = box((ox, 0, 0), (ox + 1, 4, 6)), box((ox, 0, 0), (ox + 6, 4, 1))
                a, b = (s1, s0) if swapped else (s0, s1)
                live += [wx, wz]; slots += [a, b]
                roles[0].append(a); roles[1].append(b)
                low = 0 if a < b else 1
                if three:                                                 # a third tie: the floor's (grown) top at y = 1, met along (-1, -1, -1)
                    fl = np.zeros((), R.COL)
                    fl["kind"], fl["lo"], fl["hi"] = 1, (ox, -1, 0), (ox + 6, 1, 6)
                    s2 = max(a, b) + 1 if not swapped else min(a, b) - 1
                    live.append(fl); slots.append(s2); roles[2].append(s2)
                    low = 2 if s2 < min(a, b) else low
                for _ in range(24):
                    # multiples of 2^-10: every coordinate, and so the direction to - from, is exact at every corner's magnitude -- the walls see the
                    # same gap and the same closing rate, and a face-on cast ends with its first step: the same fraction, bit for bit
                    g = int(rng.integers(308, 563))
                    gap = F32(g / 1024.0)
                    step = F32(int(rng.integers(max(103, g - 276), 308)) / 1024.0)
                    px = F32(ox + 1) + gap
                    off = F32(px - F32(ox))                               # the same offset from each wall's face: p.z - 1 == p.x - (ox + 1) bit for bit
                    pz = F32(1) + (px - F32(ox + 1))
                    assert pz - F32(1) == px - F32(ox + 1) and off > 0
                    if three:
                        py = F32(1) + (px - F32(ox + 1))
                        frm.append((px, py, pz)); to.append((px - step, py - step, pz - step))
                    else:
                        frm.append((px, 2.0, pz)); to.append((px - step, 2.0, pz - step))
                    first.append(low)
            cols = place(live, 64 * nc, slots)
            q = queries(np.array(frm), np.array(to), forward=True)
            out.append(Batch("ties", f"corners_nc{nc}" + ("_swapped" if swapped else ""), cols, q, meta={"first": np.array(first), "roles": roles}))
    # a seam: two boxes side by side, met on the line between them (equal normals: either winner reports the same)
    seam = [box((2, 0, 2), (3, 1, 4)), box((3, 0, 2), (4, 1, 4))]
    f = np.array([(3.0, 2.5 + 0.1 * i, 2.5 + 0.1 * i) for i in range(10)])
    out.append(Batch("ties", "seam", place(seam, 65, [64, 3]), queries(f, f - np.array([0.0, 1.5, 0.0]), UP, R.MAX_SLOPE_COS), meta={"first": None}))
    return out


def assert_lowest_slot_wins(b, got, sweep_fn):
    """a ties batch under one implementation (sweep_fn(cols, queries) -> SWEEP_OUT): cast against the x walls alone, the z walls alone and the floors
    alone, the implementation's OWN fractions of a corner's walls are bit-equal -- and then the sweep over all of them must report the wall in the lowest
    slot (meta["first"]), whatever lane and k the slots fall on"""
    alone = [sweep_fn(np.ascontiguousarray(b.cols[r]), b.queries) for r in b.meta["roles"]]
    first = b.meta["first"]
    for q in range(len(b.queries)):
        tied = [r for r in range(3) if alone[r]["hit"][q]]
        assert len(tied) >= 2 and first[q] in tied, (b, q, tied)
        bits = {alone[r]["fraction"][q].tobytes() for r in tied}
        assert len(bits) == 1, (b, q, "the walls' fractions differ", [alone[r]["fraction"][q] for r in tied])
        normals = {alone[r]["normal"][q].tobytes() for r in tied}
        assert len(normals) == len(tied), (b, q, "the walls' normals must differ")
        w = alone[first[q]]
        assert got["hit"][q] == 1 and got["fraction"][q].tobytes() == w["fraction"][q].tobytes(), (b, q)
        assert got["normal"][q].tobytes() == w["normal"][q].tobytes(), (b, q, "winner", got["normal"][q], "lowest slot", w["normal"][q])


def class_slope():
    """falls onto (and jumps up against) the rounded long edge of a box at contact angles 30 .. 60 degrees from the vertical: dot(up, n) on both sides
    of MAX_SLOPE_COS; under the box's edge a floor that a rejected hit must leave to be found"""
    rng = np.random.default_rng(505)
    bx, floor = box((10, 2, 10), (11, 3, 14)), box((0, 0, 0), (40, 1, 40))
    top, bot = float(bx["hi"][1]), float(bx["lo"][1])
    frm, to, frm_u, to_u = [], [], [], []
    for _ in range(500):
        th = np.deg2rad(rng.uniform(30.0, 60.0))
        x = 11.0 + (R.CAP_R - R.ALLOWED_CCD_PEN) * np.sin(th)
        z = rng.uniform(10.5, 13.5)
        y0 = top + rng.uniform(0.4, 1.0)
        frm.append((x, y0, z)); to.append((x, y0 - rng.uniform(1.5, 55.0 / 15.0), z))
        yu = bot - rng.uniform(0.35, 0.6)
        frm_u.append((x, yu, z)); to_u.append((x, yu + rng.uniform(0.1, 0.41), z))
    q = np.concatenate([queries(np.array(frm), np.array(to), UP, R.MAX_SLOPE_COS), queries(np.array(frm_u), np.array(to_u), DOWN, R.MAX_SLOPE_COS)])
    return [Batch("slope", "edge_over_floor", place([bx, floor], 2), q), Batch("slope", "edge_over_floor_128", place([floor, bx], 128, [3, 127]), q[::3])]


def class_hex():
    rng = np.random.default_rng(606)
    floor = box((-20, 0, -20), (20, 1, 20))
    walls = [box((2.0, 1, -0.25), (5.0, 3, 0.25), 0), box((-1.5, 1, 3.0), (1.5, 3, 3.5), 1), box((-6.0, 1, -0.25), (-3.0, 3, 0.25), 2),
             box((3.0, 1, 6.0), (4.0, 2, 7.0))]
    cols = place([floor] + walls, 64, [0, 1, 17, 40, 63])
    q = [_mode_queries(rng, cols[s], 90) for s in (1, 17, 40, 63)]
    # walks along and across the diagonals of a wall's footprint, in its frame: onto a vertical edge head-on and slightly off it, from all four corners
    frm, to = [], []
    for s in (1, 17, 40):
        lo, hi = cols[s]["lo"].astype(np.float64), cols[s]["hi"].astype(np.float64)
        for cx, cz in ((lo[0], lo[2]), (lo[0], hi[2]), (hi[0], lo[2]), (hi[0], hi[2])):
            inward = _unit(np.array([(lo[0] + hi[0]) / 2 - cx, 0.0, (lo[2] + hi[2]) / 2 - cz]))
            for _ in range(12):
                ang = rng.uniform(-0.5, 0.5)
                d = np.array([inward[0] * np.cos(ang) - inward[2] * np.sin(ang), 0.0, inward[0] * np.sin(ang) + inward[2] * np.cos(ang)])
                start = np.array([cx, hi[1] - rng.uniform(0.1, 0.7), cz]) - d * rng.uniform(0.3, 0.55)
                frm.append(_to_world(cols[s], start)); to.append(_to_world(cols[s], start + d * rng.uniform(0.1, 0.3)))
    q.append(queries(np.array(frm), np.array(to), forward=True))
    q = np.concatenate(q)
    return [Batch("hex", "three_frames_64", cols, q), Batch("hex", "three_frames_5", place([floor] + walls, 5), q[::2])]


def class_ball():
    """football_cases' geometries as single casts: dropped onto the resting ball at offsets 0, 0.3, 0.9, 1.3, and walked into from eight headings"""
    rng = np.random.default_rng(707)
    bl, floor, other = ball((6.0, 2.0, 6.0)), box((0, 0, 0), (14, 1, 12)), capsule((9.0, 1.815, 9.0))
    frm, to, up, msd = [], [], [], []
    for off in (0.0, 0.3, 0.9, 1.3):
        for _ in range(40):
            y0 = rng.uniform(3.6, 4.8)
            frm.append((6.0 + off, y0, 6.0)); to.append((6.0 + off, y0 - rng.uniform(0.2, 55.0 / 15.0), 6.0)); up.append(UP); msd.append(R.MAX_SLOPE_COS)
    for k in range(8):
        ang = np.pi / 4 * k
        u = np.array([np.cos(ang), 0.0, np.sin(ang)])
        for _ in range(40):
            r0 = rng.uniform(1.25, 1.7)
            p = np.array([6.0, 1.815, 6.0]) + u * r0
            side = np.array([-u[2], 0.0, u[0]]) * rng.uniform(-0.15, 0.15)
            q = p - u * rng.uniform(0.05, 0.3) + side
            frm.append(p); to.append(q); up.append(np.asarray(p, F32) - np.asarray(q, F32)); msd.append(0.0)
    q = np.zeros(len(frm), R.QUERY)
    q["from"], q["to"], q["up"], q["min_slope_dot"] = np.array(frm), np.array(to), np.array(up), np.array(msd)
    return [Batch("ball", "resting_ball", place([bl, other, floor], 3), q), Batch("ball", "resting_ball_64", place([bl, other, floor], 64, [0, 1, 63]), q[::2])]


def class_pushout():
    rng = np.random.default_rng(808)
    bx = box((10, 1, 10), (11, 2, 11))
    hix = F32(bx["hi"][0])
    pos = []
    for k in range(-3, 4):                                                 # depths around MAX_PEN_DEPTH, ulp by ulp and coarser
        pos.append((_ulps(hix + CR - F32(R.MAX_PEN_DEPTH), k), 1.9, 10.5))
    for depth in rng.uniform(0.03, 0.052, 60):
        pos.append((hix + CR - F32(depth), 1.9, 10.5))
    for _ in range(400):                                                   # anywhere in and around the box: faces, edges, corners, the inside
        pos.append(rng.uniform((9.6, 0.3, 9.6), (11.4, 2.8, 11.4)))
    out = [Batch("pushout", "box_1", bx.reshape(1), positions=np.array(pos, F32)),
           Batch("pushout", "box_65", place([bx], 65, [64]), positions=np.array(pos, F32)[::2])]
    # two walls facing each other 0.5 apart: each push out of one goes deeper than MAX_PEN_DEPTH into the other -- five pushes used up
    wa, wb = box((20, 1, 10), (21, 3, 12)), box((21.5, 1, 10), (22.5, 3, 12))
    pp = [(21.0 + g, 2.0, 11.0) for g in np.linspace(0.05, 0.45, 41)]
    for slots, n in (((0, 1), 2), ((1, 0), 2), ((3, 67), 128), ((130, 2), 256)):
        out.append(Batch("pushout", f"between_walls_{n}_{slots[0]}", place([wa, wb], n, slots), positions=np.array(pp, F32)))
    # a shallow first slot beside a deep later one; and capsules
    sh = box((30, 1, 10), (31, 2, 11))
    dp = box((31.55, 1, 10), (32.5, 2, 11))
    cp = capsule((40.0, 1.815, 10.0))
    ps = [(31.0 + float(CR) - s, 1.9, 10.5) for s in (0.0, 0.02, 0.035, 0.0405)]
    pc = [(40.0 + r * np.cos(a), 1.815 + dy, 10.0 + r * np.sin(a)) for r in (0.0, 1e-7, 0.3, 0.6, 0.62, 0.7) for a in (0.0, 2.0) for dy in (0.0, 0.9, 1.3)]
    out.append(Batch("pushout", "shallow_then_deep", place([sh, dp, cp], 64, [0, 63, 31]), positions=np.array(ps + pc, F32)))
    bl = ball((50.0, 2.0, 10.0))
    pb = [(50.0 + r, 2.0 + dy, 10.0) for r in (0.0, 0.5, 1.2, 1.29, 1.3, 1.4) for dy in (0.0, 0.5, 1.0)]
    out.append(Batch("pushout", "ball", place([bl, capsule((50.9, 2.0, 10.4))], 2), positions=np.array(pb, F32)))
    hw = box((2.0, 1, -0.25), (5.0, 3, 0.25), 1)
    ph = [_to_world(hw, np.array([rng.uniform(1.8, 5.2), 2.0, rng.uniform(-0.6, 0.6)])) for _ in range(60)]
    out.append(Batch("pushout", "hex_wall", place([hw], 1), positions=np.array(ph, F32)))
    return out


def _agent(pos, hv=(0.0, 0.0), vvel=0.0, voffset=0.0, step_offset=0.2, jump_speed=10.0, was_jumping=0):
    a = np.zeros((), R.AGENT)
    a["pos"], a["hvx"], a["hvz"], a["vvel"], a["voffset"] = pos, hv[0], hv[1], vvel, voffset
    a["step_offset"], a["jump_speed"], a["was_jumping"] = step_offset, jump_speed, was_jumping
    return a


def class_steps():
    """player_step scenes on one floor (top 1): a wall, inner and outer corners, a seam, ledges, a ceiling, a box to land on, an edge to walk off,
    another capsule -- and, for the Football variant, the ball"""
    floor = box((0, 0, 0), (40, 1, 40))
    wall_x, wall_z = box((0, 1, 0), (1, 4, 40)), box((0, 1, 0), (40, 4, 1))
    block = box((10, 1, 10), (11, 2, 11))
    seam_a, seam_b = box((14, 1, 5), (15, 3, 6)), box((15, 1, 5), (16, 3, 6))
    ledges = [box((20 + 2 * i, 1, 5), (21 + 2 * i, 1 + h, 8)) for i, h in enumerate((0.19, 0.20, 0.21))]
    ceiling = box((28, 2.95, 5), (30, 3.5, 8))
    table = box((32, 1, 5), (34, 1.6, 8))
    other = capsule((36.0, 1.0 + REST, 6.0))
    y = 1.0 + REST
    ag = []
    for deg in (0, 1, 5, 15, 30, 45, 60, 75, 85, 88, 89):                 # into the wall x in [0, 1) at 0 .. 89 degrees from its normal
        th = np.deg2rad(deg)
        for gap in (0.0, 0.05, 0.2):
            ag.append(_agent((1.0 + float(CR) - 0.04 + gap, y, 20.0), (-4.5 * np.cos(th), 4.5 * np.sin(th))))
    for deg in (40, 44, 45, 46, 50, 60, 80):                              # into the inner corner of the two walls until the target stops changing
        th = np.deg2rad(deg)
        for gap in (0.0, 0.03, 0.1):
            ag.append(_agent((1.0 + float(CR) - 0.04 + gap, y, 1.0 + float(CR) - 0.04 + gap), (-4.5 * np.cos(th), -4.5 * np.sin(th))))
    for off in (-0.2, 0.0, 0.2, 0.29, 0.4):                               # past and into the outer corner (the block's vertical edges)
        ag.append(_agent((11.0 + 0.29 + 0.1, y, 11.0 + off), (-4.5, 0.0)))
        ag.append(_agent((11.0 + 0.25, y, 11.0 + 0.25 + off * 0.1), (-3.0, -3.0)))
    for x in (14.6, 15.0, 15.4):                                          # along and into the seam between two boxes
        ag.append(_agent((x, y, 6.0 + float(CR) - 0.04), (3.0, -2.0)))
        ag.append(_agent((x, y, 6.0 + float(CR) + 0.1), (0.0, -4.5)))
    for i in range(3):                                                    # onto ledges of 0.19, 0.20, 0.21
        for gap in (0.0, 0.1):
            ag.append(_agent((20.0 + 2 * i - float(CR) + 0.04 - gap, y, 6.5), (4.5, 0.0)))
    for vv in (6.2, 4.0, 2.0, 0.5):                                       # head under a ceiling while jumping
        ag.append(_agent((29.0, y, 6.5), (1.0, 0.0), vvel=vv, jump_speed=6.2, was_jumping=1))
        ag.append(_agent((29.0, y + 0.3, 6.5), (0.0, 0.0), vvel=vv, jump_speed=6.2, was_jumping=1))
    for h in (0.05, 0.3, 1.0, 2.5):                                       # landing on a box; falling beside it
        ag.append(_agent((33.0, 1.6 + REST + h, 6.5), (0.5, 0.0), vvel=-3.0, jump_speed=6.2, was_jumping=1))
        ag.append(_agent((34.0 + 0.2, 1.6 + REST + h, 6.5), (0.0, 0.0), vvel=-3.0))
    for gap in (0.3, 0.1, 0.0, -0.1, -0.3):                               # walking off the box's edge
        ag.append(_agent((34.0 - gap, 1.6 + REST, 6.5), (4.5, 0.0)))
    for deg in (0, 20, 45, 80):                                           # against another capsule
        th = np.deg2rad(deg)
        ag.append(_agent((36.0 - 0.7 * np.cos(th), y, 6.0 - 0.7 * np.sin(th)), (4.5 * np.cos(th + 0.2), 4.5 * np.sin(th + 0.2))))
    ag.append(_agent((5.0, y, 30.0)))                                      # standing still; free fall; a free jump
    ag.append(_agent((5.0, y + 3.0, 30.0), vvel=-10.0))
    ag.append(_agent((5.0, y, 30.0), (2.0, 1.0), vvel=6.2, jump_speed=6.2, was_jumping=1))
    ag = np.array(ag)
    live = [floor, wall_x, wall_z, block, seam_a, seam_b] + ledges + [ceiling, table, other]
    out = [Batch("steps", "room_12", place(live, 12), agents=ag),
           Batch("steps", "room_64", place(live, 64, [0, 63, 1, 62, 2, 61, 3, 60, 4, 59, 5, 58]), agents=ag),
           Batch("steps", "room_128", place(live, 128, [127, 64, 63, 0, 100, 101, 20, 84, 21, 85, 22, 86]), agents=ag[::2]),
           Batch("steps", "room_256", place(live, 256, [255, 192, 128, 64, 1, 65, 129, 193, 2, 66, 130, 194]), agents=ag[::2])]
    bl = ball((6.0, 2.0, 6.0))
    fb = [_agent((6.0 + r * np.cos(a), y, 6.0 + r * np.sin(a)), (-4.5 * np.cos(a + t), -4.5 * np.sin(a + t)))
          for r in (1.25, 1.4, 1.6) for a in np.pi / 4 * np.arange(8) for t in (0.0, 0.5)]
    fb += [_agent((6.0 + off, 4.6 - h, 6.0), vvel=-4.0) for off in (0.0, 0.3, 0.9, 1.3) for h in (0.0, 0.5, 1.0)]
    out.append(Batch("steps", "ball_room", place([bl, capsule((9.0, y, 9.0)), box((0, 0, 0), (14, 1, 12)), box((0, 1, 0), (1, 4, 12))], 4), agents=np.array(fb)))
    hw = [box((-20, 0, -20), (20, 1, 20)), box((2.0, 1, -0.25), (5.0, 3, 0.25), 0), box((2.0, 1, -0.25), (5.0, 3, 0.25), 1), box((-6.0, 1, -0.25), (-3.0, 3, 0.25), 2)]
    hx = []
    for w in hw[1:]:
        for lx in (2.5, 3.5, 4.9, 5.2):
            for deg in (0, 30, 60, 85):
                th = np.deg2rad(deg)
                p = _to_world(w, np.array([lx, y, 0.25 + float(CR) - 0.04 + 0.02]))
                v = _to_world(w, np.array([4.5 * np.sin(th), 0.0, -4.5 * np.cos(th)]))
                hx.append(_agent(p, (v[0], v[2])))
    out.append(Batch("steps", "hex_walls", place(hw, 64, [0, 5, 33, 63]), agents=np.array(hx)))
    return out


CLASSES = {"boxes": class_boxes, "grazing": class_grazing, "threshold": class_threshold, "ties": class_ties, "slope": class_slope, "hex": class_hex,
           "ball": class_ball, "pushout": class_pushout, "steps": class_steps}
_cache = {}


def batches(cls=None):
    """every Batch of one class (or of all), generated once"""
    if not _cache:
        for k, fn in CLASSES.items():
            _cache[k] = fn()
    return _cache[cls] if cls else [b for k in CLASSES for b in _cache[k]]
