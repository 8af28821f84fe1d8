"""Python restatement of the Football scenario for its tests: the episode generator (Env::reset + FootballScenario::reset + spawnAgents,
env.cpp:57-76, scenario_football.cpp:7-22,112-129, platforms.hpp:221-244, scenario_default.hpp:80-97) on boxagone_model's mt19937 / randRange /
frand, and one tick of the ball -- the stated sequential-impulse model of DESIGN.md section 7 (mv_tick_football.h: ball_step) plus
FootballScenario::step's kicks -- in np.float32, operation for operation in the device's source order, on the device's records (mv_types.h:
FootballBlob, FootballState)."""
import numpy as np

from boxagone_model import MT19937, frand, rand_range  # noqa: F401  (re-exported for the tests)

MAX_AGENTS, MAX_LAYOUT = 8, 8
F32 = np.float32
LAYOUT_BOX = np.dtype([("min", "<i4", 3), ("type", "<i4"), ("max", "<i4", 3), ("slot", "<i4")])
BLOB = np.dtype([
    ("seq", "<i4"), ("num_boxes", "<i4"), ("length", "<i4"), ("width", "<i4"), ("height", "<i4"), ("episode_len", "<f4"), ("pad", "<i4", 2),
    ("spawn", "<f4", (MAX_AGENTS, 3)), ("yaw_frand", "<f4", MAX_AGENTS), ("boxes", LAYOUT_BOX, MAX_LAYOUT),
])
STATE = np.dtype([
    ("pos", "<f4", 3), ("radius", "<f4"), ("vel", "<f4", 3), ("kicks", "<i4"), ("ang", "<f4", 3), ("contacts", "<i4"), ("force", "<f4", 3),
    ("pad", "<i4"),
])
assert BLOB.itemsize == 416 and STATE.itemsize == 64

# ---- constants, as the device forms them (mv_physics.h, mv_tick_football.h)
DT = F32(F32(1.0) / F32(15.0))
CAP_R = F32(0.33)
CAP_HH = F32(F32(1.05) * F32(0.5))
BALL_R = F32(1.0)
BALL0 = (F32(5.0), F32(5.0), F32(5.0))
BALL_G = F32(-10.0)
BALL_I = F32(1.6)
BALL_INV_I = F32(F32(1.0) / BALL_I)
BALL_MU = F32(F32(0.5) * F32(0.5))
BALL_MU_ROLL = F32(F32(0.1) * F32(0.5))
BALL_MU_SPIN = F32(F32(0.1) * F32(0.5))
BALL_BREAK = F32(0.02)
BALL_ERP, BALL_ERP2, BALL_SPLIT = F32(0.2), F32(0.8), F32(-0.04)
BALL_ITERS = 10
BALL_CAP_R = F32(BALL_R + CAP_R)
PLANE_SQRT12 = F32(0.7071067811865475244)
FLT_EPSILON = F32(np.finfo(np.float32).eps)
KICK_DIST, KICK_FORCE = F32(1.8), F32(70.0)
ACT_INTERACT = 1 << 8
ZERO = F32(0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the generator

def merge_room(L, H, W):
    """the room's voxels (floor + four walls H high) merged as every layout is: seeds in (y, z, x) order, grown along x, then z, then y"""
    solid = np.zeros((H, W, L), bool)
    solid[0] = True
    solid[:, :, 0] = solid[:, :, L - 1] = True
    solid[:, 0, :] = solid[:, W - 1, :] = True
    used = np.zeros_like(solid)

    def open_cell(x, y, z):
        return 0 <= x < L and 0 <= y < H and 0 <= z < W and solid[y, z, x] and not used[y, z, x]

    boxes = []
    for y in range(H):
        for z in range(W):
            for x in range(L):
                if not open_cell(x, y, z):
                    continue
                x1, z1, y1 = x + 1, z + 1, y + 1
                while open_cell(x1, y, z):
                    x1 += 1
                row_ok = lambda yy, zz: all(open_cell(xx, yy, zz) for xx in range(x, x1))  # noqa: E731
                while row_ok(y, z1):
                    z1 += 1
                while all(row_ok(y1, zz) for zz in range(z, z1)):
                    y1 += 1
                used[y:y1, z:z1, x:x1] = True
                boxes.append(((x, y, z), (x1, y1, z1)))
    return boxes


def generate(rng, num_agents, base_len):
    """one FootballBlob (seq 0), advancing `rng` as the host generator does"""
    out = np.zeros((), BLOB)
    rng.seed(rand_range(0, 1 << 30, rng))
    L = rand_range(14, 24, rng)
    W = rand_range(12, 24, rng)
    H = rand_range(3, 7, rng)
    out["length"], out["width"], out["height"] = L, W, H
    boxes = merge_room(L, H, W)
    out["num_boxes"] = min(len(boxes), MAX_LAYOUT)
    for i, (lo, hi) in enumerate(boxes[:MAX_LAYOUT]):
        out["boxes"][i]["min"], out["boxes"][i]["max"], out["boxes"][i]["type"] = lo, hi, 3
    taken, found = set(), []
    for _ in range(num_agents):
        for _attempt in range(10):
            x = rand_range(1, L - 1, rng)
            z = rand_range(1, W - 1, rng)
            if (x, z) in taken:
                continue
            taken.add((x, z))
            found.append((x, 1, z))
            break
    while len(found) < num_agents:
        found.append(found[0])
    for i, p in enumerate(found):
        out["spawn"][i] = p
    out["episode_len"] = base_len
    for i in range(num_agents):
        out["yaw_frand"][i] = frand(rng)
    return out


def episodes(num_agents, env_seed, n, base_len=60.0):
    rng = MT19937(env_seed)
    return [generate(rng, num_agents, base_len) for _ in range(n)]


def room_boxes(blob):
    """the room's boxes in world units (voxel size 1): [(lo, hi)] as float32 triples"""
    return [(tuple(F32(v) for v in blob["boxes"][i]["min"]), tuple(F32(v) for v in blob["boxes"][i]["max"])) for i in range(int(blob["num_boxes"]))]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the ball

def fmin_sel(a, b):
    return b if b < a else a


def fmax_sel(a, b):
    return b if a < b else a


def add(a, b):
    return (F32(a[0] + b[0]), F32(a[1] + b[1]), F32(a[2] + b[2]))


def sub(a, b):
    return (F32(a[0] - b[0]), F32(a[1] - b[1]), F32(a[2] - b[2]))


def mul(a, s):
    return (F32(a[0] * s), F32(a[1] * s), F32(a[2] * s))


def dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def cross(a, b):
    return (F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])), F32(F32(a[0] * b[1]) - F32(a[1] * b[0])))


def raw_box(p, lo, hi, r):
    """mv_physics.h raw_box: (v, d, dist)"""
    q = tuple(fmin_sel(fmax_sel(p[i], lo[i]), hi[i]) for i in range(3))
    v = sub(p, q)
    d2 = dot(v, v)
    if d2 > ZERO:
        d = F32(np.sqrt(d2))
        return v, d, F32(d - r)
    m, n = F32(p[0] - lo[0]), (F32(-1), ZERO, ZERO)
    for t, nn in ((F32(hi[0] - p[0]), (F32(1), ZERO, ZERO)), (F32(p[1] - lo[1]), (ZERO, F32(-1), ZERO)), (F32(hi[1] - p[1]), (ZERO, F32(1), ZERO)),
                  (F32(p[2] - lo[2]), (ZERO, ZERO, F32(-1))), (F32(hi[2] - p[2]), (ZERO, ZERO, F32(1)))):
        if t < m:
            m, n = t, nn
    return n, F32(1.0), F32(F32(-m) - r)


def raw_capsule(p, centre, half_len, r):
    qy = fmin_sel(fmax_sel(p[1], F32(centre[1] - half_len)), F32(centre[1] + half_len))
    v = (F32(p[0] - centre[0]), F32(p[1] - qy), F32(p[2] - centre[2]))
    d2 = dot(v, v)
    if d2 > F32(1e-12):
        d = F32(np.sqrt(d2))
        return v, d, F32(d - r)
    return (F32(1), ZERO, ZERO), F32(1.0), F32(-r)


def plane_space(n):
    if abs(n[2]) > PLANE_SQRT12:
        a = F32(F32(n[1] * n[1]) + F32(n[2] * n[2]))
        k = F32(F32(1.0) / F32(np.sqrt(a)))
        p = (ZERO, F32(-n[2] * k), F32(n[1] * k))
        q = (F32(a * k), F32(-n[0] * p[2]), F32(n[0] * p[1]))
    else:
        a = F32(F32(n[0] * n[0]) + F32(n[1] * n[1]))
        k = F32(F32(1.0) / F32(np.sqrt(a)))
        p = (F32(-n[1] * k), F32(n[0] * k), ZERO)
        q = (F32(-n[2] * p[1]), F32(n[2] * p[0]), F32(a * k))
    return p, q


def contact_setup(n, dist, v, w):
    r = (-n[0], -n[1], -n[2])
    vc = add(v, cross(w, r))
    slip = sub(vc, mul(n, dot(n, vc)))
    s2 = dot(slip, slip)
    p, q = plane_space(n)
    t = mul(slip, F32(F32(1.0) / F32(np.sqrt(s2)))) if s2 > FLT_EPSILON else p
    rt = cross(r, t)
    jf = F32(F32(1.0) / F32(F32(1.0) + F32(BALL_INV_I * dot(rt, rt))))
    if dist > ZERO:
        bias = F32(-dist / DT)
    elif dist > BALL_SPLIT:
        bias = F32(F32(-dist * BALL_ERP) / DT)
    else:
        bias = ZERO
    pbias = ZERO if dist > BALL_SPLIT else F32(F32(-dist * BALL_ERP2) / DT)
    return dict(n=n, t=t, rt=rt, p=p, q=q, dist=dist, jf=jf, bias=bias, pbias=pbias, ln=ZERO, lf=ZERO, lp=ZERO, lr=[ZERO, ZERO, ZERO])


def find_contacts(c, boxes, caps):
    """the ball's contacts at centre c: agents' capsules (ghost origins, index order), then the room's boxes -- [(n, dist)], contact bits"""
    out, bits = [], 0
    for j, o in enumerate(caps):
        v, d, dist = raw_capsule(c, o, CAP_HH, BALL_CAP_R)
        if dist <= BALL_BREAK:
            out.append((mul(v, F32(F32(1.0) / d)), dist))
            bits |= 1 << j
    for k, (lo, hi) in enumerate(boxes):
        v, d, dist = raw_box(c, lo, hi, BALL_R)
        if dist <= BALL_BREAK:
            out.append((mul(v, F32(F32(1.0) / d)), dist))
            bits |= 1 << (8 + k)
    return out, bits


def ball_step(s, boxes, caps):
    """mv_tick_football.h ball_step on a STATE record (copied): boxes [(lo, hi)], caps [ghost origin of every agent at the tick's start]"""
    s = s.copy()
    f = s["force"]
    v = (F32(s["vel"][0] + F32(F32(f[0] + ZERO) * DT)), F32(s["vel"][1] + F32(F32(f[1] + BALL_G) * DT)), F32(s["vel"][2] + F32(F32(f[2] + ZERO) * DT)))
    w = tuple(F32(x) for x in s["ang"])
    s["force"] = 0.0
    c = tuple(F32(x) for x in s["pos"])
    found, bits = find_contacts(c, boxes, caps)
    cs = [contact_setup(n, dist, v, w) for n, dist in found]
    for _ in range(BALL_ITERS):
        for k in cs:
            dl = F32(k["bias"] - dot(k["n"], v))
            tot = fmax_sel(F32(k["ln"] + dl), ZERO)
            d = F32(tot - k["ln"])
            k["ln"] = tot
            v = add(v, mul(k["n"], d))
        for k in cs:
            if not k["ln"] > ZERO:
                continue
            lim = F32(BALL_MU * k["ln"])
            vt = F32(dot(k["t"], v) + dot(k["rt"], w))
            tot = fmin_sel(fmax_sel(F32(k["lf"] + F32(ZERO - F32(vt * k["jf"]))), -lim), lim)
            d = F32(tot - k["lf"])
            k["lf"] = tot
            v = add(v, mul(k["t"], d))
            w = add(w, mul(k["rt"], F32(BALL_INV_I * d)))
        for k in cs:
            if not k["ln"] > ZERO:
                continue
            for a, (ax, mu) in enumerate(((k["n"], BALL_MU_SPIN), (k["p"], BALL_MU_ROLL), (k["q"], BALL_MU_ROLL))):
                lim = fmin_sel(F32(mu * k["ln"]), mu)
                va = dot(ax, w)
                tot = fmin_sel(fmax_sel(F32(k["lr"][a] + F32(ZERO - F32(va * BALL_I))), -lim), lim)
                d = F32(tot - k["lr"][a])
                k["lr"][a] = tot
                w = add(w, mul(ax, F32(BALL_INV_I * d)))
    vp = (ZERO, ZERO, ZERO)
    for _ in range(BALL_ITERS):
        for k in cs:
            if not k["pbias"] > ZERO:
                continue
            dl = F32(k["pbias"] - dot(k["n"], vp))
            tot = fmax_sel(F32(k["lp"] + dl), ZERO)
            d = F32(tot - k["lp"])
            k["lp"] = tot
            vp = add(vp, mul(k["n"], d))
    s["pos"] = [F32(F32(c[i] + F32(vp[i] * DT)) + F32(v[i] * DT)) for i in range(3)]
    s["vel"], s["ang"] = v, w
    s["contacts"] = bits
    s["radius"] = BALL_R
    return s


def kicks(s, agents_after, actions):
    """FootballScenario::step on a STATE record after ball_step (copied): agents_after = ghost origins after the controllers, actions = bit masks"""
    s = s.copy()
    n = 0
    for o, act in zip(agents_after, actions):
        if not act & ACT_INTERACT:
            continue
        d = (F32(s["pos"][0] - o[0]), F32(s["pos"][1] - F32(o[1] + F32(0.05))), F32(s["pos"][2] - o[2]))
        ln = F32(np.sqrt(dot(d, d)))
        if ln < KICK_DIST:
            inv = F32(F32(1.0) / ln)
            s["force"][0] = F32(s["force"][0] + F32(KICK_FORCE * F32(d[0] * inv)))
            s["force"][1] = F32(s["force"][1] + F32(KICK_FORCE * F32(0.5)))
            s["force"][2] = F32(s["force"][2] + F32(KICK_FORCE * F32(d[2] * inv)))
            n += 1
    s["kicks"] = n
    return s


def step(s, boxes, caps_before, caps_after, actions):
    """one tick of the ball: the model, then the kicks"""
    return kicks(ball_step(s, boxes, caps_before), caps_after, actions)


def reset_state():
    s = np.zeros((), STATE)
    s["pos"], s["radius"] = BALL0, F32(0.5)
    return s
