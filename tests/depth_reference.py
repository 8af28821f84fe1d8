"""What a depth plane (mv_set_depth_obs) must hold, in float64 closed forms derived from the lines tests/canonical_frames.py cites -- never read off a kernel.

The depth of a pixel is the ray parameter t of its nearest hit along the camera-space direction dc = (x, y, -1) (canonical_frames.ray): the PLANAR depth -z_cam
in world units, 0 where the ray hits nothing.  Forms:
  (a) a planar face seen square-on by a pitch-0 camera at distance d: t = d for EVERY pixel of the face (planar, not Euclidean);
  (b) the floor (top y = 1) under a standing agent: t = (EYE_Y - 1) / (-dc_y) for the rows below the horizon;
  (c) a movable box's front face at distance d: t = d;
  (d) cast_boxes: a float64 ray / AABB caster over the world boxes of a snapshot (its `boxes` records, and TowerBuilding's movable `objects` as cubes of
      half extent 0.39 around their voxel's centre), from the pose of the state-observation row -- camera as the oracle's camera_of_t (agent.cpp:33, :95,
      :110-126): eye 0.05 + 0.41 above the capsule centre, columns right / up / back, pitch about the local x axis;
  (e) cast_sphere: a float64 ray / sphere for Football's ball.

Compared pixels are INTERIOR ones: the 3 x 3 neighbourhood in the float64 oracle's `prim` map (oracle_lib.OracleGym.render_f64) shows one primitive, and
that primitive is a world box (a ball for (e)) -- or shows background alone, where the depth must be 0.  The neighbourhood is clipped to the frame, so the
frame's own border rows and columns -- the edge tiles' pixels -- are compared too.  uniform3x3 computes it; tests/test_depth_obs.py asserts on the CPU, on the
oracle alone, that every pose used keeps at least 80 % of the frame interior.

Tolerance for (a)-(d), derived.  A slab hit on axis k is (plane - eye_k) * (1 / dw_k): three roundings (the difference, the reciprocal, the product: 3 x 2^-24
relative), plus the relative error of dw_k, whose absolute error is a few 2^-24 (1 + tan 50 deg + tan_y) from the two products and two sums that form it.  So
    |d - t64| <= t64 (2^-21 + 2^-18 / |dw64_k|),   k the hit face's axis;
2^-18 is about four times the arithmetic bound, which covers the camera basis's own fp32 error (an fp32 sine and cosine of the pitch, products with the yaw
basis).  slab_model_f32 restates the formula in numpy float32, operation for operation; test_depth_obs.py asserts that it stays inside the bound against
cast_boxes at every compared pixel of every pose.  Largest ratio |model - t64| / bound seen over those poses: 0.031 (Empty, pitched down, 40 x 24).
For (e) the bound is measured the same way -- sphere_model_f32, the quadratic in numpy float32, against cast_sphere inside 0.8 of the ball's projected radius:
largest |model - t64| / t64 seen 7.8e-7 (128 x 128; the discriminant cancels), x 4 -> SPHERE_REL = 3.2e-6.  Never the kernel's own output.
Wrong conventions miss all of these by orders of magnitude: Euclidean depth differs from planar depth by up to 1 / cos 57 deg at the frame's corners, a
flipped row order swaps floor and sky, an off-by-one tile edge shifts a face's silhouette."""
import numpy as np

from canonical_frames import BOX_HALF, TAN, TAN_Y

NEAR_Z, FAR_Z = 0.01, 120.0
EYE_REST, EYE_UP = 0.05, 0.41
INTERIOR_SHARE = 0.8
SPHERE_REL = 3.2e-6
PRIM_BOX = 1   # oracle prim_table kind of a box; frame < 0: the world frame


def camera64(pos, basis, pitch):
    """the oracle's camera_of_t<double>: fp32 pose taken as given -> (eye [3], C [3, 3]: columns right / up / back in world space)"""
    x, y, z = (float(v) for v in pos)
    m00, m02, m20, m22 = (float(v) for v in basis)
    sp, cp = np.sin(float(pitch)), np.cos(float(pitch))
    eye = np.array([x, (y + EYE_REST) + EYE_UP, z])
    C = np.array([[m00, m02 * sp, m02 * cp], [0.0, cp, -sp], [m20, m22 * sp, m22 * cp]])
    return eye, C


def rays64(W, H):
    """camera-space directions through the pixel centres, [H, W, 3], row 0 the bottom row"""
    dcx = ((np.arange(W) + 0.5) / W * 2 - 1) * TAN
    dcy = ((np.arange(H) + 0.5) / H * 2 - 1) * TAN_Y
    dc = np.empty((H, W, 3))
    dc[..., 0], dc[..., 1], dc[..., 2] = dcx[None, :], dcy[:, None], -1.0
    return dc


def world_boxes(snap):
    """the world boxes of a snapshot -> (lo [n, 3], hi [n, 3]) float64: the layout's `boxes` and TowerBuilding's movable objects resting in the world"""
    nb = int(snap["num_boxes"])
    b = np.asarray(snap["boxes"][:nb])
    b = b[(b[:, 6] & 2) != 0].astype(np.float64)   # (the opaque ones: walls that are not drawn stay solid and unseen, layout_utils.cpp:17-50)
    lo, hi = [b[:, 0:3]], [b[:, 3:6]]
    if int(snap["scenario"]) == 0:   # TowerBuilding: the building zone's slab, 0.05 thick on the floor (layout_utils.cpp:53-68)
        bz = [float(v) for v in snap["bz"]]
        lo.append(np.array([[bz[0], 1.0, bz[2]]])); hi.append(np.array([[bz[1], 1.05, bz[3]]]))
    for o in snap["objects"][: int(snap["num_objects"])]:
        if int(o[3]) == 0:
            c = np.array([int(o[0]) + 0.5, int(o[1]) + 0.5, int(o[2]) + 0.5])
            lo.append((c - BOX_HALF)[None]); hi.append((c + BOX_HALF)[None])
    return np.concatenate(lo), np.concatenate(hi)


def cast_boxes(eye, C, W, H, lo, hi):
    """(d) float64 slab test of every pixel's ray against every box -> (t [H, W], inf for a miss; box [H, W] index, -1; axis [H, W] of the entry face;
    dwk [H, W] the world direction's component on that axis)"""
    dw = rays64(W, H) @ C.T
    t = np.full((H, W), np.inf); box = np.full((H, W), -1); axis = np.zeros((H, W), int)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dw
        for i in range(len(lo)):
            t1, t2 = (lo[i] - eye) * inv, (hi[i] - eye) * inv
            tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
            te, tx = tn.max(-1), tf.min(-1)
            ok = (te <= tx) & (te >= NEAR_Z) & (te <= FAR_Z) & (te < t)
            t[ok], box[ok], axis[ok] = te[ok], i, tn.argmax(-1)[ok]
    dwk = np.take_along_axis(dw, axis[..., None], -1)[..., 0]
    return t, box, axis, dwk


def slab_bound(t64, dwk64):
    """the derived tolerance of (a)-(d)"""
    return t64 * (2.0 ** -21 + 2.0 ** -18 / np.abs(dwk64))


def slab_model_f32(pos, basis, pitch, W, H, lo, hi, box, axis):
    """the kernel's slab formula restated in numpy float32, operation for operation, at the face cast_boxes found per pixel: camera from the fp32 pose,
    dw = (c_k0 dcx + c_k1 dcy) + (-c_k2), bounds relative to the eye, t = (plane - eye_k) * (1 / dw_k) with the nearer of the slab's two planes"""
    f = np.float32
    x, y, z = (f(v) for v in pos)
    m00, m02, m20, m22 = (f(v) for v in basis)
    sp, cp = f(np.sin(f(pitch))), f(np.cos(f(pitch)))
    eye = np.array([x, (y + f(EYE_REST)) + f(EYE_UP), z], f)
    C = np.array([[m00, m02 * sp, m02 * cp], [f(0), cp, -sp], [m20, m22 * sp, m22 * cp]], f)
    dcx = ((((np.arange(W, dtype=f) + f(0.5)) / f(W)) * f(2) - f(1)) * f(1.19175359)).astype(f)
    dcy = ((((np.arange(H, dtype=f) + f(0.5)) / f(H)) * f(2) - f(1)) * (f(1.19175359) / (f(128.0) / f(72.0)))).astype(f)
    out = np.zeros((H, W), f)
    for k in range(3):
        dwk = ((C[k, 0] * dcx)[None, :] + (C[k, 1] * dcy)[:, None]) + (-C[k, 2])
        with np.errstate(divide="ignore"):
            inv = (f(1) / dwk).astype(f)
        sel = (axis == k) & (box >= 0)
        b = np.where(box >= 0, box, 0)
        rlo = (lo[b, k].astype(f) - eye[k]).astype(f)
        rhi = (hi[b, k].astype(f) - eye[k]).astype(f)
        tk = np.minimum(rlo * inv, rhi * inv).astype(f)
        out[sel] = tk[sel]
    return out


def uniform3x3(prim):
    """pixels whose 3 x 3 neighbourhood in the float64 prim map, clipped to the frame, shows ONE primitive (or background alone)"""
    H, W = prim.shape
    p = np.pad(prim, 1, mode="edge")
    same = np.ones((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            same &= p[dy:H + dy, dx:W + dx] == prim
    return same


def interior_mask(prim, table, want):
    """the compared hit pixels: uniform3x3, and the one primitive p satisfies want(kind, frame)"""
    good = np.zeros(len(table) + 1, bool)
    for p in range(len(table)):
        good[p] = bool(want(int(table[p, 0]), int(table[p, 1])))
    return uniform3x3(prim) & (prim >= 0) & good[np.where(prim >= 0, prim, len(table))]


def background_mask(prim):
    """the compared no-hit pixels: uniform3x3 of background, where the depth must be 0"""
    return uniform3x3(prim) & (prim < 0)


def is_world_box(kind, frame):
    return kind == PRIM_BOX and frame < 0


def interior_share(prim):
    """the share of the frame that is interior (uniform3x3): what the 80 % condition is stated on"""
    return float(uniform3x3(prim).mean())


def cast_sphere(eye, C, W, H, centre, radius):
    """(e) float64 ray / sphere: the nearer root of |eye + t dw - centre|^2 = r^2 -> (t [H, W], inf for a miss; s [H, W]: the ray's distance from the
    centre's direction as a share of the projected radius, by the discriminant: 1 - disc / (r^2 |dw|^2) is sin^2 ratio)"""
    dw = rays64(W, H) @ C.T
    oc = np.asarray(centre, float) - eye
    A = (dw * dw).sum(-1); B = dw @ oc; Cc = oc @ oc - radius * radius
    disc = B * B - A * Cc
    with np.errstate(invalid="ignore"):
        t = np.where(disc >= 0, (B - np.sqrt(np.maximum(disc, 0))) / A, np.inf)
    t = np.where((t >= NEAR_Z) & (t <= FAR_Z), t, np.inf)
    # perpendicular distance of the centre from the ray, over the radius
    perp2 = np.maximum(oc @ oc - B * B / A, 0.0)
    return t, np.sqrt(perp2) / radius


def sphere_model_f32(pos, basis, pitch, W, H, centre, radius):
    """the quadratic of a unit-sphere hit in numpy float32 (the direction scaled by 1 / r, the nearer root (B - sqrt(B B - A C)) / A), from the fp32 camera"""
    f = np.float32
    x, y, z = (f(v) for v in pos)
    m00, m02, m20, m22 = (f(v) for v in basis)
    sp, cp = f(np.sin(f(pitch))), f(np.cos(f(pitch)))
    eye = np.array([x, (y + f(EYE_REST)) + f(EYE_UP), z], f)
    C = np.array([[m00, m02 * sp, m02 * cp], [f(0), cp, -sp], [m20, m22 * sp, m22 * cp]], f)
    dcx = ((((np.arange(W, dtype=f) + f(0.5)) / f(W)) * f(2) - f(1)) * f(1.19175359)).astype(f)
    dcy = ((((np.arange(H, dtype=f) + f(0.5)) / f(H)) * f(2) - f(1)) * (f(1.19175359) / (f(128.0) / f(72.0)))).astype(f)
    dw = np.stack([((C[k, 0] * dcx)[None, :] + (C[k, 1] * dcy)[:, None]) + (-C[k, 2]) for k in range(3)], -1).astype(f)
    r = f(radius)
    rel = ((np.asarray(centre, f) - eye) / r).astype(f)    # the centre relative to the eye, in radii
    d = (dw / r).astype(f)
    A = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f)
    B = ((d[..., 0] * rel[0] + d[..., 1] * rel[1]) + d[..., 2] * rel[2]).astype(f)
    Cc = f(((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2]) - f(1))
    disc = (B * B - A * Cc).astype(f)
    with np.errstate(invalid="ignore"):
        return np.where(disc >= 0, ((B - np.sqrt(np.maximum(disc, f(0)))) / A).astype(f), f(0))


# ---- the poses the known-answer tests use, applied alike to an OracleGym and a MegaverseGym (they share the debug hooks) ----------------------------------
SIZES = [(128, 128), (40, 24), (41, 23)]   # 40 x 24: W no multiple of 16, H none of the tile height; 41 x 23: odd W (the half-precision rows' other store path)
TOWER_ENVS, TOWER_SEED = 8, 3
EMPTY_ENVS, EMPTY_SEED = 4, 3
LOOK_DOWN, LOOK_UP = 1 << 9, 1 << 10       # action mask bits (agent.cpp:110-126); multi-discrete: the sixth action, 1 = down, 2 = up
EMPTY_POSES = {"pitch 0": [], "pitched up": [LOOK_UP] * 6, "pitched down": [LOOK_DOWN] * 8}
WALL_DIST, BOX_DIST = 3.0, 2.5
BALL_DIST, BALL_RADIUS = 4.0, 0.5


def _tick(g, n_agents, mask):
    """one tick in which every agent acts `mask`, undrawn, on either kind of gym"""
    if hasattr(g, "set_action_masks"):
        g.set_action_masks(np.full(n_agents, mask, np.int32)); g.step_norender()
    else:
        acts = np.zeros((n_agents, 6), np.int32)
        acts[:, 5] = 2 if mask & LOOK_UP else 1 if mask & LOOK_DOWN else 0
        g.set_actions_batched(acts); g.step_no_render()


def pose_tower_wall(og, gyms):
    """(a) + (b): square-on to the wall x in [0, 1) at WALL_DIST, standing on the floor -> env"""
    from canonical_frames import face_wall, find_wall_env
    hit = find_wall_env(og, TOWER_ENVS, 15, 1.5)
    assert hit, "no env with a drawn wall and a free lane among the first envs"
    for g in gyms:
        face_wall(g, hit[0], hit[1], WALL_DIST)
    return hit[0]


def pose_tower_box(og, gyms):
    """(c): square-on to the +x face of an isolated movable box at BOX_DIST -> (env, (ox, oz))"""
    from canonical import find_isolated_box
    from canonical_frames import REST_Y
    e, (ox, oz) = next((e, b) for e in range(TOWER_ENVS) for b in [find_isolated_box(og.snapshot(e))] if b)
    c, s = float(np.float32(np.cos(np.pi / 2))), float(np.float32(np.sin(np.pi / 2)))
    for g in gyms:
        g.debug_set_agent_pos(e, 0, ox + 0.5 + BOX_HALF + BOX_DIST, REST_Y, oz + 0.5)
        g.debug_set_agent_yaw(e, 0, c, s)
        g.debug_set_agent_velocity(e, 0, 0.0, 0.0, 0.0)
    return e, (ox, oz)


def pose_empty(gyms, name):
    """(d): env 0 of Empty as its reset left it, the camera pitched by looking up or down for a few ticks -> env"""
    for g in gyms:
        for mask in EMPTY_POSES[name]:
            _tick(g, EMPTY_ENVS, mask)
    return 0


def expected_boxes(snap, agent, W, H):
    """cast_boxes on a snapshot's world boxes from its agent's pose -> (t, box, axis, dwk, lo, hi)"""
    a = snap["agents"][agent]
    lo, hi = world_boxes(snap)
    eye, C = camera64(a["pos"], a["basis"], a["pitch"])
    return cast_boxes(eye, C, W, H, lo, hi) + (lo, hi)


def pose_football(gyms, n_agents=2):
    """(e): env 0 of Football; agent 0 at mid field looking along -x at pitch 0, the ball BALL_DIST in front of its eye at eye height, the other agent behind
    it -> (env, centre, radius)"""
    from canonical_frames import REST_Y
    c, s = float(np.float32(np.cos(np.pi / 2))), float(np.float32(np.sin(np.pi / 2)))
    centre = None
    for g in gyms:
        snap = g.snapshot(0) if hasattr(g, "snapshot") else None
        if snap is None:
            from hip_util import hip_snapshot
            snap = hip_snapshot(g, 0)
        ax, az = int(snap["L"]) / 2 + 3.0, int(snap["W"]) / 2 + 0.5
        g.debug_set_agent_pos(0, 0, ax, REST_Y, az); g.debug_set_agent_yaw(0, 0, c, s); g.debug_set_agent_velocity(0, 0, 0.0, 0.0, 0.0)
        g.debug_set_agent_pos(0, 1, ax + 3.0, REST_Y, az); g.debug_set_agent_velocity(0, 1, 0.0, 0.0, 0.0)
        eye_y = float((np.float32(REST_Y) + np.float32(EYE_REST)) + np.float32(EYE_UP))
        centre = (float(np.float32(ax - BALL_DIST)), eye_y, float(np.float32(az)))
        (g.set_football_state if hasattr(g, "set_football_state") else g.debug_set_football_state)(0, centre, radius=BALL_RADIUS)
    return 0, centre, BALL_RADIUS


def is_ball(kind, frame):
    return kind == 4   # the oracle's unit sphere scaled by its radius (build_prims)
