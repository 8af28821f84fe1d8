"""What a normal plane (mv_set_normal_obs) must hold, in float64 closed forms built on tests/depth_reference.py -- never read off a kernel.

The value of a pixel is the unit outward normal of the surface it shows, in the viewer's camera frame (x right, y up, z back: the columns of camera64's C),
with a 4th component 1; four zeros where the ray hits nothing.  Forms, each on the float64 camera of the fp32 pose (depth_reference.camera64):
  (a) a world box: n_cam = C^T (-sign(dw_axis) e_axis) = -sign(dw_axis) * row `axis` of C, axis and dw_axis from depth_reference.cast_boxes;
  (b) Football's ball: n_cam = C^T (P - centre) / r, P = eye + t dw the hit of depth_reference.cast_sphere, inside 0.8 of the projected radius as depth does;
  (c) another agent's capsule seen face to face (seg_reference.pose_face_to_face), on its cylinder part: the horizontal unit vector from the capsule's axis
      to the hit point, carried into camera space.  The capsule is overview_reference's: radius 0.35, half length 0.36, centre 0.05 + 0.09 above the pose.
Compared pixels are interior ones in depth's sense (depth_reference.uniform3x3 on the oracle's float64 prim map shows one primitive).

Tolerance: per component, |got - n64| <= FP32 term + format term.
  The fp32 term.  box_normal_f32, sphere_normal_f32 and capsule_normal_f32 restate the camera basis and the arithmetic of (a), (b), (c) in numpy float32,
  operation for operation; tests/test_normal_obs.py measures their largest component deviation from the float64 forms over the poses used (depth's poses at
  depth_reference.SIZES; the capsule pose at the same sizes) on the CPU and asserts 4 x that value stays inside the constants below -- 4 x for depth's
  reason: it covers the orderings and reciprocal forms a kernel may choose that the restatement does not.  Measured (largest, over every pose and size):
      (a) boxes     2.02e-8 (Empty, pitched; 0 at pitch 0: an fp32 sine / cosine and one product)  -> BOX_ABS     = 8.1e-8
      (b) ball      3.36e-6 (128 x 128; the hit's t carries the discriminant's cancellation, over r) -> SPHERE_ABS  = 1.35e-5
      (c) capsule   2.50e-6 (128 x 128; the same quadratic in the horizontal plane)                 -> CAPSULE_ABS = 1.0e-5
  The format term is derived: NORMAL_F16 rounds a value of magnitude <= 1 to nearest, at most half a unit of the last of 11 significant bits: 2^-12;
  NORMAL_SNORM8 is q(v) / 127 with |127 v - q(v)| <= 1/2: 1/254.
The device is judged against float64 within the sum; the kernel's own output never sets a bound.

Planar consistency (plane_normals, plane_bound): on a planar face the normal must agree with the normalised cross product of the camera-space positions
P = dc t of the pixel's four neighbours, t from a float32 depth plane.  With depth's slab_bound as each neighbour's error in t, the position errors are
e_i = |dc_i| slab_bound(t_i, |n . dc_i|) (n . dc is the ray's component on the face's axis, whichever frame the box lives in: the direction is rotated, the
dot product is not), and the cross product of the two differences a = P_east - P_west, b = P_north - P_south turns by at most
    (e_east + e_west) / |a| + (e_north + e_south) / |b|,   divided by sin of the angle between a and b;
computed in float64.  A pixel whose four neighbours do not lie on ONE face (the edge between two faces of a box runs through them) is recognised from the
depth plane alone -- the centre's position misses the neighbours' plane by more than the errors allow -- and left out.  Pixels whose bound is under PLANE_MAX_ANGLE are judged (the bound itself, plus the format term, is the tolerance on each component); the
rest are counted.  n in the conditioning term is the cross product's own direction, i.e. it comes from the depth plane, which its own tests hold to float64."""
import numpy as np

import depth_reference as dr
from overview_reference import CAPSULE_HL, CAPSULE_R, CAPSULE_UP

MV_NORMAL_F16, MV_NORMAL_SNORM8 = 0, 1
BOX_ABS, SPHERE_ABS, CAPSULE_ABS = 8.1e-8, 1.35e-5, 1.0e-5
FORMAT_ABS = {MV_NORMAL_F16: 2.0 ** -12, MV_NORMAL_SNORM8: 1.0 / 254.0}
PLANE_MAX_ANGLE = 0.02
PRIM_CAPSULE = 2   # oracle prim_table kind of an agent's capsule


# ---- the closed forms -------------------------------------------------------------------------------------------------------------------------------
def box_normals(C, axis, dwk):
    """(a) -> [H, W, 3]: -sign(dw_axis) * row `axis` of C"""
    return -np.sign(dwk)[..., None] * np.asarray(C)[axis]


def sphere_normals(eye, C, W, H, centre, radius, t):
    """(b) -> [H, W, 3] (nan where t is not finite)"""
    dw = dr.rays64(W, H) @ C.T
    with np.errstate(invalid="ignore"):
        P = eye + np.where(np.isfinite(t), t, np.nan)[..., None] * dw
    return ((P - np.asarray(centre, float)) / radius) @ C


def capsule_centre(pos):
    x, y, z = (float(v) for v in pos)
    return np.array([x, (y + dr.EYE_REST) + CAPSULE_UP, z])


def cast_capsule_cylinder(eye, C, W, H, centre, radius=CAPSULE_R, half_len=CAPSULE_HL):
    """(c) float64 ray / vertical cylinder: the nearer root in the horizontal plane, kept where the hit lies on the cylinder part
    -> (t [H, W], inf elsewhere; n_cam [H, W, 3])"""
    dw = dr.rays64(W, H) @ C.T
    ox, oz = eye[0] - centre[0], eye[2] - centre[2]
    A = dw[..., 0] ** 2 + dw[..., 2] ** 2
    B = ox * dw[..., 0] + oz * dw[..., 2]
    Cc = ox * ox + oz * oz - radius * radius
    disc = B * B - A * Cc
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0))) / A, np.inf)
        y = eye[1] + t * dw[..., 1]
        ok = np.isfinite(t) & (t >= dr.NEAR_Z) & (t <= dr.FAR_Z) & (np.abs(y - centre[1]) <= half_len)
        t = np.where(ok, t, np.inf)
        nw = np.stack([(ox + t * dw[..., 0]) / radius, np.zeros_like(t), (oz + t * dw[..., 2]) / radius], -1)
    return t, np.where(ok[..., None], nw, np.nan) @ C


# ---- the same in numpy float32, operation for operation ------------------------------------------------------------------------------------------------
def camera_f32(pos, basis, pitch):
    f = np.float32
    x, y, z = (f(v) for v in pos)
    m00, m02, m20, m22 = (f(v) for v in basis)
    sp, cp = f(np.sin(f(pitch))), f(np.cos(f(pitch)))
    eye = np.array([x, (y + f(dr.EYE_REST)) + f(dr.EYE_UP), z], f)
    C = np.array([[m00, m02 * sp, m02 * cp], [f(0), cp, -sp], [m20, m22 * sp, m22 * cp]], f)
    return eye, C


def rays_f32(C, W, H):
    f = np.float32
    dcx = ((((np.arange(W, dtype=f) + f(0.5)) / f(W)) * f(2) - f(1)) * f(1.19175359)).astype(f)
    dcy = ((((np.arange(H, dtype=f) + f(0.5)) / f(H)) * f(2) - f(1)) * (f(1.19175359) / (f(128.0) / f(72.0)))).astype(f)
    return np.stack([((C[k, 0] * dcx)[None, :] + (C[k, 1] * dcy)[:, None]) + (-C[k, 2]) for k in range(3)], -1).astype(f)


def tmul_f32(C, n):
    """C^T n as the kernel's mat_tmul: (c0k n0 + c1k n1) + c2k n2 per component"""
    f = np.float32
    return np.stack([((C[0, k] * n[..., 0] + C[1, k] * n[..., 1]) + C[2, k] * n[..., 2]).astype(f) for k in range(3)], -1)


def box_normal_f32(pos, basis, pitch, axis, dwk):
    """sgn * row `axis` of the fp32 camera matrix"""
    _, C = camera_f32(pos, basis, pitch)
    sgn = np.where(dwk > 0, np.float32(-1), np.float32(1))
    return (sgn[..., None] * C[axis]).astype(np.float32)


def sphere_normal_f32(pos, basis, pitch, W, H, centre, radius):
    """the scaled unit sphere: ray into unit space, the nearer root, the unit-space hit point scaled back by 1 / r, normalised, then C^T"""
    f = np.float32
    eye, C = camera_f32(pos, basis, pitch)
    dw = rays_f32(C, W, H)
    r = f(radius)
    rel = (np.asarray(centre, f) - eye).astype(f)
    oo = ((f(0) - rel) / r).astype(f)
    dd = (dw / r).astype(f)
    A = ((dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]).astype(f)
    B = ((oo[0] * dd[..., 0] + oo[1] * dd[..., 1]) + oo[2] * dd[..., 2]).astype(f)
    Cc = f(((oo[0] * oo[0] + oo[1] * oo[1]) + oo[2] * oo[2]) - f(1))
    disc = (B * B - A * Cc).astype(f)
    with np.errstate(invalid="ignore"):
        t = ((-B - np.sqrt(np.maximum(disc, f(0)))) / A).astype(f)
        nl = np.stack([(oo[k] + t * dd[..., k]).astype(f) for k in range(3)], -1)
        n = (nl / r).astype(f)
        n = (n * (f(1) / np.sqrt(((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(f)))[..., None]).astype(f)
    return np.where((disc >= 0)[..., None], tmul_f32(C, n), f(0))


def capsule_normal_f32(pos, basis, pitch, W, H, other_pos, radius=CAPSULE_R):
    """the cylinder part of ray_capsule: the horizontal quadratic, the hit point over r, then C^T"""
    f = np.float32
    eye, C = camera_f32(pos, basis, pitch)
    dw = rays_f32(C, W, H)
    ox, oz = f(eye[0] - f(other_pos[0])), f(eye[2] - f(other_pos[2]))
    r = f(radius)
    A = (dw[..., 0] * dw[..., 0] + dw[..., 2] * dw[..., 2]).astype(f)
    B = (ox * dw[..., 0] + oz * dw[..., 2]).astype(f)
    Cc = f((ox * ox + oz * oz) - r * r)
    disc = (B * B - A * Cc).astype(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = ((-B - np.sqrt(np.maximum(disc, f(0)))) / A).astype(f)
        inv = f(1) / r
        n = np.stack([((ox + t * dw[..., 0]) * inv).astype(f), np.zeros_like(t), ((oz + t * dw[..., 2]) * inv).astype(f)], -1)
    return tmul_f32(C, n)


# ---- the judge ---------------------------------------------------------------------------------------------------------------------------------------
def widen(plane):
    """a stored plane [..., 4] of float16 or int8 -> (xyz float64 [..., 3], w float64 [...])"""
    p = np.asarray(plane)
    v = p.astype(np.float64) / (127.0 if p.dtype == np.int8 else 1.0)
    return v[..., :3], v[..., 3]


def format_of(plane):
    return MV_NORMAL_SNORM8 if np.asarray(plane).dtype == np.int8 else MV_NORMAL_F16


def judge(plane, want, mask, fp_abs, background=None):
    """plane [H, W, 4] as stored against the float64 normals want [H, W, 3] at mask: every component within fp_abs + the format term, w == 1; four zeros at
    `background` -> (ok, largest error as a share of the bound)"""
    xyz, w = widen(plane)
    tol = fp_abs + FORMAT_ABS[format_of(plane)]
    if not mask.any():
        return False, np.inf
    err = np.abs(xyz[mask] - want[mask]).max(-1)
    ok = bool(np.isfinite(err).all() and (err <= tol).all() and (w[mask] == 1.0).all())
    if background is not None:
        ok = ok and not np.asarray(plane)[background].any()
    return ok, float(np.nanmax(err) / tol)


# ---- planar consistency ------------------------------------------------------------------------------------------------------------------------------
def plane_normals(depth, W, H):
    """depth [H, W] (float32 plane, 0: no surface) -> (n [H, W, 3]: the unit normal of the plane through the four neighbours' camera-space positions, facing
    the viewer; bound [H, W]: the angle it may be off by, inf at the frame's border and where a neighbour shows no surface) -- float64"""
    dc = dr.rays64(W, H)
    t = np.asarray(depth, np.float64)
    P = dc * t[..., None]
    n = np.full((H, W, 3), np.nan); bound = np.full((H, W), np.inf)
    e, w_, no, so = (slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)), (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))
    a, b = P[e] - P[w_], P[no] - P[so]
    c = np.cross(a, b)
    ln = np.linalg.norm(c, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = c / ln[..., None]
        nn = np.where((nn * dc[1:-1, 1:-1]).sum(-1)[..., None] > 0, -nn, nn)
        la, lb = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)
        sin_ab = ln / (la * lb)
        err = {}
        for name, s in (("e", e), ("w", w_), ("n", no), ("s", so)):
            along = np.abs((nn * dc[s]).sum(-1))
            err[name] = np.linalg.norm(dc[s], axis=-1) * dr.slab_bound(t[s], along)
        bd = ((err["e"] + err["w"]) / la + (err["n"] + err["s"]) / lb) / sin_ab
        # one face: were the five points coplanar up to their errors, the centre would lie within bd |P_c - P_k| + e_c + e_k of the plane through any
        # neighbour k.  A pixel whose neighbours straddle an edge of its box misses that by about a pixel's spacing: it is not judged
        ctr = (slice(1, -1), slice(1, -1))
        e_c = np.linalg.norm(dc[ctr], axis=-1) * dr.slab_bound(t[ctr], np.abs((nn * dc[ctr]).sum(-1)))
        flat = np.ones(ln.shape, bool)
        for name, s in (("e", e), ("w", w_), ("n", no), ("s", so)):
            off = P[ctr] - P[s]
            flat &= np.abs((nn * off).sum(-1)) <= bd * np.linalg.norm(off, axis=-1) + e_c + err[name]
    have = (t[e] > 0) & (t[w_] > 0) & (t[no] > 0) & (t[so] > 0) & (t[1:-1, 1:-1] > 0) & np.isfinite(bd) & flat
    n[1:-1, 1:-1] = np.where(have[..., None], nn, np.nan)
    bound[1:-1, 1:-1] = np.where(have, bd, np.inf)
    return n, bound


def interior5(prim):
    """pixels whose 5 x 5 neighbourhood shows ONE primitive: the four neighbours of the cross product are interior too (their own 3 x 3 is uniform)"""
    H, W = prim.shape
    p = np.pad(prim, 2, mode="edge")
    same = np.ones((H, W), bool)
    for dy in range(5):
        for dx in range(5):
            same &= p[dy:H + dy, dx:W + dx] == prim
    same[:2] = same[-2:] = False; same[:, :2] = same[:, -2:] = False
    return same


def box_interior(prim, table):
    """interior BOX pixels (any frame of reference) for the planar check"""
    kinds = np.append(np.asarray(table)[:, 0], 0)
    return interior5(prim) & (prim >= 0) & (kinds[np.where(prim >= 0, prim, len(table))] == dr.PRIM_BOX)


def reference_boxes(snap):
    """every box the snapshot states in the WORLD frame -> (lo [n, 3], hi [n, 3]) float64: depth_reference.world_boxes' list and, for the scenarios whose
    structure is HexRec records (HexMemory, HexExplore, BoxAGone, Football), the records whose frame nibble is 0 (overview_reference reads Football's the same
    way); a record in a rotated wall frame has no float64 depth here"""
    lo, hi = dr.world_boxes(snap)
    recs = [b for b in snap["hex_boxes"][: int(snap["hex_num_boxes"])] if int(b["meta"]) & 15 == 0]
    if recs:
        lo = np.concatenate([lo, np.array([np.asarray(b["a"], np.float64) for b in recs])])
        hi = np.concatenate([hi, np.array([np.asarray(b["b"], np.float64) for b in recs])])
    return lo, hi


# ---- planted mistakes the judge must reject ------------------------------------------------------------------------------------------------------------
def pack(xyz, hit, fmt):
    """float64 normals -> a stored plane, in numpy (the rule of mv_normal_obs.h)"""
    v = np.where(hit[..., None], np.asarray(xyz, np.float32), np.float32(0))
    if fmt == MV_NORMAL_F16:
        out = np.concatenate([v.astype(np.float16), np.where(hit, np.float16(1), np.float16(0))[..., None]], -1)
    else:
        c = np.clip(v, np.float32(-1), np.float32(1))
        q = (np.float32(127) * c + np.where(v >= 0, np.float32(0.5), np.float32(-0.5))).astype(np.float32).astype(np.int32)
        out = np.concatenate([q, np.where(hit, 127, 0)[..., None]], -1).astype(np.int8)
    return out


def planted(want, hit, C):
    """name -> wrong normals [H, W, 3] built from the right ones"""
    return {
        "rows flipped": want[::-1],
        "world space": want @ np.asarray(C).T,      # C n_cam = n_world
        "inward": -want,
        "un-normalised": want * 0.9,                # (shorter, not longer: SNORM8 clamps a component above 1)
        "one tile shift": np.roll(want, 16, axis=1),
    }
