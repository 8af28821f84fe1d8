"""The float64 model the controller's sweeps and push-outs are judged against (numpy only; no implementation is imported).

Written from the geometry, not from mv_physics.h or oracle/mv_oracle.cpp: the agent is a vertical capsule (radius CAP_R, segment half length CAP_HH);
a collider is a box, a box in one of the three hex wall frames, another agent's capsule or the ball.  The capsule against a box is its CENTRE
against the box grown by CAP_HH in +-y, minus CAP_R (the records carry the grown bounds: growing them is the tick header's work, not the sweep's);
against a vertical segment of half length h it is the distance to the segment minus the summed radius R (another agent: h = 2 CAP_HH, R = 2 CAP_R;
the ball: h = CAP_HH, R = CAP_R + r_ball).  Inside a box the distance is taken through the nearest face.

The records (packed, 4-byte fields) are the ones mv_debug_sweep / mv_debug_recover / mv_debug_player_step and the oracle's twins take: COL, QUERY,
SWEEP_OUT, RECOVER_OUT, AGENT below.  Collider kinds are the device's: 0 none, 1 box, 2 capsule, 3 + f box in hex frame f, 7 the ball.

The model's parameters are the fp32 constants of the controller taken exactly (0.33f, 0.04f, 0.001f ... as float64 values, and the hex frames' fp32
rotation entries): a constant is part of the model, not a rounding error of it.

E -- the fp32 error of ONE distance evaluation, derived (u = 2^-24 is the unit roundoff, M = max(1, largest |coordinate| of the sweep's end points
-- and of a segment's ends, which the code forms as centre.y -+ half length --), |d| the sweep's length, |v| the centre's distance from its closest
point, at most |dist0| + 1.5 + |d| for dist0 the distance at the start and radii up to 1.33):
  x = p + lambda d: per coordinate one rounded product (<= u |d_j|) and one rounded sum (<= u M); lambda carries the roundings of its own quotient
  and sum (<= 3 u lambda: <= 3 u |d| of position)                                   -> position error <= sqrt(3) u (M + |d|) + 3 u |d| < 1.8 u M + 4.8 u |d|
  v = x - clamp(x): the clamp is exact (the bounds are inputs), the difference is rounded RELATIVE TO ITS RESULT                     -> u |v|
  the distance is 1-Lipschitz in the position, so the two above enter as they are;
  len2: three rounded products and two rounded sums (relative 3 u of d2 = 1.5 u of |v|), sqrt (u |v|), |v| - r (u |dist|), + 0.04 (u)   -> < 3.5 u |v| + 2 u
  sum: E < u (1.8 M + 4.8 |d| + 4.5 |v| + 2) <= u (1.8 M + 9.3 |d| + 4.5 |dist0| + 8.75); the code below uses
      E = u (2 M + 10 |d| + 5 |dist0| + 9.5),   and   u (8 M + 16 |d| + 5 |dist0| + 9.5) for a box in a hex frame
  (rotating the start and the direction into the frame: two rounded products and a sum per horizontal coordinate of each, < 6 u M + 6 u |d| more).

The rules (tests/test_physics_reference.py holds the oracle to them on the CPU, tests/test_physics_kernels_gpu.py the kernels):

(G) every reported hit, fragile or not.  x = from + fraction d (float64, from the reported fp32 fraction), w = the collider whose float64 normal the
    reported one matches.  The loop ends on fl(dist + 0.04f) <= 0.001f at the fp32 point, so signed_distance64(w, x) <= (0.001f - 0.04f) + E.  The
    distance of a convex set along a line is convex in the fraction, so an advancement step -- the tangent's root -- never passes the level it
    aims at: started shallower than 0.001f - 0.04f, the hit is no deeper than -0.04f - E, and fraction <= first_crossing64(level = -0.04f) + E / rho
    with rho = -(d . n64) the closing rate at the hit.  | |normal| - 1 | <= 4 u (one rounded reciprocal, one rounded product per coordinate, len2's
    three roundings); the normal is within E / |v| of the float64 gradient at x (v = the centre minus its closest point: an error E of v turns
    v / |v| by at most E / |v|; centre inside the grown box or on a capsule's axis: the normal is a constant and must be equal).

(D) hit or miss, the winner (seen through its normal) and the fraction equal sweep64's, the fraction within tol_lambda.  tol_lambda is carried
    through the float64 run: an advancement step is Newton's on f = dist + 0.04 with slope -rho, so an error e_k of lambda_k enters lambda_(k+1) only
    through the curvature, e_(k+1) <= kappa_k e_k + (E + step tol_rho) / rho + 4 u with kappa_k = f f'' / rho^2 <= step |d|^2 / (|v| rho), and
    tol_rho = sum_j (|d_j| nerr_j + 4 u |d_j n_j|) + |d|^2 e_k / |v| the error of the closing rate (nerr_j = E / |v|, or 0 for a coordinate of the
    normal that is exactly 0 or +-1 in fp32 too: a face, a capsule met level with its segment -- as long as the position is further than its error from
    where that ends; a hex frame adds the rounding of the rotated direction).  The rule is waived only where the float64 run is FRAGILE: some comparison
    lies within its tolerance of its threshold -- dist + 0.04 against CAST_RADIUS (E + rho e_k), the closing rate against eps (tol_rho; a comparison
    BOTH of whose outcomes end the cast as a miss decides nothing: where the step of the branch that goes on, at least dist / (rho + tol_rho + eps),
    leaves the sweep), lambda against 1 (e_k), the slope filter (the normal's error), a position within its error of where the normal jumps (a box's
    surface, the change of the nearest face inside it, a segment's axis), or two accepted hits with different normals whose fractions lie within the
    sum of their tolerances (an EXACT tie is not fragile: the lowest slot wins).  A fragile query
    still has to meet (G).  At most 1 % of the queries of any class but the threshold class may be fragile (FRAGILE_CAP).

(R) push-out: the collider pushed is the lowest slot deeper than MAX_PEN_DEPTH (fragile within E of it); the push runs along the outward normal by
    minus the distance, which takes a convex collider's distance to exactly 0: after each push the pushed collider's signed_distance64 at the new
    position is 0 +- E_R, E_R = E + 4 u (|push| + M + 1) (the push's own product and sum); the number of pushes equals recover64's.

Measured, not derived: nothing -- every bound above is derived.  For orientation, the largest ratios (seen / bound) the ORACLE (fp32, on the CPU) left
against them over the committed query set of tests/physics_cases.py (test_physics_reference.py prints them per class; coordinates up to 64, beyond
that unmeasured): MEASURED below.  No kernel was measured to set anything.
"""
import numpy as np

U = 2.0 ** -24
F32 = np.float32


def _c(x):
    return float(F32(x))


CAP_R = _c(0.33)
CAP_HH = float(F32(1.05) * F32(0.5))
ALLOWED_CCD_PEN = _c(0.04)
CAST_RADIUS = _c(0.001)
CAST_MAX_ITER = 64
SIMD_EPS = float(np.finfo(np.float32).eps)
MAX_PEN_DEPTH = _c(0.041)
MAX_SLOPE_COS = _c(0.70710678)
AXIS_D2 = _c(1e-12)                 # a capsule met within sqrt(1e-12) of its axis: the stated fallback normal (1, 0, 0)
HIT_LEVEL = CAST_RADIUS - ALLOWED_CCD_PEN   # -0.039: where a cast may stop
CCD_LEVEL = -ALLOWED_CCD_PEN                # -0.04: where it aims
HEX_C, HEX_S = _c(0.8660254), 0.5
KIND_NONE, KIND_BOX, KIND_CAPSULE, KIND_HEX0, KIND_BALL = 0, 1, 2, 3, 7
FRAGILE_CAP = 0.01

COL = np.dtype([("kind", "<i4"), ("lo", "<f4", 3), ("hi", "<f4", 3)])
QUERY = np.dtype([("from", "<f4", 3), ("to", "<f4", 3), ("up", "<f4", 3), ("min_slope_dot", "<f4")])
SWEEP_OUT = np.dtype([("hit", "<i4"), ("fraction", "<f4"), ("normal", "<f4", 3)])
RECOVER_OUT = np.dtype([("pushes", "<i4"), ("pos", "<f4", (5, 3))])
AGENT = np.dtype([("pos", "<f4", 3), ("hvx", "<f4"), ("hvz", "<f4"), ("vvel", "<f4"), ("voffset", "<f4"), ("step_offset", "<f4"),
                  ("jump_speed", "<f4"), ("was_jumping", "<i4"), ("reach2", "<f4")])

# the largest ratios (seen / derived bound) the oracle left, and the class they came from; orientation only, nothing is set from them
MEASURED = {"G_upper": (0.0, "every class: a hit ends well under -0.039"), "G_lower": (0.253, "boxes"), "G_crossing": (0.253, "boxes"),
            "G_normal": (0.417, "boxes"), "G_unit": (0.616, "boxes"), "D_lambda": (0.413, "boxes"), "D_normal": (0.212, "grazing"), "R_zero": (0.131, "pushout")}

WHY_HIT, WHY_AWAY, WHY_BEYOND, WHY_STALL, WHY_ITERS = 0, 1, 2, 3, 4
_FACE_N = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], np.float64)


def error_bound(cols, p, d):
    """E of the module header for colliders [..] (COL records) and sweeps from p [.., 3] along d [.., 3]"""
    cols, p, d = np.asarray(cols, COL), np.asarray(p, np.float64), np.asarray(d, np.float64)
    m = np.maximum(1.0, np.maximum(np.abs(p).max(-1), np.abs(p + d).max(-1)))
    segment = (cols["kind"] == KIND_CAPSULE) | (cols["kind"] == KIND_BALL)
    m = np.maximum(m, np.where(segment, np.abs(cols["lo"][..., 1]) + np.abs(cols["hi"][..., 0]), 0.0))   # (a segment's ends: centre.y -+ half length, rounded)
    hexf = (cols["kind"] >= KIND_HEX0) & (cols["kind"] < KIND_HEX0 + 3)
    dist0 = np.abs(closest64(cols, p)["dist"])
    return U * (np.where(hexf, 8.0, 2.0) * m + np.where(hexf, 16.0, 10.0) * np.linalg.norm(d, axis=-1) + 5.0 * dist0 + 9.5)


def _frame(kind):
    """(c, s) of the frame a collider's bounds are stated in: local = (c x - s z, y, s x + c z); the world's for everything but hex boxes"""
    f = kind - KIND_HEX0
    hexf = (f >= 0) & (f < 3)
    c = np.where(hexf, np.where(f == 2, 0.0, HEX_C), 1.0)
    s = np.where(hexf, np.where(f == 0, HEX_S, np.where(f == 1, -HEX_S, 1.0)), 0.0)
    return c, s


def _to_local(c, s, v):
    return np.stack([c * v[..., 0] - s * v[..., 2], v[..., 1], s * v[..., 0] + c * v[..., 2]], -1)


def _to_world(c, s, v):
    return np.stack([c * v[..., 0] + s * v[..., 2], v[..., 1], c * v[..., 2] - s * v[..., 0]], -1)


def closest64(cols, x):
    """cols [..] COL, x [.., 3] float64 (broadcast together) -> dict: dist (signed distance of the capsule's surface), n (unit outward normal, world),
    vlen (|v|: the centre's distance from its closest point; 0 where the normal is a stated constant: inside a box, on a capsule's axis),
    nloc (the normal in the collider's frame), zero [.., 3] (that coordinate of v is exactly 0) with inner [.., 3] (how far the position may move before
    it no longer is), border (the position's distance from where the normal jumps: a box's surface, the change of the nearest face inside it, a
    segment's axis)"""
    x = np.asarray(x, np.float64)
    cols, _ = np.broadcast_arrays(np.asarray(cols, COL), x[..., 0])
    x = np.broadcast_to(x, cols.shape + (3,))
    kind = cols["kind"]
    lo, hi = cols["lo"].astype(np.float64), cols["hi"].astype(np.float64)
    boxlike = (kind == KIND_BOX) | ((kind >= KIND_HEX0) & (kind < KIND_HEX0 + 3))
    c, s = _frame(kind)
    # ---- boxes (in their frame)
    pl = _to_local(c, s, x)
    q = np.minimum(np.maximum(pl, lo), hi)
    v = pl - q
    d = np.linalg.norm(v, axis=-1)
    outside = d > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        n_out = v / d[..., None]
    faces = np.stack([pl[..., 0] - lo[..., 0], hi[..., 0] - pl[..., 0], pl[..., 1] - lo[..., 1], hi[..., 1] - pl[..., 1],
                      pl[..., 2] - lo[..., 2], hi[..., 2] - pl[..., 2]], -1)
    fi = np.argmin(faces, -1)          # the first of equal faces, in the order -x +x -y +y -z +z
    fm = np.take_along_axis(faces, fi[..., None], -1)[..., 0]
    box_dist = np.where(outside, d - CAP_R, -fm - CAP_R)
    box_n = np.where(outside[..., None], n_out, _FACE_N[fi])
    inner = np.minimum(pl - lo, hi - pl)                           # how far inside the slab of each axis (negative: outside it)
    box_zero = np.where(outside[..., None], v == 0.0, True)        # coordinates of v that are exactly 0 as long as the position stays in the slab
    box_inner = np.where(outside[..., None], np.where(v == 0.0, inner, np.inf), (np.sort(faces, -1)[..., 1] - fm)[..., None] / 2)
    box_border = np.where(outside, d, np.sort(faces, -1)[..., 1] - fm)   # where the normal jumps: at the surface; inside, where the nearest face changes
    # ---- vertical segments
    h = hi[..., 0]
    rad = np.where(kind == KIND_BALL, hi[..., 1], 2.0 * CAP_R)
    qy = np.minimum(np.maximum(x[..., 1], lo[..., 1] - h), lo[..., 1] + h)
    vc = np.stack([x[..., 0] - lo[..., 0], x[..., 1] - qy, x[..., 2] - lo[..., 2]], -1)
    dc2 = (vc * vc).sum(-1)
    off = dc2 > AXIS_D2
    dc = np.sqrt(dc2)
    with np.errstate(invalid="ignore", divide="ignore"):
        cap_n = np.where(off[..., None], vc / dc[..., None], np.array([1.0, 0.0, 0.0]))
    cap_dist = np.where(off, dc - rad, -rad)
    seg = np.minimum(x[..., 1] - (lo[..., 1] - h), (lo[..., 1] + h) - x[..., 1])      # how far inside the segment's span
    zeros = np.zeros_like(off)
    cap_zero = np.where(off[..., None], np.stack([zeros, vc[..., 1] == 0.0, zeros], -1), True)
    cap_inner = np.stack([np.full(off.shape, np.inf), np.where(off, seg, np.inf), np.full(off.shape, np.inf)], -1)
    cap_border = np.abs(dc - np.sqrt(AXIS_D2))
    nloc = np.where(boxlike[..., None], box_n, cap_n)
    return {"dist": np.where(boxlike, box_dist, cap_dist), "n": np.where(boxlike[..., None], _to_world(c, s, box_n), cap_n), "nloc": nloc,
            "vlen": np.where(boxlike, np.where(outside, d, 0.0), np.where(off, dc, 0.0)),
            "zero": np.where(boxlike[..., None], box_zero, cap_zero), "inner": np.where(boxlike[..., None], box_inner, cap_inner),
            "border": np.where(boxlike, box_border, cap_border),
            "frame": (c, s)}


def signed_distance64(collider, p):
    """the signed distance of the capsule's surface, its centre at p, to one collider (a COL record), and the unit outward normal"""
    r = closest64(np.asarray(collider, COL), np.asarray(p, np.float64))
    return float(r["dist"]), r["n"]


def advance64_batch(cols, p, d, E=None):
    """Conservative advancement in float64, Bullet's plain form: lambda += dist / (-(d . n)) with the unit normal n, the code's thresholds (0.04, 0.001,
    64 iterations, lambda > 1, closing rate <= eps).  cols [..] COL against sweeps from p [.., 3] along d [.., 3] (broadcast together) -> dict of
    arrays: hit, lam, n, why (WHY_*), iters, rho (the closing rate at the end), vlen, tol_lam (the module header's e_k at the end), tol_n (the
    normal's error bound), margins {dist, rho, lam, border: the smallest distance of that decision quantity from its threshold over the run}, slack
    (the smallest of distance-from-threshold minus its tolerance over all comparisons of the run; < 0: FRAGILE), slacks (the same by quantity)"""
    p = np.asarray(p, np.float64)
    d = np.asarray(d, np.float64)
    cols = np.asarray(cols, COL)
    shape = np.broadcast_shapes(cols.shape, p.shape[:-1], d.shape[:-1])
    cols = np.broadcast_to(cols, shape).reshape(-1)
    p = np.broadcast_to(p, shape + (3,)).reshape(-1, 3)
    d = np.broadcast_to(d, shape + (3,)).reshape(-1, 3)
    E = error_bound(cols, p, d) if E is None else np.broadcast_to(np.asarray(E, np.float64), shape).reshape(-1)
    n_pairs = len(cols)
    dl = np.linalg.norm(d, axis=-1)
    c, s = _frame(cols["kind"])
    d_loc = _to_local(c, s, d)
    hexf = (cols["kind"] >= KIND_HEX0) & (cols["kind"] < KIND_HEX0 + 3)

    lam = np.zeros(n_pairs)
    tol = np.zeros(n_pairs)
    iters = np.zeros(n_pairs, np.int64)
    why = np.full(n_pairs, -1, np.int64)
    slack = np.full(n_pairs, np.inf)
    mg = {k: np.full(n_pairs, np.inf) for k in ("dist", "rho", "lam", "border")}
    sl = {k: np.full(n_pairs, np.inf) for k in ("dist", "rho", "lam", "border")}   # the same, minus the tolerance

    def evaluate(idx, lam_i, tol_i):
        r = closest64(cols[idx], p[idx] + lam_i[:, None] * d[idx])
        poserr = E[idx] + dl[idx] * tol_i
        zero = r["zero"] & (r["inner"] > poserr[:, None])          # exactly 0 in fp32 too
        alone = (~r["zero"]).sum(-1) == 1                           # one coordinate of v left: it is the whole of it, the normal's is exactly +-1
        exact = zero | ((~r["zero"]) & (alone & (zero.sum(-1) == 2))[:, None]) | (r["vlen"] == 0)[:, None]
        nerr = np.where(exact, 0.0, (E[idx] / np.maximum(r["vlen"], 1e-300))[:, None])
        rho = -(d_loc[idx] * r["nloc"]).sum(-1)
        curv = np.where(r["vlen"] > 0, dl[idx] ** 2 / np.maximum(r["vlen"], 1e-300), 0.0) * np.where(exact.all(-1), 0.0, 1.0)
        dh = np.abs(d[idx][:, 0]) + np.abs(d[idx][:, 2])
        dloc_err = np.where(hexf[idx], 2.0 * U * dh, 0.0)[:, None] * np.array([1.0, 0.0, 1.0])    # rotating the direction into a hex frame
        tol_rho = (np.abs(d_loc[idx]) * nerr).sum(-1) + curv * tol_i + ((4.0 * U * np.abs(d_loc[idx]) + dloc_err) * np.abs(r["nloc"])).sum(-1)
        return r, rho, tol_rho, curv, r["border"] - poserr, r["border"]

    def note(idx, key, dist_from, tolerance):
        mg[key][idx] = np.minimum(mg[key][idx], dist_from)
        sl[key][idx] = np.minimum(sl[key][idx], dist_from - tolerance)
        slack[idx] = np.minimum(slack[idx], dist_from - tolerance)

    def note_rho(idx, rho_i, tol_rho_i, dist_i):
        # both outcomes of this comparison end the cast as a miss -- it decides nothing -- where the step of the branch that goes on, at least
        # dist / (rho + tol_rho + eps), leaves the sweep
        away = np.abs(rho_i - SIMD_EPS)
        neutral = (dist_i > CAST_RADIUS + E[idx]) & (dist_i > (np.abs(rho_i) + tol_rho_i + SIMD_EPS) * (1.0 - lam[idx] + tol[idx] + 4.0 * U))
        note(idx, "rho", away, np.where(neutral, -np.inf, tol_rho_i))

    act = np.arange(n_pairs)
    r, rho, tol_rho, curv, bslack, braw = evaluate(act, lam, tol)
    dist = r["dist"] + ALLOWED_CCD_PEN
    n_now, vlen_now, rho_now, tolrho_now = r["n"].copy(), r["vlen"].copy(), rho.copy(), tol_rho.copy()
    slack = np.minimum(slack, bslack)
    sl["border"] = np.minimum(sl["border"], bslack)
    mg["border"] = np.minimum(mg["border"], braw)
    note_rho(act, rho, tol_rho, dist)
    away = rho <= SIMD_EPS
    why[act[away]] = WHY_AWAY
    act = act[~away]
    dist_a, rho_a, tolrho_a, curv_a = dist[~away], rho[~away], tol_rho[~away], curv[~away]
    for _ in range(CAST_MAX_ITER + 2):
        if len(act) == 0:
            break
        note(act, "dist", np.abs(dist_a - CAST_RADIUS), E[act] + rho_a * tol[act])
        done = ~(dist_a > CAST_RADIUS)
        why[act[done]] = WHY_HIT
        keep = ~done
        act, dist_a, rho_a, tolrho_a, curv_a = act[keep], dist_a[keep], rho_a[keep], tolrho_a[keep], curv_a[keep]
        if len(act) == 0:
            break
        # (the closing rate of this point was compared when it was evaluated)
        step = dist_a / rho_a
        kappa = step * curv_a / rho_a
        tol[act] = kappa * tol[act] + (E[act] + step * tolrho_a) / rho_a + 4.0 * U
        lam[act] = lam[act] + step
        note(act, "lam", np.abs(lam[act] - 1.0), tol[act])
        beyond = lam[act] > 1.0
        why[act[beyond]] = WHY_BEYOND
        keep = ~beyond
        act = act[keep]
        if len(act) == 0:
            break
        r, rho_a, tolrho_a, curv_a, bslack, braw = evaluate(act, lam[act], tol[act])
        dist_a = r["dist"] + ALLOWED_CCD_PEN
        n_now[act], vlen_now[act], rho_now[act], tolrho_now[act] = r["n"], r["vlen"], rho_a, tolrho_a
        slack[act] = np.minimum(slack[act], bslack)
        sl["border"][act] = np.minimum(sl["border"][act], bslack)
        mg["border"][act] = np.minimum(mg["border"][act], braw)
        iters[act] += 1
        over = iters[act] > CAST_MAX_ITER
        why[act[over]] = WHY_ITERS
        keep = ~over
        act, dist_a, rho_a, tolrho_a, curv_a = act[keep], dist_a[keep], rho_a[keep], tolrho_a[keep], curv_a[keep]
        if len(act) == 0:
            break
        # the next iteration's closing-rate test
        note_rho(act, rho_a, tolrho_a, dist_a)
        away = rho_a <= SIMD_EPS
        why[act[away]] = WHY_AWAY
        keep = ~away
        act, dist_a, rho_a, tolrho_a, curv_a = act[keep], dist_a[keep], rho_a[keep], tolrho_a[keep], curv_a[keep]
    assert len(act) == 0 and (why >= 0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_n = np.where(vlen_now > 0, E / np.maximum(vlen_now, 1e-300), 0.0) + np.where(vlen_now > 0, dl / np.maximum(vlen_now, 1e-300), 0.0) * tol \
            + (4.0 + 3.0 * hexf) * U
    out = {"hit": why == WHY_HIT, "lam": lam, "n": n_now, "why": why, "iters": iters, "rho": rho_now, "vlen": vlen_now, "tol_lam": tol, "tol_n": tol_n,
           "slack": slack, "E": E, "margins": mg, "slacks": sl}
    return {k: (v.reshape(shape + v.shape[1:]) if isinstance(v, np.ndarray) else {kk: vv.reshape(shape) for kk, vv in v.items()}) for k, v in out.items()}


def advance64(collider, p, d):
    """one cast: (hit, lambda, n, why, margins); margins: the smallest distance of any decision quantity from its threshold over the run, by quantity,
    and "slack": the smallest distance minus its tolerance (< 0: fragile)"""
    r = advance64_batch(np.asarray(collider, COL).reshape(1), np.asarray(p, np.float64).reshape(1, 3), np.asarray(d, np.float64).reshape(1, 3))
    margins = {k: float(v[0]) for k, v in r["margins"].items()}
    margins["slack"] = float(r["slack"][0])
    return bool(r["hit"][0]), float(r["lam"][0]), r["n"][0], int(r["why"][0]), margins


def first_crossing64_batch(cols, p, d, level):
    """the first t in [0, 1] at which the signed distance along p + t d falls to `level` (nan: it never does), for cols [K] against sweeps p, d [K, 3].
    The distance of a convex set along a line is convex in t: minimise (golden section), then bisect between the start and the minimum."""
    cols = np.asarray(cols, COL).reshape(-1)
    p, d = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    f = lambda t: closest64(cols, p + t[:, None] * d)["dist"] - level
    k = len(cols)
    a, b, g = np.zeros(k), np.ones(k), (np.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = b - g * (b - a), a + g * (b - a)
    f1, f2 = f(x1), f(x2)
    for _ in range(60):
        left = f1 <= f2
        b, a = np.where(left, x2, b), np.where(left, a, x1)
        nx1, nx2 = np.where(left, b - g * (b - a), x2), np.where(left, x1, a + g * (b - a))
        nf1, nf2 = np.where(left, np.nan, f2), np.where(left, f1, np.nan)
        x1, x2 = nx1, nx2
        f1 = np.where(left, f(x1), nf1)
        f2 = np.where(left, nf2, f(x2))
    cand = np.stack([0.5 * (a + b), np.ones(k), x1, x2], -1)
    fc = np.stack([f(cand[:, j]) for j in range(4)], -1)
    tm = np.take_along_axis(cand, np.argmin(fc, -1)[:, None], -1)[:, 0]
    never = fc.min(-1) > 0.0
    lo, hi = np.zeros(k), tm
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        above = f(mid) > 0.0
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    out = np.where(f(np.zeros(k)) <= 0.0, 0.0, hi)
    return np.where(never & (out > 0.0), np.nan, out)


def first_crossing64(collider, p, d, level):
    """one sweep's first crossing of `level` (None: never)"""
    t = float(first_crossing64_batch(np.asarray(collider, COL).reshape(1), np.asarray(p, np.float64).reshape(1, 3), np.asarray(d, np.float64).reshape(1, 3), level)[0])
    return None if np.isnan(t) else t


def sweep64(cols, queries):
    """the nearest accepted hit of every query over all colliders, the controller's filters applied (|n|^2 > 1e-4, fraction < 1, dot(up, n) >= minSlopeDot),
    ties towards the lowest slot.  cols [C] COL, queries [Q] QUERY -> dict: hit [Q], slot [Q] (-1: none), lam [Q], n [Q, 3], tol_lam, tol_n [Q] (the
    winner's), ties [Q, C] (accepted hits within tolerance of the winner's fraction, the winner included), fragile [Q], per (the per-pair result of
    advance64_batch, [Q, C], with "accepted" and "E")"""
    cols = np.asarray(cols, COL).reshape(-1)
    queries = np.asarray(queries, QUERY).reshape(-1)
    nq, nc = len(queries), len(cols)
    p = queries["from"].astype(np.float64)
    d = queries["to"].astype(np.float64) - p
    up = queries["up"].astype(np.float64)
    msd = queries["min_slope_dot"].astype(np.float64)
    per = advance64_batch(cols[None, :], p[:, None, :], d[:, None, :])
    present = (cols["kind"] != KIND_NONE)[None, :]
    slope = (up[:, None, :] * per["n"]).sum(-1)
    # the slope filter's tolerance: the error of each coordinate of the normal (0 for the exact ones is not tracked at the end point: the bound is tol_n)
    tol_slope = np.abs(up).sum(-1)[:, None] * per["tol_n"]
    exact_n = (per["vlen"] == 0)
    tol_slope = np.where(exact_n, 4.0 * U, tol_slope)
    hit = per["hit"] & present
    acc = hit & (per["lam"] < 1.0) & ~(slope < msd[:, None])
    fragile_pair = present & (per["slack"] < 0)
    fragile_pair |= hit & (np.abs(per["lam"] - 1.0) <= per["tol_lam"])
    fragile_pair |= hit & (np.abs(slope - msd[:, None]) <= tol_slope) & np.isfinite(msd)[:, None]
    lam = np.where(acc, per["lam"], np.inf)
    slot = np.where(acc.any(1), np.argmin(lam, 1), -1)      # argmin: the first of equal fractions == the lowest slot
    best = np.take_along_axis(lam, np.maximum(slot, 0)[:, None], 1)[:, 0]
    bt = np.take_along_axis(per["tol_lam"], np.maximum(slot, 0)[:, None], 1)[:, 0]
    with np.errstate(invalid="ignore"):
        ties = acc & (lam - best[:, None] <= per["tol_lam"] + bt[:, None])
    wn = np.take_along_axis(per["n"], np.maximum(slot, 0)[:, None, None], 1)[:, 0]
    other_normal = np.abs(per["n"] - wn[:, None, :]).max(-1) > 1e-6
    fragile = fragile_pair.any(1) | (ties & other_normal & (lam != best[:, None])).any(1)
    per["accepted"] = acc
    take = lambda a: np.take_along_axis(a, np.maximum(slot, 0)[:, None], 1)[:, 0]
    return {"hit": slot >= 0, "slot": slot, "lam": np.where(slot >= 0, best, 1.0), "n": np.where((slot >= 0)[:, None], wn, 0.0), "tol_lam": take(per["tol_lam"]),
            "tol_n": take(per["tol_n"]), "rho": take(per["rho"]), "vlen": take(per["vlen"]), "ties": ties, "exact_ties": acc & (lam == best[:, None]),
            "fragile": fragile, "per": per, "p": p, "d": d}


def recover64(cols, pos):
    """the push-out: the first slot deeper than MAX_PEN_DEPTH is pushed out by minus its distance along its normal, at most five times.
    cols [C] COL, pos [3] -> (pushes, positions [pushes, 3], slots [pushes], fragile: some slot up to the chosen one within E of MAX_PEN_DEPTH)"""
    cols = np.asarray(cols, COL).reshape(-1)
    cur = np.asarray(pos, np.float64).copy()
    out_pos, out_slot, fragile = [], [], False
    for _ in range(5):
        r = closest64(cols, cur[None, :])
        E = error_bound(cols, cur[None, :], np.zeros((1, 3)))
        pen = (r["dist"] < -MAX_PEN_DEPTH) & (cols["kind"] != KIND_NONE)
        near = (np.abs(r["dist"] + MAX_PEN_DEPTH) <= E) & (cols["kind"] != KIND_NONE)
        first = int(np.argmax(pen)) if pen.any() else len(cols)
        fragile |= bool(near[: first + 1].any())
        if first == len(cols):
            break
        cur = cur + r["n"][first] * (-r["dist"][first])
        out_pos.append(cur.copy())
        out_slot.append(first)
    return len(out_pos), np.array(out_pos).reshape(-1, 3), out_slot, fragile


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rules, applied to an implementation's records


def check_G(cols, queries, got, ref=None):
    """rule (G) on every reported hit of `got` (SWEEP_OUT [Q]).  -> (failures: list of text, ratios: dict of the largest got / bound seen)"""
    cols = np.asarray(cols, COL).reshape(-1)
    ref = ref or sweep64(cols, queries)
    fails, ratios = [], {"G_upper": 0.0, "G_lower": 0.0, "G_normal": 0.0, "G_crossing": 0.0, "G_unit": 0.0}
    I = np.nonzero(got["hit"] != 0)[0]
    if len(I) == 0:
        return fails, ratios
    p, d = ref["p"][I], ref["d"][I]
    f = got["fraction"][I].astype(np.float64)
    n32 = got["normal"][I].astype(np.float64)
    unit = np.abs(np.linalg.norm(n32, axis=-1) - 1.0)
    ratios["G_unit"] = float(unit.max() / (4.0 * U))
    for k in np.nonzero(unit > 4.0 * U)[0]:
        fails.append(f"query {I[k]}: |normal| - 1 = {unit[k]!r}")
    for k in np.nonzero(~((f >= 0.0) & (f < 1.0)))[0]:
        fails.append(f"query {I[k]}: fraction {f[k]!r} outside [0, 1)")
    x = p + f[:, None] * d
    r = closest64(cols[None, :], x[:, None, :])
    E = error_bound(cols[None, :], p[:, None, :], d[:, None, :])
    ntol = np.where(r["vlen"] > 0, E / np.maximum(r["vlen"], 1e-300), 0.0)
    ndiff = np.linalg.norm(r["n"] - n32[:, None, :], axis=-1)
    present = (cols["kind"] != KIND_NONE)[None, :]
    cand = present & (ndiff <= ntol) & (r["dist"] <= HIT_LEVEL + E)
    rs = np.maximum(ref["slot"][I], 0)
    w = np.where(np.take_along_axis(cand, rs[:, None], 1)[:, 0], rs, np.argmax(cand, 1))
    none = ~cand.any(1)
    for k in np.nonzero(none)[0]:
        # the collider that comes closest to explaining the hit, for the message
        j = int(np.argmin(np.where(present[0], np.maximum(ndiff[k] - ntol[k], 0) + np.maximum(r["dist"][k] - HIT_LEVEL - E[k], 0), np.inf)))
        fails.append(f"query {I[k]}: no collider is within {HIT_LEVEL!r} + E at fraction {f[k]!r} with the reported normal {n32[k].tolist()} "
                     f"(closest: slot {j}, dist64 {r['dist'][k, j]!r}, E {E[k, j]!r}, normal off by {ndiff[k, j]!r}, allowed {ntol[k, j]!r})")
    ok = ~none
    take = lambda a: np.take_along_axis(a, w[:, None], 1)[:, 0]
    dist_w, E_w, nt_w, nd_w = take(r["dist"]), take(E), take(ntol), take(ndiff)
    if ok.any():
        ratios["G_upper"] = float(((dist_w - HIT_LEVEL) / E_w)[ok].max())
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios["G_normal"] = float(np.where(nt_w > 0, nd_w / nt_w, 0.0)[ok].max())
    start = closest64(cols[w], p)["dist"]
    low = ok & (start > HIT_LEVEL + E_w)
    if low.any():
        ratios["G_lower"] = float(((CCD_LEVEL - dist_w) / E_w)[low].max())
        for k in np.nonzero(low & (dist_w < CCD_LEVEL - E_w))[0]:
            fails.append(f"query {I[k]}: slot {w[k]} is {dist_w[k]!r} deep at the hit, deeper than {CCD_LEVEL!r} - E ({E_w[k]!r})")
        L = np.nonzero(low)[0]
        t0 = first_crossing64_batch(cols[w[L]], p[L], d[L], CCD_LEVEL)
        nw = np.take_along_axis(r["n"], w[:, None, None], 1)[:, 0][L]
        rho = np.maximum(-(d[L] * nw).sum(-1), 1e-300)
        over = (f[L] - t0) * rho / E_w[L]
        have = ~np.isnan(t0)
        if have.any():
            ratios["G_crossing"] = float(over[have].max())
        for k in np.nonzero(have & (over > 1.0))[0]:
            fails.append(f"query {I[L[k]]}: fraction {f[L[k]]!r} is past the crossing of the contact depth at {t0[k]!r} (+ {E_w[L[k]] / rho[k]!r})")
    return fails, ratios


def check_D(cols, queries, got, ref=None):
    """rule (D): `got` against sweep64 wherever the float64 run is not fragile.  -> (failures, ratios, fragile [Q])"""
    ref = ref or sweep64(cols, queries)
    fails, ratios = [], {"D_lambda": 0.0, "D_normal": 0.0}
    for i in np.nonzero(~ref["fragile"])[0]:
        if bool(got["hit"][i]) != bool(ref["hit"][i]):
            fails.append(f"query {i}: hit {int(got['hit'][i])}, float64 says {bool(ref['hit'][i])} (slot {int(ref['slot'][i])}, fraction {ref['lam'][i]!r})")
            continue
        if not ref["hit"][i]:
            if float(got["fraction"][i]) != 1.0:
                fails.append(f"query {i}: a miss reports fraction {got['fraction'][i]!r}")
            continue
        dl = abs(float(got["fraction"][i]) - ref["lam"][i])
        tol = ref["tol_lam"][i] + U      # (+ the fraction's own fp32 representation)
        ratios["D_lambda"] = max(ratios["D_lambda"], dl / tol)
        if dl > tol:
            fails.append(f"query {i}: fraction {got['fraction'][i]!r}, float64 {ref['lam'][i]!r}: off by {dl!r}, allowed {tol!r}")
        dn = float(np.linalg.norm(got["normal"][i].astype(np.float64) - ref["n"][i]))
        ratios["D_normal"] = max(ratios["D_normal"], dn / ref["tol_n"][i])
        if dn > ref["tol_n"][i]:
            fails.append(f"query {i}: normal {got['normal'][i].tolist()}, float64's winner (slot {int(ref['slot'][i])}) has {ref['n'][i].tolist()}: "
                         f"off by {dn!r}, allowed {ref['tol_n'][i]!r}")
    return fails, ratios, ref["fragile"]


def check_R(cols, positions, got):
    """rule (R) on RECOVER_OUT records [n] for start positions [n, 3].  -> (failures, ratios, fragile [n])"""
    cols = np.asarray(cols, COL).reshape(-1)
    fails, ratios, frag = [], {"R_zero": 0.0}, np.zeros(len(positions), bool)
    present = cols["kind"] != KIND_NONE
    for i in range(len(positions)):
        want, _, _, fragile = recover64(cols, positions[i])
        frag[i] = fragile
        k = int(got["pushes"][i])
        if not 0 <= k <= 5:
            fails.append(f"position {i}: {k} pushes")
            continue
        prev = positions[i].astype(np.float64)
        chain_fragile = False
        for j in range(k):
            now = got["pos"][i, j].astype(np.float64)
            r = closest64(cols, prev[None, :])
            E = error_bound(cols, prev[None, :], np.zeros((1, 3)))
            pen = present & (r["dist"] < -MAX_PEN_DEPTH)
            near = present & (np.abs(r["dist"] + MAX_PEN_DEPTH) <= E)
            if not (pen | near).any():
                fails.append(f"position {i}: push {j} from {prev.tolist()} where nothing is deeper than MAX_PEN_DEPTH")
                break
            # the lowest slot deeper than MAX_PEN_DEPTH; a slot within E of it before that one may have been taken instead
            first = int(np.argmax(pen)) if pen.any() else len(cols)
            allowed = [s for s in np.nonzero(near)[0] if s <= first] + ([first] if first < len(cols) else [])
            chain_fragile |= bool(near[: first + 1].any())
            ok = False
            for s in allowed:
                ER = E[s] + 4.0 * U * (abs(r["dist"][s]) + np.abs(prev).max() + 1.0)
                after = float(closest64(cols[s], now)["dist"])
                moved = np.linalg.norm(now - (prev + r["n"][s] * (-r["dist"][s])))
                if abs(after) <= ER and moved <= ER:
                    ratios["R_zero"] = max(ratios["R_zero"], abs(after) / ER, moved / ER)
                    ok = True
                    break
            if not ok:
                s = allowed[-1]
                fails.append(f"position {i}: push {j} from {prev.tolist()} to {now.tolist()}: slot {s} (dist64 {r['dist'][s]!r}) is not left at distance 0 "
                             f"along its normal (it is at {float(closest64(cols[s], now)['dist'])!r})")
                break
            prev = now
        else:
            if not np.array_equal(got["pos"][i, k:], np.broadcast_to(got["pos"][i, k - 1] if k else positions[i].astype(F32), (5 - k, 3))) and k > 0:
                fails.append(f"position {i}: the entries after push {k} do not repeat the last position")
            if not (fragile or chain_fragile) and k != want:
                fails.append(f"position {i}: {k} pushes, float64 makes {want}")
        frag[i] |= chain_fragile
    return fails, ratios, frag


def merge_ratios(into, more):
    for k, v in more.items():
        into[k] = max(into.get(k, 0.0), v)
    return into
