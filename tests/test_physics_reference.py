"""The float64 model of the controller's sweeps and push-outs (tests/physics_reference.py) on the CPU: the model against closed forms, the
fragile cap of every query class for the reference ALONE, the oracle's fp32 twins (mvo_debug_sweep / _recover / _player_step) against the rules
(G), (D) and (R) on every class -- the measured ratios are printed here --, and a rejection demo: a restated cast with one planted mistake fails
the rules although two copies of it agree bit for bit.  The GPU twin (test_physics_kernels_gpu.py) holds the kernels to the same rules."""
import functools

import numpy as np
import pytest

import canonical
import oracle_lib
import physics_cases as PC
import physics_reference as R

F32 = np.float32
SWEEP_CLASSES = [c for c in PC.CLASSES if c not in ("pushout", "steps")]


@functools.lru_cache(maxsize=None)
def reference(cls, name):
    """sweep64 of one batch, computed once and shared (tests must not change it)"""
    b = next(b for b in PC.batches(cls) if b.name == name)
    return R.sweep64(b.cols, b.queries)


# ---- (a) the model against closed forms -------------------------------------------------------------------------------------------------------------

def test_face_on_cast_is_one_exact_step():
    """face-on, the distance falls linearly: lambda = (gap + 0.04) / |d| in ONE iteration, for canonical.py's poses -- dropped one unit above the
    resting height on a movable box, three units in front of the wall x in [0, 1), a jump under a ceiling"""
    top = 1.5 - 0.05 + 0.39 * 1.15
    cases = [(PC.box((4, 1.0 - 0.05 + 0.5 - 0.39 * 1.15, 4), (5, top, 5)), (4.5, canonical.REST_ON(top) + 1.0, 4.5), (0.0, -55.0 / 15.0, 0.0)),
             (PC.box((0, 1, 0), (1, 4, 16)), (3.0, canonical.REST_ON(1.0), 8.0), (-2.0, 0.0, 0.0)),
             (PC.box((0, 4, 0), (8, 5, 8)), (4.0, canonical.REST_ON(1.0), 4.0), (0.0, 6.2, 0.0))]
    for col, p, d in cases:
        p, d = np.array(p, np.float64), np.array(d, np.float64)
        gap, n0 = R.signed_distance64(col, p)
        hit, lam, n, why, margins = R.advance64(col, p, d)
        assert hit and why == R.WHY_HIT
        assert abs(lam - (gap + R.ALLOWED_CCD_PEN) / np.linalg.norm(d)) <= 1e-15
        assert np.array_equal(n, n0) and abs(np.abs(n).sum() - 1.0) == 0.0          # an axis
        assert R.advance64_batch(col, p, d)["iters"] == 1
        assert abs(R.signed_distance64(col, p + lam * d)[0] - R.CCD_LEVEL) <= 1e-15
        assert abs(R.first_crossing64(col, p, d, R.CCD_LEVEL) - lam) <= 1e-12
    # the resting height itself: 0.04 inside the floor's nominal surface (REST_ON), to the rounding of the fp32 constants
    assert abs(R.signed_distance64(PC.box((0, 0, 0), (8, 1, 8)), (4.0, canonical.REST_ON(1.0), 4.0))[0] + canonical.CCD) <= 1e-7
    # two agents head-on (canonical.head_on: 3.0 and 9.0 along x): the summed radii
    assert abs(R.signed_distance64(PC.capsule((9.0, 1.8, 5.0)), (3.0, 1.8, 5.0))[0] - (6.0 - 2 * canonical.R)) <= 1e-7


def test_corner_cast_ends_at_the_quadratics_root():
    """towards a box's vertical edge the contact depth is reached where |p + t d - corner| = CAP_R - 0.04: the smaller root of a quadratic.  The
    advancement stops short of it by at most CAST_RADIUS / rho and never passes it; first_crossing64 finds it"""
    col = PC.box((10, 1, 10), (11, 3, 11))
    rng = np.random.default_rng(1)
    corner = np.array([11.0, 11.0])
    r = R.CAP_R - R.ALLOWED_CCD_PEN
    for _ in range(50):
        ang = rng.uniform(0.2, np.pi / 2 - 0.2)
        p = np.array([11.0 + 0.6 * np.cos(ang), 2.0, 11.0 + 0.6 * np.sin(ang)])
        aim = corner + rng.uniform(-0.1, 0.1, 2) * np.array([-np.sin(ang), np.cos(ang)])
        d = np.array([aim[0] - p[0], 0.0, aim[1] - p[2]]) * 0.9
        w = np.array([p[0] - corner[0], p[2] - corner[1]])
        dd = np.array([d[0], d[2]])
        a, b, c = dd @ dd, 2 * (w @ dd), w @ w - r * r
        root = (-b - np.sqrt(b * b - 4 * a * c)) / (2 * a)
        assert 0 < root < 1
        hit, lam, n, why, _ = R.advance64(col, p, d)
        assert hit
        rho = -(d @ n)
        assert root - R.CAST_RADIUS / rho - 1e-12 <= lam <= root + 1e-12, (lam, root)
        assert abs(R.first_crossing64(col, p, d, R.CCD_LEVEL) - root) <= 1e-9
        assert R.CCD_LEVEL - 1e-12 <= R.signed_distance64(col, p + lam * d)[0] <= R.HIT_LEVEL + 1e-12


def test_model_geometry_of_every_collider_kind():
    """the signed distance from the geometry: boxes through the nearest face inside, hex boxes in their wall's frame, segments with their radii"""
    bx = PC.box((0, 0, 0), (2, 1, 4))
    assert abs(R.signed_distance64(bx, (1.0, 1.0 + R.CAP_HH + 0.5, 2.0))[0] - (0.5 - R.CAP_R)) < 1e-12            # above the top
    dist, n = R.signed_distance64(bx, (1.9, 0.5, 2.0))                                                             # inside: out through +x
    assert abs(dist + 0.1 + R.CAP_R) < 1e-6 and n.tolist() == [1.0, 0.0, 0.0]
    dist, n = R.signed_distance64(bx, (2.3, 1.0 + R.CAP_HH + 0.4, 2.0))                                             # beside the top edge
    assert abs(dist - (0.5 - R.CAP_R)) < 1e-12 and abs(n[0] - 0.6) < 1e-12 and abs(n[1] - 0.8) < 1e-12
    for f, ang in ((0, np.pi / 6), (1, -np.pi / 6), (2, np.pi / 2)):   # frame f: the world turned about y by ang (c = cos, s = sin)
        hw = PC.box((2.0, 1, -0.25), (5.0, 3, 0.25), f)
        local = np.array([3.0, 2.0, 0.25 + 0.7])
        world = np.array([np.cos(ang) * local[0] + np.sin(ang) * local[2], local[1], np.cos(ang) * local[2] - np.sin(ang) * local[0]])
        dist, n = R.signed_distance64(hw, world)
        assert abs(dist - (0.7 - R.CAP_R)) < 1e-6
        assert np.allclose(n, [np.sin(ang), 0.0, np.cos(ang)], atol=1e-7)
    assert abs(R.signed_distance64(PC.capsule((0, 0, 0)), (1.0, 0.3, 0.0))[0] - (1.0 - 2 * R.CAP_R)) < 1e-12
    assert abs(R.signed_distance64(PC.capsule((0, 0, 0)), (0.0, 2 * R.CAP_HH + 1.0, 0.0))[0] - (1.0 - 2 * R.CAP_R)) < 1e-12
    assert abs(R.signed_distance64(PC.ball((0, 0, 0), 1.0), (2.0, 0.2, 0.0))[0] - (2.0 - R.CAP_R - 1.0)) < 1e-7
    assert abs(R.signed_distance64(PC.ball((0, 0, 0), 1.0), (0.0, R.CAP_HH + 2.0, 0.0))[0] - (2.0 - R.CAP_R - 1.0)) < 1e-7


# ---- (b) the fragile cap, for the reference alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [c for c in PC.CLASSES if c not in ("threshold", "steps")])
def test_fragile_cap_of_the_reference_alone(cls):
    """no implementation involved: the generators keep the float64 run's own margins clear of the thresholds for all but 1 % of a class"""
    fragile = total = 0
    for b in PC.batches(cls):
        if b.queries is not None:
            f = reference(cls, b.name)["fragile"]
            fragile, total = fragile + int(f.sum()), total + len(f)
        else:
            fl = [R.recover64(b.cols, p)[3] for p in b.positions]
            fragile, total = fragile + sum(fl), total + len(fl)
    print(f"{cls}: {fragile} of {total} fragile")
    assert total >= 500 and fragile <= R.FRAGILE_CAP * total, (cls, fragile, total)


def test_classes_reach_what_they_are_named_for():
    """a class cannot quietly stop exercising its edge: judged on the float64 run alone"""
    per = lambda cls: [(b, reference(cls, b.name)) for b in PC.batches(cls)]
    sizes = {len(b.cols) for b in PC.batches()}
    assert {1, 63, 64, 65, 128, 256} <= sizes
    for b, ref in per("boxes"):
        assert 0.3 < ref["hit"].mean() < 0.9 and ref["per"]["iters"].max() >= 3                # faces (1 step), edges and corners (more)
    graze = [ref for _, ref in per("grazing")]
    whys = np.concatenate([np.take_along_axis(r["per"]["why"], np.zeros((len(r["hit"]), 1), int), 1)[:, 0] for r in graze[2:]])
    assert (whys == R.WHY_HIT).any() and sum((~r["hit"]).sum() for r in graze) > 50           # under and over the contact depth
    thr = per("threshold")[0]
    tags = np.array(thr[0].meta["tags"])
    assert thr[1]["fragile"][tags == "start_on_radius"].any() and thr[1]["fragile"][tags == "lambda_one"].any()
    fwd = np.arange(len(tags)) < len(tags) // 2                                                  # (the second half repeats the queries under the slope filter)
    assert (thr[1]["hit"] & (thr[1]["lam"] == 0.0))[(tags == "start_inside") & fwd].all()
    assert not thr[1]["hit"][thr[0].meta["cull"]].any()
    for b, ref in per("ties"):
        if b.meta["first"] is not None:
            assert ref["hit"].all() and (ref["exact_ties"].sum(1) >= 2).all() and (ref["exact_ties"].sum(1) == 3).any()
            live = np.nonzero(ref["exact_ties"])                                                   # the reference's winner: the lowest slot of each tie
            assert all(ref["slot"][q] == np.nonzero(ref["exact_ties"][q])[0][0] for q in range(len(ref["slot"])))
    for b, ref in per("slope"):
        slope = (b.queries["up"].astype(np.float64)[:, None, :] * ref["per"]["n"]).sum(-1)
        edge = ref["per"]["hit"][:, np.argmax(b.cols["hi"][:, 1] > 3)]                            # the raised box's own cast
        s = slope[:, np.argmax(b.cols["hi"][:, 1] > 3)][edge]
        assert (s < R.MAX_SLOPE_COS).any() and (s > R.MAX_SLOPE_COS).any()
        rejected_then_floor = edge & (slope[:, np.argmax(b.cols["hi"][:, 1] > 3)] < R.MAX_SLOPE_COS) & ref["hit"]
        assert rejected_then_floor.sum() > 20                                                       # a nearer rejected hit, a farther accepted one
    for b, ref in per("hex"):
        kinds = b.cols["kind"][ref["slot"][ref["hit"]]]
        assert {3, 4, 5, 1} <= set(kinds.tolist())
    for b, ref in per("ball"):
        assert (b.cols["kind"][ref["slot"][ref["hit"]]] == R.KIND_BALL).sum() > 50
    pushes = np.concatenate([[R.recover64(b.cols, p)[0] for p in b.positions] for b in PC.batches("pushout")])
    assert {0, 1, 2, 5} <= set(pushes.tolist())


# ---- (c) the oracle's twins against the rules -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", SWEEP_CLASSES)
def test_oracle_sweeps_meet_G_and_D(cls):
    ratios = {}
    for b in PC.batches(cls):
        ref = reference(cls, b.name)
        got = oracle_lib.debug_sweep(b.cols, b.queries)
        fails_g, rg = R.check_G(b.cols, b.queries, got, ref)
        fails_d, rd, _ = R.check_D(b.cols, b.queries, got, ref)
        assert not fails_g and not fails_d, (b, (fails_g + fails_d)[:5])
        R.merge_ratios(ratios, rg); R.merge_ratios(ratios, rd)
    print(f"{cls}: the oracle's largest ratios against the derived bounds: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    assert all(v <= 1.0 for v in ratios.values())


def test_oracle_ties_go_to_the_lowest_slot():
    for b in PC.batches("ties"):
        if b.meta["first"] is None:
            continue
        got = oracle_lib.debug_sweep(b.cols, b.queries)
        PC.assert_lowest_slot_wins(b, got, lambda cols, q: oracle_lib.debug_sweep(cols, q))


def test_oracle_push_outs_meet_R():
    ratios = {}
    for b in PC.batches("pushout"):
        got = oracle_lib.debug_recover(b.cols, b.positions)
        fails, r, _ = R.check_R(b.cols, b.positions, got)
        assert not fails, (b, fails[:5])
        R.merge_ratios(ratios, r)
    print("pushout: the oracle's largest ratio against the derived bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values())


def test_oracle_steps_run_the_scenes():
    """class 9 on the oracle: the scenes do what they are named for (the plain loop's ten sweeps where the device's early exit fires; landings; pushes),
    the reach covers the step, and nothing ends deeper in a collider than a push-out leaves it unless the five pushes were used up"""
    for b in PC.batches("steps"):
        out, sweeps = oracle_lib.debug_player_step(b.cols, b.agents)
        assert np.isfinite(out["pos"]).all()
        assert (sweeps == 10).sum() >= 2 and (sweeps == 0).any() + (sweeps == 1).any() and ((sweeps >= 2) & (sweeps < 10)).any(), (b, np.bincount(sweeps))
        moved2 = ((out["pos"][:, [0, 2]].astype(np.float64) - b.agents["pos"][:, [0, 2]]) ** 2).sum(-1)
        assert (out["reach2"] >= moved2 * (1 - 1e-6)).all()
        landed = (b.agents["vvel"] < 0) & (out["vvel"] == 0)
        if b.name.startswith("room"):
            assert landed.any() and ((b.agents["vvel"] > 0) & (out["vvel"] == 0)).any()          # landed on the box; hit the ceiling
        for i in range(len(out)):
            dist = R.closest64(b.cols, out["pos"][i].astype(np.float64)[None, :])["dist"]
            again = oracle_lib.debug_recover(b.cols, out["pos"][i])
            assert dist.min() >= -(R.MAX_PEN_DEPTH + 1e-5) or again["pushes"][0] >= 1, (b, i, dist.min())


# ---- (d) rejection demo -----------------------------------------------------------------------------------------------------------------------------

def restated_sweep(cols, queries, mistake=None):
    """a plain fp32 restatement of the sweep (Bullet's form, scalar numpy float32), with one planted mistake: "hh" the boxes are not grown by CAP_HH,
    "ccd" the allowed penetration is dropped, "rawnormal" the unnormalised v is returned, "hightie" ties go to the highest slot"""
    f = F32
    r_cap, ccd, cast_r, eps = f(R.CAP_R), f(0.0 if mistake == "ccd" else R.ALLOWED_CCD_PEN), f(R.CAST_RADIUS), f(R.SIMD_EPS)
    out = np.zeros(len(queries), R.SWEEP_OUT)

    def closest(col, x):
        if col["kind"] == 1:
            lo, hi = col["lo"].copy(), col["hi"].copy()
            if mistake == "hh":
                lo[1] += f(R.CAP_HH); hi[1] -= f(R.CAP_HH)
            v = x - np.minimum(np.maximum(x, lo), hi)
            d2 = f(f(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if d2 > 0:
                d = np.sqrt(d2)
                return f(d - r_cap), v, d
            faces = np.array([x[0] - lo[0], hi[0] - x[0], x[1] - lo[1], hi[1] - x[1], x[2] - lo[2], hi[2] - x[2]], f)
            k = int(np.argmin(faces))
            return f(-faces[k] - r_cap), R._FACE_N[k].astype(f), f(1)
        h = col["hi"][0]
        qy = min(max(x[1], f(col["lo"][1] - h)), f(col["lo"][1] + h))
        v = np.array([x[0] - col["lo"][0], x[1] - qy, x[2] - col["lo"][2]], f)
        d = np.sqrt(f(f(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        return f(d - f(2) * r_cap), v, d

    for qi, q in enumerate(queries):
        p, d = q["from"], (q["to"] - q["from"]).astype(f)
        best, bn, hit = f(1), np.zeros(3, f), False
        for col in cols:
            if col["kind"] == 0:
                continue
            lam, x, it, ok = f(0), p, 0, True
            dist, v, vl = closest(col, x)
            dist = f(dist + ccd)
            n = (v / vl).astype(f)
            while dist > cast_r:
                proj = -f(f(d[0] * n[0] + d[1] * n[1]) + d[2] * n[2])
                if proj <= eps:
                    ok = False; break
                lam = f(lam + f(dist / proj))
                if lam > 1:
                    ok = False; break
                x = (p + lam * d).astype(f)
                dist, v, vl = closest(col, x)
                dist = f(dist + ccd)
                n = (v / vl).astype(f)
                it += 1
                if it > R.CAST_MAX_ITER:
                    ok = False; break
            proj0 = -f(f(d[0] * n[0] + d[1] * n[1]) + d[2] * n[2])
            if not ok or (lam == 0 and proj0 <= eps):
                continue
            nn = v if mistake == "rawnormal" else n
            if not (lam < best or (mistake == "hightie" and lam == best and hit)) or lam >= 1:
                continue
            if f(q["up"] @ n) < q["min_slope_dot"]:
                continue
            best, bn, hit = lam, nn, True
        out[qi] = (int(hit), best, bn)
    return out


def _demo_batches():
    boxes = next(b for b in PC.batches("boxes") if b.name == "voxel_5")
    ties = next(b for b in PC.batches("ties") if b.name == "corners_nc1")
    return [(boxes.cols, boxes.queries[::4], reference("boxes", "voxel_5")), (ties.cols, ties.queries, reference("ties", "corners_nc1"))]


def _sub(ref, idx):
    """the rows `idx` of a sweep64 result"""
    return {k: ({kk: (vv[idx] if isinstance(vv, np.ndarray) else {k3: v3[idx] for k3, v3 in vv.items()}) for kk, vv in v.items()} if isinstance(v, dict)
                else v[idx]) for k, v in ref.items()}


@pytest.mark.parametrize("mistake", [None, "hh", "ccd", "rawnormal", "hightie"])
def test_rules_reject_a_planted_mistake_that_parity_accepts(mistake):
    """two copies of the same restated cast agree bit for bit whatever is wrong with it -- that is all a parity test of code against its restatement can
    see.  The rules see each of the four mistakes; the unplanted restatement passes them"""
    fails = []
    for (cols, q, ref_all), step in zip(_demo_batches(), (4, 1)):
        ref = _sub(ref_all, np.arange(0, len(ref_all["hit"]), step))
        one, two = restated_sweep(cols, q, mistake), restated_sweep(cols, q, mistake)
        assert one.tobytes() == two.tobytes()                                       # "parity" holds
        fails += R.check_G(cols, q, one, ref)[0] + R.check_D(cols, q, one, ref)[0]
    if mistake is None:
        assert not fails, fails[:5]
    else:
        print(f"{mistake}: {len(fails)} violations, e.g. {fails[0] if fails else None}")
        assert len(fails) >= 10, (mistake, fails[:3])
