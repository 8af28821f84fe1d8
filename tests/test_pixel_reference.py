"""The float64 reference of the render model (oracle: mvo_render_f64 / mvo_explain_f64) and the pixel acceptance rule built on it
(tests/pixel_reference.py), on the CPU: the oracle's own fp32 frames pass the rule over the whole matrix, delta_px is the figure
measured here, the matrix covers every primitive kind and frame class, the rule rejects what the old count rule accepts, and the reference agrees with
the hand-derived frames of test_canonical_frames.py.  The GPU twin (test_pixel_reference_gpu.py) holds the kernels to the same rule."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
import pixel_reference as pr
import test_canonical_frames as canon

os.environ.setdefault("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels

CELLS = [(s, a, w, h) for s, a in pr.MATRIX for w, h in pr.SIZES + ([pr.SIZES_LARGE[s]] if s in pr.SIZES_LARGE else [])]


@functools.lru_cache(maxsize=None)
def cell(scenario, A, W, H):
    """the oracle's fp32 frames of one matrix cell under the rule -> (verdict at DELTA_ORACLE, verdict with no probes but the centre, kinds and frame
    classes that win pixels)"""
    og = oracle_lib.OracleGym(scenario, W, H, pr.N_ENVS, A, 1)
    og.seed(pr.SEED); og.reset()
    v, centre = pr.Verdict(f"oracle fp32 {scenario} A={A} {W}x{H}"), pr.Verdict(f"oracle fp32 {scenario} A={A} {W}x{H}, centre only")
    kinds, classes = set(), set()
    for tick in range(pr.TICKS + 1):
        if tick % pr.EVERY == 0:
            if tick:
                og.render()
            for e in range(pr.N_ENVS):
                for a in range(A):
                    ref = pr.reference(og, e, a)
                    got = og.get_observation(e, a)
                    pr.judge(v, og, e, a, got, pr.DELTA_ORACLE, pr.EPS_4ULP, ref)
                    pr.judge(centre, og, e, a, got, 0.0, pr.EPS_4ULP, ref)
                    _, prim, table = ref
                    for p in np.unique(prim[prim >= 0]):
                        kinds.add(int(table[p, 0])); classes.add(pr.frame_class(int(table[p, 1]), a))
        if tick < pr.TICKS:
            pr.step_oracle(og, pr.N_ENVS, A, tick)
    og.close()
    return v, centre, kinds, classes


@pytest.mark.parametrize("scenario,A,W,H", CELLS)
def test_oracle_fp32_frames_pass_the_rule(scenario, A, W, H):
    """every pixel of the fp32 oracle's frames is right or explained against the float64 reference, the explained share within the cap: the seeds
    and poses of the matrix are fit to hold the kernels to"""
    cell(scenario, A, W, H)[0].check()


def test_what_the_oracle_needs_of_delta_px():
    """The measurement pixel_reference.py's header reports: over the whole matrix the oracle's fp32 frames need NO probe beside the centre -- every
    pixel of theirs that is not right is a curved primitive's hit that the reference's own criterion (moved discriminants) accounts for; no box edge
    falls within fp32 rounding of a pixel centre in these 2.2 M pixels.  So DELTA_ORACLE is the arithmetic bound, and this test keeps that true."""
    wrong = need_criterion = pixels = 0
    for c in CELLS:
        _, centre, _, _ = cell(*c)
        assert not centre.failures, centre.line()
        wrong += len(centre.explained); need_criterion += len(centre.ill); pixels += centre.pixels
    print(f"oracle fp32 against float64: {pixels} px, not right {wrong} ({wrong / pixels:.2e}), of them accepted only by the criterion {need_criterion}")
    assert 0 < wrong <= pr.CAP * pixels


def test_matrix_covers_every_primitive_kind_and_frame_class():
    kinds, classes = set(), set()
    for c in CELLS:
        _, _, k, cl = cell(*c)
        kinds |= k; classes |= cl
    assert kinds == {1, 2, 3, 4, 5, 6}, f"primitive kinds that win a pixel somewhere in the matrix: {sorted(kinds)}"
    assert classes == {"world", "viewer", "other agent", "hex"}, f"frame classes that win a pixel somewhere in the matrix: {sorted(classes)}"


def old_count_rule_accepts(ref, got):
    """test_fast_pixels_gpu.compare as it stands (that module needs the device extension to import, so its two assertions are restated)"""
    PIX_GT1, PIX_ANY = 1e-4, 5e-4
    d = np.abs(ref.astype(np.int16) - got.astype(np.int16)).max(axis=-1)
    return got[..., 3].min() == 255 and int((d > 1).sum()) <= max(2, PIX_GT1 * d.size) and int((d > 0).sum()) <= max(4, PIX_ANY * d.size)


@pytest.fixture(scope="module")
def tower_frame():
    og = oracle_lib.OracleGym("TowerBuilding", 64, 64, pr.N_ENVS, 2, 1)
    og.seed(pr.SEED); og.reset()
    for tick in range(40):
        pr.step_oracle(og, pr.N_ENVS, 2, tick)
    og.render()
    e, a = next((e, a) for e in range(pr.N_ENVS) for a in range(2) if (og.get_observation(e, a)[..., :3].max(axis=-1) > 0).mean() > 0.5)
    frames = {(i, j): og.get_observation(i, j).copy() for i in range(pr.N_ENVS) for j in range(2)}   # the frame set a GPU test compares at this tick
    yield og, e, a, frames, pr.reference(og, e, a)
    og.close()


def interior(prim, rgba, got, margin=2):
    """pixels that are right and not within `margin` pixels of a pixel whose winning primitive differs"""
    H, W = prim.shape
    same = np.ones_like(prim, bool)
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            sh = np.full_like(prim, -3)
            sh[max(0, dy): H + min(0, dy), max(0, dx): W + min(0, dx)] = prim[max(0, -dy): H + min(0, -dy), max(0, -dx): W + min(0, -dx)]
            same &= sh == prim
    right = np.abs(got[..., :3].astype(np.int16) - rgba[..., :3].astype(np.int16)).max(axis=-1) <= 1
    return same & right


def test_the_rule_has_teeth_where_the_count_rule_has_none(tower_frame):
    og, e, a, frames, ref = tower_frame
    frame, (rgba, prim, table) = frames[(e, a)], ref
    v = pr.Verdict("accepted frame")
    assert not pr.judge(v, og, e, a, frame, pr.DELTA_FAST, pr.EPS_FAST_SHORT, ref) and not v.explained
    # three interior pixels of boxes, two steps off in one channel
    box = np.array([p >= 0 and table[p, 0] == 1 for p in prim.ravel()]).reshape(prim.shape)
    ys, xs = np.nonzero(interior(prim, rgba, frame) & box & (frame[..., 1] < 250))
    assert len(ys) >= 3
    pick = [(int(xs[k]), int(ys[k])) for k in (0, len(ys) // 2, len(ys) - 1)]
    bent = frame.copy()
    for x, y in pick:
        bent[y, x, 1] += 2
    v = pr.Verdict("three interior pixels off by 2")
    failed = pr.judge(v, og, e, a, bent, pr.DELTA_FAST, pr.EPS_FAST_SHORT, ref)
    assert sorted(failed) == sorted(pick) and not v.explained
    with pytest.raises(AssertionError):
        v.check()
    assert old_count_rule_accepts(np.stack(list(frames.values())), np.stack([bent if k == (e, a) else f for k, f in frames.items()])), "the count rule (test_fast_pixels_gpu.compare) accepts the same frame: that is the gap"
    # a dropped primitive: the pixels of one 16 x 4 tile that a box covers show what is behind it
    target = next(int(p) for p in np.unique(prim[prim >= 0]) if table[p, 0] == 1 and table[p, 1] < 0 and any(
        (prim[ty: ty + 4, tx: tx + 16] == p).sum() >= 16 for ty in range(0, 64, 4) for tx in range(0, 64, 16)) and _behind(og, e, a, int(p)) is not None)
    behind = _behind(og, e, a, target)
    ty, tx = next((ty, tx) for ty in range(0, 64, 4) for tx in range(0, 64, 16) if (prim[ty: ty + 4, tx: tx + 16] == target).sum() >= 16)
    dropped = frame.copy()
    tile = np.zeros(prim.shape, bool); tile[ty: ty + 4, tx: tx + 16] = True
    tile &= prim == target
    dropped[tile] = behind[tile]
    changed = tile & (np.abs(dropped[..., :3].astype(np.int16) - frame[..., :3].astype(np.int16)).max(axis=-1) > 1)
    assert changed.sum() >= 8
    v = pr.Verdict("dropped primitive")
    failed = pr.judge(v, og, e, a, dropped, pr.DELTA_FAST, pr.EPS_FAST_SHORT, ref)
    ys, xs = np.nonzero(changed)
    assert sorted(failed) == sorted((int(x), int(y)) for x, y in zip(xs, ys)), "every pixel whose colour changed by more than 1 is rejected"


def _behind(og, e, a, target):
    """the float64 frame without primitive `target`: what a kernel that dropped it would draw (the box is moved out of sight through the snapshot-free
    route the oracle offers: none -- so the frame behind is composed from the reference's candidates with the depth window opened wide)"""
    rgba, prim = og.render_f64(e, a)
    ys, xs = np.nonzero(prim == target)
    if not len(ys):
        return None
    out = rgba.copy()
    colors, counts = og.explain_f64(e, a, np.stack([xs, ys], axis=1), 0.0, 1e9)   # every primitive the centre ray meets, and nothing else
    for k, (x, y) in enumerate(zip(xs, ys)):
        other = [c for c in colors[k, : counts[k]] if c[3] == 255 and not np.array_equal(c[:3], rgba[y, x, :3])]
        out[y, x] = other[0] if other else (0, 0, 0, 255)
        out[y, x, 3] = 255
    return out


class F64Gym:
    """an OracleGym whose observations are the float64 reference's frames"""

    def __init__(self, g):
        self.g = g

    def __getattr__(self, name):
        return getattr(self.g, name)

    def render(self):
        pass

    def get_observation(self, e, a):
        return self.g.render_f64(e, a)[0]


@pytest.mark.parametrize("case", [canon.test_wall_seen_square_on, canon.test_sky_above_a_distant_wall_and_the_horizon_rows,
                                  canon.test_a_movable_box_lands_on_the_derived_columns_and_rows, canon.test_rows_are_bottom_up], ids=lambda f: f.__name__)
def test_reference_reproduces_the_hand_derived_frames(case):
    """the four cases of test_canonical_frames.py, every pixel they assert, on the float64 reference's frames"""
    g = oracle_lib.OracleGym("TowerBuilding", canon.W, canon.H, canon.N_ENVS, 1, 1, False, {})
    g.seed(3); g.reset()
    try:
        case(F64Gym(g))
    finally:
        g.close()


def test_bindings():
    og = oracle_lib.OracleGym("TowerBuilding", 48, 20, 2, 2, 1)
    og.seed(pr.SEED); og.reset()
    rgba, prim = og.render_f64(1, 1)
    table = og.prim_table(1, 1)
    assert rgba.shape == (20, 48, 4) and rgba.dtype == np.uint8 and prim.shape == (20, 48) and prim.dtype == np.int32
    assert (rgba[..., 3] == 255).all() and prim.min() >= -1 and prim.max() < len(table) and table.shape[1] == 2
    assert set(np.unique(table[:, 0])) <= {1, 2, 3, 4, 5, 6} and (table[:, 1] >= -1).all()
    miss = prim == -1
    assert miss.any(), "a TowerBuilding frame of this seed that shows some sky"
    assert (rgba[miss][:, :3] == 0).all() and (rgba[~miss][:, :3].max(axis=-1) > 0).all(), "a miss gives -1 and the clear colour"
    ys, xs = np.nonzero(miss)
    xy = [[int(xs[0]), int(ys[0])], [24, 2], [0, 0]]
    colors, counts = og.explain_f64(1, 1, xy, 0.0, pr.EPS_4ULP)
    assert colors.shape == (3, oracle_lib.EXPLAIN_MAX, 4) and counts.shape == (3,) and oracle_lib.EXPLAIN_MAX >= 36
    for k, (x, y) in enumerate(xy):   # delta_px = 0: the centre's candidates only -- among them the frame's own colour, first
        assert counts[k] >= 1 and colors[k, 0].tolist() == rgba[y, x].tolist()
    assert counts[0] == 1 and colors[0, 0].tolist() == [0, 0, 0, 255]
    wide, nwide = og.explain_f64(1, 1, xy, 0.5, 1e9)   # half a pixel around, every depth: a superset of the centre's
    for k in range(3):
        have = {tuple(c[:3]) for c in wide[k, : nwide[k]]}
        assert {tuple(c[:3]) for c in colors[k, : counts[k]]} <= have and nwide[k] <= oracle_lib.EXPLAIN_MAX
    with pytest.raises(AssertionError):
        og.explain_f64(1, 1, [[48, 0]], 0.0, 0.0)
    og.close()
