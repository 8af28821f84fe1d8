"""The controller's physics kernels (mv_physics.h: sweep, recover_up_to_5, player_step) through the debug entries mv_debug_sweep / mv_debug_recover /
mv_debug_player_step, in each of the five instantiations the step kernels use: bit for bit against the oracle's twins, and -- so that a mistake the
oracle shares still fails -- directly against the float64 model's rules (G), (D) and (R) of tests/physics_reference.py, on the query classes of
tests/physics_cases.py.  One launch per collider array; every test takes seconds."""
import functools

import numpy as np
import pytest

import oracle_lib
import physics_cases as PC
import physics_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
VARIANTS = [(0, "nc1"), (1, "nc2"), (2, "nc4"), (3, "hex"), (4, "ball")]
ids = [n for _, n in VARIANTS]


def _call(hip, fn, variant, cols, rec, out):
    lib = hip.load_library()
    cols = np.ascontiguousarray(cols, R.COL)
    rc = getattr(lib, fn)(0, variant, cols.ctypes.data, len(cols), rec.ctypes.data, len(rec), out.ctypes.data)
    assert rc == 0, lib.mv_last_error()
    return out


def hip_sweep(hip, variant, cols, queries):
    q = np.ascontiguousarray(queries, R.QUERY)
    return _call(hip, "mv_debug_sweep", variant, cols, q, np.zeros(len(q), R.SWEEP_OUT))


def hip_recover(hip, variant, cols, positions):
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    return _call(hip, "mv_debug_recover", variant, cols, p, np.zeros(len(p), R.RECOVER_OUT))


def hip_player_step(hip, variant, cols, agents):
    a = np.ascontiguousarray(agents, R.AGENT)
    return _call(hip, "mv_debug_player_step", variant, cols, a, np.zeros(len(a), R.AGENT))


@functools.lru_cache(maxsize=None)
def reference(cls, name):
    """sweep64 of one batch: computed once, shared by the variants and the tests (which must not change it)"""
    b = next(b for b in PC.batches(cls) if b.name == name)
    return R.sweep64(b.cols, b.queries)


def of_variant(variant, what):
    return [b for b in PC.batches() if variant in b.variants and getattr(b, what) is not None]


def same_records(got, want, b):
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{b}: {len(bad)} of {len(got)} records differ from the oracle's, first {bad[0]}: kernel {got[bad[0]]}, oracle {want[bad[0]]}")


@pytest.mark.parametrize("variant,name", VARIANTS, ids=ids)
def test_sweep_bit_for_bit_and_against_float64(hip, variant, name):
    """hit flag, fraction bits and normal bits equal the oracle's; the same records meet (G) everywhere and (D) wherever the float64 run is not fragile"""
    todo = of_variant(variant, "queries")
    assert len(todo) >= 5 and {b.cls for b in todo} >= {"boxes", "grazing", "threshold", "ties", "slope"}
    assert max(len(b.cols) for b in todo) == 64 * PC.NC_OF[variant]
    ratios = {}
    for b in todo:
        got = hip_sweep(hip, variant, b.cols, b.queries)
        same_records(got, oracle_lib.debug_sweep(b.cols, b.queries), b)
        ref = reference(b.cls, b.name)
        fails_g, rg = R.check_G(b.cols, b.queries, got, ref)
        fails_d, rd, _ = R.check_D(b.cols, b.queries, got, ref)
        assert not fails_g and not fails_d, (b, (fails_g + fails_d)[:5])
        R.merge_ratios(ratios, rg); R.merge_ratios(ratios, rd)
    print(f"{name}: largest ratios against the derived bounds: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))


@pytest.mark.parametrize("variant,name", VARIANTS, ids=ids)
def test_ties_go_to_the_lowest_slot_under_any_permutation(hip, variant, name):
    """bit-equal fractions in (same lane, different k), (different lane, same k) and (both differ), and the same walls with their slots exchanged: the
    kernel's own single-wall casts tie bit for bit, and the sweep reports the wall in the lowest slot"""
    todo = [b for b in of_variant(variant, "queries") if b.cls == "ties" and b.meta["first"] is not None]
    assert len(todo) >= 2 and any("swapped" in b.name for b in todo) and max(len(b.cols) for b in todo) == 64 * PC.NC_OF[variant]
    for b in todo:
        got = hip_sweep(hip, variant, b.cols, b.queries)
        PC.assert_lowest_slot_wins(b, got, lambda cols, q: hip_sweep(hip, variant, cols, q))
    plain, swapped = [next(b for b in todo if b.name == f"corners_nc{PC.NC_OF[variant]}" + s) for s in ("", "_swapped")]
    a, s = hip_sweep(hip, variant, plain.cols, plain.queries), hip_sweep(hip, variant, swapped.cols, swapped.queries)
    assert np.array_equal(a["fraction"].view(np.uint32), s["fraction"].view(np.uint32))            # the permutation changes the winner, nothing else
    assert (plain.meta["first"] != swapped.meta["first"]).all() and not (a["normal"] == s["normal"]).all(1).any()


@pytest.mark.parametrize("variant,name", VARIANTS, ids=ids)
def test_cull_is_exact(hip, variant, name):
    """cast_can_hit only ever skips casts that miss: for every query whose path's bounding box lies on the cull's border (exactly CAP_R from the box, an
    ulp inside, an ulp outside, and within 1e-3 of it) the kernel's result is sweep64's, which knows no cull; those decisions are robust ones"""
    todo = [b for b in of_variant(variant, "queries") if b.cls == "threshold"]
    assert todo
    for b in todo:
        ref = reference(b.cls, b.name)
        cull = b.meta["cull"]
        got = hip_sweep(hip, variant, b.cols, b.queries)
        robust = cull & ~ref["fragile"]
        assert cull.sum() >= 100 and robust.sum() >= 0.9 * cull.sum(), (b, int(cull.sum()), int(robust.sum()))
        assert np.array_equal(got["hit"][robust] != 0, ref["hit"][robust]), b
        assert not got["hit"][cull].any() and (got["fraction"][cull] == 1.0).all(), b       # (no centre on such a path comes within CAP_R - 0.039 of the box)


@pytest.mark.parametrize("variant,name", VARIANTS, ids=ids)
def test_push_out_bit_for_bit_and_against_float64(hip, variant, name):
    """every intermediate position and the number of pushes equal the oracle's; the same records meet (R)"""
    todo = of_variant(variant, "positions")
    assert len(todo) >= 3
    for b in todo:
        got = hip_recover(hip, variant, b.cols, b.positions)
        same_records(got, oracle_lib.debug_recover(b.cols, b.positions), b)
        fails, _, _ = R.check_R(b.cols, b.positions, got)
        assert not fails, (b, fails[:5])


@pytest.mark.parametrize("variant,name", VARIANTS, ids=ids)
def test_player_step_bit_for_bit_with_the_plain_loop(hip, variant, name):
    """every physics field and reach2 equal the oracle's player_step, whose stepForwardAndStrafe runs the plain ten-iteration loop: the kernel's early
    exit ("once an iteration maps the target onto itself") changes nothing, on scenes where the plain loop does run all ten sweeps"""
    todo = of_variant(variant, "agents")
    assert todo
    ten = 0
    for b in todo:
        want, sweeps = oracle_lib.debug_player_step(b.cols, b.agents)
        got = hip_player_step(hip, variant, b.cols, b.agents)
        same_records(got, want, b)
        ten += int((sweeps == 10).sum())
        moved2 = ((got["pos"][:, [0, 2]].astype(np.float64) - b.agents["pos"][:, [0, 2]]) ** 2).sum(-1)
        assert (got["reach2"] >= moved2 * (1 - 1e-6)).all(), b
    assert ten >= 2, "no scene in which the early exit can fire"


def test_debug_entries_refuse_what_a_variant_cannot_hold(hip):
    lib = hip.load_library()
    q, out = np.zeros(1, R.QUERY), np.zeros(1, R.SWEEP_OUT)
    hexbox = PC.place([PC.box((0, 0, 0), (1, 1, 1), 1)], 1)
    assert lib.mv_debug_sweep(0, 0, hexbox.ctypes.data, 1, q.ctypes.data, 1, out.ctypes.data) < 0 and b"kind" in lib.mv_last_error()
    many = PC.place([], 65)
    assert lib.mv_debug_sweep(0, 0, many.ctypes.data, 65, q.ctypes.data, 1, out.ctypes.data) < 0
    assert lib.mv_debug_sweep(0, 9, many.ctypes.data, 1, q.ctypes.data, 1, out.ctypes.data) < 0
    assert lib.mv_debug_sweep(0, 1, many.ctypes.data, 65, q.ctypes.data, 0, out.ctypes.data) == 0      # nothing to do


def test_a_gym_launches_what_it_launched(hip):
    """the debug entries have no gym: calling them between a gym's steps changes neither its launch counts nor what it computes (a twin never calls them)"""
    from megaverse_amd.extension import MegaverseGym
    gyms = [MegaverseGym("TowerBuilding", 32, 32, 4, 1, 1, False, {}) for _ in range(2)]
    for g in gyms:
        g.seed(3); g.reset(); g.step()
    before = gyms[0].debug_launch_counts()
    b = PC.batches("boxes")[0]
    hip_sweep(hip, 1, b.cols, b.queries[:8])
    hip_recover(hip, 1, b.cols, b.queries["from"][:8])
    assert gyms[0].debug_launch_counts() == before
    for g in gyms:
        g.step()
    assert gyms[0].debug_launch_counts() == gyms[1].debug_launch_counts()
    assert np.array_equal(gyms[0].get_observation(0, 0), gyms[1].get_observation(0, 0))
    for g in gyms:
        g.close()
