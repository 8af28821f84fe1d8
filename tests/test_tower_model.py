"""TowerBuilding's stacking rules: the CPU oracle under an independent float64 model (tests/tower_model.py: rules (E), (R), (U)) through the scripted cases of
tests/tower_cases.py, the model itself against closed forms, and the rejection demo -- copies of the model with one planted mistake each must be rejected.
Prints the largest reward-error / bound ratio, the fragile shares and the event counts (DESIGN.md records them)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
import tower_cases as TC
import tower_model as M


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle through a case under the model, once: (judge, the rewards of every tick)"""
    case = TC.CASES[name]
    g = case.make(oracle_lib.OracleGym)
    judge, rewards = TC.run_judged(case, g)
    g.close()
    return judge, rewards


def report(name, judge):
    c = judge.counts()
    share = judge.fragile / max(1, judge.interact_ticks)
    print(f"\n[tower model] {name}: interact ticks {judge.interact_ticks}, judged {judge.judged}, fragile {judge.fragile} ({100 * share:.2f} %), finished "
          f"{judge.finished}, rewards unjudged {judge.reward_unjudged}, respawns {judge.respawns}, smallest margin {judge.min_margin:.4f}, largest reward error / bound {judge.worst_ratio:.3f}, {c}")
    return c, share


def test_coefficient_table():
    """buildingRewardCoeffForHeight for h in [-30, 15]: the model's float64 closed form against the oracle's fp32 one, within the two roundings of rule (R);
    hand values; the cap binds from h = 9 (0.05 * 2^9 = 25.6 > 20)"""
    L = oracle_lib.lib()
    for h in range(-30, 16):
        want, got = M.coeff(h), float(L.mvo_building_reward_coeff(float(h)))
        assert abs(got - want) <= 2 * M.U * abs(want) + 1e-45, (h, got, want)
    c = M.C05
    assert M.coeff(0) == c and M.coeff(1) == c + 2 * c and M.coeff(8) == 8 * c + 256 * c and M.coeff(9) == 9 * c + 20.0 and M.coeff(12) == 12 * c + 20.0
    assert M.coeff(8) < 20 < c * 2 ** 9
    assert M.coeff(-30) == -30 * c + c * 2.0 ** -30


def test_interact_points_by_hand():
    """eye + R(yaw, pitch) offset at hand-picked poses: level looks along the four axes, a look straight up, a quarter turn with pitch"""
    p = (10.5, 1.815, 7.5)
    eye = 1.815 + 0.46
    for (dx, dz) in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        basis = (-dz, -dx, dx, -dz)   # (c, s, -s, c), forward = (-s, 0, -c)
        assert np.allclose(M.interact_point(p, basis, 0.0, M.PICK_OFFSET), (10.5 + dx, eye - 0.44, 7.5 + dz), atol=1e-15)
        assert np.allclose(M.interact_point(p, basis, 0.0, M.PLACE_OFFSET), (10.5 + dx, eye - 0.74, 7.5 + dz), atol=1e-15)
    up = M.interact_point(p, (1, 0, 0, 1), np.pi / 2, M.PICK_OFFSET)   # straight up: the point is 1 above the eye, 0.44 ahead
    assert np.allclose(up, (10.5, eye + 1.0, 7.5 - 0.44), atol=1e-15)
    a = 0.5
    q = M.interact_point(p, (0, -1, 1, 0), a, M.PLACE_OFFSET)          # facing +x
    assert np.allclose(q, (10.5 + np.cos(a) + 0.74 * np.sin(a), eye - 0.74 * np.cos(a) + np.sin(a), 7.5), atol=1e-15)
    assert M.floor3((-0.5, 1.0, 2.999)) == (-1, 1, 2) and abs(M.margin_of((0.25, 1.9, 2.5)) - 0.1) < 1e-12


def test_fp32_point_bound():
    """rule (E)'s condition: mv_sincos against numpy over [-1.6, 1.6] (the largest error is printed; tower_model.SINCOS_ERR must cover it four times), and
    FRAGILE >= 10 x the bound of the fp32 interact point"""
    L = oracle_lib.lib()
    worst = 0.0
    s, c = C.c_float(), C.c_float()
    for x in np.linspace(-1.6, 1.6, 20001).astype(np.float32):
        L.mvo_sincos(float(x), C.byref(s), C.byref(c))
        worst = max(worst, abs(s.value - np.sin(np.float64(x))), abs(c.value - np.cos(np.float64(x))))
    print(f"\n[tower model] largest sincos error on [-1.6, 1.6]: {worst:.3g}; SINCOS_ERR {M.SINCOS_ERR:.3g}; POINT_BOUND {M.POINT_BOUND:.3g}")
    assert 4 * worst <= M.SINCOS_ERR
    assert M.FRAGILE >= 10 * M.POINT_BOUND


SCRIPTED = [n for n, c in TC.CASES.items() if c.scripted]
STRESS = [n for n, c in TC.CASES.items() if not c.scripted]


@pytest.mark.parametrize("name", SCRIPTED)
def test_oracle_through_scripted_case(name):
    """the oracle through a scripted case under (E), (R), (U): nothing fragile, no respawn, every difference a failure"""
    judge, _ = oracle_run(name)
    report(name, judge)
    assert judge.failures == [], judge.failures[:10]
    assert judge.fragile == 0 and judge.respawns == 0 and judge.finish_unjudged == 0 and judge.interact_ticks > 0
    assert judge.min_margin >= TC.MARGIN


def test_scripted_outcomes():
    """what the scripted cases are for, stated on the oracle's side (the model agreed above): the sweep took and put down every index, the tower stands, ..."""
    judge, rewards = oracle_run("sweep")
    picks = sorted(ev[3] for ev in judge.events if ev[1] == "pick")
    places = sorted(ev[3] for ev in judge.events if ev[1] == "place")
    assert picks == list(range(80)) and places == list(range(80))
    assert all(ev[0] == ev[3] for ev in judge.events)   # env e: index e
    for name, A in (("tower_a1", 1), ("tower_a2", 2), ("tower_a4", 4)):
        judge, rewards = oracle_run(name)
        ys = [ev[4][1] for ev in judge.events if ev[0] == 0 and ev[1] == "place"]
        assert ys == list(range(1, TC.TOWER_TOP + 1)) + [2], ys
        pad = max(1, TC.CASES[name].replay)
        for k in range(TC.TOWER_TOP):   # each delta against the closed form, spirit 0: the actor gets all of it
            assert abs(float(rewards[k * pad][0]) - M.coeff(k + 1)) <= 1e-4, (name, k)
        assert abs(float(rewards[(TC.TOWER_TOP + 1) * pad][0]) - (M.coeff(2) - M.coeff(1))) <= 1e-5   # the moved box: its removal is in the delta
    judge, _ = oracle_run("pick")
    got = {ev[0]: ev for ev in judge.events if ev[1] == "pick" and ev[0] < 8}
    assert sorted(got) == [0, 1, 3, 5, 7] and got[0][4][1] == 2 and got[1][4][1] == 2 and got[3][3] == 1 and got[5][4][1] == 3 and got[7][4][1] == 1, got
    assert [ev[1] for ev in judge.events if ev[0] == 8] == ["pick", "place", "pick"]
    judge, _ = oracle_run("place")
    g = TC.CASES["place"].make(oracle_lib.OracleGym)
    exp = TC.place_expect([TC.snapshot(g, e) for e in range(TC.CASES["place"].N)])
    g.close()
    assert len(exp) == 15
    placed = {ev[0]: ev[4] for ev in judge.events if ev[1] == "place"}
    want = {"x < bz1 inside", "x = bz0 inside", "z < bz3 inside", "z = bz2 inside", "own voxel", "drop to the floor", "drop onto a stack", "onto a column one higher"}
    assert {n for n, e in exp.items() if e in placed} == want, {n for n, e in exp.items() if e in placed}
    assert placed[exp["drop to the floor"]][1] == 1 and placed[exp["drop onto a stack"]][1] == 3 and placed[exp["onto a column one higher"]][1] == 4
    assert placed[exp["own voxel"]][1] == 1
    judge, _ = oracle_run("order")
    assert [(ev[0], ev[1], ev[2]) for ev in judge.events] == [(0, "pick", 0), (1, "place", 0), (1, "pick", 1), (2, "place", 1)], judge.events
    judge, rewards = oracle_run("visit")
    r = np.stack(rewards)
    assert np.allclose(r[:, 0], [0, 0.1, 0, 0], atol=1e-7) and np.allclose(r[:, 1], [0.2, 0, 0, 0], atol=1e-7) and not r[:, 2].any(), r
    judge, _ = oracle_run("end")
    first = {}
    for o in judge.objectives:
        first.setdefault(o[0], o)
    assert len(first) >= 1 and all(o[1] == 3.0 and o[2] == 3 and not o[3] for o in first.values()), judge.objectives
    assert all(o[1] == o[2] for o in judge.objectives)


@pytest.mark.parametrize("name", STRESS)
def test_oracle_through_stress_run(name):
    """an interact-biased run from dense start layouts, judged every tick; the run must hold enough of what the random rollouts never reach"""
    judge, _ = oracle_run(name)
    c, share = report(name, judge)
    assert judge.failures == [], judge.failures[:10]
    assert judge.respawns == 0 and judge.finish_unjudged == 0
    assert share <= 0.02, share
    assert c["picks"] >= 100 and c["placements"] >= 50 and c["picks_48"] >= 10 and c["placements_48"] >= 10 and c["placements_y3"] >= 5, c


@pytest.mark.parametrize("mistake", list(M.MISTAKES))
def test_planted_mistake_is_rejected(mistake):
    """a copy of the model with one planted mistake, judged against the oracle's outcome, is rejected by at least one scripted case"""
    rules = M.Rules(**M.MISTAKES[mistake])
    rejected = []
    for name in SCRIPTED:
        case = TC.CASES[name]
        if name in ("end", "tower_a2"):
            continue
        g = case.make(oracle_lib.OracleGym)
        judge, _ = TC.run_judged(case, g, rules)
        g.close()
        if judge.failures:
            rejected.append(name)
            break
    print(f"\n[tower model] planted mistake '{mistake}': rejected by {rejected}")
    assert rejected, mistake


def test_setters_refuse_inconsistent_input():
    """mvo_debug_set_objects: two boxes carried by one agent, a carrier the env does not have, two placed boxes in one voxel, a placed box in a solid voxel,
    more than 80 boxes; another scenario"""
    g = oracle_lib.OracleGym("TowerBuilding", 32, 32, 1, 2)
    g.seed(1); g.reset()
    before = g.snapshot(0).tobytes()
    for bad in ([[0, 0, 0, 1], [0, 0, 0, 1]], [[0, 0, 0, 3]], [[3, 1, 3, 0], [3, 1, 3, 0]], [[0, 1, 3, 0]], [[3, 1, 3, -1]], [[2, 4, 2, 0]] * 81):
        with pytest.raises(RuntimeError):
            g.debug_set_objects(0, bad)
    assert g.snapshot(0).tobytes() == before   # a refused call changes nothing
    g.debug_set_objects(0, [[3, 1, 3, 0], [0, 0, 0, 2], [3, 2, 3, 0]])
    s = g.snapshot(0)
    assert int(s["num_objects"]) == 3 and [int(a["carrying"]) for a in s["agents"][:2]] == [-1, 1]
    g.close()
    o = oracle_lib.OracleGym("ObstaclesEasy", 32, 32, 1, 1)
    o.seed(1); o.reset()
    with pytest.raises(RuntimeError):
        o.debug_set_objects(0, [])
    o.close()
