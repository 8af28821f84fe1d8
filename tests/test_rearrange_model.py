"""Rearrange's rules: the CPU oracle under an independent model (tests/rearrange_model.py; rules (E), (R), (U) of tests/tower_model.py, applied by
tests/rule_judge.py) through the scripted cases and the courier runs of tests/rearrange_cases.py; what every scripted case is named after, asserted on the
oracle's own rewards, dones and objectives; and the rejection demo -- copies of the model with one planted mistake each must be rejected.  Prints the
event counts, the fragile shares and the largest reward-error / bound ratio (DESIGN.md records them)."""
import functools

import numpy as np
import pytest

import oracle_lib
import rearrange_cases as RC
import rearrange_model as M
import rule_judge
import tower_cases as TC

SCRIPTED = [n for n, c in RC.CASES.items() if c.scripted]
STRESS = [n for n, c in RC.CASES.items() if not c.scripted]


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle through a case under the model, once: (judge, rewards [ticks, N, A], dones [ticks, N], the objectives of the envs finishing per tick)"""
    case = RC.CASES[name]
    g = case.make(oracle_lib.OracleGym)
    judge, rewards, dones, objectives = rule_judge.run_judged(case, g, M, min_margin=RC.MARGIN if case.scripted else None)
    g.close()
    return judge, np.stack(rewards).reshape(len(rewards), case.N, case.A), np.stack(dones), objectives


def test_matching_by_hand():
    """countMatchingObjects on a hand-made record: shape, colour and offset all have to agree; a carried item never counts; any item's place will do"""
    class S:
        pass
    st = S()
    st.items = [(0, 7, (0, 0, 0)), (0, 7, (1, 0, 0)), (1, 7, (0, 1, 0)), (0, 9, (-1, 0, 0))]
    at = lambda off, state=0: [M.RIGHT[0] + off[0], M.RIGHT[1] + off[1], M.RIGHT[2] + off[2], state]
    st.objects = [at((1, 0, 0)), at((0, 0, 0)), at((0, 1, 0)), at((-1, 0, 0))]
    assert M.count_matching(st, M.REFERENCE) == 4          # items 0 and 1 look alike and lie on each other's places
    st.objects[3] = at((-1, 0, 0), 1)
    assert M.count_matching(st, M.REFERENCE) == 3          # carried
    st.objects = [at((-1, 0, 0)), at((0, 1, 0)), at((0, 0, 0)), at((1, 0, 0))]
    assert M.count_matching(st, M.REFERENCE) == 0          # wrong by the colour, by shape and y offset, by shape and y offset, by the colour
    assert M.count_matching(st, M.Rules(match_colour=False)) == 2 and M.count_matching(st, M.Rules(match_y=False)) == 2
    assert M.solid(13, 1, 5, 4) and M.solid(16, 1, 8, 4) and not M.solid(17, 1, 5, 4) and not M.solid(13, 2, 5, 4) and M.solid(8, 1, 5, 4) and not M.solid(9, 1, 5, 4)
    assert M.solid(0, 3, 7, 4) and not M.solid(0, 4, 7, 4) and M.solid(18, 5, 13, 6) and M.solid(7, 0, 7, 4) and not M.solid(19, 0, 0, 4)


@pytest.mark.parametrize("name", SCRIPTED)
def test_oracle_through_scripted_case(name):
    """the oracle through a scripted case under (E), (R), (U): nothing fragile, nothing unjudged, every difference a failure"""
    judge, _, _, _ = oracle_run(name)
    judge.report("rearrange model", name)
    assert judge.failures == [], judge.failures[:10]
    assert judge.fragile == 0 and judge.finish_unjudged == 0
    assert name == "timeout" or (judge.interact_ticks > 0 and judge.min_margin >= RC.MARGIN)


def test_scripted_outcomes():
    """what the scripted cases are named after, on the oracle's side (the model agreed above)"""
    judge, r, d, _ = oracle_run("match")
    notes = RC.CASES["match"].notes
    assert len(notes) >= 2
    for e, n in notes.items():   # +1 once; the second placement on the same cell pays nothing
        assert r[n["t_first"], e, 0] == 1.0 and r[n["t_second"], e, 0] == 0.0 and np.count_nonzero(r[:, e]) == 1
        assert [ev[1] for ev in judge.events if ev[0] == e] == ["pick", "place", "pick", "place"]
        places = [ev[4] for ev in judge.events if ev[0] == e and ev[1] == "place"]
        assert places[0] == places[1]
    judge, r, d, obj = oracle_run("solve")
    notes = RC.CASES["solve"].notes
    assert len(notes) >= 6 and max(n["items"] for n in notes.values()) >= 5
    for e, n in notes.items():   # +1 and +10 on one tick; solved; the timer clamped: done four ticks on (0.3 s less the solving tick's own dt); objective 1
        t = n["t_solve"]
        assert r[t, e, 0] == 11.0 and not r[t + 1:, e].any()
        assert np.nonzero(d[:, e])[0].tolist() == [t + 4] and obj[t + 4][e] == 1.0
    assert judge.solves == len(notes) == judge.clamps and judge.finished == len(notes)
    g = RC.CASES["solve"].make(oracle_lib.OracleGym)   # the next episode was swapped in
    for _ in TC.play(RC.CASES["solve"], g):
        pass
    for e, n in notes.items():
        s = g.snapshot(e)
        assert int(s["solved"]) == 0 and int(s["num_frames"]) <= 3 and float(s["episode_sec"]) < 0.3
    g.close()
    judge, r, d, obj = oracle_run("timeout")
    assert not r.any() and d.sum() == 2 and all(v == 0.0 for o in obj for v in o.values()) and judge.objectives and judge.solves == 0
    judge, r, d, _ = oracle_run("stacked")
    notes = RC.CASES["stacked"].notes
    assert notes
    for e, n in notes.items():
        ev = {k: [x for x in judge.events if x[0] == e and x[1] in ("pick", "place")][-3 + i] for i, k in enumerate(("up", "covered", "back"))}
        assert ev["up"][1] == "place" and ev["up"][3] == n["upper"] and ev["up"][4][1] == 3          # onto the lower item
        assert ev["covered"][1] == "pick" and ev["covered"][3] == n["upper"] and ev["covered"][4][1] == 3   # aimed at the lower one: the upper one comes
        assert ev["back"][1] == "place" and ev["back"][4] == ev["up"][4]
    judge, r, d, _ = oracle_run("refusals")
    notes = RC.CASES["refusals"].notes
    assert sorted(n["rule"] for n in notes.values()) == sorted(RC.REFUSALS)
    assert not r.any() and [ev[1] for ev in judge.events] == ["pick"] * len(notes)   # nothing was put down, nothing changed (the model followed every record)
    judge, r, d, _ = oracle_run("descent")
    for e, n in RC.CASES["descent"].notes.items():
        place = [ev for ev in judge.events if ev[0] == e and ev[1] == "place"]
        assert len(place) == 1 and place[0][4] == (n["cell"][0], 2, n["cell"][1])
    judge, r, d, _ = oracle_run("spirit")
    for e, n in RC.CASES["spirit"].notes.items():   # the actor: 1 * (1 - 0.5) + 1 * 0.5 / 2; its mate: 1 * 0.5 / 2
        assert r[n["t_place"], e].tolist() == [0.25, 0.75] and np.count_nonzero(r[:, e]) == 2
    judge, r, d, _ = oracle_run("wrong_colour")
    assert RC.CASES["wrong_colour"].notes and not r.any() and judge.counts()["place"] == len(RC.CASES["wrong_colour"].notes)
    judge, r, d, _ = oracle_run("carried")
    notes = RC.CASES["carried"].notes
    assert notes
    for e, n in notes.items():   # as many match as before: nothing; the lifted item back in place: one more than ever
        assert not r[n["t_place"], e].any() and r[n["t_back"], e, 1] in (1.0, 11.0) and r[n["t_back"], e, 0] == 0.0
    judge, r, d, obj = oracle_run("both")
    notes = RC.CASES["both"].notes
    assert notes
    for e, n in notes.items():   # agent 0 acts first: +1; agent 1's placement solves: +1 and +10
        t = n["t_both"]
        assert r[t, e].tolist() == [1.0, 11.0] and d[t + 4, e] and obj[t + 4][e] == 1.0


@pytest.mark.parametrize("name", STRESS)
def test_oracle_through_courier_run(name):
    """the courier: teleports, quarter turns with offsets, pitches and Interact on most ticks, judged every tick; the run must hold what random rollouts
    never reach"""
    judge, _, _, _ = oracle_run(name)
    c, share = judge.report("rearrange model", name)
    assert judge.failures == [], judge.failures[:10]
    assert share <= 0.02, share
    assert c["pick"] >= 100 and c["place"] >= 100 and c["reward_ticks"] >= 20 and c["solved_episodes"] >= 2 and c["timed_out_episodes"] >= 2, c
    assert judge.finish_unjudged <= 0.1 * judge.finished


@pytest.mark.parametrize("mistake", list(M.MISTAKES))
def test_planted_mistake_is_rejected(mistake):
    """a copy of the model with one planted mistake, judged against the oracle's outcome, is rejected by at least one scripted case"""
    rules = M.Rules(**M.MISTAKES[mistake])
    rejected = []
    for name in SCRIPTED:
        case = RC.CASES[name]
        g = case.make(oracle_lib.OracleGym)
        judge, _, _, _ = rule_judge.run_judged(case, g, M, rules)
        g.close()
        if judge.failures:
            rejected.append(name)
            break
    print(f"\n[rearrange model] planted mistake '{mistake}': rejected by {rejected}")
    assert rejected, mistake
