"""Sokoban's rules on the device: the HIP gym through the scripted cases and the pusher runs of tests/sokoban_cases.py (levels: tests/golden/boxoban_solvable)
under the independent model (tests/sokoban_model.py; rules (E), (R), (U) applied by tests/rule_judge.py) tick by tick -- step_kernel<1> for the one-agent
cases, step_kernel<MAX_AGENTS> for the others -- and bit-equal to the CPU oracle in rewards, dones, true objectives and the final snapshots; then the launch
shapes: the replayable scripts out of a device action ring, one batched call per segment (the setter-free tail of `corridor`, the solving push through the
tick that ends the episode and swaps the next level in, is ONE call), and with the Sokoban gym as the first member of a MultiTaskGym beside an Empty gym
-- the union step kernels.  Every replay asserts the step launches it took."""
import functools

import pytest

import puzzle_gpu_util as U
import sokoban_cases as SC
import sokoban_model as M

pytestmark = pytest.mark.gpu

REPLAY = [n for n, c in SC.CASES.items() if c.replay]


@pytest.fixture(autouse=True)
def boxoban_env(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", SC.LEVEL_DIR)


@functools.lru_cache(maxsize=None)
def hip_run(name, group=False):
    return U.hip_run(SC.CASES[name], M, group, levels=SC.levels())


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    return U.oracle_run(SC.CASES[name])


@pytest.mark.parametrize("name", list(SC.CASES))
def test_hip_through_case(hip, name):
    """the HIP gym, stepped tick by tick, through a case under (E), (R), (U) -- the same assertions the oracle meets in test_sokoban_model.py -- and bit-equal
    to the oracle"""
    case = SC.CASES[name]
    run = hip_run(name)
    judge = run[0]
    c, share = judge.report("sokoban model, HIP", name)
    assert judge.failures == [], judge.failures[:10]
    assert judge.finish_unjudged == 0 and judge.interact_ticks > 0
    if case.scripted:
        assert judge.fragile == 0 and judge.min_margin >= SC.MARGIN
    else:
        assert share <= 0.02
        assert c["push"] >= 100 and c["reward_ticks"] >= 20 and c["solved_episodes"] >= 2 and c["timed_out_episodes"] >= 2 and c["enter"] >= 5 and c["leave"] >= 5, c
        assert c["refuse_wall"] >= 10 and c["refuse_box"] >= 10 and c["refuse_distance"] >= 10 and (case.A == 1 or c["refuse_agent"] >= 10), c
    if name in ("corridor", "goals"):
        assert judge.solves == len(case.notes) == judge.clamps == c["solved_episodes"]
    U.assert_equal_to_oracle(case, run, oracle_run(name))


@pytest.mark.parametrize("name,pipelining", [(n, on) for n in REPLAY for on in (True, False)])
def test_replay_through_an_action_ring(hip, name, pipelining):
    """the replayable cases in batched calls: rewards and dones of every tick, the true objectives behind the last call and the final state are those of
    the tick-by-tick run the model judged; with one agent per env every call is ONE step launch, with several one per tick"""
    case = SC.CASES[name]
    U.assert_replay_equals(case, hip_run(name), U.replay_single(case, pipelining))


@pytest.mark.parametrize("name", REPLAY)
def test_replay_as_a_group_member(hip, name):
    """... and as the first member of a MultiTaskGym beside an Empty gym, one call per segment: the union step kernels"""
    U.replay_in_group(SC.CASES[name], hip_run(name, True), True)


@pytest.mark.parametrize("name", ["corridor", "two_agents"])
def test_replay_as_a_group_member_tick_by_tick(hip, name):
    """... and one union launch per tick (step_union_kernel, MultiTaskGym.step)"""
    U.replay_in_group(SC.CASES[name], hip_run(name, True), False)
