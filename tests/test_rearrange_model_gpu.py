"""Rearrange's rules on the device: the HIP gym through the scripted cases and the courier runs of tests/rearrange_cases.py under the independent model
(tests/rearrange_model.py; rules (E), (R), (U) applied by tests/rule_judge.py) tick by tick -- step_kernel<1> for the one-agent cases, step_kernel<MAX_AGENTS>
for the others -- and bit-equal to the CPU oracle in rewards, dones, true objectives and the final snapshots; then the launch shapes: the replayable
scripts out of a device action ring, one batched call per segment (the setter-free tail of `solve` and `both`, the solving tick through the tick that
ends the episode and swaps the next one in, is ONE call), and with the Rearrange gym as the first member of a MultiTaskGym beside an Empty gym -- the
union step kernels, whose Rearrange reward path no other test reaches with a non-zero reward.  Every replay asserts the step launches it took."""
import functools

import pytest

import puzzle_gpu_util as U
import rearrange_cases as RC
import rearrange_model as M

pytestmark = pytest.mark.gpu

REPLAY = [n for n, c in RC.CASES.items() if c.replay]


@functools.lru_cache(maxsize=None)
def hip_run(name, group=False):
    return U.hip_run(RC.CASES[name], M, group)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    return U.oracle_run(RC.CASES[name])


@pytest.mark.parametrize("name", list(RC.CASES))
def test_hip_through_case(hip, name):
    """the HIP gym, stepped tick by tick, through a case under (E), (R), (U) -- the same assertions the oracle meets in test_rearrange_model.py -- and
    bit-equal to the oracle"""
    case = RC.CASES[name]
    run = hip_run(name)
    judge = run[0]
    c, share = judge.report("rearrange model, HIP", name)
    assert judge.failures == [], judge.failures[:10]
    assert judge.finish_unjudged == 0
    if case.scripted:
        assert judge.fragile == 0 and (name == "timeout" or judge.min_margin >= RC.MARGIN)
    else:
        assert share <= 0.02
        assert c["pick"] >= 100 and c["place"] >= 100 and c["reward_ticks"] >= 20 and c["solved_episodes"] >= 2 and c["timed_out_episodes"] >= 2, c
    if name in ("solve", "both"):
        assert judge.solves == len(case.notes) == judge.clamps and c["solved_episodes"] == len(case.notes)
    U.assert_equal_to_oracle(case, run, oracle_run(name))


@pytest.mark.parametrize("name,pipelining", [(n, on) for n in REPLAY for on in (True, False)])
def test_replay_through_an_action_ring(hip, name, pipelining):
    """the replayable cases in batched calls: rewards and dones of every tick, the true objectives behind the last call and the final state are those of
    the tick-by-tick run the model judged; with one agent per env every call is ONE step launch, with several one per tick"""
    case = RC.CASES[name]
    U.assert_replay_equals(case, hip_run(name), U.replay_single(case, pipelining))


@pytest.mark.parametrize("name", REPLAY)
def test_replay_as_a_group_member(hip, name):
    """... and as the first member of a MultiTaskGym beside an Empty gym, one call per segment: the union step kernels"""
    U.replay_in_group(RC.CASES[name], hip_run(name, True), True)


@pytest.mark.parametrize("name", ["solve", "both"])
def test_replay_as_a_group_member_tick_by_tick(hip, name):
    """... and one union launch per tick (step_union_kernel, MultiTaskGym.step)"""
    U.replay_in_group(RC.CASES[name], hip_run(name, True), False)
