"""The step bodies on the GPU (megaverse_amd/csrc/mv_step_kernels.h): the resident multi-tick body against the one-tick-per-launch body, every option on at once.

Two gyms with the same seed get the same calls.  One is pipelined, so step_n and macro_step run the resident step_ticks_body (FRAMES_ALL for render 'every',
FRAMES_NONE / FRAMES_BY_MASK for 'none' and 'last'; k = 9 is a launch of 8 ticks and one of 1, so the carried option state crosses a launch boundary through
memory); its twin has set_pipelining(False) and runs one step_body launch per tick.  Attached to both: a step mask that freezes two envs, an episode budget of
1 on one env and 2 on another, a draw mask that leaves one env out, still frames, state and scene rows, the episode log and an output ring of 16.
episodeLengthSec is 4.3, the shortest a gym steps with resident launches; TowerBuilding adds 4 s per object of the level, so the envs' clocks are first
advanced, each by its own number of undrawn ticks (Rig.stagger), until every stepping env's episode ends on a chosen tick of the calls: on the last tick of
a launch of 8, in the launch of 1 behind it, on a call's first tick and inside a launch; the budget of 1 halts its env there.  Behind every call every byte
must be equal: the observation, reward and done rings, rewards, dones, true objectives, both row records, the drained log, the budgets and the halted count;
a rendered call at the end shows the stale bytes' effect.

Which env stepped in which tick is then read off the scene rows (episode time and counter) and checked against the host twins of the rules --
debug_episode_budget_host (step_n), debug_macro_rule_host (macro_step) and debug_still_rule_host -- so that the two device paths cannot agree on a wrong rule.
Of the still rule's verdicts the bytes show whether an env's rows were written (drawn, or still: carried from the entry that holds the last drawn frame) or
left alone (user-undrawn, or a tick without a pass); drawn and still rows hold the same bytes by design (tests/test_still_frames_gpu.py tells them apart)."""
import numpy as np
import pytest

import episode_log_util as U
from megaverse_amd.extension import SCENE_OBS_FIELDS, MegaverseGym

pytestmark = pytest.mark.gpu

N, S, RING, K, MACRO_K = 7, 32, 16, 9, 11
SENT = 0xA5
DEV = "cuda:0"
STEP_MASK = np.array([1, 1, 0, 1, 1, 0, 1], np.uint8)            # envs 2 and 5 are frozen
BUDGET = np.array([-1, 1, -1, 2, -1, -1, -1], np.int32)          # env 1 halts behind its first done, env 3 behind its second
DRAW_MASK = np.array([1, 1, 1, 1, 0, 1, 1], np.uint8)            # env 4 is left out
MACRO_TICKS = np.array([0, 1, 11, 12, 15, 5, 3], np.int32)       # 0, 1, and values above k (clamped to it)
SEC, LEN, CONSUMED = SCENE_OBS_FIELDS["episode_sec"], SCENE_OBS_FIELDS["episode_len"], SCENE_OBS_FIELDS["episodes_consumed"]
TICKS_PER_SEC = 15.0
# the tick of the test's calls, counted in the env's own stepped ticks from 0, on which its episode ends (-1: a frozen env, or one that never gets there)
STEP_N_ENDS = np.array([9 + 7, 18 + 3, -1, 27 + 7, 36 + 8, -1, 45 + 0])      # calls of 9 ticks: launches of 8 and 1
MACRO_ENDS = np.array([-1, 3, -1, 11 + 8, 22 + 3, -1, 12 + 1])               # calls of MACRO_TICKS ticks: env 0 never steps


def ticks_until_done(sec, length):
    """the ticks a clock at `sec` steps until it reaches `length`, in the tick's own fp32 arithmetic (mv_tick_tower.h: episode_sec += DT; done at >= len)"""
    sec, dt, n = np.float32(sec), np.float32(1.0) / np.float32(15.0), 0
    while sec < np.float32(length):
        sec, n = np.float32(sec + dt), n + 1
    return n


class Rig:
    """one gym with every option attached, and the torch buffers of its rings"""

    def __init__(self, A, resident, ends):
        import torch
        U.boxoban_env()
        self.A, self.ticks, self.warm = A, 0, 0
        self.g = g = MegaverseGym("TowerBuilding", S, S, N, A, 1, False, {"episodeLengthSec": 4.3})
        g.set_pixel_mode("fast")
        g.seed(11)
        g.set_episode_log(64)
        if not resident:
            g.set_pipelining(False)
        g.reset()
        self.age = self.stagger(ends)
        self.obs = torch.full((RING, N * A, S, S, 4), SENT, dtype=torch.uint8, device=DEV)
        self.rew = torch.full((RING, N * A), -7.0, dtype=torch.float32, device=DEV)
        self.done = torch.full((RING, N), 9, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        g.set_output_ring(RING, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        g.set_step_mask(STEP_MASK.astype(bool))
        g.set_episode_budget(BUDGET.copy())
        g.set_draw_mask(DRAW_MASK.astype(bool))
        g.set_still_frames(True)
        self.state, self.scene = g.set_state_obs(True), g.set_scene_obs(True)

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def stagger(self, ends):
        """the clocks read off the scene rows; env e is stepped, undrawn, until ends[e] ticks are left of its episode (step masks) -> the ticks every env stepped"""
        g = self.g
        g.set_scene_obs(True)
        g.render()   # (refreshes the rows)
        rows = np.stack([g.get_scene_observation(e) for e in range(N)])
        g.set_scene_obs(None)
        adv = np.array([ticks_until_done(rows[e, SEC], rows[e, LEN]) - 1 - ends[e] if ends[e] >= 0 else 0 for e in range(N)], np.int64)
        assert (adv >= 0).all(), f"episodes shorter than the test's calls: {adv}"
        left = adv.copy()
        while (left > 0).any():
            k = int(min(left[left > 0].min(), 64))
            g.set_step_mask(left > 0)
            g.step_n(k, "multidiscrete", 5, self.warm, render="none")
            self.warm += k
            left = np.where(left > 0, left - k, 0)
        g.set_step_mask(None)
        assert len(g.drain_episode_log()) == 0
        return adv

    def plant(self, entries):
        """the sentinel into every observation byte of the entries the next call fills (never the entry that holds the last drawn frames)"""
        self.sync()
        self.obs[entries] = SENT
        self.sync()

    def step_n(self, k, render):
        entries = [(self.ticks + j) % RING for j in range(k)]
        self.plant(entries)
        self.g.step_n(k, "multidiscrete", 9, self.ticks, render=render)
        self.ticks += k
        return entries

    def macro(self, render):
        entries = [self.ticks % RING]
        self.plant(entries)
        acts = (np.arange(N * self.A * 6).reshape(N * self.A, 6) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)
        self.g.macro_step(MACRO_K, acts, MACRO_TICKS.copy(), render=render)
        self.ticks += 1
        return entries

    def outputs(self):
        """everything a call leaves behind, as bytes by name"""
        self.sync()
        g = self.g
        out = {"obs ring": self.obs, "reward ring": self.rew, "done ring": self.done, "state rows": self.state, "scene rows": self.scene,
               "budget": g.episode_budget()}
        out = {k: v.cpu().numpy() for k, v in out.items()}
        out.update(rewards=g.get_rewards_array(), dones=g.get_dones(), objectives=g.get_true_objectives(), log=g.drain_episode_log(),
                   halted=np.array([g.halted_count()]))
        return out


def close(*rigs):
    for r in rigs:
        r.sync()
        r.g.close()


def twins(A, ends):
    m, t = Rig(A, True, ends), Rig(A, False, ends)
    assert np.array_equal(m.age, t.age)
    return m, t


def same(m, t, what):
    """-> the resident gym's outputs, every byte the twin's"""
    a, b = m.outputs(), t.outputs()
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), f"{what}: {name} differs between the resident body and one step_body launch per tick"
    return a


def written(out, entries, A):
    """[len(entries)][N]: whether any byte of the env's rows in the entry is not the sentinel; an env's A rows are written together or not at all"""
    w = (out["obs ring"][entries].reshape(len(entries), N, A, -1) != SENT).any(axis=3)
    assert (w.all(axis=2) == w.any(axis=2)).all(), "an env's frames were written in part"
    return w.any(axis=2)


def check_still(stepped, has_pass, stale, out, entries, A, what):
    """the still rule's host twin over the call's ticks -> stale behind it; its verdicts against the bytes"""
    from megaverse_amd.extension import debug_still_rule_host
    verdict, stale = debug_still_rule_host(stepped.astype(np.uint8), np.asarray(has_pass, np.uint8), DRAW_MASK, stale)
    rows = verdict if len(entries) == len(verdict) else verdict[-1:]   # (a macro step fills one entry: its last tick's)
    expect = (rows == 1) | (rows == -2)
    assert np.array_equal(written(out, entries, A), expect), f"{what}: rows written {written(out, entries, A).astype(int)}, verdicts {rows}"
    return stale


def has_pass_of(render, k):
    return [1] * k if render == "every" else [0] * (k - 1) + [1 if render == "last" else 0]


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("render", ["every", "last", "none"])
def test_step_n_9_every_option_on(hip, A, render):
    """8 calls of step_n(9): a launch of 8 ticks and one of 1 per call; the episodes end on STEP_N_ENDS"""
    m, t = twins(A, STEP_N_ENDS)
    left, stale, prev, seen_done = BUDGET.copy(), np.ones(N, np.uint8), None, 0
    for c in range(8):
        entries = m.step_n(K, render)
        assert t.step_n(K, render) == entries
        out = same(m, t, f"call {c}")
        rows = out["scene rows"][entries][:, :, [SEC, CONSUMED]]
        dones = out["done ring"][entries]
        seen_done += int(dones.sum())
        if prev is not None:   # (which env stepped in which tick: its episode time or counter moved)
            stepped = (np.concatenate([prev[None], rows])[1:] != np.concatenate([prev[None], rows])[:-1]).any(axis=2)
            steps, left_out = hip.debug_episode_budget_host(dones, STEP_MASK, left)
            assert np.array_equal(stepped, steps != 0), f"call {c}: stepped {stepped.astype(int)}, the rule {steps}"
            assert np.array_equal(out["budget"], left_out), f"call {c}: budgets {out['budget']}, the rule {left_out}"
            stale = check_still(stepped, has_pass_of(render, K), stale, out, entries, A, f"call {c}")
        else:
            # (the first call has no row in front of its first tick.  No episode ends in it; every env is due when the option is switched on, so a call with a
            # pass behind its last tick draws every env the draw mask lets it draw, and a call without one leaves them all due)
            assert np.array_equal(out["budget"], BUDGET) and not dones.any()
            stale = np.where((DRAW_MASK != 0) & (render != "none"), 0, 1).astype(np.uint8)
        left, prev = out["budget"].copy(), rows[-1]
    assert seen_done == 5 and out["halted"][0] == 1, f"the episodes did not end inside the calls as staggered: {seen_done} dones"
    assert np.array_equal(out["budget"][[1, 3]], [0, 1])
    # the stale bytes' visible effect: the next rendered call's frames
    entries = m.step_n(3, "every")
    t.step_n(3, "every")
    out = same(m, t, "the rendered call at the end")
    assert written(out, entries, A)[:, DRAW_MASK != 0].all() and not written(out, entries, A)[:, DRAW_MASK == 0].any()
    close(m, t)


@pytest.mark.parametrize("A", [1, 3])
def test_macro_step_11_every_option_on(hip, A):
    """8 macro steps of up to 11 ticks (a launch of 8 ticks and one of 3), per-env ticks 0, 1 and above k; render 'last' and 'none' in turn; the episodes
    end on MACRO_ENDS"""
    m, t = twins(A, MACRO_ENDS)
    left, stale, age, prev, seen_done = BUDGET.copy(), np.ones(N, np.uint8), m.age.copy(), None, 0
    ticks = np.minimum(MACRO_TICKS, MACRO_K)
    for c in range(8):
        render = "last" if c % 2 == 0 else "none"
        entries = m.macro(render)
        assert t.macro(render) == entries
        out = same(m, t, f"macro step {c}")
        row = out["scene rows"][entries[0]][:, [SEC, CONSUMED]]
        done = out["done ring"][entries[0]] != 0
        seen_done += int(done.sum())
        if prev is not None:
            # the ticks every env stepped in: from its episode time, or -- where the call finished its episode -- from the length the log recorded
            n = np.rint((row[:, 0] - prev[:, 0]) * TICKS_PER_SEC).astype(np.int64)
            for e in np.nonzero(done)[0]:
                rec = out["log"][out["log"]["agent"] == e * A]
                assert len(rec) == 1, f"macro step {c}: env {e} finished, log records {rec}"
                n[e] = int(rec["length"][0]) - age[e]
            d = np.zeros((MACRO_K, N), np.uint8)
            for e in np.nonzero(done)[0]:
                assert 1 <= n[e] <= MACRO_K
                d[n[e] - 1, e] = 1
            steps, left_out, _ = hip.debug_macro_rule_host(d, STEP_MASK, left, ticks)
            assert np.array_equal(steps.sum(axis=0), n), f"macro step {c}: ticks stepped {n}, the rule {steps.sum(axis=0)}"
            assert np.array_equal(out["budget"], left_out), f"macro step {c}: budgets {out['budget']}, the rule {left_out}"
            stale = check_still(steps != 0, has_pass_of(render, MACRO_K), stale, out, entries, A, f"macro step {c}")
            age = np.where(done, 0, age + n)
        else:   # (the first call: all envs due, drawn by its pass; the frozen envs and the env with 0 ticks did not move)
            assert not done.any()
            n = np.where((STEP_MASK != 0), ticks, 0)
            age = age + n
            stale = np.where(DRAW_MASK != 0, np.uint8(0), np.uint8(1)).astype(np.uint8)
        left, prev = out["budget"].copy(), row
    assert seen_done == 4 and out["halted"][0] == 1, f"the episodes did not end inside the calls as staggered: {seen_done} dones"
    assert np.array_equal(out["budget"][[1, 3]], [0, 1])
    entries = m.step_n(3, "every")
    t.step_n(3, "every")
    out = same(m, t, "the rendered call at the end")
    assert written(out, entries, A)[:, DRAW_MASK != 0].all() and not written(out, entries, A)[:, DRAW_MASK == 0].any()
    close(m, t)
