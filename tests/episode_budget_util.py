"""Shared by tests/test_episode_budget*.py: the rule of episode budgets (include/megaverse_hip.h: mv_set_episode_budget) restated in numpy, and the episode
log with budgets, independent of the library under test."""
import numpy as np

import step_mask_util
from reset_envs_util import H, N, W  # noqa: F401  (re-exported)


def rule(dones, mask, left):
    """dones [k][N]: what tick t stages for env e IF it steps; mask [N] or None; left [N] -> (steps bool [k][N], left behind the last tick).
    An env steps when its mask byte (if any) is non-zero and its budget is not 0; a stepped tick that staged done takes one off a positive budget."""
    dones = np.asarray(dones) != 0
    k, n = dones.shape
    left = np.array(left, np.int64).copy()
    on = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    steps = np.zeros((k, n), bool)
    for t in range(k):
        steps[t] = on & (left != 0)
        left -= (steps[t] & dones[t] & (left > 0)).astype(np.int64)
    return steps, left.astype(np.int32)


class BudgetModel(step_mask_util.MaskedModel):
    """step_mask_util's model plus mv_set_episode_budget: self.left is the budget (None: none attached); a tick of a halted env counts like a frozen one's --
    nothing added, no record -- and a finishing tick spends"""

    left = None

    def attach(self, budget):
        self.left = None if budget is None else np.array(budget, np.int32).copy()

    def feed(self, rewards, dones, tobj, step_mask=None):
        if self.left is None:
            return super().feed(rewards, dones, tobj, step_mask)
        on = np.ones(self.N, bool) if step_mask is None else np.asarray(step_mask) != 0
        for r, d, o in zip(rewards, dones, tobj):
            steps = on & (self.left != 0)
            super().feed(r[None], d[None], o[None], steps.astype(np.uint8))
            self.left -= (steps & (np.asarray(d) != 0) & (self.left > 0)).astype(np.int32)


# ---- the GPU tests' schedules, from the CPU oracle as it is ------------------------------------------------------------------------------------------
# The envs are independent, so what env e of a gym must be behind a tick is env e of an oracle that stepped on exactly the gym ticks env e stepped on, with
# the actions of those tick indices.  Which ticks those are follows from the rule and the oracle's own dones, tick by tick (walk).
import functools

import episode_log_util as U
import oracle_lib
from megaverse_amd.rollout import action_masks, sample_actions

POLICY_SEED = 5
PAST = 10           # ticks compared behind the last halt
TARGETS = (7, 8, 2, 3, 4, 5, 6, 9)   # wanted halting ticks, relative to the attach: tick 7 and tick 8 of a 16-tick call (two launches of 8), the others inside a launch
# family -> (scenario, params, ticks of oracle P searched for episode ends; 0: the endings depend on the actions -- delays are searched, not computed;
# the env seed: ObstaclesEasy's is one with which no env ends its first episodes by what it does).
# The scenarios whose episodes are as long as episodeLengthSec says get 4.3 s = 65 ticks: the shortest episodes the library still steps in resident
# multi-tick launches (below 64 ticks mv_step_n goes tick by tick: include/megaverse_hip.h).  The tick-by-tick oracle tests would take 1 - 2 s as well; they
# use 4.3 because they share ONE schedule with the entry matrix, the log tests and the mask test, which need the resident launches: what the oracle pins
# tick by tick is then the very schedule the batched entries are compared on.  TowerBuilding, Collect and HexMemory add seconds per generated
# object, the Obstacles family never goes below 35 s per platform: their envs' clocks are staggered over hundreds of ticks instead, stepped without rendering.
FAMILIES = {"tower": ("TowerBuilding", {"episodeLengthSec": -180.0}, 3000, 11), "obstacles_easy": ("ObstaclesEasy", {"episodeLengthSec": 1.0}, 3000, 1),
            "collect": ("Collect", {"episodeLengthSec": -60.0}, 3000, 11), "rearrange": ("Rearrange", {"episodeLengthSec": 4.3}, 200, 11),
            "sokoban": ("Sokoban", {"episodeLengthSec": 4.3}, 200, 11), "hex_memory": ("HexMemory", {"episodeLengthSec": -42.0}, 3000, 11),
            "boxagone": ("BoxAGone", {}, 0, 11), "football": ("Football", {"episodeLengthSec": 4.3}, 200, 11), "empty": ("Empty", {"episodeLengthSec": 4.3}, 200, 11)}
# The same scenarios with episodeLengthSec = 4.3: TowerBuilding, Collect and HexMemory add their seconds per object on top, so their envs' first episodes end
# thousands of ticks in -- too far for oracle walks that render, near enough for gyms stepped without rendering.  The tests that compare two paths of the
# library (the entry matrix) use these, so that the library steps them in resident multi-tick launches; which ticks the envs halt on is read off the
# tick-by-tick twin there.
FAMILIES.update({"tower_long": ("TowerBuilding", {"episodeLengthSec": 4.3}, 4500, 3), "collect_long": ("Collect", {"episodeLengthSec": 4.3}, 4500, 11),
                 "hex_memory_long": ("HexMemory", {"episodeLengthSec": 4.3}, 4500, 11)})
ORACLE_FAMILIES = sorted(f for f in FAMILIES if not f.endswith("_long"))
SEARCH_TA, MAX_DELAY = 12, 12   # action-dependent endings: the attach tick, and the delays searched (0 .. MAX_DELAY - 1)


def new_oracle(family, A):
    scenario, params, _, seed = FAMILIES[family]
    U.boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, dict(params))
    og.seed(seed)
    og.reset()
    return og


def actions(t, A):
    return sample_actions(POLICY_SEED, t, N * A)


def capture(og, scenario, A, e):
    """env e of test_reset_envs_gpu.capture's dictionary (what its check_env compares an env of the gym with); the other envs' states and frames are left out"""
    out = {"snap": [og.snapshot(q) if q == e else None for q in range(N)], "rewards": og.get_last_rewards().copy(), "dones": og.get_dones().copy(),
           "tobj": np.array([og.true_objective(q, a) for q in range(N) for a in range(A)], np.float32),
           "frames": [og.get_observation(q // A, q % A).copy() if q // A == e else None for q in range(N * A)]}
    if scenario == "BoxAGone":
        out["bag"] = [og.boxagone_state(q) if q == e else None for q in range(N)]
    if scenario == "Football":
        out["ball"] = [og.football_state(q) if q == e else None for q in range(N)]
    return out


def frozen(c):
    """what a frozen tick leaves of capture c: the state and the frames, rewards +0.0f, dones 0"""
    return dict(c, rewards=np.zeros_like(c["rewards"]), dones=np.zeros_like(c["dones"]))


@functools.lru_cache(maxsize=None)
def done_ticks(family, A, delay, ticks):
    """the gym ticks on which each env reports done when every env is frozen for the first `delay` ticks and steps from then on (no rendering)"""
    og = new_oracle(family, A)
    out = [[] for _ in range(N)]
    for t in range(delay, ticks):
        og.set_action_masks(action_masks(actions(t, A)))
        og.step_norender()
        for e in np.flatnonzero(og.get_dones()).tolist():
            out[e].append(t)
    og.close()
    return out


@functools.lru_cache(maxsize=None)
def plan(family, A=1):
    """-> (TA, candidates): the budget is attached in front of gym tick TA; env e is frozen for its first d ticks, d one of candidates[e] (all < TA, the
    preferred one first), so that with budget 1 the envs halt on TA + TARGETS -- checked by schedule() on the walks, not assumed"""
    scenario, params, horizon, _ = FAMILIES[family]
    if horizon == 0:   # the endings depend on the actions, which go by the gym's tick index: one oracle per delay
        f = np.array([[min([t for t in done_ticks(family, A, d, SEARCH_TA + 96)[e] if t >= SEARCH_TA], default=-1) for e in range(N)]
                      for d in range(MAX_DELAY)])
        delay, used = [None] * N, set()
        for target in TARGETS[:2]:
            hit = [(d, e) for e in range(N) for d in range(MAX_DELAY) if delay[e] is None and f[d, e] >= 0 and (f[d, e] - SEARCH_TA) % 16 == target]
            assert hit, f"{family}: no delay lets an env halt on tick {target} of a 16-tick call"
            d, e = min(hit, key=lambda de: (f[de], de[1], de[0]))
            delay[e] = d
            used.add(int(f[d, e]))
        for e in range(N):
            if delay[e] is None:
                ok = [d for d in range(MAX_DELAY) if f[d, e] >= 0]
                fresh = [d for d in ok if int(f[d, e]) not in used]
                delay[e] = min(fresh or ok, key=lambda d: (f[d, e], d))
                used.add(int(f[delay[e], e]))
        return SEARCH_TA, tuple((d,) for d in delay)
    # the endings depend on the clock and on the generated episode: freezing an env for d ticks moves its episode ends d ticks back.  Env e ends an episode
    # of more than TARGETS[e] ticks on c: frozen for TA + TARGETS[e] - c ticks, it ends it on TA + TARGETS[e], and the episode before it ends before TA.
    # (Where an env can also end an episode by what it does -- the Obstacles family -- a shifted env acts on other actions and may end elsewhere: the later
    # ends of the same env are the next candidates.)
    P = done_ticks(family, A, 0, horizon)
    ends = []
    for e in range(N):
        ends.append([t for q, t in enumerate(P[e]) if t >= TARGETS[e] and t - (P[e][q - 1] if q else -1) > TARGETS[e]])
        assert ends[e], f"{family}: env {e} ends no episode of more than {TARGETS[e]} ticks within {horizon} ticks"
    TA = max(ends[e][0] - TARGETS[e] for e in range(N))
    return TA, tuple(tuple(TA + TARGETS[e] - c for c in ends[e] if 0 <= TA + TARGETS[e] - c) for e in range(N))


@functools.lru_cache(maxsize=None)
def walk(family, A, e, delay, attaches, first, ticks=None):
    """Env e on the rule, from an oracle that steps exactly when env e steps: frozen for the first `delay` ticks; attaches: ((tick, budget of env e), ...), each
    in front of its tick.  -> {gym tick: (capture, stepped, left behind the tick)} for the ticks from `first` on (the earlier ones are not rendered) up to
    `ticks`, or (None) up to the env's first halt."""
    scenario = FAMILIES[family][0]
    og = new_oracle(family, A)
    cap, left, out, t = None, -1, {}, 0
    while t < ticks if ticks is not None else (left != 0 or t <= first):
        for ta, b in attaches:
            if ta == t:
                left = b
        steps = t >= delay and left != 0
        if steps:
            og.set_action_masks(action_masks(actions(t, A)))
            og.step_norender()
            if og.get_dones()[e] and left > 0:
                left -= 1
        if t >= first:
            if steps or cap is None:
                og.render_env(e)   # (env e's frames only: the other envs of this oracle are nobody's reference)
                cap = capture(og, scenario, A, e)
            out[t] = (cap if steps else frozen(cap), steps, left)
        t += 1
        assert t < 6000, f"{scenario}: env {e} does not halt"
    og.close()
    return out


def at(w, t):
    """entry t of a walk that ended with the env's halt: behind it the env stands still"""
    if t in w:
        return w[t]
    last = max(w)
    assert t > last and w[last][2] == 0
    return frozen(w[last][0]), False, 0


def schedule(family, A=1, budget=1):
    """the schedule of the oracle tests for one family: (scenario, params, env seed, TA, delays, per-env walks from tick TA - 1 on, halting ticks relative to TA)"""
    scenario, params, _, seed = FAMILIES[family]
    TA, candidates = plan(family, A)
    delays, walks = [], []
    for e in range(N):
        tried = []
        for d in candidates[e]:
            assert 0 <= d < TA, (family, TA, candidates[e])
            tried.append((d, walk(family, A, e, d, ((TA, budget),), TA - 1)))
            if budget != 1 or len(candidates[e]) == 1 or (max(tried[-1][1]) - TA) % 16 == TARGETS[e]:
                break
        else:
            tried.append(tried[0])
        delays.append(tried[-1][0])
        walks.append(tried[-1][1])
    halts = [max(w) - TA for w in walks]
    return scenario, params, seed, TA, delays, walks, halts


def assert_condition(halts, what):
    """what the 8 halting ticks (relative to the attach, where 16-tick calls of two 8-tick launches start) must cover"""
    assert len(set(halts)) >= 4, f"{what}: halting ticks {halts}"
    assert any(h % 16 == 7 for h in halts) and any(h % 16 == 8 for h in halts), f"{what}: nobody halts on ticks 7 and 8 of a 16-tick call: {halts}"
    assert any(h % 8 not in (0, 7) for h in halts), f"{what}: nobody halts inside a launch: {halts}"
    assert min(halts) >= 0


def stagger_plan(family, A=1):
    """-> (TA, delays) for the gym-side stagger: the walked schedule's, or -- the *_long families -- the plan's preferred delays"""
    if family.endswith("_long"):
        TA, candidates = plan(family, A)
        return TA, tuple(c[0] for c in candidates)
    _, _, _, TA, delays, _, _ = schedule(family, A)
    return TA, tuple(delays)
