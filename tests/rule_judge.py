"""The tick-by-tick judge shared by the puzzle scenarios' models (tests/rearrange_model.py, tests/sokoban_model.py).  TEST INFRASTRUCTURE ONLY.

It follows one gym-like object (OracleGym, MegaverseGym) env by env and applies the three rules of tests/tower_model.py to a model module that offers
    State(snap, A, prev=None, **kw)          the record a tick starts from (prev: the state the model held for this env, or None)
    judge_tick(st, masks, poses, rules)      one tick of one env: st changes in place -> Result (rewards [A] of tower_model.Reward, margin, events,
                                             interact, solved_now, done: the model's own statement of whether the episode ends on this tick)
    differences(st, snap, A)                 the model's state after the tick against the implementation's record
(E) where no floored point lies within FRAGILE of a voxel boundary every discrete output is equal; (R) every reward is within the bound its Reward
carries; (U) what is not judged is counted: fragile ticks, and the tick an env finishes on -- there true_objective == the model's `solved` is checked
(unless an agent interacted on that very tick while the puzzle was unsolved: it may have solved it, the finished episode's poses are gone with it;
counted as finish_unjudged), then the model resynchronises."""
import numpy as np

import tower_model as T

ACT_INTERACT = T.ACT_INTERACT
FRAGILE = T.FRAGILE


class Judge:
    def __init__(self, model, snapshot_of, N, A, rules=None, **state_kw):
        self.model, self.snapshot_of, self.N, self.A, self.rules, self.state_kw = model, snapshot_of, N, A, rules, state_kw
        self.states = [None] * N
        self.ticks = self.interact_ticks = self.fragile = self.judged = self.finished = self.finish_unjudged = 0
        self.reward_ticks = self.solves = self.clamps = 0
        self.worst_ratio, self.min_margin = 0.0, float("inf")
        self.events = []       # (env, kind, agent, ...) of every tick
        self.objectives = []   # (env, true_objective, the model's solved, whether the last tick is unjudged) of every finished episode
        self.failures = []

    def sync(self, envs=None, fresh=False):
        """the model takes the implementation's record; fresh: a new episode, nothing of the old state is kept"""
        for e in (range(self.N) if envs is None else envs):
            self.states[e] = self.model.State(self.snapshot_of(e), self.A, prev=None if fresh else self.states[e], **self.state_kw)
            for d in getattr(self.states[e], "complaints", []):
                self.failures.append(f"env {e}: {d}")

    def tick(self, masks, rewards, dones, true_objective=None, min_margin=None):
        """after the implementation stepped: masks [N, A], rewards [N * A] fp32, dones [N]; min_margin: the scripted cases' own condition"""
        masks = np.asarray(masks).reshape(self.N, self.A)
        rewards = np.asarray(rewards, np.float32).reshape(self.N, self.A)
        self.ticks += 1
        for e in range(self.N):
            st = self.states[e]
            acted = any(int(m) & ACT_INTERACT for m in masks[e])
            self.reward_ticks += bool(rewards[e].any())
            if dones[e]:   # (U): the record is the next episode's
                self.finished += 1
                unjudged = acted and not st.solved
                self.finish_unjudged += unjudged
                if not acted and not self.model.ends_without_interaction(st):
                    self.failures.append(f"env {e}: done at episode_sec {st.sec!r} of {st.len!r}, the model's timer does not end here")
                if true_objective is not None:
                    got = [true_objective(e, a) for a in range(self.A)]
                    if not unjudged and not all(g == float(st.solved) for g in got):
                        self.failures.append(f"env {e}: true_objective {got} vs the model's solved {st.solved}")
                    self.objectives.append((e, got[0], st.solved, unjudged))
                self.sync([e], fresh=True)
                continue
            snap = self.snapshot_of(e)
            res = self.model.judge_tick(st, masks[e], T.poses_of(snap, self.A), self.rules)
            self.interact_ticks += res.interact > 0
            self.events += [(e,) + ev for ev in res.events]
            if res.interact:
                self.min_margin = min(self.min_margin, res.margin)
            if min_margin is not None and res.margin < min_margin:
                self.failures.append(f"env {e}: a scripted tick with margin {res.margin:.4f} < {min_margin}")
            if res.margin < FRAGILE:
                self.fragile += 1
                self.sync([e])
                continue
            self.judged += 1
            self.solves += res.solved_now
            self.clamps += res.clamped
            before = len(self.failures)
            if res.done:
                self.failures.append(f"env {e}: the model's timer ends the episode on this tick, the implementation goes on")
            for d in self.model.differences(st, snap, self.A):
                self.failures.append(f"env {e}: {d}")
            for a in range(self.A):
                r = res.rewards[a]
                err = abs(float(rewards[e, a]) - r.v)
                if r.bound > 0:
                    self.worst_ratio = max(self.worst_ratio, err / r.bound)
                if err > r.bound:
                    self.failures.append(f"env {e} agent {a}: reward {float(rewards[e, a])!r} vs the model's {r.v!r}, bound {r.bound:.3g}")
            if len(self.failures) > before:
                self.sync([e])   # (one difference is reported once)

    def report(self, tag, name):
        share = self.fragile / max(1, self.interact_ticks)
        print(f"\n[{tag}] {name}: ticks {self.ticks}, interact ticks {self.interact_ticks}, judged {self.judged}, fragile {self.fragile} ({100 * share:.2f} %), "
              f"finished {self.finished} (unjudged {self.finish_unjudged}), smallest margin {self.min_margin:.4f}, largest reward error / bound "
              f"{self.worst_ratio:.3f}, {self.counts()}")
        return self.counts(), share

    def counts(self):
        kinds = {}
        for ev in self.events:
            kinds[ev[1]] = kinds.get(ev[1], 0) + 1
        kinds.update(reward_ticks=self.reward_ticks, solves=self.solves, clamps=self.clamps,
                     solved_episodes=sum(o[1] == 1.0 for o in self.objectives), timed_out_episodes=sum(o[1] == 0.0 for o in self.objectives))
        return kinds


def run_judged(case, g, model, rules=None, min_margin=None, **state_kw):
    """plays a case (tests/tower_cases.py: play) on g under the model's eyes -> (Judge, [ticks] rewards [N * A] fp32, [ticks] dones [N], [ticks] true
    objectives of the envs that finished on the tick: {env: value})"""
    import tower_cases as TC
    judge = Judge(model, lambda e: TC.snapshot(g, e), case.N, case.A, rules, **state_kw)
    judge.sync(fresh=True)
    rewards, dones, objectives = [], [], []
    for what, row in TC.play(case, g):
        if what == "setup":   # poses and shaping only: the model reads both from the record
            judge.sync()
            continue
        r = np.asarray(g.get_last_rewards(), np.float32)
        d = TC.dones_of(g, case.N).astype(bool)
        rewards.append(r)
        dones.append(d)
        objectives.append({int(e): g.true_objective(int(e), 0) for e in np.nonzero(d)[0]})
        judge.tick(row[:, 4].reshape(case.N, case.A) << 8, r, d, g.true_objective, min_margin)
    return judge, rewards, dones, objectives
