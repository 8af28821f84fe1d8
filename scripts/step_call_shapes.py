#!/usr/bin/env python
"""What every shape of stepping call enqueues and computes: a fixed list of small calls on seeded gyms, one after the other, each on gyms of its own.
Per shape one line: the launch-count deltas of every call (mv_debug_launch_counts: step launches + observation launches) and, after a synchronise, a SHA-256
over the observations, rewards, dones, true objectives and whatever rings, row records or log records the shape attached.  Two commits whose lines are
equal enqueue the same launches for these shapes and compute the same bytes; profiles/step_call_shapes.txt is the output of the commit that keeps it.
Needs a GPU.
    python scripts/step_call_shapes.py [--only SUBSTRING] [--out FILE]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402
from megaverse_amd.extension import GymGroup, MegaverseGym   # noqa: E402

N, S = 7, 32   # envs, observation size
SHAPES = []


def shape(fn):
    SHAPES.append(fn)
    return fn


class Run:
    """one shape: the gyms it made, the calls it timed, what it hashes"""

    def __init__(self):
        self.gyms, self.groups, self.keep, self.deltas, self.sha = [], [], [], [], hashlib.sha256()

    def gym(self, scenario="TowerBuilding", A=1, seed=11, ring=0, params=None, reset=True):
        g = MegaverseGym(scenario, S, S, N, A, 1, False, params or {})
        g.set_pixel_mode("fast")
        g.seed(seed)
        if reset:
            g.reset()
        self.gyms.append(g)
        if ring:   # observations, rewards and dones each in a ring of their own
            t = (torch.zeros((ring, N * A, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((ring, N * A), dtype=torch.float32, device="cuda"),
                 torch.zeros((ring, N), dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            g.set_output_ring(ring, *[x.data_ptr() for x in t])
            self.keep.extend(t)
        return g

    def call(self, g, fn, *args, **kw):
        """one stepping call: its launch-count delta (g: the gym, or the leader of the group)"""
        before = g.debug_launch_counts()
        fn(*args, **kw)
        after = g.debug_launch_counts()
        self.deltas.append(f"{after[0] - before[0]}+{after[1] - before[1]}")

    def add(self, *arrays):
        for a in arrays:
            self.sha.update(np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes())

    def finish(self):
        for g in self.gyms:
            g.synchronize()
        torch.cuda.synchronize()
        for g in self.gyms:
            self.add(*[g.get_observation(e, a) for e in range(N) for a in range(g.num_agents_per_env)])
            self.add(g.get_rewards_array(), g.get_dones(), g.get_true_objectives())
            for t in (g.state_obs(), g.scene_obs_ring()):
                if t is not None:
                    self.add(t)
            if g.episode_log_capacity():
                self.add(g.drain_episode_log())
        self.add(*self.keep)
        for grp in self.groups:
            grp.close()
        for g in self.gyms:
            g.close()
        return " ".join(self.deltas), self.sha.hexdigest()


def single_ticks(r, g, ticks=3, render=True):
    for st in range(ticks):
        g.sample_random_actions(9, st)
        r.call(g, g.step if render else g.step_no_render)


def batched(r, g, ks=(8, 16), policy="multidiscrete", render="every"):
    st = 0
    for k in ks:
        r.call(g, g.step_n, k, policy, 9, st, render=render)
        st += k


def action_ring(r, g, count=8):
    a = (np.random.default_rng(7).integers(0, 1 << 30, (count, N * g.num_agents_per_env, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)
    t = torch.as_tensor(a).to("cuda")
    torch.cuda.synchronize()
    g.set_action_ring(count, t.data_ptr())
    r.keep.append(t)


@shape
def one_tick_pipelined(r):
    g = r.gym()
    single_ticks(r, g)
    g.set_actions_batched(np.ones((N, 6), np.int32))   # (host actions: the upload on the simulation stream)
    r.call(g, g.step)
    single_ticks(r, g, 2, render=False)


@shape
def one_tick_two_agents(r):
    single_ticks(r, r.gym(A=2))


@shape
def one_tick_not_pipelined(r):
    g = r.gym()
    g.set_pipelining(False)
    single_ticks(r, g)
    single_ticks(r, g, 2, render=False)


@shape
def k8_k16_ring(r):
    batched(r, r.gym(ring=16))


@shape
def k8_k16_ring_two_agents(r):
    batched(r, r.gym(A=2, ring=16))


@shape
def k8_k16_no_ring(r):
    batched(r, r.gym())


@shape
def k8_k16_not_pipelined(r):
    g = r.gym(ring=16)
    g.set_pipelining(False)
    batched(r, g)


@shape
def k8_exact_pixels(r):
    g = r.gym(ring=16)
    g.set_pixel_mode("exact")
    batched(r, g, (8,))


@shape
def ring_2k_pass_overlap(r):
    g = r.gym(ring=32)
    g.set_pass_overlap(True)
    batched(r, g, (16, 16, 8, 8, 8))


@shape
def render_none_last_resident(r):
    g = r.gym(ring=16)
    batched(r, g, (8, 16), render="none")
    batched(r, g, (8, 16, 3), render="last")


@shape
def render_none_last_single_tick_fallback(r):
    g = r.gym("ObstaclesEasy", A=2, ring=16)
    batched(r, g, (8,), render="none")
    batched(r, g, (8, 16), render="last")


@shape
def sequence_action_ring(r):
    g = r.gym(ring=16)
    action_ring(r, g)
    batched(r, g, (8, 16), policy="sequence")
    batched(r, g, (8,), policy="sequence", render="last")


@shape
def macro_8_and_12(r):
    g = r.gym(ring=4)
    act = (np.arange(N * 6).reshape(N, 6) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)
    r.call(g, g.macro_step, 8, act)
    r.call(g, g.macro_step, 12, act, np.arange(N, dtype=np.int32) * 2)
    r.call(g, g.macro_step, 12, act, None, render="none")


@shape
def profile_whole_call(r):
    g = r.gym(ring=16)
    g.profile_begin(2)
    batched(r, g, (8, 8, 8))
    g.profile_end()


@shape
def profile_per_tick(r):
    g = r.gym()
    g.profile_begin(5)
    batched(r, g, (4, 4))   # (the second call runs out of entries after its first tick)
    single_ticks(r, g, 1)
    g.profile_end()


def group_of_two(r, ring=0, exact=False):
    gs = [r.gym(seed=11, ring=ring), r.gym(seed=12, ring=ring)]
    if exact:
        for g in gs:
            g.set_pixel_mode("exact")
    grp = GymGroup(gs)
    r.groups.append(grp)
    return gs[0], grp


@shape
def group_tick_by_tick(r):
    L, grp = group_of_two(r)
    for st in range(2):
        r.call(L, grp.step, 1, True, "multidiscrete", 3, st)
    r.call(L, grp.step, 4, True, "multidiscrete", 3, 2)   # (no rings: one union launch per tick)
    r.call(L, grp.step, 2, False, "multidiscrete", 3, 6)


@shape
def group_batched(r):
    L, grp = group_of_two(r, ring=8)
    r.call(L, grp.step, 8, True, "multidiscrete", 3, 0)
    r.call(L, grp.step, 12, True, "multidiscrete", 3, 8)


@shape
def group_exact_pixels(r):
    L, grp = group_of_two(r, ring=8, exact=True)
    r.call(L, grp.step, 4, True, "multidiscrete", 3, 0)


def with_option(r, attach, ring=16):
    g = r.gym(ring=ring)
    attach(g)
    batched(r, g, (8, 16))
    batched(r, g, (8,), render="last")
    single_ticks(r, g, 2)
    return g


@shape
def option_step_mask(r):
    with_option(r, lambda g: g.set_step_mask(np.arange(N) % 2 == 0))


@shape
def option_draw_mask(r):
    with_option(r, lambda g: g.set_draw_mask(np.arange(N) % 3 != 0))


@shape
def option_still_frames_ring(r):
    def attach(g):
        g.set_step_mask(np.arange(N) % 2 == 0)   # (frozen envs: frames that stay still)
        g.set_still_frames(True)
    with_option(r, attach)


@shape
def option_still_frames_no_ring(r):
    with_option(r, lambda g: g.set_still_frames(True), ring=0)


@shape
def option_episode_budget(r):
    with_option(r, lambda g: g.set_episode_budget(np.arange(N, dtype=np.int32) % 2))


@shape
def option_state_obs(r):
    with_option(r, lambda g: g.set_state_obs(True))


@shape
def option_scene_obs(r):
    with_option(r, lambda g: g.set_scene_obs(True))


@shape
def both_row_records(r):
    def attach(g):
        g.set_state_obs(True)
        g.set_scene_obs(True)
    g = with_option(r, attach)
    r.call(g, g.macro_step, 12, np.ones((N, 6), np.int32))
    g.render()   # (the refresh of both records)


@shape
def both_row_records_two_agents_no_ring(r):
    g = r.gym(A=2)
    g.set_state_obs(True)
    g.set_scene_obs(True)
    batched(r, g, (8,))
    batched(r, g, (4,), render="none")


@shape
def episode_log(r):
    g = r.gym(ring=16, params={"episodeLengthSec": 6.0})
    g.set_episode_log(64)
    batched(r, g, (16,) * 8)
    batched(r, g, (8,), render="none")
    single_ticks(r, g, 2)


@shape
def episode_log_not_pipelined(r):
    g = r.gym(params={"episodeLengthSec": 6.0})
    g.set_pipelining(False)
    g.set_episode_log(64)
    batched(r, g, (8,) * 14)


@shape
def host_fed_not_pipelined(r):
    g = r.gym("ObstaclesEasy")
    g.set_pipelining(False)
    single_ticks(r, g)
    batched(r, g, (8,))


@shape
def status_period_one(r):
    g = r.gym(ring=8, params={"episodeLengthSec": 2.0})
    batched(r, g, (8, 3))
    single_ticks(r, g, 2)


def stagger(g, ends):
    """TowerBuilding adds 4 s per object to episodeLengthSec: the clocks are read off the scene rows, and env e is stepped, undrawn, until its episode ends
    on its ends[e]-th tick from here (-1: the env is left alone)"""
    g.set_scene_obs(True)
    g.render()   # (refreshes the rows)
    rows = np.stack([g.get_scene_observation(e) for e in range(N)])
    g.set_scene_obs(None)
    left = np.zeros(N, np.int64)
    for e in range(N):
        sec, dt = np.float32(rows[e, 5]), np.float32(1.0) / np.float32(15.0)   # (columns 5, 6: episode_sec, episode_len; the tick's own fp32 sum)
        while ends[e] >= 0 and sec < rows[e, 6]:
            sec, left[e] = np.float32(sec + dt), left[e] + 1
        left[e] = max(left[e] - 1 - ends[e], 0)
    st = 0
    while (left > 0).any():
        k = int(min(left[left > 0].min(), 64))
        g.set_step_mask(left > 0)
        g.step_n(k, "multidiscrete", 5, st, render="none")
        st += k
        left = np.where(left > 0, left - k, 0)
    g.set_step_mask(None)


def every_option(r, scenario="TowerBuilding", A=1, still=True, params=None, ends=None):
    """a gym with every option on at once: a step mask that freezes two envs, an episode budget of 1 on one env and 2 on another, a draw mask that leaves one
    env out, still frames, state and scene rows, the episode log, an output ring of 16.  ends: the ticks the envs' episodes end on (stagger)"""
    g = r.gym(scenario, A=A, ring=16, params={"episodeLengthSec": 4.3} if params is None else params)
    g.set_episode_log(64)
    if ends is not None:
        stagger(g, ends)
    g.set_step_mask(np.array([1, 1, 0, 1, 1, 0, 1], bool))
    g.set_episode_budget(np.array([-1, 1, -1, 2, -1, -1, -1], np.int32))
    g.set_draw_mask(np.array([1, 1, 1, 1, 0, 1, 1], bool))
    if still:
        g.set_still_frames(True)
    g.set_state_obs(True)
    g.set_scene_obs(True)
    return g


def every_option_done(r, g):
    r.add(g.episode_budget(), np.array([g.halted_count()], np.int64))   # (halted_count waits for the gym's stream)


def every_option_step_n(r, A, render):
    """8 calls of 9 ticks: a launch of 8 ticks and one of 1, the carried option state crosses the boundary through memory; then a rendered call"""
    g = every_option(r, A=A, ends=(9 + 7, 18 + 3, -1, 27 + 7, 36 + 8, -1, 45 + 0))   # (the end of a launch of 8, the launch of 1, a call's first tick, inside)
    batched(r, g, (9,) * 8, render=render)
    batched(r, g, (3,))
    every_option_done(r, g)


def every_option_macro(r, A):
    """8 macro steps of up to 11 ticks with per-env ticks 0, 1 and above k, render 'last' and 'none' in turn; then a rendered call"""
    g = every_option(r, A=A, ends=(-1, 3, -1, 11 + 8, 22 + 3, -1, 12 + 1))   # (in the env's own ticks)
    act = (np.arange(N * A * 6).reshape(N * A, 6) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)
    for c in range(8):
        r.call(g, g.macro_step, 11, act, np.array([0, 1, 11, 12, 15, 5, 3], np.int32), render="last" if c % 2 == 0 else "none")
    batched(r, g, (3,))
    every_option_done(r, g)


def every_option_obstacles(r, pipe):
    """ObstaclesEasy, one agent, the two-wave kernel forced on or off (still frames off: a gym with them never launches it)"""
    before = os.environ.get("MV_STEP_PIPE")
    os.environ["MV_STEP_PIPE"] = pipe   # (read at every launch)
    try:
        g = every_option(r, "ObstaclesEasy", still=False, params={})
        batched(r, g, (9, 9, 9))
        batched(r, g, (9,), render="last")
        every_option_done(r, g)
        for x in r.gyms:
            x.synchronize()
    finally:
        if before is None:
            del os.environ["MV_STEP_PIPE"]
        else:
            os.environ["MV_STEP_PIPE"] = before


for _A in (1, 3):
    for _render in ("every", "last", "none"):
        shape(lambda r, A=_A, render=_render: every_option_step_n(r, A, render)).__name__ = f"every_option_k9_{_render}_a{_A}"
    shape(lambda r, A=_A: every_option_macro(r, A)).__name__ = f"every_option_macro_11_a{_A}"
for _pipe in ("1", "0"):
    shape(lambda r, pipe=_pipe: every_option_obstacles(r, pipe)).__name__ = f"every_option_obstacles_pipe_{_pipe}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the shape of this name, or the shapes whose name contains this")
    ap.add_argument("--list", action="store_true", help="print the shapes' names and stop")
    ap.add_argument("--out", default="", help="write the lines here as well")
    args = ap.parse_args()
    if args.list:
        return print("\n".join(fn.__name__ for fn in SHAPES))
    if not torch.cuda.is_available():
        sys.exit("step_call_shapes: no GPU")
    lines = []
    exact = args.only in [fn.__name__ for fn in SHAPES]   # (a whole name runs that shape alone)
    for fn in SHAPES:
        if args.only == fn.__name__ or (not exact and args.only in fn.__name__):
            r = Run()
            fn(r)
            deltas, sha = r.finish()
            lines.append(f"{fn.__name__:<40} launches {deltas}  sha256 {sha}")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
