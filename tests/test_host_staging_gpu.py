"""The host forms' way to the device (megaverse_amd/csrc/mv_staging.h: StagingPool, StagingPair), through its six users at once: host step mask, host draw
mask, host episode budget, host fork map, host masked reset, host level seeds.

Every gym has 5 envs -- an odd count, so the pairs' second halves and the N + 1 words of the budget's copy sit at offsets that are no multiple of anything
-- two agents and 32 x 32 frames.  A run is six rounds of the six calls and step_n(2) into an output ring of 12 entries: every tick of the run stays.  The
host forms are called through the C ABI with arrays of the test's own, which are overwritten with other VALID values as soon as a call returns: a staging
buffer read too late, reused too early, a wrong half or a wrong byte count shows as different bytes somewhere in what is compared -- the gym that never
waits starts behind a kernel that keeps its stream busy, so that its first rounds are enqueued before any of their copies has run.  Every comparison is exact
equality, and nothing is left out: every ring entry's observations, rewards and dones, the state rows of every tick, every env's snapshot, the budgets, the
halted count and the drained episode log."""
import numpy as np
import pytest

from megaverse_amd.extension import MegaverseGym

pytestmark = pytest.mark.gpu

N, A, W, H = 5, 2, 32, 32
ROUNDS, K = 6, 2
RING = ROUNDS * K
ENV_SEED, POLICY_SEED = 42, 1234
DEV = "cuda:0"
SENT = 0xA5
# TowerBuilding twice.  Default episodes outlast the run: no stepping call waits on the host, so behind a busy stream every host call of the first rounds
# returns before any copy has run (what shows a staging buffer reused too early); nothing finishes, so a budget acts only where it is 0 and the log stays
# empty.  episodeLengthSec -250 (the scenario adds 4 s per object): an episode lasts one tick or some hundred, by its object count -- envs that finish tick
# after tick (records for the log, budgets that run out) next to envs in the middle of an episode (whose state a fork carries over); with episodes that
# short every stepping call waits for the status words of the one before, so the host runs at most a round ahead.
TOWER = ("TowerBuilding", {})
TOWER_SHORT = ("TowerBuilding", {"episodeLengthSec": -250.0})
OBSTACLES = ("ObstaclesEasy", {})


def round_values(r):
    """the six arrays of round r, every one different from round to round: step mask, draw mask, budget, fork map, reset mask, seeds"""
    rng = np.random.RandomState(1000 + r)

    def mask():
        m = rng.randint(0, 2, N).astype(np.uint8)
        m[rng.randint(N)] = 0
        m[(int(np.flatnonzero(m == 0)[0]) + 1 + rng.randint(N - 1)) % N] = 1   # (at least one byte of either kind)
        return m

    step, draw = mask(), mask()
    budget = rng.choice(np.array([-1, 0, 1, 2, 3], np.int32), N).astype(np.int32)
    src = int(rng.randint(N))
    fork = np.full(N, -1, np.int32)
    for d in rng.permutation([e for e in range(N) if e != src])[:1 + r % 2]:   # one source, one or two destinations: no chain
        fork[d] = src
    reset = mask()
    seeds = np.where(rng.randint(0, 2, N) == 1, rng.randint(0, 1 << 30, N), -1).astype(np.int32)
    seeds[r % N] = 7 + r   # (at least one env re-seeded)
    return step, draw, budget, fork, reset, seeds


def other_values(r):
    """what the caller's arrays hold right after a host call has returned: valid too, and different -- the masks inverted, the rest the next round's"""
    step, draw, _, _, reset, _ = round_values(r)
    _, _, budget, fork, _, seeds = round_values(r + 1)
    return 1 - step, 1 - draw, budget, fork, 1 - reset, seeds


class Rig:
    """one gym, reset, with the episode log on, its outputs in rings that keep every tick of a run and its state rows attached"""

    def __init__(self, scenario, params, log=256):
        import torch
        self.g = g = MegaverseGym(scenario, W, H, N, A, 1, False, dict(params))
        g.seed(ENV_SEED)
        if log:
            g.set_episode_log(log)
        g.reset()
        self.obs = torch.full((RING, N * A, H, W, 4), SENT, dtype=torch.uint8, device=DEV)   # (an undrawn env's rows keep the sentinel: in every gym alike)
        self.rew = torch.full((RING, N * A), -7.0, dtype=torch.float32, device=DEV)
        self.done = torch.full((RING, N), 9, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        g.set_output_ring(RING, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        self.state = g.set_state_obs(True)
        self.ticks = 0
        self.held = []

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def keep_stream_busy(self):
        """a kernel that spins for some 80 ms on the gym's stream (torch's current one: the null stream): the host calls that follow return before any
        of their copies has run, until one waits on the host -- a pool has to grow, a pair has to wait for the call before last"""
        import torch
        torch.cuda._sleep(200_000_000)

    def call(self, name, *args):
        """a call of the C ABI: 0, not a warning and not an error"""
        g = self.g
        assert getattr(g._lib, name)(g._g, *args) == 0, f"{name}: {g._lib.mv_last_error().decode()}"

    def round_host(self, r, wait):
        """round r through the host forms, each from an array that is overwritten as soon as the call has returned; wait: the host waits behind every call"""
        names = ("mv_set_step_mask_host", "mv_set_draw_mask_host", "mv_set_episode_budget_host", "mv_fork_envs_host", "mv_reset_envs_host", "mv_seed_envs_host")
        for name, values, other in zip(names, round_values(r), other_values(r)):
            mine = values.copy()
            self.call(name, mine.ctypes.data, *((1,) if name == "mv_reset_envs_host" else ()))
            mine[:] = other
            if wait:
                self.sync()
        self.step_n(wait)

    def round_device(self, r):
        """round r through the device forms (tensors, held until the run is over), the host waiting behind every call"""
        import torch
        g = self.g
        step, draw, budget, fork, reset, seeds = (torch.as_tensor(v).to(DEV) for v in round_values(r))
        torch.cuda.synchronize()
        self.held += [step, draw, budget, fork, reset, seeds]
        for fn, t in ((g.set_step_mask, step), (g.set_draw_mask, draw), (g.set_episode_budget, budget), (g.fork_envs, fork), (g.reset_envs, reset),
                      (g.seed_envs, seeds)):
            fn(t)
            self.sync()
        self.step_n(True)

    def step_n(self, wait):
        self.call("mv_step_n", K, MegaverseGym.POLICIES["multidiscrete"], POLICY_SEED, self.ticks)
        self.ticks += K
        if wait:
            self.sync()

    def everything(self):
        """-> {name: bytes} of all a run leaves behind"""
        self.sync()
        g = self.g
        out = {"observations": self.obs.cpu().numpy().tobytes(), "rewards": self.rew.cpu().numpy().tobytes(), "dones": self.done.cpu().numpy().tobytes(),
               "state rows": self.state.cpu().numpy().tobytes(), "snapshots": b"".join(g.debug_snapshot_bytes(e).tobytes() for e in range(N)),
               "true objectives": g.get_true_objectives().tobytes()}
        if g.has_episode_budget():
            out["budgets"] = g.episode_budget().cpu().numpy().tobytes()
            out["halted count"] = g.halted_count()
        if g.episode_log_capacity():
            out["episode log"] = g.drain_episode_log().tobytes()
            assert g.episode_log_dropped == 0
        return out

    def close(self):
        self.sync()
        self.g.close()


def assert_same(got, ref, what):
    assert sorted(got) == sorted(ref)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"{what}: {bad} differ"


def test_round_values_differ_from_round_to_round():
    """(the rounds' own premise, checked where it is made: no array repeats the round before, and what overwrites a caller's array differs from it)"""
    for r in range(ROUNDS):
        for now, before, other in zip(round_values(r + 1), round_values(r), other_values(r + 1)):
            assert now.tobytes() != before.tobytes() and now.tobytes() != other.tobytes() and now.dtype == other.dtype and now.shape == other.shape == (N,)


@pytest.mark.parametrize("scenario,params", [TOWER, TOWER_SHORT], ids=["long_episodes", "short_episodes"])
def test_host_forms_without_a_wait_equal_device_forms_with_waits(hip, scenario, params):
    """1. TowerBuilding, two gyms from one seed.  Gym a: six rounds of host step mask, host draw mask, host budget, host fork map, host masked reset, host
    level seeds, step_n(2), without a synchronisation anywhere and behind a kernel that keeps the stream busy while the first rounds are enqueued.  Gym b: the same rounds through the device forms, the host waiting behind every call."""
    a, b = Rig(scenario, params), Rig(scenario, params)
    a.keep_stream_busy()
    for r in range(ROUNDS):
        a.round_host(r, wait=False)
    for r in range(ROUNDS):
        b.round_device(r)
    got, ref = a.everything(), b.everything()
    dones = np.frombuffer(ref["dones"], np.uint8)
    if params:
        assert (dones == 1).any() and (dones == 0).any() and len(ref["episode log"]) > 0, "the run finished no episode, or nothing else: it would prove little"
    else:
        assert ref["halted count"] > 0 and not dones.any(), "nobody halted, or an episode ended: not the run this case is meant to be"
    assert np.ptp(np.frombuffer(ref["observations"], np.uint8).reshape(RING, -1), axis=1).all(), "a tick drew nothing"
    assert_same(got, ref, "host forms, no wait, against device forms with waits")
    a.close(); b.close()


def test_host_forms_on_a_host_fed_gym_with_and_without_waits(hip):
    """2. ObstaclesEasy, whose episodes come from the host's feeder (the masked reset and the level seeds take the current consumed counts and refill), host
    forms only: the six rounds without a synchronisation of the test's own, and with one behind every call."""
    a, b = Rig(*OBSTACLES), Rig(*OBSTACLES)
    a.keep_stream_busy()
    for r in range(ROUNDS):
        a.round_host(r, wait=False)
    for r in range(ROUNDS):
        b.round_host(r, wait=True)
    assert_same(a.everything(), b.everything(), "host forms on a host-fed gym, no wait against waits")
    a.close(); b.close()


@pytest.mark.parametrize("scenario,params", [TOWER, OBSTACLES], ids=["tower", "obstacles"])
def test_gyms_created_and_closed_in_turn(hip, scenario, params):
    """3. four gyms one after the other in one process: each steps, uses every host form once (the fork right behind a stepping call, where a host map may
    travel on the simulation stream), steps, is read and closed.  mv_arena_bytes grows by what the host forms own -- N bytes per mask, 2 N + 1 words of
    budget -- in every gym alike, and every gym's outputs are the first's."""
    first = None
    for i in range(4):
        m = Rig(scenario, params, log=0)
        before = m.g.arena_bytes()
        m.step_n(False)
        step, draw, budget, fork, reset, seeds = round_values(0)
        for name, values in (("mv_fork_envs_host", fork), ("mv_set_step_mask_host", step), ("mv_set_draw_mask_host", draw),
                             ("mv_set_episode_budget_host", budget), ("mv_seed_envs_host", seeds)):
            m.call(name, values.ctypes.data)
        m.call("mv_reset_envs_host", reset.ctypes.data, 1)
        m.step_n(False)
        got = m.everything()
        got["arena bytes"] = (before, m.g.arena_bytes())
        assert got["arena bytes"][1] - before == 2 * N + (2 * N + 1) * 4
        m.close()
        if first is None:
            first = got
        assert_same(got, first, f"gym {i} against the first")
