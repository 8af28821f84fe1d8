"""GPU parity for Football: host-generated episodes (mv_gen_football.cpp) + the HIP tick (mv_tick_football.h: the ball's stated model on one lane,
then the controllers against the ball's new pose with the sphere collider of mv_physics.h in lane 0, the capsules in lanes 1..8, the room's boxes
from lane 9; kicks; timers; auto-reset) + raster against the CPU oracle's restatement (oracle/mv_oracle.cpp: its own containers, serial
colliders in the reference's object order): bit-exact state, the FootballState record, rewards, dones, true objectives and exact-mode pixels --
after resets, through rollouts with the events of test_oracle_football.py, at the scripted geometric edges of the collider (football_cases.py)
and over the launch shapes."""
import numpy as np
import pytest

import football_cases as FC
from hip_util import diff_snapshots, hip_snapshot, make_pair
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = pytest.mark.gpu


def frames(g, N, A):
    return np.stack([g.get_observation(e, a) for e in range(N) for a in range(A)])


def same_ball(og, hg, N, tag, envs=None):
    for e in range(N) if envs is None else envs:
        so, sh = og.football_state(e), FC.record(hg.debug_football_state(e))
        assert so.tobytes() == sh.tobytes(), (tag, e, so, sh)


def same_state(og, hg, N, A, tag, envs=None):
    for e in range(N) if envs is None else envs:
        d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
        assert not d, (tag, e, d[:5])
    same_ball(og, hg, N, tag, envs)


def set_actions(og, hg, acts):
    og.set_action_masks(action_masks(acts))
    hg.set_actions_batched(acts)


def orange(img):
    rgb = img[..., :3].astype(np.int16)
    return (rgb[..., 0] - rgb[..., 2] > 60) & (rgb[..., 0] >= rgb[..., 1]) & (rgb[..., 1] >= rgb[..., 2])


@pytest.mark.parametrize("A,seed", [(1, 3), (2, 14), (5, 15), (8, 92)])
def test_reset_parity(hip, A, seed):
    N = 24
    og, hg = make_pair(N, A, 32, 32, seed=seed, scenario="Football")
    same_state(og, hg, N, A, "reset")
    assert np.array_equal(frames(og, N, A), frames(hg, N, A))
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", [(128, 72), (64, 64), (40, 24)])
def test_pixels_after_reset_and_first_tick(hip, W, H):
    """the frames right after the reset (the ball drawn at radius 0.5), then after one no-op tick (radius 1.0): agent 0 of every env is put three
    to four units from the ball, looking at it, so the ball is on screen in at least a quarter of the frames (counted on the oracle's)"""
    N, A = 12, 2
    og, hg = make_pair(N, A, W, H, seed=65, scenario="Football")
    for e in range(N):
        ball = og.football_state(e)["pos"]
        pos = (float(ball[0]) + 3.0 + 0.1 * e, float(ball[1]) - 0.46 - 0.05 * e, float(ball[2]) + 0.3 * (e % 3))
        for g in (og, hg):
            g.debug_set_agent_pos(e, 0, *pos)
            g.debug_set_agent_yaw(e, 0, *FC.facing(pos, ball))
    og.render(); hg.render()
    for tag, radius in (("reset", 0.5), ("first tick", 1.0)):
        fo, fh = frames(og, N, A), frames(hg, N, A)
        bad = [i for i in range(N * A) if not np.array_equal(fo[i], fh[i])]
        assert not bad, (tag, bad, int((fo != fh).any(axis=-1).sum()))
        seen = orange(fo).reshape(N * A, -1).sum(axis=1)
        assert (seen >= 4).mean() >= 0.25, (tag, seen)
        assert all(float(og.football_state(e)["radius"]) == radius for e in range(N))
        same_state(og, hg, N, A, tag)
        if tag == "reset":
            set_actions(og, hg, np.zeros((N * A, 6), np.int32))
            og.step(); hg.step()
    og.close(); hg.close()


ROLLOUT = {"N": 8, "T": 400, "params": {"episodeLengthSec": 10.0}}   # 150-tick episodes: two auto-resets per env


# master seeds for which the oracle's run holds every event (searched on the CPU; the run is a pure function of the seed)
ROLLOUT_SEEDS = {(1, "random"): 7, (2, "random"): 1, (4, "random"): 1, (8, "random"): 1,
                 (1, "chaser"): 21, (2, "chaser"): 22, (4, "chaser"): 24, (8, "chaser"): 28}


@pytest.mark.parametrize("kind", ["random", "chaser"])
@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_rollout_parity(hip, A, kind):
    """rewards, dones, true objectives and the FootballState record of every env on every tick; the whole state on every done and every 10th
    tick; exact pixels every 20th tick against the tiled oracle raster.  "chaser": even envs chase the ball and kick -- their actions computed from
    the ORACLE's state and fed to both gyms --, odd envs act at random (test_oracle_football.py's mix); "random": everybody acts at random.  The
    run holds kicks, wall contacts, capsule contacts, resets and agents stopped by the ball (asserted, from the oracle's records)."""
    N, T = ROLLOUT["N"], ROLLOUT["T"]
    seed = ROLLOUT_SEEDS[(A, kind)]
    og, hg = make_pair(N, A, 48, 27, seed=seed, params=ROLLOUT["params"], scenario="Football")
    og.set_raster(True)   # the tiled raster: the brute-force image, byte for byte (tests/test_oracle_properties.py)
    events = FC.Events()
    snaps = [og.snapshot(e) for e in range(N)]
    for t in range(T):
        acts = FC.policy_actions(kind, og, N, A, seed, t)
        masks = action_masks(acts).reshape(N, A)
        set_actions(og, hg, acts)
        if t % 20 == 19:
            og.step(); hg.step()
            fo, fh = frames(og, N, A), frames(hg, N, A)
            assert np.array_equal(fo, fh), (t, int((fo != fh).any(axis=-1).sum()))
        else:
            og.step_norender(); hg.step_no_render()
        ro, rh = og.get_last_rewards(), hg.get_rewards_array()
        assert not ro.any() and ro.tobytes() == rh.tobytes(), (t, ro, rh)
        do = og.get_dones().astype(bool)
        assert np.array_equal(do, hg.get_dones().astype(bool)), (t, do)
        to = np.array([og.true_objective(e, a) for e in range(N) for a in range(A)], np.float32)
        assert not to.any() and to.tobytes() == hg.get_true_objectives().tobytes(), (t, to)
        same_ball(og, hg, N, t)
        if do.any() or t % 10 == 9:
            same_state(og, hg, N, A, t)
        for e in range(N):
            snap = og.snapshot(e)
            events.tick(A, masks[e], snaps[e], snap, og.football_state(e), bool(do[e]))
            snaps[e] = snap
    assert events.all_seen() and events.resets == 2 * N, events
    og.close(); hg.close()


@pytest.mark.parametrize("A", [1, 2])
def test_scripted_contacts(hip, A):
    """one env per case of football_cases.scripted_cases() -- walking into the ball from eight headings, drops onto it, the degenerate axis in
    the ball's contact search and in the controller's recovery, a moving ball into a standing agent, the corner with three contacts, a push and a
    pending force, two agents kicking on one tick, an agent placed inside both the ball and another capsule (the recovery's order), free flight out of the room -- set identically on both gyms through the debug hooks: the whole
    state and the ball's record after every tick, exact pixels after the last; and each case did what it is named after (on the oracle)"""
    cases = [c for c in FC.scripted_cases() if len(c.agents) == A]
    N, T = len(cases), 45
    og, hg = make_pair(N, A, 64, 36, seed=5, scenario="Football")
    for e, c in enumerate(cases):
        c.place(hg, e)
    acts = np.stack([a for c in cases for a in c.actions])

    def device_tick(t):
        hg.set_actions_batched(acts)
        hg.step_no_render()
        for e, c in enumerate(cases):
            d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
            assert not d, (c.name, t, d[:5])
            so, sh = og.football_state(e), FC.record(hg.debug_football_state(e))
            assert so.tobytes() == sh.tobytes(), (c.name, t, so, sh)

    traces = FC.run_on_oracle(og, cases, T, after_tick=device_tick)
    og.render(); hg.render()
    fo, fh = frames(og, N, A), frames(hg, N, A)
    bad = [cases[i // A].name for i in range(N * A) if not np.array_equal(fo[i], fh[i])]
    assert not bad, bad
    for c, trace in zip(cases, traces):
        try:
            c.expect(trace)
        except AssertionError as ex:
            raise AssertionError(f"case {c.name}: {ex}") from ex
    og.close(); hg.close()


def test_launch_shapes_against_the_oracle(hip):
    """N = 33 envs, 64 x 64, exact pixels, 64 ticks of the counter-based random policy: the oracle steps tick by tick; beside it (a) step() per
    tick, (b) step_n(16) into an output ring of 16, (c) step() with pipelining off.  Rewards, dones and frames of every tick (the ring's entry),
    the whole state after every 16 ticks"""
    import torch
    N, A, W, H, K, seed = 33, 1, 64, 64, 16, 77
    og, ga = make_pair(N, A, W, H, seed=5, scenario="Football")
    gb = MegaverseGym("Football", W, H, N, A, 1, False, {})
    gc = MegaverseGym("Football", W, H, N, A, 1, False, {})
    for g in (gb, gc):
        g.seed(5); g.reset()
    gc.set_pipelining(False)
    for g in (ga, gb, gc):
        assert g.pixel_mode() == "exact"
    ring = (torch.zeros((K, N, H, W, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((K, N), dtype=torch.float32, device="cuda:0"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    gb.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    og.set_raster(True)
    for call in range(4):
        gb.step_n(K, "multidiscrete", seed, K * call)
        gb.synchronize(); torch.cuda.synchronize()
        o, r, d = ring[0].cpu().numpy(), ring[1].cpu().numpy(), ring[2].cpu().numpy()
        for j in range(K):
            t = K * call + j
            og.set_action_masks(action_masks(sample_actions(seed, t, N * A)))
            og.step()
            fo, ro, do = frames(og, N, A), og.get_last_rewards(), og.get_dones()
            for g in (ga, gc):
                g.sample_random_actions(seed, t)
                g.step()
            for what, fh, rh, dh in (("step", frames(ga, N, A), ga.get_rewards_array(), ga.get_dones()), ("step_n", o[j], r[j], d[j]),
                                     ("unpipelined", frames(gc, N, A), gc.get_rewards_array(), gc.get_dones())):
                assert np.array_equal(fo, fh), (what, t, int((fo != fh).any(axis=-1).sum()))
                assert ro.tobytes() == np.ascontiguousarray(rh, np.float32).tobytes() and np.array_equal(do.astype(bool), np.asarray(dh).astype(bool)), (what, t)
        for what, g in (("step", ga), ("step_n", gb), ("unpipelined", gc)):
            same_state(og, g, N, A, (what, call))
    og.close(); ga.close(); gb.close(); gc.close()
