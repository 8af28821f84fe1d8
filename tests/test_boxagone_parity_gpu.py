"""GPU parity for BoxAGone: host-generated episodes (mv_gen_boxagone.cpp) + HIP step (mv_tick_boxagone.h: the room, the platforms in the 3 x 3
cells around each agent, the placed temporary platforms, the other agents; the platform table, timers and ring of temporary platforms) + raster
against the CPU oracle's independent restatement (every platform and temporary a collider, the reference's containers): bit-exact state, the
BoxAGoneState record, rewards, dones, true objectives and exact-mode pixels."""
import numpy as np
import pytest

import boxagone_model as M
import oracle_lib
from hip_util import diff_snapshots, hip_snapshot, make_pair
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1200)]


def frames(g, N, A):
    return np.stack([g.get_observation(e, a) for e in range(N) for a in range(A)])


def same_state(og, hg, N, A, tag, envs=None):
    for e in range(N) if envs is None else envs:
        d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
        assert not d, (tag, e, d[:5])
        so, sh = og.boxagone_state(e), hg.debug_boxagone_state(e).view(M.STATE)[0]
        bad = [n for n in M.STATE.names if so[n].tobytes() != sh[n].tobytes()]
        assert not bad, (tag, e, bad)


def set_actions(og, hg, acts):
    masks = action_masks(acts)
    og.set_action_masks(masks)
    hg.set_actions_batched(acts)


def policy(kind, seed, step, n):
    return sample_actions(seed, step, n) if kind == "random" else M.forward_actions(seed, step, n)


@pytest.mark.parametrize("A,seed", [(1, 3), (2, 14), (5, 15), (8, 92)])
def test_reset_parity(hip, A, seed):
    N = 24
    og, hg = make_pair(N, A, 32, 32, seed=seed, scenario="BoxAGone")
    same_state(og, hg, N, A, "reset")
    og.close(); hg.close()


@pytest.mark.parametrize("W,H", [(128, 72), (64, 64), (40, 24)])
def test_pixels_after_reset(hip, W, H):
    N, A = 12, 2
    og, hg = make_pair(N, A, W, H, seed=65, scenario="BoxAGone")
    fo, fh = frames(og, N, A), frames(hg, N, A)
    bad = [i for i in range(N * A) if not np.array_equal(fo[i], fh[i])]
    assert not bad, (bad, int((fo != fh).sum()))
    rgb = fo[..., :3].astype(np.int16)
    coloured = (rgb.max(axis=-1) - rgb.min(axis=-1)) > 20    # the room is white (grey when shaded): coloured pixels are platforms (or an agent)
    assert coloured.mean() > 0.05, coloured.mean()
    og.close(); hg.close()


@pytest.mark.parametrize("kind", ["random", "forward"])
@pytest.mark.parametrize("A", [1, 2, 4, 8])
def test_rollout_parity(hip, A, kind):
    """rewards, dones and true objectives of every env on every tick (the ending tick's included); the whole state and the BoxAGoneState record
    on every done and every 10 ticks; exact pixels every 20 ticks.  Episodes end when every agent is on the floor: resets happen all through the
    run, the ring of temporary platforms wraps, and temporary platforms grow and expire under agents (all asserted)"""
    N, T = 12, 600
    seed = A * 10 + (kind == "forward")
    og, hg = make_pair(N, A, 48, 27, seed=seed, scenario="BoxAGone")
    og.set_raster(True)   # the tiled raster: the brute-force image, byte for byte (tests/test_oracle_properties.py)
    resets = wraps = grow_under = expire_under = 0
    sts = [og.boxagone_state(e) for e in range(N)]
    for t in range(T):
        set_actions(og, hg, policy(kind, seed, t, N * A))
        render = t % 20 == 19
        if render:
            og.step(); hg.step()
            fo, fh = frames(og, N, A), frames(hg, N, A)
            assert np.array_equal(fo, fh), (t, int((fo != fh).any(axis=-1).sum()))
        else:
            og.step_norender(); hg.step_no_render()
        ro, rh = og.get_last_rewards(), hg.get_rewards_array()
        assert ro.tobytes() == rh.tobytes(), (t, ro, rh)
        do = og.get_dones().astype(bool)
        assert np.array_equal(do, hg.get_dones().astype(bool)), (t, do)
        to = np.array([og.true_objective(e, a) for e in range(N) for a in range(A)], np.float32)
        assert to.tobytes() == hg.get_true_objectives().tobytes(), (t, to, hg.get_true_objectives())
        resets += int(do.sum())
        if do.any() or t % 10 == 9:
            same_state(og, hg, N, A, t)
        for e in range(N):   # what happened, from the oracle's record (equal to the device's wherever compared)
            st, st0 = og.boxagone_state(e), sts[e]
            sts[e] = st
            if do[e]:
                continue
            wraps += int(st["takes"]) > 3 * A >= int(st0["takes"])
            s = og.snapshot(e)
            for i in range(A):
                p = int(st["last_platform"][i])
                if p < 0:
                    continue
                pl = st["plat"][p]
                on = M.agent_cell(s["agents"][i]["pos"]) == (int(pl["x"]), int(pl["y"]), int(pl["z"]))
                grow_under += on and 1 <= st["ticks"][p] <= 5 and M.on_ground(s["agents"][i])
                expire_under += on and st0["ticks"][p] == 1 and M.platform_status(st, p) == M.REMOVED
    assert resets > 0 and wraps > 0, (resets, wraps)
    if kind == "random":
        assert grow_under > 0 and expire_under > 0, (grow_under, expire_under)
    og.close(); hg.close()


def test_benchmark_shape(hip):
    """the benchmark's shape: 1024 envs x 1 agent at 128 x 128, the product's default path (device-drawn actions, fast pixels, one tick per
    call as mv_recommended_ticks_per_call says) beside a multi-threaded oracle for 300 ticks: rewards and dones of every env on every tick, the
    true objectives of the envs that finish, every env's state and BoxAGoneState record every 50 ticks, exact pixels of eight sampled envs then
    (and the fast mode within DESIGN.md's tolerance)"""
    N, A, W, H, T = 1024, 1, 128, 128, 300
    og = oracle_lib.OracleGym("BoxAGone", W, H, N, A, 16, False, {})
    hg = MegaverseGym("BoxAGone", W, H, N, A, 8, False, {})
    hg.set_pixel_mode("fast")
    assert hg.recommended_ticks_per_call() == 1
    og.seed(42); hg.seed(42)
    og.reset(); hg.reset()
    sample = [int(e) for e in np.linspace(0, N - 1, 8)]
    ndone = 0
    for st in range(T):
        og.set_action_masks(action_masks(sample_actions(1234, st, N * A)))
        og.step_norender()
        hg.sample_random_actions(1234, st); hg.step()
        do = og.get_dones().astype(bool)
        assert np.array_equal(do, hg.get_dones().astype(bool)), f"dones differ at tick {st}: envs {np.nonzero(do != hg.get_dones().astype(bool))[0][:8].tolist()}"
        ro, rh = og.get_last_rewards(), hg.get_rewards_array()
        assert np.array_equal(ro.view(np.uint32), rh.view(np.uint32)), f"rewards differ at tick {st}: agents {np.nonzero(ro.view(np.uint32) != rh.view(np.uint32))[0][:8].tolist()}"
        ndone += int(do.sum())
        for e in np.nonzero(do)[0]:
            assert og.true_objective(int(e), 0) == hg.true_objective(int(e), 0), (st, int(e))
        if st % 50 == 49:
            same_state(og, hg, N, A, st)
            hg.set_pixel_mode("exact"); hg.render()
            exact = {e: hg.get_observation(e, 0).copy() for e in sample}
            hg.set_pixel_mode("fast"); hg.render()
            ndiff = ngt1 = npx = 0
            for e in sample:
                og.render_env(e)
                ref = og.get_observation(e, 0)
                assert np.array_equal(ref, exact[e]), f"tick {st}: env {e}: exact pixels differ from the oracle"
                d = np.abs(ref.astype(np.int16) - hg.get_observation(e, 0).astype(np.int16)).max(axis=-1)
                ndiff += int((d > 0).sum()); ngt1 += int((d > 1).sum()); npx += d.size
            assert ngt1 <= max(2, 1e-4 * npx) and ndiff <= max(4, 5e-4 * npx), f"tick {st}: fast pixels: {ndiff} differ, {ngt1} by more than 1 of {npx}"
    assert ndone > N // 2, ndone
    og.close(); hg.close()
