"""The frame-order table of a batched call (megaverse_amd/csrc/mv_raster.hip: frame_order_ticks_kernel, GymView::lpt_forder): one small kernel behind the
call's step launches writes every tick's frames in the cost order of the fast pass and zeroes the tick's histogram; the passes read order[position] instead
of walking the histogram in every workgroup.  The order only schedules, so every byte a call produces must equal what a gym without the table
(MV_FRAME_ORDER=0 at mv_create: the in-kernel look-up) produces, and what single mv_step calls produce; a frame nobody drew would show (the ring is
pre-filled with 0x01, a drawn pixel's alpha is 255); a second and third call on the same gym show that the histograms were left clean and still rotate in
step with the hand-over slots.
The batched launch has no fine-grained tail (launch_raster_batch never sets tail_div, at any env count), and at 64 x 64 the single-tick launch has none
either (64 tiles per frame, it takes 128): the tail's position arithmetic meets the table in test_table_under_the_fine_grained_tail, 1024 frames of
128 x 128 drawn tick by tick behind a batched step launch -- the smallest frame count at which that launch cuts its tail finer."""
import numpy as np
import pytest

from megaverse_amd.extension import MegaverseGym

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

K, CALLS = 16, 3


def batched(monkeypatch, table, scenario, N, W, H):
    """CALLS calls of step_n(K) into a ring of K -> per call (observations, rewards, dones) of all K entries, and the launch counts"""
    import torch
    if table:
        monkeypatch.delenv("MV_FRAME_ORDER", raising=False)
    else:
        monkeypatch.setenv("MV_FRAME_ORDER", "0")
    obs = torch.full((K, N, H, W, 4), 1, dtype=torch.uint8, device="cuda:0")
    rew = torch.zeros((K, N), dtype=torch.float32, device="cuda:0")
    done = torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g = MegaverseGym(scenario, W, H, N, 1, 1, False, {})
    monkeypatch.delenv("MV_FRAME_ORDER", raising=False)   # (read at mv_create only)
    g.set_pixel_mode("fast")
    g.set_output_ring(K, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
    g.seed(31); g.reset()
    out = []
    for call in range(CALLS):
        obs.fill_(1); torch.cuda.synchronize()
        g.step_n(K, "multidiscrete", 7, K * call); g.synchronize()
        out.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
    counts = g.debug_launch_counts()
    arena = g.arena_bytes()
    g.close()
    return out, counts, arena


def single_steps(scenario, N, W, H):
    """the same ticks as CALLS x K single mv_step calls -> per tick (observations, rewards, dones)"""
    g = MegaverseGym(scenario, W, H, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(31); g.reset()
    out = []
    for st in range(CALLS * K):
        g.sample_random_actions(7, st); g.step()
        out.append((np.stack([g.get_observation(e, 0) for e in range(N)]), g.get_rewards_array(), g.get_dones()))
    g.close()
    return out


def check(got, ref, ticks, what):
    for call in range(CALLS):
        o, r, d = got[call]
        assert o[..., 3].min() == 255 and o[..., 3].max() == 255, f"{what} call {call}: a frame or pixel was not drawn"
        assert o[..., :3].max() > 0
        ro, rr, rd = ref[call]
        assert np.array_equal(o, ro), f"{what} call {call}: {int((o != ro).any(axis=-1).sum())} pixels differ from the gym without the table"
        assert np.array_equal(r.view(np.uint32), rr.view(np.uint32)) and np.array_equal(d, rd), f"{what} call {call}: rewards / dones differ"
        if ticks is None:
            continue
        for j in range(K):
            so, sr, sd = ticks[call * K + j]
            assert np.array_equal(o[j], so), f"{what} call {call} tick {j}: {int((o[j] != so).any(axis=-1).sum())} pixels differ from the single step's"
            assert np.array_equal(r[j].view(np.uint32), sr.view(np.uint32)) and np.array_equal(d[j], sd), f"{what} call {call} tick {j}: rewards / dones"


@pytest.mark.parametrize("N", [12, 64])   # (12: not a multiple of 8, the short last group of positions)
def test_tower_batched_calls_equal_the_in_kernel_lookup_and_single_steps(hip, monkeypatch, N):
    (got, gcounts, garena), (ref, rcounts, rarena) = batched(monkeypatch, True, "TowerBuilding", N, 64, 64), batched(monkeypatch, False, "TowerBuilding", N, 64, 64)
    assert list(gcounts) == list(rcounts) and gcounts[1] < CALLS * K   # (the batched path both ways: not one observation launch per tick)
    assert garena > rarena                                           # (the tables live in the gym's arena, one per hand-over slot)
    check(got, ref, single_steps("TowerBuilding", N, 64, 64), f"TowerBuilding {N} envs")


@pytest.mark.parametrize("scenario", ["ObstaclesEasy", "Collect"])   # (Collect: the long-list kernel shares the prologue and takes the table with it)
def test_other_scenarios_equal_the_in_kernel_lookup(hip, monkeypatch, scenario):
    got, _, _ = batched(monkeypatch, True, scenario, 32, 64, 64)
    ref, _, _ = batched(monkeypatch, False, scenario, 32, 64, 64)
    check(got, ref, None, f"{scenario} 32 envs")


def test_table_under_the_fine_grained_tail(hip, monkeypatch):
    """a batched step launch whose ticks are drawn tick by tick (no output ring: every tick into the one slab) -- the single-tick launch, which at 1024 frames
    of 128 x 128 cuts the cheapest eighth of the cost order finer (tail_div): its segment arithmetic must index the table as it indexed the histogram"""
    N, W, H = 1024, 128, 128

    def last(table):
        if not table:
            monkeypatch.setenv("MV_FRAME_ORDER", "0")
        g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
        monkeypatch.delenv("MV_FRAME_ORDER", raising=False)
        g.set_pixel_mode("fast"); g.seed(31); g.reset()
        for call in range(2):
            g.step_n(4, "multidiscrete", 7, 4 * call)
        g.synchronize()
        frames = np.stack([g.get_observation(e, 0) for e in range(0, N, 8)])
        sums = g.get_rewards_array().view(np.uint32).copy()
        g.close()
        return frames, sums

    (fa, ra), (fb, rb) = last(True), last(False)
    assert fa[..., 3].min() == 255 and fa[..., :3].max() > 0
    assert np.array_equal(fa, fb) and np.array_equal(ra, rb)
