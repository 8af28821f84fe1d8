"""HexMemory's and HexExplore's episodes drawn ON THE DEVICE (megaverse_amd/csrc/mv_hex_draw.h, hex_draw_kernel): the kernel against the host generator, record
by record, and a gym whose feeder runs in device mode (MV_HEX_DEVICE_GEN=1) against the oracle and against a host-fed twin -- resets, rollouts with natural
auto-resets, forced resets and a re-seed in mid-run, batched calls with the host far ahead, the switch."""
import numpy as np
import pytest

from draw_util import draw_device
from hip_util import diff_snapshots, hip_snapshot, make_pair, set_same_actions
from test_hex_draw import NAMES, assert_same_episode
from test_host_generators import generate

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


@pytest.fixture(scope="module")
def seeds():
    return [0, 1, 42, (1 << 30) - 1] + [int(s) for s in np.random.default_rng(77).integers(0, 1 << 30, 252)]


@pytest.fixture
def device_gen(monkeypatch):
    monkeypatch.setenv("MV_HEX_DEVICE_GEN", "1")


def same_state(og, hg, N, A, tag):
    for e in range(N):
        d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
        assert not d, (tag, e, d[:5])


@pytest.mark.parametrize("agents,n", [(1, 1), (4, 2), (8, 3)])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_draws_the_host_generators_episodes(hip, seeds, name, agents, n):
    got, ms = draw_device(name, agents, seeds, n)
    print(f"hex_draw_kernel {name}: {len(seeds)} episodes per launch, {ms:.2f} ms per launch")
    for i, s in enumerate(seeds):
        assert got[i]["seq"] == n, (s, got[i]["seq"])
        assert_same_episode(got[i], generate(name, agents, s, n), agents, (name, s, n))


@pytest.mark.parametrize("A,seed", [(1, 3), (3, 15)])
@pytest.mark.parametrize("name", NAMES)
def test_gym_reset_parity(hip, device_gen, name, A, seed):
    N = 16
    og, hg = make_pair(N, A, 32, 32, seed=seed, scenario=name)
    assert hg.device_generator() and hg.host_generator_threads() == 0
    same_state(og, hg, N, A, "reset")
    assert np.array_equal(og.get_observation(3, 0), hg.get_observation(3, 0))
    og.close(); hg.close()


@pytest.mark.parametrize("name,base", [("HexExplore", 2.0), ("HexMemory", -5.0)])
def test_gym_rollout_with_auto_resets_forced_resets_and_a_reseed(hip, device_gen, name, base):
    """300 ticks against the oracle: HexExplore's episodes last 30 ticks, HexMemory's 3 s per good object less 5 s (the smallest mazes' end inside the run: three
    of them on the oracle), so envs auto-reset on their own; two forced resets and a seed in mid-run.  Rewards and dones every tick, the state on the ticks behind a reset."""
    N, A = 8, 2
    og, hg = make_pair(N, A, 32, 32, seed=6, params={"episodeLengthSec": base}, scenario=name)
    resets = 0
    for st in range(300):
        set_same_actions(og, hg, N, A, 77, st)
        og.step_norender(); hg.step_no_render()
        assert og.get_last_rewards().tobytes() == hg.get_rewards_array().tobytes(), st
        do = np.array([og.is_done(e) for e in range(N)])
        assert np.array_equal(do, hg.get_dones().astype(bool)), st
        resets += int(do.sum())
        if st in (100, 200):
            if st == 200:
                og.seed(1234); hg.seed(1234)
            og.reset(); hg.reset()
        if do.any() or st % 50 == 0:
            same_state(og, hg, N, A, st)
    assert resets > 0, resets
    og.close(); hg.close()


def test_batched_calls_equal_the_host_fed_gym(hip, monkeypatch, recwarn):
    """step_n(8) into a ring of 16, open loop, 320 ticks of short HexMemory episodes: the device-fed gym never starves, hits no capacity, and ends in the
    very state and pixels the host-fed gym ends in."""
    import torch
    from megaverse_amd.extension import MegaverseGym
    N, A, W, H, k, ticks = 32, 1, 32, 32, 8, 320

    def run(device):
        monkeypatch.setenv("MV_HEX_DEVICE_GEN", "1" if device else "0")
        g = MegaverseGym("HexMemory", W, H, N, A, 8, False, {"episodeLengthSec": -5.0})
        assert g.device_generator() == device and (g.host_generator_threads() == 0) == device
        g.set_pixel_mode("fast")
        ring = torch.zeros((2 * k, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0")
        g.set_output_ring(2 * k, ring.data_ptr())
        g.seed(9); g.reset()
        for st in range(0, ticks, k):
            g.step_n(k, "multidiscrete", 31, st)
        g.synchronize(); torch.cuda.synchronize()
        snaps = [hip_snapshot(g, e).copy() for e in range(N)]
        last = ring[(ticks - 1) % (2 * k)].cpu().numpy().copy()
        g.close()
        return snaps, last

    a = run(True)
    assert not [w for w in recwarn.list if "capacity" in str(w.message) or "resident" in str(w.message)], [str(w.message) for w in recwarn.list]
    b = run(False)
    for e in range(N):
        d = diff_snapshots(a[0][e], b[0][e], A)
        assert not d, (e, d[:4])
    assert np.array_equal(a[1], b[1]) and a[1][..., :3].max() > 0


def test_switch_matrix(hip, monkeypatch):
    from megaverse_amd.extension import MegaverseGym
    for name, hex_switch, obstacles_switch, want in (("HexMemory", None, None, False), ("HexMemory", "0", None, False), ("HexMemory", "1", None, True),
                                                     ("HexExplore", None, "1", False), ("ObstaclesEasy", "1", None, False)):
        for var, value in (("MV_HEX_DEVICE_GEN", hex_switch), ("MV_OBSTACLES_DEVICE_GEN", obstacles_switch)):
            if value is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, value)
        g = MegaverseGym(name, 32, 32, 4, 1, 2, False, {})
        assert g.device_generator() is want, (name, hex_switch, obstacles_switch)
        assert (g.host_generator_threads() == 0) is want, (name, hex_switch, obstacles_switch)
        g.reset()
        g.close()
