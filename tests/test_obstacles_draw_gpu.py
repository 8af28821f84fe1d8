"""The Obstacles family's and Empty's episodes drawn ON THE DEVICE (megaverse_amd/csrc/mv_obstacles_draw.h, obstacles_draw_kernel): the kernel against the host
generator, record by record, and a gym whose feeder runs in device mode (MV_OBSTACLES_DEVICE_GEN=1) against the oracle and against a host-fed twin -- the same
tests the host-fed gym passes: resets, rollouts with natural auto-resets, forced resets and a re-seed in mid-run, batched calls with the host far ahead, masked
resets with level seeds, a group of four scenarios."""
import numpy as np
import pytest

from hip_util import diff_snapshots, hip_snapshot, make_pair, set_same_actions
from megaverse_amd import extension as ext
from test_host_generators import EPISODE_BLOB, generate
from test_obstacles_draw import CLASH_SEEDS, assert_same_episode, draw_stats

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# env seeds whose first ObstaclesHard episode turns left AND right (found on the CPU, test_obstacles_draw.py's hook: the widest grids), beside the clash seeds
TWO_TURN_SEEDS = [0, 3, 4, 5]


def draw_device(name, agents, seeds, n, base_len=60.0):
    lib = ext.load_library()
    seeds = np.asarray(seeds, np.int32)
    out = np.zeros(len(seeds), EPISODE_BLOB)
    ms = np.zeros(1, np.float32)
    rc = lib.mv_debug_obstacles_draw_device(0, name.encode(), agents, seeds.ctypes.data, len(seeds), n, base_len, out.ctypes.data, out.nbytes, ms.ctypes.data)
    assert rc == 0, ext.last_error() if hasattr(ext, "last_error") else rc
    return out, float(ms[0])


def test_the_seed_set_holds_what_it_is_chosen_for():
    for s in CLASH_SEEDS:
        assert draw_stats("ObstaclesHard", 1, s, 1)[0][0] > 1, s
    for s in TWO_TURN_SEEDS:
        host = draw_stats("ObstaclesHard", 1, s, 1)[0]
        assert host[1] > 0 and host[2] > 0, (s, host)


@pytest.mark.parametrize("name,agents,n", [("ObstaclesHard", 1, 1), ("ObstaclesHard", 8, 3), ("ObstaclesEasy", 2, 2), ("ObstaclesSteps", 1, 2), ("ObstaclesLava", 4, 1),
                                           ("Empty", 3, 2)])
def test_kernel_draws_the_host_generators_episodes(hip, name, agents, n):
    rng = np.random.default_rng(99 + agents)
    fixed = [0, 1, 42, (1 << 30) - 1] + CLASH_SEEDS + TWO_TURN_SEEDS[1:]
    seeds = fixed + [int(s) for s in rng.integers(0, 1 << 30, 256 - len(fixed))]
    assert len(seeds) == 256
    got, ms = draw_device(name, agents, seeds, n)
    print(f"obstacles_draw_kernel {name}: {len(seeds)} episodes per launch, {ms:.2f} ms per launch")
    for i, s in enumerate(seeds):
        assert got[i]["seq"] == n, (s, got[i]["seq"])
        assert_same_episode(got[i], generate(name, agents, s, n), agents, (name, s, n))


def test_a_full_batch_of_episodes_in_one_launch(hip):
    # 1024 envs' worth in one launch (what a forced reset asks for; the waves draw four episodes each): the rate, and a sample of the records
    seeds = np.arange(1024, dtype=np.int32) * 7919 + 13
    got, ms = draw_device("ObstaclesHard", 1, seeds, 2)
    print(f"obstacles_draw_kernel ObstaclesHard: 1024 episodes per launch, {ms:.2f} ms per launch = {1024 / ms:.0f} k episodes/s")
    for i in range(0, 1024, 37):
        assert got[i]["seq"] == 2
        assert_same_episode(got[i], generate("ObstaclesHard", 1, int(seeds[i]), 2), 1, int(seeds[i]))


@pytest.fixture
def device_gen(monkeypatch):
    monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", "1")


@pytest.mark.parametrize("name", ["ObstaclesHard", "ObstaclesEasy"])
@pytest.mark.parametrize("A,seed", [(1, 3), (5, 15)])
def test_gym_reset_parity(hip, device_gen, name, A, seed):
    N = 32
    og, hg = make_pair(N, A, 32, 32, seed=seed, scenario=name)
    assert hg.device_generator() and hg.host_generator_threads() == 0
    for e in range(N):
        d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
        assert not d, (e, d[:5])
    assert np.array_equal(og.get_observation(3, 0), hg.get_observation(3, 0))
    og.close(); hg.close()


@pytest.mark.parametrize("name,steps", [("ObstaclesHard", (4600, 5600, 100)), ("ObstaclesEasy", (1300, 1800, 100))])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_gym_rollouts_with_auto_resets(hip, device_gen, name, steps, case):
    """Rollouts against the oracle at episodeLengthSec 6.0, -24.0 and -500.0 with Collect's floors on the number of episodes the envs go through: 10, 15, 900.

    In the Obstacles family episodeLengthSec is only a FLOOR of the episode length: an episode lasts max(episodeLengthSec, 35 s per platform + 1 s per movable
    box) (mv_gen_obstacles.cpp, scenario_obstacles.cpp), 525 ticks at the very least, whatever the parameter -- no value of it makes an env consume an episode
    per tick, as -500.0 does in Collect.  The first two floors are met by rolling out long enough for natural auto-resets (ObstaclesHard's first episode ends
    after 1155 ticks).  What Collect's third case is there for -- the device feeder asked for an episode per env on every tick, some 900 device-drawn episodes
    checked against the oracle -- natural resets cannot give here (900 of them are 90 000 ticks of ObstaclesEasy, 450 000 of ObstaclesHard), so the -500.0 case
    ends every env's episode itself: one tick, then a reset of all ten envs, a hundred times, every env's new episode compared with the oracle's each time.  The
    floor stays 900: episodes the envs finished or abandoned, every one replaced by a device-drawn one."""
    base, min_done = ((6.0, 10), (-24.0, 15), (-500.0, 900))[case]
    every_tick = case == 2
    N, A = 10, 2
    og, hg = make_pair(N, A, 32, 32, seed=6, params={"episodeLengthSec": base}, scenario=name)
    ndone, checked = 0, 0
    for st in range(steps[case]):
        set_same_actions(og, hg, N, A, 77, st)
        og.step_norender(); hg.step_no_render()
        do = np.array([og.is_done(e) for e in range(N)])
        assert np.array_equal(do, hg.get_dones().astype(bool)), st
        ndone += int(do.sum())
        assert np.array_equal(og.get_last_rewards().view(np.uint32), hg.get_rewards_array().view(np.uint32)), st
        if every_tick:
            og.reset(); hg.reset()
            ndone += N - int(do.sum())   # (an env that finished on this very tick is counted once)
        if every_tick or st % 250 == 0 or st == steps[case] - 1 or (do.any() and checked < 40):   # (the ticks behind a reset: the new episode as the device drew it)
            checked += int(do.any())
            for e in range(N):
                d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
                assert not d, (st, e, d[:5])
    og.render(); hg.render()
    for e in range(0, N, 3):
        assert np.array_equal(og.get_observation(e, 0), hg.get_observation(e, 0)), e
    print(f"{name} episodeLengthSec {base}: {ndone} episodes ended in {steps[case]} ticks")
    assert ndone >= min_done, ndone
    og.close(); hg.close()


@pytest.mark.parametrize("name", ["ObstaclesHard", "ObstaclesEasy"])
def test_gym_forced_resets_and_reseed(hip, device_gen, name):
    N, A = 8, 2
    og, hg = make_pair(N, A, 32, 32, seed=9, scenario=name)
    for rd in range(5):
        for st in range(3):
            set_same_actions(og, hg, N, A, 3, 10 * rd + st)
            og.step_norender(); hg.step_no_render()
        og.reset(); hg.reset()
        if rd == 2:
            og.seed(1234); hg.seed(1234)
            og.reset(); hg.reset()
        for e in range(N):
            assert not diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A), (rd, e)
    og.close(); hg.close()


def test_empty_against_the_oracle(hip, device_gen):
    N, A = 8, 3
    og, hg = make_pair(N, A, 32, 32, seed=21, scenario="Empty")
    assert hg.device_generator() and hg.host_generator_threads() == 0
    for st in range(50):
        set_same_actions(og, hg, N, A, 5, st)
        og.step_norender(); hg.step_no_render()
        assert np.array_equal(og.get_last_rewards().view(np.uint32), hg.get_rewards_array().view(np.uint32)), st
        if st in (17, 33):
            og.reset(); hg.reset()
        if st % 8 == 0 or st in (17, 33, 49):
            for e in range(N):
                d = diff_snapshots(og.snapshot(e), hip_snapshot(hg, e), A)
                assert not d, (st, e, d[:5])
    og.render(); hg.render()
    assert np.array_equal(og.get_observation(2, 1), hg.get_observation(2, 1))
    og.close(); hg.close()


@pytest.mark.parametrize("name", ["ObstaclesHard", "ObstaclesEasy"])
def test_batched_calls_equal_the_host_fed_gym(hip, monkeypatch, recwarn, name):
    """The bench's launch shape (calls of 16 ticks into a ring of 32, open loop, the host far ahead), 1600 ticks -- every ObstaclesEasy env past its first
    auto-reset, many past their second; ObstaclesHard's shortest episodes (1050 ticks) over too: the device-fed gym never starves, hits no capacity, and ends in the very state and pixels the host-fed gym ends in."""
    import torch
    from megaverse_amd.extension import MegaverseGym
    N, A, W, H, k, ticks = 64, 1, 32, 32, 16, 1600

    def run(device):
        monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", "1" if device else "0")
        g = MegaverseGym(name, W, H, N, A, 8, False, {})
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


def test_level_seeds_and_masked_resets_equal_the_host_fed_gym(hip, monkeypatch):
    """seed_envs (host form) + reset_envs (host form) of a third of the envs in mid-run: the named envs restart from their new streams, the others go on."""
    import torch
    from megaverse_amd.extension import MegaverseGym
    N, A, W, H, k = 48, 2, 32, 32, 8
    third = list(range(1, N, 3))

    def run(device):
        monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", "1" if device else "0")
        g = MegaverseGym("ObstaclesHard", W, H, N, A, 4, False, {})
        assert g.device_generator() == device
        g.set_pixel_mode("fast")
        ring = torch.zeros((2 * k, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0")
        g.set_output_ring(2 * k, ring.data_ptr())
        g.seed(5); g.reset()
        st, mids = 0, []
        for rd in range(3):
            for _ in range(6):
                g.step_n(k, "multidiscrete", 13, st); st += k
            g.seed_envs({e: 7000 + 31 * e + rd for e in third})
            mask = np.zeros(N, bool); mask[third] = True
            g.reset_envs(mask)
            g.synchronize()
            mids.append([hip_snapshot(g, e).copy() for e in range(N)])
        for _ in range(6):
            g.step_n(k, "multidiscrete", 13, st); st += k
        g.synchronize(); torch.cuda.synchronize()
        snaps = [hip_snapshot(g, e).copy() for e in range(N)]
        last = ring[(st - 1) % (2 * k)].cpu().numpy().copy()
        g.close()
        return mids + [snaps], last

    a, b = run(True), run(False)
    for rd, (sa, sb) in enumerate(zip(a[0], b[0])):
        for e in range(N):
            d = diff_snapshots(sa[e], sb[e], A)
            assert not d, (rd, e, d[:4])
    assert np.array_equal(a[1], b[1])


def test_a_group_with_device_fed_obstacles_gyms_equals_the_host_fed_group(hip, monkeypatch):
    """TowerBuilding, ObstaclesHard, Collect and ObstaclesEasy in one mv_group (union launches, one simulation stream for all members), 40 single steps and 48
    batched calls: device-drawn against host-generated Obstacles episodes -- every env's state, rewards, dones and pixels; who draws what, per member."""
    import torch
    from megaverse_amd.multitask import MultiTaskGym
    names, N, A, W, H = ["TowerBuilding", "ObstaclesHard", "Collect", "ObstaclesEasy"], 32, 1, 32, 32

    def run(device):
        monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", "1" if device else "0")
        monkeypatch.setenv("MV_COLLECT_DEVICE_GEN", "0")
        mt = MultiTaskGym(names, W, H, N, A, 2, {"episodeLengthSec": 3.0})
        mt.set_pixel_mode("fast")
        obs = mt.attach("cuda:0")
        mt.seed(11); mt.reset()
        assert mt.device_generator() == [True, device, False, device]
        assert [g.host_generator_threads() == 0 for g in mt.gyms] == [True, device, False, device]
        st = 0
        for _ in range(40):
            mt.sample_random_actions(9, st); mt.step(); st += 1
        for k in (8, 8, 5, 8) * 12:
            mt.step_n(k, "multidiscrete", 9, st); st += k
        mt.synchronize(); torch.cuda.synchronize()
        out = ([g.debug_snapshot_bytes(j).tobytes() for g in mt.gyms for j in range(N // len(names))], [g.get_rewards_array().tobytes() for g in mt.gyms],
               [g.get_dones().tobytes() for g in mt.gyms], obs.cpu().numpy().copy())
        mt.close()
        return out

    a, b = run(True), run(False)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and a[3][..., :3].max() > 0


def test_device_generator_query(hip, monkeypatch):
    from megaverse_amd.extension import MegaverseGym
    monkeypatch.delenv("MV_OBSTACLES_DEVICE_GEN", raising=False)
    for name, switch, want in (("TowerBuilding", None, True), ("ObstaclesEasy", None, False), ("ObstaclesEasy", "0", False), ("ObstaclesEasy", "1", True),
                               ("Empty", "1", True)):
        if switch is None:
            monkeypatch.delenv("MV_OBSTACLES_DEVICE_GEN", raising=False)
        else:
            monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", switch)
        g = MegaverseGym(name, 32, 32, 4, 1, 2, False, {})
        assert g.device_generator() is want, (name, switch)
        assert (g.host_generator_threads() == 0) is want, (name, switch, g.host_generator_threads())
        arena = g.arena_bytes()
        g.reset()
        g.close()
        if name == "ObstaclesEasy":   # the draw kernel's grid regions are the gym's and are counted: 4 envs, 4 regions of two bit planes
            grid = 4 * 2 * ((152 * 152 * 37 + 31) // 32) * 4
            if want:
                device_arena = arena
            else:
                host_arena = arena
    assert device_arena - host_arena == grid, (device_arena, host_arena, grid)
    assert ext.load_library().mv_device_generator(None) == -1


def test_parameters_beyond_the_device_generators_capacities_are_refused(hip, monkeypatch):
    """The obstacles* float parameters can ask for more than the device generator's fixed arrays hold (40 platforms in a row: test_capacity_flags_gpu.py's
    level): with the switch set mv_create says so, with it unset the gym is host-fed as ever."""
    from megaverse_amd.extension import MegaverseGym
    params = {"obstaclesMinNumPlatforms": 40.0, "obstaclesMaxNumPlatforms": 40.0}
    monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", "1")
    with pytest.raises(RuntimeError, match="MV_OBSTACLES_DEVICE_GEN"):
        MegaverseGym("ObstaclesHard", 32, 32, 8, 1, 2, False, params)
    monkeypatch.setenv("MV_OBSTACLES_DEVICE_GEN", "0")
    g = MegaverseGym("ObstaclesHard", 32, 32, 8, 1, 2, False, params)
    assert not g.device_generator() and g.host_generator_threads() > 0
    g.close()
