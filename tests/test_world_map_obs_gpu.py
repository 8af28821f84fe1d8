"""World map observations on the GPU (include/megaverse_hip.h: mv_set_world_map_obs): one allocentric grid per agent, 3 planes of M x M int16, that every
drawn frame is merged into and that is cleared before the first frame of a new episode.  Every comparison is exact: the kernel alone against float64 numpy
(world_map_reference) on planes whose fragile pixels were zeroed, and the gym's grids against the rule's host twin folded over the gym's own planes, cameras
and dones."""
import numpy as np
import pytest

import episode_log_util as U
from megaverse_amd import MultiTaskGym
from megaverse_amd import extension as ext
from megaverse_amd.extension import MegaverseGym
from world_map_reference import CAM, CELL_SIZE, ORIGIN, safe_planes, world_map_numpy

pytestmark = pytest.mark.gpu

N, A, W, H, M, CELL, GYM_ORIGIN = 4, 2, 64, 64, 32, 1.0, (-16.0, -16.0)
# episodes of a few ticks: dones inside 24 ticks -- which the library steps one tick per call, however large k is.  Rearrange's 4.3 s are the shortest episodes
# (65 ticks) it still steps 8 ticks per call: their done falls inside the ninth step_n(8), whose frames read it from the tick's own slot
SHORT = {"TowerBuilding": {"episodeLengthSec": -190.0}, "HexMemory": {"episodeLengthSec": -8.0}, "Rearrange": {"episodeLengthSec": 4.3}}


def kernel(depth, seg, M, grid, clear=False):
    import torch
    g = torch.as_tensor(grid).cuda()
    ext.debug_world_map_device(torch.as_tensor(depth).cuda(), torch.as_tensor(seg.view(np.int16) if seg.dtype == np.uint16 else seg).cuda(),
                               torch.as_tensor(CAM).cuda(), M, CELL_SIZE[M], ORIGIN, g, clear)
    return g.cpu().numpy()


@pytest.mark.parametrize("M", (8, 64))
@pytest.mark.parametrize("w,h", ((40, 24), (41, 23)))
@pytest.mark.parametrize("instance", (False, True))
@pytest.mark.parametrize("depth_dtype", (np.float32, np.float16))
def test_kernel_equals_float64(depth_dtype, instance, w, h, M):
    """(41, 23): row tails and rows off the 16-byte grid; M = 8: many pixels share a cell.  Into a grid the reference made from another seed, and with clear = 1
    over that grid"""
    prev = safe_planes(w + M, w, h, depth_dtype, instance, M)
    depth, seg, cls = safe_planes(w + M + 1, w, h, depth_dtype, instance, M)
    old = world_map_numpy(prev[0], prev[2], CAM, M, CELL_SIZE[M], ORIGIN)[0]
    assert old[0].any()
    assert np.array_equal(kernel(depth, seg, M, old), world_map_numpy(depth, cls, CAM, M, CELL_SIZE[M], ORIGIN, old)[0])
    assert np.array_equal(kernel(depth, seg, M, old, clear=True), world_map_numpy(depth, cls, CAM, M, CELL_SIZE[M], ORIGIN)[0])


def test_kernel_saturates():
    """128 x 128 pixels into cells whose counts stand at 32760: the cells that get more than 7 pixels stop at 32767, their heights and classes still merge"""
    depth, seg, cls = safe_planes(9, 128, 128, np.float16, False, 8)
    old = world_map_numpy(depth[:64], cls[:64], CAM, 8, CELL_SIZE[8], ORIGIN)[0]
    old[0][old[0] > 0] = 32760
    want = world_map_numpy(depth, cls, CAM, 8, CELL_SIZE[8], ORIGIN, old)[0]
    assert np.array_equal(kernel(depth, seg, 8, old), want) and (want[0] == 32767).any()


def make_gym(scenario, mode, attach=True, params=None, ticks=24):
    """a reset gym with depth and labels attached, an action ring of random actions and (attach) world maps -> gym, depth, labels, grids"""
    import torch
    U.boxoban_env()
    g = MegaverseGym(scenario, W, H, N, A, 1, False, SHORT[scenario] if params is None else params)
    g.set_pixel_mode(mode)
    g.seed(42)
    g.reset()
    sizes = np.asarray(g.action_space_sizes())
    g.keep = torch.as_tensor(np.random.default_rng(3).integers(0, sizes, (ticks, N * A, sizes.size)).astype(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    g.set_action_ring(ticks, g.keep.data_ptr())
    d, s = g.set_depth_obs(True, "float16" if scenario == "TowerBuilding" else "float32"), g.set_seg_obs(True, "class" if scenario == "TowerBuilding" else "instance")
    m = g.set_world_map_obs(True, M, CELL, GYM_ORIGIN) if attach else None
    return g, d, s, m


def host(g, *tensors):
    import torch
    g.synchronize()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def fold(g, d, s, want, clear):
    """the host twin: the gym's current planes and cameras merged into want [N*A, 3, M, M]; clear [N]: those envs' grids are read as zeros"""
    dp, sp = host(g, d, s)
    for f in range(N * A):
        seg = sp[0, f].view(np.uint16) if sp.dtype == np.int16 else sp[0, f]
        want[f] = ext.debug_world_map_host(dp[0, f], seg, g.debug_map_camera(f // A, f % A), M, CELL, GYM_ORIGIN, want[f], clear=bool(clear[f // A]))
    return want


@pytest.mark.parametrize("mode", ("exact", "fast"))
@pytest.mark.parametrize("scenario,ticks", (("TowerBuilding", 24), ("HexMemory", 24), ("Rearrange", 72)))
def test_gym_grids_equal_the_host_twin_folded_over_the_gyms_own_frames(scenario, ticks, mode):
    g, d, s, m = make_gym(scenario, mode, ticks=ticks)
    assert tuple(m.shape) == (N * A, 3, M, M) and g._lib.mv_get_world_map_obs(g._g) == 1 and g._lib.mv_world_map_obs_cells(g._g) == M
    want = np.zeros((N * A, 3, M, M), np.int16)   # (attached behind the reset's frame: empty grids)
    dones = np.zeros(N, bool)
    for t in range(ticks):
        g.step_n(1, "sequence", 0, t)
        done = g.get_dones() != 0
        want, dones = fold(g, d, s, want, done), dones | done
        assert np.array_equal(host(g, m)[0], want), t
    assert dones.any() and want[:, 0].any()   # grids were cleared on the way
    assert np.array_equal(g.get_world_map_observation(N - 1, A - 1), want[-1])
    twin, _, _, tm = make_gym(scenario, mode, ticks=ticks)   # the batched call's per-slot done
    for c in range(ticks // 8):
        twin.step_n(8, "sequence", 0, 8 * c)
    assert np.array_equal(host(twin, tm)[0], want)
    for x in (g, twin):
        x.close()


def test_resets_and_a_callers_clear():
    import torch
    g, d, s, m = make_gym("TowerBuilding", "fast", params={})
    for t in range(3):
        g.step_n(1, "sequence", 0, t)
    before = host(g, m)[0]
    g.render()   # merges the same frames again: counts grow, nothing is cleared
    again = host(g, m)[0]
    assert (again[:, 0] >= before[:, 0]).all() and again[:, 0].sum() > before[:, 0].sum() and np.array_equal(again[:, 1:], before[:, 1:])
    g.reset_envs(torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device="cuda:0"))
    want = fold(g, d, s, again.copy(), [0, 1, 0, 1])
    assert np.array_equal(host(g, m)[0], want)
    m[:A].zero_()   # env 0's grids, cleared by the caller on the gym's stream (torch's current stream is the gym's here)
    want[:A] = 0
    g.step_n(1, "sequence", 0, 3)
    assert np.array_equal(host(g, m)[0], fold(g, d, s, want, g.get_dones()))
    g.reset()
    assert np.array_equal(host(g, m)[0], fold(g, d, s, want, np.ones(N)))
    g.close()


def test_refusals():
    import torch
    g, d, s, m = make_gym("TowerBuilding", "fast", params={})
    text = "world map observations are attached .mv_set_world_map_obs."
    for name, call in (("mv_step_no_render", g.step_no_render), ("mv_step_n_render", lambda: g.step_n(2, "sequence", 0, 0, render="last")),
                       ("mv_step_n_render", lambda: g.step_n(2, "sequence", 0, 0, render="none")),
                       ("mv_macro_step", lambda: g.macro_step(2, torch.zeros((N * A, 6), dtype=torch.int32, device="cuda:0"))),
                       ("mv_reset_envs_host", lambda: g.reset_envs(np.ones(N, np.uint8), render=False)),
                       ("mv_set_draw_mask_host", lambda: g.set_draw_mask(np.ones(N, np.uint8))),
                       ("mv_set_depth_obs", lambda: g.set_depth_obs(None)), ("mv_set_seg_obs", lambda: g.set_seg_obs(None))):
        with pytest.raises(RuntimeError, match=f"{name}.*{text}"):
            call()
    g.set_world_map_obs(None)
    assert g.world_map_obs() is None and g._lib.mv_get_world_map_obs(g._g) == 0
    g.set_draw_mask(np.ones(N, np.uint8))
    with pytest.raises(RuntimeError, match="mv_set_world_map_obs.*a draw mask attached .mv_set_draw_mask."):
        g.set_world_map_obs(True)
    g.set_draw_mask(None)
    g.set_map_obs(True)   # the two map streams attach independently
    g.set_world_map_obs(True, 8, 4.0)
    g.step_n(2, "sequence", 0, 0)
    for x in ("world_map", "map", "seg"):
        getattr(g, f"set_{x}_obs")(None)
    with pytest.raises(RuntimeError, match="mv_set_world_map_obs.*mv_set_seg_obs"):   # no label plane
        g.set_world_map_obs(True)
    g.close()
    mt = MultiTaskGym(["ObstaclesEasy", "ObstaclesHard"], 40, 24, 2, 1)
    with pytest.raises(RuntimeError, match="set_world_map_obs"):
        mt.set_world_map_obs(True)
    mt.close()


def test_one_launch_per_drawn_tick_and_nothing_without_it():
    g, d, s, _ = make_gym("TowerBuilding", "fast", params={})
    bare, bd, bs, _ = make_gym("TowerBuilding", "fast", attach=False, params={})
    before, bare_before = g.debug_launch_counts(), bare.debug_launch_counts()
    for x in (g, bare):
        x.step_n(4, "sequence", 0, 0)
        x.step_n(1, "sequence", 0, 4)
    after, bare_after = g.debug_launch_counts(), bare.debug_launch_counts()
    assert after[0] - before[0] == bare_after[0] - bare_before[0] and after[1] - before[1] == bare_after[1] - bare_before[1] + 5
    for a, b in zip(host(g, d, s), host(bare, bd, bs)):
        assert np.array_equal(a, b)
    assert all(np.array_equal(g.get_observation(e, a), bare.get_observation(e, a)) for e in range(N) for a in range(A))
    assert np.array_equal(g.get_rewards_array(), bare.get_rewards_array()) and np.array_equal(g.get_dones(), bare.get_dones())
    for x in (g, bare):
        x.close()
