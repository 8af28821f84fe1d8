"""Scan observations on the GPU (include/megaverse_hip.h: mv_set_scan_obs): per drawn frame 3 planes of K int16 -- range, class, count of the frame's pixels
binned into a fan of beams.  Every comparison is exact: the kernel alone against float64 numpy (scan_reference) on planes whose fragile pixels were zeroed, and
the gym's fans against the rule's host twin fed with the gym's own planes and camera."""
import ctypes as C

import numpy as np
import pytest

import episode_log_util as U
from megaverse_amd import MultiTaskGym
from megaverse_amd import extension as ext
from megaverse_amd.extension import MegaverseGym
from scan_reference import BEAMS, CAMERAS, case, planes

pytestmark = pytest.mark.gpu

BAND = ext.SCAN_DEFAULT_BAND


def device(a):
    import torch
    return torch.as_tensor(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("K", BEAMS)
@pytest.mark.parametrize("w,h", ((40, 24), (41, 23), (128, 128)))
@pytest.mark.parametrize("instance", (False, True))
@pytest.mark.parametrize("depth_dtype", (np.float32, np.float16))
def test_kernel_equals_float64(depth_dtype, instance, w, h, K, cam):
    """(40, 24), (41, 23): C = 5 and 6 chunks per row, 256 % C != 0, and 41's short last chunk and rows off the 16-byte grid; (128, 128): C = 16, every lane
    with a strip of its own; 'down': the beams drift over the columns, accumulators flush in mid-column"""
    if K == 2 * w and cam != "down":
        # (an unpitched camera and two beams per column: s * bscale is an odd integer at EVERY pixel centre, so float64 cannot say which side of the beam
        # boundary the fp32 evaluation rounds to and every hit would be fragile.  The host twin -- the same fp32 operations -- is the judge of these cells)
        cam12, band = CAMERAS[cam]
        depth, seg, _ = planes(w * K, w, h, depth_dtype, instance)
        want = ext.debug_scan_host(depth, seg, cam12, K, *band)
    else:
        seg, depth, zeroed, want, cam12, band = case(w, h, depth_dtype, instance, K, cam)
        assert zeroed <= 0.10
    got =ext.debug_scan_device(device(depth), device(seg), device(cam12), K, *band)
    assert np.array_equal(got.cpu().numpy(), want) and want[2].any()


def make_gym(scenario, mode, K=64, ring=0, n=4, A=2, w=64, h=64, depth="float16", seg="class", ticks=16):
    """a reset gym with depth, labels and scans attached behind output rings of `ring` entries, and an action ring of random actions"""
    import torch
    U.boxoban_env()
    g = MegaverseGym(scenario, w, h, n, A, 1, False, {})
    g.set_pixel_mode(mode)
    g.seed(42)
    g.reset()
    g.keep =[torch.zeros((ring, n * A, h, w, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((ring, n * A), dtype=torch.float32, device="cuda:0"),
              torch.zeros((ring, n), dtype=torch.uint8, device="cuda:0")] if ring else []
    sizes = np.asarray(g.action_space_sizes())
    g.keep.append(torch.as_tensor(np.random.default_rng(3).integers(0, sizes, (ticks, n * A, sizes.size)).astype(np.int32)).to("cuda:0"))
    torch.cuda.synchronize()
    if ring:
        g.set_output_ring(ring, *(r.data_ptr() for r in g.keep[:3]))
    g.set_action_ring(ticks, g.keep[-1].data_ptr())
    return g, g.set_depth_obs(True, depth), g.set_seg_obs(True, seg), g.set_scan_obs(True, K)


def host(g, *tensors):
    import torch
    g.synchronize()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("ring", (0, 4))
@pytest.mark.parametrize("mode", ("exact", "fast"))
@pytest.mark.parametrize("scenario,depth,seg", (("TowerBuilding", "float16", "class"), ("HexMemory", "float32", "instance")))
def test_gym_fans_equal_the_host_twin_on_the_gyms_own_planes(scenario, depth, seg, mode, ring):
    """after reset and over twelve ticks, four of them one step_n batch: every frame's fan is the host twin's on the planes and the camera of that frame"""
    import torch
    g, d, s, m = make_gym(scenario, mode, ring=ring, depth=depth, seg=seg)
    assert m.dtype == torch.int16 and tuple(m.shape) == (max(1, ring), 8, 3, 64) and g._lib.mv_get_scan_obs(g._g) == max(1, ring)
    assert g._lib.mv_scan_obs_beams(g._g) == 64
    seen, classes = 0, set()

    def check(entry):
        nonlocal seen
        dp, sp, mp = host(g, d, s, m)
        for f in range(8):
            cam = g.debug_map_camera(f // 2, f % 2)
            labels = sp[entry, f].view(np.uint16) if seg == "instance" else sp[entry, f]
            assert np.array_equal(mp[entry, f], ext.debug_scan_host(dp[entry, f], labels, cam, 64, *BAND)), (entry, f)
        seen += int((mp[entry, :, 0] >= 0).sum())
        classes.update(np.unique(mp[entry, :, 1]).tolist())

    last = lambda: (max(1, g._ring_ticks) - 1) % max(1, ring)   # (the entry the last tick went to)
    g.reset()
    check(last())
    for t in range(8):
        g.step_n(1, "sequence", 0, t)
        check(last())
    g.step_n(4, "sequence", 0, 8)   # (a ring of 4: an entry per tick; without one the one entry holds the last tick's)
    check(last())
    assert seen > 0 and classes - {0, 1}   # (some beam is hit, and by more than floor)
    assert np.array_equal(g.get_scan_observation(3, 1), host(g, m)[0][last(), 7]) and np.array_equal(g.scan_obs().cpu().numpy(), host(g, m)[0][last()])
    launches = []
    for attached in (True, False):   # (one launch per drawn tick, counted with the call's pass launches; the second call after a detach: steady again)
        g.step_n(1, "sequence", 0, 12)
        before = g.debug_launch_counts()[1]
        g.step_n(1, "sequence", 0, 13)
        launches.append(g.debug_launch_counts()[1] - before)
        g.set_scan_obs(None)
    assert launches[0] - launches[1] == 1
    g.close()


def test_refusals_and_detach():
    import torch
    U.boxoban_env()
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(1); g.reset()
    with pytest.raises(RuntimeError, match="mv_set_scan_obs.*mv_set_depth_obs"):   # no depth plane
        g.set_scan_obs(True)
    g.set_depth_obs(True)
    with pytest.raises(RuntimeError, match="mv_set_scan_obs.*mv_set_seg_obs"):   # no label plane
        g.set_scan_obs(True)
    g.set_seg_obs(True)
    for bad in ({"beams": 12}, {"beams": 0}, {"beams": 264}, {"band": (1.0, 1.0)}, {"band": (0.0, float("inf"))}):
        with pytest.raises(ValueError, match="set_scan_obs"):
            g.set_scan_obs(True, **bad)
    assert g._lib.mv_set_scan_obs(g._g, 16, 12, -1.0, 1.0) == -1 and b"multiple of 8 in [8, 256]" in g._lib.mv_last_error()
    assert g._lib.mv_set_scan_obs(g._g, 16, 8, 1.0, -1.0) == -1 and b"h_lo < h_hi" in g._lib.mv_last_error()
    assert tuple(g.set_scan_obs(True, 8).shape) == (1, 4, 3, 8)
    for change in (lambda: g.set_depth_obs(None), lambda: g.set_depth_obs(True, "float16"), lambda: g.set_seg_obs(None), lambda: g.set_seg_obs(True, "instance")):
        with pytest.raises(RuntimeError, match="mv_set_(depth|seg)_obs.*mv_set_scan_obs"):
            change()
    ring = torch.zeros((2, 4, 24, 40, 4), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="mv_set_output_ring.*scan observations are attached .mv_set_scan_obs."):
        g.set_output_ring(2, ring.data_ptr())
    with pytest.raises(RuntimeError, match="mv_set_render_resolution.*mv_set_scan_obs"):
        g.set_render_resolution(64, 36)
    with pytest.raises(RuntimeError, match="mv_set_still_frames.*mv_set_scan_obs"):
        g.set_still_frames(True)
    other = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    other.seed(2); other.reset()
    handles, out, lib = (C.c_void_p * 2)(g._g.value, other._g.value), C.c_void_p(), g._lib
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1
    assert lib.mv_last_error().decode() == "mv_group_create: a gym has scan observations attached (mv_set_scan_obs): the union launches write none; detach them first"
    assert lib.mv_step_many(handles, 2, 1, 1, 0, 0) == -1
    assert lib.mv_last_error().decode() == "mv_step_many: gym 0 has scan observations attached (mv_set_scan_obs): step it on its own, or detach them first"
    g.draw_hires()   # ignores the option
    other.close()
    g.set_scan_obs(None)
    assert g.scan_obs() is None and g._lib.mv_get_scan_obs(g._g) == 0 and g._lib.mv_scan_obs_beams(g._g) == 0
    assert tuple(g.set_scan_obs(True, 256, (-2.0, 2.0)).shape) == (1, 4, 3, 256)   # another K
    g.step()
    assert (host(g, g.scan_obs())[0][:, 2] > 0).any()
    for x in ("scan", "seg", "depth"):   # (detached in this order, the planes leave again)
        getattr(g, f"set_{x}_obs")(None)
    g.close()
    mt = MultiTaskGym(["ObstaclesEasy", "ObstaclesHard"], 40, 24, 2, 1)
    with pytest.raises(RuntimeError, match="set_scan_obs"):
        mt.set_scan_obs(True)
    mt.close()
