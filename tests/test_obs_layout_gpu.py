"""GPU: the planar observation layout (include/megaverse_hip.h: mv_set_obs_layout, MV_OBS_RGB_PLANAR) -- frames [3][h][w] written by the observation
pass itself -- against the default RGBA slab: byte for byte rgba[..., :3].permute(0, 3, 1, 2), in every scenario, pixel mode, size, launch shape and
group form, and against the CPU oracle; the surfaces that hand frames out keep their contracts."""
import os

import numpy as np
import pytest

import oracle_lib
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.megaverse_env import SUPPORTED_SCENARIOS, MegaverseEnv
from megaverse_amd.multitask import MEGAVERSE8, MultiTaskGym
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = pytest.mark.gpu
BOXOBAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban")


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)   # Sokoban: synthetic Boxoban-format levels


def _gym(scenario, N, A, W, H, layout, mode, seed=42):
    """a gym in `layout` rendering into a torch slab of its own; -> (gym, slab)"""
    import torch
    g = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    g.set_pixel_mode(mode)
    if layout == "chw":
        g.set_obs_layout("chw")
    shape = (N * A, 3, H, W) if layout == "chw" else (N * A, H, W, 4)
    slab = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
    g.set_obs_buffer(slab.data_ptr())
    g.seed(seed)
    g.reset()
    return g, slab


def _pair(scenario, N, A, W, H, mode, seed=42):
    a, sa = _gym(scenario, N, A, W, H, "rgba", mode, seed)
    b, sb = _gym(scenario, N, A, W, H, "chw", mode, seed)
    assert b.obs_layout() == "chw" and a.obs_layout() == "rgba"
    return a, sa, b, sb


def _same_frames(rgba, chw, tag):
    import torch
    torch.cuda.synchronize()
    want = rgba[..., :3].permute(0, 3, 1, 2)
    assert tuple(chw.shape) == tuple(want.shape), tag
    if not torch.equal(want, chw):
        bad = (want != chw).any(dim=1)
        raise AssertionError(f"{tag}: {int(bad.sum())} pixels differ (first frame {int(bad.flatten(1).any(1).nonzero()[0])})")
    assert int(rgba[..., 3].min()) == 255, tag


def _same_outputs(a, b, tag):
    a.synchronize(); b.synchronize()
    assert a.get_rewards_array().tobytes() == b.get_rewards_array().tobytes(), tag
    assert np.array_equal(a.get_dones(), b.get_dones()), tag
    assert a.get_true_objectives().tobytes() == b.get_true_objectives().tobytes(), tag


def _tick(gyms, N, A, seed, st):
    acts = sample_actions(seed, st, N * A)
    for g in gyms:
        g.set_actions_batched(acts)
        g.step()


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("scenario", SUPPORTED_SCENARIOS)
def test_every_scenario_planar_equals_rgba(hip, scenario, mode):
    """two gyms with equal seeds and actions, one RGBA, one planar: after reset and after 40 random ticks the planar slab is the RGBA one's
    channels, byte for byte, and rewards, dones and true objectives are equal"""
    N, A, W, H = 4, 2, 128, 72
    a, sa, b, sb = _pair(scenario, N, A, W, H, mode)
    _same_frames(sa, sb, f"{scenario} {mode}: reset")
    for st in range(40):
        _tick((a, b), N, A, 77, st)
    _same_frames(sa, sb, f"{scenario} {mode}: 40 ticks")
    _same_outputs(a, b, f"{scenario} {mode}")
    assert int(sb.max()) > 0
    a.close(); b.close()


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("W,H", [(128, 128), (64, 64), (128, 72), (72, 40), (100, 60), (67, 41), (30, 17)])
@pytest.mark.parametrize("scenario", ["TowerBuilding", "Collect", "HexMemory"])
def test_sizes(hip, scenario, W, H, A):
    """two pixels per lane (128 x 128), one (64 x 64), 128 x 72; rows of whole dwords but not whole tiles (72 x 40, 100 x 60: the quads' dword stores in
    the partial edge tiles, clear_tile's pixel-by-pixel path); rows of neither (W % 4 != 0: byte stores) -- fast pixels, tick by tick and multi-tick
    calls without rings (one pass per tick; the one-launch passes of a call: test_batched_passes_into_rings)"""
    N = 4
    a, sa, b, sb = _pair(scenario, N, A, W, H, "fast")
    _same_frames(sa, sb, f"{scenario} {W}x{H} A={A}: reset")
    for st in range(12):
        _tick((a, b), N, A, 5, st)
    _same_frames(sa, sb, f"{scenario} {W}x{H} A={A}: ticks")
    for g in (a, b):
        g.step_n(4, "multidiscrete", 5, 12)
    _same_frames(sa, sb, f"{scenario} {W}x{H} A={A}: step_n")
    _same_outputs(a, b, f"{scenario} {W}x{H} A={A}")
    a.close(); b.close()


@pytest.mark.parametrize("W,H", [(64, 64), (128, 128)])
@pytest.mark.parametrize("scenario", ["Collect", "HexMemory", "Rearrange", "TowerBuilding"])
def test_batched_passes_into_rings(hip, scenario, W, H):
    """step_n into output rings at least a call deep: the k passes of a call are ONE launch (raster_glist_batch_kernel for Collect / Hex, the scaled-shape
    raster_fast_batch_kernel for Rearrange; one pixel per lane at 64 x 64, two at 128 x 128) -- every ring entry of the planar gym is the RGBA gym's"""
    import torch
    N, A, K = 8, 1, 8   # (one agent per env: the one-launch step a batched pass goes with, mv_api_step.hip)
    a, sa, b, sb = _pair(scenario, N, A, W, H, "fast", seed=13)
    rings = []
    for g, shape in ((a, (K, N * A, H, W, 4)), (b, (K, N * A, 3, H, W))):
        obs = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
        rew = torch.zeros((K, N * A), dtype=torch.float32, device="cuda:0")
        don = torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        g.set_output_ring(K, obs.data_ptr(), rew.data_ptr(), don.data_ptr())
        rings.append((obs, rew, don))
    st = 0
    for k in (K, 3, K):
        for g in (a, b):
            g.step_n(k, "multidiscrete", 21, st)
        st += k
        a.synchronize(); b.synchronize(); torch.cuda.synchronize()
        (oa, ra, da), (ob, rb, db) = rings
        for e in range(K):
            _same_frames(oa[e], ob[e], f"{scenario} {W}x{H}: ring entry {e} after a call of {k}")
        assert torch.equal(ra, rb) and torch.equal(da, db)
    assert int(rings[1][0].max()) > 0
    a.close(); b.close()


def test_group_at_a_size_of_unaligned_frames(hip, monkeypatch):
    """a MultiTaskGym slab of 20 x 17 planar frames: the sub-gyms' slices start at byte offsets that are multiples of 3 * 20 * 17 (no alignment needed:
    byte stores) -- planar equals RGBA"""
    monkeypatch.setenv("MV_MULTITASK_UNION", "1")
    scen = ["TowerBuilding", "Collect", "ObstaclesEasy"]
    mts = []
    for layout in ("rgba", "chw"):
        mt = MultiTaskGym(scen, 20, 17, 3, 1, 2, obs_layout=layout)
        mt.set_pixel_mode("fast")
        obs = mt.attach("cuda:0")
        mt.seed(2); mt.reset()
        mts.append((mt, obs))
    (a, oa), (b, ob) = mts
    for st in range(10):
        for g in (a, b):
            g.sample_random_actions(4, st); g.step()
    a.synchronize(); b.synchronize()
    _same_frames(oa, ob, "20 x 17 group")
    a.close(); b.close()


@pytest.mark.parametrize("pipelined,overlap", [(True, False), (False, False), (True, True)])
def test_bench_shape_rings(hip, pipelined, overlap):
    """the benchmark's shape: TowerBuilding, 1024 envs, 128 x 128, step_n(16) into output rings of 16 (one launch for the 16 passes); pipelining on
    and off; overlapped passes with rings two calls deep -- every ring entry of the planar gym is the RGBA gym's channels"""
    import torch
    N, A, W, H, K = 1024, 1, 128, 128, 16
    R = 2 * K if overlap else K
    a, sa, b, sb = _pair("TowerBuilding", N, A, W, H, "fast", seed=3)
    rings = []
    for g, shape in ((a, (R, N * A, H, W, 4)), (b, (R, N * A, 3, H, W))):
        g.set_pipelining(pipelined)
        obs = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
        rew = torch.zeros((R, N * A), dtype=torch.float32, device="cuda:0")
        don = torch.zeros((R, N), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        g.set_output_ring(R, obs.data_ptr(), rew.data_ptr(), don.data_ptr())
        if overlap:
            g.set_pass_overlap(True)
        rings.append((obs, rew, don))
    st = 0
    for _ in range(3 if overlap else 2):
        for g in (a, b):
            g.step_n(K, "multidiscrete", 11, st)
        st += K
    a.synchronize(); b.synchronize(); torch.cuda.synchronize()
    (oa, ra, da), (ob, rb, db) = rings
    for e in range(R):
        _same_frames(oa[e], ob[e], f"ring entry {e}")
    assert torch.equal(ra, rb) and torch.equal(da, db)
    assert int(ob.max()) > 0
    a.close(); b.close()


@pytest.mark.parametrize("scenarios", [MEGAVERSE8, ["TowerBuilding", "ObstaclesEasy", "Sokoban", "Rearrange"], ["Collect", "HexMemory", "HexExplore"]],
                         ids=["megaverse8", "short-lists", "long-lists"])
@pytest.mark.parametrize("W,H", [(64, 64), (128, 72)])
def test_groups(hip, monkeypatch, scenarios, W, H):
    """MultiTaskGym planar against RGBA: tick by tick (both list lengths: the union-all launch; one length: the union launches) and batched group calls
    into rings of 8 (the one-launch group pass)"""
    import torch
    monkeypatch.setenv("MV_MULTITASK_UNION", "1")
    S = len(scenarios)
    N, A = 4 * S, 1

    def make(layout):
        mt = MultiTaskGym(scenarios, W, H, N, A, 2, obs_layout=layout)
        mt.set_pixel_mode("fast")
        obs = mt.attach("cuda:0")
        mt.seed(5); mt.reset()
        return mt, obs

    a, oa = make("rgba")
    b, ob = make("chw")
    assert a.union and b.union and tuple(ob.shape) == (N * A, 3, H, W)

    def same(tag):
        a.synchronize(); b.synchronize()
        _same_frames(oa, ob, tag)
        for k in range(S):
            assert a.gyms[k].get_rewards_array().tobytes() == b.gyms[k].get_rewards_array().tobytes(), (tag, k)
            assert np.array_equal(a.gyms[k].get_dones(), b.gyms[k].get_dones()), (tag, k)

    same("reset")
    st = 0
    for _ in range(20):
        for g in (a, b):
            g.sample_random_actions(9, st); g.step()
        st += 1
    same("single ticks")
    ra, _, _ = a.set_output_ring(8)
    rb, _, _ = b.set_output_ring(8)
    assert tuple(rb[0].shape) == (8, N // S * A, 3, H, W)
    for k in (8, 5, 8):
        for g in (a, b):
            g.step_n(k, "multidiscrete", 9, st)
        st += k
    a.synchronize(); b.synchronize(); torch.cuda.synchronize()
    for q in range(S):
        for e in range(8):
            _same_frames(ra[q][e], rb[q][e], f"ring {scenarios[q]} entry {e}")
    a.close(); b.close()


@pytest.mark.parametrize("scenario,W,H", [("TowerBuilding", 128, 72), ("Collect", 64, 64), ("HexMemory", 64, 36)])
def test_planar_frames_equal_the_oracle(hip, scenario, W, H):
    """exact pixels: the planar frames are the CPU oracle's frames, transposed"""
    N, A = 4, 2
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, None)
    og.seed(42)
    og.reset()
    hg, slab = _gym(scenario, N, A, W, H, "chw", "exact")

    def same(tag):
        hg.synchronize()
        got = slab.cpu().numpy()
        for e in range(N):
            for a in range(A):
                want = og.get_observation(e, a)[..., :3].transpose(2, 0, 1)
                assert np.array_equal(got[e * A + a], want), (tag, e, a)

    same("reset")
    for st in range(20):
        acts = sample_actions(1234, st, N * A)
        masks = action_masks(acts)
        for e in range(N):
            for a in range(A):
                og.set_action_mask(e, a, int(masks[e * A + a]))
        hg.set_actions_batched(acts)
        og.step()
        hg.step()
    same("20 ticks")
    og.close(); hg.close()


def test_surfaces(hip):
    """get_observation is (h, w, 4) RGBA in both layouts; MegaverseEnv.step lists and step_device agree, the planar tensors are contiguous; the
    hires frames are RGBA and unchanged"""
    import torch
    N, A, W, H = 4, 2, 128, 72
    ea = MegaverseEnv("TowerBuilding", N, A, img_w=W, img_h=H)
    eb = MegaverseEnv("TowerBuilding", N, A, img_w=W, img_h=H, obs_layout="chw")
    for e in (ea, eb):
        e.env.set_pixel_mode("fast")
        e.seed(7)
    la, lb = ea.reset(), eb.reset()
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    for st in range(6):
        acts = sample_actions(3, st, N * A)
        oa, raw, da, _ = ea.step(acts)
        ob, rbw, db, _ = eb.step(acts)
        assert all(x.shape == (3, H, W) and np.array_equal(x, y) for x, y in zip(oa, ob))
        assert np.array_equal(raw, rbw) and da == db
    for e in range(N):
        for a in range(A):
            x, y = ea.env.get_observation(e, a), eb.env.get_observation(e, a)
            assert x.shape == y.shape == (H, W, 4) and np.array_equal(x, y) and int(y[..., 3].min()) == 255
    ta, tb = ea.observations_tensor(), eb.observations_tensor()
    assert tb.is_contiguous() and not ta.is_contiguous() and torch.equal(ta, tb)
    with pytest.raises(ValueError):
        eb.observations_tensor(rgba=True)
    for st in range(6, 10):
        acts = torch.from_numpy(sample_actions(3, st, N * A)).to("cuda:0")
        oa, ra, da = ea.step_device(acts)
        ob, rb, db = eb.step_device(acts)
        assert ob.is_contiguous() and tuple(ob.shape) == (N * A, 3, H, W)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
    for e in (ea, eb):
        e.env.set_render_resolution(96, 64)
        e.env.draw_hires()
    for e in range(N):
        for a in range(A):
            x, y = ea.env.get_hires_observation(e, a), eb.env.get_hires_observation(e, a)
            assert y.shape == (64, 96, 4) and np.array_equal(x, y)
    ea.close(); eb.close()


def test_errors(hip):
    """late call (after reset, an output ring, an obs buffer), bad value, grouped gym, mixed-layout group"""
    from megaverse_amd.extension import GymGroup
    g = MegaverseGym("TowerBuilding", 64, 64, 2, 1, 1, False, {})
    with pytest.raises(RuntimeError, match="mv_set_obs_layout"):
        g.set_obs_layout(2)
    with pytest.raises(ValueError, match="'rgba' and 'chw'"):
        g.set_obs_layout("hwc")
    g.set_obs_layout("chw")
    g.set_obs_layout("rgba")
    g.set_obs_layout("chw")
    g.reset()
    with pytest.raises(RuntimeError, match="before the gym's first"):
        g.set_obs_layout("rgba")
    assert g.obs_layout() == "chw"
    for late in ("set_output_ring", "set_obs_buffer"):
        h = MegaverseGym("TowerBuilding", 64, 64, 2, 1, 1, False, {})
        if late == "set_output_ring":
            h.set_output_ring(0)
        else:
            h.set_obs_buffer(0)
        with pytest.raises(RuntimeError, match="before the gym's first"):
            h.set_obs_layout("chw")
        h.close()
    x = MegaverseGym("TowerBuilding", 64, 64, 2, 1, 1, False, {})
    y = MegaverseGym("Collect", 64, 64, 2, 1, 1, False, {})
    y.set_obs_layout("chw")
    with pytest.raises(RuntimeError, match="layout"):
        GymGroup([x, y])
    z = MegaverseGym("Collect", 64, 64, 2, 1, 1, False, {})
    grp = GymGroup([x, z])
    with pytest.raises(RuntimeError, match="group"):
        z.set_obs_layout("chw")
    grp.close()
    for q in (g, x, y, z):
        q.close()
