"""Visible-entity observations on the GPU (include/megaverse_hip.h: mv_set_visible_obs): per drawn frame E rows of 5 int32 -- count and inclusive pixel bounds of
every entity row in the frame's instance label plane.  Every comparison is exact: the rows the kernel left against numpy (visible_reference: entity_row_of,
np.bincount, minima and maxima) applied to the label plane of the same ring entry, read back."""
import ctypes as C

import numpy as np
import pytest

import episode_log_util as U
from hip_util import hip_snapshot
from megaverse_amd.extension import MegaverseGym
from visible_reference import rows_numpy

pytestmark = pytest.mark.gpu

SCENARIOS = ("TowerBuilding", "ObstaclesHard", "Collect", "Sokoban", "HexMemory", "Football")
SENT = 0x5A5A5A5A


def make_gym(scenario, A, n, w, h, mode, ring=0):
    """a reset gym with an instance label plane and visible rows attached (behind output rings of `ring` entries) -> gym, labels, rows, what keeps the rings alive"""
    import torch
    U.boxoban_env()
    g = MegaverseGym(scenario, w, h, n, A, 1, False, {})
    g.set_pixel_mode(mode)
    g.seed(42)
    g.reset()
    rings = None
    if ring:
        rings = (torch.zeros((ring, n * A, h, w, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((ring, n * A), dtype=torch.float32, device="cuda:0"),
                 torch.zeros((ring, n), dtype=torch.uint8, device="cuda:0"))
        torch.cuda.synchronize()
        g.set_output_ring(ring, *(r.data_ptr() for r in rings))
    seg = g.set_seg_obs(True, "instance")
    vis = g.set_visible_obs(True)
    assert vis.dtype == torch.int32 and tuple(vis.shape) == (max(1, ring), n * A, g.entity_rows(), 5) and g._lib.mv_get_visible_obs(g._g) == max(1, ring)
    return g, seg, vis, rings


def host(g, *tensors):
    import torch
    g.synchronize()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def truth(g, scenario, A, planes):
    """numpy over the label planes [frames, h, w] of one entry -> [frames, E, 5]; Sokoban's goal cells and room width from the gym's snapshot"""
    out = []
    for f, words in enumerate(planes.view(np.uint16)):
        snap = hip_snapshot(g, f // A) if scenario == "Sokoban" else None
        out.append(rows_numpy(words, scenario, A, *((int(snap["W"]), snap["soko"]) if snap is not None else ())))
    return np.stack(out)


@pytest.mark.parametrize("mode", ("fast", "exact"))
@pytest.mark.parametrize("A", (1, 2))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_rollout_rows_equal_numpy_of_the_same_entry(scenario, A, mode):
    """4 envs at 64 x 36, 20 ticks of step_n(4, 'sequence') into rings of 4: every entry's rows are numpy's of that entry's label plane"""
    import torch
    n, k, ticks = 4, 4, 20
    g, seg, vis, rings = make_gym(scenario, A, n, 64, 36, mode, ring=k)
    sizes = np.asarray(g.action_space_sizes())
    script = torch.as_tensor(np.random.default_rng(3).integers(0, sizes, (ticks, n * A, sizes.size)).astype(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    g.set_action_ring(ticks, script.data_ptr())
    seen = 0
    for t0 in range(0, ticks, k):
        vis.fill_(SENT)
        torch.cuda.synchronize()
        g.step_n(k, "sequence", 0, t0)
        planes, rows = host(g, seg, vis)
        for j in range(k):
            assert np.array_equal(rows[j], truth(g, scenario, A, planes[j])), f"tick {t0 + j}"
        seen += int(rows[..., 0].sum())
    assert np.array_equal(g.get_visible_observation(n - 1, A - 1), rows[k - 1][n * A - 1])
    assert seen > 0 or scenario == "ObstaclesHard", "no entity came into any agent's view in 20 ticks"
    g.close()


@pytest.mark.parametrize("mode", ("fast", "exact"))
@pytest.mark.parametrize("w,h", ((40, 24), (41, 23)))
def test_row_tails_and_a_partly_filled_last_wave(w, h, mode):
    """40 x 24: 120 chunks of 8 words, the second wave 56 lanes full; 41 x 23: every row ends in a chunk of ONE word and starts off the 16-byte grid.
    step, then the frame behind render"""
    g, seg, vis, _ = make_gym("TowerBuilding", 2, 3, w, h, mode)
    for draw in (g.step, g.render):
        vis.fill_(SENT)
        draw()
        planes, rows = host(g, seg, vis)
        assert np.array_equal(rows[0], truth(g, "TowerBuilding", 2, planes[0])) and rows[0][..., 0].sum() > 0
    g.close()


def test_undrawn_frames_keep_their_bytes():
    g, seg, vis, _ = make_gym("TowerBuilding", 2, 4, 40, 24, "fast")
    g.step()
    vis.fill_(SENT)
    g.step_n(3, "multidiscrete", 1, 0, render="none")
    g.step_no_render()
    assert (host(g, vis)[0] == SENT).all()
    g.set_draw_mask(np.array([1, 0, 1, 0], np.uint8))
    g.step()
    rows = host(g, vis)[0][0].reshape(4, 2, -1)
    assert (rows[[1, 3]] == SENT).all() and not (rows[[0, 2]] == SENT).any()
    g.close()


def test_refusals():
    import torch
    U.boxoban_env()
    g = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    g.seed(1); g.reset()
    with pytest.raises(RuntimeError, match="mv_set_visible_obs.*mv_set_seg_obs"):   # no label plane
        g.set_visible_obs(True)
    g.set_seg_obs(True, "class")
    with pytest.raises(RuntimeError, match="mv_set_visible_obs.*instance-format.*mv_set_seg_obs"):   # not an instance plane
        g.set_visible_obs(True)
    g.set_seg_obs(None)
    g.set_seg_obs(True, "instance")
    g.set_visible_obs(True)
    for change in (lambda: g.set_seg_obs(None), lambda: g.set_seg_obs(True, "class")):
        with pytest.raises(RuntimeError, match="mv_set_seg_obs.*mv_set_visible_obs.*instance-format"):
            change()
    ring = torch.zeros((2, 4, 24, 40, 4), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="mv_set_output_ring.*visible-entity observations are attached .mv_set_visible_obs."):
        g.set_output_ring(2, ring.data_ptr())
    with pytest.raises(RuntimeError, match="mv_set_render_resolution.*mv_set_visible_obs"):
        g.set_render_resolution(64, 36)
    other = MegaverseGym("TowerBuilding", 40, 24, 4, 1, 1, False, {})
    other.seed(1); other.reset()
    lib, handles, out = g._lib, (C.c_void_p * 2)(g._g.value, other._g.value), C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1 and b"visible-entity observations attached (mv_set_visible_obs)" in lib.mv_last_error()
    g.set_visible_obs(None)
    g.set_seg_obs(None)   # (detached in this order, the label plane leaves again)
    assert lib.mv_group_create(handles, 2, C.byref(out)) == 0
    assert lib.mv_set_visible_obs(g._g, ring.data_ptr()) == -1 and b"mv_group" in lib.mv_last_error()
    lib.mv_group_destroy(out)
    g.close(); other.close()
