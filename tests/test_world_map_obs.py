"""CPU: world map observations (mv_set_world_map_obs) without a device -- the rule's host twin mv_debug_world_map_host against float64 numpy
(world_map_reference) on random planes whose fragile pixels were zeroed first, byte for byte: a frame into an empty grid, a second frame into that result, a
frame with clear = 1 over it; counts at saturation; the new symbols; the Python check."""
import re

import numpy as np
import pytest

from megaverse_amd import extension as ext
from world_map_reference import CAM, CELL_SIZE, ORIGIN, safe_planes, world_map_numpy

NAMES = ("mv_set_world_map_obs", "mv_get_world_map_obs", "mv_world_map_obs_cells", "mv_get_world_map_observation", "mv_debug_world_map_host",
         "mv_debug_world_map_device")


@pytest.mark.parametrize("M", (8, 64))
@pytest.mark.parametrize("w,h", ((40, 24), (41, 23)))
@pytest.mark.parametrize("depth_dtype,instance", ((np.float32, False), (np.float16, True)))
def test_host_twin_equals_float64(depth_dtype, instance, w, h, M):
    a = safe_planes(w + M, w, h, depth_dtype, instance, M)
    b = safe_planes(w + M + 1, w, h, depth_dtype, instance, M)
    want1 = world_map_numpy(a[0], a[2], CAM, M, CELL_SIZE[M], ORIGIN)[0]
    got1 = ext.debug_world_map_host(a[0], a[1], CAM, M, CELL_SIZE[M], ORIGIN)
    assert got1.dtype == np.int16 and np.array_equal(got1, want1)
    # part of the plane lands in the grid and part of it is dropped
    assert w * h // 8 < want1[0].sum() < np.count_nonzero(a[0])
    want2 = world_map_numpy(b[0], b[2], CAM, M, CELL_SIZE[M], ORIGIN, want1)[0]
    assert np.array_equal(ext.debug_world_map_host(b[0], b[1], CAM, M, CELL_SIZE[M], ORIGIN, want1), want2) and want2[0].sum() > want1[0].sum()
    cleared = ext.debug_world_map_host(a[0], a[1], CAM, M, CELL_SIZE[M], ORIGIN, want2, clear=True)
    assert np.array_equal(cleared, want1)


def test_saturated_counts_stay():
    depth, seg, cls = safe_planes(5, 40, 24, np.float32, False, 8)
    old = world_map_numpy(depth, cls, CAM, 8, CELL_SIZE[8], ORIGIN)[0]
    old[0][old[0] > 0] = 32767
    got = ext.debug_world_map_host(depth, seg, CAM, 8, CELL_SIZE[8], ORIGIN, old)
    assert np.array_equal(got, world_map_numpy(depth, cls, CAM, 8, CELL_SIZE[8], ORIGIN, old)[0]) and got[0].max() == 32767 and np.array_equal(got[0], old[0])


def test_symbols_and_python_check():
    header = open(ext.__file__.replace("extension.py", "../include/megaverse_hip.h")).read()
    lib, bound = ext.load_library(), {s[0] for s in ext.SYMBOLS}
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header) and name in bound and hasattr(lib, name), name
    assert ext.OBS_STREAMS["world_map"].setter == "mv_set_world_map_obs"
    with pytest.raises(ValueError, match=r"set_world_map_obs: the buffer must be a contiguous int16 CUDA tensor of shape \(8, 3, 64, 64\) on device 0"):
        ext.check_world_map_obs(np.zeros((8, 3, 32, 64), np.int16), 8, 64, 0)
