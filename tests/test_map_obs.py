"""CPU: map observations (mv_set_map_obs) without a device -- the rule's host twin mv_debug_map_host against float64 numpy (map_reference) on random planes
whose fragile pixels were zeroed first, byte for byte; the tie rules on hand-made planes; the hook's refusals; the Python tables."""
import numpy as np
import pytest

import megaverse_amd
from megaverse_amd import extension as ext
from map_reference import camera, map_numpy, planes, safe_depth

CAMERAS = {"level": camera(0.7, 0.0), "up": camera(-2.1, 0.4), "down": camera(3.9, -0.6)}
CELL_SIZE = {8: 16.0, 64: 2.0}   # the grid spans 128 world units either way: the planes' depths reach 120
LEVEL = camera(0.0, 0.0)


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("M", (8, 64))
@pytest.mark.parametrize("w,h", ((40, 24), (41, 23)))
@pytest.mark.parametrize("instance", (False, True))
@pytest.mark.parametrize("depth_dtype", (np.float32, np.float16))
def test_host_twin_equals_float64(depth_dtype, instance, w, h, M, cam):
    depth, seg, cls = planes(w * M + len(cam), w, h, depth_dtype, instance)
    depth, zeroed = safe_depth(depth, cls, CAMERAS[cam], M, CELL_SIZE[M])
    assert zeroed < 0.10
    want, fragile = map_numpy(depth, cls, CAMERAS[cam], M, CELL_SIZE[M])
    assert not fragile.any()
    got = ext.debug_map_host(depth, seg, CAMERAS[cam], M, CELL_SIZE[M])
    assert got.dtype == np.int16 and np.array_equal(got, want) and want[0].sum() > w * h // 4


def test_tie_rules():
    """a level camera, every depth 6.  2 x 2 pixels into cells of 4 units: u = -+3.57 -> columns 3 and 4 of row 1; the bottom pixels are counted at
    floor(32 * -2.01) = -65, the top ones are HUD and are not; every other cell is three zeros.  1 x 4 pixels into cells of 64 units: two pixels of equal
    height 0 per cell, the greater class wins"""
    got = ext.debug_map_host(np.full((2, 2), 6.0, np.float32), np.array([[3, 9], [14, 14]], np.uint8), LEVEL, 8, 4.0)
    assert got[:, 1, 3].tolist() == [1, -65, 3] and got[:, 1, 4].tolist() == [1, -65, 9] and got[0].sum() == 2
    got[:, 1, 3:5] = 0
    assert not got.any()
    same = ext.debug_map_host(np.full((1, 4), 6.0, np.float32), np.array([[5, 9, 7, 2]], np.uint8), LEVEL, 8, 64.0)
    assert same[:, 0, 3].tolist() == [2, 0, 9] and same[:, 0, 4].tolist() == [2, 0, 7] and same[0].sum() == 4


def test_count_saturates():
    """256 x 256 pixels of one depth into cells of 512 units: every pixel right of the axis shares one cell, 32768 > 32767 of them"""
    got = ext.debug_map_host(np.full((256, 256), 6.0, np.float16), np.full((256, 256), 4 << 12 | 77, np.uint16), LEVEL, 8, 512.0)
    assert got[0, 0, 4] == 32767 and got[0, 0, 3] == 32767 and got[2, 0, 4] == 4 and got[0].sum() == 2 * 32767


@pytest.mark.parametrize("bad", ({"cells": 12}, {"cells": 0}, {"cells": 72}, {"cell_size": 0.0}, {"cell_size": -1.0}, {"cell_size": float("inf")},
                                 {"cell_size": float("nan")}, {"depth_format": 2}, {"seg_format": 2}))
def test_the_hook_refuses_and_writes_nothing(bad):
    lib = ext.load_library()
    depth, seg, cam, out = np.ones((4, 8), np.float32), np.ones((4, 8), np.uint8), LEVEL, np.full((3, 72, 72), 0x5A5A, np.int16)
    a = {"cells": 8, "cell_size": 1.0, "depth_format": 0, "seg_format": 0, **bad}
    assert lib.mv_debug_map_host(depth.ctypes.data, a["depth_format"], seg.ctypes.data, a["seg_format"], 8, 4, cam.ctypes.data, a["cells"], a["cell_size"],
                                 out.ctypes.data) == -1
    assert b"mv_debug_map_host" in lib.mv_last_error() and (out == 0x5A5A).all()
    for null in range(4):
        ptrs = [depth.ctypes.data, seg.ctypes.data, cam.ctypes.data, out.ctypes.data]
        ptrs[null] = None
        assert lib.mv_debug_map_host(ptrs[0], 0, ptrs[1], 0, 8, 4, ptrs[2], 8, 1.0, ptrs[3]) == -1 and (out == 0x5A5A).all()


def test_python_tables():
    assert "map" in ext.OBS_STREAMS and ext.OBS_STREAMS["map"].setter == "mv_set_map_obs"
    assert megaverse_amd.MAP_OBS_FIELDS == ("count", "height", "class") and megaverse_amd.MAP_HEIGHT_UNIT == 1 / 32
