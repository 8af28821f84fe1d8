"""What the observation pass takes from the host per launch (megaverse_amd/csrc/mv_raster.h: RasterConsts, raster_ray_table, raster_div_magic), without a
device: the constants and tables carry the bits of the single-precision expressions the kernels evaluated per workgroup before -- evaluated here in numpy
float32, one IEEE rounding per operation -- and the reciprocal form of the integer divisions is exact over the range the kernels meet."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from megaverse_amd import extension

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAN_HALF_FOV = F(1.19175359)                      # mv_frame.h
TAN_HALF_FOV_Y = F(1.19175359) / (F(128.0) / F(72.0))
TILE_W = 16
SIZES = [(128, 128), (64, 64), (128, 72), (100, 60)]


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def host_consts(W, H):
    lib = extension.load_library()
    consts, inv = np.zeros(4, np.float32), C.c_uint32(0)
    dcx, dcy = np.zeros(W, np.float32), np.zeros(H, np.float32)
    assert lib.mv_debug_raster_consts_host(W, H, consts.ctypes.data, C.addressof(inv), dcx.ctypes.data, dcy.ctypes.data) == 0
    return consts, inv.value, dcx, dcy


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_debug_raster_consts_host", 6), ("mv_debug_raster_div_host", 4)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert lib.mv_abi_version() == 2   # (additive)


@pytest.mark.parametrize("W,H", SIZES)
def test_affine_ray_constants_carry_the_kernel_expressions_bits(W, H):
    """sx = 2 TAN / W, ox = (1 / W - 1) TAN, and the same in y (the head of classify_tiles)"""
    consts, _, _, _ = host_consts(W, H)
    fw, fh = F(W), F(H)
    want = [F(2.0) * TAN_HALF_FOV / fw, (F(1.0) / fw - F(1.0)) * TAN_HALF_FOV,
            F(2.0) * TAN_HALF_FOV_Y / fh, (F(1.0) / fh - F(1.0)) * TAN_HALF_FOV_Y]
    assert all(type(w) is np.float32 for w in want)
    assert bits(consts).tolist() == bits(want).tolist()


@pytest.mark.parametrize("W,H", SIZES)
def test_ray_tables_carry_the_prologue_expressions_bits(W, H):
    """dcx[i] = (((i + .5) / W) 2 - 1) TAN, dcy[j] likewise with TAN_Y (fast_prologue)"""
    _, _, dcx, dcy = host_consts(W, H)
    i, j = np.arange(W).astype(np.float32), np.arange(H).astype(np.float32)
    wx = (((i + F(0.5)) / F(W)) * F(2.0) - F(1.0)) * TAN_HALF_FOV
    wy = (((j + F(0.5)) / F(H)) * F(2.0) - F(1.0)) * TAN_HALF_FOV_Y
    assert wx.dtype == np.float32 and wy.dtype == np.float32
    assert np.array_equal(bits(dcx), bits(wx)) and np.array_equal(bits(dcy), bits(wy))
    # (what the tables replace really varies: no two neighbours alike, antisymmetric about the frame's centre)
    assert np.all(np.diff(dcx) > 0) and np.all(np.diff(dcy) > 0)


@pytest.mark.parametrize("W,H", SIZES)
def test_tile_row_reciprocal_matches_the_size(W, H):
    _, inv, _, _ = host_consts(W, H)
    tiles_x = (W + TILE_W - 1) // TILE_W
    assert inv == (0 if tiles_x == 1 else (2 ** 32 + tiles_x - 1) // tiles_x)


def test_reciprocal_division_is_exact_over_the_kernels_range():
    """q == n // d for every tile index below 2^16 and every divisor 1..64"""
    lib = extension.load_library()
    n = np.arange(1 << 16, dtype=np.uint32)
    q = np.zeros(1 << 16, np.uint32)
    for d in range(1, 65):
        magic = C.c_uint32(0)
        assert lib.mv_debug_raster_div_host(d, n.size, C.addressof(magic), q.ctypes.data) == 0
        assert magic.value == (0 if d == 1 else (2 ** 32 + d - 1) // d)   # (0: d = 1 has no 32-bit reciprocal, n / 1 = n)
        assert np.array_equal(q, n // np.uint32(d)), f"divisor {d}"


def test_bad_sizes_are_refused():
    lib = extension.load_library()
    assert lib.mv_debug_raster_consts_host(0, 64, None, None, None, None) < 0
    assert lib.mv_debug_raster_consts_host(64, 1025, None, None, None, None) < 0
    assert lib.mv_debug_raster_div_host(0, 0, None, None) < 0
