"""The world-map rule (megaverse_amd/csrc/mv_world_map_obs.h) in float64 numpy, for tests/test_world_map_obs.py and tests/test_world_map_obs_gpu.py, beside
map_reference.py, whose `camera` and `planes` it uses.

world_map_numpy(depth [h, w] float, cls [h, w] int, cam12, cells, cell_size, origin, grid=None) -> (int16 [3, M, M], fragile [h, w] bool): the frame merged
into `grid` (None: an empty one).  A pixel is fragile when (P.x - origin_x) inv, (P.z - origin_z) inv or 32 P.y lies within 1e-2 of an integer -- map_reference's
argument: the fp32 evaluation differs from this one by a few ulps of at most 4000, under 2e-3.  safe_depth zeroes the fragile pixels' depths (no hit) once,
before either side sees the plane."""
import numpy as np

from map_reference import HUD, TAN_X, TAN_Y, camera, planes  # noqa: F401

CAM = camera(-2.1, 0.4, eye=(1.3, 2.46, 3.7))
ORIGIN = (-64.0, -64.0)
CELL_SIZE = {8: 16.0, 64: 2.0}   # the grid spans 128 world units either way; the planes' depths reach 120, so part of every plane falls outside


def world_map_numpy(depth, cls, cam12, cells, cell_size, origin, grid=None):
    h, w = depth.shape
    M, t = int(cells), depth.astype(np.float64)
    cam = np.asarray(cam12, np.float32).astype(np.float64)
    x = (((np.arange(w) + 0.5) / w) * 2 - 1) * np.float64(np.float32(TAN_X))
    y = (((np.arange(h) + 0.5) / h) * 2 - 1) * np.float64(np.float32(TAN_Y))
    P = cam[:3, None, None] + np.einsum("kj,jhw->khw", cam[3:].reshape(3, 3), np.stack([x[None, :] * t, y[:, None] * t, -t]))
    inv = np.float64(np.float32(1.0) / np.float32(cell_size))   # (the rule's own factor: 1.0f / cell_size, formed once)
    q = np.stack([(P[0] - np.float64(np.float32(origin[0]))) * inv, (P[2] - np.float64(np.float32(origin[1]))) * inv, P[1] * 32])
    fragile = (np.abs(q - np.rint(q)) < 1e-2).any(0) & (t != 0)
    col, row = np.floor(q[0]).astype(np.int64), np.floor(q[1]).astype(np.int64)
    hq = np.clip(np.floor(q[2]), -32767, 32767).astype(np.int64)
    ok = (t != 0) & (cls != HUD) & (col >= 0) & (col < M) & (row >= 0) & (row < M)
    cell, key = (row * M + col)[ok], (((hq + 32768) << 4) | cls.astype(np.int64))[ok]
    old = np.zeros((3, M * M), np.int64) if grid is None else np.asarray(grid, np.int16).astype(np.int64).reshape(3, M * M)
    count = old[0] + np.bincount(cell, minlength=M * M)
    best = np.where(old[0] > 0, ((old[1] + 32768) << 4) | old[2], 0)   # (the buffer is the state: the key back from planes 1 and 2)
    np.maximum.at(best, cell, key)
    out = np.stack([np.minimum(count, 32767), np.where(count > 0, (best >> 4) - 32768, 0), np.where(count > 0, best & 15, 0)])
    return out.reshape(3, M, M).astype(np.int16), fragile


def safe_planes(seed, w, h, depth_dtype, instance, M):
    """map_reference's random planes with the fragile pixels' depths zeroed (at most 8 % of the plane: a condition, asserted) -> depth, seg, cls"""
    depth, seg, cls = planes(seed, w, h, depth_dtype, instance)
    fragile = world_map_numpy(depth, cls, CAM, M, CELL_SIZE[M], ORIGIN)[1]
    assert fragile.mean() <= 0.08
    return np.where(fragile, depth.dtype.type(0), depth), seg, cls
