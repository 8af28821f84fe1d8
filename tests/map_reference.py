"""The map-observation rule (megaverse_amd/csrc/mv_map_obs.h) in float64 numpy, for tests/test_map_obs.py and tests/test_map_obs_gpu.py.

map_numpy(depth [h, w] float, cls [h, w] int, cam12, cells, cell_size) -> (int16 [3, M, M], fragile [h, w] bool).  A pixel is fragile when u / cell_size,
f / cell_size or 32 hgt lies within 1e-2 of an integer: the fp32 evaluation differs from this one by a few ulps of at most 120 * 32 = 3840, under 2e-3, so a
pixel that is not fragile falls in the same cell with the same height on both sides.  safe_depth zeroes the fragile pixels' depths (no hit) once."""
import numpy as np

TAN_X, TAN_Y, HUD = 1.19175359, 1.19175359 / (128.0 / 72.0), 14


def map_numpy(depth, cls, cam12, cells, cell_size):
    h, w = depth.shape
    M, t = int(cells), depth.astype(np.float64)
    c = np.asarray(cam12, np.float32).astype(np.float64)[3:].reshape(3, 3)
    x = (((np.arange(w) + 0.5) / w) * 2 - 1) * np.float64(np.float32(TAN_X))
    y = (((np.arange(h) + 0.5) / h) * 2 - 1) * np.float64(np.float32(TAN_Y))
    d = np.einsum("kj,jhw->khw", c, np.stack([x[None, :] * t, y[:, None] * t, -t]))
    R = c[:, 0]
    inv = np.float64(np.float32(1.0) / np.float32(cell_size))   # (the rule's own factor: 1.0f / cell_size, formed once)
    q = np.stack([(d[0] * R[0] + d[2] * R[2]) * inv, (d[0] * R[2] - d[2] * R[0]) * inv, d[1] * 32])
    fragile = (np.abs(q - np.rint(q)) < 1e-2).any(0) & (t != 0)
    col, row = np.floor(q[0]).astype(np.int64) + M // 2, np.floor(q[1]).astype(np.int64)
    hq = np.clip(np.floor(q[2]), -32767, 32767).astype(np.int64)
    ok = (t != 0) & (cls != HUD) & (col >= 0) & (col < M) & (row >= 0) & (row < M)
    cell, key = (row * M + col)[ok], (((hq + 32768) << 4) | cls.astype(np.int64))[ok]
    count, best = np.bincount(cell, minlength=M * M), np.zeros(M * M, np.int64)
    np.maximum.at(best, cell, key)
    out = np.stack([np.minimum(count, 32767), np.where(count > 0, (best >> 4) - 32768, 0), np.where(count > 0, best & 15, 0)])
    return out.reshape(3, M, M).astype(np.int16), fragile


def safe_depth(depth, cls, cam12, cells, cell_size):
    """depth with its fragile pixels zeroed -> (depth, the share of pixels zeroed)"""
    fragile = map_numpy(depth, cls, cam12, cells, cell_size)[1]
    return np.where(fragile, depth.dtype.type(0), depth), float(fragile.mean())


def camera(yaw, pitch, eye=(1.0, 2.0, 3.0)):
    """eye(3) c(9) of a camera without roll: columns right / up / back, yaw about y and pitch about the right axis (radians)"""
    right = np.array([np.cos(yaw), 0.0, -np.sin(yaw)])
    back = np.array([np.sin(yaw) * np.cos(pitch), -np.sin(pitch), np.cos(yaw) * np.cos(pitch)])
    return np.concatenate([eye, np.stack([right, np.cross(back, right), back], 1).ravel()]).astype(np.float32)


def planes(seed, w, h, depth_dtype, instance):
    """random planes: depths in [0.01, 120] with three zeros in ten, classes in [0, 15) (HUD among them), instance words where asked.  (A level camera makes
    the middle row and column of an odd-sized plane fragile as a whole, hgt = 0 and u = 0: with the generic 6 % that is 13 % of the hits, 9 % of the pixels)"""
    rng = np.random.default_rng(seed)
    depth = np.where(rng.random((h, w)) < 0.3, 0.0, rng.uniform(0.01, 120.0, (h, w))).astype(depth_dtype)
    cls = rng.integers(0, 15, (h, w))
    seg = (cls << 12 | rng.integers(0, 4096, (h, w))).astype(np.uint16) if instance else cls.astype(np.uint8)
    return depth, seg, cls
