"""Stored outputs of the reference's own helpers (oracle/_ref: util.hpp, math_utils.hpp, string_utils.cpp, perlin_noise.hpp and the maze
library, compiled in place from the reference tree) for fixed inputs: tests/golden/ref_vectors.npz, written by
tests/golden/make_ref_vectors.py.  The oracle is pinned against these vectors on every checkout; where oracle/_ref is built the tests
also recompute them with the live libraries and require the very same bytes."""
import ctypes as C
import os

import numpy as np

import oracle_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "ref_vectors.npz")

RAND_RANGE_SEEDS = [0, 1, 42, 12345, 2**31 - 1, 4294967295]
FRAND_SEEDS = [0, 7, 42, 99999]
FRAND_N = 20000
ENV_SEEDS_N = 64
TRIANGULAR_N = 40
PERLIN_CASES = [(0, 1), (1, 3), (123456789, 9), (999999999, 5), (4294967295, 2)]
MAZE_SIZES = [2, 3, 5, 8, 10]
MAZE_SEEDS = (0, 1, 12345, 2 ** 31 + 7)
SPLIT_TEXTS = ["; 0\n##########\n#  @ $ . #\n##########\n\n; 1\n####\n#@$.#\n", "\n\n\nabc\n\n\ndef\n", "no newline at all", "", "\n", "a\r\nb\r\n",
               "; 3\n" + "#" * 40 + "\n" * 7 + "tail"]
SPLIT_CAP = 4096


def rand_range_inputs(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    lo = rng.integers(-50, 50, n).astype(np.int32)
    hi = (lo + rng.integers(1, 2000, n)).astype(np.int32)
    hi[:50] = lo[:50] + 1                       # range of one value still consumes a draw
    lo[50:60], hi[50:60] = 0, 1 << 30           # the seeding range (megaverse.cpp:66, env.cpp:61)
    return lo, hi


def perlin_inputs(seed):
    rng = np.random.default_rng(seed & 0xffff)
    n = 4000
    xs = rng.uniform(0, 12, n); ys = rng.uniform(0, 12, n)
    xs[:64] = np.arange(64) / (42 / 9.9); ys[:64] = np.arange(64)[::-1] / (42 / 0.1)   # the x / fx, z / fz grid of scenario_collect.cpp:86-88
    return xs, ys


def bind_maze(lib, name):
    fn = getattr(lib, name)
    fn.argtypes = [C.c_int, C.c_uint, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    return fn


def maze(fn, size, seed):
    cells = C.c_int(0)
    n = fn(size, seed, C.byref(cells), None, None, None, None, None)
    counts = np.zeros(cells.value, np.int32); to = np.zeros(n, np.int32); xy = np.zeros((n, 4), np.float64)
    centers = np.zeros((cells.value, 2), np.float64); bounds = np.zeros(4, np.float64)
    assert fn(size, seed, C.byref(cells), counts.ctypes.data, to.ctypes.data, xy.ctypes.data, centers.ctypes.data, bounds.ctypes.data) == n
    return cells.value, counts, to, xy, centers, bounds


MAZE_FIELDS = ("cells", "counts", "to", "xy", "centers", "bounds")


def maze_arrays(fn, size, seed):
    return {f"maze_{size}_{seed}_{k}": np.asarray(v) for k, v in zip(MAZE_FIELDS, maze(fn, size, seed))}


def stored_maze(z, size, seed):
    return tuple(int(z[f"maze_{size}_{seed}_cells"]) if k == "cells" else z[f"maze_{size}_{seed}_{k}"] for k in MAZE_FIELDS)


def load():
    return np.load(PATH)


def util_lib():
    """oracle/_ref/libmv_ref_util.so with the split_string binding, or None where the reference tree was not there to build it"""
    ref = oracle_lib.ref_lib()
    if ref is not None and hasattr(ref, "mvref_split_string"):
        ref.mvref_split_string.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    return ref


def mazes_lib():
    p = os.path.join(oracle_lib.ORACLE_DIR, "_ref", "libmv_ref_mazes.so")
    return bind_maze(C.CDLL(p), "mvref_hex_maze") if os.path.exists(p) else None


def util_vectors(ref):
    """every stored array that comes from libmv_ref_util.so: the inputs and what the reference helpers return for them"""
    out = {}
    for seed in RAND_RANGE_SEEDS:
        lo, hi = rand_range_inputs(seed)
        b = np.empty(len(lo), np.int32)
        ref.mvref_rand_range_seq(seed, lo.ctypes.data, hi.ctypes.data, len(lo), b.ctypes.data)
        out[f"rand_range_{seed}_lo"], out[f"rand_range_{seed}_hi"], out[f"rand_range_{seed}"] = lo, hi, b
    for seed in FRAND_SEEDS:
        b = np.empty(FRAND_N, np.float32)
        ref.mvref_frand_seq(seed, FRAND_N, b.ctypes.data)
        out[f"frand_{seed}"] = b
    b = np.empty(ENV_SEEDS_N, np.int32)
    ref.mvref_env_seeds(42, ENV_SEEDS_N, b.ctypes.data)
    out["env_seeds_42"] = b
    out["triangular"] = np.array([ref.mvref_triangular_number(n) for n in range(TRIANGULAR_N)], np.int64)
    for seed, octaves in PERLIN_CASES:
        xs, ys = perlin_inputs(seed)
        b = np.empty(len(xs))
        ref.mvref_perlin_octave2_01(seed, xs.ctypes.data, ys.ctypes.data, len(xs), octaves, b.ctypes.data)
        out[f"perlin_{seed}_{octaves}_xs"], out[f"perlin_{seed}_{octaves}_ys"], out[f"perlin_{seed}_{octaves}"] = xs, ys, b
    counts, joined = [], []
    for t in SPLIT_TEXTS:
        buf = C.create_string_buffer(SPLIT_CAP)
        counts.append(ref.mvref_split_string(t.encode(), b"\n", buf, SPLIT_CAP))
        joined.append(buf.value)
    out["split_counts"] = np.array(counts, np.int64)
    out["split_joined"] = np.array(joined, dtype=f"S{SPLIT_CAP}")
    return out


def maze_vectors(fn):
    out = {}
    for size in MAZE_SIZES:
        for seed in MAZE_SEEDS:
            out.update(maze_arrays(fn, size, seed))
    return out


def assert_same_as_stored(fresh, keys=None):
    z = load()
    for k in (keys if keys is not None else fresh):
        a, b = np.asarray(fresh[k]), z[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"oracle/_ref disagrees with the stored vector {k}"
