"""Shared by tests/test_seed_envs*.py: the shapes, masks and seeds of the GPU tests, the per-env seed words of a master seed, and the host generators' episodes
as bytes."""
import ctypes as C

import numpy as np

from megaverse_amd import extension
from megaverse_amd.distributed import env_seeds

N = 8
W, H = 32, 32
FLAGGED = [0, 3, N - 1]
S1, S2 = 42, 777          # master seeds: every gym starts from S1; the flagged envs move to S2's per-env seeds
PERM = [3, 3, 0, 5, 5, 5, 1, 7]   # test 2: env d plays the levels of env PERM[d] of a gym seeded with S2


def mask_of(envs, n=N):
    m = np.zeros(n, np.bool_)
    m[list(envs)] = True
    return m


MASK = mask_of(FLAGGED)
MASKS = {"flagged_0_3_last": MASK, "complement": ~MASK}


def seed_words(master, mask, n=N):
    """int32 [n]: env_seeds(master, n)[e] where mask[e], -1 elsewhere"""
    s = np.asarray(env_seeds(master, n), np.int64)
    return np.where(np.asarray(mask, bool), s, -1).astype(np.int32)


def host_episode(scenario, A, seed, n, base_len=60.0):
    """the n-th (1-based) episode of an env seeded with `seed`, as the record's bytes: mv_debug_generate_episode, or the scenario's own generator hook
    (Sokoban, Football).  The generators leave the record's first word (seq) to the feeder."""
    lib = extension.load_library()
    if scenario in ("Sokoban", "Football"):
        fn = lib.mv_debug_generate_sokoban if scenario == "Sokoban" else lib.mv_debug_generate_football
        size = fn(A, seed, n, C.c_float(base_len), None, 0)
        out = np.zeros((n, size), np.uint8)
        assert fn(A, int(seed), n, C.c_float(base_len), out.ctypes.data, out.nbytes) == n, lib.mv_last_error()
        return out[n - 1].tobytes()
    size = lib.mv_debug_generate_episode(scenario.encode(), A, int(seed), n, C.c_float(base_len), None, 0)
    assert size > 0, lib.mv_last_error()
    out = np.zeros(size, np.uint8)
    assert lib.mv_debug_generate_episode(scenario.encode(), A, int(seed), n, C.c_float(base_len), out.ctypes.data, size) == size, lib.mv_last_error()
    return out.tobytes()
