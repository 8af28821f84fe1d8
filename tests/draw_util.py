"""The two hooks every device episode generator is tested through (megaverse_amd/csrc/mv_draw.hip: mv_debug_draw_host, mv_debug_draw_device over the table of
draw kinds, mv_draw.h): the n-th episode of an env as the scenario's device generator draws it on the host, and as its kernel draws it on the device."""
import numpy as np

from megaverse_amd import extension as ext
from test_host_generators import COLLECT_BLOB, EPISODE_BLOB, HEX_BLOB


def record_dtype(name):
    """the episode record of the scenario's family, as test_host_generators.py states it"""
    return COLLECT_BLOB if name.lower() == "collect" else HEX_BLOB if name.lower().startswith("hex") else EPISODE_BLOB


def draw_host(name, agents, env_seed, n, base_len=60.0):
    lib = ext.load_library()
    dt = record_dtype(name)
    size = lib.mv_debug_draw_host(name.encode(), agents, env_seed, n, base_len, None, 0)
    assert size == dt.itemsize, (size, lib.mv_last_error().decode())
    buf = np.zeros(1, dt)
    assert lib.mv_debug_draw_host(name.encode(), agents, env_seed, n, base_len, buf.ctypes.data, size) == size
    return buf[0]


def draw_device(name, agents, seeds, n, base_len=60.0):
    """-> (the envs' n-th episodes, ms per launch)"""
    lib = ext.load_library()
    seeds = np.asarray(seeds, np.int32)
    out = np.zeros(len(seeds), record_dtype(name))
    ms = np.zeros(1, np.float32)
    rc = lib.mv_debug_draw_device(0, name.encode(), agents, seeds.ctypes.data, len(seeds), n, base_len, out.ctypes.data, out.nbytes, ms.ctypes.data)
    assert rc == 0, lib.mv_last_error().decode()
    return out, float(ms[0])
