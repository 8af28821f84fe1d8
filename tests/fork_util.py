"""Shared by tests/test_fork*.py: the one fork map the GPU tests use, the action columns it implies, and a numpy model of the episode log."""
import numpy as np

N = 8
# env 0 and the last env are sources, each serves two destinations; entry 4 points at itself; the rest are left alone
MAP = [-1, 0, 0, 7, 4, 7, -1, -1]
W, H = 64, 36


def columns(m=MAP):
    """the env whose episode env e runs after the fork -- and whose column of the script it therefore acts on to stay its twin: the source, or itself"""
    return [s if s >= 0 and s != e else e for e, s in enumerate(m)]


def remap(script, cols, A, from_tick):
    """script [T, N*A, 6] with, from tick from_tick on, env e's agents acting on env cols[e]'s columns"""
    out = script.copy()
    for e, c in enumerate(cols):
        out[from_tick:, e * A:(e + 1) * A] = script[from_tick:, c * A:(c + 1) * A]
    return out


def log_model(rewards, dones, true_obj, A):
    """the episode log (include/megaverse_hip.h: mv_set_episode_log) in numpy: rewards / true_obj [T][N*A] float32, dones [T][N] -> the records as tuples
    (agent, length, end_tick, true_objective, ret) in log order, and the final running (ret float64 [N*A], len int32 [N])"""
    T, n = dones.shape
    ret, length, records = np.zeros(n * A, np.float64), np.zeros(n, np.int32), []
    for t in range(T):
        ret += rewards[t].astype(np.float64)
        length += 1
        for e in np.flatnonzero(dones[t]):
            for a in range(A):
                i = e * A + a
                records.append((i, int(length[e]), t, float(true_obj[t, i]), float(ret[i])))
                ret[i] = 0.0
            length[e] = 0
    return records, ret, length
