"""Env stores without a device (include/megaverse_hip.h: mv_save_envs / mv_load_envs): the rule of the two maps, the record's layout, pack and unpack --
the host-only hooks run the functions the kernels run (megaverse_amd/csrc/mv_env_store.h) -- against numpy models, and the Python argument checks."""
import numpy as np
import pytest

from megaverse_amd.extension import (check_env_store, check_fork_map, debug_env_record_layout_host, debug_env_record_pack_host,
                                     debug_env_record_unpack_host, debug_env_store_plan_host)

IDENTITY = [19, 20, 28, 29]   # EnvHeader dwords next_seed, seed_is_env_seed, episodes_consumed, starved (mv_fork.h: IDENTITY_DWORDS)
HEADER = 64                   # bytes of the record header
ENV_HDR = 128


# ---- the maps' rule ------------------------------------------------------------------------------------------------------------------------------------
def model_plan(m, slots, is_save):
    m = np.asarray(m, np.int64)
    in_range = (m >= 0) & (m < slots)
    invalid = (m != -1) & ~in_range
    if is_save:
        times = np.bincount(m[in_range], minlength=max(slots, 1))
        invalid |= in_range & (times[np.where(in_range, m, 0)] > 1)
    resolved = np.where(in_range & ~invalid, m, -1)
    return resolved.astype(np.int32), invalid.astype(np.int32)


def check_plan(m, slots):
    for is_save in (True, False):
        resolved, invalid = debug_env_store_plan_host(m, slots, is_save)
        want_r, want_i = model_plan(m, slots, is_save)
        assert resolved.tolist() == want_r.tolist() and invalid.tolist() == want_i.tolist(), (list(m), slots, is_save)


def test_map_rule_on_hand_written_maps():
    r, i = debug_env_store_plan_host([0, 1, 2, -1, 3, 3, 16, -2], 16, True)
    assert r.tolist() == [0, 1, 2, -1, -1, -1, -1, -1] and i.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    r, i = debug_env_store_plan_host([0, 1, 2, -1, 3, 3, 16, -2], 16, False)
    assert r.tolist() == [0, 1, 2, -1, 3, 3, -1, -1] and i.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    r, i = debug_env_store_plan_host([5, 5, 5, 4], 6, True)   # three envs on one slot: all three invalid
    assert r.tolist() == [-1, -1, -1, 4] and i.tolist() == [1, 1, 1, 0]
    r, i = debug_env_store_plan_host([-1] * 8, 3, True)
    assert r.tolist() == [-1] * 8 and not i.any()
    # an entry out of range names no slot: it does not make another entry a duplicate
    r, i = debug_env_store_plan_host([3, 3 + 2 ** 16, -1], 4, True)
    assert r.tolist() == [3, -1, -1] and i.tolist() == [0, 1, 0]


@pytest.mark.parametrize("N", [1, 2, 8, 64])
def test_map_rule_against_numpy_on_random_maps(N):
    rng = np.random.default_rng(100 + N)
    for slots in (1, 3, 2 * N):
        check_plan(np.arange(N) % slots, slots)
        check_plan(np.full(N, -1), slots)
        for _ in range(200):
            check_plan(rng.integers(-3, slots + 3, N), slots)
            check_plan(np.where(rng.random(N) < 0.5, -1, rng.permutation(max(N, slots))[:N]), slots)   # mostly valid saves


# ---- pack and unpack -----------------------------------------------------------------------------------------------------------------------------------
SHAPES = {"rows_only": ([4096, 640, 176 * 2, 16], 2), "with_a_dword_and_a_byte_array": ([64, 4, 48, 1, 32], 3)}


def up16(b):
    return (b + 15) & ~15


def model_layout(array_bytes, A):
    off, o = [HEADER], HEADER + ENV_HDR
    for b in array_bytes:
        off.append(o)
        o = up16(o + b)
    off.append(o); o = up16(o + 8 * A)
    off.append(o); o = up16(o + 4)
    return o, off


def random_env(rng, array_bytes, A):
    """an env as the hooks take it: EnvHeader, the arrays, ret[A], len"""
    return rng.integers(0, 256, ENV_HDR + sum(array_bytes) + 8 * A + 4, dtype=np.uint8)


def split(env, array_bytes, A):
    parts, o = [env[:ENV_HDR].view(np.uint32)], ENV_HDR
    for b in array_bytes + [8 * A, 4]:
        parts.append(env[o:o + b]); o += b
    return parts   # header dwords, the arrays ..., ret, len


@pytest.mark.parametrize("shape", list(SHAPES))
def test_record_layout(shape):
    array_bytes, A = SHAPES[shape]
    size, off = debug_env_record_layout_host(array_bytes, A)
    want_size, want_off = model_layout(array_bytes, A)
    assert size == want_size and off.tolist() == want_off
    assert size % 16 == 0 and all(o % 16 == 0 for o in off.tolist())


@pytest.mark.parametrize("log_on", [True, False], ids=["log_on", "log_off"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pack_against_numpy(shape, log_on):
    array_bytes, A = SHAPES[shape]
    rng = np.random.default_rng(7)
    word = 0x0123456789ABCDEF
    env = random_env(rng, array_bytes, A)
    rec = debug_env_record_pack_host(array_bytes, A, word, log_on, env)
    size, off = model_layout(array_bytes, A)
    want = np.zeros(size, np.uint8)
    want[:HEADER].view(np.uint32)[:7] = [0x5652454D, 1, word & 0xFFFFFFFF, word >> 32, size, 0, 1 if log_on else 0]
    parts = split(env, array_bytes, A)
    want[off[0]:off[0] + ENV_HDR] = env[:ENV_HDR]   # the whole header, identity included
    for k, b in enumerate(array_bytes):
        want[off[1 + k]:off[1 + k] + b] = parts[1 + k]
    if log_on:
        want[off[-2]:off[-2] + 8 * A], want[off[-1]:off[-1] + 4] = parts[-2], parts[-1]
    assert rec.tobytes() == want.tobytes()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pack_then_unpack_is_a_fork(shape):
    """env s packed, the record unpacked into env d: d is s on every array and on the non-identity header dwords, its identity dwords are its own"""
    array_bytes, A = SHAPES[shape]
    rng = np.random.default_rng(11)
    word = 0xFEDCBA9876543210
    s, d = random_env(rng, array_bytes, A), random_env(rng, array_bytes, A)
    rec = debug_env_record_pack_host(array_bytes, A, word, True, s)
    refused, out = debug_env_record_unpack_host(array_bytes, A, word, True, rec, d)
    assert not refused
    ps, pd, po = split(s, array_bytes, A), split(d, array_bytes, A), split(out, array_bytes, A)
    for i in range(32):
        assert po[0][i] == (pd[0][i] if i in IDENTITY else ps[0][i]), f"header dword {i}"
    for k in range(1, len(ps)):
        assert po[k].tobytes() == ps[k].tobytes(), f"array {k}"
    # into an env whose log is off: the accumulators are left alone
    refused, out = debug_env_record_unpack_host(array_bytes, A, word, False, rec, d)
    po = split(out, array_bytes, A)
    assert not refused and po[-2].tobytes() == pd[-2].tobytes() and po[-1].tobytes() == pd[-1].tobytes()
    assert all(po[k].tobytes() == ps[k].tobytes() for k in range(1, len(ps) - 2))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_refused_records_leave_the_env_untouched(shape):
    array_bytes, A = SHAPES[shape]
    rng = np.random.default_rng(13)
    word = 0x1111222233334444
    s, d = random_env(rng, array_bytes, A), random_env(rng, array_bytes, A)
    size, _ = model_layout(array_bytes, A)
    refused, out = debug_env_record_unpack_host(array_bytes, A, word, True, np.zeros(size, np.uint8), d)   # a slot never written
    assert refused and out.tobytes() == d.tobytes()
    rec = debug_env_record_pack_host(array_bytes, A, word ^ 1, True, s)   # a genuine record of another layout word
    refused, out = debug_env_record_unpack_host(array_bytes, A, word, True, rec, d)
    assert refused and out.tobytes() == d.tobytes()
    # ... and of another record size: the same arrays with one more row
    other = array_bytes[:-1] + [array_bytes[-1] + 16]
    rec = debug_env_record_pack_host(other, A, word, True, random_env(rng, other, A))
    refused, out = debug_env_record_unpack_host(array_bytes, A, word, True, rec[:size], d)
    assert refused and out.tobytes() == d.tobytes()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_record_saved_with_the_log_off_counts_from_the_load(shape):
    array_bytes, A = SHAPES[shape]
    rng = np.random.default_rng(17)
    word = 5
    s, d = random_env(rng, array_bytes, A), random_env(rng, array_bytes, A)
    rec = debug_env_record_pack_host(array_bytes, A, word, False, s)
    refused, out = debug_env_record_unpack_host(array_bytes, A, word, True, rec, d)
    po, ps = split(out, array_bytes, A), split(s, array_bytes, A)
    assert not refused and not po[-2].any() and not po[-1].any()
    assert all(po[k].tobytes() == ps[k].tobytes() for k in range(1, len(ps) - 2))


# ---- the Python argument checks ------------------------------------------------------------------------------------------------------------------------
class FakeTensor:
    """what check_env_store / check_fork_map look at, without a device"""

    def __init__(self, shape, dtype="torch.uint8", cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous, self.device = tuple(shape), dtype, cuda, contiguous, "cuda:0" if cuda else "cpu"

    def data_ptr(self):
        return 4096

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


def test_argument_checks():
    assert check_env_store(FakeTensor((16, 1024)), 1024, "save_envs") == 16
    with pytest.raises(ValueError, match="contiguous"):
        check_env_store(FakeTensor((16, 1024), contiguous=False), 1024, "save_envs")
    with pytest.raises(ValueError, match=r"\(slots, 1024\)"):
        check_env_store(FakeTensor((16, 1040)), 1024, "load_envs")   # a store of another gym's record size
    with pytest.raises(ValueError, match=r"\(slots, 1024\)"):
        check_env_store(FakeTensor((16 * 1024,)), 1024, "load_envs")
    with pytest.raises(ValueError, match="torch.uint8 CUDA"):
        check_env_store(FakeTensor((16, 1024), dtype="torch.int8"), 1024, "save_envs")
    with pytest.raises(ValueError, match="torch.uint8 CUDA"):
        check_env_store(FakeTensor((16, 1024), cuda=False), 1024, "save_envs")
    with pytest.raises(ValueError, match="torch.uint8 CUDA"):
        check_env_store(np.zeros((16, 1024), np.uint8), 1024, "save_envs")
    # the map: fork_envs' rule under the caller's name
    assert check_fork_map(FakeTensor((8,), dtype="torch.int32"), 8, "save_envs") == "device"
    with pytest.raises(ValueError, match="save_envs: a tensor map must be a contiguous int32 CUDA tensor"):
        check_fork_map(FakeTensor((8,), dtype="torch.int64"), 8, "save_envs")
    with pytest.raises(ValueError, match="load_envs: a tensor map"):
        check_fork_map(FakeTensor((8, 1), dtype="torch.int32"), 8, "load_envs")
    with pytest.raises(ValueError, match="load_envs: the map must be 8 integers"):
        check_fork_map([0] * 7, 8, "load_envs", "slot_of[d] = the record env d continues from")
    with pytest.raises(ValueError, match="save_envs: the map must be 8 integers"):
        check_fork_map(np.zeros(8, np.float32), 8, "save_envs", "slot_of[e]")
    assert check_fork_map(list(range(8)), 8, "save_envs").dtype == np.int32


def test_env_surface_builds_the_maps():
    """MegaverseEnv.save / load: env_ids and slots become the gym's map"""
    from megaverse_amd.megaverse_env import MegaverseEnv

    class Recorder:
        def __init__(self):
            self.calls = []

        def save_envs(self, m, store):
            self.calls.append(("save", m.tolist(), store))

        def load_envs(self, m, store):
            self.calls.append(("load", m.tolist(), store))

    env = MegaverseEnv.__new__(MegaverseEnv)
    env.num_envs, env.env = 8, Recorder()
    env.save([1, 5], "store")
    env.load([0, 2, 3], "store", slots=[5, 5, 1])
    assert env.env.calls == [("save", [-1, 1, -1, -1, -1, 5, -1, -1], "store"), ("load", [5, -1, 5, 1, -1, -1, -1, -1], "store")]
    with pytest.raises(ValueError, match="env_ids"):
        env.save([8], "store")
    with pytest.raises(ValueError, match="twice"):
        env.load([1, 1], "store")
    with pytest.raises(ValueError, match="one record per env"):
        env.load([1, 2], "store", slots=[0])
