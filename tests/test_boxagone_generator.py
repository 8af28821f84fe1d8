"""BoxAGone's host-side episode generator (mv_gen_boxagone.cpp, reached through mv_debug_generate_episode -- no GPU involved) against the
Python restatement in boxagone_model.py: the restatement's mt19937 / randRange / frand / std::shuffle are pinned against the oracle's C++
and the stored reference vectors first, then the generator's records must be byte-identical, episode after episode of each env's stream."""
import numpy as np
import pytest

import boxagone_model as M
import oracle_lib
from megaverse_amd import extension as ext

REF = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "ref_vectors.npz"))


def test_mt19937_matches_oracle():
    r = M.MT19937(5489)
    v = [r() for _ in range(10000)]
    assert v[-1] == 4123659995   # [rand.predef]
    L = oracle_lib.lib()
    for seed in (0, 42, 123456789):
        r = M.MT19937(seed)
        got = [r() for _ in range(700)]
        assert got[0] == L.mvo_mt19937_nth(seed, 1) and got[699] == L.mvo_mt19937_nth(seed, 700)


@pytest.mark.parametrize("seed", [0, 42, 4294967295])
def test_rand_range_and_frand_match_oracle_and_stored_vectors(seed):
    L = oracle_lib.lib()
    lo, hi = REF[f"rand_range_{seed}_lo"].astype(np.int32), REF[f"rand_range_{seed}_hi"].astype(np.int32)
    r = M.MT19937(seed)
    got = np.array([M.rand_range(int(a), int(b), r) for a, b in zip(lo, hi)], np.int32)
    assert np.array_equal(got, REF[f"rand_range_{seed}"])
    o = np.empty(lo.size, np.int32)
    L.mvo_rand_range_seq(seed & 0xFFFFFFFF, lo.ctypes.data, hi.ctypes.data, lo.size, o.ctypes.data)
    assert np.array_equal(got, o)
    r = M.MT19937(seed)
    f = np.array([M.frand(r) for _ in range(5000)], np.float32)
    of = np.empty(5000, np.float32)
    L.mvo_frand_seq(seed & 0xFFFFFFFF, 5000, of.ctypes.data)
    assert np.array_equal(f.view(np.uint32), of.view(np.uint32))
    if f"frand_{seed}" in REF.files:
        assert np.array_equal(f.view(np.uint32), REF[f"frand_{seed}"][:5000].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 10, 99, 100, 1023])
def test_shuffle_matches_std_shuffle(n):
    o = np.empty(n, np.int32)
    oracle_lib.lib().mvo_shuffle_iota(99, n, o.ctypes.data)
    seq = list(range(n))
    M.shuffle(seq, M.MT19937(99))
    assert seq == o.tolist()


def env_seeds(master, n):
    r = M.MT19937(master)
    return [M.rand_range(0, 1 << 30, r) for _ in range(n)]


def generated(agents, env_seed, n, base_len=300.0):
    lib = ext.load_library()
    size = lib.mv_debug_generate_episode(b"BoxAGone", agents, env_seed, n, base_len, None, 0)
    assert size == M.BLOB.itemsize, (size, M.BLOB.itemsize)
    buf = np.zeros(size, np.uint8)
    assert lib.mv_debug_generate_episode(b"BoxAGone", agents, env_seed, n, base_len, buf.ctypes.data, size) == size
    return buf


@pytest.mark.parametrize("agents", [1, 2, 4])
def test_generator_matches_restatement_byte_for_byte(agents):
    for env_seed in env_seeds(2024 + agents, 8):
        rng = M.MT19937(env_seed)
        for n in range(1, 26):
            want = M.generate(rng, agents)
            got = generated(agents, env_seed, n)
            assert np.array_equal(got, M.blob_bytes(want)), (env_seed, n)
            check_ranges(got.view(M.BLOB)[0], agents)


def check_ranges(b, agents):
    L = int(b["num_levels"])
    assert L in (2, 3)
    heights = [int(h) for h in b["level_y"][:L]]
    assert heights[0] in (3, 4) and all(1 <= h1 - h0 - 1 <= 2 for h0, h1 in zip(heights, heights[1:]))
    assert b["num_boxes"] == 5 and b["boxes"][0]["max"].tolist() == [24, 1, 24]
    plats = b["platforms"][: int(b["num_platforms"])]
    assert 0 < len(plats) <= M.MAX_PLATFORMS and not b["platforms"][len(plats):].view(np.uint32).any()
    for lv in range(L):
        p = plats[plats["state"] == lv]
        assert len(p) and (p["y"] == heights[lv]).all()
        xs, zs = p["x"].astype(int), p["z"].astype(int)
        assert 1 <= xs.max() - xs.min() + 1 <= 18 and 1 <= zs.max() - zs.min() + 1 <= 18
        assert xs.min() >= 12 - 9 and xs.max() <= 12 + 8 and zs.min() >= 3 and zs.max() <= 20
    top = {(int(p["x"]), int(p["z"])) for p in plats[plats["state"] == L - 1]}
    for i in range(agents):   # every agent spawns above a top-level platform's cell
        s = b["spawn"][i]
        assert s[1] == (heights[-1] + 0.5) * 2 and (int(s[0] // 2), int(s[2] // 2)) in top
        assert 0.0 <= b["yaw_frand"][i] < 1.0
    assert b["episode_len"] == 300.0


def test_params_reach_the_generator():
    b = generated(1, 5, 1, base_len=2.0).view(M.BLOB)[0]
    assert b["episode_len"] == 2.0


def test_name_is_accepted_and_football_is_not():
    lib = ext.load_library()
    assert lib.mv_debug_generate_episode(b"boxagone", 1, 1, 1, 300.0, None, 0) == M.BLOB.itemsize
    assert lib.mv_debug_generate_episode(b"Football", 1, 1, 1, 300.0, None, 0) < 0
