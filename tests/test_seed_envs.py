"""Level seeds without a device (include/megaverse_hip.h: mv_seed_envs): the ABI, the episode feeder's re-seed of a subset (EpisodeFeeder::reseed_envs through
mv_debug_feeder_reseed_script) against the host generators' own episodes, the Python argument forms."""
import os
import re

import numpy as np
import pytest

from megaverse_amd import extension
from megaverse_amd.extension import check_env_seeds, debug_feeder_reseed_script
from seed_envs_util import host_episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    """1. both calls are declared with two parameters, exported and bound; the hook too.  The ABI version stays 2: the calls are an addition, and every earlier
    feature's test pins the version at 2 for additions."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_seed_envs", 2), ("mv_seed_envs_host", 2), ("mv_debug_feeder_reseed_script", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == arity, f"{name}: declared with {m.group(1)!r}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert lib.mv_abi_version() == 2   # (additive)
    for cls, names in ((extension.MegaverseGym, ("seed_envs",)),):
        for n in names:
            assert callable(getattr(cls, n))
    from megaverse_amd.megaverse_env import MegaverseEnv
    from megaverse_amd.multitask import MultiTaskGym
    assert callable(MegaverseEnv.seed_envs) and callable(MegaverseEnv.start_levels) and callable(MultiTaskGym.seed_envs)
    assert "seed_envs" in open(os.path.join(ROOT, "megaverse_amd", "pybind", "megaverse_module.cpp")).read()


def test_no_gym_is_an_error_with_text():
    lib = extension.load_library()
    seeds = np.ones(4, np.int32)
    for fn in (lib.mv_seed_envs, lib.mv_seed_envs_host):
        assert fn(None, seeds.ctypes.data) == -1
        assert b"null gym" in lib.mv_last_error()


# ---- 2. the feeder -------------------------------------------------------------------------------------------------------------------------------------
FEEDER_N, FEEDER_A = 12, 2
NEW_A, NEW_B, NEW_C = 555, 90210, 31337
# scenarios whose generator clears the whole record: every byte behind seq compares.  HexMemory's clears everything in front of its box list, whose used
# prefix travels: the used bytes compare.  Collect's clears what it uses: its scalars and the used prefix of every list compare, field by field.
WHOLE = ("ObstaclesEasy", "Rearrange", "BoxAGone", "Football", "Sokoban")


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("scenario", ["ObstaclesEasy", "Collect", "Rearrange", "HexMemory", "BoxAGone", "Football", "Sokoban"])
def test_feeder_reseeds_a_subset(scenario, threads, monkeypatch):
    """2. 12 envs, episodes 1..2 of every env consumed; ONE reseed_envs call for envs {0, 5, 11} (0 and 11 get the same value); then, nothing consumed in
    between, a second call re-seeds env 5 again; then three more episodes of every env.
    Inside the hook every delivered episode is compared with sequential generation from the same seeds.  Here, on the delivered bytes: envs 0 and 11
    deliver episodes 1, 2, 3 of NEW_A and env 5 those of NEW_C -- the LAST seed's -- as the scenario's generator hook draws them; every other env delivers
    episodes 3, 4, 5 of its original seed, among them the one that was ready or in flight at the re-seed (the feeder generates one episode ahead).
    Sokoban: an env's shuffled level list is carried across Env::seed, so a re-seeded env's levels are NOT those of a fresh env with that seed (the
    generator hook's): its episodes are pinned by the hook's inside comparison, whose model carries the list; the byte comparison here covers its
    unflagged envs and all five episodes in front of the re-seed."""
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(ROOT, "tests", "golden", "boxoban"))
    N, A = FEEDER_N, FEEDER_A
    seeds = [1000 + 7 * i for i in range(N)]
    script = [("take", e) for _ in range(2) for e in range(N)]
    script += [("seed", 0, NEW_A), ("seed", 5, NEW_B), ("seed", 11, NEW_A), ("commit",), ("seed", 5, NEW_C), ("commit",)]
    script += [("take", e) for _ in range(3) for e in (list(range(N)) if _ != 1 else list(reversed(range(N))))]
    got = debug_feeder_reseed_script(scenario, A, threads, seeds, script)
    assert len(got) == 5 * N
    per_env = {e: [] for e in range(N)}
    for e, rec, used in got:
        per_env[e].append((rec, used))
    new = {0: NEW_A, 5: NEW_C, 11: NEW_A}
    for e in range(N):
        assert len(per_env[e]) == 5
        for j, (rec, used) in enumerate(per_env[e]):
            assert int(np.frombuffer(rec[:4], np.int32)[0]) == j + 1, f"env {e}: sequence number of its delivery {j}"
            if j < 2 or e not in new:
                seed, n = seeds[e], j + 1
            elif scenario == "Sokoban":
                continue
            else:
                seed, n = new[e], j - 1
            want = host_episode(scenario, A, seed, n)
            if scenario == "Collect":   # (the generator clears what it uses: the scalars, then the used prefix of every list)
                from test_host_generators import COLLECT_BLOB
                a, b = np.frombuffer(rec, COLLECT_BLOB)[0], np.frombuffer(want, COLLECT_BLOB)[0]
                what = f"Collect, env {e}, delivery {j}: not episode {n} of seed {seed}"
                for name in ("num_boxes", "num_objects", "num_rewards", "num_positive", "layout_color", "wall_color", "dim", "episode_len", "spawn", "heightmap"):
                    assert a[name].tobytes() == b[name].tobytes(), f"{what}: {name}"
                assert a["yaw_frand"][:A].tobytes() == b["yaw_frand"][:A].tobytes(), what
                for name, count in (("boxes", "num_boxes"), ("objects", "num_objects"), ("rewards", "num_rewards")):
                    assert a[name][:int(b[count])].tobytes() == b[name][:int(b[count])].tobytes(), f"{what}: {name}"
                assert used == COLLECT_BLOB.fields["boxes"][1] + int(b["num_boxes"]) * 32
                continue
            end = len(rec) if scenario in WHOLE else used
            assert 4 < end <= len(rec)
            assert rec[4:end] == want[4:end], f"{scenario}, env {e}, delivery {j}: not episode {n} of seed {seed}"
    if scenario not in ("Sokoban", "Collect"):   # (Collect: bytes behind a list's used prefix are whatever the slot held)
        for j in range(2, 5):
            u = per_env[0][j][1]
            assert per_env[0][j][0][:u] == per_env[11][j][0][:u], "two envs with the same seed deliver different episodes"
            assert per_env[0][j][0][:u] != per_env[1][j][0][:u]


def test_feeder_hook_sees_a_difference():
    """the hook's inside comparison is not vacuous: a script that re-seeds nothing passes, and the delivered episodes of a re-seeded env differ from its
    original stream's"""
    N, A = 4, 1
    seeds = [11, 22, 33, 44]
    plain = debug_feeder_reseed_script("ObstaclesEasy", A, 2, seeds, [("take", e) for _ in range(3) for e in range(N)])
    moved = debug_feeder_reseed_script("ObstaclesEasy", A, 2, seeds, [("take", e) for e in range(N)] + [("seed", 2, 99), ("commit",)]
                                       + [("take", e) for _ in range(2) for e in range(N)])
    same = [p[1] == m[1] for p, m in zip(plain, moved)]
    assert same == [True] * N + [e != 2 for e in range(N)] * 2
    with pytest.raises(RuntimeError, match="bad script entry"):
        debug_feeder_reseed_script("ObstaclesEasy", A, 1, seeds, [("take", N)])
    with pytest.raises(RuntimeError, match="host-generated"):
        debug_feeder_reseed_script("TowerBuilding", A, 1, seeds, [("take", 0)])


# ---- 3. the Python argument forms ----------------------------------------------------------------------------------------------------------------------
def test_argument_forms_normalise_to_the_same_array():
    want = np.array([5, -1, 0, -1, 2 ** 31 - 1], np.int32)
    forms = ([5, None, 0, -1, 2 ** 31 - 1], (5, -1, 0, None, 2 ** 31 - 1), np.array([5, -1, 0, -1, 2 ** 31 - 1], np.int64), np.array([5, -1, 0, -1, 2 ** 31 - 1], np.int32),
             {0: 5, 2: 0, 4: 2 ** 31 - 1}, {4: 2 ** 31 - 1, 0: 5, 2: 0, 1: None, 3: -7}, np.array([5, None, 0, -1, 2 ** 31 - 1], object))
    for f in forms:
        m = check_env_seeds(f, 5)
        assert m.dtype == np.int32 and m.flags.c_contiguous and m.shape == (5,)
        assert ((m < 0) == (want < 0)).all() and (m[want >= 0] == want[want >= 0]).all(), f
    assert check_env_seeds({}, 3).tolist() == [-1, -1, -1]
    assert check_env_seeds(np.array([1, 2, 3], np.uint8), 3).tolist() == [1, 2, 3]


def test_wrong_shape_or_dtype_is_a_value_error():
    for bad in ([1, 2], np.zeros((3, 1), np.int32), np.zeros(3, np.float32), [0.5, 1, 2], [True, 1, 2], {3: 1}, {-1: 1}, {0: 1.5}, {"0": 1}, 7, None,
                [1, 2, 2 ** 31], np.array([1, 2, 2 ** 31], np.int64), {0: 2 ** 31}, "abc"):
        with pytest.raises(ValueError, match="seed_envs"):
            check_env_seeds(bad, 3)


def test_an_object_with_only_a_data_ptr_is_a_value_error():
    class Tensor:
        def __init__(self, shape=(3,), dtype="torch.int32", cuda=True, contiguous=True):
            self.shape, self.dtype, self.is_cuda, self._c = shape, dtype, cuda, contiguous

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            return 0

    class NoShape:
        def data_ptr(self):
            return 0

    assert check_env_seeds(Tensor(), 3) == "device"
    for bad in (Tensor(shape=(4,)), Tensor(shape=(3, 1)), Tensor(dtype="torch.int64"), Tensor(dtype="torch.uint8"), Tensor(cuda=False), Tensor(contiguous=False),
                NoShape()):
        with pytest.raises(ValueError, match="seed_envs"):
            check_env_seeds(bad, 3)


def test_env_wrapper_words():
    """MegaverseEnv.seed_envs / start_levels build {env: seed} from (env_ids, seeds): one seed per env, or one int for all"""
    from megaverse_amd.megaverse_env import MegaverseEnv

    class Fake:
        num_envs = 6
    words, ids = MegaverseEnv._seed_words(Fake(), [4, 1], [10, 20], "seed_envs")
    assert words == {4: 10, 1: 20} and ids.tolist() == [4, 1]
    assert MegaverseEnv._seed_words(Fake(), range(3), 9, "seed_envs")[0] == {0: 9, 1: 9, 2: 9}
    for ids, seeds in (([6], [1]), ([-1], [1]), ([0, 1], [1]), ([0], [-1]), ([0], [1.5]), ([0], [2 ** 31])):
        with pytest.raises(ValueError, match="start_levels"):
            MegaverseEnv._seed_words(Fake(), ids, seeds, "start_levels")
