"""The scenario table (mv_scenarios.h) from the outside, no GPU involved: what mv_create answers to an unknown name, the record size or the refusal each
host-only hook gives for each of the fifteen names, the episodes the one generator call draws, the feeder driven through both of its hooks, and the
Python side's one table.  Every literal was recorded from the library BEFORE the table existed: the table changes where facts are stated, not the facts.
(One case had no such record: mv_debug_feeder_selftest accepted BoxAGone but sized and compared its record as an Obstacles one, and failed; read from the
row it passes.)"""
import ctypes as C
import hashlib
import os

import pytest

import megaverse_amd.extension as ext
from megaverse_amd import megaverse_env, multitask, rl

BOXOBAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban")   # the synthetic levels the Sokoban tests use
UNKNOWN = ("mv_create: Unknown scenario {} (this build accelerates: TowerBuilding, ObstaclesEasy/Medium/Hard/Walls/Steps/Lava, Collect, Rearrange, Sokoban, "
           "HexMemory, HexExplore, BoxAGone, Football, Empty)")
REFUSE = None
REFUSALS = ("mv_debug_generate_episode: the Obstacles family, Empty, Collect, Rearrange, HexMemory, HexExplore and BoxAGone (Sokoban: mv_debug_generate_sokoban, "
            "Football: mv_debug_generate_football)",
            "mv_debug_feeder_selftest: the Obstacles family, Collect, Rearrange, HexMemory and HexExplore",
            "mv_debug_feeder_reseed_script: a host-generated scenario")
# name -> (mv_debug_generate_episode's record size, mv_debug_feeder_selftest's result, mv_debug_feeder_reseed_script's record size); REFUSE: the hook's
# refusal text.  The three sets of refusals differ.
RECORDS = {
    'TowerBuilding': (REFUSE, REFUSE, REFUSE),
    'ObstaclesEasy': (5184, 0, 5184),
    'ObstaclesMedium': (5184, 0, 5184),
    'ObstaclesHard': (5184, 0, 5184),
    'ObstaclesWalls': (5184, 0, 5184),
    'ObstaclesSteps': (5184, 0, 5184),
    'ObstaclesLava': (5184, 0, 5184),
    'Collect': (35440, 0, 35440),
    'Sokoban': (REFUSE, REFUSE, 5600),
    'HexMemory': (69792, 0, 69792),
    'HexExplore': (69792, 0, 69792),
    'Rearrange': (976, 0, 976),
    'Empty': (5184, REFUSE, 5184),
    'BoxAGone': (4320, 0, 4320),
    'Football': (REFUSE, REFUSE, 416),
}
# SHA-256 of episode 2 of an env seeded with 7, two agents, 60 s: mv_debug_generate_episode(name, 2, 7, 2, 60.0)
EPISODE_SHA256 = {
    'ObstaclesEasy': '64783089a6c72a900e3ba66f196e2bac80923285d03625de27ab1947ae60d86d',
    'ObstaclesMedium': '8df1c8d2963052dbf46cf04094b5980fda8efe77134c4dbc566fb0d373a77db4',
    'ObstaclesHard': '5bd316e6fd3a7c7b2a2f725778559372a5bb4d6c72ee733996cfc884e15f48ef',
    'ObstaclesWalls': '6874d855b00d6cc1de2d76eb0804a3bbca8e2fafa2378e4202b91a9a5893db65',
    'ObstaclesSteps': 'fe4c7ff056c105bdf85f3ef921cf83201b96d53d9ccf9103c0733de8a9d5ffb3',
    'ObstaclesLava': '620ffcf0aad10ae86a6cbb9c76b2449ec4821a2591f071052fa3bcf50aa61687',
    'Collect': '35eeb01b196e2dcff8a3bb1fac2a1cf49f48ad0d4a8d94cf9dd2793a46965b85',
    'HexMemory': 'e09c28a9bc04f211ae87e8d478b111577b916960ad78e12bd5376c154172665c',
    'HexExplore': '66cd17988d703d1c02f8a54bb5019261203dafae73a92de23482611aa938c534',
    'Rearrange': '0d0a146e559d2c726d1abbdec890640f0b392b953c1997035a6ce79c46426e72',
    'Empty': '037c64d06483ba2f0d8972abe00e52829f8c1a9f6a9081de0c08c088c8eb1249',
    'BoxAGone': 'fd8f6363c81fcad69f3c3cf531422da4b3b90d764202c98700b5cf3a4cfcb2b4',
}
# the same episode through the scenario's own hook (record 2 of mv_debug_generate_football / mv_debug_generate_sokoban(2, 7, 2, 60.0)): (record size, SHA-256)
OWN_HOOK = {'Football': (416, 'ccc94fe04b9ff614d637cfe06ff9c91b34fd752ee868022dd78800124d12a97a'),
            'Sokoban': (5600, '01a336e39e947946bc49b7ea069e6d091933731dd4ec3609995c650c40cd45f6')}
FAMILY = {'TowerBuilding': 0, 'ObstaclesEasy': 1, 'ObstaclesMedium': 1, 'ObstaclesHard': 1, 'ObstaclesWalls': 1, 'ObstaclesSteps': 1, 'ObstaclesLava': 1,
          'Collect': 2, 'Sokoban': 4, 'HexMemory': 6, 'HexExplore': 7, 'Rearrange': 3, 'Empty': 5, 'BoxAGone': 8, 'Football': 9}
NAMES = list(RECORDS)
MEGAVERSE8 = ['TowerBuilding', 'ObstaclesEasy', 'ObstaclesHard', 'Collect', 'Sokoban', 'HexMemory', 'HexExplore', 'Rearrange']


@pytest.fixture(scope="module")
def lib():
    return ext.load_library()


@pytest.fixture
def boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)


def last_error(lib):
    return lib.mv_last_error().decode()


def test_unknown_scenario_text():
    """the name is looked up before any device call: the full text, with the list of what the build accelerates, on a machine without a GPU too"""
    for bogus in ("NoSuchScenario", "ObstaclesImpossible", "Obstacles", ""):
        with pytest.raises(RuntimeError) as e:
            ext.MegaverseGym(bogus, 32, 32, 4, 1, 0, False, {})
        assert str(e.value) == UNKNOWN.format(bogus.lower())


@pytest.mark.parametrize("name", NAMES)
def test_record_size_or_refusal_of_each_hook(lib, name, boxoban):
    calls = (lambda: lib.mv_debug_generate_episode(name.encode(), 2, 7, 2, 60.0, None, 0),
             lambda: lib.mv_debug_feeder_selftest(name.encode(), 2, 2, 2, 3),   # (2 envs, 2 agents, 2 threads, 3 rounds: 0 = every episode as generated in turn)
             lambda: lib.mv_debug_feeder_reseed_script(name.encode(), 1, 1, 1, None, None, 0, None, 0, None))
    for call, want, refusal in zip(calls, RECORDS[name], REFUSALS):
        got = call()
        if want is REFUSE:
            assert got < 0 and last_error(lib) == refusal
        else:
            assert got == want, last_error(lib)


@pytest.mark.parametrize("name", list(EPISODE_SHA256))
def test_generated_episode_is_unchanged(lib, name):
    size = RECORDS[name][0]
    buf = (C.c_uint8 * size)()
    assert lib.mv_debug_generate_episode(name.encode(), 2, 7, 2, 60.0, buf, size) == size, last_error(lib)
    assert hashlib.sha256(bytes(buf)).hexdigest() == EPISODE_SHA256[name]


@pytest.mark.parametrize("name", list(OWN_HOOK))
def test_own_hook_episode_is_unchanged(lib, name, boxoban):
    if name == "Sokoban" and not os.path.isdir(os.path.join(BOXOBAN, "unfiltered", "train")):
        pytest.skip("the Boxoban levels the Sokoban tests use are not here")
    fn = lib.mv_debug_generate_football if name == "Football" else lib.mv_debug_generate_sokoban
    size, sha = OWN_HOOK[name]
    assert fn(2, 7, 2, 60.0, None, 0) == size
    buf = (C.c_uint8 * (2 * size))()
    assert fn(2, 7, 2, 60.0, buf, 2 * size) == 2, last_error(lib)
    assert hashlib.sha256(bytes(buf)[size:]).hexdigest() == sha


@pytest.mark.parametrize("name", [n for n in NAMES if RECORDS[n][2] is not REFUSE])
def test_reseed_script_succeeds(name, boxoban):
    """two envs: take, re-seed one, take -- every delivered episode equals sequential generation (the hook's own check), and the re-seeded env's differs"""
    script = [("take", 0), ("take", 1), ("seed", 1, 99), ("commit",), ("take", 0), ("take", 1)]
    takes = ext.debug_feeder_reseed_script(name, 2, 2, [11, 12], script)
    assert [t[0] for t in takes] == [0, 1, 0, 1] and all(0 < t[2] <= RECORDS[name][2] for t in takes)
    plain = ext.debug_feeder_reseed_script(name, 2, 2, [11, 12], [("take", 0), ("take", 1), ("take", 0), ("take", 1)])
    assert takes[:3] == plain[:3] and takes[3] != plain[3]


def test_python_table():
    assert megaverse_env.SUPPORTED_SCENARIOS == NAMES
    for name, fam in FAMILY.items():
        assert ext.scenario_family(name) == ext.scenario_family(name.upper()) == ext.scenario_family(fam) == fam
    for bogus in ("NoSuchScenario", "Obstacles", 10, -1, True):
        with pytest.raises(ValueError):
            ext.scenario_family(bogus)
    assert megaverse_env.MEGAVERSE8 == multitask.MEGAVERSE8 == rl.MEGAVERSE8 == multitask.MEGAVERSE_IN_SCOPE == MEGAVERSE8
    assert [s.name for s in rl.MEGAVERSE_ENVS] == MEGAVERSE8 + ["multitask_Obstacles", "multitask_megaverse8"]
