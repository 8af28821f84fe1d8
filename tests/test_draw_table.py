"""The table of draw kinds (megaverse_amd/csrc/mv_draw.h) as the generic host hook shows it (mv_debug_draw_host: no GPU involved): which scenarios have a
device episode generator, the record each draws, the message the others get, and the arguments the hook refuses."""
import numpy as np
import pytest

from draw_util import record_dtype
from megaverse_amd import extension as ext
from test_host_generators import MAX_AGENTS

DEVICE_DRAWN = {"Collect", "ObstaclesEasy", "ObstaclesMedium", "ObstaclesHard", "ObstaclesWalls", "ObstaclesSteps", "ObstaclesLava", "Empty", "HexMemory",
                "HexExplore"}


def test_every_scenario_has_its_record_or_the_listing_message():
    lib = ext.load_library()
    drawn = set()
    for name in ext.SCENARIOS:
        size = lib.mv_debug_draw_host(name.encode(), 1, 0, 1, 60.0, None, 0)
        if size > 0:
            assert size == record_dtype(name).itemsize, (name, size)
            drawn.add(name)
            continue
        assert size == -1, (name, size)
        message = lib.mv_last_error().decode()
        assert "no device generator" in message, (name, message)
        listed = {w.strip() for w in message.split(":")[-1].split(",")}
        assert listed == {d.lower() for d in DEVICE_DRAWN}, (name, message)   # (the table's names, lower case as scenario names are compared)
        assert name.lower() not in listed
    assert drawn == DEVICE_DRAWN, drawn ^ DEVICE_DRAWN
    assert lib.mv_debug_draw_host(b"NoSuchScenario", 1, 0, 1, 60.0, None, 0) == -1 and "no device generator" in lib.mv_last_error().decode()
    assert lib.mv_debug_draw_host(None, 1, 0, 1, 60.0, None, 0) == -1


@pytest.mark.parametrize("name", ["Collect", "ObstaclesHard", "Empty", "HexMemory"])
def test_bad_arguments_are_refused(name):
    lib = ext.load_library()
    dt = record_dtype(name)
    buf = np.full(dt.itemsize, 0xAB, np.uint8)

    def host(agents, n, out_bytes):
        return lib.mv_debug_draw_host(name.encode(), agents, 7, n, 60.0, buf.ctypes.data, out_bytes)

    for agents, n, out_bytes, what in ((1, 0, dt.itemsize, "bad arguments"), (0, 1, dt.itemsize, "bad arguments"), (MAX_AGENTS + 1, 1, dt.itemsize, "bad arguments"),
                                       (1, 1, dt.itemsize - 1, "buffer too small")):
        assert host(agents, n, out_bytes) == -1, (agents, n, out_bytes)
        assert what in lib.mv_last_error().decode(), (agents, n, out_bytes, lib.mv_last_error().decode())
        assert (buf == 0xAB).all(), "a refused call writes nothing"
    assert host(MAX_AGENTS, 1, dt.itemsize) == dt.itemsize and buf.view(dt)[0]["seq"] == 1
