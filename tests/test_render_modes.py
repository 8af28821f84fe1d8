"""Render modes of batched calls (include/megaverse_hip.h: mv_step_n_render) -- what can be checked without a device: the C ABI carries the entry point
and the three modes, the Python surface defaults to 'every' and refuses unknown modes."""
import inspect
import os
import re

import pytest

import megaverse_amd.extension as ext

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "megaverse_hip.h")


def test_symbol_and_modes_exist():
    """mv_step_n_render is exported by the loaded library and typed by the binding; the header's enum and the binding's table agree"""
    lib = ext.load_library()
    assert hasattr(lib, "mv_step_n_render")
    typed = {name: args for name, _, args in ext.SYMBOLS}
    assert len(typed["mv_step_n_render"]) == len(typed["mv_step_n"]) + 1
    text = open(HEADER).read()
    m = re.search(r"enum\s*\{\s*MV_RENDER_EVERY\s*=\s*(\d+)\s*,\s*MV_RENDER_LAST\s*=\s*(\d+)\s*,\s*MV_RENDER_NONE\s*=\s*(\d+)\s*\}", text)
    assert m, "include/megaverse_hip.h declares no MV_RENDER_* enum"
    assert tuple(int(x) for x in m.groups()) == (0, 1, 2)
    assert ext.RENDER_MODES == {"every": 0, "last": 1, "none": 2}
    assert re.search(r"int\s+mv_step_n_render\s*\(\s*mv_gym\s*\*g,\s*int32_t k,\s*int32_t policy,\s*uint32_t seed,\s*uint32_t first_step_index,\s*int32_t render_mode\)",
                     text)
    assert lib.mv_abi_version() == 2


def test_python_default_is_every():
    from megaverse_amd.megaverse_env import MegaverseEnv
    assert inspect.signature(ext.MegaverseGym.step_n).parameters["render"].default == "every"
    assert inspect.signature(MegaverseEnv.step_sequence).parameters["render"].default == "every"


@pytest.mark.parametrize("bad", ["all", "", "EVERY", None, 1, ["last"]])
def test_unknown_mode_raises(bad):
    with pytest.raises(ValueError, match="render"):
        ext.render_mode_of(bad)
    for name, mode in ext.RENDER_MODES.items():
        assert ext.render_mode_of(name) == mode


def test_unknown_mode_raises_before_the_library_is_called():
    """step_n checks its render argument first: on an object that holds no gym at all the ValueError is what comes out"""
    g = object.__new__(ext.MegaverseGym)
    with pytest.raises(ValueError, match="render"):
        g.step_n(4, "multidiscrete", 0, 0, render="sometimes")
