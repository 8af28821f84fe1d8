"""CPU: the observation-layout call (include/megaverse_hip.h: mv_set_obs_layout) is exported, bound in both Python flavours, and fails cleanly
without a gym or a device."""


def test_obs_layout_symbols_are_exported_and_bound():
    import megaverse_amd.extension as ext
    lib = ext.load_library()
    bound = {n: (res, args) for n, res, args in ext.SYMBOLS}
    for name in ("mv_set_obs_layout", "mv_get_obs_layout"):
        assert hasattr(lib, name), f"{name} not exported"
        assert name in bound, f"{name} missing from megaverse_amd.extension.SYMBOLS"
    assert len(bound["mv_set_obs_layout"][1]) == 2
    assert callable(getattr(ext.MegaverseGym, "set_obs_layout", None))
    assert callable(getattr(ext.MegaverseGym, "obs_layout", None))


def test_obs_layout_without_a_gym_fails_cleanly():
    import megaverse_amd.extension as ext
    lib = ext.load_library()
    assert lib.mv_set_obs_layout(None, 1) < 0
    assert lib.mv_last_error()
    assert lib.mv_set_obs_layout(None, 0) < 0
    assert lib.mv_get_obs_layout(None) == -1


def test_obs_layout_is_in_the_pybind_extras():
    from megaverse_amd import build
    build.build_pybind()
    from megaverse_amd.pybind import megaverse as m
    assert hasattr(m.MegaverseGym, "set_obs_layout")
    assert hasattr(m.MegaverseGym, "obs_layout")


def test_layout_keyword_is_checked_before_any_device_work():
    import pytest
    from megaverse_amd.megaverse_env import MegaverseEnv
    from megaverse_amd.multitask import MultiTaskGym
    with pytest.raises(ValueError, match="obs_layout"):
        MegaverseEnv("TowerBuilding", 1, 1, obs_layout="hwc3")
    with pytest.raises(ValueError, match="obs_layout"):
        MultiTaskGym(["TowerBuilding"], 64, 64, 1, 1, obs_layout="nhwc")


def test_header_documents_the_two_layouts():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "megaverse_hip.h")).read()
    assert "MV_OBS_RGBA = 0" in text and "MV_OBS_RGB_PLANAR = 1" in text
