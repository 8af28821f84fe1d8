"""Draw masks without a device: the ABI, the Python argument checks, the refusals that need no gym."""
import os
import re

import numpy as np
import pytest

from megaverse_amd import extension
from megaverse_amd.extension import check_draw_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    """1. the three calls: declared in the header, exported by the library, bound with the declared arity; the ABI version stays 2 (additive)"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)
    lib = extension.load_library()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    for name, arity in (("mv_set_draw_mask", 2), ("mv_set_draw_mask_host", 2), ("mv_get_draw_mask", 1)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == arity
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound and len(bound[name][1]) == arity
    assert lib.mv_abi_version() == 2


def test_mask_argument_check():
    """2. check_step_mask's rules under set_draw_mask's name: None, sequences and numpy arrays; a wrong shape or dtype is a ValueError"""
    assert check_draw_mask(None, 3) is None
    m = check_draw_mask([True, False, True], 3)
    assert m.dtype == np.uint8 and m.tolist() == [1, 0, 1] and m.flags.c_contiguous
    assert check_draw_mask(np.array([0, 2, 255], np.uint8), 3).tolist() == [0, 1, 1]
    assert check_draw_mask(np.zeros(3, np.bool_), 3).tolist() == [0, 0, 0]
    assert check_draw_mask(np.array([1, 0, 1, 0, 1, 0], np.bool_)[::2], 3).tolist() == [1, 1, 1]   # (a strided numpy mask is copied)
    for bad in ([True, False], np.zeros((3, 1), np.bool_), np.zeros(3, np.int32), np.zeros(3, np.float32), [0.5, 0.0, 1.0], np.zeros(3, np.uint16)):
        with pytest.raises(ValueError, match="set_draw_mask"):
            check_draw_mask(bad, 3)


class FakeTensor:
    """what _check_env_mask asks of a tensor, with no device behind it; data_ptr() records that nobody asked for it"""

    def __init__(self, shape=(3,), dtype="torch.bool", is_cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous, self.device, self.asked = shape, dtype, is_cuda, contiguous, "cuda:0", 0

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        self.asked += 1
        return 0


class RaisingLib:
    """a library whose every call fails the test: set_draw_mask must raise before it reaches one"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


@pytest.mark.parametrize("bad", [FakeTensor(shape=(4,)), FakeTensor(shape=(3, 1)), FakeTensor(dtype="torch.int32"), FakeTensor(dtype="torch.float32"),
                                 FakeTensor(contiguous=False), FakeTensor(is_cuda=False)],
                         ids=["length", "rank", "int32", "float32", "strided", "cpu"])
def test_tensor_masks_are_checked_before_any_device_call(bad):
    """2. a wrong shape, a wrong dtype, a non-contiguous or a host tensor: ValueError from MegaverseGym.set_draw_mask itself, the library untouched"""
    gym = extension.MegaverseGym.__new__(extension.MegaverseGym)
    gym._lib, gym._g, gym.num_envs, gym._draw_mask_held = RaisingLib(), None, 3, "before"
    with pytest.raises(ValueError, match="set_draw_mask"):
        gym.set_draw_mask(bad)
    assert bad.asked == 0 and gym._draw_mask_held == "before"
    assert check_draw_mask(FakeTensor(), 3) == "device"   # (the right tensor takes the device form)


def test_multitask_refuses_with_text():
    """3. MultiTaskGym.set_draw_mask raises before it touches a device"""
    from megaverse_amd.multitask import MultiTaskGym
    with pytest.raises(RuntimeError, match="mv_set_draw_mask"):
        MultiTaskGym.set_draw_mask(type("G", (), {"_group": None})(), [True])
    with pytest.raises(RuntimeError, match="mv_set_draw_mask"):
        MultiTaskGym.set_draw_mask(type("G", (), {"_group": None})(), None)


def test_no_gym_is_an_error_with_text():
    """4. a null gym: -1 with text, from all three"""
    lib = extension.load_library()
    mask = np.ones(4, np.uint8)
    for fn, args in ((lib.mv_set_draw_mask, (mask.ctypes.data,)), (lib.mv_set_draw_mask_host, (mask.ctypes.data,)), (lib.mv_set_draw_mask, (None,)),
                     (lib.mv_set_draw_mask_host, (None,)), (lib.mv_get_draw_mask, ())):
        assert fn(None, *args) == -1
        assert b"null gym" in lib.mv_last_error() and b"mv_" in lib.mv_last_error() and b"draw_mask" in lib.mv_last_error()


def test_env_draw_only_and_draw_all():
    """the MegaverseEnv surface: draw_only(env_ids) leaves every other env undrawn, draw_all() detaches"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    assert all(hasattr(MegaverseEnv, name) for name in ("set_draw_mask", "draw_only", "draw_all"))
    calls = []
    env = MegaverseEnv.__new__(MegaverseEnv)
    env.num_envs = 6
    env.env = type("G", (), {"set_draw_mask": lambda self, mask: calls.append(None if mask is None else np.asarray(mask).tolist())})()
    env.draw_only([1, 4])
    env.draw_all()
    assert calls == [[False, True, False, False, True, False], None]
    with pytest.raises(ValueError, match="draw_only"):
        env.draw_only([6])
