"""The tensor checks of the five observation streams (check_state_obs, check_scene_obs, check_entity_obs, check_depth_obs, check_seg_obs), text for text: every
way a tensor can be wrong, fed as an attribute-only stand-in (no torch, no device), against the full ValueError text.  EXPECTED holds the texts the checks
gave before they were folded onto one helper; they are literals, not derived from the code under test."""
import pytest

from megaverse_amd import extension
from megaverse_amd.extension import MV_DEPTH_F16, MV_DEPTH_F32, MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16


class FakeTensor:
    """what the checks ask of a tensor, with no device behind it"""

    def __init__(self, shape, dtype, is_cuda=True, contiguous=True, index=0):
        self.shape, self.dtype, self.is_cuda, self._contiguous = shape, dtype, is_cuda, contiguous
        self.device = type("D", (), {"index": index, "__str__": lambda s: f"cuda:{index}" if is_cuda else "cpu"})()

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return 0


class NoPointer:
    """a right tensor in every attribute, but without data_ptr"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.is_cuda, self.device = shape, dtype, True, "cuda:0"

    def is_contiguous(self):
        return True


# variant -> (the check, its arguments between `entries` and `device`, the shape of a right tensor behind its entries, its dtype)
VARIANTS = {
    "state": (extension.check_state_obs, (6,), (6, 16), "torch.float32"),
    "scene": (extension.check_scene_obs, (3,), (3, 32), "torch.float32"),
    "entity": (extension.check_entity_obs, (3, 178), (3, 178, 8), "torch.float32"),
    "depth-f32": (extension.check_depth_obs, (6, 36, 64, MV_DEPTH_F32), (6, 36, 64), "torch.float32"),
    "depth-f16": (extension.check_depth_obs, (6, 36, 64, MV_DEPTH_F16), (6, 36, 64), "torch.float16"),
    "seg-class": (extension.check_seg_obs, (6, 36, 64, MV_SEG_CLASS_U8), (6, 36, 64), "torch.uint8"),
    "seg-instance": (extension.check_seg_obs, (6, 36, 64, MV_SEG_INSTANCE_U16), (6, 36, 64), "torch.int16"),
}
ENTRIES = 2
# kind -> (the stand-in from (tail, dtype), the `entries` argument): each wrong in one way
KINDS = {
    "shape": (lambda tail, dtype: FakeTensor((ENTRIES,) + tail[:-1] + (tail[-1] + 1,), dtype), ENTRIES),
    "entries": (lambda tail, dtype: FakeTensor((ENTRIES + 1,) + tail, dtype), ENTRIES),
    "dtype": (lambda tail, dtype: FakeTensor((ENTRIES,) + tail, "torch.float64"), ENTRIES),
    "other-device": (lambda tail, dtype: FakeTensor((ENTRIES,) + tail, dtype, index=1), ENTRIES),
    "strided": (lambda tail, dtype: FakeTensor((ENTRIES,) + tail, dtype, contiguous=False), ENTRIES),
    "cpu": (lambda tail, dtype: FakeTensor((ENTRIES,) + tail, dtype, is_cuda=False, index=None), ENTRIES),
    "no-data-ptr": (lambda tail, dtype: NoPointer((ENTRIES,) + tail, dtype), ENTRIES),
    "any-entries-rank": (lambda tail, dtype: FakeTensor(tail, dtype), None),
    "any-entries-tail": (lambda tail, dtype: FakeTensor((5,) + (tail[0] + 1,) + tail[1:], dtype), None),
}

EXPECTED = {
    ('state', 'shape'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float32 (2, 6, 17) on cuda:0',
    ('state', 'entries'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float32 (3, 6, 16) on cuda:0',
    ('state', 'dtype'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float64 (2, 6, 16) on cuda:0',
    ('state', 'other-device'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float32 (2, 6, 16) on cuda:1',
    ('state', 'strided'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float32 (2, 6, 16) on cuda:0',
    ('state', 'cpu'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float32 (2, 6, 16) on cpu',
    ('state', 'no-data-ptr'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 16) on device 0, got torch.float32 (2, 6, 16) on cuda:0',
    ('state', 'any-entries-rank'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (1, 6, 16) on device 0, got torch.float32 (6, 16) on cuda:0',
    ('state', 'any-entries-tail'):
        'set_state_obs: the buffer must be a contiguous float32 CUDA tensor of shape (5, 6, 16) on device 0, got torch.float32 (5, 7, 16) on cuda:0',
    ('scene', 'shape'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float32 (2, 3, 33) on cuda:0',
    ('scene', 'entries'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float32 (3, 3, 32) on cuda:0',
    ('scene', 'dtype'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float64 (2, 3, 32) on cuda:0',
    ('scene', 'other-device'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float32 (2, 3, 32) on cuda:1',
    ('scene', 'strided'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float32 (2, 3, 32) on cuda:0',
    ('scene', 'cpu'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float32 (2, 3, 32) on cpu',
    ('scene', 'no-data-ptr'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 32) on device 0, got torch.float32 (2, 3, 32) on cuda:0',
    ('scene', 'any-entries-rank'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (1, 3, 32) on device 0, got torch.float32 (3, 32) on cuda:0',
    ('scene', 'any-entries-tail'):
        'set_scene_obs: the buffer must be a contiguous float32 CUDA tensor of shape (5, 3, 32) on device 0, got torch.float32 (5, 4, 32) on cuda:0',
    ('entity', 'shape'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float32 (2, 3, 178, 9) on cuda:0',
    ('entity', 'entries'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float32 (3, 3, 178, 8) on cuda:0',
    ('entity', 'dtype'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float64 (2, 3, 178, 8) on cuda:0',
    ('entity', 'other-device'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float32 (2, 3, 178, 8) on cuda:1',
    ('entity', 'strided'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float32 (2, 3, 178, 8) on cuda:0',
    ('entity', 'cpu'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float32 (2, 3, 178, 8) on cpu',
    ('entity', 'no-data-ptr'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 3, 178, 8) on device 0, got torch.float32 (2, 3, 178, 8) on cuda:0',
    ('entity', 'any-entries-rank'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (1, 3, 178, 8) on device 0, got torch.float32 (3, 178, 8) on cuda:0',
    ('entity', 'any-entries-tail'):
        'set_entity_obs: the buffer must be a contiguous float32 CUDA tensor of shape (5, 3, 178, 8) on device 0, got torch.float32 (5, 4, 178, 8) on cuda:0',
    ('depth-f32', 'shape'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float32 (2, 6, 36, 65) on cuda:0',
    ('depth-f32', 'entries'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float32 (3, 6, 36, 64) on cuda:0',
    ('depth-f32', 'dtype'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float64 (2, 6, 36, 64) on cuda:0',
    ('depth-f32', 'other-device'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float32 (2, 6, 36, 64) on cuda:1',
    ('depth-f32', 'strided'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float32 (2, 6, 36, 64) on cuda:0',
    ('depth-f32', 'cpu'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float32 (2, 6, 36, 64) on cpu',
    ('depth-f32', 'no-data-ptr'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float32 (2, 6, 36, 64) on cuda:0',
    ('depth-f32', 'any-entries-rank'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (1, 6, 36, 64) on device 0, got torch.float32 (6, 36, 64) on cuda:0',
    ('depth-f32', 'any-entries-tail'):
        'set_depth_obs: the buffer must be a contiguous float32 CUDA tensor of shape (5, 6, 36, 64) on device 0, got torch.float32 (5, 7, 36, 64) on cuda:0',
    ('depth-f16', 'shape'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float16 (2, 6, 36, 65) on cuda:0',
    ('depth-f16', 'entries'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float16 (3, 6, 36, 64) on cuda:0',
    ('depth-f16', 'dtype'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float64 (2, 6, 36, 64) on cuda:0',
    ('depth-f16', 'other-device'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float16 (2, 6, 36, 64) on cuda:1',
    ('depth-f16', 'strided'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float16 (2, 6, 36, 64) on cuda:0',
    ('depth-f16', 'cpu'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float16 (2, 6, 36, 64) on cpu',
    ('depth-f16', 'no-data-ptr'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float16 (2, 6, 36, 64) on cuda:0',
    ('depth-f16', 'any-entries-rank'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (1, 6, 36, 64) on device 0, got torch.float16 (6, 36, 64) on cuda:0',
    ('depth-f16', 'any-entries-tail'):
        'set_depth_obs: the buffer must be a contiguous float16 CUDA tensor of shape (5, 6, 36, 64) on device 0, got torch.float16 (5, 7, 36, 64) on cuda:0',
    ('seg-class', 'shape'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.uint8 (2, 6, 36, 65) on cuda:0',
    ('seg-class', 'entries'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.uint8 (3, 6, 36, 64) on cuda:0',
    ('seg-class', 'dtype'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float64 (2, 6, 36, 64) on cuda:0',
    ('seg-class', 'other-device'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.uint8 (2, 6, 36, 64) on cuda:1',
    ('seg-class', 'strided'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.uint8 (2, 6, 36, 64) on cuda:0',
    ('seg-class', 'cpu'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.uint8 (2, 6, 36, 64) on cpu',
    ('seg-class', 'no-data-ptr'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.uint8 (2, 6, 36, 64) on cuda:0',
    ('seg-class', 'any-entries-rank'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (1, 6, 36, 64) on device 0, got torch.uint8 (6, 36, 64) on cuda:0',
    ('seg-class', 'any-entries-tail'):
        'set_seg_obs: the buffer must be a contiguous uint8 CUDA tensor of shape (5, 6, 36, 64) on device 0, got torch.uint8 (5, 7, 36, 64) on cuda:0',
    ('seg-instance', 'shape'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.int16 (2, 6, 36, 65) on cuda:0',
    ('seg-instance', 'entries'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.int16 (3, 6, 36, 64) on cuda:0',
    ('seg-instance', 'dtype'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.float64 (2, 6, 36, 64) on cuda:0',
    ('seg-instance', 'other-device'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.int16 (2, 6, 36, 64) on cuda:1',
    ('seg-instance', 'strided'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.int16 (2, 6, 36, 64) on cuda:0',
    ('seg-instance', 'cpu'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.int16 (2, 6, 36, 64) on cpu',
    ('seg-instance', 'no-data-ptr'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (2, 6, 36, 64) on device 0, got torch.int16 (2, 6, 36, 64) on cuda:0',
    ('seg-instance', 'any-entries-rank'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (1, 6, 36, 64) on device 0, got torch.int16 (6, 36, 64) on cuda:0',
    ('seg-instance', 'any-entries-tail'):
        'set_seg_obs: the buffer must be a contiguous int16 / uint16 CUDA tensor of shape (5, 6, 36, 64) on device 0, got torch.int16 (5, 7, 36, 64) on cuda:0',
}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_wrong_tensor_text(variant, kind):
    """one stand-in, wrong in one way: the check's ValueError, character for character"""
    check, args, tail, dtype = VARIANTS[variant]
    make, entries = KINDS[kind]
    with pytest.raises(ValueError) as e:
        check(make(tail, dtype), entries, *args, 0)
    assert str(e.value) == EXPECTED[variant, kind]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_right_tensor_is_returned_unchanged(variant):
    """a right stand-in comes back as it is, with the entry count given and with any (entries None); an 'instance' label plane may be uint16 too"""
    check, args, tail, dtype = VARIANTS[variant]
    for dt in (dtype, "torch.uint16") if variant == "seg-instance" else (dtype,):
        for shape, entries in (((ENTRIES,) + tail, ENTRIES), ((7,) + tail, None)):
            good = FakeTensor(shape, dt)
            before = dict(vars(good))
            assert check(good, entries, *args, 0) is good and vars(good) == before
