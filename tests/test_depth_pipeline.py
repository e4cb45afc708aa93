"""CPU: the addressing rule of the depth label kernel (csrc/depth_pipeline.hip) pinned on the host.  `depth_resize_reference` is the
kernel's mirror written as integer indexing; here it is held against what the collator does today -- `collate.depth_image_fn`
(F.interpolate(mode="nearest")) and, with shifts, `shift_gather_reference` on top of it -- bit for bit: a gather moves values, so
the only thing that can differ is WHICH source pixel an output pixel takes, and any difference is a wrong index.
tests/test_depth_pipeline_gpu.py then holds the kernel against `depth_resize_reference`."""
import pytest
import torch

from dreamvla_amd import preprocess as P
from dreamvla_amd.collate import depth_image_fn
from tests.depth_cases import bits, depth_maps, shift_rows

# (h, w) -> size: CALVIN's two cameras, the identity, the exact 2x shortcut of ATen's index, a non-square downscale, tiny maps
# (every output index clamps or repeats) and a single pixel; 15 / 16 are the targets of the GPU test's small cases
RESIZES = [((200, 200), 224), ((84, 84), 224), ((224, 224), 224), ((448, 448), 224), ((225, 300), 224), ((3, 5), 224), ((7, 7), 224),
           ((1, 1), 224), ((200, 200), 15), ((200, 200), 16), ((5, 7), 15), ((5, 7), 16)]


def _interpolate(d, size):
    return depth_image_fn([m.numpy() for m in d], size)                 # (n, 1, size, size) fp32, the collator's own call


@pytest.mark.parametrize("hw,size", RESIZES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"to{v}")
def test_reference_equals_interpolate_nearest(hw, size):
    d = depth_maps(3, *hw, seed=1)
    got, want = P.depth_resize_reference(d, size=size), _interpolate(d, size)
    assert got.shape == want.shape == (3, 1, size, size) and got.dtype == torch.float32
    assert torch.equal(bits(got), bits(want))
    # pad without shifts and shifts without pad are the plain resize
    assert torch.equal(bits(P.depth_resize_reference(d, None, 10, size)), bits(want))
    assert torch.equal(bits(P.depth_resize_reference(d, shift_rows(3, 4), 0, size)), bits(want))


@pytest.mark.parametrize("pad", [10, 4])
@pytest.mark.parametrize("hw,size", [((200, 200), 224), ((84, 84), 224), ((5, 7), 15), ((5, 7), 16), ((225, 300), 224)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"to{v}")
def test_reference_with_shifts_equals_shift_gather_of_interpolate(hw, size, pad):
    n = 7
    d = depth_maps(n, *hw, seed=2)
    sh = shift_rows(n, pad, seed=pad)
    assert sh[:4].tolist() == [[0, 0], [2 * pad, 2 * pad], [0, 2 * pad], [2 * pad, 0]]
    sh[4] = pad                                                        # the centred row: no displacement
    got = P.depth_resize_reference(d, sh, pad, size)
    want = P.shift_gather_reference(_interpolate(d, size), sh, pad)
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(got), bits(_interpolate(d, size)))     # the shifts did move something


def test_test_data_holds_the_values_it_promises():
    d = depth_maps(2, 200, 200, seed=1)
    u = d.view(torch.int32)
    assert bool((d == 0).any()) and bool(torch.isinf(d).any()) and not bool(torch.isnan(d).any())
    assert bool(((u & 0x7F800000) == 0).logical_and((u & 0x007FFFFF) != 0).any())                     # denormals
    tie = (u & 0xFFFF) == 0x8000
    assert bool((tie & ((u >> 16) & 1 == 0)).any()) and bool((tie & ((u >> 16) & 1 == 1)).any())      # ties to even, both ways


def test_symbol_and_abi_version():
    from dreamvla_amd import _lib
    assert "dvla_depth_preprocess" in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 9
    assert callable(P.preprocess_depth)


def test_preprocess_depth_has_no_cpu_fallback():
    from dreamvla_amd import _lib
    with pytest.raises(_lib.DvlaError):
        P.preprocess_depth(torch.zeros(1, 5, 7))
    with pytest.raises(TypeError):
        P.preprocess_depth(torch.zeros(1, 5, 7, dtype=torch.float64))


def test_collator_refuses_device_labels_without_a_device():
    from dreamvla_amd.collate import DeviceCollator
    from tests.collate_samples import fake_tokenize
    with pytest.raises(ValueError):
        DeviceCollator(fake_tokenize, window_size=4, device="cpu", device_labels=True)
    with pytest.raises(ValueError):
        DeviceCollator(fake_tokenize, window_size=4, device_labels=True, label_dtype=torch.float16)
    col = DeviceCollator(fake_tokenize, window_size=4, device="cpu")
    assert col.device_labels is False
