"""CPU: the host half of the device resize (dreamvla_amd/preprocess.py: bicubic_tables, resize_u8_reference, resize_frames_u8's
argument checks).  Pillow resamples 8-bit images in integer arithmetic on float64-built tables, so the restatement must agree
with `clip_image_resize_u8` (Pillow) on EVERY byte: no tolerance, no allowed share of mismatches.  The kernel itself is tested
against Pillow on the GPU (tests/test_image_resize_gpu.py)."""
import numpy as np
import pytest
import torch

from dreamvla_amd import preprocess as P
from tests.resize_cases import CONTENTS, SIZES, frames, pillow


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_equals_pillow_byte_for_byte(hw):
    h, w = hw
    for kind in CONTENTS:
        a = frames(h, w, kind, 2)
        got = P.resize_u8_reference(a)
        want = pillow(a)
        assert got.shape == want.shape == (2, 224, 224, 3) and got.dtype == np.uint8
        assert int((got != want).sum()) == 0, (hw, kind, int((got != want).sum()))
    # a tensor in, a tensor out; one frame without a batch axis
    t = P.resize_u8_reference(torch.from_numpy(a[0]))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), want[0])


def test_reference_other_target_size():
    a = frames(200, 200, "noise", 1) [0]
    for n_px in (96, 225):           # 225: rows of 675 bytes, not a multiple of 16
        assert np.array_equal(P.resize_u8_reference(a, n_px), P.clip_image_resize_u8(a, n_px))


@pytest.mark.parametrize("pair", [(200, 224), (84, 224), (128, 224), (256, 224), (640, 298), (1280, 398), (300, 298), (720, 224)],
                         ids=lambda p: f"{p[0]}to{p[1]}")
def test_bicubic_tables(pair):
    insz, outsz = pair
    bounds, kk = P.bicubic_tables(insz, outsz)
    scale = max(insz / outsz, 1.0)
    ksize = int(np.ceil(2.0 * scale)) * 2 + 1
    assert bounds.shape == (outsz, 2) and kk.shape == (outsz, ksize) and bounds.dtype == kk.dtype == np.int32
    if pair in ((200, 224), (84, 224)):
        assert ksize == 5
    first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= insz).all()
    assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()           # the kernel's tile bounds rely on it
    # the normalised float64 taps sum to 1; each is rounded to the nearest multiple of 2^-22 (half an ulp each)
    assert (np.abs(kk.astype(np.int64).sum(axis=1) - (1 << 22)) <= 0.5 * count + 1e-6).all()
    assert all(not kk[i, count[i]:].any() for i in range(outsz))                          # nothing behind the tap count
    assert P.bicubic_tables(insz, outsz)[1] is kk                                         # cached per size pair


def test_device_entry_is_bound_and_has_no_cpu_fallback():
    from dreamvla_amd import _lib
    assert "dvla_image_resize_u8" in _lib.SYMBOLS and _lib.ABI_VERSION == 9
    with pytest.raises(_lib.DvlaError):
        P.resize_frames_u8(torch.zeros(1, 200, 200, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        P.resize_frames_u8(torch.zeros(1, 200, 200, 3))


def test_collator_refuses_mixed_frame_sizes():
    from dreamvla_amd.collate import DeviceCollator
    from tests.collate_samples import CASES, fake_tokenize, make_samples
    smp = make_samples(CASES[0])
    col = DeviceCollator(fake_tokenize, window_size=4, device="cpu", device_resize=True)
    raw = col._raw_frames_u8(smp, "rgb_static")
    assert raw.shape == (2, 4, 200, 200, 3) and raw.dtype == torch.uint8
    assert np.array_equal(raw[1, 2].numpy(), np.asarray(smp[1]["rgb_obs"]["rgb_static"][2]))
    smp[1]["rgb_obs"]["rgb_static"][2] = smp[1]["rgb_obs"]["rgb_gripper"][0]           # an 84 x 84 frame among 200 x 200 ones
    with pytest.raises(ValueError, match="one size"):
        col._raw_frames_u8(smp, "rgb_static")
