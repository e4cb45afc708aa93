"""CPU: the host half of the per-frame resized crop (dreamvla_amd/preprocess.py: draw_resized_crops, resized_crop_u8_reference, the
table store's layout, the argument checks of resized_crop_u8 / resized_crop).  The reference restates Pillow's integer arithmetic,
so it must agree with Pillow's crop -> resize(BICUBIC) -> transpose(FLIP_LEFT_RIGHT) on EVERY byte: no tolerance.  The kernel itself
is tested against Pillow on the GPU (tests/test_resized_crop_gpu.py)."""
import math

import numpy as np
import pytest
import torch

from dreamvla_amd import preprocess as P
from tests.resize_cases import frames
from tests.resized_crop_cases import SOURCES, crops_for, edge_crops, pillow_crops


@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_equals_pillow_byte_for_byte(hw):
    h, w = hw
    crops = crops_for(h, w, 16)
    assert crops.shape == (24, 5) and set(crops[:, 4].tolist()) == {0, 1}
    for kind in ("noise", "extreme"):
        a = frames(h, w, kind, len(crops))
        got = P.resized_crop_u8_reference(a, crops)
        want = pillow_crops(a, crops)
        assert got.shape == want.shape == (24, 224, 224, 3) and got.dtype == np.uint8
        diff = [(i, int((got[i] != want[i]).sum())) for i in range(len(crops)) if (got[i] != want[i]).any()]
        assert not diff, (hw, kind, diff)
    t = P.resized_crop_u8_reference(torch.from_numpy(a[:2]), crops[:2])           # a tensor in, a tensor out
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), want[:2])


def test_reference_other_target_sizes():
    a = frames(200, 200, "noise", 8)
    for n_px in (96, 225):
        crops = torch.tensor(edge_crops(200, 200, n_px), dtype=torch.int32)
        assert np.array_equal(P.resized_crop_u8_reference(a, crops, n_px), pillow_crops(a, crops, n_px))


def test_draw_is_reproducible_and_inside_the_frame():
    h = w = 200
    scale, ratio = (0.2, 1.0), (3.0 / 4.0, 4.0 / 3.0)
    a = P.draw_resized_crops(4096, h, w, generator=torch.Generator().manual_seed(5))
    b = P.draw_resized_crops(4096, h, w, generator=torch.Generator().manual_seed(5))
    c = P.draw_resized_crops(4096, h, w, generator=torch.Generator().manual_seed(6))
    assert a.dtype == torch.int32 and a.shape == (4096, 5) and not a.is_cuda
    assert torch.equal(a, b) and not torch.equal(a, c)
    top, left, ch, cw, flip = a.to(torch.float64).unbind(1)
    assert bool(((top >= 0) & (left >= 0) & (ch >= 1) & (cw >= 1) & (top + ch <= h) & (left + cw <= w)).all())
    # a side is round(x) of the real-valued side x the attempt drew, so x lies in [side - 1/2, side + 1/2]: the drawn area share lies
    # in [(ch - 1/2)(cw - 1/2), (ch + 1/2)(cw + 1/2)] / (h w) and the drawn ratio in [(cw - 1/2) / (ch + 1/2), (cw + 1/2) / (ch - 1/2)];
    # each interval must meet the range it was drawn from (the fallback -- the whole frame here -- is inside both as it is)
    assert bool(((ch + 0.5) * (cw + 0.5) / (h * w) >= scale[0]).all()) and bool(((ch - 0.5) * (cw - 0.5) / (h * w) <= scale[1]).all())
    assert bool(((cw + 0.5) / (ch - 0.5) >= ratio[0]).all()) and bool(((cw - 0.5) / (ch + 0.5) <= ratio[1]).all())
    assert len(set(map(tuple, a[:, :4].tolist()))) > 3000                          # boxes differ from frame to frame
    assert 0.45 <= float(flip.mean()) <= 0.55                                      # binomial standard deviation 0.008 at n = 4096
    assert set(flip.tolist()) == {0.0, 1.0}
    assert not P.draw_resized_crops(512, h, w, p_flip=0.0, generator=torch.Generator().manual_seed(1))[:, 4].any()
    assert P.draw_resized_crops(512, h, w, p_flip=1.0, generator=torch.Generator().manual_seed(1))[:, 4].all()
    # offsets reach both borders
    assert int(a[:, 0].min()) == 0 and int(a[:, 1].min()) == 0 and int((a[:, 0] + a[:, 2]).max()) == h and int((a[:, 1] + a[:, 3]).max()) == w


def test_draw_falls_back_to_the_central_crop():
    # no attempt fits a 10 x 1000 frame at 90 % of its area and a ratio of at most 4/3: full height, cw = round(10 * 4/3), centred
    a = P.draw_resized_crops(64, 10, 1000, scale=(0.9, 1.0), generator=torch.Generator().manual_seed(0))
    assert a[:, :4].tolist() == [[0, 493, 10, 13]] * 64
    # the transposed frame: full width, ch = round(10 / (3/4)), centred
    a = P.draw_resized_crops(64, 1000, 10, scale=(0.9, 1.0), generator=torch.Generator().manual_seed(0))
    assert a[:, :4].tolist() == [[493, 0, 13, 10]] * 64
    # a ratio inside the range: the whole frame
    a = P.draw_resized_crops(8, 30, 30, scale=(4.0, 5.0), generator=torch.Generator().manual_seed(0))
    assert a[:, :4].tolist() == [[0, 0, 30, 30]] * 8
    assert P.draw_resized_crops(0, 30, 30).shape == (0, 5)


def test_table_store_layout():
    """the directory and the tables behind it, as csrc/image_resized_crop.hip reads them"""
    n_px, max_size = 16, 40
    store = P._pack_crop_tables(max_size, n_px)
    assert store.dtype == np.int32 and store[0] == 0 and store[1] == 0
    end = 2 * (max_size + 1)
    for s in range(1, max_size + 1):
        off, ks = int(store[2 * s]), int(store[2 * s + 1])
        bounds, kk = P._axis_tables(s, n_px)
        assert off % 2 == 0 and off >= end and ks == kk.shape[1] == (1 if s == n_px else 2 * math.ceil(2.0 * max(s / n_px, 1.0)) + 1)
        assert np.array_equal(store[off:off + 2 * n_px].reshape(n_px, 2), bounds)
        assert np.array_equal(store[off + 2 * n_px:off + 2 * n_px + n_px * ks].reshape(n_px, ks), kk)
        first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (first >= 0).all() and (count >= 1).all() and (count <= ks).all() and (first + count <= s).all()
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()       # the kernel's tile bounds rely on it
        end = off + 2 * n_px + n_px * ks
    assert end <= store.size <= end + 1


def test_device_entry_is_bound_and_arguments_are_checked_before_any_launch():
    from dreamvla_amd import _lib
    from dreamvla_amd.vit_mae import MAEFrameAugment
    assert "dvla_image_resized_crop" in _lib.SYMBOLS and _lib.ABI_VERSION == 9
    f = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    good = torch.tensor([[0, 0, 20, 30, 0], [3, 4, 5, 6, 1]], dtype=torch.int32)
    for fn in (P.resized_crop_u8, P.resized_crop):
        with pytest.raises(_lib.DvlaError):                    # no CPU fallback
            fn(f, good)
        with pytest.raises(TypeError):
            fn(f.float(), good)
        with pytest.raises(TypeError):
            fn(f, good.float())
        with pytest.raises(TypeError):
            fn(f, good.tolist())
        for bad in ([[0, 0, 21, 30, 0], [0, 0, 1, 1, 0]],      # a box below the frame
                    [[0, 1, 20, 30, 0], [0, 0, 1, 1, 0]],      # a box right of the frame
                    [[-1, 0, 5, 5, 0], [0, 0, 1, 1, 0]],
                    [[0, -1, 5, 5, 0], [0, 0, 1, 1, 0]],
                    [[0, 0, 0, 5, 0], [0, 0, 1, 1, 0]],        # zero size
                    [[0, 0, 5, 0, 0], [0, 0, 1, 1, 0]],
                    [[0, 0, 5, 5, 2], [0, 0, 1, 1, 0]],        # flip = 2
                    [[0, 0, 5, 5, -1], [0, 0, 1, 1, 0]],
                    [[0, 0, 5, 5, 0]],                         # one row for two frames
                    [[0, 0, 5, 5], [0, 0, 1, 1]]):             # four columns
            with pytest.raises(ValueError):
                fn(f, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError):
        P.resized_crop(f, good, n_px=225)                      # the bf16 kind stores 8 pixels at a time
    with pytest.raises(_lib.DvlaError):
        MAEFrameAugment()(f)
    with pytest.raises(ValueError):
        P.resized_crop_u8_reference(f.numpy(), [[0, 0, 21, 30, 0], [0, 0, 1, 1, 0]])
