"""The helpers of the GEMM addressing checks (tests/gpu_checks.py make_view / window_mask / outside_window_intact) on the CPU: the
view builder yields the stride, origin and alignment it is asked for, and the sentinel check sees a single foreign element
anywhere outside the window -- a check that could not fail would make tests/test_gemm_addressing_gpu.py worthless."""
import pytest
import torch

from tests import gpu_checks as G


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("pad,offset", [(0, 0), (8, 8), (24, 16), (5, 0), (0, 1), (3, 7)])
def test_view_builder_yields_the_requested_stride_origin_and_alignment(dtype, pad, offset):
    rows, cols = 7, 40
    backing, view = G.make_view(rows, cols, pad, offset, dtype)
    assert view.shape == (rows, cols) and view.stride() == (cols + pad, 1)
    origin = view.storage_offset()
    assert origin >= 2 * (cols + pad) + offset                           # rows of the buffer in front of the window
    assert (origin - offset) % 64 == 0                                    # `offset` elements behind a 128-byte boundary
    assert backing.numel() >= origin + (rows + 2) * (cols + pad)          # ... and behind it
    vec = 16 // backing.element_size()
    assert ((view.data_ptr() - backing.data_ptr()) % 16 == 0) == (offset % vec == 0)
    assert view.data_ptr() == backing.data_ptr() + origin * backing.element_size()
    # every element is the sentinel, bit for bit; the mask covers exactly the window
    assert G.outside_window_intact(backing, None)["ok"]
    mask = G.window_mask(backing, view)
    assert int(mask.sum()) == rows * cols
    view.fill_(1.0)
    assert bool((backing[mask] == 1.0).all()) and bool((backing[~mask] == G.VIEW_SENTINEL).all())
    assert G.outside_window_intact(backing, view)["ok"]                   # writes inside the window are not reported


def test_bias_view_is_one_row():
    backing, view = G.make_view(1, 96, 0, 8, torch.float32)
    assert view[0].shape == (96,) and view[0].data_ptr() % 16 == backing.data_ptr() % 16
    assert int(G.window_mask(backing, view).sum()) == 96


WHERE = {"row before the window": lambda o, ld, rows, cols: o - ld,
         "element left of the origin": lambda o, ld, rows, cols: o - 1,
         "first padding column of row 0": lambda o, ld, rows, cols: o + cols,
         "last padding column of a middle row": lambda o, ld, rows, cols: o + 3 * ld + ld - 1,
         "element right of the last row": lambda o, ld, rows, cols: o + (rows - 1) * ld + cols,
         "row after the window": lambda o, ld, rows, cols: o + rows * ld + 2,
         "first element of the buffer": lambda o, ld, rows, cols: 0,
         "last element of the buffer": lambda o, ld, rows, cols: -1}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("where", sorted(WHERE))
def test_sentinel_check_sees_one_planted_element(where, dtype):
    rows, cols, pad = 6, 24, 8
    backing, view = G.make_view(rows, cols, pad, 8, dtype)
    view.copy_(torch.randn(rows, cols).to(dtype))
    assert G.outside_window_intact(backing, view)["ok"]
    at = WHERE[where](view.storage_offset(), cols + pad, rows, cols) % backing.numel()
    assert not bool(G.window_mask(backing, view)[at])
    backing[at] = 0.5
    s = G.outside_window_intact(backing, view)
    assert not s["ok"] and s["bad"] == 1 and s["first_bad"] == at


def test_sentinel_check_is_bitwise():
    """a value that compares equal to the sentinel but has other bits cannot exist for a finite non-zero sentinel; a zero or a NaN
    planted outside the window must be reported as well"""
    for planted in (0.0, -0.0, float("nan"), float("inf"), -6.6875):
        backing, view = G.make_view(4, 16, 8, 0, torch.bfloat16)
        backing[view.storage_offset() + 16] = planted
        assert not G.outside_window_intact(backing, view)["ok"], planted


def test_wide_stride_is_the_smallest_vector_stride_past_4_gib():
    s = G.WIDE_OUT_STRIDE
    assert s % 8 == 0 and (G.WINDOW_ROWS - 1) * s * 2 >= 1 << 32 and (G.WINDOW_ROWS - 1) * (s - 8) * 2 < 1 << 32
    assert s == 16_909_328
