"""GPU: the depth label kernel (csrc/depth_pipeline.hip: nearest resize + shift gather + cast, one launch) against its host
mirror `preprocess.depth_resize_reference`, which tests/test_depth_pipeline.py pins to F.interpolate(mode="nearest") and
`shift_gather_reference`.

Bounds: the kernel moves values and rounds once -- the fp32 output is the source's bits, the bf16 output the bits of
`reference.to(torch.bfloat16)` (round to nearest even, the data holds ties, denormals and infinities: tests/depth_cases.py) -- so
every comparison is equality of bit patterns; the expected number of differing elements is 0 and nothing else passes.

Shapes: (5, 7) -> 15 and -> 16 (rows of 30 / 60 bytes: the scalar head and tail of every row, and 16 as the aligned all-vector
case; upscaling by non-integer ratios; shifts of up to 2 pad = 20 against a 15-pixel output clamp on all four edges), (84, 84) ->
224 and (200, 200) -> 224 (CALVIN's cameras: 7 row blocks per frame, more than one workgroup), 4 100 frames of (5, 7) -> 16 (more
units of work than the grid's 4 096 workgroups: the stride loop) and 42 900 frames of (1, 2) -> 224 (output element offsets past
2^31)."""
import pytest
import torch

from dreamvla_amd import preprocess as P
from tests.depth_cases import bits, depth_maps, shift_rows

BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(3, (5, 7), 15), (3, (5, 7), 16), (2, (84, 84), 224), (2, (200, 200), 224)]
IDS = ["3x5x7to15", "3x5x7to16", "2x84x84to224", "2x200x200to224"]
GUARD = 1024                     # sentinel elements in front of and behind an output (a multiple of 8: keeps the alignment)
ARG, UNSUPPORTED = -1, -3


def _want(d, sh, pad, size, dtype):
    return P.depth_resize_reference(d, sh, pad, size).to(dtype)


def _shift_sets(n, pad):
    """no shift; rows at both extremes; random rows"""
    g = torch.Generator().manual_seed(n + pad)
    return [("none", None), ("extremes", shift_rows(n, pad, seed=1)), ("max", torch.full((n, 2), 2 * pad, dtype=torch.int32)),
            ("random", torch.randint(0, 2 * pad + 1, (n, 2), generator=g, dtype=torch.int32))]


def _differing(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((bits(got.cpu()) != bits(want)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n,hw,size", SHAPES, ids=IDS)
def test_kernel_equals_reference_bit_for_bit(n, hw, size, dtype):
    d = depth_maps(n, *hw, seed=3)
    dev = d.cuda()
    bad = {}
    for pad in (4, 10):
        for name, sh in _shift_sets(n, pad):
            got = P.preprocess_depth(dev, sh, pad, size, dtype)
            assert got.shape == (n, 1, size, size) and got.dtype == dtype and got.is_cuda
            bad[f"pad{pad}.{name}"] = _differing(got, _want(d, sh, pad, size, dtype))
    bad["pad0.shifts_ignored"] = _differing(P.preprocess_depth(dev, shift_rows(n, 4), 0, size, dtype), _want(d, None, 0, size, dtype))
    print(bad)
    assert not any(bad.values()), bad


def _call(src, sh, out, n, h, w, oh, ow, pad, dt):
    from dreamvla_amd import _lib
    from dreamvla_amd.ops import _stream
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return _lib.load().dvla_depth_preprocess(ptr(src), ptr(sh), ptr(out), n, h, w, oh, ow, pad, dt, _stream())


def _guarded(n, size, dtype, offset):
    """an output of n frames `offset` elements behind a 16-byte boundary, between two NaN-filled sentinel regions"""
    numel = n * size * size
    buf = torch.full((2 * GUARD + numel + 8,), float("nan"), dtype=dtype, device="cuda")
    out = buf[GUARD + offset:GUARD + offset + numel]
    assert out.data_ptr() % 16 == offset * buf.element_size()
    return buf, out


def _sentinels_intact(buf, out):
    first = (out.data_ptr() - buf.data_ptr()) // buf.element_size()
    nan = bits(torch.full((1,), float("nan"), dtype=buf.dtype))[0].item()
    b = bits(buf)
    return bool((b[:first] == nan).all()) and bool((b[first + out.numel():] == nan).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n,hw,size", SHAPES, ids=IDS)
def test_c_abi_on_caller_owned_buffers(n, hw, size, dtype):
    """an output one element (2 / 4 bytes) off a 16-byte boundary and an aligned one: every element written, to the reference's
    bits, nothing outside written, and a second launch gives the same bytes"""
    from dreamvla_amd import _lib
    dt = _lib.DT_BF16 if dtype == BF else _lib.DT_F32
    d = depth_maps(n, *hw, seed=4)
    dev, pad = d.cuda(), 10
    sh = shift_rows(n, pad, seed=2)
    sh_dev = sh.cuda()
    want = _want(d, sh, pad, size, dtype).flatten()
    for offset in (1, 0, 3):
        buf, out = _guarded(n, size, dtype, offset)
        rc = _call(dev, sh_dev, out, n, hw[0], hw[1], size, size, pad, dt)
        torch.cuda.synchronize()
        first = out.clone()
        assert rc == 0
        assert not bool(torch.isnan(first).any())                      # the data holds no NaN: an element still NaN was not written
        assert _differing(first, want) == 0, (offset, _differing(first, want))
        assert _sentinels_intact(buf, out), offset
        rc = _call(dev, sh_dev, out, n, hw[0], hw[1], size, size, pad, dt)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(bits(out), bits(first)) and _sentinels_intact(buf, out)
    # shift == NULL: no shift, whatever pad says
    buf, out = _guarded(n, size, dtype, 1)
    assert _call(dev, None, out, n, hw[0], hw[1], size, size, pad, dt) == 0
    torch.cuda.synchronize()
    assert _differing(out, _want(d, None, 0, size, dtype).flatten()) == 0 and _sentinels_intact(buf, out)


@pytest.mark.gpu
def test_return_codes():
    from dreamvla_amd import _lib
    src = depth_maps(2, 5, 7, seed=5).cuda()
    sh = shift_rows(2, 4).cuda()
    buf, out = _guarded(2, 15, BF, 1)
    base = dict(src=src, sh=sh, out=out, n=2, h=5, w=7, oh=15, ow=15, pad=4, dt=_lib.DT_BF16)
    call = lambda **kw: _call(**{**base, **kw})
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert _sentinels_intact(buf, out) and bool(torch.isnan(out).all())          # n == 0 wrote nothing
    for bad in (dict(src=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(oh=0), dict(ow=-3), dict(pad=-1)):
        assert call(**bad) == ARG, bad
    assert call(src=None, n=0) == ARG                                            # the arguments are checked before n == 0 returns
    for bad in (dict(dt=2), dict(dt=-1)):
        assert call(**bad) == UNSUPPORTED, bad
    assert call(oh=16000, ow=400) == UNSUPPORTED                                 # the index tables no longer fit the LDS plan
    assert call(out=out.data_ptr() + 1) == UNSUPPORTED                           # not aligned to the element
    torch.cuda.synchronize()
    assert _sentinels_intact(buf, out) and bool(torch.isnan(out).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and _sentinels_intact(buf, out)


@pytest.mark.gpu
def test_non_contiguous_input_and_leading_axes():
    big = depth_maps(6, 12, 16, seed=6)
    dev = big.cuda()
    window = dev[:, 3:8, 2:9]                                                     # (5, 7) maps cut out of larger ones
    assert not window.is_contiguous()
    sh = shift_rows(6, 4, seed=3)
    assert _differing(P.preprocess_depth(window, sh, 4, 15), _want(big[:, 3:8, 2:9].contiguous(), sh, 4, 15, BF)) == 0
    every_second = dev[::2]
    assert _differing(P.preprocess_depth(every_second, None, 0, 16, F32), _want(big[::2].contiguous(), None, 0, 16, F32)) == 0
    bt = dev.view(2, 3, 12, 16)                                                   # leading axes are kept
    got = P.preprocess_depth(bt, sh, 4, 15)
    assert got.shape == (2, 3, 1, 15, 15)
    assert _differing(got.view(6, 1, 15, 15), _want(big, sh, 4, 15, BF)) == 0
    assert P.preprocess_depth(dev[:0], None, 0, 15).shape == (0, 1, 15, 15)
    with pytest.raises(TypeError):
        P.preprocess_depth(dev.double())
    with pytest.raises(TypeError):
        P.preprocess_depth(dev, dtype=torch.float16)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_more_units_of_work_than_workgroups(dtype):
    """4 100 frames of one unit each against the grid's cap of 4 096 workgroups: the last frames are reached by the stride loop"""
    n, pad = 4100, 4
    d = depth_maps(n, 5, 7, seed=7)
    g = torch.Generator().manual_seed(11)
    sh = torch.randint(0, 2 * pad + 1, (n, 2), generator=g, dtype=torch.int32)
    assert _differing(P.preprocess_depth(d.cuda(), sh, pad, 16, dtype), _want(d, sh, pad, 16, dtype)) == 0


@pytest.mark.gpu
def test_output_offsets_past_2_31_elements():
    """42 900 frames x 224 x 224 = 2.15e9 output elements (4.3 GB of bf16): the element offsets of the last frames do not fit 32
    bits.  (1, 2) sources: every output row of a frame is the frame's two values spread by the column index table -- compared on
    the device, every element."""
    n = 42900
    assert n * 224 * 224 > 2 ** 31
    g = torch.Generator().manual_seed(13)
    d = torch.rand(n, 1, 2, generator=g) * 5
    out = P.preprocess_depth(d.cuda(), None, 0, 224)
    idx = P.nearest_index(2, 224)
    assert idx.min() == 0 and idx.max() == 1
    want_row = d.to(BF)[:, 0, :][:, idx].cuda()                                   # (n, 224)
    assert bool((out[:, 0] == want_row.view(n, 1, 224)).all())
