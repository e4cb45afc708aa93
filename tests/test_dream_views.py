"""CPU: the references of the dream pictures (tests/dream_view_ref.py) against hand-placed cases and against the training code's own
arithmetic, FeaturePalette.fit, and the surface: symbols, header, ABI version, argument validation.  The kernels themselves are
checked against these references in tests/test_dream_views_gpu.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dream_view_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvla_depth_range_partial_len", "dvla_depth_colorize", "dvla_flow_unshuffle", "dvla_flow_wheel", "dvla_motion_mask",
           "dvla_motion_overlay", "dvla_feature_render"]


# ---------------------------------------------------------------------------------------------------
# the wheel
# ---------------------------------------------------------------------------------------------------
AXES = [((1.0, 0.0), 0, (255, 0, 0)), ((0.0, 1.0), 45, (128, 255, 0)), ((-1.0, 0.0), 90, (0, 255, 255)), ((0.0, -1.0), 135, (128, 0, 255))]


@pytest.mark.parametrize("direction,hue,rgb", AXES)
def test_axis_flows_have_the_reference_hues(direction, hue, rgb):
    flow = np.asarray(direction) * 9.0                                       # 32 * 9 > 255: V saturates
    half, v32 = R.wheel_parts(flow)
    assert int(np.trunc(half)) == hue and v32 >= 255
    assert tuple(R.flow_wheel(flow)) == rgb
    # at half brightness: V = trunc(32 * 4.01) = 128, X = (128 * 15 + 15) // 30 = 64 on the two diagonal hues
    dim = R.flow_wheel(np.asarray(direction) * 4.01)
    want = tuple({255: 128, 128: 64, 0: 0}[c] for c in rgb)
    assert tuple(dim) == want


def test_zero_flow_is_black_and_8_px_saturates():
    assert tuple(R.flow_wheel(np.zeros(2))) == (0, 0, 0)
    for mag in (7.96, 7.97, 8.0, 50.0):
        v = R.flow_wheel(np.asarray([mag, 0.0]))[0]
        assert v == min(int(32 * mag), 255)
    assert R.flow_wheel(np.asarray([8.0, 0.0]))[0] == 255 == R.flow_wheel(np.asarray([7.97, 0.0]))[0]
    assert R.flow_wheel(np.asarray([7.96, 0.0]))[0] == 254


def test_hsv_sextants_are_continuous():
    """neighbouring hues differ by at most ceil(255 / 30) levels per channel: no sextant is wired to the wrong channel"""
    rgb = R.hsv_to_rgb(np.arange(180), np.full(180, 255)).astype(int)
    step = np.abs(np.diff(np.concatenate((rgb, rgb[:1])), axis=0))
    assert step.max() <= 9
    assert (rgb.max(axis=1) == 255).all() and (rgb.min(axis=1) == 0).all()


def test_nearest_map_is_floor_of_the_scaled_index():
    img = np.arange(28 * 28).reshape(1, 28, 28)
    up = R.nearest(img, 30, 30)
    for y in (0, 1, 14, 15, 29):
        for x in (0, 7, 29):
            assert up[0, y, x] == img[0, y * 28 // 30, x * 28 // 30]


# ---------------------------------------------------------------------------------------------------
# unshuffle and the mask against the training code's arithmetic
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,g", [(1, 3), (2, 14), (4, 5)])
def test_unshuffle_reference_is_pixel_shuffle(f, g):
    pred = torch.randn(3, g * g, 2 * f * f, generator=torch.Generator().manual_seed(f))
    want = F.pixel_shuffle(pred.reshape(3, g, g, 2 * f * f).permute(0, 3, 1, 2), f).permute(0, 2, 3, 1)
    assert np.array_equal(R.flow_unshuffle(pred.numpy()), want.numpy())
    # ... and the inverse of losses.calvin_losses' tlab: pixel_unshuffle of the (b, c, h, w) label, tokens row-major
    back = F.pixel_unshuffle(want.permute(0, 3, 1, 2), f).flatten(2).permute(0, 2, 1)
    assert torch.equal(back, pred)


def fmask_restated(flow, dilate):
    """losses.calvin_losses' fmask on a (n, 28, 28, 2) float32 flow -> (n, 14, 14) bool"""
    tp = flow.permute(0, 3, 1, 2)
    m = (torch.norm(F.avg_pool2d(tp, kernel_size=2, stride=2), dim=1) > 1.0).unsqueeze(1).to(torch.float32)
    if dilate:
        m = F.max_pool2d(m, kernel_size=3, stride=1, padding=1)
    return m[:, 0] > 0


@pytest.mark.parametrize("dilate", [False, True])
def test_mask_reference_is_fmask_at_f2(dilate):
    flow = torch.randn(4, 28, 28, 2, generator=torch.Generator().manual_seed(3))     # 13 % of tokens move, 73 % dilated
    pred = F.pixel_unshuffle(flow.permute(0, 3, 1, 2), 2).flatten(2).permute(0, 2, 1).contiguous()
    mask, q = R.motion_mask(pred.numpy(), 1.0, dilate)
    assert np.abs(q - 1.0).min() > 1e-6                                       # no token on the threshold: the comparison is exact
    assert 0.05 < mask.mean() < 0.95
    assert np.array_equal(mask, fmask_restated(flow, dilate).numpy())


def test_dilation_reaches_corners_and_edges_only_inside_the_grid():
    m = np.zeros((1, 5, 5), dtype=bool)
    m[0, 0, 0] = m[0, 2, 4] = True
    d = R.dilate3(m)[0]
    want = np.zeros((5, 5), dtype=bool)
    want[0:2, 0:2] = True
    want[1:4, 3:5] = True
    assert np.array_equal(d, want)


# ---------------------------------------------------------------------------------------------------
# depth level, blend
# ---------------------------------------------------------------------------------------------------
def test_level_restatement_edges():
    f = np.float32
    v = np.asarray([0.0, 1.0, 0.5, -3.0, 7.0, 0.25], dtype=f)
    assert R.level_f32(v, f(0), f(1)).tolist() == [0, 255, 128, 0, 255, 64]    # 127.5 -> 128, 63.75 -> 64
    assert R.level_f32(v, f(2), f(2)).tolist() == [0] * 6                      # hi == lo: index 0, whatever s / 0 is
    assert R.level_f32(np.asarray([2.0], dtype=f), f(2), f(2)).tolist() == [0]


def test_blend_formula():
    frame = np.full((1, 4, 4, 3), 200, dtype=np.uint8)
    mask = np.asarray([[[1, 0], [0, 1]]])
    out = R.blend(frame, mask, (255, 64, 0), 96)
    assert out[0, 0, 0].tolist() == [(200 * 160 + 255 * 96 + 128) >> 8, (200 * 160 + 64 * 96 + 128) >> 8, (200 * 160 + 128) >> 8]
    assert out[0, 0, 2].tolist() == [200, 200, 200] and out[0, 3, 3].tolist() == out[0, 0, 0].tolist()


# ---------------------------------------------------------------------------------------------------
# FeaturePalette
# ---------------------------------------------------------------------------------------------------
def _planted(seed=0, N=4000, D=24):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(D, 3, generator=g, dtype=torch.float64))
    scale = torch.tensor([5.0, 2.0, 0.7], dtype=torch.float64)
    x = (torch.randn(N, 3, generator=g, dtype=torch.float64) * scale) @ q.t() + 1e-3 * torch.randn(N, D, generator=g, dtype=torch.float64)
    return x + torch.randn(D, generator=g, dtype=torch.float64), q


def test_fit_recovers_planted_directions_in_order_with_the_sign_rule():
    from dreamvla_amd.dream_view import FeaturePalette
    x, q = _planted()
    pal = FeaturePalette.fit(x)
    cos = (pal.components @ q).abs()                                            # (3 fitted, 3 planted)
    assert torch.all(cos.diagonal() > 0.995), cos                               # descending eigenvalue = descending planted scale
    big = pal.components.abs().argmax(dim=1)
    assert torch.all(pal.components[torch.arange(3), big] > 0)
    assert torch.allclose(pal.mean, x.mean(dim=0), atol=1e-12)
    proj = (x - pal.mean) @ pal.components.t()
    for k in range(3):
        assert abs(float((proj[:, k] < pal.lo[k]).double().mean()) - 0.01) < 1e-3
        assert abs(float((proj[:, k] > pal.hi[k]).double().mean()) - 0.01) < 1e-3
    # b in float64, rounded once
    b64 = -(pal.components @ pal.mean)
    assert pal.b == tuple(float(v) for v in b64.to(torch.float32))
    assert pal.W.dtype == torch.float32 and tuple(pal.W.shape) == (24, 3)


def test_fit_is_invariant_to_row_order_and_leading_shape():
    from dreamvla_amd.dream_view import FeaturePalette
    x, _ = _planted(1)
    a = FeaturePalette.fit(x)
    b = FeaturePalette.fit(x[torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(5))].reshape(40, 100, -1))
    for k in ("mean", "components", "lo", "hi"):
        assert float((a.state_dict()[k] - b.state_dict()[k]).abs().max()) < 1e-9, k


def test_state_dict_round_trip_is_exact():
    from dreamvla_amd.dream_view import FeaturePalette
    x, _ = _planted(2)
    a = FeaturePalette.fit(x.float(), quantiles=(0.05, 0.9))
    b = FeaturePalette(torch.zeros(24), torch.zeros(3, 24), torch.zeros(3), torch.ones(3)).load_state_dict(a.state_dict())
    c = FeaturePalette.from_state_dict(a.state_dict()).to("cpu")
    for other in (b, c):
        for k, v in a.state_dict().items():
            assert torch.equal(v, other.state_dict()[k]) and v.dtype == torch.float64
        assert torch.equal(a.W, other.W) and a.b == other.b and a.lo32 == other.lo32 and a.hi32 == other.hi32
    with pytest.raises(ValueError):
        FeaturePalette.fit(x, quantiles=(0.9, 0.1))
    with pytest.raises(ValueError):
        FeaturePalette.fit(x[:, :2])


def test_default_depth_palette_is_closed_form_and_monotone_in_lightness():
    from dreamvla_amd.dream_view import depth_palette
    pal = depth_palette()
    assert pal.dtype == torch.uint8 and tuple(pal.shape) == (256, 3)
    assert pal[0].tolist() == [0, 0, 0] and pal[255].tolist() == [255, 255, 255]
    luma = pal.double() @ torch.tensor([0.30, 0.59, 0.11], dtype=torch.float64)
    assert torch.all(luma[8:] - luma[:-8] > 0)                                  # rounding to bytes may stall single steps
    assert len({tuple(c) for c in pal.tolist()}) == 256


# ---------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------
def _header():
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "float": ctypes.c_float}


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_entry_points_are_exported_and_bound_as_declared(symbol):
    from dreamvla_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, symbol)
    assert lib.dvla_abi_version() == 9 == _lib.ABI_VERSION
    assert "#define DVLA_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "dvla.h")).read()
    ret, decl = re.search(r"(int64_t|int)\s+%s\s*\((.*?)\)\s*;" % symbol, _header(), flags=re.S).groups()
    want = []
    for arg in decl.split(","):
        typ = re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*\s*$", "", " ".join(arg.split()))       # drop the parameter name
        want.append(ctypes.c_void_p if typ.endswith("*") else C_TYPES[typ])
    res, args = _lib.SYMBOLS[symbol]
    assert res is C_TYPES[ret] and list(args) == want
    assert list(_lib.SYMBOLS)[-len(SYMBOLS):] == SYMBOLS                        # appended: nothing before them moved


def test_operators_are_public_and_dream_render_is_as_it_was():
    from dreamvla_amd import ops
    for name in ("depth_colorize", "flow_unshuffle", "flow_wheel", "motion_mask", "motion_overlay", "feature_render"):
        assert callable(getattr(ops, name))
    x = torch.zeros(1, 4, 8)
    assert ops.dream_render(x, "traj") is x and ops.dream_render(x, "dino") is x
    assert "have no picture" not in ops.dream_render.__doc__ and "feature_render" in ops.dream_render.__doc__


def test_host_side_argument_checks_need_no_gpu():
    from dreamvla_amd import _lib, ops
    from dreamvla_amd.dream_view import FeaturePalette
    lib = _lib.load()
    assert lib.dvla_depth_range_partial_len(0, 5, 7) == 0
    assert lib.dvla_depth_range_partial_len(3, 5, 7) == 3 * 1 * 2
    assert lib.dvla_depth_range_partial_len(2, 224, 224) == 2 * 13 * 2        # 4096-pixel chunks
    assert lib.dvla_depth_range_partial_len(1, 4096, 4096) <= 64 * 2          # never more than 64 partials per map
    with pytest.raises(_lib.DvlaError):
        ops.depth_colorize(torch.zeros(1, 4, 4))                               # no CPU fallback
    with pytest.raises(TypeError):
        ops.depth_colorize(torch.zeros(1, 4, 4, dtype=torch.float64))
    with pytest.raises(_lib.DvlaError):
        ops.feature_render(torch.zeros(1, 4, 8, dtype=torch.bfloat16), FeaturePalette.fit(torch.randn(50, 8)), 32)
    # the C entry points refuse bad arguments before touching a device
    assert lib.dvla_flow_unshuffle(None, None, 1, 4, 2, None) == -1
    assert lib.dvla_flow_wheel(None, None, 0, 4, 4, 8, 8, None) == -1
    assert lib.dvla_motion_mask(8, 8, -1, 4, 2, 1.0, 0, None) == -1
    assert lib.dvla_motion_mask(8, 8, 0, 4, 2, 1.0, 0, None) == 0               # n == 0: nothing launched
    assert lib.dvla_motion_mask(8, 8, 1, 5, 2, 1.0, 0, None) == -3              # 5 tokens: no square grid
    assert lib.dvla_flow_unshuffle(8, 8, 1, 4, 3, None) == -3                   # factor 3
    assert lib.dvla_feature_render(16, 16, 16, 1, 4, 12, 8, 8, *([0.0] * 9), None) == -3     # D = 12
    assert lib.dvla_feature_render(16, 24, 16, 1, 4, 8, 8, 8, *([0.0] * 9), None) == -3      # a misaligned matrix
    assert lib.dvla_motion_overlay(8, 8, 8, 1, 14, 224, 224, *([0.5] * 6), 300, 0, 0, 96, None) == -1
    assert lib.dvla_motion_overlay(8, 8, 8, 1, 14, 225, 224, *([0.5] * 6), 255, 0, 0, 96, None) == -3
    assert lib.dvla_depth_colorize(8, 8, 1, 4, 4, 8, 0, 2.0, 1.0, 0, 0, 0, None, None) == -1   # lo > hi
    assert lib.dvla_depth_colorize(8, 8, 1, 4, 4, 8, 1, 0.0, 0.0, 0, 0, 0, None, None) == -1   # own range without workspace


def _engine_stub(dreams):
    from dreamvla_amd.rollout import RolloutEngine
    return types.SimpleNamespace(dreams=dreams, device=torch.device("cpu"), _VIEW_OPTIONS=RolloutEngine._VIEW_OPTIONS)


def test_dream_views_argument_validation():
    from dreamvla_amd.dream_view import FeaturePalette
    from dreamvla_amd.rollout import RolloutEngine
    check = RolloutEngine._check_dream_views
    pal = FeaturePalette.fit(torch.randn(50, 8))
    stub = _engine_stub(("depth", "sam", "traj"))
    assert check(stub, None) == {}
    got = check(stub, dict(depth=True, sam=pal, traj=dict(thr=0.5)))
    assert list(got) == ["depth", "sam", "traj"] and got["traj"] == {"thr": 0.5} and tuple(got["depth"]["palette"].shape) == (256, 3)
    assert check(stub, dict(depth=dict(lo=0.0, hi=2.0)))["depth"]["hi"] == 2.0
    for bad in (dict(dino=pal),                      # not among dreams
                dict(image=True),                    # no such view
                dict(sam=True),                      # a feature view needs its palette
                dict(depth=dict(lo=0.0)),            # half a range
                dict(depth=dict(low=0.0, hi=1.0)),   # unknown option
                dict(traj=3),
                ["depth"]):
        with pytest.raises(ValueError):
            check(stub, bad)
    with pytest.raises(ValueError):
        check(_engine_stub(("image",)), dict(depth=True))
