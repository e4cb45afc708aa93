"""GPU: the dream pictures (csrc/dream_view.hip) against the references of tests/dream_view_ref.py,
and RolloutEngine(dream_views=...) eager and under hipGraph replay.

Bounds, none of them measured on the code under test:
  depth      bit for bit: the kernel promises its operation order, the reference restates it in numpy float32.
  unshuffle  exact: a permutation and a widening.
  wheel      every byte equal to the float64 reference except where the reference's angle / 2 or 32 |flow| lies within 1e-3 of an
             integer (fp32 atan2 / sqrt are good to a few 1e-5 there); those pixels may be at most 1 % (the reference alone puts
             0.40 % there for N(0, 2 px) flows).  The hand-placed flows sit a quarter unit from every boundary: exact.
  mask       equal wherever the reference's pooled dx^2 + dy^2 is not within 1e-5 thr^2 of thr^2, and equal to the training rule
             `fmask` at f = 2.
  overlay    unmasked pixels equal ops.dream_render's de-normalisation, masked pixels the integer blend of it: exact.
  features   within 1 level of the float64 reference, and equal wherever its pre-rounding value is further than
             delta = 255 (D + 4) 2^-24 sum_d |x_d W[d, k]| / (hi_k - lo_k) from a half-integer (the standard accumulation bound).
tests/gpu_dream_views_perf.py --parity writes the measured figures to profiles/r26_parity_dream_views.jsonl (the recorded run: no
byte of any case differs; 0.22 % and 0.19 % of the wheel's pixels lie in the band)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dream_view_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ops():
    from dreamvla_amd import ops
    return ops


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == BF else t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def depth_maps(shape):
    """float32 (n, h, w): map 0 random with NaN / +-inf pixels, map 1 constant, the others random; (5, ..): map 3 a ramp whose
    levels hit .5 ties under the fixed range, map 4 without one finite pixel"""
    n, h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    d = rng.uniform(0.2, 6.0, size=shape).astype(np.float32)
    bad = rng.uniform(size=(h, w)) < 0.1
    d[0][bad] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], dtype=np.float32), size=int(bad.sum()))
    d[1] = np.float32(1.7)
    if n >= 5:
        d[3] = (np.arange(h * w, dtype=np.float32).reshape(h, w) % 511) * np.float32(3.5 / 510) + np.float32(0.5)
        d[4] = np.float32(np.nan)
        d[4, ::2] = np.float32(np.inf)
    return d


def _palette(kind):
    from dreamvla_amd.dream_view import depth_palette
    if kind == "default":
        return depth_palette("cuda")
    return torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).cuda()


def depth_mismatch(shape, rng_kind, pal_kind):
    """the number of bytes that differ from the numpy float32 restatement"""
    d = depth_maps(shape)
    lo, hi = (None, None) if rng_kind == "own" else (0.5, 4.0)
    pal = _palette(pal_kind)
    nan_color = (255, 0, 255)
    got = _ops().depth_colorize(torch.from_numpy(d).cuda(), lo, hi, None if pal_kind == "default" else pal, nan_color)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape + (3,)
    want = R.depth_colorize(d, _np(pal), lo, hi, nan_color)
    return int((_np(got) != want).sum()), got


@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 224, 224)])
@pytest.mark.parametrize("rng_kind", ["own", "fixed"])
@pytest.mark.parametrize("pal_kind", ["default", "random"])
def test_depth_colorize_bit_for_bit(shape, rng_kind, pal_kind):
    bad, got = depth_mismatch(shape, rng_kind, pal_kind)
    print(f"depth {shape} {rng_kind} {pal_kind}: {bad} bytes differ")
    assert bad == 0
    g = _np(got)
    d = depth_maps(shape)
    assert (g[0][~np.isfinite(d[0])] == np.asarray([255, 0, 255])).all()        # the NaN colour, and only there
    pal = _np(_palette(pal_kind))
    if rng_kind == "own":
        assert (g[1] == pal[0]).all()                                           # a constant map: hi == lo -> index 0


@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 224, 224)])
def test_depth_colorize_does_not_depend_on_the_batch(shape):
    d = torch.from_numpy(depth_maps(shape)).cuda()
    whole = _ops().depth_colorize(d)
    for i in range(shape[0]):
        assert torch.equal(_ops().depth_colorize(d[i:i + 1])[0], whole[i]), i
    lead = _ops().depth_colorize(d.view(1, *shape), 0.5, 4.0)                   # leading dimensions are carried
    assert tuple(lead.shape) == (1,) + shape + (3,) and torch.equal(lead[0], _ops().depth_colorize(d, 0.5, 4.0))


# ---------------------------------------------------------------------------------------------------
# flow: unshuffle, wheel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("g", [2, 14])
@pytest.mark.parametrize("n", [1, 9])
def test_flow_unshuffle_is_exact(f, g, n):
    pred = torch.randn(n, g * g, 2 * f * f, generator=torch.Generator().manual_seed(100 * f + g + n)).to(BF)
    got = _ops().flow_unshuffle(pred.cuda())
    assert got.dtype == torch.float32 and np.array_equal(_np(got), R.flow_unshuffle(pred.float().numpy()))


@functools.lru_cache(maxsize=None)
def wheel_case():
    flow = (torch.randn(4, 28, 28, 2, generator=torch.Generator().manual_seed(28)) * 2.0).numpy()
    return flow, R.flow_wheel(flow), R.wheel_band(flow)


def wheel_stats(size):
    """(share of pixels in the reference's uncertainty band, differing bytes outside it, differing bytes inside it)"""
    flow, ref, band = wheel_case()
    got = _np(_ops().flow_wheel(torch.from_numpy(flow).cuda(), size))
    want, band_up = R.nearest(ref, size, size), R.nearest(band, size, size)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = (got != want).any(axis=-1)
    return float(band_up.mean()), int((diff & ~band_up).sum()), int((diff & band_up).sum())


@pytest.mark.parametrize("size", [224, 30])
def test_flow_wheel_vs_float64_reference(size):
    share, outside, inside = wheel_stats(size)
    print(f"wheel {size}: {100 * share:.3f} % of pixels in the band, {outside} differ outside it, {inside} inside")
    assert share <= 0.01
    assert outside == 0


def test_flow_wheel_hand_placed():
    """hue k and brightness V a quarter unit from their boundaries: angle = 2 k + 0.5 degrees, 32 |flow| = V + 0.25"""
    cells, want = [(0.0, 0.0)], [(0, 0, 0)]
    full = {0: (255, 0, 0), 45: (128, 255, 0), 90: (0, 255, 255), 135: (128, 0, 255)}
    for hue, rgb in full.items():
        a = np.radians(2 * hue + 0.5)
        cells.append((9.0 * np.cos(a), 9.0 * np.sin(a)))                       # saturated
        want.append(rgb)
        cells.append((128.25 / 32 * np.cos(a), 128.25 / 32 * np.sin(a)))       # V = 128: X = (128 * 15 + 15) // 30 = 64
        want.append(tuple({255: 128, 128: 64, 0: 0}[c] for c in rgb))
    flow = np.asarray(cells, dtype=np.float32).reshape(1, 3, 3, 2)
    want = np.asarray(want, dtype=np.uint8).reshape(1, 3, 3, 3)
    assert np.array_equal(R.flow_wheel(flow), want)                            # the reference agrees with the hand values
    for size in (3, 6, 7):
        assert np.array_equal(_np(_ops().flow_wheel(torch.from_numpy(flow).cuda(), size)), R.nearest(want, size, size)), size
    bad = torch.tensor([[[[float("nan"), 1.0], [float("inf"), 0.0]]]]).cuda()
    assert int(_ops().flow_wheel(bad, 2).max()) == 0                           # a non-finite flow is black


# ---------------------------------------------------------------------------------------------------
# mask
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(f, g, thr):
    """bf16 (3, g g, 2 f f): flows whose token means are N(0, 0.45 thr) (9 % of them move); every tenth token moves as one at thr (1 +- 1e-2) (bf16 rounding shifts that by
    at most 0.4 %), corners and an edge token among them"""
    gen = torch.Generator().manual_seed(10 * f + g)
    n, ff = 3, f * f
    pred = torch.randn(n, g * g, 2 * ff, generator=gen) * (0.45 * thr * f)
    near = torch.arange(n * g * g).view(n, g * g) % 10 == 0
    near[:, [0, g - 1, g * g - g, g * g - 1, g // 2]] = True
    ang = torch.rand(n, g * g, generator=gen) * 6.2831853
    mag = thr * (1.0 + 1e-2 * (torch.randint(0, 2, (n, g * g), generator=gen) * 2 - 1))
    placed = torch.cat(((mag * ang.cos()).unsqueeze(-1).expand(-1, -1, ff), (mag * ang.sin()).unsqueeze(-1).expand(-1, -1, ff)), dim=-1)
    return torch.where(near.unsqueeze(-1), placed, pred).to(BF)


def fmask_restated(flow, dilate):
    """losses.calvin_losses' fmask on a (n, 28, 28, 2) float32 flow -> (n, 14, 14) bool"""
    tp = flow.permute(0, 3, 1, 2)
    m = (torch.norm(F.avg_pool2d(tp, kernel_size=2, stride=2), dim=1) > 1.0).unsqueeze(1).to(torch.float32)
    if dilate:
        m = F.max_pool2d(m, kernel_size=3, stride=1, padding=1)
    return m[:, 0] > 0


@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("g,thr", [(14, 1.0), (3, 0.5)])
@pytest.mark.parametrize("dilate", [False, True])
def test_motion_mask_vs_reference(f, g, thr, dilate):
    pred = mask_case(f, g, thr)
    got = _ops().motion_mask(pred.cuda(), thr, dilate)
    assert got.dtype == torch.bool and tuple(got.shape) == (3, g, g)
    want, q = R.motion_mask(pred.float().numpy(), thr, dilate)
    trust = R.mask_trusted(q, thr, dilate)
    assert trust.mean() > 0.99 and (g < 14 or 0.02 < want.mean() < 0.98)
    assert np.array_equal(_np(got)[trust], want[trust])
    if f == 2 and g == 14 and thr == 1.0:
        flow = _ops().flow_unshuffle(pred.cuda()).cpu()
        assert np.array_equal(_np(got), fmask_restated(flow, dilate).numpy())


# ---------------------------------------------------------------------------------------------------
# overlay
# ---------------------------------------------------------------------------------------------------
def _masks(n, g):
    yy, xx = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
    return {"zero": torch.zeros(n, g, g, dtype=torch.bool), "one": torch.ones(n, g, g, dtype=torch.bool),
            "checker": ((yy + xx) % 2 == 0).expand(n, g, g).contiguous()}


@pytest.mark.parametrize("kind", ["zero", "one", "checker"])
def test_motion_overlay_vs_dream_render(kind):
    """frames that are constant on each 16 x 16 patch: with a zero prediction ops.dream_render returns exactly their
    de-normalisation (the patch mean of 768 equal bf16 values is that value in fp32, the variance 0)"""
    ops = _ops()
    n, g = 2, 14
    gen = torch.Generator().manual_seed(14)
    cells = (torch.randn(n, 3, g, g, generator=gen) * 1.3).to(BF)
    cells = cells.mean(dim=1, keepdim=True).to(BF).expand(n, 3, g, g)           # one value per patch over all three channels
    cur = cells.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3).contiguous().cuda()
    plain = ops.dream_render(torch.zeros(n, g * g, 768, dtype=BF, device="cuda"), "image", cur)
    assert len(torch.unique(plain)) > 40                                         # a real picture, not all clamped
    mask = _masks(n, g)[kind]
    got = ops.motion_overlay(mask.cuda(), cur, tint=(255, 64, 0), alpha=96)
    assert np.array_equal(_np(got), R.blend(_np(plain), mask.numpy(), (255, 64, 0), 96))
    if kind == "zero":
        assert torch.equal(got, plain)
    assert torch.equal(ops.motion_overlay(mask.cuda().view(torch.uint8), cur), got)          # a uint8 mask is the same mask


def overlay_stats(g):
    """random frames against the float64 de-normalisation: (largest level difference, differing bytes further than 1e-3 from a tie,
    differing bytes in all); fp32 is good to 255 * 3 * 2^-24 = 5e-5 levels there"""
    n = 3
    cur = (torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(g)) * 1.5).to(BF)
    got = _np(_ops().motion_overlay(torch.zeros(n, g, g, dtype=torch.bool).cuda(), cur.cuda())).astype(np.int64)
    u = R.denorm_levels(cur.float().numpy())
    want = np.rint(u).astype(np.int64)
    away = np.abs(u - np.floor(u) - 0.5) > 1e-3
    diff = got != want
    return int(np.abs(got - want).max()), int((diff & away).sum()), int(diff.sum())


@pytest.mark.parametrize("g", [14, 28])
def test_motion_overlay_random_frames(g):
    ops = _ops()
    worst, outside, total = overlay_stats(g)
    print(f"overlay g={g}: max level difference {worst}, {outside} bytes differ away from ties, {total} in all")
    assert worst <= 1 and outside == 0
    cur = (torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5)) * 1.5).to(BF).cuda()
    base = ops.motion_overlay(torch.zeros(2, g, g, dtype=torch.bool).cuda(), cur)
    for kind, mask in _masks(2, g).items():
        got = ops.motion_overlay(mask.cuda(), cur, tint=(10, 200, 255), alpha=200)
        assert np.array_equal(_np(got), R.blend(_np(base), mask.numpy(), (10, 200, 255), 200)), kind


# ---------------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------------
def _feature_palette(D):
    from dreamvla_amd.dream_view import FeaturePalette
    gen = torch.Generator().manual_seed(D)
    comp = torch.randn(3, D, generator=gen, dtype=torch.float64) / D ** 0.5
    mean = torch.randn(D, generator=gen, dtype=torch.float64) * 0.1
    return FeaturePalette(mean, comp, torch.tensor([-2.0, -1.5, -2.5]), torch.tensor([2.0, 2.5, 1.5]), device="cuda")


@functools.lru_cache(maxsize=None)
def feature_case(D, values, tokens, n):
    gen = torch.Generator().manual_seed(D + tokens + n)
    x = torch.randn(n, tokens, D, generator=gen)
    if values == "one channel 100 x":
        x[..., 3] *= 100.0
    elif values == "saturating":
        x *= 12.0
    return x.to(BF)


def feature_stats(D, values, tokens, n, size):
    """-> (largest level difference, differing bytes outside the band, share of differing bytes)"""
    pal = _feature_palette(D)
    x = feature_case(D, values, tokens, n)
    got = _np(_ops().feature_render(x.cuda(), pal, size)).astype(np.int64)
    u, delta = R.feature_levels(x.float().numpy(), _np(pal.W), pal.b, pal.lo32, pal.hi32)
    want = R.token_blocks(np.rint(u).astype(np.int64), size, size)
    sure = R.token_blocks(np.abs(u - np.floor(u) - 0.5) > delta, size, size)
    assert got.shape == want.shape == (n, size, size, 3)
    diff = got != want
    if values == "saturating":
        assert ((want == 0) | (want == 255)).mean() > 0.5
    return int(np.abs(got - want).max()), int((diff & sure).sum()), float(diff.mean())


@pytest.mark.parametrize("D", [8, 256, 768, 776])
@pytest.mark.parametrize("values", ["normal", "one channel 100 x", "saturating"])
def test_feature_render_vs_float64_reference(D, values):
    for tokens in (4, 256):
        for n in (1, 5):
            for size in (224, 30):
                worst, outside, share = feature_stats(D, values, tokens, n, size)
                print(f"feature D={D} {values} tokens={tokens} n={n} size={size}: max level difference {worst}, {outside} bytes differ "
                      f"outside the band, {100 * share:.4f} % of bytes differ")
                assert worst <= 1 and outside == 0, (tokens, n, size)


def test_feature_render_refuses_what_it_does_not_take():
    from dreamvla_amd import _lib
    ops = _ops()
    with pytest.raises(_lib.DvlaError):
        ops.feature_render(torch.zeros(1, 4, 12, dtype=BF, device="cuda"), _feature_palette(12), 32)        # D % 8 != 0
    with pytest.raises(ValueError):
        ops.feature_render(torch.zeros(1, 4, 16, dtype=BF, device="cuda"), _feature_palette(8), 32)         # another D than fitted
    with pytest.raises(ValueError):
        ops.feature_render(torch.zeros(1, 5, 8, dtype=BF, device="cuda"), _feature_palette(8), 32)          # no square grid
    with pytest.raises(ValueError):
        ops.flow_unshuffle(torch.zeros(1, 4, 6, dtype=BF, device="cuda"))                                   # 6 is not 2 f^2
    with pytest.raises(ValueError):
        ops.motion_mask(torch.zeros(1, 5, 8, dtype=BF, device="cuda"))
    assert tuple(ops.feature_render(torch.zeros(0, 4, 8, dtype=BF, device="cuda"), _feature_palette(8), 32).shape) == (0, 32, 32, 3)
    assert tuple(ops.depth_colorize(torch.zeros(0, 4, 4, device="cuda")).shape) == (0, 4, 4, 3)


# ---------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------
def _views_for(names, use_graph):
    from dreamvla_amd.dream_view import FeaturePalette
    v = {}
    if "depth" in names:
        v["depth"] = True if use_graph else dict(lo=-1.0, hi=3.0)
    if "traj" in names:
        v["traj"] = dict(thr=0.05)                # an untrained head predicts small flows: a threshold that splits them
    for k, D in (("dino", 768), ("sam", 256)):
        if k in names:
            v[k] = FeaturePalette.fit(torch.randn(400, D, generator=torch.Generator().manual_seed(D), dtype=torch.float64) * 0.2)
    return v


def _expected_views(ops, views, dreams, cur, every):
    """ops.* applied to `last_dreams`; cur (B, [S,] 2, 3, h, w): the frames the overlay is drawn on"""
    va = 2 if every else 1
    out = {}
    for k, opt in views.items():
        d = dreams[k]
        if k == "depth":
            out[k] = ops.depth_colorize(d, **(opt if isinstance(opt, dict) else {}))
        elif k == "traj":
            mask = torch.stack([ops.motion_mask(d.select(va, v), opt["thr"], dilate=(v == 0)) for v in range(d.shape[va])], dim=va)
            flow = ops.flow_unshuffle(d)
            out[k] = {"flow": flow, "wheel": ops.flow_wheel(flow, 224), "mask": mask,
                      "overlay": ops.motion_overlay(mask, cur[(slice(None),) * va + (slice(0, d.shape[va]),)])}
        else:
            out[k] = ops.feature_render(d, opt.to("cuda"), 224)
    return out


def engine_checks(name, use_graph, sample, episodes=1):
    from dreamvla_amd.rollout import RolloutEngine
    from tests.dream_checks import _model
    from tests.rollout_checks import WindowOracle
    ops = _ops()
    fx, m, (ip, iw, st, tx) = _model(name)
    S, B = fx["S"], episodes
    names = tuple(k for k in m.dream_names() if k != "image")
    views = _views_for(names, use_graph)
    every = sample == "all"
    bad = []
    with ops.gemm_trials(False):
        eng = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=1, sample=sample, dreams=names, dream_views=views)
        plain = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=1, sample=sample, dreams=names)
        assert plain.last_dream_views == {} and plain.dream_views == {}
        g = torch.Generator().manual_seed(43)
        text = tx[0, :1].expand(B, -1).contiguous()
        oracle = WindowOracle(S)
        total, reset_at = S + 2, (S + 2) // 2
        for t in range(total):
            k = t % S
            if t == reset_at:
                eng.reset()
                plain.reset()
                oracle = WindowOracle(S)
            if B > 1:
                fp = torch.randn(B, 3, 224, 224, generator=g).to(BF).cuda()
                fw = torch.randn(B, 3, 224, 224, generator=g).to(BF).cuda()
                fs = torch.rand(B, st.shape[-1], generator=g).to(BF).cuda()
            else:
                fp, fw, fs = ip[:, k], iw[:, k], st[:, k]
            noise = torch.randn(B * S, fx["test_noise"].shape[1], 7, generator=g).to(BF).float().cuda()
            a1 = eng.step(fp, fw, fs, text, noise=noise)
            a0 = plain.step(fp, fw, fs, text, noise=noise)
            if not all(torch.equal(x, y) for x, y in zip(a1, a0)):
                bad.append(f"t{t}: actions differ from an engine without dream_views")
            if sorted(eng.last_dreams) != sorted(names) or not all(torch.equal(eng.last_dreams[k2], plain.last_dreams[k2]) for k2 in names):
                bad.append(f"t{t}: last_dreams differ from an engine without dream_views")
            got = eng.last_dream_views
            if list(got) != list(views):
                bad.append(f"t{t}: last_dream_views holds {list(got)}")
                continue
            if B > 1:
                continue
            window, _ = oracle.push(k)
            cur = torch.stack((ip[:, window], iw[:, window]), dim=2) if every else torch.stack((fp, fw), dim=1)
            want = _expected_views(ops, views, eng.last_dreams, cur, every)
            for k2, w in want.items():
                for k3, (a, b) in ({"": (got[k2], w)} if not isinstance(w, dict) else {k3: (got[k2][k3], w[k3]) for k3 in w}).items():
                    if a.dtype != b.dtype or a.shape != b.shape or not torch.equal(a, b):
                        bad.append(f"t{t}: {k2}.{k3} {tuple(a.shape)} {a.dtype} is not ops.* of last_dreams ({tuple(b.shape)} {b.dtype})")
        if use_graph and not eng.graphs_captured:
            bad.append("graphs not captured")
    return bad, eng


@pytest.mark.parametrize("name", ["R", "E"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("sample", ["newest", "all"])
def test_engine_dream_views(name, use_graph, sample):
    """fixture R: depth + sam, fixture E: trajectory + dino + sam; S + 2 control steps with a reset mid-way"""
    bad, eng = engine_checks(name, use_graph, sample)
    assert not bad, bad
    v = eng.last_dream_views
    lead = (1, eng.S) if sample == "all" else (1,)
    if name == "R":
        assert v["depth"].dtype == torch.uint8 and tuple(v["depth"].shape) == lead + (2, 224, 224, 3)
        assert len(torch.unique(v["depth"])) > 8                                  # a picture, not one colour
    else:
        t = v["traj"]
        side = 14 * int(round((eng.last_dreams["traj"].shape[-1] // 2) ** 0.5))          # 196 tokens of 2 f^2 values: a 14 f flow
        assert t["flow"].dtype == torch.float32 and tuple(t["flow"].shape) == lead + (2, side, side, 2)
        assert t["mask"].dtype == torch.bool and tuple(t["mask"].shape) == lead + (2, 14, 14)
        assert tuple(t["wheel"].shape) == tuple(t["overlay"].shape) == lead + (2, 224, 224, 3)
        assert tuple(v["dino"].shape) == lead + (2, 224, 224, 3)
    assert v["sam"].dtype == torch.uint8 and tuple(v["sam"].shape) == lead + (2, 224, 224, 3)


def test_engine_dream_views_lockstep_64_episodes():
    bad, eng = engine_checks("E", True, "newest", episodes=64)
    assert not bad, bad
    v = eng.last_dream_views
    side = 14 * int(round((eng.last_dreams["traj"].shape[-1] // 2) ** 0.5))
    assert tuple(v["traj"]["flow"].shape) == (64, 2, side, side, 2) and bool(torch.isfinite(v["traj"]["flow"]).all())
    assert tuple(v["traj"]["mask"].shape) == (64, 2, 14, 14) and v["traj"]["mask"].dtype == torch.bool
    for k in (v["traj"]["wheel"], v["traj"]["overlay"], v["dino"], v["sam"]):
        assert k.dtype == torch.uint8 and tuple(k.shape) == (64, 2, 224, 224, 3)


def test_engine_dream_views_must_be_among_dreams():
    from dreamvla_amd.rollout import RolloutEngine
    from tests.dream_checks import _model
    _, m, _ = _model("E")
    with pytest.raises(ValueError):
        RolloutEngine(m, 1, use_graph=False, dreams=("sam",), dream_views=dict(traj=True))
    with pytest.raises(ValueError):
        RolloutEngine(m, 1, use_graph=False, dreams=("sam",), dream_views=dict(sam=True))
