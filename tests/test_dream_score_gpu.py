"""GPU: scoring the dreams (csrc/dream_score.hip) -- ops.image_quality and ops.depth_quality against the
float64 restatement of tests/dream_score_ref.py, their layout and determinism properties, and RolloutEngine(score_dreams=True)
eager and under hipGraph replay.

Bounds.  `sse` and both depth counts are exact.  The float bounds are 4 x the largest deviation measured over ALL the cases of this
file on an MI355X (tests/gpu_dream_score_perf.py --parity writes them to profiles/r12_parity_dream_score.jsonl); the factor is for
operand-dependent fp32 rounding on other inputs.  SSIM may not exceed 1e-3 absolute and the depth metrics 1e-4 relative: above
that the kernel's arithmetic is at fault, not the bound."""
import functools

import numpy as np
import pytest
import torch

from tests import dream_score_ref as R

# measured (profiles/r12_parity_dream_score.jsonl): the largest |ssim - float64| over the image cases below is 7.601e-08 (the gradient
# against its shift), the largest relative deviation of a depth metric 1.112e-07 (30 % zeros, 13 x 9, n = 5)
SSIM_BOUND = 4 * 7.601e-08
DEPTH_REL_BOUND = 4 * 1.112e-07
assert SSIM_BOUND <= 1e-3 and DEPTH_REL_BOUND <= 1e-4
F32_ROUND = 2.0 ** -23          # mse / psnr: one float64 formula of the exact integer, rounded to float32 once (1 ulp with the log)


def _rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _gradient(h, w):
    y, x = np.mgrid[0:h, 0:w + 1]
    g = np.stack((2.5 * x + 0.7 * y, 255 - 1.9 * x - 1.1 * y, 40 + 60 * np.sin(x / 7.0) + 60 * np.cos(y / 5.0) + 70), axis=-1)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image_cases():
    """(name, a, b) uint8 (n, h, w, 3) numpy"""
    cases = []
    for i, (h, w) in enumerate(((11, 11), (12, 17), (43, 75), (224, 224))):
        for n in (1, 3):
            cases.append((f"random {h}x{w} n={n}", _rand_u8((n, h, w, 3), 10 * i + n), _rand_u8((n, h, w, 3), 10 * i + n + 5)))
    cases.append(("random 16x16 n=130", _rand_u8((130, 16, 16, 3), 90), _rand_u8((130, 16, 16, 3), 91)))
    g = _gradient(43, 75)
    cases.append(("gradient vs 1-pixel shift 43x75", g[None, :, :-1].copy(), g[None, :, 1:].copy()))
    img = _rand_u8((1, 43, 75, 3), 92)
    img[0, :, :, :] = (img[0].astype(np.int32) // 3 + g[:, :-1] // 2).clip(0, 255).astype(np.uint8)
    cases.append(("image vs inverse 43x75", img, 255 - img))
    cases.append(("image vs itself 43x75", img, img.copy()))
    cases.append(("black vs white 43x75", np.zeros((1, 43, 75, 3), np.uint8), np.full((1, 43, 75, 3), 255, np.uint8)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def image_reference(i):
    _, a, b = image_cases()[i]
    return R.image_quality(a, b)


def _depth_pair(n, h, w, seed, zeros=0.0, negative=False, all_zero=False):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.2, 6.0, size=(n, h, w)).astype(np.float32)
    p = (t * rng.uniform(0.6, 1.6, size=t.shape)).astype(np.float32)
    if negative:
        p[rng.uniform(size=p.shape) < 0.2] *= -1.0
    # keep every ratio 1e-3 away from the delta threshold (checked in float64 by the test: > 1e-4)
    ratio = np.maximum(p.astype(np.float64) / t, t / np.where(p > 0, p, 1e-30).astype(np.float64))
    p[np.abs(ratio - 1.25) < 1e-3] *= np.float32(1.01)
    if zeros:
        t[rng.uniform(size=t.shape) < zeros] = 0.0
    if all_zero:
        t[0] = 0.0
    return p, t


@functools.lru_cache(maxsize=None)
def depth_cases():
    cases = []
    for (h, w) in ((13, 9), (224, 224)):
        for n in (1, 5):
            cases.append((f"positive {h}x{w} n={n}", *_depth_pair(n, h, w, 100 + h + n)))
            cases.append((f"30% zeros {h}x{w} n={n}", *_depth_pair(n, h, w, 200 + h + n, zeros=0.3)))
    cases.append(("all-zero target 13x9", *_depth_pair(1, 13, 9, 300, all_zero=True)))
    cases.append(("negative predictions 13x9", *_depth_pair(1, 13, 9, 301, negative=True)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def depth_reference(i):
    _, p, t = depth_cases()[i]
    return R.depth_quality(p, t)


def image_deviation(i):
    """(largest |ssim - float64|, the kernel's dict on the host) of case i"""
    from dreamvla_amd import ops
    _, a, b = image_cases()[i]
    got = {k: v.cpu().numpy() for k, v in ops.image_quality(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).items()}
    return float(np.max(np.abs(got["ssim"].astype(np.float64) - image_reference(i)["ssim"]))), got


def depth_deviation(i):
    """(largest relative deviation of the float metrics over maps with a valid pixel, the kernel's dict on the host) of case i"""
    from dreamvla_amd import ops
    _, p, t = depth_cases()[i]
    got = {k: v.cpu().numpy() for k, v in ops.depth_quality(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()).items()}
    ref = depth_reference(i)
    worst = 0.0
    for k in ("abs_rel", "rmse", "silog"):
        ok = ref["valid"] > 0
        if ok.any():
            worst = max(worst, float(np.max(np.abs(got[k][ok].astype(np.float64) - ref[k][ok]) / np.abs(ref[k][ok]))))
    return worst, got


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(image_cases())), ids=[c[0] for c in image_cases()])
def test_image_quality_vs_float64(i):
    name, a, b = image_cases()[i]
    ref = image_reference(i)
    dev, got = image_deviation(i)
    print(f"image_quality [{name}] max |ssim - float64| = {dev:.3e}  ssim[0] = {got['ssim'][0]:.6f}")
    assert got["sse"].dtype == np.int64 and got["sse"].shape == (len(a),) and np.array_equal(got["sse"], ref["sse"])
    for k in ("mse", "psnr", "ssim"):
        assert got[k].dtype == np.float32 and got[k].shape == (len(a),)
    assert dev <= SSIM_BOUND, dev
    assert np.all(np.abs(got["mse"] - ref["mse"]) <= F32_ROUND * ref["mse"])
    finite = np.isfinite(ref["psnr"])
    assert np.array_equal(np.isposinf(got["psnr"]), ~finite)
    assert np.all(np.abs(got["psnr"][finite] - ref["psnr"][finite]) <= 2 * F32_ROUND * np.maximum(np.abs(ref["psnr"][finite]), 1.0))
    if "itself" in name:
        assert got["sse"][0] == 0 and np.isposinf(got["psnr"][0]) and got["mse"][0] == 0 and got["ssim"][0] >= 1 - 1e-6
    if "inverse" in name:
        assert ref["ssim"][0] < 0 and got["ssim"][0] < 0
    if "black" in name:
        assert abs(ref["ssim"][0] - R.C1 / (255.0 ** 2 + R.C1)) < 1e-12 and got["sse"][0] == 43 * 75 * 3 * 255 ** 2


@pytest.mark.gpu
def test_image_quality_layout_and_determinism():
    from dreamvla_amd import _lib, ops
    lib = _lib.load()
    a, b = torch.from_numpy(_rand_u8((7, 43, 75, 3), 7)).cuda(), torch.from_numpy(_rand_u8((7, 43, 75, 3), 8)).cuda()
    first = ops.image_quality(a, b)
    again = ops.image_quality(a, b)
    assert all(torch.equal(first[k], again[k]) for k in first)                               # the same input twice: bit-equal
    for i in range(7):                                                                        # a frame alone == inside the batch
        one = ops.image_quality(a[i:i + 1], b[i:i + 1])
        assert all(torch.equal(one[k][0], first[k][i]) for k in first), i
    # raw entry point: NaN-poisoned workspace, sentinels around the outputs and the workspace
    n, h, w = 7, 43, 75
    words = lib.dvla_image_quality_partial_len(n, h, w)
    ws = torch.full((words + 16,), float("nan"), device="cuda")
    sse = torch.full((n + 4,), -77, dtype=torch.int64, device="cuda")
    f3 = torch.full((3 * n + 8,), -55.0, device="cuda")
    rc = lib.dvla_image_quality(a.data_ptr(), b.data_ptr(), n, h, w, sse[2:].data_ptr(), f3[4:].data_ptr(), ws[8:].data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(sse[2:2 + n], first["sse"]) and sse[:2].tolist() == [-77, -77] and sse[-2:].tolist() == [-77, -77]
    got3 = f3[4:4 + 3 * n].view(n, 3)
    assert torch.equal(got3[:, 0], first["mse"]) and torch.equal(got3[:, 1], first["psnr"]) and torch.equal(got3[:, 2], first["ssim"])
    assert bool((f3[:4] == -55).all()) and bool((f3[-4:] == -55).all())
    assert bool(torch.isnan(ws[:8]).all()) and bool(torch.isnan(ws[-8:]).all()) and not bool(torch.isnan(ws[8:-8]).any())
    # leading dimensions, and operands that are neither contiguous nor word-aligned
    five = ops.image_quality(a[:6].view(3, 2, h, w, 3), b[:6].view(3, 2, h, w, 3))
    assert all(tuple(v.shape) == (3, 2) and torch.equal(v.reshape(-1), first[k][:6]) for k, v in five.items())
    wide_a, wide_b = torch.zeros(7, 43, 80, 3, dtype=torch.uint8, device="cuda"), torch.zeros(7, 45, 75, 3, dtype=torch.uint8, device="cuda")
    wide_a[:, :, 3:78], wide_b[:, 1:44] = a, b
    strided = ops.image_quality(wide_a[:, :, 3:78], wide_b[:, 1:44])
    assert all(torch.equal(strided[k], first[k]) for k in first)
    flat = torch.zeros(a.numel() + 3, dtype=torch.uint8, device="cuda")
    flat[3:] = a.reshape(-1)
    odd = ops.image_quality(flat[3:].view_as(a), b)                                          # base address 3 mod 4
    assert all(torch.equal(odd[k], first[k]) for k in first)
    empty = ops.image_quality(a[:0], b[:0])
    assert all(tuple(v.shape) == (0,) for v in empty.values())


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(depth_cases())), ids=[c[0] for c in depth_cases()])
def test_depth_quality_vs_float64(i):
    name, p, t = depth_cases()[i]
    assert R.min_ratio_gap(p, t) > 1e-4                     # no pixel's ratio at the delta threshold (a CPU check of the inputs)
    ref = depth_reference(i)
    dev, got = depth_deviation(i)
    print(f"depth_quality [{name}] max relative deviation = {dev:.3e}")
    assert got["valid"].dtype == np.int64 and np.array_equal(got["valid"], ref["valid"])
    some = ref["valid"] > 0
    # the delta count is exact: delta1 is that count over `valid`, rounded to float32 once
    assert np.array_equal(got["delta1"][some], (ref["delta1_count"][some] / ref["valid"][some]).astype(np.float32))
    for k in ("abs_rel", "rmse", "silog", "delta1"):
        assert got[k].dtype == np.float32 and np.all(np.isnan(got[k][~some]))
    assert dev <= DEPTH_REL_BOUND, dev
    if "all-zero" in name:
        assert got["valid"][0] == 0
    if "negative" in name:
        assert (p < 0).sum() > 10 and ref["delta1_count"][0] < ref["valid"][0]


@pytest.mark.gpu
def test_depth_quality_layout_and_determinism():
    from dreamvla_amd import _lib, ops
    lib = _lib.load()
    p, t = _depth_pair(6, 37, 131, 5, zeros=0.2)
    p, t = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    first = ops.depth_quality(p, t)
    again = ops.depth_quality(p, t)
    bits = lambda x: x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x     # NaN rows compare as bits
    eq = lambda x, y: torch.equal(bits(x), bits(y))
    assert all(eq(first[k], again[k]) for k in first)
    for i in range(6):
        one = ops.depth_quality(p[i:i + 1], t[i:i + 1])
        assert all(eq(one[k][0], first[k][i]) for k in first), i
    n, h, w = 6, 37, 131
    words = lib.dvla_depth_quality_partial_len(n, h, w)
    ws = torch.full((words + 16,), float("nan"), device="cuda")
    valid = torch.full((n + 4,), -77, dtype=torch.int64, device="cuda")
    f4 = torch.full((4 * n + 8,), -55.0, device="cuda")
    rc = lib.dvla_depth_quality(p.data_ptr(), t.data_ptr(), n, h, w, valid[2:].data_ptr(), f4[4:].data_ptr(), ws[8:].data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(valid[2:2 + n], first["valid"]) and valid[:2].tolist() == [-77, -77] and valid[-2:].tolist() == [-77, -77]
    got4 = f4[4:4 + 4 * n].view(n, 4)
    assert all(eq(got4[:, j].contiguous(), first[k]) for j, k in enumerate(("abs_rel", "rmse", "silog", "delta1")))
    assert bool((f4[:4] == -55).all()) and bool((f4[-4:] == -55).all())
    assert bool(torch.isnan(ws[:8]).all()) and bool(torch.isnan(ws[-8:]).all())
    two = ops.depth_quality(p.view(3, 2, h, w), t.view(3, 2, h, w))
    assert all(tuple(v.shape) == (3, 2) and eq(v.reshape(-1), first[k]) for k, v in two.items())


def _engine_model(S):
    """a small model with the image and the depth head: 2 trunk layers at the shipped width"""
    from dreamvla_amd.dreamvla_model import DreamVLA
    from oracle import weights
    cfg = dict(finetune_type="calvin", sequence_length=S, num_resampler_query=16, num_obs_token_per_image=9, action_pred_steps=3,
               transformer_layers=2, hidden_dim=1024, transformer_heads=16, phase="finetune", obs_pred=True, depth_pred=True,
               use_dit_head=True, attn_implementation="sdpa")
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg)
    m.load_state_dict(weights.fill_state_dict(m.state_dict()), strict=True)
    m = m.to(torch.bfloat16).to("cuda")
    m._init_model_type()
    return m.eval()


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_engine_scores_its_dreams(use_graph):
    """8 control steps of 3 episodes through step_raw, horizon 3, episode 1 reset before step 5.  Every step: the valid rows of
    last_dream_scores are ops.image_quality / ops.depth_quality of what the test itself saved three steps earlier against this
    step's frames, bit for bit; the other rows hold NaN / -1; actions, dreams and frames are those of an engine that does not score."""
    from dreamvla_amd import ops
    from dreamvla_amd.rollout import RolloutEngine
    from tests.resize_cases import frames
    S, B, T, h = 4, 3, 8, 3
    m = _engine_model(S)
    g = torch.Generator().manual_seed(17)
    text = torch.randint(1, 49000, (B, 77), generator=g)
    text[:, 20] = 49407
    text[:, 21:] = 0
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    with ops.gemm_trials(False):
        eng = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=2, dreams=("image", "depth"), score_dreams=True, horizon=h)
        plain = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=2, dreams=("image", "depth"))
        saved = []
        born = [0] * B
        for t in range(T):
            if t == 5:
                mask = torch.tensor([False, True, False])
                eng.reset(mask)
                plain.reset(mask)
                born[1] = t
            prim, wrist = frames(200, 200, "noise", B, seed=t), frames(84, 84, "noise", B, seed=50 + t)
            state = torch.cat([torch.rand(B, 6, generator=g), (torch.rand(B, 1, generator=g) > 0.5).float()], -1).to(torch.bfloat16)
            noise = torch.randn(B * S, 3, 7, generator=g).to(torch.bfloat16).float().cuda()
            depth_now = (torch.rand(B, 2, 224, 224, generator=g) * 4).cuda() if t != 4 else None
            if depth_now is not None:
                depth_now[:, :, :7] = 0.0                                        # some pixels without a label
            got = eng.step_raw(prim, wrist, state, text, noise=noise, depth_now=depth_now)
            want = plain.step_raw(prim, wrist, state, text, noise=noise)
            assert all(torch.equal(x, y) for x, y in zip(got, want)), t
            assert torch.equal(eng.last_frames_u8, plain.last_frames_u8)
            assert sorted(eng.last_dreams) == sorted(plain.last_dreams) == ["depth", "image"]
            assert all(torch.equal(bits(eng.last_dreams[k]), bits(plain.last_dreams[k])) for k in eng.last_dreams)
            assert plain.last_dream_scores == {}
            s = eng.last_dream_scores
            valid = [t - b0 >= h for b0 in born]
            assert s["valid"].tolist() == valid, (t, s["valid"])
            assert ("depth" in s) == (depth_now is not None)
            rows = torch.tensor(valid, device="cuda")
            if any(valid):
                old = saved[t - h]
                want_s = {"image": ops.image_quality(old["image"], eng.last_frames_u8),
                          "persistence": ops.image_quality(old["frames"], eng.last_frames_u8)}
                if depth_now is not None:
                    want_s["depth"] = ops.depth_quality(old["depth"], depth_now)
                for name, d in want_s.items():
                    assert sorted(s[name]) == sorted(d)
                    for k, v in d.items():
                        assert tuple(s[name][k].shape) == (B, 2) and s[name][k].dtype == v.dtype
                        assert torch.equal(bits(s[name][k])[rows], bits(v)[rows]), (t, name, k)
            for name in ("image", "persistence", "depth"):
                if name in s:
                    for k, v in s[name].items():
                        off = v[~rows]
                        assert bool((off == -1).all()) if v.dtype == torch.int64 else bool(torch.isnan(off).all()), (t, name, k)
            saved.append({"image": eng.last_dreams["image"].clone(), "depth": eng.last_dreams["depth"].clone(),
                          "frames": eng.last_frames_u8.clone()})
        if use_graph:
            assert eng.graphs_captured and plain.graphs_captured
    # the dreams of this random-weight model are no better than anything; the numbers are finite and in range where valid
    v = eng.last_dream_scores
    assert bool(torch.isfinite(v["image"]["ssim"][v["valid"]]).all()) and bool((v["image"]["ssim"][v["valid"]].abs() <= 1).all())
    with pytest.raises(ValueError):
        eng.step(torch.zeros(B, 3, 224, 224), torch.zeros(B, 3, 224, 224), torch.zeros(B, 7), text)     # scoring, but no frames
