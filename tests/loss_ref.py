"""float64 reference of the three training-loss reductions of csrc/losses.hip (patch_mse, cosine, silog), the input families
the loss tests run them on, and the error budgets those tests hold the fp32 ATen formulation (CPU, tests/test_loss_ref.py)
and the HIP kernels (GPU, tests/test_losses_gpu.py) to.  Plain torch, gradients by autograd, nothing imported from the
package: the formulas are restated from the header comment of losses.hip.

Budgets (derived from the arithmetic, not from any kernel's output):
  * loss scalars of patch_mse / cosine: sums of non-negative fp32 terms in a tree of depth ~ 12 + log2(units per wave);
    relative error <= about (depth + 20) * 2^-24 ~ 3e-6.  LOSS_RTOL = 2e-5 (~ 6x that; the value check_fused_losses uses).
  * silog subtracts two means: LOSS_RTOL * cond, cond = mean(d^2) / (mean(d^2) - lambd * mean(d)^2) in float64; the input
    families keep cond <= COND_MAX = 20.
  * silog also returns mean d (the backward reads it): a sum of signed fp32 terms, so its error is relative to mean |d|:
    LOSS_RTOL * mean |d| / |mean d|.
  * gradients are bf16 elements computed in fp32, checked per element: |got - ref64| <= 2^-8 |ref64| + a.  bf16 keeps 8
    significant bits, so round-to-nearest of the exact value costs up to 2^-8 |ref| by itself (a correctly rounded exact
    gradient uses 0.993 of the budget on these inputs); the fp32 arithmetic gets a = an absolute term: 1e-5 * max |ref64| over
    the row (cosine) or the 16x16 patch (silog); for patch_mse the normalised label of a nearly flat patch is ill-conditioned
    (the fp32 error of the patch mean is multiplied by rstd, up to 1000), so a = 1e-5 * rstd64 * max |x| of that patch *
    |d loss / d (pred - label)| scale (= |g| * 2 / N, times the patch's mask).
"""
import math

import torch

F64 = torch.float64
LOSS_RTOL = 2e-5
COND_MAX = 20.0
BF16_ULP = 2.0 ** -8
ABS_TERM = 1e-5
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)       # the normalisation preprocess.py applies to uint8 frames
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def bf16r(t):
    """nearest bf16-representable values, in the dtype of t"""
    return t.to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the three operations, float64
# ---------------------------------------------------------------------------------------------------------------------
def patches_of(frames):
    """(n, 3, 224, 224) -> (n, 196, 768): patch (h, w), element (py * 16 + px) * 3 + c = frames[n, c, 16 h + py, 16 w + px]"""
    n = frames.shape[0]
    x = frames.reshape(n, 3, 14, 16, 14, 16)                    # n c h py w px
    return x.permute(0, 2, 4, 3, 5, 1).reshape(n, 196, 768)     # n h w py px c


def patch_label(frames):
    """per-patch (x - mean) / sqrt(unbiased variance + 1e-6) of the patchified frames"""
    p = patches_of(frames.to(F64))
    mean = p.mean(dim=-1, keepdim=True)
    var = ((p - mean) ** 2).sum(dim=-1, keepdim=True) / 767.0
    return (p - mean) / torch.sqrt(var + 1e-6)


def patch_stats(frames):
    """(rstd, max |x|) per patch, (n, 196) each, float64: what the patch_mse gradient budget is built from"""
    p = patches_of(frames.to(F64))
    var = ((p - p.mean(dim=-1, keepdim=True)) ** 2).sum(dim=-1) / 767.0
    return 1.0 / torch.sqrt(var + 1e-6), p.abs().amax(dim=-1)


def patch_mse(pred, frames, mask=None):
    """pred (n, 196, 768), frames (n, 3, 224, 224), mask None or (n, 196) of {0, 1}: mean over all n * 196 * 768 elements of
    (pred * m - label * m)^2 -- masked elements stay in the count"""
    d = pred.to(F64) - patch_label(frames)
    if mask is not None:
        d = d * mask.to(F64).unsqueeze(-1)
    return (d * d).sum() / d.numel()


def cosine(pred, label):
    """pred, label (..., cols): mean over rows of 1 - x.y / sqrt(max(|x|^2 |y|^2, 1e-16))"""
    x, y = pred.to(F64).reshape(-1, pred.shape[-1]), label.to(F64).reshape(-1, label.shape[-1])
    den = torch.sqrt(torch.clamp((x * x).sum(-1) * (y * y).sum(-1), min=1e-16))
    return (1.0 - (x * y).sum(-1) / den).mean()


def depth_patches_of(depth):
    """(n, 224, 224) -> (n, 196, 256): patch (h, w), element py * 16 + px = depth[n, 16 h + py, 16 w + px]"""
    n = depth.shape[0]
    return depth.reshape(n, 14, 16, 14, 16).permute(0, 1, 3, 2, 4).reshape(n, 196, 256)


def silog_terms(pred, depth):
    """d = log(t + 1e-6) - log(p + 1e-6), pairing prediction patch elements with the pixels they un-patchify to"""
    t = depth_patches_of(depth.to(F64).reshape(-1, 224, 224))
    return torch.log(t + 1e-6) - torch.log(pred.to(F64) + 1e-6)


def silog(pred, depth, lambd):
    """pred (n, 196, 256) of 16x16 depth patches, depth (n, 1, 224, 224) or (n, 224, 224)"""
    d = silog_terms(pred, depth)
    return torch.sqrt((d * d).mean() - lambd * d.mean() ** 2)


def silog_cond(pred, depth, lambd):
    """condition number of the final subtraction: mean(d^2) / (mean(d^2) - lambd * mean(d)^2)"""
    d = silog_terms(pred, depth)
    m2, md = float((d * d).mean()), float(d.mean())
    rest = m2 - lambd * md * md
    return math.inf if rest <= 0.0 else m2 / rest


def value_and_grad(fn, pred, *args, g=1.0, chunk=None):
    """float64 loss and g * d loss / d pred.  chunk: evaluate a loss that is a plain mean over frames in slices of `chunk`
    frames (patch_mse, cosine at training scale: bounds the float64 temporaries); every tensor argument is sliced alike."""
    n = pred.shape[0]
    if chunk is None or chunk >= n:
        p = pred.to(F64).clone().requires_grad_(True)
        loss = fn(p, *args)
        loss.backward()
        return float(loss.detach()), g * p.grad
    total, grads = 0.0, []
    for lo in range(0, n, chunk):
        sl = slice(lo, min(lo + chunk, n))
        p = pred[sl].to(F64).clone().requires_grad_(True)
        part = fn(p, *[a[sl] if torch.is_tensor(a) else a for a in args]) * ((sl.stop - sl.start) / n)
        part.backward()
        total += float(part.detach())
        grads.append(g * p.grad)
    return total, torch.cat(grads)


# ---------------------------------------------------------------------------------------------------------------------
# budgets
# ---------------------------------------------------------------------------------------------------------------------
def grad_budget_patch_mse(ref, frames, mask, g):
    rstd, amax = patch_stats(frames)
    scale = abs(g) * 2.0 / ref.numel()
    a = ABS_TERM * rstd * amax * scale
    if mask is not None:
        a = a * mask.to(F64)
    return BF16_ULP * ref.abs() + a.unsqueeze(-1)


def grad_budget_rows(ref):
    """cosine: per row of the last dimension; silog: per 16x16 patch, which is the last dimension of (n, 196, 256) too"""
    return BF16_ULP * ref.abs() + ABS_TERM * ref.abs().amax(dim=-1, keepdim=True)


def grad_metrics(name, got, ref, budget, headroom=1.0):
    """per-element check |got - ref| <= budget / headroom, plus rel-L2 for comparison with the older checks.  An element
    whose budget is 0 (reference exactly 0 and no absolute term) must be exactly 0."""
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).abs()
    finite = bool(torch.isfinite(got).all())
    ratio = torch.where(budget > 0, err / budget.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max()) if finite else math.inf
    rel = float((got - ref).norm() / max(float(ref.norm()), 1e-300)) if finite else math.inf
    return dict(name=name, ok=finite and worst * headroom <= 1.0, worst_elem_ratio=worst, headroom=headroom, rel_l2=rel,
                max_abs=float(err.max()) if finite else math.inf, tol="2^-8 |ref| + a", n=ref.numel())


def loss_metrics(name, got, ref, rtol, headroom=1.0):
    err = abs(got - ref)
    ok = math.isfinite(got) and err * headroom <= rtol * abs(ref)
    return dict(name=name, ok=ok, got=got, ref=ref, rel_err=err / abs(ref) if ref != 0 else (0.0 if err == 0 else math.inf),
                rel_l2=err / abs(ref) if ref != 0 else (0.0 if err == 0 else math.inf), max_abs=err, tol=rtol, headroom=headroom)


# ---------------------------------------------------------------------------------------------------------------------
# input families (all values bf16-representable fp32 CPU tensors)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def normalised_u8(u8):
    """uint8 (n, 3, 224, 224) -> the CLIP-normalised frames preprocess.py produces, rounded to bf16"""
    mean = torch.tensor(CLIP_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    return bf16r((u8.float() / 255.0 - mean) / std)


IMAGE_FAMILIES = ("randn", "constant_frames", "border16", "border24", "one_pixel")


def image_inputs(family, n, seed=0):
    """(pred (n, 196, 768), frames (n, 3, 224, 224)).  randn: the old fixtures' distribution.  The others are uint8 camera-like
    frames normalised as preprocess.py does: constant_frames = every second frame one colour (all 196 patches flat: variance 0,
    rstd 1000); border16 / border24 = a one-colour border of that many pixels around noise (border patches fully / half flat);
    one_pixel = one colour except a single pixel that differs by one grey level (variance ~ 1e-6, the size of eps)."""
    g = _gen(7000 + seed)
    pred = bf16r(torch.randn(n, 196, 768, generator=g))
    if family == "randn":
        return pred, bf16r(torch.randn(n, 3, 224, 224, generator=g))
    u8 = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8)
    colour = torch.randint(0, 256, (n, 3, 1, 1), generator=g, dtype=torch.uint8)
    flat = colour.expand(n, 3, 224, 224).clone()
    if family == "constant_frames":
        u8[::2] = flat[::2]
    elif family in ("border16", "border24"):
        b = 16 if family == "border16" else 24
        inner = u8[:, :, b:224 - b, b:224 - b].clone()
        u8 = flat
        u8[:, :, b:224 - b, b:224 - b] = inner
    elif family == "one_pixel":
        u8 = flat
        for i in range(n):
            y, x = int(torch.randint(0, 224, (1,), generator=g)), int(torch.randint(0, 224, (1,), generator=g))
            c = u8[i, :, y, x].to(torch.int16)
            u8[i, :, y, x] = torch.where(c < 255, c + 1, c - 1).to(torch.uint8)
    else:
        raise ValueError(family)
    return pred, normalised_u8(u8)


MASK_KINDS = (None, "random", "zeros", "ones")


def patch_mask(kind, n, seed=0):
    if kind is None:
        return None
    if kind == "random":
        return (torch.rand(n, 196, generator=_gen(7100 + seed)) > 0.5).float()
    return torch.zeros(n, 196) if kind == "zeros" else torch.ones(n, 196)


COSINE_FAMILIES = ("randn", "zero_label_rows", "zero_pred_rows")


def cosine_inputs(family, n, rows, cols, seed=0):
    """(pred, label) of (n, rows, cols).  zero_label_rows / zero_pred_rows: about one row in five all zero on that side
    (at least the first and the last row)."""
    g = _gen(7200 + seed)
    pred = bf16r(torch.randn(n, rows, cols, generator=g))
    label = bf16r(torch.randn(n, rows, cols, generator=g))
    if family != "randn":
        z = (torch.rand(n * rows, generator=g) < 0.2)
        z[0] = z[-1] = True
        (label if family == "zero_label_rows" else pred).view(n * rows, cols)[z] = 0.0
    return pred, label


DEPTH_FAMILIES = ("plain", "zero_pixels", "pred_range", "equal_frame")
SMALLEST_BF16 = 2.0 ** -133        # smallest positive (subnormal) bf16
SMALLEST_NORMAL_BF16 = 2.0 ** -126


def depth_inputs(family, n, seed=0):
    """(pred (n, 196, 256), depth (n, 1, 224, 224)).  plain: the old fixtures' ranges (depth rand * 10 + 0.01, post-ReLU predictions
    rand * 5 + 0.05).  zero_pixels: 10 % of the depth pixels are 0 (log(0 + 1e-6)).  pred_range: predictions log-uniform over
    [1e-8, 1e3] with 2 % each of exact 0, the smallest subnormal and the smallest normal bf16 and 1e3 -- what a ReLU head can emit.
    equal_frame: plain, with pred == depth on the whole first frame (every term of that frame is exactly 0)."""
    g = _gen(7300 + seed)
    depth = bf16r(torch.rand(n, 1, 224, 224, generator=g) * 10 + 0.01)
    pred = bf16r(torch.rand(n, 196, 256, generator=g) * 5 + 0.05)
    if family == "zero_pixels":
        depth[torch.rand(depth.shape, generator=g) < 0.1] = 0.0
    elif family == "pred_range":
        u = torch.rand(n, 196, 256, generator=g)
        pred = bf16r(torch.exp(math.log(1e-8) + u * (math.log(1e3) - math.log(1e-8))))
        pick = torch.rand(n, 196, 256, generator=g)
        for k, v in enumerate((0.0, SMALLEST_BF16, SMALLEST_NORMAL_BF16, 1e3)):
            pred[(pick >= 0.02 * k) & (pick < 0.02 * (k + 1))] = v
        pred = bf16r(pred)
    elif family == "equal_frame":
        pred[0] = depth_patches_of(depth[0])[0]
    elif family != "plain":
        raise ValueError(family)
    return pred, depth
