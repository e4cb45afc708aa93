"""CPU: what makes tests/loss_ref.py (the float64 reference the GPU loss tests compare the HIP kernels with) trustworthy, and
what shows that the budgets of those tests are not tuned on the kernels.

1. On the inputs of the four cases of tests/golden/losses.pt the reference agrees with dreamvla_amd/losses.py::calvin_losses
   (fused=False, compute_dtype=float64) -- which tests/test_losses_golden.py pins to the real training loop -- on the image /
   depth / dino / sam terms and on the prediction gradients, to 1e-12 (float64 on both sides, other summation order).
2. The fp32 ATen formulation sits inside every budget of tests/loss_ref.py with at least 4x headroom on every input family
   of tests/test_losses_gpu.py at n_frames = 7.  Measured here (torch 2.10 CPU), worst case over the family, as a fraction
   of the budget:
     patch_mse  loss 2e-5:               randn 0.003, constant_frames 0.004, border16 0.005, border24 0.007, one_pixel 0.005
     patch_mse  grad 2^-8 |ref| + a:     randn 0.006, constant_frames 0.008, border16 0.008, border24 0.011, one_pixel 0.005
     cosine     loss 2e-5:               0.007 over cols 8 .. 1024 x rows 1 / 3 / 256, zero label / prediction rows included
     cosine     grad 2^-8 |ref| + a:     0.006 (the fp32 result is not rounded to bf16, so the 2^-8 term is almost all headroom)
     silog      loss 2e-5 * cond:        plain 0.003, zero_pixels 0.003, pred_range 0.002, equal_frame 0.002
     silog      grad 2^-8 |ref| + a:     plain 0.004, zero_pixels 0.002, pred_range 0.0006, equal_frame 0.003
     silog      cond:                    1.02 .. 1.96 over the families x lambd 0.5 / 0.85 / 1.0 (asserted <= 20)
   (the assertion is <= 0.25 for each).
"""
import os

import pytest
import torch
import torch.nn.functional as F

from dreamvla_amd import losses
from oracle.make_golden_losses import loss_case_tensors
from tests import loss_ref as LR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.pt")
FX = torch.load(GOLD, map_location="cpu")
HEADROOM = 4.0
N = 7


def _flow_mask(tracks, dilate):
    """(b, t, 784, 2) track flow on a 28x28 grid -> (b * t, 196) {0,1}: mean flow of each 2x2 cell longer than 1 px, optionally grown
    by one cell in every direction"""
    b, t = tracks.shape[:2]
    f = tracks.to(LR.F64).reshape(b * t, 14, 2, 14, 2, 2).mean(dim=(2, 4))           # 2x2 cells of the 28x28 grid
    m = (f.pow(2).sum(-1).sqrt() > 1.0).to(LR.F64)
    if dilate:
        m = F.max_pool2d(m.unsqueeze(1), kernel_size=3, stride=1, padding=1).squeeze(1)
    return m.reshape(b * t, 196)


@pytest.mark.parametrize("name", sorted(FX["cases"]))
def test_reference_matches_the_pinned_loss_block_in_float64(name):
    case = FX["cases"][name]["case"]
    batch, preds = loss_case_tensors(case)
    batch["actions"][..., 6:] = (batch["actions"][..., 6:] + 1) // 2
    S, ag = case["S"], case.get("atten_goal", 0)
    T, B = S - ag, case["B"]
    lo, hi = 3, 3 + T

    def leaves():
        return {k: v.to(LR.F64).clone().requires_grad_(True) for k, v in preds.items()}
    a = leaves()
    g = a.get
    out = (a["arm"], g("gripper", a["arm"]), g("image"), None, None, None, g("depth"), g("traj"), g("dino"), g("sam"))
    lab = losses.label_actions(batch["actions"], S, 3, atten_goal=ag)
    total, parts = losses.calvin_losses(out, batch, sequence_length=S, atten_goal=ag, use_dit_head=case["use_dit_head"],
                                        label_action=lab, flow_as_mask=case["flow_as_mask"], compute_dtype=torch.float64, fused=False)
    assert total.dtype == torch.float64
    total.backward()

    r = leaves()
    view = lambda k, v: r[k].reshape(B, S, *r[k].shape[1:])[:, :T, v, 0].flatten(0, 1)        # (B * T, rows, cols)
    label = lambda k: batch[k][:, lo:hi].flatten(0, 1)
    masks = (None, None)
    if case["flow_as_mask"]:
        masks = (_flow_mask(batch["tracks"][:, :T], True), _flow_mask(batch["tracks_gripper"][:, :T], False))
    ref = {"image": 0.5 * (LR.patch_mse(view("image", 0), label("image_primary"), masks[0])
                           + LR.patch_mse(view("image", 1), label("image_wrist"), masks[1]))}
    if "depth" in r:
        ref["depth"] = 0.5 * (LR.silog(view("depth", 0), label("depth_primary"), 0.5) + LR.silog(view("depth", 1), label("depth_wrist"), 0.5))
    for k in ("dino", "sam"):
        if k in r:
            ref[k] = 0.5 * (LR.cosine(view(k, 0), label(k + "_primary")) + LR.cosine(view(k, 1), label(k + "_wrist")))
    weights = {"image": 0.1, "depth": 0.001, "dino": 0.01, "sam": 0.01}                       # the total of the training loop
    sum(weights[k] * v for k, v in ref.items()).backward()
    for k, v in ref.items():
        assert float(v.detach()) == pytest.approx(float(parts[k].detach()), rel=1e-12), k
        assert float(parts[k]) != 0.0, k
        err = float((r[k].grad - a[k].grad).norm() / a[k].grad.norm())
        assert err <= 1e-12, (k, err)
        if ag:
            assert float(r[k].grad.reshape(B, S, -1)[:, T:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 ATen formulation inside the budgets, with headroom
# ---------------------------------------------------------------------------------------------------------------------
def _aten32(fn, pred, g):
    p = pred.float().clone().requires_grad_(True)
    loss = fn(p)
    assert loss.dtype == torch.float32
    loss.backward()
    return float(loss), g * p.grad


def _check(ms):
    for m in ms:
        print(m)
    for m in ms:
        assert m["ok"], m


@pytest.mark.parametrize("mask", LR.MASK_KINDS, ids=str)
@pytest.mark.parametrize("family", LR.IMAGE_FAMILIES)
def test_aten_patch_mse_inside_budget(family, mask):
    pred, frames = LR.image_inputs(family, N)
    m = LR.patch_mask(mask, N)
    g = 0.5

    def aten(p):
        lab = losses.normalize_patchfied_image(losses.patchify(frames, 16))
        return F.mse_loss(p, lab) if m is None else F.mse_loss(p * m.unsqueeze(-1), lab * m.unsqueeze(-1))
    got, gg = _aten32(aten, pred, g)
    ref, rg = LR.value_and_grad(LR.patch_mse, pred, frames, m, g=g)
    tag = f"aten32 patch_mse {family} mask={mask}"
    if mask == "zeros":
        assert got == 0.0 and ref == 0.0 and float(gg.abs().max()) == 0.0 and float(rg.abs().max()) == 0.0
        return
    _check([LR.loss_metrics(tag + " loss", got, ref, LR.LOSS_RTOL, HEADROOM),
            LR.grad_metrics(tag + " dpred", gg, rg, LR.grad_budget_patch_mse(rg, frames, m, g), HEADROOM)])


def test_chunked_reference_equals_whole():
    pred, frames = LR.image_inputs("border24", N)
    m = LR.patch_mask("random", N)
    whole, wg = LR.value_and_grad(LR.patch_mse, pred, frames, m, g=0.5)
    part, pg = LR.value_and_grad(LR.patch_mse, pred, frames, m, g=0.5, chunk=3)
    assert part == pytest.approx(whole, rel=1e-14)
    assert float((pg - wg).abs().max()) <= 1e-15 * float(wg.abs().max())


COLS = (8, 64, 248, 256, 264, 512, 520, 768, 1024)


@pytest.mark.parametrize("family", LR.COSINE_FAMILIES)
@pytest.mark.parametrize("rows", (1, 3, 256))
@pytest.mark.parametrize("cols", COLS)
def test_aten_cosine_inside_budget(cols, rows, family):
    pred, label = LR.cosine_inputs(family, N, rows, cols)
    g = 0.5
    got, gg = _aten32(lambda p: (1 - F.cosine_similarity(p, label, dim=-1)).mean(), pred, g)
    ref, rg = LR.value_and_grad(LR.cosine, pred, label, g=g)
    tag = f"aten32 cosine {family} {rows}x{cols}"
    ms = [LR.loss_metrics(tag + " loss", got, ref, LR.LOSS_RTOL, HEADROOM)]
    if family == "zero_pred_rows":
        # F.cosine_similarity clamps each norm, the formula clamps the product: at x = 0 the two have different gradients
        # (tests/test_losses_gpu.py says more); the rows with a non-zero prediction are checked
        keep = pred.abs().amax(-1) > 0
        gg, rg = gg[keep], rg[keep]
    if family == "zero_label_rows":
        zero = label.abs().amax(-1) == 0
        assert float(rg[zero].abs().max()) == 0.0 and float(gg[zero].abs().max()) == 0.0
    ms.append(LR.grad_metrics(tag + " dpred", gg, rg, LR.grad_budget_rows(rg), HEADROOM))
    _check(ms)


@pytest.mark.parametrize("lambd", (0.5, 0.85, 1.0))
@pytest.mark.parametrize("family", LR.DEPTH_FAMILIES)
def test_aten_silog_inside_budget(family, lambd):
    pred, depth = LR.depth_inputs(family, N)
    g = 0.5
    cond = LR.silog_cond(pred, depth, lambd)
    print(f"silog {family} lambd={lambd} cond={cond:.3f}")
    assert cond <= LR.COND_MAX
    got, gg = _aten32(lambda p: losses.silog_loss(losses.unpatchify(p.unsqueeze(1), 16), depth.unsqueeze(1), lambd), pred, g)
    ref, rg = LR.value_and_grad(LR.silog, pred, depth, lambd, g=g)
    tag = f"aten32 silog {family} lambd={lambd}"
    if family == "equal_frame":
        assert float(LR.silog_terms(pred, depth)[0].abs().max()) == 0.0
    _check([LR.loss_metrics(tag + " loss", got, ref, LR.LOSS_RTOL * cond, HEADROOM),
            LR.grad_metrics(tag + " dpred", gg, rg, LR.grad_budget_rows(rg), HEADROOM)])
