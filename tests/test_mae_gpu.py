"""GPU: the MAE kernels (csrc/mae.hip) against their ATen restatements, and MaskedAutoencoderViT's forward / loss / backward
against the REAL reference's fixtures (tests/make_golden_mae.py) in the bf16 and the fp32-master mode."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = torch.bfloat16
DEV = "cuda"


def ref_masking(x, noise, len_keep, cls_row):
    ids_shuffle = torch.argsort(noise, dim=1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=1, stable=True)
    keep = ids_shuffle[:, :len_keep]
    xm = torch.gather(x, 1, keep.unsqueeze(-1).expand(-1, -1, x.shape[-1]))
    mask = torch.ones_like(noise)
    mask[:, :len_keep] = 0
    mask = torch.gather(mask, 1, ids_restore)
    return torch.cat((cls_row.view(1, 1, -1).expand(x.shape[0], 1, -1), xm), 1), mask, ids_restore, keep


CASES = [(L, D, r) for L in (196, 256, 1024) for D in (768, 1024) for r in (0.5, 0.75, 0.9)]


@pytest.mark.parametrize("L,D,ratio", CASES)
def test_masking_exact(L, D, ratio):
    from dreamvla_amd import ops
    torch.manual_seed(L + D)
    N = 6
    len_keep = int(L * (1 - ratio))
    x = torch.randn(N, L, D, device=DEV).to(BF).requires_grad_(True)
    cls = (0.02 * torch.randn(D, device=DEV)).requires_grad_(True)
    noise = torch.rand(N, L, device=DEV)
    out, mask, ids = ops.mae_random_masking(x, noise, len_keep, cls_row=cls)
    want, mask_r, ids_r, keep = ref_masking(x.detach(), noise, len_keep, cls.detach().to(BF))
    assert torch.equal(ids, ids_r) and torch.equal(mask, mask_r)
    assert torch.equal(out, want)
    dout = torch.randn_like(out)
    out.backward(dout)
    dx = torch.zeros(N, L, D, dtype=BF, device=DEV).scatter_(1, keep.unsqueeze(-1).expand(-1, -1, D), dout[:, 1:])
    assert torch.equal(x.grad, dx)
    torch.testing.assert_close(cls.grad, dout[:, 0].float().sum(0), rtol=1e-5, atol=1e-5)


def test_masking_stable_ties_and_no_cls():
    from dreamvla_amd import ops
    torch.manual_seed(3)
    N, L, D, len_keep = 5, 196, 768, 49
    noise = torch.randint(0, 7, (N, L), device=DEV).float() / 8.0      # seven values: every one tied many times
    noise[1] = 0.5                                                     # one row all tied: identity order
    noise[2, :10] = -0.0
    x = torch.randn(N, L, D, device=DEV).to(BF)
    out, mask, ids = ops.mae_random_masking(x, noise, len_keep)
    want, mask_r, ids_r, _ = ref_masking(x, noise, len_keep, torch.zeros(D, device=DEV, dtype=BF))
    assert torch.equal(ids, ids_r) and torch.equal(mask, mask_r)
    assert torch.equal(out, want[:, 1:])
    assert torch.equal(ids[1], torch.arange(L, device=DEV))


def test_masking_rejects_unsupported_shapes():
    from dreamvla_amd import ops
    from dreamvla_amd._lib import DvlaError
    x = torch.zeros(2, 1025, 64, dtype=BF, device=DEV)
    with pytest.raises(DvlaError):
        ops.mae_random_masking(x, torch.rand(2, 1025, device=DEV), 10)
    x = torch.zeros(2, 196, 60, dtype=BF, device=DEV)
    with pytest.raises(DvlaError):
        ops.mae_random_masking(x, torch.rand(2, 196, device=DEV), 10)


@pytest.mark.parametrize("N,L,D,len_keep,mt_dtype", [(4, 196, 512, 49, torch.float32), (8, 256, 512, 64, BF),
                                                      (3, 196, 384, 98, torch.float32), (2, 1024, 1024, 102, BF)])
def test_unshuffle(N, L, D, len_keep, mt_dtype):
    from dreamvla_amd import ops
    torch.manual_seed(N * L)
    y = torch.randn(N, 1 + len_keep, D, device=DEV).to(BF).requires_grad_(True)
    mt = (0.02 * torch.randn(1, 1, D, device=DEV)).to(mt_dtype).requires_grad_(True)
    pos = torch.randn(1, 1 + L, D, device=DEV).to(BF)
    ids = torch.argsort(torch.argsort(torch.rand(N, L, device=DEV), 1), 1)
    out = ops.mae_unshuffle(y, mt, ids, pos)
    # the reference's four ATen passes (models/vit_mae.py:213-219) on the same bf16 operands
    ya = y.detach().clone().requires_grad_(True)
    mta = mt.detach().to(BF).requires_grad_(True)
    mtoks = mta.repeat(N, L + 1 - ya.shape[1], 1)
    x_ = torch.cat([ya[:, 1:, :], mtoks], 1)
    x_ = torch.gather(x_, 1, ids.unsqueeze(-1).repeat(1, 1, D))
    want = torch.cat([ya[:, :1, :], x_], 1) + pos
    assert torch.equal(out, want)
    dout = torch.randn_like(out)
    out.backward(dout)
    want.backward(dout)
    assert torch.equal(y.grad, ya.grad)
    removed = ids >= len_keep
    dmt = dout[:, 1:][removed].float().sum(0)
    assert mt.grad.dtype == mt_dtype and mt.grad.shape == mt.shape
    err = (mt.grad.float().flatten() - dmt).abs().max() / dmt.abs().max()
    assert err <= (1e-3 if mt_dtype == torch.float32 else 2.0 ** -8), float(err)


def oracle_loss(pred, imgs, mask, p, norm_pix):
    """forward_loss (models/vit_mae.py:129-141,234-250) in fp64 on the same values, and its gradient"""
    N, _, H, W = imgs.shape
    t = imgs.double().reshape(N, 3, H // p, p, W // p, p)
    t = torch.einsum('nchpwq->nhwpqc', t).reshape(N, (H // p) * (W // p), p * p * 3)
    if norm_pix:
        t = (t - t.mean(-1, keepdim=True)) / (t.var(-1, keepdim=True) + 1e-6) ** .5
    pr = pred.detach().double().requires_grad_(True)
    loss = (((pr - t) ** 2).mean(-1) * mask.double()).sum() / mask.double().sum()
    loss.backward()
    return loss.detach(), pr.grad


def bf16_ulp(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("img_dtype", [torch.float32, BF])
@pytest.mark.parametrize("p,N,with_cls", [(16, 16, True), (16, 256, False), (14, 8, True)])
def test_loss(norm_pix, img_dtype, p, N, with_cls):
    from dreamvla_amd import ops
    torch.manual_seed(p * N + norm_pix)
    L, P = (224 // p) ** 2, 3 * p * p
    imgs = torch.randn(N, 3, 224, 224, device=DEV).to(img_dtype)
    full = torch.randn(N, 1 + L, P, device=DEV).to(BF).requires_grad_(True)
    pred = full if with_cls else full[:, 1:, :]                   # the strided view: rows read in place
    mask = (torch.rand(N, L, device=DEV) < 0.75).float()
    loss = ops.mae_loss(pred, imgs, mask, p, norm_pix)
    want, dwant = oracle_loss(full[:, 1:, :], imgs, mask, p, norm_pix)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    loss.backward(torch.tensor(1.7, device=DEV))
    g = full.grad.double()
    assert torch.equal(full.grad[:, 0], torch.zeros_like(full.grad[:, 0]))
    dwant = 1.7 * dwant
    # one bf16 ulp; the absolute term covers the fp32 target where pred - target cancels
    assert bool(((g[:, 1:] - dwant).abs() <= bf16_ulp(dwant) + 1e-6 * float(dwant.abs().max())).all())


# ---------------------------------------------------------------------------------------------------------------------
# the whole module against the REAL reference's fixtures
def build(name, mode):
    from dreamvla_amd.nn import LayerNorm
    from dreamvla_amd.vit_mae import MaskedAutoencoderViT
    from oracle import weights
    fx = torch.load(os.path.join(GOLD, f"{name}.pt"), map_location="cpu")
    cfg = fx["cfg"]
    m = MaskedAutoencoderViT(**cfg["model"], norm_layer=lambda d: LayerNorm(d, eps=1e-6), norm_pix_loss=cfg["norm_pix_loss"])
    m.load_state_dict(weights.fill_state_dict(m.state_dict()), strict=True)
    m = m.to(DEV) if mode == "fp32" else m.to(BF).to(DEV)
    return fx, m


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["mae_b16", "mae_b16_np"])
def test_module_matches_reference(name, mode):
    from tests.make_golden_mae import images
    from tests.model_checks import GRAD_MEDIAN_FACTOR, GRAD_P90_FACTOR, GRAD_TOL_FLOOR, REF_DEV_FACTOR, TOL_FLOOR
    fx, m = build(name, mode)
    cfg = fx["cfg"]
    imgs = images(cfg).to(DEV)
    if mode == "bf16":
        imgs = imgs.to(BF)                     # exact: the fixture images are bf16 values
    noise = fx["noise"].to(DEV)
    loss, pred, mask = m(imgs, cfg["mask_ratio"], noise=noise)
    loss.backward()
    with torch.no_grad():
        latent, mask2, ids = m.forward_encoder(imgs, cfg["mask_ratio"], noise=noise)
    assert torch.equal(ids.cpu(), fx["ids_restore"]) and torch.equal(mask.cpu(), fx["mask"]) and torch.equal(mask2, mask)
    dev = fx["ref_bf16_deviation"]
    fails = []
    for k, got in (("loss", loss), ("pred", pred), ("latent", latent)):
        tol = max(TOL_FLOOR, REF_DEV_FACTOR * max(dev["amp"][k], dev["cast"][k]))
        if k == "loss":
            r = abs(float(got) - float(fx["loss"])) / abs(float(fx["loss"]))
        else:
            assert list(got.shape) == fx[k]["shape"]
            r = rel(got.detach().float().cpu().flatten()[fx[k]["idx"]], fx[k]["vals"])
        print(f"{name} {mode} {k}: rel {r:.3e} tol {tol:.3e}")
        if r > tol:
            fails.append((k, r, tol))
    params = dict(m.named_parameters())
    ratios = []
    for k, e in fx["grads"].items():
        p = params[k]
        assert p.grad is not None and p.grad.dtype == p.dtype, k
        ref_dev = max(e["amp_rel_l2"], e["cast_rel_l2"])
        tol = max(GRAD_TOL_FLOOR, 2.0 * ref_dev)
        r = rel(p.grad.float().cpu().flatten()[e["idx"]], e["vals"])
        ratios.append(r / max(ref_dev, GRAD_TOL_FLOOR / 2.0))
        if r > tol:
            fails.append((k, r, tol))
    rt = torch.tensor(ratios)
    med, p90 = float(rt.quantile(0.5)), float(rt.quantile(0.9))
    print(f"{name} {mode} gradients / reference bf16 deviation: median {med:.2f} p90 {p90:.2f} max {float(rt.max()):.2f}")
    assert med <= GRAD_MEDIAN_FACTOR and p90 <= GRAD_P90_FACTOR, (med, p90)
    assert not fails, fails[:10]


def test_checkpoint_handoff_to_dreamvla(tmp_path, monkeypatch):
    """one optimizer step of MAE pretraining on the GPU, saved as {"model": sd}, loaded by DreamVLA(vit_checkpoint_path=...): its
    vision encoder computes exactly what the pretrained module's frozen-encoder call does"""
    import json
    from dreamvla_amd import ops
    from dreamvla_amd.dreamvla_model import DreamVLA
    from tests.make_golden_mae import images
    fx, m = build("mae_b16", "fp32")
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    imgs = images(fx["cfg"]).to(DEV)
    w0 = m.blocks[0].attn.qkv.weight.detach().clone()
    loss, _, _ = m(imgs, 0.75)
    loss.backward()
    opt.step()
    path = tmp_path / "mae.pth"
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}}, path)
    with open(os.path.join(GOLD, "state_dict_surface_W.json")) as f:
        cfg = json.load(f)["cfg"]
    dv = DreamVLA(clip_device="cpu", vit_checkpoint_path=str(path), **cfg)
    enc = dv.vision_encoder.to(DEV)
    monkeypatch.setattr(ops.GemmTuner, "frozen", True)       # the same GEMM configuration for both calls
    with torch.no_grad():
        want = m.forward_encoder(imgs, 0.0)[0]
        got = enc.forward_encoder(imgs, 0.0)[0]
    assert not torch.equal(m.blocks[0].attn.qkv.weight.detach(), w0)     # the step changed the encoder
    assert torch.equal(got, want)
