"""Timing of MAE pretraining (GPU box only, not a test): one training step -- forward, loss, backward -- of DreamVLA's ViT-B/16
encoder with the default 512 / 8 / 16 decoder at 224^2, mask_ratio 0.75, on MaskedAutoencoderViT (the HIP kernels) and on an
eager PyTorch restatement with the same bf16 weights in the same process (F.conv2d patch embedding, ATen LayerNorm / Linear /
GELU, scaled_dot_product_attention, the reference's argsort / gather / cat masking and its loss); then each kernel of
csrc/mae.hip against the ATen sequence it replaces, in us and in effective TB/s over the bytes the algorithm must move; last,
the step's two attention shapes against eager SDPA (tests/gpu_attn_hd_perf.py).
Prints JSON lines; with `--out PATH` also writes them to PATH (profiles/r07_mae_perf.jsonl is such a run)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dreamvla_amd import ops  # noqa: E402
from dreamvla_amd.nn import LayerNorm  # noqa: E402
from dreamvla_amd.vit_mae import MaskedAutoencoderViT  # noqa: E402
from tests.gpu_perf import timeit  # noqa: E402

BF = torch.bfloat16
MODEL = dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, decoder_embed_dim=512, decoder_depth=8,
             decoder_num_heads=16, mlp_ratio=4)
RATIO = 0.75


# ---- eager restatement (models/vit_mae.py + timm Block), parameters taken from the HIP module's state_dict -----------------
def eager_block(x, P, pre, H):
    N, L, D = x.shape
    h = F.layer_norm(x, (D,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], 1e-6)
    qkv = F.linear(h, P[pre + "attn.qkv.weight"], P[pre + "attn.qkv.bias"]).view(N, L, 3, H, D // H).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(N, L, D)
    x = x + F.linear(o, P[pre + "attn.proj.weight"], P[pre + "attn.proj.bias"])
    h = F.layer_norm(x, (D,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], 1e-6)
    h = F.gelu(F.linear(h, P[pre + "mlp.fc1.weight"], P[pre + "mlp.fc1.bias"]))
    return x + F.linear(h, P[pre + "mlp.fc2.weight"], P[pre + "mlp.fc2.bias"])


def eager_step(P, imgs, noise, p=16):
    N = imgs.shape[0]
    x = F.conv2d(imgs, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    x = x + P["pos_embed"][:, 1:, :]
    L, D = x.shape[1], x.shape[2]
    len_keep = int(L * (1 - RATIO))
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    x = torch.gather(x, 1, ids_shuffle[:, :len_keep].unsqueeze(-1).repeat(1, 1, D))
    mask = torch.ones(N, L, device=x.device)
    mask[:, :len_keep] = 0
    mask = torch.gather(mask, 1, ids_restore)
    cls = P["cls_token"] + P["pos_embed"][:, :1, :]
    x = torch.cat((cls.expand(N, -1, -1), x), 1)
    for i in range(MODEL["depth"]):
        x = eager_block(x, P, f"blocks.{i}.", MODEL["num_heads"])
    x = F.layer_norm(x, (D,), P["norm.weight"], P["norm.bias"], 1e-6)
    x = F.linear(x, P["decoder_embed.weight"], P["decoder_embed.bias"])
    mt = P["mask_token"].repeat(N, L + 1 - x.shape[1], 1)
    x_ = torch.cat([x[:, 1:, :], mt], 1)
    x_ = torch.gather(x_, 1, ids_restore.unsqueeze(-1).repeat(1, 1, x.shape[2]))
    x = torch.cat([x[:, :1, :], x_], 1) + P["decoder_pos_embed"]
    for i in range(MODEL["decoder_depth"]):
        x = eager_block(x, P, f"decoder_blocks.{i}.", MODEL["decoder_num_heads"])
    x = F.layer_norm(x, (x.shape[-1],), P["decoder_norm.weight"], P["decoder_norm.bias"], 1e-6)
    pred = F.linear(x, P["decoder_pred.weight"], P["decoder_pred.bias"])[:, 1:, :]
    t = torch.einsum("nchpwq->nhwpqc", imgs.reshape(N, 3, 14, p, 14, p)).reshape(N, L, p * p * 3)
    loss = (((pred - t) ** 2).mean(-1) * mask).sum() / mask.sum()
    loss.backward()
    return loss


def step_timing(N, iters, warmup):
    torch.manual_seed(0)
    m = MaskedAutoencoderViT(**MODEL, norm_layer=lambda d: LayerNorm(d, eps=1e-6)).to(BF).cuda()
    imgs = torch.randn(N, 3, 224, 224, device="cuda").to(BF)
    noise = torch.rand(N, 196, device="cuda")

    def hip():
        m.zero_grad(set_to_none=True)
        loss, _, _ = m(imgs, RATIO, noise=noise)
        loss.backward()
        return loss
    P = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    P.update({k: v for k, v in m.named_buffers()})

    def eager():
        for v in P.values():
            v.grad = None
        return eager_step(P, imgs, noise)
    lh, le = float(hip()), float(eager())
    r = {"name": "mae_train_step", "N": N, "mask_ratio": RATIO, "hip_loss": lh, "eager_loss": le,
         "hip_ms": timeit(hip, iters=iters, warmup=warmup) * 1e3, "eager_ms": timeit(eager, iters=iters, warmup=warmup) * 1e3}
    r["speedup_vs_eager"] = r["eager_ms"] / r["hip_ms"]
    return r


def kernel_timing(N=256, L=196, D=768, Dd=512, p=16, iters=50):
    """hip_us: the library entry point called directly (preallocated outputs; what the kernel(s) take); hip_op_us: the same
    through ops.* and autograd (allocations, Python); aten_us: the ATen sequence the op replaces, through autograd for backward"""
    from dreamvla_amd import _lib
    lib = _lib.load()
    st = lambda: torch.cuda.current_stream().cuda_stream
    torch.manual_seed(1)
    lk = int(L * (1 - RATIO))
    P = 3 * p * p
    out = []
    raw = {}

    def rec(name, hip_op_s, aten_s, nbytes):
        hip_s = timeit(raw[name], iters=iters)
        r = {"name": name, "N": N, "hip_us": hip_s * 1e6, "hip_op_us": hip_op_s * 1e6, "aten_us": aten_s * 1e6, "bytes": nbytes,
             "hip_TBps": nbytes / hip_s / 1e12, "speedup_vs_aten": aten_s / hip_s}
        out.append(r)
        print(json.dumps(r), flush=True)
    # masking + cls concat
    x = torch.randn(N, L, D, device="cuda").to(BF)
    cls = torch.randn(1, 1, D, device="cuda").to(BF)
    noise = torch.rand(N, L, device="cuda")
    hip_f = lambda: ops.mae_random_masking(x, noise, lk, cls_row=cls)

    def aten_f():
        ids_shuffle = torch.argsort(noise, dim=1)
        ids_restore = torch.argsort(ids_shuffle, dim=1)
        xm = torch.gather(x, 1, ids_shuffle[:, :lk].unsqueeze(-1).repeat(1, 1, D))
        mask = torch.ones(N, L, device="cuda")
        mask[:, :lk] = 0
        mask = torch.gather(mask, 1, ids_restore)
        return torch.cat((cls.expand(N, -1, -1), xm), 1), mask, ids_restore
    o_, m_, i_ = hip_f()
    raw["mae_mask_fwd"] = lambda: lib.dvla_mae_mask_fwd(noise.data_ptr(), x.data_ptr(), cls.data_ptr(), N, L, D, lk, i_.data_ptr(),
                                                        m_.data_ptr(), o_.data_ptr(), st())
    nb = N * L * 4 + N * lk * D * 2 + D * 2 + N * (1 + lk) * D * 2 + N * L * 8 + N * L * 4
    rec("mae_mask_fwd", timeit(hip_f, iters=iters), timeit(aten_f, iters=iters), nb)
    xg = x.clone().requires_grad_(True)
    o, _, ids = ops.mae_random_masking(xg, noise, lk, cls_row=cls)
    do = torch.randn_like(o)
    hip_b = lambda: torch.autograd.grad(o, xg, do, retain_graph=True)
    xa = x.clone().requires_grad_(True)
    oa = torch.cat((cls.expand(N, -1, -1), torch.gather(xa, 1, torch.argsort(noise, 1)[:, :lk].unsqueeze(-1).repeat(1, 1, D))), 1)
    aten_b = lambda: torch.autograd.grad(oa, xa, do, retain_graph=True)
    dx_ = torch.empty_like(x)
    raw["mae_mask_bwd"] = lambda: lib.dvla_mae_mask_bwd(ids.data_ptr(), do.data_ptr(), 1, N, L, D, lk, dx_.data_ptr(), st())
    rec("mae_mask_bwd", timeit(hip_b, iters=iters), timeit(aten_b, iters=iters), N * lk * D * 2 + N * L * 8 + N * L * D * 2)
    # decoder un-shuffle
    y = torch.randn(N, 1 + lk, Dd, device="cuda").to(BF)
    mt = torch.randn(1, 1, Dd, device="cuda").to(BF)
    pos = torch.randn(1, 1 + L, Dd, device="cuda").to(BF)
    hip_f = lambda: ops.mae_unshuffle(y, mt, ids, pos)

    def aten_u(y, mt):
        x_ = torch.cat([y[:, 1:, :], mt.repeat(N, L + 1 - y.shape[1], 1)], 1)
        x_ = torch.gather(x_, 1, ids.unsqueeze(-1).repeat(1, 1, Dd))
        return torch.cat([y[:, :1, :], x_], 1) + pos
    u_ = hip_f()
    raw["mae_unshuffle_fwd"] = lambda: lib.dvla_mae_unshuffle_fwd(y.data_ptr(), mt.data_ptr(), ids.data_ptr(), pos.data_ptr(), N, L,
                                                                  Dd, lk, u_.data_ptr(), st())
    nb = N * (1 + lk) * Dd * 2 + (1 + L) * Dd * 2 + N * L * 8 + N * (1 + L) * Dd * 2
    rec("mae_unshuffle_fwd", timeit(hip_f, iters=iters), timeit(lambda: aten_u(y, mt), iters=iters), nb)
    yg, mtg = y.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    o = ops.mae_unshuffle(yg, mtg, ids, pos)
    do = torch.randn_like(o)
    hip_b = lambda: torch.autograd.grad(o, (yg, mtg), do, retain_graph=True)
    oa = aten_u(yg, mtg)
    aten_b = lambda: torch.autograd.grad(oa, (yg, mtg), do, retain_graph=True)
    dy_, dmt_ = torch.empty_like(y), torch.empty(Dd, dtype=BF, device="cuda")
    part_ = torch.empty(4 * N * Dd, device="cuda")
    raw["mae_unshuffle_bwd"] = lambda: lib.dvla_mae_unshuffle_bwd(do.data_ptr(), ids.data_ptr(), N, L, Dd, lk, dy_.data_ptr(),
                                                                  dmt_.data_ptr(), 0, part_.data_ptr(), st())
    rec("mae_unshuffle_bwd", timeit(hip_b, iters=iters), timeit(aten_b, iters=iters),
        N * (1 + L) * Dd * 2 + N * L * 8 + N * (1 + lk) * Dd * 2)
    # loss (fp32 images, the decoder output with its cls row)
    imgs = torch.randn(N, 3, 224, 224, device="cuda")
    full = torch.randn(N, 1 + L, P, device="cuda").to(BF).requires_grad_(True)
    mask = (torch.rand(N, L, device="cuda") < RATIO).float()
    hip_f = lambda: ops.mae_loss(full, imgs, mask, p)

    def aten_l():
        t = torch.einsum("nchpwq->nhwpqc", imgs.reshape(N, 3, 14, p, 14, p)).reshape(N, L, P)
        return (((full[:, 1:, :] - t) ** 2).mean(-1) * mask).sum() / mask.sum()
    prm = _lib.MaeLossParams(full.data_ptr(), full.stride(0), full.stride(1), 1, p, imgs.data_ptr(), _lib.DT_F32, 0, 224, 224,
                             mask.data_ptr(), N)
    out2_, lpart_ = torch.empty(2, device="cuda"), torch.empty(lib.dvla_mae_loss_partial_len(), device="cuda")
    g_, dp_ = torch.ones(1, device="cuda"), torch.empty_like(full)
    raw["mae_loss_fwd"] = lambda: lib.dvla_mae_loss_fwd(ctypes.byref(prm), out2_.data_ptr(), lpart_.data_ptr(), st())
    raw["mae_loss_bwd"] = lambda: lib.dvla_mae_loss_bwd(ctypes.byref(prm), out2_.data_ptr(), g_.data_ptr(), dp_.data_ptr(), st())
    nb = N * L * P * 2 + N * 3 * 224 * 224 * 4 + N * L * 4
    with torch.no_grad():
        rec("mae_loss_fwd", timeit(hip_f, iters=iters), timeit(aten_l, iters=iters), nb)
    lh, la = hip_f(), aten_l()
    hip_b = lambda: torch.autograd.grad(lh, full, retain_graph=True)
    aten_b = lambda: torch.autograd.grad(la, full, retain_graph=True)
    rec("mae_loss_bwd", timeit(hip_b, iters=iters), timeit(aten_b, iters=iters), nb + N * (1 + L) * P * 2)
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=8, help="steps before timing (the GEMM tuner locks its choices in these)")
    args = ap.parse_args()
    out = []
    for N in (128, 256):
        r = step_timing(N, args.iters, args.warmup)
        out.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    out += kernel_timing()
    # the step's attention shapes at N = 256: encoder (L = 50, head_dim 64) and decoder (L = 197, head_dim 32), against SDPA
    from tests.gpu_attn_hd_perf import one
    for shape in [(256, 12, 50, 64), (256, 16, 197, 32)]:
        r = dict(one(*shape, "dense", 0.0), name="mae_attention")
        out.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
