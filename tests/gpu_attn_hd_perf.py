"""Timing of the head-width-generic attention kernels (csrc/attention_hd.hip; GPU box only, not a test) at the shapes the
models of other widths run: the W trunk (hidden 384 / 12 heads: head_dim 32, real mask, L = 651, B = 32, with and without
dropout) and the dream-head decoders (16 heads, unmasked, L = 205 / 265: head_dim 24 at hidden 384, 48 at hidden 768).
Next to each: eager torch.nn.functional.scaled_dot_product_attention on the same inputs with the additive mask (forward, and
forward + backward minus forward for the backward), and, for scale, the head_dim-64 kernels at the trunk shape.
Prints JSON lines; with `--out PATH` also writes them to PATH (profiles/r07_attn_hd_perf.jsonl is such a run)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dreamvla_amd import ops  # noqa: E402
from dreamvla_amd.dreamvla_model import generate_attention_mask  # noqa: E402
from tests.gpu_perf import timeit  # noqa: E402

BF = torch.bfloat16


def one(B, H, L, D, mk, p):
    qkv = torch.randn(B, L, 3 * H * D, device="cuda", dtype=BF)
    v5 = qkv.view(B, L, 3, H, D)
    q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
    mt, mask = None, None
    if mk == "trunk":
        mask = generate_attention_mask(L // 93, 36, 57, 0, False, False, False, 0.0, 54, 3)
        mt = ops.build_mask_tables(mask, device="cuda")
        mask = mask.to("cuda", BF)
    scale = D ** -0.5
    f = lambda: ops.attn_fwd_raw(q, k, v, scale=scale, mask_tables=mt, dropout_p=p, seed=(3, 4), head_dim=D)
    tf = timeit(f, iters=20)
    o, lse = f()
    do = torch.randn_like(o)
    dqkv = torch.zeros_like(qkv)
    d5 = dqkv.view(B, L, 3, H, D)
    g = lambda: ops.attn_bwd_raw(q, k, v, o, lse, do, d5[:, :, 0], d5[:, :, 1], d5[:, :, 2], scale=scale, mask_tables=mt,
                                 dropout_p=p, seed=(3, 4), head_dim=D)
    tb = timeit(g, iters=20)
    r = {"B": B, "H": H, "L": L, "D": D, "mask": mk, "dropout_p": p, "fwd_us": tf * 1e6, "bwd_us": tb * 1e6}
    # eager SDPA, same inputs, (B, H, L, D) views, additive mask; dropout through SDPA's own dropout_p
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    sf = lambda: F.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask, dropout_p=p, scale=scale)
    r["sdpa_fwd_us"] = timeit(sf, iters=20) * 1e6
    qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (qs, ks, vs))
    dog = do.permute(0, 2, 1, 3)

    def sfb():
        y = F.scaled_dot_product_attention(qg, kg, vg, attn_mask=mask, dropout_p=p, scale=scale)
        y.backward(dog)
    r["sdpa_fwd_bwd_us"] = timeit(sfb, iters=20) * 1e6
    r["sdpa_bwd_us"] = r["sdpa_fwd_bwd_us"] - r["sdpa_fwd_us"]
    r["fwd_speedup_vs_sdpa"] = r["sdpa_fwd_us"] / r["fwd_us"]
    r["bwd_speedup_vs_sdpa"] = r["sdpa_bwd_us"] / r["bwd_us"]
    return r


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    torch.manual_seed(0)
    out = []
    for shape in [(32, 12, 651, 32, "trunk", 0.1), (32, 12, 651, 32, "trunk", 0.0), (32, 16, 651, 64, "trunk", 0.1),
                 (32, 16, 205, 24, "dense", 0.0), (32, 16, 265, 24, "dense", 0.0),
                 (32, 16, 205, 48, "dense", 0.0), (32, 16, 265, 48, "dense", 0.0)]:
        r = one(*shape)
        out.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
