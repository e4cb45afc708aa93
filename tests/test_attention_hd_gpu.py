"""GPU: the attention kernels for head widths other than 64 (csrc/attention_hd.hip, dvla_attn_hd_fwd / _bwd) through
ops.self_attention, forward + backward, against oracle/torch_ref.py::attention_bf16 (the kernels' rounding points: 1e-3 / 2e-3)
and the unrounded fp32 restatement ::attention (TOL_ATTN_F32 / TOL_GRAD) -- the tolerances of tests/gpu_checks.py, unchanged.
Dropout is checked with the keep mask of the head-width-64 kernels (attn_drop_keep_mask): the same hash serves both."""
import ctypes as C

import pytest
import torch

from oracle import torch_ref as R
from tests.gpu_checks import (BF, DEV, TOL_ATTN, TOL_ATTN_F32, TOL_ATTN_GRAD, TOL_GRAD, _sample_rows, make_block_mask, metrics,
                              rnd)


def _trunk_mask(L):
    """the REAL trunk mask of head set C (36 conditioning + 57 query tokens per step; L = 93 S), as tests/gpu_checks.py uses it"""
    from dreamvla_amd.dreamvla_model import generate_attention_mask
    S = L // 93
    assert L == 93 * S
    return generate_attention_mask(S, 36, 57, 0, False, False, False, 0.0, 54, 3)


def check_self_attention_hd(B, H, L, D, mask_kind="none", dropout_p=0.0, seed=0, rows=None, compact_to=None):
    from dreamvla_amd import ops
    from dreamvla_amd.ops import _Seeds
    g = torch.Generator().manual_seed(101 + 7 * D + seed)
    qkv = rnd((B, L, 3 * H * D), g)
    do = rnd((B, L, H * D), g)
    mask = None
    if mask_kind == "block":
        mask = make_block_mask(L, 19, 12)
    elif mask_kind == "trunk":
        mask = _trunk_mask(L)
    mt = ops.build_mask_tables(mask, device=DEV) if mask is not None else None
    if compact_to is not None:
        assert mt.key_index is not None and mt.Lk == compact_to, (mt.Lk, compact_to)
    qd = qkv.to(DEV, BF).requires_grad_(True)
    _Seeds.counter = 2000 + seed
    o = ops.self_attention(qd, H, mask_tables=mt, dropout_p=dropout_p, head_dim=D)
    sd = (_Seeds.counter, _Seeds.next()[1])
    _Seeds.counter -= 1
    o.backward(do.to(DEV, BF))
    sel = _sample_rows(B, rows)
    idx = torch.tensor(sel)
    drop_cols = None
    if mt is not None and mt.key_index is not None:
        drop_cols = torch.zeros(L, dtype=torch.int64)
        drop_cols[mt.key_index.cpu().long()] = torch.arange(mt.Lk)
    drop = (dropout_p, sd) if dropout_p > 0 else None
    W = H * D
    scale = D ** -0.5
    tag = f"self_attn_hd B{B} H{H} L{L} D{D} mask={mask_kind} p{dropout_p}" + ("" if len(sel) == B else f" ({len(sel)} rows)")
    o_h = o.detach().float().cpu()[idx]
    g_h = qd.grad.detach().float().cpu()[idx]
    qs, dos = qkv[idx], do[idx]
    split = lambda t: t.view(len(sel), L, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = split(qs)
    do4 = dos.view(len(sel), L, H, D).permute(0, 2, 1, 3)
    res = R.attention_bf16(q, k, v, scale=scale, mask=mask, drop=drop, drop_cols=drop_cols, dout=do4, batch_index=sel)
    dq, dk, dv = (R.merge_heads(t) for t in res[2:])
    out = [metrics(tag + " o", o_h, R.merge_heads(res[0]), TOL_ATTN),
           metrics(tag + " dq", g_h[..., :W], dq, TOL_ATTN_GRAD),
           metrics(tag + " dk", g_h[..., W:2 * W], dk, TOL_ATTN_GRAD),
           metrics(tag + " dv", g_h[..., 2 * W:], dv, TOL_ATTN_GRAD)]
    qr = qs.clone().requires_grad_(True)
    q, k, v = split(qr)
    orf = R.merge_heads(R.attention(q, k, v, scale=scale, mask=mask, drop=drop, drop_cols=drop_cols, batch_index=sel))
    orf.backward(dos)
    out += [metrics(tag + " o (fp32 oracle)", o_h, orf, TOL_ATTN_F32),
            metrics(tag + " dqkv (fp32 oracle)", g_h, qr.grad, TOL_GRAD)]
    return out


CASES = (
    # every padded width (DP = 32 / 64 / 96 / 128) and the decoder widths of W (24) and V (48), unmasked at the decoder lengths
    [dict(B=2, H=3, L=205, D=D) for D in (16, 24, 32, 48, 96, 128)]
    + [dict(B=2, H=2, L=L, D=D) for L in (133, 265) for D in (24, 48)]
    + [dict(B=1, H=2, L=65, D=40), dict(B=2, H=2, L=64, D=128)]         # the lengths just past the short kernel
    # block mask at odd L
    + [dict(B=2, H=2, L=133, D=32, mask_kind="block"), dict(B=2, H=2, L=99, D=96, mask_kind="block")]
    # the real trunk mask: L = 651 with key compaction 651 -> 630 (training window), L = 930 (evaluation window)
    + [dict(B=1, H=3, L=651, D=32, mask_kind="trunk", compact_to=630), dict(B=1, H=2, L=930, D=32, mask_kind="trunk"),
       dict(B=1, H=2, L=651, D=48, mask_kind="trunk")]
    # dropout forward + backward (the trunk's attn_pdrop 0.1), unmasked and under the compacted trunk mask
    + [dict(B=2, H=2, L=205, D=24, dropout_p=0.1), dict(B=1, H=2, L=651, D=32, mask_kind="trunk", dropout_p=0.1),
       dict(B=2, H=2, L=133, D=128, mask_kind="block", dropout_p=0.1)]
    # the W trunk at the benchmark's batch, oracle on sampled rows
    + [dict(B=32, H=12, L=651, D=32, mask_kind="trunk", dropout_p=0.1, rows=3)]
)


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_attention_hd_parity(case):
    results = check_self_attention_hd(**case)
    from tests.model_checks import report
    report(results)
    for m in results:
        assert m["ok"], f"{m['name']}: rel_l2={m.get('rel_l2')} max_abs={m.get('max_abs')} tol={m.get('tol')}"


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 136, 60, 4])
def test_attention_hd_refuses_unsupported_head_widths(D):
    """DVLA_ERR_UNSUPPORTED (-3) from both entry points outside {multiples of 8 in [8, 128]} \\ {64}, before any launch"""
    from dreamvla_amd import _lib, ops
    lib = _lib.load()
    B, L, H = 1, 40, 2
    q = torch.zeros(B, L, H, max(D, 8), dtype=BF, device=DEV)
    o = torch.zeros_like(q)
    lse = torch.zeros(B, H, L, dtype=torch.float32, device=DEV)
    p = ops._attn_params(q, q, q, o, H, L, 0.125, None, 0.0, (0, 0), lse, q.shape[3])
    assert lib.dvla_attn_hd_fwd(C.byref(p), D, ops._stream()) == -3
    p.dout, p.delta, p.dq, p.dk, p.dv = o.data_ptr(), lse.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr()
    assert lib.dvla_attn_hd_bwd(C.byref(p), D, ops._stream()) == -3
    torch.cuda.synchronize()
