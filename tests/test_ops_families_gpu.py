"""GPU: the branches of the LayerNorm and self-attention host wrappers (dreamvla_amd/ops.py) that no other test pins: the fork's
one-sided backwards and fp32 parameters, the concatenating LayerNorm with mismatched or absent parameters, and the dead-key
zero-fill of the merged self-attention Function at a head width other than 64.

LayerNorm shapes: 520 columns = 65 sixteen-byte vectors, so the second vector slot of a wave holds a single lane (the smallest
width past the one-vector-per-lane switch with a ragged tail); 9 rows = two workgroups, the last one partly empty."""
import pytest
import torch

from oracle import torch_ref as R
from tests.gpu_checks import (BF, DEV, TOL_ATTN, TOL_ATTN_F32, TOL_ATTN_GRAD, TOL_FWD, TOL_GRAD, make_block_mask, metrics, rnd)

pytestmark = pytest.mark.gpu

ROWS, COLS, EPS = 9, 520, 1e-5


def _ln_inputs(seed, pdt=BF):
    g = torch.Generator().manual_seed(seed)
    x = R.bf16_round(rnd((ROWS, COLS), g, 2.0) + 0.5)
    w, b = R.bf16_round(rnd((COLS,), g) + 1.0), R.bf16_round(rnd((COLS,), g))
    dy, dres = rnd((ROWS, COLS), g), rnd((ROWS, COLS), g)
    fresh = lambda: (x.to(DEV, BF).requires_grad_(True), w.to(DEV, pdt).requires_grad_(True), b.to(DEV, pdt).requires_grad_(True))
    return x, w, b, dy, dres, fresh


def _same(name, got, want):
    """bit for bit (as values: tolerance 0)"""
    d = float((got.float() - want.float()).abs().max())
    print(f"{name}: max |diff| = {d}")
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), f"{name}: max |diff| = {d}"


def _all_ok(results):
    for m in results:
        print({k: m[k] for k in ("name", "rel_l2", "max_abs", "tol") if k in m})
    for m in results:
        assert m["ok"], f"{m['name']}: rel_l2={m.get('rel_l2')} max_abs={m.get('max_abs')} tol={m.get('tol')}"


def test_fork_with_only_the_normalised_branch_equals_layer_norm():
    """no residual gradient arrives (dres is None): the plain LayerNorm's kernel with the plain LayerNorm's operands"""
    from dreamvla_amd import ops
    _, _, _, dy, _, fresh = _ln_inputs(501)
    x1, w1, b1 = fresh()
    _, y1 = ops.layer_norm_fork(x1, w1, b1, EPS)
    assert type(y1.grad_fn).__name__ == "_LayerNormForkBackward"
    y1.backward(dy.to(DEV, BF))
    x2, w2, b2 = fresh()
    y2 = ops.layer_norm(x2, w2, b2, EPS)
    y2.backward(dy.to(DEV, BF))
    _same("y", y1.detach(), y2.detach())
    _same("dx", x1.grad, x2.grad)
    _same("dgamma", w1.grad, w2.grad)
    _same("dbeta", b1.grad, b2.grad)


def test_fork_with_only_the_residual_gradient_passes_it_through():
    """the normalised branch is not used (dy is None): the input's gradient IS the residual gradient, the parameters get none"""
    from dreamvla_amd import ops
    _, _, _, _, dres, fresh = _ln_inputs(502)
    x1, w1, b1 = fresh()
    r, _ = ops.layer_norm_fork(x1, w1, b1, EPS)
    d = dres.to(DEV, BF)
    r.backward(d)
    _same("dx", x1.grad, d)
    assert w1.grad is None and b1.grad is None


def test_fork_with_fp32_parameters_against_the_oracle():
    from dreamvla_amd import ops
    x, w, b, dy, dres, fresh = _ln_inputs(503, torch.float32)
    xd, wd, bd = fresh()
    r, y = ops.layer_norm_fork(xd, wd, bd, EPS)
    torch.autograd.backward([r, y], [dres.to(DEV, BF), dy.to(DEV, BF)])
    assert wd.grad.dtype == torch.float32 and bd.grad.dtype == torch.float32
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = R.layer_norm(xr, wr, br, EPS)
    torch.autograd.backward([xr * 1.0, yr], [dres, dy])
    tag = f"layernorm_fork {ROWS}x{COLS} pf32"
    _all_ok([metrics(tag + " residual is x", r, x, 0.0), metrics(tag + " y", y, yr, TOL_FWD),
             metrics(tag + " dx", xd.grad, xr.grad, TOL_GRAD),
             metrics(tag + " dgamma", wd.grad, wr.grad, TOL_GRAD, round_ref=False),
             metrics(tag + " dbeta", bd.grad, br.grad, TOL_GRAD, round_ref=False)])


N, LA, LB = 2, 3, 2


def _concat_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    a = R.bf16_round(rnd((N, LA, COLS), g, 2.0) + 0.5)
    b = R.bf16_round(rnd((N, LB, COLS), g, 1.5) - 0.25)
    wa, ba = R.bf16_round(rnd((COLS,), g) + 1.0), R.bf16_round(rnd((COLS,), g))
    dy = rnd((N, LA + LB, COLS), g)
    return a, b, wa, ba, dy


@pytest.mark.parametrize("side", ["a", "b"])
def test_concat_refuses_a_bf16_weight_with_an_fp32_bias_before_any_launch(side, monkeypatch):
    from dreamvla_amd import _lib, ops
    a, b, w, bias, _ = _concat_inputs(504)
    good = (w.to(DEV, BF), bias.to(DEV, BF))
    bad = (w.to(DEV, BF), bias.to(DEV, torch.float32))
    pa, pb = (bad, good) if side == "a" else (good, bad)
    lib = _lib.load()
    launches = []
    real = lib.dvla_layernorm_fwd_rows
    monkeypatch.setattr(lib, "dvla_layernorm_fwd_rows", lambda *args: launches.append(args) or real(*args))
    with pytest.raises(TypeError, match="dtype mismatch"):
        ops.layer_norm_concat(a.to(DEV, BF), pa[0], pa[1], EPS, b.to(DEV, BF), pb[0], pb[1], EPS)
    assert launches == []
    ops.layer_norm_concat(a.to(DEV, BF), *good, EPS, b.to(DEV, BF), *good, EPS)      # (the recorder does see a launch)
    assert len(launches) == 2


def test_concat_with_one_side_without_parameters_equals_cat_of_two_layer_norms():
    from dreamvla_amd import ops
    a, b, wa, ba, dy = _concat_inputs(505)
    dev = lambda t: t.to(DEV, BF).requires_grad_(True)
    a1, b1, wa1, ba1 = dev(a), dev(b), dev(wa), dev(ba)
    y1 = ops.layer_norm_concat(a1, wa1, ba1, EPS, b1, None, None, EPS)
    y1.backward(dy.to(DEV, BF))
    a2, b2, wa2, ba2 = dev(a), dev(b), dev(wa), dev(ba)
    y2 = torch.cat((ops.layer_norm(a2, wa2, ba2, EPS), ops.layer_norm(b2, None, None, EPS)), dim=1)
    y2.backward(dy.to(DEV, BF))
    _same("y", y1.detach(), y2.detach())
    _same("da", a1.grad, a2.grad)
    _same("db", b1.grad, b2.grad)


def test_merged_attention_zero_fills_dead_keys_at_head_width_24():
    """B=2, H=2, L=40, D=24 under a mask whose last 3 keys of every 8-token step nobody sees: the key axis is compacted, the backward
    kernels do not write dk / dv of those keys, and _SelfAttention.backward must (exact zeros, on a dirtied allocator pool)"""
    from dreamvla_amd import ops
    B, H, L, D = 2, 2, 40, 24
    W = H * D
    g = torch.Generator().manual_seed(506)
    qkv, do = rnd((B, L, 3 * W), g), rnd((B, L, W), g)
    mask = make_block_mask(L, 8, 5)
    mt = ops.build_mask_tables(mask, device=DEV)
    dead = mt.dead_keys.cpu()
    assert mt.key_index is not None and mt.Lk == 25 and dead.tolist() == [s * 8 + j for s in range(5) for j in (5, 6, 7)]
    torch.full((B, L, 3 * W), 7.0, device=DEV, dtype=BF)          # (dirty the allocator's pool: an unwritten gradient row would show)
    qd = qkv.to(DEV, BF).requires_grad_(True)
    o = ops.self_attention(qd, H, mask_tables=mt, head_dim=D)
    assert type(o.grad_fn).__name__ == "_SelfAttentionBackward"
    dod = do.to(DEV, BF)
    torch.full((B, L, 3 * W), 7.0, device=DEV, dtype=BF)          # (again: the block the gradient buffer is about to take)
    o.backward(dod)
    grad = qd.grad.detach().float().cpu()
    dkv_dead = grad[:, dead, W:]
    print("dead-key dk / dv: max |value| =", float(dkv_dead.abs().max()))
    assert bool((dkv_dead == 0).all())
    # everything (the dead rows' zeros included: a key nobody sees has no gradient) against the oracles of tests/test_attention_hd_gpu.py
    drop_cols = torch.zeros(L, dtype=torch.int64)
    drop_cols[mt.key_index.cpu().long()] = torch.arange(mt.Lk)
    split = lambda t: t.view(B, L, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = split(qkv)
    sel = list(range(B))
    res = R.attention_bf16(q, k, v, scale=D ** -0.5, mask=mask, drop_cols=drop_cols, dout=do.view(B, L, H, D).permute(0, 2, 1, 3),
                           batch_index=sel)
    dq, dk, dv = (R.merge_heads(t) for t in res[2:])
    qr = qkv.clone().requires_grad_(True)
    q, k, v = split(qr)
    orf = R.merge_heads(R.attention(q, k, v, scale=D ** -0.5, mask=mask, drop_cols=drop_cols, batch_index=sel))
    orf.backward(do)
    tag = f"self_attn B{B} H{H} L{L} D{D} dead keys"
    _all_ok([metrics(tag + " o", o, R.merge_heads(res[0]), TOL_ATTN),
             metrics(tag + " dq", grad[..., :W], dq, TOL_ATTN_GRAD),
             metrics(tag + " dk", grad[..., W:2 * W], dk, TOL_ATTN_GRAD),
             metrics(tag + " dv", grad[..., 2 * W:], dv, TOL_ATTN_GRAD),
             metrics(tag + " o (fp32 oracle)", o, orf, TOL_ATTN_F32),
             metrics(tag + " dqkv (fp32 oracle)", grad, qr.grad, TOL_GRAD)])
