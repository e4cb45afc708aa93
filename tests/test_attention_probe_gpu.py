"""GPU: the attention probe kernel (csrc/attention_probe.hip through ops.attention_probe / ops.self_attention_probe) against the
float64 restatement of tests/attention_probe_ref.py, at the smallest shapes that can go wrong: key counts around the 32-key tile
(1, 31, 32, 33), the resampler's 16 x 212, the trunk's 651; head widths 8, 24, 64, 72, 128 (one vector in one lane, three lanes,
a full row of lanes, the second vector of a lane); 1, 3, 16 heads; 1 and 3 sequences with different rows each; 1, 3, 32 rows.

Exact, no tolerance: every element of the output is written (NaN pre-fill) and nothing around it (sentinels); columns the row cannot
see, blind rows and rows out of range are 0.0; two runs and a sequence alone against the same sequence in a batch of three agree
bit for bit.  Values: the derived bound of the reference module, which must itself stay below 1e-3 p* + 1e-7.  Tie to the product
kernels: per-head P times V in float64 against the same rows of ops.attn_fwd_raw's output at the attention tests' own tolerance.
One line per case (worst error / bound) goes to $DVLA_PARITY_REPORT (profiles/r22_parity_attention_probe.jsonl)."""
import math

import numpy as np
import pytest
import torch

from tests import attention_mask_cases as MC
from tests import attention_probe_ref as PR
from tests.gpu_checks import BF, DEV, TOL_ATTN, metrics
from tests.model_checks import report

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel floats on either side of the output


def _inputs(B, Lq, Lk, H, D, layout, seed):
    """bf16 q (B, Lq, H, D), k / v (B, Lk, H, D) on the device as views, and their values as float64 arrays.
    layout "packed": thirds of one qkv buffer (Lq == Lk); "kv": q of its own, k the first half of a [k | v] buffer; "offset": views
    that start one element into their buffers (2-byte aligned only: the scalar load path) with padded token strides."""
    g = torch.Generator().manual_seed(1000 + seed)
    if layout == "packed":
        assert Lq == Lk
        buf = torch.randn(B, Lq, 3, H, D, generator=g).to(BF).to(DEV)
        q, k, v = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
    elif layout == "kv":
        q = torch.randn(B, Lq, H, D, generator=g).to(BF).to(DEV)
        kv = torch.randn(B, Lk, 2, H, D, generator=g).to(BF).to(DEV)
        k, v = kv[:, :, 0], kv[:, :, 1]
    else:
        qb = torch.randn(B * Lq * (H * D + 3) + 1, generator=g).to(BF).to(DEV)
        kb = torch.randn(B * Lk * (2 * H * D + 5) + 1, generator=g).to(BF).to(DEV)
        q = qb[1:].view(B, Lq, H * D + 3)[:, :, :H * D].view(B, Lq, H, D)
        kv = kb[1:].view(B, Lk, 2 * H * D + 5)[:, :, :2 * H * D].view(B, Lk, 2, H, D)
        k, v = kv[:, :, 0], kv[:, :, 1]
        assert q.data_ptr() % 4 == 2 and k.data_ptr() % 4 == 2
    return q, k, v


def _rows(B, R, Lq, seed, extra=()):
    """different rows for every sequence; `extra` values (out of range, blind rows) overwrite the leading entries of sequence 0 / B - 1"""
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, Lq, size=R) for _ in range(B)]).astype(np.int32)
    for i, x in enumerate(extra):
        rows[(0 if i % 2 == 0 else B - 1), (i // 2) % R] = x
    return rows


def _run(q, k, rows, scale, mt, per_head):
    """the probe into a NaN-filled buffer between sentinels -> the output; asserts that the sentinels survived"""
    from dreamvla_amd import ops
    B, Lq, H, _ = q.shape
    R, Lk = rows.shape[1], k.shape[1]
    shape = (B, H, R, Lk) if per_head else (B, R, Lk)
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    buf[:GUARD] = 12345.0
    buf[GUARD + n:] = 54321.0
    out = buf[GUARD:GUARD + n].view(shape)
    got = ops.attention_probe(q, k, torch.from_numpy(rows).to(DEV), scale=scale, mask_tables=mt, per_head=per_head, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + n:] == 54321.0).all()), "wrote outside its output"
    return out.clone()


def _check(tag, q, k, rows, scale, vis, mt, per_head):
    """exactness + the derived bound for one call; returns the report row"""
    B, Lq, H, D = q.shape
    got = _run(q, k, rows, scale, mt, per_head)
    assert bool(torch.isfinite(got).all()), f"{tag}: an element was not written (NaN pre-fill) or is not finite"
    again = _run(q, k, rows, scale, mt, per_head)
    assert torch.equal(got, again), f"{tag}: two runs differ"
    ref = PR.probabilities(q.float().cpu().numpy(), k.float().cpu().numpy(), rows, scale, vis)
    want = ref["per_head" if per_head else "mean"]
    g = got.double().cpu().numpy()
    assert (g[want == 0.0] == 0.0).all(), f"{tag}: an invisible column / blind row / row out of range is not exactly 0"
    Lk_axis = k.shape[1] if mt is None else mt.Lk
    bnd = PR.bound(ref, D, Lk_axis, per_head)
    assert (bnd <= PR.issue_cap(want)).all(), f"{tag}: the derived bound exceeds 1e-3 p* + 1e-7 -- wrong test inputs"
    err = np.abs(g - want)
    live = want > 0
    ratio = float((err[live] / bnd[live]).max()) if live.any() else 0.0
    row = {"name": tag, "worst_err_over_bound": ratio, "max_abs_err": float(err.max()), "max_bound": float(bnd.max()),
           "rel_l2": float(np.linalg.norm(g - want) / max(np.linalg.norm(want), 1e-300)), "tol": 1.0, "ok": bool((err <= bnd).all())}
    print(row)
    report([row])
    assert row["ok"], row
    if live.any():
        sums = g.sum(axis=-1)
        seen = want.sum(axis=-1) > 0
        assert np.allclose(sums[seen], 1.0, atol=1e-5) and (sums[~seen] == 0.0).all()
    return got


# (id, Lq, Lk, D, H, B, R, layout, per_head, extra rows)
PLAIN = [
    ("L1-D64-H1-B1-R1", 1, 1, 64, 1, 1, 1, "packed", False, ()),
    ("L31-D8-H3-B3-R3", 31, 31, 8, 3, 3, 3, "packed", False, (-1, 31)),
    ("L32-D24-H3-B1-R32", 32, 32, 24, 3, 1, 32, "packed", True, ()),
    ("L33-D72-H1-B3-R3", 33, 33, 72, 1, 3, 3, "packed", False, ()),
    ("L33-D64-H3-B3-R3-offset", 33, 33, 64, 3, 3, 3, "offset", False, (33,)),
    ("L31-D24-H3-B1-R1-offset", 31, 31, 24, 3, 1, 1, "offset", True, ()),
    ("resampler-16x212-D64-H3-B3-R16", 16, 212, 64, 3, 3, 16, "kv", False, ()),
    ("L651-D128-H16-B1-R3", 651, 651, 128, 16, 1, 3, "packed", False, ()),
    ("L651-D64-H16-B3-R1", 651, 651, 64, 16, 3, 1, "packed", False, (-5,)),
    ("L212-D8-H16-B1-R32", 212, 212, 8, 16, 1, 32, "packed", True, ()),
]


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_unmasked_probe_against_float64(case):
    tag, Lq, Lk, D, H, B, R, layout, per_head, extra = case
    q, k, _ = _inputs(B, Lq, Lk, H, D, layout, seed=len(tag))
    rows = _rows(B, R, Lq, seed=Lq + R, extra=extra)
    _check("probe " + tag, q, k, rows, 1.0 / math.sqrt(D), None, None, per_head)


# families of tests/attention_mask_cases.py: (case id there, D override, per_head)
MASKED = [("bern-D64-L133", False), ("tiles-D64-L133", True), ("blind-D64-L133", False), ("edges-D64-L133", False),
          ("corner-D64-L133", True), ("tiles-D64-L133-random", False), ("blind-D64-L133-uncompacted", True),
          ("blind-D64-L40x133", False), ("blind-D24-L133-p0.1", False), ("edges-D128-L133", False)]


@pytest.mark.parametrize("cid,per_head", MASKED, ids=[c[0] for c in MASKED])
def test_masked_probe_against_float64(cid, per_head):
    case = MC.BY_ID[cid]
    vis, _, mt = MC.tables(case, device=DEV)
    Lq, Lk, D = case["Lq"], case["Lk"], case["D"]
    B, H, R = 3, 3, 32
    q, k, _ = _inputs(B, Lq, Lk, H, D, "packed" if Lq == Lk else "kv", seed=len(cid))
    blind = np.nonzero(~vis.any(axis=1))[0]
    rows = _rows(B, R, Lq, seed=7, extra=tuple(int(x) for x in blind[:3]) + (Lq, -1))
    _check("probe " + cid, q, k, rows, 1.0 / math.sqrt(D), vis, mt, per_head)


def _rule_tables():
    """the trunk's evaluation mask at L = 651 (7 window steps of 36 + 54 + 3 tokens) from the rule, on the device, with
    atten_only_obs and a non-zero mask_l_obs_ratio; and the same mask as a boolean matrix (ops.mask_rule_visible)"""
    from dreamvla_amd import ops
    rule = dict(K=7, num_A=36, num_B=57, atten_goal=0, atten_goal_state=False, atten_only_obs=True, attn_robot_proprio_state=True,
                num_obs_token=54, action_pred_steps=3)
    np.random.seed(11)
    drop = ops.draw_mask_drop(rule["K"], 54, 3, True, 0.3)
    mt = ops.build_mask_tables_device(DEV, drop=drop, **rule)
    vis = ops.mask_rule_visible(drop=drop, **rule)
    return rule, vis, mt


def test_rule_mask_from_the_device_builder():
    """action rows of a different window step per sequence + one dream query + one image token: the compacted, audience-ordered
    key axis of csrc/masks.hip is undone on the store; under atten_only_obs an action row's mass stays inside its own step"""
    rule, vis, mt = _rule_tables()
    assert mt.key_index is not None and mt.Lk < 651
    B, H, D, blk = 3, 16, 64, 93
    q, k, _ = _inputs(B, 651, 651, H, D, "packed", seed=5)
    rows = np.array([[s * blk + 90, s * blk + 91, s * blk + 92, s * blk + 40, s * blk + 5] for s in (6, 0, 3)], dtype=np.int32)
    got = _check("probe rule-mask-L651", q, k, rows, 0.125, vis, mt, False)
    for b, s in enumerate((6, 0, 3)):
        other = torch.ones(651, dtype=torch.bool)
        other[s * blk:(s + 1) * blk] = False
        assert float(got[b, :3][:, other.to(DEV)].abs().max()) == 0.0


def test_a_sequence_does_not_depend_on_its_batch():
    """sequence b of a B = 3 call against the same sequence alone, bit for bit; masked and unmasked, both outputs"""
    vis, _, mt = MC.tables(MC.BY_ID["blind-D64-L133"], device=DEV)
    cases = [(None, None, 33, 72, 3), (vis, mt, 133, 64, 3)]
    for vis, mt, L, D, H in cases:
        q, k, _ = _inputs(3, L, L, H, D, "packed", seed=2)
        rows = _rows(3, 3, L, seed=9)
        for per_head in (False, True):
            full = _run(q, k, rows, 0.2, mt, per_head)
            for b in range(3):
                alone = _run(q[b:b + 1], k[b:b + 1], rows[b:b + 1], 0.2, mt, per_head)
                assert torch.equal(full[b:b + 1], alone), (L, per_head, b)


@pytest.mark.parametrize("cid", [None, "blind-D64-L133", "bern-D64-L133", "edges-D128-L133", "blind-D24-L133-p0.1"])
def test_probe_reports_what_the_product_kernels_applied(cid):
    """per-head P times V in float64 against the same rows of ops.attn_fwd_raw's o, at the attention tests' tolerance TOL_ATTN.
    That tolerance belongs to the bf16-faithful restatement (oracle/torch_ref.py::attention_bf16): the product kernels round the
    unnormalised probabilities 2^(s log2 e - M) to bf16 before P.V and divide by the fp32 row sum afterwards.  The probe's P is
    put through the same two steps, with the row's scalar `flash_sum` from the float64 scores: o = (bf16(P * flash_sum) V) / flash_sum."""
    from dreamvla_amd import ops
    if cid is None:
        vis, mt, L, D = None, None, 212, 64
    else:
        case = MC.BY_ID[cid]
        vis, _, mt = MC.tables(case, device=DEV)
        L, D = case["Lq"], case["D"]
    B, H, R = 2, 3, 32
    q, k, v = _inputs(B, L, L, H, D, "packed", seed=3)
    scale = 1.0 / math.sqrt(D)
    rows = _rows(B, R, L, seed=4)
    P = _run(q, k, rows, scale, mt, True).double().cpu()                                # (B, H, R, L)
    o, _ = ops.attn_fwd_raw(q, k, v, scale=scale, mask_tables=mt, want_lse=False, head_dim=D)
    ref = PR.probabilities(q.float().cpu().numpy(), k.float().cpu().numpy(), rows, scale, vis)
    fs = torch.from_numpy(ref["flash_sum"]).unsqueeze(-1)                                # (B, H, R, 1)
    Pt = (P * fs).float().to(BF).double()
    pv = torch.einsum("bhrl,blhd->bhrd", Pt, v.double().cpu()) / torch.where(fs > 0, fs, torch.ones_like(fs))
    pv = pv.permute(0, 2, 1, 3)                                                           # (B, R, H, D)
    idx = torch.from_numpy(rows).long()
    o_rows = torch.stack([o[b, idx[b]] for b in range(B)]).float().cpu()                # (B, R, H, D)
    m = metrics(f"probe P.V vs attn_fwd o ({cid or 'unmasked L212'})", o_rows, pv.float(), TOL_ATTN)
    print(m)
    report([m])
    assert m["ok"], m


def test_packed_wrapper_and_unsupported_shapes():
    from dreamvla_amd import _lib, ops
    import ctypes as C
    q, k, _ = _inputs(2, 33, 33, 3, 64, "packed", seed=1)
    qkv = torch.stack((q, k, k), dim=2).reshape(2, 33, 3 * 3 * 64).contiguous()
    rows = torch.from_numpy(_rows(2, 3, 33, seed=1)).to(DEV)
    a = ops.self_attention_probe(qkv, 3, rows, head_dim=64)
    b = ops.attention_probe(q, k, rows, scale=0.125)
    assert torch.equal(a, b)
    # the library's own limits: DVLA_ERR_UNSUPPORTED before any launch, the output untouched
    lib = _lib.load()
    out = torch.full((2, 3, 33), 7.0, device=DEV)
    ws = torch.empty((2, 3, 3, 33), device=DEV)
    p = _lib.AttnParams()
    p.q, p.k = q.data_ptr(), k.data_ptr()
    for n, t in (("q", q), ("k", k)):
        setattr(p, n + "_stride_b", t.stride(0)); setattr(p, n + "_stride_t", t.stride(1)); setattr(p, n + "_stride_h", t.stride(2))
    p.B, p.H, p.Lq, p.Lk, p.scale = 2, 3, 33, 33, 0.125
    stream = torch.cuda.current_stream().cuda_stream
    for R, D in ((0, 64), (33, 64), (3, 4), (3, 136), (3, 20)):
        rc = lib.dvla_attn_probe(C.byref(p), rows.data_ptr(), R, D, 33, 0, out.data_ptr(), ws.data_ptr(), stream)
        assert rc == -3, (R, D, rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
