"""Kernel-level parity checks: HIP path (through the C ABI) vs oracle/torch_ref.py on identical seeded inputs.

Each check returns a dict of error metrics and a `ok` flag; tests/test_kernels_gpu.py asserts on them and
tests/gpu_diag.py dumps all of them into gpurun_out/ in one go (no stop at first failure).

Tolerances (written here, used everywhere):
  * bf16 outputs are compared with the fp32 oracle result rounded to bf16:   rel-L2 <= 1e-3
  * fp32 outputs (GEMM with fp32 C, LayerNorm statistics, LSE):              rel-L2 <= 1e-5 / abs 1e-4
  * attention outputs vs oracle/torch_ref.py::attention_bf16 -- the restatement that rounds the probabilities (P.V operand)
    and the score gradients (dQ / dK operand) to bf16 exactly where the kernels do:           rel-L2 <= 1e-3
    attention gradients vs the same:                                                          rel-L2 <= 2e-3
    (round 2 compared with the unrounded fp32 restatement and had to allow 3e-3 / 4e-3 for those two roundings -- the SDPA
    flash backend the reference dispatches to has them too; that comparison is still made, as the link to the
    reference-pinned fp32 oracle, and recorded under the names "... (fp32 oracle)")
  * other gradients (bf16, through bf16-rounded intermediates):              rel-L2 <= 4e-3
rel-L2 = ||a - b||_2 / max(||b||_2, tiny).
"""
import math
import os

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import torch

from oracle import torch_ref as R

TOL_FWD = 1e-3
TOL_F32 = 1e-5
TOL_GRAD = 4e-3
TOL_ATTN = 1e-3          # vs the bf16-faithful oracle
TOL_ATTN_GRAD = 2e-3
TOL_ATTN_F32 = 3e-3      # vs the unrounded fp32 oracle (bf16 P not modelled)
DEV = "cuda"
BF = torch.bfloat16


def rel_l2(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def elem_ulps(tol):
    """element-wise budget that goes with a rel-L2 tolerance class, in bf16 ulps (2^-8) of the reference's largest
    magnitude: 2 for single-op bf16 outputs (one rounding flip of an intermediate + the final rounding), more where bf16
    intermediates are part of the op (attention probabilities, gradients through them) or of a multi-layer pipeline.  A
    misplaced row / tile is off by ~256 ulps on this scale, which a rel-L2 over a large output cannot see."""
    for t, k in ((1e-3, 2.0), (3e-3, 6.0), (4e-3, 8.0), (1e-2, 16.0), (2e-2, 24.0), (3e-2, 32.0)):
        if tol <= t:
            return k
    return 48.0


def metrics(name, got, ref, tol, round_ref=True, k_ulp=None):
    """two criteria, both must hold: rel-L2 <= tol, and max |got - ref| <= k_ulp * 2^-8 * max |ref| (bf16 outputs) or
    <= 2e-4 * max |ref| (fp32 outputs: summation-order differences only)."""
    ref_c = R.bf16_round(ref) if round_ref else ref
    g = got.detach().float().cpu()
    r = rel_l2(g, ref_c)
    d = (g - ref_c).abs()
    finite = bool(torch.isfinite(g).all())
    idx = int(d.flatten().argmax()) if d.numel() else 0
    max_abs = float(d.max()) if d.numel() else 0.0
    absmax = float(ref_c.abs().max()) if d.numel() else 0.0
    if round_ref:
        k = elem_ulps(tol) if k_ulp is None else k_ulp
        elem_tol = k * 2.0 ** -8 * absmax + 1e-30
    else:
        k = None
        elem_tol = (2e-4 if tol <= 1e-4 else 20 * tol) * absmax + 1e-6
    return {"name": name, "rel_l2": r, "max_abs": max_abs, "ref_absmax": absmax, "max_abs_tol": elem_tol, "k_ulp": k,
            "worst_index": idx, "shape": list(g.shape), "finite": finite, "tol": tol,
            "ok": bool(finite and r <= tol and max_abs <= elem_tol)}


def rnd(shape, gen, scale=1.0):
    """bf16-representable fp32 CPU tensor."""
    return R.bf16_round(torch.randn(shape, generator=gen) * scale)


# ---------------------------------------------------------------------------------------------------
def check_gemm(M, N, K, a_trans=False, b_trans=False, bias=False, act="none", residual=False, out_f32=False,
               split_k=1, dropout_p=0.0, dact=None, want_preact=False, seed=0, variant=None):
    from dreamvla_amd import ops
    from dreamvla_amd._lib import ACT
    g = torch.Generator().manual_seed(1234 + seed)
    A = rnd((M, K), g)
    B = rnd((N, K), g, 1.0 / math.sqrt(max(K, 1)))
    bias_t = rnd((N,), g) if bias else None
    res_t = rnd((M, N), g) if residual else None
    aux_t = rnd((M, N), g) if dact else None
    a_dev = (A.t().contiguous() if a_trans else A).to(DEV, BF)
    b_dev = (B.t().contiguous() if b_trans else B).to(DEV, BF)
    sd = (77, 4242)
    with ops.forward_split_k(), torch.no_grad():      # (the rule of the rollout engine: a no-op for every other case here)
        r = ops.gemm(a_dev, b_dev, a_trans=a_trans, b_trans=b_trans,
                     bias=None if bias_t is None else bias_t.to(DEV, BF), act=ACT[act], want_preact=want_preact,
                     dact_aux=None if aux_t is None else aux_t.to(DEV, BF), dact=ACT[dact] if dact else 0,
                     dropout_p=dropout_p, seed=sd, residual=None if res_t is None else res_t.to(DEV, BF),
                     out_dtype=torch.float32 if out_f32 else BF, split_k=split_k, variant=variant)
    got, pre = r if want_preact else (r, None)
    ref = A @ B.t()
    if bias:
        ref = ref + bias_t
    out = []
    if want_preact:
        out.append(metrics("preact", pre, ref, TOL_FWD))
        ref = R.bf16_round(ref)
    ref = R.act(ref, act)
    if dropout_p > 0:
        ref = R.dropout_elementwise(ref, dropout_p, sd)
    # the reference materialises `dropout(act(linear(x)))` / `dY @ W` as a bf16 tensor BEFORE the residual add /
    # the act' multiply (models/gpt2.py:329-339, autograd of gpt2.py:296-301): one rounding in between
    if (dact or residual) and not out_f32:
        ref = R.bf16_round(ref)
    if dact:
        x = aux_t.clone().requires_grad_(True)
        R.act(x, dact).sum().backward()
        ref = ref * x.grad
    if residual:
        ref = ref + res_t
    tag = f"gemm{'' if variant is None else ' v%d' % variant} M{M} N{N} K{K} at{int(a_trans)} bt{int(b_trans)} bias{int(bias)} {act} res{int(residual)} f32{int(out_f32)} sk{split_k} p{dropout_p} dact{dact}"
    out.insert(0, metrics(tag, got, ref, TOL_F32 if out_f32 else TOL_FWD, round_ref=not out_f32))
    return out


def check_gemm_wide_stride(variant=7, M=300, N=256, K=128, stride=8_500_000):
    """round-5 ADVICE: the ring kernels address a DMA piece as a 32-bit byte offset from the tile's origin.  A k-contiguous operand
    that is a VIEW into a wider buffer (row stride `stride` elements: row 255 of a tile lies 4.3 GB behind row 0) cannot be addressed
    that way: the dispatcher has to hand the problem to the register-staged kernel (64-bit addressing) -- same values as for a
    contiguous copy of the operand, `dvla_last_gemm_variant() == 2`."""
    from dreamvla_amd import ops
    from dreamvla_amd._lib import load
    g = torch.Generator().manual_seed(77)
    A = rnd((M, K), g)
    B = rnd((N, K), g, 1.0 / math.sqrt(K))
    big = torch.empty((M - 1) * stride + K, device=DEV, dtype=BF)          # 5.1 GB: only the M x K window is ever touched
    a_view = torch.as_strided(big, (M, K), (stride, 1))
    a_view.copy_(A.to(DEV, BF))
    with torch.no_grad():
        got = ops.gemm(a_view, B.to(DEV, BF), variant=variant)
    ran = int(load().dvla_last_gemm_variant())
    out = [metrics(f"gemm v{variant} forced on a k-contiguous operand with a row stride of {stride} elements", got, A @ B.t(), TOL_FWD)]
    out.append({"name": f"  ... ran the register-staged kernel (last variant {ran})", "rel_l2": 0.0, "tol": 0.0, "ok": ran == 2})
    del big
    torch.cuda.empty_cache()
    return out


def check_gemm_retired_variant(variant, M=256, N=256, K=128):
    """a forced variant number that names nothing -- 44 and 85 were measurement builds of the phase kernel (NN layout, plain
    epilogue) until they were removed -- selects nothing but the fallback: right values from the register-staged kernel,
    `dvla_last_gemm_variant() == 2`.  The shape is the smallest the phase kernel takes (one 256 x 256 tile, two K-tiles)."""
    from dreamvla_amd._lib import load
    out = check_gemm(M=M, N=N, K=K, variant=variant)
    ran = int(load().dvla_last_gemm_variant())
    out.append({"name": f"  ... retired variant {variant} ran the register-staged kernel (last variant {ran})", "rel_l2": 0.0, "tol": 0.0,
                "ok": ran == 2})
    return out


# the whole-line epilogue of the ring / phase kernels addresses a wave's window of at most 128 rows (csrc/gemm_impl.h
# EPI_WINDOW_ROWS) with 32-bit byte offsets: the smallest bf16 row stride, in whole 16-byte vectors, at which the window's last
# row lies >= 4 GiB behind its first -- (128 - 1) * stride * 2 >= 2^32 -> 16 909 328 elements
WINDOW_ROWS = 128
WIDE_OUT_STRIDE = (-(-(1 << 32) // (2 * (WINDOW_ROWS - 1))) + 7) // 8 * 8


def check_gemm_wide_stride_out(variant=4, which="out", M=256, N=256, K=128):
    """the output side of check_gemm_wide_stride: `out=` (which = "out") or `residual` (which = "residual") is a view whose row stride
    is WIDE_OUT_STRIDE = 16 909 328 elements, the smallest multiple of 8 at which row 127 of a wave's 128-row window lies >= 4 GiB
    behind row 0 (127 x 16 909 328 x 2 B = 2^32 + 2016).  The ring / phase kernels' RowWindow (32-bit byte offsets) cannot reach
    that row; the dispatcher's bound (csrc/gemm.hip ring_ok, one bound for every configuration: the tallest window) has to hand the
    problem to the register-staged kernel, which addresses in 64 bits -- the kernel the operand-side case already runs at such
    strides.  Right values, every element of the M x N window written, `dvla_last_gemm_variant() == 2`.  The backing buffer covers
    all M rows in full (M x stride elements, 8.66 GB) and is freed before the case returns."""
    from dreamvla_amd import ops
    from dreamvla_amd._lib import load
    stride = WIDE_OUT_STRIDE
    g = torch.Generator().manual_seed(78)
    A = rnd((M, K), g)
    B = rnd((N, K), g, 1.0 / math.sqrt(K))
    res = rnd((M, N), g)
    ref = A.double() @ B.double().t()
    big = torch.empty(M * stride, device=DEV, dtype=BF)
    view = torch.as_strided(big, (M, N), (stride, 1))
    with torch.no_grad():
        if which == "out":
            view.fill_(float("nan"))          # an element the kernel does not write stays non-finite
            got = ops.gemm(A.to(DEV, BF), B.to(DEV, BF), out=view, variant=variant)
        else:
            view.copy_(res.to(DEV, BF))
            got = ops.gemm(A.to(DEV, BF), B.to(DEV, BF), residual=view, variant=variant)
            ref = R.bf16_round(ref).double() + res.double()
    ran = int(load().dvla_last_gemm_variant())
    got = got.float().cpu()
    tag = f"gemm v{variant} forced, {which} a view with a row stride of {stride} elements"
    out = [metrics(tag, got, ref, TOL_FWD),
           {"name": tag + ": window fully written", "rel_l2": 0.0, "tol": 0.0, "ok": bool(torch.isfinite(got).all())},
           {"name": tag + f": ran the register-staged kernel (last variant {ran})", "rel_l2": 0.0, "tol": 0.0, "ok": ran == 2}]
    del big, view
    torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------------------------------------------
# GEMM addressing: operands, outputs and epilogue operands as VIEWS into wider buffers (own leading dimension and origin each),
# the periodic residual, the fp32 bias.  tests/test_gemm_addressing_gpu.py holds the case matrix, tests/test_gemm_views.py checks
# the helpers themselves on the CPU.
# ---------------------------------------------------------------------------------------------------
VIEW_SENTINEL = -6.625      # finite, exact in bf16 and fp32; the backing buffers are filled with it before a call
ERR_UNSUPPORTED = -3        # csrc/common.h DVLA_ERR_UNSUPPORTED


def make_view(rows, cols, pad=0, offset=0, dtype=BF, device="cpu", lead_rows=2, trail_rows=2, sentinel=VIEW_SENTINEL):
    """-> (backing, view): a rows x cols window with leading dimension cols + pad inside a 1-D buffer filled with `sentinel`.  The
    window's origin lies `offset` elements behind a 128-byte boundary that has at least `lead_rows` rows of the buffer in front of
    it; `trail_rows` rows follow the last one.  (offset % 8 == 0 and pad % 8 == 0 -- fp32: % 4 -- give what the vector paths need.)"""
    ld = cols + pad
    origin = -(-(lead_rows * ld) // 64) * 64 + offset
    backing = torch.full((origin + (rows + trail_rows) * ld,), sentinel, dtype=dtype, device=device)
    return backing, torch.as_strided(backing, (rows, cols), (ld, 1), origin)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def window_mask(backing, view):
    """bool per element of `backing`: inside the rows x cols window `view` covers"""
    origin = view.storage_offset() - backing.storage_offset()
    rows, cols = view.shape
    ld = max(int(view.stride(0)), 1)
    idx = torch.arange(backing.numel(), device=backing.device) - origin
    return (idx >= 0) & (idx < (rows - 1) * ld + cols) & (idx % ld < cols)


def outside_window_intact(backing, view, sentinel=VIEW_SENTINEL):
    """every element of `backing` outside the window of `view` (padding columns, rows before / after, the elements left and right
    of an offset origin) is bit-identical to the sentinel; view = None: the whole buffer"""
    want = int(_bits(torch.tensor([sentinel], dtype=backing.dtype))[0])
    bad = _bits(backing) != want
    if view is not None:
        bad &= ~window_mask(backing, view)
    n = int(bad.sum())
    return {"ok": n == 0, "bad": n, "first_bad": int(bad.nonzero()[0]) if n else -1}


_VIEW_DATA = {}


def _view_case_data(M, N, K, seed=0):
    """seeded operands of a view case + their float64 product, computed once per shape and shared (never modified)"""
    key = (M, N, K, seed)
    if key not in _VIEW_DATA:
        if len(_VIEW_DATA) >= 8:
            _VIEW_DATA.clear()
        g = torch.Generator().manual_seed(9000 + seed)
        d = {"A": rnd((M, K), g), "B": rnd((N, K), g, 1.0 / math.sqrt(K)), "bias": rnd((N,), g), "res": rnd((M, N), g),
             "aux": rnd((M, N), g), "c0": rnd((M, N), g)}
        d["bias32"] = (d["bias"] * 1.0009765625).float()        # fp32 master values that are NOT bf16-representable
        d["prod"] = d["A"].double() @ d["B"].double().t()
        _VIEW_DATA[key] = d
    return _VIEW_DATA[key]


# (pad, origin offset) in elements of every view of an ALIGNED case: all different, all whole 16-byte vectors
ALIGNED_VIEWS = {"a": (8, 8), "b": (16, 24), "out": (24, 16), "res": (40, 8), "aux": (8, 32), "bias": (0, 8), "preact": (56, 40)}


def _gemm_call(lib, variant, a, b, out, M, N, K, a_trans, b_trans, bias, act, preact, aux, dact, dropout_p, seed, res, res_rows,
               accumulate, split_k):
    """dvla_gemm_bf16 through ctypes (every leading dimension as the tensors have it) -> (return code, what ran)"""
    import ctypes as C
    from dreamvla_amd import ops
    from dreamvla_amd._lib import ACT, GemmParams
    p = GemmParams()
    p.A, p.lda, p.a_trans = a.data_ptr(), a.stride(0), int(a_trans)
    p.B, p.ldb, p.b_trans = b.data_ptr(), b.stride(0), int(b_trans)
    p.C, p.ldc, p.c_dtype = out.data_ptr(), out.stride(0), 1 if out.dtype == torch.float32 else 0
    p.M, p.N, p.K = M, N, K
    if bias is not None:
        p.bias, p.bias_dtype = bias.data_ptr(), 1 if bias.dtype == torch.float32 else 0
    p.act = ACT[act]
    if preact is not None:
        p.preact, p.ld_preact = preact.data_ptr(), preact.stride(0)
    if aux is not None:
        p.dact_aux, p.ld_dact, p.dact = aux.data_ptr(), aux.stride(0), ACT[dact]
    p.dropout_p, p.seed_lo, p.seed_hi = float(dropout_p), seed[0], seed[1]
    if res is not None:
        p.residual, p.ld_res, p.res_rows = res.data_ptr(), res.stride(0), int(res_rows)
    p.accumulate, p.split_k = int(accumulate), int(split_k)
    ws = torch.empty((split_k, M, N), dtype=torch.float32, device=a.device) if split_k > 1 else None
    if ws is not None:
        p.workspace = ws.data_ptr()
    lib.dvla_set_gemm_variant(int(variant or 0))
    try:
        rc = int(lib.dvla_gemm_bf16(C.byref(p), ops._stream()))
    finally:
        lib.dvla_set_gemm_variant(0)
    torch.cuda.synchronize()          # (the workspace outlives the launches)
    return rc, (int(lib.dvla_last_gemm_variant()) if rc == 0 else None)


def check_gemm_views(M, N, K, a_trans=False, b_trans=False, bias=None, act="none", residual=False, res_rows=0, out_f32=False,
                     accumulate=False, split_k=1, dropout_p=0.0, dact=None, want_preact=False, variant=None, expect=None,
                     views=None, expect_rc=0, via_ops=False, seed=0):
    """check_gemm with every tensor a view into a wider, sentinel-filled buffer: A, B, `out`, the pre-activation, the residual
    (res_rows > 0: a table of that many rows, row m % res_rows added to output row m), the act' operand and the bias
    ("bf16" / "f32").  `views` overrides (pad, origin offset) per tensor (ALIGNED_VIEWS otherwise).  The library is called through
    ctypes (own ld_preact); via_ops: through ops.gemm(out=...) inside `with ops.forward_split_k()` instead.
    Asserted: (1) the values against the float64 product of the bf16 operand values run through the epilogue oracle, tolerances
    of check_gemm; (2) every element of the backing buffers of `out` / the pre-activation outside their M x N windows is
    bit-identical to the sentinel, and no input buffer changed; (3) if a call on contiguous copies of the same data reports the
    same dvla_last_gemm_variant(), its results are torch.equal (strides do not change summation order); (4) `expect`: the
    configuration that ran.  expect_rc != 0: the call must return that code and write nothing at all."""
    from dreamvla_amd import _lib, ops
    from dreamvla_amd._lib import ACT
    lib = _lib.load()
    d = _view_case_data(M, N, K, seed)
    vw = dict(ALIGNED_VIEWS, **(views or {}))
    sd = (77, 4242)
    odt = torch.float32 if out_f32 else BF

    def view_of(name, src, dtype=BF):
        src = src.view(1, -1) if src.dim() == 1 else src
        backing, v = make_view(src.shape[0], src.shape[1], vw[name][0], vw[name][1], dtype, DEV)
        v.copy_(src.to(DEV, dtype))
        return backing, v

    a_b, a_v = view_of("a", d["A"].t() if a_trans else d["A"])
    b_b, b_v = view_of("b", d["B"].t() if b_trans else d["B"])
    inputs = {"A": a_b, "B": b_b}
    bias_v = res_v = aux_v = pre_b = pre_v = None
    bias_val = None
    if bias:
        bias_val = d["bias32"] if bias == "f32" else d["bias"]
        inputs["bias"], bias2 = view_of("bias", bias_val, torch.float32 if bias == "f32" else BF)
        bias_v = bias2[0]
    if residual:
        inputs["residual"], res_v = view_of("res", d["res"][:res_rows] if res_rows > 0 else d["res"])
    if dact:
        inputs["dact_aux"], aux_v = view_of("aux", d["aux"])
    out_b, out_v = make_view(M, N, vw["out"][0], vw["out"][1], odt, DEV)
    if accumulate:
        out_v.copy_(d["c0"].to(DEV, odt))
    if want_preact:
        pre_b, pre_v = make_view(M, N, vw["preact"][0], vw["preact"][1], BF, DEV)
    before = {k: v.clone() for k, v in inputs.items()}
    common = dict(M=M, N=N, K=K, a_trans=a_trans, b_trans=b_trans, act=act, dact=dact, dropout_p=dropout_p, seed=sd,
                  res_rows=res_rows, accumulate=accumulate)
    opts = [f"bias-{bias}" if bias else "", act if act != "none" else "", "preact" if want_preact else "", f"p{dropout_p}" if dropout_p else "",
            f"dact-{dact}" if dact else "", ("res%" + str(res_rows) if res_rows else "res") if residual else "", "f32" if out_f32 else "",
            "acc" if accumulate else "", f"sk{split_k}" if split_k > 1 else "", "via-ops" if via_ops else ""]
    opts += [f"{k}:{v[0]}+{v[1]}" for k, v in sorted((views or {}).items())]
    tag = (f"gemm views v{0 if variant is None else variant} {M}x{N}x{K} {'NT'[int(a_trans)]}{'NT'[int(b_trans)]} " + " ".join(o for o in opts if o)).rstrip()
    out = []
    if via_ops:       # the opportunistic forward split: must run UNSPLIT when the reduction pass cannot vectorise, and be right
        would = ops.fwd_split_k(M, N, K) > 1 and not ops._fwd_split_epilogue_ok(out_v, bias_v, res_v, N)
        out.append({"name": tag + ": a split the rule would take, refused for its epilogue operands", "rel_l2": 0.0, "tol": 0.0, "ok": bool(would)})
        with ops.forward_split_k(), torch.no_grad():
            ops.gemm(a_v, b_v, a_trans=a_trans, b_trans=b_trans, bias=bias_v, act=ACT[act], residual=res_v, res_rows=res_rows, out=out_v)
        torch.cuda.synchronize()
        rc, ran = 0, int(lib.dvla_last_gemm_variant())
    else:
        rc, ran = _gemm_call(lib, variant, a_v, b_v, out_v, bias=bias_v, preact=pre_v, aux=aux_v, res=res_v, split_k=split_k, **common)
    if expect_rc != 0:
        clean = outside_window_intact(out_b, None)
        return [{"name": tag + f": return code {rc} (expected {expect_rc})", "rel_l2": 0.0, "tol": 0.0, "ok": rc == expect_rc},
                {"name": tag + f": nothing written ({clean['bad']} elements changed)", "rel_l2": 0.0, "tol": 0.0, "ok": clean["ok"]}]
    out.append({"name": tag + f": return code {rc}", "rel_l2": 0.0, "tol": 0.0, "ok": rc == 0})
    if rc != 0:
        return out
    # (1) values
    ref = d["prod"]
    if bias:
        ref = ref + bias_val.double()
    pre_ref = ref
    if want_preact:
        ref = R.bf16_round(ref).double()
    ref = R.act(ref, act)
    if dropout_p > 0:
        ref = R.dropout_elementwise(ref, dropout_p, sd)
    if (dact or residual) and not out_f32:
        ref = R.bf16_round(ref).double()
    if dact:
        x = d["aux"].double().requires_grad_(True)
        R.act(x, dact).sum().backward()
        ref = ref * x.grad
    if residual:
        ref = ref + (d["res"][torch.arange(M) % res_rows] if res_rows > 0 else d["res"]).double()
    if accumulate:
        ref = ref + d["c0"].double()
    out.append(metrics(tag, out_v, ref, TOL_F32 if out_f32 else TOL_FWD, round_ref=not out_f32))
    if want_preact:
        out.append(metrics(tag + " preact", pre_v, pre_ref, TOL_FWD))
    # (2) nothing outside the windows written, no input touched
    for name, (bk, v) in {"out": (out_b, out_v), "preact": (pre_b, pre_v)}.items():
        if bk is not None:
            s = outside_window_intact(bk, v)
            out.append({"name": tag + f": buffer around `{name}` intact ({s['bad']} elements changed, first at {s['first_bad']})",
                        "rel_l2": float(s["bad"]), "tol": 0.0, "ok": s["ok"]})
    changed = [k for k, v in inputs.items() if not torch.equal(_bits(v), _bits(before[k]))]
    out.append({"name": tag + f": input buffers unchanged (changed: {changed})", "rel_l2": float(len(changed)), "tol": 0.0, "ok": not changed})
    # (3) the same data contiguous: same configuration -> same bits (via_ops: the configuration that ran, forced and UNSPLIT -- a
    # forward split that was taken after all would sum in another order)
    cont = lambda t: None if t is None else torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)    # a fresh allocation
    out_c = torch.empty((M, N), dtype=odt, device=DEV)
    if accumulate:
        out_c.copy_(d["c0"].to(DEV, odt))
    pre_c = torch.empty((M, N), dtype=BF, device=DEV) if want_preact else None
    rc_c, ran_c = _gemm_call(lib, ran if via_ops else variant, cont(a_v), cont(b_v), out_c, bias=cont(bias_v), preact=pre_c,
                             aux=cont(aux_v), res=cont(res_v), split_k=1 if via_ops else split_k, **common)
    same = rc_c == 0 and ran_c == ran
    equal = (not same) or (torch.equal(out_v, out_c) and (pre_v is None or torch.equal(pre_v, pre_c)))
    out.append({"name": tag + f": contiguous call ran {ran_c}, strided {ran}" + (": results bit-identical" if same else ": not compared"),
                "rel_l2": 0.0, "tol": 0.0, "ok": bool(rc_c == 0 and equal), "compared": bool(same), "ran": ran})
    # (4) what ran
    if expect is not None:
        out.append({"name": tag + f": configuration {expect} ran (dvla_last_gemm_variant = {ran})", "rel_l2": 0.0, "tol": 0.0,
                    "ok": ran == expect, "ran": ran})
    return out


def check_gemm_skinny(forced=True, **kw):
    """the few-rows kernel (csrc/gemm_skinny.h: M <= 512, k-contiguous operands -- the shapes of a single-episode control step):
    the same oracle as every other configuration, plus the assertion that it is what ran (forced = variant 11; not forced = the
    library's own choice for such a problem must be this kernel)"""
    from dreamvla_amd import _lib
    out = check_gemm(variant=11 if forced else None, **kw)
    ran = int(_lib.load().dvla_last_gemm_variant())
    out.append({"name": f"gemm skinny M{kw['M']} N{kw['N']} K{kw['K']}: few-rows kernel ran (dvla_last_gemm_variant = {ran})", "rel_l2": 0.0,
                "tol": 0.0, "ok": ran == 11})
    return out


def check_act_bwd_colsum(rows, cols, act="none", dropout_p=0.0, out_bf16=False, seed=0):
    """dvla_act_bwd_colsum: dropout / activation backward and the bias gradient (column sums of dz) in one pass -- dz bit-identical
    to dvla_act_bwd's, the sums against an fp64 sum of those stored values"""
    from dreamvla_amd import ops
    from dreamvla_amd._lib import ACT
    g = torch.Generator().manual_seed(99 + seed)
    dy = rnd((rows, cols), g).to(DEV, BF)
    pre = rnd((rows, cols), g).to(DEV, BF) if act != "none" else None
    sd = (123, 456)
    dz_ref = ops.act_bwd_raw(dy, pre, ACT[act], dropout_p, sd)
    r = ops.act_bwd_colsum(dy, pre, ACT[act], dropout_p, sd, BF if out_bf16 else torch.float32)
    tag = f"act_bwd+colsum {rows}x{cols} {act} p{dropout_p} bf16out{int(out_bf16)}"
    if r is None:
        return [{"name": tag + ": shape not taken", "rel_l2": 0.0, "tol": 0.0, "ok": cols % 8 != 0}]
    dz, db = r
    want = dz_ref.double().sum(0).float().cpu()
    return [{"name": tag + " dz bit-identical to dvla_act_bwd", "rel_l2": 0.0, "tol": 0.0, "ok": bool(torch.equal(dz, dz_ref))},
            metrics(tag + " column sums", db, want, TOL_FWD if out_bf16 else 1e-5, round_ref=out_bf16)]


def check_dit_team(bs=1, model_type="DiT-B", seeds=(0, 1, 2, 3), call_per_phase=False, fp32_master=False):
    """dvla_dit_sample -- the evaluation sampler (DDIM-10 + CFG through all DiT blocks) as one persistent kernel on one XCD --
    against the launch-by-launch sampler (ActionModel.sample_ddim_cfg with team_sampler = False: few-rows GEMMs, flash attention,
    dvla_ddim_cfg_step) and the fp32 oracle of the loop (oracle/model_ref.py ddim_sample, the model's bf16 weights in fp32).
    Both HIP paths are bf16 computations of the same function with the same rounding points; ten sampler steps amplify their
    rounding noise alike, so the persistent kernel's deviation from the fp32 samples may be at most 1.5 x the launch-by-launch
    path's (pooled over the seeds) -- and it must be bit-reproducible, finish every exchange, and run on one XCC.
    fp32_master (round-4 ADVICE): the parameters stay fp32 masters (`--precision fp32`, every shipped script); the launch-by-launch
    path then hands the fp32 BIASES to the GEMM epilogues while the persistent kernel reads their bf16 shadows -- one more rounding
    of a bias (relative 2^-9 of the bias value), the same bounds must hold."""
    from dreamvla_amd import ops
    from dreamvla_amd.action_model.action_model import ActionModel
    from oracle import model_ref, weights
    if call_per_phase:          # the library reads DVLA_DIT_AHEAD once per process: this variant runs in a process of its own
        import subprocess, sys, json
        code = ("import json, sys; sys.path.insert(0, %r); from tests import gpu_checks; "
                "print('RESULT' + json.dumps(gpu_checks.check_dit_team(bs=%d, model_type=%r, seeds=%r)))" % (ROOT_DIR, bs, model_type, tuple(seeds)))
        env = dict(os.environ, DVLA_DIT_AHEAD="0")
        env.pop("DVLA_PARITY_REPORT", None)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
        if not line:
            return [{"name": f"dit_team call-per-phase kernel: subprocess failed: {r.stderr[-300:]}", "rel_l2": 0.0, "tol": 0.0, "ok": False}]
        out = json.loads(line[0][6:])
        for m in out:
            m["name"] = m["name"].replace("dit_team", "dit_team (call-per-phase kernel)")
        return out
    depth, heads = {"DiT-B": (12, 12), "DiT-L": (24, 16)}[model_type]
    am = ActionModel(token_size=1024, model_type=model_type, in_channels=7, future_action_window_size=2, past_action_window_size=0)
    am.load_state_dict(weights.fill_state_dict(am.state_dict()), strict=True)
    if fp32_master:       # values that are NOT bf16-representable: shadows (weights: both paths; biases: the team kernel) really round
        am.load_state_dict({k: (v * 1.0009765625 if v.is_floating_point() else v) for k, v in am.state_dict().items()})
        am = am.to(DEV).eval()
        # the oracle computes on what the kernels' GEMMs compute on: bf16-rounded weight matrices, fp32 biases / vectors
        sd32 = {k: (v.to(BF).float() if v.dim() >= 2 else v.float()).cpu() for k, v in am.state_dict().items()}
    else:
        am = am.to(BF).to(DEV).eval()
        sd32 = {k: v.float().cpu() for k, v in am.state_dict().items()}
    am.create_ddim(10)
    tag = f"dit_team {model_type} bs{bs}" + (" fp32 masters" if fp32_master else "")
    hidden = am.net.x_embedder.linear.out_features
    taken = ops.dit_team_ok(hidden, heads, 7, 3, bs, torch.device(DEV, torch.cuda.current_device()))
    res = [{"name": tag + ": shape taken by the persistent kernel", "rel_l2": 0.0, "tol": 0.0, "ok": bool(taken)}]
    num_t = num_l = num_p = den = 0.0
    worst_pair = 0.0
    for sd in seeds:
        g = torch.Generator().manual_seed(700 + sd)
        cond = rnd((bs, 3, 1024), g).to(DEV, BF)
        noise = rnd((bs, 3, 7), g).to(BF).float().to(DEV)
        if fp32_master:
            cond = cond.float()
        am.team_sampler = True
        out_t = am.sample_ddim_cfg(cond, noise, 1.5)
        out_t2 = am.sample_ddim_cfg(cond, noise, 1.5)
        am.team_sampler = False
        out_l = am.sample_ddim_cfg(cond, noise, 1.5)
        with torch.no_grad():
            ref = model_ref.ddim_sample(sd32, "net", cond.float().cpu(), noise.cpu(), 1.5, depth=depth, heads=heads)
        if sd == seeds[0]:
            res.append({"name": tag + ": finite, bit-reproducible", "rel_l2": 0.0, "tol": 0.0,
                        "ok": bool(torch.isfinite(out_t).all()) and bool(torch.equal(out_t, out_t2))})
        t, l = out_t.float().cpu(), out_l.float().cpu()
        num_t += float(((t - ref) ** 2).sum()); num_l += float(((l - ref) ** 2).sum()); num_p += float(((t - l) ** 2).sum())
        den += float((ref ** 2).sum())
        worst_pair = max(worst_pair, float((t - l).abs().max()))
    e_t, e_l, e_p = (num_t / den) ** 0.5, (num_l / den) ** 0.5, (num_p / den) ** 0.5
    res.append({"name": tag + f": rel-L2 to the fp32 samples, persistent kernel (launch-by-launch: {e_l:.3e})", "rel_l2": e_t,
                "tol": 1.5 * e_l + 1e-3, "ok": e_t <= 1.5 * e_l + 1e-3})
    res.append({"name": tag + ": persistent kernel vs launch-by-launch", "rel_l2": e_p, "tol": 2.5 * e_l + 1e-3, "max_abs": worst_pair,
                "ok": e_p <= 2.5 * e_l + 1e-3})
    mask = int(getattr(am, "team_xcc_mask", 0))
    res.append({"name": tag + f": team ran on one XCC (mask {mask:#x})", "rel_l2": float(bin(mask).count("1")), "tol": 1.0,
                "ok": bin(mask).count("1") == 1})
    return res


def check_gemm_tail(**kw):
    """the phase kernel with a PARTIAL last K-tile (gemm_phase.h DBG & 128: K % 64 = 16 / 32 / 48, k-major operands, fp32 class):
    forced configuration 8 + the assertion that it ran -- before round 4 such a problem fell back to the BK-32 ring kernel"""
    from dreamvla_amd import _lib
    out = check_gemm(variant=8, a_trans=True, b_trans=True, **kw)
    ran = int(_lib.load().dvla_last_gemm_variant())
    out.append({"name": f"gemm K-tail M{kw['M']} N{kw['N']} K{kw['K']} sk{kw.get('split_k', 1)}: phase kernel ran (dvla_last_gemm_variant = {ran})",
                "rel_l2": 0.0, "tol": 0.0, "ok": ran == 8})
    return out


def check_gemm_ln(M, N, K, bias=True, act="none", residual=False, eps=1e-6, seed=0):
    """dvla_gemm_bf16 with a_layernorm: Linear(LayerNorm(x)) from x in one launch (the DiT blocks' parameter-free LayerNorms at
    evaluation).  Oracle: F.layer_norm without affine -> rounded to bf16 (what dvla_layernorm_fwd_rows writes) -> the GEMM epilogue."""
    from dreamvla_amd import _lib, ops
    from dreamvla_amd._lib import ACT
    g = torch.Generator().manual_seed(4321 + seed)
    A = rnd((M, K), g) * (1.0 + torch.arange(M).float().view(M, 1) % 5) + 0.5        # rows of different scale and a common offset
    A = R.bf16_round(A)
    B = rnd((N, K), g, 1.0 / math.sqrt(K))
    bias_t = rnd((N,), g) if bias else None
    res_t = rnd((M, N), g) if residual else None
    dev = lambda t: None if t is None else t.to(DEV, BF)
    got = ops.gemm(dev(A), dev(B), bias=dev(bias_t), act=ACT[act], residual=dev(res_t), a_ln_eps=eps)
    ran = int(_lib.load().dvla_last_gemm_variant())
    n = R.bf16_round(R.layer_norm(A, None, None, eps))
    ref = n @ B.t()
    if bias:
        ref = ref + bias_t
    ref = R.act(ref, act)
    if residual:
        ref = R.bf16_round(ref) + res_t
    tag = f"gemm+layernorm M{M} N{N} K{K} bias{int(bias)} {act} res{int(residual)}"
    # the normalised operand is rounded to bf16 in both; a value that sits on a rounding boundary may flip (stats summed in another order)
    return [metrics(tag, got, ref, 2e-3, k_ulp=4.0),
            {"name": tag + f": few-rows kernel ran ({ran})", "rel_l2": 0.0, "tol": 0.0, "ok": ran == 11}]


def check_gemm_ksum(M, N, K, which, split_k=1, variant=None, a_trans=True, b_trans=True, out_f32=False, ksum_f32=False, seed=0):
    """dvla_gemm_bf16 with ksum_operand: the k-sums of operand `which` ("a": sum_k A(i, k), "b": sum_k B(j, k)) next to the
    product -- the bias gradient of a weight-gradient GEMM (utils/train_utils.py:599-608: autograd's dz.sum(0)).  Oracle: fp32
    sums of the bf16 operand values; tolerance: the bf16 rounding of the result (or 1e-5 for fp32 output)."""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(555 + seed)
    A = R.bf16_round(rnd((M, K), g))
    B = R.bf16_round(rnd((N, K), g, 1.0 / math.sqrt(max(K, 1))) + 0.01)      # a non-zero mean: the sums are not noise
    a_dev = (A.t().contiguous() if a_trans else A).to(DEV, BF)
    b_dev = (B.t().contiguous() if b_trans else B).to(DEV, BF)
    klen = M if which == "a" else N
    kout = torch.full((klen,), float("nan"), dtype=torch.float32 if ksum_f32 else BF, device=DEV)
    got = ops.gemm(a_dev, b_dev, a_trans=a_trans, b_trans=b_trans, out_dtype=torch.float32 if out_f32 else BF, split_k=split_k,
                   variant=variant, ksum=(which, kout))
    ref = A @ B.t()
    kref = (A if which == "a" else B).sum(1)
    tag = f"gemm+ksum({which}){'' if variant is None else ' v%d' % variant} M{M} N{N} K{K} at{int(a_trans)} bt{int(b_trans)} sk{split_k} f32{int(out_f32)}"
    return [metrics(tag, got, ref, TOL_F32 if out_f32 else TOL_FWD, round_ref=not out_f32),
            metrics(tag + " k-sums", kout, kref, 1e-5 if ksum_f32 else TOL_FWD, round_ref=not ksum_f32)]


# the GEMM problems of the benchmarked training step (BASELINE configs[1]: B = 32, S = 7, head set C; profiles/r02_gemm_breakdown.json)
# at FULL size, with their real K and epilogue, under every kernel configuration the tuner locks for them (bench.py's
# tuner_wins_by_problem_key) -- round-2 VERDICT: the forced-variant tests stopped at K <= 448 / M <= 4300, where the stream-K
# schedules never engage and a tile sees 2-7 K-tiles instead of 12-64.  `variants`: 0 = the library's cost model (no assertion
# on what ran), anything else is FORCED and the test asserts through dvla_last_gemm_variant() that it ran (9 / 10 only count
# when the stream-K schedule actually engaged).  Every forced variant runs twice in a row (stream-K scratch / flags reused).
MODEL_GEMMS = {
    "trunk fc1 fwd": dict(M=20832, N=4096, K=1024, b_trans=True, bias=True, act="gelu_tanh", want_preact=True, variants=(8, 9, 10)),
    "trunk fc1 dact": dict(M=20832, N=4096, K=1024, dact="gelu_tanh", variants=(9, 10)),
    "trunk fc2 fwd": dict(M=20832, N=1024, K=4096, b_trans=True, bias=True, residual=True, dropout_p=0.1, variants=(0, 9, 10)),
    "trunk fc2 dX": dict(M=20832, N=1024, K=4096, variants=(9, 10)),
    "trunk c_attn fwd": dict(M=20832, N=3072, K=1024, b_trans=True, bias=True, variants=(8, 10)),
    "trunk c_proj fwd": dict(M=20832, N=1024, K=1024, b_trans=True, bias=True, residual=True, dropout_p=0.1, variants=(0, 7, 10)),
    "vit fc1": dict(M=88256, N=3072, K=768, bias=True, act="gelu_erf", variants=(8, 10)),
    "trunk dW fc1": dict(M=1024, N=4096, K=20832, a_trans=True, b_trans=True, split_k=4, variants=(0, 4, 8)),   # 8: partial last K-tile
    "trunk dW c_attn": dict(M=1024, N=3072, K=20832, a_trans=True, b_trans=True, split_k=5, variants=(8,)),
    "decoder dW fc2": dict(M=4096, N=1024, K=91840, a_trans=True, b_trans=True, split_k=4, variants=(8,)),
    "decoder fc2 dX": dict(M=91840, N=1024, K=4096, b_trans=True, variants=(9, 10)),
}


def check_gemm_model_scale(name):
    from dreamvla_amd import _lib, ops
    from dreamvla_amd._lib import ACT
    c = dict(MODEL_GEMMS[name])
    variants = c.pop("variants")
    M, N, K = c["M"], c["N"], c["K"]
    a_trans, b_trans = c.get("a_trans", False), c.get("b_trans", False)
    act, dact, p_drop = c.get("act", "none"), c.get("dact"), c.get("dropout_p", 0.0)
    want_preact, split_k = c.get("want_preact", False), c.get("split_k", 1)
    g = torch.Generator().manual_seed(4321)
    A = rnd((M, K), g)
    B = rnd((N, K), g, 1.0 / math.sqrt(K))
    bias_t = rnd((N,), g) if c.get("bias") else None
    res_t = rnd((M, N), g) if c.get("residual") else None
    aux_t = rnd((M, N), g) if dact else None
    sd = (77, 4242)
    ref = A @ B.t()
    if bias_t is not None:
        ref += bias_t
    pre_ref = ref.clone() if want_preact else None
    if want_preact:
        ref = R.bf16_round(ref)
    ref = R.act(ref, act)
    if p_drop > 0:
        ref = R.dropout_elementwise(ref, p_drop, sd)
    if dact or res_t is not None:
        ref = R.bf16_round(ref)
    if dact:
        x = aux_t.clone().requires_grad_(True)
        R.act(x, dact).sum().backward()
        ref = ref * x.grad
    if res_t is not None:
        ref = ref + res_t
    dev = lambda t: None if t is None else t.to(DEV, BF)
    a_dev = (A.t().contiguous() if a_trans else A).to(DEV, BF)
    b_dev = (B.t().contiguous() if b_trans else B).to(DEV, BF)
    bias_d, res_d, aux_d = dev(bias_t), dev(res_t), dev(aux_t)
    del A, B
    lib = _lib.load()
    out = []
    for v in variants:
        for rep in range(1 if v == 0 else 2):
            r = ops.gemm(a_dev, b_dev, a_trans=a_trans, b_trans=b_trans, bias=bias_d, act=ACT[act], want_preact=want_preact,
                         dact_aux=aux_d, dact=ACT[dact] if dact else 0, dropout_p=p_drop, seed=sd, residual=res_d,
                         split_k=split_k, variant=v)
            ran = int(lib.dvla_last_gemm_variant())
            got, pre = r if want_preact else (r, None)
            tag = f"gemm[{name}] {M}x{N}x{K} sk{split_k} v{v} run{rep}"
            out.append(metrics(tag, got, ref, TOL_FWD))
            if want_preact:
                out.append(metrics(tag + " preact", pre, pre_ref, TOL_FWD))
            if v != 0:
                out.append({"name": tag + f": forced configuration ran (dvla_last_gemm_variant = {ran})", "rel_l2": 0.0, "tol": 0.0,
                            "ok": ran == v})
            del r, got, pre
    return out


# ---------------------------------------------------------------------------------------------------
# Every (shape, layout, epilogue) problem of the TIMED training step under the configuration the tuner locked for it
# (round-3 VERDICT weak #3: MODEL_GEMMS above is a hand-picked list of 10 of the 121 problem keys).  The keys come from the
# plan file bench.py --save-plan wrote on the GPU (profiles/r0N_gemm_plan.json: the kernel mix the bench line was measured
# with).  Per key, at full size:
#   (1) the whole output against the oracle's formulas (oracle/torch_ref.py act / drop_keep_mask) evaluated in fp32 ON THE
#       DEVICE (an fp32 ATen matmul of the same bf16 operand values; the outputs are up to 1 GB, a host round trip per key
#       would take minutes) -- rel-L2 + the element-wise bound of `metrics`;
#   (2) a block of sampled rows x sampled columns (first / last rows and columns, the rows and columns either side of
#       every kind of tile boundary: 31/32, 127/128, 255/256, seeded random others) against the CPU oracle proper;
#   (3) dvla_last_gemm_variant(): the locked configuration ran (or its documented fallback inside the library: the
#       register-staged kernel for shapes a configuration does not take, the plain schedule when stream-K does not engage).
# ---------------------------------------------------------------------------------------------------
ACT_NAMES = {0: "none", 1: "gelu_erf", 2: "gelu_tanh", 3: "relu", 4: "silu", 5: "quick_gelu", 6: "tanh", 7: "sigmoid"}


def load_gemm_plan():
    """-> (file name, [(key tuple, variant)]) of the newest committed plan"""
    import glob
    import json
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    files = sorted(glob.glob(os.path.join(root, "r[0-9][0-9]_gemm_plan.json")))
    if not files:
        return None, []
    with open(files[-1]) as f:
        plan = json.load(f)
    return os.path.basename(files[-1]), [(tuple(k), int(v)) for k, v in plan]


def _sample_index(n, count, seed):
    pts = {0, 1, n - 1, n - 2}
    for edge in (32, 128, 256):
        for mult in (1, 2, (n // edge) - 1, n // edge):
            for d in (-1, 0):
                pts.add(mult * edge + d)
    g = torch.Generator().manual_seed(seed)
    pts |= set(torch.randint(0, n, (count,), generator=g).tolist())
    pts = sorted(i for i in pts if 0 <= i < n)
    if len(pts) > count:
        keep = set(torch.randperm(len(pts), generator=g)[:count].tolist())
        pts = [v for i, v in enumerate(pts) if i in keep or v in (0, n - 1)]
    return torch.tensor(pts, dtype=torch.int64)


def _dev_metrics(name, got, ref, tol, round_ref=True, k_ulp=None):
    """`metrics` evaluated on the device (no host copy of the output)"""
    g = got.detach().float()
    ref_c = ref.to(BF).float() if round_ref else ref
    num = float((g - ref_c).norm())
    den = max(float(ref_c.norm()), 1e-12)
    d = (g - ref_c).abs()
    max_abs, absmax = float(d.max()), float(ref_c.abs().max())
    finite = bool(torch.isfinite(g).all())
    if round_ref:
        k = elem_ulps(tol) if k_ulp is None else k_ulp
        elem_tol = k * 2.0 ** -8 * absmax + 1e-30
    else:
        k = None
        elem_tol = (2e-4 if tol <= 1e-4 else 20 * tol) * absmax + 1e-6
    r = num / den
    return {"name": name, "rel_l2": r, "max_abs": max_abs, "ref_absmax": absmax, "max_abs_tol": elem_tol, "k_ulp": k,
            "shape": list(g.shape), "finite": finite, "tol": tol, "ok": bool(finite and r <= tol and max_abs <= elem_tol)}


def check_gemm_plan_entry(key, variant):
    from dreamvla_amd import _lib, ops
    (M, N, K, a_trans, b_trans, split_k, act_i, dact_i, has_bias, want_preact, has_aux, has_res, has_drop, out_f32, accumulate,
     ksum_i) = key[:16]
    act, dact = ACT_NAMES[int(act_i)], (ACT_NAMES[int(dact_i)] if has_aux else None)
    p_drop = 0.1 if has_drop else 0.0
    g = torch.Generator(device=DEV).manual_seed(20260926 + (M * 31 + N * 17 + K) % 100003)
    A = torch.randn((M, K), generator=g, device=DEV).to(BF)
    Bm = (torch.randn((N, K), generator=g, device=DEV) / math.sqrt(K) + (0.01 if ksum_i else 0.0)).to(BF)
    bias = torch.randn((N,), generator=g, device=DEV).to(BF) if has_bias else None
    res = torch.randn((M, N), generator=g, device=DEV).to(BF) if has_res else None
    aux = torch.randn((M, N), generator=g, device=DEV).to(BF) if has_aux else None
    c0 = torch.randn((M, N), generator=g, device=DEV) if accumulate else None
    sd = (77, 4242)
    rows, cols = _sample_index(M, 96, 1), _sample_index(N, 128, 2)

    def oracle(a32, b32, bias32, res32, aux32, ridx, cidx, c_init):
        """the epilogue of include/dvla.h in the oracle's formulas; a32 (m, K), b32 (n, K) fp32 on any device"""
        ref = a32 @ b32.t()
        if bias32 is not None:
            ref = ref + bias32
        pre = ref.clone() if want_preact else None
        if want_preact:
            ref = R.bf16_round(ref) if ref.device.type == "cpu" else ref.to(BF).float()
        ref = R.act(ref, act)
        if p_drop > 0:
            keep = R.drop_keep_mask(sd, ridx[:, None], cidx[None, :], p_drop)
            ref = torch.where(keep, ref / (1.0 - p_drop), torch.zeros_like(ref))
        if dact or res32 is not None:
            ref = ref.to(BF).float()
        if dact:
            x = aux32.clone().requires_grad_(True)
            R.act(x, dact).sum().backward()
            ref = ref * x.grad
        if res32 is not None:
            ref = ref + res32
        if c_init is not None:
            ref = ref + c_init
        return ref, pre

    a_dev = A.t().contiguous() if a_trans else A
    b_dev = Bm.t().contiguous() if b_trans else Bm
    kout = None
    if ksum_i:
        kout = torch.full((M if ksum_i == 1 else N,), float("nan"), dtype=torch.float32, device=DEV)
    out_buf = c0.clone() if accumulate else None
    out = []
    tag = (f"plan gemm {M}x{N}x{K} at{int(a_trans)} bt{int(b_trans)} sk{split_k} act{act_i} dact{dact_i} b{int(has_bias)} "
           f"pre{int(want_preact)} res{int(has_res)} drop{int(has_drop)} f32{int(out_f32)} acc{int(accumulate)} ksum{ksum_i} v{variant}")
    lib = _lib.load()
    r = ops.gemm(a_dev, b_dev, a_trans=bool(a_trans), b_trans=bool(b_trans), bias=bias, act=int(act_i), want_preact=bool(want_preact),
                 dact_aux=aux, dact=int(dact_i) if has_aux else 0, dropout_p=p_drop, seed=sd, residual=res,
                 out_dtype=torch.float32 if out_f32 else BF, out=out_buf, accumulate=bool(accumulate), split_k=int(split_k),
                 variant=int(variant) if variant else None, ksum=(("a" if ksum_i == 1 else "b"), kout) if ksum_i else None)
    ran = int(lib.dvla_last_gemm_variant())
    got, pre = r if want_preact else (r, None)
    tol = TOL_F32 if out_f32 else TOL_FWD
    # (1) whole output, oracle formulas in fp32 on the device
    f = lambda t: None if t is None else t.float()
    ref, pre_ref = oracle(A.float(), Bm.float(), f(bias), f(res), f(aux), torch.arange(M, device=DEV), torch.arange(N, device=DEV), c0)
    out.append(_dev_metrics(tag + " [whole output, device fp32]", got, ref, tol, round_ref=not out_f32))
    if want_preact:
        out.append(_dev_metrics(tag + " preact [whole output, device fp32]", pre, pre_ref, TOL_FWD))
    del ref, pre_ref
    # (2) sampled rows x columns against the CPU oracle
    rd, cd = rows.to(DEV), cols.to(DEV)
    blk = lambda t: None if t is None else t[rd][:, cd].float().cpu()
    ref_b, pre_b = oracle(A[rd].float().cpu(), Bm[cd].float().cpu(), None if bias is None else bias[cd].float().cpu(), blk(res),
                          blk(aux), rows, cols, None if c0 is None else c0[rd][:, cd].cpu())
    out.append(metrics(tag + f" [{len(rows)} x {len(cols)} sampled block, CPU oracle]", got[rd][:, cd], ref_b, tol, round_ref=not out_f32))
    if want_preact:
        out.append(metrics(tag + " preact [sampled block, CPU oracle]", pre[rd][:, cd], pre_b, TOL_FWD))
    if ksum_i:
        src = A if ksum_i == 1 else Bm
        kref = src.float().cpu().double().sum(1).float()
        out.append(metrics(tag + " k-sums [CPU oracle]", kout, kref, 1e-5, round_ref=False))
    # (3) what ran
    lv = int(variant) % 100      # (108 / 109: the tuner's "phase kernel without the k-sum dots + column-sum pass": the library runs 8 / 9)
    allowed = {lv, 2} | ({8} if lv in (9, 10) else set())
    out.append({"name": tag + f": locked configuration ran (dvla_last_gemm_variant = {ran})", "rel_l2": 0.0, "tol": 0.0,
                "ok": variant == 0 or ran in allowed, "ran": ran})
    return out


def check_layernorm(rows, cols, affine=True, eps=1e-5, param_f32=False, seed=0):
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(99 + seed)
    x = rnd((rows, cols), g, 2.0) + 0.5
    x = R.bf16_round(x)
    w = rnd((cols,), g) + 1.0 if affine else None
    b = rnd((cols,), g) if affine else None
    if affine:
        w, b = R.bf16_round(w), R.bf16_round(b)
    dy = rnd((rows, cols), g)
    pdt = torch.float32 if param_f32 else BF
    xd = x.to(DEV, BF).requires_grad_(True)
    wd = w.to(DEV, pdt).requires_grad_(True) if affine else None
    bd = b.to(DEV, pdt).requires_grad_(True) if affine else None
    y = ops.layer_norm(xd, wd, bd, eps)
    y.backward(dy.to(DEV, BF))
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True) if affine else None
    br = b.clone().requires_grad_(True) if affine else None
    yr = R.layer_norm(xr, wr, br, eps)
    yr.backward(dy)
    tag = f"layernorm {rows}x{cols} affine{int(affine)} eps{eps} pf32{int(param_f32)}"
    out = [metrics(tag + " y", y, yr, TOL_FWD), metrics(tag + " dx", xd.grad, xr.grad, TOL_GRAD)]
    if affine:
        out.append(metrics(tag + " dgamma", wd.grad, wr.grad, TOL_GRAD, round_ref=not param_f32))
        out.append(metrics(tag + " dbeta", bd.grad, br.grad, TOL_GRAD, round_ref=not param_f32))
        # an input that needs no gradient (round 6: dx == NULL in dvla_layernorm_bwd_add -- the resampler's norm_media over the frozen
        # ViT's tokens): the parameter gradients must be the SAME numbers, and no input gradient may appear
        x0 = x.to(DEV, BF)
        w0 = wd.detach().clone().requires_grad_(True)
        b0 = bd.detach().clone().requires_grad_(True)
        ops.layer_norm(x0, w0, b0, eps).backward(dy.to(DEV, BF))
        out.append(metrics(tag + " dgamma (input without gradient)", w0.grad, wd.grad.detach().float().cpu(), 0.0, round_ref=not param_f32))
        out.append(metrics(tag + " dbeta (input without gradient)", b0.grad, bd.grad.detach().float().cpu(), 0.0, round_ref=not param_f32))
        out.append({"name": tag + " no input gradient", "ok": x0.grad is None, "rel_l2": 0.0, "max_abs": 0.0, "tol": 0.0})
    return out


def check_layernorm_fork(rows, cols, affine=True, eps=1e-5, seed=0):
    """ops.layer_norm_fork: (x, LN(x)) whose backward is dvla_layernorm_bwd_add (dres + LN'(dy) in one kernel), against
    the oracle's two-path autograd: loss = <x, dres> + <LN(x), dy>."""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(199 + seed)
    x = R.bf16_round(rnd((rows, cols), g, 2.0) + 0.5)
    w = R.bf16_round(rnd((cols,), g) + 1.0) if affine else None
    b = R.bf16_round(rnd((cols,), g)) if affine else None
    dy, dres = rnd((rows, cols), g), rnd((rows, cols), g)
    xd = x.to(DEV, BF).requires_grad_(True)
    wd = w.to(DEV, BF).requires_grad_(True) if affine else None
    bd = b.to(DEV, BF).requires_grad_(True) if affine else None
    r, y = ops.layer_norm_fork(xd, wd, bd, eps)
    torch.autograd.backward([r, y], [dres.to(DEV, BF), dy.to(DEV, BF)])
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True) if affine else None
    br = b.clone().requires_grad_(True) if affine else None
    yr = R.layer_norm(xr, wr, br, eps)
    torch.autograd.backward([xr * 1.0, yr], [dres, dy])
    tag = f"layernorm_fork {rows}x{cols} affine{int(affine)}"
    out = [metrics(tag + " residual is x", r, x, 0.0), metrics(tag + " y", y, yr, TOL_FWD),
           metrics(tag + " dx", xd.grad, xr.grad, TOL_GRAD)]
    if affine:
        out.append(metrics(tag + " dgamma", wd.grad, wr.grad, TOL_GRAD))
        out.append(metrics(tag + " dbeta", bd.grad, br.grad, TOL_GRAD))
    return out


def check_layernorm_last_tokens(n, L, keep, cols, param_f32=False, eps=1e-5, seed=0):
    """ops.layer_norm_last_tokens (dvla_layernorm_fwd_rows / _bwd_rows, round 6): LayerNorm(x[:, -keep:, :]) of x (n, L, cols) without the
    strided copy, against the oracle's LayerNorm on the materialised slice; the input gradient is the gradient of the WHOLE buffer
    (zeros in the leading L - keep tokens of every sequence: the buffer is pre-filled with NaN-free garbage by the allocator, the
    kernel must write them)."""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(299 + seed)
    x = R.bf16_round(rnd((n, L, cols), g, 2.0) + 0.5)
    w = R.bf16_round(rnd((cols,), g) + 1.0)
    b = R.bf16_round(rnd((cols,), g))
    dy = rnd((n * keep, cols), g)
    pdt = torch.float32 if param_f32 else BF
    torch.full((n, L, cols), 7.0, device=DEV, dtype=BF)          # (dirty the allocator's pool: an unwritten gradient row would show)
    xd = x.to(DEV, BF).requires_grad_(True)
    wd = w.to(DEV, pdt).requires_grad_(True)
    bd = b.to(DEV, pdt).requires_grad_(True)
    y = ops.layer_norm_last_tokens(xd, wd, bd, eps, keep)
    y.backward(dy.to(DEV, BF))
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = R.layer_norm(xr[:, L - keep:, :].reshape(-1, cols), wr, br, eps)
    yr.backward(dy)
    tag = f"layernorm_last_tokens {n}x{L}(keep {keep})x{cols} pf32{int(param_f32)}"
    lead = xd.grad[:, :L - keep, :]
    out = [metrics(tag + " y", y, yr, TOL_FWD), metrics(tag + " dx (whole buffer)", xd.grad, xr.grad, TOL_GRAD),
           {"name": tag + " leading tokens get exact zeros", "ok": bool((lead == 0).all()) if lead.numel() else True, "rel_l2": 0.0,
            "max_abs": float(lead.float().abs().max()) if lead.numel() else 0.0, "tol": 0.0},
           metrics(tag + " dgamma", wd.grad, wr.grad, TOL_GRAD, round_ref=not param_f32),
           metrics(tag + " dbeta", bd.grad, br.grad, TOL_GRAD, round_ref=not param_f32)]
    # the same numbers as the two-step path (copy the slice, plain LayerNorm): bit for bit
    xd2 = x.to(DEV, BF).requires_grad_(True)
    w2, b2 = wd.detach().clone().requires_grad_(True), bd.detach().clone().requires_grad_(True)
    y2 = ops.layer_norm(xd2[:, L - keep:, :].reshape(-1, cols), w2, b2, eps)
    y2.backward(dy.to(DEV, BF))
    out.append(metrics(tag + " y == LayerNorm(copy of the slice)", y, y2.detach().float().cpu(), 0.0))
    out.append(metrics(tag + " dx == the two-step path", xd.grad, xd2.grad.detach().float().cpu(), 0.0))
    return out


def check_layernorm_concat(n, La, Lb, cols, a_needs_grad=True, seed=0):
    """ops.layer_norm_concat (dvla_layernorm_*_rows with map_output, round 6): cat((LN_a(a), LN_b(b)), dim=1) written by two launches into
    one buffer, against the oracle's two LayerNorms + cat; and bit for bit against ops.layer_norm + torch.cat on the device.
    a_needs_grad=False: the resampler's media tokens (no input gradient for a, parameter gradients still)."""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(399 + seed)
    a = R.bf16_round(rnd((n, La, cols), g, 2.0) + 0.5)
    b = R.bf16_round(rnd((n, Lb, cols), g, 1.5) - 0.25)
    wa, ba = R.bf16_round(rnd((cols,), g) + 1.0), R.bf16_round(rnd((cols,), g))
    wb, bb = R.bf16_round(rnd((cols,), g) + 1.0), R.bf16_round(rnd((cols,), g))
    dy = rnd((n, La + Lb, cols), g)
    def dev(t, grad=True):
        return t.to(DEV, BF).requires_grad_(grad)
    ad, bd = dev(a, a_needs_grad), dev(b)
    wad, bad, wbd, bbd = dev(wa), dev(ba), dev(wb), dev(bb)
    y = ops.layer_norm_concat(ad, wad, bad, 1e-5, bd, wbd, bbd, 1e-5)
    y.backward(dy.to(DEV, BF))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    war, bar, wbr, bbr = (t.clone().requires_grad_(True) for t in (wa, ba, wb, bb))
    yr = torch.cat((R.layer_norm(ar, war, bar, 1e-5), R.layer_norm(br, wbr, bbr, 1e-5)), dim=1)
    yr.backward(dy)
    tag = f"layernorm_concat {n}x({La}+{Lb})x{cols} a_grad{int(a_needs_grad)}"
    out = [metrics(tag + " y", y, yr, TOL_FWD), metrics(tag + " db_in", bd.grad, br.grad, TOL_GRAD),
           metrics(tag + " dgamma_a", wad.grad, war.grad, TOL_GRAD), metrics(tag + " dbeta_a", bad.grad, bar.grad, TOL_GRAD),
           metrics(tag + " dgamma_b", wbd.grad, wbr.grad, TOL_GRAD), metrics(tag + " dbeta_b", bbd.grad, bbr.grad, TOL_GRAD)]
    if a_needs_grad:
        out.append(metrics(tag + " da_in", ad.grad, ar.grad, TOL_GRAD))
    else:
        out.append({"name": tag + " no gradient for a", "ok": ad.grad is None, "rel_l2": 0.0, "max_abs": 0.0, "tol": 0.0})
    # the ATen form on the device: same numbers
    a2, b2 = dev(a, a_needs_grad), dev(b)
    wa2, ba2, wb2, bb2 = dev(wa), dev(ba), dev(wb), dev(bb)
    y2 = torch.cat((ops.layer_norm(a2, wa2, ba2, 1e-5), ops.layer_norm(b2, wb2, bb2, 1e-5)), dim=1)
    y2.backward(dy.to(DEV, BF))
    cpu = lambda t: t.detach().float().cpu()
    out.append(metrics(tag + " y == cat of two LayerNorms", y, cpu(y2), 0.0))
    out.append(metrics(tag + " db_in == ATen form", bd.grad, cpu(b2.grad), 0.0))
    out.append(metrics(tag + " dgamma_a == ATen form", wad.grad, cpu(wa2.grad), 0.0))
    out.append(metrics(tag + " dgamma_b == ATen form", wbd.grad, cpu(wb2.grad), 0.0))
    return out


def make_block_mask(L, blk, nA):
    """small analogue of generate_attention_mask (dreamvla_model.py:25-66): block-causal over `blk`-token steps,
    the last blk-nA tokens of every step are never keys."""
    m = torch.zeros(L, L)
    nsteps = (L + blk - 1) // blk
    for i in range(nsteps):
        s, e = i * blk, min((i + 1) * blk, L)
        m[s:e, e:] = -float("inf")
        m[:, s + nA:e] = -float("inf")
    return m


def _sample_rows(B, rows):
    if rows is None or rows >= B:
        return list(range(B))
    idx = sorted(set([0, 1, B // 2, B - 2, B - 1] + [int(x) for x in torch.randint(0, B, (max(rows - 5, 0),), generator=torch.Generator().manual_seed(B))]))
    return [i for i in idx if 0 <= i < B]


def check_self_attention(B, H, L, mask_kind="none", dropout_p=0.0, grad=True, seed=0, scale=None, rows=None, period=None):
    """HIP self-attention (forward + backward) against oracle/torch_ref.py::attention_bf16 (1e-3 / 2e-3) and, as the link
    to the reference-pinned fp32 restatement, against ::attention (3e-3 / 4e-3).
    rows   : the oracle is evaluated on that many batch rows only (first / last / middle + seeded random ones; the CPU
             restatement materialises B*H*L*L scores) -- for the benchmark-scale cases (B = 32 / 448);
    period : batch row b carries the inputs of row b % period; without dropout the kernels are deterministic, so EVERY row of the
             device result must equal its representative bit for bit -- full coverage of the batch at no oracle cost."""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(7 + seed)
    P = B if period is None else min(B, period)
    qkv = rnd((P, L, 3 * H * 64), g)
    do = rnd((P, L, H * 64), g)
    if P < B:
        rep = -(-B // P)
        qkv = qkv.repeat(rep, 1, 1)[:B].contiguous()
        do = do.repeat(rep, 1, 1)[:B].contiguous()
    mask = None
    if mask_kind == "block":
        mask = make_block_mask(L, 19, 12)
    elif mask_kind == "causal":
        mask = torch.full((L, L), -float("inf")).triu(1)
    elif mask_kind.startswith("dreamvla"):
        # the REAL trunk mask of the benchmarked head set (obs + depth + sam dream heads: 54 query tokens + 3 action tokens per
        # window step, 36 conditioning tokens): L = 93 S; S = 7 is the training window (L = 651, key compaction 651 -> 378),
        # S = 10 the evaluation window (L = 930).  The generator is pinned bit for bit against the reference (tests/test_mask.py).
        # "dreamvla_D" / "dreamvla_E" (round 5): the same generator for the other shipped head sets -- D = LIBERO finetune_long.sh
        # (obs + sam: 36 + 39 tokens per step, L = 525 at S = 7), E = all dream heads of BASELINE configs[3] (obs + dino + sam +
        # traj: 36 + 75, L = 777).  L = 1302 = 93 x 14 is the survey's maximum (head set C at the pretrain window).
        from dreamvla_amd.dreamvla_model import generate_attention_mask
        num_b = {"dreamvla": 57, "dreamvla_D": 39, "dreamvla_E": 75}[mask_kind]
        S = L // (36 + num_b)
        assert L == (36 + num_b) * S
        mask = generate_attention_mask(S, 36, num_b, 0, False, False, False, 0.0, num_b - 3, 3)
    mt = None
    if mask_kind == "pretrain":
        # the shipped PRETRAIN mask (pretrain.sh:37-52: S = 14, obs head + 3 action tokens -> 36 + 21 tokens per step, L = 798,
        # --atten_goal 4 --atten_goal_state --atten_only_obs --attn_robot_proprio_state): the kernels' tables come from the RULE
        # evaluated on the device (csrc/masks.hip, what the pretrain phase runs every step), the oracle gets the mask tensor
        # of the reference-pinned generator
        from dreamvla_amd.dreamvla_model import generate_attention_mask
        S = L // 57
        assert L == 57 * S
        rule = dict(K=S, num_A=36, num_B=21, atten_goal=4, atten_goal_state=True, atten_only_obs=True,
                    attn_robot_proprio_state=True, num_obs_token=18, action_pred_steps=3)
        mask = generate_attention_mask(mask_l_obs_ratio=0.0, **rule)
        mt = ops.build_mask_tables_device(DEV, drop=None, **rule)
    qd = qkv.to(DEV, BF).requires_grad_(grad)
    if mt is None and mask is not None:
        mt = ops.build_mask_tables(mask, device=DEV)
    from dreamvla_amd.ops import _Seeds
    _Seeds.counter = 1000 + seed
    o = ops.self_attention(qd, H, mask_tables=mt, dropout_p=dropout_p, scale=scale)
    sd = (_Seeds.counter, _Seeds.next()[1])
    _Seeds.counter -= 1
    if grad:
        o.backward(do.to(DEV, BF))
    sel = _sample_rows(B, rows)
    idx = torch.tensor(sel)
    drop_cols = None
    if mt is not None and mt.key_index is not None:
        drop_cols = torch.zeros(L, dtype=torch.int64)
        drop_cols[mt.key_index.cpu().long()] = torch.arange(mt.Lk)
    drop = (dropout_p, sd) if dropout_p > 0 else None
    W = H * 64
    tag = f"self_attn B{B} H{H} L{L} mask={mask_kind} p{dropout_p}" + ("" if len(sel) == B else f" ({len(sel)} rows)")
    o_h = o.detach().float().cpu()[idx]
    g_h = qd.grad.detach().float().cpu()[idx] if grad else None
    qs, dos = qkv[idx], do[idx]
    # (1) the bf16-faithful restatement: same rounding points as the kernels
    q, k, v = R.split_qkv(qs, H)
    do4 = dos.view(len(sel), L, H, 64).permute(0, 2, 1, 3)
    res = R.attention_bf16(q, k, v, scale=scale, mask=mask, drop=drop, drop_cols=drop_cols, dout=do4 if grad else None,
                           batch_index=sel)
    out = [metrics(tag + " o", o_h, R.merge_heads(res[0]), TOL_ATTN)]
    if grad:
        dq, dk, dv = (R.merge_heads(t) for t in res[2:])
        out.append(metrics(tag + " dq", g_h[..., :W], dq, TOL_ATTN_GRAD))
        out.append(metrics(tag + " dk", g_h[..., W:2 * W], dk, TOL_ATTN_GRAD))
        out.append(metrics(tag + " dv", g_h[..., 2 * W:], dv, TOL_ATTN_GRAD))
    # (2) the unrounded fp32 restatement of the reference's softmax attention (what the golden fixtures pin)
    qr = qs.clone().requires_grad_(grad)
    q, k, v = R.split_qkv(qr, H)
    orf = R.merge_heads(R.attention(q, k, v, scale=scale, mask=mask, drop=drop, drop_cols=drop_cols, batch_index=sel))
    out.append(metrics(tag + " o (fp32 oracle)", o_h, orf, TOL_ATTN_F32))
    if grad:
        orf.backward(dos)
        out.append(metrics(tag + " dqkv (fp32 oracle)", g_h, qr.grad, TOL_GRAD))
    # (3) every batch row equals its representative (deterministic kernels, no dropout)
    if P < B and dropout_p == 0.0:
        of = o.detach().view(-1, L * W)
        same = bool(torch.equal(of[P:], of[:B - P]))
        if grad:
            gf = qd.grad.detach().view(-1, 3 * L * W)
            same = same and bool(torch.equal(gf[P:], gf[:B - P]))
        out.append({"name": tag + f" all {B} rows == their representative (period {P})", "rel_l2": 0.0, "tol": 0.0, "ok": same})
    return out


def check_self_attention_small(B, H, L, D, seed=0):
    """the short-sequence, generic-head_dim kernel (csrc/attention_small.hip: DiT-S, head_dim 96) against the same two oracles"""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(27 + seed)
    qkv = rnd((B, L, 3 * H * D), g)
    do = rnd((B, L, H * D), g)
    qd = qkv.to(DEV, BF).requires_grad_(True)
    o = ops.self_attention(qd, H, head_dim=D)
    o.backward(do.to(DEV, BF))
    t = qkv.view(B, L, 3, H, D).permute(2, 0, 3, 1, 4)
    do4 = do.view(B, L, H, D).permute(0, 2, 1, 3)
    of, _, dq, dk, dv = R.attention_bf16(t[0], t[1], t[2], dout=do4)
    W = H * D
    tag = f"self_attn_small B{B} H{H} L{L} D{D}"
    out = [metrics(tag + " o", o, R.merge_heads(of), TOL_ATTN),
           metrics(tag + " dq", qd.grad[..., :W], R.merge_heads(dq), TOL_ATTN_GRAD),
           metrics(tag + " dk", qd.grad[..., W:2 * W], R.merge_heads(dk), TOL_ATTN_GRAD),
           metrics(tag + " dv", qd.grad[..., 2 * W:], R.merge_heads(dv), TOL_ATTN_GRAD)]
    qr = qkv.clone().requires_grad_(True)
    t = qr.view(B, L, 3, H, D).permute(2, 0, 3, 1, 4)
    orf = R.merge_heads(R.attention(t[0], t[1], t[2]))
    orf.backward(do)
    out += [metrics(tag + " o (fp32 oracle)", o, orf, TOL_ATTN_F32), metrics(tag + " dqkv (fp32 oracle)", qd.grad, qr.grad, TOL_GRAD)]
    return out


def check_cross_attention(B, H, Lq, Lk, seed=0):
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(17 + seed)
    q = rnd((B, Lq, H * 64), g)
    kv = rnd((B, Lk, 2 * H * 64), g)
    do = rnd((B, Lq, H * 64), g)
    qd = q.to(DEV, BF).requires_grad_(True)
    kvd = kv.to(DEV, BF).requires_grad_(True)
    o = ops.cross_attention(qd, kvd, H)
    o.backward(do.to(DEV, BF))
    tag = f"cross_attn B{B} H{H} Lq{Lq} Lk{Lk}"
    q4 = q.view(B, Lq, H, 64).permute(0, 2, 1, 3)
    kv5 = kv.view(B, Lk, 2, H, 64).permute(2, 0, 3, 1, 4)
    of, _, dq, dk, dv = R.attention_bf16(q4, kv5[0], kv5[1], dout=do.view(B, Lq, H, 64).permute(0, 2, 1, 3))
    dkv = torch.stack((dk, dv), 0).permute(1, 3, 0, 2, 4).reshape(B, Lk, 2 * H * 64)     # (2,B,H,Lk,64) -> (B,Lk,2,H,64)
    out = [metrics(tag + " o", o, R.merge_heads(of), TOL_ATTN), metrics(tag + " dq", qd.grad, R.merge_heads(dq), TOL_ATTN_GRAD),
           metrics(tag + " dkv", kvd.grad, dkv, TOL_ATTN_GRAD)]
    qr = q.clone().requires_grad_(True)
    kvr = kv.clone().requires_grad_(True)
    q4 = qr.view(B, Lq, H, 64).permute(0, 2, 1, 3)
    kv5 = kvr.view(B, Lk, 2, H, 64).permute(2, 0, 3, 1, 4)
    orf = R.merge_heads(R.attention(q4, kv5[0], kv5[1]))
    orf.backward(do)
    out += [metrics(tag + " o (fp32 oracle)", o, orf, TOL_ATTN_F32), metrics(tag + " dq (fp32 oracle)", qd.grad, qr.grad, TOL_GRAD),
            metrics(tag + " dkv (fp32 oracle)", kvd.grad, kvr.grad, TOL_GRAD)]
    return out


def _exact(name, ok, **extra):
    return dict({"name": name, "rel_l2": 0.0, "tol": 0.0, "ok": bool(ok)}, **extra)


def check_attention_masked(case):
    """HIP attention under an arbitrary 0 / -inf mask (a case of tests/attention_mask_cases.py) through ops.attn_fwd_raw /
    ops.attn_bwd_raw: any (Lq, Lk), lse and pre-filled gradient buffers within reach.  q, k, v are strided views of one packed
    buffer when Lq == Lk (what _SelfAttention passes), of a q and a kv buffer otherwise (_CrossAttention); dq, dk, dv are views of
    buffers pre-filled with NaN.  Checked per case:
      values    o, dq, dk, dv against oracle/torch_ref.py::attention_bf16, TOL_ATTN / TOL_ATTN_GRAD, both criteria of `metrics`
      lse       finite rows against the oracle's (TOL_F32); rows of a query that sees no key are +inf exactly
      blind     such a query's o and dq rows are == 0 (its dout is random data: a leak into dk / dv fails the value check)
      writes    no NaN left in dq; with a key_index the dk / dv rows it names are NaN-free and every other row still holds the
                pre-fill (the "NOT written" rule of include/dvla.h); without one every row is written, dead keys' rows == 0
      period    batch row b carries the inputs of row b % period: every row of o, lse, dq, dk, dv equals its representative bit
                for bit (several items per workgroup of the forward ring kernel); the oracle then sees `rows` sampled rows
    -> (list of metric dicts, structure of the mask)"""
    from dreamvla_amd import ops
    from tests import attention_mask_cases as MC
    B, H, Lq, Lk, D, p_drop = case["B"], case["H"], case["Lq"], case["Lk"], case["D"], case["dropout_p"]
    vis, mask, mt = MC.tables(case, device=DEV)
    struct = MC.structure(vis, mt)
    scale = D ** -0.5
    g = torch.Generator().manual_seed(4100 + 13 * D + case["seed"])
    P = B if case["period"] is None else min(B, case["period"])
    W = H * D
    if Lq == Lk:
        src = [rnd((P, Lq, 3 * W), g)]
    else:
        src = [rnd((P, Lq, W), g), rnd((P, Lk, 2 * W), g)]
    do = rnd((P, Lq, W), g)
    if P < B:
        tile = lambda t: t.repeat(-(-B // P), 1, 1)[:B].contiguous()
        src, do = [tile(t) for t in src], tile(do)
    dev = [t.to(DEV, BF) for t in src]
    grad = [torch.full_like(t, float("nan")) for t in dev]
    if Lq == Lk:
        v5, d5 = dev[0].view(B, Lq, 3, H, D), grad[0].view(B, Lq, 3, H, D)
        (q, k, v), (dq, dk, dv) = v5.unbind(2), d5.unbind(2)
        q_h, k_h, v_h = src[0].view(B, Lq, 3, H, D).unbind(2)
    else:
        kv5, dkv5 = dev[1].view(B, Lk, 2, H, D), grad[1].view(B, Lk, 2, H, D)
        q, (k, v), dq, (dk, dv) = dev[0].view(B, Lq, H, D), kv5.unbind(2), grad[0].view(B, Lq, H, D), dkv5.unbind(2)
        q_h, (k_h, v_h) = src[0].view(B, Lq, H, D), src[1].view(B, Lk, 2, H, D).unbind(2)
    sd = (4711 + case["seed"], 1234567)
    kw = dict(scale=scale, mask_tables=mt, dropout_p=p_drop, seed=sd, head_dim=D)
    do_d = do.to(DEV, BF).view(B, Lq, H, D)
    o, lse = ops.attn_fwd_raw(q, k, v, **kw)
    ops.attn_bwd_raw(q, k, v, o, lse, do_d, dq, dk, dv, **kw)
    torch.cuda.synchronize()

    # oracle on the sampled batch rows, (B, H, L, D) layout
    sel = _sample_rows(B, case["rows"])
    idx = torch.tensor(sel)
    heads = lambda t: t[idx].permute(0, 2, 1, 3)
    key_index = None if mt is None or mt.key_index is None else mt.key_index.cpu().long()
    drop_cols = None
    if key_index is not None:
        drop_cols = torch.zeros(Lk, dtype=torch.int64)
        drop_cols[key_index] = torch.arange(mt.Lk)
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = R.attention_bf16(
        heads(q_h), heads(k_h), heads(v_h), scale=scale, mask=mask, drop=(p_drop, sd) if p_drop > 0 else None,
        drop_cols=drop_cols, dout=heads(do.view(B, Lq, H, D)), batch_index=sel)
    host = lambda t: t.detach().float().cpu()[idx].permute(0, 2, 1, 3)
    got = {"o": host(o), "dq": host(dq), "dk": host(dk), "dv": host(dv)}
    lse_h = lse.detach().cpu()[idx]
    tag = "attn_masked " + case["id"]
    named = torch.ones(Lk, dtype=torch.bool)
    if key_index is not None:
        named[:] = False
        named[key_index] = True
    blind = torch.zeros(Lq, dtype=torch.bool) if vis is None else torch.from_numpy(~vis.any(axis=1))
    dead = torch.zeros(Lk, dtype=torch.bool) if vis is None else torch.from_numpy(~vis.any(axis=0))

    # values (rows of dk / dv that the kernels do not write are compared where they ARE written: the named rows)
    out = [metrics(tag + " o", got["o"], ref_o, TOL_ATTN), metrics(tag + " dq", got["dq"], ref_dq, TOL_ATTN_GRAD),
           metrics(tag + " dk", got["dk"][:, :, named], ref_dk[:, :, named], TOL_ATTN_GRAD),
           metrics(tag + " dv", got["dv"][:, :, named], ref_dv[:, :, named], TOL_ATTN_GRAD)]
    # lse
    fin = ~blind
    if bool(fin.any()):
        out.append(metrics(tag + " lse", lse_h[:, :, fin], ref_lse[:, :, fin], TOL_F32, round_ref=False))
    pinf = lse_h[:, :, blind] == float("inf")
    out.append(_exact(tag + f": lse of the {int(blind.sum())} blind queries is +inf", pinf.all()))
    # blind queries
    zero = lambda t: bool((t == 0).all())
    out.append(_exact(tag + ": o and dq of blind queries are 0", zero(got["o"][:, :, blind]) and zero(got["dq"][:, :, blind])))
    # coverage of writes, over the WHOLE batch
    nan_rows = lambda t: torch.isnan(t.detach().float()).any(dim=-1).any(dim=2).any(dim=0).cpu()      # (B, L, H, D) -> per token row
    all_nan = lambda t: torch.isnan(t.detach().float()).all(dim=-1).all(dim=2).all(dim=0).cpu()
    out.append(_exact(tag + ": every dq row written", not bool(nan_rows(dq).any())))
    for name, t in (("dk", dk), ("dv", dv)):
        out.append(_exact(tag + f": every {name} row the tables name is written", not bool(nan_rows(t)[named].any())))
        if key_index is not None:
            out.append(_exact(tag + f": the {int((~named).sum())} {name} rows the tables do not name keep their pre-fill",
                              all_nan(t)[~named].all()))
        else:
            out.append(_exact(tag + f": {name} of the {int(dead.sum())} dead keys is 0", zero(got[name][:, :, dead])))
    finite = all(bool(torch.isfinite(t.detach().float()).all()) for t in (o, dq)) and \
        all(bool(torch.isfinite(got[n][:, :, named]).all()) for n in ("dk", "dv"))
    out.append(_exact(tag + ": everything written is finite", finite))
    # every batch row equals its representative
    if P < B and p_drop == 0.0:
        same = all(torch.equal(_bits(t)[P:], _bits(t)[:B - P]) for t in (o, dq, dk, dv)) and torch.equal(lse[P:], lse[:B - P])
        out.append(_exact(tag + f": all {B} batch rows == their representative (period {P})", same))
    return out, struct


def check_attention_values(case):
    """HIP attention on one value regime (a case of tests/attention_value_ref.py: one-hot rows, sinks, staircases of the running
    maximum, mixed temperatures in one wave, outlier channels, tiny / big magnitudes, huge logits behind the mask, ties, exact
    integers) against the float64 reference of that module.  Forward: o and lse.  Backward: the kernels' dq, dk, dv, run on their
    own o and lse exactly as the product does, against the float64 backward CONDITIONED on the o the kernel stored.  Per tensor
    tol = max(suite tolerance, 4 E), k_ulp = max(suite k, 4 U) with E, U the yardstick of the case (what correct float32 restatements
    differ from the reference by; capped on the CPU at 1e-2 / 16 ulps).  Exact, no tolerance: everything written is finite, a query
    that sees no key has o = 0, lse = +inf, dq = 0, and the `exact` family's o and dv equal the float64 result bit for bit.
    via "raw": ops.attn_fwd_raw / attn_bwd_raw on strided views of packed buffers, gradients into NaN-pre-filled views;
    via "self" / "cross": the autograd wrappers (o is the returned tensor; they do not return lse).
    -> (list of metric dicts, yardstick)"""
    from dreamvla_amd import ops
    from tests import attention_value_ref as V
    B, H, Lq, Lk, D, p_drop = case["B"], case["H"], case["Lq"], case["Lk"], case["D"], case["p"]
    data, yard = V.yardstick(case)
    vis = data["vis"]
    mt = V.tables(case, vis, device=DEV)
    scale = D ** -0.5
    tok = lambda t: t.permute(0, 2, 1, 3)                                   # (B, H, L, D) <-> (B, L, H, D)
    host = lambda t: tok(t.detach().float().cpu())
    W = H * D
    tag = "attn_values " + case["id"]
    got = {}
    if case["via"] == "self":
        assert Lq == Lk and p_drop == 0
        qkv = torch.stack((tok(data["q"]), tok(data["k"]), tok(data["v"])), dim=2).reshape(B, Lq, 3 * W).to(DEV, BF).requires_grad_(True)
        o = ops.self_attention(qkv, H, mask_tables=mt, head_dim=D)
        o.backward(tok(data["dout"]).reshape(B, Lq, W).to(DEV, BF))
        g5 = qkv.grad.view(B, Lq, 3, H, D)
        got = {"o": host(o.view(B, Lq, H, D)), "dq": host(g5[:, :, 0]), "dk": host(g5[:, :, 1]), "dv": host(g5[:, :, 2])}
    elif case["via"] == "cross":
        assert mt is None and p_drop == 0 and D == 64
        qd = tok(data["q"]).reshape(B, Lq, W).to(DEV, BF).requires_grad_(True)
        kvd = torch.stack((tok(data["k"]), tok(data["v"])), dim=2).reshape(B, Lk, 2 * W).to(DEV, BF).requires_grad_(True)
        o = ops.cross_attention(qd, kvd, H)
        o.backward(tok(data["dout"]).reshape(B, Lq, W).to(DEV, BF))
        g5 = kvd.grad.view(B, Lk, 2, H, D)
        got = {"o": host(o.view(B, Lq, H, D)), "dq": host(qd.grad.view(B, Lq, H, D)), "dk": host(g5[:, :, 0]), "dv": host(g5[:, :, 1])}
    else:
        if Lq == Lk:
            buf = torch.stack((tok(data["q"]), tok(data["k"]), tok(data["v"])), dim=2).contiguous().to(DEV, BF)      # (B, L, 3, H, D)
            gbuf = torch.full_like(buf, float("nan"))
            (q, k, v), (dq, dk, dv) = buf.unbind(2), gbuf.unbind(2)
        else:
            q = tok(data["q"]).contiguous().to(DEV, BF)
            kv = torch.stack((tok(data["k"]), tok(data["v"])), dim=2).contiguous().to(DEV, BF)
            dq, gkv = torch.full_like(q, float("nan")), torch.full_like(kv, float("nan"))
            (k, v), (dk, dv) = kv.unbind(2), gkv.unbind(2)
        kw = dict(scale=scale, mask_tables=mt, dropout_p=p_drop, seed=V.drop_of(case)[1] if p_drop > 0 else (0, 0), head_dim=D)
        o, lse = ops.attn_fwd_raw(q, k, v, **kw)
        ops.attn_bwd_raw(q, k, v, o, lse, tok(data["dout"]).contiguous().to(DEV, BF), dq, dk, dv, **kw)
        torch.cuda.synchronize()
        got = {"o": host(o), "lse": lse.detach().float().cpu(), "dq": host(dq), "dk": host(dk), "dv": host(dv)}
    named = None
    if mt is not None and mt.key_index is not None:
        named = torch.zeros(Lk, dtype=torch.bool)
        named[mt.key_index.cpu().long()] = True
    out = V.judge(case, data, yard, got, tag=tag, named=named)
    # exact: finiteness of everything written, the convention for a query that sees no key
    rows_k = slice(None) if named is None else named
    finite = all(bool(torch.isfinite(got[n]).all()) for n in ("o", "dq")) and all(bool(torch.isfinite(got[n][:, :, rows_k]).all()) for n in ("dk", "dv"))
    blind = torch.zeros(Lq, dtype=torch.bool) if vis is None else torch.from_numpy(~vis.any(axis=1))
    if "lse" in got:
        finite = finite and bool(torch.isfinite(got["lse"][..., ~blind]).all())
        out.append(_exact(tag + f": lse of the {int(blind.sum())} blind queries is +inf", (got["lse"][..., blind] == float("inf")).all()))
    out.append(_exact(tag + ": everything written is finite", finite))
    zero = lambda t: bool((t == 0).all())
    out.append(_exact(tag + ": o and dq of blind queries are 0", zero(got["o"][:, :, blind]) and zero(got["dq"][:, :, blind])))
    return out, yard


def check_attention_probe_values(regime, mask, compact, L=133, D=64, B=2, H=2, R_rows=32):
    """ops.attention_probe on a value regime of tests/attention_value_ref.py against the float64 softmax of
    tests/attention_probe_ref.py, by the derived bound tests/test_attention_probe_gpu.py uses.  On top of it one absolute term: a
    probability below 2^-126 has no normal fp32 representation (the kernel may flush it to 0), so 2^-126 is added to the bound.
    Exact: a key the row cannot see, a blind row hold 0.0; every element is written (NaN pre-fill) and finite."""
    import numpy as np
    from dreamvla_amd import ops
    from tests import attention_probe_ref as PR
    from tests import attention_value_ref as V
    case = V._case("probe", regime, L, D=D, B=B, H=H, mask=mask, compact=compact)
    data = V.values(case)
    vis = data["vis"]
    mt = V.tables(case, vis, device=DEV)
    tok = lambda t: t.permute(0, 2, 1, 3).contiguous()
    q, k = tok(data["q"]).to(DEV, BF), tok(data["k"]).to(DEV, BF)
    rng = np.random.default_rng(5)
    rows = np.stack([rng.permutation(L)[:R_rows] for _ in range(B)]).astype(np.int32)
    rows[0, 0], rows[B - 1, 1] = 0, L - 1
    if vis is not None:
        rows[0, 2] = int(np.nonzero(~vis.any(axis=1))[0][0])              # a blind row
    scale = D ** -0.5
    tag = f"probe values {regime} mask={mask}" + ("" if compact else " uncompacted")
    res = []
    for per_head in (True, False):
        shape = (B, H, R_rows, L) if per_head else (B, R_rows, L)
        out = torch.full(shape, float("nan"), device=DEV)
        ops.attention_probe(q, k, torch.from_numpy(rows).to(DEV), scale=scale, mask_tables=mt, per_head=per_head, out=out)
        torch.cuda.synchronize()
        g = out.double().cpu().numpy()
        ref = PR.probabilities(tok(data["q"]).numpy(), tok(data["k"]).numpy(), rows, scale, vis)
        want = ref["per_head" if per_head else "mean"]
        bnd = PR.bound(ref, D, L if mt is None else mt.Lk, per_head) + 2.0 ** -126
        err = np.abs(g - want)
        finite = bool(np.isfinite(g).all())
        zeros = bool((g[want == 0.0] == 0.0).all())
        live = want > 0
        ratio = float((err[live] / bnd[live]).max()) if finite and live.any() else float("inf")
        res.append({"name": tag + (" per head" if per_head else " head mean"), "worst_err_over_bound": ratio, "max_abs_err": float(np.nanmax(err)),
                    "top_probability_median": float(np.median(ref["per_head"].max(axis=-1)[ref["per_head"].max(axis=-1) > 0])),
                    "rel_l2": float(np.linalg.norm(np.nan_to_num(g - want)) / max(np.linalg.norm(want), 1e-300)), "tol": 1.0,
                    "ok": bool(finite and zeros and ratio <= 1.0)})
    return res


def check_self_attention_uncompacted(case, runs=2):
    """_SelfAttention.backward allocates its gradient with torch.empty_like and, under tables without a key_index (compact_keys =
    False), zero-fills nothing: the dK/dV kernels must write every row themselves, dead keys' rows included.  ops.self_attention +
    backward, `runs` times on freshly allocated inputs; before each backward a NaN-filled tensor of qkv's size is freed, so that
    empty_like is likely to be handed poisoned memory.  qkv.grad must be finite and equal to the oracle's every time."""
    from dreamvla_amd import ops
    from tests import attention_mask_cases as MC
    B, H, L, D = case["B"], case["H"], case["Lq"], case["D"]
    vis, mask, mt = MC.tables(case, device=DEV)
    g = torch.Generator().manual_seed(4200 + case["seed"])
    qkv, do = rnd((B, L, 3 * H * D), g), rnd((B, L, H * D), g)
    q, k, v = R.split_qkv(qkv, H)
    res = R.attention_bf16(q, k, v, scale=D ** -0.5, mask=mask, dout=do.view(B, L, H, D).permute(0, 2, 1, 3))
    want = torch.cat([R.merge_heads(t) for t in res[2:]], dim=-1)
    dead = torch.from_numpy(~vis.any(axis=0))
    W = H * D
    tag = "self_attention " + case["id"]
    out = [_exact(tag + ": tables carry neither a key_index nor a dead-key list", mt.key_index is None and not hasattr(mt, "dead_keys"))]
    for run in range(runs):
        qd = qkv.to(DEV, BF).requires_grad_(True)
        o = ops.self_attention(qd, H, mask_tables=mt, head_dim=D)
        poison = torch.full_like(qd, float("nan"))
        del poison
        probe = torch.empty_like(qd)          # (reported, not asserted: the caching allocator hands the freed block back)
        poisoned = bool(torch.isnan(probe).all())
        del probe
        o.backward(do.to(DEV, BF))
        got = qd.grad.detach().float().cpu()
        out.append(metrics(tag + f" run {run} o", o, R.merge_heads(res[0]), TOL_ATTN))
        out += [metrics(tag + f" run {run} {n}", got[..., i * W:(i + 1) * W], want[..., i * W:(i + 1) * W], TOL_ATTN_GRAD)
                for i, n in enumerate(("dq", "dk", "dv"))]
        out.append(_exact(tag + f" run {run}: dk / dv of the {int(dead.sum())} dead keys are 0", bool((got[:, dead, W:] == 0).all()),
                          gradient_memory_was_nan=poisoned))
        del qd, o
    return out


def check_linear_fn(M, K, N, act="none", conv1d=False, residual=False, bias=True, dropout_p=0.0, seed=0):
    from dreamvla_amd import ops
    from dreamvla_amd.ops import _Seeds
    g = torch.Generator().manual_seed(31 + seed)
    x = rnd((3, M // 3, K), g) if M % 3 == 0 else rnd((M, K), g)
    w = rnd((K, N) if conv1d else (N, K), g, 1.0 / math.sqrt(K))
    b = rnd((N,), g) if bias else None
    res = rnd(x.shape[:-1] + (N,), g) if residual else None
    dy = rnd(x.shape[:-1] + (N,), g)
    xd = x.to(DEV, BF).requires_grad_(True)
    wd = w.to(DEV, BF).requires_grad_(True)
    bd = b.to(DEV, BF).requires_grad_(True) if bias else None
    rd = res.to(DEV, BF).requires_grad_(True) if residual else None
    _Seeds.counter = 500 + seed
    y = ops.linear(xd, wd, bd, act=act, conv1d=conv1d, residual=rd, dropout_p=dropout_p)
    sd = (_Seeds.counter, _Seeds.next()[1])
    y.backward(dy.to(DEV, BF))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    rr = res.clone().requires_grad_(True) if residual else None
    pre = R.linear(xr, wr, br, conv1d)
    if act != "none":
        pre = pre + (R.bf16_round(pre.detach()) - pre.detach())  # forward sees the stored (bf16) pre-activation
    yr = R.act(pre, act)
    if dropout_p > 0:
        yr = R.dropout_elementwise(yr.reshape(-1, N), dropout_p, sd).view(yr.shape)
    if residual:
        yr = yr + (R.bf16_round(yr.detach()) - yr.detach())  # the reference adds the residual to a bf16 tensor
        yr = yr + rr
    yr.backward(dy)
    tag = f"linear M{M} K{K} N{N} {act} conv1d{int(conv1d)} res{int(residual)} p{dropout_p}"
    out = [metrics(tag + " y", y, yr, TOL_FWD), metrics(tag + " dx", xd.grad, xr.grad, TOL_GRAD),
           metrics(tag + " dw", wd.grad, wr.grad, TOL_GRAD)]
    if bias:
        out.append(metrics(tag + " db", bd.grad, br.grad, TOL_GRAD))
    if residual:
        out.append(metrics(tag + " dres", rd.grad, rr.grad, TOL_GRAD))
    return out


def check_mlp_fn(M, K, Hd, act="gelu_erf", conv1d=False, dropout_p=0.0, seed=0):
    from dreamvla_amd import ops
    from dreamvla_amd.ops import _Seeds
    g = torch.Generator().manual_seed(41 + seed)
    x = rnd((M, K), g)
    w1 = rnd((K, Hd) if conv1d else (Hd, K), g, 1.0 / math.sqrt(K))
    w2 = rnd((Hd, K) if conv1d else (K, Hd), g, 1.0 / math.sqrt(Hd))
    b1, b2 = rnd((Hd,), g), rnd((K,), g)
    dy = rnd((M, K), g)
    dev = [t.to(DEV, BF).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    _Seeds.counter = 900 + seed
    y = ops.mlp(dev[0], dev[1], dev[2], dev[3], dev[4], act=act, conv1d=conv1d, residual=dev[0], dropout_p=dropout_p)
    sd = (_Seeds.counter, _Seeds.next()[1])
    y.backward(dy.to(DEV, BF))
    ref = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    u = R.linear(ref[0], ref[1], ref[2], conv1d)
    u = u + (R.bf16_round(u.detach()) - u.detach())
    h = R.act(u, act)
    h = h + (R.bf16_round(h.detach()) - h.detach())  # h is stored in bf16 between the two GEMMs
    z = R.linear(h, ref[3], ref[4], conv1d)
    if dropout_p > 0:
        z = R.dropout_elementwise(z, dropout_p, sd)
    z = z + (R.bf16_round(z.detach()) - z.detach())  # `hidden + mlp(hidden)`: the branch output is a bf16 tensor
    yr = ref[0] + z
    yr.backward(dy)
    tag = f"mlp M{M} K{K} H{Hd} {act} conv1d{int(conv1d)} p{dropout_p}"
    names = ["dx", "dw1", "db1", "dw2", "db2"]
    out = [metrics(tag + " y", y, yr, TOL_FWD)]
    for n, d, r in zip(names, dev, ref):
        out.append(metrics(tag + " " + n, d.grad, r.grad, TOL_GRAD))
    return out


def check_misc():
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(5)
    out = []
    x = rnd((777, 1000), g)
    out.append(metrics("colsum 777x1000", ops.colsum(x.to(DEV, BF)), x.sum(0), TOL_F32 * 10, round_ref=False))
    x = rnd((50, 24), g)
    out.append(metrics("colsum 50x24", ops.colsum(x.to(DEV, BF)), x.sum(0), TOL_F32 * 10, round_ref=False))
    x = rnd((123, 96), g)
    sd = (5, 6)
    out.append(metrics("dropout 123x96 p0.1", ops.dropout_raw(x.to(DEV, BF), 0.1, sd), R.dropout_elementwise(x, 0.1, sd), TOL_FWD))
    keep = (ops.dropout_raw(torch.ones(4096, 1024, device=DEV, dtype=BF), 0.1, (9, 9)) != 0).float().mean().item()
    out.append({"name": "dropout keep-rate p0.1", "rel_l2": abs(keep - 0.9), "tol": 2e-3, "ok": abs(keep - 0.9) < 2e-3,
                "max_abs": keep, "finite": True})
    for a in ("gelu_erf", "gelu_tanh", "relu", "silu", "quick_gelu", "tanh", "sigmoid"):
        x = rnd((64, 256), g, 2.0)
        xr = x.clone().requires_grad_(True)
        yr = R.act(xr, a)
        dy = rnd((64, 256), g)
        yr.backward(dy)
        xd = x.to(DEV, BF).requires_grad_(True)
        y = ops.activation(xd, a)
        y.backward(dy.to(DEV, BF))
        out.append(metrics(f"act {a} fwd", y, yr, TOL_FWD))
        out.append(metrics(f"act {a} bwd", xd.grad, xr.grad, TOL_GRAD))
    x = rnd((1000, 64), g)
    out.append(metrics("cast f32->bf16", ops.cast_to(x.to(DEV) * 1.001, BF), (x * 1.001), TOL_FWD))
    b = rnd((64,), g)
    out.append(metrics("add bcast", ops.add_raw(x.to(DEV, BF), b.to(DEV, BF), 64), x + b, TOL_FWD))
    return out


def all_checks(quick=False):
    """yield (callable, kwargs) for the whole kernel matrix"""
    L = []
    # GEMM: all four layouts, ragged edges, tiny K, epilogues
    for at in (False, True):
        for bt in (False, True):
            L.append((check_gemm, dict(M=256, N=256, K=64, a_trans=at, b_trans=bt)))
            L.append((check_gemm, dict(M=197, N=200, K=72, a_trans=at, b_trans=bt, out_f32=True)))
    L += [
        (check_gemm, dict(M=300, N=136, K=40, bias=True, act="gelu_erf", residual=True)),
        (check_gemm, dict(M=130, N=264, K=96, bias=True, act="gelu_tanh", want_preact=True)),
        (check_gemm, dict(M=64, N=7, K=768, bias=True)),
        (check_gemm, dict(M=100, N=1024, K=6, bias=True)),
        (check_gemm, dict(M=100, N=64, K=7, b_trans=True, bias=True)),
        (check_gemm, dict(M=257, N=129, K=33)),
        (check_gemm_wide_stride, dict(variant=7)),
        (check_gemm_wide_stride, dict(variant=4)),
        # the DiT head's GEMMs at one episode (2 x 10 x 6 = 120 rows, models/action_model/models.py:128-160), the timestep MLP,
        # the output layer (N = 7), the CLIP tower at 77 rows, one-row problems, ragged N / M, fp32 output, pre-activation store
        (check_gemm_skinny, dict(M=120, N=2304, K=768, bias=True)),
        (check_gemm_skinny, dict(M=120, N=768, K=768, bias=True, residual=True, forced=False)),
        (check_gemm_skinny, dict(M=120, N=3072, K=768, bias=True, act="gelu_tanh", forced=False)),
        (check_gemm_skinny, dict(M=120, N=768, K=3072, bias=True, residual=True, forced=False)),
        (check_gemm_skinny, dict(M=20, N=768, K=256, bias=True, act="silu", forced=False)),
        (check_gemm_skinny, dict(M=120, N=7, K=768, bias=True, forced=False)),
        (check_gemm_skinny, dict(M=77, N=2048, K=512, bias=True, act="quick_gelu")),
        (check_gemm_skinny, dict(M=1, N=1024, K=512, bias=True, forced=False)),
        (check_gemm_skinny, dict(M=128, N=1000, K=80, act="relu", out_f32=True)),
        (check_gemm_skinny, dict(M=100, N=40, K=48, bias=True, act="gelu_erf", want_preact=True)),
        (check_gemm_skinny, dict(M=33, N=96, K=4096, bias=True, dropout_p=0.1, residual=True)),
        (check_act_bwd_colsum, dict(rows=20832, cols=1024, dropout_p=0.1)),                        # trunk c_proj / fc2 branches
        (check_act_bwd_colsum, dict(rows=1000, cols=4096, act="gelu_tanh", dropout_p=0.1, out_bf16=True)),
        (check_act_bwd_colsum, dict(rows=333, cols=520, act="relu")),                              # ragged strip (520 = 512 + 8)
        (check_act_bwd_colsum, dict(rows=7, cols=64, dropout_p=0.5)),                              # fewer rows than row slabs
        (check_act_bwd_colsum, dict(rows=100, cols=36, dropout_p=0.1)),                            # cols % 8 != 0: not taken
        # split-K with the epilogue in the reduction pass (forward GEMMs of the evaluation engine's trunk at one episode)
        (check_gemm, dict(M=930, N=1024, K=4096, b_trans=True, bias=True, residual=True, split_k=4)),   # GPT-2 MLP down-projection, Conv1D
        (check_gemm, dict(M=930, N=1024, K=4096, b_trans=True, bias=True, residual=True)),             # ... as ops.gemm splits it by itself
        (check_gemm, dict(M=651, N=1024, K=4096, bias=True, act="gelu_tanh", split_k=2, variant=6)),
        (check_gemm, dict(M=700, N=520, K=2048, bias=True, act="relu", residual=True, split_k=2)),      # ragged tiles
        (check_gemm, dict(M=600, N=256, K=2048, residual=True, out_f32=True, split_k=3)),
        (check_dit_team, dict(bs=1, model_type="DiT-B")),                                           # one episode: 12 token rows
        (check_dit_team, dict(bs=1, model_type="DiT-B", seeds=(7, 8), call_per_phase=True)),       # the kernel without look-ahead (A/B variant)
        (check_dit_team, dict(bs=1, model_type="DiT-B", seeds=(4, 5), fp32_master=True)),          # fp32 master parameters: bf16 bias shadows
        (check_gemm_tail, dict(M=256, N=256, K=160, out_f32=True)),                                # 2.5 K-tiles
        (check_gemm_tail, dict(M=512, N=256, K=208, out_f32=True)),                                # tail of one k16-step
        (check_gemm_tail, dict(M=256, N=768, K=1264, out_f32=True)),                               # tail of three, 19.75 K-tiles
        (check_gemm_tail, dict(M=1024, N=512, K=2080, split_k=3)),                                 # split-K: only the last slice is ragged
        (check_gemm_tail, dict(M=768, N=1024, K=4128, split_k=4, out_f32=True)),
        (check_gemm_ln, dict(M=120, N=2304, K=768)),                                                # DiT qkv(norm1(x))
        (check_gemm_ln, dict(M=120, N=3072, K=768, act="gelu_tanh")),                               # fc1(norm2(x))
        (check_gemm_ln, dict(M=120, N=7, K=768)),                                                   # output layer
        (check_gemm_ln, dict(M=33, N=96, K=1536, residual=True, eps=1e-5)),
        (check_gemm_ln, dict(M=512, N=64, K=512, bias=False)),
        (check_gemm_skinny, dict(M=394, N=2304, K=768, bias=True, forced=False)),                 # the ViT on the newest frame's two views
        (check_gemm_skinny, dict(M=394, N=768, K=3072, bias=True, residual=True, forced=False)),
        (check_gemm_skinny, dict(M=512, N=320, K=496, act="gelu_erf", bias=True)),                # four-wave variant (K < 512), ragged K share
        (check_gemm, dict(M=128, N=128, K=2048, a_trans=True, b_trans=True, split_k=4)),
        (check_gemm, dict(M=200, N=72, K=1000, a_trans=True, b_trans=True, split_k=3)),
        (check_gemm, dict(M=256, N=128, K=64, dropout_p=0.1, residual=True)),
        (check_gemm, dict(M=256, N=128, K=64, dact="gelu_tanh")),
        (check_gemm, dict(M=1024, N=1024, K=1024, bias=True, act="relu")),
        # persistent ring kernels: several work items per workgroup, ragged M / N edges, every epilogue flavour
        (check_gemm, dict(M=4352, N=4096, K=96, bias=True)),
        (check_gemm, dict(M=4224, N=2048, K=64, b_trans=True)),
        (check_gemm, dict(M=4300, N=1152, K=128, bias=True, act="gelu_erf", residual=True)),
        (check_gemm, dict(M=2100, N=1024, K=160, bias=True, act="gelu_tanh", want_preact=True)),
        (check_gemm, dict(M=2048, N=1024, K=96, b_trans=True, dact="gelu_tanh")),
        (check_gemm, dict(M=2049, N=1088, K=64, bias=True, dropout_p=0.1, residual=True)),
        (check_gemm, dict(M=1024, N=768, K=4128, a_trans=True, b_trans=True, split_k=5, out_f32=True)),
        (check_gemm, dict(M=1300, N=832, K=64, bias=True, out_f32=True, residual=True)),
        (check_gemm, dict(M=768, N=3072, K=2048, a_trans=True, b_trans=True, split_k=3)),
    ]
    # every hand-written configuration forced in turn over the epilogue matrix (the tuner locks 2 / 4 / 5 / 6 on the model's
    # shapes; a forced configuration that does not take a shape falls back inside the library, which is still a valid run):
    # 2 = register-staged 128x128, 4 / 6 / 7 = LDS-DMA ring 256x256 / 128x128 / 256x128 BK 64, 8 = phase kernel 256x256 BK 64
    # (9 = the same kernel under the stream-K hybrid schedule: below, at sizes where it engages)
    for v in (2, 4, 6, 7, 8):
        L += [
            (check_gemm, dict(M=2100, N=1024, K=256, bias=True, act="gelu_tanh", want_preact=True, variant=v)),
            (check_gemm, dict(M=4300, N=1152, K=128, bias=True, act="gelu_erf", residual=True, variant=v)),
            (check_gemm, dict(M=2049, N=1088, K=192, bias=True, dropout_p=0.1, residual=True, variant=v)),
            (check_gemm, dict(M=2048, N=1024, K=320, b_trans=True, dact="gelu_tanh", variant=v)),
            (check_gemm, dict(M=2304, N=1024, K=256, dact="gelu_erf", variant=v)),
            (check_gemm, dict(M=1111, N=768, K=768, bias=True, variant=v)),
            (check_gemm, dict(M=1500, N=1024, K=512, b_trans=True, variant=v)),
            (check_gemm, dict(M=1024, N=768, K=4224, a_trans=True, b_trans=True, split_k=3, out_f32=True, variant=v)),
            (check_gemm, dict(M=768, N=1024, K=2048, a_trans=True, b_trans=True, out_f32=True, variant=v)),
            (check_gemm, dict(M=1300, N=832, K=128, bias=True, out_f32=True, residual=True, variant=v)),
            (check_gemm, dict(M=1024, N=512, K=1024, a_trans=True, variant=v)),
        ]
    # k-sums next to the product (the bias gradient rides on the weight-gradient GEMM): both operands, every configuration
    # (2 has no summing code: the library runs its column-sum kernel on the operand), ragged M / N, split-K and not, bf16 / fp32
    for v in (None, 2, 4, 6, 7, 8, 9):
        L += [
            (check_gemm_ksum, dict(M=1024, N=768, K=4224, which="a", split_k=3, variant=v)),
            (check_gemm_ksum, dict(M=1024, N=768, K=4224, which="b", split_k=3, variant=v)),
            (check_gemm_ksum, dict(M=1100, N=832, K=2048, which="a", split_k=4, variant=v, ksum_f32=True)),
            (check_gemm_ksum, dict(M=1100, N=832, K=2048, which="b", split_k=1, out_f32=True, variant=v, ksum_f32=True)),
            (check_gemm_ksum, dict(M=300, N=4096, K=20832, which="b", split_k=4, variant=v)),
        ]
    L += [(check_gemm_ksum, dict(M=4096, N=1024, K=20832, which="b", split_k=4)),          # trunk fc2 dW + db (Conv1D layout)
          (check_gemm_ksum, dict(M=1024, N=4096, K=20832, which="b", split_k=4, variant=4)),
          (check_gemm_ksum, dict(M=4096, N=1024, K=91840, which="a", split_k=4, variant=8)),  # decoder fc1 dW + db (nn.Linear layout)
          (check_gemm_ksum, dict(M=512, N=512, K=1024, which="a", split_k=1)),             # bf16 C, no split: not the fp32 class -> column-sum kernel
          (check_gemm_ksum, dict(M=640, N=512, K=1024, which="a", split_k=2, a_trans=False, b_trans=False, variant=4))]   # any layout when fused (ring kernels)
    # 9 = the phase kernel's stream-K hybrid schedule: it only engages from one tile per CU upwards (328 tiles here: 20.5
    # super-tiles of 16, i.e. ragged), with tiles shared by two workgroups -- every epilogue class, both slab paths, twice in a
    # row on the same scratch (the flags must come back down)
    for rep in range(2):
        L += [
            (check_gemm, dict(M=20832, N=1024, K=320, bias=True, act="gelu_tanh", want_preact=True, variant=9, seed=rep)),
            (check_gemm, dict(M=20832, N=1024, K=192, bias=True, dropout_p=0.1, residual=True, b_trans=True, variant=9, seed=rep)),
            (check_gemm, dict(M=20832, N=1024, K=448, dact="gelu_erf", variant=9, seed=rep)),
            (check_gemm, dict(M=20992, N=1024, K=256, a_trans=True, b_trans=True, out_f32=True, variant=9, seed=rep)),
            (check_gemm, dict(M=21000, N=1088, K=128, bias=True, act="gelu_erf", residual=True, variant=9, seed=rep)),
        ]
    # 10 = the FULL stream-K schedule (every tile in the K-iteration ranges): same shapes as 9
    for rep in range(2):
        L += [
            (check_gemm, dict(M=20832, N=1024, K=320, bias=True, act="gelu_tanh", want_preact=True, variant=10, seed=rep)),
            (check_gemm, dict(M=20832, N=1024, K=192, bias=True, dropout_p=0.1, residual=True, b_trans=True, variant=10, seed=rep)),
            (check_gemm, dict(M=20992, N=1024, K=256, a_trans=True, b_trans=True, out_f32=True, variant=10, seed=rep)),
            (check_gemm, dict(M=21000, N=1088, K=128, bias=True, act="gelu_erf", residual=True, variant=10, seed=rep)),
        ]
    # the benchmarked step's own GEMM problems at full size, real K, real epilogue, every locked configuration
    L += [(check_gemm_model_scale, dict(name=n)) for n in MODEL_GEMMS]
    L += [(check_flat_adamw, dict()), (check_direct_grads, dict()), (check_assemble_tokens, dict()),
          (check_concat_shared_suffix, dict()), (check_concat_shared_suffix, dict(n=5, nq=9, ns=256, D=3072, seed=1))]
    L += [(check_fused_losses, dict(case_name=c)) for c in ("C_calvin_dit", "E_libero_all_heads", "E_atten_goal")]
    L += [(check_fused_losses_vs_training_loop, dict(case_name=c)) for c in ("C_calvin_dit", "A_mlp_head", "E_libero_all_heads", "E_atten_goal")]
    L += [
        (check_layernorm, dict(rows=37, cols=768, eps=1e-6)),
        (check_layernorm, dict(rows=1000, cols=1024)),
        (check_layernorm, dict(rows=5000, cols=1024, param_f32=True)),
        (check_layernorm, dict(rows=64, cols=512)),
        (check_layernorm, dict(rows=33, cols=768, affine=False, eps=1e-6)),
        (check_layernorm, dict(rows=9, cols=2048)),
        (check_layernorm_fork, dict(rows=1000, cols=1024)),
        (check_layernorm_fork, dict(rows=77, cols=768, affine=False, eps=1e-6)),
        (check_layernorm_last_tokens, dict(n=5, L=205, keep=196, cols=1024)),
        (check_layernorm_last_tokens, dict(n=3, L=265, keep=256, cols=1024, param_f32=True)),
        (check_layernorm_last_tokens, dict(n=7, L=21, keep=21, cols=768, eps=1e-6)),
        (check_layernorm_last_tokens, dict(n=4, L=40, keep=1, cols=512)),
        (check_layernorm_concat, dict(n=6, La=196, Lb=16, cols=768, a_needs_grad=False)),
        (check_layernorm_concat, dict(n=5, La=33, Lb=7, cols=1024)),
    ]
    L += [
        (check_self_attention, dict(B=2, H=2, L=32)),
        (check_self_attention, dict(B=2, H=3, L=197)),
        (check_self_attention, dict(B=3, H=2, L=6)),
        (check_self_attention, dict(B=1, H=2, L=265)),
        # the packed path of ops.self_attention (short sequences under a block-diagonal mask): the DiT head's shape class
        # (L = 6: 16 sequences per 96-token pack), a length that does not divide 32 and a batch that forces a smaller pack
        (check_self_attention, dict(B=224, H=12, L=6)),
        (check_self_attention, dict(B=130, H=2, L=11, seed=3)),
        (check_self_attention, dict(B=64, H=3, L=16, seed=4)),
        (check_self_attention, dict(B=2, H=2, L=133, mask_kind="block")),
        (check_self_attention, dict(B=1, H=4, L=399, mask_kind="block")),
        (check_self_attention, dict(B=2, H=2, L=77, mask_kind="causal")),
        (check_self_attention, dict(B=2, H=2, L=133, mask_kind="block", dropout_p=0.1)),
        (check_self_attention, dict(B=1, H=1, L=64, dropout_p=0.25)),
        # the benchmarked configuration's attention problem: real generate_attention_mask, 16 heads, forward + backward
        (check_self_attention, dict(B=2, H=16, L=651, mask_kind="dreamvla")),
        (check_self_attention, dict(B=2, H=16, L=651, mask_kind="dreamvla", dropout_p=0.1)),
        (check_self_attention, dict(B=2, H=16, L=930, mask_kind="dreamvla")),
        (check_self_attention, dict(B=2, H=16, L=930, mask_kind="dreamvla", dropout_p=0.1)),
        # ... at the benchmark's batch: B = 32 trunk (oracle on 8 sampled rows; all rows == their representative without
        # dropout), the decoders' B = 2 * 32 * 7 = 448 sequences of 9 + 196 / 9 + 256 tokens, the DiT head's 1792 x 6
        (check_self_attention, dict(B=2, H=16, L=798, mask_kind="pretrain")),
        (check_self_attention, dict(B=2, H=16, L=798, mask_kind="pretrain", dropout_p=0.1)),
        # round-4 VERDICT missing #4: the real mask at the other shipped lengths -- LIBERO (L = 525), all dream heads (L = 777) and
        # the survey's maximum L = 1302, where the dK/dV kernel's 80-KiB LDS cap decides between the ring kernel and the staged one
        (check_self_attention, dict(B=2, H=16, L=525, mask_kind="dreamvla_D")),
        (check_self_attention, dict(B=2, H=16, L=525, mask_kind="dreamvla_D", dropout_p=0.1)),
        (check_self_attention, dict(B=2, H=16, L=777, mask_kind="dreamvla_E")),
        (check_self_attention, dict(B=2, H=16, L=777, mask_kind="dreamvla_E", dropout_p=0.1)),
        (check_self_attention, dict(B=1, H=16, L=1302, mask_kind="dreamvla")),
        (check_self_attention, dict(B=1, H=16, L=1302, mask_kind="dreamvla", dropout_p=0.1)),
        # walks of more than 64 tiles (L > 2048): the ring kernels keep their tile flags in SGPR words up to 64 tiles (round 5)
        # and walk the LDS table beyond -- these two run the table walk
        (check_self_attention, dict(B=1, H=2, L=2085, seed=5)),
        (check_self_attention, dict(B=1, H=2, L=2085, mask_kind="block", dropout_p=0.1, seed=6)),
        (check_self_attention, dict(B=32, H=16, L=651, mask_kind="dreamvla", dropout_p=0.1, rows=8)),
        (check_self_attention, dict(B=32, H=16, L=651, mask_kind="dreamvla", rows=6, period=5)),
        (check_self_attention, dict(B=448, H=16, L=205, rows=10, period=9)),
        (check_self_attention, dict(B=448, H=16, L=265, rows=10, period=9, seed=1)),
        (check_self_attention, dict(B=448, H=12, L=197, rows=8, period=7, grad=False)),
        (check_self_attention, dict(B=1792, H=12, L=6, rows=32, period=48)),
        (check_self_attention_small, dict(B=5, H=4, L=6, D=96)),
        (check_self_attention_small, dict(B=3, H=2, L=33, D=128, seed=1)),
        (check_self_attention_small, dict(B=2, H=3, L=64, D=40, seed=2)),
        (check_cross_attention, dict(B=3, H=8, Lq=16, Lk=212)),
        (check_cross_attention, dict(B=448, H=8, Lq=16, Lk=212, seed=2)),     # the resampler at the step's batch: 2 views x 32 x 7
        (check_cross_attention, dict(B=2, H=2, Lq=40, Lk=33)),
    ]
    L += [
        (check_linear_fn, dict(M=192, K=96, N=160)),
        (check_linear_fn, dict(M=192, K=96, N=160, conv1d=True, residual=True, dropout_p=0.1)),
        (check_linear_fn, dict(M=150, K=64, N=72, act="relu")),
        (check_linear_fn, dict(M=90, K=7, N=64, bias=True)),
        (check_linear_fn, dict(M=2500, K=128, N=128, bias=False)),
        (check_mlp_fn, dict(M=200, K=128, Hd=512)),
        (check_mlp_fn, dict(M=333, K=64, Hd=256, act="gelu_tanh", conv1d=True, dropout_p=0.1)),
        (check_misc, dict()),
    ]
    # the output side of the wide-stride case (appended here: the ids of the cases above stay what they were).  One 8.66-GB
    # buffer at a time, freed inside the case
    for v in (4, 7, 8):
        L += [(check_gemm_wide_stride_out, dict(variant=v, which="out")),
              (check_gemm_wide_stride_out, dict(variant=v, which="residual"))]
    # forced variant numbers that name nothing (any more): the fallback, and nothing else, runs
    for v in (44, 85):
        L.append((check_gemm_retired_variant, dict(variant=v)))
    return L


def check_fused_losses(case_name):
    """the HIP loss kernels (dvla_patch_mse_* / dvla_cosine_loss_* / dvla_silog_loss_*) against the ATen formulation of
    dreamvla_amd/losses.py -- which is pinned to the real training loop (tests/test_losses_golden.py) -- on the same
    bf16 inputs: loss terms (fp32 sums in another order: 2e-5 rel) and the bf16 prediction gradients."""
    from dreamvla_amd import losses
    from oracle.make_golden_losses import CASES, loss_case_tensors
    case = CASES[case_name]
    batch, preds = loss_case_tensors(case)
    batch["actions"][..., 6:] = (batch["actions"][..., 6:] + 1) // 2
    S, ag = case["S"], case.get("atten_goal", 0)
    dev_batch = {k: (v.to(DEV, BF) if torch.is_floating_point(v) else v.to(DEV)) for k, v in batch.items()}
    lab = losses.label_actions(dev_batch["actions"], S, 3, atten_goal=ag)
    out, results = [], {}
    for fused in (True, False):
        leaves = {k: v.to(DEV, BF).clone().requires_grad_(True) for k, v in preds.items()}
        if case["use_dit_head"]:
            leaves["arm"] = preds["arm"].to(DEV).float().requires_grad_(True)
        g = leaves.get
        o = (leaves["arm"], g("gripper", leaves["arm"]), g("image"), None, None, None, g("depth"), g("traj"), g("dino"), g("sam"))
        total, parts = losses.calvin_losses(o, dev_batch, sequence_length=S, atten_goal=ag, use_dit_head=case["use_dit_head"],
                                            label_action=lab, flow_as_mask=case["flow_as_mask"], fused=None if fused else False)
        total.backward()
        results[fused] = (total.detach(), {k: v.detach() for k, v in parts.items()},
                          {k: v.grad.detach().float() for k, v in leaves.items() if v.grad is not None})
    tf, pf, gf = results[True]
    ta, pa, ga = results[False]
    tag = f"fused losses {case_name}"
    out.append(metrics(tag + " total", tf.reshape(1), ta.reshape(1).cpu(), 2e-5, round_ref=False))
    for k in ("image", "depth", "dino", "sam"):
        out.append(metrics(f"{tag} {k}", pf[k].float().reshape(1), pa[k].float().reshape(1).cpu(), 2e-5, round_ref=False))
    for k in ("image", "depth", "dino", "sam"):
        if k in ga:
            out.append(metrics(f"{tag} d{k}", gf[k], ga[k].cpu(), TOL_GRAD, round_ref=False))
    return out


def check_fused_losses_vs_training_loop(case_name):
    """ONE hop (round-2 VERDICT: a12 was HIP <-> product ATen code <-> real loop): the HIP loss kernels on the GPU against the
    loss values and prediction gradients of the REAL reference training loop (utils/train_utils.py:train_one_epoch_calvin run
    on CPU by oracle/make_golden_losses.py -> tests/golden/losses.pt).  The fixture's inputs are bf16-representable, so the
    bf16 kernels see exactly the numbers the loop saw: loss terms differ by fp32 summation order only, the bf16 prediction
    gradients by their final rounding."""
    import os
    from dreamvla_amd import losses
    from oracle.make_golden_losses import loss_case_tensors
    fx = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.pt"), map_location="cpu")["cases"][case_name]
    case = fx["case"]
    batch, preds = loss_case_tensors(case)
    batch["actions"][..., 6:] = (batch["actions"][..., 6:] + 1) // 2
    S, ag = case["S"], case.get("atten_goal", 0)
    dev_batch = {k: (v.to(DEV, BF) if torch.is_floating_point(v) else v.to(DEV)) for k, v in batch.items()}
    lab = losses.label_actions(dev_batch["actions"], S, 3, atten_goal=ag)
    leaves = {k: v.to(DEV, BF).clone().requires_grad_(True) for k, v in preds.items()}
    if case["use_dit_head"]:
        leaves["arm"] = preds["arm"].to(DEV).float().requires_grad_(True)
    g = leaves.get
    o = (leaves["arm"], g("gripper", leaves["arm"]), g("image"), None, None, None, g("depth"), g("traj"), g("dino"), g("sam"))
    total, parts = losses.calvin_losses(o, dev_batch, sequence_length=S, atten_goal=ag, use_dit_head=case["use_dit_head"],
                                        label_action=lab, flow_as_mask=case["flow_as_mask"], fused=None)
    total.backward()
    want = fx["losses"]
    names = {"loss_arm_action": "arm_action", "loss_gripper_action": "gripper_action", "loss_image": "image", "loss_depth": "depth",
             "loss_dino_feat": "dino", "loss_sam_feat": "sam", "loss_pred_trajectory": "trajectory"}
    tag = f"HIP losses vs real training loop {case_name}"
    out = [metrics(tag + " total", total.detach().float().reshape(1), torch.tensor([want["loss"]]), 3e-5, round_ref=False)]
    for k_ref, k in names.items():
        if want[k_ref] != 0.0:
            out.append(metrics(f"{tag} {k}", parts[k].detach().float().reshape(1), torch.tensor([want[k_ref]]), 3e-5, round_ref=False))
    for k, smp in fx["grads"].items():
        if leaves[k].grad is None or leaves[k].dim() == 0:
            continue
        gv = leaves[k].grad.detach().float().cpu().flatten()[smp["idx"]]
        out.append(metrics(f"{tag} d{k}", gv, smp["vals"], TOL_FWD if leaves[k].dtype == BF else 1e-5, round_ref=leaves[k].dtype == BF))
    return out


def check_assemble_tokens(B=3, S=4, H=1024, seed=0):
    """ops.assemble_tokens (dvla_assemble_tokens) == torch.cat(parts, dim=2) + pos bit for bit (bf16 add of the same two
    values), with ordinary parts, a per-sample embedding broadcast over time and learned tokens broadcast over (B, S);
    gradients == autograd of the cat formulation."""
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(321 + seed)
    mk = lambda *s: rnd(s, g).to(DEV, BF)
    out = []
    leaves = {}
    for mode in ("hip", "ref"):
        gg = torch.Generator().manual_seed(321 + seed)
        mk = lambda *s: rnd(s, gg).to(DEV, BF).requires_grad_(True)
        text, state, img = mk(B, 1, 1, H), mk(B, S, 1, H), mk(B, S, 16, H)
        tok_a, tok_b, pos = mk(1, 1, 18, H), mk(1, 1, 3, H), mk(1, S, 1, H)
        sliced = mk(B, S, 40, H)
        parts = [text.expand(B, S, 1, H), state, img, sliced[:, :, 5:7], tok_a.expand(B, S, -1, -1), tok_b.expand(B, S, -1, -1)]
        y = ops.assemble_tokens(parts, pos) if mode == "hip" else torch.cat(parts, dim=2) + pos
        w = rnd(tuple(y.shape), torch.Generator().manual_seed(9)).to(DEV, BF)
        (y.float() * w.float()).sum().backward()
        leaves[mode] = (y.detach(), [t.grad.detach().float() for t in (text, state, img, tok_a, tok_b, pos, sliced)])
    yh, gh = leaves["hip"]
    yr, gr = leaves["ref"]
    out.append({"name": "assemble_tokens == cat + pos (bit-exact)", "rel_l2": rel_l2(yh, yr), "tol": 0.0, "ok": bool(torch.equal(yh, yr))})
    for nm, a, b in zip(("text", "state", "img", "tok_a", "tok_b", "pos", "sliced"), gh, gr):
        out.append(metrics(f"assemble_tokens d{nm}", a, b.cpu(), 1e-6, round_ref=False))
    return out


def check_concat_shared_suffix(n=37, nq=9, ns=196, D=1024, seed=0):
    """ops.concat_shared_suffix == torch.cat((prefix, suffix.expand(n, ...)), 1) bit for bit; prefix gradient = the slice,
    suffix gradient = the batch sum (fp32 accumulation, one bf16 rounding -- what autograd's expand-backward does)."""
    from dreamvla_amd import ops
    res = {}
    for mode in ("hip", "ref"):
        gg = torch.Generator().manual_seed(77 + seed)
        big = rnd((n, nq + 2, D), gg).to(DEV, BF).requires_grad_(True)
        suffix = rnd((ns, D), gg).to(DEV, BF).requires_grad_(True)
        prefix = big[:, 1:1 + nq]                                  # a strided view, as a caller may hand over
        y = ops.concat_shared_suffix(prefix, suffix) if mode == "hip" else torch.cat((prefix, suffix.unsqueeze(0).expand(n, -1, -1)), 1)
        w = rnd(tuple(y.shape), torch.Generator().manual_seed(9)).to(DEV, BF)
        (y.float() * w.float()).sum().backward()
        res[mode] = (y.detach(), big.grad.detach().float(), suffix.grad.detach().float())
    yh, gph, gsh = res["hip"]
    yr, gpr, gsr = res["ref"]
    return [{"name": "concat_shared_suffix == cat (bit-exact)", "rel_l2": rel_l2(yh, yr), "tol": 0.0, "ok": bool(torch.equal(yh, yr))},
            metrics("concat_shared_suffix dprefix", gph, gpr.cpu(), 1e-6, round_ref=False),
            metrics("concat_shared_suffix dsuffix", gsh, gsr.cpu(), 4e-3, round_ref=False)]


def check_direct_grads(seed=0):
    """GradBucketReducer(direct_grads=True): the backward kernels write weight / bias / LayerNorm gradients into the bucket
    slots and autograd adopts them (no accumulation add) -- same gradients as plain autograd, and p.grad aliases the slot."""
    import dreamvla_amd.nn as dnn
    from dreamvla_amd.ddp import GradBucketReducer
    torch.manual_seed(11 + seed)
    blk = torch.nn.Sequential(dnn.Block(128, 2, mlp_ratio=4, qkv_bias=True), dnn.Block(128, 2, mlp_ratio=4, qkv_bias=True))
    head = dnn.Linear(128, 64)
    mods = torch.nn.ModuleList([blk, head]).to(DEV, BF)
    params = list(mods.parameters())
    g = torch.Generator().manual_seed(5 + seed)
    out = []
    ref = None
    for mode in ("plain", "direct"):
        red = GradBucketReducer(params, bucket_bytes=200_000, direct_grads=True) if mode == "direct" else None
        for step in range(2):
            x = rnd((6, 40, 128), torch.Generator().manual_seed(100 + step)).to(DEV, BF)
            if red is not None:
                red.zero_grad()
            else:
                for p in params:
                    p.grad = None
            y = head(blk(x))
            y.float().pow(2).mean().backward()
            if red is not None:
                red.finish()
        grads = [(red.grad_of(p) if red is not None else p.grad).detach().float().cpu() for p in params]
        if mode == "plain":
            ref = grads
        else:
            aliased = sum(int(p.grad is not None and p.grad.data_ptr() == red.grad_of(p).data_ptr()) for p in params)
            out.append({"name": f"direct_grads: {aliased}/{len(params)} gradients in their slot, {red.copied} copied by the hook",
                        "rel_l2": 0.0, "tol": 0.0, "ok": aliased == len(params) and red.copied == 0})
            got = torch.cat([t.reshape(-1) for t in grads])
            want = torch.cat([t.reshape(-1) for t in ref])
            out.append(metrics("direct_grads: gradients == plain autograd", got, want, TOL_GRAD, round_ref=False))
            for p in params:                   # leave the parameters as plain leaves
                p.grad = None
    return out


def check_flat_adamw(seed=0):
    """dreamvla_amd.optim.FlatAdamW (dvla_sumsq_bf16 + dvla_adamw_bf16) vs the oracle's clip + AdamW restatement."""
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    g = torch.Generator().manual_seed(77 + seed)
    shapes = [(1024, 1024), (1024,), (333, 77), (5,), (4096, 256)]
    host = [(torch.randn(s, generator=g) * 0.2).to(BF) for s in shapes]
    params = [torch.nn.Parameter(h.clone().to(DEV)) for h in host]
    red = GradBucketReducer(params, bucket_bytes=3 << 20)      # several buckets
    opt = FlatAdamW(red, lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, max_grad_norm=0.1)
    mine = [h.clone() for h in host]
    m = [torch.zeros_like(h) for h in host]
    v = [torch.zeros_like(h) for h in host]
    out = []
    for step in range(1, 4):
        grads = [(torch.randn(s, generator=g) * (2.0 if step != 2 else 1e-3)).to(BF) for s in shapes]
        red.zero_grad()
        for p, gr in zip(params, grads):
            p.grad.copy_(gr.to(DEV))
        opt.step()
        norm_o = R.clip_adamw_step(mine, grads, m, v, step, 1e-2, (0.9, 0.95), 1e-8, 0.05, max_norm=0.1)
        out.append(metrics(f"flat_adamw step{step} grad_norm", opt.grad_norm().cpu(), norm_o.reshape(1), 1e-5, round_ref=False))
        got = torch.cat([p.detach().float().cpu().reshape(-1) for p in params])
        ref = torch.cat([q.float().reshape(-1) for q in mine])
        out.append(metrics(f"flat_adamw step{step} params", got, ref, 1e-3 if step > 1 else 1e-6, round_ref=False))
    # --- checkpoint / resume (the reference saves optimizer_state_dict): state_dict -> step -> restore -> same step again
    sd = opt.state_dict()
    snap = [s["p"].clone() for s in opt.flat]
    gr = [(torch.randn(s, generator=g) * 2.0).to(BF) for s in shapes]

    def one_step():
        red.zero_grad()
        for p, t in zip(params, gr):
            p.grad.copy_(t.to(DEV))
        opt.step()
        return torch.cat([p.detach().float().cpu().reshape(-1) for p in params])
    first = one_step()
    for s_, keep in zip(opt.flat, snap):
        s_["p"].copy_(keep)
    opt.load_state_dict(sd)
    again = one_step()
    out.append({"name": "flat_adamw state_dict round trip reproduces the step bit for bit", "rel_l2": rel_l2(again, first), "tol": 0.0,
                "ok": bool(torch.equal(again, first)) and opt.step_count == sd["step"] + 1})
    # --- a torch LR scheduler drives it (train.py attaches one to its AdamW)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.25)
    out.append({"name": "flat_adamw accepts a torch LR scheduler", "rel_l2": 0.0, "tol": 0.0,
                "ok": abs(opt.param_groups[0]["lr"] - 0.25e-2) < 1e-12 and sched is not None})
    # --- parameters the reducer learned to be unused are left alone (torch AdamW skips p.grad is None): no decay
    bi = next(i for i, b in enumerate(red.buckets) if len(b["params"]) > 1)
    red.buckets[bi]["expected"][0] = False
    victim = red.buckets[bi]["params"][0]
    before = victim.detach().clone()
    others_before = params[0].detach().clone() if params[0] is not victim else params[1].detach().clone()
    one_step()
    other = params[0] if params[0] is not victim else params[1]
    out.append({"name": "flat_adamw leaves never-used parameters untouched", "rel_l2": 0.0, "tol": 0.0,
                "ok": bool(torch.equal(victim.detach(), before)) and not torch.equal(other.detach(), others_before)})
    return out


# ---------------------------------------------------------------------------------------------------
# LayerNorm and element-wise kernels on the paths of tests/rowwise_cases.py, against the UNROUNDED float64 result
# (tests/test_layernorm_paths_gpu.py, tests/test_elementwise_paths_gpu.py).
#   LayerNorm y / dx, per row:   |got - ref64| <= ulp_bf16(ref64) / 2 + (1 + kappa_row) * 2^-20 * max_row |ref64|
#     the final rounding, plus fp32 round-off (2^-24) amplified by the row's conditioning kappa = |mean| * rstd, with a factor 16
#     for the accumulations.  A misplaced row or lane is off by about max_row |ref64|.
#   activations, per element:    |got - ref64| <= ulp_bf16(ref64) / 2 + 2^-20 * |dy| * max(1, |x|)        (forward: dy = 1)
#     8 fp32 ulps of 1: two 1-ulp hardware approximations (v_exp_f32, v_rcp_f32), doubled in tanh2, and the 1.5e-7 of the erfc form.
# `slack` is the largest part of an error that the rounding term did not cover, relative to the row's (element's) scale, and
# `allow_frac` the largest fraction of the allowance that was used: what DESIGN.md quotes.
# ---------------------------------------------------------------------------------------------------
LN_ALLOW = 2.0 ** -20
ACT_ALLOW = 2.0 ** -20


def ulp_bf16(ref64):
    """spacing of bf16 at |ref64| (float64 tensor); subnormal spacing 2^-133 below 2^-126"""
    _, e = torch.frexp(ref64.abs())
    e = torch.where(ref64 == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(ref64), (e - 1).clamp(min=-126) - 7)


def rowwise(name, got, ref64, kappa):
    """the per-row LayerNorm criterion; ref64 (rows, cols) float64, kappa (rows,)"""
    g = got.detach().double().cpu().reshape(ref64.shape)
    finite = bool(torch.isfinite(g).all()) and bool(torch.isfinite(ref64).all())
    d = (g - ref64).abs()
    ex_row = (d - 0.5 * ulp_bf16(ref64)).clamp(min=0).amax(-1)
    rowmax = ref64.abs().amax(-1)
    allow = (1.0 + kappa.double()) * LN_ALLOW * rowmax
    bad = ex_row > allow
    nz = rowmax > 0
    slack = float((ex_row[nz] / rowmax[nz]).max()) if bool(nz.any()) else 0.0
    fr = torch.where(nz, ex_row / allow.clamp(min=1e-300), torch.zeros_like(ex_row))
    frac = float(fr.max()) if fr.numel() else 0.0
    idx = int(d.flatten().argmax()) if d.numel() else 0
    return {"name": name, "rel_l2": rel_l2(g, ref64), "max_abs": float(d.max()) if d.numel() else 0.0, "worst_index": idx,
            "slack": slack, "allow_frac": frac, "allow_frac_row": int(fr.argmax()) if fr.numel() else -1, "bad_rows": int(bad.sum()), "first_bad_row": int(bad.nonzero()[0]) if bool(bad.any()) else -1,
            "finite": finite, "tol": LN_ALLOW, "shape": list(g.shape), "ok": bool(finite and not bad.any())}


def elementwise(name, got, ref64, scale):
    """the per-element activation criterion; scale = |dy| * max(1, |x|) (float64, broadcastable)"""
    g = got.detach().double().cpu().reshape(ref64.shape)
    finite = bool(torch.isfinite(g).all()) and bool(torch.isfinite(ref64).all())
    d = (g - ref64).abs()
    ex = (d - 0.5 * ulp_bf16(ref64)).clamp(min=0)
    allow = ACT_ALLOW * scale.expand_as(ref64)
    bad = ex > allow
    nz = allow > 0
    slack = float((ex[nz] / scale.expand_as(ref64)[nz]).max()) if bool(nz.any()) else 0.0
    idx = int((ex - allow).flatten().argmax()) if d.numel() else 0
    return {"name": name, "rel_l2": rel_l2(g, ref64), "max_abs": float(d.max()) if d.numel() else 0.0, "worst_index": idx,
            "slack": slack, "allow_frac": slack / ACT_ALLOW, "bad": int(bad.sum()), "finite": finite, "tol": ACT_ALLOW,
            "shape": list(g.shape), "ok": bool(finite and not bad.any())}


def same_bits(name, got, want):
    """bit for bit (NaN patterns: NaN where NaN is wanted)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    ok = got.dtype == want.dtype and got.shape == want.shape
    n = -1
    if ok:
        nan = torch.isnan(want) if want.is_floating_point() else torch.zeros(want.shape, dtype=torch.bool)
        diff = torch.where(nan, ~torch.isnan(got), _bits(got) != _bits(want)) if want.is_floating_point() else got != want
        n = int(diff.sum())
    return {"name": name, "rel_l2": 0.0, "max_abs": 0.0, "tol": 0.0, "differing": n, "ok": bool(ok and n == 0)}


def _dirty_pool(shape):
    torch.full(tuple(shape), 7.0, device=DEV, dtype=BF)          # (dirty the allocator's pool: an unwritten gradient row would show)


def _ln_ref64(x, w, b, eps, dy, dres=None):
    """(y, dx, dgamma, dbeta) of R.layer_norm in float64 with autograd; dres: the fork's second path, loss += <x, dres>"""
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True) if w is not None else None
    br = b.double().requires_grad_(True) if b is not None else None
    yr = R.layer_norm(xr, wr, br, eps)
    if dres is None:
        yr.backward(dy.double())
    else:
        torch.autograd.backward([xr * 1.0, yr], [dres.double(), dy.double()])
    dg = wr.grad if wr is not None else None
    if dg is not None:
        # rows of equal elements have x - mean = 0; the float64 oracle leaves ~1e-13 there, and where EVERY row is such a row that
        # noise is all of dgamma.  Below 2^-36 sum_r |dy| (a real entry is ~sqrt(rows)) the reference is zero.
        dg = torch.where(dg.abs() <= 2.0 ** -36 * dy.double().abs().sum(0), torch.zeros_like(dg), dg)
    return yr.detach(), xr.grad, dg, (br.grad if br is not None else None)


def _ln_run(kind, x, w, b, eps, dy, dres, pdt):
    from dreamvla_amd import ops
    xd = x.to(DEV, BF).requires_grad_(True)
    wd = w.to(DEV, pdt).requires_grad_(True) if w is not None else None
    bd = b.to(DEV, pdt).requires_grad_(True) if b is not None else None
    _dirty_pool(x.shape)
    if kind == "plain":
        y = ops.layer_norm(xd, wd, bd, eps)
        _dirty_pool(x.shape)
        y.backward(dy.to(DEV, BF))
    else:
        r, y = ops.layer_norm_fork(xd, wd, bd, eps)
        _dirty_pool(x.shape)
        if dres is None:
            y.backward(dy.to(DEV, BF))
        else:
            torch.autograd.backward([r, y], [dres.to(DEV, BF), dy.to(DEV, BF)])
    return y.detach(), xd.grad, (wd.grad if wd is not None else None), (bd.grad if bd is not None else None)


def ln_case_path(case):
    from tests import rowwise_cases as RC
    f, b = RC.ln_geometry(case["rows"], case["cols"]), RC.ln_geometry(case["rows"], case["cols"], backward=True)
    return (f"fwd {f['blocks']} blocks x {f['trips']} trips (last {f['last_trip_rows']} rows), bwd {b['blocks']} x {b['trips']} "
            f"(last {b['last_trip_rows']}), VPL {f['vpl']}, {f['last_slot_lanes']} lanes in the last slot")


def check_layernorm_paths(case, seed=0):
    """one row of tests.rowwise_cases.LN_CASES: ops.layer_norm / ops.layer_norm_fork against the float64 oracle, row by row"""
    from dreamvla_amd import ops
    from tests import rowwise_cases as RC
    rows, cols, eps, kind = case["rows"], case["cols"], case["eps"], case["kind"]
    x, _ = RC.make_rows(case["data"], rows, cols, 1000 + seed, eps)
    w, b = RC.ln_params(cols, seed, case["affine"])
    dy = RC.grad_like((rows, cols), seed)
    dres = RC.grad_like((rows, cols), seed + 1) if kind == "fork" else None
    pdt = torch.float32 if case["pf32"] else BF
    kappa = RC.row_kappa(x, eps)[0]
    y, dx, dg, db = _ln_run(kind, x, w, b, eps, dy, dres, pdt)
    yr, dxr, dgr, dbr = _ln_ref64(x, w, b, eps, dy, dres)
    tag = f"ln-paths {case['id']}"
    out = [rowwise(tag + " y", y, yr, kappa), rowwise(tag + " dx", dx, dxr, kappa)]
    if case["affine"]:
        assert dg.dtype == pdt and db.dtype == pdt
        out.append(metrics(tag + " dgamma", dg, dgr.float(), TOL_GRAD, round_ref=not case["pf32"]))
        out.append(metrics(tag + " dbeta", db, dbr.float(), TOL_GRAD, round_ref=not case["pf32"]))
    if case["data"] == "unit":          # the suite's two criteria on the suite's kind of data, at unchanged tolerances
        out.append(metrics(tag + " y (rel-L2)", y, yr.float(), TOL_FWD))
        out.append(metrics(tag + " dx (rel-L2)", dx, dxr.float(), TOL_GRAD))
    if kind == "fork":                  # no residual gradient arrives: the plain LayerNorm's numbers, bit for bit
        y1, dx1, dg1, db1 = _ln_run("fork", x, w, b, eps, dy, None, pdt)
        y2, dx2, dg2, db2 = _ln_run("plain", x, w, b, eps, dy, None, pdt)
        out += [same_bits(tag + " y == plain (dres None)", y1, y2), same_bits(tag + " dx == plain (dres None)", dx1, dx2)]
        if case["affine"]:
            out += [same_bits(tag + " dgamma == plain (dres None)", dg1, dg2), same_bits(tag + " dbeta == plain (dres None)", db1, db2)]
    if case["stats"]:
        xd = x.to(DEV, BF)
        ys, mean, rstd = ops.layernorm_fwd(xd, w.to(DEV, pdt), b.to(DEV, pdt), eps, True)
        _, m64, r64, _ = RC.row_kappa(x, eps)
        q = cols * 2.0 ** -24 * x.double().abs().mean(-1)             # recursive summation: cols * u * mean |x_i|
        dm = (mean.double().cpu() - m64).abs()
        dr = (rstd.double().cpu() - r64).abs() / r64
        allow_r = q * r64 + 2.0 ** -22                                 # q over the row's (regularised) std, plus rsqrtf
        fin = bool(torch.isfinite(mean).all() and torch.isfinite(rstd).all())
        out.append({"name": tag + " mean", "rel_l2": rel_l2(mean, m64), "max_abs": float(dm.max()), "allow_frac": float((dm / q).max()),
                    "tol": 2.0 ** -24, "finite": fin, "ok": bool(fin and (dm <= q).all())})
        out.append({"name": tag + " rstd", "rel_l2": rel_l2(rstd, r64), "max_abs": float(dr.max()), "allow_frac": float((dr / allow_r).max()),
                    "tol": 2.0 ** -22, "finite": fin, "ok": bool(fin and (dr <= allow_r).all())})
        out.append(same_bits(tag + " y of layernorm_fwd(want_stats) == y of layer_norm", ys, y))
    return out


def check_layernorm_last_tokens_paths(case, seed=0):
    """one row of LAST_TOKENS_CASES: the row groups iterate (the zero-fill of the rows outside the groups on later trips); mixed rows"""
    from dreamvla_amd import ops
    from tests import rowwise_cases as RC
    n, L, keep, cols, eps = case["n"], case["L"], case["keep"], case["cols"], 1e-5
    x2, _ = RC.make_rows("mixed", n * L, cols, 2000 + seed, eps)
    x = x2.view(n, L, cols)
    w, b = RC.ln_params(cols, seed)
    dy = RC.grad_like((n * keep, cols), seed)
    kappa = RC.row_kappa(x2, eps)[0]
    k_kept = kappa.view(n, L)[:, L - keep:].reshape(-1)

    def run(two_step):
        xd = x.to(DEV, BF).requires_grad_(True)
        wd, bd = w.to(DEV, BF).requires_grad_(True), b.to(DEV, BF).requires_grad_(True)
        _dirty_pool(x.shape)
        y = ops.layer_norm(xd[:, L - keep:, :].reshape(-1, cols), wd, bd, eps) if two_step else ops.layer_norm_last_tokens(xd, wd, bd, eps, keep)
        _dirty_pool(x.shape)
        y.backward(dy.to(DEV, BF))
        return y.detach(), xd.grad, wd.grad, bd.grad
    y, dx, dg, db = run(False)
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = R.layer_norm(xr[:, L - keep:, :].reshape(-1, cols), wr, br, eps)
    yr.backward(dy.double())
    tag = f"ln-paths {case['id']}"
    lead = dx[:, :L - keep, :]
    out = [rowwise(tag + " y", y, yr.detach(), k_kept), rowwise(tag + " dx (whole buffer)", dx, xr.grad.view(n * L, cols), kappa),
           {"name": tag + " leading tokens get exact zeros", "ok": bool((lead == 0).all()) if lead.numel() else True, "rel_l2": 0.0,
            "max_abs": float(lead.float().abs().max()) if lead.numel() else 0.0, "tol": 0.0},
           metrics(tag + " dgamma", dg, wr.grad.float(), TOL_GRAD), metrics(tag + " dbeta", db, br.grad.float(), TOL_GRAD)]
    y2, dx2, dg2, db2 = run(True)
    out += [same_bits(tag + " y == LayerNorm(copy of the slice)", y, y2), same_bits(tag + " dx == the two-step path", dx, dx2),
            same_bits(tag + " dgamma == the two-step path", dg, dg2), same_bits(tag + " dbeta == the two-step path", db, db2)]
    return out


def check_layernorm_concat_paths(case, seed=0):
    """one row of CONCAT_CASES: both launches with map_output, mixed rows, one side without input gradient"""
    from dreamvla_amd import ops
    from tests import rowwise_cases as RC
    n, La, Lb, cols, eps, a_grad = case["n"], case["La"], case["Lb"], case["cols"], 1e-5, case["a_needs_grad"]
    a2, _ = RC.make_rows("mixed", n * La, cols, 3000 + seed, eps)
    b2, _ = RC.make_rows("mixed", n * Lb, cols, 3001 + seed, eps)
    a, b = a2.view(n, La, cols), b2.view(n, Lb, cols)
    (wa, ba), (wb, bb) = RC.ln_params(cols, seed), RC.ln_params(cols, seed + 1)
    dy = RC.grad_like((n, La + Lb, cols), seed)
    ka, kb = RC.row_kappa(a2, eps)[0], RC.row_kappa(b2, eps)[0]
    k_all = torch.cat((ka.view(n, La), kb.view(n, Lb)), 1).reshape(-1)

    def run(aten):
        dev = lambda t, grad=True: t.to(DEV, BF).requires_grad_(grad)
        ad, bd, p = dev(a, a_grad), dev(b), [dev(t) for t in (wa, ba, wb, bb)]
        _dirty_pool(dy.shape)
        if aten:
            y = torch.cat((ops.layer_norm(ad, p[0], p[1], eps), ops.layer_norm(bd, p[2], p[3], eps)), dim=1)
        else:
            y = ops.layer_norm_concat(ad, p[0], p[1], eps, bd, p[2], p[3], eps)
        _dirty_pool(a.shape)
        y.backward(dy.to(DEV, BF))
        return y.detach(), ad.grad, bd.grad, [t.grad for t in p]
    y, da, db_in, pg = run(False)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (wa, ba, wb, bb)]
    yr = torch.cat((R.layer_norm(ar, pr[0], pr[1], eps), R.layer_norm(br, pr[2], pr[3], eps)), dim=1)
    yr.backward(dy.double())
    tag = f"ln-paths {case['id']}"
    out = [rowwise(tag + " y", y, yr.detach().view(-1, cols), k_all), rowwise(tag + " db_in", db_in, br.grad.view(-1, cols), kb)]
    out += [metrics(tag + f" {nm}", g, r.grad.float(), TOL_GRAD) for nm, g, r in zip(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"), pg, pr)]
    if a_grad:
        out.append(rowwise(tag + " da_in", da, ar.grad.view(-1, cols), ka))
    else:
        out.append({"name": tag + " no gradient for a", "ok": da is None, "rel_l2": 0.0, "max_abs": 0.0, "tol": 0.0})
    y2, da2, db2, pg2 = run(True)
    out += [same_bits(tag + " y == cat of two LayerNorms", y, y2), same_bits(tag + " db_in == ATen form", db_in, db2)]
    out += [same_bits(tag + f" {nm} == ATen form", g, g2) for nm, g, g2 in zip(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"), pg, pg2)]
    if a_grad:
        out.append(same_bits(tag + " da_in == ATen form", da, da2))
    return out


def finish_case(case_id, path, results):
    """one row per case to $DVLA_PARITY_REPORT (worst rel-L2, worst element, slack used, the path the geometry says ran), every
    metric printed, then the assertion"""
    from tests.model_checks import report
    sig = lambda v: float("%.4g" % v)
    worst = max(results, key=lambda m: m.get("max_abs", 0.0))
    row = {"case": case_id, "ok": all(m["ok"] for m in results), "checks": len(results), "rel_l2": sig(max(m.get("rel_l2", 0.0) for m in results)),
           "max_abs": sig(worst.get("max_abs", 0.0)), "worst": worst["name"], "worst_index": worst.get("worst_index"),
           "slack": sig(max(m.get("slack", 0.0) for m in results)), "allow_frac": sig(max(m.get("allow_frac", 0.0) for m in results)),
           "path": path}
    report([row])
    for m in results:
        print(("ok   " if m["ok"] else "FAIL ") + m["name"], {k: (sig(v) if isinstance(v, float) else v) for k, v in m.items()
                                                               if k in ("rel_l2", "max_abs", "slack", "allow_frac", "allow_frac_row", "bad_rows",
                                                                        "first_bad_row", "bad", "differing", "worst_index")})
    bad = [m for m in results if not m["ok"]]
    assert not bad, "; ".join(f"{m['name']}: " + ", ".join(f"{k}={m[k]}" for k in ("rel_l2", "max_abs", "slack", "allow_frac", "bad_rows",
                                                                                  "first_bad_row", "bad", "differing", "worst_index") if k in m)
                              for m in bad)
