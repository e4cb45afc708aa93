"""GPU: the training-loss kernels (csrc/losses.hip: dvla_patch_mse_* / dvla_cosine_loss_* / dvla_silog_loss_*, forward and
backward) through the C ABI against the float64 reference of tests/loss_ref.py, at the launch shapes of a training step and
on degenerate data.  tests/test_loss_ref.py pins that reference to the real training loop's loss block and shows that the
fp32 ATen formulation sits inside the same budgets with 4x headroom; the budgets themselves are derived in tests/loss_ref.py.

Every case (`_run`):
  * inputs are bf16-representable CPU tensors, so the kernels and the reference see the same numbers;
  * the prediction lives at [:, :T, view, 0] of a (bs, S, 2, 1, rows, cols) buffer whose other elements are NaN, the label at
    [:, off : off + T] of a (bs, window, ...) buffer whose other frames are NaN: reading outside the view poisons the result;
  * `partial` and `out2` are NaN before every forward: a finite result shows that the finaliser read only what was written;
  * the backward writes into a whole buffer of a bf16 NaN sentinel: afterwards every element of the view differs from the
    sentinel and every other element still is the sentinel, bit for bit;
  * forward and backward run twice: scalars and gradients are bit-identical;
  * loss within LOSS_RTOL (x cond for silog) of float64, every gradient element within 2^-8 |ref| + a, rel-L2 within the
    TOL_GRAD of the older checks.

Launch shapes: one patch / row per wave, 4 per workgroup, at most 2 048 workgroups.  n_frames 41 / 42 (x 196 patches) sit just
below / above that cap, 224 frames (bs 32, S 7) are the benchmarked step (5.36 patches per wave), and the T = 6 < S case reads
labels out of a longer window so that stride_b != T * stride_t on every view.  The cosine kernel switches at cols = 256 from
two rows per wave to one; its grid is capped above 8 192 rows and the two-rows-per-wave loop takes a second trip above 16 384.

Measured on an MI355X (profiles/r09_parity_losses.jsonl, written by these tests through tests.model_checks.report), worst case
over the cases of a family as a fraction of the budget:
  loss:      patch_mse 0.005 (randn), 0.002 / 0.0001 / 0.003 / 0.002 (constant_frames / border16 / border24 / one_pixel);
             cosine 0.006 (zero label / prediction rows 0.006); silog 0.004 / 0.006 / 0.003 / 0.002 (plain / zero_pixels /
             pred_range / equal_frame), its mean d 0.002 .. 0.005        -- i.e. relative errors of 1e-9 .. 1.2e-7
  gradient:  0.986 .. 0.994 per element in every family: what the bf16 rounding of the float64 gradient costs by itself
             (0.993); rel-L2 1.66e-3 .. 2.1e-3 against TOL_GRAD = 4e-3
"""
import ctypes as C
import math

import pytest
import torch

from tests import loss_ref as LR
from tests.gpu_checks import BF, DEV, TOL_GRAD

SENTINEL = 0x7FA5                # a bf16 NaN with a payload no computation produces
G = 0.375                        # upstream gradient handed to every backward (exact in fp32)
UNSUPPORTED, ARG = -3, -1


class Layout:
    """n_frames = bs * T frames living in (bs, S, 2, ...) prediction buffers and (bs, window, ...) label buffers"""

    def __init__(self, bs, S=None, T=None, view=0, window=None, off=0):
        self.bs, self.S, self.view = bs, S or 1, view
        self.T = T or self.S
        self.window, self.off = window or self.T, off
        self.n = bs * self.T

    def __repr__(self):
        return f"bs{self.bs}S{self.S}T{self.T}v{self.view}" + (f"w{self.window}+{self.off}" if self.window != self.T else "")


# n_frames -> layout.  7 frames: T < S with one frame per sample; 192: the T = 6 < S case of the 224-frame shape
LAYOUTS = {1: Layout(1, 1, 1, view=1), 7: Layout(7, 2, 1, view=1), 41: Layout(41, 1, 1, view=0), 42: Layout(6, 7, 7, view=1),
           224: Layout(32, 7, 7, view=0), 192: Layout(32, 7, 6, view=1, window=10, off=3)}


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=BF)


def _pred_buffer(vals, lay):
    rows, cols = vals.shape[-2:]
    buf = _nan((lay.bs, lay.S, 2, 1, rows, cols))
    buf[:, :lay.T, lay.view, 0] = vals.reshape(lay.bs, lay.T, rows, cols).to(BF)
    buf = buf.to(DEV)
    return buf, buf[:, :lay.T, lay.view, 0]


def _label_buffer(vals, lay):
    inner = vals.shape[1:]
    buf = _nan((lay.bs, lay.window, *inner))
    buf[:, lay.off:lay.off + lay.T] = vals.reshape(lay.bs, lay.T, *inner).to(BF)
    buf = buf.to(DEV)
    return buf, buf[:, lay.off:lay.off + lay.T]


def _run(kind, lay, pred, label, mask=None, lambd=0.5):
    """both entry points of one family, twice, with the layout / poison / sentinel checks of the module docstring.
    pred (n, rows, cols), label (n, ...) fp32 CPU.  -> dict(loss, aux, grad (n, rows, cols) float64, loss_bits, grad_bits)"""
    from dreamvla_amd import _lib, losses
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n, rows, cols = pred.shape
    assert n == lay.n and label.shape[0] == n
    assert bool((pred.to(BF).float() == pred).all()) and bool((label.to(BF).float() == label).all()), "inputs must be bf16-representable"
    pbuf, pv = _pred_buffer(pred, lay)
    lbuf, lv = _label_buffer(label, lay)
    fp, fl = losses._frame_view(pv), losses._frame_view(lv)
    if lay.T > 1 and lay.window != lay.T:
        assert fp.stride_b != lay.T * fp.stride_t and fl.stride_b != lay.T * fl.stride_t
    mk = None if mask is None else mask.to(DEV, torch.float32).contiguous()
    mp = None if mk is None else mk.data_ptr()
    gout = torch.tensor([G], dtype=torch.float32, device=DEV)
    plen = int(lib.dvla_loss_partial_len())
    runs = []
    for _ in range(2):
        out2 = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
        part = torch.full((plen,), float("nan"), dtype=torch.float32, device=DEV)
        dbuf = torch.full(pbuf.shape, SENTINEL, dtype=torch.int16, device=DEV)
        dv = dbuf.view(BF)[:, :lay.T, lay.view, 0]
        fd = losses._frame_view(dv)
        assert (fd.stride_b, fd.stride_t, fd.T) == (fp.stride_b, fp.stride_t, fp.T)
        if kind == "patch_mse":
            rc = lib.dvla_patch_mse_fwd(C.byref(fp), C.byref(fl), mp, n, out2.data_ptr(), part.data_ptr(), stream)
            rb = lib.dvla_patch_mse_bwd(C.byref(fp), C.byref(fl), mp, n, gout.data_ptr(), C.byref(fd), stream)
        elif kind == "cosine":
            rc = lib.dvla_cosine_loss_fwd(C.byref(fp), C.byref(fl), rows, cols, n, out2.data_ptr(), part.data_ptr(), stream)
            rb = lib.dvla_cosine_loss_bwd(C.byref(fp), C.byref(fl), rows, cols, n, gout.data_ptr(), C.byref(fd), stream)
        else:
            rc = lib.dvla_silog_loss_fwd(C.byref(fp), C.byref(fl), n, float(lambd), out2.data_ptr(), part.data_ptr(), stream)
            rb = lib.dvla_silog_loss_bwd(C.byref(fp), C.byref(fl), n, float(lambd), out2.data_ptr(), gout.data_ptr(), C.byref(fd), stream)
        assert (rc, rb) == (0, 0), (kind, rc, rb)
        torch.cuda.synchronize()
        runs.append((out2.cpu(), dbuf.cpu()))
    (o0, d0), (o1, d1) = runs
    tag = f"{kind} {lay}"
    assert bool(torch.isfinite(o0).all()), f"{tag}: out2 = {o0.tolist()}: the finaliser read a partial this launch did not write"
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)), f"{tag}: forward not deterministic: {o0.tolist()} vs {o1.tolist()}"
    assert torch.equal(d0, d1), f"{tag}: backward not deterministic"
    inside = d0[:, :lay.T, lay.view, 0]
    assert bool((inside != SENTINEL).all()), f"{tag}: {int((inside == SENTINEL).sum())} gradient elements of the view were not written"
    rest = d0.clone()
    rest[:, :lay.T, lay.view, 0] = SENTINEL
    assert bool((rest == SENTINEL).all()), f"{tag}: {int((rest != SENTINEL).sum())} elements outside the view were written"
    grad = inside.contiguous().view(BF).to(LR.F64).reshape(n, rows, cols)
    return dict(loss=float(o0[0]), aux=float(o0[1]), grad=grad, loss_bits=o0.view(torch.int32), grad_bits=inside.contiguous())


def _finish(ms):
    from tests.model_checks import report
    for m in ms:
        print({k: v for k, v in m.items()})
    report(ms)
    for m in ms:
        assert m["ok"], m


def _grad_metrics(tag, got, ref, budget):
    m = LR.grad_metrics(tag, got, ref, budget)
    m["tol_rel_l2"] = TOL_GRAD
    m["ok"] = m["ok"] and m["rel_l2"] <= TOL_GRAD
    return m


# ---------------------------------------------------------------------------------------------------------------------
# patch_mse
# ---------------------------------------------------------------------------------------------------------------------
def _patch_mse_case(family, n, mask_kind, seed=0):
    lay = LAYOUTS[n]
    pred, frames = LR.image_inputs(family, lay.n, seed)
    mask = LR.patch_mask(mask_kind, lay.n, seed)
    got = _run("patch_mse", lay, pred, frames, mask)
    ref, rg = LR.value_and_grad(LR.patch_mse, pred, frames, mask, g=G, chunk=16)
    tag = f"losses_gpu patch_mse {family} n{lay.n} {lay} mask={mask_kind}"
    return got, ref, rg, tag, (pred, frames, mask)


PATCH_CASES = ([("randn", n, None) for n in (1, 7, 41, 42, 224)] + [("randn", 192, "random")]
               + [("randn", n, "random") for n in (7, 42)]
               + [(f, 7, None) for f in LR.IMAGE_FAMILIES[1:]] + [(f, 42, "random") for f in ("constant_frames", "border24", "one_pixel")])


@pytest.mark.gpu
@pytest.mark.parametrize("family,n,mask_kind", PATCH_CASES, ids=[f"{f}-n{n}-{m}" for f, n, m in PATCH_CASES])
def test_patch_mse(family, n, mask_kind):
    got, ref, rg, tag, (pred, frames, mask) = _patch_mse_case(family, n, mask_kind)
    _finish([LR.loss_metrics(tag + " loss", got["loss"], ref, LR.LOSS_RTOL),
             _grad_metrics(tag + " dpred", got["grad"], rg, LR.grad_budget_patch_mse(rg, frames, mask, G))])
    assert got["aux"] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", (7, 42))
def test_patch_mse_all_zero_mask_gives_exact_zeros(n):
    got, ref, rg, tag, _ = _patch_mse_case("border16", n, "zeros")
    assert ref == 0.0 and got["loss"] == 0.0, (tag, got["loss"])
    assert float(got["grad"].abs().max()) == 0.0, tag


@pytest.mark.gpu
@pytest.mark.parametrize("family,n", [("randn", 42), ("border24", 7)])
def test_patch_mse_all_one_mask_is_bit_identical_to_no_mask(family, n):
    a = _patch_mse_case(family, n, None)[0]
    b = _patch_mse_case(family, n, "ones")[0]
    assert torch.equal(a["loss_bits"], b["loss_bits"]) and torch.equal(a["grad_bits"], b["grad_bits"])


# ---------------------------------------------------------------------------------------------------------------------
# cosine
# ---------------------------------------------------------------------------------------------------------------------
COLS = (8, 64, 248, 256, 264, 512, 520, 768, 1024)
# (layout, rows_per_frame, cols).  Scale: 41 / 42 frames x 196 rows = 8 036 / 8 232 rows straddle the 2 048-workgroup cap in both
# regimes and the second trip of the one-row-per-wave loop (cols 768, 264); x 392 rows = 16 072 / 16 464 straddle the second trip of
# the two-rows-per-wave loop (cols 256, 64); 224 frames x 256 rows = 57 344 rows is the benchmarked step; 5 463 frames x 3 rows is an
# odd row count (a dead half-wave in the last pair) beyond the second trip.
COSINE_SCALE = ([(LAYOUTS[n], 196, c) for n in (1, 7, 41, 42) for c in (256, 768)]
                + [(LAYOUTS[n], 392, c) for n in (41, 42) for c in (256, 64)]
                + [(LAYOUTS[n], 196, 264) for n in (41, 42)]
                + [(LAYOUTS[224], 256, 768), (LAYOUTS[192], 256, 256), (Layout(5463, 1, 1, view=1), 3, 64)])
# widths: every cols x rows_per_frame 1 / 3 / 256 at 7 frames (7 and 21 rows: odd totals), and a single row
COSINE_WIDTHS = [(LAYOUTS[7], r, c) for c in COLS for r in (1, 3, 256)] + [(LAYOUTS[1], 1, c) for c in (8, 256, 264, 1024)]


def _cosine_id(case):
    lay, rows, cols = case
    return f"{lay}-r{rows}-c{cols}"


def _cosine_case(lay, rows, cols, family):
    pred, label = LR.cosine_inputs(family, lay.n, rows, cols, seed=cols + rows)
    got = _run("cosine", lay, pred, label)
    ref, rg = LR.value_and_grad(LR.cosine, pred, label, g=G, chunk=32 if lay.n * rows * cols > (1 << 24) else None)
    return got, ref, rg, pred, label, f"losses_gpu cosine {family} n{lay.n} {lay} {rows}x{cols}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", COSINE_SCALE + COSINE_WIDTHS, ids=_cosine_id)
def test_cosine(case):
    got, ref, rg, _, _, tag = _cosine_case(*case, "randn")
    _finish([LR.loss_metrics(tag + " loss", got["loss"], ref, LR.LOSS_RTOL),
             _grad_metrics(tag + " dpred", got["grad"], rg, LR.grad_budget_rows(rg))])
    assert got["aux"] == 0.0


DEGENERATE = [(LAYOUTS[7], 3, 8), (LAYOUTS[7], 3, 256), (LAYOUTS[7], 256, 264), (LAYOUTS[42], 196, 768), (LAYOUTS[42], 392, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEGENERATE, ids=_cosine_id)
def test_cosine_zero_label_rows(case):
    """an all-zero label row: the clamp max(|x|^2 |y|^2, 1e-16) makes its term exactly 1 and its gradient row exactly 0"""
    got, ref, rg, pred, label, tag = _cosine_case(*case, "zero_label_rows")
    zero = label.abs().amax(-1) == 0
    assert int(zero.sum()) >= 2
    assert float(got["grad"][zero].abs().max()) == 0.0, tag
    _finish([LR.loss_metrics(tag + " loss", got["loss"], ref, LR.LOSS_RTOL),
             _grad_metrics(tag + " dpred", got["grad"], rg, LR.grad_budget_rows(rg))])
    lay, rows, cols = case
    if lay.n * rows == 21:          # every label zero: the loss is exactly 1
        all_zero = _run("cosine", lay, pred, torch.zeros_like(label))
        assert all_zero["loss"] == 1.0 and float(all_zero["grad"].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEGENERATE, ids=_cosine_id)
def test_cosine_zero_prediction_rows(case):
    """an all-zero PREDICTION row.  Its loss term is 1 under every reading of the clamp, so the loss is held to the budget.  Its
    gradient has no single reference: the formula the kernel cites, x.y / sqrt(max(|x|^2 |y|^2, eps^2)), has the constant
    denominator eps there, so d/dx = -y / eps (1e8 |y|), which is what the kernel writes; F.cosine_similarity of torch 2.10
    clamps each norm instead, x.y / (max(|x|, eps) max(|y|, eps)), and gives -y / (eps |y|), |y| times smaller.  A trained linear
    head does not emit an exactly zero row.  So for those rows only finiteness of the gradient is asserted; every row with a
    non-zero prediction is checked as usual."""
    got, ref, rg, pred, label, tag = _cosine_case(*case, "zero_pred_rows")
    zero = pred.abs().amax(-1) == 0
    assert int(zero.sum()) >= 2 and math.isfinite(got["loss"])
    assert bool(torch.isfinite(got["grad"]).all()), tag
    keep = ~zero
    _finish([LR.loss_metrics(tag + " loss", got["loss"], ref, LR.LOSS_RTOL),
             _grad_metrics(tag + " dpred (rows with a non-zero prediction)", got["grad"][keep], rg[keep], LR.grad_budget_rows(rg[keep]))])


# ---------------------------------------------------------------------------------------------------------------------
# silog
# ---------------------------------------------------------------------------------------------------------------------
SILOG_CASES = ([("plain", n, 0.5) for n in (1, 7, 41, 42)] + [("plain", 224, 0.85), ("zero_pixels", 192, 0.5)]
               + [(f, 7, lam) for f in LR.DEPTH_FAMILIES for lam in (0.5, 0.85, 1.0) if (f, lam) != ("plain", 0.5)]
               + [("pred_range", 42, 1.0), ("equal_frame", 42, 0.85)])


@pytest.mark.gpu
@pytest.mark.parametrize("family,n,lambd", SILOG_CASES, ids=[f"{f}-n{n}-l{lam}" for f, n, lam in SILOG_CASES])
def test_silog(family, n, lambd):
    lay = LAYOUTS[n]
    pred, depth = LR.depth_inputs(family, lay.n, seed=n)
    cond = LR.silog_cond(pred, depth, lambd)
    assert cond <= LR.COND_MAX, cond
    got = _run("silog", lay, pred, depth, lambd=lambd)
    ref, rg = LR.value_and_grad(LR.silog, pred, depth, lambd, g=G)
    d = LR.silog_terms(pred, depth)
    if family == "equal_frame":
        assert float(d[0].abs().max()) == 0.0
    tag = f"losses_gpu silog {family} n{lay.n} {lay} lambd={lambd}"
    ms = [LR.loss_metrics(tag + " loss", got["loss"], ref, LR.LOSS_RTOL * cond),
          LR.loss_metrics(tag + " mean d", got["aux"], float(d.mean()), LR.LOSS_RTOL * float(d.abs().mean() / d.mean().abs())),
          _grad_metrics(tag + " dpred", got["grad"], rg, LR.grad_budget_rows(rg))]
    ms[0]["cond"] = cond
    _finish(ms)


@pytest.mark.gpu
@pytest.mark.parametrize("lambd", (0.5, 1.0))
def test_silog_backward_of_a_zero_loss_is_zero(lambd):
    """pred == depth on every pixel: every d is exactly 0, so loss = mean d = 0 exactly.  The analytic gradient is 0 / 0; the
    backward divides by max(loss, 1e-20) and multiplies by (d - lambd mean d) = 0, so the expected result is a finite, exactly
    zero gradient (a step that changes nothing), not NaN or inf."""
    lay = LAYOUTS[7]
    _, depth = LR.depth_inputs("plain", lay.n)
    pred = LR.depth_patches_of(depth.reshape(-1, 224, 224)).clone()
    got = _run("silog", lay, pred, depth, lambd=lambd)
    assert got["loss"] == 0.0 and got["aux"] == 0.0
    assert bool(torch.isfinite(got["grad"]).all()) and float(got["grad"].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# refusals: every one of these returns before any launch
# ---------------------------------------------------------------------------------------------------------------------
def _refusal_setup(rows=4, cols=64, n=2):
    from dreamvla_amd import _lib
    lib = _lib.load()
    buf = lambda: torch.zeros(n * rows * cols + 64, dtype=BF, device=DEV)
    t = dict(pred=buf(), label=buf(), dpred=buf(), out2=torch.zeros(2, device=DEV), gout=torch.ones(1, device=DEV),
             part=torch.zeros(int(lib.dvla_loss_partial_len()), device=DEV))
    fv = lambda x, off=0, sb=rows * cols, st=rows * cols: _lib.FrameView(x.data_ptr() + 2 * off, sb, st, 1)
    return lib, t, fv, torch.cuda.current_stream().cuda_stream


def _cosine_calls(lib, t, stream, fp, fl, fd, rows, cols, n, out2=True):
    o = t["out2"].data_ptr() if out2 else None
    return (lib.dvla_cosine_loss_fwd(C.byref(fp), C.byref(fl), rows, cols, n, o, t["part"].data_ptr(), stream),
            lib.dvla_cosine_loss_bwd(C.byref(fp), C.byref(fl), rows, cols, n, t["gout"].data_ptr(), C.byref(fd), stream))


@pytest.mark.gpu
@pytest.mark.parametrize("cols", (12, 1032, 0))
def test_cosine_refuses_unsupported_widths(cols):
    lib, t, fv, stream = _refusal_setup()
    assert _cosine_calls(lib, t, stream, fv(t["pred"]), fv(t["label"]), fv(t["dpred"]), 4, cols, 2) == (UNSUPPORTED, UNSUPPORTED)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("pred", "label", "dpred"))
@pytest.mark.parametrize("how", ("base", "stride_b", "stride_t"))
def test_cosine_refuses_views_that_are_not_16_byte_aligned(which, how):
    """rows are read and written as 16-byte vectors: a base that is not 16-byte aligned or a stride that is not a multiple of
    8 elements is DVLA_ERR_UNSUPPORTED from both entry points (the forward does not look at dpred)"""
    lib, t, fv, stream = _refusal_setup()
    bad = dict(base=dict(off=1), stride_b=dict(sb=4 * 64 + 4), stride_t=dict(st=4 * 64 + 12))[how]
    views = {k: fv(t[k], **(bad if k == which else {})) for k in ("pred", "label", "dpred")}
    rc = _cosine_calls(lib, t, stream, views["pred"], views["label"], views["dpred"], 4, 64, 2)
    assert rc == ((0, UNSUPPORTED) if which == "dpred" else (UNSUPPORTED, UNSUPPORTED))
    torch.cuda.synchronize()
    assert _cosine_calls(lib, t, stream, fv(t["pred"]), fv(t["label"]), fv(t["dpred"]), 4, 64, 2) == (0, 0)      # the aligned twin runs
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ("n_frames", "base", "out2"))
def test_loss_entry_points_refuse_bad_arguments(what):
    """n_frames = 0, a null base, a null out2 -> DVLA_ERR_ARG from every entry point that takes the argument"""
    from dreamvla_amd import _lib
    lib, t, _, stream = _refusal_setup(rows=196, cols=768, n=1)
    img = torch.zeros(3 * 224 * 224, dtype=BF, device=DEV)
    n = 0 if what == "n_frames" else 1
    null = what == "base"
    fv = lambda x, inner: _lib.FrameView(None if null else x.data_ptr(), inner, inner, 1)
    o = None if what == "out2" else t["out2"].data_ptr()
    p, g = t["part"].data_ptr(), t["gout"].data_ptr()
    fp, fd, fi = fv(t["pred"], 196 * 768), fv(t["dpred"], 196 * 768), fv(img, 3 * 224 * 224)
    rcs = [lib.dvla_patch_mse_fwd(C.byref(fp), C.byref(fi), None, n, o, p, stream),
           lib.dvla_cosine_loss_fwd(C.byref(fp), C.byref(fp), 196, 768, n, o, p, stream),
           lib.dvla_silog_loss_fwd(C.byref(fp), C.byref(fi), n, 0.5, o, p, stream),
           lib.dvla_silog_loss_bwd(C.byref(fp), C.byref(fi), n, 0.5, o, g, C.byref(fd), stream)]
    if what != "out2":
        rcs += [lib.dvla_patch_mse_bwd(C.byref(fp), C.byref(fi), None, n, g, C.byref(fd), stream),
                lib.dvla_cosine_loss_bwd(C.byref(fp), C.byref(fp), 196, 768, n, g, C.byref(fd), stream)]
    assert rcs == [ARG] * len(rcs), rcs
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_cos_loss_takes_the_aten_path_for_misaligned_labels():
    """losses.calvin_losses with feature labels that start 2 bytes off a 16-byte boundary: fused=None computes the ATen
    formulation (bit-identical to fused=False) instead of handing the view to the kernel, fused=True raises"""
    from dreamvla_amd import losses
    bs, S, rows, cols = 2, 3, 256, 64
    W = S + 3
    g = torch.Generator().manual_seed(5)
    n = bs * W * rows * cols
    raw = {k: torch.randn(n + 8, generator=g).to(DEV, BF) for k in ("dino_primary", "dino_wrist")}
    batch = {k: v[1:1 + n].view(bs, W, rows, cols) for k, v in raw.items()}
    assert all(v.data_ptr() % 16 == 2 for v in batch.values())
    batch["image_primary"] = torch.zeros(bs, W, 1, device=DEV)
    pred = torch.randn(bs * S, 2, 1, rows, cols, generator=g).to(DEV, BF)
    arm = torch.zeros((), device=DEV)
    out = (arm, arm, None, None, None, None, None, None, pred, None)
    res = {f: losses.calvin_losses(out, batch, sequence_length=S, fused=f)[1]["dino"] for f in (None, False)}
    assert torch.equal(res[None], res[False])
    with pytest.raises(TypeError):
        losses.calvin_losses(out, batch, sequence_length=S, fused=True)
    aligned = {k: v[0:n].view(bs, W, rows, cols) for k, v in raw.items()}
    aligned["image_primary"] = batch["image_primary"]
    fused = losses.calvin_losses(out, aligned, sequence_length=S, fused=True)[1]["dino"]
    want = losses.calvin_losses(out, aligned, sequence_length=S, fused=False)[1]["dino"]
    assert abs(float(fused) - float(want)) <= LR.LOSS_RTOL * abs(float(want))
