"""The GEMM library's ADDRESSING (tests/gpu_checks.py check_gemm_views): every tensor of a dvla_gemm_bf16 call a view into a wider,
sentinel-filled buffer with its own leading dimension and origin; the periodic residual (res_rows); the fp32 bias; one operand
at a time misaligned; the stream-K schedules on padded views; the cost model's own choice pinned.  Values against the float64
product of the bf16 operand values through the epilogue oracle (TOL_FWD + elem_ulps for bf16 outputs, TOL_F32 for fp32 ones), the buffers around `out` and the
pre-activation bit-identical to the sentinel, the same bits as a call on contiguous copies whenever the same configuration ran,
and the configuration that ran.

Shapes: the smallest the tiled configurations take with an edge left -- read off ring_ok / phase_ok / skinny_ok (csrc/gemm.hip,
csrc/gemm_skinny.h): N % 64 == 0, whole K-tiles of 64, M >= 256 and N >= 256 (the 256 x 256 tiles), an r-contiguous operand in
whole tiles (M or N = 512); where a layout admits them, M = 300 (ragged against 128 and 256) and N = 320 (ragged against 128
and 256), 2 x 2 to 4 x 4 tiles so that tile origins are computed with ld != width.  The few-rows kernel at M = 120 / 33,
N = 96 / 40.  The stream-K schedules at the smallest shape the suite engages them at (20832 x 1024, K = 192).

Measured on an MI355X: 352 cases, all passing, the file runs in about 6 s; the metrics are in
profiles/r14_parity_gemm_addressing.jsonl ($DVLA_PARITY_REPORT).  The 13 automatic-choice cases added since run in 5 s together."""
import pytest

from tests import gpu_checks as G

LAYOUTS = {"NN": dict(M=300, N=320, K=192), "NT": dict(M=300, N=512, K=192, b_trans=True),
           "TN": dict(M=512, N=320, K=192, a_trans=True), "TT": dict(M=512, N=512, K=128, a_trans=True, b_trans=True)}
FORCED = (2, 4, 6, 7, 8)
EPILOGUES = {
    "plain": dict(),
    "bias-tanh-preact": dict(bias="bf16", act="gelu_tanh", want_preact=True),
    "bias-erf-res": dict(bias="bf16", act="gelu_erf", residual=True),
    "drop-res": dict(dropout_p=0.1, residual=True),
    "dact": dict(dact="gelu_tanh"),
    "f32": dict(out_f32=True),
    "f32-acc": dict(out_f32=True, accumulate=True),
    "splitk-f32": dict(out_f32=True, split_k=2),
    "splitk-epi": dict(bias="bf16", act="gelu_tanh", residual=True, split_k=2),
}
FEW = dict(M=120, N=96, K=192)           # few-rows kernel: 4 x 3 tiles of 32 x 32, ragged M
FEW_RAGGED = dict(M=33, N=40, K=64)      # ... ragged M and N: its element-wise epilogue on the last column tile

CASES = []


def case(name, **kw):
    CASES.append(pytest.param(kw, id=name))


# ---- aligned views: paddings in whole 16-byte vectors, 16-byte aligned origins -> the forced configuration must be what ran
for lname, shape in LAYOUTS.items():
    for v in FORCED + ((11,) if lname == "NN" else ()) + (None,):
        for ename, epi in EPILOGUES.items():
            if v == 11 and epi.get("split_k", 1) > 1:
                continue                      # (skinny_ok: split_k == 1 only)
            case(f"aligned-{lname}-v{v or 0}-{ename}", variant=v, expect=v, **shape, **epi)
for ename in ("plain", "bias-tanh-preact", "bias-erf-res", "drop-res", "dact", "f32"):
    case(f"aligned-few-ragged-v11-{ename}", variant=11, expect=11, **FEW_RAGGED, **EPILOGUES[ename])

# ---- periodic residual: the position table of the ViT patch embedding (row m % res_rows); 50 and 196 divide no tile height, are
# no multiple of 32, and M = 300 is a multiple of neither
for rr in (50, 196):
    for v in FORCED + (11,):
        case(f"periodic-{rr}-v{v}", variant=v, expect=v, bias="bf16", residual=True, res_rows=rr, **LAYOUTS["NN"])
    case(f"periodic-{rr}-v6-splitk-epi", variant=6, expect=6, bias="bf16", act="gelu_erf", residual=True, res_rows=rr, split_k=2, **LAYOUTS["NN"])
    case(f"periodic-{rr}-v4-f32", variant=4, expect=4, residual=True, res_rows=rr, out_f32=True, **LAYOUTS["NN"])
    case(f"periodic-{rr}-v8-drop-erf", variant=8, expect=8, bias="bf16", act="gelu_erf", dropout_p=0.1, residual=True, res_rows=rr, **LAYOUTS["NT"])
case("periodic-50-v11-few", variant=11, expect=11, bias="bf16", residual=True, res_rows=50, **FEW)
case("periodic-50-v0-few", variant=None, expect=11, bias="bf16", act="gelu_tanh", residual=True, res_rows=50, **FEW)
case("periodic-196-v8-table-contiguous", variant=8, expect=8, bias="bf16", residual=True, res_rows=196, views={"res": (0, 0)}, **LAYOUTS["NN"])
case("periodic-196-v2-splitk-epi-TT", variant=2, expect=2, bias="bf16", residual=True, res_rows=196, split_k=2, **LAYOUTS["TT"])

# ---- fp32 bias (`--precision fp32`: fp32 master biases go straight to the epilogues), values that are not bf16-representable
for v in FORCED:
    case(f"bias32-NN-v{v}-tanh-preact", variant=v, expect=v, bias="f32", act="gelu_tanh", want_preact=True, **LAYOUTS["NN"])
    case(f"bias32-NN-v{v}-erf-res", variant=v, expect=v, bias="f32", act="gelu_erf", residual=True, **LAYOUTS["NN"])
    case(f"bias32-NT-v{v}", variant=v, expect=v, bias="f32", **LAYOUTS["NT"])
    case(f"bias32-TT-v{v}-f32", variant=v, expect=v, bias="f32", out_f32=True, **LAYOUTS["TT"])
for name, shape in (("few", FEW), ("few-ragged", FEW_RAGGED)):
    case(f"bias32-{name}-v11", variant=11, expect=11, bias="f32", **shape)
    case(f"bias32-{name}-v11-silu", variant=11, expect=11, bias="f32", act="silu", **shape)
for lname in ("NN", "NT"):
    case(f"bias32-{lname}-v6-splitk-epi", variant=6, expect=6, bias="f32", split_k=2, **LAYOUTS[lname])
    case(f"bias32-{lname}-v6-splitk-epi-tanh-res", variant=6, expect=6, bias="f32", act="gelu_tanh", residual=True, split_k=2, **LAYOUTS[lname])

# ---- one flag at a time: everything aligned but ONE tensor, by a one-element origin offset or a padding that is no whole vector.
# A forced ring / phase configuration must hand the call to the register-staged kernel (2) and be right.
BASE = {"a": dict(bias="bf16", residual=True), "b": dict(bias="bf16", residual=True), "out": dict(bias="bf16", residual=True),
        "res": dict(bias="bf16", residual=True), "bias": dict(bias="bf16", residual=True), "aux": dict(dact="gelu_erf"),
        "preact": dict(bias="bf16", act="gelu_tanh", want_preact=True)}
for v in (4, 7, 8):
    for which, epi in BASE.items():
        for how, mis in (("offset1", lambda p, o: (p, o + 1)), ("pad4", lambda p, o: (p + 4, o))):
            if which == "bias" and how == "pad4":
                continue                      # (a vector has no leading dimension)
            case(f"flag-{which}-{how}-v{v}", variant=v, expect=2, views={which: mis(*G.ALIGNED_VIEWS[which])}, **LAYOUTS["NN"], **epi)
    case(f"flag-out32-offset1-v{v}", variant=v, expect=2, out_f32=True, views={"out": (24, 17)}, **LAYOUTS["NN"])
    case(f"flag-out32-pad2-v{v}", variant=v, expect=2, out_f32=True, views={"out": (26, 16)}, **LAYOUTS["NN"])
    case(f"flag-bias32-offset1-v{v}", variant=v, expect=2, bias="f32", views={"bias": (0, 9)}, **LAYOUTS["NN"])
    case(f"flag-out32-offset1-v{v}-splitk", variant=v, expect=2, out_f32=True, split_k=2, views={"out": (24, 17)}, **LAYOUTS["TT"])
# the few-rows kernel needs A and B vectorisable (else: configuration 2); out / epilogue operands select its element-wise epilogue
for which in ("a", "b"):
    case(f"flag-{which}-offset1-v11", variant=11, expect=2, views={which: (G.ALIGNED_VIEWS[which][0], G.ALIGNED_VIEWS[which][1] + 1)}, bias="bf16", residual=True, **FEW)
for which in ("out", "res", "bias", "aux", "preact"):
    p, o = G.ALIGNED_VIEWS[which]
    case(f"flag-{which}-offset1-v11", variant=11, expect=11, views={which: (p, o + 1)}, **FEW, **BASE[which])
    if which != "bias":
        case(f"flag-{which}-pad4-v11", variant=11, expect=11, views={which: (p + 4, o)}, **FEW_RAGGED, **BASE[which])
case("flag-bias32-offset1-v11", variant=11, expect=11, bias="f32", act="silu", views={"bias": (0, 9)}, **FEW)
# an EXPLICIT split with an epilogue the reduction pass cannot vectorise: DVLA_ERR_UNSUPPORTED before any launch ...
SPLIT_EPI = dict(bias="bf16", act="gelu_tanh", residual=True)
for which, mis in (("bias", (0, 9)), ("res", (44, 8)), ("out", (24, 17))):
    case(f"flag-{which}-explicit-split-unsupported", split_k=2, expect_rc=G.ERR_UNSUPPORTED, views={which: mis}, **LAYOUTS["NN"], **SPLIT_EPI)
    # ... while the opportunistic forward split (a shape ops.fwd_split_k cuts in two) runs unsplit and is right
    case(f"flag-{which}-opportunistic-split-runs-unsplit", via_ops=True, views={which: mis}, M=600, N=256, K=2048, **SPLIT_EPI)

# ---- stream-K (9: hybrid, 10: full) with `out` and the residual as padded views, twice in a row on the same scratch and flags
for v in (9, 10):
    for rep in range(2):
        case(f"streamk-v{v}-run{rep}", variant=v, expect=v, bias="bf16", residual=True, M=20832, N=1024, K=192)

# ---- the library's own choice (variant 0), pinned: what the cost model of csrc/gemm.hip picked on an MI355X (256 CUs) BEFORE its
# dispatch became one table -- recorded from that library, so that a table row out of order, a changed constant or a changed tie
# shows here.  A sweep of that library (M, N in 256 .. 20832 with M x N <= 2^25, K = 64 .. 512, four layouts, plain and
# bias-tanh-preact: 2350 calls) chose 11, 6, 7, 4 and 8 -- every one of them is below, plain and fused -- and never the stream-K
# hybrid 9: up to K = 512 its 18 us never pay for the half round it saves (4096 x 4352 x 512, 17 super-tiles, runs 7).  2 is the
# fallback: a ragged N, a misaligned operand.
FUSED = EPILOGUES["bias-tanh-preact"]
case("auto-few-rows-NN-plain", variant=None, expect=11, **LAYOUTS["NN"])
case("auto-few-rows-NN-fused", variant=None, expect=11, **LAYOUTS["NN"], **FUSED)
case("auto-ring128-NT-plain", variant=None, expect=6, **LAYOUTS["NT"])                                    # one round: short K
case("auto-ring128-TT-fused", variant=None, expect=6, **LAYOUTS["TT"], **FUSED)
case("auto-ring128-three-rounds-NN", variant=None, expect=6, bias="bf16", residual=True, M=20832, N=1024, K=192)
case("auto-ring256x128-NT-plain", variant=None, expect=7, M=300, N=512, K=256, b_trans=True)               # one round: K >= 256
case("auto-ring256x128-TN-fused", variant=None, expect=7, M=512, N=320, K=512, a_trans=True, **FUSED)
case("auto-ring256-NN-plain", variant=None, expect=4, M=2048, N=4352, K=64)                                # 136 tiles of 256^2: one round
case("auto-ring256-TT-fused", variant=None, expect=4, M=2048, N=4352, K=64, a_trans=True, b_trans=True, **FUSED)
case("auto-phase-NN-plain", variant=None, expect=8, M=2048, N=4352, K=512)
case("auto-phase-NT-fused", variant=None, expect=8, M=2048, N=4352, K=512, b_trans=True, **FUSED)
case("auto-fallback-ragged-N-plain", variant=None, expect=2, M=600, N=328, K=192)
case("auto-fallback-misaligned-A-fused", variant=None, expect=2, M=600, N=320, K=192, views={"a": (8, 9)}, **FUSED)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", CASES)
def test_gemm_addressing(kw):
    results = G.check_gemm_views(**kw)
    from tests.model_checks import report
    # one row per case in $DVLA_PARITY_REPORT: the parity metrics of `out` (and of the pre-activation), what ran, whether the
    # result was compared bit for bit with the contiguous call
    par = [m for m in results if "max_abs" in m]
    row = {"name": results[0]["name"].rsplit(":", 1)[0].replace("gemm views ", ""), "ok": all(m["ok"] for m in results)}
    if par:
        row.update({k: par[0][k] for k in ("rel_l2", "max_abs")})
        row.update({"preact_" + k: m[k] for m in par[1:] for k in ("rel_l2", "max_abs")})
    row.update({k: m[k] for m in results for k in ("ran", "compared") if k in m})
    report([{k: float("%.4g" % v) if isinstance(v, float) else v for k, v in row.items()}])
    for m in results:
        print(("ok   " if m["ok"] else "FAIL ") + m["name"], "rel_l2=%.3g max_abs=%s tol=%s" % (m.get("rel_l2", 0.0), m.get("max_abs"), m.get("max_abs_tol")))
    bad = [m for m in results if not m["ok"]]
    assert not bad, "; ".join(f"{m['name']}: rel_l2={m.get('rel_l2')} max_abs={m.get('max_abs')} tol={m.get('tol')}" for m in bad)
