"""GPU: the element-wise kernels of csrc/elementwise.hip on the paths no other test runs (tests/rowwise_cases.py lists them and
tests/test_rowwise_cases.py proves that each case reaches its path): the second grid-stride trip of every kernel, odd element
counts under dropout's two-elements-per-thread loop, the scalar branch / slab cap / short slabs / row-strided views of the column
sums -- and the values: every activation on EVERY bf16 input of its domain against the float64 oracle, element by element
(tests.gpu_checks.elementwise), the casts bit for bit on every rounding tie, dropout against the hash oracle.

The activations' domain is |x| <= 2^40 (x^3 finite in fp32).  One row per case goes to $DVLA_PARITY_REPORT
(profiles/r16_parity_rowwise.jsonl).

Measured on an MI355X: 71 rows, all ok.  Largest error the rounding term does not cover, in units of max(1, |x|): forward 9.5e-8
(silu; tanh 8.9e-8, gelu_erf 1.4e-8), backward 6.7e-8 (gelu_erf) -- a tenth of the 2^-20 allowed; every bit-for-bit row has 0
differing elements.  The file runs in about 3 s."""
import pytest
import torch

from oracle import torch_ref as R
from tests import gpu_checks as G
from tests import rowwise_cases as RC
from tests.gpu_checks import BF, DEV, TOL_F32, TOL_FWD

pytestmark = pytest.mark.gpu

SEED = (123, 456)


def _act_code(name):
    from dreamvla_amd._lib import ACT
    return ACT[name]


def _p32(p):
    """the probability as the C ABI's float carries it (the keep threshold is floor(p * 2^32) of THAT number)"""
    return float(torch.tensor(p, dtype=torch.float32))


_ACT = {}


def _act_ref(name):
    """(x bf16, act(x) and act'(x) in float64) on the whole input set; computed once per activation"""
    if name not in _ACT:
        x = RC.act_inputs()
        x64 = x.double().requires_grad_(True)
        y = R.act(x64, name)
        (d,) = torch.autograd.grad(y, x64, torch.ones_like(y))
        _ACT[name] = (x, y.detach(), d.detach())
    return _ACT[name]


def _xscale(x):
    return x.double().abs().clamp(min=1.0)


@pytest.mark.parametrize("act", RC.ACTS)
def test_activation_forward_on_every_input(act):
    from dreamvla_amd import ops
    x, y64, _ = _act_ref(act)
    y = ops.act_fwd_raw(x.to(DEV), _act_code(act))
    res = [G.elementwise(f"act {act} fwd, all {x.numel()} inputs", y, y64, _xscale(x))]
    tiled = ops.act_fwd_raw(x.repeat(RC.ACT_TILE).to(DEV), _act_code(act))
    res.append(G.same_bits(f"act {act} fwd x{RC.ACT_TILE} (second grid-stride trip) == tiling of the one-trip result", tiled, y.repeat(RC.ACT_TILE)))
    G.finish_case(f"act-fwd-{act}", f"{RC.ew_geometry(x.numel() * RC.ACT_TILE)['trips']} trips when tiled", res)


@pytest.mark.parametrize("dy_kind", ["ones", "seeded"])
@pytest.mark.parametrize("act", RC.ACTS)
def test_activation_backward_on_every_input(act, dy_kind):
    from dreamvla_amd import ops
    x, _, d64 = _act_ref(act)
    shape = (2, x.numel() // 2)
    dy = torch.ones(shape) if dy_kind == "ones" else RC.grad_like(shape, 11)
    dz = ops.act_bwd_raw(dy.to(DEV, BF), x.view(shape).to(DEV), _act_code(act))
    ref = dy.double() * d64.view(shape)
    res = [G.elementwise(f"act {act} bwd dy={dy_kind}", dz, ref, dy.double().abs() * _xscale(x).view(shape))]
    G.finish_case(f"act-bwd-{act}-{dy_kind}", "one trip", res)


def test_cast_f32_to_bf16_rounds_every_tie_to_even():
    from dreamvla_amd import ops
    x = RC.cast_f2b_inputs().repeat(RC.CAST_F2B_TILE)
    got = ops.cast_to(x.to(DEV), BF)
    G.finish_case("cast-f32-bf16", f"{x.numel()} elements, {RC.ew_geometry(x.numel())['trips']} trips",
                  [G.same_bits("cast f32->bf16 == torch's cast, bit for bit (ties, subnormals, inf, FLT_MAX, NaN)", got, x.to(BF))])


def test_cast_bf16_to_f32_on_every_pattern():
    from dreamvla_amd import ops
    x = RC.cast_b2f_inputs().repeat(RC.CAST_B2F_TILE)
    got = ops.cast_to(x.to(DEV), torch.float32)
    G.finish_case("cast-bf16-f32", f"{x.numel()} elements, {RC.ew_geometry(x.numel())['trips']} trips",
                  [G.same_bits("cast bf16->f32 == torch's cast, all 65536 patterns", got, x.float())])


def _nonzero(t):
    return torch.where(t == 0, torch.ones_like(t), t)


def _keep(rows, cols, p):
    return R.drop_keep_mask(SEED, torch.arange(rows, dtype=torch.int64)[:, None], torch.arange(cols, dtype=torch.int64)[None, :], _p32(p))


@pytest.mark.parametrize("case", RC.DROPOUT_CASES, ids=lambda c: f"{c['rows']}x{c['cols']}-p{c['p']}")
def test_dropout_against_the_hash_oracle(case):
    from dreamvla_amd import ops
    rows, cols, p = case["rows"], case["cols"], case["p"]
    x = _nonzero(RC.grad_like((rows, cols), 21))
    xd = x.to(DEV, BF)
    G._dirty_pool((rows, cols))
    y = ops.dropout_raw(xd, p, SEED)
    keep = _keep(rows, cols, p)
    assert bool(keep[-1, -1])           # the lone last element is a kept one
    ref = torch.where(keep, x.double() / (1.0 - _p32(p)), torch.zeros((), dtype=torch.float64))
    n_diff = int(((y.cpu() != 0) != keep).sum())
    res = [{"name": f"dropout {rows}x{cols} p{p} zero pattern == drop_keep_mask", "rel_l2": 0.0, "max_abs": float(n_diff), "tol": 0.0, "ok": n_diff == 0},
           G.elementwise(f"dropout {rows}x{cols} p{p} kept values", y, ref, _xscale(x))]
    g = RC.ew_geometry(rows * cols, 2)
    G.finish_case(f"dropout-{rows}x{cols}-p{p}", f"{rows * cols} elements (odd), {g['trips']} trips", res)


@pytest.mark.parametrize("case", RC.ACT_BWD_DROP_CASES, ids=lambda c: f"{c['rows']}x{c['cols']}-p{c['p']}-{c['act']}")
def test_activation_backward_with_dropout_against_the_hash_oracle(case):
    from dreamvla_amd import ops
    rows, cols, p, act = case["rows"], case["cols"], case["p"], case["act"]
    dy = _nonzero(RC.grad_like((rows, cols), 31))
    pre = RC.grad_like((rows, cols), 32, 2.0) if act != "none" else None
    dz = ops.act_bwd_raw(dy.to(DEV, BF), pre.to(DEV, BF) if pre is not None else None, _act_code(act), p, SEED)
    keep = _keep(rows, cols, p)
    ref = torch.where(keep, dy.double() / (1.0 - _p32(p)), torch.zeros((), dtype=torch.float64))
    scale = dy.double().abs()
    if pre is not None:
        p64 = pre.double().requires_grad_(True)
        (d,) = torch.autograd.grad(R.act(p64, act).sum(), p64)
        ref, scale = ref * d, scale * _xscale(pre)
    n_diff = int(((dz.cpu() != 0) != keep).sum())
    res = [{"name": f"act_bwd {rows}x{cols} {act} p{p} zero pattern == drop_keep_mask", "rel_l2": 0.0, "max_abs": float(n_diff), "tol": 0.0,
            "ok": n_diff == 0},
           G.elementwise(f"act_bwd {rows}x{cols} {act} p{p} kept values", dz, ref, scale)]
    if cols % 8 != 0:       # the fused form declines this shape; the caller's fall-back is the kernel just checked
        res.append({"name": "act_bwd_colsum declines", "rel_l2": 0.0, "max_abs": 0.0, "tol": 0.0,
                    "ok": ops.act_bwd_colsum(dy.to(DEV, BF), pre.to(DEV, BF) if pre is not None else None, _act_code(act), p, SEED, torch.float32) is None})
    G.finish_case(f"act-bwd-drop-{rows}x{cols}-{act}-p{p}", f"{RC.ew_geometry(rows * cols)['trips']} trips", res)


@pytest.mark.parametrize("case", RC.ADD_CASES, ids=lambda c: f"{c['n']}-period{c['period']}")
def test_add_with_a_periodic_operand(case):
    from dreamvla_amd import ops
    n, period = case["n"], case["period"]
    a, b = RC.grad_like((n,), 41, 3.0), RC.grad_like((period or n,), 42)
    got = ops.add_raw(a.to(DEV, BF), b.to(DEV, BF), period)
    b_full = b[torch.arange(n) % period] if period else b
    G.finish_case(f"add-{n}-period{period}", f"{RC.ew_geometry(n)['trips']} trips",
                  [G.same_bits(f"add {n} period {period} == (a + b[i % period]) rounded once", got, (a + b_full).to(BF))])


# ---------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------
def _colsum_data(rows, cols):
    return RC.grad_like((rows, cols), 51 + rows + cols)


def _colsum_operand(case, x):
    """-> (backing or None, the operand on the device)"""
    if case["pad"] is None:
        return None, x.to(DEV, BF)
    backing, view = G.make_view(case["rows"], case["cols"], pad=case["pad"], offset=case["offset"], device=DEV)
    view.copy_(x.to(DEV, BF))
    assert view.stride() == (RC.colsum_case_ld(case), 1) and (view.data_ptr() % 16 == 0) == (case["offset"] % 8 == 0)
    return backing, view


@pytest.mark.parametrize("out_dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", RC.COLSUM_CASES, ids=[c["id"] for c in RC.COLSUM_CASES])
def test_colsum_against_float64_sums(case, out_dtype):
    from dreamvla_amd import ops
    x = _colsum_data(case["rows"], case["cols"])
    backing, operand = _colsum_operand(case, x)
    before = backing.clone() if backing is not None else None
    got = ops.colsum(operand, out_dtype)
    want = x.double().sum(0)
    tag = f"colsum {case['id']} {'bf16' if out_dtype == BF else 'f32'} out"
    res = [G.metrics(tag, got, want, TOL_FWD) if out_dtype == BF else G.metrics(tag, got, want, TOL_F32 * 10, round_ref=False)]
    if backing is not None:       # the backing store is only read: the window unchanged, the sentinel around it intact
        w = G.outside_window_intact(backing, operand)
        res.append({"name": tag + ": backing store untouched", "rel_l2": 0.0, "max_abs": float(w["bad"]), "tol": 0.0,
                    "ok": w["ok"] and bool(torch.equal(G._bits(backing), G._bits(before)))})
    g = RC.colsum_case_geometry(case)
    G.finish_case(f"colsum-{case['id']}-{'bf16' if out_dtype == BF else 'f32'}",
                  f"{g['strips']} strips x {g['slabs']} slabs, vec_ok {int(g['vec_ok'])}, {g['scalar_lanes']} scalar lanes", res)


@pytest.mark.parametrize("rows,cols", [(50, 36), (300, 1001)])
def test_colsum_scalar_and_vector_branches_agree_bit_for_bit(rows, cols):
    from dreamvla_amd import ops
    cases = [c for c in RC.COLSUM_CASES if (c["rows"], c["cols"]) == (rows, cols)]
    assert {RC.colsum_case_geometry(c)["vec_ok"] for c in cases} == {True, False} and len(cases) == 4
    x = _colsum_data(rows, cols)
    outs = {c["id"]: ops.colsum(_colsum_operand(c, x)[1]).cpu() for c in cases}
    first = outs[cases[0]["id"]]
    G.finish_case(f"colsum-branches-{rows}x{cols}", "contiguous, aligned view, shifted view, odd leading dimension",
                  [G.same_bits(f"colsum {k} == {cases[0]['id']}", v, first) for k, v in outs.items()])


def test_colsum_refuses_a_view_whose_columns_are_not_adjacent():
    """dvla_colsum_dt takes one leading dimension: a column stride other than 1 cannot be expressed, and no caller has one"""
    from dreamvla_amd import ops
    x = RC.grad_like((24, 40), 61).to(DEV, BF)
    with pytest.raises(ValueError, match="stride"):
        ops.colsum(x.t())
    with pytest.raises(ValueError, match="stride"):
        ops.colsum(x[:, ::2])
    got = ops.colsum(x[::2])            # a row stride is fine
    assert G.metrics("colsum of every second row", got, x[::2].double().sum(0).cpu(), TOL_F32 * 10, round_ref=False)["ok"]


@pytest.mark.parametrize("act,p", [("none", 0.0), ("gelu_tanh", 0.1)])
@pytest.mark.parametrize("out_dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", RC.ACT_BWD_COLSUM_CASES, ids=lambda c: f"{c['rows']}x{c['cols']}")
def test_act_bwd_colsum_at_the_slab_cap(case, out_dtype, act, p):
    from dreamvla_amd import ops
    rows, cols = case["rows"], case["cols"]
    dy = _nonzero(RC.grad_like((rows, cols), 71))
    pre = RC.grad_like((rows, cols), 72, 2.0) if act != "none" else None
    dyd, pred = dy.to(DEV, BF), (pre.to(DEV, BF) if pre is not None else None)
    dz, db = ops.act_bwd_colsum(dyd, pred, _act_code(act), p, SEED, out_dtype)
    keep = _keep(rows, cols, p) if p else torch.ones((rows, cols), dtype=torch.bool)
    ref = torch.where(keep, dy.double() / (1.0 - _p32(p)), torch.zeros((), dtype=torch.float64))
    scale = dy.double().abs()
    if pre is not None:
        p64 = pre.double().requires_grad_(True)
        (d,) = torch.autograd.grad(R.act(p64, act).sum(), p64)
        ref, scale = ref * d, scale * _xscale(pre)
    tag = f"act_bwd+colsum {rows}x{cols} {act} p{p} {'bf16' if out_dtype == BF else 'f32'} out"
    want = dz.double().sum(0).cpu()
    res = [G.elementwise(tag + " dz", dz, ref, scale),
           G.same_bits(tag + " dz == dvla_act_bwd", dz, ops.act_bwd_raw(dyd, pred, _act_code(act), p, SEED)),
           G.metrics(tag + " column sums of the stored dz", db, want, TOL_FWD) if out_dtype == BF
           else G.metrics(tag + " column sums of the stored dz", db, want, 1e-5, round_ref=False)]
    g = RC.colsum_geometry(rows, cols)
    G.finish_case(f"act-bwd-colsum-{rows}x{cols}-{act}-{'bf16' if out_dtype == BF else 'f32'}",
                  f"{g['slabs']} slabs (capped {int(g['capped'])}), {g['rows_per_slab_min']} rows in the shortest", res)
