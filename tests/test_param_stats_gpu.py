"""GPU: FlatAdamW.parameter_stats() -- dvla_segment_stats_* / dvla_segment_adam_* -- against the float64 restatement of
tests/param_stats_ref.py.

The real GradBucketReducer over hand-made parameter lists: it pads every parameter to 128 elements, so there are alignment gaps,
and a small bucket_bytes cuts the list into three or more buckets.  The sizes are those at which the kernels take another path:
empty, below / at / above one 16-byte vector (ragged ends of 1 and 7 elements), around the reducer's padding, and around one
chunk (STATS_CHUNK - 1, STATS_CHUNK, STATS_CHUNK + 1: a second chunk of one element) and several chunks with a ragged end.
Parameter NO_GRAD never receives a gradient: the step leaves it alone.  Data is of mixed scale, 1e-3 .. 1e3 per parameter.

Tolerances (u = 2^-24, the unit roundoff of fp32; every term of the sums is non-negative, so relative errors add and do not
amplify).  The sum of squares as built: a thread adds at most STATS_CHUNK / 256 elements of its chunk, one fmaf each (the square
is not rounded on its own), + 1 for the thread that also takes an element of the ragged end; six adds of the wave reduction; two
levels of adds over the four waves; stage 2 adds the chunks in double (2^-53 each: nothing); one rounding to fp32.  That is
(STATS_CHUNK / 256 + 1 + 6 + 2 + 1) u = (STATS_CHUNK / 256 + 10) u on the SUM, to first order.  A norm has half the relative error
of its sum plus the roundings of the square root and of the host's scaling (3 u at most), so the bound on the sum, taken as the
tolerance on the NORM, leaves a factor of two that covers those and the second-order terms.  The Adam term r = m / denom carries
5 roundings on fp32 masters (sqrt, / bc2_sqrt, + eps, m / denom, and bc2_sqrt itself, rounded to fp32 on the host; 4 on bf16,
where the multiply-add is fused): 5 u on r, 10 u on r^2, added to the bound.  Maximum and counts are exact."""
import functools
import math

import pytest
import torch

from dreamvla_amd import _lib
from tests import param_stats_ref as ref

BF, F32 = torch.bfloat16, torch.float32
CHUNK = _lib.STATS_CHUNK
U = 2.0 ** -24
TOL = (CHUNK // 256 + 10) * U               # sums of squares of a buffer, used on the norm (module docstring)
TOL_ADAM = TOL + 2 * 5 * U                  # + the roundings of r
# every size of the issue, not in order: the long ones land in different buckets, the empty one sits between two others
SIZES = [129, 3 * CHUNK + 5, 0, 1, CHUNK, 7, 8, CHUNK + 1, 9, 127, 128, CHUNK - 1]
NO_GRAD = 10                                # index into SIZES (128 elements): never receives a gradient
DTYPES = {"f32": [F32] * 12, "bf16": [BF] * 12, "mixed": [BF] * 6 + [F32] * 6}
MODES = sorted(DTYPES)
SMALL, LARGE = 32 << 10, 1 << 30            # bucket_bytes: four or more buckets / one bucket per dtype
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2
KEYS3 = ("grad_norm", "grad_absmax", "grad_nonfinite")


def _scales(shift):
    return [10.0 ** (-3 + 6 * ((i * 5 + shift) % 12) / 11) for i in range(12)]          # 1e-3 .. 1e3, every decade-ish once


@functools.lru_cache(maxsize=None)
def _init(mode):
    gen = torch.Generator().manual_seed(21)
    return [(torch.randn(n, generator=gen) * s).to(dt) for n, s, dt in zip(SIZES, _scales(0), DTYPES[mode])]


@functools.lru_cache(maxsize=None)
def _grads(mode, k):
    """the k-th gradient of every parameter on the CPU (read-only)"""
    gen = torch.Generator().manual_seed(500 + k)
    return [(torch.randn(n, generator=gen) * s).to(dt) for n, s, dt in zip(SIZES, _scales(3 + k), DTYPES[mode])]


def _make(mode, bucket_bytes=SMALL, init=None, **kw):
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    params = [torch.nn.Parameter(t.clone().cuda()) for t in (_init(mode) if init is None else init)]
    red = GradBucketReducer(params, bucket_bytes=bucket_bytes)
    for b in red.buckets:                       # what the reducer learns of a parameter no gradient reaches
        b["expected"] = [p is not params[NO_GRAD] for p in b["params"]]
    kw.setdefault("max_grad_norm", 0.1)
    opt = FlatAdamW(red, lr=kw.pop("lr", LR), betas=BETAS, eps=EPS, weight_decay=WD, **kw)
    return red, opt


def _set_grads(red, grads):
    for i, (p, g) in enumerate(zip(red.params, grads)):
        if i != NO_GRAD:
            red.grad_of(p).copy_(g)


def _run(mode, steps, bucket_bytes=SMALL, init=None, **kw):
    red, opt = _make(mode, bucket_bytes, init, **kw)
    for k in range(steps):
        _set_grads(red, _grads(mode, k))
        opt.step()
    return red, opt


def _slices(red, opt, key):
    """per parameter (reducer.params order): its slice of buffer `key` of its bucket"""
    index = {id(p): i for i, p in enumerate(red.params)}
    out = [None] * len(red.params)
    for b, s in zip(red.buckets, opt.flat):
        for p, off in zip(b["params"], b["offsets"]):
            out[index[id(p)]] = s[key][off:off + p.numel()]
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == F32 else t


def _same_bits(a, b, skip=()):
    assert sorted(a) == sorted(b)
    keep = [i for i in range(len(SIZES)) if i not in skip]
    for key in a:
        x, y = _bits(a[key])[keep], _bits(b[key])[keep]
        assert torch.equal(x, y), f"{key}: parameters {[keep[i] for i in (x != y).nonzero().flatten().tolist()]} differ"


def _close(got, want, tol, what):
    """|got - want| <= tol * want, printed before it is asserted"""
    err = abs(got - want) / want if want else abs(got)
    print(f"{what}: got {got!r} want {want!r} relative error {err:.3g} (tolerance {tol:.3g})")
    assert err <= tol, what


def _check_buffer(stats, prefix, tensors):
    """norm within TOL of the float64 reference, absmax and count exact"""
    for i, x in enumerate(tensors):
        sumsq, absmax, bad = ref.segment_stats(x)
        _close(float(stats[prefix + "_norm"][i]), math.sqrt(sumsq), TOL, f"{prefix}_norm[{i}] ({SIZES[i]} elements)")
        assert float(stats[prefix + "_absmax"][i]) == absmax, (prefix, i)
        assert int(stats[prefix + "_nonfinite"][i]) == bad == 0, (prefix, i)


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gradient_and_parameter_statistics_match_the_float64_reference(mode):
    red, opt = _make(mode)
    assert len(red.buckets) >= 3 and opt.master_mode == (mode != "bf16")
    assert sum(b["flat"].numel() for b in red.buckets) > sum(SIZES) + 500          # alignment gaps
    _set_grads(red, _grads(mode, 0))
    stats = opt.parameter_stats(("grad", "param"))
    assert sorted(stats) == sorted(("param_norm", "param_absmax", "param_nonfinite") + KEYS3)
    for key, t in stats.items():
        assert t.is_cuda and t.shape == (len(SIZES),) and t.dtype == (torch.int64 if key.endswith("nonfinite") else F32), key
    grads = [g if i != NO_GRAD else torch.zeros_like(g) for i, g in enumerate(_grads(mode, 0))]
    _check_buffer(stats, "grad", grads)
    _check_buffer(stats, "param", _init(mode))
    for key in KEYS3:
        assert float(stats[key][NO_GRAD]) == 0.0 and float(stats[key][SIZES.index(0)]) == 0.0
    # the default asks for everything; a string is one entry
    assert sorted(opt.parameter_stats()) == sorted(list(stats) + ["update_norm"]) and sorted(opt.parameter_stats("grad")) == sorted(KEYS3)


# ---- planted non-finite values -----------------------------------------------------------------------------------------------------
A, B, C, D = SIZES.index(3 * CHUNK + 5), SIZES.index(CHUNK + 1), SIZES.index(127), SIZES.index(9)
PLANTS = {A: [(0, "nan"), (3 * CHUNK + 4, "nan")],         # first element; last element, in the ragged end of the fourth chunk
          B: [(CHUNK, "inf")],                              # last element: a chunk of its own, one scalar load
          C: [(123, "-inf")],                               # in the ragged end 120 .. 126
          D: [(0, "inf"), (8, "nan")]}                      # first element of a vector and the one-element ragged end


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_planted_nan_and_inf_are_counted_exactly_and_touch_no_other_parameter(mode):
    red, opt = _make(mode)
    _set_grads(red, _grads(mode, 0))
    clean = opt.parameter_stats(("grad",))
    planted = [g.clone() for g in _grads(mode, 0)]
    for i, plants in PLANTS.items():
        for at, v in plants:
            planted[i][at] = float(v)
    _set_grads(red, planted)
    got = opt.parameter_stats(("grad",))
    _same_bits(got, clean, skip=PLANTS)
    assert got["grad_nonfinite"].tolist() == [len(PLANTS.get(i, ())) for i in range(len(SIZES))]
    assert torch.isinf(got["grad_absmax"]).nonzero().flatten().tolist() == sorted((B, C, D))
    for i in PLANTS:
        sumsq, absmax, bad = ref.segment_stats(planted[i])
        assert float(got["grad_absmax"][i]) == absmax and int(got["grad_nonfinite"][i]) == bad
        norm = float(got["grad_norm"][i])
        assert math.isnan(norm) if math.isnan(sumsq) else norm == math.inf == sumsq, i
    assert math.isfinite(float(got["grad_absmax"][A])) and float(got["grad_absmax"][A]) > 0.0      # the NaNs were dropped


# ---- gaps, determinism -------------------------------------------------------------------------------------------------------------
def _poison_gaps(red, opt):
    n_gap = 0
    for b, s in zip(red.buckets, opt.flat):
        gap = torch.ones(b["flat"].numel(), dtype=torch.bool, device="cuda")
        for p, off in zip(b["params"], b["offsets"]):
            gap[off:off + p.numel()] = False
        n_gap += int(gap.sum())
        for buf in (b["flat"], s["p"], s["m"], s["v"]):
            buf[gap] = float("nan")
    return n_gap


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_two_calls_give_the_same_bits_and_nan_in_the_alignment_gaps_changes_none(mode):
    red, opt = _run(mode, 2)
    first, second = opt.parameter_stats(), opt.parameter_stats()
    _same_bits(first, second)
    assert _poison_gaps(red, opt) > 500
    assert opt.flat[0]["m"].isnan().any() and red.buckets[0]["flat"].isnan().any()
    _same_bits(opt.parameter_stats(), first)
    assert not any(t.isnan().any() for t in first.values()) and bool((first["update_norm"] > 0).sum() == len(SIZES) - 2)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_parameter_gets_the_same_bits_whatever_bucket_it_sits_in(mode):
    """the same parameters and gradients under two bucket_bytes (clipping off: the clip norm is one sum over the buckets, in
    bucket order, so with it the moments themselves would depend on the cut)"""
    red_a, opt_a = _run(mode, 2, SMALL, max_grad_norm=None)
    red_b, opt_b = _run(mode, 2, LARGE, max_grad_norm=None)
    assert len(red_a.buckets) >= 3 and len(red_b.buckets) == (2 if mode == "mixed" else 1)
    _same_bits(opt_a.parameter_stats(), opt_b.parameter_stats())


# ---- consistency with the step's own norm ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_the_per_parameter_gradient_norms_add_up_to_the_clip_norm_of_the_step(mode):
    """dvla_sumsq_* on these buckets (at most 25 000 elements: no thread takes more than one vector): 8 fmafs + 1 of the ragged
    end, 6 + 3 adds in the workgroup, 6 + 3 in the final kernel, one add per further bucket -- (26 + buckets) u on its sum"""
    red, opt = _run(mode, 1)
    total = float(opt.grad_norm())
    per_param = opt.parameter_stats(("grad",))["grad_norm"].double().cpu()
    _close(math.sqrt(float((per_param ** 2).sum())), total, TOL + (26 + len(red.buckets)) * U, f"sum of grad_norm^2 vs grad_norm() [{mode}]")
    assert total > 100 * 0.1          # the step was clipped; the buffers still hold the unclipped gradient


# ---- update_norm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_update_norm_on_fp32_masters_is_the_norm_of_what_the_first_step_added():
    """from all-zero parameters the decayed parameter is 0 and p_new = rn(step_size r): the parameter IS the Adam term (+ one
    rounding per element and one of step_size: 2^-24 on the norm)"""
    red, opt = _run("f32", 1, init=[torch.zeros(n) for n in SIZES])
    got = opt.parameter_stats(("update",))["update_norm"]
    for i, p in enumerate(red.params):
        want = math.sqrt(ref.segment_stats(p)[0])
        assert (want > 0) == (SIZES[i] > 0 and i != NO_GRAD)
        _close(float(got[i]), want, TOL_ADAM + U, f"update_norm[{i}] vs the norm of the stepped zero parameter")


@pytest.mark.gpu
def test_update_norm_on_fp32_masters_matches_the_moments_of_the_checkpoint():
    red, opt = _run("f32", 3)
    got = opt.parameter_stats(("update",))["update_norm"]
    state = opt.state_dict()["state"]
    assert sorted(state) == [i for i in range(len(SIZES)) if i != NO_GRAD]
    for i in range(len(SIZES)):
        want = ref.update_norm(state[i]["exp_avg"], state[i]["exp_avg_sq"], LR, *BETAS, EPS, 3, True) if i in state else 0.0
        _close(float(got[i]), want, TOL_ADAM, f"update_norm[{i}] after 3 steps")


def _check_update(red, opt, step, lrs, what):
    """against the reference on the moments as stored; beta2 of a bf16 bucket as its step kernel receives it: a float"""
    got = opt.parameter_stats(("update",))["update_norm"]
    ms, vs = _slices(red, opt, "m"), _slices(red, opt, "v")
    for i, (m, v) in enumerate(zip(ms, vs)):
        master = m.dtype == F32
        beta2 = BETAS[1] if master else float(torch.tensor(BETAS[1], dtype=F32))
        want = ref.update_norm(m, v, lrs[i], BETAS[0], beta2, EPS, step, master)
        assert (want > 0) == (SIZES[i] > 0 and i != NO_GRAD)
        _close(float(got[i]), want, TOL_ADAM, f"update_norm[{i}] {what}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [False, True], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_update_norm_on_bf16_buckets_matches_the_moments_as_stored(mode, sr):
    red, opt = _run(mode, 3, **({"stochastic_rounding": True, "sr_seed": 5} if sr else {}))
    _check_update(red, opt, 3, [LR] * len(SIZES), f"[{mode}, stochastic_rounding={sr}]")


# ---- feature combinations ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "mixed"])
def test_every_parameter_is_scaled_by_the_lr_of_its_group_read_afresh(mode):
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    params = [torch.nn.Parameter(t.clone().cuda()) for t in _init(mode)]
    red = GradBucketReducer(params, bucket_bytes=SMALL)
    for b in red.buckets:
        b["expected"] = [p is not params[NO_GRAD] for p in b["params"]]
    groups = [{"params": params[0::2], "lr": 1e-3}, {"params": params[1::2], "lr": 3e-4, "weight_decay": 0.0}]
    opt = FlatAdamW(red, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.1, ema_decay=0.999, param_groups=groups)
    for k in range(2):
        _set_grads(red, _grads(mode, k))
        opt.step()
    before = _check_update(red, opt, 2, [1e-3, 3e-4] * 6, "two groups")
    opt.param_groups[1]["lr"] = 6e-4
    after = _check_update(red, opt, 2, [1e-3, 6e-4] * 6, "two groups, one lr edited")
    assert torch.equal(after[0::2], before[0::2]) and not torch.equal(after[1::2], before[1::2])


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_under_the_guard_the_step_count_is_the_applied_count_and_the_culprit_is_named(mode):
    red, opt = _make(mode, skip_nonfinite=True, ema_decay=0.999)
    assert not bool(opt.parameter_stats(("update",))["update_norm"].any())          # before any step
    _set_grads(red, _grads(mode, 0))
    opt.step()
    bad = [g.clone() for g in _grads(mode, 1)]
    bad[B][CHUNK] = float("nan")
    _set_grads(red, bad)
    opt.step()
    assert opt.parameter_stats(("grad",))["grad_nonfinite"].nonzero().flatten().tolist() == [B]      # before zero_grad()
    _set_grads(red, _grads(mode, 2))
    opt.step()
    _check_update(red, opt, 2, [LR] * len(SIZES), "applied, skipped, applied: t = 2")
    assert opt.applied_steps == 2 and opt.skipped_steps == 1
    # t = 3 would not have passed
    m, v = _slices(red, opt, "m")[A], _slices(red, opt, "v")[A]
    beta2 = BETAS[1] if mode == "f32" else float(torch.tensor(BETAS[1], dtype=F32))
    t2, t3 = (ref.update_norm(m, v, LR, BETAS[0], beta2, EPS, t, mode == "f32") for t in (2, 3))
    assert abs(t3 - t2) > 100 * TOL_ADAM * t2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_before_the_first_step_update_norm_is_zero_and_inside_ema_weights_the_call_raises(mode):
    red, opt = _make(mode, ema_decay=0.999)
    _set_grads(red, _grads(mode, 0))
    got = opt.parameter_stats()["update_norm"]
    assert got.shape == (len(SIZES),) and not bool(got.any())
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.parameter_stats(("grad",))
    with pytest.raises(ValueError, match="unknown entry"):
        opt.parameter_stats(("grad", "ema"))
    assert sorted(opt.parameter_stats(("grad",))) == sorted(KEYS3)


# ---- per module ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stats_by_module_on_a_two_level_module():
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW, stats_by_module
    torch.manual_seed(3)
    model = torch.nn.Sequential()
    model.add_module("trunk", torch.nn.Sequential(torch.nn.Linear(40, 50), torch.nn.LayerNorm(50), torch.nn.Linear(50, 50)))
    model.add_module("head", torch.nn.Linear(50, 3))
    model.cuda()
    extra = torch.nn.Parameter(torch.randn(77, device="cuda"))                  # in the reducer, in no module
    red = GradBucketReducer(list(model.parameters()) + [extra], bucket_bytes=4 << 10)
    opt = FlatAdamW(red, lr=LR)
    assert len(red.buckets) >= 3
    gen = torch.Generator().manual_seed(4)
    for i, p in enumerate(red.params):
        red.grad_of(p).copy_(torch.randn(p.shape, generator=gen) * 10.0 ** (i % 4 - 2))
    stats = opt.parameter_stats(("grad", "param"))
    want_names = {1: ["trunk", "head", "<unnamed>"], 2: ["trunk.0", "trunk.1", "trunk.2", "head.weight", "head.bias", "<unnamed>"]}
    named = dict(model.named_parameters())
    for depth, want in want_names.items():
        names, out = stats_by_module(stats, model, red, depth=depth)
        assert names == want and all(t.is_cuda and t.shape == (len(names),) for t in out.values())
        for k, name in enumerate(names):
            mine = [extra] if name == "<unnamed>" else [p for n, p in named.items() if (n + ".").startswith(name + ".")]
            for prefix, pick in (("grad", red.grad_of), ("param", lambda p: p.data)):
                x = torch.cat([pick(p).reshape(-1) for p in mine])
                sumsq, absmax, bad = ref.segment_stats(x)
                _close(float(out[prefix + "_norm"][k]), math.sqrt(sumsq), TOL, f"{prefix}_norm of {name} (depth {depth})")
                assert float(out[prefix + "_absmax"][k]) == absmax and int(out[prefix + "_nonfinite"][k]) == bad == 0


# ---- the step is what it was -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_calling_parameter_stats_between_steps_changes_no_bit_of_the_step(mode):
    def run(call):
        red, opt = _make(mode, ema_decay=0.999)
        for k in range(3):
            _set_grads(red, _grads(mode, k))
            if call:
                opt.parameter_stats()
            opt.step()
            if call:
                opt.parameter_stats()
        return [_bits(s[key]).clone() for s in opt.flat for key in ("p", "m", "v", "sh", "ema", "g") if key in s]
    with_calls, without = run(True), run(False)
    assert len(with_calls) == len(without) >= 15
    assert all(torch.equal(a, b) for a, b in zip(with_calls, without))
