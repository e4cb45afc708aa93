"""GPU: FlatAdamW(stochastic_rounding=True) -- dvla_sr_cast_f32_to_bf16 and dvla_adamw_bf16_sr.

The generator and the rounding are held bit for bit against tests/sr_ref.py (integer arithmetic on the host): through the
stand-alone cast on arbitrary data, and through the optimizer in the cases whose fp32 value before rounding is a one- or
two-operation expression that numpy float32 reproduces exactly.  Everything else is a comparison of two GPU runs as integers, or
the trajectory bound that tests/test_stochastic_rounding.py first holds on the host.  The stand-in buckets, gradients and helpers
are those of tests/test_guarded_step_gpu.py and tests/test_param_groups_gpu.py."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import sr_ref
from tests.test_guarded_step_gpu import BETAS, BF, EPS, F32, LR, POISON, WD, _bits, _Buckets, _grads, _init, _poisoned, _set_grads
from tests.test_param_groups_gpu import BIG_SIZES, GROUP_OF2, PAIRS, _grads2, _init2
from tests.test_stochastic_rounding import SEED, SEED_B, TRAJ_BETAS, TRAJ_EPS, TRAJ_HALF, TRAJ_LR, TRAJ_N, TRAJ_P0, TRAJ_T, traj_check, traj_grad

DECAY = 0.999
KEYS = ("p", "m", "v", "sh", "ema")
ERR_ARG = -1


def _u16(t):
    """the bits of a bf16 tensor as a numpy uint16 array"""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32_of_bits(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _opt(init, *, guard=False, ema=False, groups=None, pairs=None, sr=True, seed=SEED, max_norm=0.1, lr=LR, wd=WD, expected=None):
    """-> (reducer, optimizer) over clones of `init` (a list of buckets of tensors); groups: the group of every parameter, with
    pairs[g] = (lr, weight_decay) of group g"""
    from dreamvla_amd.optim import FlatAdamW
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in init])
    if expected is not None:
        for b, e in zip(red.buckets, expected):
            b["expected"] = list(e)
    kw = dict(lr=lr, weight_decay=wd, betas=BETAS, eps=EPS, max_grad_norm=max_norm, skip_nonfinite=guard, stochastic_rounding=sr,
              sr_seed=seed)
    if ema:
        kw.update(ema_decay=DECAY, ema_warmup=True)
    if groups is not None:
        kw["param_groups"] = [{"params": [p for p, g in zip(red.params, groups) if g == k], "lr": a, "weight_decay": b}
                              for k, (a, b) in enumerate(pairs)]
    return red, FlatAdamW(red, **kw)


def _snap(opt):
    return [{k: _bits(s[k]).clone() for k in KEYS if k in s} for s in opt.flat]


def _assert_same(a, b, what="", keys=None):
    assert len(a) == len(b)
    for bi, (x, y) in enumerate(zip(a, b)):
        for k in (keys or sorted(set(x) | set(y))):
            assert k in x and k in y, (what, bi, k)
            assert torch.equal(x[k], y[k]), f"{what}: bucket {bi}, {k}: {int((x[k] != y[k]).sum())} elements differ"


def _steps(red, opt, grads):
    for g in grads:
        _set_grads(red, g)
        opt.step()
    return _snap(opt)


# ---- 1. the cast against the host, bit for bit -------------------------------------------------------------------------------------
SPECIALS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x7F800001, 0xFF80FFFF, 0x7FC00000, 0x7F7FFFFF,
            0xFF7FFFFF, 0x3F800000, 0xBF800000, 0xC0490FDB, 0x0000FFFF, 0x007FFFFF, 0x3F80FFFF, 0x3F808000, 0x3F807FFF, 0x7F7F0001]
SENTINEL = 0x5A5A


@functools.lru_cache(maxsize=None)
def _cast_data(n):
    """n fp32 values as uint32 bits: every special value, then normals scaled over 60 binades"""
    gen = np.random.default_rng(77)
    x = (gen.standard_normal(n) * np.exp2(gen.uniform(-30, 30, n))).astype(np.float32).view(np.uint32)
    k = min(n, len(SPECIALS))
    x[:k] = np.array(SPECIALS[:k], dtype=np.uint32)
    if n > 4000:                    # and once more beyond the first block and in the last elements
        x[3000:3000 + len(SPECIALS)] = np.array(SPECIALS, dtype=np.uint32)
        x[-len(SPECIALS):] = np.array(SPECIALS, dtype=np.uint32)
    return x


CAST_CASES = [(n, 0, (0, 1, 2)) for n in (0, 1, 7, 8, 9, 3027)] + [(sum(BIG_SIZES), 0, (2,)), (3027, (1 << 32) - 1000, (0, 1, 2)),
                                                                  (9, (1 << 40) + 3, (1,))]


@pytest.mark.gpu
@pytest.mark.parametrize("n,base,streams", CAST_CASES, ids=[f"n{n}-base{b}" for n, b, _ in CAST_CASES])
def test_cast_is_the_host_restatement_bit_for_bit(n, base, streams):
    from dreamvla_amd import _lib
    lib = _lib.load()
    assert sum(BIG_SIZES) % 8 != 0 and sum(BIG_SIZES) > 4096 * 256 * 8
    bits = _cast_data(n)
    x = torch.from_numpy(bits.view(np.float32).copy()).cuda()
    pad = 19                        # out starts 38 bytes into the buffer: the cast works at any address
    for stream in streams:
        buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int16, device="cuda")
        rc = lib.dvla_sr_cast_f32_to_bf16(x.data_ptr() if n else buf.data_ptr(), buf.data_ptr() + 2 * pad, n, SEED, 7, 3, stream, base,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        got = buf.cpu().numpy().view(np.uint16)
        assert (got[:pad] == SENTINEL).all() and (got[pad + n:] == SENTINEL).all(), "the sentinel around `out` was overwritten"
        want = sr_ref.sr_cast(bits.view(np.float32), SEED, 7, 3, stream, base)
        bad = np.nonzero(got[pad:pad + n] != want)[0]
        assert bad.size == 0, (stream, bad[:5], [hex(int(bits[i])) for i in bad[:5]])


@pytest.mark.gpu
def test_the_python_binding_is_the_cast():
    from dreamvla_amd import ops
    bits = _cast_data(3027)
    x = torch.from_numpy(bits.view(np.float32).copy()).cuda().view(3, 1009)
    out = ops.stochastic_round_bf16(x, seed=SEED_B, step=2, bucket=1, stream=1, index_base=40)
    assert out.dtype == BF and out.shape == x.shape
    assert np.array_equal(_u16(out).reshape(-1), sr_ref.sr_cast(bits.view(np.float32), SEED_B, 2, 1, 1, 40))
    # defaults, and NaN stays NaN / inf stays inf through torch's eyes
    out0 = ops.stochastic_round_bf16(x)
    assert np.array_equal(_u16(out0).reshape(-1), sr_ref.sr_cast(bits.view(np.float32)))
    assert torch.equal(torch.isnan(out0), torch.isnan(x)) and torch.equal(torch.isinf(out0) & torch.isinf(x), torch.isinf(x))
    with pytest.raises(TypeError):
        ops.stochastic_round_bf16(x.to(BF))


# ---- 2. the optimizer draws exactly the specified bits -----------------------------------------------------------------------------
def _layouts():
    return {"LAYOUT": (_init("bf16"), [0, 1, 0], lambda k: _grads("bf16", k)),
            "LAYOUT2": (_init2("bf16"), GROUP_OF2, lambda k: _grads2("bf16", k))}


def _f(x):
    return np.float32(x)


def _decay(lr, wd):
    """1 - lr wd as the kernel forms it from the float lr and wd: fused in the vector loop, two roundings in the ragged tail.
    The cases here use pairs for which both are the same float (asserted), so one expectation serves both loops."""
    fused = _f(1.0 - float(_f(lr)) * float(_f(wd)))          # the product of two floats is exact in a double
    two = _f(1) - _f(lr) * _f(wd)
    assert fused == two, (lr, wd)
    return two


def _variant(init, groups, variant, **kw):
    """plain / guarded: one group with PAIRS[0]; grouped: the layout's groups with PAIRS"""
    if variant == "grouped":
        return _opt(init, groups=groups, pairs=PAIRS[:max(groups) + 1], **kw), [PAIRS[g] for g in groups]
    lr, wd = PAIRS[0]
    return _opt(init, guard=variant == "guarded", lr=lr, wd=wd, **kw), [PAIRS[0]] * len(groups)


def _per_parameter(red, opt):
    """(bucket index, offset, size, position in reducer.params) of every parameter"""
    index = {id(p): i for i, p in enumerate(red.params)}
    return [(bi, off, p.numel(), index[id(p)]) for bi, b in enumerate(red.buckets) for p, off in zip(b["params"], b["offsets"])]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "guarded", "grouped"])
@pytest.mark.parametrize("layout", ["LAYOUT", "LAYOUT2"])
def test_weight_decay_alone_draws_stream_0_of_every_step(layout, variant):
    """zero gradient, zero moments, wd > 0: p' = sr(p (1 - lr wd)) under the key of step 1, 2, 3 -- which pins the step key"""
    init, groups, _ = _layouts()[layout]
    (red, opt), pair_of = _variant(init, groups, variant, max_norm=None)
    where = _per_parameter(red, opt)
    cur = [_u16(s["p"]).copy() for s in opt.flat]
    for step in (1, 2, 3):
        red.zero_grad()
        opt.step()
        for bi, off, n, i in where:
            lr, wd = pair_of[i]
            if wd == 0.0:
                want = cur[bi][off:off + n]                  # p * 1 is p, a bf16: unchanged for every r
            else:
                val = _f32_of_bits(cur[bi][off:off + n]) * _decay(lr, wd)
                r = sr_ref.sr_bits(SEED, step, bi, 0, np.uint64(off) + np.arange(n, dtype=np.uint64))
                want = sr_ref.sr_bf16(val.view(np.uint32), r)
            got = _u16(opt.flat[bi]["p"])[off:off + n]
            assert np.array_equal(got, want), (step, bi, off, int((got != want).sum()))
            cur[bi][off:off + n] = want
        for s in opt.flat:
            assert not _bits(s["m"]).any() and not _bits(s["v"]).any()
    if variant == "guarded":
        assert opt.applied_steps == 3 and opt.skipped_steps == 0
    # the decay did land on some weights, which round-to-nearest never allows at lr wd = 1e-5
    first = np.concatenate([_u16(torch.cat([p.reshape(-1) for p in g])) for g in init])
    last = np.concatenate([c[off:off + n] for (bi, off, n, i) in where for c in [cur[bi]]])
    assert 0 < int((first != last).sum()) < first.size


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "guarded", "grouped"])
@pytest.mark.parametrize("layout", ["LAYOUT", "LAYOUT2"])
def test_first_step_draws_streams_1_and_2_for_the_moments(layout, variant):
    """from zero moments, no clip: m' = sr(g (1 - beta1)), v' = sr(((1 - beta2) g) g)"""
    init, groups, grads = _layouts()[layout]
    (red, opt), _ = _variant(init, groups, variant, max_norm=None)
    g = grads(0)
    _set_grads(red, g)
    opt.step()
    b1, b2 = _f(BETAS[0]), _f(BETAS[1])
    for bi, off, n, i in _per_parameter(red, opt):
        gf = _f32_of_bits(_u16(g[i]).reshape(-1))
        idx = np.uint64(off) + np.arange(n, dtype=np.uint64)
        want_m = sr_ref.sr_bf16(((_f(1) - b1) * gf).view(np.uint32), sr_ref.sr_bits(SEED, 1, bi, 1, idx))
        want_v = sr_ref.sr_bf16((((_f(1) - b2) * gf) * gf).view(np.uint32), sr_ref.sr_bits(SEED, 1, bi, 2, idx))
        assert np.array_equal(_u16(opt.flat[bi]["m"])[off:off + n], want_m), (bi, off, "exp_avg")
        assert np.array_equal(_u16(opt.flat[bi]["v"])[off:off + n], want_v), (bi, off, "exp_avg_sq")


# ---- 3. one step from a common state: stochastic next to round-to-nearest ----------------------------------------------------------
def _ordinal(bits16):
    """bf16 bits (int16 tensor) -> their position on the number line (so that neighbours differ by 1; +0 and -0 coincide)"""
    b = bits16.to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b & 0x7FFF), b)


def _common_state(opt, step_count=5):
    gen = torch.Generator().manual_seed(21)
    for s in opt.flat:
        n = s["p"].numel()
        s["m"].copy_((torch.randn(n, generator=gen) * 0.05).to(BF))
        s["v"].copy_((torch.randn(n, generator=gen) * 0.05).square().to(BF))
    opt.step_count = step_count


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm", [0.1, None], ids=["clip", "noclip"])
def test_one_step_lands_on_a_neighbour_of_the_round_to_nearest_step(max_norm):
    runs = {}
    for sr in (False, True):
        red, opt = _opt(_init("bf16"), sr=sr, max_norm=max_norm)
        _common_state(opt)
        runs[sr] = _steps(red, opt, [_grads("bf16", 0)])
    for bi, (a, b) in enumerate(zip(runs[False], runs[True])):
        for k in ("p", "m", "v"):
            d = (_ordinal(a[k]) - _ordinal(b[k])).abs()
            assert int(d.max()) <= 1, (bi, k, int(d.max()))         # both are neighbours of the same fp32 value
            assert 0 < int((d != 0).sum()) < d.numel(), (bi, k)     # some are rounded the other way, not all


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "guarded", "grouped"])
def test_with_lr_zero_the_parameters_keep_every_bit(variant):
    init = _init("bf16")
    if variant == "grouped":
        red, opt = _opt(init, groups=[0, 1, 0], pairs=[(0.0, 0.01), (0.0, 0.3)])
    else:
        red, opt = _opt(init, guard=variant == "guarded", lr=0.0)
    if variant != "guarded":
        _common_state(opt)
    before = _snap(opt)
    after = _steps(red, opt, [_grads("bf16", 0), _grads("bf16", 1)])
    _assert_same(before, after, "lr = 0", keys=("p",))
    assert any(not torch.equal(a["m"], b["m"]) for a, b in zip(before, after))       # the moments did move


# ---- 4. combinations ---------------------------------------------------------------------------------------------------------------
STEPS = 4


@functools.lru_cache(maxsize=None)
def _plain_run(mode, ema=False, sr=True):
    red, opt = _opt(_init(mode), ema=ema, sr=sr)
    return _steps(red, opt, [_grads(mode, k) for k in range(STEPS)])


@pytest.mark.gpu
@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_guarded_without_a_skip_is_the_plain_step(mode, ema):
    red, opt = _opt(_init(mode), guard=True, ema=ema)
    got = _steps(red, opt, [_grads(mode, k) for k in range(STEPS)])
    assert opt.applied_steps == STEPS and opt.skipped_steps == 0
    _assert_same(got, _plain_run(mode, ema), "guarded / plain")


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_two_groups_with_equal_hyper_parameters_are_one_group(mode, ema, guard):
    red, opt = _opt(_init(mode), guard=guard, ema=ema, groups=[0, 1, 0], pairs=[(LR, WD), (LR, WD)])
    assert len(opt.param_groups) == 2
    got = _steps(red, opt, [_grads(mode, k) for k in range(STEPS)])
    _assert_same(got, _plain_run(mode, ema), "two equal groups / one group")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_the_ema_leaves_the_step_alone_and_follows_the_stored_parameter(mode):
    from tests.test_ema_step_gpu import _d
    red, opt = _opt(_init(mode), ema=True)
    ref = [s["p"].float().clone() for s in opt.flat]
    for k in range(STEPS):
        _set_grads(red, _grads(mode, k))
        opt.step()
        for s, r in zip(opt.flat, ref):
            r.lerp_(s["p"].float(), 1.0 - _d(DECAY, True, k + 1))
            assert torch.equal(_bits(s["ema"]), _bits(r)), f"step {k + 1}"
    _assert_same(_snap(opt), _plain_run(mode, False), "with / without EMA", keys=("p", "m", "v"))


@pytest.mark.gpu
def test_fp32_buckets_of_a_mixed_reducer_are_stepped_as_without_the_flag():
    on, off = _plain_run("mixed", False, True), _plain_run("mixed", False, False)
    assert "sh" in on[1] and "sh" not in on[0]
    _assert_same(on[1:], off[1:], "fp32 bucket, flag on / off")
    assert not torch.equal(on[0]["p"], off[0]["p"])                  # while the bf16 bucket is rounded differently


# ---- 5. skipped steps --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
@pytest.mark.parametrize("grouped", [False, True], ids=["one-group", "grouped"])
@pytest.mark.parametrize("where", ["first", "last_tail"])
def test_a_skipped_step_draws_nothing_and_does_not_advance_the_key(where, grouped):
    """g1, POISON, g2 is g1, g2 bit for bit in every buffer (the EMA included): first vector / ragged tail"""
    kw = dict(groups=[0, 1, 0], pairs=[(LR, WD), (3e-4, 0.0)]) if grouped else {}
    g1, g2 = _grads("bf16", 0), _grads("bf16", 1)
    red, opt = _opt(_init("bf16"), guard=True, ema=True, **kw)
    got = _steps(red, opt, [g1, _poisoned(g2, where, POISON["nan"]), g2])
    assert opt.applied_steps == 2 and opt.skipped_steps == 1
    red, ref = _opt(_init("bf16"), guard=True, ema=True, **kw)
    want = _steps(red, ref, [g1, g2])
    assert ref.applied_steps == 2 and ref.skipped_steps == 0
    _assert_same(got, want, "g1, POISON, g2 / g1, g2")


# ---- 6. geometry -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _init3():
    gen = torch.Generator().manual_seed(31)
    return [[(torch.randn(s, generator=gen) * 0.5).to(BF).cuda() for s in [(1300,), (517,), (1203,)]]]


@functools.lru_cache(maxsize=None)
def _grads3(k):
    gen = torch.Generator().manual_seed(3000 + k)
    return [(torch.randn(s, generator=gen) * 0.3).to(BF).cuda() for s in [(1300,), (517,), (1203,)]]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "guarded", "grouped"])
def test_a_bucket_stepped_in_two_ranges_draws_the_bits_of_one_stepped_whole(variant):
    """the parameter in the middle receives no gradient (`expected` false): two ranges, or 255 in the group map"""
    kw = dict(groups=[0, 1, 1], pairs=[(LR, WD), (3e-4, 0.05)]) if variant == "grouped" else dict(guard=variant == "guarded")
    grads = [_grads3(k) for k in range(3)]
    red, whole = _opt(_init3(), ema=True, **kw)
    a = _steps(red, whole, grads)[0]
    red, split = _opt(_init3(), ema=True, expected=[[True, False, True]], **kw)
    if variant != "grouped":
        assert split._ranges(0) == [(0, 1304), (1824, 3027)]
    before = _snap(split)[0]
    b = _steps(red, split, grads)[0]
    for lo, hi, same_as in ((0, 1300, a), (1824, 3027, a), (1304, 1304 + 517, before)):
        for k in KEYS:
            if k in a:
                assert torch.equal(b[k][lo:hi], same_as[k][lo:hi]), (k, lo, hi)
    assert not torch.equal(a["p"][1304:1821], before["p"][1304:1821])


@pytest.mark.gpu
def test_the_same_seed_agrees_and_another_seed_differs():
    runs = []
    for seed in (SEED, SEED, SEED_B, 0, 2 ** 64 - 1):
        red, opt = _opt(_init("bf16"), seed=seed)
        runs.append(_steps(red, opt, [_grads("bf16", 0), _grads("bf16", 1)]))
    _assert_same(runs[0], runs[1], "the same seed twice")
    for other in runs[2:]:
        for a, b in zip(runs[0], other):
            assert all(not torch.equal(a[k], b[k]) for k in ("p", "m", "v"))


# ---- 7. trajectory, with a control that must fail ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stochastic", [True, False], ids=["stochastic", "nearest-control"])
def test_trajectory_follows_float64_adamw_where_round_to_nearest_stalls(stochastic):
    """65541 bf16 weights at 0.75, g = +0.5 / -0.5 / 0, lr = 1e-4, 200 steps: float64 AdamW ends at 0.75 -+ 0.02.  Bounds and
    their derivation: tests/test_stochastic_rounding.py::traj_check (|mean(p) - p_f64| <= 2e-3 per half = 13 standard deviations
    of the mean's rounding noise and a tenth of the stall's error; moments within 1 %).  The control -- the same run with
    round-to-nearest stores -- leaves every weight at 0.75 and misses the bound by 0.02."""
    from dreamvla_amd.optim import FlatAdamW
    p0 = torch.full((TRAJ_N,), TRAJ_P0, dtype=BF, device="cuda")
    red = _Buckets([[torch.nn.Parameter(p0.clone())]])
    opt = FlatAdamW(red, lr=TRAJ_LR, betas=TRAJ_BETAS, eps=TRAJ_EPS, weight_decay=0.0, stochastic_rounding=stochastic, sr_seed=SEED)
    _set_grads(red, [torch.from_numpy(traj_grad()).to(BF).cuda()])
    for _ in range(TRAJ_T):
        opt.step()
    s = opt.flat[0]
    traj_check(*[s[k].double().cpu().numpy() for k in ("p", "m", "v")], stochastic)
    assert torch.equal(_bits(s["p"][2 * TRAJ_HALF:]), _bits(p0[2 * TRAJ_HALF:]))        # zero gradient: bit for bit p0
    if not stochastic:
        assert torch.equal(_bits(s["p"]), _bits(p0))


# ---- 8. checkpoints ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_a_resumed_run_continues_bit_for_bit(mode, guard):
    grads = [_grads(mode, k) for k in range(5)]
    red, whole = _opt(_init(mode), guard=guard)
    want = _steps(red, whole, grads)
    red, first = _opt(_init(mode), guard=guard)
    _steps(red, first, grads[:3])
    sd = copy.deepcopy(first.state_dict())
    saved = sd["param_groups"][0] if mode == "mixed" else sd
    assert saved["stochastic_rounding"] == {"seed": SEED}
    red2, second = _opt([[p.detach().clone() for p in b["params"]] for b in red.buckets], guard=guard, seed=SEED_B)
    second.load_state_dict(sd)
    assert second.sr_seed == SEED and second.step_count == 3
    _assert_same(_steps(red2, second, grads[3:]), want, "3 + 2 steps / 5 steps", keys=("p", "m", "v"))
    if mode == "mixed":
        fresh = [torch.nn.Parameter(p.detach().float().clone()) for p in red.params]
        torch.optim.AdamW(fresh, lr=LR).load_state_dict(sd)                             # torch accepts the extra key
    # a checkpoint without the key leaves the constructor's seed
    del saved["stochastic_rounding"]
    red3, third = _opt([[p.detach().clone() for p in b["params"]] for b in red.buckets], guard=guard, seed=SEED_B)
    third.load_state_dict(sd)
    assert third.sr_seed == SEED_B
    # and an optimizer without the flag writes no key
    plain = _opt(_init(mode), sr=False)[1].state_dict()
    assert "stochastic_rounding" not in plain and "stochastic_rounding" not in plain["param_groups"][0]


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    from dreamvla_amd import _lib
    from dreamvla_amd.optim import FlatAdamW
    with pytest.raises(ValueError, match="no bf16 bucket"):
        _opt(_init("f32"))
    for seed in (-1, 2 ** 64, 1.5, "7", None, True):
        with pytest.raises(ValueError, match="sr_seed"):
            _opt(_init("bf16"), seed=seed)
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init("f32")])
    FlatAdamW(red, stochastic_rounding=False, sr_seed=5)                                # the seed alone is harmless
    lib = _lib.load()
    x = torch.zeros(64, dtype=F32, device="cuda")
    out = torch.zeros(64, dtype=BF, device="cuda")
    cast = lib.dvla_sr_cast_f32_to_bf16
    assert cast(None, out.data_ptr(), 64, 0, 0, 0, 0, 0, None) == ERR_ARG
    assert cast(x.data_ptr(), None, 64, 0, 0, 0, 0, 0, None) == ERR_ARG
    assert cast(x.data_ptr(), out.data_ptr(), -1, 0, 0, 0, 0, 0, None) == ERR_ARG
    assert cast(x.data_ptr(), out.data_ptr(), 64, 0, 0, 0, 3, 0, None) == ERR_ARG
    assert cast(x.data_ptr(), out.data_ptr(), 64, 0, 0, 0, -1, 0, None) == ERR_ARG
    assert cast(x.data_ptr(), out.data_ptr(), 0, 0, 0, 0, 0, 0, None) == 0
    p = torch.zeros(64, dtype=BF, device="cuda").data_ptr()
    one = ctypes.c_double * 1
    gmap = torch.zeros(8, dtype=torch.uint8, device="cuda").data_ptr()

    def step(param=p, grad=p, n=64, gm=None, n_groups=1, step=1, base=0):
        return lib.dvla_adamw_bf16_sr(param, grad, p, p, None, n, gm, n_groups, one(1e-3), one(0.0), 0.9, 0.999, 1e-8, step, None, 0.0,
                                      None, None, 1, 0, 0, base, None)

    assert step(param=None) == ERR_ARG and step(grad=None) == ERR_ARG and step(n=-1) == ERR_ARG and step(step=0) == ERR_ARG
    assert step(n_groups=2) == ERR_ARG and step(gm=gmap, n_groups=0) == ERR_ARG and step(base=-8) == ERR_ARG
    assert step(n=0) == 0


# ---- 10. the real reducer ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_step_over_the_real_reducer_with_flag_guard_and_weight_decay_groups(monkeypatch):
    """a small bf16 model over GradBucketReducer (every parameter padded to 128 elements: gaps in the map), as
    tests/test_param_groups_gpu.py::test_weight_decay_groups_over_the_real_reducer builds it"""
    from dreamvla_amd import _lib
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW, weight_decay_groups
    torch.manual_seed(5)
    proto = torch.nn.Sequential(torch.nn.Linear(40, 50), torch.nn.LayerNorm(50), torch.nn.Linear(50, 3)).cuda().to(BF)
    x = torch.randn(16, 40, device="cuda").to(BF)
    lib = _lib.load()
    calls = []
    for name in _lib.SYMBOLS:
        if name.startswith("dvla_adamw_"):
            real = getattr(lib, name)
            monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    counts = {}
    for sr in (False, True):
        model = copy.deepcopy(proto)
        red = GradBucketReducer(list(model.parameters()))
        opt = FlatAdamW(red, lr=LR, max_grad_norm=0.1, skip_nonfinite=True, ema_decay=DECAY, stochastic_rounding=sr, sr_seed=SEED,
                        param_groups=weight_decay_groups(model, 0.05))
        before = [s["p"].clone() for s in opt.flat]
        del calls[:]
        opt.zero_grad()
        loss = model(x).float().square().mean()
        loss.backward()
        red.finish()
        opt.step()
        counts[sr] = len(calls)
        assert set(calls) == {"dvla_adamw_bf16_sr" if sr else "dvla_adamw_bf16_grouped"}
        assert opt.applied_steps == 1 and opt.skipped_steps == 0
        assert torch.isfinite(loss).item()
        for s, b in zip(opt.flat, before):
            assert all(torch.isfinite(s[k].float()).all().item() for k in KEYS if k in s)
            assert not torch.equal(s["p"], b)
    assert counts[True] == counts[False] == len(red.buckets)                            # one launch per bucket, as without the flag
