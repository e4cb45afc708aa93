"""GPU: FlatAdamW(clip="group") -- dvla_group_sumsq + dvla_adamw_bf16_grouped_clip / dvla_adamw_f32_master_grouped_clip /
dvla_adamw_bf16_sr_clip.

The oracle of the step is the one-group entry point itself: a parameter of group g must come out -- bit for bit, buffers are
compared as integers -- as dvla_adamw_bf16 / dvla_adamw_f32_master / their _ema twins / dvla_adamw_bf16_sr (group_map NULL) give it
over a clone of the same bucket with (lr_g, weight_decay_g), grad_sumsq pointing at S_g (group_grad_sumsq()) and max_norm = m_g;
grad_sumsq NULL for a group that is not clipped.  The norms are held against float64 at the bound the reduction's structure gives
(DESIGN.md 4.3): 42 u on a parameter's sum of squares, one more rounding for the group's, u = 2^-24, and as there the NORM is held
to the bound on the sum.

The layout is that of tests/test_param_groups_gpu.py (a group boundary inside a wave, a one-vector parameter, a ragged bucket tail
in another group than the vector before it) plus a third bucket with one parameter of 16389 elements: three records, the last
ragged.  Clip values (0.1, 1e3, None): group 0 clips (and takes the constructor's value: it has no key), group 1 has a coefficient
of 1, group 2 is not clipped."""
import copy
import ctypes
import functools
import math

import pytest
import torch

from tests.test_group_clip import group_clip_adamw_f64
from tests.test_guarded_step_gpu import _bits, _Buckets, _set_grads
from tests.test_master_adamw_gpu import _within
from tests.test_param_groups_gpu import GROUP_OF2, LAMBDAS, LAYOUT2, PAIRS, SHAPES2, _snap

BF, F32 = torch.bfloat16, torch.float32
BETAS, EPS, DECAY = (0.9, 0.999), 1e-8, 0.999
LONG = 16389                                                      # 2 * DVLA_STATS_CHUNK + 5
SHAPES3 = SHAPES2 + [[(LONG,)]]
LAYOUT3 = {mode: dts + [dts[0]] for mode, dts in LAYOUT2.items()}      # the long parameter: bf16 in "mixed"
GROUP_OF3 = GROUP_OF2 + [0]
CLIPS = (0.1, 1e3, None)
MODES = ["bf16", "f32", "mixed"]
STEPS = 4
U = 2.0 ** -24
SUM_BOUND = 43 * U                                                # (STATS_CHUNK / 256 + 10) u per parameter + the group's one rounding


@functools.lru_cache(maxsize=None)
def _init3(mode):
    gen = torch.Generator().manual_seed(21)
    return [[(torch.randn(s, generator=gen) * 0.5).to(dt).cuda() for s in shapes] for dt, shapes in zip(LAYOUT3[mode], SHAPES3)]


@functools.lru_cache(maxsize=None)
def _grads3(mode, k):
    """the k-th gradient of every parameter (read-only)"""
    gen = torch.Generator().manual_seed(4000 + k)
    return [(torch.randn(s, generator=gen) * 0.3).to(dt).cuda() for dt, shapes in zip(LAYOUT3[mode], SHAPES3) for s in shapes]


def _groups(red, group_of, clips=CLIPS, pairs=PAIRS):
    """torch groups; group 0 carries no "max_grad_norm" (it takes the constructor's, clips[0])"""
    groups = [{"params": [p for p, g in zip(red.params, group_of) if g == k], "lr": lr, "weight_decay": wd}
              for k, (lr, wd) in enumerate(pairs)]
    for g, m in list(zip(groups, clips))[1:]:
        g["max_grad_norm"] = m
    return groups


def _make(mode, guard=False, ema=False, sr=False, init=None, group_of=GROUP_OF3, clips=CLIPS, pairs=PAIRS, clip="group"):
    from dreamvla_amd.optim import FlatAdamW
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in (_init3(mode) if init is None else init)])
    kw = dict(ema_decay=DECAY, ema_warmup=True) if ema else {}
    opt = FlatAdamW(red, betas=BETAS, eps=EPS, max_grad_norm=clips[0], skip_nonfinite=guard, stochastic_rounding=sr, sr_seed=77,
                    param_groups=_groups(red, group_of, clips, pairs), clip=clip, **kw)
    return red, opt


def _twin(opt, before, bi, lr, wd, sumsq_ptr, max_norm, step):
    """the one-group entry point over a clone of bucket bi as it stood before the step -> the clone's buffers"""
    from dreamvla_amd import _lib
    lib, check = _lib.load(), _lib.check
    stream = torch.cuda.current_stream().cuda_stream
    s = {k: t.clone() for k, t in before[bi].items()}
    g = opt.flat[bi]["g"]
    n = g.numel()
    mx = 0.0 if max_norm is None else max_norm
    ss = None if max_norm is None else sumsq_ptr
    w = (ctypes.c_float * _lib.STEP_MAX_CANDIDATES)()
    if "ema" in s:
        check(lib.dvla_ema_weights(DECAY, 1, step, 1, w), "dvla_ema_weights")
    ptr = {k: t.data_ptr() for k, t in s.items()}
    if g.dtype == F32:
        if "ema" in s:
            check(lib.dvla_adamw_f32_master_ema(ptr["p"], g.data_ptr(), ptr["m"], ptr["v"], ptr["sh"], ptr["ema"], n, lr, *BETAS, EPS, wd,
                                                step, ss, mx, w[0], stream), "dvla_adamw_f32_master_ema")
        else:
            check(lib.dvla_adamw_f32_master(ptr["p"], g.data_ptr(), ptr["m"], ptr["v"], ptr["sh"], n, lr, *BETAS, EPS, wd, step, ss, mx,
                                            stream), "dvla_adamw_f32_master")
    elif opt.stochastic_rounding:
        one = ctypes.c_double * 1
        check(lib.dvla_adamw_bf16_sr(ptr["p"], g.data_ptr(), ptr["m"], ptr["v"], ptr.get("ema"), n, None, 1, one(lr), one(wd), *BETAS, EPS,
                                     step, ss, mx, None, w if "ema" in s else None, 1, opt.sr_seed, bi, 0, stream), "dvla_adamw_bf16_sr")
    elif "ema" in s:
        check(lib.dvla_adamw_bf16_ema(ptr["p"], g.data_ptr(), ptr["m"], ptr["v"], ptr["ema"], n, lr, *BETAS, EPS, wd, step, ss, mx, w[0],
                                      stream), "dvla_adamw_bf16_ema")
    else:
        check(lib.dvla_adamw_bf16(ptr["p"], g.data_ptr(), ptr["m"], ptr["v"], n, lr, *BETAS, EPS, wd, step, ss, mx, stream),
              "dvla_adamw_bf16")
    return s


def _buffers(opt):
    return [{k: t.clone() for k, t in s.items() if k != "g"} for s in opt.flat]


def _assert_every_parameter_is_its_twins(red, opt, before, hyper, step, group_of):
    """hyper[g] = (lr, wd, max_norm) as the step read them; S_g from group_grad_sumsq()"""
    sums = opt.group_grad_sumsq()
    for g, (lr, wd, m) in enumerate(hyper):
        for bi, b in enumerate(red.buckets):
            mine = [(p, off) for p, off in zip(b["params"], b["offsets"]) if group_of[_index(red, p)] == g]
            if not mine:
                continue
            want = _twin(opt, before, bi, lr, wd, sums.data_ptr() + 4 * g, m, step)
            for p, off in mine:
                for key, t in want.items():
                    a, w = opt.flat[bi][key][off:off + p.numel()], t[off:off + p.numel()]
                    assert torch.equal(_bits(a), _bits(w)), \
                        f"step {step}, parameter {_index(red, p)} (group {g}): {int((_bits(a) != _bits(w)).sum())} elements of {key} differ"


def _index(red, p):
    return next(i for i, q in enumerate(red.params) if q is p)


def _read_hyper(opt):
    from dreamvla_amd.optim import group_max_norms
    return [(float(g["lr"]), float(g["weight_decay"]), m)
            for g, m in zip(opt.param_groups, group_max_norms(opt.param_groups, opt.max_grad_norm))]


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------
CASES = [(mode, guard, ema, sr) for mode in MODES for guard in (False, True) for ema in (False, True) for sr in (False, True)
         if not (sr and mode == "f32")]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,guard,ema,sr", CASES,
                         ids=[f"{m}-{'guarded' if g else 'plain'}-{'ema' if e else 'noema'}-{'sr' if s else 'rne'}" for m, g, e, s in CASES])
def test_every_parameter_is_stepped_as_the_one_group_entry_point_on_its_groups_norm(mode, guard, ema, sr):
    """4 steps, the lrs rewritten every step by LambdaLR with one lambda per group, group 0's max_grad_norm edited after step 2"""
    red, opt = _make(mode, guard, ema, sr)
    assert [b["flat"].numel() for b in red.buckets] == [3027, 3005, LONG] and opt.clip == "group"
    assert [g.get("max_grad_norm", "absent") for g in opt.param_groups] == ["absent", 1e3, None]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, LAMBDAS)
    coefs = []
    for k in range(STEPS):
        if k == 2:
            opt.param_groups[0]["max_grad_norm"] = 0.05
        hyper = _read_hyper(opt)
        assert [h[2] for h in hyper] == [0.05 if k >= 2 else 0.1, 1e3, None]
        before = _buffers(opt)
        _set_grads(red, _grads3(mode, k))
        opt.step()
        _assert_every_parameter_is_its_twins(red, opt, before, hyper, k + 1, GROUP_OF3)
        norms = opt.group_grad_norms().tolist()
        coefs.append([None if m is None else m / (n + 1e-6) for (_, _, m), n in zip(hyper, norms)])
        sched.step()
    assert all(c[0] < 1.0 and c[1] >= 1.0 and c[2] is None for c in coefs), coefs      # one clips, one does not, one is not asked
    assert [g["lr"] for g in opt.param_groups] == [PAIRS[k][0] * LAMBDAS[k](STEPS) for k in range(3)]
    if guard:
        assert opt.applied_steps == STEPS and opt.skipped_steps == 0
        assert int(opt._state_view("faults", torch.int64)[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("guard,sr", [(False, False), (True, False), (True, True)], ids=["plain", "guarded", "guarded-sr"])
def test_a_step_is_one_launch_per_bucket(monkeypatch, guard, sr):
    from dreamvla_amd import _lib
    lib = _lib.load()
    calls = []
    for name in _lib.SYMBOLS:
        if name.startswith(("dvla_adamw_", "dvla_sumsq_bf16", "dvla_sumsq_f32", "dvla_group_", "dvla_segment_")):
            real = getattr(lib, name)
            monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    red, opt = _make("mixed", guard, True, sr)
    for k in range(2):
        _set_grads(red, _grads3("mixed", k))
        opt.step()
    bf = "dvla_adamw_bf16_sr_clip" if sr else "dvla_adamw_bf16_grouped_clip"
    norm = ["dvla_segment_stats_bf16", "dvla_segment_stats_f32", "dvla_segment_stats_bf16", "dvla_segment_combine", "dvla_group_sumsq"]
    assert calls == (norm + [bf, "dvla_adamw_f32_master_grouped_clip", bf]) * 2      # and no dvla_sumsq_* pass


# ---- 2. the norms ---------------------------------------------------------------------------------------------------------------------------
def _f64_sums(red, group_of, n_groups=3):
    sums = [0.0] * n_groups
    for i, p in enumerate(red.params):
        sums[group_of[i]] += float((red.grad_of(p).double() ** 2).sum())
    return sums


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_group_norms_against_float64_and_twice_the_same_bits(mode):
    red, opt = _make(mode)
    _set_grads(red, _grads3(mode, 0))
    opt.step()
    norms, sums, total = opt.group_grad_norms(), opt.group_grad_sumsq(), opt.grad_norm()
    assert norms.shape == (3,) and norms.dtype == F32 and norms.is_cuda and sums.shape == (3,)
    want = _f64_sums(red, GROUP_OF3)
    for g in range(3):
        err = abs(float(norms[g]) - want[g] ** 0.5) / want[g] ** 0.5
        print(f"{mode}: group {g} norm {float(norms[g]):.9g}, float64 {want[g] ** 0.5:.9g}, relative error {err:.3g} (bound {SUM_BOUND:.3g})")
        assert err <= SUM_BOUND
        assert abs(float(sums[g]) - want[g]) <= SUM_BOUND * want[g]
    err = abs(float(total) - sum(want) ** 0.5) / sum(want) ** 0.5
    print(f"{mode}: total norm relative error {err:.3g}")
    assert err <= SUM_BOUND + 2 * U                  # + the two fp32 additions over the three groups
    chain = (sums[0] + sums[1]) + sums[2]            # the groups' sums added in group order, in fp32
    assert torch.equal(_bits(total.reshape(1)), _bits(chain.sqrt().reshape(1)))
    # the same gradient again: the same bits, and the accessors hand out copies
    keep = _bits(sums).clone()
    _set_grads(red, _grads3(mode, 0))
    opt.step()
    assert torch.equal(_bits(opt.group_grad_sumsq()), keep) and torch.equal(_bits(opt.grad_norm().reshape(1)), _bits(total.reshape(1)))
    _set_grads(red, _grads3(mode, 1))
    opt.step()
    assert torch.equal(_bits(sums), keep) and not torch.equal(_bits(opt.group_grad_sumsq()), keep)


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_a_groups_norm_does_not_depend_on_the_bucket_layout(mode, guard):
    """the same parameters and gradients in three buckets and in one: the same bits, guarded (dvla_step_verdict adds the groups'
    sums) or not (dvla_group_sumsq does)"""
    out = []
    for init in (_init3(mode), [[p for g in _init3(mode) for p in g]]):
        red, opt = _make(mode, guard=guard, init=init)
        assert len(red.buckets) == len(init)
        _set_grads(red, _grads3(mode, 0))
        opt.step()
        out.append((_bits(opt.group_grad_sumsq()).clone(), _bits(opt.grad_norm().reshape(1)).clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 3. isolation and degenerate groups -------------------------------------------------------------------------------------------------
def _poison_group_1(grads, value=float("nan")):
    grads = [g.clone() for g in grads]
    grads[3].view(-1)[1] = value                     # the 3-element parameter of group 1: bucket 0's ragged tail
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_nan_in_one_groups_gradient_unguarded_stays_in_that_group(mode):
    runs = []
    for poisoned in (False, True):
        red, opt = _make(mode, ema=True)
        _set_grads(red, _grads3(mode, 0))
        opt.step()
        g = _grads3(mode, 1)
        _set_grads(red, _poison_group_1(g) if poisoned else g)
        opt.step()
        runs.append((_snap(red, opt), opt.group_grad_norms().tolist()))
    (clean, clean_norms), (dirty, dirty_norms) = runs
    for i, g in enumerate(GROUP_OF3):
        if g != 1:
            for key in clean[i]:
                assert torch.equal(clean[i][key], dirty[i][key]), f"parameter {i} (group {g}), {key}: a NaN of group 1 got here"
    assert math.isnan(dirty_norms[1]) and dirty_norms[0] == clean_norms[0] and dirty_norms[2] == clean_norms[2]
    # the poisoned element itself is NaN -- the NaN was not dropped either.  (Its neighbours are finite: as in the one-group
    # kernels a NaN norm gives the coefficient 1, `c < 1 ? c : 1`.)
    assert bool(red.params[3].data.float().isnan()[1]) and not any(bool(p.data.float().isnan().any()) for p in red.params[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,sr", [(m, s) for m in MODES for s in (False, True) if not (s and m == "f32")])
def test_a_nan_in_one_group_guarded_skips_the_step_for_every_group(mode, sr):
    red, opt = _make(mode, guard=True, ema=True, sr=sr)
    before = _snap(red, opt)
    _set_grads(red, _poison_group_1(_grads3(mode, 0)))
    opt.step()
    after = _snap(red, opt)
    # (the bf16 shadows of fp32 masters are published by the first step whether it is applied or not: they are the masters' cast)
    assert all(torch.equal(a[key], b[key]) for a, b in zip(before, after) for key in a if key != "sh"), "a skipped step moved a buffer"
    assert all(torch.equal(s["sh"], s["p"].to(BF)) for s in opt.flat if "sh" in s)
    with pytest.warns(RuntimeWarning, match=r"parameter group\(s\) 1; parameter_stats\(\"grad\"\)\[\"grad_nonfinite\"\]"):
        assert opt.skipped_steps == 1 and opt.applied_steps == 0
    h = opt.health()
    assert "skipped_bucket_norms" not in h and h["skipped_group_norms"].shape == (3,)
    assert [math.isfinite(x) for x in h["skipped_group_norms"].tolist()] == [True, False, True]
    assert int(h["last_ok"]) == 0 and int(h["last_skipped_step"]) == 1 and math.isnan(float(opt.grad_norm()))
    assert int(opt.parameter_stats("grad")["grad_nonfinite"][3]) == 1
    # the next step is the first applied one: the twins at step 1
    hyper = _read_hyper(opt)
    buffers = _buffers(opt)
    _set_grads(red, _grads3(mode, 1))
    opt.step()
    _assert_every_parameter_is_its_twins(red, opt, buffers, hyper, 1, GROUP_OF3)
    assert opt.applied_steps == 1 and opt.skipped_steps == 1 and int(opt.health()["last_ok"]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_group_whose_gradient_is_all_zero_sees_weight_decay_only(mode):
    """clipped on a norm of 0: the coefficient is min(1, m / 1e-6) = 1, nothing divides by zero"""
    red, opt = _make(mode, clips=(0.1, 1e3, 0.1))
    grads = [g.clone() for g in _grads3(mode, 0)]
    grads[4].zero_()                                 # the one parameter of group 2
    p0 = red.params[4].data.clone()
    hyper, before = _read_hyper(opt), _buffers(opt)
    _set_grads(red, grads)
    opt.step()
    assert opt.group_grad_sumsq().tolist()[2] == 0.0
    _assert_every_parameter_is_its_twins(red, opt, before, hyper, 1, GROUP_OF3)
    snap = _snap(red, opt)[4]
    assert not bool(snap["m"].any()) and not bool(snap["v"].any()) and bool(red.params[4].data.float().isfinite().all())
    lr, wd = PAIRS[2]
    if red.params[4].dtype == F32:                   # the master kernel: p * (float)(1 - lr wd), then + step_size * (0 / eps)
        assert torch.equal(red.params[4].data, p0 * (1.0 - lr * wd))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_group_of_parameters_the_reducer_never_steps(mode):
    """group 2 is bucket 1's one parameter; the reducer has learned that it receives no gradient: the bucket is not launched, the
    group keeps every bit, its norm is still reported and the other groups are their twins"""
    red, opt = _make(mode)
    red.buckets[1]["expected"][0] = False
    kept = _snap(red, opt)[4]
    for k in range(2):
        hyper, before = _read_hyper(opt), _buffers(opt)
        _set_grads(red, _grads3(mode, k))
        opt.step()
        _assert_every_parameter_is_its_twins(red, opt, before, hyper[:2], k + 1, GROUP_OF3)
    assert all(torch.equal(kept[key], _snap(red, opt)[4][key]) for key in kept)
    want = _f64_sums(red, GROUP_OF3)[2] ** 0.5
    assert abs(opt.group_grad_norms().tolist()[2] - want) <= SUM_BOUND * want


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("mode", MODES)
def test_a_group_that_holds_only_an_empty_parameter(mode, guard):
    """a fourth group whose one parameter has no element (first in bucket 1): its sum is 0, nothing of it is stepped, the verdict
    stays finite and every other parameter is its twin"""
    init = [list(g) for g in _init3(mode)]
    init[1].insert(0, torch.zeros(0, dtype=init[1][0].dtype, device="cuda"))
    group_of = [0, 1, 0, 1, 3, 2, 0]
    red, opt = _make(mode, guard=guard, init=init, group_of=group_of, clips=CLIPS + (0.1,), pairs=PAIRS + [(1e-3, 0.0)])
    assert red.buckets[1]["offsets"] == [0, 0] and red.buckets[1]["flat"].numel() == 3005 and len(opt.param_groups) == 4
    for k in range(2):
        hyper, before = _read_hyper(opt), _buffers(opt)
        grads = _grads3(mode, k)
        _set_grads(red, grads[:4] + [init[1][0]] + grads[4:])
        opt.step()
        _assert_every_parameter_is_its_twins(red, opt, before, hyper, k + 1, group_of)
    assert opt.group_grad_sumsq().tolist()[3] == 0.0 and math.isfinite(float(opt.grad_norm()))
    if guard:
        assert opt.applied_steps == 2 and opt.skipped_steps == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_nan_in_the_alignment_gaps_of_the_gradient_is_never_read(mode):
    """bucket 0 has gaps behind the 1300- and the 5-element parameter (elements 1300 .. 1303 and 1309 .. 1311): with NaN in them
    the norms have the bits they had, and so has every element of every parameter"""
    runs = []
    for poisoned in (False, True):
        red, opt = _make(mode, guard=True)
        for k in range(2):
            _set_grads(red, _grads3(mode, k))
            if poisoned:
                flat = red.buckets[0]["flat"]
                flat[1300:1304] = float("nan")
                flat[1309:1312] = float("nan")
            opt.step()
        runs.append((_snap(red, opt), _bits(opt.group_grad_sumsq()).clone(), opt.applied_steps))
    assert runs[1][2] == 2 and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a[key], b[key]) for a, b in zip(runs[0][0], runs[1][0]) for key in a)


# ---- 4. the fp32-master trajectory against float64 ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fp32_master_trajectory_matches_the_float64_statement_per_group():
    """the bound of tests/test_master_adamw_gpu.py for the global clip (TOL 2e-6 on the scale of the terms, each step evaluated
    from the kernel's own fp32 state), for its 5 steps; the clip coefficient and with it the scale are the group's"""
    red, opt = _make("f32")
    where = {}
    for b, s in zip(red.buckets, opt.flat):
        for p, off in zip(b["params"], b["offsets"]):
            where[_index(red, p)] = (s, slice(off, off + p.numel()))
    n = len(red.params)
    for step in range(1, 6):
        grads = [g.reshape(-1) for g in _grads3("f32", step - 1)]
        p0, m0, v0 = ([where[i][0][key][where[i][1]].double().cpu() for i in range(n)] for key in ("p", "m", "v"))
        hyper = _read_hyper(opt)
        _set_grads(red, _grads3("f32", step - 1))
        opt.step()
        torch.cuda.synchronize()
        p64, m64, v64, sums = group_clip_adamw_f64(p0, [g.cpu() for g in grads], m0, v0, step, GROUP_OF3, hyper, BETAS, EPS)
        got = opt.group_grad_sumsq().tolist()
        bc1 = 1.0 - BETAS[0] ** step
        for i, g in enumerate(GROUP_OF3):
            lr, _, m = hyper[g]
            assert abs(got[g] - sums[g]) <= 1e-6 * sums[g], (got[g], sums[g])
            coef = 1.0 if m is None else min(1.0, m / (sums[g] ** 0.5 + 1e-6))
            gc = grads[i].double().cpu() * coef
            s, sl = where[i]
            _within(s["m"][sl], m64[i], BETAS[0] * m0[i].abs() + (1 - BETAS[0]) * gc.abs(), f"m step {step} parameter {i}")
            _within(s["v"][sl], v64[i], 0.0, f"v step {step} parameter {i}")
            denom = v64[i].sqrt() / (1.0 - BETAS[1] ** step) ** 0.5 + EPS
            _within(s["p"][sl], p64[i], p0[i].abs() + (lr / bc1) * (m64[i] / denom).abs(), f"p step {step} parameter {i}")


# ---- 5. the surface ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_constructor_step_and_accessors_refuse_what_the_mode_cannot_be():
    from dreamvla_amd.optim import FlatAdamW

    def fresh():
        return _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init3("mixed")])

    with pytest.raises(ValueError, match="global clip"):
        FlatAdamW(fresh(), max_grad_norm=0.1, clip="group")
    red = fresh()
    with pytest.raises(ValueError, match="global clip"):
        FlatAdamW(red, max_grad_norm=0.1, clip="group", param_groups=[{"params": list(red.params)}])
    with pytest.raises(ValueError, match='"global" or "group"'):
        FlatAdamW(fresh(), clip="per-group")
    red, opt = _make("mixed", clip="global")
    _set_grads(red, _grads3("mixed", 0))
    opt.step()
    for call in (opt.group_grad_norms, opt.group_grad_sumsq):
        with pytest.raises(RuntimeError, match='clip="group"'):
            call()
    red, opt = _make("mixed", guard=True)
    before = _snap(red, opt)
    _set_grads(red, _grads3("mixed", 0))
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        opt.param_groups[1]["max_grad_norm"] = bad
        with pytest.raises(ValueError, match="group 1 has max_grad_norm"):
            opt.step()
    opt.param_groups[1]["max_grad_norm"] = 1e3
    assert all(torch.equal(a[k], b[k]) for a, b in zip(_snap(red, opt), before) for k in a) and opt.applied_steps == 0
    opt.step()
    assert opt.applied_steps == 1 and opt.skipped_steps == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f32"], ids=["bf16-format", "torch-format"])
def test_max_grad_norm_round_trips_through_the_checkpoint_and_the_run_continues_bit_for_bit(mode):
    red, opt = _make(mode)
    opt.param_groups[0]["max_grad_norm"] = 0.05
    for k in range(2):
        _set_grads(red, _grads3(mode, k))
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert [g["max_grad_norm"] for g in sd["param_groups"]] == [0.05, 1e3, None] and "clip" not in sd
    assert ("state" in sd) == (mode == "f32")
    red2, opt2 = _make(mode, clips=(7.0, 7.0, 7.0))
    for p, q in zip(red2.params, red.params):
        p.data.copy_(q.data)
    opt2.load_state_dict(copy.deepcopy(sd))
    assert [g["max_grad_norm"] for g in opt2.param_groups] == [0.05, 1e3, None]
    for r, o in ((red, opt), (red2, opt2)):
        _set_grads(r, _grads3(mode, 2))
        o.step()
    for a, b in zip(_snap(red, opt), _snap(red2, opt2)):
        assert all(torch.equal(a[key], b[key]) for key in a)
    assert torch.equal(_bits(opt.group_grad_sumsq()), _bits(opt2.group_grad_sumsq()))
    # a checkpoint written without the key leaves the groups as constructed (group 0: the constructor's max_grad_norm)
    for g in sd["param_groups"]:
        del g["max_grad_norm"]
    red3, opt3 = _make(mode, clips=(7.0, 5.0, None))
    opt3.load_state_dict(sd)
    from dreamvla_amd.optim import group_max_norms
    assert group_max_norms(opt3.param_groups, opt3.max_grad_norm) == [7.0, 5.0, None]


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
def test_with_the_global_clip_a_groups_max_grad_norm_key_changes_nothing(guard):
    """clip="global", today's behaviour: the key is carried along and not used"""
    runs = []
    for clips in ((0.1, 1e-9, 1e-9), None):
        from dreamvla_amd.optim import FlatAdamW
        red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init3("mixed")])
        groups = _groups(red, GROUP_OF3, clips) if clips else [{k: v for k, v in g.items() if k != "max_grad_norm"}
                                                                for g in _groups(red, GROUP_OF3)]
        opt = FlatAdamW(red, betas=BETAS, eps=EPS, max_grad_norm=0.1, skip_nonfinite=guard, ema_decay=DECAY, param_groups=groups)
        assert opt.clip == "global" and ("max_grad_norm" in opt.param_groups[1]) == bool(clips)
        snaps = []
        for k in range(3):
            _set_grads(red, _grads3("mixed", k))
            opt.step()
            snaps.append((_snap(red, opt), _bits(opt.grad_norm().reshape(1)).clone()))
        runs.append(snaps)
    for (a, na), (b, nb) in zip(*runs):
        assert torch.equal(na, nb) and all(torch.equal(x[key], y[key]) for x, y in zip(a, b) for key in x)
