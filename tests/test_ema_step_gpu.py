"""GPU: FlatAdamW(ema_decay=...) -- dvla_adamw_*_ema, dvla_adamw_*_ema_guarded, dvla_ema_swap_f32 / dvla_ema_swap_bf16.

Bit for bit throughout (buffers are compared as integers): the step with the EMA IS the step without it, the EMA IS
`ref.lerp_(p.float(), w)` of ATen applied after every step, a skipped step leaves the EMA alone and does not advance its warm-up,
and ema_weights() exchanges the weights and gives them back exactly.  The stand-in buckets, gradients and helpers are those of
tests/test_guarded_step_gpu.py (3015 = 8 * 376 + 7 and 3005 = 8 * 375 + 5 elements: the vector body and the ragged tail of
both kernels)."""
import ctypes
import functools

import pytest
import torch

from tests.test_guarded_step_gpu import (BETAS, BF, EPS, F32, LAYOUT, LR, MODES, NORMS, POISON, WD, _bits, _Buckets, _grads, _init,
                                         _poisoned, _set_grads)

DECAY = 0.999
STEPS = 12
ERR_UNSUPPORTED = -3
KEYS = ("p", "m", "v", "sh")


def _d(decay, warmup, t):
    """the decay of applied step t (1-based) in Python doubles: what dvla_ema_weights rounds 1 - d(t) of to fp32"""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


def _make(mode, max_norm, guard, decay, warmup=False):
    from dreamvla_amd.optim import FlatAdamW
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init(mode)])
    kw = {} if decay is None else {"ema_decay": decay, "ema_warmup": warmup}
    opt = FlatAdamW(red, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm, skip_nonfinite=guard, **kw)
    assert ("ema" in opt.flat[0]) == (decay is not None)
    return red, opt


def _snap(opt, keys=KEYS):
    return [_bits(s[k]).clone() for s in opt.flat for k in keys if k in s]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _plain(mode, max_norm, guard):
    """ema_decay=None over the 12 good gradients: snapshot and norm bits per step (shared, read-only)"""
    red, opt = _make(mode, max_norm, guard, None)
    snaps, norms = [], []
    for k in range(STEPS):
        _set_grads(red, _grads(mode, k))
        opt.step()
        snaps.append(_snap(opt))
        norms.append(_bits(opt.grad_norm()).clone())
    return snaps, norms


@pytest.mark.gpu
@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_step_is_untouched_and_the_ema_is_atens_lerp(mode, max_norm, guard, warmup):
    """Per step: p, m, v, sh and the gradient norm are those of the optimizer without EMA, and the EMA buffer is
    `ref.lerp_(p.float(), 1 - d(t))` (torch, on the GPU) applied to a copy of the initial parameters after every step.  With
    warm-up the 12 weights run from 9/11 down to 9/22: both branches of lerp (w >= 0.5 up to t = 8).
    Float64: after the 12 steps |e - e64| <= 12 * 2^-23 * max(|p|, |e|), e64 the float64 EMA of the stored parameter
    trajectory -- each step rounds twice (the difference, the fma), at most 0.5 + 0.5 ulp of the larger magnitude, and
    d <= 1 contracts earlier error: 12 ulp for 12 steps."""
    want, want_norms = _plain(mode, max_norm, guard)
    red, opt = _make(mode, max_norm, guard, DECAY, warmup)
    ref = [s["p"].float().clone() for s in opt.flat]
    e64 = [r.double() for r in ref]
    assert all(torch.equal(_bits(s["ema"]), _bits(r)) and s["ema"].dtype == F32 for s, r in zip(opt.flat, ref))
    for k in range(STEPS):
        _set_grads(red, _grads(mode, k))
        opt.step()
        assert _same(_snap(opt), want[k]), f"step {k + 1}: the step with the EMA is not the step without it"
        assert torch.equal(_bits(opt.grad_norm()), want_norms[k]), f"grad_norm() of step {k + 1}"
        w = 1.0 - _d(DECAY, warmup, k + 1)
        for bi, (s, r) in enumerate(zip(opt.flat, ref)):
            r.lerp_(s["p"].float(), w)
            e64[bi] += w * (s["p"].double() - e64[bi])
            if not torch.equal(_bits(s["ema"]), _bits(r)):
                i = int((_bits(s["ema"]) != _bits(r)).nonzero()[0])
                raise AssertionError(f"step {k + 1}, bucket {bi}, element {i}: kernel {float(s['ema'][i])!r} "
                                     f"vs ATen {float(r[i])!r} (w = {w!r}, p = {float(s['p'][i])!r})")
    if guard:
        assert opt.applied_steps == STEPS and opt.skipped_steps == 0
    worst = 0.0
    for s, x in zip(opt.flat, e64):
        err = (s["ema"].double() - x).abs()
        bound = STEPS * 2.0 ** -23 * torch.maximum(s["p"].double().abs(), s["ema"].double().abs())
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), f"float64 EMA: worst error / bound {worst}"
    print(f"float64 sanity: worst error / bound = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_skipped_steps_neither_move_the_ema_nor_advance_its_warmup(mode, max_norm):
    """10 steps back to back (nothing between them waits for the device), steps 3 and 4 (a pair) and 8 poisoned; warm-up on, so
    the weight of every applied step depends on the applied count: the end state equals the unguarded run over the 7 good
    gradients only if the kernels picked the weight of the count that was current with steps in flight"""
    bad = {3: ("first", "nan"), 4: ("last_tail", "inf"), 8: ("first", "inf")}
    seq = [_poisoned(_grads(mode, k), *[bad[k + 1][0], POISON[bad[k + 1][1]]]) if k + 1 in bad else _grads(mode, k)
           for k in range(10)]
    good = [k for k in range(10) if k + 1 not in bad]
    red, opt = _make(mode, max_norm, True, DECAY, True)
    keys = KEYS + ("ema",)
    snaps = []
    for g in seq:
        _set_grads(red, g)
        opt.step()
        snaps.append(_snap(opt, keys))
    for k in bad:
        assert _same(snaps[k - 1], snaps[k - 2]), f"skipped step {k} touched a buffer"
    red2, opt2 = _make(mode, max_norm, False, DECAY, True)
    for k in good:
        _set_grads(red2, _grads(mode, k))
        opt2.step()
    assert _same(snaps[-1], _snap(opt2, keys)), "not the unguarded run over the 7 good gradients: wrong weight index"
    assert opt.applied_steps == 7 and opt.skipped_steps == 3
    assert int(opt._state_view("faults", torch.int64)[0]) == 0


BIG = 4096 * 2048 + 2053          # the grid cap of 4096 blocks x 256 threads x 8 elements wraps, and a ragged tail of 5 remains


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("dtype,max_norm", [(F32, 0.1), (BF, None)], ids=["f32-clip", "bf16-noclip"])
def test_grid_stride_loop_and_tail_on_a_bucket_beyond_the_grid_cap(dtype, max_norm, guard):
    """The fp32 bucket the grid cap wraps on.  And a bf16 one of the same length, unclipped: dvla_adamw_bf16's element function
    is plain C++ whose products the compiler is free to fuse, and a twin that fuses another one of them differs from it in
    about 2 elements per million and step (one bf16 ulp of exp_avg_sq) -- invisible on 6000 elements, 30 expected here."""
    from dreamvla_amd import ops
    from dreamvla_amd.optim import FlatAdamW
    gen = torch.Generator(device="cuda").manual_seed(5)
    p0 = (torch.randn(BIG, generator=gen, device="cuda") * 0.5).to(dtype)
    grads = [(torch.randn(BIG, generator=gen, device="cuda") * 0.3).to(dtype) for _ in range(2)]
    runs = {}
    for decay in (None, DECAY):
        red = _Buckets([[torch.nn.Parameter(p0.clone())]])
        kw = {} if decay is None else {"ema_decay": decay, "ema_warmup": True}
        opt = FlatAdamW(red, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm, skip_nonfinite=guard, **kw)
        assert opt.flat[0]["p"].numel() == BIG and BIG % 8 == 5 and BIG // 8 > 4096 * 256
        ref = p0.float().clone()
        snaps = []
        for k, g in enumerate(grads):
            _set_grads(red, [g])
            opt.step()
            snaps.append(_snap(opt))
            if decay is not None:
                ref.lerp_(opt.flat[0]["p"].float(), 1.0 - _d(decay, True, k + 1))
                assert torch.equal(_bits(opt.flat[0]["ema"]), _bits(ref)), f"step {k + 1}"
        runs[decay] = snaps
    for k, (a, b) in enumerate(zip(runs[None], runs[DECAY])):
        for name, x, y in zip(KEYS, a, b):
            assert torch.equal(x, y), f"step {k + 1}: {int((x != y).sum())} elements of {name} differ from the step without EMA"
    s = opt.flat[0]
    before = {k: _bits(s[k]).clone() for k in KEYS + ("ema",) if k in s}
    with opt.ema_weights():
        if dtype == F32:
            assert torch.equal(_bits(s["p"]), before["ema"]) and torch.equal(_bits(s["ema"]), before["p"])
            assert torch.equal(_bits(s["sh"]), _bits(ops.cast_to(s["p"], BF)))
        else:
            assert torch.equal(_bits(s["p"]), _bits(before["ema"].view(F32).to(BF))) and torch.equal(_bits(s["ema"]), before["ema"])
    assert all(torch.equal(_bits(s[k]), b) for k, b in before.items())


@pytest.mark.gpu
def test_misaligned_ema_is_unsupported_and_zero_elements_is_ok():
    from dreamvla_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(256, dtype=F32, device="cuda")
    state = torch.zeros(ctypes.sizeof(_lib.StepState), dtype=torch.uint8, device="cuda")
    p, st = buf.data_ptr(), state.data_ptr()
    assert p % 16 == 0 and st % 16 == 0
    w = (ctypes.c_float * _lib.STEP_MAX_CANDIDATES)(*([0.001] * _lib.STEP_MAX_CANDIDATES))
    hp = (LR, BETAS[0], BETAS[1], EPS, WD)
    stream = torch.cuda.current_stream().cuda_stream
    for n, ema, rc in ((8, p + 4, ERR_UNSUPPORTED), (0, p, 0)):       # neither launches anything
        assert lib.dvla_adamw_f32_master_ema(p, p, p, p, p, ema, n, *hp, 1, None, 0.0, 0.001, stream) == rc
        assert lib.dvla_adamw_bf16_ema(p, p, p, p, ema, n, *hp, 1, None, 0.0, 0.001, stream) == rc
        assert lib.dvla_adamw_f32_master_ema_guarded(p, p, p, p, p, ema, n, *hp, 0.1, st, w, 1, stream) == rc
        assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, ema, n, *hp, 0.1, st, w, 1, stream) == rc
        assert lib.dvla_ema_swap_f32(p, ema, p, n, stream) == rc
        assert lib.dvla_ema_swap_bf16(p, ema, p, n, 0, stream) == rc
    torch.cuda.synchronize()
    assert not bool(buf.any())


class _Boom(Exception):
    pass


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [3, 0], ids=["after3", "before_any_step"])
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("mode", MODES)
def test_ema_weights_swaps_in_and_gives_the_training_weights_back(mode, guard, steps):
    from dreamvla_amd import ops
    red, opt = _make(mode, 0.1, guard, DECAY, True)
    for k in range(steps):
        _set_grads(red, _grads(mode, k))
        opt.step()
    keys = ("p", "ema", "m", "v")
    before = [{k: _bits(s[k]).clone() for k in keys + ("sh",) if k in s} for s in opt.flat]
    if steps:      # the EMA has moved away from the parameters: the exchange below is visible
        assert all(not torch.equal(s["p"].float(), s["ema"]) for s in opt.flat)

    def inside():
        for s, b in zip(opt.flat, before):
            if "sh" in s:
                assert torch.equal(_bits(s["p"]), b["ema"]), "fp32: the flat parameters are not the EMA's former bits"
                assert torch.equal(_bits(s["ema"]), b["p"]), "fp32: the EMA buffer does not hold the former parameters"
                assert torch.equal(_bits(s["sh"]), _bits(ops.cast_to(s["p"], BF))), "shadow != dvla_cast_f32_to_bf16(p)"
                continue
            assert torch.equal(_bits(s["p"]), _bits(b["ema"].view(F32).to(BF))), "bf16: the parameters are not bf16_rne(EMA)"
            assert torch.equal(_bits(s["ema"]), b["ema"]), "bf16: the EMA was modified"
        # the parameters themselves (views into the flat buffers) show the EMA
        lay = opt._layout()
        for s, b, l in zip(opt.flat, before, lay):
            for i, off, shape in l:
                n = red.params[i].numel()
                assert torch.equal(red.params[i].detach().float().reshape(-1), b["ema"].view(F32)[off:off + n]
                                   if "sh" in s else b["ema"].view(F32)[off:off + n].to(BF).float())

    def outside():
        for s, b in zip(opt.flat, before):
            for k in keys:
                assert torch.equal(_bits(s[k]), b[k]), f"{k} did not come back bit for bit"
            if "sh" in s:
                # the shadow buffer is first written by the first step; from then on it comes back bit for bit as well.  In
                # either case it is the shadow of the parameters that are back
                assert torch.equal(_bits(s["sh"]), _bits(ops.cast_to(s["p"], BF)))
                assert steps == 0 or torch.equal(_bits(s["sh"]), b["sh"])

    with opt.ema_weights():
        inside()
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with opt.ema_weights():
                pass
        inside()                     # neither refusal disturbed anything
    outside()
    with pytest.raises(_Boom):
        with opt.ema_weights():
            inside()
            raise _Boom()
    outside()
    assert opt._ema_active is False
    # and training goes on: the next step is the step of an optimizer that never swapped
    red2, opt2 = _make(mode, 0.1, guard, DECAY, True)
    for k in range(steps + 1):
        _set_grads(red2, _grads(mode, k))
        opt2.step()
    _set_grads(red, _grads(mode, steps))
    opt.step()
    assert _same(_snap(opt, KEYS + ("ema",)), _snap(opt2, KEYS + ("ema",)))


@pytest.mark.gpu
def test_the_model_computes_on_the_ema_inside_the_context(monkeypatch):
    """dreamvla_amd.nn.Mlp on fp32 masters (weights through ops.shadow, fp32 biases read as they are), the real reducer, three
    training steps.  The forward inside ema_weights() is the forward of a fresh Mlp loaded with ema_model_state_dict(); no
    fp32 -> bf16 cast is launched for a weight inside the context (the swap kernel wrote the shadows), nor after it."""
    from dreamvla_amd import _lib, ops
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.nn import Mlp
    from dreamvla_amd.optim import FlatAdamW
    torch.manual_seed(3)
    mlp = Mlp(64, 256).cuda()
    assert all(p.dtype == F32 for p in mlp.parameters())
    red = GradBucketReducer(list(mlp.parameters()))
    opt = FlatAdamW(red, lr=1e-2, weight_decay=WD, max_grad_norm=1.0, ema_decay=0.9)
    assert opt.master_mode and len(red.buckets) == 1
    x = torch.randn(40, 64, device="cuda").to(BF)
    for _ in range(3):
        opt.zero_grad()
        mlp(x).float().pow(2).mean().backward()
        red.finish()
        opt.step()
    sd = opt.ema_model_state_dict(mlp)
    assert list(sd) == list(mlp.state_dict()) and all(v.dtype == F32 for v in sd.values())
    assert all(not torch.equal(sd[n], p.detach()) for n, p in mlp.named_parameters())
    fresh = Mlp(64, 256).cuda()
    fresh.load_state_dict(sd)
    lib = _lib.load()
    casts = []
    real = lib.dvla_cast_f32_to_bf16
    monkeypatch.setattr(lib, "dvla_cast_f32_to_bf16", lambda *a: (casts.append(a), real(*a))[1])
    weights = [mlp.fc1.weight, mlp.fc2.weight]
    s, b = opt.flat[0], red.buckets[0]
    off = {id(p): o for p, o in zip(b["params"], b["offsets"])}

    def served_from_the_flat_shadow():
        for w in weights:
            o = off[id(w)]
            assert ops.shadow_is_current(w, s["sh"][o:o + w.numel()].view(w.shape))
            assert ops.shadow(w).data_ptr() == s["sh"].data_ptr() + 2 * o

    with torch.no_grad():
        y_train = mlp(x)
        with opt.ema_weights():
            served_from_the_flat_shadow()
            y_ema = mlp(x)
            served_from_the_flat_shadow()
        served_from_the_flat_shadow()
        y_back = mlp(x)
        assert casts == [], "a cast was launched for a master whose shadow the swap kernel had written"
        y_fresh = fresh(x)
    assert len(casts) == 2               # (the fresh Mlp's two weights: the counter does count)
    assert torch.equal(_bits(y_ema), _bits(y_fresh))
    assert torch.equal(_bits(y_back), _bits(y_train))
    assert not torch.equal(_bits(y_ema), _bits(y_train))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_checkpoints(mode):
    red, opt = _make(mode, 0.1, False, DECAY, True)
    red0, opt0 = _make(mode, 0.1, False, None)
    for k in range(3):
        for r, o in ((red, opt), (red0, opt0)):
            _set_grads(r, _grads(mode, k))
            o.step()
    # the optimizer's own checkpoint keeps its format
    sd, sd0 = opt.state_dict(), opt0.state_dict()
    assert list(sd) == list(sd0)
    if opt.master_mode:
        assert list(sd["state"]) == list(sd0["state"]) and all(list(sd["state"][i]) == ["step", "exp_avg", "exp_avg_sq"] for i in sd["state"])
        assert list(sd["param_groups"][0]) == list(sd0["param_groups"][0])
        pt = [torch.nn.Parameter(p.detach().clone()) for p in red.params]
        opt_t = torch.optim.AdamW(pt, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        opt_t.load_state_dict(sd)
        assert all(float(opt_t.state[p]["step"]) == 3.0 for p in pt)
    # the EMA's checkpoint
    esd = opt.ema_state_dict()
    assert list(esd) == ["decay", "warmup", "ema"] and esd["decay"] == DECAY and esd["warmup"] is True
    assert list(esd["ema"]) == list(range(len(red.params)))
    for i, p in enumerate(red.params):
        assert esd["ema"][i].dtype == F32 and esd["ema"][i].shape == p.shape
    red2, opt2 = _make(mode, 0.1, False, DECAY, True)
    assert not _same(_snap(opt2, ("ema",)), _snap(opt, ("ema",)))
    opt2.load_ema_state_dict(esd)
    assert _same(_snap(opt2, ("ema",)), _snap(opt, ("ema",)))
    esd["ema"][0] = esd["ema"][0][:-1]
    with pytest.raises(ValueError, match="shape"):
        opt2.load_ema_state_dict(esd)
    # the clones do not alias the buffers
    opt.ema_state_dict()["ema"][1].zero_()
    assert _same(_snap(opt2, ("ema",)), _snap(opt, ("ema",)))
    # ema_reset
    assert all(not torch.equal(s["ema"], s["p"].float()) for s in opt.flat)
    opt.ema_reset()
    assert all(torch.equal(_bits(s["ema"]), _bits(s["p"].float())) for s in opt.flat)
    # without ema_decay the methods refuse
    for call in (opt0.ema_reset, opt0.ema_state_dict, lambda: opt0.load_ema_state_dict(esd), lambda: opt0.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()
    assert all("ema" not in s for s in opt0.flat)
