"""GPU: FlatAdamW(param_groups=[...]) -- dvla_adamw_bf16_grouped / dvla_adamw_f32_master_grouped.

The oracle is the one-group path that was there before.  AdamW is element-wise once the (global) clip norm is known, so a
parameter of group g must come out of the grouped step exactly -- bit for bit, buffers are compared as integers -- as it comes
out of a one-group optimizer with (lr_g, weight_decay_g) on the same gradients.  The stand-in buckets and helpers are those of
tests/test_guarded_step_gpu.py; the layout with group boundaries inside a wave, a one-vector parameter and a tail parameter
is this file's own (LAYOUT2)."""
import copy
import ctypes
import functools

import pytest
import torch

from tests.test_guarded_step_gpu import (BETAS, BF, EPS, F32, LAYOUT, LR, MODES, NORMS, POISON, WD, _bits, _Buckets, _grads, _init,
                                         _poisoned, _set_grads)

DECAY = 0.999
KEYS = ("p", "m", "v", "sh", "ema")
ERR_ARG, ERR_UNSUPPORTED = -1, -3

# bucket 0: 1300 | 5 | 1711 | 3 elements at offsets 0, 1304, 1312, 3024 in groups 0, 1, 0, 1 -- the first boundary falls inside a
# wave (vector 163), the 5-element parameter is one vector of its own, and the 3-element one is the bucket's ragged tail
# (3027 = 8 * 378 + 3) in another group than the vector before it.  bucket 1: 3005 = 8 * 375 + 5 elements in group 2.
SHAPES2 = [[(1300,), (5,), (1711,), (3,)], [(5, 601)]]
LAYOUT2 = {"bf16": [BF, BF], "f32": [F32, F32], "mixed": [BF, F32]}
GROUP_OF2 = [0, 1, 0, 1, 2]
PAIRS = [(1e-3, 1e-2), (3e-4, 0.0), (2e-3, 0.05)]          # (lr, weight_decay) per group; one without decay
LAMBDAS = [lambda e: 1.0 / (1 + e), lambda e: 0.5 ** e, lambda e: 1.0 + 0.25 * e]
STEPS = 4


@functools.lru_cache(maxsize=None)
def _init2(mode):
    gen = torch.Generator().manual_seed(12)
    return [[(torch.randn(s, generator=gen) * 0.5).to(dt).cuda() for s in shapes] for dt, shapes in zip(LAYOUT2[mode], SHAPES2)]


@functools.lru_cache(maxsize=None)
def _grads2(mode, k):
    gen = torch.Generator().manual_seed(2000 + k)
    return [(torch.randn(s, generator=gen) * 0.3).to(dt).cuda() for dt, shapes in zip(LAYOUT2[mode], SHAPES2) for s in shapes]


def _kw(max_norm, guard, ema):
    kw = dict(betas=BETAS, eps=EPS, max_grad_norm=max_norm, skip_nonfinite=guard)
    if ema:
        kw.update(ema_decay=DECAY, ema_warmup=True)
    return kw


def _make(init, group_of, pairs, pair, max_norm, guard, ema):
    """pair None: the grouped optimizer (parameter i in group group_of[i] with pairs[group_of[i]]); pair k: the one-group
    optimizer with pairs[k] over the same parameters"""
    from dreamvla_amd.optim import FlatAdamW
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in init])
    if pair is not None:
        return red, FlatAdamW(red, lr=pairs[pair][0], weight_decay=pairs[pair][1], **_kw(max_norm, guard, ema))
    groups = [{"params": [p for p, g in zip(red.params, group_of) if g == k], "lr": lr, "weight_decay": wd}
              for k, (lr, wd) in enumerate(pairs)]
    opt = FlatAdamW(red, **_kw(max_norm, guard, ema), param_groups=groups)
    assert len(opt.param_groups) == len(pairs)
    return red, opt


def _snap(red, opt):
    """per parameter (reducer.params order): the bits of its slice of every buffer"""
    index = {id(p): i for i, p in enumerate(red.params)}
    out = [None] * len(red.params)
    for b, s in zip(red.buckets, opt.flat):
        for p, off in zip(b["params"], b["offsets"]):
            out[index[id(p)]] = {k: _bits(s[k][off:off + p.numel()]).clone() for k in KEYS if k in s}
    return out


def _trajectory(init, grads, group_of, pairs, pair, max_norm, guard, ema, lambdas=None):
    """-> per step (per-parameter snapshots, norm bits)"""
    red, opt = _make(init, group_of, pairs, pair, max_norm, guard, ema)
    sched = None
    if lambdas is not None:
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambdas if pair is None else lambdas[pair])
    out = []
    for g in grads:
        _set_grads(red, g)
        opt.step()
        out.append((_snap(red, opt), _bits(opt.grad_norm()).clone()))
        if sched is not None:
            sched.step()
    if guard:
        assert opt.applied_steps == len(grads) and opt.skipped_steps == 0
    return out


def _assert_each_parameter_is_its_pairs(got, refs, group_of, with_norm=True):
    for k, (snaps, norm) in enumerate(got):
        for i, g in enumerate(group_of):
            want = refs[g][k][0][i]
            assert sorted(snaps[i]) == sorted(want)
            for key in want:
                assert torch.equal(snaps[i][key], want[key]), \
                    f"step {k + 1}, parameter {i} (group {g}): {int((snaps[i][key] != want[key]).sum())} elements of {key} differ"
        if with_norm:
            assert torch.equal(norm, refs[0][k][1]), f"grad_norm() of step {k + 1}"


# ---- 1. the same hyper-parameters in two groups: the one-group optimizer ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_group(mode, max_norm, guard, ema):
    return _trajectory(_init(mode), [_grads(mode, k) for k in range(STEPS)], None, [(LR, WD)], 0, max_norm, guard, ema)


@pytest.mark.gpu
@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_two_groups_with_the_same_hyper_parameters_are_the_one_group_optimizer(mode, max_norm, guard, ema):
    assert [len(shapes) for _, shapes in LAYOUT[mode]] == [2, 1]
    got = _trajectory(_init(mode), [_grads(mode, k) for k in range(STEPS)], [0, 1, 0], [(LR, WD), (LR, WD)], None, max_norm, guard, ema)
    ref = _one_group(mode, max_norm, guard, ema)
    # (the unguarded step computes the norm only when it clips)
    _assert_each_parameter_is_its_pairs(got, [ref, ref], [0, 1, 0], with_norm=guard or max_norm is not None)


@pytest.mark.gpu
def test_one_group_given_as_a_list_takes_the_one_group_path():
    from dreamvla_amd.optim import FlatAdamW
    mode = "mixed"
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init(mode)])
    opt = FlatAdamW(red, lr=LR, weight_decay=WD, **_kw(0.1, False, False), param_groups=[{"params": list(red.params)}])
    assert len(opt.param_groups) == 1
    for k in range(2):
        _set_grads(red, _grads(mode, k))
        opt.step()
    assert opt._group_maps == {}
    ref = _one_group(mode, 0.1, False, False)
    assert all(torch.equal(a[key], b[key]) for a, b in zip(_snap(red, opt), ref[1][0]) for key in b)
    assert list(opt.state_dict()["param_groups"][0]["params"]) == [0, 1, 2]


# ---- 2. different hyper-parameters, scheduled ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_run(mode, max_norm, guard, ema, pair, scheduled):
    return _trajectory(_init2(mode), [_grads2(mode, k) for k in range(STEPS)], GROUP_OF2, PAIRS, pair, max_norm, guard, ema,
                       LAMBDAS if scheduled else None)


@pytest.mark.gpu
@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_every_parameter_is_stepped_as_the_one_group_optimizer_of_its_pair_steps_it(mode, max_norm, guard, ema):
    """three (lr, weight_decay) pairs, the lrs rewritten every step by LambdaLR with one lambda per group"""
    from dreamvla_amd.optim import build_group_map
    red, opt = _make(_init2(mode), GROUP_OF2, PAIRS, None, max_norm, guard, ema)
    assert [b["flat"].numel() for b in red.buckets] == [3027, 3005] and red.buckets[0]["offsets"] == [0, 1304, 1312, 3024]
    m = opt._group_map(0)
    assert m.is_cuda and m.dtype == torch.uint8 and opt._group_map(0) is m          # cached
    assert torch.equal(m.cpu(), build_group_map([0, 1304, 1312, 3024], [1300, 5, 1711, 3], 3027, [0, 1, 0, 1], [True] * 4, 3))
    assert m.cpu().tolist() == [0] * 163 + [1] + [0] * 214 + [1] and set(opt._group_map(1).cpu().tolist()) == {2}
    got = _pair_run(mode, max_norm, guard, ema, None, True)
    refs = [_pair_run(mode, max_norm, guard, ema, k, True) for k in range(3)]
    _assert_each_parameter_is_its_pairs(got, refs, GROUP_OF2, with_norm=guard or max_norm is not None)
    # the schedule did move every group's lr, each by its own lambda
    sched = torch.optim.lr_scheduler.LambdaLR(opt, LAMBDAS)
    _set_grads(red, _grads2(mode, 0))
    opt.step()
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [PAIRS[k][0] * LAMBDAS[k](1) for k in range(3)]
    # and the groups do differ: the same parameter under another pair is another parameter
    assert not torch.equal(refs[0][-1][0][1]["p"], refs[1][-1][0][1]["p"])


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
def test_a_grouped_step_is_one_launch_per_bucket(monkeypatch, guard):
    """whatever the number of groups: the grouped entry point once per bucket and none of the one-group entry points"""
    from dreamvla_amd import _lib
    lib = _lib.load()
    calls = []
    for name in _lib.SYMBOLS:
        if name.startswith("dvla_adamw_"):
            real = getattr(lib, name)
            monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    red, opt = _make(_init2("mixed"), GROUP_OF2, PAIRS, None, 0.1, guard, True)
    for k in range(2):
        _set_grads(red, _grads2("mixed", k))
        opt.step()
    assert calls == ["dvla_adamw_bf16_grouped", "dvla_adamw_f32_master_grouped"] * 2


# ---- 3. beyond the grid cap ---------------------------------------------------------------------------------------------------------
BIG_SIZES = [1000003 + 16 * i for i in range(9)]            # none a multiple of 8; 9 000 603 elements > 4096 * 256 * 8
BIG_GROUP_OF = [0, 1, 2] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,max_norm", [(F32, 0.1), (BF, None)], ids=["f32-clip", "bf16-noclip"])
def test_grid_stride_loop_and_bf16_arithmetic_on_a_bucket_beyond_the_grid_cap(dtype, max_norm):
    """The grid of 4096 blocks wraps, and -- bf16 -- nine million elements go through an element function whose roundings are
    written out to be those the compiler chose for dvla_adamw_bf16: one product fused differently shows as about 2 elements per
    million and step one bf16 ulp off."""
    gen = torch.Generator(device="cuda").manual_seed(6)
    init = [[(torch.randn(n, generator=gen, device="cuda") * 0.5).to(dtype) for n in BIG_SIZES]]
    grads = [[(torch.randn(n, generator=gen, device="cuda") * 0.3).to(dtype) for n in BIG_SIZES] for _ in range(2)]
    red, opt = _make(init, BIG_GROUP_OF, PAIRS, None, max_norm, False, False)
    total = red.buckets[0]["flat"].numel()
    assert total // 8 > 4096 * 256 and total % 8 == 3
    del red, opt
    got = _trajectory(init, grads, BIG_GROUP_OF, PAIRS, None, max_norm, False, False)
    refs = [_trajectory(init, grads, BIG_GROUP_OF, PAIRS, k, max_norm, False, False) for k in range(3)]
    _assert_each_parameter_is_its_pairs(got, refs, BIG_GROUP_OF, with_norm=max_norm is not None)


# ---- 4. the guard ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
@pytest.mark.parametrize("where", ["first", "last_tail"])
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_a_poisoned_step_in_the_middle_changes_nothing_and_does_not_count(mode, max_norm, where):
    """g1 g2* g3 g4 g5* g6 back to back (nothing between the steps waits for the device), EMA with warm-up on: the grouped guarded
    run ends where the grouped unguarded run over g1 g3 g4 g6 ends only if every launch picked the scalars -- the groups' step
    sizes among them -- and the EMA weight of the applied count that was current with steps in flight"""
    good = [0, 2, 3, 5]
    seq = [_grads2(mode, k) if k in good else _poisoned(_grads2(mode, k), where, POISON["nan" if k == 1 else "inf"]) for k in range(6)]
    red, opt = _make(_init2(mode), GROUP_OF2, PAIRS, None, max_norm, True, True)
    snaps = []
    for g in seq:
        _set_grads(red, g)
        opt.step()
        snaps.append(_snap(red, opt))
    for k in (1, 4):
        assert all(torch.equal(a[key], b[key]) for a, b in zip(snaps[k], snaps[k - 1]) for key in a), f"skipped step {k + 1} moved a buffer"
    red2, opt2 = _make(_init2(mode), GROUP_OF2, PAIRS, None, max_norm, False, True)
    for j, k in enumerate(good):
        _set_grads(red2, _grads2(mode, k))
        opt2.step()
        want = _snap(red2, opt2)
        at = k          # the guarded run's snapshot after gradient k
        for i, (a, b) in enumerate(zip(snaps[at], want)):
            for key in b:
                assert torch.equal(a[key], b[key]), f"after good step {j + 1}, parameter {i}, {key}"
    h = opt.health()
    assert int(h["applied"]) == 4 and int(h["skipped"]) == 2 and int(h["last_ok"]) == 1 and int(h["last_skipped_step"]) == 5
    assert opt.applied_steps == 4 and opt.skipped_steps == 2
    assert int(opt._state_view("faults", torch.int64)[0]) == 0


# ---- 5. a parameter the step leaves alone ---------------------------------------------------------------------------------------------
SHAPES5 = [[(1300,), (40,), (1711,)]]
GROUP_OF5 = [0, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_an_unstepped_parameter_between_two_groups_keeps_every_bit(dtype, guard):
    """two steps with every parameter stepped, then the reducer learns that parameter 1 receives no gradient (the cached map is
    rebuilt), two more: parameter 1 keeps p, m, v, shadow and EMA of step 2 although its gradient slice is not zero, and its
    neighbours -- of two different groups -- are those of their one-group runs (which skip it by launching per range)"""
    gen = torch.Generator().manual_seed(13)
    init = [[(torch.randn(s, generator=gen) * 0.5).to(dtype).cuda() for s in SHAPES5[0]]]
    grads = [[(torch.randn(s, generator=gen) * 0.3).to(dtype).cuda() for s in SHAPES5[0]] for _ in range(4)]

    def run(pair):
        red, opt = _make(init, GROUP_OF5, PAIRS[:2], pair, 0.1, guard, True)
        snaps = []
        for k, g in enumerate(grads):
            if k == 2:
                red.buckets[0]["expected"][1] = False
            _set_grads(red, g)
            opt.step()
            snaps.append(_snap(red, opt))
        return red, opt, snaps

    red, opt, got = run(None)
    assert opt._group_maps[0][0] == (True, False, True)
    assert opt._group_map(0).cpu().tolist() == [0] * 163 + [255] * 5 + [1] * 214
    assert red.buckets[0]["flat"].numel() % 8 == 7
    for k in (2, 3):
        for key in got[1][1]:
            assert torch.equal(got[k][1][key], got[1][1][key]), f"step {k + 1}: {key} of the unstepped parameter moved"
    assert bool(red.grad_of(red.params[1]).any())
    refs = [run(k)[2] for k in range(2)]
    for k in range(4):
        for i in (0, 2):
            for key in got[k][i]:
                assert torch.equal(got[k][i][key], refs[GROUP_OF5[i]][k][i][key]), f"step {k + 1}, parameter {i}, {key}"


# ---- 6. torch.optim.AdamW with the same groups ------------------------------------------------------------------------------------------
ORDER6 = [[4, 1, 3], [2, 0]]                     # the groups, as indices into reducer.params: not in reducer.params order
HYPER6 = [(3e-4, 0.0), (1e-3, 1e-2)]


def _make6(params=None):
    from dreamvla_amd.optim import FlatAdamW
    src = [p for g in _init2("f32") for p in g] if params is None else params
    it = iter(src)
    red = _Buckets([[torch.nn.Parameter(next(it).detach().clone()) for _ in shapes] for shapes in SHAPES2])
    groups = [{"params": [red.params[i] for i in idx], "lr": lr, "weight_decay": wd} for idx, (lr, wd) in zip(ORDER6, HYPER6)]
    return red, FlatAdamW(red, betas=BETAS, eps=EPS, param_groups=groups)


def _torch6(params):
    pt = [torch.nn.Parameter(p.detach().clone()) for p in params]
    groups = [{"params": [pt[i] for i in idx], "lr": lr, "weight_decay": wd} for idx, (lr, wd) in zip(ORDER6, HYPER6)]
    return pt, torch.optim.AdamW(groups, betas=BETAS, eps=EPS)


def _where6(red, opt):
    """reducer.params index -> (flat buffers of its bucket, offset, numel)"""
    out = {}
    index = {id(p): i for i, p in enumerate(red.params)}
    for b, s in zip(red.buckets, opt.flat):
        for p, off in zip(b["params"], b["offsets"]):
            out[index[id(p)]] = (s, off, p.numel())
    return out


def _grads6(k):
    gen = torch.Generator().manual_seed(3000 + k)
    return [(torch.randn(s, generator=gen) * (1.0 if k % 2 == 0 else 1e-3)).float().cuda() for shapes in SHAPES2 for s in shapes]


def _held_as_the_one_group_kernel_is(red, opt, pt, opt_t, p0, grads, step, resync):
    """the assertion of tests/test_master_adamw_gpu.py::test_master_kernel_matches_torch_adamw_fp32, per parameter with its
    group's lr"""
    from tests.test_master_adamw_gpu import _within
    lr_of = {i: lr for idx, (lr, _) in zip(ORDER6, HYPER6) for i in idx}
    for i, (s, off, n) in _where6(red, opt).items():
        st = opt_t.state[pt[i]]
        tp, tm, tv = (x.detach().reshape(-1).double().cpu() for x in (pt[i], st["exp_avg"], st["exp_avg_sq"]))
        g = grads[i].reshape(-1).double().cpu()
        sl = slice(off, off + n)
        _within(s["m"][sl], tm, BETAS[0] * tm.abs() + (1 - BETAS[0]) * g.abs(), f"m step {step} parameter {i}")
        _within(s["v"][sl], tv, 0.0, f"v step {step} parameter {i}")
        denom = tv.sqrt() / (1.0 - BETAS[1] ** step) ** 0.5 + EPS
        _within(s["p"][sl], tp, p0[i].abs() + lr_of[i] / (1.0 - BETAS[0] ** step) * (tm / denom).abs(), f"p step {step} parameter {i}")
        if resync:      # the trajectories must not drift apart: continue both from torch's state
            s["p"][sl].copy_(pt[i].detach().reshape(-1)); s["m"][sl].copy_(st["exp_avg"].reshape(-1))
            s["v"][sl].copy_(st["exp_avg_sq"].reshape(-1))


@pytest.mark.gpu
def test_fp32_groups_match_torch_adamw_with_the_same_groups():
    """clip off, 5 steps from the same state, two groups that are not in reducer.params order"""
    red, opt = _make6()
    pt, opt_t = _torch6(red.params)
    for step in range(1, 6):
        grads = _grads6(step - 1)
        _set_grads(red, grads)
        for p, g in zip(pt, grads):
            p.grad = g.clone()
        p0 = [p.detach().reshape(-1).double().cpu() for p in pt]
        opt_t.step()
        opt.step()
        torch.cuda.synchronize()
        _held_as_the_one_group_kernel_is(red, opt, pt, opt_t, p0, grads, step, resync=True)


@pytest.mark.gpu
def test_master_checkpoint_is_torchs_with_several_groups_in_both_directions():
    red, opt = _make6()
    for k in range(3):
        _set_grads(red, _grads6(k))
        opt.step()
    sd = opt.state_dict()
    # torch's numbering: position in the concatenation of the groups' lists (4 1 3 | 2 0 of reducer.params)
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4]]
    assert [(g["lr"], g["weight_decay"]) for g in sd["param_groups"]] == HYPER6
    where = _where6(red, opt)
    for t, i in enumerate(ORDER6[0] + ORDER6[1]):
        s, off, n = where[i]
        assert float(sd["state"][t]["step"]) == 3.0 and sd["state"][t]["exp_avg"].shape == red.params[i].shape
        assert torch.equal(_bits(sd["state"][t]["exp_avg"].reshape(-1)), _bits(s["m"][off:off + n]))
        assert torch.equal(_bits(sd["state"][t]["exp_avg_sq"].reshape(-1)), _bits(s["v"][off:off + n]))
    # FlatAdamW -> torch.optim.AdamW(groups)
    pt, opt_t = _torch6(red.params)
    opt_t.load_state_dict(copy.deepcopy(sd))           # (torch adopts the dict's step tensors and counts on in them: a copy)
    assert [(g["lr"], g["weight_decay"]) for g in opt_t.param_groups] == HYPER6
    for t, i in enumerate(ORDER6[0] + ORDER6[1]):
        assert torch.equal(_bits(opt_t.state[pt[i]]["exp_avg"]), _bits(sd["state"][t]["exp_avg"]))
    # torch's dict -> a fresh FlatAdamW over the parameters as they stand
    sd_t = opt_t.state_dict()
    red2, opt2 = _make6(list(red.params))
    for g in opt2.param_groups:
        g["lr"], g["weight_decay"] = 7.0, 7.0           # load_state_dict writes every group's hyper-parameters
    opt2.load_state_dict(copy.deepcopy(sd_t))
    assert opt2.step_count == 3 and [(g["lr"], g["weight_decay"]) for g in opt2.param_groups] == HYPER6
    # all three continue for two steps: the reloaded FlatAdamW IS the uninterrupted run; torch is held to it as in the test above
    for step in (4, 5):
        grads = _grads6(step - 1)
        p0 = [p.detach().reshape(-1).double().cpu() for p in pt]
        for r, o in ((red, opt), (red2, opt2)):
            _set_grads(r, grads)
            o.step()
        for p, g in zip(pt, grads):
            p.grad = g.clone()
        opt_t.step()
        torch.cuda.synchronize()
        for a, b in zip(_snap(red, opt), _snap(red2, opt2)):
            assert all(torch.equal(a[key], b[key]) for key in a), f"step {step}: the reloaded optimizer left the uninterrupted run"
        _held_as_the_one_group_kernel_is(red, opt, pt, opt_t, p0, grads, step, resync=False)
    # another partition of the same indices is refused
    bad = copy.deepcopy(sd_t)
    bad["param_groups"][0]["params"], bad["param_groups"][1]["params"] = [0, 1], [2, 3, 4]
    with pytest.raises(ValueError, match="2 parameter groups"):
        opt2.load_state_dict(bad)
    one = copy.deepcopy(sd_t)
    one["param_groups"] = [dict(one["param_groups"][0], params=[0, 1, 2, 3, 4])]
    with pytest.raises(ValueError, match="2 parameter groups"):
        opt2.load_state_dict(one)


# ---- 7. the bf16-only checkpoint ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bf16_checkpoint_round_trips_with_group_params():
    mode = "bf16"
    red, opt = _make(_init2(mode), GROUP_OF2, PAIRS, None, 0.1, False, False)
    for k in range(2):
        _set_grads(red, _grads2(mode, k))
        opt.step()
    sd = opt.state_dict()
    assert sd["group_params"] == [[0, 2], [1, 3], [4]] and sd["step"] == 2
    assert [(g["lr"], g["weight_decay"]) for g in sd["param_groups"]] == PAIRS
    red2, opt2 = _make(_init2(mode), GROUP_OF2, [(7.0, 7.0)] * 3, None, 0.1, False, False)
    for p, q in zip(red2.params, red.params):
        p.data.copy_(q.data)
    opt2.load_state_dict(sd)
    assert [(g["lr"], g["weight_decay"]) for g in opt2.param_groups] == PAIRS
    for r, o in ((red, opt), (red2, opt2)):
        _set_grads(r, _grads2(mode, 2))
        o.step()
    for a, b in zip(_snap(red, opt), _snap(red2, opt2)):
        assert all(torch.equal(a[key], b[key]) for key in a)
    # another partition, a dict without the key, and a grouped dict into a one-group optimizer
    with pytest.raises(ValueError, match="parameter groups"):
        opt2.load_state_dict(dict(sd, group_params=[[0, 1], [2, 3], [4]]))
    with pytest.raises(ValueError, match="parameter groups"):
        opt2.load_state_dict({k: v for k, v in sd.items() if k != "group_params"})
    red1, opt1 = _make(_init2(mode), GROUP_OF2, PAIRS, 0, 0.1, False, False)
    assert "group_params" not in opt1.state_dict()          # one group: the dict is what it was
    with pytest.raises(ValueError, match="parameter groups"):
        opt1.load_state_dict(sd)


# ---- 8. the C entry points and the constructor ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c_entry_points_check_their_arguments():
    from dreamvla_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(256, dtype=F32, device="cuda")
    gmap = torch.zeros(32, dtype=torch.uint8, device="cuda")
    state = torch.zeros(ctypes.sizeof(_lib.StepState), dtype=torch.uint8, device="cuda")
    p, mp, st = buf.data_ptr(), gmap.data_ptr(), state.data_ptr()
    assert p % 16 == 0 and st % 16 == 0
    hp = (ctypes.c_double * 65)(*([1e-3] * 65))
    w = (ctypes.c_float * _lib.STEP_MAX_CANDIDATES)(*([0.001] * _lib.STEP_MAX_CANDIDATES))
    stream = torch.cuda.current_stream().cuda_stream

    def master(param=p, ema=None, n=8, gm=mp, n_groups=2, step=1, state=None, ema_w=None, n_cand=1, lr=hp):
        return lib.dvla_adamw_f32_master_grouped(param, p, p, p, p, ema, n, gm, n_groups, lr, hp, 0.9, 0.999, 1e-8, step, None, 0.0,
                                                 state, ema_w, n_cand, stream)

    def bf16(param=p, ema=None, n=8, gm=mp, n_groups=2, step=1, state=None, ema_w=None, n_cand=1, lr=hp):
        return lib.dvla_adamw_bf16_grouped(param, p, p, p, ema, n, gm, n_groups, lr, hp, 0.9, 0.999, 1e-8, step, None, 0.0, state,
                                           ema_w, n_cand, stream)

    for fn in (master, bf16):       # none of these launches anything
        assert fn(param=p + 4) == ERR_UNSUPPORTED and fn(ema=p + 4, ema_w=w) == ERR_UNSUPPORTED
        assert fn(state=st + 8) == ERR_UNSUPPORTED
        assert fn(n_groups=65) == ERR_ARG and fn(n_groups=0) == ERR_ARG
        assert fn(param=None) == ERR_ARG and fn(gm=None) == ERR_ARG and fn(lr=None) == ERR_ARG and fn(n=-1) == ERR_ARG
        assert fn(step=0) == ERR_ARG and fn(ema=p) == ERR_ARG and fn(state=st, n_cand=0) == ERR_ARG and fn(state=st, n_cand=10) == ERR_ARG
        assert fn(n=0) == 0 and fn(n=0, state=st, ema=p, ema_w=w, n_cand=9) == 0
    torch.cuda.synchronize()
    assert not bool(buf.any())


@pytest.mark.gpu
def test_constructor_and_step_refuse_what_the_groups_cannot_be():
    from dreamvla_amd.optim import FlatAdamW

    def fresh():
        return _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init("f32")])

    red = fresh()
    with pytest.raises(ValueError, match="is in no group"):
        FlatAdamW(red, param_groups=[{"params": red.params[:2]}])
    red = fresh()
    with pytest.raises(ValueError, match="group 1 has betas"):
        FlatAdamW(red, param_groups=[{"params": red.params[:2]}, {"params": red.params[2:], "betas": (0.8, 0.9)}])
    red = fresh()
    opt = FlatAdamW(red, lr=LR, weight_decay=WD, param_groups=[{"params": red.params[:2]}, {"params": red.params[2:], "lr": 1e-4}])
    assert [(g["lr"], g["weight_decay"], g["betas"], g["eps"]) for g in opt.param_groups] == \
        [(LR, WD, (0.9, 0.999), 1e-8), (1e-4, WD, (0.9, 0.999), 1e-8)]          # missing keys: the constructor's
    with pytest.raises(RuntimeError, match="add_param_group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(8, device="cuda"))]})
    before = _snap(red, opt)
    opt.param_groups[1]["eps"] = 1e-6
    _set_grads(red, _grads("f32", 0))
    with pytest.raises(ValueError, match="group 1 has"):
        opt.step()
    assert opt.step_count == 0 and all(torch.equal(a[k], b[k]) for a, b in zip(_snap(red, opt), before) for k in a)


# ---- the real reducer and weight_decay_groups ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_weight_decay_groups_over_the_real_reducer():
    """GradBucketReducer pads every parameter to 128 elements: the gaps are nobody's (255).  Linear + LayerNorm in fp32 masters;
    every parameter is stepped as the one-group optimizer with its group's weight decay steps it."""
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW, weight_decay_groups
    torch.manual_seed(5)
    proto = torch.nn.Sequential(torch.nn.Linear(40, 50), torch.nn.LayerNorm(50), torch.nn.Linear(50, 3)).cuda()
    gen = torch.Generator().manual_seed(7)
    grads = [[(torch.randn(p.shape, generator=gen) * 0.3).cuda() for p in proto.parameters()] for _ in range(3)]

    def run(groups_of, **kw):
        model = copy.deepcopy(proto)
        red = GradBucketReducer(list(model.parameters()))
        opt = FlatAdamW(red, lr=LR, max_grad_norm=0.1, ema_decay=DECAY, param_groups=groups_of(model), **kw)
        for g in grads:         # the gradient of sum(p * c) is c: through the reducer's hooks, as in training
            opt.zero_grad()
            sum((p * c).sum() for p, c in zip(model.parameters(), g)).backward()
            red.finish()
            opt.step()
        return model, red, opt

    model, red, opt = run(lambda m: weight_decay_groups(m, 0.05))
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.05] and [len(g["params"]) for g in opt.param_groups] == [4, 2]
    assert opt.master_mode and 255 in opt._group_map(0).cpu().tolist()
    refs = {wd: run(lambda m: None, weight_decay=wd) for wd in (0.0, 0.05)}
    got = _snap(red, opt)
    for i, p in enumerate(red.params):
        wd = 0.05 if p.ndim > 1 else 0.0
        want = _snap(refs[wd][1], refs[wd][2])[i]
        for key in want:
            assert torch.equal(got[i][key], want[key]), f"parameter {i} ({tuple(p.shape)}), {key}"
