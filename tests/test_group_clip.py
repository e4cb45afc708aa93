"""CPU: the host side of FlatAdamW(clip="group") -- the new symbols and the argument checks of their entry points that return
before anything touches a device, optim.prefix_groups, the validation of `clip` and of the per-group max_grad_norm, and the
float64 statement of the semantics that tests/test_group_clip_gpu.py holds the fp32-master trajectory against."""
import ctypes
import os
import re

import pytest
import torch

from dreamvla_amd import _lib
from dreamvla_amd.optim import group_max_norms, prefix_groups, resolve_clip
from tests.test_master_adamw import clip_adamw_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3
NEW = ("dvla_group_sumsq", "dvla_adamw_bf16_grouped_clip", "dvla_adamw_f32_master_grouped_clip", "dvla_adamw_bf16_sr_clip")


def group_clip_adamw_f64(params, grads, exp_avg, exp_avg_sq, step, group_of, hyper, betas, eps):
    """The semantics of clip="group" in float64: clip_adamw_f64 (clip_grad_norm_(max_norm) + AdamW) applied per group, to the
    tensors of that group alone.  group_of[i]: the group of tensor i; hyper[g] = (lr, weight_decay, max_norm or None).
    -> (params, exp_avg, exp_avg_sq) as lists in the order given, and the groups' sums of squares"""
    n = len(params)
    out_p, out_m, out_v, sums = [None] * n, [None] * n, [None] * n, []
    for g, (lr, wd, max_norm) in enumerate(hyper):
        idx = [i for i in range(n) if group_of[i] == g]
        p, m, v, ss = clip_adamw_f64([params[i] for i in idx], [grads[i] for i in idx], [exp_avg[i] for i in idx],
                                     [exp_avg_sq[i] for i in idx], step, lr, betas, eps, wd, max_norm=max_norm)
        sums.append(ss)
        for k, i in enumerate(idx):
            out_p[i], out_m[i], out_v[i] = p[k], m[k], v[k]
    return out_p, out_m, out_v, sums


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_the_new_symbols_are_bound_declared_and_the_abi_version_stays_9():
    lib = _lib_loaded()
    hdr = open(os.path.join(ROOT, "include", "dvla.h")).read()
    assert _lib.ABI_VERSION == 9 and lib.dvla_abi_version() == 9 and re.search(r"#define DVLA_ABI_VERSION 9\b", hdr)
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
        assert re.search(r"\nint " + name + r"\(", hdr), name


def test_the_float64_statement_clips_every_group_on_its_own_norm():
    gen = torch.Generator().manual_seed(0)
    shapes = [(7,), (3, 5), (11,), (2,)]
    group_of = [0, 1, 0, 2]
    p = [torch.randn(s, generator=gen).double() for s in shapes]
    g = [torch.randn(s, generator=gen).double() * sc for s, sc in zip(shapes, (1.0, 100.0, 1.0, 1.0))]
    z = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    hyper = [(1e-3, 1e-2, 0.1), (1e-3, 0.0, 1e3), (2e-3, 0.0, None)]
    out_p, out_m, out_v, sums = group_clip_adamw_f64(p, g, z, z, 1, group_of, hyper, (0.9, 0.999), 1e-8)
    assert sums == pytest.approx([float((g[0] ** 2).sum() + (g[2] ** 2).sum()), float((g[1] ** 2).sum()), float((g[3] ** 2).sum())])
    # exp_avg after one step from zero is (1 - beta1) * the clipped gradient: the loud group 1 scales nobody but itself
    coef = [min(1.0, 0.1 / (sums[0] ** 0.5 + 1e-6)), min(1.0, 1e3 / (sums[1] ** 0.5 + 1e-6)), 1.0]
    assert coef[0] < 1.0 and coef[1] == 1.0
    for i, gi in enumerate(group_of):
        assert torch.allclose(out_m[i], 0.1 * g[i] * coef[gi], rtol=1e-12, atol=0)
    # and group 0 is what clip_adamw_f64 gives for its two tensors alone
    ref = clip_adamw_f64([p[0], p[2]], [g[0], g[2]], [z[0], z[2]], [z[0], z[2]], 1, 1e-3, (0.9, 0.999), 1e-8, 1e-2, max_norm=0.1)
    assert torch.equal(out_p[0], ref[0][0]) and torch.equal(out_p[2], ref[0][1])


# ---- `clip` and the per-group max_grad_norm ----------------------------------------------------------------------------------------
def test_clip_is_global_or_group_and_group_needs_two_groups():
    assert resolve_clip("global", 1) == "global" and resolve_clip("global", 3) == "global" and resolve_clip("group", 2) == "group"
    for n in (0, 1):
        with pytest.raises(ValueError, match="global clip"):
            resolve_clip("group", n)
    for bad in ("per_group", None, True, "Group"):
        with pytest.raises(ValueError, match='"global" or "group"'):
            resolve_clip(bad, 2)


def test_every_group_takes_its_own_value_none_or_the_constructors():
    groups = [{"params": []}, {"params": [], "max_grad_norm": 1e3}, {"params": [], "max_grad_norm": None},
              {"params": [], "max_grad_norm": 1}]
    assert group_max_norms(groups, 0.1) == [0.1, 1e3, None, 1.0]
    assert group_max_norms(groups, None) == [None, 1e3, None, 1.0]
    assert all(m is None or isinstance(m, float) for m in group_max_norms(groups, 0.1))
    for bad in (0.0, -1.0, float("inf"), float("nan"), "loud", True):
        with pytest.raises(ValueError, match="group 1 has max_grad_norm"):
            group_max_norms([{"params": []}, {"params": [], "max_grad_norm": bad}], 0.1)
    with pytest.raises(ValueError, match="group 0 has max_grad_norm"):       # the constructor's value is checked where it is used
        group_max_norms([{"params": []}, {"params": [], "max_grad_norm": 1.0}], -0.1)


# ---- prefix_groups -----------------------------------------------------------------------------------------------------------------
class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.trunk = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
        self.image_decoder = torch.nn.Linear(4, 3)
        self.image_decoder_pos = torch.nn.Parameter(torch.zeros(3))
        self.action_head = torch.nn.Linear(4, 2)
        self.frozen = torch.nn.Parameter(torch.zeros(2), requires_grad=False)
        self.misc = torch.nn.Parameter(torch.zeros(1))


def test_prefix_groups_partitions_the_trainable_parameters_in_order():
    model = _Model()
    groups = prefix_groups(model, {"heads": ("image_decoder", "action_head."), "trunk": ("trunk.",)},
                           max_grad_norm={"heads": 0.05, "rest": None}, lr={"trunk": 1e-4})
    assert [g["name"] for g in groups] == ["heads", "trunk", "rest"]
    names = {id(p): n for n, p in model.named_parameters()}
    assert [[names[id(p)] for p in g["params"]] for g in groups] == [
        ["image_decoder_pos", "image_decoder.weight", "image_decoder.bias", "action_head.weight", "action_head.bias"],
        ["trunk.0.weight", "trunk.0.bias", "trunk.1.weight", "trunk.1.bias"], ["misc"]]
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert sorted(id(p) for g in groups for p in g["params"]) == sorted(id(p) for p in trainable)        # each exactly once
    assert groups[0]["max_grad_norm"] == 0.05 and "lr" not in groups[0]
    assert groups[1]["lr"] == 1e-4 and "max_grad_norm" not in groups[1]
    assert groups[2]["max_grad_norm"] is None and set(groups[2]) == {"name", "params", "max_grad_norm"}


def test_prefix_groups_rest_and_the_longest_prefix():
    model = _Model()
    # nothing left over: no `rest` group; a longer prefix takes its parameters out of a shorter one's group
    groups = prefix_groups(model, {"all": ("",), "decoder": ("image_decoder.",)}, rest="other")
    assert [g["name"] for g in groups] == ["all", "decoder"] and len(groups[1]["params"]) == 2 and len(groups[0]["params"]) == 8
    # named pairs work as a module does; a shared parameter counts once, under its first name
    w, b = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    groups = prefix_groups([("a.w", w), ("b.tied", w), ("b.b", b)], {"a": "a."}, rest="everything_else")
    assert [g["name"] for g in groups] == ["a", "everything_else"] and groups[0]["params"][0] is w and groups[1]["params"] == [b]
    with pytest.raises(ValueError, match="matches no prefix"):
        prefix_groups(model, {"trunk": ("trunk.",)}, rest=None)
    assert [g["name"] for g in prefix_groups(model, {"all": ("",)}, rest=None)] == ["all"]


def test_prefix_groups_names_what_it_cannot_place():
    model = _Model()
    with pytest.raises(ValueError, match="'dino_decoder' .*matches no trainable parameter"):
        prefix_groups(model, {"heads": ("image_decoder", "dino_decoder")})
    with pytest.raises(ValueError, match="'frozen' .*matches no trainable parameter"):
        prefix_groups(model, {"cold": ("frozen",)})
    with pytest.raises(ValueError, match="given to two groups"):
        prefix_groups(model, {"a": ("trunk.",), "b": ("trunk.",)})
    with pytest.raises(ValueError, match="names the group 'head'"):
        prefix_groups(model, {"heads": ("image_decoder",)}, max_grad_norm={"head": 0.1})
    with pytest.raises(ValueError, match="everything else"):
        prefix_groups(model, {"rest": ("trunk.",)})


# ---- the C entry points' argument checks (nothing here reaches a device) -------------------------------------------------------------
def test_group_sumsq_checks_its_arguments_before_touching_the_device():
    lib = _lib_loaded()
    p = 4096          # never dereferenced: every call below returns from its argument checks

    def call(ps=p, gof=p, n_params=3, n_groups=2, out=p, total=p):
        return lib.dvla_group_sumsq(ps, gof, n_params, n_groups, out, total, None)

    for name in ("ps", "gof", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(n_params=-1) == ERR_ARG and call(n_groups=0) == ERR_ARG and call(n_groups=_lib.STEP_MAX_GROUPS + 1) == ERR_ARG


def test_the_clip_step_entry_points_check_their_arguments_before_touching_the_device():
    lib = _lib_loaded()
    p = 4096          # aligned, never dereferenced
    hp = (ctypes.c_double * 65)(*([1e-3] * 65))
    mn = (ctypes.c_float * 65)(*([0.1] * 65))
    w = (ctypes.c_float * _lib.STEP_MAX_CANDIDATES)(*([0.001] * _lib.STEP_MAX_CANDIDATES))

    def master(param=p, grad=p, m=p, v=p, sh=p, ema=None, n=8, gm=p, n_groups=2, step=1, state=None, ema_w=None, n_cand=1, lr=hp, wd=hp,
               gs=p, max_norm=mn):
        return lib.dvla_adamw_f32_master_grouped_clip(param, grad, m, v, sh, ema, n, gm, n_groups, lr, wd, 0.9, 0.999, 1e-8, step, gs,
                                                      max_norm, state, ema_w, n_cand, None)

    def bf16(param=p, grad=p, m=p, v=p, sh=None, ema=None, n=8, gm=p, n_groups=2, step=1, state=None, ema_w=None, n_cand=1, lr=hp, wd=hp,
             gs=p, max_norm=mn):
        return lib.dvla_adamw_bf16_grouped_clip(param, grad, m, v, ema, n, gm, n_groups, lr, wd, 0.9, 0.999, 1e-8, step, gs, max_norm,
                                                state, ema_w, n_cand, None)

    def sr(param=p, grad=p, m=p, v=p, sh=None, ema=None, n=8, gm=p, n_groups=2, step=1, state=None, ema_w=None, n_cand=1, lr=hp, wd=hp,
           gs=p, max_norm=mn, base=0):
        return lib.dvla_adamw_bf16_sr_clip(param, grad, m, v, ema, n, gm, n_groups, lr, wd, 0.9, 0.999, 1e-8, step, gs, max_norm,
                                           state, ema_w, n_cand, 7, 0, base, None)

    for fn in (master, bf16, sr):
        for name in ("param", "grad", "m", "v", "gm", "lr", "wd", "gs", "max_norm"):
            assert fn(**{name: None}) == ERR_ARG, (fn.__name__, name)
        assert fn(n=-1) == ERR_ARG and fn(step=0) == ERR_ARG
        assert fn(n_groups=0) == ERR_ARG and fn(n_groups=_lib.STEP_MAX_GROUPS + 1) == ERR_ARG
        assert fn(ema=p) == ERR_ARG                                              # an EMA buffer without its weights
        assert fn(state=p, n_cand=0) == ERR_ARG and fn(state=p, n_cand=_lib.STEP_MAX_CANDIDATES + 1) == ERR_ARG
        assert fn(n=0, gs=None) == ERR_ARG and fn(n=0, max_norm=None) == ERR_ARG   # also where nothing would be launched
        for name in ("param", "grad", "m", "v"):
            assert fn(**{name: p + 4}) == ERR_UNSUPPORTED, (fn.__name__, name)
        assert fn(ema=p + 4, ema_w=w) == ERR_UNSUPPORTED and fn(state=p + 8) == ERR_UNSUPPORTED
        assert fn(n=0) == 0 and fn(n=0, state=p, ema=p, ema_w=w, n_cand=_lib.STEP_MAX_CANDIDATES) == 0
    assert master(sh=p + 4) == ERR_UNSUPPORTED
    assert sr(gm=None, n_groups=1) == ERR_ARG          # one group has one clip norm: dvla_adamw_bf16_sr
    assert sr(base=-1) == ERR_ARG
