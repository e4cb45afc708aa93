"""CPU: the fp32-master optimizer step (FlatAdamW master mode; dvla_sumsq_f32 + dvla_adamw_f32_master).

* the C ABI: the header declares both kernels and the built library exports them with the ctypes bindings _lib.py gives;
* `clip_adamw_f64`, the float64 restatement of `clip_grad_norm_` + torch's AdamW on fp32 parameters that the GPU tests
  (tests/test_master_adamw_gpu.py) check the kernels against, pinned here against torch itself;
* the conversion between torch.optim.AdamW's state format and the flat moment buffers (checkpoint interop)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dreamvla_amd", "libdvla_hip.so")


def clip_adamw_f64(params, grads, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay, max_norm=None, sumsq=None):
    """One clip_grad_norm_(max_norm) + torch AdamW (decoupled weight decay) step in float64 on lists of tensors (returned as new
    float64 tensors, inputs untouched): the operation sequence of torch/optim/adam.py::_multi_tensor_adam, without its fp32
    roundings.  sumsq: use this total sum of squares for the clip coefficient instead of the gradients' own.
    Returns (params, exp_avg, exp_avg_sq, sum of squares)."""
    g64 = [g.double() for g in grads]
    ss = sum(float((g * g).sum()) for g in g64) if sumsq is None else float(sumsq)
    coef = 1.0
    if max_norm is not None:
        coef = min(1.0, max_norm / (ss ** 0.5 + 1e-6))
    b1, b2 = betas
    bc1 = 1.0 - b1 ** step
    bc2_sqrt = (1.0 - b2 ** step) ** 0.5
    out_p, out_m, out_v = [], [], []
    for p, g, m, v in zip(params, g64, exp_avg, exp_avg_sq):
        g = g * coef
        p = p.double() * (1.0 - lr * weight_decay)
        m = m.double() + (1.0 - b1) * (g - m.double())
        v = b2 * v.double() + (1.0 - b2) * g * g
        denom = v.sqrt() / bc2_sqrt + eps
        p = p - (lr / bc1) * (m / denom)
        out_p.append(p); out_m.append(m); out_v.append(v)
    return out_p, out_m, out_v, ss


def test_header_and_library_export_the_master_kernels():
    hdr = open(os.path.join(ROOT, "include", "dvla.h")).read()
    assert re.search(r"int dvla_sumsq_f32\(const float\* x, int64_t n, float\* partial, float\* out, int32_t accumulate, "
                     r"void\* stream\);", hdr)
    assert re.search(r"int dvla_adamw_f32_master\(float\* param, const float\* grad, float\* exp_avg, float\* exp_avg_sq, "
                     r"void\* shadow_bf16, int64_t n,\s+double lr, double beta1, double beta2, double eps, double weight_decay, "
                     r"int64_t step,\s+const float\* grad_sumsq, float max_norm, void\* stream\);", hdr)
    from dreamvla_amd import _lib
    P, D = ctypes.c_void_p, ctypes.c_double
    assert _lib.SYMBOLS["dvla_sumsq_f32"] == (ctypes.c_int, [P, ctypes.c_int64, P, P, ctypes.c_int32, P])
    assert _lib.SYMBOLS["dvla_adamw_f32_master"] == (ctypes.c_int, [P, P, P, P, P, ctypes.c_int64, D, D, D, D, D, ctypes.c_int64,
                                                                    P, ctypes.c_float, P])
    assert _lib.ABI_VERSION == 9
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    lib = _lib.load()
    for name in ("dvla_sumsq_f32", "dvla_adamw_f32_master"):
        fn = getattr(lib, name)
        assert fn.restype is _lib.SYMBOLS[name][0] and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    assert lib.dvla_abi_version() == 9


@pytest.mark.parametrize("max_norm", [None, 0.1], ids=["clip_off", "clip_on"])
def test_f64_restatement_matches_torch_clip_adamw(max_norm):
    g = torch.Generator().manual_seed(11)
    shapes = [(37, 19), (128,), (5, 7, 3)]
    params = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.3) for s in shapes]
    p64 = [p.detach().double() for p in params]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    lr, betas, eps, wd = 1e-2, (0.9, 0.95), 1e-8, 0.05
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=True)
    for step in range(1, 6):
        grads = [torch.randn(p.shape, generator=g) * (3.0 if step % 2 else 0.01) for p in params]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        if max_norm is not None:
            norm_t = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        p64, m64, v64, ss = clip_adamw_f64(p64, grads, m64, v64, step, lr, betas, eps, wd, max_norm=max_norm)
        if max_norm is not None:
            assert abs(float(norm_t) - ss ** 0.5) <= 1e-6 * ss ** 0.5
        for p, q, m, v in zip(params, p64, m64, v64):
            st = opt.state[p]
            # fp32 storage against float64: a few fp32 roundings per step, accumulated over <= 5 steps
            assert float((p.detach().double() - q).abs().max()) <= 1e-6 * float(q.abs().max())
            assert float((st["exp_avg"].double() - m).norm()) <= 1e-6 * float(m.norm())
            assert float((st["exp_avg_sq"].double() - v).norm()) <= 1e-6 * float(v.norm())


def _cpu_reducer(params):
    from dreamvla_amd.ddp import GradBucketReducer
    return GradBucketReducer(params, bucket_bytes=4096, last_bucket_bytes=0)     # small buckets: several of them


def test_torch_state_round_trips_through_the_flat_layout():
    from dreamvla_amd import optim as O
    g = torch.Generator().manual_seed(3)
    shapes = [(300,), (16, 33), (7,), (64, 20), (5, 5)]
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    red = _cpu_reducer(params)
    assert len(red.buckets) >= 2
    layout = O.flat_layout(red)
    assert sorted(i for lay in layout for i, _, _ in lay) == list(range(len(params)))
    # torch AdamW over independent copies; parameters 1 and 3 never receive a gradient (no state in torch's dict)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.1)
    for _ in range(2):
        for i, p in enumerate(ref):
            p.grad = None if i in (1, 3) else torch.randn(p.shape, generator=g)
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 2, 4]
    ms = [torch.full_like(b["flat"], 7.0) for b in red.buckets]     # garbage: loading must overwrite every element
    vs = [torch.full_like(b["flat"], 7.0) for b in red.buckets]
    assert O.flat_from_torch_state(layout, sd["state"], ms, vs) == 2
    for lay, m, v in zip(layout, ms, vs):
        covered = torch.zeros(m.numel(), dtype=torch.bool)
        for i, off, shape in lay:
            n = ref[i].numel()
            covered[off:off + n] = True
            if i in sd["state"]:
                assert torch.equal(m[off:off + n].view(shape), sd["state"][i]["exp_avg"])
                assert torch.equal(v[off:off + n].view(shape), sd["state"][i]["exp_avg_sq"])
            else:
                assert not m[off:off + n].any() and not v[off:off + n].any()
        assert not m[~covered].any() and not v[~covered].any()       # alignment gaps are zero
    with_state = [[i in sd["state"] for i, _, _ in lay] for lay in layout]
    back = O.torch_state_from_flat(layout, ms, vs, 2, with_state)
    assert sorted(back) == [0, 2, 4]
    for i, st in back.items():
        assert st["step"].dtype == torch.float32 and float(st["step"]) == 2.0 and st["step"].dim() == 0
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    # what comes back loads into torch.optim.AdamW and steps exactly like the original
    ref2 = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    opt2 = torch.optim.AdamW(ref2, lr=1e-2, weight_decay=0.1)
    groups = [O._torch_group(dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), len(params))]
    assert set(groups[0]) == set(sd["param_groups"][0])
    opt2.load_state_dict({"state": back, "param_groups": groups})
    for p, q in zip(ref, ref2):
        p.grad = torch.ones_like(p)
        q.grad = torch.ones_like(q)
    opt.step()
    opt2.step()
    for p, q in zip(ref, ref2):
        assert torch.equal(p, q)


def test_disagreeing_step_counts_raise():
    from dreamvla_amd import optim as O
    params = [torch.nn.Parameter(torch.zeros(10)), torch.nn.Parameter(torch.zeros(4))]
    red = _cpu_reducer(params)
    layout = O.flat_layout(red)
    st = {i: {"step": torch.tensor(float(i + 1)), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
          for i, p in enumerate(params)}
    ms = [torch.zeros_like(b["flat"]) for b in red.buckets]
    vs = [torch.zeros_like(b["flat"]) for b in red.buckets]
    with pytest.raises(ValueError, match="step counts disagree"):
        O.flat_from_torch_state(layout, st, ms, vs)
    assert O.flat_from_torch_state(layout, {}, ms, vs) == 0
