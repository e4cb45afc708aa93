"""GPU: the optimizer step of the shipped precision (`--precision fp32 --bf16_module vision_encoder`): fp32 masters, fp32
gradients and moments, bf16 shadows -- dvla_sumsq_f32 + dvla_adamw_f32_master and FlatAdamW's master mode.

Bounds.  The kernel restates torch's fp32 AdamW op for op, so against the float64 restatement
(tests/test_master_adamw.py::clip_adamw_f64, evaluated from the kernel's own fp32 state of each step) an element is off by a
few fp32 roundings of the terms it is made of: |x - x64| <= 2e-6 * (|x64| + s) + 1e-30, where s is the magnitude of the terms
summed to form x (m: |beta1 m| + |(1 - beta1) g|; p: |p| + |lr / bc1 * m / denom|; v: no cancellation, s = 0) -- plain
relative error would be unbounded where the sum cancels to ~0.  The shadow is compared bit for bit."""
import json
import os

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_master_adamw import clip_adamw_f64

BF = torch.bfloat16
TOL = 2e-6
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2


def _lib():
    from dreamvla_amd import _lib as L
    return L.load(), L.check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _within(x, ref, scale, what):
    x = x.double().cpu()
    err = (x - ref).abs()
    lim = TOL * (ref.abs() + scale) + 1e-30
    bad = err > lim
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / lim).max()))


def _bucket(n, gen, grad_scale):
    """fp32 buffers as FlatAdamW allocates them (16-B aligned; p kept away from 0 so that |p| is the scale of p)"""
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    p = (sign * (0.5 + torch.rand(n, generator=gen))).float()
    return {"p": p.cuda(), "m": torch.zeros(n, device="cuda"), "v": torch.zeros(n, device="cuda"),
            "sh": torch.zeros(n, dtype=BF, device="cuda"), "scale": grad_scale}


def _run_kernel_steps(sizes, max_norm, grad_scale, steps=5, seed=0):
    from dreamvla_amd import ops
    lib, check = _lib()
    gen = torch.Generator().manual_seed(seed)
    bufs = [_bucket(n, gen, grad_scale) for n in sizes]
    partial = torch.empty(int(lib.dvla_sumsq_partial_len()), device="cuda")
    sumsq = torch.zeros(1, device="cuda")
    for step in range(1, steps + 1):
        grads = [(torch.randn(b["p"].numel(), generator=gen) * b["scale"]).float() for b in bufs]
        g_dev = [g.cuda() for g in grads]
        before = [(b["p"].double().cpu(), b["m"].double().cpu(), b["v"].double().cpu()) for b in bufs]
        if max_norm is not None:
            for i, g in enumerate(g_dev):
                check(lib.dvla_sumsq_f32(g.data_ptr(), g.numel(), partial.data_ptr(), sumsq.data_ptr(), 1 if i else 0, _stream()),
                      "dvla_sumsq_f32")
        for b, g in zip(bufs, g_dev):
            check(lib.dvla_adamw_f32_master(b["p"].data_ptr(), g.data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(),
                                            b["sh"].data_ptr(), g.numel(), LR, BETAS[0], BETAS[1], EPS, WD, step,
                                            sumsq.data_ptr() if max_norm is not None else None,
                                            max_norm if max_norm is not None else 0.0, _stream()), "dvla_adamw_f32_master")
        torch.cuda.synchronize()
        p64, m64, v64, ss = clip_adamw_f64([x[0] for x in before], grads, [x[1] for x in before], [x[2] for x in before], step,
                                           LR, BETAS, EPS, WD, max_norm=max_norm)
        if max_norm is not None:
            assert abs(float(sumsq) - ss) <= 1e-6 * ss, (float(sumsq), ss)
        coef = 1.0 if max_norm is None else min(1.0, max_norm / (ss ** 0.5 + 1e-6))
        bc1 = 1.0 - BETAS[0] ** step
        for b, g, (p0, m0, v0), p, m, v in zip(bufs, grads, before, p64, m64, v64):
            gc = g.double() * coef
            _within(b["m"], m, BETAS[0] * m0.abs() + (1 - BETAS[0]) * gc.abs(), f"m step {step}")
            _within(b["v"], v, 0.0, f"v step {step}")
            denom = v.sqrt() / (1.0 - BETAS[1] ** step) ** 0.5 + EPS
            _within(b["p"], p, p0.abs() + (LR / bc1) * (m / denom).abs(), f"p step {step}")
            assert torch.equal(b["sh"], ops.cast_to(b["p"], BF)), f"shadow step {step}"
    return bufs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 128, 1000003])
@pytest.mark.parametrize("max_norm", [None, 0.1, 1e30], ids=["noclip", "clip", "clip_inactive"])
@pytest.mark.parametrize("grad_scale", [1e4, 1e-12], ids=["large", "tiny"])
def test_master_kernel_matches_f64_restatement(n, max_norm, grad_scale):
    _run_kernel_steps([n], max_norm, grad_scale, seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm", [None, 0.1], ids=["noclip", "clip"])
def test_master_kernel_multi_bucket_one_norm(max_norm):
    _run_kernel_steps([300, 128 * 5, 100003, 9], max_norm, 1.0, seed=7)


@pytest.mark.gpu
def test_master_kernel_matches_torch_adamw_fp32():
    """against torch.optim.AdamW's default (foreach) path on fp32 CUDA tensors, clip off, 5 steps from the same state"""
    from dreamvla_amd import ops
    lib, check = _lib()
    gen = torch.Generator().manual_seed(1)
    n = 1000003
    b = _bucket(n, gen, 1.0)
    ref = torch.nn.Parameter(b["p"].clone())
    opt = torch.optim.AdamW([ref], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    report = []
    for step in range(1, 6):
        g = (torch.randn(n, generator=gen) * (1.0 if step % 2 else 1e-3)).float().cuda()
        ref.grad = g.clone()
        p0 = ref.detach().double().cpu()
        opt.step()
        check(lib.dvla_adamw_f32_master(b["p"].data_ptr(), g.data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), b["sh"].data_ptr(),
                                        n, LR, BETAS[0], BETAS[1], EPS, WD, step, None, 0.0, _stream()), "dvla_adamw_f32_master")
        torch.cuda.synchronize()
        st = opt.state[ref]
        tp, tm, tv = ref.detach().double().cpu(), st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu()
        _within(b["m"], tm, BETAS[0] * tm.abs() + (1 - BETAS[0]) * g.double().cpu().abs(), f"m step {step}")
        _within(b["v"], tv, 0.0, f"v step {step}")
        denom = tv.sqrt() / (1.0 - BETAS[1] ** step) ** 0.5 + EPS
        _within(b["p"], tp, p0.abs() + LR / (1.0 - BETAS[0] ** step) * (tm / denom).abs(), f"p step {step}")
        assert torch.equal(b["sh"], ops.cast_to(b["p"], BF))
        report.append({"step": step, "p_bit_identical": bool(torch.equal(b["p"], ref.detach())),
                       "m_bit_identical": bool(torch.equal(b["m"], st["exp_avg"])),
                       "v_bit_identical": bool(torch.equal(b["v"], st["exp_avg_sq"])),
                       "p_elements_differing": int((b["p"] != ref.detach()).sum())})
        # the trajectories must not drift apart: continue both from torch's state
        b["p"].copy_(ref.detach()); b["m"].copy_(st["exp_avg"]); b["v"].copy_(st["exp_avg_sq"])
    print("torch foreach AdamW vs dvla_adamw_f32_master:", json.dumps(report))
    out = os.environ.get("DVLA_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "master_vs_torch_adamw.json"), "w") as f:
            json.dump(report, f)


# ----------------------------------------------------------------------------------------------------------------------------
# FlatAdamW over hand-made parameters
# ----------------------------------------------------------------------------------------------------------------------------
def _params(gen, dtypes):
    shapes = [(300,), (16, 40), (129,), (64, 24)]
    return [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.5).to(dt).cuda()) for s, dt in zip(shapes, dtypes)]


def _set_grads(red, grads):
    for p, g in zip(red.params, grads):
        red.grad_of(p).copy_(g)


@pytest.mark.gpu
def test_mixed_buckets_one_clip_norm_and_bf16_part_unchanged():
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    lib, check = _lib()
    gen = torch.Generator().manual_seed(2)
    dts = [BF, BF, torch.float32, torch.float32]       # one bf16 trainable module (weight + bias) + fp32 masters
    init = _params(gen, dts)
    grads = [[(torch.randn(p.shape, generator=gen) * 0.3).to(p.dtype).cuda() for p in init] for _ in range(3)]

    def mixed(max_norm):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in init]
        red = GradBucketReducer(ps)
        assert {b["flat"].dtype for b in red.buckets} == {BF, torch.float32}
        return ps, red, FlatAdamW(red, lr=LR, weight_decay=WD, max_grad_norm=max_norm)

    # clip on: one norm over both kinds; the bf16 buckets are exactly what dvla_adamw_bf16 makes with that norm
    ps, red, opt = mixed(0.1)
    assert opt.master_mode
    for step in range(1, 4):
        _set_grads(red, grads[step - 1])
        before = [{k: s[k].clone() for k in ("p", "m", "v")} for s in opt.flat]
        opt.step()
        torch.cuda.synchronize()
        ss = sum(float((g.double() ** 2).sum()) for g in grads[step - 1])
        assert abs(float(opt.grad_norm()) ** 2 - ss) <= 1e-6 * ss
        for s, bs in zip(opt.flat, before):
            if "sh" in s:
                continue
            p, m, v = bs["p"], bs["m"], bs["v"]
            check(lib.dvla_adamw_bf16(p.data_ptr(), s["g"].data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), LR, BETAS[0],
                                      BETAS[1], EPS, WD, step, opt._sumsq.data_ptr(), 0.1, _stream()), "dvla_adamw_bf16")
            assert torch.equal(p, s["p"]) and torch.equal(m, s["m"]) and torch.equal(v, s["v"])
    # clip off: the bf16 parameters step bit for bit as under today's FlatAdamW on a bf16-only reducer
    ps, red, opt = mixed(None)
    ps16 = [torch.nn.Parameter(p.detach().clone()) for p in init[:2]]
    red16 = GradBucketReducer(ps16)
    opt16 = FlatAdamW(red16, lr=LR, weight_decay=WD)
    assert not opt16.master_mode
    for step in range(3):
        _set_grads(red, grads[step])
        _set_grads(red16, grads[step][:2])
        opt.step()
        opt16.step()
    for a, b in zip(ps[:2], ps16):
        assert torch.equal(a, b)
    # and the fp32 masters against the float64 restatement (one clip norm: none)
    p64 = [p.detach().double().cpu() for p in init[2:]]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    for step in range(3):
        p64, m64, v64, _ = clip_adamw_f64(p64, [g.cpu() for g in grads[step][2:]], m64, v64, step + 1, LR, BETAS, EPS, WD)
    for a, r in zip(ps[2:], p64):
        assert float((a.detach().double().cpu() - r).abs().max()) <= 3 * TOL * float(r.abs().max())


def _loss_small(ps, coefs):
    return sum((p.float() * c).sum() for p, c in zip(ps, coefs) if c is not None)


@pytest.mark.gpu
def test_checkpoint_round_trips_with_torch_adamw():
    """torch AdamW 2 steps -> state_dict -> FlatAdamW.load_state_dict -> step 3 == torch's step 3; and the reverse direction
    loads into torch.optim.AdamW unchanged.  Parameter 1 never receives a gradient (no state on either side)."""
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    gen = torch.Generator().manual_seed(4)
    f32 = [torch.float32] * 4
    init = _params(gen, f32)
    coefs = [[None if i == 1 else (torch.randn(p.shape, generator=gen)).cuda() for i, p in enumerate(init)] for _ in range(3)]

    def torch_run(ps, steps):
        opt = torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        for k in steps:
            opt.zero_grad()
            _loss_small(ps, coefs[k]).backward()
            opt.step()
        return opt

    def flat_run(ps):
        red = GradBucketReducer(ps, bucket_bytes=4096, last_bucket_bytes=0)
        return red, FlatAdamW(red, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)

    def flat_step(red, opt, ps, k):
        opt.zero_grad()
        _loss_small(ps, coefs[k]).backward()
        red.finish()
        opt.step()

    def close(a, b, what):
        for x, y in zip(a, b):
            y = y.detach().double().cpu()
            assert float((x.detach().double().cpu() - y).abs().max()) <= 3 * TOL * float(y.abs().max()) + 1e-30, what

    # torch -> flat
    pt = [torch.nn.Parameter(p.detach().clone()) for p in init]
    opt_t = torch_run(pt, [0, 1])
    sd = opt_t.state_dict()
    assert sorted(sd["state"]) == [0, 2, 3]
    pf = [torch.nn.Parameter(p.detach().clone()) for p in pt]          # the model checkpoint
    red, opt_f = flat_run(pf)
    assert opt_f.master_mode
    opt_f.load_state_dict(sd)
    assert opt_f.step_count == 2
    # the flat side learns the unused parameter in its first finish(), as a resumed run does
    flat_step(red, opt_f, pf, 2)
    opt_t.zero_grad()
    _loss_small(pt, coefs[2]).backward()
    opt_t.step()
    close(pf, pt, "torch -> flat, step 3")
    assert torch.equal(pf[1], init[1])
    for i in (0, 2, 3):
        close([opt_f.state_dict()["state"][i]["exp_avg"]], [opt_t.state[pt[i]]["exp_avg"]], "m")
        close([opt_f.state_dict()["state"][i]["exp_avg_sq"]], [opt_t.state[pt[i]]["exp_avg_sq"]], "v")

    # flat -> torch
    pf = [torch.nn.Parameter(p.detach().clone()) for p in init]
    red, opt_f = flat_run(pf)
    flat_step(red, opt_f, pf, 0)
    flat_step(red, opt_f, pf, 1)
    sd = opt_f.state_dict()
    assert sorted(sd["state"]) == [0, 2, 3] and float(sd["state"][0]["step"]) == 2.0
    pt = [torch.nn.Parameter(p.detach().clone()) for p in pf]
    opt_t = torch.optim.AdamW(pt, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    opt_t.load_state_dict(sd)
    flat_step(red, opt_f, pf, 2)
    opt_t.zero_grad()
    _loss_small(pt, coefs[2]).backward()
    opt_t.step()
    close(pf, pt, "flat -> torch, step 3")

    # layouts that do not match raise clearly
    bad = dict(sd, param_groups=[dict(sd["param_groups"][0], params=[0, 1])])
    with pytest.raises(ValueError, match="ONE parameter group"):
        opt_f.load_state_dict(bad)
    with pytest.raises(ValueError, match="step counts disagree"):
        st = {k: dict(v) for k, v in sd["state"].items()}
        st[0]["step"] = torch.tensor(5.0)
        opt_f.load_state_dict(dict(sd, state=st))
    with pytest.raises(ValueError, match="amsgrad"):
        FlatAdamW(red, amsgrad=True)


# ----------------------------------------------------------------------------------------------------------------------------
# the whole model in the shipped flags
# ----------------------------------------------------------------------------------------------------------------------------
def _shipped_model(fixture):
    from tests import model_checks as C
    from tests.test_ddp_one_gpu import _make
    m, cfg, S, b, losses = _make(fixture)              # bf16 model; rebuilt below in the shipped precision
    del m
    m = C.build_hip_model(cfg)
    m = m.float()                                      # --precision fp32
    m.vision_encoder.bfloat16()                        # --bf16_module vision_encoder
    m.vision_encoder.requires_grad_(False)
    m.clip_model.requires_grad_(False)
    m = m.to("cuda")
    m._init_model_type()
    m.eval()                                           # no dropout: both optimizers see the same function
    return m, cfg, S, b, losses


class _CastCounter:
    """counts ops.cast_to fp32 -> bf16 calls on trainable masters (by address, re-read every step)"""

    def __init__(self, model):
        from dreamvla_amd import ops
        self.ops, self.model, self.orig, self.hits = ops, model, ops.cast_to, []

    def __enter__(self):
        self.uses = {}
        fwd = self.fwd = self.ops._Shadow.forward

        def counted(ctx, w):                          # shadow() calls per master (a weight used twice in one step has two)
            self.uses[id(w)] = self.uses.get(id(w), 0) + 1
            return fwd(ctx, w)
        self.ops._Shadow.forward = staticmethod(counted)

        def wrapped(x, dtype):
            if x.dtype == torch.float32 and dtype == BF and x.data_ptr() in self.ptrs:
                self.hits.append(self.ptrs[x.data_ptr()])
            return self.orig(x, dtype)
        self.ops.cast_to = wrapped
        return self

    def arm(self):
        self.ptrs = {p.data_ptr(): n for n, p in self.model.named_parameters() if p.requires_grad and p.dtype == torch.float32}
        self.hits = []

    def __exit__(self, *exc):
        self.ops.cast_to = self.orig
        self.ops._Shadow.forward = staticmethod(self.fwd)
        return False


def _copy_recorder():
    from dreamvla_amd.ddp import GradBucketReducer

    class Rec(GradBucketReducer):
        """records which parameters' gradients the reducer's hook had to copy into their slot"""

        def _make_hook(self, bi, pi):
            inner = super()._make_hook(bi, pi)

            def hook(param):
                if param.grad is not None and param.grad.data_ptr() != param._dvla_grad_view.data_ptr():
                    self.copied_ids = getattr(self, "copied_ids", set()) | {id(param)}
                inner(param)
            return hook
    return Rec


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("fixture", ["A", "B"], ids=["mlp_head_obs_depth_sam", "dit_head"])
def test_shipped_flags_flat_master_matches_torch_loop(fixture):
    from dreamvla_amd import ops
    from dreamvla_amd.optim import FlatAdamW
    from tests.test_ddp_one_gpu import _dit_noise, _loss
    steps = 3
    ops.GemmTuner.enabled = False          # the same kernel configuration in both runs
    try:
        runs = {}
        for mode in ("torch", "flat"):
            m, cfg, S, batch, losses = _shipped_model(fixture)
            names = [n for n, p in m.named_parameters() if p.requires_grad]
            params = [p for p in m.parameters() if p.requires_grad]
            init = {n: p.detach().clone() for n, p in zip(names, params)}
            if mode == "torch":
                opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-4)
            else:
                red = _copy_recorder()(params, bucket_bytes=8 << 20, direct_grads=True)
                assert {b["flat"].dtype for b in red.buckets} == {torch.float32}
                opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1)
                assert opt.master_mode
            res = {"loss": [], "casts": [], "norm": [], "params": [], "m": []}
            weights_seen = set()
            with _CastCounter(m) as cc:
                for step in range(steps):
                    cc.arm()
                    opt.zero_grad()
                    loss = _loss(m, cfg, S, batch, losses, slice(0, 2), _dit_noise(cfg, S, 2, 100 + step, [0, 1]))
                    res["casts"].append(list(cc.hits))
                    if step == 0:
                        weights_seen = set(cc.hits)
                        ids = {id(p): n for n, p in zip(names, params)}
                        res["multi_use"] = {ids[k] for k, c in cc.uses.items() if c > 1 and k in ids}
                    loss.backward()
                    if mode == "torch":
                        res["norm"].append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), 0.1)))
                    else:
                        red.finish()
                    opt.step()
                    if mode == "flat":
                        res["norm"].append(float(opt.grad_norm()))
                        # the handed-over shadows are the bf16 copies of the masters as they are now, bit for bit
                        fresh = 0
                        for n, p in zip(names, params):
                            ent = ops._Shadow.cache.get(id(p))
                            if ent is not None and ent[0]() is p and n in weights_seen:
                                assert torch.equal(ent[4], cc.orig(p.detach(), BF)), (step, n)
                                fresh += 1
                        assert fresh > 20, (step, fresh)
                    res["loss"].append(float(loss))
                    res["params"].append({n: p.detach().double().cpu() for n, p in zip(names, params)})
                    if mode == "torch":
                        res["m"].append({n: opt.state[p]["exp_avg"].double().cpu() for n, p in zip(names, params) if p in opt.state})
                    else:
                        sd = opt.state_dict()["state"]
                        res["m"].append({names[i]: st["exp_avg"].double().cpu() for i, st in sd.items()})
            if mode == "flat":
                fired = {id(bp) for b in red.buckets for bp, f in zip(b["params"], b["fired"]) if f}
                res["unused"] = [n for n, p in zip(names, params) if id(p) not in fired]
                res["copied"] = [n for n, p in zip(names, params) if id(p) in getattr(red, "copied_ids", set())]
            res["init"] = {n: t.double().cpu() for n, t in init.items()}
            runs[mode] = res
            del m, opt, params
            torch.cuda.empty_cache()
    finally:
        ops.GemmTuner.enabled = True
    t, f = runs["torch"], runs["flat"]
    weights = set(t["casts"][0])                 # the masters the forward multiplies on through bf16 shadows
    assert len(weights) > 20
    # the shadows: the reference loop re-casts every trainable weight each step; the flat path only before its first step
    assert all(set(c) == weights for c in t["casts"]), "torch loop: every weight re-cast each step"
    assert set(f["casts"][0]) == weights and f["casts"][1] == [] and f["casts"][2] == [], f["casts"][1:]
    # gradients of weights are widened straight into their bucket slots; a weight that goes through shadow() twice in one step
    # (the first block of a decoder that runs a shared prefix and a suffix on the same qkv weight) has two backward nodes,
    # autograd sums their outputs out of place, and the reducer copies that sum once
    once = weights - f["multi_use"]
    assert len(once) > 20 and not (set(f["copied"]) & once), sorted(set(f["copied"]) & once)
    print(f"fixture {fixture}: {len(weights)} shadowed weights, copied: {sorted(set(f['copied']) & weights)} "
          f"(used twice: {sorted(f['multi_use'])})")
    # step 1: identical gradients (same kernels, same weights); the only difference is the clip norm (torch: norm of per-tensor
    # norms; here: one fp32 sum of squares) -> coefficient ratio 1 + d, and the kernel's own rounding (TOL): parameters within
    # TOL + d relative to their operands, first moments likewise
    assert f["loss"][0] == t["loss"][0]
    d = abs(f["norm"][0] / t["norm"][0] - 1.0)
    assert d <= 1e-5, d
    tol1 = TOL + 2 * d
    for n in t["params"][0]:
        a, r, p0 = f["params"][0][n], t["params"][0][n], t["init"][n]
        assert float(((a - r).abs() - tol1 * (r.abs() + p0.abs() + 1e-3)).max()) <= 1e-30, n
        if n in t["m"][0]:
            ma, mr = f["m"][0][n], t["m"][0][n]
            assert float(((ma - mr).abs() - tol1 * mr.abs() - 1e-30).max()) <= 0, n
        else:
            assert n not in f["m"][0], n
    # steps 2-3: the masters differ by fp32 ulps, which flips the bf16 rounding of a few shadow elements; the losses then differ
    # at bf16-noise level and Adam's sign-like early updates (m / sqrt(v) = +-1 whatever the gradient's size) turn that into
    # O(lr) differences on elements whose gradient is at noise level: compared by the L2 of the parameter updates, with the bound
    # tests/test_ddp_one_gpu.py uses for the same effect (a stale shadow is excluded directly above: the handed-over shadows are
    # checked bit for bit against the masters after every step)
    # The losses move by 0.1-0.2 from step to step here (lr 1e-3 on sign-like updates of every parameter).  Measured: fixture B
    # stays at update rel-L2 1e-4 / 1e-3 (steps 2 / 3); in fixture A the depth decoder's MLP weights diverge as whole tensors
    # (update rel-L2 0.19 / 0.25, loss 0.4 % apart at step 3).  1 % of the loss is a few percent of one step's change.
    for k in (1, 2):
        assert abs(f["loss"][k] - t["loss"][k]) <= 1e-2 * abs(t["loss"][k]), (k, f["loss"], t["loss"])
        num = den = 0.0
        per = []
        for n in t["params"][k]:
            dn = float((f["params"][k][n] - t["params"][k][n]).norm()) ** 2
            num += dn
            den += float((t["params"][k][n] - t["init"][n]).norm()) ** 2
            per.append((dn, n))
        print(f"fixture {fixture} step {k + 1}: largest update differences", sorted(per)[-4:])
        assert den > 0 and (num / den) ** 0.5 < 0.35, (k, (num / den) ** 0.5, sorted(per)[-4:])
        mn = sum(float((f["m"][k][n] - t["m"][k][n]).norm()) ** 2 for n in t["m"][k])
        md = sum(float(t["m"][k][n].norm()) ** 2 for n in t["m"][k])
        assert (mn / md) ** 0.5 < 0.35, (k, (mn / md) ** 0.5)
        print(f"fixture {fixture} step {k + 1}: update rel-L2 {(num / den) ** 0.5:.3g}, exp_avg rel-L2 {(mn / md) ** 0.5:.3g}")
    # parameters without a gradient are untouched by both
    assert len(f["unused"]) > 0
    for n in f["unused"]:
        assert torch.equal(f["params"][-1][n], f["init"][n]) and torch.equal(t["params"][-1][n], t["init"][n]), n


# ----------------------------------------------------------------------------------------------------------------------------
# two gloo ranks sharing the GPU, master mode (tests/test_ddp_one_gpu.py does the same for bf16 parameters)
# ----------------------------------------------------------------------------------------------------------------------------
def _ddp_worker(rank, world, port, fixture, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    from tests.test_ddp_one_gpu import STEPS, _dit_noise, _loss
    m, cfg, S, batch, losses = _shipped_model(fixture)
    params = [p for p in m.parameters() if p.requires_grad]
    red = GradBucketReducer(params, bucket_bytes=8 << 20, direct_grads=True)
    opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1)
    assert opt.master_mode
    rows = slice(2 * rank, 2 * rank + 2)
    sel = list(range(2 * rank, 2 * rank + 2))
    unused = None
    for step in range(STEPS):
        opt.zero_grad()
        _loss(m, cfg, S, batch, losses, rows, _dit_noise(cfg, S, 2, 100 + step, sel)).backward()
        red.finish()
        if step == 0:
            fired = {id(bp) for b in red.buckets for bp, f in zip(b["params"], b["fired"]) if f}
            unused = sorted(n for n, p in m.named_parameters() if p.requires_grad and id(p) not in fired)
            if rank == 0:
                q.put(("grads", {n: red.grad_of(p).detach().cpu().numpy().copy() for n, p in m.named_parameters()
                                 if p.requires_grad}))
        opt.step()
    torch.cuda.synchronize()
    if rank == 0:
        q.put(("final", {n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters() if p.requires_grad}))
        q.put(("meta", {"buckets": len(red.buckets), "unused": unused}))
    dist.barrier()
    dist.destroy_process_group()


def _ddp_single(fixture):
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    from tests.test_ddp_one_gpu import STEPS, _dit_noise, _loss
    m, cfg, S, batch, losses = _shipped_model(fixture)
    params = [p for p in m.parameters() if p.requires_grad]
    init = {n: p.detach().cpu().clone() for n, p in m.named_parameters() if p.requires_grad}
    red = GradBucketReducer(params, bucket_bytes=8 << 20)
    opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1)
    grads0 = None
    for step in range(STEPS):
        opt.zero_grad()
        _loss(m, cfg, S, batch, losses, slice(0, 4), _dit_noise(cfg, S, 4, 100 + step, [0, 1, 2, 3])).backward()
        red.finish()
        if step == 0:
            grads0 = {n: red.grad_of(p).detach().cpu().clone() for n, p in m.named_parameters() if p.requires_grad}
        opt.step()
    torch.cuda.synchronize()
    return grads0, {n: p.detach().cpu().clone() for n, p in m.named_parameters() if p.requires_grad}, init


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("fixture", ["A", "B"], ids=["mlp_head_obs_depth_sam", "dit_head"])
def test_two_ranks_master_mode_match_the_full_batch_run(fixture):
    from tests.test_ddp_one_gpu import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, fixture, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(3):
        k, v = q.get(timeout=600)
        got[k] = v
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    ref_grads, ref_final, init = _ddp_single(fixture)
    meta = got["meta"]
    assert meta["buckets"] >= 2 and len(meta["unused"]) > 0, meta
    # step-0 gradients: the fp32 average of two half-batch gradients against the full-batch one.  Weight gradients are bf16 GEMM
    # results widened to fp32 (each half rounds on its own), the rest fp32: the bf16-ulp scale of tests/test_ddp_one_gpu.py
    worst, n = (0.0, ""), 0
    for name, g_ref in ref_grads.items():
        g = torch.from_numpy(got["grads"][name])
        assert g.dtype == torch.float32
        den = float(g_ref.norm())
        if den == 0.0:
            assert float(g.norm()) == 0.0, name
            continue
        r = float((g - g_ref).norm()) / den
        n += 1
        worst = max(worst, (r, name))
    assert n > 100 and worst[0] < 2e-2, worst
    # after three steps: L2 of the updates (Adam's sign-like first steps; see tests/test_ddp_one_gpu.py), unused untouched
    num = den = 0.0
    for name, p_ref in ref_final.items():
        fin = torch.from_numpy(got["final"][name])
        num += float((fin - p_ref).norm()) ** 2
        den += float((p_ref - init[name]).norm()) ** 2
        if name in meta["unused"]:
            assert torch.equal(fin, init[name]) and torch.equal(p_ref, init[name]), name
    assert den > 0 and (num / den) ** 0.5 < 0.35, (num, den)
