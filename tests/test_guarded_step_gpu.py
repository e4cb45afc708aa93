"""GPU: FlatAdamW(skip_nonfinite=True) -- dvla_step_verdict + dvla_adamw_bf16_guarded / dvla_adamw_f32_master_guarded.

Everything here is bit for bit (buffers are compared as integers): a guarded run without a bad step IS the unguarded run, and a
guarded run with bad steps IS the unguarded run on the good gradients alone -- which is what proves that the bias corrections
follow the number of applied steps.

Buckets are a few thousand elements long and no multiple of 8 (3015 = 8 * 376 + 7 and 3005 = 8 * 375 + 5: two blocks of the
vector loop and the ragged tail of both kernels).  GradBucketReducer pads every parameter to 128 elements, so a stand-in with
the same fields carries them; the two-rank case uses the real reducer."""
import copy
import functools
import os
import warnings

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_master_adamw_gpu import _set_grads

BF, F32 = torch.bfloat16, torch.float32
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2
LAYOUT = {"bf16": [(BF, [(1300,), (1711,)]), (BF, [(3005,)])],
          "f32": [(F32, [(1300,), (1711,)]), (F32, [(5, 601)])],
          "mixed": [(BF, [(1300,), (1711,)]), (F32, [(5, 601)])]}
MODES = ["bf16", "f32", "mixed"]
NORMS = [0.1, None]
POISON = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}


class _Buckets:
    """the fields FlatAdamW reads of a gradient reducer, over buckets whose length is the test's choice: parameters start on
    multiples of 8 elements and the last one is not padded"""

    def __init__(self, groups):
        self.params = [p for g in groups for p in g]
        self.buckets = []
        for g in groups:
            offsets, off, end = [], 0, 0
            for p in g:
                offsets.append(off)
                end = off + p.numel()
                off = -(-end // 8) * 8
            flat = torch.zeros(end, dtype=g[0].dtype, device="cuda")
            for p, o in zip(g, offsets):
                p._dvla_grad_view = flat[o:o + p.numel()].view_as(p)
            self.buckets.append({"flat": flat, "params": list(g), "offsets": offsets, "expected": [True] * len(g)})

    def grad_of(self, p):
        return p._dvla_grad_view

    def zero_grad(self):
        for b in self.buckets:
            b["flat"].zero_()


@functools.lru_cache(maxsize=None)
def _init(mode):
    gen = torch.Generator().manual_seed(11)
    return [[(torch.randn(s, generator=gen) * 0.5).to(dt).cuda() for s in shapes] for dt, shapes in LAYOUT[mode]]


@functools.lru_cache(maxsize=None)
def _grads(mode, k):
    """the k-th good gradient of every parameter (read-only: poisoned copies are made by _poisoned)"""
    gen = torch.Generator().manual_seed(1000 + k)
    return [(torch.randn(s, generator=gen) * 0.3).to(dt).cuda() for dt, shapes in LAYOUT[mode] for s in shapes]


def _poisoned(grads, where, value):
    grads = [g.clone() for g in grads]
    if where == "first":                 # element 0 of bucket 0
        grads[0].view(-1)[0] = value
    elif where == "last_tail":           # the last element of the last bucket: in the ragged tail (3005 = 8 * 375 + 5)
        grads[-1].view(-1)[-1] = value
    else:                                # "fp32_only": somewhere in the vector body of the mixed mode's fp32 bucket
        assert grads[-1].dtype == F32 and grads[0].dtype == BF
        grads[-1].view(-1)[1234] = value
    return grads


def _make(mode, max_norm, guard):
    from dreamvla_amd.optim import FlatAdamW
    red = _Buckets([[torch.nn.Parameter(p.clone()) for p in g] for g in _init(mode)])
    assert [b["flat"].numel() % 8 for b in red.buckets] == [7, 5]
    opt = FlatAdamW(red, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm, skip_nonfinite=guard)
    assert opt.master_mode == (mode != "bf16")
    return red, opt


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _snap(opt, keys=("p", "m", "v", "sh")):
    """parameters, both moments and the shadows of every bucket, as integers"""
    return [_bits(s[k]).clone() for s in opt.flat for k in keys if k in s]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _run(mode, max_norm, guard, seq):
    """step through the gradients `seq` with no host synchronisation in between -> (reducer, optimizer, snapshot and norm bits per step)"""
    red, opt = _make(mode, max_norm, guard)
    snaps, norms = [], []
    for g in seq:
        _set_grads(red, g)
        opt.step()
        snaps.append(_snap(opt))
        norms.append(_bits(opt.grad_norm()).clone())
    return red, opt, snaps, norms


@functools.lru_cache(maxsize=None)
def _control(mode, max_norm, ks):
    """the unguarded optimizer on the good gradients ks (shared, read-only)"""
    _, _, snaps, norms = _run(mode, max_norm, False, [_grads(mode, k) for k in ks])
    return snaps, norms


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_without_a_bad_step_the_guarded_run_is_the_unguarded_run(mode, max_norm):
    ks = tuple(range(12))
    ref, _ = _control(mode, max_norm, ks)
    _, ref_norms = _control(mode, 0.1, ks)       # the unguarded step computes the norm only when it clips: same gradients, same sum
    _, opt, snaps, norms = _run(mode, max_norm, True, [_grads(mode, k) for k in ks])
    for k in ks:
        assert _same(snaps[k], ref[k]), f"step {k + 1}"
        assert torch.equal(norms[k], ref_norms[k]), f"grad_norm() of step {k + 1}"
    h = opt.health()
    assert int(h["applied"]) == 12 and int(h["skipped"]) == 0 and int(h["last_ok"]) == 1
    assert torch.equal(_bits(h["last_grad_norm"]).reshape(1), ref_norms[-1])
    assert opt.applied_steps == 12 and opt.skipped_steps == 0
    assert int(opt._state_view("faults", torch.int64)[0]) == 0


def _poison_cases():
    for mode in MODES:
        for where in ("first", "last_tail") + (("fp32_only",) if mode == "mixed" else ()):
            yield mode, where


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
@pytest.mark.parametrize("value", list(POISON))
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode,where", list(_poison_cases()))
def test_one_poisoned_step_changes_nothing_and_does_not_count(mode, where, max_norm, value):
    seq = [_grads(mode, 0), _poisoned(_grads(mode, 1), where, POISON[value]), _grads(mode, 2), _grads(mode, 3)]
    ref, ref_norms = _control(mode, max_norm, (0, 2, 3))
    _, opt, snaps, norms = _run(mode, max_norm, True, seq)
    assert _same(snaps[0], ref[0])
    assert _same(snaps[1], snaps[0]), "the poisoned step touched a buffer"
    assert _same(snaps[2], ref[1])
    assert _same(snaps[3], ref[2]), "not the unguarded run on g1, g3, g4: wrong bias-correction index"
    assert not bool(torch.isfinite(norms[1].view(torch.float32)).any())
    h = opt.health()
    assert int(h["applied"]) == 3 and int(h["skipped"]) == 1 and int(h["last_ok"]) == 1
    bad_bucket = 0 if where == "first" else 1
    assert (~torch.isfinite(h["skipped_bucket_norms"])).tolist() == [i == bad_bucket for i in range(2)]
    assert int(h["last_skipped_step"]) == 2
    assert opt.applied_steps == 3 and opt.skipped_steps == 1
    assert opt.bucket_parameters(0) == [0, 1] and opt.bucket_parameters(1) == [2]


@pytest.mark.gpu
def test_first_confirmed_skip_warns_once_and_names_step_and_bucket():
    mode = "mixed"
    seq = [_grads(mode, 0), _poisoned(_grads(mode, 1), "fp32_only", POISON["nan"]), _grads(mode, 2),
           _poisoned(_grads(mode, 3), "first", POISON["inf"])]
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        _, opt, _, _ = _run(mode, 0.1, True, seq)
        assert opt.skipped_steps == 2
    got = [str(w.message) for w in got if issubclass(w.category, RuntimeWarning) and "FlatAdamW" in str(w.message)]
    # one warning.  It names the step whose record it read from the device together with that step's buckets: step 2 (the fp32
    # bucket), or step 4 (bucket 0) if that had already run when step 2 was confirmed -- then step 2 is named as the first
    assert len(got) == 1, got
    assert ("step 2 was skipped: non-finite gradient in bucket(s) [1];" in got[0]
            or ("step 4 was skipped: non-finite gradient in bucket(s) [0] (the first confirmed skip was step 2)" in got[0])), got


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
@pytest.mark.parametrize("max_norm", NORMS, ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_twenty_steps_back_to_back_four_of_them_poisoned(mode, max_norm):
    """nothing between the steps waits for the device, so the window of 8 unconfirmed steps fills and step() itself waits for
    the oldest readback; steps 3, 4, 5 and 17 (1-based) are bad, three of them in a row"""
    bad = {3: ("first", "nan"), 4: ("last_tail", "inf"), 5: ("first", "-inf"), 17: ("last_tail", "nan")}
    seq, good = [], []
    for k in range(20):
        if k + 1 in bad:
            where, value = bad[k + 1]
            seq.append(_poisoned(_grads(mode, k), where, POISON[value]))
        else:
            seq.append(_grads(mode, k))
            good.append(k)
    torch.cuda.synchronize()
    red, opt = _make(mode, max_norm, True)
    inflight = []
    issued = opt._ledger.issued
    opt._ledger.issued = lambda ticket: (issued(ticket), inflight.append(opt._ledger.inflight))
    # these steps are a few microseconds of device work each, so the host would never get ahead of them: put ~0.2 s of
    # element-wise work in front (no synchronisation), behind which the steps queue up until the window is full
    ballast = torch.empty(1 << 28, device="cuda")
    for _ in range(40):
        ballast.normal_()
    for g in seq:
        _set_grads(red, g)
        opt.step()
    assert max(inflight) == opt.WINDOW, inflight         # step() itself waited for the oldest readback, and for nothing more
    del ballast
    ref, _ = _control(mode, max_norm, tuple(good))
    assert _same(_snap(opt), ref[-1])
    assert opt.applied_steps == 16 and opt.skipped_steps == 4
    assert int(opt._state_view("faults", torch.int64)[0]) == 0
    assert opt._ledger.inflight == 0


@pytest.mark.gpu
def test_finite_gradients_whose_norm_overflows_are_skipped():
    mode = "f32"
    red, opt = _make(mode, 0.1, True)
    before = _snap(opt, ("p", "m", "v"))         # (the shadows are first written by the first step, applied or not: see below)
    _set_grads(red, [torch.full_like(g, 1e20) for g in _grads(mode, 0)])
    opt.step()
    with pytest.warns(RuntimeWarning, match="step 1 "):
        assert opt.skipped_steps == 1 and opt.applied_steps == 0
    assert _same(_snap(opt, ("p", "m", "v")), before)
    assert float(opt.grad_norm()) == float("inf")
    _set_grads(red, _grads(mode, 0))
    opt.step()
    ref, _ = _control(mode, 0.1, (0,))
    assert _same(_snap(opt), ref[0]) and opt.applied_steps == 1


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
def test_a_skipped_first_step_leaves_current_shadows_behind():
    """the unguarded step always rewrites the bf16 shadows it hands to dreamvla_amd.ops; a skipped one writes nothing, so what it
    hands over must be current by other means -- also after the masters were rewritten from outside (a checkpoint load)"""
    from dreamvla_amd import ops
    mode = "f32"
    red, opt = _make(mode, 0.1, True)
    bad = _poisoned(_grads(mode, 0), "first", POISON["nan"])

    def served():
        for p in red.params:
            ent = ops._Shadow.cache.get(id(p))
            assert ent is not None and ent[0]() is p and ent[1] == p._version and ent[2] == p.data_ptr()
            assert torch.equal(_bits(ent[4]), _bits(ops.cast_to(p.detach(), BF)))

    _set_grads(red, bad)
    opt.step()
    served()
    with torch.no_grad():
        for p in red.params:
            p.mul_(1.5)                  # through the parameter: its version moves
    _set_grads(red, bad)
    opt.step()
    served()
    _set_grads(red, _grads(mode, 0))
    opt.step()
    served()
    assert opt.applied_steps == 1 and opt.skipped_steps == 2


@functools.lru_cache(maxsize=None)
def _checkpoint_case():
    """master mode, g1 g2* g3 g4 under the guard, then the checkpoint; one further step (g5) of the optimizer itself, of a fresh
    guarded FlatAdamW that loaded the checkpoint, and of a torch.optim.AdamW that loaded it (all over clones of the parameters)"""
    from dreamvla_amd.optim import FlatAdamW
    mode = "f32"
    seq = [_grads(mode, 0), _poisoned(_grads(mode, 1), "last_tail", POISON["nan"]), _grads(mode, 2), _grads(mode, 3)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        red, opt, _, _ = _run(mode, None, True, seq)
        sd = opt.state_dict()
    g5 = _grads(mode, 4)
    pt = [torch.nn.Parameter(p.detach().clone()) for p in red.params]
    p_saved = [p.detach().clone() for p in red.params]
    opt_t = torch.optim.AdamW(pt, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    opt_t.load_state_dict(copy.deepcopy(sd))          # (torch adopts the dict's step tensors and counts on in them: a copy)
    for p, g in zip(pt, g5):
        p.grad = g.clone()
    opt_t.step()
    red2 = _Buckets([[torch.nn.Parameter(p.detach().clone()) for p in b["params"]] for b in red.buckets])
    opt2 = FlatAdamW(red2, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    counts = [(opt2.applied_steps, opt2.skipped_steps)]
    plain = {"state": sd["state"], "param_groups": [{k: v for k, v in sd["param_groups"][0].items() if k != "skipped_steps"}]}
    opt2.load_state_dict(plain)          # a dict without the key: no skips on record
    counts.append((opt2.applied_steps, opt2.skipped_steps))
    for r, o in ((red, opt), (red2, opt2)):
        _set_grads(r, g5)
        o.step()
    torch.cuda.synchronize()
    return {"sd": sd, "red": red, "opt": opt, "red2": red2, "opt2": opt2, "pt": pt, "opt_t": opt_t, "counts": counts, "p_saved": p_saved}


@pytest.mark.gpu
def test_checkpoint_stores_the_applied_count_and_loads_into_torch_adamw_and_back():
    from dreamvla_amd.optim import FlatAdamW
    c = _checkpoint_case()
    sd = c["sd"]
    assert sorted(sd["state"]) == [0, 1, 2] and all(float(st["step"]) == 3.0 for st in sd["state"].values())
    assert sd["param_groups"][0]["skipped_steps"] == 1
    assert c["counts"] == [(3, 1), (3, 0)]
    # the reloaded guarded optimizer continues exactly as the one that wrote the checkpoint
    assert _same(_snap(c["opt"]), _snap(c["opt2"]))
    assert c["opt"].applied_steps == 4 and c["opt2"].applied_steps == 4
    assert float(c["opt"].state_dict()["state"][0]["step"]) == 4.0
    # torch.optim.AdamW took the dict, extra key and all, and counted on from 3; its moments after the further step are the
    # kernel's bit for bit (its parameters: the next test)
    sd4 = c["opt"].state_dict()["state"]
    for i, p in enumerate(c["pt"]):
        st = c["opt_t"].state[p]
        assert float(st["step"]) == 4.0
        assert torch.equal(_bits(st["exp_avg"]), _bits(sd4[i]["exp_avg"])) and torch.equal(_bits(st["exp_avg_sq"]), _bits(sd4[i]["exp_avg_sq"]))
    # the guard off: a dict with the key loads, and the dict written is today's
    red3 = _Buckets([[torch.nn.Parameter(p.detach().clone()) for p in b["params"]] for b in c["red"].buckets])
    opt3 = FlatAdamW(red3, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    opt3.load_state_dict(sd)
    assert opt3.step_count == 3 and "skipped_steps" not in opt3.state_dict()["param_groups"][0]


@pytest.mark.gpu
def test_checkpoint_continues_in_torch_adamw():
    """One further step of torch.optim.AdamW (default foreach path) from the guarded optimizer's checkpoint against the optimizer's
    own further step.  The moments agree bit for bit (the test above).  The parameters cannot: the guarded step runs
    dvla_adamw_f32_master's element function, which must stay as it is, and that takes sqrt(v) with __fsqrt_rn -- the native
    v_sqrt_f32 of the HIP headers, good to one ulp, where torch's sqrt is correctly rounded.
    Bound, per element: both sides round the new parameter once, so each is within half an ulp of its own exact value, and the
    exact values differ by the relative error of sqrt(v) (<= 2^-23, carried through one division: <= 2^-22, taken as 2^-21)
    times the size of the update u = |p_new - p (1 - lr wd)|:  |x - t| <= ulp(max(|x|, |t|)) + 2^-21 u.  For all but
    parameters that the update nearly cancels that is one ulp.  Also held: the bound
    tests/test_master_adamw_gpu.py::test_checkpoint_round_trips_with_torch_adamw puts on the unguarded path.
    Measured: 2 of 6016 elements differ, by one ulp each."""
    from tests.test_master_adamw_gpu import TOL
    c = _checkpoint_case()
    differing, worst = 0, 0
    for a, t, p0 in zip(c["red"].params, c["pt"], c["p_saved"]):
        a, t = a.detach(), t.detach()
        d = (_bits(a).long() - _bits(t).long()).abs()       # (for reporting) the distance in ulps
        differing += int((d != 0).sum())
        worst = max(worst, int(d.max()))
        big = torch.maximum(a.abs(), t.abs())
        ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
        u = (t.double() - p0.double() * (1.0 - LR * WD)).abs()
        assert bool(((a.double() - t.double()).abs() <= ulp + 2.0 ** -21 * u).all())
        assert float((a.double() - t.double()).abs().max()) <= 3 * TOL * float(t.double().abs().max()) + 1e-30
    total = sum(p.numel() for p in c["pt"])
    print(f"torch.optim.AdamW vs the guarded step after one further step: {differing} of {total} parameter elements differ, "
          f"at most {worst} ulp")


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:FlatAdamW. step:RuntimeWarning")
def test_bf16_checkpoint_round_trip_keeps_both_counts():
    mode = "bf16"
    seq = [_grads(mode, 0), _poisoned(_grads(mode, 1), "first", POISON["inf"]), _grads(mode, 2)]
    red, opt, _, _ = _run(mode, 0.1, True, seq)
    sd = opt.state_dict()
    assert sd["step"] == 2 and sd["param_groups"][0]["skipped_steps"] == 1
    red2, opt2 = _make(mode, 0.1, True)
    for p, q in zip(red2.params, red.params):
        p.data.copy_(q.data)
    opt2.load_state_dict(sd)
    assert "skipped_steps" not in opt2.param_groups[0]
    for r, o in ((red, opt), (red2, opt2)):
        _set_grads(r, _grads(mode, 3))
        o.step()
    assert _same(_snap(opt), _snap(opt2))
    assert (opt2.applied_steps, opt2.skipped_steps) == (3, 1)


# ----------------------------------------------------------------------------------------------------------------------------
# two gloo ranks sharing the GPU: only rank 1's local gradient is bad, both ranks skip (the verdict is taken on the reduced bucket)
# ----------------------------------------------------------------------------------------------------------------------------
DDP_SHAPES = [(300,), (16, 40), (129,), (64, 24)]


def _ddp_init():
    gen = torch.Generator().manual_seed(21)
    return [torch.randn(s, generator=gen) * 0.5 for s in DDP_SHAPES]


def _ddp_coefs(rank, step):
    """the local gradient of loss = sum(p * c): c itself; rank 1's is +inf in one element at step 2 (index 1)"""
    gen = torch.Generator().manual_seed(100 * rank + step)
    cs = [torch.randn(s, generator=gen) * 0.3 for s in DDP_SHAPES]
    if rank == 1 and step == 1:
        cs[2][5] = float("inf")
    return cs


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    warnings.simplefilter("ignore", RuntimeWarning)
    ps = [torch.nn.Parameter(p.cuda()) for p in _ddp_init()]
    red = GradBucketReducer(ps, bucket_bytes=4096, last_bucket_bytes=0)
    opt = FlatAdamW(red, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.1, skip_nonfinite=True)
    for step in range(4):
        opt.zero_grad()
        sum((p * c.cuda()).sum() for p, c in zip(ps, _ddp_coefs(rank, step))).backward()
        red.finish()
        opt.step()
    q.put((rank, len(red.buckets), opt.applied_steps, opt.skipped_steps, [p.detach().cpu().numpy().copy() for p in ps]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_reach_the_same_verdict_without_communication():
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    from tests.test_ddp_one_gpu import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        r = q.get(timeout=240)
        got[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the control: one process, guard off, the averaged gradients of steps 1, 3 and 4 (gloo sums on the host in fp32 and the
    # reducer divides by the world size: (c0 + c1) / 2, the same two roundings here)
    ps = [torch.nn.Parameter(p.cuda()) for p in _ddp_init()]
    red = GradBucketReducer(ps, bucket_bytes=4096, last_bucket_bytes=0)
    opt = FlatAdamW(red, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.1)
    for step in (0, 2, 3):
        opt.zero_grad()
        for p, c0, c1 in zip(ps, _ddp_coefs(0, step), _ddp_coefs(1, step)):
            red.grad_of(p).copy_(((c0 + c1) / 2).cuda())
        opt.step()
    torch.cuda.synchronize()
    for rank in (0, 1):
        buckets, applied, skipped, final = got[rank]
        assert buckets >= 2 and (applied, skipped) == (3, 1), (rank, buckets, applied, skipped)
        for p, f in zip(ps, final):
            assert torch.equal(_bits(p.detach().cpu()), _bits(torch.from_numpy(f))), f"rank {rank}"
