"""Fused gradient clipping + AdamW over the flat buffers of the data-parallel gradient reducer.

The reference's step is caller code: `torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)` followed by
`torch.optim.AdamW.step()` (train.py / utils/train_utils.py:600-608), i.e. ~80 multi-tensor launches over ~1000
tensors.  Here every trainable parameter is re-homed as a view into one flat bf16 buffer per gradient bucket of
`dreamvla_amd.ddp.GradBucketReducer` (same element order as the bucket), both moments are flat too, and a step is
`dvla_sumsq_bf16` per bucket (gradient norm, accumulated into one device scalar -- no host synchronisation) plus
`dvla_adamw_bf16` per bucket.  Element-wise semantics are those of torch's AdamW with bf16 parameters (moments kept in
bf16, math in fp32) and of `clip_grad_norm_` (scaled gradient rounded to bf16).

Master mode (the shipped `--precision fp32 --bf16_module vision_encoder` runs): buckets of fp32 parameters are re-homed the
same way into flat fp32 master buffers with fp32 moments, clipped by `dvla_sumsq_f32` into the same device scalar and stepped
by `dvla_adamw_f32_master` (torch's foreach AdamW on fp32 parameters, clip in fp32), which also writes the bf16 compute
shadow of every master into one flat bf16 buffer per bucket.  After the step those buffers ARE the shadows
`dreamvla_amd.ops.shadow` multiplies on: the next forward issues no fp32 -> bf16 cast for a trainable weight.  A reducer
may mix bf16 and fp32 buckets; one clip norm spans both.  With any fp32 bucket, `state_dict()` is torch.optim.AdamW's
format (indexed in `reducer.params` order), so checkpoints move between this optimizer and the reference's loop.

Guarded step (`skip_nonfinite=True`, an addition): the sums of squares go into one slot per bucket,
`dvla_step_verdict` adds them, decides on the device whether the step is applied and picks the bias corrections of the step
count that is then current, and `dvla_adamw_bf16_guarded` / `dvla_adamw_f32_master_guarded` do nothing on a skipped step.

EMA of the weights (`ema_decay=...`, an addition): one fp32 EMA buffer per bucket, updated by the step kernels
themselves (`dvla_adamw_*_ema`, `dvla_adamw_*_ema_guarded`: e <- lerp(e, p, 1 - decay) on the parameter just written, ATen's
lerp bit for bit), and exchanged with the weights for evaluation by `dvla_ema_swap_f32` / `dvla_ema_swap_bf16`.

Parameter groups (`param_groups=[...]`, an addition): with two or more groups a step is one
`dvla_adamw_bf16_grouped` / `dvla_adamw_f32_master_grouped` launch per bucket; a map of one byte per 8 elements tells the kernel
which group's lr and weight decay a vector takes, guard and EMA included.  `weight_decay_groups` builds the usual two groups.

Stochastic rounding (`stochastic_rounding=True`, an addition): bf16 buckets are stepped by `dvla_adamw_bf16_sr`,
which stores parameters and both moments rounded up with a probability equal to the discarded fraction, from counter-based random
bits (include/dvla.h); launch for launch the step of the same combination of guard, EMA and groups.

Per-parameter statistics (`parameter_stats()`, `stats_by_module`, an addition): every parameter is a segment of the
flat buffers, so `dvla_segment_stats_*` / `dvla_segment_adam_*` (one launch per bucket and buffer) and `dvla_segment_combine` (one
launch) give per-parameter gradient and parameter norms, absmax and non-finite counts and the norm of the Adam update, with no
atomics, no host synchronisation and no change to the step.

Per-group clipping (`clip="group"`, an addition): every parameter group has its own clip norm and max_grad_norm.
The per-parameter sums of squares of that segmented reduction, added per group by `dvla_group_sumsq`, replace the `dvla_sumsq_*`
pass, and `dvla_adamw_*_grouped_clip` / `dvla_adamw_bf16_sr_clip` look the coefficient up per group next to lr and weight decay:
still one launch per bucket.  `prefix_groups` cuts a model into such groups by parameter name.
"""
import collections
import contextlib
import ctypes
import math
import operator
import types
import warnings

import torch

from . import _lib, ops
from ._lib import check


class _StepLedger:
    """Host-side account of the guarded steps that are enqueued but not yet known to be applied or skipped (pure Python).

    Every step ends in a readback (applied, skipped, faults, ok, sumsq -- the device's counters after that step) that completes
    some time later.  A `ticket` stands for one readback: `ticket.done()` -> bool without blocking, `ticket.wait()` blocks until
    it is there, `ticket.read()` returns the five values.  `begin()` retires, oldest first, every ticket that is done, which gives
    `confirmed_applied`; the `inflight` steps behind it may each have been applied or not, so the step about to be issued finds
    confirmed_applied + j steps applied for some j in 0 .. inflight, and `candidates()` lists the step counts
    confirmed_applied + 1 + j its bias corrections may need.  With `window` steps in flight `begin()` waits for the oldest -- the
    only place that blocks besides `drain()`.  A readback with faults != 0 (the device found its count outside the table it
    was given) raises RuntimeError."""

    def __init__(self, applied=0, skipped=0, window=8, on_skip=None):
        self.window = int(window)
        self.on_skip = on_skip              # called with the 1-based number of a step once it is confirmed skipped
        self.reset(applied, skipped)

    def reset(self, applied=0, skipped=0):
        """forget what is in flight; the device's counters are (applied, skipped) from here on"""
        self.confirmed_applied, self.confirmed_skipped = int(applied), int(skipped)
        self._pending = collections.deque()

    @property
    def inflight(self):
        return len(self._pending)

    def _retire(self, ticket):
        applied, skipped, faults, ok, _ = ticket.read()
        if faults:
            raise RuntimeError(f"guarded optimizer step: the device counted {int(faults)} step(s) whose applied count lay outside "
                               f"the candidates it was given (host confirmed {self.confirmed_applied}, device {int(applied)}): "
                               f"the optimizer state was changed behind the optimizer's back")
        self.confirmed_applied, self.confirmed_skipped = int(applied), int(skipped)
        if not ok and self.on_skip is not None:
            self.on_skip(int(applied) + int(skipped))

    def begin(self):
        """start of a step: -> (confirmed_applied, number of candidates)"""
        while self._pending and self._pending[0].done():
            self._retire(self._pending.popleft())
        while len(self._pending) >= self.window:
            ticket = self._pending.popleft()
            ticket.wait()
            self._retire(ticket)
        return self.confirmed_applied, len(self._pending) + 1

    def candidates(self):
        return [self.confirmed_applied + 1 + j for j in range(len(self._pending) + 1)]

    def issued(self, ticket):
        self._pending.append(ticket)

    def drain(self):
        """wait for everything in flight (blocks)"""
        while self._pending:
            ticket = self._pending.popleft()
            ticket.wait()
            self._retire(ticket)


class _Readback:
    """one slot of the pinned ring + the event recorded behind the copy into it (a _StepLedger ticket)"""

    def __init__(self, slot):
        self.slot = slot                                   # 32 pinned bytes: the head of dvla_step_state
        self.event = torch.cuda.Event()

    def done(self):
        return self.event.query()

    def wait(self):
        self.event.synchronize()

    def read(self):
        i64, i32, f32 = self.slot.view(torch.int64), self.slot.view(torch.int32), self.slot.view(torch.float32)
        return int(i64[0]), int(i64[1]), int(i64[2]), int(i32[6]), float(f32[7])


class FlatAdamW(torch.optim.Optimizer):
    """torch.optim.Optimizer surface (param_groups with `lr` -- so torch's LR schedulers, which the reference attaches to its
    AdamW (train.py:176-200), drive it unchanged --, state_dict / load_state_dict for checkpoint / resume) over flat buffers.
    Parameters the reducer has learned never to receive a gradient (the reference's constructed-but-unused modules) are left
    alone -- no weight decay, no moment update -- exactly as torch's AdamW skips `p.grad is None` parameters.

    skip_nonfinite=True (off by default; nothing above changes with it off): a step whose gradient holds a NaN or an inf
    leaves every parameter, moment and shadow untouched and is counted, decided on the device with no host synchronisation.
    The gradient norm is computed for the verdict also when max_grad_norm is None (clipping stays off).  The bias
    corrections follow the number of APPLIED steps, so the run continues exactly as if the bad batch had not been there: an
    applied step is the unguarded step, bit for bit.  `health()` gives the counters as device tensors,
    `applied_steps` / `skipped_steps` as host ints (these wait for the device), `bucket_parameters(i)` names what lives in a
    bucket; the first confirmed skip raises one RuntimeWarning (that one reads the per-bucket record back, synchronously).
    Under data parallelism every rank steps on the same reduced buckets, so every rank reaches the same verdict without
    talking to the others.  Not covered: a torch LR scheduler (or GradScaler) stepped on the host advances on skipped steps
    too; the guarded step copies 32 bytes back per step and is therefore not graph-capturable; finite gradients whose norm
    overflows fp32 are skipped as well.  With the guard on, `step_count` is the applied count last confirmed by the device
    (it lags by up to WINDOW steps; `applied_steps` is exact).

    ema_decay=d, 0 < d < 1 (None by default: no buffer, and the launches above): every bucket also carries an fp32 EMA of
    its parameters (fp32 for bf16 buckets too: 1 - d is below a bf16 ulp), initialised from them here and updated inside the
    step kernel, e <- lerp(e, p, 1 - d(t)) on the stored parameter, bit for bit what `ema.lerp_(p.float(), 1 - d(t))` gives;
    parameters, moments and shadows are those of the step without it.  ema_warmup=True: d(t) = min(d, (1 + t) / (10 + t)),
    t the 1-based count of applied steps (a skipped step neither moves the EMA nor advances t).  Parameters that receive no
    gradient keep their initial copy.  `ema_weights()` is the context in which the model computes on the EMA;
    `ema_model_state_dict(model)` the state dict an evaluation script loads; `ema_state_dict()` / `load_ema_state_dict()`
    the checkpoint (state_dict() / load_state_dict() keep their formats and do not touch the EMA); `ema_reset()` restarts
    it from the current parameters.  Under data parallelism every rank steps the same reduced buckets, so every rank holds
    the same EMA without communication.

    param_groups=[{"params": [...], "lr": ..., "weight_decay": ...}, ...] (None by default: one group over reducer.params, and the
    launches above; a list of one group likewise): torch's groups, every parameter of reducer.params in exactly one of them, at
    most 64, missing keys taken from the constructor; betas and eps are common (ValueError otherwise, here and at step()).
    `self.param_groups` is the list torch's schedulers write (`LambdaLR(opt, [f0, f1])`), and step() reads every group's lr and
    weight_decay afresh.  A parameter of group g is stepped exactly -- bit for bit -- as the one-group optimizer with
    (lr_g, weight_decay_g) steps it; the clip norm stays one norm over everything (clip="group" below gives every group its own).
    add_param_group raises.  Checkpoints: master
    mode keeps torch.optim.AdamW's format with several groups (a parameter's index is its position in the concatenation of the
    groups' lists, torch's numbering); the bf16-only format gains "group_params" (reducer.params indices per group).

    stochastic_rounding=True (off by default; nothing above changes with it off), sr_seed=s, an integer in [0, 2^64): the three
    bf16 stores of a bf16 bucket's step -- parameter and both moments -- are rounded stochastically instead of to nearest: up in
    magnitude with a probability equal to the discarded fraction, so every stored value is its fp32 value in expectation.  With
    round-to-nearest a bf16 weight with |p| > 512 lr never moves and exp_avg_sq never decays at beta2 = 0.999; with
    this flag the pure-bf16 mode trains at the same 14 B per parameter.  The fp32 arithmetic is that of the step without the flag;
    the clipped gradient is still rounded to nearest; fp32 master buckets of a mixed reducer are stepped as without the flag (a
    reducer with no bf16 bucket raises ValueError); the EMA follows the parameter as stored.  Works with skip_nonfinite, ema_decay
    and param_groups in any combination, at the launch count of that combination.  The random bits are a pure function of
    (sr_seed, the count of applied steps, the bucket's index, the element's offset in the bucket) -- nothing depends on the rank,
    the grid or how a bucket is split into ranges -- so ranks that pass the same sr_seed (they must; the default does) hold the
    same weights with no communication, a skipped step draws nothing, and a run resumed from state_dict() continues bit for bit:
    the checkpoint carries the seed ("stochastic_rounding": {"seed": s}; in master-mode format inside param_groups[0]), and
    load_state_dict() takes it over (a checkpoint without it leaves the constructor's seed).

    clip="global" (the default) is everything above: one clip norm over all groups, and a "max_grad_norm" key inside a group dict
    is carried along (state_dict() included) and not used.  clip="group" (two or more param_groups; ValueError otherwise): group
    g's gradient is scaled by min(1, m_g / (sqrt(S_g) + 1e-6)), S_g the sum of squares over the gradients of group g's parameters
    alone as the buckets stand after reducer.finish() -- torch's clip_grad_norm_(g["params"], m_g) -- and m_g the group's
    "max_grad_norm": a positive float, None for a group that is not clipped, the constructor's max_grad_norm for a group without
    the key; read afresh at every step() as lr and weight_decay are (<= 0 or not finite: ValueError at step()).  A parameter of
    group g is stepped bit for bit as the one-group optimizer with (lr_g, weight_decay_g, m_g) steps it on a gradient whose sum
    of squares is S_g, and depends on no other group's gradient: unguarded, a NaN in one group's gradient stays in that group (its
    norm is NaN, its coefficient therefore 1 as in the one-group kernels, the elements it sits in become NaN) and leaves every
    other group's bits alone.  Works with skip_nonfinite, ema_decay and stochastic_rounding in any combination, at
    one step launch per bucket.  The guard still takes ONE verdict per step, on the sum of the groups' sums in group order: a
    non-finite group skips the step for every group; health() then reports "skipped_group_norms" and the first-skip warning names
    the group(s).  As with the global clip, a scheduler that rewrites lr or max_grad_norm on the host advances on skipped steps.
    grad_norm() stays the global norm; group_grad_norms() / group_grad_sumsq() give the groups' (device tensors, no
    synchronisation; RuntimeError under clip="global").  A group's norm is built from per-parameter sums and does not depend on
    bucket_bytes; its relative error is parameter_stats()' plus one fp32 rounding.  `clip` is a constructor property and is not
    stored; every group's "max_grad_norm" round-trips through state_dict() in both formats, and a checkpoint without the key
    leaves the groups as constructed."""

    WINDOW = 8     # guarded steps in flight before step() waits for the oldest readback

    def __init__(self, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, amsgrad=False,
                 maximize=False, skip_nonfinite=False, ema_decay=None, ema_warmup=False, param_groups=None, stochastic_rounding=False,
                 sr_seed=0, clip="global"):
        if amsgrad or maximize:
            raise ValueError("FlatAdamW: amsgrad and maximize are not supported")
        param_groups = None if param_groups is None else list(param_groups)
        self.clip = resolve_clip(clip, 1 if param_groups is None else len(param_groups))
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"FlatAdamW: ema_decay must lie strictly between 0 and 1 ({ema_decay!r} given)")
        self.stochastic_rounding = bool(stochastic_rounding)
        self.sr_seed = _sr_seed(sr_seed)
        if self.stochastic_rounding and not any(b["flat"].dtype == torch.bfloat16 for b in reducer.buckets):
            raise ValueError("FlatAdamW(stochastic_rounding=True): the reducer has no bf16 bucket, so there is nothing to round "
                             "(fp32 masters are stored exactly)")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema_active = False            # inside ema_weights()
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.skip_nonfinite and len(reducer.buckets) > _lib.STEP_MAX_BUCKETS:
            raise ValueError(f"FlatAdamW(skip_nonfinite=True): at most {_lib.STEP_MAX_BUCKETS} gradient buckets "
                             f"({len(reducer.buckets)} given)")
        self.reducer = reducer
        defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay))
        if param_groups is None:
            super().__init__(list(reducer.params), defaults)
        else:       # (copies: torch fills the defaults into the dicts it is given)
            super().__init__([dict(g) for g in resolve_param_groups(reducer.params, param_groups, defaults)], defaults)
        self._groups_fixed = True
        self._group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        self._group_maps = {}               # bucket -> (what _stepped(bucket) was, the device map built from it)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.step_count = 0
        self.flat = []
        lib = _lib.load()
        for b in reducer.buckets:
            g = b["flat"]
            if not g.is_cuda or g.dtype not in (torch.bfloat16, torch.float32):
                raise TypeError("FlatAdamW: bf16 or fp32 (master) CUDA gradient buckets only (no CPU fallback)")
            flat_p = torch.zeros_like(g)
            for p, off in zip(b["params"], b["offsets"]):       # same (256-B aligned) offsets as the gradient views
                n = p.numel()
                flat_p[off:off + n].copy_(p.data.reshape(-1))
                p.data = flat_p[off:off + n].view_as(p)        # the parameter now lives inside the flat buffer
            ent = {"p": flat_p, "g": g, "m": torch.zeros_like(g), "v": torch.zeros_like(g)}
            if g.dtype == torch.float32:                        # fp32 masters: + the flat bf16 shadow (same offsets)
                ent["sh"] = torch.zeros(g.numel(), dtype=torch.bfloat16, device=g.device)
                ops.register_flat_shadow(flat_p, ent["sh"])
            if self.ema_decay is not None:                      # always fp32, at the same offsets
                ent["ema"] = flat_p.to(torch.float32, copy=True)
            self.flat.append(ent)
        if self.ema_decay is not None:
            self._ema_w = (ctypes.c_float * _lib.STEP_MAX_CANDIDATES)()       # dvla_ema_weights writes it, the step reads it
        self.master_mode = any("sh" in s for s in self.flat)
        dev = reducer.buckets[0]["flat"].device
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._partial = torch.empty(int(lib.dvla_sumsq_partial_len()), dtype=torch.float32, device=dev)
        if self.clip == "group":            # per parameter and per group: the sums of squares of the last step's gradient
            self._param_sumsq = torch.zeros(len(reducer.params), dtype=torch.float32, device=dev)
            self._group_sumsq = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)
            self._group_ids = torch.tensor([self._group_of[id(p)] for p in reducer.params], dtype=torch.uint8).to(dev)
        if self.skip_nonfinite:
            self._slots = torch.zeros(len(self.flat), dtype=torch.float32, device=dev)         # one sum of squares per bucket
            self._state = torch.zeros(ctypes.sizeof(_lib.StepState), dtype=torch.uint8, device=dev)      # dvla_step_state
            self._cand = (_lib.StepScalars * _lib.STEP_MAX_CANDIDATES)()
            ring = torch.zeros(self.WINDOW, _lib.STEP_READBACK_BYTES, dtype=torch.uint8).pin_memory()
            self._ring = [_Readback(ring[i]) for i in range(self.WINDOW)]
            self._issued = 0
            self._skip_warned = False
            self._ledger = _StepLedger(window=self.WINDOW, on_skip=self._on_skip)

    def _ranges(self, bi):
        """element ranges of bucket bi that hold parameters which receive gradients (maximal runs; alignment gaps between two
        used neighbours are included -- they are zero in every buffer)"""
        b = self.reducer.buckets[bi]
        total = b["flat"].numel()
        used = self._stepped(bi)
        if not any(used):
            return []
        if all(used):
            return [(0, total)]
        runs, start = [], None
        bounds = list(b["offsets"]) + [total]
        for i, u in enumerate(used):
            if u and start is None:
                start = bounds[i]
            if not u and start is not None:
                runs.append((start, bounds[i]))
                start = None
        if start is not None:
            runs.append((start, total))
        return runs

    def _stepped(self, bi):
        """per parameter of bucket bi: does the step update it.  fp32 masters: a bucket no gradient has reached since the
        reducer's first finish() (it holds only unused parameters; the reducer does not learn from a bucket where nothing
        fired) is left alone, as torch leaves parameters without a gradient"""
        b = self.reducer.buckets[bi]
        if "sh" in self.flat[bi] and "ever_fired" in b and not b["ever_fired"]:
            return [False] * len(b["params"])
        return b["expected"]

    def _sr_launch(self, lib, bi, lo, hi, gmap, lrs, wds, b1, b2, eps, step, sumsq, max_norm, state, ema_w, n_cand, stream,
                   per_group=False):
        """elements lo .. hi of bf16 bucket bi through dvla_adamw_bf16_sr: the plain / guarded / EMA / grouped step of a bf16
        bucket (gmap None: one group) with stochastically rounded stores; the element index of the random bits starts at lo.
        per_group: through dvla_adamw_bf16_sr_clip, sumsq the groups' sums on the device and max_norm the host array"""
        s = self.flat[bi]
        o = 2 * lo
        fn = lib.dvla_adamw_bf16_sr_clip if per_group else lib.dvla_adamw_bf16_sr
        check(fn(s["p"].data_ptr() + o, s["g"].data_ptr() + o, s["m"].data_ptr() + o, s["v"].data_ptr() + o,
                 s["ema"].data_ptr() + 4 * lo if ema_w is not None else None, hi - lo, gmap, len(lrs), lrs, wds,
                 float(b1), float(b2), eps, step, sumsq, max_norm, state, ema_w, n_cand, self.sr_seed, bi, lo,
                 stream), "dvla_adamw_bf16_sr")

    def _issue_readback(self):
        """behind a guarded step's launches: the head of the device state into the next slot of the pinned ring, as a ledger ticket"""
        ticket = self._ring[self._issued % self.WINDOW]       # free: fewer than WINDOW steps are in flight after begin()
        self._issued += 1
        ticket.slot.copy_(self._state[:_lib.STEP_READBACK_BYTES], non_blocking=True)
        ticket.event.record(torch.cuda.current_stream())
        self._ledger.issued(ticket)

    def _on_skip(self, step):
        if self._skip_warned:
            return
        self._skip_warned = True
        # one synchronous read of the device's latch: the number of the LAST skipped step and its per-bucket sums, which belong
        # together (the step just confirmed may be an earlier one)
        tail = self._state.cpu()
        last = int(tail[_lib.StepState.latched_step.offset:][:8].view(torch.int64)[0])
        n_slots = len(self.param_groups) if self.clip == "group" else len(self.flat)      # what the verdict was fed
        sums = tail[_lib.StepState.skipped_bucket_sumsq.offset:][:4 * n_slots].view(torch.float32).tolist()
        bad = [i for i, x in enumerate(sums) if not math.isfinite(x)]
        first = "" if last == step else f" (the first confirmed skip was step {step})"
        if self.clip == "group":
            named = [f"{i} ({self.param_groups[i]['name']!r})" if "name" in self.param_groups[i] else str(i) for i in bad]
            where = f"non-finite gradient in parameter group(s) {', '.join(named)}" if bad else "the gradient norm overflows fp32"
            see = 'parameter_stats("grad")["grad_nonfinite"] names the parameter(s)'
        else:
            where = f"non-finite gradient in bucket(s) {bad}" if bad else "the gradient norm overflows fp32"
            see = "see bucket_parameters()"
        warnings.warn(f"FlatAdamW: step {last} was skipped: {where}{first}; {see}.  Further skips are counted "
                      f"in health() / skipped_steps without a warning.", RuntimeWarning, stacklevel=3)

    def _state_view(self, field, dtype):
        f = getattr(_lib.StepState, field)
        return self._state[f.offset:f.offset + f.size].view(dtype)

    def _require_guard(self, what):
        if not self.skip_nonfinite:
            raise RuntimeError(f"FlatAdamW.{what}: construct the optimizer with skip_nonfinite=True")

    def health(self):
        """the guard's account as device tensors (copies enqueued on the current stream, no synchronisation): steps applied and
        skipped, the last step's verdict (1 applied / 0 skipped) and gradient norm, and the 1-based number and per-bucket gradient
        norms of the last skipped step (bucket_parameters(i) says what lives in bucket i).  With clip="group" the verdict is taken
        over the groups' sums, and "skipped_group_norms" (one per parameter group) stands in place of "skipped_bucket_norms"."""
        self._require_guard("health()")
        out = {"applied": self._state_view("applied", torch.int64)[0].clone(),
               "skipped": self._state_view("skipped", torch.int64)[0].clone(),
               "last_ok": self._state_view("ok", torch.int32)[0].clone(),
               "last_grad_norm": self._state_view("sumsq", torch.float32)[0].sqrt(),
               "last_skipped_step": self._state_view("latched_step", torch.int64)[0].clone()}
        latched = self._state_view("skipped_bucket_sumsq", torch.float32)
        if self.clip == "group":
            out["skipped_group_norms"] = latched[:len(self.param_groups)].sqrt()
        else:
            out["skipped_bucket_norms"] = latched[:len(self.flat)].sqrt()
        return out

    def bucket_parameters(self, i):
        """indices into reducer.params of the parameters in gradient bucket i"""
        index = {id(p): k for k, p in enumerate(self.reducer.params)}
        return [index[id(p)] for p in self.reducer.buckets[i]["params"]]

    @property
    def applied_steps(self):
        """steps applied so far (host int).  Waits for every enqueued step: a synchronisation."""
        self._require_guard("applied_steps")
        self._ledger.drain()
        self.step_count = self._ledger.confirmed_applied
        return self._ledger.confirmed_applied

    @property
    def skipped_steps(self):
        """steps skipped so far (host int).  Waits for every enqueued step: a synchronisation."""
        self._require_guard("skipped_steps")
        self._ledger.drain()
        return self._ledger.confirmed_skipped

    def _reset_guard(self, applied, skipped):
        """device state and ledger to a resumed run's counts (ordered behind whatever is enqueued on the current stream)"""
        head = torch.zeros(self._state.numel(), dtype=torch.uint8)
        head[:16].view(torch.int64).copy_(torch.tensor([int(applied), int(skipped)], dtype=torch.int64))
        self._state.copy_(head)
        torch.cuda.current_stream().synchronize()          # the readbacks still in flight are forgotten with the ledger
        self._ledger.reset(applied, skipped)
        self.step_count = int(applied)

    def _norm_pass(self, lib, stream, guard, clip, per_group):
        """The gradient's sums of squares as this step needs them -> (slots, n_slots, sumsq): what a guarded step's verdict adds
        up (a device tensor and how many of its entries) and the address the unguarded step kernels read their clip from (None:
        no clip, or guarded -- those kernels read the verdict's total from the state).  Global clip: dvla_sumsq_* per bucket,
        accumulated into self._sumsq or, guarded, into one slot per bucket (without a clip as well: the verdict needs the norm).
        clip="group": _group_norms; the groups' sums are the verdict's slots and the `_clip` kernels' table, guarded or not."""
        if per_group:
            self._group_norms(lib, stream, None if guard else self._sumsq.data_ptr())
            return self._group_sumsq, len(self.param_groups), self._group_sumsq.data_ptr()
        if guard or clip:
            for i, s in enumerate(self.flat):
                fn = lib.dvla_sumsq_f32 if "sh" in s else lib.dvla_sumsq_bf16
                out, accumulate = (self._slots.data_ptr() + 4 * i, 0) if guard else (self._sumsq.data_ptr(), 1 if i > 0 else 0)
                check(fn(s["g"].data_ptr(), s["g"].numel(), self._partial.data_ptr(), out, accumulate, stream), "dvla_sumsq")
        if guard:
            return self._slots, len(self.flat), None
        return None, 0, (self._sumsq.data_ptr() if clip else None)

    def _launch_range(self, lib, bi, lo, hi, hp):
        """elements lo .. hi of bucket bi through the entry point of this step's combination (hp: what step() derived).  One
        group: dvla_adamw_{bf16,f32_master}[_ema][_guarded]; two or more (whole buckets, with the group map):
        dvla_adamw_{bf16,f32_master}_grouped, `_grouped_clip` with clip="group"; a bf16 bucket under stochastic rounding: _sr_launch"""
        s = self.flat[bi]
        master, grouped, guard, ema = "sh" in s, len(hp.lrs) > 1, hp.state is not None, hp.ema_w is not None
        gmap = self._group_map(bi).data_ptr() if grouped else None
        if self.stochastic_rounding and not master:
            return self._sr_launch(lib, bi, lo, hi, gmap, hp.lrs, hp.wds, hp.b1, hp.b2, hp.eps, hp.base, hp.sumsq, hp.max_norm,
                                   hp.state, hp.ema_w, hp.n_cand, hp.stream, per_group=hp.per_group)
        o = (4 if master else 2) * lo       # byte offset in the parameter's dtype
        bufs = [s[k].data_ptr() + o for k in ("p", "g", "m", "v")] + ([s["sh"].data_ptr() + 2 * lo] if master else [])
        e = s["ema"].data_ptr() + 4 * lo if ema else None
        name = "dvla_adamw_f32_master" if master else "dvla_adamw_bf16"
        if grouped:
            name += "_grouped_clip" if hp.per_group else "_grouped"
            args = bufs + [e, hi - lo, gmap, len(hp.lrs), hp.lrs, hp.wds, hp.b1, hp.b2, hp.eps, hp.base, hp.sumsq, hp.max_norm,
                           hp.state, hp.ema_w, hp.n_cand]
        else:
            name += ("_ema" if ema else "") + ("_guarded" if guard else "")
            args = bufs + ([e] if ema else []) + [hi - lo, hp.lrs[0], hp.b1, hp.b2, hp.eps, hp.wds[0]]
            args += [hp.max_norm, hp.state] if guard else [hp.base, hp.sumsq, hp.max_norm]
            if ema:
                args += [hp.ema_w, hp.n_cand] if guard else [hp.ema_w[0]]
        check(getattr(lib, name)(*args, hp.stream), name)

    @torch.no_grad()
    def step(self, closure=None):
        """One flow for every combination of guard, EMA, groups, stochastic rounding and clip: the norm pass, guarded the verdict
        on the device, the EMA weights of the step counts still possible, one step launch per range (one group) or per bucket
        (groups), guarded the readback ticket.  Every group's lr, weight_decay and max_grad_norm are read afresh."""
        if self._ema_active:
            raise RuntimeError("FlatAdamW.step() inside ema_weights(): the model holds the EMA weights, not the training weights")
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        groups = self.param_groups
        n_groups, per_group = len(groups), self.clip == "group"
        guard, ema, clip = self.skip_nonfinite, self.ema_decay is not None, self.max_grad_norm is not None
        b1, b2, eps = common_betas_eps(groups)
        hp = types.SimpleNamespace(
            lrs=(ctypes.c_double * n_groups)(*[float(g["lr"]) for g in groups]),
            wds=(ctypes.c_double * n_groups)(*[float(g["weight_decay"]) for g in groups]),
            b1=b1, b2=b2, eps=eps, per_group=per_group, stream=stream, ema_w=self._ema_w if ema else None,
            max_norm=self.max_grad_norm if clip else 0.0)       # guarded, <= 0: the norm only feeds the verdict
        if per_group:   # (0: the group is not clipped; its norm still feeds the verdict and group_grad_norms())
            hp.max_norm = (ctypes.c_float * n_groups)(*[0.0 if m is None else m for m in group_max_norms(groups, self.max_grad_norm)])
        if guard:       # the step count is the device's: the host knows the counts still possible
            confirmed, hp.n_cand = self._ledger.begin()
            self.step_count = confirmed
            hp.base, hp.state = confirmed + 1, self._state.data_ptr()
        else:
            self.step_count += 1
            hp.base, hp.n_cand, hp.state = self.step_count, 1, None
        slots, n_slots, hp.sumsq = self._norm_pass(lib, stream, guard, clip, per_group)
        if guard:       # of the candidates the grouped kernels use what no lr enters
            check(lib.dvla_step_candidates(hp.lrs[0], b1, b2, hp.base, hp.n_cand, self._cand), "dvla_step_candidates")
            check(lib.dvla_step_verdict(slots.data_ptr(), n_slots, self._sumsq.data_ptr(), hp.state, confirmed, hp.n_cand,
                                        self._cand, stream), "dvla_step_verdict")
        if ema:         # the weights of the same candidate counts base + j; the guarded kernels pick the verdict's row
            check(lib.dvla_ema_weights(self.ema_decay, int(self.ema_warmup), hp.base, hp.n_cand, self._ema_w), "dvla_ema_weights")
        for bi, s in enumerate(self.flat):
            whole = [(0, s["p"].numel())] if any(self._stepped(bi)) else []
            for lo, hi in (whole if n_groups > 1 else self._ranges(bi)):
                if hi > lo:
                    self._launch_range(lib, bi, lo, hi, hp)
        if guard:
            self._issue_readback()
        if self.master_mode:
            self._publish_shadows_guarded() if guard else self._publish_shadows()

    def add_param_group(self, param_group):
        if getattr(self, "_groups_fixed", False):
            raise RuntimeError("FlatAdamW.add_param_group: the groups are fixed at construction (pass param_groups=[...]); every "
                               "parameter of the reducer already lives in a flat buffer and belongs to one group")
        super().add_param_group(param_group)

    def _group_map(self, bi):
        """the device map of bucket bi (dvla.h: one byte per 8 elements), rebuilt when _stepped(bi) changes -- the reducer learns
        its unused parameters after the first finish()"""
        stepped = tuple(bool(u) for u in self._stepped(bi))
        hit = self._group_maps.get(bi)
        if hit is None or hit[0] != stepped:
            b = self.reducer.buckets[bi]
            cpu = build_group_map(b["offsets"], [p.numel() for p in b["params"]], b["flat"].numel(),
                                  [self._group_of[id(p)] for p in b["params"]], stepped, len(self.param_groups))
            hit = (stepped, cpu.to(b["flat"].device))
            self._group_maps[bi] = hit
        return hit[1]

    def _publish_shadows(self):
        """hand the freshly written bf16 copies to dreamvla_amd.ops as the shadows of the stepped masters (recorded at each
        master's current version and address; parameters the step skipped keep whatever entry they had)"""
        for bi, s in enumerate(self.flat):
            if "sh" not in s:
                continue
            b = self.reducer.buckets[bi]
            for p, off, used in zip(b["params"], b["offsets"], self._stepped(bi)):
                if used:
                    ops.adopt_shadow(p, s["sh"][off:off + p.numel()].view(p.shape))

    def _publish_shadows_guarded(self):
        """_publish_shadows after a guarded step, which may not have written the copies: a bucket in which some stepped master
        is not already served from this flat shadow at its current version -- the first step, or masters rewritten since (a
        checkpoint load) -- first gets its whole shadow cast anew from the masters, so the copies are current whether or not
        the step was applied.  In the steady state that is no launch."""
        for bi, s in enumerate(self.flat):
            if "sh" not in s:
                continue
            b = self.reducer.buckets[bi]
            views = [(p, s["sh"][off:off + p.numel()].view(p.shape))
                     for p, off, used in zip(b["params"], b["offsets"], self._stepped(bi)) if used]
            if not all(ops.shadow_is_current(p, sh) for p, sh in views):
                check(_lib.load().dvla_cast_f32_to_bf16(s["p"].data_ptr(), s["sh"].data_ptr(), s["p"].numel(),
                                                        torch.cuda.current_stream().cuda_stream), "dvla_cast_f32_to_bf16")
            for p, sh in views:
                ops.adopt_shadow(p, sh)

    def zero_grad(self, set_to_none=True):
        self.reducer.zero_grad()

    def grad_norm(self):
        """total gradient norm of the last step() with clipping (device scalar tensor); with clip="group" the root of the groups'
        sums of squares added in group order"""
        return self._sumsq.sqrt()

    def _group_norms(self, lib, stream, total):
        """clip="group": every group's sum of squares of the gradient buckets as they stand into self._group_sumsq -- stage 1 of
        the segmented reduction per bucket and its combine over parameter_stats()' tables (per parameter, so a group's sum does not
        depend on the bucket layout), then dvla_group_sumsq; `total` (a device address or None) receives their sum"""
        tabs, n_records, segs, scratch = self._stats_tables()
        n = len(self.reducer.params)
        for s, (chunks, n_chunks, first) in zip(self.flat, tabs):
            if n_chunks:
                fn = lib.dvla_segment_stats_f32 if s["g"].dtype == torch.float32 else lib.dvla_segment_stats_bf16
                check(fn(s["g"].data_ptr(), s["g"].numel(), chunks.data_ptr(), n_chunks,
                         scratch.data_ptr() + first * _lib.STATS_PARTIAL_BYTES, stream), "dvla_segment_stats")
        check(lib.dvla_segment_combine(scratch.data_ptr(), n_records, segs.data_ptr(), n, self._param_sumsq.data_ptr(), None, None, n,
                                       stream), "dvla_segment_combine")
        check(lib.dvla_group_sumsq(self._param_sumsq.data_ptr(), self._group_ids.data_ptr(), n, len(self.param_groups),
                                   self._group_sumsq.data_ptr(), total, stream), "dvla_group_sumsq")

    def _require_group_clip(self, what):
        if self.clip != "group":
            raise RuntimeError(f'FlatAdamW.{what}: construct the optimizer with clip="group" (with clip="global" there is one norm: '
                               f'grad_norm())')

    def group_grad_sumsq(self):
        """clip="group": the sum of squares of every parameter group's gradient at the last step(), before clipping, groups that
        are not clipped included -> (n_groups,) fp32 device tensor (a copy; no host synchronisation)"""
        self._require_group_clip("group_grad_sumsq()")
        return self._group_sumsq.clone()

    def group_grad_norms(self):
        """clip="group": the gradient norm of every parameter group at the last step(), before clipping -- what each group's
        max_grad_norm is held against -> (n_groups,) fp32 device tensor (no host synchronisation)"""
        self._require_group_clip("group_grad_norms()")
        return self._group_sumsq.sqrt()

    # ---- per-parameter statistics (parameter_stats) ----------------------------------------------------------------------------
    def _stats_tables(self):
        """the chunk table of every bucket (device tensor, number of chunks, index of its first record), the segment table of all
        buckets together and the scratch of one record per chunk: built and uploaded on first use"""
        if getattr(self, "_stats_cache", None) is None:
            index = {id(p): i for i, p in enumerate(self.reducer.params)}
            dev = self.reducer.buckets[0]["flat"].device
            tabs, all_segs, first = [], [], 0
            for b in self.reducer.buckets:
                chunks, segs = build_chunk_table(b["offsets"], [p.numel() for p in b["params"]], b["flat"].numel(),
                                                 [index[id(p)] for p in b["params"]], first_record=first)
                pad = torch.zeros(1, 2, dtype=torch.int64)          # (an empty table still has an address)
                tabs.append((torch.cat([chunks, pad]).to(dev), chunks.shape[0], first))
                all_segs.append(segs)
                first += chunks.shape[0]
            segs = torch.cat(all_segs + [torch.zeros(1, 3, dtype=torch.int64)]).to(dev)
            scratch = torch.empty(max(first, 1) * _lib.STATS_PARTIAL_BYTES, dtype=torch.uint8, device=dev)
            self._stats_cache = (tabs, first, segs, scratch)
        return self._stats_cache

    def _group_masks(self):
        """per parameter group: 1.0 at its parameters' positions in reducer.params (device fp32, built once: the groups are fixed)"""
        if getattr(self, "_stats_masks", None) is None:
            dev = self.reducer.buckets[0]["flat"].device
            which = torch.tensor([self._group_of[id(p)] for p in self.reducer.params], dtype=torch.int64)
            self._stats_masks = [(which == gi).to(torch.float32).to(dev) for gi in range(len(self.param_groups))]
        return self._stats_masks

    @torch.no_grad()
    def parameter_stats(self, what=("grad", "param", "update")):
        """Per-parameter reductions over the flat buffers -> dict of 1-D device tensors of length len(reducer.params), in
        reducer.params order, computed by segmented reductions on the current stream (one launch per bucket and buffer and one
        more per buffer, no atomics, no host synchronisation but the one named below); the step is not touched and a run that never calls this
        issues the launches it always did.  `what` selects:
          "grad"    grad_norm, grad_absmax (largest |g| over the elements that are not NaN; inf if there is an inf),
                    grad_nonfinite (int64: the number of NaN / inf elements) of the gradient buckets as they stand.  The step
                    kernels do not write the gradient, so after reducer.finish() -- before or after step() -- this is the
                    reduced, UNCLIPPED gradient; after a skipped step grad_nonfinite.nonzero() names the parameter(s) that
                    made it skip, until zero_grad().
          "param"   param_norm, param_absmax, param_nonfinite of the parameters (the fp32 masters in master mode)
          "update"  update_norm = lr_g |1 / (1 - beta1^t)| sqrt(sum r^2), r = exp_avg / denom(exp_avg_sq) with the step's own
                    denominator, t the current step count and lr_g the lr of the parameter's group read afresh from param_groups.
                    On fp32 masters this is the norm of the Adam term the LAST step added to the parameter, element for
                    element, before weight decay.  On bf16 buckets it is the same term recomputed from the moments AS STORED
                    (rounded to bf16, or stochastically rounded), not the fp32 values the step held in registers.  0 before the
                    first step and for parameters the step leaves alone (their moments stay zero).  With skip_nonfinite t is
                    `applied_steps`, so the call waits for every enqueued step exactly as that property does.
        A parameter's numbers depend on its own elements only -- not on the bucket it sits in or on bucket_bytes -- and two
        calls give the same bits; the relative error of a norm is below (STATS_CHUNK / 256 + 10) 2^-24.
        Alignment gaps are never read.  Raises RuntimeError inside ema_weights() (the buffers hold the EMA) and ValueError for an
        unknown entry of `what`.  Tables and scratch are allocated on first use.  stats_by_module() sums over modules."""
        what = (what,) if isinstance(what, str) else tuple(what)
        for w in what:
            if w not in STATS_KEYS:
                raise ValueError(f"FlatAdamW.parameter_stats: unknown entry {w!r} of `what` (known: {', '.join(STATS_KEYS)})")
        if self._ema_active:
            raise RuntimeError("FlatAdamW.parameter_stats() inside ema_weights(): the flat buffers hold the EMA weights")
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        tabs, n_records, segs, scratch = self._stats_tables()
        n = len(self.reducer.params)
        dev = scratch.device
        out = {}

        def stage1(fn, s, keys, chunks, n_chunks, first, *more):
            if n_chunks:        # (a bucket of empty parameters has no buffer to speak of)
                check(fn(*[s[k].data_ptr() for k in keys], s[keys[0]].numel(), chunks.data_ptr(), n_chunks,
                         scratch.data_ptr() + first * _lib.STATS_PARTIAL_BYTES, *more, stream), "dvla_segment_*")

        for w, key in (("grad", "g"), ("param", "p")):
            if w not in what:
                continue
            sumsq, absmax = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
            bad = torch.zeros(n, dtype=torch.int64, device=dev)
            for s, tab in zip(self.flat, tabs):
                stage1(lib.dvla_segment_stats_f32 if s[key].dtype == torch.float32 else lib.dvla_segment_stats_bf16, s, (key,), *tab)
            check(lib.dvla_segment_combine(scratch.data_ptr(), n_records, segs.data_ptr(), n, sumsq.data_ptr(), absmax.data_ptr(),
                                           bad.data_ptr(), n, stream), "dvla_segment_combine")
            out[w + "_norm"], out[w + "_absmax"], out[w + "_nonfinite"] = sumsq.sqrt_(), absmax, bad
        if "update" in what:
            t = self.applied_steps if self.skip_nonfinite else self.step_count
            sumsq = torch.zeros(n, dtype=torch.float32, device=dev)
            if t > 0:
                b1, b2, eps = common_betas_eps(self.param_groups)
                for s, tab in zip(self.flat, tabs):
                    stage1(lib.dvla_segment_adam_f32 if "sh" in s else lib.dvla_segment_adam_bf16, s, ("m", "v"), *tab, b2, eps, t)
                check(lib.dvla_segment_combine(scratch.data_ptr(), n_records, segs.data_ptr(), n, sumsq.data_ptr(), None, None, n,
                                               stream), "dvla_segment_combine")
                bc1 = abs(1.0 / (1.0 - b1 ** t))
                if len(self.param_groups) == 1:
                    scale = float(self.param_groups[0]["lr"]) * bc1
                else:       # Python scalars times cached device masks: no upload
                    scale = torch.zeros(n, dtype=torch.float32, device=dev)
                    for g, mask in zip(self.param_groups, self._group_masks()):
                        scale.add_(mask, alpha=float(g["lr"]) * bc1)
                sumsq = sumsq.sqrt_().mul_(scale)
            out["update_norm"] = sumsq
        return out

    def _layout(self):
        return flat_layout(self.reducer)

    # ---- EMA of the weights (ema_decay=...) ------------------------------------------------------------------------------------
    def _require_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError(f"FlatAdamW.{what}: construct the optimizer with ema_decay=...")
        if self._ema_active:
            raise RuntimeError(f"FlatAdamW.{what} inside ema_weights(): the EMA buffers are swapped with the training weights")

    def ema_reset(self):
        """the EMA restarts from the current parameters (after a checkpoint was loaded into the model, say)"""
        self._require_ema("ema_reset()")
        for s in self.flat:
            s["ema"].copy_(s["p"])

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the EMA values are the model's weights; on exit the training weights are back bit for bit, also
        when the body raises.  fp32 masters: one launch per bucket exchanges the master and the EMA buffer in place and writes
        the bf16 shadow of what the master buffer then holds, so no cast and no ops.invalidate_shadows() is needed; bf16 buckets
        are stashed (allocated on entry, freed on exit) and hold the EMA rounded to bf16.  Works before the first step and right
        after load_state_dict.  step(), nesting and the other ema_* methods raise RuntimeError inside.  A RolloutEngine built
        outside the context must be reset() or rebuilt inside it (and again after it): its captured graphs read the same
        addresses, but its per-instruction and per-frame caches were computed from the other weights."""
        self._require_ema("ema_weights()")
        lib = _lib.load()
        self._ema_active = True
        stashes = {}
        try:
            self._ema_swap(lib, stashes, restore=0)
            yield self
        finally:
            self._ema_swap(lib, stashes, restore=1)
            self._ema_active = False

    def _ema_swap(self, lib, stashes, restore):
        """whole buckets, on the current stream.  restore: undo exactly what the entry did (a bucket the entry did not reach --
        it raised -- is left alone)"""
        stream = torch.cuda.current_stream().cuda_stream
        for bi, s in enumerate(self.flat):
            n = s["p"].numel()
            if restore and bi not in stashes:
                continue
            if "sh" in s:
                check(lib.dvla_ema_swap_f32(s["p"].data_ptr(), s["ema"].data_ptr(), s["sh"].data_ptr(), n, stream),
                      "dvla_ema_swap_f32")
                b = self.reducer.buckets[bi]
                for p, off in zip(b["params"], b["offsets"]):      # the shadow was written in that launch
                    ops.adopt_shadow(p, s["sh"][off:off + p.numel()].view(p.shape))
                stashes[bi] = None
                continue
            stash = stashes[bi] if restore else torch.empty_like(s["p"])
            check(lib.dvla_ema_swap_bf16(s["p"].data_ptr(), s["ema"].data_ptr(), stash.data_ptr(), n, restore, stream),
                  "dvla_ema_swap_bf16")
            stashes[bi] = stash
        if restore:
            stashes.clear()

    def ema_state_dict(self):
        """{"decay", "warmup", "ema": {i: fp32 clone in the shape of reducer.params[i]}}"""
        self._require_ema("ema_state_dict()")
        out = {}
        for lay, s in zip(self._layout(), self.flat):
            for i, off, shape in lay:
                out[i] = s["ema"][off:off + math.prod(shape)].view(shape).clone()
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "ema": dict(sorted(out.items()))}

    def load_ema_state_dict(self, sd):
        """the inverse of ema_state_dict(); a tensor of another shape than its parameter raises ValueError"""
        self._require_ema("load_ema_state_dict()")
        ema = sd["ema"]
        layout = self._layout()
        for lay in layout:
            for i, off, shape in lay:
                if i not in ema or tuple(ema[i].shape) != tuple(shape):
                    got = tuple(ema[i].shape) if i in ema else None
                    raise ValueError(f"FlatAdamW.load_ema_state_dict: parameter {i} has shape {tuple(shape)}, the checkpoint's "
                                     f"EMA {got}")
        for lay, s in zip(layout, self.flat):
            for i, off, shape in lay:
                s["ema"][off:off + math.prod(shape)].copy_(ema[i].reshape(-1))
        self.ema_decay, self.ema_warmup = float(sd["decay"]), bool(sd["warmup"])

    def ema_model_state_dict(self, model):
        """model.state_dict() with every entry that belongs to a parameter of reducer.params (matched by identity through
        named_parameters) replaced by its EMA value in the entry's dtype: what an evaluation script loads"""
        self._require_ema("ema_model_state_dict()")
        where = {}
        for lay, s in zip(self._layout(), self.flat):
            for i, off, shape in lay:
                where[id(self.reducer.params[i])] = s["ema"][off:off + math.prod(shape)].view(shape)
        sd = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in where and name in sd:
                sd[name] = where[id(p)].to(sd[name].dtype, copy=True)
        return sd

    def state_dict(self):
        """master mode: torch.optim.AdamW's format (see torch_state_from_flat).  bf16 buckets only: step count, hyper-parameters
        and both moments (flat, per bucket) + the layout they belong to.  With skip_nonfinite the stored step is the number of
        APPLIED steps (this waits for every enqueued step) and param_groups[0]["skipped_steps"] is added.  With
        stochastic_rounding "stochastic_rounding": {"seed": sr_seed} is added (master mode: to param_groups[0])."""
        if self.skip_nonfinite:
            sd = self._state_dict(self.applied_steps)
            sd["param_groups"][0]["skipped_steps"] = self._ledger.confirmed_skipped
        else:
            sd = self._state_dict(self.step_count)
        if self.stochastic_rounding:
            (sd["param_groups"][0] if self.master_mode else sd)["stochastic_rounding"] = {"seed": self.sr_seed}
        return sd

    def _state_dict(self, step):
        if self.master_mode:
            with_state = [[bool(u) and step > 0 for u in self._stepped(bi)] for bi in range(len(self.flat))]
            starts = [sum(len(g["params"]) for g in self.param_groups[:k]) for k in range(len(self.param_groups))]
            return {"state": torch_state_from_flat(self._torch_layout(), [s["m"] for s in self.flat], [s["v"] for s in self.flat],
                                                   step, with_state),
                    "param_groups": [_torch_group(g, len(g["params"]), k) for g, k in zip(self.param_groups, starts)]}
        sd = {"step": step,
              "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
              "layout": [[int(p.numel()) for p in b["params"]] for b in self.reducer.buckets],
              "exp_avg": [s["m"].clone() for s in self.flat], "exp_avg_sq": [s["v"].clone() for s in self.flat]}
        if len(self.param_groups) > 1:
            sd["group_params"] = self._group_params()
        return sd

    def _group_params(self):
        """per group: the indices into reducer.params of its parameters"""
        index = {id(p): i for i, p in enumerate(self.reducer.params)}
        return [[index[id(p)] for p in g["params"]] for g in self.param_groups]

    def _torch_layout(self):
        """_layout() with every parameter numbered as torch.optim.Optimizer.state_dict() numbers it: by its position in the
        concatenation of the groups' `params` lists (with one group over reducer.params that is _layout())"""
        order = {id(p): i for i, p in enumerate(p for g in self.param_groups for p in g["params"])}
        return [[(order[id(self.reducer.params[i])], off, shape) for i, off, shape in lay] for lay in self._layout()]

    def load_state_dict(self, sd):
        """the inverse of state_dict().  With skip_nonfinite the device's counters and the ledger restart from the loaded step
        (as the applied count) and the dict's "skipped_steps" (0 if it has none); without it that key is ignored.  With
        stochastic_rounding the dict's seed replaces the constructor's (a dict without one leaves it); without it that key is
        ignored."""
        self._load_state_dict(sd)
        saved = (sd["param_groups"][0] if self.master_mode else sd).get("stochastic_rounding")
        if self.stochastic_rounding and saved is not None:
            self.sr_seed = _sr_seed(saved["seed"])
        skipped = int(self.param_groups[0].pop("skipped_steps", 0) if not self.master_mode
                      else sd["param_groups"][0].get("skipped_steps", 0))
        if self.skip_nonfinite:
            self._reset_guard(self.step_count, skipped)

    def _load_state_dict(self, sd):
        if self.master_mode:
            groups = sd.get("param_groups") if isinstance(sd, dict) else None
            n = len(self.reducer.params)
            sizes = [len(g["params"]) for g in self.param_groups]
            want = [list(range(sum(sizes[:k]), sum(sizes[:k + 1]))) for k in range(len(sizes))]
            if "state" not in sd or not groups or [list(g.get("params", ())) for g in groups] != want:
                if len(want) > 1:
                    raise ValueError(f"FlatAdamW.load_state_dict: expected torch.optim.AdamW's format with {len(want)} parameter "
                                     f"groups of {sizes} parameters (indices 0..{n - 1} in the order of the groups' lists)")
                raise ValueError(f"FlatAdamW.load_state_dict: expected torch.optim.AdamW's format with ONE parameter group over "
                                 f"the {n} trainable parameters (indices 0..{n - 1}, reducer.params order)")
            if any(g.get("amsgrad") or g.get("maximize") for g in groups):
                raise ValueError("FlatAdamW.load_state_dict: amsgrad / maximize checkpoints are not supported")
            common_betas_eps(groups)
            self.step_count = flat_from_torch_state(self._torch_layout(), sd["state"], [s["m"] for s in self.flat],
                                                    [s["v"] for s in self.flat])
            for mine, saved in zip(self.param_groups, groups):
                for k in ("lr", "betas", "eps", "weight_decay"):
                    mine[k] = saved[k]
                if "max_grad_norm" in saved:        # (a checkpoint without it keeps what the group has)
                    mine["max_grad_norm"] = saved["max_grad_norm"]
            return
        layout = [[int(p.numel()) for p in b["params"]] for b in self.reducer.buckets]
        if sd["layout"] != layout:
            raise ValueError("FlatAdamW.load_state_dict: the checkpoint's bucket layout does not match this model / reducer")
        mine = self._group_params() if len(self.param_groups) > 1 else None
        if sd.get("group_params") != mine:
            raise ValueError(f"FlatAdamW.load_state_dict: the checkpoint's parameter groups (reducer.params indices per group: "
                             f"{sd.get('group_params')}) are not this optimizer's ({mine})")
        self.step_count = int(sd["step"])
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update(saved)
        for s, m, v in zip(self.flat, sd["exp_avg"], sd["exp_avg_sq"]):
            s["m"].copy_(m)
            s["v"].copy_(v)


def _sr_seed(seed):
    """sr_seed as an int in [0, 2^64) (ValueError otherwise; bools and floats are not seeds)"""
    try:
        value = None if isinstance(seed, bool) else operator.index(seed)
    except TypeError:
        value = None
    if value is None or not 0 <= value < 2 ** 64:
        raise ValueError(f"FlatAdamW: sr_seed must be an integer in [0, 2^64) ({seed!r} given)")
    return value


def flat_layout(reducer):
    """per bucket: [(index in reducer.params, element offset, shape) ...] -- where each parameter's moments sit in the flat
    buffers; reducer.params is the order of `[p for p in model.parameters() if p.requires_grad]`, torch.optim.AdamW's indices"""
    index = {id(p): i for i, p in enumerate(reducer.params)}
    return [[(index[id(p)], off, tuple(p.shape)) for p, off in zip(b["params"], b["offsets"])] for b in reducer.buckets]


def resolve_param_groups(params, param_groups, defaults):
    """torch-style groups ({"params": [...], "lr": ..., "weight_decay": ...}; missing keys take `defaults`) checked against the
    reducer's parameter list (pure; works on CPU tensors): every parameter of `params` in exactly one group, nothing else in any,
    at most DVLA_STEP_MAX_GROUPS groups, betas / eps those of `defaults`.  ValueError names the offender by its position."""
    groups = [dict(g) for g in param_groups]
    if not groups or not all("params" in g for g in groups):
        raise ValueError("FlatAdamW: param_groups must be a non-empty list of dicts with a 'params' list")
    if len(groups) > _lib.STEP_MAX_GROUPS:
        raise ValueError(f"FlatAdamW: at most {_lib.STEP_MAX_GROUPS} parameter groups ({len(groups)} given)")
    index = {id(p): i for i, p in enumerate(params)}
    owner = {}
    for gi, g in enumerate(groups):
        g["params"] = [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])
        for k, p in enumerate(g["params"]):
            if id(p) not in index:
                raise ValueError(f"FlatAdamW: parameter {k} of group {gi} (shape {tuple(p.shape)}) is not a parameter of the reducer")
            if id(p) in owner:
                raise ValueError(f"FlatAdamW: parameter {index[id(p)]} of reducer.params (shape {tuple(p.shape)}) is in two groups "
                                 f"({owner[id(p)]} and {gi})")
            owner[id(p)] = gi
        for key in ("betas", "eps"):
            if key in g and _hyper(g[key]) != _hyper(defaults[key]):
                raise ValueError(f"FlatAdamW: group {gi} has {key} = {g[key]!r}, the optimizer {defaults[key]!r}: betas and eps "
                                 f"are common to all groups (the bias corrections depend on them)")
    for i, p in enumerate(params):
        if id(p) not in owner:
            raise ValueError(f"FlatAdamW: parameter {i} of reducer.params (shape {tuple(p.shape)}) is in no group")
    return groups


def _hyper(x):
    return tuple(float(v) for v in x) if isinstance(x, (tuple, list)) else float(x)


def common_betas_eps(groups):
    """(beta1, beta2, eps) of group 0, which every group must share (ValueError: someone edited one group's)"""
    betas, eps = _hyper(groups[0]["betas"]), _hyper(groups[0]["eps"])
    for gi, g in enumerate(groups):
        if _hyper(g["betas"]) != betas or _hyper(g["eps"]) != eps:
            raise ValueError(f"FlatAdamW: group {gi} has betas = {g['betas']!r}, eps = {g['eps']!r}, group 0 {groups[0]['betas']!r}, "
                             f"{groups[0]['eps']!r}: betas and eps are common to all groups")
    return betas[0], betas[1], eps


def resolve_clip(clip, n_groups):
    """FlatAdamW's `clip` checked against the number of parameter groups (pure): "global" or "group"; "group" needs two groups"""
    if clip not in ("global", "group"):
        raise ValueError(f'FlatAdamW: clip must be "global" or "group" ({clip!r} given)')
    if clip == "group" and n_groups < 2:
        raise ValueError(f'FlatAdamW(clip="group"): {n_groups} parameter group given; with fewer than two groups this would be the '
                         f'global clip -- pass param_groups=[...] with two or more groups, or clip="global"')
    return clip


def group_max_norms(groups, default):
    """every group's clip value for FlatAdamW(clip="group") (pure): the group's "max_grad_norm" -- a positive finite float, or
    None: the group is not clipped --, `default` (the constructor's max_grad_norm) for a group without the key.  ValueError names
    the group of a value that is <= 0, not finite or not a number."""
    out = []
    for gi, g in enumerate(groups):
        m = g.get("max_grad_norm", default)
        if m is not None:
            try:
                m = None if isinstance(m, bool) else float(m)
            except (TypeError, ValueError):
                m = None
            if m is None or not (m > 0.0 and math.isfinite(m)):
                raise ValueError(f"FlatAdamW: group {gi} has max_grad_norm = {g.get('max_grad_norm', default)!r}: a positive finite "
                                 f"number, or None for a group that is not clipped")
        out.append(m)
    return out


def prefix_groups(model_or_named_parameters, prefixes, rest="rest", **per_group):
    """Parameter groups cut by parameter name (pure), as plain torch groups that also carry "name":
    prefixes = {"heads": ("image_decoder", "action_head."), "trunk": ("transformer.",)} puts a trainable parameter into the group
    one of whose prefixes its name starts with (str.startswith; the longest matching prefix decides between groups), everything
    else into the group named `rest` (rest=None: an unmatched parameter is a ValueError).  Frozen parameters are left out and a
    parameter shared under two names counts once, under its first.  Every keyword is a group key given per group name,
    max_grad_norm={"heads": 0.05, "trunk": None}, lr={"trunk": 1e-4}: a group that is not named does not get the key (FlatAdamW
    fills in its constructor's value).  Groups come in the order of `prefixes`, `rest` last (omitted if empty), parameters in
    the order of named_parameters().  ValueError names a prefix that matches nothing, a prefix given to two groups and a group name
    no group has."""
    named = model_or_named_parameters
    named = named.named_parameters() if hasattr(named, "named_parameters") else named
    owner = {}
    for name, pres in prefixes.items():
        for pre in ((pres,) if isinstance(pres, str) else tuple(pres)):
            if pre in owner:
                raise ValueError(f"prefix_groups: the prefix {pre!r} is given to two groups ({owner[pre]!r} and {name!r})")
            owner[pre] = name
    if rest is not None and rest in prefixes:
        raise ValueError(f"prefix_groups: {rest!r} is the name of the group of everything else and of a group of `prefixes`")
    params = {name: [] for name in prefixes}
    if rest is not None:
        params[rest] = []
    hit, seen = set(), set()
    for pname, p in named:
        if not p.requires_grad or id(p) in seen:
            continue
        seen.add(id(p))
        match = max((pre for pre in owner if pname.startswith(pre)), key=len, default=None)
        if match is None and rest is None:
            raise ValueError(f"prefix_groups: the parameter {pname!r} matches no prefix and there is no `rest` group")
        hit.add(match)
        params[rest if match is None else owner[match]].append(p)
    for pre in owner:
        if pre not in hit:
            raise ValueError(f"prefix_groups: the prefix {pre!r} (group {owner[pre]!r}) matches no trainable parameter")
    for key, values in per_group.items():
        for name in values:
            if name not in params:
                raise ValueError(f"prefix_groups: {key} names the group {name!r}; the groups are {', '.join(map(repr, params))}")
    groups = []
    for name, ps in params.items():
        if name == rest and not ps:
            continue
        g = {"name": name, "params": ps}
        g.update({key: values[name] for key, values in per_group.items() if name in values})
        groups.append(g)
    return groups


def build_group_map(offsets, sizes, total, group_ids, stepped, n_groups):
    """the group map of one bucket (include/dvla.h; pure): a CPU uint8 tensor of ceil(total / 8) bytes, one per vector of 8
    elements.  Parameter j occupies elements offsets[j] .. offsets[j] + sizes[j]; its vectors (the last one may be partial, and
    may be the bucket's ragged tail) get group_ids[j] if stepped[j], everything else -- parameters the step leaves alone,
    alignment gaps -- 255.  Parameters start on multiples of 8 elements, so no vector belongs to two of them."""
    out = torch.full(((int(total) + 7) // 8,), 255, dtype=torch.uint8)
    for off, n, gid, used in zip(offsets, sizes, group_ids, stepped):
        if off % 8:
            raise ValueError(f"FlatAdamW: a parameter starts at element {off} of its bucket, not on a multiple of 8")
        if not 0 <= gid < n_groups or gid >= 255:
            raise ValueError(f"FlatAdamW: group id {gid} outside 0 .. {n_groups - 1}")
        if off + n > total:
            raise ValueError(f"FlatAdamW: a parameter ends at element {off + n} of a bucket of {total}")
        if used and n > 0:
            out[off // 8:(off + n + 7) // 8] = gid
    return out


def build_chunk_table(offsets, sizes, total, out_index=None, chunk=_lib.STATS_CHUNK, first_record=0):
    """the chunk table of one bucket for the segmented reductions (include/dvla.h; pure) -> (chunks, segs), CPU int64 tensors.
    Parameter j occupies elements offsets[j] .. offsets[j] + sizes[j] of its bucket and is cut into chunks of `chunk` elements
    counted from ITS OWN first element (the last one shorter), so the cuts -- and with them the order in which a parameter's
    elements are added -- do not depend on where the parameter sits or on what else the bucket holds.  chunks[c] = (element
    offset in the bucket, length), a parameter's chunks in consecutive rows; segs[j] = (first_record + its first chunk, number of
    chunks -- 0 for an empty parameter --, out_index[j], by default j): the buckets of an optimizer share one scratch of records.  Every parameter is in the table, stepped or not; alignment gaps are in no
    chunk.  Parameters start on multiples of 8 elements and `chunk` is a multiple of 8, so every chunk does."""
    if chunk <= 0 or chunk % 8:
        raise ValueError(f"FlatAdamW: the chunk length {chunk} is not a positive multiple of 8")
    out_index = list(range(len(sizes))) if out_index is None else list(out_index)
    chunks, segs = [], []
    for off, n, o in zip(offsets, sizes, out_index):
        off, n = int(off), int(n)
        if off % 8:
            raise ValueError(f"FlatAdamW: a parameter starts at element {off} of its bucket, not on a multiple of 8")
        if off < 0 or n < 0 or off + n > total:
            raise ValueError(f"FlatAdamW: a parameter ends at element {off + n} of a bucket of {total}")
        segs.append((int(first_record) + len(chunks), -(-n // chunk), int(o)))
        chunks.extend((off + lo, min(chunk, n - lo)) for lo in range(0, n, chunk))
    return (torch.tensor(chunks, dtype=torch.int64).reshape(-1, 2), torch.tensor(segs, dtype=torch.int64).reshape(-1, 3))


STATS_KEYS = {"grad": ("grad_norm", "grad_absmax", "grad_nonfinite"), "param": ("param_norm", "param_absmax", "param_nonfinite"),
              "update": ("update_norm",)}


def stats_by_module(stats, model_or_named_parameters, reducer, depth=2):
    """FlatAdamW.parameter_stats() per module -> (names, dict of tensors of length len(names)).  The parameters of `reducer.params`
    are matched by identity with the model's named parameters (as ema_model_state_dict does; a shared parameter counts once, under
    its first name) and a name is cut to its first `depth` dotted components: "trunk.h.3.attn.c_attn.weight" is "trunk.h" at
    depth 2.  Parameters of the reducer the model does not name go under "<unnamed>".  `*_norm` entries combine as the root of
    the sum of squares, `*_absmax` as the maximum, `*_nonfinite` as the sum.  names are in order of first appearance in
    reducer.params.  Pure torch on tiny tensors (a few launches on the tensors' device; CPU tensors work)."""
    named = model_or_named_parameters
    named = named.named_parameters(remove_duplicate=False) if hasattr(named, "named_parameters") else named
    name_of = {}
    for name, p in named:
        name_of.setdefault(id(p), name)
    names, owner = [], []
    for p in reducer.params:
        full = name_of.get(id(p))
        key = "<unnamed>" if full is None else ".".join(full.split(".")[:max(1, int(depth))])
        if key not in names:
            names.append(key)
        owner.append(names.index(key))
    out = {}
    for key, t in stats.items():
        if t.shape != (len(owner),):
            raise ValueError(f"stats_by_module: {key!r} has shape {tuple(t.shape)}, the reducer {len(owner)} parameters")
        idx = torch.tensor(owner, dtype=torch.int64).to(t.device)
        if key.endswith("_norm"):
            acc = torch.zeros(len(names), dtype=torch.float64, device=t.device)
            out[key] = acc.index_add_(0, idx, t.double() ** 2).sqrt().to(t.dtype)
        elif key.endswith("_absmax"):
            out[key] = torch.zeros(len(names), dtype=t.dtype, device=t.device).scatter_reduce_(0, idx, t, "amax", include_self=True)
        elif key.endswith("_nonfinite"):
            out[key] = torch.zeros(len(names), dtype=t.dtype, device=t.device).index_add_(0, idx, t)
        else:
            raise ValueError(f"stats_by_module: do not know how to combine {key!r} (expected *_norm, *_absmax or *_nonfinite)")
    return names, out


def weight_decay_groups(module_or_named_parameters, weight_decay, skip=()):
    """The two parameter groups of the usual rule, as plain torch groups (for FlatAdamW(param_groups=...) and torch.optim.AdamW
    alike): weight_decay = 0.0 for trainable parameters with ndim <= 1 (biases, LayerNorm weights), a name ending in ".bias" or
    a name in `skip` (cls_token, pos_embed, ... of a ViT); `weight_decay` for every other trainable parameter.  Frozen parameters
    are left out; a group that would be empty is omitted.  -> [no-decay group, decay group]"""
    named = module_or_named_parameters
    named = named.named_parameters() if hasattr(named, "named_parameters") else named
    skip = set(skip)
    plain, decayed = [], []
    for name, p in named:
        if not p.requires_grad:
            continue
        (plain if p.ndim <= 1 or name.endswith(".bias") or name in skip else decayed).append(p)
    groups = [{"params": plain, "weight_decay": 0.0}, {"params": decayed, "weight_decay": float(weight_decay)}]
    return [g for g in groups if g["params"]]


def _torch_group(g, n, start=0):
    """a parameter group as torch.optim.AdamW.state_dict() writes it (every key its load_state_dict expects)"""
    out = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"], "amsgrad": False,
           "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
           "decoupled_weight_decay": True}
    if "max_grad_norm" in g:        # a group's own clip value (FlatAdamW(clip="group")); torch carries extra keys along
        out["max_grad_norm"] = g["max_grad_norm"]
    out["params"] = list(range(start, start + n))
    return out


def torch_state_from_flat(layout, exp_avg, exp_avg_sq, step, with_state):
    """torch.optim.AdamW "state" from flat moments.  layout[b] = [(parameter index, offset, shape) ...] of bucket b;
    exp_avg / exp_avg_sq[b] the flat moment buffers; with_state[b][j]: parameter j of bucket b has state (torch keeps none
    for a parameter that never received a gradient).  The moments are copied in their storage dtype."""
    state = {}
    for lay, m, v, has in zip(layout, exp_avg, exp_avg_sq, with_state):
        for (i, off, shape), h in zip(lay, has):
            if not h:
                continue
            n = 1
            for d in shape:
                n *= d
            state[i] = {"step": torch.tensor(float(step), dtype=torch.float32),
                        "exp_avg": m[off:off + n].view(shape).clone(), "exp_avg_sq": v[off:off + n].view(shape).clone()}
    return dict(sorted(state.items()))


def flat_from_torch_state(layout, state, exp_avg, exp_avg_sq):
    """the inverse of torch_state_from_flat: fills the flat moments (zero for parameters without state) and returns the step
    count, which must be the same for every parameter that has state (ValueError otherwise)"""
    steps = set()
    for lay, m, v in zip(layout, exp_avg, exp_avg_sq):
        m.zero_()
        v.zero_()
        for i, off, shape in lay:
            st = state.get(i)
            if st is None:
                continue
            n = 1
            for d in shape:
                n *= d
            if tuple(st["exp_avg"].shape) != tuple(shape) or tuple(st["exp_avg_sq"].shape) != tuple(shape):
                raise ValueError(f"FlatAdamW.load_state_dict: parameter {i} has shape {tuple(shape)}, the checkpoint's moments "
                                 f"{tuple(st['exp_avg'].shape)}")
            m[off:off + n].copy_(st["exp_avg"].reshape(-1))
            v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(float(st["step"]))
    if len(steps) > 1:
        raise ValueError(f"FlatAdamW.load_state_dict: the parameters' step counts disagree ({sorted(steps)}); the flat "
                         f"optimizer keeps one step count")
    step = steps.pop() if steps else 0.0
    if step != int(step):
        raise ValueError(f"FlatAdamW.load_state_dict: non-integer step count {step}")
    return int(step)
