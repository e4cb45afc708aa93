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
"""
import torch

from . import _lib, ops
from ._lib import check


class FlatAdamW(torch.optim.Optimizer):
    """torch.optim.Optimizer surface (param_groups with `lr` -- so torch's LR schedulers, which the reference attaches to its
    AdamW (train.py:176-200), drive it unchanged --, state_dict / load_state_dict for checkpoint / resume) over flat buffers.
    Parameters the reducer has learned never to receive a gradient (the reference's constructed-but-unused modules) are left
    alone -- no weight decay, no moment update -- exactly as torch's AdamW skips `p.grad is None` parameters."""

    def __init__(self, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, amsgrad=False,
                 maximize=False):
        if amsgrad or maximize:
            raise ValueError("FlatAdamW: amsgrad and maximize are not supported")
        self.reducer = reducer
        super().__init__(list(reducer.params), dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                                    weight_decay=float(weight_decay)))
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
            self.flat.append(ent)
        self.master_mode = any("sh" in s for s in self.flat)
        dev = reducer.buckets[0]["flat"].device
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._partial = torch.empty(int(lib.dvla_sumsq_partial_len()), dtype=torch.float32, device=dev)

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

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        self.step_count += 1
        grp = self.param_groups[0]
        lr, (b1, b2), eps, wd = float(grp["lr"]), grp["betas"], float(grp["eps"]), float(grp["weight_decay"])
        clip = self.max_grad_norm is not None
        if clip:
            for i, s in enumerate(self.flat):
                fn = lib.dvla_sumsq_f32 if "sh" in s else lib.dvla_sumsq_bf16
                check(fn(s["g"].data_ptr(), s["g"].numel(), self._partial.data_ptr(), self._sumsq.data_ptr(), 1 if i > 0 else 0,
                         stream), "dvla_sumsq")
        for bi, s in enumerate(self.flat):
            for (lo, hi) in self._ranges(bi):
                if hi <= lo:
                    continue
                if "sh" in s:
                    o = 4 * lo      # fp32 byte offset
                    check(lib.dvla_adamw_f32_master(s["p"].data_ptr() + o, s["g"].data_ptr() + o, s["m"].data_ptr() + o,
                                                    s["v"].data_ptr() + o, s["sh"].data_ptr() + 2 * lo, hi - lo, lr, float(b1),
                                                    float(b2), eps, wd, self.step_count,
                                                    self._sumsq.data_ptr() if clip else None,
                                                    self.max_grad_norm if clip else 0.0, stream), "dvla_adamw_f32_master")
                    continue
                o = 2 * lo      # bf16 byte offset
                check(lib.dvla_adamw_bf16(s["p"].data_ptr() + o, s["g"].data_ptr() + o, s["m"].data_ptr() + o, s["v"].data_ptr() + o,
                                          hi - lo, lr, float(b1), float(b2), eps, wd, self.step_count,
                                          self._sumsq.data_ptr() if clip else None, self.max_grad_norm if clip else 0.0, stream),
                      "dvla_adamw_bf16")
        if self.master_mode:
            self._publish_shadows()

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

    def zero_grad(self, set_to_none=True):
        self.reducer.zero_grad()

    def grad_norm(self):
        """total gradient norm of the last step() with clipping (device scalar tensor)"""
        return self._sumsq.sqrt()

    def _layout(self):
        return flat_layout(self.reducer)

    def state_dict(self):
        """master mode: torch.optim.AdamW's format (see torch_state_from_flat).  bf16 buckets only: step count, hyper-parameters
        and both moments (flat, per bucket) + the layout they belong to"""
        if self.master_mode:
            with_state = [[bool(u) and self.step_count > 0 for u in self._stepped(bi)] for bi in range(len(self.flat))]
            return {"state": torch_state_from_flat(self._layout(), [s["m"] for s in self.flat], [s["v"] for s in self.flat],
                                                   self.step_count, with_state),
                    "param_groups": [_torch_group(g, len(self.reducer.params)) for g in self.param_groups]}
        return {"step": self.step_count,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                "layout": [[int(p.numel()) for p in b["params"]] for b in self.reducer.buckets],
                "exp_avg": [s["m"].clone() for s in self.flat], "exp_avg_sq": [s["v"].clone() for s in self.flat]}

    def load_state_dict(self, sd):
        if self.master_mode:
            groups = sd.get("param_groups") if isinstance(sd, dict) else None
            n = len(self.reducer.params)
            if "state" not in sd or not groups or len(groups) != 1 or list(groups[0].get("params", ())) != list(range(n)):
                raise ValueError(f"FlatAdamW.load_state_dict: expected torch.optim.AdamW's format with ONE parameter group over "
                                 f"the {n} trainable parameters (indices 0..{n - 1}, reducer.params order)")
            if groups[0].get("amsgrad") or groups[0].get("maximize"):
                raise ValueError("FlatAdamW.load_state_dict: amsgrad / maximize checkpoints are not supported")
            self.step_count = flat_from_torch_state(self._layout(), sd["state"], [s["m"] for s in self.flat],
                                                    [s["v"] for s in self.flat])
            for k in ("lr", "betas", "eps", "weight_decay"):
                self.param_groups[0][k] = groups[0][k]
            return
        layout = [[int(p.numel()) for p in b["params"]] for b in self.reducer.buckets]
        if sd["layout"] != layout:
            raise ValueError("FlatAdamW.load_state_dict: the checkpoint's bucket layout does not match this model / reducer")
        self.step_count = int(sd["step"])
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update(saved)
        for s, m, v in zip(self.flat, sd["exp_avg"], sd["exp_avg_sq"]):
            s["m"].copy_(m)
            s["v"].copy_(v)


def flat_layout(reducer):
    """per bucket: [(index in reducer.params, element offset, shape) ...] -- where each parameter's moments sit in the flat
    buffers; reducer.params is the order of `[p for p in model.parameters() if p.requires_grad]`, torch.optim.AdamW's indices"""
    index = {id(p): i for i, p in enumerate(reducer.params)}
    return [[(index[id(p)], off, tuple(p.shape)) for p, off in zip(b["params"], b["offsets"])] for b in reducer.buckets]


def _torch_group(g, n):
    """a parameter group as torch.optim.AdamW.state_dict() writes it (every key its load_state_dict expects)"""
    out = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"], "amsgrad": False,
           "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
           "decoupled_weight_decay": True}
    out["params"] = list(range(n))
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
