"""What per-group clipping costs in the optimizer step (a measurement script, not a test): FlatAdamW.step() alone on the parameter
layout of tests/gpu_param_groups_perf.py (head set C, 24 layers: the trainable parameters in GradBucketReducer's default
buckets), once as fp32 masters -- the shipped precision -- and once as bf16 buckets.  One JSON line per arm and one summary line per
layout on stdout and, appended, in the file named by --out=PATH (the recorded run is kept as profiles/r23_group_clip_perf.jsonl).

    python tests/gpu_group_clip_perf.py [--out=PATH] [--synthetic] [--arms=a,b,...] [--dtypes=f32,bf16] [--rounds=N] [--tree=NAME]

Arms (the two groups of weight_decay_groups, max_grad_norm = 0.1), each with an optimizer, parameters, moments and gradients of
its own, built afresh for every timed block and dropped after it:
  global        clip="global": dvla_sumsq_* per bucket, then one grouped launch per bucket
  global_again  the same arm once more: what two runs of the same code differ by
  group         clip="group": dvla_segment_stats_* per bucket + dvla_segment_combine + dvla_group_sumsq instead of the dvla_sumsq_*
                pass, then one `_clip` launch per bucket
  torch_clip    what a user could do without it: torch.nn.utils.clip_grad_norm_(group's parameters, 0.1) per group on the gradient
                views, then step() with max_grad_norm=None
Timing as in tests/gpu_guarded_step_perf.py: device events around a block of back-to-back steps sized to at least a second, ROUNDS
rounds with the arms interleaved, medians."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARGS = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
OUT = ARGS.get("out")
TREE = ARGS.get("tree", "this")
ROUNDS = int(ARGS.get("rounds", 5))
LR, WD, BETAS, EPS, MAX_NORM = 1e-3, 1e-4, (0.9, 0.999), 1e-8, 0.1
ARMS = {"global": "global", "global_again": "global", "group": "group", "torch_clip": "torch_clip"}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def emit(row):
    row = {"tree": TREE, **row}
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


class Arm:
    def __init__(self, shapes, kind, dtype):
        from dreamvla_amd.ddp import GradBucketReducer
        from dreamvla_amd.optim import FlatAdamW
        from gpu_param_groups_perf import two_groups
        gen = torch.Generator(device="cuda").manual_seed(17)
        params = [torch.nn.Parameter((torch.randn(s, generator=gen, device="cuda") * 0.02).to(dtype)) for s in shapes]
        self.red = GradBucketReducer(params, direct_grads=True)
        kw = {"clip": "group"} if kind == "group" else {}
        self.opt = FlatAdamW(self.red, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, param_groups=two_groups(params),
                             max_grad_norm=None if kind == "torch_clip" else MAX_NORM, **kw)
        assert self.opt.master_mode == (dtype == torch.float32) and len(self.opt.param_groups) == 2
        for b in self.red.buckets:
            b["flat"].normal_(0.0, 1e-3, generator=gen)
        self.kind = kind
        n_buckets = len(self.opt.flat)
        self.launches = {"global": 3 * n_buckets, "group": 2 * n_buckets + 2}.get(kind)
        if kind == "torch_clip":        # the views a training loop would hand to clip_grad_norm_
            for p in params:
                p.grad = self.red.grad_of(p)

    def step(self):
        if self.kind == "torch_clip":
            for g in self.opt.param_groups:
                torch.nn.utils.clip_grad_norm_(g["params"], MAX_NORM)
        self.opt.step()


def measure(shapes, layout, dtype_name):
    from dreamvla_amd import ops
    from gpu_param_groups_perf import time_block
    dtype = DTYPES[dtype_name]
    names = ARGS["arms"].split(",") if "arms" in ARGS else list(ARMS)
    ms, host_ms, iters, info = {n: [] for n in names}, {n: [] for n in names}, {}, {}
    for r in range(ROUNDS):
        for n in names:                                      # interleaved: drift of the box shows in every arm
            arm = Arm(shapes, ARMS[n], dtype)
            time_block(arm, 10)                              # warm-up (first launches, tables, the first step's shadow hand-over)
            if n not in iters:                               # size the block to >= 1 s
                iters[n] = max(20, int(1100.0 / time_block(arm, 20)[0]) + 1)
            dev, host = time_block(arm, iters[n])
            ms[n].append(dev)
            host_ms[n].append(host)
            info[n] = {"launches_per_step": arm.launches}
            if r == 0 and n == names[0]:
                emit({"what": "setup", "dtype": dtype_name, "layout": layout, "tensors": len(shapes),
                      "elements": sum(p.numel() for p in arm.red.params), "buckets": [int(b["flat"].numel()) for b in arm.red.buckets],
                      "group_elements": [sum(p.numel() for p in g["params"]) for g in arm.opt.param_groups], "rounds": ROUNDS,
                      "max_grad_norm": MAX_NORM, "device": torch.cuda.get_device_name(0)})
            del arm
            ops.invalidate_shadows()                         # the cached shadows keep the arm's flat buffers alive
    for n in names:
        emit({"what": "arm", "dtype": dtype_name, "arm": n, **info[n], "steps_per_block": iters[n],
              "ms_per_step": [round(x, 4) for x in ms[n]], "median_ms": round(statistics.median(ms[n]), 4),
              "min_ms": round(min(ms[n]), 4), "max_ms": round(max(ms[n]), 4),
              "host_ms_per_step_call": round(statistics.median(host_ms[n]), 4)})
    med = {n: statistics.median(v) for n, v in ms.items()}
    summary = {"what": "summary", "dtype": dtype_name}
    if "global" in med and "global_again" in med:
        both = ms["global"] + ms["global_again"]
        summary["global_again_over_global"] = round(med["global_again"] / med["global"], 4)
        summary["global_scatter_ms"] = round(max(both) - min(both), 4)
        summary["global_scatter_relative"] = round(summary["global_scatter_ms"] / med["global"], 4)
    if "global" in med and "group" in med:
        summary["group_over_global"] = round(med["group"] / med["global"], 4)
        summary["group_minus_global_ms"] = round(med["group"] - med["global"], 4)
    if "group" in med and "torch_clip" in med:
        summary["torch_clip_over_group"] = round(med["torch_clip"] / med["group"], 4)
    if len(summary) > 2:
        emit(summary)


def main():
    assert torch.cuda.is_available(), "a measurement on the GPU: no fallback"
    from gpu_guarded_step_perf import SYNTHETIC_BUCKETS, model_shapes
    layout = "synthetic"
    shapes = [(n,) for n in SYNTHETIC_BUCKETS]
    if "synthetic" not in ARGS:
        try:
            shapes, layout = model_shapes(), "model"
        except Exception as e:            # the fallback the docstring names; the row says which layout was timed
            print(f"model layout unavailable ({type(e).__name__}: {e}); synthetic buckets", flush=True)
    for dtype_name in ARGS.get("dtypes", "f32,bf16").split(","):
        measure(shapes, layout, dtype_name)


if __name__ == "__main__":
    main()
