"""What parameter groups cost in the optimizer step (a measurement script, not a test): FlatAdamW.step() alone on the parameter
layout of the shipped precision (`--precision fp32 --bf16_module vision_encoder`, head set C, 24 layers: the trainable parameters
as fp32 masters in GradBucketReducer's default buckets -- the workload of tests/gpu_guarded_step_perf.py and
tests/gpu_ema_step_perf.py, whose layout and timing this script reuses).  One JSON line per arm and one summary line on stdout
and, appended, in the file named by --out=PATH (the recorded run is kept as profiles/r19_param_groups_perf.jsonl).

    python tests/gpu_param_groups_perf.py [--out=PATH] [--synthetic] [--arms=a,b,...] [--rounds=N] [--tree=NAME]

--tree=NAME is copied into every row.  The script runs unchanged from a checkout of an older commit (copied into its tests/, next
to gpu_guarded_step_perf.py) with --arms=one: that arm passes no new argument to FlatAdamW.

Arms (max_grad_norm = 0.1, the shipped configuration), each with an optimizer, parameters, moments and gradients of its own, built
afresh for every timed block and dropped after it:
  one         one group: the step as it was                                            30 B / element, one launch per bucket
  one_again   the same arm once more: what two runs of the same code differ by
  grouped     the two groups of weight_decay_groups (no decay on parameters with ndim <= 1) through
              dvla_adamw_f32_master_grouped                                             + 0.125 B / element, one launch per bucket
  per_range   the same two groups applied with the one-group entry point dvla_adamw_f32_master, one launch per parameter (the clip
              norm as the step computes it): what a user could do without the grouped kernels
Timing as in tests/gpu_guarded_step_perf.py: device events around a block of back-to-back steps sized to at least a second, ROUNDS
rounds with the arms interleaved, medians."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARGS = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
OUT = ARGS.get("out")
TREE = ARGS.get("tree", "this")
ROUNDS = int(ARGS.get("rounds", 5))
LR, WD, BETAS, EPS, MAX_NORM = 1e-3, 1e-4, (0.9, 0.999), 1e-8, 0.1
ARMS = {"one": "one", "one_again": "one", "grouped": "grouped", "per_range": "per_range"}


def emit(row):
    row = {"tree": TREE, **row}
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def two_groups(params):
    """weight_decay_groups by shape alone (the layout has no names); a layout of 1-D tensors only (--synthetic) is split by
    parity instead, so that the grouped arm does have two interleaved groups"""
    from dreamvla_amd.optim import weight_decay_groups
    groups = weight_decay_groups([(f"p{i}", p) for i, p in enumerate(params)], WD)
    if len(groups) == 2:
        return groups
    return [{"params": params[0::2], "weight_decay": 0.0}, {"params": params[1::2], "weight_decay": WD}]


class Arm:
    def __init__(self, shapes, kind):
        from dreamvla_amd.ddp import GradBucketReducer
        from dreamvla_amd.optim import FlatAdamW
        gen = torch.Generator(device="cuda").manual_seed(17)
        params = [torch.nn.Parameter(torch.randn(s, generator=gen, device="cuda") * 0.02) for s in shapes]
        self.red = GradBucketReducer(params, direct_grads=True)
        kw = {"param_groups": two_groups(params)} if kind == "grouped" else {}
        self.opt = FlatAdamW(self.red, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM, **kw)
        assert self.opt.master_mode
        for b in self.red.buckets:
            b["flat"].normal_(0.0, 1e-3, generator=gen)
        self.kind = kind
        self.launches = 2 * len(self.opt.flat) + len(self.opt.flat)
        if kind == "grouped":
            assert len(self.opt.param_groups) == 2
            self.group_sizes = [sum(p.numel() for p in g["params"]) for g in self.opt.param_groups]
        if kind == "per_range":
            wd_of = {id(p): g["weight_decay"] for g in two_groups(params) for p in g["params"]}
            self.ranges = [(s, off, p.numel(), wd_of[id(p)]) for b, s in zip(self.red.buckets, self.opt.flat)
                           for p, off in zip(b["params"], b["offsets"])]
            self.launches = 2 * len(self.opt.flat) + len(self.ranges)
            self.count = 0

    def step(self):
        if self.kind != "per_range":
            return self.opt.step()
        from dreamvla_amd import _lib
        lib, opt = _lib.load(), self.opt
        stream = torch.cuda.current_stream().cuda_stream
        self.count += 1
        for i, s in enumerate(opt.flat):
            _lib.check(lib.dvla_sumsq_f32(s["g"].data_ptr(), s["g"].numel(), opt._partial.data_ptr(), opt._sumsq.data_ptr(),
                                          1 if i > 0 else 0, stream), "dvla_sumsq_f32")
        sumsq = opt._sumsq.data_ptr()
        for s, off, n, wd in self.ranges:
            o = 4 * off
            _lib.check(lib.dvla_adamw_f32_master(s["p"].data_ptr() + o, s["g"].data_ptr() + o, s["m"].data_ptr() + o,
                                                 s["v"].data_ptr() + o, s["sh"].data_ptr() + 2 * off, n, LR, BETAS[0], BETAS[1], EPS,
                                                 wd, self.count, sumsq, MAX_NORM, stream), "dvla_adamw_f32_master")


def time_block(arm, iters):
    """-> (device ms per step, host ms per step() call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        arm.step()
    host = (time.perf_counter() - t0) / iters * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters, host


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
    from dreamvla_amd import ops
    names = ARGS["arms"].split(",") if "arms" in ARGS else list(ARMS)
    ms, host_ms, iters, info = {n: [] for n in names}, {n: [] for n in names}, {}, {}
    for r in range(ROUNDS):
        for n in names:                                      # interleaved: drift of the box shows in every arm
            arm = Arm(shapes, ARMS[n])
            time_block(arm, 10)                              # warm-up (first launches, the first step's shadow hand-over)
            if n not in iters:                               # size the block to >= 1 s
                iters[n] = max(20, int(1100.0 / time_block(arm, 20)[0]) + 1)
            dev, host = time_block(arm, iters[n])
            ms[n].append(dev)
            host_ms[n].append(host)
            info[n] = {"launches_per_step": arm.launches}
            if ARMS[n] == "grouped":
                info[n]["group_elements"] = arm.group_sizes
                info[n]["map_bytes"] = sum(int(m[1].numel()) for m in arm.opt._group_maps.values())
            if r == 0 and n == names[0]:
                emit({"what": "setup", "layout": layout, "tensors": len(shapes), "elements": sum(p.numel() for p in arm.red.params),
                      "buckets": [int(b["flat"].numel()) for b in arm.red.buckets], "rounds": ROUNDS, "max_grad_norm": MAX_NORM,
                      "device": torch.cuda.get_device_name(0)})
            del arm
            ops.invalidate_shadows()                         # the cached shadows keep the arm's flat buffers alive
    for n in names:
        emit({"what": "arm", "arm": n, **info[n], "steps_per_block": iters[n],
              "ms_per_step": [round(x, 4) for x in ms[n]], "median_ms": round(statistics.median(ms[n]), 4),
              "min_ms": round(min(ms[n]), 4), "max_ms": round(max(ms[n]), 4),
              "host_ms_per_step_call": round(statistics.median(host_ms[n]), 4)})
    med = {n: statistics.median(v) for n, v in ms.items()}
    summary = {"what": "summary"}
    if "one" in med and "one_again" in med:
        summary["one_again_over_one"] = round(med["one_again"] / med["one"], 4)
        summary["one_scatter_ms"] = round(max(ms["one"] + ms["one_again"]) - min(ms["one"] + ms["one_again"]), 4)
        summary["one_scatter_relative"] = round(summary["one_scatter_ms"] / med["one"], 4)
    if "one" in med and "grouped" in med:
        summary["grouped_over_one"] = round(med["grouped"] / med["one"], 4)
        summary["grouped_over_one_estimated_from_bytes"] = round(30.125 / 30.0, 4)
    if "one" in med and "per_range" in med:
        summary["per_range_over_one"] = round(med["per_range"] / med["one"], 4)
    if "grouped" in med and "per_range" in med:
        summary["per_range_over_grouped"] = round(med["per_range"] / med["grouped"], 4)
    if len(summary) > 1:
        emit(summary)


if __name__ == "__main__":
    main()
