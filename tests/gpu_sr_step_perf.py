"""What stochastic rounding costs in the optimizer step (a measurement script, not a test): FlatAdamW.step() alone on the
trainable parameters of head set C (24 layers) as **bf16** buckets of GradBucketReducer -- the pure-bf16 mode `bench.py --precision
bf16` measures: parameters, gradients and both moments bf16, 14 B / parameter / step.  Layout and timing are those of
tests/gpu_guarded_step_perf.py and tests/gpu_param_groups_perf.py.  One JSON line per arm and one summary line on stdout and,
appended, in the file named by --out=PATH (the recorded run is kept as profiles/r20_sr_step_perf.jsonl).

    python tests/gpu_sr_step_perf.py [--out=PATH] [--synthetic] [--arms=a,b,...] [--rounds=N] [--tree=NAME]

--tree=NAME is copied into every row.  The script runs unchanged from a checkout of an older commit (copied into its tests/, next
to gpu_guarded_step_perf.py) with --arms=off,off_again: those arms pass no new argument to FlatAdamW.

Arms (max_grad_norm = 0.1), each with an optimizer, parameters, moments and gradients of its own, built afresh for every timed
block and dropped after it:
  off         stochastic_rounding off: dvla_adamw_bf16, the step as it was
  on          stochastic_rounding=True: dvla_adamw_bf16_sr -- the same bytes, two more hashes and three integer roundings per element
  off_again   the off arm once more: what two runs of the same code differ by
Timing: device events around a block of back-to-back steps sized to at least a second, ROUNDS rounds with the arms interleaved,
medians."""
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
LR, WD, BETAS, EPS, MAX_NORM = 1e-4, 1e-4, (0.9, 0.999), 1e-8, 0.1
ARMS = {"off": False, "on": True, "off_again": False}
BYTES_PER_ELEMENT = 14 + 2          # the step's 14 B + the gradient read once more for the clip norm


def emit(row):
    row = {"tree": TREE, **row}
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def build_arm(shapes, sr):
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    gen = torch.Generator(device="cuda").manual_seed(17)
    params = [torch.nn.Parameter((torch.randn(s, generator=gen, device="cuda") * 0.02).to(torch.bfloat16)) for s in shapes]
    red = GradBucketReducer(params, direct_grads=True)
    opt = FlatAdamW(red, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM,
                    **({"stochastic_rounding": True, "sr_seed": 1234} if sr else {}))
    assert not opt.master_mode
    for b in red.buckets:
        b["flat"].copy_(torch.randn(b["flat"].numel(), generator=gen, device="cuda") * 1e-3)
    return red, opt


def time_block(opt, iters):
    """-> (device ms per step, host ms per step() call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        opt.step()
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
    names = ARGS["arms"].split(",") if "arms" in ARGS else list(ARMS)
    ms, host_ms, iters, elements = {n: [] for n in names}, {n: [] for n in names}, {}, 0
    for r in range(ROUNDS):
        for n in names:                                      # interleaved: drift of the box shows in every arm
            red, opt = build_arm(shapes, ARMS[n])
            time_block(opt, 10)                              # warm-up
            if n not in iters:                               # size the block to >= 1 s
                iters[n] = max(20, int(1100.0 / time_block(opt, 20)[0]) + 1)
            dev, host = time_block(opt, iters[n])
            ms[n].append(dev)
            host_ms[n].append(host)
            elements = sum(int(b["flat"].numel()) for b in red.buckets)
            if r == 0 and n == names[0]:
                emit({"what": "setup", "layout": layout, "dtype": "bf16", "tensors": len(shapes),
                      "elements": sum(p.numel() for p in red.params), "buckets": [int(b["flat"].numel()) for b in red.buckets],
                      "rounds": ROUNDS, "max_grad_norm": MAX_NORM, "device": torch.cuda.get_device_name(0)})
            del red, opt
    for n in names:
        med = statistics.median(ms[n])
        emit({"what": "arm", "arm": n, "stochastic_rounding": ARMS[n], "steps_per_block": iters[n],
              "ms_per_step": [round(x, 4) for x in ms[n]], "median_ms": round(med, 4), "min_ms": round(min(ms[n]), 4),
              "max_ms": round(max(ms[n]), 4), "host_ms_per_step_call": round(statistics.median(host_ms[n]), 4),
              "tb_per_s_at_16_bytes_per_element": round(elements * BYTES_PER_ELEMENT / (med * 1e-3) / 1e12, 3)})
    med = {n: statistics.median(v) for n, v in ms.items()}
    summary = {"what": "summary"}
    if "off" in med and "off_again" in med:
        both = ms["off"] + ms["off_again"]
        summary["off_again_over_off"] = round(med["off_again"] / med["off"], 4)
        summary["off_scatter_ms"] = round(max(both) - min(both), 4)
        summary["off_scatter_relative"] = round(summary["off_scatter_ms"] / med["off"], 4)
    if "off" in med and "on" in med:
        summary["on_over_off"] = round(med["on"] / med["off"], 4)
    if len(summary) > 1:
        emit(summary)


if __name__ == "__main__":
    main()
