"""What the EMA inside the optimizer step costs (a measurement script, not a test): FlatAdamW.step() alone on the parameter
layout of the shipped precision (`--precision fp32 --bf16_module vision_encoder`, head set C, 24 layers: the trainable parameters
as fp32 masters in GradBucketReducer's default buckets -- the workload of tests/gpu_guarded_step_perf.py, whose layout and timing
this script reuses).  One JSON line per arm and one summary line on stdout and, appended, in the file named by --out=PATH (the
recorded run is kept as profiles/r18_ema_step_perf.jsonl).

    python tests/gpu_ema_step_perf.py [--out=PATH] [--synthetic] [--arms=a,b,...] [--rounds=N] [--tree=NAME]

--tree=NAME is copied into every row.  The script runs unchanged from a checkout of an older commit (copied into its tests/, next
to gpu_guarded_step_perf.py) with --arms=plain: that arm passes no new argument to FlatAdamW.

Arms (max_grad_norm = 0.1, the shipped configuration), each with an optimizer, parameters, moments and gradients of its own, built
afresh for every timed block and dropped after it:
  plain         no EMA: the step as it was                                            30 B / element
  plain_again   the same arm once more: what two runs of the same code differ by
  fused         ema_decay = 0.9999: the EMA updated by the step kernel                + 8 B / element
  foreach_lerp  plain, followed by torch._foreach_lerp_(emas, params, 1 - 0.9999) over per-parameter fp32 EMA tensors -- what a
                user keeps by hand beside the optimizer                               + 12 B / element, ~9 multi-tensor launches
Timing as in tests/gpu_guarded_step_perf.py: device events around a block of back-to-back steps sized to at least a second, ROUNDS
rounds with the arms interleaved, medians.  Then one ema_weights() enter + exit on the fused arm's optimizer (two launches per
bucket: 8 + 8 + 2 B / element each), device time by events, median of 5."""
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
DECAY = 0.9999
ARMS = {"plain": (False, False), "plain_again": (False, False), "fused": (True, False), "foreach_lerp": (False, True)}   # ema_decay, by hand


def emit(row):
    row = {"tree": TREE, **row}
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


class Arm:
    def __init__(self, shapes, fused, by_hand):
        from dreamvla_amd.ddp import GradBucketReducer
        from dreamvla_amd.optim import FlatAdamW
        gen = torch.Generator(device="cuda").manual_seed(17)
        params = [torch.nn.Parameter(torch.randn(s, generator=gen, device="cuda") * 0.02) for s in shapes]
        self.red = GradBucketReducer(params, direct_grads=True)
        self.opt = FlatAdamW(self.red, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1, **({"ema_decay": DECAY} if fused else {}))
        assert self.opt.master_mode
        for b in self.red.buckets:
            b["flat"].normal_(0.0, 1e-3, generator=gen)
        self.params = [p.data for p in params]
        self.emas = [p.detach().clone() for p in params] if by_hand else None

    def step(self):
        self.opt.step()
        if self.emas is not None:
            torch._foreach_lerp_(self.emas, self.params, 1.0 - DECAY)


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


def time_swap(opt, reps=5):
    """device ms of one ema_weights() enter + exit"""
    out = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        with opt.ema_weights():
            pass
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out[1:]                                           # the first one loads the kernel


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
    ms, host_ms, iters, swap_ms = {n: [] for n in names}, {n: [] for n in names}, {}, None
    for r in range(ROUNDS):
        for n in names:                                      # interleaved: drift of the box shows in every arm
            arm = Arm(shapes, *ARMS[n])
            time_block(arm, 10)                              # warm-up (first launches, the first step's shadow hand-over)
            if n not in iters:                               # size the block to >= 1 s
                iters[n] = max(20, int(1100.0 / time_block(arm, 20)[0]) + 1)
            dev, host = time_block(arm, iters[n])
            ms[n].append(dev)
            host_ms[n].append(host)
            if r == 0 and n == names[0]:
                emit({"what": "setup", "layout": layout, "tensors": len(shapes), "elements": sum(p.numel() for p in arm.red.params),
                      "buckets": [int(b["flat"].numel()) for b in arm.red.buckets], "rounds": ROUNDS, "ema_decay": DECAY,
                      "device": torch.cuda.get_device_name(0)})
            if n == "fused" and r == ROUNDS - 1:
                swap_ms = time_swap(arm.opt)
            del arm
            ops.invalidate_shadows()                         # the cached shadows keep the arm's flat buffers alive
    for n in names:
        emit({"what": "arm", "arm": n, "ema_in_step": ARMS[n][0], "foreach_lerp_after_step": ARMS[n][1], "steps_per_block": iters[n],
              "ms_per_step": [round(x, 4) for x in ms[n]], "median_ms": round(statistics.median(ms[n]), 4),
              "min_ms": round(min(ms[n]), 4), "max_ms": round(max(ms[n]), 4),
              "host_ms_per_step_call": round(statistics.median(host_ms[n]), 4)})
    med = {n: statistics.median(v) for n, v in ms.items()}
    summary = {"what": "summary"}
    if "plain" in med and "plain_again" in med:
        summary["plain_again_over_plain"] = round(med["plain_again"] / med["plain"], 4)
        summary["plain_scatter_ms"] = round(max(ms["plain"] + ms["plain_again"]) - min(ms["plain"] + ms["plain_again"]), 4)
    if "plain" in med and "fused" in med:
        summary["fused_over_plain"] = round(med["fused"] / med["plain"], 4)
        summary["fused_over_plain_estimated_from_bytes"] = round(38.0 / 30.0, 4)
    if "plain" in med and "foreach_lerp" in med:
        summary["foreach_lerp_over_plain"] = round(med["foreach_lerp"] / med["plain"], 4)
        summary["foreach_lerp_over_plain_estimated_from_bytes"] = round(42.0 / 30.0, 4)
    if "fused" in med and "foreach_lerp" in med:
        summary["fused_is_faster_than_foreach_lerp"] = bool(med["fused"] < med["foreach_lerp"])
        summary["fused_minus_foreach_lerp_ms"] = round(med["fused"] - med["foreach_lerp"], 4)
    if swap_ms is not None:
        summary["ema_weights_enter_plus_exit_ms"] = [round(x, 4) for x in swap_ms]
        summary["ema_weights_enter_plus_exit_median_ms"] = round(statistics.median(swap_ms), 4)
    if len(summary) > 1:
        emit(summary)


if __name__ == "__main__":
    main()
