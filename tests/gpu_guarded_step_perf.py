"""What the guarded optimizer step costs (a measurement script, not a test): FlatAdamW.step() alone, guard off against
FlatAdamW(skip_nonfinite=True), on the parameter layout of the shipped precision (`--precision fp32 --bf16_module
vision_encoder`, head set C, 24 layers: the trainable parameters as fp32 masters in GradBucketReducer's default buckets).  One
JSON line per arm and one summary line on stdout and, appended, in the file named by --out=PATH (the recorded run is kept as
profiles/r17_guarded_step_perf.jsonl).

    python tests/gpu_guarded_step_perf.py [--out=PATH] [--synthetic] [--arms=a,b,...] [--rounds=N] [--tree=NAME]

--tree=NAME is copied into every row.  The script runs unchanged from a checkout of an older commit (copied into its tests/)
with --arms=off_clip,off_noclip: the unguarded arms pass no new argument to FlatAdamW.  The recorded file holds such rows of
the parent commit (tree "parent"), taken in the same call as the rows of this tree.

Layout: the shapes of the model's trainable parameters (the model is built on the host only to read them); if the model cannot be
built, or with --synthetic, one tensor per bucket with the bucket sizes of that layout (496 627 470 elements: seven 256-MiB buckets,
one of 10 088 206 elements and the 64-MiB bucket that is filled last).  Every parameter is stepped (no learned unused set), the
gradients are normal noise of norm >> 0.1, so clipping is active.

Arms, each with an optimizer, parameters, moments and gradients of its own, built afresh for every timed block and dropped after
it -- dreamvla_amd.ops walks every cached shadow and every registered flat buffer after each step(), so five optimizers alive at
once would make each other's steps host-bound:
  off_clip             guard off, max_grad_norm = 0.1 (the shipped configuration)
  on_clip              guard on,  max_grad_norm = 0.1
  on_clip_all_skipped  guard on,  max_grad_norm = 0.1, one NaN in the gradient: every step is skipped
  off_noclip           guard off, max_grad_norm = None: computes no norm
  on_noclip            guard on,  max_grad_norm = None: computes the norm for the verdict -- that pass is the cost of this arm
Timing: device events around a block of back-to-back step() calls sized to at least a second (the guarded arms keep at most 8 steps
in flight, which is part of what is measured), ROUNDS rounds with the arms interleaved; per arm the per-round ms per step, median,
min and max, and the host's wall time per step() call in the same blocks (enqueue only for the unguarded arms; with the guard it
includes waiting for the oldest readback once 8 steps are in flight).  The margin for `on_clip - off_clip` is the scatter
(max - min) of off_clip in the same run."""
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARGS = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
OUT = ARGS.get("out")
TREE = ARGS.get("tree", "this")
ROUNDS = int(ARGS.get("rounds", 5))
SYNTHETIC_BUCKETS = [67108864] * 7 + [10088206, 16777216]
ARMS = {"off_clip": (False, 0.1, False), "on_clip": (True, 0.1, False), "on_clip_all_skipped": (True, 0.1, True),
        "off_noclip": (False, None, False), "on_noclip": (True, None, False)}      # guard, max_grad_norm, poisoned


def emit(row):
    row = {"tree": TREE, **row}
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def model_shapes():
    """shapes of the trainable parameters of head set C in the shipped precision, in model.parameters() order"""
    from bench import model_cfg
    from dreamvla_amd.dreamvla_model import DreamVLA
    model = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **model_cfg("C", 7, 24))
    model.vision_encoder.requires_grad_(False)
    model.clip_model.requires_grad_(False)
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


def build_arm(shapes, guard, max_norm, poisoned):
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    gen = torch.Generator(device="cuda").manual_seed(17)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, device="cuda") * 0.02) for s in shapes]
    red = GradBucketReducer(params, direct_grads=True)
    opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-4, max_grad_norm=max_norm, **({"skip_nonfinite": True} if guard else {}))
    assert opt.master_mode
    for b in red.buckets:
        b["flat"].normal_(0.0, 1e-3, generator=gen)
    if poisoned:
        red.buckets[-1]["flat"][12345] = float("nan")
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
    warnings.simplefilter("ignore", RuntimeWarning)          # the all-skipped arm announces its first skip
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
            red, opt = build_arm(shapes, *ARMS[n])
            time_block(opt, 10)                              # warm-up (first launches, the first step's shadow refresh)
            if n not in iters:                               # size the block to >= 1 s
                iters[n] = max(20, int(1100.0 / time_block(opt, 20)[0]) + 1)
            dev, host = time_block(opt, iters[n])
            ms[n].append(dev)
            host_ms[n].append(host)
            guard, max_norm, _ = ARMS[n]
            info[n] = {"launches_per_step": (2 * len(opt.flat) if guard or max_norm is not None else 0)
                       + sum(len(opt._ranges(bi)) for bi in range(len(opt.flat))) + (1 if guard else 0),
                       "copies_per_step": 1 if guard else 0}
            if guard:
                info[n].update({"applied": opt.applied_steps, "skipped": opt.skipped_steps})
            if r == 0 and n == names[0]:
                emit({"what": "setup", "layout": layout, "tensors": len(shapes), "elements": sum(p.numel() for p in red.params),
                      "buckets": [int(b["flat"].numel()) for b in red.buckets], "rounds": ROUNDS,
                      "device": torch.cuda.get_device_name(0)})
            del red, opt
            ops.invalidate_shadows()                         # the cached shadows keep the arm's flat buffers alive
    for n in names:
        emit({"what": "arm", "arm": n, "guard": ARMS[n][0], "max_grad_norm": ARMS[n][1], "steps_per_block": iters[n],
              "ms_per_step": [round(x, 4) for x in ms[n]], "median_ms": round(statistics.median(ms[n]), 4),
              "min_ms": round(min(ms[n]), 4), "max_ms": round(max(ms[n]), 4),
              "host_ms_per_step_call": round(statistics.median(host_ms[n]), 4), **info[n]})
    med = {n: statistics.median(v) for n, v in ms.items()}
    summary = {"what": "summary"}
    if "off_clip" in med and "on_clip" in med:
        scatter = max(ms["off_clip"]) - min(ms["off_clip"])
        d = med["on_clip"] - med["off_clip"]
        summary.update({"on_clip_minus_off_clip_us": round(d * 1e3, 2), "off_clip_scatter_us": round(scatter * 1e3, 2),
                        "within_scatter": bool(abs(d) <= scatter),
                        "added_per_step": "1 single-wave launch (dvla_step_verdict), 1 32-byte device-to-host copy, 1 event"})
        if "on_clip_all_skipped" in med:
            summary["all_skipped_ms"] = round(med["on_clip_all_skipped"], 4)
    if "off_noclip" in med and "on_noclip" in med:
        summary["on_noclip_minus_off_noclip_us"] = round((med["on_noclip"] - med["off_noclip"]) * 1e3, 2)
        summary["on_noclip_note"] = "the norm pass over every gradient bucket, which the unguarded step without clipping does not run"
    if len(summary) > 1:
        emit(summary)


if __name__ == "__main__":
    main()
