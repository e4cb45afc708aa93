"""Timing of the training step in the shipped precision (GPU box only, not a test): head set C, B = 32, 24 layers,
`--precision fp32 --bf16_module vision_encoder` (trainable parameters are fp32 masters, the vision encoder bf16 and frozen).
Two optimizer variants, alternated in one process on two copies of the model:

  unchanged_caller : plain autograd gradients, clip_grad_norm_(0.1) + torch.optim.AdamW (train.py:174 as written: default
                     foreach path); every trainable weight is re-cast to its bf16 shadow at the next forward
  flat_master      : GradBucketReducer(direct_grads=True) + FlatAdamW master mode (dvla_sumsq_f32 + dvla_adamw_f32_master,
                     which also writes the shadows: no re-cast)

For each: ms per whole step and the optimizer phase alone (device events around it), repeated, with the spread; the trainable
fp32 parameter count and the byte lower bound of the fused step; fp32 -> bf16 casts of trainable weights per step.
`--variant flat_master --steps N --no-tune` is the short run to put under `rocprofv3 --kernel-trace --stats`.
Prints JSON lines; with `--out PATH` also writes them to PATH (profiles/r07_master_step_perf.jsonl is such a run)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF = torch.bfloat16
HBM_TBS = 6.3        # achievable HBM bandwidth of the MI355X (float4 copy; 8.0 TB/s spec)


def build(heads, S, B, layers, variant):
    from bench import label_heads, model_cfg
    from dreamvla_amd import losses
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.dreamvla_model import DreamVLA
    from dreamvla_amd.optim import FlatAdamW
    from dreamvla_amd.synthetic import synthetic_batch
    torch.manual_seed(1234)
    cfg = model_cfg(heads, S, layers)
    model = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg)
    model = model.float()                                   # --precision fp32
    model.vision_encoder.bfloat16()                         # --bf16_module vision_encoder
    model.vision_encoder.requires_grad_(False)
    model.clip_model.requires_grad_(False)
    model = model.to("cuda")
    model._init_model_type()
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    assert all(p.dtype == torch.float32 for p in params)
    b = synthetic_batch(B, S, window=S + 3, seed=1234, heads=label_heads(heads))
    b["actions"][..., 6:] = (b["actions"][..., 6:] > 0.5).float()
    batch = {k: v.to("cuda") for k, v in b.items()}        # fp32 inputs, as under `--precision fp32`
    lab = losses.label_actions(batch["actions"], S, 3)
    red = opt = None
    if variant == "flat_master":
        red = GradBucketReducer(params, direct_grads=True)
        opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1)
        assert opt.master_mode
        red.flat_optimizer = opt
    else:
        opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-4)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def step(timed=False):
        if red is not None:
            red.zero_grad()
        else:
            opt.zero_grad()
        if timed:
            ev[0].record()
        out = model(batch["image_primary"][:, :S], batch["image_wrist"][:, :S], batch["state"][:, :S],
                    batch["text_token"][:, :S], action=batch["actions"][:, :S], action_label=lab, mode="train")
        total, _ = losses.calvin_losses(out, batch, sequence_length=S, use_dit_head=cfg["use_dit_head"], label_action=lab)
        total.backward()
        if red is not None:
            red.finish()
        if timed:
            ev[1].record()
        if red is None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
        opt.step()
        if timed:
            ev[2].record()
        return total

    info = {"trainable_params": sum(p.numel() for p in params), "trainable_tensors": len(params)}
    if red is not None:
        info["buckets"] = len(red.buckets)
    return model, params, step, ev, info, red


def count_weight_casts(model, step):
    """fp32 -> bf16 cast_to calls in one (untimed) step: on trainable masters / on anything else"""
    from dreamvla_amd import ops
    ptrs = {p.data_ptr() for p in model.parameters() if p.requires_grad and p.dtype == torch.float32}
    orig, n = ops.cast_to, {"trainable_weights": 0, "other": 0}

    def wrapped(x, dtype):
        if x.dtype == torch.float32 and dtype == BF:
            n["trainable_weights" if x.data_ptr() in ptrs else "other"] += 1
        return orig(x, dtype)
    ops.cast_to = wrapped
    try:
        step()
        torch.cuda.synchronize()
    finally:
        ops.cast_to = orig
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", default="C")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=7)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--variant", default="both", choices=["both", "unchanged_caller", "flat_master"])
    ap.add_argument("--steps", type=int, default=10, help="timed steps per repeat and variant (> 1 s at B = 32)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tune-steps", type=int, default=16)
    ap.add_argument("--no-tune", action="store_true", help="GEMM tuner off (the short profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available()
    from dreamvla_amd.ops import GemmTuner
    if args.no_tune:
        GemmTuner.enabled = False
    variants = ["unchanged_caller", "flat_master"] if args.variant == "both" else [args.variant]
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    runs = {v: build(args.heads, args.seq, args.batch, args.layers, v) for v in variants}
    for v in variants:
        model, params, step, ev, info, red = runs[v]
        for _ in range(0 if args.no_tune else args.tune_steps):
            step()
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if red is not None:
            red.copied = 0
        casts = count_weight_casts(model, step)
        extra = {}
        if red is not None:
            extra["reducer_copied_in_that_step"] = red.copied
        emit({"what": "setup", "variant": v, **info, "fp32_to_bf16_casts_per_step": casts, **extra})
    res = {v: {"step_ms": [], "opt_ms": [], "opt_ms_per_step": []} for v in variants}
    for r in range(args.repeats):
        for v in variants:          # alternated: drift of the box shows in both
            model, params, step, ev, info, red = runs[v]
            opt_ms = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(timed=True)
                ev[2].synchronize()
                opt_ms.append(ev[1].elapsed_time(ev[2]))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[v]["step_ms"].append(dt / args.steps * 1e3)
            res[v]["opt_ms"].append(statistics.median(opt_ms))
    for v in variants:
        model, params, step, ev, info, red = runs[v]
        s, o = res[v]["step_ms"], res[v]["opt_ms"]
        d = {"what": "timing", "variant": v, "heads": args.heads, "batch": args.batch, "layers": args.layers,
             "steps_per_repeat": args.steps, "repeats": args.repeats,
             "step_ms_median": round(statistics.median(s), 2), "step_ms_min": round(min(s), 2), "step_ms_max": round(max(s), 2),
             "opt_phase_ms_median": round(statistics.median(o), 3), "opt_phase_ms_min": round(min(o), 3),
             "opt_phase_ms_max": round(max(o), 3),
             "note": "step_ms: host wall clock over the repeat, each step ends with an event sync (the optimizer-phase "
                     "timing); opt phase: device events from after backward (+ reducer.finish) to after the optimizer"}
        if v == "flat_master":
            opt = red.flat_optimizer
            n = sum(hi - lo for bi in range(len(opt.flat)) for lo, hi in opt._ranges(bi))   # after learning the unused set
            d["stepped_elements"] = n
            # read p, g, m, v (16 B) + write p, m, v (12 B) + shadow (2 B) in the AdamW kernel, + the norm pass reading g (4 B)
            bytes_lb = n * (16 + 12 + 2 + 4)
            d.update({"bytes_per_element": 34, "bytes_lower_bound": bytes_lb,
                      "hbm_bound_ms_at_6.3TBs": round(bytes_lb / (HBM_TBS * 1e12) * 1e3, 3),
                      "achieved_TBs": round(bytes_lb / (statistics.median(o) * 1e-3) / 1e12, 2)})
        emit(d)
    if len(variants) == 2:
        a, b = (statistics.median(res[v]["step_ms"]) for v in variants)
        oa, ob = (statistics.median(res[v]["opt_ms"]) for v in variants)
        emit({"what": "swap", "step_ms_saved": round(a - b, 2), "opt_phase_ms_saved": round(oa - ob, 3),
              "step_speedup": round(a / b, 3)})
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
