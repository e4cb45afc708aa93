#!/usr/bin/env python
"""bench.py -- DreamVLA training-step throughput on MI355X (the metric of BASELINE.json).

    python bench.py --gpus N --steps K --warmup W          (N > 1: one rank per GPU under torch.distributed.run; started
                                                            without a launcher, the command re-executes itself under it)

One "step" = one full optimizer step of the hot path on one synthetic batch that is already resident in HBM:
DreamVLA.forward (frozen CLIP text tower + frozen ViT-B/16 on 2 views, resampler, 24-layer trunk with dropout, dream
heads, DiT diffusion head) -> reference loss block -> backward -> gradient all-reduce (N > 1) -> clip_grad_norm_(0.1)
-> AdamW, in bf16 (`--precision bf16` semantics of train.py:122-123).  Workload = BASELINE.json configs[1]
(B = 32 per GPU, S = 7, 2 x 224^2 views, 77 text tokens) with the head set of the shipped CALVIN finetune script
(obs + depth + sam dream heads, DiT head; L = 651).  rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set up (model, batch, GEMM tuner steps or a plan), warm up, time the steps,
write --dump-outputs if asked, print the line.  The legs below run after the timed region, and only with --full (each can
then be left out with its --no-* option); without --full their objects in the line are null.

Extra objects in the line (--full):
  fwd_ms_per_step : forward-only latency (train mode, autograd graph recorded, no backward), 3 steps after 1 un-timed.
  roofline     : the dominant kernels (gemm_ring_kernel / gemm_kernel, bf16 MFMA).  achieved = algorithmic FLOPs of every GEMM launch of one
                 instrumented step / summed launch durations (HIP events on the launch stream), peak = 2500 TFLOP/s dense.
  cpu_baseline : the oracle (oracle/model_ref.py, "port") timed on this box's host cores on a bounded sample (B = 2).
  eager_rocm_baseline : the same step run eagerly on PyTorch-ROCm bf16 on this GPU (the >= 4x target's denominator).
  loss_parity  : the loss of the trained HIP module against the oracle restatement in fp32 / bf16 on this GPU (loss_parity()).
  integration_levels : the untouched reference loop / + HIP loss block / headline configuration (integration_levels()).
  rollout      : BASELINE configs[4], 64 episodes in lock-step through the hipGraph-captured engine (tests/gpu_rollout_bench.py).
  other_configs : after the timed region, a few steps each of the configurations BASELINE.json names next to the headline one --
                 head set E (all dream heads, configs[3]), head set D driven with the LIBERO flags of finetune_long.sh (B = 16,
                 4-pass gradient accumulation through reducer.no_sync()), head set C at CALVIN's own window S = 10 (finetune.sh:37).
  rccl (N > 1 or --torch-ddp) : what the collective layer saw -- ranks counted by an all-reduce over the RCCL group, buckets,
                 bytes, how many buckets launched during backward, whether the robust GEMM schedule engaged.
--torch-ddp / --torch-adamw select the UNCHANGED caller's path (train.py:173-174, utils/train_utils.py:598-608: torch DDP with
find_unused_parameters, clip_grad_norm_, torch.optim.AdamW) at any N, N = 1 included (a one-rank RCCL group).
--dump-outputs DIR writes what the last timed step computed as .npy files (dump_outputs), so that two builds can be compared output
for output: with the same arguments the model, the batch, the dropout / DiT noise streams and (a committed plan replayed) the GEMM
configurations are the same from run to run.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HEAD_SETS = {
    "A": dict(obs_pred=True, use_dit_head=False),
    "B": dict(obs_pred=True, use_dit_head=True),
    "C": dict(obs_pred=True, depth_pred=True, sam_feat_pred=True, use_dit_head=True),      # CALVIN finetune.sh
    "D": dict(obs_pred=True, sam_feat_pred=True, use_dit_head=True),                      # LIBERO finetune_*.sh
    "E": dict(obs_pred=True, dino_feat_pred=True, sam_feat_pred=True, trajectory_pred=True, use_dit_head=True),
}
# algorithmic training GFLOP per sample (SURVEY.md section 8d / BASELINE.md section 4; mask-aware trunk attention)
TRAIN_GFLOP_PER_SAMPLE = {"A": 1802.0, "B": 1974.0, "C": 3485.0, "D": 2798.0, "E": 4317.0}
BF16_PEAK_TFLOPS = 2500.0


def model_cfg(heads, S, layers=24, phase="finetune"):
    cfg = dict(finetune_type="calvin", sequence_length=S, num_resampler_query=16, num_obs_token_per_image=9,
               action_pred_steps=3, transformer_layers=layers, hidden_dim=1024, transformer_heads=16, phase=phase,
               attn_implementation="sdpa",
               track_label_patch_size=8)     # the CLI default train.py passes (utils/arguments_utils.py:227), not the ctor's 4
    cfg.update(HEAD_SETS[heads])
    return cfg


def label_heads(heads):
    h = HEAD_SETS[heads]
    return tuple(k for k, f in (("depth", "depth_pred"), ("dino", "dino_feat_pred"), ("sam", "sam_feat_pred"),
                                ("traj", "trajectory_pred")) if h.get(f))


def cpu_baseline(heads, S):
    """Oracle forward + loss + backward on the host cores: BASELINE configs[0] (B = 2, S = 7, fp32), one un-timed
    warm-up step, then three timed steps (bounded: ~25-35 s on 16 threads)."""
    from oracle import model_ref as M
    from oracle import weights
    from dreamvla_amd.dreamvla_model import DreamVLA
    from dreamvla_amd import losses
    nthreads = min(os.cpu_count(), 16)   # oversubscribing a 256-thread host made this leg take 8 minutes
    torch.set_num_threads(nthreads)
    cfg = model_cfg(heads, S)
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg)
    sd = {k: (v.float() if torch.is_floating_point(v) else v) for k, v in m.state_dict().items()}
    del m
    leaves = {k: v.requires_grad_(True) for k, v in sd.items()
              if torch.is_floating_point(v) and not k.startswith(("clip_model.", "vision_encoder.")) and k != "attention_mask"
              and "decoder_position_embedding" not in k}
    B = 2
    b = weights.synthetic_batch(B, S, window=S + 3, seed=7, heads=label_heads(heads))
    b["actions"][..., 6:] = (b["actions"][..., 6:] > 0.5).float()
    lab = losses.label_actions(b["actions"], S, 3)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(8 * B * S, 3, 7, generator=g)
    tstep = torch.randint(0, 100, (8 * B * S,), generator=g)
    nsteps = 3
    t_fwd = 0.0
    t0 = None
    for it in range(nsteps + 1):
        if it == 1:
            t0 = time.time()           # the first (cold: allocator, thread pool, page faults) step is not timed
            t_fwd = 0.0
        for v in leaves.values():
            v.grad = None
        t1 = time.time()
        out = M.dreamvla_forward(sd, cfg, b["image_primary"][:, :S], b["image_wrist"][:, :S], b["state"][:, :S],
                                 b["text_token"][:, :S], action_label=lab, mode="train", dit_noise=noise, dit_timestep=tstep)
        t_fwd += time.time() - t1
        total, _ = losses.calvin_losses(out, b, sequence_length=S, use_dit_head=cfg["use_dit_head"], label_action=lab)
        total.backward()
    dt = time.time() - t0
    return {"value": B * nsteps / dt, "unit": "samples/s", "cores": nthreads, "kind": "port",
            "sample": f"{nsteps} timed steps after 1 warm-up of oracle/model_ref.py forward+loss+backward, fp32, B={B}, S={S}, "
                      f"head set {heads}, full 1024/24/16 model, {nthreads} threads of {os.cpu_count()}; "
                      f"fwd {t_fwd / nsteps:.2f} s + bwd {(dt - t_fwd) / nsteps:.2f} s per step"}


def eager_rocm_baseline(heads, S, B, steps=5):
    """The >= 4x target's denominator: the reference step run EAGERLY on
    PyTorch-ROCm on this same GPU in bf16 -- hipBLASLt GEMMs + SDPA + ATen elementwise, fused AdamW -- at the same B, S and
    head set.  The reference itself cannot travel to the GPU box, so this drives the oracle's functional restatement of it
    (tests/gpu_eager_baseline.py: same ATen op sequence; no dropout and no (B,1,L,L) mask copy, both of which would only
    make eager slower).  Baseline leg only: nothing here is on the product path."""
    from tests import gpu_eager_baseline
    return gpu_eager_baseline.run(heads, B, steps, S=S)


def reference_loop_loss_block(out, batch, lab, S, use_dit_head):
    """What the reference's OWN training loop does with the forward's outputs every step (utils/train_utils.py:158-596), for the
    integration-levels leg: the loss block as plain ATen ops in the model dtype (`dreamvla_amd.losses.calvin_losses(fused=False)`:
    the formulation tests/test_losses_golden.py pins against the real loop's values and gradients) AND the loop's per-step host work
    -- the four example images (:198-213: un-patchify the WHOLE prediction / label, take sample 0, `.detach().cpu().float().numpy()`,
    min-max normalise on the host), the four depth examples when the depth head is on (:382-396), and `loss.item()` (:596)."""
    import numpy as np
    from dreamvla_amd import losses
    total, parts = losses.calvin_losses(out, batch, sequence_length=S, use_dit_head=use_dit_head, label_action=lab, fused=False,
                                        compute_dtype=out[2].dtype if out[2] is not None else torch.bfloat16)
    image_pred, depth_pred = out[2], out[6]
    bs = batch["image_primary"].shape[0]
    lo, hi = 3, 3 + S

    def example(t):                                             # (B', P, 3, H, W) -> sample 0 / step 0 on the host, min-max normalised
        e = t[0][0].permute(1, 2, 0).detach().cpu().float().numpy()
        return (e - e.min()) / (e.max() - e.min())
    examples = []
    if image_pred is not None:
        ip = image_pred.reshape(bs, S, *image_pred.shape[1:]).reshape(-1, *image_pred.shape[1:])
        for v, key in ((0, "image_primary"), (1, "image_wrist")):
            examples.append(example(losses.unpatchify(ip[:, v])))
            lab_img = losses.normalize_patchfied_image(losses.patchify(batch[key][:, lo:hi].flatten(0, 1), 16))
            examples.append(example(losses.unpatchify(lab_img.unsqueeze(1))))
    if depth_pred is not None:
        dp = depth_pred.reshape(bs, S, *depth_pred.shape[1:]).reshape(-1, *depth_pred.shape[1:])
        for v, key in ((0, "depth_primary"), (1, "depth_wrist")):
            examples.append(example(losses.unpatchify(dp[:, v])))
            examples.append(example(batch[key][:, lo:hi].flatten(0, 1).unsqueeze(1)))
    loss_value = total.item()                                   # :596 mv_avg_loss.append(loss.item())
    return total, parts, (loss_value, len(examples))


def integration_levels(args, cfg, S, B, dev, headline_samples_per_s, steps=5, warmup=2):
    """Round-5 VERDICT #6: what a maintainer gets at each level of adoption, same box, same batch, N = 1, `steps` timed steps each:
      level 0 "untouched loop": only the import is swapped -- the HIP module inside the reference's own
              `DistributedDataParallel(find_unused_parameters=True)` (train.py:173), its own loss block incl. the per-step example-image
              copies and `.item()` reads (utils/train_utils.py:158-596, 726), `clip_grad_norm_` + `torch.optim.AdamW` as train.py:174
              builds it (no `fused=`);
      level 1 "+ HIP loss block": `dreamvla_amd.losses.calvin_losses` instead of the loop's loss block (one edit), no host reads inside
              the step;
      level 2 "+ reducer + flat optimizer" = the headline configuration (GradBucketReducer + FlatAdamW): the timed region's number."""
    import socket
    import torch.distributed as dist
    from dreamvla_amd import losses
    from dreamvla_amd.dreamvla_model import DreamVLA
    from dreamvla_amd.synthetic import synthetic_batch
    own_group = not dist.is_initialized()
    if own_group:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        BF = torch.bfloat16
        torch.manual_seed(1234)
        model = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg).bfloat16()
        model.clip_model.requires_grad_(False)
        model.vision_encoder.requires_grad_(False)
        model = model.to(dev)
        model._init_model_type()
        model.train()
        ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev.index], find_unused_parameters=True)      # train.py:173
        opt = torch.optim.AdamW([p for p in ddp.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-4)            # train.py:174
        b = synthetic_batch(B, S, window=S + 3, seed=1234, heads=label_heads(args.heads))
        b["actions"][..., 6:] = (b["actions"][..., 6:] > 0.5).float()
        batch = {k: (v.to(dev, BF) if torch.is_floating_point(v) else v.to(dev)) for k, v in b.items()}
        lab = losses.label_actions(batch["actions"], S, 3)
        inputs = (batch["image_primary"][:, :S].contiguous(), batch["image_wrist"][:, :S].contiguous(),
                  batch["state"][:, :S].contiguous(), batch["text_token"][:, :S].contiguous())

        def step(level):
            out = ddp(*inputs, action=batch["actions"][:, :S], action_label=lab, mode="train")
            if level == 0:
                total, parts, _ = reference_loop_loss_block(out, batch, lab, S, cfg["use_dit_head"])
            else:
                total, parts = losses.calvin_losses(out, batch, sequence_length=S, use_dit_head=cfg["use_dit_head"], label_action=lab)
            total.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)                                                         # :600
            opt.step()
            opt.zero_grad()
            if level == 0:                       # :726 t.set_postfix(...): nine .item() reads per step
                _ = [float(x.detach()) for x in (total, *(parts[k] for k in ("image", "depth", "arm_action", "gripper_action", "trajectory", "dino", "sam")))]
            return total
        res = {}
        for level, name in ((0, "untouched_loop"), (1, "hip_loss_block")):
            for _ in range(warmup):
                step(level)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(level)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            res[name] = {"samples_per_s": B / dt, "ms_per_step": dt * 1e3}
        res["reducer_and_flat_optimizer"] = {"samples_per_s": headline_samples_per_s, "ms_per_step": B / headline_samples_per_s * 1e3,
                                             "note": "the timed region of this line"}
        res["what"] = ("level 0: the HIP module in train.py's own DDP(find_unused_parameters=True) + the loop's ATen loss block with its per-step "
                       "example-image copies and .item() reads (utils/train_utils.py:158-596, 726) + clip_grad_norm_ + torch.optim.AdamW "
                       "(train.py:174, unfused); level 1: + dreamvla_amd.losses.calvin_losses; level 2: + GradBucketReducer + FlatAdamW")
        res["steps"] = steps
        return res
    finally:
        if own_group:
            dist.destroy_process_group()
            import ctypes
            ctypes.CDLL(None).fflush(None)      # (RCCL's version banner goes through C stdio: out now, not behind the JSON line)


def loss_parity(model, cfg, batch, lab, inputs, S, B, dev):
    """Cross-check of the number the timed steps print as `loss` (round-3 VERDICT weak #3: it was compared with nothing).
    After the timed region, with the weights as the optimizer left them: the loss of the HIP module in eval() mode (dropout
    off), DiT noise / timesteps injected, against the oracle's restatement of the reference forward + the same loss block on
    the SAME weights, batch and noise, run on this GPU by ATen in fp32 (`eager_fp32`: the value) and in bf16 (`eager_bf16`:
    what the reference's own `--precision bf16` arithmetic makes of it).  `rel` = |hip - fp32| / fp32;
    `reference_bf16_rel` = |eager_bf16 - fp32| / fp32 is the floor any bf16 implementation sits on.  Checker only: nothing
    of this runs inside the timed region."""
    from dreamvla_amd import losses
    from oracle import model_ref as M
    from oracle import torch_ref as R
    from tests.gpu_eager_baseline import sdpa_attention
    BF = torch.bfloat16
    use_dit = cfg["use_dit_head"]
    g = torch.Generator(device=dev).manual_seed(7)
    noise = torch.randn(8 * B * S, 3, 7, device=dev, generator=g).to(BF)
    tstep = torch.randint(0, 100, (8 * B * S,), device=dev, generator=g)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if use_dit:
                model.action_model._injected = (noise, tstep)
            out = model(*inputs, action=batch["actions"][:, :S], action_label=lab, mode="train")
            total, parts = losses.calvin_losses(out, batch, sequence_length=S, use_dit_head=use_dit, label_action=lab)
            l_hip = float(total)
    finally:
        if use_dit:
            model.action_model._injected = None
        model.train(was_training)
    res = {}
    keep = R.attention
    R.attention = sdpa_attention
    try:
        for name, dt in (("eager_fp32", torch.float32), ("eager_bf16", BF)):
            sd = {k: (v.detach().to(dt) if torch.is_floating_point(v) else v.detach()) for k, v in model.state_dict().items()}
            sd["attention_mask"] = sd["attention_mask"].float()
            bt = {k: (v.to(dt) if torch.is_floating_point(v) else v) for k, v in batch.items()}
            lb = lab.to(dt)
            with torch.no_grad():
                tf = M.clip_text(sd, "clip_model", bt["text_token"][:, :S].flatten(0, 1))
                o = M.dreamvla_forward(sd, cfg, bt["image_primary"][:, :S], bt["image_wrist"][:, :S], bt["state"][:, :S],
                                       bt["text_token"][:, :S], action_label=lb, mode="train", dit_noise=noise.to(dt),
                                       dit_timestep=tstep, text_feature=tf)
                t, _ = losses.calvin_losses(o, bt, sequence_length=S, use_dit_head=use_dit, label_action=lb)
            res[name] = float(t)
            del sd, bt, o
            torch.cuda.empty_cache()
    finally:
        R.attention = keep
    ref = res["eager_fp32"]
    rel = abs(l_hip - ref) / max(abs(ref), 1e-12)
    rel16 = abs(res["eager_bf16"] - ref) / max(abs(ref), 1e-12)
    return {"hip": l_hip, "eager_fp32": ref, "eager_bf16": res["eager_bf16"], "rel": rel, "reference_bf16_rel": rel16,
            "tolerance": max(1e-3, 1.25 * rel16), "ok": rel <= max(1e-3, 1.25 * rel16),
            "sample": "eval() (dropout off), weights after the timed steps, the bench batch, DiT noise / timesteps injected; "
                      "oracle restatement (oracle/model_ref.py) on this GPU in fp32 and bf16 as the checker"}


OTHER_CONFIGS = [
    # name, head set, S, per-GPU batch, accumulation passes, extra constructor keywords, extra loss keywords, synthetic-batch keywords
    ("E_all_dream_heads", "E", 7, 32, 1, {}, {}, {}),
    ("D_libero_finetune_long", "D", 7, 16, 4, dict(finetune_type="libero_finetune", gripper_width=True), dict(flow_as_mask=True),
     dict(gripper_width=True, tracks=True)),
    ("C_calvin_window_10", "C", 10, 32, 1, {}, {}, {}),
]


def other_config(name, heads, S, B, accum, extra_cfg, loss_kw, batch_kw, dev, steps=5, warmup=1):
    """One of the configurations BASELINE.json names beside the headline one, timed like the headline (same step: forward, loss
    block, backward, reducer, clip + AdamW; `accum` > 1: utils/train_utils.py:588-607's accumulation, all but the last pass under
    reducer.no_sync(), B samples per pass).  The GEMM configurations come from the committed plan of this configuration
    (profiles/r05_gemm_plan_<name>.json, written by `DVLA_SAVE_OTHER_PLANS=1 python bench.py` on the GPU) -- no tuner trials; without the
    file the tuner runs 12 untimed steps first."""
    from dreamvla_amd import losses, ops
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.dreamvla_model import DreamVLA
    from dreamvla_amd.ops import GemmTuner
    from dreamvla_amd.optim import FlatAdamW
    from dreamvla_amd.synthetic import synthetic_batch
    BF = torch.bfloat16
    cfg = model_cfg(heads, S)
    cfg.update(extra_cfg)
    torch.manual_seed(4321)
    model = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg).bfloat16()
    model.clip_model.requires_grad_(False)
    model.vision_encoder.requires_grad_(False)
    model = model.to(dev)
    model._init_model_type()
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    reducer = GradBucketReducer(params, direct_grads=True)
    opt = FlatAdamW(reducer, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1)
    passes = []
    for a in range(accum):
        b = synthetic_batch(B, S, window=S + 3, seed=99 + a, heads=label_heads(heads), **batch_kw)
        b["actions"][..., 6:] = (b["actions"][..., 6:] > 0.5).float()
        bt = {k: (v.to(dev, BF) if torch.is_floating_point(v) else v.to(dev)) for k, v in b.items()}
        lab = losses.label_actions(bt["actions"], S, 3)
        inp = tuple(bt[k][:, :S].contiguous() for k in ("image_primary", "image_wrist", "state", "text_token"))
        passes.append((bt, lab, inp))

    def one_pass(bt, lab, inp):
        out = model(*inp, action=bt["actions"][:, :S], action_label=lab, mode="train")
        total, _ = losses.calvin_losses(out, bt, sequence_length=S, use_dit_head=cfg["use_dit_head"], label_action=lab, **loss_kw)
        (total / accum).backward()
        return total

    def step():
        reducer.zero_grad()
        for bt, lab, inp in passes[:-1]:
            with reducer.no_sync():
                one_pass(bt, lab, inp)
        total = one_pass(*passes[-1])
        reducer.finish()
        opt.step()
        return total

    plan = os.path.join(ROOT, "profiles", f"r05_gemm_plan_{name}.json")
    GemmTuner.reset()
    GemmTuner.frozen = False
    tuned = "committed plan"
    if os.path.exists(plan):
        GemmTuner.load_plan(plan)
    elif GemmTuner.enabled:
        tuned = "12 untimed tuner steps (no committed plan for this configuration)"
        for _ in range(12):
            step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if os.environ.get("DVLA_SAVE_OTHER_PLANS"):
        GemmTuner.save_plan(plan)
    ms = dt / steps * 1e3
    res = {"samples_per_s": B * accum * steps / dt, "ms_per_optimizer_step": ms, "per_gpu_batch": B, "accumulation_passes": accum,
           "seq_len": S, "head_set": heads, "tokens_per_sample": int(model.attention_mask.shape[-1]) if hasattr(model, "attention_mask") else None,
           "flags": {**extra_cfg, **loss_kw}, "steps": steps, "loss": float(last.detach()),
           "loss_after_optimizer_steps": steps + warmup + (12 if tuned.startswith("12") else 0),      # (random init, lr 1e-3: the first steps start high)
           "gemm_configurations": tuned,
           "whole_step_frac_of_bf16_peak": TRAIN_GFLOP_PER_SAMPLE[heads] * (S / 7.0 if S != 7 else 1.0) * (B * accum * steps / dt) / 1e3 / BF16_PEAK_TFLOPS}
    del model, reducer, opt, params, passes
    GemmTuner.reset()
    GemmTuner.frozen = False
    torch.cuda.empty_cache()
    return res


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_spawn(n):
    """Re-execute `bench.py <same arguments>` as n ranks of one node (rendezvous on 127.0.0.1: the container host name may not
    resolve); returns the launcher's exit code.  Rank 0 of the children prints the JSON line on the inherited stdout."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
    port = env.get("MASTER_PORT") or str(free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def launch_selftest(rank, world, args):
    """`--launch-selftest`: everything of the N > 1 launch path that does not need a GPU -- environment of the launcher,
    rendezvous (gloo), the barrier and the max-over-ranks of the timed region -- ending in the JSON line on rank 0
    (tests/test_bench_launch.py runs it with --gpus 2 on CPU).  No model, no kernels: `value` is null."""
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "train samples/sec (CALVIN ABC->D, seq_len=7)", "value": None, "unit": "samples/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "launch_selftest": True,
                          "max_over_ranks_s": dt, "scaling": "weak"}), flush=True)
    if world > 1:
        dist.destroy_process_group()


DUMP_PER_TENSOR = 4096


def committed_gemm_plan():
    """the newest round's committed GEMM plan (profiles/rNN_gemm_plan.json, written by `bench.py --save-plan`), or None"""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_gemm_plan.json")))
    return cands[-1] if cands else None


def dump_outputs(out_dir, total, parts, named_params, grad_of):
    """--dump-outputs: what the timed path handed its caller in its last step, rank 0, right after the timed region (before any
    diagnostic leg steps the model again):
      loss.npy, loss_<part>.npy : the total loss and each term of the loss block (float64, shape (1,));
      params.npy, grads.npy     : for every trainable parameter in named_parameters() order, the same fixed sample (numpy
                                  default_rng(0), at most DUMP_PER_TENSOR elements per tensor, ascending) of the parameter after the
                                  optimizer step and of the gradient its storage holds (the reducer's bucket, or p.grad; zeros for a
                                  parameter without one), float32, concatenated -- ~11 MB for the default workload;
      param_sizes.npy           : how many sampled elements each parameter contributed (float64), to split the two above."""
    os.makedirs(out_dir, exist_ok=True)

    def save(name, a):
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    save("loss", np.array([float(total.detach())], dtype=np.float64))
    for k, v in parts.items():
        if torch.is_tensor(v):
            save(f"loss_{k}", np.array([float(v.detach())], dtype=np.float64))
    rng = np.random.default_rng(0)
    ps, gs, sizes = [], [], []
    for _, p in named_params:
        n = p.numel()
        idx = np.arange(n) if n <= DUMP_PER_TENSOR else np.sort(rng.choice(n, DUMP_PER_TENSOR, replace=False))
        idx = torch.from_numpy(idx).to(p.device)
        ps.append(p.detach().reshape(-1)[idx].float().cpu())
        g = grad_of(p)
        gs.append(torch.zeros(len(idx)) if g is None else g.detach().reshape(-1)[idx].float().cpu())
        sizes.append(len(idx))
    save("params", torch.cat(ps).numpy())
    save("grads", torch.cat(gs).numpy())
    save("param_sizes", np.array(sizes, dtype=np.float64))


def require_finite_loss(loss_val):
    """A model whose parameters have gone non-finite runs FASTER on this chip (round 6, measured: 139 -> 124 ms per step once every
    operand is NaN -- the matrix pipe toggles less and the clocks rise), so such a run must never print a throughput line."""
    if not math.isfinite(loss_val):
        raise SystemExit(f"bench.py: the loss of the last timed step is {loss_val} -- the timed steps did not train a finite model; "
                         "no throughput is reported (tests/probes/loss_trace.py prints loss / gradient norm / finiteness per step)")
    return loss_val


def extra_legs(args, rank, world):
    """The legs this rank runs after the timed region: none without --full; with it, every leg whose --no-* option is not given
    and that applies to this rank, world size, head set and path."""
    if not args.full:
        return frozenset()
    alone = rank == 0 and world == 1
    on = {
        "fwd": (rank == 0 or world > 1) and not args.no_fwd,
        "roofline": not args.no_roofline,
        "loss_parity": alone and not args.no_loss_parity,
        "cpu_baseline": alone and not args.no_cpu_baseline,
        "eager_baseline": alone and not args.no_eager_baseline,
        "integration_levels": alone and not args.no_integration_levels and not args.torch_ddp,
        "rollout": alone and not args.no_rollout and args.heads == "C",
        "other_configs": alone and not args.no_other_configs and args.heads == "C" and not args.torch_ddp,
        "rccl": world > 1 or args.torch_ddp,
    }
    return frozenset(k for k, v in on.items() if v)


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch (BASELINE configs[1]: 32)")
    ap.add_argument("--seq", type=int, default=7)
    ap.add_argument("--heads", default="C", choices=sorted(HEAD_SETS))
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--phase", default="finetune", choices=["finetune", "pretrain"],
                    help="pretrain: the attention mask is regenerated every training step (dreamvla_model.py:610-628) -- here "
                         "as device-side tables from the rule (SURVEY 8 f4); same shapes, for the f4 timing comparison")
    ap.add_argument("--plan", default=None, metavar="FILE",
                    help="replay the GEMM configuration choices saved by --save-plan (no tuner trials: for profiler / counter passes "
                         "of the tuned step); default: $DVLA_GEMM_PLAN")
    ap.add_argument("--save-plan", default=None, metavar="FILE", help="write the tuner's locked choices after the tune steps")
    ap.add_argument("--tune-steps", type=int, default=32,
                    help="untimed steps BEFORE the warm-up in which dreamvla_amd.ops.GemmTuner tries each GEMM kernel "
                         "configuration once per problem shape and locks the fastest (setup, like building the extension); "
                         "eight candidates (ten for the problems that also produce a k-sum) x GemmTuner.ROUNDS (3) trials (median): shapes that occur once per step need 30 steps to lock")
    ap.add_argument("--torch-profile", default=None, metavar="FILE",
                    help="diagnostics: after the timed region, one more step under torch.profiler; ATen / autograd operators by "
                         "device time (with input shapes) are written to FILE")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the legs below (forward-only latency, roofline, loss parity, CPU and eager "
                         "baselines, integration levels, rollout, other configurations; the rccl block at N > 1 or with --torch-ddp): "
                         "~90 s more at N = 1.  Without it those objects of the line are null")
    ap.add_argument("--no-fwd", action="store_true", help="skip the forward-only latency leg (counter passes: whole steps only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-eager-baseline", action="store_true",
                    help="skip the eager PyTorch-ROCm comparator (rank 0, N = 1 only; ~10 s after the timed region)")
    ap.add_argument("--no-loss-parity", action="store_true",
                    help="skip the loss cross-check (after the timed region: the loss of the HIP module, dropout off, against the "
                         "oracle restatement run in fp32 and in bf16 on this GPU with the same weights / batch / DiT noise; ~5 s)")
    ap.add_argument("--no-integration-levels", action="store_true",
                    help="skip the integration-levels leg (untouched reference loop / + HIP loss block / headline: N = 1 only, 5 steps each)")
    ap.add_argument("--no-rollout", action="store_true",
                    help="skip the closed-loop rollout leg (BASELINE configs[4]: 64 episodes in lock-step through the hipGraph-"
                         "captured engine, S = 10, DDIM-10; rank 0, N = 1 only; ~15 s after the timed region)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the other_configs leg (head sets E, D with the LIBERO flags, C at S = 10: 5 steps each after the timed "
                         "region; rank 0, N = 1 only; ~40 s)")
    ap.add_argument("--launch-selftest", action="store_true",
                    help="CPU-only check of the N > 1 launch path (self-spawn, rendezvous, max over ranks, JSON line); no model")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed (loss, loss terms, a fixed sample of the updated "
                         "parameters and of their gradients) as DIR/<name>.npy (rank 0).  Without --plan / $DVLA_GEMM_PLAN the newest "
                         "committed plan (profiles/rNN_gemm_plan.json) is replayed: the tuner's timing-dependent choices round differently "
                         "from run to run, and the training steps amplify that")
    ap.add_argument("--torch-ddp", action="store_true", help="use torch DDP instead of dreamvla_amd.ddp.GradBucketReducer")
    ap.add_argument("--torch-adamw", action="store_true",
                    help="clip_grad_norm_ + torch.optim.AdamW(fused) instead of dreamvla_amd.optim.FlatAdamW (HIP, flat buffers)")
    return ap


def main():
    ap = make_parser()
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: re-execute this very command under torch.distributed.run, one rank per
        # GPU of this node (train.py is started the same way: scripts/CALVIN_ABC_D/DreamVLA/finetune.sh:6-8 use torchrun)
        raise SystemExit(self_spawn(args.gpus))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.launch_selftest:
        return launch_selftest(rank, world, args)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback for the product path)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1 or args.torch_ddp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:               # --torch-ddp on one GPU: a one-rank RCCL group, what a 1-GPU `torchrun` job of train.py has
            os.environ.setdefault("MASTER_PORT", str(free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)

    from dreamvla_amd import losses, ops
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.dreamvla_model import DreamVLA
    from dreamvla_amd.synthetic import synthetic_batch

    torch.manual_seed(1234 + rank)
    np.random.seed(1234 + rank)      # the pretrain phase draws its per-step mask columns from numpy's global stream
    ops.set_seed_salt(rank)
    BF = torch.bfloat16
    S, B = args.seq, args.batch
    cfg = model_cfg(args.heads, S, args.layers, args.phase)
    model = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg).bfloat16()
    model.clip_model.requires_grad_(False)
    model.vision_encoder.requires_grad_(False)
    model = model.to(dev)
    model._init_model_type()
    model.train()
    if world > 1:  # identical initial weights on every rank (DDP's constructor broadcast)
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t.data, src=0)
    params = [p for p in model.parameters() if p.requires_grad]
    n_train = sum(p.numel() for p in params)
    reducer = None
    ddp_model = model
    if args.torch_ddp:               # train.py:173, at any world size (round-4 VERDICT: the flag used to be ignored at N = 1)
        ddp_model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local_rank], find_unused_parameters=True)
    else:
        reducer = GradBucketReducer(params, direct_grads=True)   # backward kernels write gradients into the bucket slots
    flat_opt = None
    if reducer is not None and not args.torch_adamw:
        from dreamvla_amd.optim import FlatAdamW
        flat_opt = FlatAdamW(reducer, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.1)   # finetune.sh:23,26 + clip 0.1
        opt = None
    else:
        # train.py:174 as written (no `fused=`); with --torch-adamw alone (our reducer, torch's optimizer) the fused kernel
        opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-4, **({} if args.torch_ddp else {"fused": True}))   # finetune.sh:23,26

    b = synthetic_batch(B, S, window=S + 3, seed=1234 + rank, heads=label_heads(args.heads))
    b["actions"][..., 6:] = (b["actions"][..., 6:] > 0.5).float()
    batch = {k: (v.to(dev, BF) if torch.is_floating_point(v) else v.to(dev)) for k, v in b.items()}
    lab = losses.label_actions(batch["actions"], S, 3)
    inputs = (batch["image_primary"][:, :S].contiguous(), batch["image_wrist"][:, :S].contiguous(),
              batch["state"][:, :S].contiguous(), batch["text_token"][:, :S].contiguous())

    def forward_loss():
        out = ddp_model(*inputs, action=batch["actions"][:, :S], action_label=lab, mode="train")
        return losses.calvin_losses(out, batch, sequence_length=S, use_dit_head=cfg["use_dit_head"], label_action=lab)

    def step():
        if reducer is not None:
            reducer.zero_grad()
        else:
            opt.zero_grad(set_to_none=False)
        total, parts = forward_loss()
        total.backward()
        if reducer is not None:
            reducer.finish()
        if flat_opt is not None:
            flat_opt.step()          # gradient norm + clip + AdamW, two HIP kernels per bucket
        else:
            torch.nn.utils.clip_grad_norm_(model.parameters() if args.torch_ddp else params, 0.1)   # utils/train_utils.py:600
            opt.step()
        return total, parts

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    from dreamvla_amd.ops import GemmTuner
    plan = args.plan or os.environ.get("DVLA_GEMM_PLAN")
    if not plan and args.dump_outputs:
        plan = committed_gemm_plan()
    if plan and os.path.exists(plan):
        GemmTuner.load_plan(plan)
    elif GemmTuner.enabled:
        for _ in range(args.tune_steps):
            step()
        sync()
    if args.save_plan and rank == 0:
        GemmTuner.save_plan(args.save_plan)
    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last, last_parts = step()
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    legs = extra_legs(args, rank, world)
    rccl = None
    if "rccl" in legs:
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)                                      # over the RCCL group: how many ranks the collective layer sees
        rccl = {"backend": dist.get_backend(), "ranks_seen_by_all_reduce": int(ones.item()), "world_size": world}
        if reducer is not None:
            rccl.update({"buckets": len(reducer.buckets), "bucket_MiB": [round(b["flat"].numel() * b["flat"].element_size() / 2**20, 1) for b in reducer.buckets],
                         "buckets_launched_during_backward_last_step": getattr(reducer, "last_early_launches", None),
                         "robust_gemm_schedule": bool(reducer.robust_gemm_schedule),
                         "robust_schedule_switches": getattr(reducer, "robust_switches", 0),
                         "robust_schedule_cost": {"whole_step_forced_ms": 6.55, "whole_step_forced_rel": 0.048,
                                                  "expected_at_n_gt_1_rel": 0.024, "under_16_cu_contention_rel": "+0 ... +4 % (default schedule: +53 ... +66 %)",
                                                  "source": "profiles/r06_gemm_cu_contention.txt (round-6 kernels and plan, 1 GPU, hog proxy)"},
                         "predicted_weak_scaling_efficiency_8gpu": "0.97-0.98 (DESIGN.md section 8)"})
    ms_per_step = dt / args.steps * 1e3
    value = B * world * args.steps / dt
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, last_parts, [(n, p) for n, p in model.named_parameters() if p.requires_grad],
                     reducer.grad_of if reducer is not None else (lambda p: p.grad))
    loss_val = require_finite_loss(float(last.detach()))

    if args.torch_profile and rank == 0:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            step()
            torch.cuda.synchronize()
        with open(args.torch_profile, "w") as fh:
            fh.write(prof.key_averages(group_by_input_shape=True).table(sort_by="self_cuda_time_total", row_limit=300,
                                                                         max_name_column_width=60, max_shapes_column_width=90))

    # forward-only latency (train mode, autograd graph recorded, no backward)
    fwd_ms = None
    if "fwd" in legs:
        for _ in range(1):
            forward_loss()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            forward_loss()
        torch.cuda.synchronize()
        fwd_ms = (time.perf_counter() - t1) / 3 * 1e3

    roofline = None
    if "roofline" in legs:
        prof = ops.GemmProfiler()
        with prof:
            step()
        torch.cuda.synchronize()
        r = prof.summary()          # every GEMM launch of the step is a hand-written kernel (no vendor library is linked)
        n_lib = sum(1 for sh in prof.shapes if sh[6] != "hip")
        if os.environ.get("DVLA_GEMM_BREAKDOWN"):
            with open(os.environ["DVLA_GEMM_BREAKDOWN"], "w") as f:
                json.dump(prof.breakdown(), f, indent=1)
        # HBM-side traffic of the GEMM dispatches cannot be collected from inside the process: it comes from separate
        # `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of this command (tests/pmc_traffic.sh), stored with the
        # commit they were measured on; a file from another tree is reported as stale, never presented as current
        traffic, traffic_src = None, None
        import glob
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))      # the newest round's passes
        pmc = cands[-1] if cands else ""
        if os.path.exists(pmc):
            with open(pmc) as f:
                t = json.load(f)
            traffic = t.get("gemm_bytes_per_launch")
            traffic_src = {"source": t.get("source"), "measured_on_commit": t.get("commit"),
                           "algorithmic_bytes_per_launch": t.get("algorithmic_bytes_per_launch")}
        roofline = {"bound": "mfma",
                    "kernel": "gemm_phase_kernel + gemm_ring_kernel + gemm_kernel (hand-written bf16 MFMA 32x32x16; every GEMM launch of one training step)",
                    "achieved": r["tflops"], "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": r["tflops"] / BF16_PEAK_TFLOPS,
                    "traffic": traffic, "traffic_source": traffic_src, "launches": r["launches"], "avg_launch_us": r["avg_us"],
                    "gflop_per_launch": r["gflop_per_launch"], "gemm_ms_per_step": r["total_ms"],
                    "whole_step_frac_of_bf16_peak": TRAIN_GFLOP_PER_SAMPLE[args.heads] * (B * 1e3 / ms_per_step) / 1e3 / BF16_PEAK_TFLOPS,
                    "library_gemm": {"launches": n_lib},
                    "tuner_wins_by_problem_key": GemmTuner.summary()}

    parity = None
    if "loss_parity" in legs:
        try:
            parity = loss_parity(model, cfg, batch, lab, inputs, S, B, dev)
        except Exception as e:  # noqa: BLE001
            parity = {"rel": None, "sample": f"failed: {e!r}"}

    cpu = None
    if "cpu_baseline" in legs:
        try:
            cpu = cpu_baseline(args.heads, S)
        except Exception as e:  # noqa: BLE001
            cpu = {"value": None, "unit": "samples/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {e!r}"}

    eager = None
    grad_exchange = "torch DDP" if reducer is None else "GradBucketReducer (flat bf16 buckets, async all-reduce)"
    optimizer_name = ("FlatAdamW (HIP: dvla_sumsq_bf16 + dvla_adamw_bf16 on flat buffers)" if flat_opt is not None
                      else "clip_grad_norm_ + torch.optim.AdamW (train.py:174 as written: no fused=)" if args.torch_ddp
                      else "clip_grad_norm_ + torch.optim.AdamW(fused=True)")
    if "eager_baseline" in legs:
        try:
            model = ddp_model = reducer = flat_opt = opt = params = None
            torch.cuda.empty_cache()
            eager = eager_rocm_baseline(args.heads, S, B)
            eager["ours_over_eager"] = value / eager["value"]
        except Exception as e:  # noqa: BLE001
            eager = {"value": None, "unit": "samples/s", "sample": f"failed: {e!r}"}

    levels = None
    if "integration_levels" in legs:
        try:
            model = ddp_model = reducer = flat_opt = opt = params = None      # (the timed objects: loss_parity above was their last user)
            torch.cuda.empty_cache()
            levels = integration_levels(args, cfg, S, B, dev, value)
        except Exception as e:  # noqa: BLE001
            levels = {"failed": repr(e)}
        torch.cuda.empty_cache()

    rollout = None
    if "rollout" in legs:
        try:
            from tests import gpu_rollout_bench
            torch.cuda.empty_cache()
            r = gpu_rollout_bench.run(Bs=(64, 1), naive=False, eager_engine=False, steps=12)
            rows = {row["B"]: row for row in r["rows"]}
            rollout = {"metric": "closed-loop control steps/s (BASELINE configs[4]: eval rollout, 64 episodes in lock-step, S = 10 "
                                 "history, DiT head with DDIM-10 + CFG, hipGraph-captured encode / decode, per-frame token cache; "
                                 "the sampler runs on the window position the wrapper executes -- RolloutEngine(sample='newest') -- "
                                 "and, at one episode, as one persistent kernel on one XCD)",
                       "value": rows[64]["episode_steps_per_s"]["graph"], "unit": "episode-steps/s", "episodes": 64,
                       "ms_per_lockstep": rows[64]["graph_ms_per_step"], "single_episode_ms_per_step": rows[1]["graph_ms_per_step"],
                       "dtype": "bf16", "data": "synthetic"}
        except Exception as e:  # noqa: BLE001
            rollout = {"value": None, "sample": f"failed: {e!r}"}

    others = None
    if "other_configs" in legs:
        others = {}
        for (name, heads_o, S_o, B_o, accum, extra_cfg, loss_kw, batch_kw) in OTHER_CONFIGS:
            try:
                torch.cuda.empty_cache()
                others[name] = other_config(name, heads_o, S_o, B_o, accum, extra_cfg, loss_kw, batch_kw, dev)
            except Exception as e:  # noqa: BLE001
                others[name] = {"samples_per_s": None, "failed": repr(e)}

    if rank == 0:
        line = {
            "metric": "train samples/sec (CALVIN ABC->D, seq_len=7)", "value": value, "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "fwd_ms_per_step": fwd_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic", "gemm_plan": os.path.relpath(plan, ROOT) if plan and os.path.exists(plan) else None,
            "full": args.full,
            "config": {"workload": f"DreamVLA CALVIN {args.phase} step, head set {args.heads} "
                                   f"({'+'.join(k for k in HEAD_SETS[args.heads] if HEAD_SETS[args.heads][k])}), "
                                   f"B={B}/GPU, S={S}, window {S + 3}, 2x224^2 views, 77 text tokens, hidden 1024 / "
                                   f"{args.layers} layers / 16 heads, dropout 0.1 on, AdamW + clip 0.1",
                       "global_batch": B * world, "seq_len": S, "parallelism": f"dp{world}",
                       "trainable_params_M": n_train / 1e6, "loss": loss_val,
                       "grad_exchange": grad_exchange, "optimizer": optimizer_name},
            "roofline": roofline, "loss_parity": parity, "cpu_baseline": cpu, "eager_rocm_baseline": eager, "rollout": rollout,
            "other_configs": others, "rccl": rccl, "integration_levels": levels,
        }
    if world > 1 or args.torch_ddp:
        # RCCL prints its version banner through C stdio when the group goes away: tear the group down and flush C's buffers FIRST,
        # so that the JSON line is the LAST line of stdout
        dist.barrier()
        dist.destroy_process_group()
        import ctypes
        ctypes.CDLL(None).fflush(None)
    if rank == 0:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
