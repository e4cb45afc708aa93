"""What the dream pictures cost (a measurement script, not a test), in the style of tests/gpu_dream_score_perf.py.  One JSON line
per measurement on stdout and, appended, in the file named by --out=PATH (the recorded run is profiles/r26_dream_views_perf.jsonl).

    python tests/gpu_dream_views_perf.py [--out=PATH] [--parity=PATH] [--no-steps] [--no-kernels] [B ...]

(a) every kernel alone at 128 and 832 frames (64 and 416 episodes x 2 views) of the shapes the model produces -- depth 224 x 224,
    trajectory 196 x 8 -> 28 x 28 flow -> 224 x 224, DINO 256 x 768 and SAM 256 x 256 -> 224 x 224: time per call, the algorithmic
    bytes per second (operands read once, the picture written once), and an eager PyTorch-ROCm restatement of the same picture on
    the same data in the same run.  Each figure is the median of BATCHES timed batches of ITERS calls between device events,
    after a warm-up batch; a batch runs for tens of milliseconds, so clocks have settled.
(b) the control step of RolloutEngine(dreams=(depth, traj, dino, sam)) with all four views on against off, same model, at B
    episodes (default 1 and 64), alternating legs, each arm REPEATS = 2 times.
--parity=PATH: the figures of every case of tests/test_dream_views_gpu.py (the recorded run is profiles/r26_parity_dream_views.jsonl)."""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), None)
PARITY = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parity=")), None)
BATCHES, REPEATS = 7, 2
BF = torch.bfloat16


def emit(row, path=OUT):
    print(json.dumps(row), flush=True)
    if path is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(row) + "\n")


def median_us(fn, iters):
    """median and spread over BATCHES batches of `iters` calls (device events), after one untimed batch"""
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(BATCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    us.sort()
    return us[len(us) // 2], us[-1] - us[0]


# ---- eager PyTorch restatements of the same pictures (fp32 on the device; not bit-exact twins, the same picture) ----
def _levels(v, lo, hi):
    return ((v - lo) / (hi - lo)).clamp(0, 1).mul(255).round().long()


def eager_depth(d, pal):
    fin = torch.isfinite(d)
    flat = torch.where(fin, d, torch.zeros_like(d)).flatten(1)
    masked_lo = torch.where(fin.flatten(1), flat, torch.full_like(flat, float("inf"))).amin(dim=1).view(-1, 1, 1)
    masked_hi = torch.where(fin.flatten(1), flat, torch.full_like(flat, float("-inf"))).amax(dim=1).view(-1, 1, 1)
    out = pal[_levels(torch.where(fin, d, masked_lo), masked_lo, masked_hi)]
    return torch.where(fin.unsqueeze(-1), out, torch.zeros_like(out))


def eager_unshuffle(pred):
    n, L, D = pred.shape
    g = int(L ** 0.5)
    return F.pixel_shuffle(pred.view(n, g, g, D).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).float().contiguous()


def eager_wheel(flow, size):
    idx = (torch.arange(size, device=flow.device) * flow.shape[1]) // size
    fl = flow[:, idx][:, :, idx]
    dx, dy = fl[..., 0], fl[..., 1]
    ang = torch.rad2deg(torch.atan2(dy, dx))
    ang = torch.where(ang < 0, ang + 360, ang)
    Hh = (ang / 2).long().clamp(max=179)
    V = (32 * torch.sqrt(dx * dx + dy * dy)).clamp(0, 255).long()
    X = (V * (30 - (Hh % 60 - 30).abs()) + 15) // 30
    s, Z = Hh // 30, torch.zeros_like(V)
    r = torch.where((s == 0) | (s == 5), V, torch.where((s == 1) | (s == 4), X, Z))
    g = torch.where((s == 1) | (s == 2), V, torch.where((s == 0) | (s == 3), X, Z))
    b = torch.where((s == 3) | (s == 4), V, torch.where((s == 2) | (s == 5), X, Z))
    return torch.stack((r, g, b), dim=-1).to(torch.uint8)


def eager_mask(pred, thr, dilate):
    n, L, D = pred.shape
    g = int(L ** 0.5)
    m = pred.float().view(n, g, g, 2, D // 2).mean(dim=-1)
    mask = ((m * m).sum(dim=-1) > thr * thr).float().unsqueeze(1)
    if dilate:
        mask = F.max_pool2d(mask, 3, 1, 1)
    return mask[:, 0] > 0


def eager_overlay(mask, cur, tint, alpha):
    from dreamvla_amd.preprocess import CLIP_MEAN, CLIP_STD
    mean = torch.tensor(CLIP_MEAN, device=cur.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, device=cur.device).view(1, 3, 1, 1)
    v = (cur.float() * std + mean).clamp(0, 1).mul(255).round().permute(0, 2, 3, 1).to(torch.int32)
    cell = cur.shape[-1] // mask.shape[-1]
    big = mask.repeat_interleave(cell, dim=1).repeat_interleave(cell, dim=2).unsqueeze(-1)
    mixed = (v * (256 - alpha) + torch.tensor(tint, device=cur.device, dtype=torch.int32) * alpha + 128) >> 8
    return torch.where(big, mixed, v).to(torch.uint8)


def eager_feature(x, pal, size):
    n, L, D = x.shape
    g = int(L ** 0.5)
    b, lo, hi = (torch.tensor(t, device=x.device) for t in (pal.b, pal.lo32, pal.hi32))
    lv = _levels(x.float() @ pal.W + b, lo, hi).to(torch.uint8).view(n, g, g, 3)
    idx = (torch.arange(size, device=x.device) * g) // size
    return lv[:, idx][:, :, idx]


def kernels():
    from dreamvla_amd import ops
    from dreamvla_amd.dream_view import FeaturePalette, depth_palette
    gen = torch.Generator().manual_seed(20)
    pal = depth_palette("cuda")
    pal_d = FeaturePalette.fit(torch.randn(2000, 768, generator=gen, dtype=torch.float64)).to("cuda")
    pal_s = FeaturePalette.fit(torch.randn(2000, 256, generator=gen, dtype=torch.float64)).to("cuda")
    for n in (128, 832):
        iters = 1000 if n == 128 else 200                 # a timed batch of a 20 .. 150 us kernel runs for 20 .. 150 ms, eight batches per leg
        depth = (torch.rand(n, 224, 224, generator=gen) * 5).cuda()
        pred = (torch.randn(n, 196, 8, generator=gen) * 1.5).to(BF).cuda()
        flow = ops.flow_unshuffle(pred)
        mask = ops.motion_mask(pred, 1.0, True)
        cur = torch.randn(n, 3, 224, 224, generator=gen).to(BF).cuda()
        dino = torch.randn(n, 256, 768, generator=gen).to(BF).cuda()
        sam = torch.randn(n, 256, 256, generator=gen).to(BF).cuda()
        pic = n * 224 * 224 * 3
        legs = [
            ("depth_colorize own range", lambda: ops.depth_colorize(depth), lambda: eager_depth(depth, pal), 2 * depth.numel() * 4 + pic),
            ("depth_colorize fixed range", lambda: ops.depth_colorize(depth, 0.0, 5.0), None, depth.numel() * 4 + pic),
            ("flow_unshuffle", lambda: ops.flow_unshuffle(pred), lambda: eager_unshuffle(pred), pred.numel() * 2 + flow.numel() * 4),
            ("flow_wheel 28->224", lambda: ops.flow_wheel(flow, 224), lambda: eager_wheel(flow, 224), flow.numel() * 4 + pic),
            ("motion_mask dilated", lambda: ops.motion_mask(pred, 1.0, True), lambda: eager_mask(pred, 1.0, True), pred.numel() * 2 + n * 196),
            ("motion_overlay", lambda: ops.motion_overlay(mask, cur), lambda: eager_overlay(mask, cur, (255, 64, 0), 96),
             cur.numel() * 2 + n * 196 + pic),
            ("feature_render dino 256x768", lambda: ops.feature_render(dino, pal_d, 224), lambda: eager_feature(dino, pal_d, 224),
             dino.numel() * 2 + pic),
            ("feature_render sam 256x256", lambda: ops.feature_render(sam, pal_s, 224), lambda: eager_feature(sam, pal_s, 224),
             sam.numel() * 2 + pic),
        ]
        for name, fn, eager, nbytes in legs:
            us, spread = median_us(fn, iters)
            row = {"leg": "a_" + name, "n": n, "us": us, "spread_us": spread, "algorithmic_bytes": nbytes, "GBps": nbytes / us / 1e3,
                   "iters": iters, "batches": BATCHES, "note": "host-enqueued, output allocation included; device events"}
            if eager is not None:
                us_e, spread_e = median_us(eager, max(iters // 4, 10))
                row.update({"eager_torch_us": us_e, "eager_spread_us": spread_e, "eager_over_kernel": us_e / us})
            emit(row)


def build_model():
    """the evaluation model of tests/gpu_rollout_bench.py with the four heads that have a view: depth, trajectory, DINO, SAM"""
    from dreamvla_amd.dreamvla_model import DreamVLA
    S = 10
    cfg = dict(finetune_type="calvin", sequence_length=S, num_resampler_query=16, num_obs_token_per_image=9, action_pred_steps=3,
               transformer_layers=24, hidden_dim=1024, transformer_heads=16, phase="finetune", obs_pred=True, depth_pred=True,
               sam_feat_pred=True, dino_feat_pred=True, trajectory_pred=True, use_dit_head=True, attn_implementation="sdpa")
    torch.manual_seed(0)
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg).bfloat16().to("cuda")
    m._init_model_type()
    m.eval()
    return m, S


def step_legs(m, S, B, steps):
    from dreamvla_amd.dream_view import FeaturePalette
    from dreamvla_amd.rollout import RolloutEngine
    g = torch.Generator().manual_seed(B)
    frames = [(torch.randn(B, 3, 224, 224, generator=g).to("cuda", BF), torch.randn(B, 3, 224, 224, generator=g).to("cuda", BF),
               torch.cat([torch.rand(B, 6, generator=g), torch.ones(B, 1)], -1).to("cuda", BF)) for _ in range(4)]
    text = torch.randint(1, 49000, (B, 77), generator=g).to("cuda")
    dreams = ("depth", "traj", "dino", "sam")
    views = dict(depth=True, traj=True, dino=FeaturePalette.fit(torch.randn(1000, 768, generator=g, dtype=torch.float64)),
                 sam=FeaturePalette.fit(torch.randn(1000, 256, generator=g, dtype=torch.float64)))
    engines = {"views_off": RolloutEngine(m, B, use_graph=True, warmup_decodes=6, dreams=dreams),
               "views_on": RolloutEngine(m, B, use_graph=True, warmup_decodes=6, dreams=dreams, dream_views=views)}
    for eng in engines.values():
        for i in range(S + 8):
            eng.step(*frames[i % 4], text)
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(REPEATS):
        for name, eng in engines.items():
            t0 = time.perf_counter()
            for i in range(steps):
                eng.step(*frames[i % 4], text)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    assert all(e.graphs_captured for e in engines.values())
    return times


def parity():
    from tests import test_dream_views_gpu as T
    for shape in ((3, 5, 7), (5, 224, 224)):
        for rng_kind in ("own", "fixed"):
            for pal_kind in ("default", "random"):
                emit({"kernel": "depth_colorize", "case": f"{shape} range={rng_kind} palette={pal_kind}",
                      "bytes_differing_from_float32_restatement": T.depth_mismatch(shape, rng_kind, pal_kind)[0]}, PARITY)
    for size in (224, 30):
        share, outside, inside = T.wheel_stats(size)
        emit({"kernel": "flow_wheel", "case": f"N(0, 2 px) 4 x 28 x 28 -> {size}", "share_of_pixels_in_band": share, "band_cap": 0.01,
              "pixels_differing_outside_band": outside, "pixels_differing_inside_band": inside}, PARITY)
    for g in (14, 28):
        worst, outside, total = T.overlay_stats(g)
        emit({"kernel": "motion_overlay", "case": f"N(0, 1.5) frames, grid {g}", "max_level_difference_vs_float64": worst,
              "bytes_differing_away_from_ties": outside, "bytes_differing": total}, PARITY)
    worst_share = 0.0
    for D in (8, 256, 768, 776):
        for values in ("normal", "one channel 100 x", "saturating"):
            for tokens in (4, 256):
                for n in (1, 5):
                    for size in (224, 30):
                        worst, outside, share = T.feature_stats(D, values, tokens, n, size)
                        worst_share = max(worst_share, share)
                        emit({"kernel": "feature_render", "case": f"D={D} {values} tokens={tokens} n={n} size={size}",
                              "max_level_difference_vs_float64": worst, "bytes_differing_outside_band": outside,
                              "share_of_bytes_differing": share}, PARITY)
    emit({"summary": True, "feature_render_largest_share_of_bytes_differing": worst_share}, PARITY)


def main():
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if PARITY:
        parity()
    if "--no-kernels" not in sys.argv:
        kernels()
    if "--no-steps" in sys.argv:
        return
    Bs = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [1, 64]
    m, S = build_model()
    for B in Bs:
        steps = 100 if B == 1 else 20
        t = step_legs(m, S, B, steps)
        med = {k: sum(v) / len(v) for k, v in t.items()}
        emit({"leg": "b_control_step", "B": B, "steps": steps, "ms_per_step": t, "mean_ms": med,
              "price_of_views_ms": med["views_on"] - med["views_off"], "spread_ms": {k: max(v) - min(v) for k, v in t.items()}})


if __name__ == "__main__":
    main()
