"""What scoring a dream costs (a measurement script, not a test), in the style of tests/gpu_dream_rollout_perf.py.  One JSON line per
measurement on stdout and, appended, in the file named by --out=PATH (the recorded run is profiles/r12_dream_score_perf.jsonl).

    python tests/gpu_dream_score_perf.py [--out=PATH] [--parity=PATH] [--no-steps] [B ...]

(a) the two metric kernels alone at 128 and 832 frames of 224 x 224 (64 and 416 episodes x 2 views): time per call and the
    algorithmic bytes per second (both operands read once; the outputs are a few bytes per frame).  Each figure is the median of
    BATCHES timed batches of ITERS calls between device events, after a warm-up that runs as long as one batch.
(b) the same SSIM in eager PyTorch-ROCm -- five grouped conv2d with the 11 x 11 Gaussian over float32 copies of the frames -- on the
    same data in the same run, and how far it is from the kernel's result.
(c) the control step of RolloutEngine(dreams=("image",)) at B episodes (default 1 and 64) with and without score_dreams, same
    model, alternating legs, protocol of tests/gpu_dream_rollout_perf.py.
--parity=PATH: the deviation of every case of tests/test_dream_score_gpu.py from the float64 restatement, and the largest one: the
    numbers that test's bounds are 4 x of (the recorded run is profiles/r12_parity_dream_score.jsonl)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), None)
PARITY = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parity=")), None)
BATCHES, REPEATS = 7, 3


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


def eager_ssim(a_u8, b_u8):
    """mean SSIM per frame in eager PyTorch: (n, h, w, 3) uint8 x 2 -> (n,) float32"""
    import torch.nn.functional as F
    from tests.dream_score_ref import C1, C2, gaussian_window
    w1 = torch.from_numpy(gaussian_window()).to(a_u8.device, torch.float32)
    k = torch.outer(w1, w1).expand(3, 1, 11, 11).contiguous()
    x = a_u8.permute(0, 3, 1, 2).float() - 128.0
    y = b_u8.permute(0, 3, 1, 2).float() - 128.0
    mx, my = F.conv2d(x, k, groups=3), F.conv2d(y, k, groups=3)
    vx = F.conv2d(x * x, k, groups=3) - mx * mx
    vy = F.conv2d(y * y, k, groups=3) - my * my
    vxy = F.conv2d(x * y, k, groups=3) - mx * my
    ux, uy = mx + 128.0, my + 128.0
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return s.mean(dim=(1, 2, 3))


def kernels():
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(12)
    for n in (128, 832):
        a = torch.randint(0, 256, (n, 224, 224, 3), generator=g, dtype=torch.uint8).cuda()
        b = (a.int() + torch.randint(-40, 41, a.shape, generator=g).cuda()).clamp(0, 255).to(torch.uint8)
        iters = 400 if n == 128 else 80
        nbytes = 2 * a.numel()
        us, spread = median_us(lambda: ops.image_quality(a, b), iters)
        row = {"leg": "a_image_quality", "n": n, "us": us, "spread_us": spread, "algorithmic_bytes": nbytes, "GBps": nbytes / us / 1e3,
               "iters": iters, "batches": BATCHES, "note": "host-enqueued, two launches + output and workspace allocation; device events"}
        us_e, spread_e = median_us(lambda: eager_ssim(a, b), max(iters // 8, 10))
        got, ref = ops.image_quality(a, b)["ssim"], eager_ssim(a, b)
        row.update({"eager_torch_ssim_us": us_e, "eager_spread_us": spread_e, "eager_over_kernel": us_e / us,
                    "max_abs_ssim_kernel_vs_eager": float((got - ref).abs().max()),
                    "eager_note": "SSIM only (no SSE / PSNR): 5 grouped conv2d on float32 NCHW copies + the map, ~25 launches"})
        emit(row)
        p = torch.rand(n, 224, 224, generator=g).cuda() * 5
        t = torch.rand(n, 224, 224, generator=g).cuda() * 5
        t[:, :20] = 0
        nbytes = 2 * 4 * p.numel()
        us, spread = median_us(lambda: ops.depth_quality(p, t), iters)
        emit({"leg": "a_depth_quality", "n": n, "us": us, "spread_us": spread, "algorithmic_bytes": nbytes, "GBps": nbytes / us / 1e3,
              "iters": iters, "batches": BATCHES})


def step_legs(m, S, B, steps):
    """REPEATS alternating timings of `steps` warm control steps of two engines on one model: ms per step"""
    from dreamvla_amd.rollout import RolloutEngine
    BF, dev = torch.bfloat16, "cuda"
    g = torch.Generator().manual_seed(B)
    frames = [(torch.randn(B, 3, 224, 224, generator=g).to(dev, BF), torch.randn(B, 3, 224, 224, generator=g).to(dev, BF),
               torch.cat([torch.rand(B, 6, generator=g), torch.ones(B, 1)], -1).to(dev, BF)) for _ in range(4)]
    u8 = [torch.randint(0, 256, (B, 2, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(4)]
    text = torch.randint(1, 49000, (B, 77), generator=g).to(dev)
    engines = {"dreams_image": RolloutEngine(m, B, use_graph=True, warmup_decodes=6, dreams=("image",)),
               "dreams_image_scored": RolloutEngine(m, B, use_graph=True, warmup_decodes=6, dreams=("image",), score_dreams=True)}
    kw = {"dreams_image": lambda i: {}, "dreams_image_scored": lambda i: {"frames_u8": u8[i % 4]}}
    for name, eng in engines.items():
        for i in range(S + 8):
            eng.step(*frames[i % 4], text, **kw[name](i))
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(REPEATS):
        for name, eng in engines.items():
            t0 = time.perf_counter()
            for i in range(steps):
                eng.step(*frames[i % 4], text, **kw[name](i))
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    assert all(e.graphs_captured for e in engines.values())
    return times


def parity():
    from tests import test_dream_score_gpu as T
    worst_s = worst_d = 0.0
    for i, c in enumerate(T.image_cases()):
        dev, _ = T.image_deviation(i)
        worst_s = max(worst_s, dev)
        emit({"kernel": "image_quality", "case": c[0], "max_abs_ssim_vs_float64": dev}, PARITY)
    for i, c in enumerate(T.depth_cases()):
        dev, _ = T.depth_deviation(i)
        worst_d = max(worst_d, dev)
        emit({"kernel": "depth_quality", "case": c[0], "max_rel_vs_float64": dev}, PARITY)
    emit({"summary": True, "ssim_max_abs": worst_s, "ssim_test_bound": 4 * worst_s, "ssim_cap": 1e-3,
          "depth_max_rel": worst_d, "depth_test_bound": 4 * worst_d, "depth_cap": 1e-4}, PARITY)


def main():
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if PARITY:
        parity()
    kernels()
    if "--no-steps" in sys.argv:
        return
    from tests.gpu_rollout_bench import build_model
    Bs = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [1, 64]
    m, S = build_model()
    for B in Bs:
        steps = 100 if B == 1 else 20
        t = step_legs(m, S, B, steps)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        emit({"leg": "c_control_step", "B": B, "steps": steps, "ms_per_step": t, "median_ms": med,
              "price_of_scoring_ms": med["dreams_image_scored"] - med["dreams_image"],
              "spread_ms": {k: max(v) - min(v) for k, v in t.items()}})


if __name__ == "__main__":
    main()
