"""What taking raw camera frames costs (a measurement script, not a test): CLIP's bicubic Resize + CenterCrop as the HIP kernel
(dreamvla_amd.preprocess.resize_frames_u8) against the same frames through Pillow (`clip_image_resize_u8`) on this box's host, and
the control step of RolloutEngine from raw host frames (`step_raw`) against Pillow + `step`.  One JSON line per measurement on
stdout and, appended, in the file named by --out=PATH (the recorded run is kept as profiles/r10_resize_perf.jsonl).

    python tests/gpu_resize_perf.py [--out=PATH] [--no-engine]

Frames: CALVIN's two cameras, 200 x 200 (static) and 84 x 84 (gripper), half of the frames each -- 128 frames = 64 episodes x 2
cameras of one control step, 832 = one training batch (B 32, window 13, 2 cameras).
  host     Pillow, one thread (ms per frame per size) and a 16-thread pool (Pillow releases the GIL inside the resample)
  kernel   device events around ITERS back-to-back calls of resize_frames_u8 (one launch per camera; the output allocation and the
           launch are host work inside the window -- the queue stays ahead of the device, see `host_enqueue_us`), after warm-up;
           achieved bytes/s over the algorithmic traffic (source + output bytes)
  step     warm control steps (graphs captured) from raw HOST frames, host clock around work that ends in a synchronise, the two
           legs alternating in one process: `step_raw` (upload raw, resize + normalise on the device) and `pillow_step` (Pillow
           per frame, upload 224 x 224 frames, preprocess_frames, `step`: what a caller did before `step_raw`)"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), None)
CAMERAS = ((200, 200), (84, 84))
REPEATS = 3


def emit(row):
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def host_ms(frames_by_cam, threads):
    """wall time of Pillow over all frames, best of REPEATS"""
    from dreamvla_amd.preprocess import clip_image_resize_u8
    flat = [f for a in frames_by_cam for f in a]
    best = float("inf")
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            if threads == 1:
                for f in flat:
                    clip_image_resize_u8(f)
            else:
                list(ex.map(clip_image_resize_u8, flat, chunksize=max(1, len(flat) // (4 * threads))))
            best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def kernel_us(dev_by_cam, iters):
    from dreamvla_amd.preprocess import resize_frames_u8
    run = lambda: [resize_frames_u8(d) for d in dev_by_cam]
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters * 1e3)
    t0 = time.perf_counter()                     # the host's share: enqueue only, nothing waited for
    for _ in range(iters):
        run()
    enqueue = (time.perf_counter() - t0) / iters * 1e6
    torch.cuda.synchronize()
    return times, enqueue


def kernel_legs():
    from tests.resize_cases import frames, pillow
    from dreamvla_amd.preprocess import resize_frames_u8
    for total in (128, 832):
        per_cam = total // len(CAMERAS)
        host = [frames(h, w, "noise", per_cam, seed=total) for h, w in CAMERAS]
        dev = [torch.from_numpy(a).cuda() for a in host]
        same = all(bool((resize_frames_u8(d).cpu() == torch.from_numpy(pillow(a))).all()) for d, a in zip(dev, host))
        h1, h16 = host_ms(host, 1), host_ms(host, 16)
        t, enqueue = kernel_us(dev, 200 if total == 128 else 50)
        med = sorted(t)[len(t) // 2]
        nbytes = sum(a.size for a in host) + total * 224 * 224 * 3
        emit({"leg": "kernel", "frames": total, "cameras": [list(c) for c in CAMERAS], "kernel_us": t, "median_us": med, "spread_us": max(t) - min(t),
              "host_enqueue_us": enqueue, "algorithmic_bytes": nbytes, "achieved_GBps": nbytes / (med * 1e-6) / 1e9,
              "pillow_1_thread_ms": h1, "pillow_16_threads_ms": h16, "speedup_vs_1_thread": h1 * 1e3 / med, "speedup_vs_16_threads": h16 * 1e3 / med,
              "bytes_equal_pillow": same, "faster_than_host": bool(med < h16 * 1e3 and med < h1 * 1e3)})
    for h, w in CAMERAS:                          # Pillow per frame on this host, one thread
        a = frames(h, w, "noise", 64)
        emit({"leg": "host_per_frame", "size": [h, w], "pillow_1_thread_ms_per_frame": host_ms([a], 1) / 64})


def step_legs(m, S, B, steps):
    from dreamvla_amd import preprocess as P
    from dreamvla_amd.rollout import RolloutEngine
    from tests.resize_cases import frames
    g = torch.Generator().manual_seed(B)
    raw = [(frames(200, 200, "noise", B, seed=i), frames(84, 84, "noise", B, seed=i)) for i in range(4)]
    state = torch.cat([torch.rand(B, 6, generator=g), torch.ones(B, 1)], -1).to("cuda", torch.bfloat16)
    text = torch.randint(1, 49000, (B, 77), generator=g).to("cuda")
    eng = RolloutEngine(m, B, use_graph=True, warmup_decodes=6)

    def step_raw(i):
        return eng.step_raw(raw[i % 4][0], raw[i % 4][1], state, text)

    def pillow_step(i):
        u8 = np.stack([np.stack([P.clip_image_resize_u8(f) for f in cam]) for cam in raw[i % 4]], axis=1)      # (B, 2, 224, 224, 3)
        x = P.preprocess_frames(torch.from_numpy(u8).pin_memory().to("cuda", non_blocking=True))
        return eng.step(x[:, 0], x[:, 1], state, text)

    for i in range(S + 8):
        step_raw(i)
    pillow_step(0)
    torch.cuda.synchronize()
    assert eng.graphs_captured
    times = {"step_raw": [], "pillow_step": []}
    for _ in range(REPEATS):
        for name, fn in (("step_raw", step_raw), ("pillow_step", pillow_step)):
            t0 = time.perf_counter()
            for i in range(steps):
                fn(i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    emit({"leg": "control_step_from_raw_host_frames", "B": B, "steps": steps, "ms_per_step": times, "median_ms": med,
          "spread_ms": {k: max(v) - min(v) for k, v in times.items()}, "episode_steps_per_s": {k: B / (v * 1e-3) for k, v in med.items()},
          "step_raw_not_slower": bool(med["step_raw"] <= med["pillow_step"])})


def main():
    assert torch.cuda.is_available(), "a measurement on the GPU: no fallback"
    kernel_legs()
    if "--no-engine" in sys.argv:
        return
    from tests.gpu_rollout_bench import build_model
    m, S = build_model()
    for B, steps in ((64, 10), (1, 50)):
        step_legs(m, S, B, steps)


if __name__ == "__main__":
    main()
