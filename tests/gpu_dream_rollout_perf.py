"""What a dream costs at evaluation (a measurement script, not a test): the control step of dreamvla_amd.rollout.RolloutEngine with
and without dreams, with the protocol of tests/gpu_rollout_bench.py (S = 10, 24 layers, head set C, DiT head, hipGraph, warm), and the
render kernel alone against the input-pipeline kernel.  One JSON line per measurement on stdout and, appended, in the file named
by --out=PATH when given (the recorded run is kept as profiles/r08_dream_rollout_perf.jsonl).

    python tests/gpu_dream_rollout_perf.py [--no-dreams-only] [--out=PATH] [B ...]

--no-dreams-only: leg (a) alone -- it runs on a commit without the feature too, for the same-session A/B of the plain step."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), None)
REPEATS = 3


def emit(row):
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def step_ms(m, S, B, steps, **kw):
    """REPEATS timings of `steps` warm control steps of one engine (graphs captured), ms per step each"""
    from dreamvla_amd.rollout import RolloutEngine
    BF, dev = torch.bfloat16, "cuda"
    g = torch.Generator().manual_seed(B)
    frames = [(torch.randn(B, 3, 224, 224, generator=g).to(dev, BF), torch.randn(B, 3, 224, 224, generator=g).to(dev, BF),
               torch.cat([torch.rand(B, 6, generator=g), torch.ones(B, 1)], -1).to(dev, BF)) for _ in range(4)]
    text = torch.randint(1, 49000, (B, 77), generator=g).to(dev)
    eng = RolloutEngine(m, B, use_graph=True, warmup_decodes=6, **kw)
    for i in range(S + 8):
        eng.step(*frames[i % 4], text)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for i in range(steps):
            eng.step(*frames[i % 4], text)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    assert eng.graphs_captured
    return times


def kernel_rate(fn, nbytes, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    return us, nbytes / (us * 1e-6) / 1e9


def main():
    from tests.gpu_rollout_bench import build_model
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plain_only = "--no-dreams-only" in sys.argv
    Bs = [int(a) for a in args] or [1, 64]
    m, S = build_model()
    legs = [("a_no_dreams", {})]
    if not plain_only:
        every = m.dream_names()
        legs += [("b_image_depth_newest", dict(dreams=("image", "depth"))), ("b_all_heads_newest", dict(dreams=every)),
                 ("c_image_depth_all", dict(dreams=("image", "depth"), sample="all")), ("c_all_heads_all", dict(dreams=every, sample="all"))]
    base = {}
    for B in Bs:
        steps = 100 if B == 1 else 20
        for leg, kw in legs:
            t = step_ms(m, S, B, steps, **kw)
            row = {"leg": leg, "B": B, "steps": steps, "ms_per_step": t, "median_ms": sorted(t)[len(t) // 2], "spread_ms": max(t) - min(t), **{k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}}
            if leg == "a_no_dreams":
                base[B] = row["median_ms"]
            else:
                row["price_of_a_dream_ms"] = row["median_ms"] - base[B]
            emit(row)
    if plain_only:
        return
    # (d) the render kernel alone, next to the input-pipeline kernel (the yardstick: the same frames the other way round)
    from dreamvla_amd import ops
    from dreamvla_amd.preprocess import preprocess_frames
    g = torch.Generator().manual_seed(3)
    for n in (2, 128):
        pred = torch.randn(n, 196, 768, generator=g).to(torch.bfloat16).to("cuda")
        cur = torch.randn(n, 3, 224, 224, generator=g).to(torch.bfloat16).to("cuda")
        u8 = torch.randint(0, 256, (n, 224, 224, 3), generator=g, dtype=torch.uint8).to("cuda")
        px = n * 224 * 224 * 3
        us, gbs = kernel_rate(lambda: ops.dream_render(pred, "image", cur), px * (2 + 2 + 1))
        us_p, gbs_p = kernel_rate(lambda: preprocess_frames(u8), px * (1 + 2))
        emit({"leg": "d_render_kernel", "n": n, "render_us": us, "render_GBps": gbs, "algorithmic_bytes": px * 5,
              "input_pipeline_us": us_p, "input_pipeline_GBps": gbs_p, "note": "host-enqueued launches incl. the output allocation; device events"})


if __name__ == "__main__":
    main()
