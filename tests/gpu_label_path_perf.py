"""What building the labels on the device costs (a measurement script, not a test): DeviceCollator(device_labels=True) against the
default collator followed by the training loop's `.to(device, bf16)` on its label entries, and the depth kernel alone.  One JSON line
per measurement on stdout and, appended, in the file named by --out=PATH (the recorded run is kept as
profiles/r11_label_path_perf.jsonl).

    python tests/gpu_label_path_perf.py [--out=PATH] [--parent-collate=PATH]

Batch: the benchmark's -- B 32, window 13, CALVIN's cameras (200 x 200 static, 84 x 84 gripper), depth maps of the same sizes, DINO
(256 x 768) and SAM (256 x 256) features per frame and camera, fp32 as the dataset hands them over.  Both legs resize the camera
frames on the device (device_resize=True): the cameras are common to both and Pillow on 832 frames would bury the labels.
  labels   (a) host clock from the collator call until every label is resident on the device in bf16, ended by a synchronise:
           `default` = DeviceCollator() + `.to("cuda", torch.bfloat16, non_blocking=True)` on entries 6 .. 11, `device` =
           DeviceCollator(device_labels=True) alone.  The legs alternate in one process, REPEATS timings each after a warm-up pass.
           --parent-collate=PATH adds a third alternating leg: the default collator of another revision's collate.py (the parent
           commit's, to show that the default path has not moved).
  split    where the host time of each path goes: stacking (pageable torch.stack / into pinned memory), the copies and casts
  kernel   (b) preprocess_depth alone at 832 frames per camera: device events around ITERS back-to-back calls, microseconds and
           bytes/s over the algorithmic traffic (every source map read once + the output written once)"""
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), None)
PARENT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent-collate=")), None)
B, WINDOW, REPEATS = 32, 13, 3
CAMERAS = {"static": (200, 200), "gripper": (84, 84)}
LABEL_ENTRIES = (6, 7, 8, 9, 10, 11)
BF = torch.bfloat16


def emit(row):
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def make_batch(seed):
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(B):
        out.append({
            "actions": [rng.uniform(-1, 1, 7).astype(np.float32) for _ in range(WINDOW)],
            "robot_obs": [rng.uniform(-1, 1, 15).astype(np.float32) for _ in range(WINDOW)],
            "rgb_obs": {"rgb_" + c: [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(WINDOW)] for c, (h, w) in CAMERAS.items()},
            "depth_obs": {"depth_" + c: [rng.uniform(0.1, 5, (h, w)).astype(np.float32) for _ in range(WINDOW)] for c, (h, w) in CAMERAS.items()},
            "dino_features_obs": {"dino_feats_" + c: torch.randn(WINDOW, 256, 768, generator=g) for c in CAMERAS},
            "sam_features_obs": {"sam_feats_" + c: torch.randn(WINDOW, 256, 256, generator=g) for c in CAMERAS},
            "lang": "open the drawer"})
    return out


def tokenize(strings):
    return torch.zeros(len(strings), 77, dtype=torch.int64)


def collator(module, **kw):
    return module.DeviceCollator(tokenize, window_size=WINDOW, rgb_pad=10, gripper_pad=4, traj_cons=True, device="cuda", device_resize=True,
                                 generator=torch.Generator().manual_seed(1), **kw)


def default_leg(col, batch):
    out = col(batch)
    return [out[e].to("cuda", BF, non_blocking=True) for e in LABEL_ENTRIES]        # what the training loop does with the labels


def device_leg(col, batch):
    out = col(batch)
    return [out[e] for e in LABEL_ENTRIES]


def label_legs():
    from dreamvla_amd import collate
    batches = [make_batch(s) for s in (1, 2)]
    legs = {"default": (default_leg, collator(collate)), "device": (device_leg, collator(collate, device_labels=True))}
    if PARENT:
        spec = importlib.util.spec_from_file_location("dreamvla_amd._other_collate", PARENT)
        other = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(other)
        legs["default_other_revision"] = (default_leg, collator(other))
    ref = None
    for name, (fn, col) in legs.items():                                            # warm-up, and the legs agree bit for bit
        got = [t.view(torch.int16).cpu() for t in fn(col, batches[0])]
        col.generator.manual_seed(1)
        ref = got if ref is None else ref
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), name
        fn(col, batches[1])
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for r in range(REPEATS):
        for name, (fn, col) in legs.items():
            t0 = time.perf_counter()
            keep = fn(col, batches[r % 2])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            del keep
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    label_bytes = {"depth_fp32_224": 2 * B * WINDOW * 224 * 224 * 4, "depth_raw": sum(B * WINDOW * h * w * 4 for h, w in CAMERAS.values()),
                   "dino_fp32": 2 * B * WINDOW * 256 * 768 * 4, "sam_fp32": 2 * B * WINDOW * 256 * 256 * 4}
    row = {"leg": "labels_resident_bf16", "B": B, "window": WINDOW, "ms": times, "median_ms": med, "spread_ms": spread,
           "host_bytes": label_bytes, "labels_bit_equal": True,
           "device_faster_by_more_than_spread": bool(med["default"] - med["device"] > max(spread["default"], spread["device"]))}
    if PARENT:
        row["default_within_spread_of_other_revision"] = bool(
            abs(med["default"] - med["default_other_revision"]) <= max(spread["default"], spread["default_other_revision"]))
    emit(row)
    return batches[0]


def split_legs(batch):
    """the host's share of each path, step by step, on one batch (median of REPEATS)"""
    from dreamvla_amd import collate, ops
    from dreamvla_amd import preprocess as P

    def timed(fn):
        ts = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del r
        return sorted(ts)[len(ts) // 2]
    feats = [[s[grp][key] for s in batch] for grp, key in (("dino_features_obs", "dino_feats_static"), ("dino_features_obs", "dino_feats_gripper"),
                                                           ("sam_features_obs", "sam_feats_static"), ("sam_features_obs", "sam_feats_gripper"))]
    col = collator(collate, device_labels=True)
    row = {"leg": "host_split_ms"}
    row["default.features.torch_stack_pageable"] = timed(lambda: [torch.stack(f) for f in feats])
    stacked = [torch.stack(f) for f in feats]
    row["default.features.to_device_bf16_from_pageable"] = timed(lambda: [t.to("cuda", BF, non_blocking=True) for t in stacked])
    row["default.depth.depth_image_fn_and_shift"] = timed(lambda: [col._depth(batch, "depth_" + c, p) for c, p in (("static", 10), ("gripper", 4))])
    depth_host = [col._depth(batch, "depth_" + c, p) for c, p in (("static", 10), ("gripper", 4))]
    row["default.depth.to_device_bf16_from_pageable"] = timed(lambda: [t.to("cuda", BF, non_blocking=True) for t in depth_host])

    def stack_pinned(f):
        buf = torch.empty((len(f), *f[0].shape), dtype=f[0].dtype, pin_memory=True)
        return torch.stack(f, out=buf)
    row["device.features.stack_into_pinned"] = timed(lambda: [stack_pinned(f) for f in feats])
    pinned = [stack_pinned(f) for f in feats]
    row["device.features.copy_and_cast_on_device"] = timed(lambda: [ops.cast_to(t.to("cuda", non_blocking=True), BF) for t in pinned])
    row["device.features.whole"] = timed(lambda: [col._feature_labels(f) for f in feats])
    row["device.depth.whole"] = timed(lambda: [col._depth_device(batch, "depth_" + c, p) for c, p in (("static", 10), ("gripper", 4))])
    raw = [torch.from_numpy(np.stack([np.stack(s["depth_obs"]["depth_" + c]) for s in batch])).pin_memory() for c in CAMERAS]
    row["device.depth.copy_and_kernel"] = timed(lambda: [P.preprocess_depth(t.to("cuda", non_blocking=True)) for t in raw])
    emit(row)


def kernel_legs(n=B * WINDOW * 2, iters=50):
    from dreamvla_amd import preprocess as P
    from tests.depth_cases import depth_maps
    for cam, (h, w) in CAMERAS.items():
        host = depth_maps(n, h, w, seed=11)
        dev = host.cuda()
        sh = P.draw_shifts(n, 10, traj=True, generator=torch.Generator().manual_seed(2))
        sh_dev = sh.cuda()
        for dtype, name in ((BF, "bf16"), (torch.float32, "f32")):
            got = P.preprocess_depth(dev[:8], sh[:8], 10, 224, dtype).cpu()
            same = torch.equal(got.view(torch.int16), P.depth_resize_reference(host[:8], sh[:8], 10).to(dtype).view(torch.int16))
            run = lambda: P.preprocess_depth(dev, sh_dev, 10, 224, dtype)
            for _ in range(10):
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
            med = sorted(times)[len(times) // 2]
            nbytes = n * h * w * 4 + n * 224 * 224 * (2 if dtype == BF else 4)
            emit({"leg": "kernel", "camera": cam, "frames": n, "src": [h, w], "out_dtype": name, "kernel_us": times, "median_us": med,
                  "spread_us": max(times) - min(times), "algorithmic_bytes": nbytes, "achieved_TBps": nbytes / (med * 1e-6) / 1e12,
                  "bits_equal_reference": bool(same)})


def main():
    assert torch.cuda.is_available(), "a measurement on the GPU: no fallback"
    kernel_legs()
    batch = label_legs()
    split_legs(batch)


if __name__ == "__main__":
    main()
