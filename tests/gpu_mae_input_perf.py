"""What feeding MAE pretraining from raw frames costs (a measurement script, not a test): the per-frame resized crop + flip +
normalise kernel (csrc/image_resized_crop.hip), `MAEFrameAugment` as a caller uses it, and the MAE training step behind it.  One
JSON line per measurement on stdout and, appended, in the file named by --out=PATH (the recorded run is kept as
profiles/r13_mae_input_perf.jsonl).

    python tests/gpu_mae_input_perf.py [--out=PATH] [--no-step]

  kernel   the fused bf16 launch (resident descriptors drawn with MAE's scale / ratio, output allocated per call as the public
           function does) at 256 and 832 frames of 200 x 200 and of 84 x 84, against the pair it replaces for a FIXED geometry,
           `resize_frames_u8` + `preprocess_frames`, at the same frame count and source size; the two legs alternate in one process,
           device events around ITERS back-to-back calls after warm-up, REPEATS windows each; achieved bytes/s over the algorithmic
           traffic (crop bytes read + bf16 bytes written; the pair also writes and re-reads the uint8 frames)
  augment  the steady-state `MAEFrameAugment` call at 256 frames (draw on the host + descriptor upload + launch), host clock
           around calls that end in a synchronise, against the same augmentation through Pillow on 16 host threads + upload +
           `preprocess_frames`
  step     one MAE training step (ViT-B/16 encoder, 512 / 8 / 16 decoder, mask_ratio 0.75, forward + loss + backward) at N = 256 fed by
           `MAEFrameAugment` from resident uint8 frames, against the same step on resident `imgs` (tests/gpu_mae_perf.py's
           protocol), alternating"""
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


def window(fn, iters):
    """device-event time per call of `fn` in us over one window of `iters` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernel_legs():
    import ctypes
    from dreamvla_amd import _lib, preprocess as P
    from dreamvla_amd.ops import _stream
    from tests.resize_cases import frames
    from tests.resized_crop_cases import pillow_crops
    lib = _lib.load()
    m3, s3 = (ctypes.c_float * 3)(*P.CLIP_MEAN), (ctypes.c_float * 3)(*P.CLIP_STD)
    for total in (256, 832):
        for h, w in CAMERAS:
            host = frames(h, w, "noise", total, seed=total)
            dev = torch.from_numpy(host).cuda()
            crops = P.draw_resized_crops(total, h, w, generator=torch.Generator().manual_seed(total))
            boxes, max_ch, max_cw = P._check_crops(crops, total, h, w, "perf")
            dev_boxes = boxes.cuda()
            store, max_size = P._crop_table_store(dev.device, h, w, 224)

            def fused():
                out = torch.empty((total, 3, 224, 224), dtype=torch.bfloat16, device="cuda")
                rc = lib.dvla_image_resized_crop(dev.data_ptr(), out.data_ptr(), dev_boxes.data_ptr(), store.data_ptr(), total, h, w, max_size,
                                                 max_ch, max_cw, 224, _lib.CROP_OUT_BF16, m3, s3, _stream())
                assert rc == 0
                return out

            def pair():
                return P.preprocess_frames(P.resize_frames_u8(dev))

            k = 16                                                  # results must not change: the first frames against Pillow
            same = bool((fused()[:k].view(torch.int16) == P.preprocess_frames(torch.from_numpy(pillow_crops(host[:k], crops[:k])).cuda()).view(torch.int16)).all())
            iters = 200 if total == 256 else 60
            for _ in range(20):
                fused()
                pair()
            torch.cuda.synchronize()
            tf, tp = [], []
            for _ in range(REPEATS):                                # alternate the legs
                tf.append(window(fused, iters))
                tp.append(window(pair, iters))
            mf, mp = sorted(tf)[len(tf) // 2], sorted(tp)[len(tp) // 2]
            crop_bytes = int((crops[:, 2].long() * crops[:, 3].long() * 3).sum())
            nbytes = crop_bytes + total * 224 * 224 * 3 * 2
            pair_bytes = host.size + total * 224 * 224 * 3 * (1 + 1 + 2)
            emit({"leg": "kernel", "frames": total, "size": [h, w], "fused_us": tf, "pair_us": tp, "fused_median_us": mf, "pair_median_us": mp,
                  "fused_spread_us": max(tf) - min(tf), "pair_spread_us": max(tp) - min(tp), "fused_over_pair": mf / mp,
                  "fused_algorithmic_bytes": nbytes, "fused_achieved_GBps": nbytes / (mf * 1e-6) / 1e9, "pair_algorithmic_bytes": pair_bytes,
                  "pair_achieved_GBps": pair_bytes / (mp * 1e-6) / 1e9, "mean_crop_side": float(crops[:, 2:4].float().mean()),
                  "bits_equal_pillow_then_preprocess": same, "fused_not_slower_than_pair": bool(mf <= mp)})


def augment_leg(n=256, calls=30):
    from PIL import Image
    from dreamvla_amd import preprocess as P
    from dreamvla_amd.vit_mae import MAEFrameAugment
    from tests.resize_cases import frames
    for h, w in CAMERAS:
        host = frames(h, w, "noise", n, seed=7)
        dev = torch.from_numpy(host).cuda()
        aug = MAEFrameAugment(generator=torch.Generator().manual_seed(1))
        gen = torch.Generator().manual_seed(1)

        def one(args):
            f, (top, left, ch, cw, flip) = args
            im = Image.fromarray(f).crop((left, top, left + cw, top + ch)).resize((224, 224), Image.BICUBIC)
            return np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im)

        def device_call():
            return aug(dev)

        ex = ThreadPoolExecutor(16)

        def pillow_call():
            crops = P.draw_resized_crops(n, h, w, generator=gen).tolist()
            u8 = np.stack(list(ex.map(one, zip(host, crops), chunksize=max(1, n // 64))))
            return P.preprocess_frames(torch.from_numpy(u8).pin_memory().to("cuda", non_blocking=True))

        for _ in range(5):
            device_call()
        pillow_call()
        torch.cuda.synchronize()
        times = {"augment_on_device": [], "pillow_16_threads": []}
        for _ in range(REPEATS):
            for name, fn, k in (("augment_on_device", device_call, calls), ("pillow_16_threads", pillow_call, 3)):
                t0 = time.perf_counter()
                for _ in range(k):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / k * 1e3)
        t0 = time.perf_counter()                     # the host's share of the device call: the draw alone
        for _ in range(calls):
            P.draw_resized_crops(n, h, w, generator=gen)
        draw_ms = (time.perf_counter() - t0) / calls * 1e3
        ex.shutdown()
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        emit({"leg": "augment_call", "frames": n, "size": [h, w], "ms_per_call": times, "median_ms": med, "draw_ms": draw_ms,
              "spread_ms": {k: max(v) - min(v) for k, v in times.items()}, "frames_per_s": {k: n / (v * 1e-3) for k, v in med.items()},
              "speedup_vs_pillow_16_threads": med["pillow_16_threads"] / med["augment_on_device"]})


def step_leg(n=256, iters=10, warmup=8):
    from dreamvla_amd.nn import LayerNorm
    from dreamvla_amd.vit_mae import MAEFrameAugment, MaskedAutoencoderViT
    from tests.gpu_mae_perf import MODEL, RATIO
    from tests.gpu_perf import timeit
    from tests.resize_cases import frames
    torch.manual_seed(0)
    m = MaskedAutoencoderViT(**MODEL, norm_layer=lambda d: LayerNorm(d, eps=1e-6)).to(torch.bfloat16).cuda()
    dev = torch.from_numpy(frames(200, 200, "noise", n, seed=3)).cuda()
    aug = MAEFrameAugment(generator=torch.Generator().manual_seed(2))
    imgs = aug(dev)
    noise = torch.rand(n, 196, device="cuda")

    def step(x):
        m.zero_grad(set_to_none=True)
        loss, _, _ = m(x, RATIO, noise=noise)
        loss.backward()
        return loss

    resident = lambda: step(imgs)
    from_frames = lambda: step(aug(dev))
    timeit(resident, iters=1, warmup=warmup)            # the GEMM tuner locks its choices in these
    timeit(from_frames, iters=1, warmup=2)
    times = {"resident_imgs": [], "from_uint8_frames": []}
    for _ in range(REPEATS):
        for name, fn in (("resident_imgs", resident), ("from_uint8_frames", from_frames)):
            times[name].append(timeit(fn, iters=iters, warmup=1) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    emit({"leg": "mae_train_step", "N": n, "size": [200, 200], "mask_ratio": RATIO, "ms_per_step": times, "median_ms": med,
          "spread_ms": {k: max(v) - min(v) for k, v in times.items()}, "augment_ms": med["from_uint8_frames"] - med["resident_imgs"],
          "augment_share_of_step": (med["from_uint8_frames"] - med["resident_imgs"]) / med["from_uint8_frames"],
          "images_per_s": {k: n / (v * 1e-3) for k, v in med.items()}})


def main():
    assert torch.cuda.is_available(), "a measurement on the GPU: no fallback"
    kernel_legs()
    augment_leg()
    if "--no-step" not in sys.argv:
        step_leg()


if __name__ == "__main__":
    main()
