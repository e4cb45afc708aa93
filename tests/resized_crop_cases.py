"""Crop boxes and the Pillow yardstick shared by the resized-crop tests (tests/test_resized_crop.py, tests/test_resized_crop_gpu.py)
and the measurement (tests/gpu_mae_input_perf.py).  Frame contents come from tests/resize_cases.frames."""
import numpy as np
import torch

# (h, w) of the source frame: CALVIN's two cameras, a portrait frame with a side of 225 and a landscape frame larger than 224 on
# both sides (crops of it mix down-scaling, up-scaling and the 224-sided identity pass)
SOURCES = [(200, 200), (84, 84), (300, 225), (480, 640)]


def edge_crops(h, w, n_px=224):
    """the eight (top, left, ch, cw, flip) boxes at which the geometry can go wrong: the whole frame; one pixel at either corner; a
    5-wide strip on the right border and a 3-high strip on the bottom border (taps clipped at the crop's edge on both sides at
    once); n_px on every axis the frame is large enough for (the pass Pillow skips; a fraction of the side otherwise); an interior
    box; an interior box flipped"""
    return [(0, 0, h, w, 0),
            (0, 0, 1, 1, 0),
            (h - 1, w - 1, 1, 1, 0),
            (0, w - 5, h, 5, 0),
            (h - 3, 0, 3, w, 0),
            (min(10, h - n_px) if h >= n_px else 1, 1 if w > n_px else 0, n_px if h >= n_px else h // 2, n_px if w >= n_px else w // 3, 0),
            (h // 5, w // 4, h // 2, w // 3, 0),
            (h // 3, w // 5, h // 3 + 1, w // 2 + 1, 1)]


def crops_for(h, w, drawn, n_px=224, seed=0):
    """(8 + drawn, 5) int32: the edge crops, then `drawn` boxes of draw_resized_crops (MAE's scale and ratio)"""
    from dreamvla_amd import preprocess as P
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    return torch.cat([torch.tensor(edge_crops(h, w, n_px), dtype=torch.int32), P.draw_resized_crops(drawn, h, w, generator=g)])


def pillow_crops(frames_u8, crops, n_px=224):
    """the yardstick: torchvision's resized_crop + hflip on a PIL image, which are Pillow's crop -> resize(BICUBIC) -> transpose"""
    from PIL import Image
    out = np.empty((len(frames_u8), n_px, n_px, 3), np.uint8)
    for i, (f, (top, left, ch, cw, flip)) in enumerate(zip(frames_u8, np.asarray(crops).tolist())):
        im = Image.fromarray(np.ascontiguousarray(f)).crop((left, top, left + cw, top + ch)).resize((n_px, n_px), Image.BICUBIC)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        out[i] = np.asarray(im)
    return out
