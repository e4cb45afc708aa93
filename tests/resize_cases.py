"""Frame sizes and contents shared by the resize tests (tests/test_image_resize.py, tests/test_image_resize_gpu.py) and the
measurement (tests/gpu_resize_perf.py): the camera sizes the project meets (CALVIN 200 x 200 static / 84 x 84 gripper), two
other square sizes on either side of 224, three non-square sizes with a crop on one axis, and 224-sided frames, where Pillow
skips one pass (224 x 300, 300 x 224) or both (224 x 224)."""
import numpy as np

# (h, w) of the source frame
SIZES = [(200, 200), (84, 84), (128, 128), (256, 256), (480, 640), (720, 1280), (300, 225), (224, 224), (224, 300), (300, 224)]
# noise; smooth ramps; a random {0, 255} pattern, which overshoots on both sides and clamps; the two constant extremes
CONTENTS = ["noise", "ramps", "extreme", "zeros", "ones"]


def frames(h, w, kind, n, seed=0):
    """(n, h, w, 3) uint8, every frame different where the content allows it"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    if kind == "noise":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "extreme":
        return (rng.integers(0, 2, (n, h, w, 3)) * 255).astype(np.uint8)
    if kind == "ramps":
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([yy * 255 // max(h - 1, 1), xx * 255 // max(w - 1, 1), (yy + xx) % 256], -1)
        return np.stack([(base + 7 * i) % 256 for i in range(n)]).astype(np.uint8)          # a different phase per frame
    if kind in ("zeros", "ones"):
        return np.full((n, h, w, 3), 0 if kind == "zeros" else 255, np.uint8)
    raise ValueError(kind)


def pillow(frames_u8, n_px=224):
    """the yardstick: dreamvla_amd.preprocess.clip_image_resize_u8 (Pillow's BICUBIC resize + centre crop) frame by frame"""
    from dreamvla_amd import preprocess as P
    return np.stack([P.clip_image_resize_u8(f, n_px) for f in frames_u8])
