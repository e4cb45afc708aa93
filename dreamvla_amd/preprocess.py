"""Camera-frame preprocessing: the host half (`clip_image_preprocess`, the drop-in for the
`image_processor` that `clip.load` returns and eval / data code calls: utils/data_utils.py:175-178) and the device half
(`preprocess_frames`: ToTensor + Normalize + RandomShiftsAug + bf16 cast in one HIP kernel, csrc/input_pipeline.hip).

clip's `_transform(224)` (openai/CLIP clip/clip.py) is
    Resize(224, interpolation=BICUBIC) -> CenterCrop(224) -> convert("RGB") -> ToTensor() -> Normalize(CLIP_MEAN, CLIP_STD)
torchvision's Resize / CenterCrop on a PIL image are `Image.resize((w', h'), BICUBIC)` with the SHORTER side scaled to 224
(the other side truncated to int) and a crop whose offsets are round((size - 224) / 2); restated here on PIL directly
(torchvision is not a dependency of this package).

`resize_frames_u8` is that Resize + CenterCrop on the device (csrc/image_resize.hip), byte for byte Pillow's: Pillow resamples
8-bit images in fixed point on coefficient tables computed once per (input size, output size) in double precision, so the
tables are built here on the host exactly as Pillow builds them (`bicubic_tables`) and the kernel does integer arithmetic only;
`resize_u8_reference` is the same integer arithmetic in numpy, the host mirror of the kernel.

`preprocess_depth` is the depth labels' counterpart of `preprocess_frames` (csrc/depth_pipeline.hip): the collator's nearest resize
of the raw fp32 depth maps, the shift gather and the cast in one kernel; `depth_resize_reference` is its host mirror."""
import functools
import math

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _to_pil(img):
    from PIL import Image
    if isinstance(img, Image.Image):
        return img
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[0] in (1, 3) and a.shape[2] not in (1, 3):
        a = np.transpose(a, (1, 2, 0))
    if a.dtype != np.uint8:
        a = np.clip(a * (255.0 if a.max() <= 1.0 else 1.0), 0, 255).astype(np.uint8)
    return Image.fromarray(a.squeeze() if a.ndim == 3 and a.shape[2] == 1 else a)


def clip_image_resize_u8(img, n_px=224):
    """Resize(n_px, BICUBIC) + CenterCrop(n_px) + RGB -> uint8 (n_px, n_px, 3) numpy array: the part of the CLIP transform
    that stays on the host (PIL's antialiased bicubic); the rest runs in `preprocess_frames` on the device."""
    from PIL import Image
    pil = _to_pil(img)
    w, h = pil.size
    if w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nw, nh = int(n_px * w / h), n_px
    if (nw, nh) != (w, h):
        pil = pil.resize((nw, nh), Image.BICUBIC)
    left, top = int(round((nw - n_px) / 2.0)), int(round((nh - n_px) / 2.0))
    pil = pil.crop((left, top, left + n_px, top + n_px)).convert("RGB")
    return np.asarray(pil, dtype=np.uint8)


def clip_image_preprocess(img, n_px=224):
    """`image_processor(pil)` of the reference (the second return value of clip.load): -> fp32 (3, n_px, n_px)"""
    u8 = torch.from_numpy(clip_image_resize_u8(img, n_px).copy())
    x = u8.permute(2, 0, 1).float().div(255.0)                                      # ToTensor
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=torch.float32).view(3, 1, 1)
    return x.sub_(mean).div_(std)                                                   # Normalize


PRECISION_BITS = 22          # Pillow's fixed point for 8-bit images (32 - 8 - 2)


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def bicubic_tables(insz, outsz):
    """Pillow's coefficient table of one axis for the BICUBIC filter on 8-bit data (precompute_coeffs + normalize_coeffs_8bpc of
    its Resample.c, the same float64 operations in the same order): bounds (outsz, 2) int32 = (first input index, tap count) per
    output index and kk (outsz, ksize) int32 = the taps' coefficients at 22 fractional bits (zero behind the tap count).
    Read-only arrays, cached per size pair."""
    insz, outsz = int(insz), int(outsz)
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((outsz, 2), np.int32)
    kk = np.zeros((outsz, ksize), np.int32)
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                 # int() truncates towards zero, as the C cast does
        xmax = min(int(center + support + 0.5), insz) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:                                                # summed in index order
            ww += w
        for x, w in enumerate(k):
            if ww != 0.0:
                w = w / ww
            v = w * (1 << PRECISION_BITS)
            kk[xx, x] = int(v + 0.5) if w >= 0 else int(v - 0.5)
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


@functools.lru_cache(maxsize=None)
def _identity_tables(size):
    """the table of an axis Pillow does not resample (input size == output size): one tap of 1.0, which the fixed-point pass maps
    to the input byte exactly -- ((1 << 21) + v * (1 << 22)) >> 22 == v"""
    bounds = np.stack([np.arange(size, dtype=np.int32), np.ones(size, np.int32)], axis=1)
    return bounds, np.full((size, 1), 1 << PRECISION_BITS, np.int32)


def _axis_tables(insz, outsz):
    return _identity_tables(insz) if insz == outsz else bicubic_tables(insz, outsz)


def _resize_geometry(h, w, n_px):
    """(nh, nw, top, left) of `clip_image_resize_u8`: the shorter side goes to n_px, the other to int(n_px * long / short); the crop
    offsets are int(round((size - n_px) / 2.0))"""
    if w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nw, nh = int(n_px * w / h), n_px
    return nh, nw, int(round((nh - n_px) / 2.0)), int(round((nw - n_px) / 2.0))


def _resample_axis(a, axis, bounds, kk, first, count):
    """one fixed-point pass along `axis` of a uint8 array for the output indices first .. first + count - 1"""
    a = np.moveaxis(a, axis, 0)
    out = np.empty((count,) + a.shape[1:], np.uint8)
    for i in range(count):
        xmin, n = bounds[first + i]
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)          # signed 32-bit accumulator, as Pillow's
        for t in range(n):
            acc += a[xmin + t].astype(np.int32) * kk[first + i, t]
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)                           # arithmetic shift
    return np.moveaxis(out, 0, axis)


def resize_u8_reference(frames, n_px=224):
    """`clip_image_resize_u8` restated as Pillow's integer arithmetic: frames (..., h, w, 3) uint8 (numpy array or CPU tensor) ->
    (..., n_px, n_px, 3) uint8 of the same kind.  Horizontal pass first, rounded to uint8, then the vertical pass on those bytes;
    an axis whose size does not change is not resampled; the crop selects which outputs are computed.  Host-side mirror of
    dvla_image_resize_u8 (csrc/image_resize.hip); tests pin it against Pillow byte for byte."""
    is_tensor = isinstance(frames, torch.Tensor)
    a = frames.numpy() if is_tensor else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-1] != 3:
        raise TypeError("resize_u8_reference: uint8 frames (..., h, w, 3) expected")
    h, w = a.shape[-3:-1]
    nh, nw, top, left = _resize_geometry(h, w, n_px)
    bx, kx = _axis_tables(w, nw)
    by, ky = _axis_tables(h, nh)
    r0, r1 = int(by[top, 0]), int(by[top + n_px - 1, 0] + by[top + n_px - 1, 1])   # the input rows under the cropped rows' taps
    mid = _resample_axis(a[..., r0:r1, :, :], a.ndim - 2, bx, kx, left, n_px)
    by = by - np.array([r0, 0], np.int32)
    out = np.ascontiguousarray(_resample_axis(mid, a.ndim - 3, by, ky, top, n_px))
    return torch.from_numpy(out) if is_tensor else out


_device_tables = {}


def _tables_on(device, insz, outsz):
    """(bounds, coefficients, ksize) of one axis on `device`: uploaded once per (device, size pair)"""
    key = (device, insz, outsz)
    if key not in _device_tables:
        bounds, kk = _axis_tables(insz, outsz)
        _device_tables[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(kk.copy()).to(device), kk.shape[1])
    return _device_tables[key]


def resize_frames_u8(frames_u8, n_px=224):
    """frames_u8: (..., h, w, 3) uint8 CUDA tensor (raw camera frames of one size) -> (..., n_px, n_px, 3) uint8 on the device:
    Resize(n_px, BICUBIC) + CenterCrop(n_px), bit-identical to `clip_image_resize_u8` of every frame, one HIP kernel
    (no CPU fallback)."""
    from . import _lib
    from .ops import _stream
    lib = _lib.load()
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8:
        raise TypeError("resize_frames_u8: uint8 tensor (..., h, w, 3) expected")
    if not frames_u8.is_cuda:
        raise _lib.DvlaError(f"resize_frames_u8: tensor is on {frames_u8.device}; the HIP input pipeline has no CPU fallback")
    if frames_u8.dim() < 3 or frames_u8.shape[-1] != 3:
        raise ValueError("resize_frames_u8: channels-last RGB frames expected")
    lead, (h, w) = frames_u8.shape[:-3], frames_u8.shape[-3:-1]
    if h < 1 or w < 1:
        raise ValueError("resize_frames_u8: empty frames")
    src = frames_u8.reshape(-1, h, w, 3).contiguous()
    n = src.shape[0]
    nh, nw, top, left = _resize_geometry(h, w, int(n_px))
    bx, kx, ksx = _tables_on(src.device, w, nw)
    by, ky, ksy = _tables_on(src.device, h, nh)
    out = torch.empty((n, n_px, n_px, 3), dtype=torch.uint8, device=src.device)
    _lib.check(lib.dvla_image_resize_u8(src.data_ptr(), out.data_ptr(), n, h, w, nh, nw, bx.data_ptr(), kx.data_ptr(), ksx,
                                        by.data_ptr(), ky.data_ptr(), ksy, left, top, int(n_px), _stream()), "dvla_image_resize_u8")
    return out.view(*lead, n_px, n_px, 3)


def draw_shifts(n, pad, traj=False, generator=None):
    """integer (sx, sy) per frame as RandomShiftsAug draws them (utils/data_utils.py:344-348 / 371-375):
    forward(): randint(0, 2 pad + 1), one pair per image; forward_traj(): randint(1, 2 pad + 1), one pair per frame."""
    return torch.randint(1 if traj else 0, 2 * pad + 1, (n, 2), generator=generator, dtype=torch.int32)


def shift_gather_reference(x, shifts, pad):
    """RandomShiftsAug as the gather it is (exact arithmetic): x (n, c, h, w) any dtype, shifts (n, 2) ints (sx, sy).
    Host-side mirror of the kernel's addressing; tests pin it against the real RandomShiftsAug module."""
    n, c, h, w = x.shape
    ys = torch.arange(h).view(1, h) + shifts[:, 1].view(n, 1).long() - pad
    xs = torch.arange(w).view(1, w) + shifts[:, 0].view(n, 1).long() - pad
    ys, xs = ys.clamp_(0, h - 1), xs.clamp_(0, w - 1)
    idx_n = torch.arange(n).view(n, 1, 1, 1)
    idx_c = torch.arange(c).view(1, c, 1, 1)
    return x[idx_n, idx_c, ys.view(n, 1, h, 1), xs.view(n, 1, 1, w)]


def preprocess_frames(frames_u8, shifts=None, pad=0, mean=CLIP_MEAN, std=CLIP_STD):
    """frames_u8: (..., H, W, 3) uint8 CUDA tensor (resized frames); shifts: (n, 2) int32 (sx, sy) or None.
    -> (..., 3, H, W) bf16 on the device: ToTensor + Normalize + RandomShiftsAug + cast, one HIP kernel (no CPU fallback)."""
    import ctypes as C
    from . import _lib
    from .ops import _stream
    lib = _lib.load()
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8:
        raise TypeError("preprocess_frames: uint8 tensor (..., H, W, 3) expected")
    if not frames_u8.is_cuda:
        raise _lib.DvlaError(f"preprocess_frames: tensor is on {frames_u8.device}; the HIP input pipeline has no CPU fallback")
    lead, (H, W, ch) = frames_u8.shape[:-3], frames_u8.shape[-3:]
    if ch != 3:
        raise ValueError("preprocess_frames: channels-last RGB frames expected")
    src = frames_u8.reshape(-1, H, W, 3).contiguous()
    n = src.shape[0]
    sh = None
    if shifts is not None:
        sh = shifts.to(device=src.device, dtype=torch.int32).reshape(n, 2).contiguous()
    out = torch.empty((n, 3, H, W), dtype=torch.bfloat16, device=src.device)
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.dvla_image_preprocess(src.data_ptr(), None if sh is None else sh.data_ptr(), out.data_ptr(), n, H, W, int(pad),
                                         m3, s3, _stream()), "dvla_image_preprocess")
    return out.view(*lead, 3, H, W)


def nearest_index(insz, outsz):
    """ATen's nearest-neighbour source index of every output index, as F.interpolate(mode="nearest") computes it on a float
    tensor: min(int(floorf(j * (float(insz) / outsz))), insz - 1), the scale and the product in fp32.  (outsz,) int64."""
    scale = np.float32(insz) / np.float32(outsz)
    idx = np.floor(np.arange(outsz, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, insz - 1))


def depth_resize_reference(depth, shifts=None, pad=0, size=224):
    """`collate.depth_image_fn` followed by RandomShiftsAug, as the gather the two are (exact: no arithmetic on the values):
    depth (n, h, w) fp32 CPU tensor, shifts (n, 2) ints (sx, sy) or None -> (n, 1, size, size) fp32,
        out[i, 0, y, x] = depth[i, ry[clamp(y + sy_i - pad, 0, size - 1)], rx[clamp(x + sx_i - pad, 0, size - 1)]]
    with ry / rx = `nearest_index`.  Host-side mirror of dvla_depth_preprocess (csrc/depth_pipeline.hip); tests pin it against
    F.interpolate and `shift_gather_reference` bit for bit."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 3:
        raise TypeError("depth_resize_reference: fp32 tensor (n, h, w) expected")
    n, h, w = depth.shape
    ys = torch.arange(size).view(1, size).expand(n, size)
    xs = torch.arange(size).view(1, size).expand(n, size)
    if shifts is not None and pad > 0:
        ys = ys + shifts[:, 1].view(n, 1).long() - pad
        xs = xs + shifts[:, 0].view(n, 1).long() - pad
    ys, xs = nearest_index(h, size)[ys.clamp(0, size - 1)], nearest_index(w, size)[xs.clamp(0, size - 1)]
    return depth[torch.arange(n).view(n, 1, 1), ys.view(n, size, 1), xs.view(n, 1, size)].unsqueeze(1)


def preprocess_depth(depth_f32, shifts=None, pad=0, size=224, dtype=torch.bfloat16):
    """depth_f32: (..., h, w) fp32 CUDA tensor (raw depth maps of one size); shifts: (n, 2) int32 (sx, sy) or None.
    -> (..., 1, size, size) `dtype` (bf16 or fp32) on the device: nearest resize + RandomShiftsAug + cast, one HIP kernel
    (no CPU fallback).  A non-contiguous input is made contiguous first."""
    from . import _lib
    from .ops import _stream
    if not isinstance(depth_f32, torch.Tensor) or depth_f32.dtype != torch.float32:
        raise TypeError("preprocess_depth: fp32 tensor (..., h, w) expected")
    if not depth_f32.is_cuda:
        raise _lib.DvlaError(f"preprocess_depth: tensor is on {depth_f32.device}; the HIP input pipeline has no CPU fallback")
    lib = _lib.load()
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"preprocess_depth: dtype {dtype}: torch.bfloat16 or torch.float32")
    if depth_f32.dim() < 2:
        raise ValueError("preprocess_depth: depth maps (..., h, w) expected")
    lead, (h, w) = depth_f32.shape[:-2], depth_f32.shape[-2:]
    size = int(size)
    if h < 1 or w < 1 or size < 1:
        raise ValueError("preprocess_depth: empty depth maps")
    src = depth_f32.reshape(-1, h, w).contiguous()
    n = src.shape[0]
    sh = None
    if shifts is not None:
        sh = shifts.to(device=src.device, dtype=torch.int32).reshape(n, 2).contiguous()
    out = torch.empty((n, 1, size, size), dtype=dtype, device=src.device)
    if n == 0:
        return out.view(*lead, 1, size, size)
    _lib.check(lib.dvla_depth_preprocess(src.data_ptr(), None if sh is None else sh.data_ptr(), out.data_ptr(), n, h, w, size, size,
                                         int(pad), _lib.DT_BF16 if dtype == torch.bfloat16 else _lib.DT_F32, _stream()),
               "dvla_depth_preprocess")
    return out.view(*lead, 1, size, size)
