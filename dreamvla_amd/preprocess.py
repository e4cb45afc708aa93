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

`resized_crop_u8` / `resized_crop` are MAE's augmentation on the device (csrc/image_resized_crop.hip): a crop box per frame
(`draw_resized_crops`), each crop resized to n_px x n_px with the same arithmetic on the tables of ITS size pair out of a
device-resident store of every size's tables, an optional horizontal flip, and ToTensor + Normalize + the bf16 cast fused in;
`resized_crop_u8_reference` is the host mirror.

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


def draw_resized_crops(n, h, w, scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, generator=None):
    """(n, 5) int32 CPU tensor of (top, left, ch, cw, flip): the boxes of torchvision's RandomResizedCrop.get_params and the coin of
    RandomHorizontalFlip for n frames of h x w, vectorised over n.  Ten attempts per frame, each with an area of h w U(scale) and an
    aspect ratio of exp(U(log ratio)), cw = round(sqrt(area ratio)), ch = round(sqrt(area / ratio)); the first attempt that fits the
    frame is taken at a uniform integer offset; a frame without one gets the central crop with the frame's ratio clamped to
    `ratio`.  The algorithm is torchvision's, the random stream is this function's own."""
    n, h, w = int(n), int(h), int(w)
    if n < 0 or h < 1 or w < 1:
        raise ValueError("draw_resized_crops: n >= 0 frames of at least 1 x 1 expected")
    if not (0.0 < scale[0] <= scale[1] and 0.0 < ratio[0] <= ratio[1] and 0.0 <= p_flip <= 1.0):
        raise ValueError("draw_resized_crops: 0 < scale[0] <= scale[1], 0 < ratio[0] <= ratio[1], 0 <= p_flip <= 1 expected")
    u = torch.rand(4, n, 10, generator=generator, dtype=torch.float64)
    area = (h * w) * (scale[0] + (scale[1] - scale[0]) * u[0])
    log_r = (math.log(ratio[0]), math.log(ratio[1]))
    ar = torch.exp(log_r[0] + (log_r[1] - log_r[0]) * u[1])
    cw = torch.round(torch.sqrt(area * ar)).long()
    ch = torch.round(torch.sqrt(area / ar)).long()
    ok = (cw > 0) & (cw <= w) & (ch > 0) & (ch <= h)
    first = ok.int().argmax(dim=1, keepdim=True)                       # the first attempt that fits (0 where none does)
    found = ok.any(dim=1)
    cw, ch = cw.gather(1, first)[:, 0], ch.gather(1, first)[:, 0]
    top = (u[2].gather(1, first)[:, 0] * (h - ch + 1)).floor().long().minimum(h - ch)      # randint(0, h - ch + 1)
    left = (u[3].gather(1, first)[:, 0] * (w - cw + 1)).floor().long().minimum(w - cw)
    in_ratio = w / h
    if in_ratio < ratio[0]:
        fw, fh = w, int(round(w / ratio[0]))          # w / h < ratio[0]: below h
    elif in_ratio > ratio[1]:
        fh, fw = h, int(round(h * ratio[1]))          # w / h > ratio[1]: below w
    else:
        fw, fh = w, h
    ch, cw = torch.where(found, ch, fh), torch.where(found, cw, fw)
    top, left = torch.where(found, top, (h - fh) // 2), torch.where(found, left, (w - fw) // 2)
    flip = (torch.rand(n, generator=generator, dtype=torch.float64) < p_flip).long()
    return torch.stack((top, left, ch, cw, flip), dim=1).to(torch.int32)


def _check_crops(crops, n, h, w, who):
    """the (n, 5) descriptor tensor on the host, validated before anything is launched -> (crops int32 contiguous, max ch, max cw)"""
    if not isinstance(crops, torch.Tensor) or crops.is_cuda or crops.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{who}: crops: an integer CPU tensor (n, 5) of (top, left, ch, cw, flip) expected")
    if tuple(crops.shape) != (n, 5):
        raise ValueError(f"{who}: crops of shape {tuple(crops.shape)} for {n} frames: ({n}, 5) expected")
    c = crops.to(torch.int64)
    top, left, ch, cw, flip = c.unbind(1)
    if n and not bool(((ch >= 1) & (cw >= 1) & (top >= 0) & (left >= 0) & (top + ch <= h) & (left + cw <= w)).all()):
        raise ValueError(f"{who}: a crop box is empty or leaves the {h} x {w} frame")
    if n and not bool(((flip == 0) | (flip == 1)).all()):
        raise ValueError(f"{who}: flip must be 0 or 1")
    return c.to(torch.int32).contiguous(), (int(ch.max()) if n else 1), (int(cw.max()) if n else 1)


def resized_crop_u8_reference(frames, crops, n_px=224):
    """torchvision's resized_crop(frame, top, left, ch, cw, (n_px, n_px), BICUBIC) + the horizontal flip on a PIL image, restated as
    Pillow's integer arithmetic: frames (n, h, w, 3) uint8 (numpy array or CPU tensor), crops (n, 5) of (top, left, ch, cw, flip)
    -> (n, n_px, n_px, 3) uint8 of the same kind.  The crop is cut out first (the taps clip at ITS edge), its columns are resampled
    with the table of (cw -> n_px) and rounded to uint8, then its rows with the table of (ch -> n_px); an axis of n_px pixels is
    not resampled; a flipped frame has its output columns reversed.  Host-side mirror of dvla_image_resized_crop
    (csrc/image_resized_crop.hip); tests pin it against Pillow byte for byte."""
    is_tensor = isinstance(frames, torch.Tensor)
    a = frames.numpy() if is_tensor else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3:
        raise TypeError("resized_crop_u8_reference: uint8 frames (n, h, w, 3) expected")
    n, h, w = a.shape[:3]
    boxes, _, _ = _check_crops(torch.as_tensor(np.asarray(crops)), n, h, w, "resized_crop_u8_reference")
    out = np.empty((n, n_px, n_px, 3), np.uint8)
    for i, (top, left, ch, cw, flip) in enumerate(boxes.tolist()):
        crop = a[i, top:top + ch, left:left + cw]
        mid = _resample_axis(crop, 1, *_axis_tables(cw, n_px), 0, n_px)
        res = _resample_axis(mid, 0, *_axis_tables(ch, n_px), 0, n_px)
        out[i] = res[:, ::-1] if flip else res
    return torch.from_numpy(out) if is_tensor else out


_crop_table_stores = {}


def _pack_crop_tables(max_size, n_px):
    """the tables of every input size 1 .. max_size for the output size n_px in one int32 array, as csrc/image_resized_crop.hip reads
    it: a directory of (offset, ksize) per size (size 0 unused) and behind it, at each even offset, bounds (n_px, 2) then
    coefficients (n_px, ksize)"""
    head = 2 * (max_size + 1)
    parts, directory, off = [], np.zeros((max_size + 1, 2), np.int32), head
    for s in range(1, max_size + 1):
        bounds, kk = _axis_tables(s, n_px)
        directory[s] = (off, kk.shape[1])
        parts += [bounds.reshape(-1), kk.reshape(-1)]
        off += bounds.size + kk.size
        if off % 2:                                   # bounds are read as 8-byte (first, count) pairs
            parts.append(np.zeros(1, np.int32))
            off += 1
    return np.concatenate([directory.reshape(-1)] + parts).astype(np.int32)


def _crop_table_store(device, h, w, n_px):
    """the device-resident table store of one (device, input size, n_px): built and uploaded on first use (every size up to
    max(h, w): about 2 ms of Python per size), then only looked up -> (int32 device tensor, max_size)"""
    key = (device, h, w, n_px)
    if key not in _crop_table_stores:
        max_size = max(h, w)
        _crop_table_stores[key] = (torch.from_numpy(_pack_crop_tables(max_size, n_px)).to(device), max_size)
    return _crop_table_stores[key]


def _resized_crop(frames_u8, crops, n_px, kind, mean, std, who):
    import ctypes as C
    from . import _lib
    from .ops import _stream
    lib = _lib.load()
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8:
        raise TypeError(f"{who}: uint8 tensor (..., h, w, 3) expected")
    if frames_u8.dim() < 3 or frames_u8.shape[-1] != 3:
        raise ValueError(f"{who}: channels-last RGB frames expected")
    lead, (h, w) = frames_u8.shape[:-3], frames_u8.shape[-3:-1]
    n_px = int(n_px)
    if h < 1 or w < 1 or n_px < 1:
        raise ValueError(f"{who}: empty frames")
    if kind == _lib.CROP_OUT_BF16 and n_px % 8:
        raise ValueError(f"{who}: n_px = {n_px}: the bf16 kind stores 8 pixels at a time (n_px % 8 == 0), as preprocess_frames does")
    n = math.prod(lead)
    boxes, max_ch, max_cw = _check_crops(crops, n, h, w, who)
    if not frames_u8.is_cuda:
        raise _lib.DvlaError(f"{who}: tensor is on {frames_u8.device}; the HIP input pipeline has no CPU fallback")
    src =frames_u8.reshape(-1, h, w, 3).contiguous()
    if kind == _lib.CROP_OUT_BF16:
        out = torch.empty((n, 3, n_px, n_px), dtype=torch.bfloat16, device=src.device)
        m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    else:
        out = torch.empty((n, n_px, n_px, 3), dtype=torch.uint8, device=src.device)
        m3 = s3 = None
    if n:
        store, max_size = _crop_table_store(src.device, h, w, n_px)
        dev_boxes = boxes.pin_memory().to(src.device, non_blocking=True)   # the call's one host -> device copy; the host does not wait
        _lib.check(lib.dvla_image_resized_crop(src.data_ptr(), out.data_ptr(), dev_boxes.data_ptr(), store.data_ptr(), n, h, w, max_size,
                                               max_ch, max_cw, n_px, kind, m3, s3, _stream()), "dvla_image_resized_crop")
    return out.view(*lead, *out.shape[1:])


def resized_crop_u8(frames_u8, crops, n_px=224):
    """frames_u8: (..., h, w, 3) uint8 CUDA tensor (raw frames of one size); crops: (n, 5) integer CPU tensor of (top, left, ch, cw,
    flip), one row per frame (`draw_resized_crops`) -> (..., n_px, n_px, 3) uint8 on the device: every frame cropped to its own
    box, resized to n_px x n_px (BICUBIC) and flipped where flip = 1, bit-identical to Pillow's crop -> resize -> transpose
    (`resized_crop_u8_reference`), one HIP kernel (no CPU fallback).  The boxes are validated on the host before the launch."""
    from . import _lib
    return _resized_crop(frames_u8, crops, n_px, _lib.CROP_OUT_U8, None, None, "resized_crop_u8")


def resized_crop(frames_u8, crops, n_px=224, mean=CLIP_MEAN, std=CLIP_STD):
    """`resized_crop_u8` with ToTensor + Normalize + the bf16 cast fused in -> (..., 3, n_px, n_px) bf16 on the device,
    bit-identical to `preprocess_frames(resized_crop_u8(frames_u8, crops, n_px), mean=mean, std=std)`; n_px % 8 == 0."""
    from . import _lib
    return _resized_crop(frames_u8, crops, n_px, _lib.CROP_OUT_BF16, mean, std, "resized_crop")


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
