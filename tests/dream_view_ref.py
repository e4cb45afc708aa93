"""References of the dream pictures (csrc/dream_view.hip, ops.depth_colorize .. ops.feature_render) in numpy: float64 where the
kernel computes, float32 with one rounding per operation where a kernel promises its bits.  Reads nothing outside the package and
tests/golden/.  Used by tests/test_dream_views.py (against hand-placed cases, on the CPU) and tests/test_dream_views_gpu.py."""
import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ---------------------------------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------------------------------
def level_f32(v, lo, hi):
    """the kernels' level(v, lo, hi) restated operation by operation in float32: s = v - lo; r = hi - lo; t = s / r;
    t = (r > 0 and t > 0) ? min(t, 1) : 0; rint(255 t) half to even.  v float32 array, lo / hi float32 scalars or arrays."""
    f = np.float32
    with np.errstate(all="ignore"):
        s = np.subtract(v, lo, dtype=f)
        r = np.subtract(hi, lo, dtype=f)
        t = np.divide(s, r, dtype=f)
        t = np.where((r > 0) & (t > 0), np.minimum(t, f(1)), f(0)).astype(f)
        u = np.multiply(f(255), t, dtype=f)
        return np.rint(u).astype(np.int64)


def depth_colorize(depth, palette, lo=None, hi=None, nan_color=(0, 0, 0)):
    """depth (n, h, w) float32, palette (256, 3) uint8 -> (n, h, w, 3) uint8; lo / hi None: per map the finite min / max"""
    depth = np.asarray(depth, dtype=np.float32)
    n = depth.shape[0]
    out = np.empty(depth.shape + (3,), dtype=np.uint8)
    for i in range(n):
        d = depth[i]
        fin = np.isfinite(d)
        if lo is None:
            l, h = (d[fin].min(), d[fin].max()) if fin.any() else (np.float32(np.inf), np.float32(-np.inf))
        else:
            l, h = np.float32(lo), np.float32(hi)
        idx = level_f32(np.where(fin, d, np.float32(0)), l, h)
        img = palette[np.where(fin, idx, 0)]
        img[~fin] = np.asarray(nan_color, dtype=np.uint8)
        out[i] = img
    return out


# ---------------------------------------------------------------------------------------------------
# flow
# ---------------------------------------------------------------------------------------------------
def flow_unshuffle(pred):
    """(n, g g, 2 f f) with channel = c f f + i f + j -> (n, g f, g f, 2): flow[y f + i, x f + j, c]"""
    pred = np.asarray(pred)
    n, L, D = pred.shape
    g, f = int(round(L ** 0.5)), int(round((D // 2) ** 0.5))
    assert g * g == L and 2 * f * f == D
    return pred.reshape(n, g, g, 2, f, f).transpose(0, 1, 4, 2, 5, 3).reshape(n, g * f, g * f, 2)


def hsv_to_rgb(Hh, V):
    """integers Hh in 0 .. 179 (OpenCV's 8-bit hue), S = 255, V in 0 .. 255 -> (.., 3) uint8: sextant s = Hh // 30,
    X = (V (30 - |Hh % 60 - 30|) + 15) // 30, (R, G, B) = (V,X,0) (X,V,0) (0,V,X) (0,X,V) (X,0,V) (V,0,X)"""
    Hh, V = np.asarray(Hh, dtype=np.int64), np.asarray(V, dtype=np.int64)
    X = (V * (30 - np.abs(Hh % 60 - 30)) + 15) // 30
    s = Hh // 30
    Z = np.zeros_like(V)
    table = [(V, X, Z), (X, V, Z), (Z, V, X), (Z, X, V), (X, Z, V), (V, Z, X)]
    rgb = np.zeros(V.shape + (3,), dtype=np.int64)
    for k, cols in enumerate(table):
        for c in range(3):
            rgb[..., c] = np.where(s == k, cols[c], rgb[..., c])
    return rgb.astype(np.uint8)


def wheel_parts(flow):
    """flow (.., 2) -> (angle / 2 in [0, 180), 32 |flow|) in float64, before truncation"""
    flow = np.asarray(flow, dtype=np.float64)
    dx, dy = flow[..., 0], flow[..., 1]
    ang = np.degrees(np.arctan2(dy, dx))
    ang = np.where(ang < 0, ang + 360.0, ang)
    ang = np.where(ang >= 360.0, 0.0, ang)
    return ang / 2.0, 32.0 * np.hypot(dx, dy)


def flow_wheel(flow):
    """the reference's convention (utils/visualize_utils.py): Hh = trunc(angle / 2), S = 255, V = trunc(clip(32 |flow|, 0, 255))"""
    half, v32 = wheel_parts(flow)
    return hsv_to_rgb(np.minimum(np.trunc(half), 179).astype(np.int64), np.trunc(np.clip(v32, 0, 255)).astype(np.int64))


def nearest(img, H, W):
    """(n, h, w, ...) -> (n, H, W, ...), src = dst * side_in // side_out"""
    h, w = img.shape[1:3]
    return img[:, (np.arange(H) * h) // H][:, :, (np.arange(W) * w) // W]


def wheel_band(flow, eps=1e-3):
    """True where the reference's angle / 2 or 32 |flow| (below saturation) lies within eps of an integer"""
    half, v32 = wheel_parts(flow)
    near = lambda a: np.abs(a - np.rint(a)) < eps
    return near(half) | (near(v32) & (v32 < 255 + eps))


def pooled(pred):
    """the token means of dx and dy: (n, g g, 2 f f) -> (n, g, g, 2) float64"""
    pred = np.asarray(pred, dtype=np.float64)
    n, L, D = pred.shape
    g = int(round(L ** 0.5))
    return pred.reshape(n, g, g, 2, D // 2).mean(axis=-1)


def dilate3(mask):
    """OR over the 3 x 3 neighbourhood inside the grid, (n, g, g) bool"""
    n, g, _ = mask.shape
    pad = np.zeros((n, g + 2, g + 2), dtype=bool)
    pad[:, 1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + g, dx:dx + g]
    return out


def motion_mask(pred, thr=1.0, dilate=False):
    """-> (mask (n, g, g) bool, q = mx^2 + my^2 (n, g, g) float64)"""
    m = pooled(pred)
    q = m[..., 0] ** 2 + m[..., 1] ** 2
    mask = q > thr * thr
    return (dilate3(mask) if dilate else mask), q


def mask_trusted(q, thr, dilate, rel=1e-5):
    """where the mask does not hinge on a token whose q lies within rel thr^2 of thr^2 (with dilation: none of the 3 x 3)"""
    close = np.abs(q - thr * thr) <= rel * thr * thr
    return ~(dilate3(close) if dilate else close)


# ---------------------------------------------------------------------------------------------------
# overlay
# ---------------------------------------------------------------------------------------------------
def denorm_levels(current):
    """current (n, 3, H, W) -> 255 clamp(x std + mean, 0, 1) in float64, HWC, before rounding"""
    x = np.asarray(current, dtype=np.float64)
    mean = np.asarray(CLIP_MEAN, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    std = np.asarray(CLIP_STD, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    return (np.clip(x * std + mean, 0, 1) * 255).transpose(0, 2, 3, 1)


def blend(frame_u8, mask, tint=(255, 64, 0), alpha=96):
    """frame (n, H, W, 3) uint8, mask (n, g, g): masked cells -> (v (256 - a) + tint a + 128) >> 8"""
    n, H, W, _ = frame_u8.shape
    big = nearest(np.asarray(mask).astype(bool), H, W)[..., None]
    v = frame_u8.astype(np.int64)
    mixed = (v * (256 - alpha) + np.asarray(tint, dtype=np.int64) * alpha + 128) >> 8
    return np.where(big, mixed, v).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------------
def feature_levels(x, W, b, lo, hi):
    """x (n, L, D), W (D, 3), b / lo / hi (3): everything widened to float64 -> (u = 255 clamp((x W + b - lo) / (hi - lo), 0, 1)
    before rounding, (n, L, 3); delta (n, L, 3) = 255 (D + 4) 2^-24 sum_d |x_d W[d, k]| / (hi_k - lo_k), the fp32 accumulation bound)"""
    x, W = np.asarray(x, dtype=np.float64), np.asarray(W, dtype=np.float64)
    b, lo, hi = (np.asarray(a, dtype=np.float64) for a in (b, lo, hi))
    p = x @ W + b
    u = 255.0 * np.clip((p - lo) / (hi - lo), 0, 1)
    delta = 255.0 * (x.shape[-1] + 4) * 2.0 ** -24 * (np.abs(x) @ np.abs(W)) / (hi - lo)
    return u, delta


def token_blocks(img, H, W):
    """(n, g g, 3) -> (n, H, W, 3), nearest: token = pixel * g // side"""
    n, L, c = img.shape
    g = int(round(L ** 0.5))
    return nearest(img.reshape(n, g, g, c), H, W)
