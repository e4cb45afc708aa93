"""Float64 numpy restatement of the dream-scoring metrics (dreamvla_amd/csrc/dream_score.hip), written from their definitions:
the checker of tests/test_dream_score.py and tests/test_dream_score_gpu.py.

SSIM (Wang, Bovik, Sheikh, Simoncelli 2004): 11 x 11 Gaussian window, sigma 1.5, weights normalised to sum 1; C1 = (0.01 * 255)^2,
C2 = (0.03 * 255)^2; weighted population (co)variances; the map at the (H - 10) x (W - 10) positions whose window lies inside the
image; each channel on its own; the mean over positions and channels.
Depth: over the pixels with target > 0, p = max(pred, 0): abs-rel, RMSE, SiLog (d = log(t + 1e-6) - log(p + 1e-6),
sqrt(mean d^2 - 0.5 mean(d)^2)), the share with max(p / t, t / p) < 1.25."""
import numpy as np

WIN, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def gaussian_window():
    """the 11 normalised 1-D weights; the 2-D window is their outer product (and sums to 1 as they do)"""
    x = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2
    w = np.exp(-x * x / (2 * SIGMA * SIGMA))
    return w / w.sum()


def _filter_valid(img, w):
    """(H, W) float64 -> (H - 10, W - 10): the separable window at the positions where it lies inside"""
    H, W = img.shape
    rows = sum(w[k] * img[:, k:k + W - WIN + 1] for k in range(WIN))
    return sum(w[k] * rows[k:k + H - WIN + 1, :] for k in range(WIN))


def ssim_map(x, y):
    """one channel, (H, W) of anything castable to float64 -> the SSIM map (H - 10, W - 10)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w = gaussian_window()
    ux, uy = _filter_valid(x, w), _filter_valid(y, w)
    vx = _filter_valid(x * x, w) - ux * ux
    vy = _filter_valid(y * y, w) - uy * uy
    vxy = _filter_valid(x * y, w) - ux * uy
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim(a, b):
    """a, b (H, W, C) uint8 -> the mean over channels of the per-channel mean SSIM"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[0] >= WIN and a.shape[1] >= WIN
    return float(np.mean([ssim_map(a[..., c], b[..., c]).mean() for c in range(a.shape[-1])]))


def image_quality(a, b):
    """a, b (n, H, W, 3) uint8 -> {"sse": int64 (n,), "mse", "psnr", "ssim": float64 (n,)}"""
    a, b = np.asarray(a), np.asarray(b)
    d = a.astype(np.int64) - b.astype(np.int64)
    sse = (d * d).reshape(len(a), -1).sum(axis=1)
    mse = sse / float(a[0].size)
    with np.errstate(divide="ignore"):
        psnr = np.where(sse == 0, np.inf, 10 * np.log10(255.0 ** 2 / np.where(sse == 0, 1.0, mse)))
    return {"sse": sse, "mse": mse, "psnr": psnr, "ssim": np.array([ssim(x, y) for x, y in zip(a, b)], dtype=np.float64)}


def depth_quality(pred, target):
    """pred, target (n, H, W) float32 -> {"valid", "delta1_count": int64 (n,), "abs_rel", "rmse", "silog", "delta1": float64 (n,)},
    NaN metrics where no pixel is valid.  The float32 inputs are taken as they are; all arithmetic in float64."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    out = {k: [] for k in ("valid", "delta1_count", "abs_rel", "rmse", "silog", "delta1")}
    for p, t in zip(pred, target):
        m = t > 0
        p, t = np.maximum(p[m], 0.0), t[m]
        n = int(m.sum())
        out["valid"].append(n)
        if n == 0:
            out["delta1_count"].append(0)
            for k in ("abs_rel", "rmse", "silog", "delta1"):
                out[k].append(np.nan)
            continue
        with np.errstate(divide="ignore"):
            ratio = np.maximum(p / t, t / p)
        d = np.log(t + 1e-6) - np.log(p + 1e-6)
        cnt = int((ratio < 1.25).sum())
        out["delta1_count"].append(cnt)
        out["abs_rel"].append(np.mean(np.abs(p - t) / t))
        out["rmse"].append(np.sqrt(np.mean((p - t) ** 2)))
        out["silog"].append(np.sqrt(np.mean(d * d) - 0.5 * np.mean(d) ** 2))
        out["delta1"].append(cnt / n)
    return {k: np.array(v, dtype=np.int64 if k in ("valid", "delta1_count") else np.float64) for k, v in out.items()}


def min_ratio_gap(pred, target):
    """how close any valid pixel's max(p / t, t / p) comes to the 1.25 threshold (the GPU test keeps its inputs 1e-4 away)"""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    m = target > 0
    p, t = np.maximum(pred[m], 0.0), target[m]
    if p.size == 0:
        return np.inf
    with np.errstate(divide="ignore"):
        return float(np.min(np.abs(np.maximum(p / t, t / p) - 1.25)))
