"""Palettes of the dream pictures (kernels: csrc/dream_view.hip, operators: ops.depth_colorize / ops.feature_render).

`depth_palette()`: 256 colours from a closed-form expression (Green's cubehelix, Bull. Astr. Soc. India 39, 289, 2011): lightness
rises monotonically with the index, so the picture survives a grey-scale print, and no colour-map table is stored anywhere.

`FeaturePalette`: three FIXED directions of a feature space, fitted once; every DINO / SAM picture made with it means the same."""
import math

import torch

_DEPTH_PALETTES = {}


def depth_palette(device=None, start=0.5, rotations=-1.5, hue=1.2, gamma=1.0):
    """(256, 3) uint8.  With t = (i / 255)^gamma, phi = 2 pi (start / 3 + 1 + rotations t) and a = hue t (1 - t) / 2:
        r = t + a (-0.14861 cos phi + 1.78277 sin phi)
        g = t + a (-0.29227 cos phi - 0.90649 sin phi)
        b = t + a ( 1.97294 cos phi)
    clamped to [0, 1], times 255, rounded half to even; evaluated in float64.  The default arguments are cached per device."""
    key = (str(device), start, rotations, hue, gamma)
    if key not in _DEPTH_PALETTES:
        t = (torch.arange(256, dtype=torch.float64) / 255.0) ** gamma
        phi = 2.0 * math.pi * (start / 3.0 + 1.0 + rotations * t)
        a = hue * t * (1.0 - t) / 2.0
        c, s = torch.cos(phi), torch.sin(phi)
        rgb = torch.stack((t + a * (-0.14861 * c + 1.78277 * s), t + a * (-0.29227 * c - 0.90649 * s), t + a * (1.97294 * c)), dim=1)
        pal = torch.round(rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
        _DEPTH_PALETTES[key] = pal if device is None else pal.to(device)
    return _DEPTH_PALETTES[key]


class FeaturePalette:
    """Three fixed directions of a feature space and the range of each: token features -> RGB (ops.feature_render).

    The palette is FIXED, not a PCA of the frame that is being drawn: a per-frame PCA re-orders and flips its axes from one control
    step to the next, so its colours mean nothing across steps.  Fit one palette once -- for instance on the dataset's DINO or SAM
    label features -- and the same colour means the same feature direction at every control step, and for a label and the dream
    of it alike.

    `fit(features, quantiles=(0.01, 0.99))`: features (..., D), any float dtype or device; everything in float64: the mean, the
    three eigenvectors of the covariance with the largest eigenvalues (torch.linalg.eigh), in descending order of eigenvalue, each
    signed so that its entry of largest magnitude is positive, and per direction the `quantiles` of the centred features'
    projections (linear interpolation between order statistics) as `lo` / `hi`.
    The kernel's operands: W (D, 3) fp32 = the directions rounded once, b (3) = -mean . direction evaluated in float64 and rounded
    once, lo / hi rounded once; byte_k = rint(255 clamp((x . W[:, k] + b_k - lo_k) / (hi_k - lo_k), 0, 1))."""

    def __init__(self, mean, components, lo, hi, device=None):
        self.mean = torch.as_tensor(mean, dtype=torch.float64).detach().cpu().clone()
        self.components = torch.as_tensor(components, dtype=torch.float64).detach().cpu().clone()
        self.lo = torch.as_tensor(lo, dtype=torch.float64).detach().cpu().clone()
        self.hi = torch.as_tensor(hi, dtype=torch.float64).detach().cpu().clone()
        D = self.mean.numel()
        if self.mean.dim() != 1 or tuple(self.components.shape) != (3, D) or tuple(self.lo.shape) != (3,) or tuple(self.hi.shape) != (3,):
            raise ValueError("FeaturePalette: mean (D,), components (3, D), lo (3,), hi (3,)")
        self.dim = D
        self.device = torch.device("cpu") if device is None else torch.device(device)
        # the kernel's operands: the matrix on the device, the nine scalars on the host (they are kernel arguments)
        self.W = self.components.t().contiguous().to(torch.float32).to(self.device)
        self.b = tuple(float(v) for v in (-(self.components @ self.mean)).to(torch.float32))
        self.lo32 = tuple(float(v) for v in self.lo.to(torch.float32))
        self.hi32 = tuple(float(v) for v in self.hi.to(torch.float32))

    @classmethod
    def fit(cls, features, quantiles=(0.01, 0.99)):
        q_lo, q_hi = float(quantiles[0]), float(quantiles[1])
        if not 0.0 <= q_lo < q_hi <= 1.0:
            raise ValueError("FeaturePalette.fit: quantiles (low, high) with 0 <= low < high <= 1")
        if not isinstance(features, torch.Tensor) or features.dim() < 2:
            raise ValueError("FeaturePalette.fit: features (..., D)")
        x = features.detach().reshape(-1, features.shape[-1]).to(torch.float64)
        N, D = x.shape
        if D < 3 or N < 2:
            raise ValueError("FeaturePalette.fit: at least 2 rows of at least 3 features")
        mean = x.mean(dim=0)
        xc = x - mean
        cov = (xc.t() @ xc) / (N - 1)
        _, vec = torch.linalg.eigh(cov)                      # ascending eigenvalues
        comp = vec[:, [D - 1, D - 2, D - 3]].t().contiguous()
        big = comp.abs().argmax(dim=1)
        comp = comp * torch.sign(comp[torch.arange(3), big]).unsqueeze(1)
        proj, _ = (xc @ comp.t()).sort(dim=0)

        def quantile(q):
            pos = q * (N - 1)
            i = min(int(math.floor(pos)), N - 2)
            return proj[i] + (proj[i + 1] - proj[i]) * (pos - i)
        return cls(mean, comp, quantile(q_lo), quantile(q_hi), device=features.device)

    def state_dict(self):
        return {"mean": self.mean.clone(), "components": self.components.clone(), "lo": self.lo.clone(), "hi": self.hi.clone()}

    def load_state_dict(self, state):
        self.__init__(state["mean"], state["components"], state["lo"], state["hi"], device=self.device)
        return self

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(state["mean"], state["components"], state["lo"], state["hi"], device=device)

    def to(self, device):
        return FeaturePalette(self.mean, self.components, self.lo, self.hi, device=device)
