"""Fixture of the three patch helpers the dream render is built on (CPU, from the REAL reference; needs the reference sources, so
it is run by hand and its output is committed under tests/golden/):

    python -m tests.make_golden_dream          # writes tests/golden/dream_render.pt

`patchify`, `normalize_patchfied_image` and `unpatchify` of utils/train_utils.py (37-57, 783-799) are run on two small frames
(3 x 64 x 64: a 4 x 4 grid of 16 x 16 patches, values in the range of CLIP-normalised pixels) and one depth map (64 x 64).  The
file holds inputs and results only; tests/test_dream_render.py pins the torch restatement of the render (tests/dream_checks.py)
to them and reads nothing else."""
import os

import torch

from oracle import ref_loader

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATCH, SIDE = 16, 64


def frames(seed=20):
    """two frames as the model sees them: smooth 0..255 pictures with noise, ToTensor + CLIP Normalize"""
    from dreamvla_amd.preprocess import CLIP_MEAN, CLIP_STD
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, SIDE), torch.linspace(0, 1, SIDE), indexing="ij")
    out = []
    for k in range(2):
        base = torch.stack([(0.5 + 0.5 * torch.sin(6.0 * (k + 1) * xx + c)) * (0.3 + 0.7 * yy) for c in range(3)])
        u8 = (base * 200 + 40 * torch.rand(3, SIDE, SIDE, generator=g)).clamp(0, 255).round()
        if k == 1:
            u8[:, :PATCH, :PATCH] = 255.0                    # one constant patch: variance 0, the epsilon alone under the root
        x = u8 / 255.0
        out.append((x - torch.tensor(CLIP_MEAN).view(3, 1, 1)) / torch.tensor(CLIP_STD).view(3, 1, 1))
    return torch.stack(out)


def main():
    tu = ref_loader.ref_module("utils.train_utils")
    imgs = frames()
    g = torch.Generator().manual_seed(21)
    depth_patches = torch.rand(1, 1, (SIDE // PATCH) ** 2, PATCH * PATCH, generator=g) * 3.0
    patches = tu.patchify(imgs, PATCH)
    normed = tu.normalize_patchfied_image(patches)
    fx = {
        "source": "utils/train_utils.py patchify / normalize_patchfied_image / unpatchify of the real reference (tests/make_golden_dream.py)",
        "patch": PATCH, "side": SIDE,
        "imgs": imgs, "patches": patches, "normalized": normed,
        # unpatchify takes (B, P, patches, values) and returns (B, P, C, H, W)
        "unpatchified": tu.unpatchify(patches.unsqueeze(1), PATCH, [SIDE, SIDE]),
        "unpatchified_normalized": tu.unpatchify(normed.unsqueeze(1), PATCH, [SIDE, SIDE]),
        "depth_patches": depth_patches,
        "depth_unpatchified": tu.unpatchify(depth_patches, PATCH, [SIDE, SIDE]),
    }
    path = os.path.join(GOLD, "dream_render.pt")
    torch.save(fx, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
