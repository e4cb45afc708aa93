"""MaskedAutoencoderViT on the HIP kernels -- host-side mirror of the reference's models/vit_mae.py.

Same constructor, parameter names and shapes as the reference `MaskedAutoencoderViT`, and the same methods: patchify /
unpatchify, random_masking, forward_encoder, forward_decoder, forward_loss and forward (MAE pretraining).  DreamVLA calls only
`forward_encoder(x, mask_ratio=0.0)` (dreamvla_model.py:672-673).  The masking, the decoder's token un-shuffle and the loss are
one kernel each (csrc/mae.hip); the blocks are the same fused blocks as everywhere else (decoder head_dim 32 runs on
csrc/attention_hd.hip).

Deviations (documented in DESIGN.md):
  * `random_masking(x, 0.0)` in the reference (vit_mae.py:157-182,194) keeps all patch tokens but in a random per-sample order,
    and DreamVLA drops `ids_restore`.  Attention without positional terms after the embedding is permutation-equivariant, so
    the un-shuffled result is identical up to fp rounding (<= 6e-6 fp32).  `forward_encoder(x, 0.0)`
    keeps patch order (ids_restore = identity) and consumes no RNG.
  * mask_ratio > 0: ids_shuffle is the STABLE ascending order of the noise (ties broken by index); the reference's
    torch.argsort is not stable, so exact ties in the noise (about one sample in a thousand at L = 196) may order differently.
  * `noise=` (random_masking, forward_encoder, forward) supplies the (N, L) fp32 noise instead of drawing torch.rand(N, L).
"""
from functools import partial

import numpy as np
import torch
from torch import nn

from . import ops
from . import preprocess as P
from .nn import Block, LayerNorm, Linear, PatchEmbed


# ---- fixed 2-D sin-cos position tables (numpy float32 -> identical bits to vit_mae.py:8-53) -----------
def get_1d_sincos_pos_embed_from_grid(embed_dim, pos):
    assert embed_dim % 2 == 0
    omega = np.arange(embed_dim // 2, dtype=np.float32)
    omega /= embed_dim / 2.
    omega = 1. / 10000 ** omega
    pos = pos.reshape(-1)
    out = np.einsum('m,d->md', pos, omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def get_2d_sincos_pos_embed_from_grid(embed_dim, grid):
    assert embed_dim % 2 == 0
    emb_h = get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[0])
    emb_w = get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[1])
    return np.concatenate([emb_h, emb_w], axis=1)


def get_2d_sincos_pos_embed(embed_dim, grid_size, cls_token=False):
    grid_h = np.arange(grid_size, dtype=np.float32)
    grid_w = np.arange(grid_size, dtype=np.float32)
    grid = np.meshgrid(grid_w, grid_h)  # w goes first (as in the reference)
    grid = np.stack(grid, axis=0).reshape([2, 1, grid_size, grid_size])
    pos_embed = get_2d_sincos_pos_embed_from_grid(embed_dim, grid)
    if cls_token:
        pos_embed = np.concatenate([np.zeros([1, embed_dim]), pos_embed], axis=0)
    return pos_embed


class MaskedAutoencoderViT(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=1024, depth=24, num_heads=16,
                 decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16, mlp_ratio=4.,
                 norm_layer=LayerNorm, norm_pix_loss=False):
        super().__init__()
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim), requires_grad=False)
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias=True, norm_layer=norm_layer)
                                     for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        # MAE decoder half (pretraining only: DreamVLA never runs it, but its tensors are part of the checkpoint)
        self.decoder_embed = Linear(embed_dim, decoder_embed_dim, bias=True)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, decoder_embed_dim), requires_grad=False)
        self.decoder_blocks = nn.ModuleList([Block(decoder_embed_dim, decoder_num_heads, mlp_ratio, qkv_bias=True,
                                                   norm_layer=norm_layer) for _ in range(decoder_depth)])
        self.decoder_norm = norm_layer(decoder_embed_dim)
        self.decoder_pred = Linear(decoder_embed_dim, patch_size ** 2 * in_chans, bias=True)
        self.norm_pix_loss = norm_pix_loss
        self.initialize_weights()

    def initialize_weights(self):
        gs = int(self.patch_embed.num_patches ** .5)
        pos_embed = get_2d_sincos_pos_embed(self.pos_embed.shape[-1], gs, cls_token=True)
        self.pos_embed.data.copy_(torch.from_numpy(pos_embed).float().unsqueeze(0))
        dpe = get_2d_sincos_pos_embed(self.decoder_pos_embed.shape[-1], gs, cls_token=True)
        self.decoder_pos_embed.data.copy_(torch.from_numpy(dpe).float().unsqueeze(0))
        w = self.patch_embed.proj.weight.data
        torch.nn.init.xavier_uniform_(w.view([w.shape[0], -1]))
        torch.nn.init.normal_(self.cls_token, std=.02)
        torch.nn.init.normal_(self.mask_token, std=.02)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def patchify(self, imgs):
        """imgs (N, 3, H, W) -> (N, L, p*p*3)"""
        p = self.patch_embed.patch_size[0]
        assert imgs.shape[2] == imgs.shape[3] and imgs.shape[2] % p == 0
        h = w = imgs.shape[2] // p
        x = imgs.reshape(shape=(imgs.shape[0], 3, h, p, w, p))
        x = torch.einsum('nchpwq->nhwpqc', x)
        return x.reshape(shape=(imgs.shape[0], h * w, p ** 2 * 3))

    def unpatchify(self, x):
        """(N, L, p*p*3) -> imgs (N, 3, H, W)"""
        p = self.patch_embed.patch_size[0]
        h = w = int(x.shape[1] ** .5)
        assert h * w == x.shape[1]
        x = x.reshape(shape=(x.shape[0], h, w, p, p, 3))
        x = torch.einsum('nhwpqc->nchpwq', x)
        return x.reshape(shape=(x.shape[0], 3, h * p, h * p))

    def random_masking(self, x, mask_ratio, noise=None):
        """x (N, L, D) -> x_masked (N, len_keep, D), mask (N, L) (1 = removed), ids_restore (N, L); one kernel (ops.mae_random_masking)"""
        N, L, D = x.shape
        len_keep = int(L * (1 - mask_ratio))
        if noise is None:
            noise = torch.rand(N, L, device=x.device)
        return ops.mae_random_masking(x, noise, len_keep)

    def forward_encoder(self, x, mask_ratio, noise=None):
        """x: (n, 3, H, W) -> latent (n, 1 + len_keep, embed_dim), mask (n, L), ids_restore (n, L).  mask_ratio 0.0 (DreamVLA's
        frozen encoder): all patches in patch order, mask zeros, ids_restore identity, no RNG."""
        if mask_ratio == 0.0:
            return self._encode_all(x)
        n = x.shape[0]
        L = self.patch_embed.num_patches
        x = self.patch_embed(x, pos=self.pos_embed[0, 1:, :])
        len_keep = int(L * (1 - mask_ratio))
        if noise is None:
            noise = torch.rand(n, L, device=x.device)
        # masking, the cls row and its position in one gather pass; the cls row's gradient is the column sum of row 0
        x, mask, ids_restore = ops.mae_random_masking(x, noise, len_keep, cls_row=self.cls_token + self.pos_embed[:, :1, :])
        for blk in self.blocks:
            x = blk(x)
        x = self.norm(x)
        return x, mask, ids_restore

    def _decode(self, x, ids_restore):
        """forward_decoder with the cls row kept: (N, 1 + L, p*p*3)"""
        x = self.decoder_embed(x)
        x = ops.mae_unshuffle(x, self.mask_token, ids_restore, self.decoder_pos_embed)
        for blk in self.decoder_blocks:
            x = blk(x)
        x = self.decoder_norm(x)
        return self.decoder_pred(x)

    def forward_decoder(self, x, ids_restore):
        """latent (N, 1 + len_keep, embed_dim) -> pred (N, L, p*p*3)"""
        return self._decode(x, ids_restore)[:, 1:, :]

    def forward_loss(self, imgs, pred, mask):
        """imgs (N, 3, H, W), pred (N, L, p*p*3), mask (N, L) -> mean loss on the removed patches (patchify fused in)"""
        return ops.mae_loss(pred, imgs, mask, self.patch_embed.patch_size[0], self.norm_pix_loss)

    def forward(self, imgs, mask_ratio=0.75, noise=None):
        latent, mask, ids_restore = self.forward_encoder(imgs, mask_ratio, noise=noise)
        full = self._decode(latent, ids_restore)
        # the loss reads rows 1..L of the decoder output in place; its gradient comes back with the cls rows zero
        loss = ops.mae_loss(full, imgs, mask, self.patch_embed.patch_size[0], self.norm_pix_loss)
        return loss, full[:, 1:, :], mask

    def _encode_all(self, x):
        n = x.shape[0]
        L = self.patch_embed.num_patches
        # patch-embed GEMM + bias; the fixed pos-embed add rides in the residual slot of the epilogue
        x = self.patch_embed(x, pos=self.pos_embed[0, 1:, :])
        cls_token = (self.cls_token + self.pos_embed[:, :1, :]).to(x.dtype)
        if x.dtype == torch.bfloat16 and not torch.is_grad_enabled():
            D = x.shape[-1]       # the frozen encoder of DreamVLA: one gather-write pass instead of torch.cat
            x = ops.assemble_tokens([cls_token.reshape(1, 1, 1, D).expand(n, 1, 1, D), x.reshape(n, 1, L, D)]).view(n, L + 1, D)
        else:
            x = torch.cat((cls_token.expand(n, -1, -1), x), dim=1)
        for blk in self.blocks:
            x = blk(x)
        x = self.norm(x)
        mask = torch.zeros(n, L, device=x.device)
        ids_restore = torch.arange(L, device=x.device).unsqueeze(0).expand(n, -1)
        return x, mask, ids_restore


class MAEFrameAugment:
    """The input side of MAE pretraining on the device: RandomResizedCrop(n_px, scale, ratio, BICUBIC) + RandomHorizontalFlip +
    ToTensor + Normalize of the MAE recipe, from raw uint8 frames to the `imgs` of `MaskedAutoencoderViT.forward`:

        augment = MAEFrameAugment()
        loss, pred, mask = mae(augment(frames_u8), mask_ratio=0.75)       # frames_u8 (n, h, w, 3) uint8 on the device

    One call = one draw of the boxes on the host (`preprocess.draw_resized_crops`, the algorithm of torchvision's get_params on
    this package's own random stream: DESIGN.md section 5), one upload of the (n, 5) descriptors and one launch of
    csrc/image_resized_crop.hip, whose bytes are Pillow's.  mean / std default to CLIP's: that is what DreamVLA's encoder, which
    the pretrained weights are loaded into (`vit_checkpoint_path`), is fed by `preprocess_frames`.  `last_crops` keeps the
    descriptors of the latest call."""

    def __init__(self, n_px=224, scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, mean=P.CLIP_MEAN, std=P.CLIP_STD, generator=None):
        self.n_px, self.scale, self.ratio, self.p_flip = int(n_px), tuple(scale), tuple(ratio), float(p_flip)
        self.mean, self.std = tuple(mean), tuple(std)
        self.generator = generator
        self.last_crops = None

    def __call__(self, frames_u8):
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
            raise ValueError("MAEFrameAugment: frames (n, h, w, 3) expected")
        n, h, w = frames_u8.shape[:3]
        self.last_crops = P.draw_resized_crops(n, h, w, self.scale, self.ratio, self.p_flip, generator=self.generator)
        return P.resized_crop(frames_u8, self.last_crops, self.n_px, self.mean, self.std)
