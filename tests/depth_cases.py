"""Depth maps shared by tests/test_depth_pipeline.py, tests/test_depth_pipeline_gpu.py and tests/gpu_label_path_perf.py: fp32 data a
resize + cast can get wrong -- metres in [0, 5) like CALVIN's depth, mixed with 0, -0, fp32 denormals, +-inf and values whose low 16
bits are 0x8000 (a tie under the bf16 rounding, over even and odd upper halves) or one off a tie (0x7FFF / 0x8001).  No NaN: a NaN's
payload is not a property of the resize."""
import numpy as np
import torch

SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000400, 0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000,
                    0x3F807FFF, 0x3F808001, 0x40A17FFF, 0xC0A18000, 0x7F7FFFFF, 0x00800000, 0x3F7F8000], dtype=np.uint32)


def depth_maps(n, h, w, seed=0):
    """(n, h, w) fp32 CPU tensor; the same seed gives the same maps"""
    rng = np.random.RandomState(1000 * seed + 7 * h + w + n)
    bits = rng.uniform(0, 5, (n, h, w)).astype(np.float32).view(np.uint32).copy()
    kind = rng.randint(0, 16, bits.shape)
    bits[kind == 0] = (bits[kind == 0] & 0xFFFF0000) | 0x8000                      # ties
    bits[kind == 1] = (bits[kind == 1] & 0xFFFF0000) | rng.choice([0x7FFF, 0x8001], int((kind == 1).sum())).astype(np.uint32)
    pick = kind == 2
    bits[pick] = SPECIAL[rng.randint(0, len(SPECIAL), int(pick.sum()))]
    flat = bits.reshape(-1)
    if flat.size >= 2 * len(SPECIAL):                                              # every special value at least once
        flat[rng.choice(flat.size, len(SPECIAL), replace=False)] = SPECIAL
    return torch.from_numpy(bits.view(np.float32))


def shift_rows(n, pad, seed=0):
    """(n, 2) int32 (sx, sy): rows at both extremes (0 and 2 pad, in every combination) first, random rows behind them"""
    g = torch.Generator().manual_seed(seed)
    sh = torch.randint(0, 2 * pad + 1, (n, 2), generator=g, dtype=torch.int32)
    edge = torch.tensor([[0, 0], [2 * pad, 2 * pad], [0, 2 * pad], [2 * pad, 0]], dtype=torch.int32)
    k = min(n, 4)
    sh[:k] = edge[:k]
    return sh


def bits(t):
    """the tensor's bit patterns, for exact comparison (0.0 == -0.0 and inf arithmetic play no part)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
