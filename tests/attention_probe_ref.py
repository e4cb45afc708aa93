"""float64 restatement of the attention probe (csrc/attention_probe.hip, ops.attention_probe) and of the pure-torch helpers
built on it (ops.attention_mass, ops.attention_rollout, ops.patch_heat).  numpy only, importable without a GPU, written from the
definitions and not from the code under test.

probabilities(): softmax over the VISIBLE keys of scale * q k^T from the same bf16 values, exact zeros where the kernel promises
them (a key the row cannot see, a row that sees nothing, a row number outside [0, Lq)), then the head mean.  It also returns what
the derived error bound needs (bound()).

The bound, per element of the probe's output (u = 2^-24, the unit roundoff of fp32):

    |p - p*| <= p* (2 e_s + c u)  [+ H u in the issue's statement for the head mean, see below]

  e_s  error of a computed score.  The kernel accumulates <q, k> with fp32 FMAs (the bf16 products are exact in fp32's 24 bits only
       up to the first addition, so every FMA rounds once), at most 16 in a lane, then three additions across the eight lanes of a
       key, then one multiplication by `scale`.  Counting the roundings on the longest path of the widths in use: D = 8: 8 + 0 + 1
       (one lane holds data, adding the other lanes' zeros is exact); D = 16: 8 + 1 + 1; D >= 24: at most 16 + 3 + 1 = 20 <= D + 2.
       So |s - s*| <= (D + 2) u scale sum_i |q_i k_i| <= e_s := (D + 2) u scale max_k sum_i |q_i k_i|.
       A softmax is unchanged by a shift common to all scores, so score errors within +-e_s move every probability by a factor
       within exp(+-2 e_s): relative 2 e_s, and a second-order term below (2 e_s)^2 <= 4e-8 < u, which is counted in c.
  c    everything after the scores, relative:  t = s - max s rounds once, an absolute error of at most T u in the exponent where
       T = max (max s - s) over the visible keys of the row, i.e. a relative T u in exp(t);  expf is within 1 ulp = 2 u;  the row
       sum adds positive terms: a lane's chain over the tiles of its wave (every fourth live tile, four terms each), three additions
       across the eight groups of the wave and two across the four waves -- never more roundings than one lane walking all the
       tiles, ceil(Lk / 8), plus three (adding the zero of an empty wave or lane is exact): relative (ceil(Lk / 8) + 3) u on top
       of its terms' (T + 2) u;  the division is correctly rounded on the hardware path the compiler emits, counted as 4 u to be safe
       of that.  Numerator (T + 2), denominator (T + 2) + ceil(Lk / 8) + 3, division 4, second order 1:
           c = 2 T + ceil(Lk / 8) + 12.
  H u  the head mean adds H probabilities in fp32 and divides once: H - 1 additions of positive terms and a division, relative
       H u of the mean itself.  The issue states this term as an absolute H u (p* <= 1); bound() keeps it relative, H u p*, which
       is never larger, and with it the whole bound stays below the issue's cap 1e-3 p* + 1e-7 for 16 heads as well.
With per_head there is no head mean and no H u term; the head mean's bound is the mean of the heads' bounds plus H u p*."""
import math

import numpy as np

U = 2.0 ** -24


def probabilities(q, k, rows, scale, vis=None):
    """q (B, Lq, H, D), k (B, Lk, H, D): float arrays holding bf16 values; rows (B, R) ints; vis: boolean (Lq, Lk) or None.
    -> dict(per_head (B, H, R, Lk) float64, mean (B, R, Lk), abs_dot (B, H, R) = scale max_k sum_i |q_i k_i| over the visible keys,
    spread (B, H, R) = T, flash_sum (B, H, R) = sum_j 2^(s_j log2 e - M) with M = ceil(max_j s_j log2 e): the unnormalised row sum of
    the product kernels' softmax, whose probabilities enter P.V as bf16(2^(s_j log2 e - M)) = bf16(p_j * flash_sum) -- what
    oracle/torch_ref.py::attention_bf16 restates; 0 for a row that sees nothing)."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    rows = np.asarray(rows)
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    R = rows.shape[1]
    P = np.zeros((B, H, R, Lk))
    abs_dot = np.zeros((B, H, R))
    spread = np.zeros((B, H, R))
    flash_sum = np.zeros((B, H, R))
    for b in range(B):
        for r in range(R):
            row = int(rows[b, r])
            if row < 0 or row >= Lq:
                continue
            see = np.ones(Lk, dtype=bool) if vis is None else np.asarray(vis[row], dtype=bool)
            if not see.any():
                continue
            for h in range(H):
                prod = q[b, row, h][None, :] * k[b, see, h]             # (n_visible, D)
                s = scale * prod.sum(axis=1)
                e = np.exp(s - s.max())
                P[b, h, r, see] = e / e.sum()
                abs_dot[b, h, r] = abs(scale) * np.abs(prod).sum(axis=1).max()
                spread[b, h, r] = s.max() - s.min()
                s2 = s * 1.4426950408889634
                flash_sum[b, h, r] = np.exp2(s2 - np.ceil(s2.max())).sum()
    return {"per_head": P, "mean": P.sum(axis=1) / H, "abs_dot": abs_dot, "spread": spread, "flash_sum": flash_sum}


def bound(ref, D, Lk, per_head):
    """the derived bound (module docstring) for every element of the probe's output, from what probabilities() returned; `Lk`: the
    number of keys on the kernel's (compacted) key axis."""
    H = ref["per_head"].shape[1]
    e_s = (D + 2) * U * ref["abs_dot"]                                    # (B, H, R)
    c = 2.0 * ref["spread"] + math.ceil(Lk / 8) + 12.0
    rel = (2.0 * e_s + c * U)[..., None]
    per = ref["per_head"] * rel
    if per_head:
        return per
    return per.sum(axis=1) / H + H * U * ref["mean"]


def issue_cap(p_star):
    """what the derived bound has to stay below for the test inputs (unit-normal q and k): a looser bound would hide errors"""
    return 1e-3 * p_star + 1e-7


def attention_mass(maps, groups, S):
    maps = np.asarray(maps, dtype=np.float64)
    L = maps.shape[-1]
    blk = L // S
    out = np.zeros(maps.shape[:-1] + (S, len(groups)))
    for s in range(S):
        for gi, (_, start, count) in enumerate(groups):
            for j in range(count):
                out[..., s, gi] += maps[..., s * blk + start + j]
    return out


def rollout(layer_maps, n_media):
    """layer_maps (n_layers, n_lat, n_media + n_lat) -> (n_lat, n_media): R_0 = 0, R_l = R_{l-1} / 2 + (M_l + T_l R_{l-1}) / 2"""
    layer_maps = np.asarray(layer_maps, dtype=np.float64)
    n_lat = layer_maps.shape[1]
    R = np.zeros((n_lat, n_media))
    for A in layer_maps:
        M, T = A[:, :n_media], A[:, n_media:]
        new = np.zeros_like(R)
        for i in range(n_lat):
            new[i] = 0.5 * R[i] + 0.5 * (M[i] + sum(T[i, j] * R[j] for j in range(n_lat)))
        R = new
    return R


def patch_heat(trunk, resampler, groups, position):
    """trunk (B, n_layers, R, L); resampler (2 * B * F, n_res, n_lat, n_patch + n_lat), primary views first, F = 1 or S frames per
    sequence; position: one int per sequence -> (B, 2, g, g)"""
    trunk, resampler = np.asarray(trunk, dtype=np.float64), np.asarray(resampler, dtype=np.float64)
    B, L = trunk.shape[0], trunk.shape[-1]
    blk = max(start + count for _, start, count in groups)
    F = resampler.shape[0] // (2 * B)
    n_lat = resampler.shape[2]
    n_patch = resampler.shape[3] - n_lat
    g = int(round(math.sqrt(n_patch)))
    where = {name: (start, count) for name, start, count in groups}
    heat = np.zeros((B, 2, n_patch))
    for b in range(B):
        p = int(position[b])
        for v, name in enumerate(("image_primary", "image_wrist")):
            start, _ = where[name]
            frame = v * B * F + b * F + (p if F > 1 else 0)
            roll = rollout(resampler[frame], n_patch)
            for i in range(n_lat):
                w = trunk[b, :, :, p * blk + start + i].mean()
                heat[b, v] += w * roll[i]
            tot = heat[b, v].sum()
            heat[b, v] = heat[b, v] / tot if tot > 0 else 0.0
    return heat.reshape(B, 2, g, g)
