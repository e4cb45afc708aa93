"""The VALUE axis of the attention kernels (csrc/attention.hip, attention_hd.hip, attention_small.hip, attention_probe.hip): a
reference, seeded value regimes and the case list of tests/test_attention_values_gpu.py.  Importable without a GPU;
tests/test_attention_values.py asserts on the CPU that every case means something.

Every other attention test feeds bf16-rounded unit-normal q, k, v, dout: logits ~ N(0, 1), a nearly flat softmax, a running maximum
that moves by an integer or two per key tile, no probability that underflows and delta = rowsum(dout * o) nowhere near cancelling
against dP.  A maximum taken before the mask, a rescale skipped for one tile, a flush to zero in the wrong place or a delta formed
from the wrong o are invisible there.  The regimes here (REGIMES) are what checkpoints look like instead: one-hot rows, attention
sinks, staircases of the running maximum, mixed temperatures inside one wave, outlier channels, tiny and big magnitudes, huge logits
behind the mask, ties.

The reference.  attention_ref() restates oracle/torch_ref.py::attention_bf16 expression for expression (float32, no chunking, no
jitter, no o_stored: the same bits -- pinned by the CPU test) with four knobs:
  dtype       float64 = the reference; float32 = the yardstick variants
  o_stored    delta = rowsum(dout * o_stored) instead of the function's own o.  On a row that one key dominates P (dP - delta)
              cancels, and a single bf16 flip of the stored o moves dq / dk by tens of percent: a forward-then-backward comparison
              against an oracle that uses ITS OWN o is ill-posed exactly in the regimes that matter, and no tolerance fixes that.
              Conditioned on the o the code under test stored, the backward is a well-posed function of its inputs
  chunk       matrix products accumulated over the contracted axis in chunks of that width, in order (16: the 32x32x16 MFMA chain)
  exp_jitter  a seeded relative perturbation of every exp2 result (2^-22 ~ two ulps; raw v_exp_f32 is specified to one)
The yardstick.  yardstick(case) runs a fixed ensemble of float32 variants (chunk in {None, 8, 16, 32} x {no jitter, jitter}), judges
each against the float64 reference -- its backward against the float64 backward conditioned on that variant's own o -- and returns per
tensor E (largest rel-L2) and U (largest max-abs error in bf16 ulps of the reference's largest magnitude): what correct fp32
arithmetic with these rounding points differs by.  The kernels differ from the float64 reference by the same kinds of perturbation
(summation order in MFMA chunks, a one-ulp exp2, the lse -> log2 round trip), so they are held to
    tol = max(suite tolerance, 4 E),   k_ulp = max(suite k, 4 U)
(criterion()), and a case is admitted only if 4 E <= 1e-2 and 4 U <= 16 for every tensor (CAP_E / CAP_U, asserted per case on the
CPU): a misplaced row or tile is off by ~256 ulps.  A case that cannot meet the cap has its magnitudes changed, never its tolerance."""
import functools
import math
import zlib

import torch

from oracle import torch_ref as R
from tests import attention_mask_cases as MC

LOG2E, LN2 = R.LOG2E, R.LN2
TENSORS = ("o", "lse", "dq", "dk", "dv")
MARGIN = 4.0               # over the ensemble's own spread (draw to draw it moves by up to ~3x)
CAP_E, CAP_U = 1e-2, 16.0  # 4 E and 4 U of an admissible case
JITTER = 2.0 ** -22
ENSEMBLE = tuple((c, j) for c in (None, 8, 16, 32) for j in (0.0, JITTER))
ENSEMBLE_REDUCED = ((None, 0.0), (16, JITTER), (32, 0.0))          # the L = 2085 cases (CPU time)
GIANT = 96.0               # hidden_giant: see REGIMES


def _round(x, dtype):
    return x.to(torch.bfloat16).to(dtype)


def _mm(a, b, chunk):
    """a @ b; with `chunk` the contracted axis is cut into chunks of that width whose partial products are added in order"""
    K = a.shape[-1]
    if chunk is None or chunk >= K:
        return torch.matmul(a, b)
    acc = None
    for s in range(0, K, chunk):
        part = torch.matmul(a[..., s:s + chunk], b[..., s:s + chunk, :])
        acc = part if acc is None else acc + part
    return acc


class _Exp2:
    def __init__(self, jitter, seed, dtype):
        self.jitter, self.dtype = jitter, dtype
        self.gen = torch.Generator().manual_seed(seed) if jitter else None

    def __call__(self, x):
        y = torch.exp2(x)
        if self.gen is not None:
            y = y * (1.0 + self.jitter * (2.0 * torch.rand(y.shape, generator=self.gen, dtype=self.dtype) - 1.0))
        return y


def attention_ref(q, k, v, dout, *, dtype, o_stored=None, scale, mask=None, drop=None, drop_cols=None, batch_index=None, chunk=None,
                  exp_jitter=0.0, jitter_seed=0, mutant=None, forward=None):
    """-> dict(o, lse, dq, dk, dv, dS_absmax, o_unrounded).  (B, H, L, d) tensors holding bf16 values.  `forward`: a result of this
    function on the same inputs whose o / lse are reused (the float64 forward does not depend on o_stored).
    mutant (float32 restatements that are WRONG on purpose; tests/test_attention_values.py shows that the criterion rejects them):
      "max_before_mask"  the row maximum is taken over all keys, hidden ones included
      "skip_alpha"       online softmax over 32-key tiles in which the rescale alpha = 2^(m_old - m_new) of what has been accumulated
                         is left out at the LAST tile at which the row's running maximum rises
      "delta_unrounded"  delta from the function's own o BEFORE its bf16 rounding instead of the stored o"""
    B, H, Lq, d = q.shape
    Lk = k.shape[2]
    q, k, v, dout = q.to(dtype), k.to(dtype), v.to(dtype), dout.to(dtype)
    ex2 = _Exp2(exp_jitter, jitter_seed, dtype)
    s = _mm(q, k.transpose(-1, -2), chunk)
    s2 = s * (scale * LOG2E)
    vis = None
    unmasked = s2
    if mask is not None:
        vis = (mask == 0).expand(B, H, Lq, Lk) if mask.dim() < 4 else (mask == 0)
        s2 = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    keep = None
    inv_keep = 1.0
    if drop is not None and drop[0] > 0:
        pd, seed = drop
        rows = R._drop_rows(B, H, Lq, batch_index)
        cols = (torch.arange(Lk, dtype=torch.int64) if drop_cols is None else drop_cols.to(torch.int64)).view(1, 1, 1, Lk)
        keep = R.attn_drop_keep_mask(seed, rows, cols, pd)
        inv_keep = 1.0 / (1.0 - pd)
    if forward is None:
        m = torch.ceil((unmasked if mutant == "max_before_mask" else s2).amax(dim=-1, keepdim=True))
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = ex2(s2 - m)
        if mutant == "skip_alpha":
            p = p * _skipped_alpha_weights(s2)
        l = p.sum(dim=-1, keepdim=True)
        pdrop = p if keep is None else torch.where(keep, p, torch.zeros_like(p))
        some = l > 0
        o_raw = torch.where(some, _mm(_round(pdrop, dtype), v, chunk) * (inv_keep / torch.where(some, l, torch.ones_like(l))),
                            torch.zeros(1, dtype=dtype))
        o = _round(o_raw, dtype)
        lse = torch.where(some, (m + torch.log2(torch.where(some, l, torch.ones_like(l)))) * LN2,
                          torch.full_like(l, float("inf"))).squeeze(-1)
    else:
        o_raw, o, lse = forward["o_unrounded"], forward["o"], forward["lse"]
    P = ex2(s2 - (lse * LOG2E).unsqueeze(-1))
    if vis is not None:
        P = torch.where(vis, P, torch.zeros_like(P))
    dP = _mm(dout, v.transpose(-1, -2), chunk)
    if keep is not None:
        dP = torch.where(keep, dP, torch.zeros_like(dP))
    o_for_delta = o_raw if mutant == "delta_unrounded" else (o if o_stored is None else o_stored.to(dtype))
    delta = (dout * o_for_delta).sum(dim=-1, keepdim=True)
    dS = _round(P * (dP * (scale * inv_keep) - delta * scale), dtype)
    Pd = P if keep is None else torch.where(keep, P, torch.zeros_like(P))
    dq = _round(_mm(dS, k, chunk), dtype)
    dk = _round(_mm(dS.transpose(-1, -2), q, chunk), dtype)
    dv = _round(_mm(_round(Pd, dtype).transpose(-1, -2), dout, chunk) * inv_keep, dtype)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "dS_absmax": float(dS.abs().max()), "o_unrounded": o_raw}


def tile_running_max(s2):
    """(..., Lq, n_tiles): the integer running maximum ceil(max) of the log2-domain scores after each 32-key tile (-inf while the row
    has seen nothing)"""
    Lk = s2.shape[-1]
    nkt = (Lk + 31) // 32
    pad = torch.full(s2.shape[:-1] + (nkt * 32 - Lk,), float("-inf"), dtype=s2.dtype)
    tmax = torch.ceil(torch.cat((s2, pad), dim=-1).view(s2.shape[:-1] + (nkt, 32)).amax(dim=-1))
    return torch.cummax(tmax, dim=-1).values


def _skipped_alpha_weights(s2):
    """what leaving out alpha at the last rising tile t* does to the row: everything accumulated before t* stays too large by
    2^(m(t*) - m(t* - 1)) -- a weight on the probabilities of the tiles before t* (numerator and row sum alike)"""
    run = tile_running_max(s2)                                           # (B, H, Lq, nkt)
    nkt = run.shape[-1]
    prev = torch.cat((run[..., :1], run[..., :-1]), dim=-1)
    rises = (run > prev) & torch.isfinite(prev)
    idx = torch.arange(nkt).expand(run.shape)
    t_star = torch.where(rises, idx, torch.zeros_like(idx)).amax(dim=-1, keepdim=True)        # 0: never rises
    step = torch.where(t_star > 0, torch.gather(run - prev, -1, t_star), torch.zeros_like(run[..., :1]))
    step = torch.where(torch.isfinite(step), step, torch.zeros_like(step))
    tile_of_key = (torch.arange(s2.shape[-1]) // 32).expand(s2.shape)
    return torch.where(tile_of_key < t_star, torch.exp2(step).expand(s2.shape), torch.ones_like(s2))


# ---------------------------------------------------------------------------------------------------
# value regimes: seeded, every tensor bf16-representable, (B, H, L, D) layout
# ---------------------------------------------------------------------------------------------------
REGIMES = {
    "unit": "control: bf16-rounded unit normal, what every other test uses",
    "sharp": "q, k x sqrt(8): logit std 8; near one-hot rows with close competitors",
    "sharp32": "q, k x sqrt(32): logit std 32, |s log2 e| reaches ~220",
    "sink_first": "every query + 16 u, key 0 + 16 u (u: a unit vector per head): one key holds almost all the mass",
    "sink_last": "the same with the last key (in the ragged last tile): everything accumulated before is rescaled by ~2^-40 there",
    "stair_up": "queries + 16 u, key j + (j / 32) 4 u: the running maximum rises at every tile, alpha != 1 for every lane every time",
    "stair_down": "key j - (j / 32) 4 u: the maximum is found in the first tile and stays",
    "row_temps": "query row i x 4 2^((i mod 8) - 3): the 32 lanes of a wave sit in eight regimes from flat to one-hot",
    "outlier": "channel 5 of q and k = 0.25 x + 20, channel 7 of v + 100: a large common offset in every logit, O(1) variation on top",
    "tiny": "q, k x 2^-20, v x 2^-10, dout x 2^-14: scores ~ 0, gradients far below 1",
    "big": "v x 256, dout x 1024",
    "ties_q0": "q = 0: uniform P",
    "ties_rows": "all query rows identical",
    "ties_keys": "all keys identical: uniform P and a dq that is exactly zero (judged by a bound, see criterion)",
    "exact": "q = 0, v and dout integers in [-8, 8], L = 256: P = 2^-8, every sum an exact fp32 integer; o and dv bit for bit",
    # hidden_giant:<base>: <base> (one whose queries carry + 16 u) with + GIANT u on the keys the mask hides from everybody (dead keys:
    # a span across tile boundaries, with Lk >= 128 a whole key tile).  A hidden logit is then 16 GIANT scale above every visible one
    # -- 277 log2 units at D = 64, 196 at D = 128: past 2^-149, so that a maximum taken before the mask underflows every visible
    # probability of the row IN FP32 (at the 40 units of a smaller giant such a copy would still be right: the power of two commutes
    # with everything), and a copy that multiplies by the mask instead of selecting forms inf * 0.  Hidden keys do not enter the
    # reference at all, so the yardstick of the case is that of its base.
}


def _seed(case_id):
    return zlib.crc32(case_id.encode())


def values(case):
    """-> dict(q, k, v, dout (B, H, L, D) float32 holding bf16 values, vis (boolean (Lq, Lk) or None), mask (additive or None))"""
    B, H, Lq, Lk, D = case["B"], case["H"], case["Lq"], case["Lk"], case["D"]
    g = torch.Generator().manual_seed(_seed(case["id"]))
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v, do = rn(B, H, Lq, D), rn(B, H, Lk, D), rn(B, H, Lk, D), rn(B, H, Lq, D)
    u = rn(H, D)
    u = (u / u.norm(dim=-1, keepdim=True)).view(1, H, 1, D)
    vis = visibility(case)
    regime = case["regime"]
    giant = regime.startswith("hidden_giant:")
    base = regime.split(":")[1] if giant else regime
    jk = torch.arange(Lk, dtype=torch.float32).view(1, 1, Lk, 1)
    if base == "sharp":
        q, k = q * math.sqrt(8.0), k * math.sqrt(8.0)
    elif base == "sharp32":
        q, k = q * math.sqrt(32.0), k * math.sqrt(32.0)
    elif base in ("sink_first", "sink_last"):
        q = q + 16.0 * u
        j = 0 if base == "sink_first" else Lk - 1
        k[:, :, j] += 16.0 * u[:, :, 0]
    elif base in ("stair_up", "stair_down"):
        q = q + 16.0 * u
        k = k + (1.0 if base == "stair_up" else -1.0) * (jk / 32.0) * 4.0 * u
    elif base == "row_temps":
        q = q * (4.0 * 2.0 ** ((torch.arange(Lq) % 8).float() - 3.0)).view(1, 1, Lq, 1)
    elif base == "outlier":
        q[..., 5 % D] = 0.25 * q[..., 5 % D] + 20.0
        k[..., 5 % D] = 0.25 * k[..., 5 % D] + 20.0
        v[..., 7 % D] += 100.0
    elif base == "tiny":
        q, k, v, do = q * 2.0 ** -20, k * 2.0 ** -20, v * 2.0 ** -10, do * 2.0 ** -14
    elif base == "big":
        v, do = v * 256.0, do * 1024.0
    elif base == "ties_q0":
        q = torch.zeros_like(q)
    elif base == "ties_rows":
        q = q[:, :, :1].expand(B, H, Lq, D).clone()
    elif base == "ties_keys":
        k = k[:, :, :1].expand(B, H, Lk, D).clone()
    elif base == "exact":
        q = torch.zeros_like(q)
        v = torch.randint(-8, 9, v.shape, generator=g).float()
        do = torch.randint(-8, 9, do.shape, generator=g).float()
    elif base != "unit":
        raise ValueError(regime)
    if giant:
        dead = torch.from_numpy(~vis.any(axis=0))
        k[:, :, dead] += GIANT * u
    r = R.bf16_round
    return {"q": r(q), "k": r(k), "v": r(v), "dout": r(do), "vis": vis, "mask": None if vis is None else MC.additive(vis)}


# ---------------------------------------------------------------------------------------------------
# masks: the generators of tests/attention_mask_cases.py, plus `tiles_dead` (tiles with the dead key span of `blind`)
# ---------------------------------------------------------------------------------------------------
def visibility(case):
    if case["mask"] is None:
        return None
    if case["mask"] == "tiles_dead":
        vis = MC.tiles(case["Lq"], case["Lk"], 0)
        lo, hi = MC.dead_span(case["Lk"])
        vis[:, lo:hi] = False
        return vis
    return MC.FAMILIES[case["mask"]](case["Lq"], case["Lk"], 0)


def tables(case, vis, device="cpu"):
    """MaskTables of a case (None without a mask): `tiles` in the natural key order, `blind` in the default one, as the mask tests"""
    from dreamvla_amd import ops
    if vis is None:
        return None
    mask = MC.additive(vis)
    if not case["compact"]:
        return ops.build_mask_tables(mask, device=device, compact_keys=False)
    order = MC.key_order({"order": "natural" if case["mask"].startswith("tiles") else "default", "seed": 0}, vis)
    return ops.build_mask_tables(mask, device=device, key_order=order)


def drop_of(case):
    return (case["p"], (4711, 1234567)) if case["p"] > 0 else None


def drop_cols_of(mt, Lk):
    """the key numbers the kernels hash for dropout: positions on the compacted key axis"""
    if mt is None or mt.key_index is None:
        return None
    cols = torch.zeros(Lk, dtype=torch.int64)
    cols[mt.key_index.cpu().long()] = torch.arange(mt.Lk)
    return cols


# ---------------------------------------------------------------------------------------------------
# yardstick and criterion
# ---------------------------------------------------------------------------------------------------
def errors(got, ref, rows=None):
    """(rel-L2, max-abs error in bf16 ulps of the reference's largest magnitude): the two quantities of gpu_checks.metrics.  The
    reference is rounded to bf16 first, as metrics does for bf16 outputs; `rows` restricts lse to its finite rows"""
    got, ref = got.double(), ref.double()
    if rows is not None:
        got, ref = got[..., rows], ref[..., rows]
    if ref.numel() == 0:
        return 0.0, 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    d = (got - ref).abs()
    top = float(ref.abs().max())
    return float(d.norm() / max(float(ref.norm()), 1e-12)), (float(d.max()) / (2.0 ** -8 * top) if top > 0 else (0.0 if float(d.max()) == 0 else float("inf")))


def reference_kwargs(case, data, mt=None):
    Lk = case["Lk"]
    return dict(scale=case["D"] ** -0.5, mask=data["mask"], drop=drop_of(case), drop_cols=drop_cols_of(mt, Lk))


def _tables_for_drop(case, data):
    return tables(case, data["vis"]) if case["p"] > 0 and data["vis"] is not None else None


def yardstick_of(case, data, ensemble=None, mutant=None):
    """E and U per tensor over the ensemble -> {"E": {tensor: ...}, "U": {...}}, and the per-variant rows"""
    kw = reference_kwargs(case, data, _tables_for_drop(case, data))
    t4 = (data["q"], data["k"], data["v"], data["dout"])
    ref_fwd = attention_ref(*t4, dtype=torch.float64, **kw)
    finite = torch.isfinite(ref_fwd["lse"][0, 0])
    ensemble = ensemble or (ENSEMBLE_REDUCED if case.get("ensemble") == "reduced" else ENSEMBLE)
    E, U, rows = {t: 0.0 for t in TENSORS}, {t: 0.0 for t in TENSORS}, []
    for n, (chunk, jit) in enumerate(ensemble):
        var = attention_ref(*t4, dtype=torch.float32, chunk=chunk, exp_jitter=jit, jitter_seed=1000 + n, mutant=mutant, **kw)
        ref = attention_ref(*t4, dtype=torch.float64, o_stored=var["o"], forward=ref_fwd, **kw)
        row = {}
        for t in TENSORS:
            e, ulp = errors(var[t], ref[t], rows=finite if t == "lse" else None)
            row[t] = (e, ulp)
            E[t], U[t] = max(E[t], e), max(U[t], ulp)
        rows.append(row)
    return {"E": E, "U": U, "rows": rows, "ref_fwd": ref_fwd}


@functools.lru_cache(maxsize=None)
def _cached(case_id):
    case = BY_ID[case_id]
    data = values(case)
    return data, yardstick_of(case, data)


def yardstick(case):
    """-> (data, {"E", "U", "rows", "ref_fwd"}) of a case of CASES, computed once per process"""
    return _cached(case["id"])


def suite_tolerances():
    from tests import gpu_checks as G
    return {"o": (G.TOL_ATTN, G.elem_ulps(G.TOL_ATTN)), "dq": (G.TOL_ATTN_GRAD, G.elem_ulps(G.TOL_ATTN_GRAD)),
            "dk": (G.TOL_ATTN_GRAD, G.elem_ulps(G.TOL_ATTN_GRAD)), "dv": (G.TOL_ATTN_GRAD, G.elem_ulps(G.TOL_ATTN_GRAD)),
            "lse": (G.TOL_F32, None)}


def dq_zero_bound(ref, k, Lk):
    """`ties_keys`: the true dq is exactly zero (every key is the same vector and the rows of dS sum to zero), so the reference's dq
    is rounding noise and a rel-L2 against it means nothing.  What a correct kernel leaves is the sum over Lk keys of bf16 rounding
    errors of dS (relative 2^-9 each, taken as 2^-8) times k, adding like a random walk: 2^-8 max|dS| max|k| sqrt(Lk), and twice that
    for the fp32 cancellation inside P (dP - delta) that precedes the rounding"""
    return 2.0 ** -7 * ref["dS_absmax"] * float(k.abs().max()) * math.sqrt(Lk)


def criterion(case, tensor, got, ref, yard, tag, named=None, fixed=False):
    """one metrics dict: `got` against the float64 `ref` at tol = max(suite, 4 E), k_ulp = max(suite k, 4 U) (fixed=True: the suite
    values alone -- the old way).  lse: fp32 criterion of metrics over the finite rows, its element bound widened by 4 U likewise.
    `named`: the dk / dv rows the tables name (the others are not written)"""
    from tests import gpu_checks as G
    tol0, k0 = suite_tolerances()[tensor]
    E, U = (0.0, 0.0) if fixed else (yard["E"][tensor], yard["U"][tensor])
    tol = max(tol0, MARGIN * E)
    if tensor == "lse":
        fin = torch.isfinite(ref[0, 0])
        g, r = got[..., fin].float(), ref[..., fin]
        m = G.metrics(tag + " lse", g, r.float(), tol, round_ref=False)
        m["max_abs_tol"] = max((2e-4 if tol0 <= 1e-4 else 20 * tol0) * m["ref_absmax"] + 1e-6, MARGIN * U * 2.0 ** -8 * m["ref_absmax"])
        m["tol"] = tol
        m["ok"] = bool(m["finite"] and m["rel_l2"] <= tol and m["max_abs"] <= m["max_abs_tol"])
        m["ulps"] = m["max_abs"] / (2.0 ** -8 * m["ref_absmax"]) if m["ref_absmax"] > 0 else 0.0
        m["allow_frac"] = max(m["rel_l2"] / tol, m["max_abs"] / m["max_abs_tol"])
        return m
    if named is not None:
        got, ref = got[:, :, named], ref[:, :, named]
    k_ulp = max(k0, MARGIN * U)
    m = G.metrics(tag + " " + tensor, got, ref.float(), tol, k_ulp=k_ulp)
    m["ulps"] = m["max_abs"] / (2.0 ** -8 * m["ref_absmax"]) if m["ref_absmax"] > 0 else 0.0
    m["allow_frac"] = max(m["rel_l2"] / tol, m["max_abs"] / m["max_abs_tol"])
    return m


def judge(case, data, yard, got, tag="", named=None, fixed=False, conditioned=True):
    """`got`: dict of (B, H, L, D) float tensors o, dq, dk, dv and optionally lse, as stored by the code under test.  Forward against
    the float64 reference; backward against the float64 backward conditioned on got["o"] (conditioned=False: on the reference's own
    o -- the old way).  -> list of metrics dicts; `ties_keys` has its dq judged by dq_zero_bound instead"""
    kw = reference_kwargs(case, data, _tables_for_drop(case, data))
    ref = attention_ref(data["q"], data["k"], data["v"], data["dout"], dtype=torch.float64, forward=yard["ref_fwd"],
                        o_stored=got["o"] if conditioned else None, **kw)
    out = []
    for t in TENSORS:
        if t not in got:
            continue
        if t == "dq" and case["regime"] == "ties_keys":
            bound = dq_zero_bound(ref, data["k"], case["Lk"])
            worst = float(got["dq"].abs().max())
            out.append({"name": tag + " dq (true value 0: max|dq| <= 2^-7 max|dS| max|k| sqrt(Lk))", "rel_l2": 0.0, "tol": 0.0, "max_abs": worst,
                        "max_abs_tol": bound, "allow_frac": worst / bound, "ok": bool(torch.isfinite(got["dq"]).all()) and worst <= bound})
            continue
        out.append(criterion(case, t, got[t], ref[t], yard, tag, named=named if t in ("dk", "dv") else None, fixed=fixed))
    if case["regime"] == "exact":
        for t in ("o", "dv"):
            same = torch.equal(got[t].to(torch.bfloat16), ref[t].to(torch.bfloat16))
            out.append({"name": tag + f" {t} equals the float64 result bit for bit", "rel_l2": 0.0, "tol": 0.0, "ok": bool(same)})
    return out


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
def _case(family, regime, Lq, Lk=None, D=64, B=2, H=2, p=0.0, mask=None, compact=True, via="raw", ensemble="full"):
    """family: the kernels the shape reaches (tests/test_attention_values.py re-derives it from the dispatch conditions);
    via: "raw" (ops.attn_fwd_raw / attn_bwd_raw), "self" / "cross" (the autograd wrappers: no lse)"""
    Lk = Lq if Lk is None else Lk
    cid = "".join([f"{family}-{regime.replace(':', '=')}-D{D}-L{Lq}", f"x{Lk}" if Lk != Lq else "", f"-B{B}H{H}" if (B, H) != (2, 2) else "",
                   f"-p{p}" if p else "", f"-{mask}" if mask else "", "" if compact else "-uncompacted", f"-{via}" if via != "raw" else ""])
    return dict(id=cid, family=family, regime=regime, Lq=Lq, Lk=Lk, D=D, B=B, H=H, p=p, mask=mask, compact=compact, via=via,
                ensemble=ensemble)


FIVE = ("sink_first", "sink_last", "stair_up", "row_temps", "outlier")      # what every kernel family sees at least

CASES = (
    # short forward + short backward: dense, 3 ... 9 tiles
    [_case("short", r, 197) for r in ("sink_first", "sink_last", "stair_up", "row_temps", "outlier", "sharp32", "tiny")]
    + [_case("short", r, 261) for r in ("sink_last", "stair_up", "stair_down", "big", "ties_q0", "ties_keys")]
    + [_case("short", "exact", 256)]
    # ring forward + short backward: dense, two tiles
    + [_case("ring_fwd_short_bwd", r, 40) for r in FIVE + ("ties_rows",)]
    # ring forward, ring dQ, ring dK/dV: dense with 11 tiles, dropout, masks
    + [_case("ring", r, 333) for r in FIVE + ("sharp", "unit")]
    + [_case("ring", r, 133, p=0.1) for r in ("sink_last", "stair_up")]
    + [_case("ring", r, 133, mask="blind") for r in ("sink_first", "outlier", "hidden_giant:sink_first")]
    + [_case("ring", r, 133, mask="tiles") for r in ("sink_last", "stair_up", "row_temps")]
    + [_case("ring", r, 133, mask="blind", compact=False) for r in ("sink_last", "hidden_giant:stair_up")]
    + [_case("ring", "hidden_giant:sink_first", 133, mask="tiles_dead", compact=False)]
    # staged forward, dQ, dK/dV: 66 tiles under tables that do not fit the ring kernels' LDS
    + [_case("staged", "sink_last", 2085, B=1, mask="tiles", ensemble="reduced"),
       _case("staged", "hidden_giant:sink_first", 2085, B=1, mask="tiles_dead", compact=False, ensemble="reduced")]
    # cross shapes, masked
    + [_case("ring", "sink_first", 40, 133, mask="blind"), _case("ring", "hidden_giant:sink_first", 40, 133, mask="blind", compact=False),
       _case("ring", "sink_last", 133, 40, mask="tiles"), _case("ring", "stair_up", 133, 40, mask="blind")]
    # attention_hd: the padded head widths 32 (24), 64 (48), 96, 128
    + [_case("hd", "sink_first", 133, D=32, mask="tiles"), _case("hd", "row_temps", 133, D=32),
       _case("hd", "hidden_giant:sink_first", 133, D=96, mask="blind", compact=False), _case("hd", "sink_last", 133, D=96, mask="blind"),
       _case("hd", "stair_up", 133, D=128), _case("hd", "outlier", 133, D=128, mask="tiles"), _case("hd", "exact", 256, D=128),
       _case("hd", "sink_last", 133, D=24, mask="blind", p=0.1),
       _case("hd", "stair_up", 133, D=48, mask="tiles"), _case("hd", "row_temps", 133, D=48, p=0.1)]
    # attention_small through ops.self_attention(head_dim=96)
    + [_case("small", r, 64, D=96, via="self") for r in FIVE]
    + [_case("small", r, 6, D=96, via="self") for r in ("sink_first", "ties_keys")]
    # the head-64 autograd wrappers
    + [_case("ring", "sink_first", 133, via="self", mask="blind"), _case("ring", "sink_first", 40, 133, via="cross")]
)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the probe: (regime, mask, compact) at L = 133, D = 64; rows against a float64 softmax
PROBE_CASES = [("sharp32", None, True), ("sink_last", None, True), ("hidden_giant:sink_first", "blind", False),
               ("hidden_giant:stair_up", "blind", True)]


def dispatch(case, mt):
    """the kernels a head-width-64 raw case reaches, from the conditions of dvla_attn_fwd / dvla_attn_bwd (csrc/attention.hip):
    -> (forward, backward) in {"short", "ring", "staged"} ("ring" backward: dQ and dK/dV both)"""
    nqt = (case["Lq"] + 31) // 32
    dense = mt is None and case["p"] == 0 and case["Lq"] == case["Lk"]
    ring_fwd, ring_dkv = MC.ring_kernels({"Lq": case["Lq"], "Lk": case["Lk"], "dropout_p": case["p"]}, mt)
    fwd = "short" if dense and 2 < nqt <= 9 else ("ring" if ring_fwd else "staged")
    if dense and nqt <= 9:
        return fwd, "short"
    if ring_fwd != ring_dkv:
        return fwd, "mixed"
    return fwd, "ring" if ring_fwd else "staged"
