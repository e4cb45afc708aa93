"""Cases for the LayerNorm and element-wise kernels (tests/test_layernorm_paths_gpu.py, tests/test_elementwise_paths_gpu.py), and
what makes each of them a case: the launch geometry of dreamvla_amd/csrc/layernorm.hip and elementwise.hip restated as pure
functions, seeded data generators, and the case tables.  tests/test_rowwise_cases.py asserts -- without a GPU -- that every case
reaches the loop, template instance or branch it is listed for, so that a shape edited later cannot silently stop testing it.

This module touches neither the GPU nor the library.  The constants below are the host code's, written out; one GPU test holds
the two that the library exports (dvla_layernorm_bwd_partial_rows, dvla_colsum_partial_rows) against them."""
import torch

# ---------------------------------------------------------------------------------------------------
# launch geometry
# ---------------------------------------------------------------------------------------------------
LN_ROWS_PER_BLOCK = 4          # one wave per row, 256 threads
LN_FWD_MAX_BLOCKS = 2048       # fwd_blocks()
LN_BWD_MAX_BLOCKS = 768        # LN_BWD_BLOCKS
LN_COLS_PER_SLOT = 512         # 64 lanes x 8 bf16: one 16-byte vector per lane and slot
LN_MAX_VPL = 4
CS_COLS_PER_STRIP = 512
CS_MAX_SLABS = 512             # CS_BLOCKS
EW_MAX_BLOCKS = 4096           # grid_for()
EW_THREADS = 256


def ln_supported(cols):
    return cols > 0 and cols % 8 == 0 and cols <= LN_COLS_PER_SLOT * LN_MAX_VPL


def ln_geometry(rows, cols, backward=False):
    """what ln_fwd_kernel / ln_bwd_kernel run for a rows x cols problem.  trips: loop iterations of the busiest wave (wave 0 of
    block 0); last_trip_rows: rows of the last trip (< rows_per_trip: some waves sit it out); prefetch_trips: trips of that wave
    in which `row + stride < rows` holds, i.e. the next row is requested and handed over (raw = nxt)"""
    cap = LN_BWD_MAX_BLOCKS if backward else LN_FWD_MAX_BLOCKS
    blocks = max(1, min(-(-rows // LN_ROWS_PER_BLOCK), cap))
    per_trip = blocks * LN_ROWS_PER_BLOCK
    trips = -(-rows // per_trip)
    nvec = cols // 8
    vpl = -(-cols // LN_COLS_PER_SLOT)
    return {"blocks": blocks, "rows_per_trip": per_trip, "trips": trips, "last_trip_rows": rows - (trips - 1) * per_trip,
            "prefetch_trips": trips - 1, "vpl": vpl, "last_slot_lanes": nvec - 64 * (vpl - 1)}


def ln_group_geometry(n, L, keep, backward=True):
    """row groups of layer_norm_last_tokens: n * keep rows, group = keep rows, `L - keep` rows of every sequence zero-filled by the
    wave that owns the group's first row.  zero_fill_later: some group's first row is met on a trip after the first"""
    rows = n * keep
    cap = LN_BWD_MAX_BLOCKS if backward else LN_FWD_MAX_BLOCKS
    per_trip = max(1, min(-(-rows // LN_ROWS_PER_BLOCK), cap)) * LN_ROWS_PER_BLOCK
    first_later = -(-per_trip // keep) * keep           # the first group start at or behind the first trip
    return {"rows": rows, "zero_rows_per_group": L - keep, "zero_fill_later": first_later < rows}


def ew_geometry(n, per_thread=1):
    """grid_for(): blocks of 256 threads, `per_thread` elements each, at most 4096; trips of the grid-stride loop"""
    blocks = max(1, min(-(-n // (EW_THREADS * per_thread)), EW_MAX_BLOCKS))
    span = blocks * EW_THREADS * per_thread
    return {"blocks": blocks, "trips": -(-n // span), "odd": n % 2 == 1}


def colsum_geometry(rows, cols, ld=None, offset_elems=0):
    """dvla_colsum_dt's launch.  offset_elems: the view's origin relative to a 16-byte boundary, in bf16 elements.  scalar_lanes:
    the lanes (counted over all strips) that take the element-wise branch"""
    ld = cols if ld is None else ld
    strips = -(-cols // CS_COLS_PER_STRIP)
    want = rows // 16
    vec_ok = ld % 8 == 0 and offset_elems % 8 == 0
    ragged = cols % 8 != 0
    lanes = -(-cols // 8)
    return {"strips": strips, "slabs": max(1, min(want, CS_MAX_SLABS)), "capped": want > CS_MAX_SLABS, "vec_ok": vec_ok,
            "ragged_last_octet": ragged, "scalar_lanes": lanes if not vec_ok else int(ragged),
            "rows_per_slab_min": rows // max(1, min(want, CS_MAX_SLABS))}


# ---------------------------------------------------------------------------------------------------
# data: bf16-representable fp32 CPU tensors, one class per row
# ---------------------------------------------------------------------------------------------------
ROW_CLASSES = ("unit", "offset", "outlier", "rowscale", "tiny", "huge", "const")
KAPPA_MAX = 64.0        # |mean| * rstd of every row that is not constant
CONST_MAX = 4.0
OFFSETS = ((8.0, 1.0), (-8.0, 1.0), (64.0, 1.0), (-64.0, 1.0), (256.0, 4.0))      # (mean, std)


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def row_kappa(x, eps):
    """(kappa, mean, rstd, is_const) per row in float64: kappa = |mean| * rstd with rstd = (var + eps)^-1/2"""
    xd = x.double()
    mean = xd.mean(-1)
    var = ((xd - mean[:, None]) ** 2).mean(-1)
    rstd = (var + eps).rsqrt()
    return mean.abs() * rstd, mean, rstd, (xd == xd[:, :1]).all(-1)


def _offset_rows(z, r, eps):
    """mean +-8 / +-64 with std 1, 256 with std 4.  A short row's sample std can fall below the nominal one (and bf16 spacing at
    64 is 0.25 - 0.5): the deviations of a row whose kappa would pass KAPPA_MAX are stretched by 5/4 until it does not"""
    mean = torch.tensor([OFFSETS[int(i) % len(OFFSETS)][0] for i in r])[:, None]
    std = torch.tensor([OFFSETS[int(i) % len(OFFSETS)][1] for i in r])[:, None]
    dev = z * std
    for _ in range(64):
        x = bf16_round(mean + dev)
        bad = row_kappa(x, eps)[0] > 0.95 * KAPPA_MAX
        if not bool(bad.any()):
            return x
        dev[bad] *= 1.25
    raise AssertionError("offset rows: kappa not reached")


def make_rows(kind, rows, cols, seed, eps=1e-5):
    """(rows, cols) tensor of class `kind` (one of ROW_CLASSES, or "mixed": the classes interleaved row by row) and the tuple of
    every row's class name"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((rows, cols), generator=g)
    z2 = torch.randn((rows, cols), generator=g)
    cvals = bf16_round(torch.rand((rows,), generator=g) * 2 * CONST_MAX - CONST_MAX)
    names = tuple(ROW_CLASSES[r % len(ROW_CLASSES)] if kind == "mixed" else kind for r in range(rows))
    unit = 2.0 * z + 0.5
    x = torch.empty((rows, cols))
    idx = {k: [r for r, nm in enumerate(names) if nm == k] for k in ROW_CLASSES}
    for k, r in idx.items():
        if not r:
            continue
        r = torch.tensor(r)
        if k == "unit":
            x[r] = unit[r]
        elif k == "offset":
            x[r] = _offset_rows(z[r], r, eps)
        elif k == "outlier":
            v = unit[r]
            ch = torch.arange(0, cols, 193)
            v[:, ch] = 300.0 * z2[r][:, ch] + 500.0
            x[r] = v
        elif k == "rowscale":
            e = torch.linspace(-10.0, 10.0, rows)[r]
            x[r] = unit[r] * torch.exp2(e)[:, None]
        elif k == "tiny":
            x[r] = unit[r] * 1e-3
        elif k == "huge":
            x[r] = unit[r] * 1e4
        elif k == "const":
            x[r] = cvals[r][:, None].expand(-1, cols)
    return bf16_round(x), names


def ln_params(cols, seed, affine=True):
    if not affine:
        return None, None
    g = torch.Generator().manual_seed(seed + 7919)
    return bf16_round(torch.randn((cols,), generator=g) + 1.0), bf16_round(torch.randn((cols,), generator=g))


def grad_like(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed + 104729)
    return bf16_round(torch.randn(shape, generator=g) * scale)


# ---------------------------------------------------------------------------------------------------
# LayerNorm cases.  `path` says what the case is there for; tests/test_rowwise_cases.py turns every word of it into an assertion.
# ---------------------------------------------------------------------------------------------------
def _ln(id_, kind, rows, cols, data, path, eps=1e-5, affine=True, pf32=False, stats=False):
    return {"id": id_, "kind": kind, "rows": rows, "cols": cols, "data": data, "eps": eps, "affine": affine, "pf32": pf32,
            "stats": stats, "path": path}


RAGGED_COLS = (8, 504, 512, 1032, 1536, 1544, 2040, 2048)
# cols -> (VPL, active lanes of the last vector slot)
RAGGED_EXPECT = {8: (1, 1), 504: (1, 63), 512: (1, 64), 1032: (3, 1), 1536: (3, 64), 1544: (4, 1), 2040: (4, 63), 2048: (4, 64)}

LN_CASES = [
    _ln("plain-8197x64-mixed", "plain", 8197, 64, "mixed", "fwd-2-trips-last-partial bwd-3-trips", stats=True),
    _ln("plain-16389x8-mixed", "plain", 16389, 8, "mixed", "fwd-3-trips-prefetch lanes-1"),
    _ln("plain-16389x520-mixed", "plain", 16389, 520, "mixed", "fwd-3-trips-prefetch vpl-2"),
    _ln("fork-3077x520-mixed", "fork", 3077, 520, "mixed", "bwd-2-trips vpl-2"),
]
for _c in RAGGED_COLS:
    for _k in ("plain", "fork"):
        LN_CASES.append(_ln(f"{_k}-9x{_c}-mixed", _k, 9, _c, "mixed", "ragged"))
for _c in (1032, 1544):
    for _k in ("plain", "fork"):
        LN_CASES.append(_ln(f"{_k}-9x{_c}-mixed-pf32", _k, 9, _c, "mixed", "ragged", pf32=True))
for _k in ("plain", "fork"):
    LN_CASES.append(_ln(f"{_k}-9x1032-mixed-noaffine", _k, 9, 1032, "mixed", "ragged", affine=False))
for _cols, _eps in ((768, 1e-6), (1024, 1e-5)):
    for _d in ROW_CLASSES + ("mixed",):
        for _k in ("plain", "fork"):
            LN_CASES.append(_ln(f"{_k}-64x{_cols}-{_d}", _k, 64, _cols, _d, "model-width", eps=_eps,
                                stats=(_k == "plain" and _cols == 768)))

# layer_norm_last_tokens: (n, L, keep, cols)
LAST_TOKENS_CASES = [
    {"id": "last-400x10keep8x64", "n": 400, "L": 10, "keep": 8, "cols": 64, "path": "bwd-2-trips zero-fill-later"},
    {"id": "last-3100x10keep10x8", "n": 3100, "L": 10, "keep": 10, "cols": 8, "path": "bwd-2-trips fwd-2-trips nothing-to-fill"},
    {"id": "last-3100x10keep1x8", "n": 3100, "L": 10, "keep": 1, "cols": 8, "path": "bwd-2-trips zero-fill-later"},
]
# layer_norm_concat: (n, La, Lb, cols, a_needs_grad).  700 x (4 + 1) launches 700 and 175 backward workgroups -- under the 768 at
# which ln_bwd_kernel starts to iterate -- so it covers the one-sided gradient at one trip, and 772 x (4 + 1) (3088 rows of a: the
# smallest n at which the last trip is a partly empty one) is the case in which the map_output variant iterates.
CONCAT_CASES = [
    {"id": "concat-700x(4+1)x64-a0", "n": 700, "La": 4, "Lb": 1, "cols": 64, "a_needs_grad": False, "path": "one-trip"},
    {"id": "concat-772x(4+1)x64-a0", "n": 772, "La": 4, "Lb": 1, "cols": 64, "a_needs_grad": False, "path": "bwd-2-trips"},
    {"id": "concat-772x(4+1)x64-a1", "n": 772, "La": 4, "Lb": 1, "cols": 64, "a_needs_grad": True, "path": "bwd-2-trips"},
]
LN_REFUSED_COLS = (12, 2056)

# ---------------------------------------------------------------------------------------------------
# element-wise cases
# ---------------------------------------------------------------------------------------------------
ACTS = ("gelu_erf", "gelu_tanh", "relu", "silu", "quick_gelu", "tanh", "sigmoid")
ACT_DOMAIN_EXP = 40            # |x| <= 2^40: x^3 is finite in fp32
_ACT_TOP = (127 + ACT_DOMAIN_EXP) << 7      # bf16 pattern of 2^40


def act_inputs():
    """every finite bf16 value with |x| <= 2^40 (both zeros, the subnormals), as a bf16 tensor in pattern order"""
    mag = torch.arange(0, _ACT_TOP + 1, dtype=torch.int32)
    return torch.cat((mag, mag + 0x8000 - 0x10000)).to(torch.int16).view(torch.bfloat16)


ACT_TILE = 25                  # act_inputs() tiled: the second grid-stride trip


def cast_f2b_inputs():
    """fp32 inputs of the rounding test: for every pair of adjacent finite bf16 values of either sign the fp32 midpoint (a tie) and
    its two fp32 neighbours; then +-0, fp32 subnormals, +-inf, +-FLT_MAX (rounds to inf), NaNs"""
    k = torch.arange(0, 0x7F7F, dtype=torch.int64)             # k and k + 1 are finite bf16 patterns
    mid = (k << 16) + 0x8000
    pos = torch.stack((mid - 1, mid, mid + 1), 1).flatten()
    special = torch.tensor([0x00000000, 0x80000000, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x80000001, 0x807FFFFF,
                            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=torch.int64)
    bits = torch.cat((pos, pos | 0x80000000, special))
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits)
    return bits.to(torch.int32).view(torch.float32)


CAST_F2B_TILE = 6
CAST_B2F_TILE = 17


def cast_b2f_inputs():
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    return (bits - (bits >= 0x8000).int() * 0x10000).to(torch.int16).view(torch.bfloat16)


# (under the tests' seed the LAST element of both is kept: a thread pair that skips it leaves a value missing, not a zero that
# happens to be right)
DROPOUT_CASES = [{"rows": 2049, "cols": 1025, "p": 0.1, "path": "odd trips-2"}, {"rows": 7, "cols": 9, "p": 0.25, "path": "odd straddle"}]
ACT_BWD_DROP_CASES = [{"rows": r, "cols": c, "p": p, "act": a, "path": "trips-2" if r == 4099 else "shape-not-taken-by-colsum"}
                      for (r, c) in ((4099, 257), (100, 36)) for p in (0.1, 0.5) for a in ("none", "gelu_tanh")]
ADD_CASES = [{"n": n, "period": p, "path": "trips-2" if n > 1 << 20 else "one-block"} for n in (1_048_833, 63) for p in (0, 24, 257)]

# colsum: pad / offset describe the view inside a sentinel-filled backing store (tests.gpu_checks.make_view); pad None: contiguous
COLSUM_CASES = [
    {"id": "8200x24", "rows": 8200, "cols": 24, "pad": None, "offset": 0, "path": "all-slabs"},
    {"id": "8216x24", "rows": 8216, "cols": 24, "pad": None, "offset": 0, "path": "slab-cap"},
    {"id": "7x64", "rows": 7, "cols": 64, "pad": None, "offset": 0, "path": "rows-lt-16"},
    # contiguous with cols % 8 != 0: the leading dimension itself is unaligned, every lane takes the element-wise branch
    {"id": "50x36", "rows": 50, "cols": 36, "pad": None, "offset": 0, "path": "scalar"},
    {"id": "300x1001", "rows": 300, "cols": 1001, "pad": None, "offset": 0, "path": "scalar strips-2"},
]
# the same two shapes as row-strided views.  Aligned: ld = 2 * cols + 8 rounded up to a multiple of 8 (80; 2016) -- the 16-byte
# branch with ONE ragged last octet, which a contiguous operand cannot reach; the same view 3 elements further on; ld % 8 != 0.
for _r, _c in ((50, 36), (300, 1001)):
    _pad = -(-(2 * _c + 8) // 8) * 8 - _c
    COLSUM_CASES += [
        {"id": f"{_r}x{_c}-view-aligned", "rows": _r, "cols": _c, "pad": _pad, "offset": 0, "path": "view vec ragged" + (" strips-2" if _c > 512 else "")},
        {"id": f"{_r}x{_c}-view-shifted3", "rows": _r, "cols": _c, "pad": _pad, "offset": 3, "path": "view scalar"},
        {"id": f"{_r}x{_c}-view-ld-odd", "rows": _r, "cols": _c, "pad": _pad + 3, "offset": 0, "path": "view scalar"},
    ]
# 8200 rows: rows / 16 = 512 slabs, every partial row in use; 8216: 513 wanted, capped.  One active lane per wave (8 columns).
ACT_BWD_COLSUM_CASES = [{"rows": 8200, "cols": 8, "path": "all-slabs lanes-1"}, {"rows": 8216, "cols": 8, "path": "slab-cap lanes-1"}]


def colsum_case_ld(c):
    return c["cols"] if c["pad"] is None else c["cols"] + c["pad"]


def colsum_case_geometry(c):
    return colsum_geometry(c["rows"], c["cols"], colsum_case_ld(c), c["offset"])
