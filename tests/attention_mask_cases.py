"""Arbitrary 0 / -inf attention masks for the attention kernels (csrc/attention.hip, csrc/attention_hd.hip): seeded generators and
the case list of tests/test_attention_masks_gpu.py.  Importable without a GPU; tests/test_attention_mask_cases.py asserts per case
the structural conditions (tile classes, blind rows, dead keys, walk patterns, kernel family by the LDS formulas) that make the
GPU run mean something.

Every mask the rest of the suite uses is a block-causal staircase: each query sees a prefix of the keys, the empty 32 x 32 tiles
sit in one corner, no query is blind, Lq == Lk.  The families here are everything else ops.build_mask_tables accepts:

  bern     every entry visible with probability p (0.5: every tile mixed, every bit position and accumulator register in use)
  tiles    every 32 x 32 tile drawn empty / full / mixed (density 0.3) with equal probability: holes anywhere in a walk.  Tables in
           the NATURAL key order (ascending visible columns): the default audience ordering permutes the columns and turns almost
           every tile mixed
  blind    bern(0.5) with queries that see NO key (one single row, one whole 32-row tile = a wave, one whole 128-row block = a
           workgroup when Lq >= 256, the ragged last rows), a span of dead key columns that crosses a tile boundary (for Lk >= 128
           it covers a whole key tile) and a few rows that see exactly one key
  edges    hand-placed tiles, natural key order, every key visible to somebody: per 128-query block a walk whose first and last
           tiles are empty, a walk of one live tile, walks with holes, and tiles that are live for wave 0 only / wave 3 only of a
           block ("first tiles empty for all queries of the mask" cannot reach the kernels through compacted tables -- such keys are
           dropped from the key axis; the uncompacted `blind` case carries a whole key tile nobody sees instead)
  corner   every tile mixed, holding only one of the bits (0,0), (0,31), (31,0), (31,31) of its valid area, or everything but it

Values stay bf16-rounded unit normal and tolerances stay those of tests/gpu_checks.py: a wrong result here is off by whole rows."""
import numpy as np
import torch

FA_RING = 32768            # csrc/attention.hip: FA_NS * 2 * FA_TILE
RING_LDS_LIMIT = 64 * 1024     # forward and dQ ring kernels (dvla_attn_fwd / dvla_attn_bwd: smem <= 64 KiB)
DKV_LDS_LIMIT = 80 * 1024      # dK/dV ring kernel


# ---------------------------------------------------------------------------------------------------
# generators: boolean visibility (Lq, Lk), deterministic in (shape, seed)
# ---------------------------------------------------------------------------------------------------
def bern(Lq, Lk, p=0.5, seed=0):
    return np.random.default_rng(seed).random((Lq, Lk)) < p


def _tile_grid(Lq, Lk):
    return (Lq + 31) // 32, (Lk + 31) // 32


def tiles(Lq, Lk, seed=0, density=0.3):
    rng = np.random.default_rng(seed)
    nqt, nkt = _tile_grid(Lq, Lk)
    cls = rng.integers(0, 3, size=(nqt, nkt))
    vis = np.zeros((Lq, Lk), dtype=bool)
    for qt in range(nqt):
        for kt in range(nkt):
            blk = vis[qt * 32:(qt + 1) * 32, kt * 32:(kt + 1) * 32]
            draw = rng.random(blk.shape) < density
            if cls[qt, kt] == 1:
                blk[:] = True
            elif cls[qt, kt] == 2:
                if blk.size > 1:          # really mixed: at least one bit set and one clear
                    draw.flat[0], draw.flat[-1] = True, False
                blk[:] = draw
    return vis


def dead_span(Lk):
    """the key columns `blind` hides from everybody: across a tile boundary; with Lk >= 128 all of key tile 2 and both its borders"""
    return (60, 100) if Lk >= 128 else (28, min(36, Lk))


def blind_rows(Lq):
    rows = set()
    if Lq > 8:
        rows.add(7)                                   # one single row
    if Lq >= 96:
        rows.update(range(32, 64))                    # a whole wave
    if Lq >= 256:
        rows.update(range(128, 256))                  # a whole workgroup
    if Lq % 32 and Lq > 32:
        rows.update(range(Lq // 32 * 32, Lq))         # the ragged last rows
    return sorted(rows)


def blind(Lq, Lk, seed=0):
    rng = np.random.default_rng(seed)
    vis = rng.random((Lq, Lk)) < 0.5
    lo, hi = dead_span(Lk)
    live = np.setdiff1d(np.arange(Lk), np.arange(lo, hi))
    none = blind_rows(Lq)
    one = [r for r in (3, 20, 70, 100, 200) if r < Lq and r not in none][:max(Lq // 4, 0)]
    for r in one:                                     # rows that see exactly one key
        vis[r] = False
        vis[r, int(rng.choice(live))] = True
    vis[none] = False
    vis[:, lo:hi] = False
    return vis


def _mixed_block(rows, cols, rng):
    """a mixed tile in which every column is seen by some row and every row sees some column (no dead key, no blind query)"""
    blk = rng.random((rows, cols)) < 0.5
    for j in range(cols):
        blk[j % rows, j] = True
    for i in range(rows):
        blk[i, i % cols] = True
    if rows > 1 and cols > 1:
        blk[0, 1] = False
    return blk


# (query tile -> {key tile: class}) of `edges`; 1 = full, 2 = mixed, everything else empty
EDGES_SPEC = {
    # L = 133: block A = query tiles 0..3 walks key tiles 1, 2, 3 (first and last empty; tile 1 is live for wave 0 only, tile 2 for
    # wave 3 only; every query tile has ONE live tile), block B = query tile 4 walks 0 and 4 (a hole of three tiles)
    133: {0: {1: 1}, 1: {3: 2}, 2: {3: 2}, 3: {2: 2}, 4: {0: 1, 4: 2}},
    # L = 261: block A walks key tile 5 alone; block B walks 0, 2, 4, 6, 8 (holes everywhere, first and last live, every tile live
    # for one wave only); block C (one live wave of 5 rows) walks 1, 3, 7
    261: {0: {5: 2}, 1: {5: 1}, 2: {5: 2}, 3: {5: 1}, 4: {0: 1}, 5: {8: 2}, 6: {2: 2, 6: 1}, 7: {4: 2}, 8: {1: 2, 3: 1, 7: 2}},
}
# the walks the kernels must take: key tiles per 128-query block (forward, dQ) and query tiles per 128-key block (dK/dV)
EDGES_WALKS = {
    133: {"q": {0: [1, 2, 3], 1: [0, 4]}, "k": {0: [0, 1, 2, 3, 4], 1: [4]}},
    261: {"q": {0: [5], 1: [0, 2, 4, 6, 8], 2: [1, 3, 7]}, "k": {0: [4, 6, 8], 1: [0, 1, 2, 3, 6, 7, 8], 2: [5]}},
}


def edges(L, seed=0):
    rng = np.random.default_rng(seed)
    vis = np.zeros((L, L), dtype=bool)
    for qt, row in EDGES_SPEC[L].items():
        for kt, c in row.items():
            blk = vis[qt * 32:(qt + 1) * 32, kt * 32:(kt + 1) * 32]
            blk[:] = True if c == 1 else _mixed_block(blk.shape[0], blk.shape[1], rng)
    return vis


def corner(L, seed=0):
    """tile (qt, kt) holds corner bit (qt + 3 kt) % 4 of its valid area alone, or -- ids 4..7 -- everything but that bit.  The
    ragged last row / column of tiles takes complements only, so that no key is dead and no query blind: the natural key order
    keeps every bit where it was put."""
    nqt, nkt = _tile_grid(L, L)
    vis = np.zeros((L, L), dtype=bool)
    for qt in range(nqt):
        for kt in range(nkt):
            blk = vis[qt * 32:(qt + 1) * 32, kt * 32:(kt + 1) * 32]
            r, c = blk.shape
            pid = (qt + 3 * kt) % 8
            ragged = r < 32 or c < 32
            if ragged and (r, c) != (L % 32, L % 32):
                pid |= 4
            i, j = ((0, 0), (0, c - 1), (r - 1, 0), (r - 1, c - 1))[pid % 4]
            blk[:] = pid >= 4
            blk[i, j] = pid < 4
    return vis


FAMILIES = {"bern": lambda Lq, Lk, seed: bern(Lq, Lk, 0.5, seed), "tiles": tiles, "blind": blind,
            "edges": lambda Lq, Lk, seed: edges(Lq, seed), "corner": lambda Lq, Lk, seed: corner(Lq, seed)}


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
def _case(family, Lq, Lk=None, D=64, B=2, H=2, p=0.0, order=None, compact=True, seed=0, period=None, rows=None, **expect):
    """order: "default" (audience count), "natural" (ascending visible columns), "random" (a seeded permutation of them).
    expect: minimum counts `empty` / `full` / `mixed` / `blind` / `dead`, `index` (whether the tables carry a key_index),
    `ring` = (forward + dQ ring kernels?, dK/dV ring kernel?) by the LDS formulas."""
    Lk = Lq if Lk is None else Lk
    usual = "natural" if family in ("tiles", "edges", "corner") else "default"
    order = order or usual
    cid = "".join([f"{family}-D{D}-L{Lq}", f"x{Lk}" if Lk != Lq else "", f"-B{B}H{H}" if (B, H) != (2, 2) else "", f"-p{p}" if p else "",
                   f"-{order}" if order != usual else "", "" if compact else "-uncompacted"])
    return dict(id=cid, family=family, Lq=Lq, Lk=Lk, D=D, B=B, H=H, dropout_p=p, order=order, compact=compact, seed=seed,
                period=period, rows=rows, expect=expect)


CASES = [
    # head width 64, five tiles, the last with 5 rows
    _case("bern", 133, mixed=25, index=True),
    _case("tiles", 133, empty=5, full=5, mixed=5),
    _case("blind", 133, blind=38, dead=40, mixed=9, empty=6, index=True),
    _case("edges", 133, empty=19, full=2, mixed=4, index=False),
    _case("corner", 133, mixed=25, index=False),
    _case("tiles", 133, p=0.1, empty=5, full=5, mixed=5),
    _case("blind", 133, p=0.1, blind=38, dead=40, index=True),
    # order independence: the same mask under the other two key orders
    _case("tiles", 133, order="default", empty=5, full=5, mixed=5, index=True),
    _case("tiles", 133, order="random", mixed=20, index=True),
    _case("blind", 133, p=0.1, order="natural", blind=38, dead=40, index=True),
    _case("blind", 133, p=0.1, order="random", blind=38, dead=40, index=True),
    # nine tiles: three query blocks, the last with one live wave
    _case("blind", 261, blind=166, dead=40, empty=42, mixed=21, index=True),
    _case("edges", 261, empty=69, full=5, mixed=7, index=False),
    # no key compaction: no key_index, dead keys stay on the key axis (a whole key tile of them) and every dk / dv row is written
    _case("blind", 133, compact=False, blind=38, dead=40, empty=13, mixed=12, index=False),
    # rectangular masks (nqt != nkt)
    _case("tiles", 40, 133, empty=1, full=1, mixed=1, dead=32, index=True),
    _case("blind", 40, 133, blind=9, dead=40, mixed=3, index=True),
    _case("tiles", 133, 40, empty=1, full=1, mixed=1, blind=64, index=False),
    _case("blind", 133, 40, blind=38, dead=8, mixed=3, index=True),
    _case("tiles", 1, 70, full=1, dead=1, index=True),           # one query: what it sees is compacted into full tiles
    _case("blind", 1, 70, full=1, dead=8, index=True),
    _case("tiles", 70, 33, empty=1, full=1, mixed=1, blind=1, index=False),
    _case("blind", 70, 33, blind=7, dead=5, mixed=2, index=True),
    # the 64-tile boundary of the ballot words and the LDS limits of the ring kernels
    _case("none", 2048, B=1, H=2, ring=(True, True)),
    _case("tiles", 2016, B=1, H=2, empty=1000, full=1000, mixed=1000, index=False, ring=(True, True)),
    _case("tiles", 2085, B=1, H=2, empty=1000, full=1000, mixed=1000, index=False, ring=(False, False)),
    # several (batch, head) items per workgroup of the forward ring kernel
    _case("tiles", 133, B=64, H=8, period=5, rows=6, empty=5, full=5, mixed=5),
    # the head-width-generic kernels
    _case("tiles", 133, D=32, empty=5, full=5, mixed=5),
    _case("blind", 133, D=96, blind=38, dead=40, index=True),
    _case("edges", 133, D=128, empty=19, full=2, mixed=4, index=False),
    _case("blind", 133, D=24, p=0.1, blind=38, dead=40, index=True),
    _case("tiles", 40, 133, D=48, empty=1, full=1, mixed=1, dead=32, index=True),
]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def visibility(case):
    """boolean (Lq, Lk) of a case; None for the unmasked one"""
    if case["family"] == "none":
        return None
    return FAMILIES[case["family"]](case["Lq"], case["Lk"], case["seed"])


def additive(vis):
    return torch.where(torch.from_numpy(vis), torch.zeros(()), torch.full((), -float("inf")))


def key_order(case, vis):
    """the key_order argument of ops.build_mask_tables for the case's order"""
    cols = np.nonzero(vis.any(axis=0))[0]
    if case["order"] == "natural":
        return cols
    if case["order"] == "random":
        return np.random.default_rng(1000 + case["seed"]).permutation(cols)
    return None


def tables(case, device="cpu"):
    """-> (vis, additive mask, MaskTables) of a case ((None, None, None) for the unmasked one)"""
    from dreamvla_amd import ops
    vis = visibility(case)
    if vis is None:
        return None, None, None
    mask = additive(vis)
    if case["compact"]:
        mt = ops.build_mask_tables(mask, device=device, key_order=key_order(case, vis))
    else:
        mt = ops.build_mask_tables(mask, device=device, compact_keys=False)
    return vis, mask, mt


def structure(vis, mt):
    """what the report rows and the CPU test quote: tile classes of the TABLES, blind rows and dead keys of the mask"""
    if vis is None:
        return {"empty": 0, "full": 0, "mixed": 0, "blind": 0, "dead": 0, "index": False}
    tm = mt.tile_map.cpu().numpy()
    return {"empty": int((tm == 0).sum()), "full": int((tm == 1).sum()), "mixed": int((tm == 2).sum()),
            "blind": int((~vis.any(axis=1)).sum()), "dead": int((~vis.any(axis=0)).sum()), "index": mt.key_index is not None}


def walks(tile_map, axis):
    """axis "q": per 128-query block the key tiles some wave needs; axis "k": per 128-key block the query tiles"""
    tm = np.asarray(tile_map) != 0
    tm = tm if axis == "q" else tm.T
    return {b: [int(t) for t in np.nonzero(tm[4 * b:4 * b + 4].any(axis=0))[0]] for b in range((tm.shape[0] + 3) // 4)}


def _pad16(n):
    return (n + 15) // 16 * 16


def ring_lds_bytes(nkt, Lk, has_index, has_bits):
    """fa_smem_bytes of csrc/attention.hip (forward and dQ ring kernels): ring | flags | key list | 128 visibility rows"""
    return FA_RING + _pad16(nkt) + (_pad16(Lk * 4) if has_index else 0) + (128 * nkt * 4 if has_bits else 0)


def dkv_lds_bytes(nqt, has_bits, has_drop):
    """fa_dkv_smem_bytes: ring | flags | 128 visibility rows | lse2 + delta | dropout tile keys"""
    return FA_RING + _pad16(nqt) + (128 * nqt * 4 if has_bits else 0) + 2 * 32 * nqt * 4 + (4 * 32 * nqt * 4 if has_drop else 0)


def ring_kernels(case, mt):
    """(forward + dQ take the ring kernels?, dK/dV takes the ring kernel?) for a head-width-64 case, by the LDS formulas"""
    Lq, Lk = case["Lq"], (case["Lk"] if mt is None else mt.Lk)
    nqt, nkt = _tile_grid(Lq, Lk)
    has = mt is not None
    return (ring_lds_bytes(nkt, Lk, has and mt.key_index is not None, has) <= RING_LDS_LIMIT,
            dkv_lds_bytes(nqt, has, case["dropout_p"] > 0) <= DKV_LDS_LIMIT)


# ---------------------------------------------------------------------------------------------------
# the fp32 oracle under masks with blind rows: the convention applied from outside
# ---------------------------------------------------------------------------------------------------
def attention_fp32_blind(q, k, v, vis, scale=None, drop=None, drop_cols=None):
    """oracle/torch_ref.py::attention (unchanged) under a mask with blind rows: softmax of an all -inf row is NaN there, so blind
    rows are made all-visible in the mask handed to it and its output rows multiplied by the not-blind indicator -- o = 0 for a
    blind query, and through autograd dq = 0 and no contribution to dk / dv: the kernels' convention."""
    from oracle import torch_ref as R
    v_t = torch.from_numpy(vis)
    seen = v_t.any(dim=1)
    o = R.attention(q, k, v, scale=scale, mask=additive((v_t | ~seen[:, None]).numpy()), drop=drop, drop_cols=drop_cols)
    return o * seen.view(1, 1, -1, 1).to(o.dtype)
