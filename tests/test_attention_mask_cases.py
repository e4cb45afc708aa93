"""CPU: the cases of tests/attention_mask_cases.py have the structure they are named for -- the GPU run of
tests/test_attention_masks_gpu.py is worth nothing if a seed happens to miss it -- and oracle/torch_ref.py::attention_bf16 is
finite on every one of them, with the kernels' convention for a query that sees no key."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests import attention_mask_cases as MC

IDS = [c["id"] for c in MC.CASES]


def test_case_list_covers_what_the_kernels_branch_on():
    fam = lambda f, **kw: [c for c in MC.CASES if c["family"] == f and all(c[k] == v for k, v in kw.items())]
    for f in ("bern", "tiles", "blind", "edges", "corner"):
        assert fam(f, D=64, Lq=133, Lk=133, dropout_p=0.0), f
    assert fam("tiles", D=64, dropout_p=0.1) and fam("blind", D=64, dropout_p=0.1)
    assert fam("blind", Lq=261) and fam("edges", Lq=261)
    assert fam("blind", compact=False)
    for shape in ((40, 133), (133, 40), (1, 70), (70, 33)):
        assert fam("tiles", D=64, Lq=shape[0], Lk=shape[1]) and fam("blind", D=64, Lq=shape[0], Lk=shape[1])
    assert {c["order"] for c in fam("tiles", D=64, Lq=133, B=2, dropout_p=0.0)} == {"default", "natural", "random"}
    assert {c["order"] for c in fam("blind", D=64, Lq=133, dropout_p=0.1)} == {"default", "natural", "random"}
    assert {(c["D"], c["family"]) for c in MC.CASES if c["D"] != 64} == {(32, "tiles"), (96, "blind"), (128, "edges"), (24, "blind"),
                                                                          (48, "tiles")}
    many = fam("tiles", B=64, H=8)[0]
    assert many["period"] == 5 and many["rows"] == 6


def test_generators_are_deterministic():
    for c in MC.CASES:
        if c["Lq"] <= 261 and c["family"] != "none":
            assert np.array_equal(MC.visibility(c), MC.visibility(c))


@pytest.mark.parametrize("cid", IDS)
def test_case_has_the_structure_it_is_named_for(cid):
    case = MC.BY_ID[cid]
    vis, mask, mt = MC.tables(case)
    got = MC.structure(vis, mt)
    exp = case["expect"]
    for k in ("empty", "full", "mixed", "blind", "dead"):
        assert got[k] >= exp.get(k, 0), (k, got, exp)
    if "index" in exp:
        assert got["index"] == exp["index"], got
    if vis is None:
        return
    assert (mt.Lq, mt.Lk_full) == (case["Lq"], case["Lk"])
    if case["compact"]:
        assert mt.Lk == case["Lk"] - got["dead"]
    else:
        assert mt.Lk == case["Lk"] and mt.key_index is None and not hasattr(mt, "dead_keys")
    if case["family"] == "bern":
        assert got["mixed"] == mt.tile_map.numel()
    if case["family"] == "blind":
        rows, (lo, hi) = MC.blind_rows(case["Lq"]), MC.dead_span(case["Lk"])
        assert not vis[rows].any() and not vis[:, lo:hi].any() and lo // 32 != (hi - 1) // 32
        one = int((vis.sum(axis=1) == 1).sum())
        assert one <= case["Lq"] // 4 and (one >= 2 or case["Lq"] < 64)
        if case["Lq"] >= 96:
            assert 7 in rows and set(range(32, 64)) <= set(rows) and rows[-1] == case["Lq"] - 1
        if case["Lq"] >= 256:
            assert set(range(128, 256)) <= set(rows)
        if case["Lk"] >= 128:
            assert lo <= 64 and hi >= 96                      # a whole key tile is dead
    if case["family"] == "corner":
        tile = lambda qt, kt: vis[qt * 32:(qt + 1) * 32, kt * 32:(kt + 1) * 32]
        singles, complements = set(), set()
        for qt in range(4):
            for kt in range(4):
                t = tile(qt, kt)
                n = int(t.sum())
                assert n in (1, 1023)
                where = tuple(int(x) for x in np.argwhere(t if n == 1 else ~t)[0])
                assert where in ((0, 0), (0, 31), (31, 0), (31, 31))
                (singles if n == 1 else complements).add(where)
        assert len(singles) == 4 and len(complements) == 4


@pytest.mark.parametrize("L", sorted(MC.EDGES_WALKS))
def test_edges_walk_patterns(L):
    """the exact walks of `edges`: per 128-query block the key tiles of the forward / dQ walk, per 128-key block the query tiles of
    the dK/dV walk, and the tiles that are live for one wave only"""
    case = next(c for c in MC.CASES if c["family"] == "edges" and c["Lq"] == L and c["D"] == 64)
    vis, _, mt = MC.tables(case)
    tm = mt.tile_map.numpy()
    assert MC.walks(tm, "q") == MC.EDGES_WALKS[L]["q"] and MC.walks(tm, "k") == MC.EDGES_WALKS[L]["k"]
    n = tm.shape[1]
    if L == 133:
        assert list(np.nonzero(tm[:4, 1])[0]) == [0] and list(np.nonzero(tm[:4, 2])[0]) == [3]      # wave 0 only, wave 3 only
        assert not tm[:4, 0].any() and not tm[:4, n - 1].any()                                       # first and last tile empty
        assert all((tm[qt] != 0).sum() == 1 for qt in range(4))                                      # one live tile per query tile
    else:
        assert all((tm[4:8, kt] != 0).sum() == 1 for kt in (0, 2, 4, 6, 8))                          # every tile: one wave only
        assert (tm[:4] != 0).sum(axis=0).tolist() == [0, 0, 0, 0, 0, 4, 0, 0, 0]                     # a walk of one live tile


def test_lds_formulas_put_the_boundary_cases_where_they_are_named():
    """recomputed from FA_RING = 32768, 128 n 4 (visibility rows), 2 * 32 n 4 (lse2 + delta) and 4 * 32 n 4 (dropout tile keys):
    L = 2048 unmasked and L = 2016 under `tiles` run all three ring kernels (64 and 63 tiles through the ballot words), L = 2085
    under `tiles` none of them (66 tiles: the LDS table walk of the staged kernels, with holes)"""
    assert MC.FA_RING == 32768 and MC.RING_LDS_LIMIT == 65536 and MC.DKV_LDS_LIMIT == 81920
    assert MC.ring_lds_bytes(63, 2016, False, True) == 32768 + 64 + 63 * 512 <= 65536
    assert MC.ring_lds_bytes(64, 2048, False, True) > 65536          # 2016 is the longest masked walk that fits
    assert MC.dkv_lds_bytes(63, True, False) == 32768 + 64 + 63 * 512 + 63 * 256 <= 81920
    assert MC.dkv_lds_bytes(63, True, True) > 81920
    seen = {}
    for c in MC.CASES:
        if "ring" in c["expect"]:
            _, _, mt = MC.tables(c)
            seen[c["Lq"]] = MC.ring_kernels(c, mt)
            assert seen[c["Lq"]] == c["expect"]["ring"], (c["id"], seen)
            assert mt is None or mt.key_index is None
    assert seen == {2048: (True, True), 2016: (True, True), 2085: (False, False)}
    assert -(-2048 // 32) == 64 and -(-2016 // 32) == 63 and -(-2085 // 32) == 66
    # every other head-width-64 case runs the ring kernels
    assert all(MC.ring_kernels(c, MC.tables(c)[2]) == (True, True) for c in MC.CASES if c["D"] == 64 and c["Lq"] < 2000)


def test_many_items_case_gives_some_workgroups_two_items():
    """ring_items_grid of csrc/attention.hip on 256 CUs: y = max(ceil(items / 4), ceil(3 * 256 / query blocks)), at most items"""
    c = next(c for c in MC.CASES if c["B"] == 64)
    items, nqb = c["B"] * c["H"], -(-c["Lq"] // 128)
    y = min(max(-(-items // 4), -(-3 * 256 // nqb)), items)
    assert (items, nqb, y) == (512, 2, 384) and y < items < 2 * y


@pytest.mark.parametrize("cid", IDS)
def test_faithful_oracle_is_finite_with_the_blind_convention(cid):
    case = MC.BY_ID[cid]
    vis, mask, _ = MC.tables(case)
    if vis is None:
        return
    H, Lq, Lk, D = 1, case["Lq"], case["Lk"], case["D"]
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: R.bf16_round(torch.randn(*s, generator=g))
    q, k, v, do = mk(1, H, Lq, D), mk(1, H, Lk, D), mk(1, H, Lk, D), mk(1, H, Lq, D)
    drop = (case["dropout_p"], (11, 22)) if case["dropout_p"] > 0 else None
    o, lse, dq, dk, dv = R.attention_bf16(q, k, v, scale=D ** -0.5, mask=mask, drop=drop, dout=do)
    blind, dead = ~vis.any(axis=1), ~vis.any(axis=0)
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t).all()
    assert torch.isfinite(lse[..., ~blind]).all() and (lse[..., blind] == float("inf")).all()
    assert (o[:, :, blind] == 0).all() and (dq[:, :, blind] == 0).all()
    assert (dk[:, :, dead] == 0).all() and (dv[:, :, dead] == 0).all()
