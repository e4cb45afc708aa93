"""Every case of tests/rowwise_cases.py reaches the loop, template instance or branch it is listed for (from the launch geometry
restated there), and its data meets the conditions the acceptance criteria of the GPU tests rest on.  No GPU, no library."""
import pytest
import torch

from oracle import torch_ref as R
from tests import rowwise_cases as RC


def _ids(cases):
    return [c["id"] for c in cases]


@pytest.mark.parametrize("case", RC.LN_CASES, ids=_ids(RC.LN_CASES))
def test_layernorm_case_reaches_its_path(case):
    rows, cols = case["rows"], case["cols"]
    assert RC.ln_supported(cols)
    f, b = RC.ln_geometry(rows, cols), RC.ln_geometry(rows, cols, backward=True)
    for word in case["path"].split():
        if word == "fwd-2-trips-last-partial":
            assert f["trips"] == 2 and 0 < f["last_trip_rows"] < f["rows_per_trip"] and f["blocks"] == RC.LN_FWD_MAX_BLOCKS
        elif word == "fwd-3-trips-prefetch":           # prefetch on every trip but the last, and a partly empty last trip
            assert f["trips"] >= 3 and f["prefetch_trips"] == f["trips"] - 1 >= 2 and 0 < f["last_trip_rows"] < f["rows_per_trip"]
        elif word == "bwd-3-trips":
            assert b["trips"] == 3 and b["blocks"] == RC.LN_BWD_MAX_BLOCKS
        elif word == "bwd-2-trips":
            assert b["trips"] == 2 and b["prefetch_trips"] == 1 and 0 < b["last_trip_rows"] < b["rows_per_trip"]
        elif word == "lanes-1":
            assert f["vpl"] == 1 and f["last_slot_lanes"] == 1
        elif word == "vpl-2":
            assert f["vpl"] == 2 and f["last_slot_lanes"] == 1
        elif word == "ragged":
            assert rows == 9 and f["blocks"] == 3 and f["trips"] == 1          # three workgroups, the last one with a single row
            assert (f["vpl"], f["last_slot_lanes"]) == RC.RAGGED_EXPECT[cols]
        elif word == "model-width":
            assert rows == 64 and (cols, case["eps"]) in ((768, 1e-6), (1024, 1e-5))
        else:
            raise AssertionError(f"unknown path word {word}")
    if case["kind"] == "fork":
        assert "fwd" not in case["path"]


def test_ragged_cases_cover_every_template_instance_with_full_and_single_lane_slots():
    got = {RC.RAGGED_EXPECT[c][0] for c in RC.RAGGED_COLS}
    assert got == {1, 3, 4} and RC.ln_geometry(9, 520)["vpl"] == 2
    for vpl in (1, 3, 4):
        lanes = {RC.RAGGED_EXPECT[c][1] for c in RC.RAGGED_COLS if RC.RAGGED_EXPECT[c][0] == vpl}
        assert {1, 64} <= lanes
    ids = set(_ids(RC.LN_CASES))
    for k in ("plain", "fork"):
        assert {f"{k}-9x1032-mixed-pf32", f"{k}-9x1544-mixed-pf32", f"{k}-9x1032-mixed-noaffine"} <= ids
    assert len(ids) == len(RC.LN_CASES)


@pytest.mark.parametrize("case", RC.LAST_TOKENS_CASES, ids=_ids(RC.LAST_TOKENS_CASES))
def test_last_tokens_case_reaches_its_path(case):
    n, L, keep, cols = case["n"], case["L"], case["keep"], case["cols"]
    g = RC.ln_group_geometry(n, L, keep)
    f, b = RC.ln_geometry(g["rows"], cols), RC.ln_geometry(g["rows"], cols, backward=True)
    for word in case["path"].split():
        if word == "bwd-2-trips":
            assert b["trips"] >= 2
        elif word == "fwd-2-trips":
            assert f["trips"] >= 2
        elif word == "zero-fill-later":
            assert g["zero_rows_per_group"] > 0 and g["zero_fill_later"]
        elif word == "nothing-to-fill":
            assert g["zero_rows_per_group"] == 0 and g["zero_fill_later"]
        else:
            raise AssertionError(word)


@pytest.mark.parametrize("case", RC.CONCAT_CASES, ids=_ids(RC.CONCAT_CASES))
def test_concat_case_reaches_its_path(case):
    a = RC.ln_geometry(case["n"] * case["La"], case["cols"], backward=True)
    b = RC.ln_geometry(case["n"] * case["Lb"], case["cols"], backward=True)
    if case["path"] == "bwd-2-trips":
        assert a["trips"] == 2 and 0 < a["last_trip_rows"] < a["rows_per_trip"] and b["trips"] == 1
    else:
        assert case["path"] == "one-trip" and a["trips"] == 1 and b["trips"] == 1
    assert any(not c["a_needs_grad"] for c in RC.CONCAT_CASES if c["path"] == "bwd-2-trips")


def test_refused_widths_are_outside_the_kernels_range():
    assert [RC.ln_supported(c) for c in RC.LN_REFUSED_COLS] == [False, False]
    assert RC.LN_REFUSED_COLS[0] % 8 != 0 and RC.LN_REFUSED_COLS[1] % 8 == 0 and RC.LN_REFUSED_COLS[1] > 2048


# ---------------------------------------------------------------------------------------------------
# data conditions
# ---------------------------------------------------------------------------------------------------
_DATA_KEYS = sorted({(c["data"], c["rows"], c["cols"], c["eps"]) for c in RC.LN_CASES if c["rows"] <= 64} |
                    {("mixed", 8197, 64, 1e-5), ("mixed", 3077, 520, 1e-5)})


@pytest.mark.parametrize("data,rows,cols,eps", _DATA_KEYS)
def test_layernorm_data_is_conditioned_as_the_criterion_assumes(data, rows, cols, eps):
    x, names = RC.make_rows(data, rows, cols, seed=1, eps=eps)
    assert x.shape == (rows, cols) and torch.equal(x, RC.bf16_round(x)) and bool(torch.isfinite(x).all())
    kappa, _, _, const = RC.row_kappa(x, eps)
    want_const = torch.tensor([n == "const" for n in names])
    assert torch.equal(const, want_const) or cols == 1
    assert float(kappa[~const].max() if (~const).any() else 0.0) <= RC.KAPPA_MAX
    if const.any():
        assert float(x[const].abs().max()) <= RC.CONST_MAX
    if data == "mixed":
        assert set(names) == set(RC.ROW_CLASSES) and names[:7] == RC.ROW_CLASSES
    x2, _ = RC.make_rows(data, rows, cols, seed=1, eps=eps)
    assert torch.equal(x, x2)          # seeded


def test_row_classes_are_what_they_are_called():
    eps = 1e-5
    x, _ = RC.make_rows("offset", 10, 768, 3, eps)
    m = x.double().mean(-1)
    for r, (mean, std) in enumerate(RC.OFFSETS * 2):
        assert abs(float(m[r]) - mean) < 0.5 * std and float(x[r].double().std()) >= 0.9 * std
    x, _ = RC.make_rows("outlier", 4, 768, 3, eps)
    assert float(x[:, ::193].abs().median()) > 100 and float(x[:, 1:193].abs().max()) < 12
    x, _ = RC.make_rows("rowscale", 21, 512, 3, eps)
    s = x.double().std(-1)
    assert 2.0 ** -10.2 < float(s[0]) / 2 < 2.0 ** -9.8 and 2.0 ** 9.8 < float(s[-1]) / 2 < 2.0 ** 10.2
    x, _ = RC.make_rows("tiny", 4, 768, 3, eps)
    assert float(x.double().var(-1).max()) < 10 * eps
    x, _ = RC.make_rows("huge", 4, 768, 3, eps)
    assert float(x.double().std(-1).min()) > 1e4


# ---------------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------------
def test_activation_inputs_are_every_finite_bf16_value_up_to_2_pow_40():
    x = RC.act_inputs()
    assert x.dtype == torch.bfloat16 and x.numel() == 2 * (((127 + 40) << 7) + 1) == 42754
    v = x.double()
    assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 2.0 ** 40
    assert x.view(torch.int16).unique().numel() == x.numel()
    # the next bf16 value is outside
    nxt = torch.tensor([((127 + 40) << 7) + 1], dtype=torch.int16).view(torch.bfloat16)
    assert float(nxt) > 2.0 ** 40 and float(v.abs().max()) ** 3 < torch.finfo(torch.float32).max
    g = RC.ew_geometry(x.numel() * RC.ACT_TILE)
    assert RC.ew_geometry(x.numel())["trips"] == 1 and g["trips"] == 2 and g["blocks"] == RC.EW_MAX_BLOCKS


def test_cast_inputs_hold_every_tie_and_take_the_second_trip():
    x = RC.cast_f2b_inputs()
    bits = x.view(torch.int32).long() & 0xFFFFFFFF
    ties = bits[(bits & 0xFFFF) == 0x8000]
    mags = (ties & 0x7FFFFFFF) >> 16
    assert set(range(0, 0x7F7F)) <= set(mags.tolist())                      # a tie above every finite bf16 value but the largest
    for s in (0, 0x80000000):
        have = set((bits[(bits & 0x80000000) == s] & 0x7FFFFFFF).tolist())
        assert {0x3F808000 - 1, 0x3F808000, 0x3F808000 + 1, 0x3F818000} <= have      # ties to even AND to odd neighbours
    assert int(torch.isnan(x).sum()) >= 3 and int(torch.isinf(x).sum()) == 2 and 0x7F7FFFFF in set(bits.tolist())
    assert RC.ew_geometry(x.numel() * RC.CAST_F2B_TILE)["trips"] == 2
    y = RC.cast_b2f_inputs()
    assert y.view(torch.int16).unique().numel() == 65536 and RC.ew_geometry(y.numel() * RC.CAST_B2F_TILE)["trips"] == 2


def test_dropout_and_add_cases_reach_their_paths():
    for c in RC.DROPOUT_CASES:
        g = RC.ew_geometry(c["rows"] * c["cols"], per_thread=2)
        assert g["odd"]                                     # one thread's second element lies behind the end
        p32 = float(torch.tensor(c["p"], dtype=torch.float32))
        assert bool(R.drop_keep_mask((123, 456), torch.tensor(c["rows"] - 1), torch.tensor(c["cols"] - 1), p32))      # the last element is kept
        assert g["trips"] == (2 if "trips-2" in c["path"] else 1)
    for c in RC.ACT_BWD_DROP_CASES:
        g = RC.ew_geometry(c["rows"] * c["cols"])
        assert g["trips"] == (2 if c["path"] == "trips-2" else 1)
        if c["path"] == "shape-not-taken-by-colsum":
            assert c["cols"] % 8 != 0
    assert {(c["rows"], c["cols"], c["p"], c["act"]) for c in RC.ACT_BWD_DROP_CASES} == \
        {(r, co, p, a) for (r, co) in ((4099, 257), (100, 36)) for p in (0.1, 0.5) for a in ("none", "gelu_tanh")}
    for c in RC.ADD_CASES:
        g = RC.ew_geometry(c["n"])
        assert (g["trips"], g["blocks"]) == ((2, RC.EW_MAX_BLOCKS) if c["path"] == "trips-2" else (1, 1))
    assert {(c["n"], c["period"]) for c in RC.ADD_CASES} == {(n, p) for n in (1_048_833, 63) for p in (0, 24, 257)}


@pytest.mark.parametrize("case", RC.COLSUM_CASES, ids=_ids(RC.COLSUM_CASES))
def test_colsum_case_reaches_its_path(case):
    g = RC.colsum_case_geometry(case)
    for word in case["path"].split():
        if word == "all-slabs":
            assert g["slabs"] == RC.CS_MAX_SLABS and not g["capped"]
        elif word == "slab-cap":
            assert g["slabs"] == RC.CS_MAX_SLABS and g["capped"]
        elif word == "rows-lt-16":
            assert case["rows"] < 16 and g["slabs"] == 1 and case["rows"] % 4 != 0
        elif word == "ragged":
            assert g["vec_ok"] and g["ragged_last_octet"] and g["scalar_lanes"] == 1
        elif word == "strips-2":
            assert g["strips"] == 2
        elif word == "view":
            assert RC.colsum_case_ld(case) > case["cols"]
        elif word == "vec":
            assert g["vec_ok"]
        elif word == "scalar":
            assert not g["vec_ok"] and g["scalar_lanes"] == -(-case["cols"] // 8)
        else:
            raise AssertionError(word)


def test_colsum_views_cover_an_unaligned_origin_and_an_unaligned_leading_dimension():
    views = [c for c in RC.COLSUM_CASES if c["pad"] is not None]
    assert any(c["offset"] % 8 and RC.colsum_case_ld(c) % 8 == 0 for c in views)
    assert any(c["offset"] == 0 and RC.colsum_case_ld(c) % 8 for c in views)
    assert any(c["offset"] == 0 and RC.colsum_case_ld(c) == 2 * c["cols"] + 8 and RC.colsum_case_ld(c) % 8 == 0 for c in views)
    # the 16-byte branch with a ragged last octet exists only under a view: cols % 8 != 0 makes a contiguous operand's ld unaligned
    assert all(not RC.colsum_case_geometry(c)["vec_ok"] for c in RC.COLSUM_CASES if c["pad"] is None and c["cols"] % 8)
    assert sum(g["vec_ok"] and g["ragged_last_octet"] for g in map(RC.colsum_case_geometry, views)) == 2
    for c in RC.ACT_BWD_COLSUM_CASES:
        g = RC.colsum_geometry(c["rows"], c["cols"])
        assert g["slabs"] == RC.CS_MAX_SLABS and g["capped"] == ("slab-cap" in c["path"]) and c["cols"] == 8
