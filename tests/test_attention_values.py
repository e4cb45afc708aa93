"""CPU: the reference, yardstick and cases of tests/attention_value_ref.py mean what tests/test_attention_values_gpu.py takes them to
mean.
  pin        attention_ref in float32 without chunking, jitter or o_stored returns the bits of oracle/torch_ref.py::attention_bf16
  cap        every case: 4 E <= 1e-2 and 4 U <= 16 for every tensor -- the allowance the GPU test grants stays far below the ~256 ulps
             of a misplaced row, and a case that is ill-conditioned for any bf16 flash attention is not in the list
  structure  every case is what its name says (one-hot rows, rising maxima, hidden logits far above visible ones, ...) and reaches the
             kernel family it is listed under, by the dispatch conditions of csrc/attention.hip
  teeth      float32 restatements that are wrong on purpose FAIL the criterion in the cases named for them; and the criterion's own
             mutant -- the oracle's own o and the fixed suite tolerance, the way every other attention test compares -- rejects a CORRECT
             float32 variant on the sink cases, which is why the backward reference is conditioned on the stored o"""
import pytest
import torch

from oracle import torch_ref as R
from tests import attention_mask_cases as MC
from tests import attention_value_ref as V

IDS = [c["id"] for c in V.CASES]


def _unit_inputs(B, H, Lq, Lk, D, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: R.bf16_round(torch.randn(*s, generator=g))
    return mk(B, H, Lq, D), mk(B, H, Lk, D), mk(B, H, Lk, D), mk(B, H, Lq, D)


@pytest.mark.parametrize("kind", ["mask", "dropout", "mask+dropout, Lq != Lk"])
def test_reference_is_pinned_to_the_oracle_bit_for_bit(kind):
    Lq, Lk = (40, 133) if "!=" in kind else (133, 133)
    q, k, v, do = _unit_inputs(2, 2, Lq, Lk, 64, 3)
    mask = MC.additive(MC.blind(Lq, Lk, 0)) if "mask" in kind else None
    drop = (0.1, (11, 22)) if "dropout" in kind else None
    want = R.attention_bf16(q, k, v, scale=0.125, mask=mask, drop=drop, dout=do)
    got = V.attention_ref(q, k, v, do, dtype=torch.float32, scale=0.125, mask=mask, drop=drop)
    for name, w in zip(V.TENSORS, want):
        assert torch.equal(got[name], w), name
    if mask is not None:
        assert bool(torch.isinf(want[1]).any())           # blind rows are part of the pin


def test_case_list_covers_every_family():
    fam = lambda f, **kw: {c["regime"] for c in V.CASES if c["family"] == f and all(c[k] == v for k, v in kw.items())}
    assert len(V.CASES) <= 64
    for f in ("short", "ring_fwd_short_bwd", "ring", "hd", "small"):
        assert set(V.FIVE) <= fam(f), f
    masked = lambda f: {c["regime"].split(":")[0] for c in V.CASES if c["family"] == f and c["mask"]}
    for f in ("ring", "staged", "hd"):
        assert "hidden_giant" in masked(f), f
    assert len(fam("staged")) == 2
    assert fam("short", Lq=197) and fam("short", Lq=261) and fam("ring", Lq=333) and fam("ring", p=0.1)
    assert fam("ring", mask="blind", compact=False) and fam("ring", mask="tiles") and fam("ring", Lq=40, Lk=133) and fam("ring", Lq=133, Lk=40)
    assert {c["D"] for c in V.CASES if c["family"] == "hd"} == {24, 32, 48, 96, 128}
    assert any(c["p"] > 0 for c in V.CASES if c["family"] == "hd")
    assert {c["Lq"] for c in V.CASES if c["family"] == "small"} == {6, 64}
    assert {c["via"] for c in V.CASES if c["D"] == 64 and c["regime"] == "sink_first"} == {"raw", "self", "cross"}
    assert {"ties_q0", "ties_rows", "ties_keys", "exact", "tiny", "big", "sharp", "sharp32", "stair_down", "unit"} <= {c["regime"] for c in V.CASES}
    assert all(c["regime"].split(":")[0] in V.REGIMES or c["regime"].startswith("hidden_giant:") for c in V.CASES)


@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_the_family_it_is_listed_under(cid):
    from dreamvla_amd import ops
    case = V.BY_ID[cid]
    vis = V.visibility(case)
    mt = V.tables(case, vis)
    if case["family"] == "small":
        assert case["via"] == "self" and case["D"] != 64 and mt is None and case["p"] == 0 and ops._small_attention_fits(case["B"], case["Lq"], case["D"])
        return
    if case["family"] == "hd":
        assert ops.attn_hd_supported(case["D"]) and not (case["via"] == "self" and mt is None and case["p"] == 0 and case["Lq"] <= 64)
        return
    assert case["D"] == 64
    want = {"short": ("short", "short"), "ring_fwd_short_bwd": ("ring", "short"), "ring": ("ring", "ring"), "staged": ("staged", "staged")}
    assert V.dispatch(case, mt) == want[case["family"]]
    if vis is not None and not case["compact"]:
        assert mt.key_index is None and mt.Lk == case["Lk"]


def _float64_scores(case, data):
    """(s2 masked, s2 unmasked, P) of the float64 reference, log2 domain"""
    q, k = data["q"].double(), data["k"].double()
    s2 = torch.matmul(q, k.transpose(-1, -2)) * (case["D"] ** -0.5 * V.LOG2E)
    masked = s2 if data["vis"] is None else torch.where(torch.from_numpy(data["vis"]), s2, torch.full_like(s2, float("-inf")))
    P = torch.softmax(masked * V.LN2, dim=-1)
    return masked, s2, P


@pytest.mark.parametrize("cid", IDS)
def test_case_meets_the_cap_and_is_what_its_name_says(cid):
    case = V.BY_ID[cid]
    data, yard = V.yardstick(case)
    for t in (data["q"], data["k"], data["v"], data["dout"]):
        assert torch.equal(t, R.bf16_round(t)) and bool(torch.isfinite(t).all())
    print({t: ("%.2e" % yard["E"][t], "%.2f" % yard["U"][t]) for t in V.TENSORS})
    for t in V.TENSORS:
        if t == "dq" and case["regime"] == "ties_keys":
            continue                                      # true value 0: judged by dq_zero_bound, not against the reference
        assert V.MARGIN * yard["E"][t] <= V.CAP_E and V.MARGIN * yard["U"][t] <= V.CAP_U, (t, yard["E"][t], yard["U"][t])
    ref = yard["ref_fwd"]
    vis = data["vis"]
    blind = torch.zeros(case["Lq"], dtype=torch.bool) if vis is None else torch.from_numpy(~vis.any(axis=1))
    assert bool(torch.isfinite(ref["o"]).all()) and bool(torch.isfinite(ref["lse"][..., ~blind]).all())
    assert bool((ref["lse"][..., blind] == float("inf")).all()) and bool((ref["o"][:, :, blind] == 0).all())
    masked, s2, P = _float64_scores(case, data)
    seen = ~blind
    top = P[:, :, seen].amax(dim=-1)
    regime = case["regime"]
    base = regime.split(":")[-1]
    nkt = (case["Lk"] + 31) // 32
    if base in ("sink_first", "sink_last"):
        # rows that can see the sink key put (almost) everything on it
        j = 0 if base == "sink_first" else case["Lk"] - 1
        sees = seen if vis is None else torch.from_numpy(vis[:, j].copy())
        if regime == base:
            assert int(sees.sum()) >= 0.2 * int(seen.sum())
            on_sink = P[:, :, sees][..., j]
            assert float((on_sink > 0.99).double().mean()) >= 0.9, float((on_sink > 0.99).double().mean())
        if base == "sink_last" and vis is None and nkt > 1:
            # the last tile lifts the running maximum by ~40 log2 units: what was accumulated is rescaled by ~2^-40
            run = V.tile_running_max(masked)
            assert float((run[..., -1] - run[..., -2]).median()) >= 32
    if base in ("stair_up", "stair_down"):
        run = V.tile_running_max(masked)[:, :, seen]
        fin = torch.isfinite(run[..., :-1])
        rises = ((run[..., 1:] > run[..., :-1]) & fin).sum(dim=-1).double()
        if base == "stair_up" and vis is None:
            # a step of 8 in the logit per full tile against a noise of std ~2: (nearly) every row, every full tile -- a ragged last
            # tile of a few keys need not hold the row's largest logit
            full = max(case["Lk"] // 32, 2)
            assert float(rises.mean()) >= 0.9 * (full - 1) and float(rises.min()) >= (full - 2) / 2, (float(rises.mean()), float(rises.min()))
        elif base == "stair_up":
            # under a mask a row skips the tiles it cannot see: alpha != 1 still more than once per row on average
            assert float(rises.mean()) >= min(1.5, 0.5 * (nkt - 1)), float(rises.mean())
        else:
            assert float(rises.median()) == 0 and float(rises.mean()) <= 0.25
    if base == "row_temps":
        wave = top[:, :, :32] if int(seen[:32].all()) else top
        assert float(wave.min()) < 0.3 and float(wave.max()) > 0.99     # flat and one-hot rows among the 32 lanes of one wave
    if base in ("sharp", "sharp32"):
        assert float((top > 0.5).double().mean()) >= 0.7
        if base == "sharp32":
            assert float(s2.abs().max()) >= 150
    if base == "outlier":
        assert float(masked[torch.isfinite(masked)].mean()) * V.LN2 >= 30        # the common offset of every logit
    if base == "tiny":
        assert float(s2.abs().max()) < 1e-6 and float(data["dout"].abs().max()) < 1e-3
    if base in ("ties_q0", "ties_keys", "exact"):
        n = (torch.from_numpy(vis).sum(dim=-1) if vis is not None else torch.full((case["Lq"],), case["Lk"])).double()
        assert torch.allclose(P[:, :, seen], (1.0 / n[seen]).view(1, 1, -1, 1).expand_as(P[:, :, seen]), rtol=1e-12, atol=0)
    if base == "ties_rows":
        assert bool((P == P[:, :, :1]).all())
    if base == "exact":
        assert case["Lk"] == 256 and bool((P == 2.0 ** -8).all())
        exact_o = data["v"].double().sum(dim=2, keepdim=True).expand_as(ref["o"]) / 256.0
        assert torch.equal(ref["o"], exact_o.to(torch.bfloat16).double())
        assert torch.equal(ref["dv"], (data["dout"].double().sum(dim=2, keepdim=True).expand_as(ref["dv"]) / 256.0).to(torch.bfloat16).double())
    if regime.startswith("hidden_giant:"):
        # every row that sees anything: the largest hidden logit is >= 2^5 log2 units above the largest visible one -- and past the
        # 149 units at which a maximum taken before the mask underflows the whole row in fp32
        hidden = torch.where(torch.from_numpy(vis), torch.full_like(s2, float("-inf")), s2).amax(dim=-1)
        excess = (hidden - masked.amax(dim=-1))[..., seen]
        assert int(seen.sum()) > 0 and float(excess.min()) >= 2 ** 5 and float(excess.min()) >= 150, float(excess.min())
        dead = ~vis.any(axis=0)
        assert dead.sum() >= 8 and (dead[:-1] & dead[1:])[31::32].any()       # a dead span across a tile boundary


def _variant(case, data, mutant=None, chunk=16, jitter=V.JITTER):
    kw = V.reference_kwargs(case, data, V._tables_for_drop(case, data))
    return V.attention_ref(data["q"], data["k"], data["v"], data["dout"], dtype=torch.float32, chunk=chunk, exp_jitter=jitter,
                           jitter_seed=77, mutant=mutant, **kw)


def _verdict(case, data, yard, got, **kw):
    res = V.judge(case, data, yard, {t: got[t] for t in V.TENSORS}, tag=case["id"], **kw)
    return all(m["ok"] for m in res), {m["name"]: ("%.2e" % m["rel_l2"], m["ok"]) for m in res}


def _first(family, regime, **kw):
    return next(c for c in V.CASES if c["family"] == family and c["regime"] == regime and c["via"] == "raw"
                and all(c[k] == v for k, v in kw.items()))


MUTANTS = [("max_before_mask", ("ring", "hidden_giant:sink_first", {"mask": "blind"})),
           ("max_before_mask", ("ring", "hidden_giant:stair_up", {})),
           ("max_before_mask", ("hd", "hidden_giant:sink_first", {})),
           ("skip_alpha", ("ring", "stair_up", {"Lq": 333})),
           ("skip_alpha", ("short", "stair_up", {"Lq": 197})),
           ("skip_alpha", ("ring", "sink_last", {"Lq": 333})),
           ("skip_alpha", ("ring_fwd_short_bwd", "sink_last", {})),
           ("delta_unrounded", ("ring", "sink_first", {"Lq": 333})),
           ("delta_unrounded", ("short", "sink_first", {}))]


@pytest.mark.parametrize("mutant,which", MUTANTS, ids=[f"{m}-{w[1]}-{i}" for i, (m, w) in enumerate(MUTANTS)])
def test_criterion_rejects_a_wrong_restatement_and_accepts_the_right_one(mutant, which):
    case = _first(which[0], which[1], **which[2])
    data, yard = V.yardstick(case)
    ok, detail = _verdict(case, data, yard, _variant(case, data))
    assert ok, detail                                   # the unmutated float32 variant (a draw outside the ensemble) passes
    ok, detail = _verdict(case, data, yard, _variant(case, data, mutant=mutant))
    print(detail)
    assert not ok, detail


@pytest.mark.parametrize("cid", [c["id"] for c in V.CASES if c["regime"] in ("sink_first", "sink_last") and c["mask"] is None
                                 and c["via"] == "raw" and c["p"] == 0 and c["D"] == 64])
def test_the_old_comparison_rejects_a_correct_variant_on_the_sink_cases(cid):
    """the oracle's own o and the fixed suite tolerances: a correct float32 variant (chunks of 16, jittered exp2) FAILS -- its stored o
    differs from the oracle's by single bf16 flips and P (dP - delta) amplifies them -- while the conditioned comparison accepts it"""
    case = V.BY_ID[cid]
    data, yard = V.yardstick(case)
    var = _variant(case, data)
    ok, detail = _verdict(case, data, yard, var)
    assert ok, detail
    ok, detail = _verdict(case, data, yard, var, fixed=True, conditioned=False)
    print(detail)
    assert not ok, detail
