"""GPU: the attention kernels (csrc/attention.hip, csrc/attention_hd.hip) under arbitrary 0 / -inf masks -- Bernoulli masks, random
empty / full / mixed tiles, queries that see no key, dead keys, hand-placed walks, corner bits, Lq != Lk, the 64-tile boundary of the
ballot words, tables without key compaction, several items per workgroup (tests/attention_mask_cases.py has the generators and the
case list, tests/test_attention_mask_cases.py asserts on the CPU that every case has the structure it is named for).

Per case (tests/gpu_checks.py::check_attention_masked): o, dq, dk, dv against oracle/torch_ref.py::attention_bf16 at the unchanged
TOL_ATTN / TOL_ATTN_GRAD (rel-L2 and element-wise), lse against the oracle's, and -- exactly, no tolerance -- the convention for a
query that sees no key (o = 0, lse = +inf, dq = 0), which gradient rows are written and which keep their NaN pre-fill, and bit
equality of repeated batch rows.  One row per case goes to $DVLA_PARITY_REPORT (profiles/r15_parity_attention_masks.jsonl).

Measured on an MI355X: 32 rows, all ok; worst rel-L2 o 8.4e-5, dq 1.8e-4, dk 1.8e-4, dv 1.6e-4 (o bit-identical to the oracle in 15 rows);
the file runs in about 4 s.  What the value checks can see, measured by handing the ORACLE a wrong mask: one flipped bit fails them
in the L = 133 / 261 cases (rel-L2 2.5e-3 ... 4e-1); at L = 2016 a query sees ~700 keys and one flipped bit stays below the
tolerances -- the long cases are there for the tile walks, not for single bits."""
import pytest

from tests import attention_mask_cases as MC
from tests import gpu_checks as G


def _report(case_id, struct, results):
    from tests.model_checks import report
    row = {"case": case_id, **{k: struct[k] for k in ("empty", "full", "mixed", "blind", "dead")}}
    for m in results:
        for t in ("o", "dq", "dk", "dv"):
            if m["name"].endswith(" " + t) and "max_abs" in m:
                row[t + "_rel_l2"] = float("%.4g" % max(m["rel_l2"], row.get(t + "_rel_l2", 0.0)))
                row[t + "_max_abs"] = float("%.4g" % max(m["max_abs"], row.get(t + "_max_abs", 0.0)))
    nan_mem = [m["gradient_memory_was_nan"] for m in results if "gradient_memory_was_nan" in m]
    if nan_mem:
        row["gradient_memory_was_nan"] = all(nan_mem)
    row["ok"] = all(m["ok"] for m in results)
    report([row])


def _assert_all(results):
    for m in results:
        print(("ok   " if m["ok"] else "FAIL ") + m["name"], "rel_l2=%.3g max_abs=%s tol=%s worst=%s" %
              (m.get("rel_l2", 0.0), m.get("max_abs"), m.get("max_abs_tol"), m.get("worst_index")))
    bad = [m for m in results if not m["ok"]]
    assert not bad, "; ".join(f"{m['name']}: rel_l2={m.get('rel_l2')} max_abs={m.get('max_abs')} tol={m.get('tol')} "
                              f"worst_index={m.get('worst_index')}" for m in bad)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in MC.CASES])
def test_attention_under_arbitrary_masks(cid):
    results, struct = G.check_attention_masked(MC.BY_ID[cid])
    _report(cid, struct, results)
    _assert_all(results)


@pytest.mark.gpu
def test_self_attention_backward_writes_every_row_without_key_compaction():
    """ops.self_attention(...).backward twice in a row under uncompacted tables with dead keys: the gradient buffer is
    torch.empty_like and nothing zero-fills it -- qkv.grad is finite and equal to the oracle's"""
    case = MC.BY_ID["blind-D64-L133-uncompacted"]
    results = G.check_self_attention_uncompacted(case)
    vis, _, mt = MC.tables(case)
    _report(case["id"] + " through ops.self_attention", MC.structure(vis, mt), results)
    _assert_all(results)
