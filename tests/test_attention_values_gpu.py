"""GPU: the attention kernels (csrc/attention.hip staged / ring / short, csrc/attention_hd.hip, csrc/attention_small.hip,
csrc/attention_probe.hip) on peaked, saturated and degenerate VALUES -- one-hot rows, attention sinks on the first and on the last
key, running maxima that rise at every tile, eight temperatures inside one wave, outlier channels, tiny and big magnitudes, logits
hundreds of log2 units above everything visible behind the mask, ties, exact integers (tests/attention_value_ref.py has the
reference, the regimes and the case list; tests/test_attention_values.py asserts on the CPU that every case is what its name says,
meets the conditioning cap, and that wrong restatements fail the criterion used here).

Per case (tests/gpu_checks.py::check_attention_values): o and lse against the float64 reference; dq, dk, dv -- computed by the kernels
from their own o and lse -- against the float64 backward conditioned on the o the kernel stored; tol = max(suite, 4 E), k_ulp =
max(suite k, 4 U) with (E, U) the case's yardstick.  Exact: finiteness, the blind-row convention, o and dv of the `exact` family bit
for bit.  The probe: rows of the same regimes against a float64 softmax by its derived bound.  One row per case goes to
$DVLA_PARITY_REPORT (profiles/r24_parity_attention_values.jsonl): regime, family, E / U, the kernel's rel-L2 and ulps per tensor and
the fraction of its allowance it used."""
import pytest

from tests import attention_value_ref as V
from tests import gpu_checks as G

pytestmark = pytest.mark.gpu


def _finish(case, results, yard):
    from tests.model_checks import report
    sig = lambda x: float("%.3g" % x)
    row = {"case": case["id"], "regime": case["regime"], "family": case["family"], "via": case["via"]}
    for t in V.TENSORS:
        row[f"E_{t}"], row[f"U_{t}"] = sig(yard["E"][t]), sig(yard["U"][t])
    for m in results:
        for t in V.TENSORS:
            if m["name"].split(" (")[0].endswith(" " + t) and "allow_frac" in m:
                row[f"{t}_rel_l2"], row[f"{t}_ulps"], row[f"{t}_frac"] = sig(m["rel_l2"]), sig(m.get("ulps", 0.0)), sig(m["allow_frac"])
    row["worst_frac"] = sig(max([m["allow_frac"] for m in results if "allow_frac" in m] or [0.0]))
    row["ok"] = all(m["ok"] for m in results)
    report([row])
    for m in results:
        print(("ok   " if m["ok"] else "FAIL ") + m["name"], "rel_l2=%.3g tol=%.3g max_abs=%s max_abs_tol=%s frac=%s worst=%s" %
              (m.get("rel_l2", 0.0), m.get("tol", 0.0), m.get("max_abs"), m.get("max_abs_tol"), m.get("allow_frac"), m.get("worst_index")))
    bad = [m for m in results if not m["ok"]]
    assert not bad, "; ".join(f"{m['name']}: rel_l2={m.get('rel_l2')} tol={m.get('tol')} max_abs={m.get('max_abs')} "
                              f"max_abs_tol={m.get('max_abs_tol')} worst_index={m.get('worst_index')}" for m in bad)


@pytest.mark.parametrize("cid", [c["id"] for c in V.CASES])
def test_attention_on_value_regimes(cid):
    case = V.BY_ID[cid]
    results, yard = G.check_attention_values(case)
    _finish(case, results, yard)


@pytest.mark.parametrize("regime,mask,compact", V.PROBE_CASES, ids=[f"{r.replace(':', '=')}-{m}-{'compact' if c else 'uncompacted'}"
                                                                    for r, m, c in V.PROBE_CASES])
def test_probe_on_value_regimes(regime, mask, compact):
    from tests.model_checks import report
    results = G.check_attention_probe_values(regime, mask, compact)
    report(results)
    for m in results:
        print(m)
    assert all(m["ok"] for m in results), [m for m in results if not m["ok"]]
