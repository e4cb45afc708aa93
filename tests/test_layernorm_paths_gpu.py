"""GPU: the LayerNorm kernels on the paths no other kernel-parity case runs (tests/rowwise_cases.py lists them and
tests/test_rowwise_cases.py proves that each case reaches its path): the grid-stride loops with their two-rows-in-flight
prefetch (forward past 8192 rows, backward past 3072 -- the fork's residual gradient, the row groups' zero-fill and the
map_output variants included), every template instance with a full, a ragged and a single-lane last vector slot, the
statistics outputs, and rows of mixed scale and conditioning.

y and dx are held ROW BY ROW to the unrounded float64 oracle (tests.gpu_checks.rowwise): half a bf16 ulp of the reference plus
(1 + kappa_row) * 2^-20 * max_row |ref|, kappa_row = |mean| * rstd -- a wrong low-rstd row cannot hide behind the global maximum.
Composite paths keep their bit-for-bit twins at the new shapes.  One row per case goes to $DVLA_PARITY_REPORT
(profiles/r16_parity_rowwise.jsonl).

Measured on an MI355X: 64 cases, all ok; at the model widths no data class uses more than 3 % of the allowance.  Three cases use
more than a quarter, all of them dx at 8 columns (last-3100x10keep10x8 0.67, plain-16389x8 0.48, last-3100x10keep1x8 0.28): an
outlier row there is one 500 among seven O(1) values, x-hat saturates at sqrt 7 and dx of that channel cancels -- the fp32
formulation evaluated on the CPU gives the same 0.48, exact statistics rounded to fp32 alone 0.17.  The file runs in
about 3 s."""
import pytest
import torch

from tests import gpu_checks as G
from tests import rowwise_cases as RC
from tests.gpu_checks import BF, DEV

pytestmark = pytest.mark.gpu


def test_the_library_reports_the_partial_row_counts_the_geometry_assumes():
    from dreamvla_amd import _lib
    lib = _lib.load()
    assert lib.dvla_layernorm_bwd_partial_rows() == RC.LN_BWD_MAX_BLOCKS == 768
    assert lib.dvla_colsum_partial_rows() == RC.CS_MAX_SLABS == 512


@pytest.mark.parametrize("case", RC.LN_CASES, ids=[c["id"] for c in RC.LN_CASES])
def test_layer_norm_and_fork(case):
    G.finish_case(case["id"], G.ln_case_path(case), G.check_layernorm_paths(case))


@pytest.mark.parametrize("case", RC.LAST_TOKENS_CASES, ids=[c["id"] for c in RC.LAST_TOKENS_CASES])
def test_last_tokens_with_iterating_row_groups(case):
    g = RC.ln_geometry(case["n"] * case["keep"], case["cols"], backward=True)
    G.finish_case(case["id"], f"bwd {g['blocks']} blocks x {g['trips']} trips, {case['L'] - case['keep']} rows zero-filled per group",
                  G.check_layernorm_last_tokens_paths(case))


@pytest.mark.parametrize("case", RC.CONCAT_CASES, ids=[c["id"] for c in RC.CONCAT_CASES])
def test_concat_with_map_output(case):
    g = RC.ln_geometry(case["n"] * case["La"], case["cols"], backward=True)
    G.finish_case(case["id"], f"a: bwd {g['blocks']} blocks x {g['trips']} trips (last {g['last_trip_rows']} rows)", G.check_layernorm_concat_paths(case))


class _Recorder:
    """every call of the two LayerNorm launch entry points with its return code (as in tests/test_ops_families_gpu.py)"""

    def __init__(self, monkeypatch):
        from dreamvla_amd import _lib
        self.calls = []
        lib = _lib.load()
        for name in ("dvla_layernorm_fwd_rows", "dvla_layernorm_bwd_rows", "dvla_layernorm_bwd_add"):
            real = getattr(lib, name)
            monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: self.calls.append((_n, _r(*a))) or self.calls[-1][1])


@pytest.mark.parametrize("cols", RC.LN_REFUSED_COLS)
def test_unsupported_widths_are_refused_before_any_launch(cols, monkeypatch):
    from dreamvla_amd import ops
    from dreamvla_amd._lib import DvlaError
    rec = _Recorder(monkeypatch)
    x = RC.grad_like((9, cols), 5).to(DEV, BF)
    w = torch.ones(cols, device=DEV, dtype=BF)
    with pytest.raises(DvlaError, match=r"unsupported.*\(code -3\)"):
        ops.layer_norm(x, w, w, 1e-5)
    # the entry point was asked once and answered UNSUPPORTED -- which it does in front of its launch; an output buffer handed to it
    # stays as it was
    assert rec.calls == [("dvla_layernorm_fwd_rows", G.ERR_UNSUPPORTED)]
    out = torch.full((9, cols), G.VIEW_SENTINEL, device=DEV, dtype=BF)
    with pytest.raises(DvlaError, match=r"\(code -3\)"):
        ops.layernorm_fwd(x, w, w, 1e-5, True, out=out)
    torch.cuda.synchronize()
    assert G.outside_window_intact(out.view(-1), None)["ok"]
    rec.calls.clear()
    x3 = x.view(3, 3, cols)
    with pytest.raises(ValueError, match="layer_norm_last_tokens"):
        ops.layer_norm_last_tokens(x3, w, w, 1e-5, 2)
    with pytest.raises(ValueError, match="layer_norm_concat"):
        ops.layer_norm_concat(x3, w, w, 1e-5, x3, w, w, 1e-5)
    assert rec.calls == []
    ops.layer_norm(RC.grad_like((9, 16), 5).to(DEV, BF), None, None, 1e-5)          # (the recorder does see a launch)
    assert rec.calls == [("dvla_layernorm_fwd_rows", 0)]
