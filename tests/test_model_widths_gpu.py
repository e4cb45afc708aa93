"""GPU: whole models of width other than 1024 against the REAL reference's fixtures (tests/make_golden_widths.py).
W = the reference's CLI defaults (384 / 12 heads / 12 layers: trunk head_dim 32 under the real mask, decoders at 24);
V = 768 / 12 heads, LIBERO flags with dino / sam / trajectory heads (trunk head_dim 64, decoders at 48).
Same checks and tolerances as tests/test_model_gpu.py applies to the 1024-wide fixtures."""
import pytest

from tests import model_checks, rollout_checks


def _assert_all(results):
    model_checks.report(results)
    assert results
    bad = [r for r in results if not r["ok"]]
    assert not bad, bad[:3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["W", "V"])
def test_full_model_vs_reference(name):
    _assert_all(model_checks.hip_full_model_checks(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["W", "V"])
def test_gradients_vs_reference(name):
    _assert_all(model_checks.hip_grad_checks(name))


@pytest.mark.gpu
def test_rollout_graph_captured_decode_vs_reference_W():
    _assert_all(rollout_checks.gpu_rollout_vs_reference("W", use_graph=True))
