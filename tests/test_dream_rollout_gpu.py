"""GPU: dreams at evaluation (tests/dream_checks.py) -- the dream heads in mode="test" against the real reference's train-mode
outputs (fixtures C, D, E, R: every head), the selection of the executed position, the render kernel against its float64
restatement, and RolloutEngine(dreams=...) eager and under hipGraph replay.  Reads tests/golden/ and the package only."""
import pytest

from tests import dream_checks as D
from tests import model_checks as C


def _assert_all(results):
    C.report(results)
    bad = [r for r in results if not r["ok"]]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C", "D", "E", "R"])
def test_dream_heads_in_test_mode_vs_real_reference(name):
    """C, R: image + depth + sam; D: image + sam; E: image + trajectory + dino + sam.  Bounds: the train-mode checks' own
    (max(1e-3, 1.25 x the reference's recorded bf16 deviation), element-wise 1.5 x its worst element)."""
    _assert_all(D.gpu_dream_head_checks(name))


@pytest.mark.gpu
def test_dream_render_vs_float64_restatement():
    _assert_all(D.gpu_dream_render_checks("C"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["R", "D"])
@pytest.mark.parametrize("sample", ["newest", "all"])
def test_engine_dreams_graph_and_eager(name, sample):
    """a short, padded history (the first S - 1 steps), a reset(mask) mid-way, then a sliding window; every step against the
    module-level call; the captured graph against the eager engine on the last step"""
    import torch
    fx = C.load(f"dreamvla_{name}.pt")
    S = fx["S"]
    eager, d_eager = D.gpu_dream_engine_checks(name, False, sample, reset_at=S // 2, extra_steps=S // 2 + 2)
    graph, d_graph = D.gpu_dream_engine_checks(name, True, sample, reset_at=S // 2, extra_steps=S // 2 + 2)
    res = eager + graph
    tols = C.output_tolerances(fx, C.TOL_MODEL)
    for k in d_graph:
        t_rel, t_abs, _ = tols[D.SLOT[k]]
        if k == "image":       # uint8: the bound of dream_checks._level_bound at the largest patch deviation CLIP-normalised frames reach
            worst = float((d_graph[k].float() - d_eager[k].float()).abs().max())
            res.append(D._row(f"dream.engine.{name}.{sample}.image graph replay vs eager engine (max level difference)", worst,
                              1.0 + 255.0 * 0.27577711 * 2.2 * D.PAIR * t_abs))
        else:
            res.append(D._pair(f"dream.engine.{name}.{sample}.{k} graph replay vs eager engine", d_graph[k], d_eager[k], t_rel, t_abs))
        assert d_graph[k].dtype == d_eager[k].dtype and torch.isfinite(d_graph[k].float()).all()
    _assert_all(res)


@pytest.mark.gpu
@pytest.mark.parametrize("sample", ["newest", "all"])
def test_engine_dreams_on_the_fixture_window_vs_real_reference(sample):
    """fixture R pushed frame by frame without a reset: after the S-th push the engine's window is the fixture's, and the depth /
    sam dreams of the executed position are the real reference's"""
    _assert_all(D.gpu_dream_engine_checks("R", True, sample)[0])


@pytest.mark.gpu
def test_engine_dreams_lockstep_64_episodes():
    """64 episodes in lock-step, fixture R in slot 17 (as gpu_rollout_lockstep_vs_reference): tiled GEMMs at 128 x 205 decoder rows"""
    res, dreams = D.gpu_dream_engine_checks("R", True, "newest", episodes=64, slot=17)
    assert tuple(dreams["image"].shape) == (64, 2, 224, 224, 3) and tuple(dreams["depth"].shape) == (64, 2, 224, 224)
    assert tuple(dreams["sam"].shape) == (64, 2, 256, 256)
    _assert_all(res)
