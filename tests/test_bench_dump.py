"""bench.py --dump-outputs (CPU): the files dump_outputs writes -- names, dtypes, the fixed parameter / gradient sample and its
size bound -- on a small stand-in for the trainable parameter list; and --steps below 1 is refused before any GPU work."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _params():
    g = torch.Generator().manual_seed(0)
    shapes = [(3,), (64, 100), (bench.DUMP_PER_TENSOR + 7,), (4, 3)]
    return [(f"p{i}", torch.randn(s, generator=g)) for i, s in enumerate(shapes)]


def _dump(d, named, grad_of):
    parts = {"arm_action": torch.tensor(0.25), "gripper_action": torch.tensor(0.5), "depth": None}
    bench.dump_outputs(str(d), torch.tensor(0.75), parts, named, grad_of)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_files_and_sample(tmp_path):
    named = _params()
    grads = {id(p): 2 * p for _, p in named[:-1]}                  # the last parameter has no gradient
    out = _dump(tmp_path / "a", named, lambda p: grads.get(id(p)))
    assert set(out) == {"loss", "loss_arm_action", "loss_gripper_action", "params", "grads", "param_sizes"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["loss"].tolist() == [0.75] and out["loss_arm_action"].tolist() == [0.25]
    sizes = [min(p.numel(), bench.DUMP_PER_TENSOR) for _, p in named]
    assert out["param_sizes"].tolist() == sizes and out["params"].shape == out["grads"].shape == (sum(sizes),)
    lo = 0
    for (_, p), n in zip(named, sizes):
        ps, gs = out["params"][lo:lo + n], out["grads"][lo:lo + n]
        flat = p.reshape(-1).numpy()
        assert np.isin(ps, flat).all()                                 # a sample of this parameter's own elements ...
        assert np.array_equal(gs, 2 * ps) if id(p) in grads else not gs.any()     # ... and its gradient at the same indices
        if n == p.numel():
            assert np.array_equal(ps, flat)
        lo += n
    again = _dump(tmp_path / "b", named, lambda p: grads.get(id(p)))   # fixed sample: identical from run to run
    assert all(np.array_equal(out[k], again[k]) for k in out)


def test_dump_of_the_default_workload_stays_under_64_mb():
    from dreamvla_amd.dreamvla_model import DreamVLA
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **bench.model_cfg("C", 7))
    m.clip_model.requires_grad_(False)
    m.vision_encoder.requires_grad_(False)
    n = sum(min(p.numel(), bench.DUMP_PER_TENSOR) for p in m.parameters() if p.requires_grad)
    assert 2 * 4 * n < 64 << 20, n


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_dump_replays_the_newest_committed_gemm_plan():
    """--dump-outputs without --plan fixes the GEMM configurations: the newest committed plan exists and names the step's problems"""
    import json
    plan = bench.committed_gemm_plan()
    assert plan is not None and os.path.basename(plan) == sorted(
        f for f in os.listdir(os.path.join(ROOT, "profiles")) if f[0] == "r" and f[3:] == "_gemm_plan.json")[-1]
    assert len(json.load(open(plan))) >= 100
