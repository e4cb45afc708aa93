"""Which legs bench.py runs after its timed region (CPU): none in a plain run; with --full every leg it applies to, each of which
its --no-* option leaves out.  The GPU case runs a plain bench.py end to end and checks that it printed the headline alone."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ALL_AT_ONE_GPU = {"fwd", "roofline", "loss_parity", "cpu_baseline", "eager_baseline", "integration_levels", "rollout", "other_configs"}


def legs(argv, rank=0, world=1):
    return bench.extra_legs(bench.make_parser().parse_args(argv), rank, world)


def test_a_plain_run_has_no_extra_legs():
    assert legs(["--gpus", "1", "--steps", "8", "--warmup", "2"]) == frozenset()
    assert legs(["--gpus", "1", "--dump-outputs", "out"]) == frozenset()
    assert legs(["--torch-ddp", "--torch-adamw"]) == frozenset()
    for rank in (0, 1):
        assert legs(["--gpus", "2"], rank=rank, world=2) == frozenset()


def test_full_runs_every_leg_at_one_gpu():
    assert legs(["--gpus", "1", "--steps", "8", "--warmup", "2", "--full"]) == ALL_AT_ONE_GPU


def test_each_no_option_leaves_out_its_leg():
    for leg, opt in (("fwd", "--no-fwd"), ("roofline", "--no-roofline"), ("loss_parity", "--no-loss-parity"),
                     ("cpu_baseline", "--no-cpu-baseline"), ("eager_baseline", "--no-eager-baseline"),
                     ("integration_levels", "--no-integration-levels"), ("rollout", "--no-rollout"),
                     ("other_configs", "--no-other-configs")):
        assert legs(["--full", opt]) == ALL_AT_ONE_GPU - {leg}, opt
        assert legs([opt]) == frozenset()


def test_full_legs_by_rank_path_and_head_set():
    for rank in (0, 1):                                   # N > 1: every rank runs the legs that step the model together
        assert legs(["--gpus", "2", "--full"], rank=rank, world=2) == {"fwd", "roofline", "rccl"}
    assert legs(["--full", "--torch-ddp"]) == ALL_AT_ONE_GPU - {"integration_levels", "other_configs"} | {"rccl"}
    assert legs(["--full", "--heads", "E"]) == ALL_AT_ONE_GPU - {"rollout", "other_configs"}


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone(tmp_path):
    """a short plain run (2 layers, no tuner steps): one JSON line whose extra objects are null, and the dump it was asked for"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--layers",
                        "2", "--tune-steps", "0", "--dump-outputs", str(tmp_path / "dump")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "samples/s" and d["dtype"] == "bf16"
    for k in ("fwd_ms_per_step", "roofline", "loss_parity", "cpu_baseline", "eager_rocm_baseline", "rollout", "other_configs", "rccl",
              "integration_levels"):
        assert d[k] is None, k
    assert os.path.exists(tmp_path / "dump" / "loss.npy") and os.path.exists(tmp_path / "dump" / "params.npy")
