"""What the attention probe costs (a measurement script, not a test).  One JSON line per arm on stdout and, appended, in the file
named by --out=PATH (the recorded run is kept as profiles/r22_attention_probe_perf.jsonl).

    python tests/gpu_attention_probe_perf.py [--out=PATH] [--rounds=N] [--episodes=1,64] [--skip-step]

1. The kernel alone at the trunk's evaluation shape: 64 episodes, L = 651 (7 window steps of 36 + 54 + 3 tokens), 16 heads of 64,
   the 3 action rows of the newest window step, under the rule mask built on the device (csrc/masks.hip) -- once with
   atten_only_obs (an action row sees its own step: the tiles of the other six are skipped), once without (it sees the
   conditioning tokens of every step so far).  `k_bytes` is what the kernel loads of K: head_dim * 2 bytes for every key visible to
   a selected row, per row, head and episode (keys of a loaded tile that the row cannot see are not loaded); `k_gb_per_s` is that
   over the median time.  `hip_mean`: the head-mean output (two launches), `hip_per_head`: the per-head output (one launch).
2. The same maps in eager PyTorch, the comparator: the selected q rows gathered, q k^T for them in bf16, a dense mask, float
   softmax, the mean over heads.
3. The control step of RolloutEngine on the full-size evaluation model (tests/gpu_rollout_bench.py::build_model, captured graphs)
   with attention=dict(rows="action", layers="all") against attention=None, in the same process, at each episode count.
Every arm is measured twice per round (x and x_again: what two runs of the same code differ by), the arms interleaved; device events
around blocks of back-to-back calls sized to a quarter of a second (kernel arms), a host clock around 20 synchronised steps (step
arms); medians over the rounds."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARGS = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
OUT = ARGS.get("out")
ROUNDS = int(ARGS.get("rounds", 3))
BLOCK_MS = 250.0
DEV, BF = "cuda", torch.bfloat16


def emit(row):
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def time_block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(arms):
    """arms: name -> callable; -> name (and name_again) -> list of ms per call, one per round"""
    iters, ms = {}, {}
    for n, fn in arms.items():
        time_block(fn, 3)
        iters[n] = max(5, int(BLOCK_MS / max(time_block(fn, 5), 1e-4)) + 1)
    for _ in range(ROUNDS):
        for suffix in ("", "_again"):
            for n, fn in arms.items():
                ms.setdefault(n + suffix, []).append(time_block(fn, iters[n]))
    return ms, iters


def kernel_arms():
    from dreamvla_amd import ops
    B, K, H, D, blk, R = 64, 7, 16, 64, 93, 3
    L = K * blk
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, L, 3, H, D, generator=g).to(BF).to(DEV)
    q, k = qkv[:, :, 0], qkv[:, :, 1]
    rows = torch.tensor([[(K - 1) * blk + 90 + i for i in range(R)]] * B, dtype=torch.int32, device=DEV)
    scale = D ** -0.5
    for only_obs in (True, False):
        rule = dict(K=K, num_A=36, num_B=57, atten_goal=0, atten_goal_state=False, atten_only_obs=only_obs,
                    attn_robot_proprio_state=True, num_obs_token=54, action_pred_steps=3)
        mt = ops.build_mask_tables_device(DEV, drop=None, **rule)
        vis = ops.mask_rule_visible(drop=np.zeros((K, 0), dtype=np.int32), **rule)
        sel = rows[0].cpu().numpy()
        k_bytes = int(B * H * vis[sel].sum() * D * 2)
        dense = torch.from_numpy(vis[sel]).to(DEV)                          # (R, L) visibility of the selected rows

        def eager():
            qs = q[:, rows[0].long()]                                       # (B, R, H, D)
            s = torch.einsum("brhd,blhd->bhrl", qs, k).float() * scale
            s = s.masked_fill(~dense, float("-inf"))
            return torch.softmax(s, dim=-1).mean(dim=1)

        a = ops.attention_probe(q, k, rows, scale=scale, mask_tables=mt)
        err = float((a - eager()).abs().max())                              # the comparator computes the same maps (bf16 scores)
        arms = {"hip_mean": lambda: ops.attention_probe(q, k, rows, scale=scale, mask_tables=mt),
                "hip_per_head": lambda: ops.attention_probe(q, k, rows, scale=scale, mask_tables=mt, per_head=True),
                "eager": eager}
        ms, iters = measure(arms)
        for n, x in ms.items():
            med = statistics.median(x)
            row = {"what": "kernel", "atten_only_obs": only_obs, "arm": n, "B": B, "L": L, "H": H, "D": D, "R": R,
                   "visible_keys_per_row": [int(v) for v in vis[sel].sum(axis=1)], "calls_per_block": iters[n.replace("_again", "")],
                   "us_per_call": [round(t * 1e3, 2) for t in x], "median_us": round(med * 1e3, 2),
                   "max_abs_difference_hip_vs_eager": err}
            if n.startswith("hip"):
                row["k_bytes"] = k_bytes
                row["k_gb_per_s"] = round(k_bytes / (med * 1e-3) / 1e9, 1)
            emit(row)


def step_arms(episodes):
    from dreamvla_amd.rollout import RolloutEngine
    from gpu_rollout_bench import build_model
    m, S = build_model()
    spec = dict(rows="action", layers="all")
    for B in episodes:
        g = torch.Generator().manual_seed(B)
        frames = [(torch.randn(B, 3, 224, 224, generator=g).to(DEV, BF), torch.randn(B, 3, 224, 224, generator=g).to(DEV, BF),
                   torch.cat([torch.rand(B, 6, generator=g), torch.ones(B, 1)], -1).to(DEV, BF)) for _ in range(4)]
        text = torch.randint(1, 49000, (B, 77), generator=g).to(DEV)
        engines = {"attention_none": RolloutEngine(m, B, use_graph=True, warmup_decodes=6),
                   "attention_action_all": RolloutEngine(m, B, use_graph=True, warmup_decodes=6, attention=spec)}
        for eng in engines.values():                                        # fill the window, settle the tuner, capture
            for i in range(S + 8):
                eng.step(*frames[i % 4], text)
            assert eng.graphs_captured

        def steps(eng, n=20):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                eng.step(*frames[i % 4], text)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        ms = {}
        for _ in range(ROUNDS):
            for suffix in ("", "_again"):
                for n, eng in engines.items():
                    ms.setdefault(n + suffix, []).append(steps(eng))
        med = {n: statistics.median(x) for n, x in ms.items()}
        for n, x in ms.items():
            emit({"what": "control_step", "B": B, "S": S, "arm": n, "ms_per_step": [round(t, 3) for t in x],
                  "median_ms": round(med[n], 3)})
        att = engines["attention_action_all"].last_attention
        emit({"what": "control_step_summary", "B": B, "trunk_maps": list(att["trunk"].shape),
              "overhead_ms": round(med["attention_action_all"] - med["attention_none"], 3),
              "attention_over_none": round(med["attention_action_all"] / med["attention_none"], 4),
              "none_again_over_none": round(med["attention_none_again"] / med["attention_none"], 4),
              "attention_again_over_attention": round(med["attention_action_all_again"] / med["attention_action_all"], 4)})
        del engines
        torch.cuda.empty_cache()


def main():
    assert torch.cuda.is_available(), "a measurement on the GPU: no fallback"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "block_ms": BLOCK_MS})
    kernel_arms()
    if "skip-step" not in ARGS:
        step_arms([int(x) for x in ARGS.get("episodes", "1,64").split(",")])


if __name__ == "__main__":
    main()
