"""What FlatAdamW.parameter_stats() costs (a measurement script, not a test): the per-parameter reductions over the flat buffers of
the trainable parameters of head set C (24 layers, 496.6 M parameters), once as fp32 masters (the shipped precision) and once as
bf16 buckets, against the multi-tensor torch calls a user would write over the per-parameter views, in the same process.  Layout
and timing are those of tests/gpu_sr_step_perf.py.  One JSON line per arm and one summary line per dtype on stdout and, appended,
in the file named by --out=PATH (the recorded run is kept as profiles/r21_param_stats_perf.jsonl).

    python tests/gpu_param_stats_perf.py [--out=PATH] [--synthetic] [--rounds=N] [--dtypes=f32,bf16] [--tree=NAME]

Arms, per dtype, on one optimizer that has taken two steps (moments are non-zero, t = 2):
  hip_grad / hip_param / hip_update / hip_all   parameter_stats(("grad",)) ... parameter_stats(): norm, absmax and non-finite count
                                                per parameter (update: the norm alone): one launch per bucket and buffer, and
                                                one more per buffer that combines every parameter's records
  torch_grad / torch_param                      torch._foreach_norm over the per-parameter gradient / parameter views: the norms
                                                alone -- no absmax, no count
  torch_update                                  _foreach_sqrt, _foreach_div_, _foreach_add_, _foreach_div, _foreach_norm over the moment
                                                views: the same r = m / (sqrt(v) / bc2_sqrt + eps), materialised
  torch_all                                     the three torch arms back to back
  step / stats_then_step                        step() alone, and step() timed alone right behind an untimed parameter_stats()
Every arm is measured twice per round (x and x_again: what two runs of the same code differ by), the arms interleaved, ROUNDS
rounds, device events around a block of back-to-back calls sized to at least half a second; medians.  GB/s is the bytes of the
buffers an arm has to read once (gaps excluded) over the median time."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARGS = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
OUT = ARGS.get("out")
TREE = ARGS.get("tree", "this")
ROUNDS = int(ARGS.get("rounds", 3))
LR, WD, BETAS, EPS, MAX_NORM = 1e-4, 1e-4, (0.9, 0.999), 1e-8, 0.1
BLOCK_MS = 500.0
BUFFERS = {"grad": 1, "param": 1, "update": 2, "all": 4}          # flat buffers an arm reads


def emit(row):
    row = {"tree": TREE, **row}
    print(json.dumps(row), flush=True)
    if OUT is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def build(shapes, dtype):
    from dreamvla_amd.ddp import GradBucketReducer
    from dreamvla_amd.optim import FlatAdamW
    gen = torch.Generator(device="cuda").manual_seed(17)
    params = [torch.nn.Parameter((torch.randn(s, generator=gen, device="cuda") * 0.02).to(dtype)) for s in shapes]
    red = GradBucketReducer(params, direct_grads=True)
    opt = FlatAdamW(red, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM)
    assert opt.master_mode == (dtype == torch.float32)
    for b in red.buckets:
        b["flat"].copy_(torch.randn(b["flat"].numel(), generator=gen, device="cuda") * 1e-3)
    for _ in range(2):
        opt.step()
    return red, opt


def views(red, opt, key):
    return [s[key][off:off + p.numel()] for b, s in zip(red.buckets, opt.flat) for p, off in zip(b["params"], b["offsets"]) if p.numel()]


def time_block(fn, iters):
    """device ms per call of a block of back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def time_step(opt, iters, stats_first):
    """device ms per step(), each step between its own pair of events (an untimed parameter_stats() in front of it or not)"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for e0, e1 in pairs:
        if stats_first:
            opt.parameter_stats()
        e0.record()
        opt.step()
        e1.record()
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in pairs) / iters


def main():
    assert torch.cuda.is_available(), "a measurement on the GPU: no fallback"
    from gpu_guarded_step_perf import SYNTHETIC_BUCKETS, model_shapes
    import param_stats_ref as ref
    layout = "synthetic"
    shapes = [(n,) for n in SYNTHETIC_BUCKETS]
    if "synthetic" not in ARGS:
        try:
            shapes, layout = model_shapes(), "model"
        except Exception as e:            # the fallback the docstring names; the row says which layout was timed
            print(f"model layout unavailable ({type(e).__name__}: {e}); synthetic buckets", flush=True)
    for name in ARGS.get("dtypes", "f32,bf16").split(","):
        dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[name]
        red, opt = build(shapes, dtype)
        g, p, m, v = (views(red, opt, k) for k in ("g", "p", "m", "v"))
        elements = sum(x.numel() for x in g)
        bc2_sqrt = (1.0 - BETAS[1] ** opt.step_count) ** 0.5

        def torch_update():
            d = torch._foreach_sqrt(v)
            torch._foreach_div_(d, bc2_sqrt)
            torch._foreach_add_(d, EPS)
            return torch._foreach_norm(torch._foreach_div(m, d))

        arms = {"hip_grad": lambda: opt.parameter_stats(("grad",)), "torch_grad": lambda: torch._foreach_norm(g),
                "hip_param": lambda: opt.parameter_stats(("param",)), "torch_param": lambda: torch._foreach_norm(p),
                "hip_update": lambda: opt.parameter_stats(("update",)), "torch_update": torch_update,
                "hip_all": lambda: opt.parameter_stats(),
                "torch_all": lambda: (torch._foreach_norm(g), torch._foreach_norm(p), torch_update())}
        # the two sides compute the same thing: the largest parameter's three norms against the float64 restatement
        big = max(range(len(red.params)), key=lambda i: red.params[i].numel())
        stats = opt.parameter_stats()
        where = {id(q): (s, off) for b, s in zip(red.buckets, opt.flat) for q, off in zip(b["params"], b["offsets"])}
        s, off = where[id(red.params[big])]
        sl = slice(off, off + red.params[big].numel())
        want = {"grad_norm": ref.segment_stats(s["g"][sl])[0] ** 0.5, "param_norm": ref.segment_stats(s["p"][sl])[0] ** 0.5,
                "update_norm": ref.update_norm(s["m"][sl], s["v"][sl], LR, BETAS[0],
                                               BETAS[1] if opt.master_mode else float(torch.tensor(BETAS[1])), EPS, opt.step_count,
                                               opt.master_mode)}
        emit({"what": "setup", "dtype": name, "layout": layout, "tensors": len(g), "elements": elements,
              "buckets": [int(b["flat"].numel()) for b in red.buckets], "rounds": ROUNDS, "block_ms": BLOCK_MS,
              "largest_parameter": int(red.params[big].numel()),
              "relative_error_of_its_norms": {k: abs(float(stats[k][big]) - w) / w for k, w in want.items()},
              "device": torch.cuda.get_device_name(0)})
        ms, iters = {}, {}
        for n, fn in arms.items():                                # warm-up, and the block sized to BLOCK_MS
            time_block(fn, 3)
            iters[n] = max(5, int(BLOCK_MS / time_block(fn, 5)) + 1)
        for r in range(ROUNDS):
            for suffix in ("", "_again"):
                for n, fn in arms.items():                        # interleaved: drift of the box shows in every arm
                    ms.setdefault(n + suffix, []).append(time_block(fn, iters[n]))
        step_iters = 50
        time_step(opt, 5, False), time_step(opt, 5, True)
        for r in range(ROUNDS):
            for suffix in ("", "_again"):
                ms.setdefault("step" + suffix, []).append(time_step(opt, step_iters, False))
                ms.setdefault("stats_then_step" + suffix, []).append(time_step(opt, step_iters, True))
        med = {n: statistics.median(x) for n, x in ms.items()}
        for n, x in ms.items():
            row = {"what": "arm", "dtype": name, "arm": n, "calls_per_block": iters.get(n.replace("_again", ""), step_iters),
                   "ms_per_call": [round(t, 4) for t in x], "median_ms": round(med[n], 4), "min_ms": round(min(x), 4),
                   "max_ms": round(max(x), 4)}
            kind = n.replace("_again", "").split("_", 1)[-1]
            if kind in BUFFERS and not n.startswith(("step", "stats_then")):
                nbytes = elements * p[0].element_size() * BUFFERS[kind]
                row["buffer_bytes"] = nbytes
                row["gb_per_s"] = round(nbytes / (med[n] * 1e-3) / 1e9, 1)
            emit(row)
        summary = {"what": "summary", "dtype": name}
        for kind in BUFFERS:
            summary[f"torch_{kind}_over_hip_{kind}"] = round(med[f"torch_{kind}"] / med[f"hip_{kind}"], 3)
            summary[f"hip_{kind}_again_over_hip_{kind}"] = round(med[f"hip_{kind}_again"] / med[f"hip_{kind}"], 4)
            summary[f"torch_{kind}_again_over_torch_{kind}"] = round(med[f"torch_{kind}_again"] / med[f"torch_{kind}"], 4)
        summary["stats_then_step_over_step"] = round(med["stats_then_step"] / med["step"], 4)
        summary["step_again_over_step"] = round(med["step_again"] / med["step"], 4)
        emit(summary)
        del red, opt, g, p, m, v, arms, stats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
