"""float64 restatement of FlatAdamW.parameter_stats() on CPU tensors, per parameter (tests/test_param_stats_gpu.py, shared by
tests/gpu_param_stats_perf.py).  Nothing here is the code under test: plain torch in double."""
import math

import torch


def segment_stats(x):
    """x: one parameter's elements (any dtype, any shape) -> (sum of squares: float, largest |x| over the elements that are not NaN:
    float -- 0.0 for none --, number of NaN / inf elements: int)"""
    x = x.detach().reshape(-1).double().cpu()
    sumsq = float((x * x).sum()) if x.numel() else 0.0
    kept = x[~torch.isnan(x)].abs()
    absmax = float(kept.max()) if kept.numel() else 0.0
    return sumsq, absmax, int((~torch.isfinite(x)).sum())


def adam_term_sumsq(exp_avg, exp_avg_sq, beta2, eps, step, master):
    """sum of r^2 over one parameter, r = exp_avg / denom(exp_avg_sq) from the moments exactly as stored (fp32 or bf16, widened to
    double), the denominator evaluated in float64:
        master (fp32):  sqrt(v) / sqrt(1 - beta2^step) + eps
        bf16:           sqrt(v) * (1 / sqrt(1 - beta2^step)) + eps"""
    m, v = exp_avg.detach().reshape(-1).double().cpu(), exp_avg_sq.detach().reshape(-1).double().cpu()
    if m.numel() == 0:
        return 0.0
    bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
    denom = v.sqrt() / bc2_sqrt + eps if master else v.sqrt() * (1.0 / bc2_sqrt) + eps
    r = m / denom
    return float((r * r).sum())


def update_norm(exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, master):
    """lr |1 / (1 - beta1^step)| sqrt(sum r^2); 0.0 before the first step"""
    if step < 1:
        return 0.0
    return lr * abs(1.0 / (1.0 - beta1 ** step)) * math.sqrt(adam_term_sumsq(exp_avg, exp_avg_sq, beta2, eps, step, master))
