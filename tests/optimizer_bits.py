"""The bits of every fused optimizer step entry point (include/dvla.h: the fourteen dvla_adamw_* symbols) on fixed inputs.

A helper, not a test: CASES is a fixed list, digest(case) runs one entry point once and returns the SHA-256 of the bytes of
param, exp_avg, exp_avg_sq and, where the entry point has them, the bf16 shadow and the EMA.  `python -m tests.optimizer_bits
[out.json]` records {case name: digest} (tests/golden/optimizer_bits.json by default); tests/test_optimizer_bits_gpu.py holds a
build against that record, so a change to the step kernels that moves one bit of one element anywhere shows.

Inputs come from hash32 (csrc/common.h, as tests/sr_ref.py restates it) of the element index: integers, scaled by powers of two,
so they do not depend on the torch version.  The gradient has exact zeros, exp_avg_sq has exact zeros and values next to zero.
Sizes: 5 (ragged tail only), 8*256 + 3 (one partial round and the tail) and 8*256*4096 + 8*300 + 5 (the grid is capped at 4096
blocks: the second grid-stride round, and the tail).  Every entry point runs in every combination of guard / EMA / clip / map /
stochastic rounding it can reach; a clip that is on engages (coefficient 0.05), per-group clips hold one engaged, one idle and one
unclipped group; grouped cases have 3 groups with distinct lr / weight decay and a run of unstepped vectors (map byte 255) -- at
the middle size the tail's byte is unstepped too; guarded cases pick candidate row 1 of 3 on an applied step, and on a skipped
step digest() also asserts that no output byte moved."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

from .sr_ref import hash32

SIZES = (5, 8 * 256 + 3, 8 * 256 * 4096 + 8 * 300 + 5)
LR, WD = (1e-3, 3e-4, 2e-3), (0.01, 0.0, 0.1)
B1, B2, EPS = 0.9, 0.999, 1e-8
STEP = 3                              # unguarded: the 1-based step count
MAX_NORM = 0.1
SUMSQ = 4.0                           # the global sum of squares handed over: coefficient 0.1 / (2 + 1e-6)
GROUP_SUMSQ = (4.0, 1e-4, 9.0)        # per group: engaged, idle (coefficient 1), and
GROUP_MAX_NORM = (0.1, 0.1, 0.0)      # ... not clipped (its sum is not read)
EMA_DECAY = 0.999
N_CAND, APPLIED_BEFORE = 3, 1         # guarded: the device has applied one step the host has not confirmed -> candidate row 1
SR_SEED, SR_BUCKET = 0x1234567890ABCDEF, 3
SR_BASE = 2 ** 32 - 8 * 1000          # the large size carries the element index past 32 bits


def _cases():
    out = []

    def add(entry, n, **flags):
        on = [k for k in ("guard", "ema", "map", "clip", "noshadow", "skip") if flags.get(k)]
        out.append(dict(flags, entry=entry, n=n, name="-".join([entry] + on + [f"n{n}"])))

    for n in SIZES:
        for prec in ("bf16", "f32_master"):
            for guard in (False, True):
                for ema in (False, True):
                    entry = "dvla_adamw_" + prec + ("_ema" if ema else "") + ("_guarded" if guard else "")
                    for clip in (False, True):
                        add(entry, n, guard=guard, ema=ema, clip=clip)
                    if guard:
                        add(entry, n, guard=True, ema=ema, clip=True, skip=True)
            if prec == "f32_master":
                add("dvla_adamw_f32_master", n, clip=True, noshadow=True)
            for guard in (False, True):
                for ema in (False, True):
                    for clip in (False, True):
                        add(f"dvla_adamw_{prec}_grouped", n, guard=guard, ema=ema, map=True, clip=clip)
                    add(f"dvla_adamw_{prec}_grouped_clip", n, guard=guard, ema=ema, map=True, clip=True)
                    if guard:
                        add(f"dvla_adamw_{prec}_grouped", n, guard=True, ema=ema, map=True, clip=True, skip=True)
                        add(f"dvla_adamw_{prec}_grouped_clip", n, guard=True, ema=ema, map=True, clip=True, skip=True)
        for guard in (False, True):
            for ema in (False, True):
                for gmap in (False, True):
                    for clip in (False, True):
                        add("dvla_adamw_bf16_sr", n, guard=guard, ema=ema, map=gmap, clip=clip)
                    if guard:
                        add("dvla_adamw_bf16_sr", n, guard=True, ema=ema, map=gmap, clip=True, skip=True)
                add("dvla_adamw_bf16_sr_clip", n, guard=guard, ema=ema, map=True, clip=True)
                if guard:
                    add("dvla_adamw_bf16_sr_clip", n, guard=True, ema=ema, map=True, clip=True, skip=True)
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_bits.json")


def _unit(n, salt):
    """hash32 of (index, salt) -> fp32 in [-1, 1), a multiple of 2^-23 (exact), and the hash itself"""
    h = hash32(np.arange(n, dtype=np.uint32) * np.uint32(0x9E3779B9) + np.uint32(salt))
    return ((h >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23), h


def _to_bf16_bits(x):
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)      # truncation: integer arithmetic only


def host_inputs(n):
    """fp32 numpy arrays p, g, m, v, ema and the group map (one byte per 8 elements) of size n"""
    p, _ = _unit(n, 0x1001)
    g, hg = _unit(n, 0x2002)
    g = g * np.float32(4.0)
    g[hg % np.uint32(7) == 0] = 0.0
    m, _ = _unit(n, 0x3003)
    m = m * np.float32(2.0 ** -4)
    v, hv = _unit(n, 0x4004)
    v = np.abs(v) * np.float32(2.0 ** -10)
    sel = hv % np.uint32(5)
    v[sel == 0] = 0.0
    v[sel == 1] *= np.float32(2.0 ** -100)                              # next to zero: far below eps^2
    ema, _ = _unit(n, 0x5005)
    n_map = (n + 7) // 8
    vec = np.arange(n_map, dtype=np.uint32)
    # runs of 5 vectors, shuffled every 37: every group turns up within 15 vectors, at every size above the smallest
    gmap = ((vec // np.uint32(5) + hash32(vec // np.uint32(37) + np.uint32(0x6006))) % np.uint32(3)).astype(np.uint8)
    lo = n_map // 3
    gmap[lo:lo + 50] = 255                                              # a run the step leaves alone
    if n == SIZES[0]:
        gmap[-1] = 0                                                    # the tail is all there is: stepped, its clip engaged
    elif n == SIZES[1]:
        gmap[-1] = 255                                                  # the tail's byte: left alone
    else:
        gmap[-1] = 2
    return {"p": p, "g": g, "m": m, "v": v, "ema": ema, "map": gmap}


_device_inputs = {}


def _inputs(n, bf16):
    """the inputs on the device, built once per (size, precision); callers clone what the step writes"""
    import torch
    key = (n, bf16)
    if key not in _device_inputs:
        h = host_inputs(n)
        d = {}
        for k in ("p", "g", "m", "v"):
            if bf16:
                d[k] = torch.from_numpy(_to_bf16_bits(h[k]).view(np.int16)).cuda().view(torch.bfloat16)
            else:
                d[k] = torch.from_numpy(h[k]).cuda()
        d["ema"] = torch.from_numpy(h["ema"]).cuda()
        d["map"] = torch.from_numpy(h["map"]).cuda()
        _device_inputs[key] = d
    return _device_inputs[key]


def _bytes(t):
    import torch
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy().tobytes()


def digest(case):
    """run the case's entry point once on the current device -> hex SHA-256 of its output buffers"""
    import torch
    from dreamvla_amd import _lib
    from dreamvla_amd._lib import check
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    entry, n = case["entry"], case["n"]
    guard, ema, gmap, clip, skip = (bool(case.get(k)) for k in ("guard", "ema", "map", "clip", "skip"))
    bf16 = "_bf16" in entry
    sr, per_group = "_sr" in entry, entry.endswith("_clip")
    table = gmap or sr                                   # the entry points that take lr / weight_decay as arrays
    src = _inputs(n, bf16)
    bufs = {k: src[k].clone() for k in ("p", "m", "v")}
    if not bf16 and not case.get("noshadow"):
        bufs["sh"] = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    if ema:
        bufs["ema"] = src["ema"].clone()
    before = {k: t.clone() for k, t in bufs.items()} if skip else None
    ptr = {k: t.data_ptr() for k, t in bufs.items()}
    n_groups = 3 if gmap else 1
    lrs, wds = (ctypes.c_double * n_groups)(*LR[:n_groups]), (ctypes.c_double * n_groups)(*WD[:n_groups])
    ema_w = (ctypes.c_float * _lib.STEP_MAX_CANDIDATES)()
    keep = []                                            # device scalars the launch reads

    def dev(values):
        keep.append(torch.tensor(values, dtype=torch.float32, device="cuda"))
        return keep[-1].data_ptr()

    state, n_cand, step = None, 1, STEP
    group_sumsq = dev(list(GROUP_SUMSQ))
    if guard:
        n_cand, step = N_CAND, 1                         # base: the first count still possible
        head = torch.zeros(ctypes.sizeof(_lib.StepState), dtype=torch.uint8)
        head[:8].view(torch.int64)[0] = APPLIED_BEFORE
        st = head.cuda()
        keep.append(st)
        cand = (_lib.StepScalars * _lib.STEP_MAX_CANDIDATES)()
        check(lib.dvla_step_candidates(LR[0], B1, B2, step, n_cand, cand), "dvla_step_candidates")
        sums = list(GROUP_SUMSQ) if per_group else [SUMSQ]
        if skip:
            sums[-1] = float("inf")
        group_sumsq = dev(sums)                          # the verdict's slots are the groups' sums under a per-group clip
        check(lib.dvla_step_verdict(group_sumsq, len(sums), dev([0.0]), st.data_ptr(), 0, n_cand, cand, stream), "dvla_step_verdict")
        state = st.data_ptr()
    if ema:
        check(lib.dvla_ema_weights(EMA_DECAY, 1, step, n_cand, ema_w), "dvla_ema_weights")
    if per_group:
        sumsq, max_norm = group_sumsq, (ctypes.c_float * n_groups)(*GROUP_MAX_NORM)
    elif guard:
        sumsq, max_norm = None, (MAX_NORM if clip else 0.0)      # guarded: the verdict's total, used when max_norm > 0
    else:
        sumsq, max_norm = (dev([SUMSQ]) if clip else None), (MAX_NORM if clip else 0.0)

    streams = [ptr["p"], src["g"].data_ptr(), ptr["m"], ptr["v"]] + ([] if bf16 else [ptr.get("sh")])
    if table:
        args = streams + [ptr.get("ema"), n, src["map"].data_ptr() if gmap else None, n_groups, lrs, wds, B1, B2, EPS, step, sumsq,
                          max_norm, state, ema_w if ema else None, n_cand]
        if sr:
            args += [SR_SEED, SR_BUCKET, SR_BASE]
    else:
        args = streams + ([ptr["ema"]] if ema else []) + [n, LR[0], B1, B2, EPS, WD[0]]
        args += [max_norm, state] if guard else [step, sumsq, max_norm]
        if ema:
            args += [ema_w, n_cand] if guard else [ema_w[0]]
    check(getattr(lib, entry)(*args, stream), entry)
    torch.cuda.synchronize()
    sha = hashlib.sha256()
    for k in ("p", "m", "v", "sh", "ema"):
        if k in bufs:
            if skip:
                assert torch.equal(bufs[k].view(torch.uint8), before[k].view(torch.uint8)), f"{case['name']}: a skipped step moved {k}"
            sha.update(_bytes(bufs[k]))
    return sha.hexdigest()


def main(argv):
    out = argv[1] if len(argv) > 1 else GOLDEN
    record = {}
    for case in CASES:
        record[case["name"]] = digest(case)
        print(case["name"], record[case["name"]], flush=True)
    with open(out, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(record)} digests -> {out}")


if __name__ == "__main__":
    main(sys.argv)
