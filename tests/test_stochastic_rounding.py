"""CPU: stochastic rounding of FlatAdamW's bf16 stores -- the C surface, the rounding on hand-made cases, the statistics of the
counter-based generator as tests/sr_ref.py restates it, and the trajectory bound of tests/test_stochastic_rounding_gpu.py on a
host restatement of the whole step, so that the bound is known to hold for the method before a GPU sees it.

Every statistical bound is K = 6 binomial standard deviations computed here; the seeds are fixed, so the tests are
deterministic."""
import math
import os
import re

import numpy as np
import pytest

from tests import sr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6.0
SEED = 0x9D2C5680F1A3B7E5          # a 64-bit seed with both halves in use
SEED_B = 0x0123456789ABCDEF


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_declared_and_the_abi_is_still_9():
    from dreamvla_amd import _lib
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    for name in ("dvla_sr_cast_f32_to_bf16", "dvla_adamw_bf16_sr"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert _lib.ABI_VERSION == 9 and _lib.load().dvla_abi_version() == 9
    assert re.search(r"#define\s+DVLA_ABI_VERSION\s+9\b", txt)
    # the header states the constants sr_ref restates
    for const in ("0x243F6A88", "0x85EBCA6B", "0x9E3779B9", "0x5BD1E995", "0x7feb352d", "0x846ca68b"):
        assert const in txt, const


# ---- the rounding on hand-made cases ------------------------------------------------------------------------------------------------
def _sr(u, r):
    return int(sr_ref.sr_bf16(np.array([u], dtype=np.uint32), np.array([r], dtype=np.uint32))[0])


@pytest.mark.parametrize("u", [0x3F800000, 0xBF800000, 0x3FC00000, 0x00010000, 0x80010000, 0x7F7F0000, 0xFF7F0000, 0x42280000])
def test_a_representable_value_is_returned_unchanged_for_every_r(u):
    assert _sr(u, 0) == _sr(u, 0xFFFF) == u >> 16
    r = np.arange(65536, dtype=np.uint32)
    assert (sr_ref.sr_bf16(np.full(65536, u, dtype=np.uint32), r) == u >> 16).all()


def test_zeros_denormals_infinities_and_nans():
    for r in (0, 1, 0x8000, 0xFFFF):
        assert _sr(0x00000000, r) == 0x0000 and _sr(0x80000000, r) == 0x8000            # +0, and -0 stays -0
        assert _sr(0x7F800000, r) == 0x7F80 and _sr(0xFF800000, r) == 0xFF80            # +-inf
        for nan in (0x7F800001, 0xFF800001, 0x7F80FFFF, 0x7F808000):                    # payload only in the low 16 bits
            out = _sr(nan, r)
            assert (out & 0x7F80) == 0x7F80 and (out & 0x007F) != 0 and out >> 15 == nan >> 31
        assert _sr(0x7FC00000, r) == 0x7FC0
    # the smallest denormal: stays 0 unless r is 0xFFFF, then becomes the smallest bf16 denormal -- probability 1 / 65536
    assert _sr(0x00000001, 0xFFFE) == 0x0000 and _sr(0x00000001, 0xFFFF) == 0x0001
    assert _sr(0x80000001, 0xFFFE) == 0x8000 and _sr(0x80000001, 0xFFFF) == 0x8001
    # the largest finite fp32 lies above the largest bf16: it stays there or becomes inf, as round-to-nearest makes it
    assert _sr(0x7F7FFFFF, 0) == 0x7F7F and _sr(0x7F7FFFFF, 1) == 0x7F80 and _sr(0xFF7FFFFF, 0xFFFF) == 0xFF80


def test_a_negative_value_with_a_known_fraction_goes_up_in_magnitude_with_that_probability():
    u = 0xC0490FDB                       # -3.14159274: low 16 bits 0x0FDB = 4059
    r = np.arange(65536, dtype=np.uint32)
    out = sr_ref.sr_bf16(np.full(65536, u, dtype=np.uint32), r)
    assert set(out.tolist()) == {0xC049, 0xC04A}
    assert int((out == 0xC04A).sum()) == 0x0FDB          # exactly low16 of the 65536 values of r round the magnitude up
    assert _sr(u, 65536 - 0x0FDB) == 0xC04A and _sr(u, 65535 - 0x0FDB) == 0xC049


# ---- statistics of the generator ----------------------------------------------------------------------------------------------------
N = 1 << 20
IDX = np.arange(N, dtype=np.uint64)


def test_the_fraction_rounded_up_is_low16_over_65536():
    """4096 low-16 patterns x 4096 elements each, over both signs, a denormal exponent and the top binade; the three streams"""
    n = 4096
    highs = [0x3F80, 0xBF80, 0x0000, 0x8000, 0x7F7F]
    worst = 0.0
    total_up, total_p, total_var = 0, 0.0, 0.0
    for j in range(4096):
        low = 16 * j + 8
        u = np.full(n, (highs[j % 5] << 16) | low, dtype=np.uint32)
        r = sr_ref.sr_bits(SEED, 1 + j % 7, j % 3, j % 3, np.uint64(j * n) + IDX[:n])
        up = int((sr_ref.sr_bf16(u, r) != highs[j % 5]).sum())
        p = low / 65536.0
        sd = math.sqrt(n * p * (1 - p))                  # binomial standard deviation of the count
        worst = max(worst, abs(up - n * p) / sd)
        assert abs(up - n * p) <= K * sd, (j, low, up, n * p, sd)
        total_up, total_p, total_var = total_up + up, total_p + n * p, total_var + n * p * (1 - p)
    print(f"worst pattern: {worst:.2f} sd; pooled: {(total_up - total_p) / math.sqrt(total_var):+.2f} sd")
    assert abs(total_up - total_p) <= K * math.sqrt(total_var)      # all 16.7 million draws pooled: no bias either way


def _chi2_bytes(r):
    """chi-square statistics of the high byte and of the low byte of 16-bit draws over 256 bins"""
    out = []
    for b in (r >> np.uint32(8), r & np.uint32(0xFF)):
        counts = np.bincount(b.astype(np.int64), minlength=256)
        e = len(r) / 256.0
        out.append(float(((counts - e) ** 2).sum() / e))
    return out


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_the_16_bit_draws_are_uniform(stream):
    r = sr_ref.sr_bits(SEED, 3, 1, stream, IDX)
    assert int(r.max()) < 65536
    bound = 255 + K * math.sqrt(2 * 255)                  # chi-square with 255 degrees of freedom: mean 255, variance 510
    for chi2 in _chi2_bytes(r):
        print(f"stream {stream}: chi2 = {chi2:.1f} (bound {bound:.1f})")
        assert chi2 <= bound
    # and every single bin within K binomial standard deviations
    sd = math.sqrt(N * (1 / 256) * (255 / 256))
    for b in (r >> np.uint32(8), r & np.uint32(0xFF)):
        assert np.abs(np.bincount(b.astype(np.int64), minlength=256) - N / 256).max() <= K * sd


def _assert_uncorrelated(a, b, what):
    """two sequences of 16-bit draws: each of the 16 bits agrees in half of the positions, a < b in (nearly) half of them, and
    the pair (top nibble of a, top nibble of b) is uniform over its 256 cells -- each count within K binomial standard deviations"""
    n = len(a)
    sd = math.sqrt(n * 0.25)
    for k in range(16):
        agree = int(((((a ^ b) >> np.uint32(k)) & np.uint32(1)) == 0).sum())
        assert abs(agree - n / 2) <= K * sd, (what, "bit", k, agree)
    p_less = (65536 * 65535 // 2) / 65536.0 ** 2
    less = int((a < b).sum())
    assert abs(less - n * p_less) <= K * math.sqrt(n * p_less * (1 - p_less)), (what, "a < b", less)
    cells = np.bincount(((a >> np.uint32(12)) * np.uint32(16) + (b >> np.uint32(12))).astype(np.int64), minlength=256)
    assert np.abs(cells - n / 256).max() <= K * math.sqrt(n * (1 / 256) * (255 / 256)), (what, "joint top nibbles")
    assert not np.array_equal(a, b), what


def test_streams_neighbours_steps_buckets_seeds_and_high_index_bits_are_pairwise_uncorrelated():
    def bits(stream, seed=SEED, step=5, bucket=0, idx=IDX):
        return sr_ref.sr_bits(seed, step, bucket, stream, idx)

    p, m, v = bits(0), bits(1), bits(2)
    _assert_uncorrelated(p, m, "streams p / m")
    _assert_uncorrelated(p, v, "streams p / v")
    _assert_uncorrelated(m, v, "streams m / v")
    for s, x in enumerate((p, m, v)):
        _assert_uncorrelated(x[:-1], x[1:], f"neighbouring elements, stream {s}")
        _assert_uncorrelated(x, bits(s, step=6), f"steps t / t + 1, stream {s}")
        _assert_uncorrelated(x, bits(s, bucket=1), f"buckets 0 / 1, stream {s}")
        _assert_uncorrelated(x, bits(s, seed=SEED_B), f"two seeds, stream {s}")
        _assert_uncorrelated(x, bits(s, seed=SEED ^ (1 << 32)), f"seeds that differ in bit 32, stream {s}")
        _assert_uncorrelated(x, bits(s, step=5 + (1 << 32)), f"steps that differ in bit 32, stream {s}")
        _assert_uncorrelated(x, bits(s, idx=IDX + np.uint64(1 << 32)), f"indices that differ in bit 32, stream {s}")
        _assert_uncorrelated(x, bits(s, idx=IDX + np.uint64(1 << 45)), f"indices that differ in bit 45, stream {s}")


def test_the_bits_are_a_function_of_the_element_index_alone():
    """a range that starts at `base` draws what the whole draws there (a bucket cut into ranges); across 2^32 too"""
    whole = sr_ref.sr_bits(SEED, 2, 0, 1, np.uint64((1 << 32) - 1000) + IDX[:3000])
    part = sr_ref.sr_bits(SEED, 2, 0, 1, np.uint64((1 << 32) - 1000 + 777) + IDX[:100])
    assert np.array_equal(whole[777:877], part)
    x = np.linspace(-2, 2, 3000, dtype=np.float32)
    assert np.array_equal(sr_ref.sr_cast(x, SEED, 2, 0, 1, 5)[777:], sr_ref.sr_cast(x[777:], SEED, 2, 0, 1, 5 + 777))


# ---- the trajectory: setup, oracle and host restatement (shared with tests/test_stochastic_rounding_gpu.py) ------------------------
TRAJ_N, TRAJ_HALF, TRAJ_T = 65541, 32768, 200
TRAJ_P0, TRAJ_G, TRAJ_LR, TRAJ_BETAS, TRAJ_EPS = 0.75, 0.5, 1e-4, (0.9, 0.999), 1e-8
TRAJ_P_BOUND, TRAJ_MOMENT_REL = 2e-3, 0.01


def traj_grad():
    g = np.zeros(TRAJ_N, dtype=np.float32)
    g[:TRAJ_HALF], g[TRAJ_HALF:2 * TRAJ_HALF] = TRAJ_G, -TRAJ_G
    return g


def traj_oracle(g):
    """float64 AdamW (no weight decay) on one element with the constant gradient g -> (p, m, v) after TRAJ_T steps"""
    (b1, b2), p, m, v = TRAJ_BETAS, TRAJ_P0, 0.0, 0.0
    for t in range(1, TRAJ_T + 1):
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p -= TRAJ_LR * (m / (1 - b1 ** t)) / (math.sqrt(v / (1 - b2 ** t)) + TRAJ_EPS)
    return p, m, v


def traj_check(p, m, v, stochastic):
    """p, m, v: float64 numpy arrays of the final state.  The assertions of the trajectory test; prints every figure first."""
    figures = []
    for name, sl, g in (("first half", slice(0, TRAJ_HALF), TRAJ_G), ("second half", slice(TRAJ_HALF, 2 * TRAJ_HALF), -TRAJ_G)):
        po, mo, vo = traj_oracle(g)
        assert abs(abs(po - TRAJ_P0) - 0.02) < 1e-6          # the oracle ends at 0.75 -+ 0.02
        dp = abs(float(p[sl].mean()) - po)
        dm = abs(float(np.abs(m[sl]).mean()) / abs(mo) - 1)
        dv = abs(float(v[sl].mean()) / vo - 1)
        print(f"{name}: |mean(p) - p_f64| = {dp:.3e} (bound {TRAJ_P_BOUND:.0e}); mean|m| off by {dm:.3e}, mean(v) off by {dv:.3e} "
              f"(bound {TRAJ_MOMENT_REL})")
        figures.append((dp, dm, dv))
    for dp, dm, dv in figures:
        if stochastic:
            assert dp <= TRAJ_P_BOUND and dm <= TRAJ_MOMENT_REL and dv <= TRAJ_MOMENT_REL
        else:       # the control: round-to-nearest never moves p = 0.75 by lr = 1e-4, and misses the bound by 0.02
            assert dp > TRAJ_P_BOUND and abs(dp - 0.02) < 1e-6
    return figures


def _bf2f(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _rne(x):
    u = x.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)      # finite values


def host_step(p, m, v, g, t, stochastic, seed=0, bucket=0, lr=TRAJ_LR, wd=0.0):
    """one step on bf16 bits (uint16 arrays), fp32 arithmetic in the order of the kernel's element function; not claimed to be
    bit-identical to it (numpy does not fuse)"""
    f = np.float32
    (b1, b2), eps = TRAJ_BETAS, f(TRAJ_EPS)
    inv_bc1, inv_bc2_sqrt = f(1.0 / (1.0 - f(b1) ** t)), f(1.0 / math.sqrt(1.0 - float(f(b2)) ** t))
    pf, mf, vf = _bf2f(p), _bf2f(m), _bf2f(v)
    vf = f(b2) * vf + ((f(1) - f(b2)) * g) * g
    mf = mf + (f(1) - f(b1)) * (g - mf)
    pf = (f(1) - f(lr) * f(wd)) * pf - (f(lr) * inv_bc1) * (mf / (np.sqrt(vf) * inv_bc2_sqrt + eps))
    if not stochastic:
        return _rne(pf), _rne(mf), _rne(vf)
    h = sr_ref.sr_hash(sr_ref.sr_key(seed, t, bucket), np.arange(len(p), dtype=np.uint64))
    return tuple(sr_ref.sr_bf16(x.view(np.uint32), sr_ref.sr_draw(h, s)) for s, x in enumerate((pf, mf, vf)))


@pytest.mark.parametrize("stochastic", [True, False], ids=["stochastic", "nearest-control"])
def test_trajectory_bound_holds_for_the_method_on_the_host(stochastic):
    g = traj_grad()
    p0 = _rne(np.full(TRAJ_N, TRAJ_P0, dtype=np.float32))
    p, m, v = p0.copy(), np.zeros(TRAJ_N, dtype=np.uint16), np.zeros(TRAJ_N, dtype=np.uint16)
    for t in range(1, TRAJ_T + 1):
        p, m, v = host_step(p, m, v, g, t, stochastic, seed=SEED)
    traj_check(_bf2f(p).astype(np.float64), _bf2f(m).astype(np.float64), _bf2f(v).astype(np.float64), stochastic)
    assert np.array_equal(p[2 * TRAJ_HALF:], p0[2 * TRAJ_HALF:])          # zero gradient: the last 5 keep p0 bit for bit
    if not stochastic:
        assert np.array_equal(p, p0)                                       # every p is stalled at 0.75
