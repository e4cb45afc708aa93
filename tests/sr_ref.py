"""Host restatement of the stochastic rounding of include/dvla.h (dvla_sr_cast_f32_to_bf16, dvla_adamw_bf16_sr): the
counter-based generator and the rounding, in integer arithmetic only (numpy uint32 / uint64 arrays and Python ints; no floating
point anywhere in this file except the reinterpretation of fp32 data as its 32 bits)."""
import numpy as np

M32 = 0xFFFFFFFF
STREAM_P, STREAM_M, STREAM_V = 0, 1, 2


def hash32(x):
    """the hash32 of csrc/common.h on a uint32 array (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _hash32_int(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sr_key(seed, step, bucket):
    """the launch key of (seed: 64 bits, step: 64 bits, bucket: 32 bits) -> int"""
    seed, step, bucket = int(seed), int(step), int(bucket) & M32
    assert 0 <= seed < 2 ** 64 and 0 <= step < 2 ** 64
    k = _hash32_int((seed & M32) ^ 0x243F6A88)
    k = _hash32_int(k ^ (seed >> 32))
    k = _hash32_int(k ^ (step & M32))
    k = _hash32_int(k ^ (step >> 32))
    return _hash32_int(k ^ bucket)


def sr_hash(key, index):
    """per element: index is an array of 64-bit element indices -> uint32 array"""
    i = np.asarray(index).astype(np.uint64)
    lo, hi = (i & np.uint64(M32)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32)
    return hash32((np.uint32(key) ^ (hi * np.uint32(0x85EBCA6B))) + lo * np.uint32(0x9E3779B9))


def sr_draw(h, stream):
    """the 16 random bits of stream 0 (param), 1 (exp_avg) or 2 (exp_avg_sq) from an element's hash -> uint32 array < 65536"""
    if stream == 0:
        return h >> np.uint32(16)
    if stream == 1:
        return h & np.uint32(0xFFFF)
    assert stream == 2
    return hash32(h ^ np.uint32(0x5BD1E995)) >> np.uint32(16)


def sr_bits(seed, step, bucket, stream, index):
    return sr_draw(sr_hash(sr_key(seed, step, bucket), index), stream)


def sr_bf16(u, r):
    """u: the 32 bits of fp32 values, r: 16 random bits each -> the 16 bits of the bf16 values (uint16 array)"""
    u, r = np.asarray(u, dtype=np.uint32), np.asarray(r, dtype=np.uint32)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    nan = special & ((u & np.uint32(0x007FFFFF)) != 0)
    out = np.where(special, u >> np.uint32(16), (u + r) >> np.uint32(16))      # no wrap: u < 0xFF800000 where r is added
    return np.where(nan, out | np.uint32(0x0040), out).astype(np.uint16)


def sr_cast(x, seed=0, step=0, bucket=0, stream=0, index_base=0):
    """dvla_sr_cast_f32_to_bf16 of a float32 numpy array -> uint16 array of the same shape (the bf16 bits)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    index = np.uint64(index_base) + np.arange(x.size, dtype=np.uint64)
    return sr_bf16(x.reshape(-1).view(np.uint32), sr_bits(seed, step, bucket, stream, index)).reshape(x.shape)
