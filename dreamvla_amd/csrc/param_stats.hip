// param_stats.hip -- per-parameter reductions over the flat optimizer buffers (gfx950), HBM-bound.  An addition: the reference
// has no such telemetry.
//
// Every parameter of a gradient bucket is a contiguous segment of a few flat buffers (gradients, parameters / fp32 masters, both
// moments) at the same element offsets.  One launch per bucket and buffer (stage 1) and one launch for all buckets (stage 2) give
// every per-parameter statistic, with no atomics and no host synchronisation:
//   dvla_segment_stats_bf16 / _f32 : stage 1 for the sum of squares, the largest |x| over the elements that are not NaN, and the
//                                    number of non-finite elements
//   dvla_segment_adam_bf16 / _f32  : stage 1 for the sum of squares of r = exp_avg / denom(exp_avg_sq), denom being the step's own
//                                    expression (adam_one / master_one of optimizer.hip); no lr enters, the host scales
//   dvla_segment_combine           : stage 2 of either, for every segment of every bucket
//   dvla_group_sumsq               : the per-parameter sums of squares of the gradient added per parameter group (one wave): the
//                                    clip norms of FlatAdamW(clip="group"), instead of the dvla_sumsq_* pass
// The host cuts every segment into chunks of DVLA_STATS_CHUNK elements counted from the segment's own first element (dvla.h: the
// chunk table).  Stage 1: a workgroup of four waves per chunk (grid-stride over the table), 16-byte loads, thread t of the
// workgroup owns vectors t, t + 256, ... of the chunk and adds its elements in element order; the ragged end of a segment
// (len % 8 elements) goes through scalar loads; one 16-byte record per chunk.  Stage 2: one wave per segment adds the segment's
// records in chunk order, the sum in double.  What a segment gets therefore depends on its own elements and nothing else: not on
// the grid, the bucket, its neighbours or where in the bucket it sits.  Alignment gaps between segments are never read.
#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int CHUNK = DVLA_STATS_CHUNK;
constexpr int ROUNDS = CHUNK / (256 * 8);        // 16-byte vectors of 8 elements per thread and chunk
static_assert(CHUNK % (256 * 8) == 0, "a chunk is a whole number of vectors per thread");

struct SegPartial { float ss, mx; int32_t nf, pad; };
static_assert(sizeof(SegPartial) == DVLA_STATS_PARTIAL_BYTES, "dvla.h publishes the record size");

struct Acc { float ss, mx; int32_t nf; };

__device__ __forceinline__ void stat_one(Acc& a, float x) {
  const float ax = fabsf(x);
  a.ss = fmaf(x, x, a.ss);
  a.mx = fmaxf(a.mx, ax);                            // a NaN is dropped, an inf stays
  a.nf += !(ax < __builtin_huge_valf());             // NaN or +-inf
}

// the Adam term of one element, denominators as the step kernels of optimizer.hip have them
struct AdamTerm { float c, eps; };                   // c: bc2_sqrt (fp32 masters) or inv_bc2_sqrt (bf16)
__device__ __forceinline__ void adam_one_f32(Acc& a, float m, float v, const AdamTerm& t) {
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), t.c), t.eps);      // master_one
  const float r = __fdiv_rn(m, denom);
  a.ss = fmaf(r, r, a.ss);
}
__device__ __forceinline__ void adam_one_bf16(Acc& a, float m, float v, const AdamTerm& t) {
  const float denom = fmaf(sqrtf(v), t.c, t.eps);                           // adam_one, as adamw_kernel contracts it
  const float r = m / denom;
  a.ss = fmaf(r, r, a.ss);
}

__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[2 * k] = bf2f((bf16_t)(w[k] & 0xffff)); f[2 * k + 1] = bf2f((bf16_t)(w[k] >> 16)); }
}

// One chunk in registers: W 16-byte vectors per thread and round (1 for bf16, 2 for fp32) + this thread's element of the ragged
// end.  BF16: the buffers' element type.  ADAM: x = exp_avg, y = exp_avg_sq and the record carries the sum of r^2 alone; otherwise y is
// unused.
template <bool BF16, bool ADAM>
struct Chunk {
  static constexpr int W = BF16 ? 1 : 2;
  uint4 x[ROUNDS * W], y[ADAM ? ROUNDS * W : 1];
  float tx, ty;
  int nvec, tail;
};

// n: elements of the buffers; a table row that does not lie inside them is not read and counts as an empty chunk
template <bool BF16, bool ADAM>
__device__ __forceinline__ void load_chunk(Chunk<BF16, ADAM>& k, const void* __restrict__ x_, const void* __restrict__ y_, int64_t n,
                                           const int64_t* __restrict__ chunks, int64_t c, int tid) {
  constexpr int W = Chunk<BF16, ADAM>::W;
  const int64_t start = chunks[2 * c], len = chunks[2 * c + 1];
  const bool ok = start >= 0 && (start & 7) == 0 && len >= 0 && len <= CHUNK && start <= n - len;      // uniform over the workgroup
  k.nvec = ok ? (int)(len >> 3) : 0;
  k.tail = ok ? (int)(len & 7) : 0;
  const int64_t esize = BF16 ? 2 : 4;
  const char* x = reinterpret_cast<const char*>(x_) + start * esize;
  const char* y = reinterpret_cast<const char*>(y_) + start * esize;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int v = tid + 256 * r;
#pragma unroll
    for (int h = 0; h < W; ++h) {
      if (v < k.nvec) {
        k.x[W * r + h] = reinterpret_cast<const uint4*>(x)[W * v + h];
        if (ADAM) k.y[W * r + h] = reinterpret_cast<const uint4*>(y)[W * v + h];
      }
    }
  }
  k.tx = 0.f; k.ty = 0.f;
  if (tid < k.tail) {                                // the segment's ragged end: scalar loads
    const int e = (k.nvec << 3) + tid;
    if (BF16) {
      k.tx = bf2f(reinterpret_cast<const bf16_t*>(x)[e]);
      if (ADAM) k.ty = bf2f(reinterpret_cast<const bf16_t*>(y)[e]);
    } else {
      k.tx = reinterpret_cast<const float*>(x)[e];
      if (ADAM) k.ty = reinterpret_cast<const float*>(y)[e];
    }
  }
}

// this thread's elements of the chunk, in element order: vectors tid, tid + 256, ..., then its element of the ragged end
template <bool BF16, bool ADAM>
__device__ __forceinline__ void add_chunk(Acc& a, const Chunk<BF16, ADAM>& k, const AdamTerm& t, int tid) {
  constexpr int W = Chunk<BF16, ADAM>::W;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    if (tid + 256 * r < k.nvec) {
#pragma unroll
      for (int h = 0; h < W; ++h) {
        const uint4 ux = k.x[W * r + h], uy = k.y[ADAM ? W * r + h : 0];
        if (BF16) {
          float fx[8], fy[8];
          unpack8(ux, fx);
          if (ADAM) unpack8(uy, fy);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (ADAM) adam_one_bf16(a, fx[e], fy[e], t); else stat_one(a, fx[e]);
          }
        } else {
          const float fx[4] = {__uint_as_float(ux.x), __uint_as_float(ux.y), __uint_as_float(ux.z), __uint_as_float(ux.w)};
          const float fy[4] = {__uint_as_float(uy.x), __uint_as_float(uy.y), __uint_as_float(uy.z), __uint_as_float(uy.w)};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (ADAM) adam_one_f32(a, fx[e], fy[e], t); else stat_one(a, fx[e]);
          }
        }
      }
    }
  }
  if (tid < k.tail) {
    if (ADAM) { if (BF16) adam_one_bf16(a, k.tx, k.ty, t); else adam_one_f32(a, k.tx, k.ty, t); } else stat_one(a, k.tx);
  }
}

// Grid-stride over the chunk table, the whole workgroup on one chunk at a time.  The loads of the workgroup's next chunk are issued
// before the reduction of the current one, and the four waves' partial results alternate between two LDS slots, so there is one
// barrier per chunk and memory stays busy across it.
template <bool BF16, bool ADAM>
__global__ __launch_bounds__(256) void seg_stage1_kernel(const void* __restrict__ x_, const void* __restrict__ y_, int64_t n,
                                                         const int64_t* __restrict__ chunks, int64_t n_chunks,
                                                         SegPartial* __restrict__ part, AdamTerm t) {
  __shared__ float red_ss[2][4], red_mx[2][4];
  __shared__ int32_t red_nf[2][4];
  const int tid = threadIdx.x;
  int64_t c = blockIdx.x;
  Chunk<BF16, ADAM> k;
  if (c < n_chunks) load_chunk(k, x_, y_, n, chunks, c, tid);
  int slot = 0;
  while (c < n_chunks) {
    Acc a = {0.f, 0.f, 0};
    add_chunk(a, k, t, tid);
    const int64_t nx = c + gridDim.x;
    if (nx < n_chunks) load_chunk(k, x_, y_, n, chunks, nx, tid);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {               // six steps over the wave
      a.ss += __shfl_xor(a.ss, o, 64);
      if (!ADAM) { a.mx = fmaxf(a.mx, __shfl_xor(a.mx, o, 64)); a.nf += __shfl_xor(a.nf, o, 64); }
    }
    if ((tid & 63) == 0) { red_ss[slot][tid >> 6] = a.ss; red_mx[slot][tid >> 6] = a.mx; red_nf[slot][tid >> 6] = a.nf; }
    __syncthreads();
    if (tid == 0) {                                  // two levels of adds over the four waves
      SegPartial p;
      p.ss = (red_ss[slot][0] + red_ss[slot][1]) + (red_ss[slot][2] + red_ss[slot][3]);
      p.mx = fmaxf(fmaxf(red_mx[slot][0], red_mx[slot][1]), fmaxf(red_mx[slot][2], red_mx[slot][3]));
      p.nf = red_nf[slot][0] + red_nf[slot][1] + red_nf[slot][2] + red_nf[slot][3];
      p.pad = 0;
      part[c] = p;
    }
    // no second barrier: the next chunk writes the other slot, and nobody gets to the chunk after it -- this slot again --
    // before thread 0 has passed the next barrier, that is, after it has read this one
    slot ^= 1;
    c = nx;
  }
}

// One wave per segment: the records of the segment's chunks, 64 at a time, added in chunk order (every lane runs the same
// chain on broadcast values); maximum and count are exact in any order.  segs rows: first chunk, number of chunks, index into
// the outputs.  A row that points outside the records or the outputs writes nothing.
__global__ __launch_bounds__(256) void seg_stage2_kernel(const SegPartial* __restrict__ part, int64_t n_chunks,
                                                         const int64_t* __restrict__ segs, int n_segs, float* __restrict__ sumsq,
                                                         float* __restrict__ absmax, int64_t* __restrict__ nonfinite, int64_t n_out) {
  const int seg = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (seg >= n_segs) return;
  const int64_t first = segs[3 * seg], cnt = segs[3 * seg + 1], out = segs[3 * seg + 2];
  if (out < 0 || out >= n_out || first < 0 || cnt < 0 || first > n_chunks - cnt) return;
  double s = 0.0;
  float mx = 0.f;
  long long nf = 0;
  for (int64_t base = 0; base < cnt; base += 64) {
    const int64_t rest = cnt - base;
    const int m = rest < 64 ? (int)rest : 64;
    SegPartial p = {0.f, 0.f, 0, 0};
    if (lane < m) p = part[first + base + lane];
    for (int k = 0; k < m; ++k) s += (double)__shfl(p.ss, k, 64);
    mx = fmaxf(mx, p.mx);
    nf += p.nf;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    nf += __shfl_xor(nf, o, 64);
  }
  if (lane == 0) {
    sumsq[out] = (float)s;
    if (absmax) absmax[out] = mx;
    if (nonfinite) nonfinite[out] = nf;
  }
}

// One wave: lane g owns group g.  Every lane walks the parameters in index order (64 at a time, broadcast from the lane that
// loaded them) and adds those of its own group, in double; a term is selected, never multiplied by a mask, so a NaN reaches
// its own group only.  Lane 0 then adds the groups' fp32 sums in index order: step_verdict_kernel's chain over the same slots.
__global__ __launch_bounds__(64) void group_sumsq_kernel(const float* __restrict__ param_sumsq, const uint8_t* __restrict__ group_of,
                                                         int n_params, int n_groups, float* __restrict__ group_sumsq,
                                                         float* __restrict__ total) {
  static_assert(DVLA_STEP_MAX_GROUPS == 64, "one lane per group");
  __shared__ float sums[DVLA_STEP_MAX_GROUPS];
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int base = 0; base < n_params; base += 64) {
    const int rest = n_params - base;
    const int m = rest < 64 ? rest : 64;
    float v = 0.f;
    int id = 255;
    if (lane < m) { v = param_sumsq[base + lane]; id = group_of[base + lane]; }
    for (int k = 0; k < m; ++k) {
      const float vk = __shfl(v, k, 64);
      if (__shfl(id, k, 64) == lane) s += (double)vk;
    }
  }
  const float f = (float)s;
  sums[lane] = f;
  if (lane < n_groups) group_sumsq[lane] = f;
  __syncthreads();
  if (lane == 0 && total) {
    float t = sums[0];
    for (int g = 1; g < n_groups; ++g) t = t + sums[g];
    total[0] = t;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BF16, bool ADAM>
int run(const void* x, const void* y, int64_t n, const int64_t* chunks, int64_t n_chunks, void* partial, AdamTerm t,
        hipStream_t stream) {
  // two workgroups' worth of waves per SIMD on every CU, each with a chunk in flight and one being reduced
  const int64_t blocks = n_chunks < 2048 ? n_chunks : 2048;
  hipLaunchKernelGGL((seg_stage1_kernel<BF16, ADAM>), dim3((unsigned)blocks), dim3(256), 0, stream, x, y, n, chunks, n_chunks,
                     reinterpret_cast<SegPartial*>(partial), t);
  return dvla_check_launch();
}

}  // namespace

extern "C" int dvla_segment_stats_bf16(const void* x, int64_t n, const int64_t* chunks, int64_t n_chunks, void* partial,
                                       void* stream_) {
  if (!x || !chunks || !partial || n < 0 || n_chunks < 0) return DVLA_ERR_ARG;
  if (n_chunks == 0) return DVLA_OK;
  if (!al16(x) || !al16(chunks) || !al16(partial)) return DVLA_ERR_UNSUPPORTED;
  return run<true, false>(x, x, n, chunks, n_chunks, partial, AdamTerm{0.f, 0.f}, reinterpret_cast<hipStream_t>(stream_));
}

extern "C" int dvla_segment_stats_f32(const float* x, int64_t n, const int64_t* chunks, int64_t n_chunks, void* partial,
                                      void* stream_) {
  if (!x || !chunks || !partial || n < 0 || n_chunks < 0) return DVLA_ERR_ARG;
  if (n_chunks == 0) return DVLA_OK;
  if (!al16(x) || !al16(chunks) || !al16(partial)) return DVLA_ERR_UNSUPPORTED;
  return run<false, false>(x, x, n, chunks, n_chunks, partial, AdamTerm{0.f, 0.f}, reinterpret_cast<hipStream_t>(stream_));
}

// The step-dependent scalar comes from dvla_step_candidates, which the step kernels' entry points and the guarded step's table
// share: the same float, whichever way the step that wrote the moments got it.
extern "C" int dvla_segment_adam_bf16(const void* exp_avg, const void* exp_avg_sq, int64_t n, const int64_t* chunks, int64_t n_chunks,
                                      void* partial, float beta2, float eps, int64_t step, void* stream_) {
  if (!exp_avg || !exp_avg_sq || !chunks || !partial || n < 0 || n_chunks < 0 || step < 1) return DVLA_ERR_ARG;
  if (n_chunks == 0) return DVLA_OK;
  if (!al16(exp_avg) || !al16(exp_avg_sq) || !al16(chunks) || !al16(partial)) return DVLA_ERR_UNSUPPORTED;
  dvla_step_scalars sc;
  const int rc = dvla_step_candidates(0.0, 0.0, (double)beta2, step, 1, &sc);
  if (rc != DVLA_OK) return rc;
  return run<true, true>(exp_avg, exp_avg_sq, n, chunks, n_chunks, partial, AdamTerm{sc.inv_bc2_sqrt, eps},
                         reinterpret_cast<hipStream_t>(stream_));
}

extern "C" int dvla_segment_adam_f32(const float* exp_avg, const float* exp_avg_sq, int64_t n, const int64_t* chunks, int64_t n_chunks,
                                     void* partial, double beta2, double eps, int64_t step, void* stream_) {
  if (!exp_avg || !exp_avg_sq || !chunks || !partial || n < 0 || n_chunks < 0 || step < 1) return DVLA_ERR_ARG;
  if (n_chunks == 0) return DVLA_OK;
  if (!al16(exp_avg) || !al16(exp_avg_sq) || !al16(chunks) || !al16(partial)) return DVLA_ERR_UNSUPPORTED;
  dvla_step_scalars sc;
  const int rc = dvla_step_candidates(0.0, 0.0, beta2, step, 1, &sc);
  if (rc != DVLA_OK) return rc;
  return run<false, true>(exp_avg, exp_avg_sq, n, chunks, n_chunks, partial, AdamTerm{sc.bc2_sqrt, (float)eps},
                          reinterpret_cast<hipStream_t>(stream_));
}

extern "C" int dvla_segment_combine(const void* partial, int64_t n_chunks, const int64_t* segs, int32_t n_segs, float* sumsq,
                                    float* absmax, int64_t* nonfinite, int64_t n_out, void* stream_) {
  if (!partial || !segs || !sumsq || n_chunks < 0 || n_segs < 0 || n_out < 0) return DVLA_ERR_ARG;
  if (n_segs == 0) return DVLA_OK;
  if (!al16(partial)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(seg_stage2_kernel, dim3((unsigned)((n_segs + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_),
                     reinterpret_cast<const SegPartial*>(partial), n_chunks, segs, (int)n_segs, sumsq, absmax, nonfinite, n_out);
  return dvla_check_launch();
}

// ---- per-group clip norms (additive, ABI 9) ---------------------------------------------------------------------------------
extern "C" int dvla_group_sumsq(const float* param_sumsq, const uint8_t* group_of, int32_t n_params, int32_t n_groups,
                                float* group_sumsq, float* total, void* stream_) {
  if (!param_sumsq || !group_of || !group_sumsq || n_params < 0 || n_groups < 1 || n_groups > DVLA_STEP_MAX_GROUPS)
    return DVLA_ERR_ARG;
  hipLaunchKernelGGL(group_sumsq_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_), param_sumsq, group_of,
                     (int)n_params, (int)n_groups, group_sumsq, total);
  return dvla_check_launch();
}
