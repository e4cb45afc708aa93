// attention_probe.hip -- the softmax probabilities of a few selected query rows over all keys (gfx950).  An evaluation
// instrument, read-only: the fused attention kernels never materialise a probability, this one reports the distribution they
// applied for up to DVLA_PROBE_MAX_ROWS rows of each sequence.  An addition: the reference has no such probe.
//
// One workgroup of four waves per (sequence, head, selected row); nothing is shared between workgroups, so what a row gets depends
// on its own q row, the keys and the mask alone -- not on B, the sequence's index in the batch, the grid or the other rows -- and
// is the same bits on every run.  No atomics, no host synchronisation, 32 bytes of LDS.
//   1. the workgroup zero-fills its output row (original key numbering, Lk_full columns): keys the row cannot see, keys nobody
//      sees (absent from key_index) and rows that are out of range or blind end as exactly 0.0f; a barrier;
//   2. pass A, the only one that reads K: the 32-key tiles whose mask word is zero for this row are never loaded, the others are
//      dealt to the four waves in turn (a single wave per row spent its time waiting for one tile after the other: at one
//      episode the trunk's 24 probes took 2.7 ms of a control step).  Eight lanes share a key (lane g of the eight owns the
//      16-byte vectors g and g + 8 of the key row: coalesced 128-byte rows at head_dim 64), eight keys per wave and load, the
//      four loads of a tile issued together.  score = scale * <q, k>, fp32 FMAs in element order per lane, then three xor steps
//      over the eight lanes.  The group's first lane parks the score in the output element it will later overwrite and keeps the
//      running maximum; the waves' maxima meet in LDS;
//   3. pass B: the same lanes read their scores back and add exp(score - max) in key order, one chain per lane, then three xor
//      steps over the eight groups and (w0 + w1) + (w2 + w3) over the waves;
//   4. pass C: the same lanes store exp(score - max) / sum.
// A lane only ever re-reads what it stored itself; the zero-fill, which other lanes did, is ordered before pass A by the barrier.
// The head mean (sum over h ascending, divided by H) is a second small launch over the per-head rows.
#include "common.h"
#include "launch.h"
#include "../../include/dvla.h"

namespace {

struct ProbeArgs {
  const bf16_t* q; const bf16_t* k;
  int64_t q_sb, q_st, q_sh, k_sb, k_st, k_sh;
  const int32_t* key_index; const uint32_t* bits_q; const int32_t* rows;
  float* out;                   // (B, H, R, Lk_full)
  int32_t H, R, Lq, Lk, Lk_full, D;
  float scale;
};

__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[2 * i] = bf2f((bf16_t)(w[i] & 0xffff)); f[2 * i + 1] = bf2f((bf16_t)(w[i] >> 16)); }
}

// eight consecutive bf16: one 16-byte load where the view allows it, eight 2-byte loads otherwise
template <bool VEC>
__device__ __forceinline__ uint4 load8(const bf16_t* __restrict__ p) {
  if (VEC) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)p[2 * i] | ((uint32_t)p[2 * i + 1] << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// the mask word of tile kt for this row, trimmed to the keys that exist
__device__ __forceinline__ uint32_t tile_word(const uint32_t* __restrict__ bits_row, int kt, int Lk) {
  const int n = Lk - kt * 32;
  const uint32_t valid = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
  return (bits_row ? bits_row[kt] : 0xffffffffu) & valid;
}

// the output column of compacted key kc, or -1 when the table names a column that does not exist
__device__ __forceinline__ int key_column(const int32_t* __restrict__ key_index, int kc, int Lk_full) {
  const int c = key_index ? key_index[kc] : kc;
  return (c >= 0 && c < Lk_full) ? c : -1;
}

// Passes B (PASS 0: the sum of exp(score - m) over this wave's tiles) and C (PASS 1: the scores replaced by exp(score - m) / l): the
// lanes that parked the scores in pass A, over exactly the elements they parked.
template <int PASS>
__device__ __forceinline__ float sweep_owned(const ProbeArgs& a, const uint32_t* __restrict__ bits_row, float* __restrict__ out,
                                             int nkt, int lane, int wave, float m, float l) {
  const int sub = lane >> 3;
  const bool own = (lane & 7) == 0;
  float sum = 0.f;
  int ord = 0;
  for (int base = 0; base < nkt; base += 64) {
    const int mine = base + lane;
    const uint32_t my_word = mine < nkt ? tile_word(bits_row, mine, a.Lk) : 0u;
    unsigned long long live = __ballot(my_word != 0u);
    while (live) {
      const int t = __ffsll((long long)live) - 1;
      live &= live - 1;
      if ((ord++ & 3) != wave) continue;
      const uint32_t word = (uint32_t)__shfl((int)my_word, t, 64);
      const int k0 = (base + t) * 32;
      if (own) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int j = it * 8 + sub;
          const int c = ((word >> j) & 1u) ? key_column(a.key_index, k0 + j, a.Lk_full) : -1;
          if (c >= 0) {
            const float e = expf(out[c] - m);
            if (PASS == 0) sum += e; else out[c] = e / l;
          }
        }
      }
    }
  }
  return sum;
}

template <bool VEC>
__global__ __launch_bounds__(256) void probe_rows_kernel(ProbeArgs a) {
  __shared__ float red_m[4], red_l[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = blockIdx.x;                  // (b, h, r), the order of the output rows
  const int r = (int)(w % a.R);
  const int h = (int)((w / a.R) % a.H);
  const int64_t b = w / ((int64_t)a.R * a.H);
  float* __restrict__ out = a.out + w * a.Lk_full;
  for (int c = threadIdx.x; c < a.Lk_full; c += 256) out[c] = 0.f;
  const int row = a.rows[b * a.R + r];
  if (row < 0 || row >= a.Lq) return;            // (the whole workgroup: one row)
  __syncthreads();                               // the zeros are in place before anybody parks a score

  const int g = lane & 7, sub = lane >> 3;       // lane g of the eight that share a key; the wave's key slot 0..7
  const int nv = a.D >> 3;                       // 16-byte vectors per key row, 1..16
  const bool own = g == 0;
  float qf[2][8];
  {
    const bf16_t* qrow = a.q + b * a.q_sb + (int64_t)row * a.q_st + (int64_t)h * a.q_sh;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (g + 8 * v < nv) u = load8<VEC>(qrow + (g + 8 * v) * 8);
      unpack8(u, qf[v]);
    }
  }
  const bf16_t* kbase = a.k + b * a.k_sb + (int64_t)h * a.k_sh;
  const int nkt = (a.Lk + 31) >> 5;
  const uint32_t* bits_row = a.bits_q ? a.bits_q + (int64_t)row * nkt : nullptr;

  // pass A: the row's live tiles, dealt to the four waves in turn
  float m = -__builtin_huge_valf();
  int ord = 0;
  for (int base = 0; base < nkt; base += 64) {
    const int mine = base + lane;
    const uint32_t my_word = mine < nkt ? tile_word(bits_row, mine, a.Lk) : 0u;
    unsigned long long live = __ballot(my_word != 0u);
    while (live) {
      const int t = __ffsll((long long)live) - 1;
      live &= live - 1;
      if ((ord++ & 3) != wave) continue;
      const uint32_t word = (uint32_t)__shfl((int)my_word, t, 64);
      const int k0 = (base + t) * 32;
      uint4 kv[4][2];
      int col[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int j = it * 8 + sub;
        col[it] = ((word >> j) & 1u) ? key_column(a.key_index, k0 + j, a.Lk_full) : -1;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          kv[it][v] = make_uint4(0u, 0u, 0u, 0u);
          if (col[it] >= 0 && g + 8 * v < nv) kv[it][v] = load8<VEC>(kbase + (int64_t)col[it] * a.k_st + (g + 8 * v) * 8);
        }
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        float acc = 0.f;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          float kf[8];
          unpack8(kv[it][v], kf);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc = fmaf(qf[v][e], kf[e], acc);
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        const float s = acc * a.scale;
        if (own && col[it] >= 0) { out[col[it]] = s; m = fmaxf(m, s); }
      }
    }
  }
  m = fmaxf(m, __shfl_xor(m, 8, 64));
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (lane == 0) red_m[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
  if (!(m > -__builtin_huge_valf())) return;       // the row sees no key: all zeros (every thread reads the same four values)

  float l = sweep_owned<0>(a, bits_row, out, nkt, lane, wave, m, 0.f);
  l += __shfl_xor(l, 8, 64);
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (lane == 0) red_l[wave] = l;
  __syncthreads();
  l = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
  sweep_owned<1>(a, bits_row, out, nkt, lane, wave, m, l);
}

// out[b, r, c] = (sum over h ascending of per_head[b, h, r, c]) / H
__global__ __launch_bounds__(256) void probe_head_mean_kernel(const float* __restrict__ per_head, float* __restrict__ out, int64_t n,
                                                              int32_t H, int64_t row_elems) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / row_elems, rc = i % row_elems;
  const float* src = per_head + b * H * row_elems + rc;
  float s = 0.f;
  for (int h = 0; h < H; ++h) s += src[(int64_t)h * row_elems];
  out[i] = s / (float)H;
}

}  // namespace

extern "C" int dvla_attn_probe(const dvla_attn_params* p, const int32_t* rows, int32_t R, int32_t head_dim, int32_t Lk_full,
                               int32_t per_head, float* out, float* workspace, void* stream_) {
  if (!p || !rows || !out || !p->q || !p->k) return DVLA_ERR_ARG;
  if (p->B < 1 || p->H < 1 || p->Lq < 1 || p->Lk < 1 || Lk_full < 1 || p->Lk > Lk_full) return DVLA_ERR_ARG;
  if (!p->key_index && p->Lk != Lk_full) return DVLA_ERR_ARG;
  if (p->key_index && !p->mask_bits_q) return DVLA_ERR_ARG;
  if (!per_head && !workspace) return DVLA_ERR_ARG;
  if (R < 1 || R > DVLA_PROBE_MAX_ROWS || head_dim < 8 || head_dim > 128 || head_dim % 8 != 0) return DVLA_ERR_UNSUPPORTED;
  const int64_t blocks = (int64_t)p->B * p->H * R;      // one workgroup per output row
  const int64_t n_mean = (int64_t)p->B * R * Lk_full;
  if (blocks > 0x7fffffffLL || (n_mean + 255) / 256 > 0x7fffffffLL) return DVLA_ERR_UNSUPPORTED;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  ProbeArgs a;
  a.q = reinterpret_cast<const bf16_t*>(p->q);
  a.k = reinterpret_cast<const bf16_t*>(p->k);
  a.q_sb = p->q_stride_b; a.q_st = p->q_stride_t; a.q_sh = p->q_stride_h;
  a.k_sb = p->k_stride_b; a.k_st = p->k_stride_t; a.k_sh = p->k_stride_h;
  a.key_index = p->key_index; a.bits_q = p->mask_bits_q; a.rows = rows;
  a.out = per_head ? out : workspace;
  a.H = p->H; a.R = R; a.Lq = p->Lq; a.Lk = p->Lk; a.Lk_full = Lk_full; a.D = head_dim;
  a.scale = p->scale;
  const bool vec = dvla_aligned(p->q, a.q_sb, a.q_st, a.q_sh, 16) && dvla_aligned(p->k, a.k_sb, a.k_st, a.k_sh, 16);
  if (vec) hipLaunchKernelGGL(probe_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(probe_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  int rc = dvla_check_launch();
  if (rc != DVLA_OK || per_head) return rc;
  hipLaunchKernelGGL(probe_head_mean_kernel, dim3((unsigned)((n_mean + 255) / 256)), dim3(256), 0, stream, workspace, out, n_mean,
                     p->H, (int64_t)R * Lk_full);
  return dvla_check_launch();
}
