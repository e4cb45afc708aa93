// attention_hd.hip -- fused multi-head attention for head widths other than 64: forward + backward for gfx950.
//
// Same semantics, masks, dropout keep mask and rounding points as the head-width-64 kernels of attention.hip (dvla_attn_fwd /
// dvla_attn_bwd, include/dvla.h), for head_dim D a multiple of 8 with 8 <= D <= 128, D != 64.  The kernels are templated on a
// padded width DP in {32, 64, 96, 128} (D rounded up to a multiple of 32): the d columns D..DP-1 of Q / K / V / dO are zero-filled
// where they are staged (registers or LDS), so they add nothing to any product, and output columns >= D are never stored.
//
// Structure: the register-staged "transposed flash attention" of attention.hip, widened over d.
//   * every score tile is S^T = K.Q^T with v_mfma_f32_32x32x16_bf16(a = K fragment, b = Q fragment): a lane owns one query
//     (q = lane & 31) and 16 of the tile's 32 keys (key = (r&3) + 8*(r>>2) + 4*(lane>>5)) -- DP / 16 MFMAs per tile;
//   * P (bf16) is already the B operand of O^T = V^T.P^T; V^T fragments come from a pair-interleaved LDS image [key/2][d];
//   * the running maximum is an integer in the log2 domain, the row sum is over unrounded probabilities, P and dS are rounded to
//     bf16 before the second product -- oracle/torch_ref.py::attention_bf16 describes these kernels exactly as it does the D = 64 ones;
//   * dropout: the same (seed, b, h, query, key tile, key) -> keep hash as attention.hip (common.h), so one keep mask serves both.
// K/V (forward, dQ) or Q/dO (dK/dV) tiles of 32 rows are staged global -> registers -> LDS, double-buffered, one barrier per tile.
// Backward = delta kernel (rowsum dO.O) + dQ kernel (forward orientation) + dK/dV kernel (a wave owns 32 keys, S = Q.K^T so the
// lane owns a key and dK^T / dV^T accumulate in registers).  No atomics, no host synchronisation, no allocation: capturable.
#include "common.h"
#include "launch.h"
#include "../../include/dvla.h"

namespace {

constexpr int HD_THREADS = 256;
constexpr float HD_LOG2E = 1.4426950408889634f;
constexpr float HD_LN2 = 0.6931471805599453f;

struct HdArgs {
  const bf16_t *q, *k, *v; bf16_t* o;
  int64_t qsb, qst, qsh, ksb, kst, ksh, vsb, vst, vsh, osb, ost, osh;
  int B, H, Lq, Lk, D;
  float scale;
  const int32_t* key_index;
  const uint32_t *bits_q, *bits_k;
  const uint8_t* tile_map; int nqt, nkt;
  int has_drop; uint32_t drop_thr; float inv_keep; uint32_t seed_lo, seed_hi;
  float c1;   // scale / keep
  float* lse;
  const bf16_t* dout; int64_t dsb, dst, dsh;
  float* delta;
  bf16_t *dq, *dk, *dv;
  int64_t dqsb, dqst, dqsh, dksb, dkst, dksh, dvsb, dvst, dvsh;
};

// LDS images of one 32-row tile at padded width DP
template <int DP> struct HdTile {
  static constexpr int RMS = DP + 8;                 // row-major stride in bf16 (16-B aligned rows, staggered banks)
  static constexpr int RM_BYTES = 32 * RMS * 2;
  static constexpr int PI_BYTES = 16 * DP * 4;       // pair-interleaved: [row pair][d] dwords {row even, row odd}
  static constexpr int NOCT = DP / 8;                // 16-byte pieces per row
  static constexpr int NIT = (16 * NOCT + 127) / 128;   // staging pieces (of two rows) per thread of a 128-thread group
  static constexpr int NS = DP / 16;                 // k-steps of a product over d
  static constexpr int NDB = DP / 32;                // 32-wide d blocks of an output accumulator
};

__device__ __forceinline__ int hd_acc_row(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }
__device__ __forceinline__ uint4 hd_load16(const bf16_t* p, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p) : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ f32x16 hd_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
__device__ __forceinline__ uint32_t hd_low_mask(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }
__device__ __forceinline__ bool hd_vis_bit(uint32_t vg, int r) { return (vg >> ((r & 3) + 8 * (r >> 2))) & 1u; }

// piece `it` of thread u (0..127) of a staging group: row pair pr, d-octet oct; columns >= D and rows >= nrows are zeros
template <int DP>
__device__ __forceinline__ void hd_stage_load(uint4 (&reg)[HdTile<DP>::NIT][2], const bf16_t* base, int64_t stride, int row0,
                                              int nrows, int D, const int32_t* index, int u) {
  using T = HdTile<DP>;
#pragma unroll
  for (int it = 0; it < T::NIT; ++it) {
    const int idx = u + 128 * it;
    const int pr = idx / T::NOCT, oct = idx % T::NOCT;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int row = row0 + 2 * pr + e;
      const bool ok = idx < 16 * T::NOCT && row < nrows && oct * 8 < D;
      const int src = (ok && index) ? index[row] : row;
      reg[it][e] = hd_load16(base + (int64_t)src * stride + oct * 8, ok);
    }
  }
}
template <int DP>
__device__ __forceinline__ void hd_store_rm(const uint4 (&reg)[HdTile<DP>::NIT][2], char* lds, int u) {
  using T = HdTile<DP>;
#pragma unroll
  for (int it = 0; it < T::NIT; ++it) {
    const int idx = u + 128 * it;
    if (idx >= 16 * T::NOCT) continue;
    const int pr = idx / T::NOCT, oct = idx % T::NOCT;
    *reinterpret_cast<uint4*>(lds + ((2 * pr) * T::RMS + oct * 8) * 2) = reg[it][0];
    *reinterpret_cast<uint4*>(lds + ((2 * pr + 1) * T::RMS + oct * 8) * 2) = reg[it][1];
  }
}
template <int DP>
__device__ __forceinline__ void hd_store_pi(const uint4 (&reg)[HdTile<DP>::NIT][2], char* lds, int u) {
  using T = HdTile<DP>;
#pragma unroll
  for (int it = 0; it < T::NIT; ++it) {
    const int idx = u + 128 * it;
    if (idx >= 16 * T::NOCT) continue;
    const int pr = idx / T::NOCT, oct = idx % T::NOCT;
    const uint32_t a[4] = {reg[it][0].x, reg[it][0].y, reg[it][0].z, reg[it][0].w};   // even row
    const uint32_t b[4] = {reg[it][1].x, reg[it][1].y, reg[it][1].z, reg[it][1].w};   // odd row
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[2 * i] = (a[i] & 0xffffu) | (b[i] << 16);
      o[2 * i + 1] = (a[i] >> 16) | (b[i] & 0xffff0000u);
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(lds) + pr * DP + oct * 8;
    *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(dst + 4) = make_uint4(o[4], o[5], o[6], o[7]);
  }
}
// row-major fragment: tile row `row`, d-slots 16 s + 8 g .. + 7
template <int DP>
__device__ __forceinline__ bf16x8 hd_frag_rm(const char* lds, int row, int s, int g) {
  return *reinterpret_cast<const bf16x8*>(lds + (row * HdTile<DP>::RMS + s * 16 + g * 8) * 2);
}
// transposed fragment from the pair-interleaved image: lane column c (a d value), k-slot j of lane group g = tile row
// hd_acc_row(8 mm + j, g) -- the row of P / dS register 8 mm + j
template <int DP>
__device__ __forceinline__ bf16x8 hd_frag_pi(const char* lds, int c, int mm, int g) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(lds) + (8 * mm + 2 * g) * DP + c;
  union { uint32_t w[4]; bf16x8 v; } u;
  u.w[0] = src[0]; u.w[1] = src[DP]; u.w[2] = src[4 * DP]; u.w[3] = src[5 * DP];
  return u.v;
}
__device__ __forceinline__ bf16x8 hd_pack_frag(const float* p) {
  union { uint32_t w[4]; bf16x8 v; } u;
  u.w[0] = pack2bf(p[0], p[1]); u.w[1] = pack2bf(p[2], p[3]);
  u.w[2] = pack2bf(p[4], p[5]); u.w[3] = pack2bf(p[6], p[7]);
  return u.v;
}
// Q-like operand row fragments (the MFMA B operand): row `row` of a (token, d) matrix, columns >= D zero
template <int DP>
__device__ __forceinline__ void hd_load_row_frags(bf16x8 (&f)[HdTile<DP>::NS], const bf16_t* rowp, bool ok, int D, int g) {
#pragma unroll
  for (int s = 0; s < HdTile<DP>::NS; ++s) {
    const uint4 u = hd_load16(rowp + 16 * s + 8 * g, ok && 16 * s + 8 * g < D);
    f[s] = *reinterpret_cast<const bf16x8*>(&u);
  }
}
// store the transposed accumulators (lane = token row, registers = d = 32 db + 8 rq + 4 g + e) of one token, columns < D only
template <int DP>
__device__ __forceinline__ void hd_store_token(bf16_t* dst, const f32x16 (&acc)[HdTile<DP>::NDB], float mul, int D, int g) {
#pragma unroll
  for (int db = 0; db < HdTile<DP>::NDB; ++db)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int d = 32 * db + 8 * rq + 4 * g;
      if (d < D)
        *reinterpret_cast<uint2*>(dst + d) = make_uint2(pack2bf(acc[db][4 * rq] * mul, acc[db][4 * rq + 1] * mul),
                                                        pack2bf(acc[db][4 * rq + 2] * mul, acc[db][4 * rq + 3] * mul));
    }
}

__device__ __forceinline__ int hd_tile_flag(const HdArgs& p, int qt, int kt) {
  if (qt >= p.nqt || kt >= p.nkt) return 0;
  return p.tile_map ? (int)p.tile_map[qt * p.nkt + kt] : 1;
}

// ====================================================================================================
// forward: one wave = 32 queries, a workgroup = 4 waves = 128 queries sharing the K / V tiles
// ====================================================================================================
template <int DP>
__global__ __launch_bounds__(HD_THREADS) void attn_hd_fwd_kernel(HdArgs p) {
  using T = HdTile<DP>;
  constexpr int BUF = T::RM_BYTES + T::PI_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, g = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qt0 = blockIdx.x * 4;
  const int qt = qt0 + wave;
  const int q = qt * 32 + l31;
  const bool q_ok = q < p.Lq;
  const float scale_log2 = p.scale * HD_LOG2E;

  const bf16_t* qb = p.q + (int64_t)b * p.qsb + (int64_t)h * p.qsh;
  const bf16_t* kb = p.k + (int64_t)b * p.ksb + (int64_t)h * p.ksh;
  const bf16_t* vb = p.v + (int64_t)b * p.vsb + (int64_t)h * p.vsh;

  bf16x8 qf[T::NS];
  hd_load_row_frags<DP>(qf, qb + (int64_t)(q_ok ? q : 0) * p.qst, q_ok, p.D, g);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 oacc[T::NDB];
#pragma unroll
  for (int db = 0; db < T::NDB; ++db) oacc[db] = hd_zero16();
  const int rowid = (b * p.H + h) * p.Lq + q;
  uint32_t rowkey = 0;
  if (p.has_drop) rowkey = drop_rowkey(p.seed_lo, p.seed_hi, (uint32_t)rowid);

  auto blk_need = [&](int kt) -> bool {
    return (hd_tile_flag(p, qt0, kt) | hd_tile_flag(p, qt0 + 1, kt) | hd_tile_flag(p, qt0 + 2, kt) | hd_tile_flag(p, qt0 + 3, kt)) != 0;
  };
  auto next_needed = [&](int kt) -> int {
    while (kt < p.nkt && !blk_need(kt)) ++kt;
    return kt < p.nkt ? kt : -1;
  };
  const bool is_v_loader = t < 128;
  const int u = is_v_loader ? t : t - 128;
  uint4 reg[T::NIT][2];
  auto g_load = [&](int kt) {
    if (is_v_loader) hd_stage_load<DP>(reg, vb, p.vst, kt * 32, p.Lk, p.D, p.key_index, u);
    else hd_stage_load<DP>(reg, kb, p.kst, kt * 32, p.Lk, p.D, p.key_index, u);
  };
  auto l_store = [&](int buf) {
    char* base = smem + buf * BUF;
    if (is_v_loader) hd_store_pi<DP>(reg, base + T::RM_BYTES, u);
    else hd_store_rm<DP>(reg, base, u);
  };

  int kt = next_needed(0);
  if (kt >= 0) { g_load(kt); l_store(0); }
  __syncthreads();
  int cur = 0;
  while (kt >= 0) {
    const int ktn = next_needed(kt + 1);
    if (ktn >= 0) g_load(ktn);
    const int flag = hd_tile_flag(p, qt, kt);
    if (flag != 0) {
      const char* ks = smem + cur * BUF;
      const char* vs = ks + T::RM_BYTES;
      f32x16 sacc = hd_zero16();
#pragma unroll
      for (int s = 0; s < T::NS; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_rm<DP>(ks, l31, s, g), qf[s], sacc, 0, 0, 0);
      const int k0 = kt * 32;
      uint32_t vis = 0xffffffffu;
      if (flag == 2 && q_ok) vis = p.bits_q[q * p.nkt + kt];
      if (k0 + 32 > p.Lk) vis &= hd_low_mask(p.Lk - k0);
      float sv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) sv[r] = sacc[r];
      if (__any(vis != 0xffffffffu)) {
        const uint32_t vg = vis >> (4 * g);
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[r] = hd_vis_bit(vg, r) ? sv[r] : -INFINITY;
      }
      float mt = sv[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mt = fmaxf(mt, sv[r]);
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      // integer running maximum in the log2 domain: every rescale factor is a power of two (the D = 64 kernels' arithmetic)
      const float m_new = fmaxf(m_run, ceilf(mt * scale_log2));
      const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = fast_exp2(m_run - m_safe);
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sv[r] = fast_exp2(fmaf(sv[r], scale_log2, -m_safe)); rs += sv[r]; }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;
      m_run = m_new;
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int db = 0; db < T::NDB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
      }
      if (p.has_drop) {        // the keep test of attention.hip: one hash per (row, tile), one 24-bit multiply-add per element
        const uint32_t tk = drop_tilekey(rowkey, (uint32_t)kt);
        const uint32_t dx = drop_rot(tk, (uint32_t)g);
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[r] = (drop_elem(dx, tk, DVLA_DROP_C(r)) >= p.drop_thr) ? sv[r] : 0.f;
      }
      const bf16x8 pf0 = hd_pack_frag(sv), pf1 = hd_pack_frag(sv + 8);
#pragma unroll
      for (int db = 0; db < T::NDB; ++db) {
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(vs, 32 * db + l31, 0, g), pf0, oacc[db], 0, 0, 0);
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(vs, 32 * db + l31, 1, g), pf1, oacc[db], 0, 0, 0);
      }
    }
    if (ktn >= 0) l_store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    kt = ktn;
  }
  if (q_ok) {
    const float inv_l = l_run > 0.f ? p.inv_keep / l_run : 0.f;     // 1 / keep of the dropout rides on 1 / l
    hd_store_token<DP>(p.o + (int64_t)b * p.osb + (int64_t)q * p.ost + (int64_t)h * p.osh, oacc, inv_l, p.D, g);
    if (p.lse && g == 0) p.lse[rowid] = l_run > 0.f ? (m_run + log2f(l_run)) * HD_LN2 : INFINITY;
  }
}

// ====================================================================================================
// backward: delta[b,h,q] = sum_d dO * O   (8 lanes per row)
// ====================================================================================================
__global__ void attn_hd_delta_kernel(HdArgs p) {
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = gt >> 3;
  const int part = (int)(gt & 7);
  const int64_t nrows = (int64_t)p.B * p.H * p.Lq;
  float s = 0.f;
  if (row < nrows) {
    const int64_t q = row % p.Lq, bh = row / p.Lq, h = bh % p.H, b = bh / p.H;
    const bf16_t* dop = p.dout + b * p.dsb + q * p.dst + h * p.dsh;
    const bf16_t* op = p.o + b * p.osb + q * p.ost + h * p.osh;
    for (int oct = part; oct * 8 < p.D; oct += 8) {
      const uint4 a = *reinterpret_cast<const uint4*>(dop + oct * 8);
      const uint4 c = *reinterpret_cast<const uint4*>(op + oct * 8);
      const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s += bf2f((bf16_t)(aw[i] & 0xffff)) * bf2f((bf16_t)(cw[i] & 0xffff));
        s += bf2f((bf16_t)(aw[i] >> 16)) * bf2f((bf16_t)(cw[i] >> 16));
      }
    }
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  if (row < nrows && part == 0) p.delta[row] = s;
}

// ====================================================================================================
// backward: dQ  (one wave = 32 queries, loop over key tiles; forward orientation)
//   LDS per buffer: K row-major | K pair-interleaved | V row-major
// ====================================================================================================
template <int DP>
__global__ __launch_bounds__(HD_THREADS) void attn_hd_dq_kernel(HdArgs p) {
  using T = HdTile<DP>;
  constexpr int BUF = 2 * T::RM_BYTES + T::PI_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, g = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qt0 = blockIdx.x * 4;
  const int qt = qt0 + wave;
  const int q = qt * 32 + l31;
  const bool q_ok = q < p.Lq;
  const float scale_log2 = p.scale * HD_LOG2E;
  const bf16_t* qb = p.q + (int64_t)b * p.qsb + (int64_t)h * p.qsh;
  const bf16_t* kb = p.k + (int64_t)b * p.ksb + (int64_t)h * p.ksh;
  const bf16_t* vb = p.v + (int64_t)b * p.vsb + (int64_t)h * p.vsh;
  const bf16_t* dob = p.dout + (int64_t)b * p.dsb + (int64_t)h * p.dsh;

  bf16x8 qf[T::NS], dof[T::NS];
  hd_load_row_frags<DP>(qf, qb + (int64_t)(q_ok ? q : 0) * p.qst, q_ok, p.D, g);
  hd_load_row_frags<DP>(dof, dob + (int64_t)(q_ok ? q : 0) * p.dst, q_ok, p.D, g);
  const int rowid = (b * p.H + h) * p.Lq + q;
  const float lse2 = q_ok ? p.lse[rowid] * HD_LOG2E : INFINITY;
  const float dlt = q_ok ? p.delta[rowid] * p.scale : 0.f;       // dS = P (c1 dP' - scale delta), c1 = scale / keep
  const float c1 = p.c1;
  uint32_t rowkey = 0;
  if (p.has_drop) rowkey = drop_rowkey(p.seed_lo, p.seed_hi, (uint32_t)rowid);
  f32x16 dqacc[T::NDB];
#pragma unroll
  for (int db = 0; db < T::NDB; ++db) dqacc[db] = hd_zero16();

  auto blk_need = [&](int kt) -> bool {
    return (hd_tile_flag(p, qt0, kt) | hd_tile_flag(p, qt0 + 1, kt) | hd_tile_flag(p, qt0 + 2, kt) | hd_tile_flag(p, qt0 + 3, kt)) != 0;
  };
  auto next_needed = [&](int kt) -> int {
    while (kt < p.nkt && !blk_need(kt)) ++kt;
    return kt < p.nkt ? kt : -1;
  };
  const bool is_k_loader = t < 128;
  const int u = is_k_loader ? t : t - 128;
  uint4 reg[T::NIT][2];
  auto g_load = [&](int kt) {
    if (is_k_loader) hd_stage_load<DP>(reg, kb, p.kst, kt * 32, p.Lk, p.D, p.key_index, u);
    else hd_stage_load<DP>(reg, vb, p.vst, kt * 32, p.Lk, p.D, p.key_index, u);
  };
  auto l_store = [&](int buf) {
    char* base = smem + buf * BUF;
    if (is_k_loader) { hd_store_rm<DP>(reg, base, u); hd_store_pi<DP>(reg, base + T::RM_BYTES, u); }
    else hd_store_rm<DP>(reg, base + T::RM_BYTES + T::PI_BYTES, u);
  };

  int kt = next_needed(0);
  if (kt >= 0) { g_load(kt); l_store(0); }
  __syncthreads();
  int cur = 0;
  while (kt >= 0) {
    const int ktn = next_needed(kt + 1);
    if (ktn >= 0) g_load(ktn);
    const int flag = hd_tile_flag(p, qt, kt);
    if (flag != 0) {
      const char* k_rm = smem + cur * BUF;
      const char* k_pi = k_rm + T::RM_BYTES;
      const char* v_rm = k_pi + T::PI_BYTES;
      f32x16 sacc = hd_zero16(), dpacc = hd_zero16();
#pragma unroll
      for (int s = 0; s < T::NS; ++s) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_rm<DP>(k_rm, l31, s, g), qf[s], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_rm<DP>(v_rm, l31, s, g), dof[s], dpacc, 0, 0, 0);
      }
      const int k0 = kt * 32;
      uint32_t vis = 0xffffffffu;
      if (flag == 2 && q_ok) vis = p.bits_q[q * p.nkt + kt];
      if (k0 + 32 > p.Lk) vis &= hd_low_mask(p.Lk - k0);
      const uint32_t vg = vis >> (4 * g);
      uint32_t tk = 0u, dx = 0u;
      if (p.has_drop) { tk = drop_tilekey(rowkey, (uint32_t)kt); dx = drop_rot(tk, (uint32_t)g); }
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pr = hd_vis_bit(vg, r) ? fast_exp2(fmaf(sacc[r], scale_log2, -lse2)) : 0.f;
        float dp = dpacc[r];
        if (p.has_drop) dp = (drop_elem(dx, tk, DVLA_DROP_C(r)) >= p.drop_thr) ? dp : 0.f;
        ds[r] = pr * fmaf(dp, c1, -dlt);
      }
      const bf16x8 f0 = hd_pack_frag(ds), f1 = hd_pack_frag(ds + 8);
#pragma unroll
      for (int db = 0; db < T::NDB; ++db) {
        dqacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(k_pi, 32 * db + l31, 0, g), f0, dqacc[db], 0, 0, 0);
        dqacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(k_pi, 32 * db + l31, 1, g), f1, dqacc[db], 0, 0, 0);
      }
    }
    if (ktn >= 0) l_store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    kt = ktn;
  }
  if (q_ok) hd_store_token<DP>(p.dq + (int64_t)b * p.dqsb + (int64_t)q * p.dqst + (int64_t)h * p.dqsh, dqacc, 1.0f, p.D, g);
}

// ====================================================================================================
// backward: dK, dV  (one wave = 32 keys, loop over query tiles)
//   S = Q.K^T orientation: mfma(a = Q fragment (row = query), b = K fragment) -> lane owns one key, registers = 16 queries.
//   dV^T[d][key] += dO^T[d][q] . Pdrop[q][key],  dK^T[d][key] += Q^T[d][q] . dS[q][key]
//   LDS per buffer: Q row-major | Q pair-interleaved | dO row-major | dO pair-interleaved | lse2[32] | scale * delta[32]
//   At DP = 128 the wave's own K / V fragments live in LDS behind the two buffers (each lane re-reads exactly what it wrote):
//   held in registers next to the 2 x 64 accumulators they made the kernel 444 + 188 registers, over the 512 of a lane.
// ====================================================================================================
template <int DP> struct HdDkv {
  static constexpr bool KV_LDS = DP > 96;
  static constexpr int BUF = 2 * HdTile<DP>::RM_BYTES + 2 * HdTile<DP>::PI_BYTES + 2 * 32 * 4;
  static constexpr int KV_BYTES = KV_LDS ? 4 * 2 * HdTile<DP>::RM_BYTES : 0;   // [wave][K, V] row-major tiles
};
template <int DP>
__global__ __launch_bounds__(HD_THREADS) void attn_hd_dkv_kernel(HdArgs p) {
  using T = HdTile<DP>;
  constexpr bool KV_LDS = HdDkv<DP>::KV_LDS;
  constexpr int BUF = HdDkv<DP>::BUF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, g = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int kt0 = blockIdx.x * 4;
  const int ktw = kt0 + wave;
  const int key = ktw * 32 + l31;
  const bool key_ok = key < p.Lk;
  const int key_row = key_ok ? (p.key_index ? p.key_index[key] : key) : 0;
  const float scale_log2 = p.scale * HD_LOG2E;
  const float c1 = p.c1;
  const bf16_t* qb = p.q + (int64_t)b * p.qsb + (int64_t)h * p.qsh;
  const bf16_t* kb = p.k + (int64_t)b * p.ksb + (int64_t)h * p.ksh;
  const bf16_t* vb = p.v + (int64_t)b * p.vsb + (int64_t)h * p.vsh;
  const bf16_t* dob = p.dout + (int64_t)b * p.dsb + (int64_t)h * p.dsh;

  bf16x8 kf[T::NS], vf[T::NS];
  hd_load_row_frags<DP>(kf, kb + (int64_t)key_row * p.kst, key_ok, p.D, g);
  hd_load_row_frags<DP>(vf, vb + (int64_t)key_row * p.vst, key_ok, p.D, g);
  char* kv_lds = smem + 2 * BUF + wave * 2 * T::RM_BYTES;
  if constexpr (KV_LDS) {
#pragma unroll
    for (int s = 0; s < T::NS; ++s) {
      *reinterpret_cast<bf16x8*>(kv_lds + (l31 * T::RMS + s * 16 + g * 8) * 2) = kf[s];
      *reinterpret_cast<bf16x8*>(kv_lds + T::RM_BYTES + (l31 * T::RMS + s * 16 + g * 8) * 2) = vf[s];
    }
  }
  f32x16 dkacc[T::NDB], dvacc[T::NDB];
#pragma unroll
  for (int db = 0; db < T::NDB; ++db) { dkacc[db] = hd_zero16(); dvacc[db] = hd_zero16(); }
  const int bh_row0 = (b * p.H + h) * p.Lq;
  // dropout: this lane's key is position (l31) of key tile ktw -- the register index and lane half it has in the forward layout
  const uint32_t drop_cj = DVLA_DROP_C((l31 & 3) + 4 * (l31 >> 3));
  const uint32_t drop_half = (uint32_t)((l31 >> 2) & 1);

  auto blk_need = [&](int qt) -> bool {
    return (hd_tile_flag(p, qt, kt0) | hd_tile_flag(p, qt, kt0 + 1) | hd_tile_flag(p, qt, kt0 + 2) | hd_tile_flag(p, qt, kt0 + 3)) != 0;
  };
  auto next_needed = [&](int qt) -> int {
    while (qt < p.nqt && !blk_need(qt)) ++qt;
    return qt < p.nqt ? qt : -1;
  };
  const bool is_q_loader = t < 128;
  const int u = is_q_loader ? t : t - 128;
  uint4 reg[T::NIT][2];
  float stat = 0.f;
  auto g_load = [&](int qt) {
    if (is_q_loader) hd_stage_load<DP>(reg, qb, p.qst, qt * 32, p.Lq, p.D, nullptr, u);
    else hd_stage_load<DP>(reg, dob, p.dst, qt * 32, p.Lq, p.D, nullptr, u);
    if (t < 64) {
      const int qq = qt * 32 + (t & 31);
      if (t < 32) stat = qq < p.Lq ? p.lse[bh_row0 + qq] * HD_LOG2E : INFINITY;
      else stat = qq < p.Lq ? p.delta[bh_row0 + qq] * p.scale : 0.f;
    }
  };
  auto l_store = [&](int buf) {
    char* base = smem + buf * BUF + (is_q_loader ? 0 : (T::RM_BYTES + T::PI_BYTES));
    hd_store_rm<DP>(reg, base, u);
    hd_store_pi<DP>(reg, base + T::RM_BYTES, u);
    if (t < 64) reinterpret_cast<float*>(smem + buf * BUF + 2 * T::RM_BYTES + 2 * T::PI_BYTES)[t] = stat;
  };

  int qt = next_needed(0);
  if (qt >= 0) { g_load(qt); l_store(0); }
  __syncthreads();
  int cur = 0;
  while (qt >= 0) {
    const int qtn = next_needed(qt + 1);
    if (qtn >= 0) g_load(qtn);
    const int flag = hd_tile_flag(p, qt, ktw);
    if (flag != 0) {
      const char* q_rm = smem + cur * BUF;
      const char* q_pi = q_rm + T::RM_BYTES;
      const char* do_rm = q_pi + T::PI_BYTES;
      const char* do_pi = do_rm + T::RM_BYTES;
      const float* st = reinterpret_cast<const float*>(do_pi + T::PI_BYTES);
      f32x16 sacc = hd_zero16(), dpacc = hd_zero16();
#pragma unroll
      for (int s = 0; s < T::NS; ++s) {
        const bf16x8 ks = KV_LDS ? hd_frag_rm<DP>(kv_lds, l31, s, g) : kf[s];
        const bf16x8 vs = KV_LDS ? hd_frag_rm<DP>(kv_lds + T::RM_BYTES, l31, s, g) : vf[s];
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_rm<DP>(q_rm, l31, s, g), ks, sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_rm<DP>(do_rm, l31, s, g), vs, dpacc, 0, 0, 0);
      }
      const int q0 = qt * 32;
      uint32_t vis = key_ok ? 0xffffffffu : 0u;  // bit i: query q0+i sees this lane's key
      if (flag == 2 && key_ok) vis = p.bits_k[key * p.nqt + qt];
      const uint32_t vg = vis >> (4 * g);
      float pr[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qr = hd_acc_row(r, g);
        const float lse2 = st[qr], dlt = st[32 + qr];                // q >= Lq: lse2 = +inf -> p = 0
        const float pv = hd_vis_bit(vg, r) ? fast_exp2(fmaf(sacc[r], scale_log2, -lse2)) : 0.f;
        float dp = dpacc[r], pdrop = pv;
        if (p.has_drop) {
          const uint32_t rk = drop_rowkey(p.seed_lo, p.seed_hi, (uint32_t)(bh_row0 + q0 + qr));
          const uint32_t tk = drop_tilekey(rk, (uint32_t)ktw);
          const bool keep = drop_elem(drop_rot(tk, drop_half), tk, drop_cj) >= p.drop_thr;
          dp = keep ? dp : 0.f;                // 1 / keep: in c1 for dS, on the stored dV for P
          pdrop = keep ? pdrop : 0.f;
        }
        ds[r] = pv * fmaf(dp, c1, -dlt);
        pr[r] = pdrop;
      }
      const bf16x8 pf0 = hd_pack_frag(pr), pf1 = hd_pack_frag(pr + 8);
      const bf16x8 sf0 = hd_pack_frag(ds), sf1 = hd_pack_frag(ds + 8);
#pragma unroll
      for (int db = 0; db < T::NDB; ++db) {
        dvacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(do_pi, 32 * db + l31, 0, g), pf0, dvacc[db], 0, 0, 0);
        dvacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(do_pi, 32 * db + l31, 1, g), pf1, dvacc[db], 0, 0, 0);
        dkacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(q_pi, 32 * db + l31, 0, g), sf0, dkacc[db], 0, 0, 0);
        dkacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hd_frag_pi<DP>(q_pi, 32 * db + l31, 1, g), sf1, dkacc[db], 0, 0, 0);
      }
    }
    if (qtn >= 0) l_store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    qt = qtn;
  }
  if (key_ok) {
    hd_store_token<DP>(p.dk + (int64_t)b * p.dksb + (int64_t)key_row * p.dkst + (int64_t)h * p.dksh, dkacc, 1.0f, p.D, g);
    hd_store_token<DP>(p.dv + (int64_t)b * p.dvsb + (int64_t)key_row * p.dvst + (int64_t)h * p.dvsh, dvacc, p.inv_keep, p.D, g);
  }
}

template <int DP> constexpr size_t hd_fwd_smem() { return 2 * (size_t)(HdTile<DP>::RM_BYTES + HdTile<DP>::PI_BYTES); }
template <int DP> constexpr size_t hd_dq_smem() { return 2 * (size_t)(2 * HdTile<DP>::RM_BYTES + HdTile<DP>::PI_BYTES); }
template <int DP> constexpr size_t hd_dkv_smem() { return 2 * (size_t)HdDkv<DP>::BUF + HdDkv<DP>::KV_BYTES; }
static_assert(hd_dkv_smem<128>() <= 160 * 1024 && hd_dkv_smem<96>() <= 160 * 1024, "dK/dV LDS"); 

inline bool hd_supported(int D) { return D >= 8 && D <= 128 && D % 8 == 0 && D != 64; }

int hd_fill(const dvla_attn_params* q, int head_dim, HdArgs& a) {
  if (!q || !q->q || !q->k || !q->v || !q->o) return DVLA_ERR_ARG;
  if (!hd_supported(head_dim)) return DVLA_ERR_UNSUPPORTED;
  if (q->B <= 0 || q->H <= 0 || q->Lq <= 0 || q->Lk <= 0) return DVLA_ERR_ARG;
  if (q->dropout_p < 0.f || q->dropout_p >= 1.f || !(q->scale > 0.f)) return DVLA_ERR_ARG;
  if ((int64_t)q->B * q->H * q->Lq >= (1LL << 31) || q->B > 65535 || q->H > 65535) return DVLA_ERR_UNSUPPORTED;
  if (!dvla_aligned(q->q, q->q_stride_b, q->q_stride_t, q->q_stride_h, 16) || !dvla_aligned(q->k, q->k_stride_b, q->k_stride_t, q->k_stride_h, 16) ||
      !dvla_aligned(q->v, q->v_stride_b, q->v_stride_t, q->v_stride_h, 16) || !dvla_aligned(q->o, q->o_stride_b, q->o_stride_t, q->o_stride_h, 8))
    return DVLA_ERR_UNSUPPORTED;
  if (q->tile_map && !q->mask_bits_q) return DVLA_ERR_ARG;
  a.q = (const bf16_t*)q->q; a.k = (const bf16_t*)q->k; a.v = (const bf16_t*)q->v; a.o = (bf16_t*)q->o;
  a.qsb = q->q_stride_b; a.qst = q->q_stride_t; a.qsh = q->q_stride_h;
  a.ksb = q->k_stride_b; a.kst = q->k_stride_t; a.ksh = q->k_stride_h;
  a.vsb = q->v_stride_b; a.vst = q->v_stride_t; a.vsh = q->v_stride_h;
  a.osb = q->o_stride_b; a.ost = q->o_stride_t; a.osh = q->o_stride_h;
  a.B = q->B; a.H = q->H; a.Lq = q->Lq; a.Lk = q->Lk; a.D = head_dim;
  a.scale = q->scale;
  a.key_index = q->key_index;
  a.bits_q = q->mask_bits_q; a.bits_k = q->mask_bits_k;
  a.tile_map = q->tile_map;
  a.nqt = (q->Lq + 31) / 32; a.nkt = (q->Lk + 31) / 32;
  a.has_drop = q->dropout_p > 0.f;
  a.inv_keep = a.has_drop ? 1.0f / (1.0f - q->dropout_p) : 1.0f;
  a.c1 = q->scale * a.inv_keep;
  {
    double thr = (double)q->dropout_p * 4294967296.0;
    a.drop_thr = thr >= 4294967295.0 ? 4294967295u : (uint32_t)thr;
  }
  a.seed_lo = q->seed_lo; a.seed_hi = q->seed_hi;
  a.lse = q->lse;
  a.dout = (const bf16_t*)q->dout; a.dsb = q->do_stride_b; a.dst = q->do_stride_t; a.dsh = q->do_stride_h;
  a.delta = q->delta;
  a.dq = (bf16_t*)q->dq; a.dk = (bf16_t*)q->dk; a.dv = (bf16_t*)q->dv;
  a.dqsb = q->dq_stride_b; a.dqst = q->dq_stride_t; a.dqsh = q->dq_stride_h;
  a.dksb = q->dk_stride_b; a.dkst = q->dk_stride_t; a.dksh = q->dk_stride_h;
  a.dvsb = q->dv_stride_b; a.dvst = q->dv_stride_t; a.dvsh = q->dv_stride_h;
  return DVLA_OK;
}

template <int DP>
int hd_launch_fwd(const HdArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.nqt + 3) / 4), (unsigned)a.H, (unsigned)a.B);
  (void)dvla_allow_lds(attn_hd_fwd_kernel<DP>, hd_fwd_smem<DP>());
  hipLaunchKernelGGL(attn_hd_fwd_kernel<DP>, grid, dim3(HD_THREADS), hd_fwd_smem<DP>(), stream, a);
  return dvla_check_launch();
}

template <int DP>
int hd_launch_bwd(const HdArgs& a, hipStream_t stream) {
  const int64_t nrows = (int64_t)a.B * a.H * a.Lq;
  hipLaunchKernelGGL(attn_hd_delta_kernel, dim3((unsigned)((nrows * 8 + 255) / 256)), dim3(256), 0, stream, a);
  int rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  (void)dvla_allow_lds(attn_hd_dq_kernel<DP>, hd_dq_smem<DP>());
  (void)dvla_allow_lds(attn_hd_dkv_kernel<DP>, hd_dkv_smem<DP>());
  const dim3 grid_dq((unsigned)((a.nqt + 3) / 4), (unsigned)a.H, (unsigned)a.B);
  hipLaunchKernelGGL(attn_hd_dq_kernel<DP>, grid_dq, dim3(HD_THREADS), hd_dq_smem<DP>(), stream, a);
  rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  const dim3 grid_dkv((unsigned)((a.nkt + 3) / 4), (unsigned)a.H, (unsigned)a.B);
  hipLaunchKernelGGL(attn_hd_dkv_kernel<DP>, grid_dkv, dim3(HD_THREADS), hd_dkv_smem<DP>(), stream, a);
  return dvla_check_launch();
}

}  // namespace

extern "C" int dvla_attn_hd_fwd(const dvla_attn_params* q, int32_t head_dim, void* stream_) {
  HdArgs a;
  const int rc = hd_fill(q, head_dim, a);
  if (rc != DVLA_OK) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  switch ((head_dim + 31) / 32) {
    case 1: return hd_launch_fwd<32>(a, stream);
    case 2: return hd_launch_fwd<64>(a, stream);
    case 3: return hd_launch_fwd<96>(a, stream);
    default: return hd_launch_fwd<128>(a, stream);
  }
}

extern "C" int dvla_attn_hd_bwd(const dvla_attn_params* q, int32_t head_dim, void* stream_) {
  HdArgs a;
  int rc = hd_fill(q, head_dim, a);
  if (rc != DVLA_OK) return rc;
  if (!q->dout || !q->lse || !q->delta || !q->dq || !q->dk || !q->dv) return DVLA_ERR_ARG;
  if (q->tile_map && !q->mask_bits_k) return DVLA_ERR_ARG;
  if (!dvla_aligned(q->dout, q->do_stride_b, q->do_stride_t, q->do_stride_h, 16) || !dvla_aligned(q->o, q->o_stride_b, q->o_stride_t, q->o_stride_h, 16) ||
      !dvla_aligned(q->dq, q->dq_stride_b, q->dq_stride_t, q->dq_stride_h, 8) || !dvla_aligned(q->dk, q->dk_stride_b, q->dk_stride_t, q->dk_stride_h, 8) ||
      !dvla_aligned(q->dv, q->dv_stride_b, q->dv_stride_t, q->dv_stride_h, 8))
    return DVLA_ERR_UNSUPPORTED;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  switch ((head_dim + 31) / 32) {
    case 1: return hd_launch_bwd<32>(a, stream);
    case 2: return hd_launch_bwd<64>(a, stream);
    case 3: return hd_launch_bwd<96>(a, stream);
    default: return hd_launch_bwd<128>(a, stream);
  }
}
