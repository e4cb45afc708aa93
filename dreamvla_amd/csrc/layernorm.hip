// layernorm.hip -- LayerNorm forward / backward for gfx950, HBM-bound.
//
// One wave (64 lanes) owns one row; a 256-thread block = 4 rows per pass, grid-strided.  A lane holds
// its slice of the row in registers as 16-byte vectors (8 bf16): vector index = lane + 64*i, so a wave
// reads/writes 1 KiB contiguous per instruction.  Statistics are two-pass in registers (mean, then
// sum (x-mean)^2) in fp32 and reduced with wave shuffles; nothing goes through LDS in forward.
// Algorithmic bytes: forward 2*rows*cols*2 B (+8 B/row of stats); backward 3*rows*cols*2 B (4 with the residual gradient).
// A wave keeps TWO rows in flight (the next row's vectors are requested before the current row is reduced).
//
// Backward: a lane's column set is the same for every row, so per-lane dgamma/dbeta partial sums stay
// in registers across the block's rows, are combined across the 4 waves through LDS at the end, and
// written to partial[block][2][cols]; a second tiny kernel reduces over blocks (deterministic).
#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_MAX_VPL = 4;          // vectors per lane -> cols <= 64*8*4 = 2048
constexpr int LN_BWD_BLOCKS = 768;     // persistent grid for backward (partial rows)

__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  f[0] = bf2f((bf16_t)(u.x & 0xffff)); f[1] = bf2f((bf16_t)(u.x >> 16));
  f[2] = bf2f((bf16_t)(u.y & 0xffff)); f[3] = bf2f((bf16_t)(u.y >> 16));
  f[4] = bf2f((bf16_t)(u.z & 0xffff)); f[5] = bf2f((bf16_t)(u.z >> 16));
  f[6] = bf2f((bf16_t)(u.w & 0xffff)); f[7] = bf2f((bf16_t)(u.w >> 16));
}
// eight consecutive parameters (vector index vi) as fp32; parameter tensors are 16-B aligned (checked by the host)
__device__ __forceinline__ void load_param8(const void* p, int f32, int vi, float (&f)[8]) {
  if (f32) {
    const float4 a = reinterpret_cast<const float4*>(p)[2 * vi], b = reinterpret_cast<const float4*>(p)[2 * vi + 1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    unpack8(reinterpret_cast<const uint4*>(p)[vi], f);
  }
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
}

// Row groups (round 6, dvla_layernorm_*_rows): logical row r of the normalised matrix is row (r / grp) * gstride + goff + r % grp of the
// buffer -- the last `grp` tokens of every `gstride`-token sequence, contiguous inside a sequence, `goff` rows apart across
// sequences.  grp == 0: the identity (the plain entry points).  One 32-bit division per row and wave, next to 2-4 KiB of traffic.
__device__ __forceinline__ int64_t ln_buf_row(int64_t r, int grp, int gstride, int goff) {
  if (grp == 0) return r;
  const uint32_t g = (uint32_t)r / (uint32_t)grp;
  return (int64_t)g * gstride + goff + (int64_t)((uint32_t)r - g * (uint32_t)grp);
}

// cols % 8 == 0 required (vector path); VPL = ceil(cols / 512)
template <int VPL>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(const bf16_t* __restrict__ x, const void* __restrict__ gamma,
                                                            const void* __restrict__ beta, int pf32,
                                                            bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                            float* __restrict__ rstd_out, int64_t rows, int cols,
                                                            float eps, int grp, int gstride, int goff, int omap) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = cols >> 3;
  const float inv_n = 1.0f / (float)cols;
  // a lane's columns are the same for every row: gamma / beta live in registers for the whole kernel
  float gam[VPL][8], bet[VPL][8];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + 64 * i;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gam[i][e] = 1.0f; bet[i][e] = 0.0f; }
    if (vi < nvec) {
      if (gamma) load_param8(gamma, pf32, vi, gam[i]);
      if (beta) load_param8(beta, pf32, vi, bet[i]);
    }
  }
  // Software prefetch: the raw vectors of the wave's NEXT row are requested before the current row is reduced, so a wave
  // always has two rows (2-4 KiB) in flight.  One row per wave and iteration left the memory pipe idle during the two dependent
  // wave reductions and the store: 3.9 TB/s on a >256-MiB working set, 2.9 TB/s at the trunk's 20832 rows, where a wave owns
  // only 2-3 rows and pays one full load latency for each (profiles/r02_pmc_ln_*.txt, round-2 VERDICT).
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + wave;
  uint4 raw[VPL], nxt[VPL];
  auto load_row = [&](int64_t r, uint4 (&dst)[VPL]) {
    const uint4* xr = reinterpret_cast<const uint4*>(x + (omap ? r : ln_buf_row(r, grp, gstride, goff)) * cols);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = lane + 64 * i;
      dst[i] = vi < nvec ? xr[vi] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  if (row < rows) load_row(row, raw);
  for (; row < rows; row += stride) {
    if (row + stride < rows) load_row(row + stride, nxt);
    float v[VPL][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      unpack8(raw[i], v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[i][e];
    }
    const float mean = wave_sum(s) * inv_n;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (lane + 64 * i < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; ss += d * d; }
      }
    }
    const float var = wave_sum(ss) * inv_n;
    const float rstd = rsqrtf(var + eps);
    if (lane == 0) {
      if (mean_out) mean_out[row] = mean;
      if (rstd_out) rstd_out[row] = rstd;
    }
    uint4* yr = reinterpret_cast<uint4*>(y + (omap ? ln_buf_row(row, grp, gstride, goff) : row) * cols);     // omap: the OUTPUT lives in the buffer's rows
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = lane + 64 * i;
      if (vi < nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gam[i][e] + bet[i][e];
        yr[vi] = pack8(o);
      }
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) raw[i] = nxt[i];
  }
}

template <int VPL>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                            const void* __restrict__ gamma, int pf32,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            bf16_t* __restrict__ dx, float* __restrict__ partial,
                                                            int64_t rows, int cols, const bf16_t* __restrict__ dres,
                                                            int grp, int gstride, int goff, int omap) {
  __shared__ float red[4][64 * 8];  // one vector-slot at a time: [wave][lane*8+e]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = cols >> 3;
  const float inv_n = 1.0f / (float)cols;
  float gam[VPL][8], dg[VPL][8], db[VPL][8];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + 64 * i;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gam[i][e] = 1.0f; dg[i][e] = 0.f; db[i][e] = 0.f; }
    if (gamma && vi < nvec) load_param8(gamma, pf32, vi, gam[i]);
  }
  // the same two-rows-in-flight prefetch as the forward kernel, over all the row's inputs: x, dy, the residual-stream gradient
  // (it used to be requested only AFTER the two reductions: a third serial memory round trip per row) and mean / rstd
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + wave;
  uint4 rx[VPL], rg[VPL], rr[VPL], nx[VPL], ng[VPL], nr[VPL];
  float mu = 0.f, rs = 0.f, nmu = 0.f, nrs = 0.f;
  auto load_row = [&](int64_t r, uint4 (&dx_)[VPL], uint4 (&dg_)[VPL], uint4 (&dr_)[VPL], float& m_, float& r_) {
    // row groups: x and dx in the buffer's rows (omap == 0), or dy in the buffer's rows and x / dx contiguous (omap != 0)
    const uint4* xr = reinterpret_cast<const uint4*>(x + (omap ? r : ln_buf_row(r, grp, gstride, goff)) * cols);
    const uint4* gr = reinterpret_cast<const uint4*>(dy + (omap ? ln_buf_row(r, grp, gstride, goff) : r) * cols);
    const uint4* sr = dres ? reinterpret_cast<const uint4*>(dres + r * cols) : nullptr;
    m_ = mean[r]; r_ = rstd[r];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = lane + 64 * i;
      const bool ok = vi < nvec;
      dx_[i] = ok ? xr[vi] : make_uint4(0u, 0u, 0u, 0u);
      dg_[i] = ok ? gr[vi] : make_uint4(0u, 0u, 0u, 0u);
      dr_[i] = (ok && sr) ? sr[vi] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  if (row < rows) load_row(row, rx, rg, rr, mu, rs);
  for (; row < rows; row += stride) {
    if (row + stride < rows) load_row(row + stride, nx, ng, nr, nmu, nrs);
    float xh[VPL][8], gy[VPL][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = lane + 64 * i;
      if (vi < nvec) {
        float xv[8], dv[8];
        unpack8(rx[i], xv);
        unpack8(rg[i], dv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[i][e] = (xv[e] - mu) * rs;
          gy[i][e] = dv[e] * gam[i][e];
          s1 += gy[i][e];
          s2 += gy[i][e] * xh[i][e];
          dg[i][e] += dv[e] * xh[i][e];
          db[i][e] += dv[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { xh[i][e] = 0.f; gy[i][e] = 0.f; }
      }
    }
    if (dx) {     // (dx == nullptr, round 6: the input needs no gradient -- the resampler's norm_media over the frozen ViT's patch
      // tokens -- only the parameter gradients are wanted: no row reductions, no 135-MB store)
    s1 = wave_sum(s1) * inv_n;
    s2 = wave_sum(s2) * inv_n;
    uint4* dr = reinterpret_cast<uint4*>(dx + (omap ? row : ln_buf_row(row, grp, gstride, goff)) * cols);
    if (grp != 0 && !omap && (uint32_t)row % (uint32_t)grp == 0u) {
      // row groups: dx is the gradient of the WHOLE buffer -- the rows of this sequence outside the group get zeros, written by
      // the wave that owns the group's first row
      const int64_t base = (int64_t)((uint32_t)row / (uint32_t)grp) * gstride;
      for (int j = 0; j < gstride; ++j) {
        if (j >= goff && j < goff + grp) continue;
        uint4* zr = reinterpret_cast<uint4*>(dx + (base + j) * cols);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int vi = lane + 64 * i;
          if (vi < nvec) zr[vi] = make_uint4(0u, 0u, 0u, 0u);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vi = lane + 64 * i;
      if (vi < nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rs * (gy[i][e] - s1 - xh[i][e] * s2);
        if (dres) {   // gradient of the residual stream that bypassed this LayerNorm: dx = dres + LN'(dy), one rounding
          float a[8];
          unpack8(rr[i], a);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] += a[e];
        }
        dr[vi] = pack8(o);
      }
    }
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) { rx[i] = nx[i]; rg[i] = ng[i]; rr[i] = nr[i]; }
    mu = nmu; rs = nrs;
  }
  if (partial) {
    // combine the 4 waves' register partials and write partial[block][0|1][cols]
    float* pg = partial + (int64_t)blockIdx.x * 2 * cols;
    float* pb = pg + cols;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      for (int which = 0; which < 2; ++which) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = which ? db[i][e] : dg[i][e];
        __syncthreads();
        // 256 threads sum 512 slots x 4 waves
        for (int sidx = threadIdx.x; sidx < 512; sidx += LN_THREADS) {
          const float tot = red[0][sidx] + red[1][sidx] + red[2][sidx] + red[3][sidx];
          const int col = (64 * i) * 8 + sidx;  // slot sidx = lane*8+e  -> column (lane + 64 i)*8 + e
          if (col < cols) (which ? pb : pg)[col] = tot;
        }
      }
    }
  }
}

// out[c] = sum over blocks of partial[b][which][c]; 16 columns x 16 interleaved block subsets per workgroup
// (deterministic; a thread adds nblocks / 16 partial rows with 4 loads in flight, then a 16-way LDS reduction)
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ partial, void* __restrict__ dgamma,
                                                            void* __restrict__ dbeta, int grad_bf16, int nblocks, int cols) {
  __shared__ float red[2][16][16];
  const int cl = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float sg = 0.f, sb = 0.f;
  if (c < cols)
#pragma unroll 4
    for (int b = part; b < nblocks; b += 16) {
      sg += partial[(int64_t)b * 2 * cols + c];
      sb += partial[(int64_t)b * 2 * cols + cols + c];
    }
  red[0][part][cl] = sg;
  red[1][part][cl] = sb;
  __syncthreads();
  if (part == 0 && c < cols) {
    float tg = 0.f, tb = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) { tg += red[0][q][cl]; tb += red[1][q][cl]; }
    if (grad_bf16) {   // parameter gradients in the parameters' dtype: no cast kernels behind this one
      if (dgamma) reinterpret_cast<bf16_t*>(dgamma)[c] = f2bf(tg);
      if (dbeta) reinterpret_cast<bf16_t*>(dbeta)[c] = f2bf(tb);
    } else {
      if (dgamma) reinterpret_cast<float*>(dgamma)[c] = tg;
      if (dbeta) reinterpret_cast<float*>(dbeta)[c] = tb;
    }
  }
}

int fwd_blocks(int64_t rows) {
  int64_t b = (rows + 3) / 4;
  if (b > 2048) b = 2048;   // 8 workgroups per CU; each wave keeps gamma / beta in registers over its ~rows/8192 rows
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int64_t dvla_layernorm_bwd_partial_rows(void) { return LN_BWD_BLOCKS; }

static bool ln_groups_ok(int64_t rows, int32_t grp, int32_t gstride, int32_t goff) {
  if (grp == 0) return gstride == 0 && goff == 0;
  return grp > 0 && goff >= 0 && gstride >= goff + grp && rows % grp == 0 && rows < (1ll << 31) && (rows / grp) * (int64_t)gstride < (1ll << 40);
}

extern "C" int dvla_layernorm_fwd_rows(const void* x, const void* gamma, const void* beta, int32_t param_dtype, void* y,
                                       float* mean, float* rstd, int64_t rows, int64_t cols, float eps,
                                       int32_t grp, int32_t gstride, int32_t goff, int32_t map_output, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (map_output && grp == 0) return DVLA_ERR_ARG;
  if (!x || !y || rows < 0 || cols <= 0) return DVLA_ERR_ARG;
  if (!ln_groups_ok(rows, grp, gstride, goff)) return DVLA_ERR_ARG;
  if (rows == 0) return DVLA_OK;
  if (cols % 8 != 0 || cols > 64 * 8 * LN_MAX_VPL) return DVLA_ERR_UNSUPPORTED;
  if (((reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta)) & 15) != 0) return DVLA_ERR_UNSUPPORTED;   // parameters are read as 16-B vectors
  const int vpl = (int)((cols / 8 + 63) / 64);
  const int pf32 = (param_dtype == DVLA_DT_F32);
  dim3 grid(fwd_blocks(rows)), block(LN_THREADS);
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x);
  bf16_t* yp = reinterpret_cast<bf16_t*>(y);
  switch (vpl) {
    case 1: hipLaunchKernelGGL(ln_fwd_kernel<1>, grid, block, 0, stream, xp, gamma, beta, pf32, yp, mean, rstd, rows, (int)cols, eps, grp, gstride, goff, map_output ? 1 : 0); break;
    case 2: hipLaunchKernelGGL(ln_fwd_kernel<2>, grid, block, 0, stream, xp, gamma, beta, pf32, yp, mean, rstd, rows, (int)cols, eps, grp, gstride, goff, map_output ? 1 : 0); break;
    case 3: hipLaunchKernelGGL(ln_fwd_kernel<3>, grid, block, 0, stream, xp, gamma, beta, pf32, yp, mean, rstd, rows, (int)cols, eps, grp, gstride, goff, map_output ? 1 : 0); break;
    default: hipLaunchKernelGGL(ln_fwd_kernel<4>, grid, block, 0, stream, xp, gamma, beta, pf32, yp, mean, rstd, rows, (int)cols, eps, grp, gstride, goff, map_output ? 1 : 0); break;
  }
  return dvla_check_launch();
}

static int ln_bwd_launch(const void* dy, const void* x, const void* gamma, int32_t param_dtype, const float* mean, const float* rstd,
                         const void* dres, void* dx, void* dgamma, void* dbeta, int32_t grad_dtype, float* partial, int64_t rows,
                         int64_t cols, int32_t grp, int32_t gstride, int32_t goff, int32_t map_output, void* stream_);

extern "C" int dvla_layernorm_bwd_add(const void* dy, const void* x, const void* gamma, int32_t param_dtype,
                                      const float* mean, const float* rstd, const void* dres, void* dx, void* dgamma,
                                      void* dbeta, int32_t grad_dtype, float* partial, int64_t rows, int64_t cols,
                                      void* stream_) {
  return ln_bwd_launch(dy, x, gamma, param_dtype, mean, rstd, dres, dx, dgamma, dbeta, grad_dtype, partial, rows, cols, 0, 0, 0, 0, stream_);
}

extern "C" int dvla_layernorm_bwd_rows(const void* dy, const void* x, const void* gamma, int32_t param_dtype,
                                       const float* mean, const float* rstd, void* dx, void* dgamma, void* dbeta,
                                       int32_t grad_dtype, float* partial, int64_t rows, int64_t cols,
                                       int32_t grp, int32_t gstride, int32_t goff, int32_t map_output, void* stream_) {
  if (grp <= 0 || (!dx && !map_output)) return DVLA_ERR_ARG;       // (the plain entry points are the identity case; without map_output the
                                                                   // buffer's gradient is the point; with it dx == NULL = parameter gradients only)
  return ln_bwd_launch(dy, x, gamma, param_dtype, mean, rstd, nullptr, dx, dgamma, dbeta, grad_dtype, partial, rows, cols, grp, gstride, goff,
                       map_output, stream_);
}

static int ln_bwd_launch(const void* dy, const void* x, const void* gamma, int32_t param_dtype, const float* mean, const float* rstd,
                         const void* dres, void* dx, void* dgamma, void* dbeta, int32_t grad_dtype, float* partial, int64_t rows,
                         int64_t cols, int32_t grp, int32_t gstride, int32_t goff, int32_t map_output, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!ln_groups_ok(rows, grp, gstride, goff) || (map_output && grp == 0)) return DVLA_ERR_ARG;
  if (grad_dtype != DVLA_DT_F32 && grad_dtype != DVLA_DT_BF16) return DVLA_ERR_ARG;
  const bf16_t* drp = reinterpret_cast<const bf16_t*>(dres);
  if ((reinterpret_cast<uintptr_t>(dres) & 15) != 0) return DVLA_ERR_UNSUPPORTED;
  if (!dy || !x || !mean || !rstd || rows < 0 || cols <= 0) return DVLA_ERR_ARG;
  if (!dx && (dres || !(dgamma || dbeta))) return DVLA_ERR_ARG;      // dx == NULL: parameter gradients only (nothing to do otherwise)
  if ((dgamma || dbeta) && !partial) return DVLA_ERR_ARG;
  if (rows == 0) return DVLA_OK;
  if (cols % 8 != 0 || cols > 64 * 8 * LN_MAX_VPL) return DVLA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(gamma) & 15) != 0) return DVLA_ERR_UNSUPPORTED;   // parameters are read as 16-B vectors
  const int vpl = (int)((cols / 8 + 63) / 64);
  const int pf32 = (param_dtype == DVLA_DT_F32);
  int64_t nb = (rows + 3) / 4;
  if (nb > LN_BWD_BLOCKS) nb = LN_BWD_BLOCKS;
  dim3 grid((unsigned)nb), block(LN_THREADS);
  float* part = (dgamma || dbeta) ? partial : nullptr;
  const bf16_t* dyp = reinterpret_cast<const bf16_t*>(dy);
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x);
  bf16_t* dxp = reinterpret_cast<bf16_t*>(dx);
  switch (vpl) {
    case 1: hipLaunchKernelGGL(ln_bwd_kernel<1>, grid, block, 0, stream, dyp, xp, gamma, pf32, mean, rstd, dxp, part, rows, (int)cols, drp, grp, gstride, goff, map_output ? 1 : 0); break;
    case 2: hipLaunchKernelGGL(ln_bwd_kernel<2>, grid, block, 0, stream, dyp, xp, gamma, pf32, mean, rstd, dxp, part, rows, (int)cols, drp, grp, gstride, goff, map_output ? 1 : 0); break;
    case 3: hipLaunchKernelGGL(ln_bwd_kernel<3>, grid, block, 0, stream, dyp, xp, gamma, pf32, mean, rstd, dxp, part, rows, (int)cols, drp, grp, gstride, goff, map_output ? 1 : 0); break;
    default: hipLaunchKernelGGL(ln_bwd_kernel<4>, grid, block, 0, stream, dyp, xp, gamma, pf32, mean, rstd, dxp, part, rows, (int)cols, drp, grp, gstride, goff, map_output ? 1 : 0); break;
  }
  int rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  if (part) {
    hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((unsigned)((cols + 15) / 16)), dim3(256), 0, stream, part, dgamma,
                       dbeta, grad_dtype == DVLA_DT_BF16 ? 1 : 0, (int)nb, (int)cols);
    rc = dvla_check_launch();
  }
  return rc;
}
