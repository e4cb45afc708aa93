// mae.hip -- the MAE-specific data movement and loss of MaskedAutoencoderViT (models/vit_mae.py:129-256), each one pass:
//   mask      : random_masking + the encoder's cls concat (vit_mae.py:157-199).  Per sample, the stable ascending order of the
//               noise row is computed in LDS (rank of element i = #{j : key_j < key_i or (key_j == key_i and j < i)}), which
//               gives ids_restore, the mask and the gathered token rows [cls ; x[ids_shuffle[:len_keep]]] in the same launch.
//   unshuffle : the decoder's mask-token cat + gather by ids_restore + cls cat + decoder_pos_embed add (vit_mae.py:213-219).
//               Backward gathers the kept rows' gradient and sums the removed rows into d mask_token (two-stage, fixed order).
//   loss      : forward_loss fused with patchify (vit_mae.py:129-141,234-250): one wave per patch, the target read straight
//               from the image in 'nchpwq->nhwpqc' order, optional per-patch normalisation (unbiased variance).
// Deterministic: no float atomics anywhere; partial sums are reduced in a fixed order by a second kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dvla.h"
#include "common.h"

namespace {

constexpr int MAE_THREADS = 256;
constexpr int MAE_MAX_L = 1024;          // tokens per sample held in LDS (224^2 / 14^2 = 256; 448^2 / 14^2 = 1024)
constexpr int ROWS_PER_BLOCK = 8;        // token rows per workgroup of the copy kernels
constexpr int UNSHUFFLE_SLICES = 4;      // workgroups per sample in the un-shuffle backward (partial rows per sample)
constexpr int LOSS_MAX_BLOCKS = 2048;
constexpr int LOSS_PER_LANE = 12;        // P = 3 p^2 <= 768 elements per patch, 64 lanes

// total order of fp32 values as torch sorts them: -0 == +0, every NaN after +inf (equal to each other)
__device__ __forceinline__ uint32_t sort_key(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.f) v = 0.f;
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ uint4 add8(const uint4& a, const uint4& b) {
  const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
  uint32_t r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lo = bf2f((bf16_t)(x[k] & 0xffff)) + bf2f((bf16_t)(y[k] & 0xffff));
    const float hi = bf2f((bf16_t)(x[k] >> 16)) + bf2f((bf16_t)(y[k] >> 16));
    r[k] = pack2bf(lo, hi);
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}

__device__ __forceinline__ void acc8(float (&s)[8], const uint4& u) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) { s[2 * k] += bf2f((bf16_t)(w[k] & 0xffff)); s[2 * k + 1] += bf2f((bf16_t)(w[k] >> 16)); }
}

// ---------------------------------------------------------------------------------------------------------------------
// masking: one workgroup per sample
__global__ __launch_bounds__(MAE_THREADS) void mae_mask_fwd_kernel(const float* __restrict__ noise, const uint4* __restrict__ x,
                                                                   const uint4* __restrict__ cls_row, int L, int nv, int len_keep,
                                                                   int64_t* __restrict__ ids_restore, float* __restrict__ mask,
                                                                   uint4* __restrict__ out) {
  __shared__ uint32_t key[MAE_MAX_L];
  __shared__ int order[MAE_MAX_L];
  const int64_t n = blockIdx.x;
  for (int i = threadIdx.x; i < L; i += MAE_THREADS) key[i] = sort_key(noise[n * L + i]);
  __syncthreads();
  for (int i = threadIdx.x; i < L; i += MAE_THREADS) {
    const uint32_t k = key[i];
    int rank = 0;
    for (int j = 0; j < L; ++j) {
      const uint32_t u = key[j];
      rank += (u < k) | ((u == k) & (j < i));
    }
    order[rank] = i;                       // the ranks are a permutation of [0, L): every slot is written once
    ids_restore[n * L + i] = rank;
    mask[n * L + i] = rank >= len_keep ? 1.f : 0.f;
  }
  __syncthreads();
  const int c = cls_row ? 1 : 0;
  const int rows = c + len_keep;
  const uint4* xs = x + n * L * nv;
  uint4* o = out + n * rows * nv;
  for (int t = threadIdx.x; t < rows * nv; t += MAE_THREADS) {
    const int r = t / nv, v = t - r * nv;
    o[t] = r < c ? cls_row[v] : xs[(int64_t)order[r - c] * nv + v];
  }
}

// grid (row blocks of ROWS_PER_BLOCK, N): no 64-bit index division on the copy path
__global__ __launch_bounds__(MAE_THREADS) void mae_mask_bwd_kernel(const int64_t* __restrict__ ids_restore, const uint4* __restrict__ dout,
                                                                   int c, int L, int nv, int len_keep, uint4* __restrict__ dx) {
  const int64_t n = blockIdx.y;
  const int l0 = blockIdx.x * ROWS_PER_BLOCK;
  const int rows = min(ROWS_PER_BLOCK, L - l0);
  for (int t = threadIdx.x; t < rows * nv; t += MAE_THREADS) {
    const int rr = t / nv, v = t - rr * nv;
    const int64_t row = n * L + l0 + rr;
    const int64_t r = ids_restore[row];
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if (r >= 0 && r < len_keep) val = dout[(n * (c + len_keep) + c + r) * nv + v];
    dx[row * nv + v] = val;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// decoder un-shuffle
__global__ __launch_bounds__(MAE_THREADS) void mae_unshuffle_fwd_kernel(const uint4* __restrict__ y, const uint4* __restrict__ mask_token,
                                                                        const int64_t* __restrict__ ids_restore,
                                                                        const uint4* __restrict__ pos, int L, int nv, int len_keep,
                                                                        uint4* __restrict__ out) {
  const int64_t n = blockIdx.y;
  const int j0 = blockIdx.x * ROWS_PER_BLOCK;
  const int rows = min(ROWS_PER_BLOCK, L + 1 - j0);
  const uint4* yn = y + n * (1 + len_keep) * nv;
  for (int t = threadIdx.x; t < rows * nv; t += MAE_THREADS) {
    const int jj = t / nv, v = t - jj * nv;
    const int j = j0 + jj;
    uint4 a;
    if (j == 0) {
      a = yn[v];
    } else {
      const int64_t r = ids_restore[n * L + j - 1];
      a = (r >= 0 && r < len_keep) ? yn[(1 + r) * nv + v] : mask_token[v];
    }
    out[(n * (L + 1) + j) * nv + v] = add8(a, pos[(int64_t)j * nv + v]);
  }
}

// grid (UNSHUFFLE_SLICES, N): workgroup (s, n) gathers slice s of sample n's dy rows and sums the removed rows among positions
// l = s, s + UNSHUFFLE_SLICES, ... into partial[n * UNSHUFFLE_SLICES + s, :] (fixed order)
__global__ __launch_bounds__(MAE_THREADS) void mae_unshuffle_bwd_kernel(const uint4* __restrict__ dout, const int64_t* __restrict__ ids_restore,
                                                                        int L, int nv, int len_keep, uint4* __restrict__ dy,
                                                                        float* __restrict__ partial) {
  __shared__ int src[MAE_MAX_L];         // kept rank r -> position l (or -1)
  __shared__ int rk[MAE_MAX_L];          // position l -> kept rank, or -1 for a removed position
  __shared__ float red[MAE_THREADS * 8];
  const int64_t n = blockIdx.y;
  const int sl = blockIdx.x;
  const int D = nv * 8;
  for (int r = threadIdx.x; r < len_keep; r += MAE_THREADS) src[r] = -1;
  __syncthreads();
  for (int l = threadIdx.x; l < L; l += MAE_THREADS) {
    const int64_t r = ids_restore[n * L + l];
    const bool kept = r >= 0 && r < len_keep;
    rk[l] = kept ? (int)r : -1;
    if (kept) src[r] = l;
  }
  __syncthreads();
  const uint4* dn = dout + n * (1 + L) * nv;
  uint4* yn = dy + n * (1 + len_keep) * nv;
  const int per = (1 + len_keep + UNSHUFFLE_SLICES - 1) / UNSHUFFLE_SLICES;
  const int r0 = sl * per, r1 = min(1 + len_keep, r0 + per);
  for (int t = r0 * nv + threadIdx.x; t < r1 * nv; t += MAE_THREADS) {
    const int r = t / nv, v = t - r * nv;
    const int s = r == 0 ? 0 : (src[r - 1] >= 0 ? 1 + src[r - 1] : -1);
    yn[t] = s >= 0 ? dn[(int64_t)s * nv + v] : make_uint4(0u, 0u, 0u, 0u);
  }
  // removed rows: G row groups of nv threads, each thread 8 columns
  const int G = MAE_THREADS / nv;
  const int g = threadIdx.x / nv, v = threadIdx.x - g * nv;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (g < G)
    for (int l = sl + UNSHUFFLE_SLICES * g; l < L; l += UNSHUFFLE_SLICES * G)
      if (rk[l] < 0) acc8(s, dn[(int64_t)(1 + l) * nv + v]);
  if (g < G)
#pragma unroll
    for (int k = 0; k < 8; ++k) red[g * D + v * 8 + k] = s[k];
  __syncthreads();
  for (int col = threadIdx.x; col < D; col += MAE_THREADS) {
    float tot = 0.f;
    for (int q = 0; q < G; ++q) tot += red[q * D + col];
    partial[(n * UNSHUFFLE_SLICES + sl) * D + col] = tot;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// loss: one wave per patch (u = n L + l), lane owns elements e = lane + 64 i
struct LossArgs {
  const bf16_t* pred;
  int64_t stride_n, stride_r;
  int row0, p, H, W, L, gw, P, norm_pix;
  const void* imgs;
  const float* mask;
  int64_t N;
};

__device__ __forceinline__ float ld_img(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ld_img(const bf16_t* p, int64_t i) { return bf2f(p[i]); }

template <typename TI, bool BWD>
__global__ __launch_bounds__(MAE_THREADS) void mae_loss_kernel(LossArgs a, float* __restrict__ partial, bf16_t* __restrict__ dpred,
                                                               const float* __restrict__ out2, const float* __restrict__ gout) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t units = a.N * a.L;
  const float invP = 1.0f / (float)a.P;
  float acc = 0.f, macc = 0.f, g = 0.f;
  if (BWD) g = gout[0] * 2.0f * invP / out2[1];
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < units; u += (int64_t)gridDim.x * 4) {
    const int64_t n = u / a.L;
    const int l = (int)(u - n * a.L), ph = l / a.gw, pw = l - ph * a.gw;
    const TI* im = reinterpret_cast<const TI*>(a.imgs) + n * 3 * (int64_t)a.H * a.W;
    float t[LOSS_PER_LANE];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LOSS_PER_LANE; ++i) {
      const int e = lane + 64 * i;
      t[i] = 0.f;
      if (e < a.P) {
        const int c = e % 3, q = e / 3, py = q / a.p, px = q - py * a.p;
        t[i] = ld_img(im, ((int64_t)c * a.H + ph * a.p + py) * a.W + pw * a.p + px);
        s += t[i];
      }
    }
    if (a.norm_pix) {
      const float mean = wave_sum(s) * invP;
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < LOSS_PER_LANE; ++i)
        if (lane + 64 * i < a.P) { t[i] -= mean; ss += t[i] * t[i]; }
      const float inv_std = 1.0f / sqrtf(wave_sum(ss) / (float)(a.P - 1) + 1.e-6f);   // torch.var: unbiased
#pragma unroll
      for (int i = 0; i < LOSS_PER_LANE; ++i) t[i] *= inv_std;
    }
    const float m = a.mask[u];
    const bf16_t* pr = a.pred + n * a.stride_n + (int64_t)(a.row0 + l) * a.stride_r;
    if (!BWD) {
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < LOSS_PER_LANE; ++i) {
        const int e = lane + 64 * i;
        if (e < a.P) { const float d = bf2f(pr[e]) - t[i]; sq += d * d; }
      }
      acc += m * (wave_sum(sq) * invP);
      macc += m;
    } else {
      const int64_t rows = a.row0 + a.L;
      bf16_t* dp = dpred + (n * rows + a.row0 + l) * a.P;
      const float gm = g * m;
#pragma unroll
      for (int i = 0; i < LOSS_PER_LANE; ++i) {
        const int e = lane + 64 * i;
        if (e < a.P) dp[e] = f2bf(gm * (bf2f(pr[e]) - t[i]));
      }
      if (l == 0)
        for (int r = 0; r < a.row0; ++r)
          for (int e = lane; e < a.P; e += 64) dpred[(n * rows + r) * a.P + e] = 0;
    }
  }
  if (!BWD) {
    __shared__ float red[4][2];
    if (lane == 0) { red[wave][0] = acc; red[wave][1] = macc; }
    __syncthreads();
    if (threadIdx.x < 2)
      partial[(int64_t)blockIdx.x * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  }
}

__global__ __launch_bounds__(256) void mae_loss_final_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ out2) {
  __shared__ float red[4][2];
  float s0 = 0.f, s1 = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256) { s0 += partial[2 * i]; s1 += partial[2 * i + 1]; }
  s0 = wave_sum(s0); s1 = wave_sum(s1);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s0; red[threadIdx.x >> 6][1] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float a = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    const float b = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    out2[0] = a / b;
    out2[1] = b;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int loss_args(const dvla_mae_loss_params* p, LossArgs& a, int& nb) {
  if (!p || !p->pred || !p->imgs || !p->mask || p->N <= 0 || p->row0 < 0) return DVLA_ERR_ARG;
  if (p->patch < 1 || p->patch > 16 || p->H < p->patch || p->W < p->patch || p->H % p->patch || p->W % p->patch)
    return DVLA_ERR_UNSUPPORTED;
  if (p->imgs_dtype != DVLA_DT_F32 && p->imgs_dtype != DVLA_DT_BF16) return DVLA_ERR_UNSUPPORTED;
  const int P = 3 * p->patch * p->patch;
  if (p->pred_stride_r < P || p->pred_stride_n < 0) return DVLA_ERR_ARG;
  a.pred = reinterpret_cast<const bf16_t*>(p->pred);
  a.stride_n = p->pred_stride_n; a.stride_r = p->pred_stride_r;
  a.row0 = p->row0; a.p = p->patch; a.H = p->H; a.W = p->W;
  a.gw = p->W / p->patch; a.L = (p->H / p->patch) * a.gw; a.P = P; a.norm_pix = p->norm_pix != 0;
  a.imgs = p->imgs; a.mask = p->mask; a.N = p->N;
  int64_t b = (p->N * a.L + 3) / 4;
  nb = (int)(b > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : b);
  return DVLA_OK;
}

}  // namespace

extern "C" int dvla_mae_mask_fwd(const float* noise, const void* x, const void* cls_row, int32_t N, int32_t L, int32_t D, int32_t len_keep,
                                 int64_t* ids_restore, float* mask, void* out, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!noise || !x || !ids_restore || !mask || !out || N <= 0 || L <= 0 || D <= 0) return DVLA_ERR_ARG;
  if (L > MAE_MAX_L || len_keep <= 0 || len_keep > L || D % 8 != 0) return DVLA_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(out) || (cls_row && !aligned16(cls_row))) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mae_mask_fwd_kernel, dim3(N), dim3(MAE_THREADS), 0, stream, noise, reinterpret_cast<const uint4*>(x),
                     reinterpret_cast<const uint4*>(cls_row), L, D / 8, len_keep, ids_restore, mask, reinterpret_cast<uint4*>(out));
  return dvla_check_launch();
}

extern "C" int dvla_mae_mask_bwd(const int64_t* ids_restore, const void* dout, int32_t has_cls, int32_t N, int32_t L, int32_t D,
                                 int32_t len_keep, void* dx, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!ids_restore || !dout || !dx || N <= 0 || L <= 0 || D <= 0) return DVLA_ERR_ARG;
  if (L > MAE_MAX_L || len_keep <= 0 || len_keep > L || D % 8 != 0 || N > 65535) return DVLA_ERR_UNSUPPORTED;
  if (!aligned16(dout) || !aligned16(dx)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mae_mask_bwd_kernel, dim3((L + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, N), dim3(MAE_THREADS), 0, stream, ids_restore,
                     reinterpret_cast<const uint4*>(dout), has_cls ? 1 : 0, L, D / 8, len_keep, reinterpret_cast<uint4*>(dx));
  return dvla_check_launch();
}

extern "C" int dvla_mae_unshuffle_fwd(const void* y, const void* mask_token, const int64_t* ids_restore, const void* pos, int32_t N,
                                      int32_t L, int32_t D, int32_t len_keep, void* out, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!y || !mask_token || !ids_restore || !pos || !out || N <= 0 || L <= 0 || D <= 0) return DVLA_ERR_ARG;
  if (L > MAE_MAX_L || len_keep <= 0 || len_keep > L || D % 8 != 0 || D > 8 * MAE_THREADS || N > 65535) return DVLA_ERR_UNSUPPORTED;
  if (!aligned16(y) || !aligned16(mask_token) || !aligned16(pos) || !aligned16(out)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mae_unshuffle_fwd_kernel, dim3((L + 1 + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, N), dim3(MAE_THREADS), 0, stream,
                     reinterpret_cast<const uint4*>(y), reinterpret_cast<const uint4*>(mask_token), ids_restore,
                     reinterpret_cast<const uint4*>(pos), L, D / 8, len_keep, reinterpret_cast<uint4*>(out));
  return dvla_check_launch();
}

extern "C" int dvla_mae_unshuffle_bwd(const void* dout, const int64_t* ids_restore, int32_t N, int32_t L, int32_t D, int32_t len_keep,
                                      void* dy, void* dmask_token, int32_t dmask_dtype, float* partial, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!dout || !ids_restore || !dy || !dmask_token || !partial || N <= 0 || L <= 0 || D <= 0) return DVLA_ERR_ARG;
  if (dmask_dtype != DVLA_DT_F32 && dmask_dtype != DVLA_DT_BF16) return DVLA_ERR_ARG;
  if (L > MAE_MAX_L || len_keep <= 0 || len_keep > L || D % 8 != 0 || D > 8 * MAE_THREADS || N > 65535) return DVLA_ERR_UNSUPPORTED;
  if (!aligned16(dout) || !aligned16(dy)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mae_unshuffle_bwd_kernel, dim3(UNSHUFFLE_SLICES, N), dim3(MAE_THREADS), 0, stream, reinterpret_cast<const uint4*>(dout),
                     ids_restore, L, D / 8, len_keep, reinterpret_cast<uint4*>(dy), partial);
  int rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  return dvla_reduce_partial_rows(partial, N * UNSHUFFLE_SLICES, D, D, dmask_token, dmask_dtype == DVLA_DT_BF16, stream);
}

extern "C" int64_t dvla_mae_loss_partial_len(void) { return (int64_t)LOSS_MAX_BLOCKS * 2; }

extern "C" int dvla_mae_loss_fwd(const dvla_mae_loss_params* p, float* out2, float* partial, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  LossArgs a;
  int nb = 0;
  int rc = loss_args(p, a, nb);
  if (rc != DVLA_OK) return rc;
  if (!out2 || !partial) return DVLA_ERR_ARG;
  if (p->imgs_dtype == DVLA_DT_F32)
    hipLaunchKernelGGL((mae_loss_kernel<float, false>), dim3(nb), dim3(MAE_THREADS), 0, stream, a, partial, nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL((mae_loss_kernel<bf16_t, false>), dim3(nb), dim3(MAE_THREADS), 0, stream, a, partial, nullptr, nullptr, nullptr);
  rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  hipLaunchKernelGGL(mae_loss_final_kernel, dim3(1), dim3(256), 0, stream, partial, nb, out2);
  return dvla_check_launch();
}

extern "C" int dvla_mae_loss_bwd(const dvla_mae_loss_params* p, const float* out2, const float* grad_out, void* dpred, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  LossArgs a;
  int nb = 0;
  int rc = loss_args(p, a, nb);
  if (rc != DVLA_OK) return rc;
  if (!out2 || !grad_out || !dpred) return DVLA_ERR_ARG;
  bf16_t* dp = reinterpret_cast<bf16_t*>(dpred);
  if (p->imgs_dtype == DVLA_DT_F32)
    hipLaunchKernelGGL((mae_loss_kernel<float, true>), dim3(nb), dim3(MAE_THREADS), 0, stream, a, nullptr, dp, out2, grad_out);
  else
    hipLaunchKernelGGL((mae_loss_kernel<bf16_t, true>), dim3(nb), dim3(MAE_THREADS), 0, stream, a, nullptr, dp, out2, grad_out);
  return dvla_check_launch();
}
