// dream_score.hip -- how good a dream was: image quality (exact sum of squared differences -> MSE / PSNR, and the mean SSIM of
// Wang et al. 2004) between two uint8 HWC batches, and the depth metrics (abs-rel, RMSE, SiLog, delta < 1.25) between two fp32
// map batches.  An addition: the reference logs pictures only.  Everything stays on the device; both metric
// sets are two launches: per-tile (per-chunk) partials into the caller's workspace, then one workgroup per image adds them in
// one fixed order.  No atomics: an image's result is bit-identical from run to run and does not depend on the batch around it.
//
// SSIM: 11 x 11 Gaussian window (sigma 1.5, normalised), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, population covariances, the
// map at the (H - 10) x (W - 10) positions whose window lies inside the image, every channel on its own, all averaged -- what
// skimage.metrics.structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=255, channel_axis=-1) gives.
//
// image_quality_tile_kernel: one workgroup of 256 per (image, 32 x 32 tile of the SSIM map).
//   1. The 42 x 42 pixels under the tile (tile + 10 halo), all three channels of both images, go to LDS as the bytes they are:
//      every row is fetched as the ALIGNED dwords that cover it (consecutive lanes, consecutive dwords) and stored at the same
//      offset within its word, so a row of any width at any address costs 32-33 dword loads, not 126 byte loads.  A dword that
//      would reach outside the two buffers is assembled from its inside bytes.              2 x 42 x 136 B = 11.2 KiB
//   2. SSE over the pixels the tile OWNS (its 32 x 32, the last tile row / column of the grid also the 10 behind it) in uint32:
//      at most 42 * 42 * 3 * 255^2 = 3.4e8 per tile.
//   3. Per channel: the horizontal pass -- a thread takes one row and four adjacent columns: 14 pixels of each image, centred
//      (x - 128: E[x^2] - mu^2 then cancels at 128^2 = 16384 at most instead of 65025, and exactly nothing is lost: the bytes and
//      their products are integers below 2^24), the five moments x, y, x^2, y^2, xy filtered to mom[5][42][32] fp32 (26.3 KiB) --
//      then the vertical pass -- a thread takes one column and four adjacent rows, 14 x 5 values down the column (lanes along the
//      row: conflict-free), and turns the 4 x 5 filtered moments into 4 SSIM values.
//   4. The tile's SSIM sum (per-thread in a fixed order, xor butterfly, four waves in order) and its SSE go to the workspace.
//   38 KiB LDS: four workgroups (16 waves) per CU; the LDS reads of step 3 are what the kernel waits for, so occupancy is spent there.
// image_quality_final_kernel: one workgroup per image; partials in float64 / uint64, thread-strided then a fixed tree.
#include <math.h>

#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int WIN = 11, HALO = WIN - 1, TILE = 32, IN = TILE + HALO;
constexpr int ROW_WORDS = 34, ROWB = ROW_WORDS * 4;      // 3 * 42 = 126 bytes + up to 3 in front: 33 words, one more against 32-bank strides
constexpr int THREADS = 256;
constexpr int DEPTH_CHUNK = 4096;                        // pixels per workgroup of the depth kernel: 16 per thread

struct Gauss { float w[WIN]; };

__device__ __forceinline__ uint32_t load_word(uintptr_t addr, uintptr_t lo, uintptr_t hi) {
  if (addr >= lo && addr + 4 <= hi) return *reinterpret_cast<const uint32_t*>(addr);
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uintptr_t q = addr + i;
    if (q >= lo && q < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(q) << (8 * i);
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
  return v;
}

__global__ void __launch_bounds__(THREADS) image_quality_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                     int64_t total_bytes, int H, int W, int tiles_y, int tiles_x,
                                                                     Gauss g, float* __restrict__ part_ssim,
                                                                     uint32_t* __restrict__ part_sse) {
  __shared__ __attribute__((aligned(16))) uint8_t px[2][IN * ROWB];
  __shared__ __attribute__((aligned(16))) float mom[5][IN][TILE];
  __shared__ float red_f[THREADS / 64];
  __shared__ uint32_t red_u[THREADS / 64];

  const int tid = threadIdx.x;
  const int per = tiles_y * tiles_x;
  const int64_t img = (int64_t)blockIdx.x / per;
  const int t = (int)((int64_t)blockIdx.x % per);
  const int ty = t / tiles_x, tx = t % tiles_x;
  const int y0 = ty * TILE, x0 = tx * TILE;
  const int th = min(TILE, H - HALO - y0), tw = min(TILE, W - HALO - x0);       // SSIM positions of this tile
  const int rows = th + HALO, cols = tw + HALO;                                 // the pixels under them: all inside the image
  const int nbytes = cols * 3;
  const int64_t row0 = ((img * H + y0) * (int64_t)W + x0) * 3;                  // byte offset of the region's first pixel
  const int64_t pitch = (int64_t)W * 3;
  const uintptr_t lo_a = reinterpret_cast<uintptr_t>(a), lo_b = reinterpret_cast<uintptr_t>(b);

  // 1. stage: (image, row, word) items, word fastest
  for (int it = tid; it < 2 * IN * ROW_WORDS; it += THREADS) {
    const int im = it / (IN * ROW_WORDS);
    const int rem = it - im * (IN * ROW_WORDS);
    const int r = rem / ROW_WORDS, k = rem - r * ROW_WORDS;
    if (r < rows) {
      const uintptr_t lo = im ? lo_b : lo_a;
      const uintptr_t p = lo + (uintptr_t)(row0 + r * pitch);
      const int off = (int)(p & 3);
      if (4 * k < off + nbytes)
        *reinterpret_cast<uint32_t*>(&px[im][r * ROWB + 4 * k]) = load_word(p - off + 4 * k, lo, lo + (uintptr_t)total_bytes);
    }
  }
  __syncthreads();

  // 2. SSE of the owned pixels: 8 rows per sweep, 32 lanes along a row's bytes
  uint32_t sse = 0;
  {
    const int own_r = ty == tiles_y - 1 ? rows : TILE, own_b = (tx == tiles_x - 1 ? cols : TILE) * 3;
    for (int r = tid >> 5; r < own_r; r += THREADS / 32) {
      const int oa = r * ROWB + (int)((lo_a + (uintptr_t)(row0 + r * pitch)) & 3);
      const int ob = r * ROWB + (int)((lo_b + (uintptr_t)(row0 + r * pitch)) & 3);
      for (int j = tid & 31; j < own_b; j += 32) {
        const int d = (int)px[0][oa + j] - (int)px[1][ob + j];
        sse += (uint32_t)(d * d);
      }
    }
  }

  // 3. SSIM, one channel at a time
  const float C1 = 6.5025f, C2 = 58.5225f;
  float acc = 0.f;
  for (int ch = 0; ch < 3; ++ch) {
    for (int it = tid; it < IN * (TILE / 4); it += THREADS) {
      const int r = it >> 3, c0 = (it & 7) * 4;
      const int oa = r * ROWB + (int)((lo_a + (uintptr_t)(row0 + r * pitch)) & 3) + 3 * c0 + ch;
      const int ob = r * ROWB + (int)((lo_b + (uintptr_t)(row0 + r * pitch)) & 3) + 3 * c0 + ch;
      float x[4 + HALO], y[4 + HALO];
#pragma unroll
      for (int j = 0; j < 4 + HALO; ++j) {
        x[j] = (float)px[0][oa + 3 * j] - 128.f;
        y[j] = (float)px[1][ob + 3 * j] - 128.f;
      }
      float s[5][4];
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) s[m][o] = 0.f;
#pragma unroll
      for (int j = 0; j < 4 + HALO; ++j) {
        const float xx = x[j] * x[j], yy = y[j] * y[j], xy = x[j] * y[j];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int k = j - o;                           // tap of output o that pixel j falls under
          if (k >= 0 && k < WIN) {
            const float w = g.w[k];
            s[0][o] = fmaf(w, x[j], s[0][o]);
            s[1][o] = fmaf(w, y[j], s[1][o]);
            s[2][o] = fmaf(w, xx, s[2][o]);
            s[3][o] = fmaf(w, yy, s[3][o]);
            s[4][o] = fmaf(w, xy, s[4][o]);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) *reinterpret_cast<float4*>(&mom[m][r][c0]) = make_float4(s[m][0], s[m][1], s[m][2], s[m][3]);
    }
    __syncthreads();
    {
      const int c = tid & 31, r0 = (tid >> 5) * 4;
      float s[5][4];
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) s[m][o] = 0.f;
#pragma unroll
      for (int j = 0; j < 4 + HALO; ++j) {
        float v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) v[m] = mom[m][r0 + j][c];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int k = j - o;
          if (k >= 0 && k < WIN) {
            const float w = g.w[k];
#pragma unroll
            for (int m = 0; m < 5; ++m) s[m][o] = fmaf(w, v[m], s[m][o]);
          }
        }
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const float mx = s[0][o], my = s[1][o];                       // centred means
        const float vx = s[2][o] - mx * mx, vy = s[3][o] - my * my, vxy = s[4][o] - mx * my;
        const float ux = mx + 128.f, uy = my + 128.f;
        const float num = (2.f * ux * uy + C1) * (2.f * vxy + C2);
        const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
        if (r0 + o < th && c < tw) acc += num / den;
      }
    }
    __syncthreads();
  }

  // 4. the tile's two partials
  acc = wave_sum(acc);
  sse = wave_sum_u32(sse);
  if ((tid & 63) == 0) { red_f[tid >> 6] = acc; red_u[tid >> 6] = sse; }
  __syncthreads();
  if (tid == 0) {
    part_ssim[blockIdx.x] = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
    part_sse[blockIdx.x] = red_u[0] + red_u[1] + red_u[2] + red_u[3];
  }
}

// one workgroup per image: sse (int64), out3 = (mse, psnr, ssim)
__global__ void __launch_bounds__(THREADS) image_quality_final_kernel(const float* __restrict__ part_ssim,
                                                                      const uint32_t* __restrict__ part_sse, int per, int H, int W,
                                                                      int64_t* __restrict__ sse_out, float* __restrict__ out3) {
  __shared__ double red_d[THREADS / 64];
  __shared__ unsigned long long red_u[THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * per;
  double s = 0.0;
  unsigned long long e = 0;
  for (int i = tid; i < per; i += THREADS) { s += (double)part_ssim[base + i]; e += part_sse[base + i]; }
  s = wave_sum_f64(s);
  e = wave_sum_u64(e);
  if ((tid & 63) == 0) { red_d[tid >> 6] = s; red_u[tid >> 6] = e; }
  __syncthreads();
  if (tid == 0) {
    s = (red_d[0] + red_d[1]) + (red_d[2] + red_d[3]);
    e = red_u[0] + red_u[1] + red_u[2] + red_u[3];
    const double mse = (double)e / ((double)H * W * 3.0);
    sse_out[blockIdx.x] = (int64_t)e;
    out3[3 * (int64_t)blockIdx.x + 0] = (float)mse;
    out3[3 * (int64_t)blockIdx.x + 1] = e == 0 ? INFINITY : (float)(10.0 * log10(65025.0 / mse));
    out3[3 * (int64_t)blockIdx.x + 2] = (float)(s / ((double)(H - HALO) * (W - HALO) * 3.0));
  }
}

// one workgroup per (image, chunk of DEPTH_CHUNK pixels): sums of |p - t| / t, (p - t)^2, d, d^2 and the two counts
__global__ void __launch_bounds__(THREADS) depth_quality_chunk_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                      int64_t hw, int chunks, float* __restrict__ part_f,
                                                                      uint32_t* __restrict__ part_u) {
  __shared__ float red_f[THREADS / 64][4];
  __shared__ uint32_t red_u[THREADS / 64][2];
  const int tid = threadIdx.x;
  const int64_t img = (int64_t)blockIdx.x / chunks;
  const int64_t begin = ((int64_t)blockIdx.x % chunks) * DEPTH_CHUNK;
  const int64_t end = begin + DEPTH_CHUNK < hw ? begin + DEPTH_CHUNK : hw;
  float sa = 0.f, sq = 0.f, sd = 0.f, sdd = 0.f;
  uint32_t nv = 0, nd = 0;
  for (int64_t i = begin + tid; i < end; i += THREADS) {
    const float t = tgt[img * hw + i];
    const float p = fmaxf(pred[img * hw + i], 0.f);
    if (t > 0.f) {
      const float e = p - t;
      const float d = logf(t + 1e-6f) - logf(p + 1e-6f);
      sa += fabsf(e) / t;
      sq = fmaf(e, e, sq);
      sd += d;
      sdd = fmaf(d, d, sdd);
      nv += 1;
      nd += fmaxf(p / t, t / p) < 1.25f ? 1u : 0u;
    }
  }
  sa = wave_sum(sa); sq = wave_sum(sq); sd = wave_sum(sd); sdd = wave_sum(sdd);
  nv = wave_sum_u32(nv); nd = wave_sum_u32(nd);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    red_f[w][0] = sa; red_f[w][1] = sq; red_f[w][2] = sd; red_f[w][3] = sdd;
    red_u[w][0] = nv; red_u[w][1] = nd;
  }
  __syncthreads();
  if (tid < 4) part_f[4 * (int64_t)blockIdx.x + tid] = (red_f[0][tid] + red_f[1][tid]) + (red_f[2][tid] + red_f[3][tid]);
  else if (tid < 6) part_u[2 * (int64_t)blockIdx.x + tid - 4] = red_u[0][tid - 4] + red_u[1][tid - 4] + red_u[2][tid - 4] + red_u[3][tid - 4];
}

// one workgroup per image: valid (int64), out4 = (abs_rel, rmse, silog, delta1); NaN where nothing is valid
__global__ void __launch_bounds__(THREADS) depth_quality_final_kernel(const float* __restrict__ part_f, const uint32_t* __restrict__ part_u,
                                                                      int chunks, int64_t* __restrict__ valid, float* __restrict__ out4) {
  __shared__ double red_d[THREADS / 64][4];
  __shared__ unsigned long long red_u[THREADS / 64][2];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * chunks;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned long long c[2] = {0, 0};
  for (int i = tid; i < chunks; i += THREADS) {
#pragma unroll
    for (int m = 0; m < 4; ++m) s[m] += (double)part_f[4 * (base + i) + m];
    c[0] += part_u[2 * (base + i)];
    c[1] += part_u[2 * (base + i) + 1];
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) s[m] = wave_sum_f64(s[m]);
  c[0] = wave_sum_u64(c[0]);
  c[1] = wave_sum_u64(c[1]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) red_d[tid >> 6][m] = s[m];
    red_u[tid >> 6][0] = c[0];
    red_u[tid >> 6][1] = c[1];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) s[m] = (red_d[0][m] + red_d[1][m]) + (red_d[2][m] + red_d[3][m]);
    const unsigned long long nv = red_u[0][0] + red_u[1][0] + red_u[2][0] + red_u[3][0];
    const unsigned long long nd = red_u[0][1] + red_u[1][1] + red_u[2][1] + red_u[3][1];
    valid[blockIdx.x] = (int64_t)nv;
    float* o = out4 + 4 * (int64_t)blockIdx.x;
    if (nv == 0) {
      o[0] = o[1] = o[2] = o[3] = NAN;
    } else {
      const double n = (double)nv, md = s[2] / n;
      o[0] = (float)(s[0] / n);
      o[1] = (float)sqrt(s[1] / n);
      o[2] = (float)sqrt(s[3] / n - 0.5 * md * md);
      o[3] = (float)((double)nd / n);
    }
  }
}

inline int64_t tiles_of(int32_t size) { return ((int64_t)size - HALO + TILE - 1) / TILE; }
inline int64_t chunks_of(int32_t height, int32_t width) { return ((int64_t)height * width + DEPTH_CHUNK - 1) / DEPTH_CHUNK; }

}  // namespace

extern "C" int64_t dvla_image_quality_partial_len(int64_t n, int32_t height, int32_t width) {
  if (n < 0 || height < WIN || width < WIN) return 0;
  return 2 * n * tiles_of(height) * tiles_of(width);
}

extern "C" int dvla_image_quality(const uint8_t* a, const uint8_t* b, int64_t n, int32_t height, int32_t width, int64_t* sse,
                                  float* mse_psnr_ssim, void* partial, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!a || !b || !sse || !mse_psnr_ssim || !partial || n < 0 || height < 1 || width < 1) return DVLA_ERR_ARG;
  if (height < WIN || width < WIN) return DVLA_ERR_UNSUPPORTED;
  if (n == 0) return DVLA_OK;
  const int64_t ty = tiles_of(height), tx = tiles_of(width);
  if (ty * tx > 0x7fffffff || n > 0x7fffffff || n * ty * tx > 0x7fffffff) return DVLA_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(partial) & 3) return DVLA_ERR_UNSUPPORTED;
  Gauss g;
  double w[WIN], sum = 0.0;
  for (int i = 0; i < WIN; ++i) { w[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += w[i]; }
  for (int i = 0; i < WIN; ++i) g.w[i] = (float)(w[i] / sum);
  const int64_t blocks = n * ty * tx;
  float* part_ssim = reinterpret_cast<float*>(partial);
  uint32_t* part_sse = reinterpret_cast<uint32_t*>(partial) + blocks;
  hipLaunchKernelGGL(image_quality_tile_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, a, b,
                     n * (int64_t)height * width * 3, height, width, (int)ty, (int)tx, g, part_ssim, part_sse);
  hipLaunchKernelGGL(image_quality_final_kernel, dim3((unsigned)n), dim3(THREADS), 0, stream, part_ssim, part_sse, (int)(ty * tx),
                     height, width, sse, mse_psnr_ssim);
  return dvla_check_launch();
}

extern "C" int64_t dvla_depth_quality_partial_len(int64_t n, int32_t height, int32_t width) {
  if (n < 0 || height < 1 || width < 1) return 0;
  return 6 * n * chunks_of(height, width);
}

extern "C" int dvla_depth_quality(const float* pred, const float* target, int64_t n, int32_t height, int32_t width, int64_t* valid,
                                  float* metrics4, void* partial, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!pred || !target || !valid || !metrics4 || !partial || n < 0 || height < 1 || width < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  const int64_t chunks = chunks_of(height, width);
  if (chunks > 0x7fffffff || n > 0x7fffffff || n * chunks > 0x7fffffff) return DVLA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & 3)
    return DVLA_ERR_UNSUPPORTED;
  const int64_t blocks = n * chunks;
  float* part_f = reinterpret_cast<float*>(partial);
  uint32_t* part_u = reinterpret_cast<uint32_t*>(partial) + 4 * blocks;
  hipLaunchKernelGGL(depth_quality_chunk_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, pred, target,
                     (int64_t)height * width, (int)chunks, part_f, part_u);
  hipLaunchKernelGGL(depth_quality_final_kernel, dim3((unsigned)n), dim3(THREADS), 0, stream, part_f, part_u, (int)chunks, valid,
                     metrics4);
  return dvla_check_launch();
}
