// dream_view.hip -- the depth, motion and feature dreams as pictures (an addition): what
// `ops.dream_render` hands back as numbers becomes uint8 HWC frames on the device, inside the same decode as the dreams.
//
//   depth_range_kernel + depth_colorize_kernel   fp32 map -> palette colours; the range is given, or the map's own finite min / max
//   flow_unshuffle_kernel                        trajectory prediction (tokens, 2 f^2) bf16 -> flow (g f, g f, 2) fp32, a permutation
//   flow_wheel_kernel                            flow -> the reference's HSV wheel (utils/visualize_utils.py), nearest-upsampled
//   motion_mask_kernel                           per token: |mean flow| > thr, optionally dilated 3 x 3 (losses.calvin_losses' fmask)
//   motion_overlay_kernel                        the model's CLIP-normalised input frame as bytes, masked patches blended to a tint
//   feature_render_kernel                        (tokens, D) bf16 features -> 3 fixed projections -> bytes, one wave per token
//
// Arithmetic that a test restates bit for bit is written with one rounding per operation (`#pragma clang fp contract(off)`):
//   level(v, lo, hi):  s = v - lo;  r = hi - lo;  t = s / r (IEEE division);  t = (r > 0 and t > 0) ? min(t, 1) : 0 (hi == lo and a NaN
//                      quotient give 0);  u = 255 * t;  index = rint(u), half to even.
// Everything is HBM- or launch-bound; no LDS beyond the 1 KiB palette, no atomics, vector stores only.
#include <math.h>

#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int THREADS = 256;
constexpr int RANGE_CHUNK_MIN = 4096;     // pixels per workgroup of the range kernel, at least
constexpr int RANGE_CHUNKS_MAX = 64;      // partials per map, at most: every workgroup of the map kernel reads them all

__device__ __forceinline__ int level_u8(float v, float lo, float hi) {
#pragma clang fp contract(off)
  const float s = v - lo;
  const float r = hi - lo;
  float t = s / r;
  t = (r > 0.f && t > 0.f) ? fminf(t, 1.0f) : 0.f;
  const float u = 255.0f * t;
  return (int)rintf(u);
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }     // false for NaN

__host__ __device__ __forceinline__ int range_chunk(int64_t hw) {
  int64_t c = (hw + RANGE_CHUNKS_MAX - 1) / RANGE_CHUNKS_MAX;
  c = (c + 3) & ~(int64_t)3;
  return (int)(c < RANGE_CHUNK_MIN ? RANGE_CHUNK_MIN : c);
}

// partial[(map * chunks + chunk) * 2 + {0, 1}] = min, max over the finite pixels of the chunk (+inf, -inf when it has none)
__global__ void __launch_bounds__(THREADS) depth_range_kernel(const float* __restrict__ depth, float* __restrict__ partial,
                                                              int64_t hw, int chunk, int chunks) {
  __shared__ float smin[THREADS / 64], smax[THREADS / 64];
  const int64_t map = blockIdx.y;
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < hw ? begin + chunk : hw;
  const float* src = depth + map * hw;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = begin + threadIdx.x; i < end; i += THREADS) {
    const float v = src[i];
    if (finite_f(v)) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) { lo = fminf(lo, smin[w]); hi = fmaxf(hi, smax[w]); }
    float* dst = partial + (map * chunks + blockIdx.x) * 2;
    dst[0] = lo; dst[1] = hi;
  }
}

// depth (n, hw) fp32 -> out (n, hw, 3) uint8.  A thread owns 4 consecutive pixels of one map; VEC: one 16-byte load, three 4-byte
// stores (hw % 4 == 0, aligned bases), otherwise element by element.
template <bool VEC>
__global__ void __launch_bounds__(THREADS) depth_colorize_kernel(const float* __restrict__ depth, uint8_t* __restrict__ out,
                                                                 const uint8_t* __restrict__ palette, const float* __restrict__ partial,
                                                                 int64_t hw, int chunks, float lo, float hi, uint32_t nan_rgb) {
  __shared__ uint32_t pal[256];
  {
    const uint8_t* p = palette + 3 * threadIdx.x;
    pal[threadIdx.x] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
  const int64_t map = blockIdx.y;
  if (partial) {                        // the map's own range: min / max are exact in any order
    lo = INFINITY; hi = -INFINITY;
    const float* pp = partial + map * chunks * 2;
    for (int c = 0; c < chunks; ++c) { lo = fminf(lo, pp[2 * c]); hi = fmaxf(hi, pp[2 * c + 1]); }
  }
  __syncthreads();
  const int64_t p0 = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 4;
  if (p0 >= hw) return;
  const float* src = depth + map * hw + p0;
  uint8_t* dst = out + (map * hw + p0) * 3;
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(src);
    const float d[4] = {v.x, v.y, v.z, v.w};
    uint32_t c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = finite_f(d[e]) ? pal[level_u8(d[e], lo, hi)] : nan_rgb;
    uint32_t* w = reinterpret_cast<uint32_t*>(dst);
    w[0] = c[0] | (c[1] << 24);
    w[1] = (c[1] >> 8) | (c[2] << 16);
    w[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (int e = 0; e < 4 && p0 + e < hw; ++e) {
      const float v = src[e];
      const uint32_t c = finite_f(v) ? pal[level_u8(v, lo, hi)] : nan_rgb;
      dst[3 * e] = (uint8_t)c; dst[3 * e + 1] = (uint8_t)(c >> 8); dst[3 * e + 2] = (uint8_t)(c >> 16);
    }
  }
}

// flow[n, y f + i, x f + j, c] = pred[n, y g + x, c f^2 + i f + j]; one thread per flow cell, one 8-byte store
__global__ void __launch_bounds__(THREADS) flow_unshuffle_kernel(const bf16_t* __restrict__ pred, float* __restrict__ flow,
                                                                 int64_t cells, int g, int f) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= cells) return;
  const int side = g * f;
  const int X = (int)(idx % side), Y = (int)((idx / side) % side);
  const int64_t n = idx / ((int64_t)side * side);
  const int ff = f * f;
  const bf16_t* src = pred + (n * g * g + (int64_t)(Y / f) * g + X / f) * (2 * ff) + (Y % f) * f + X % f;
  *reinterpret_cast<float2*>(flow + idx * 2) = make_float2(bf2f(src[0]), bf2f(src[ff]));
}

// the reference's wheel (utils/visualize_utils.py): angle = atan2(dy, dx) in degrees in [0, 360), Hh = trunc(angle / 2), S = 255,
// V = trunc(clip(32 |flow|, 0, 255)); HSV -> RGB on those integers: sextant s = Hh / 30, X = (V (30 - |Hh % 60 - 30|) + 15) / 30,
// (R, G, B) = (V,X,0) (X,V,0) (0,V,X) (0,X,V) (X,0,V) (V,0,X) for s = 0 .. 5.  A non-finite flow is black.
__device__ __forceinline__ uint32_t wheel_rgb(float dx, float dy) {
  if (!finite_f(dx) || !finite_f(dy)) return 0u;
  const float mag = sqrtf(dx * dx + dy * dy);         // +inf for a huge finite flow: V saturates
  float ang = atan2f(dy, dx) * 57.29577951308232f;
  if (ang < 0.f) ang += 360.0f;
  int Hh = (int)(ang * 0.5f);
  Hh = Hh > 179 ? 0 : Hh;                             // -0.0 .. rounding up to 360 is the angle 0
  const int V = (int)fminf(32.0f * mag, 255.0f);
  const int r = Hh % 60;
  const int X = (V * (30 - (r < 30 ? 30 - r : r - 30)) + 15) / 30;
  const int s = Hh / 30;
  const int R = (s == 0 || s == 5) ? V : ((s == 1 || s == 4) ? X : 0);
  const int G = (s == 1 || s == 2) ? V : ((s == 0 || s == 3) ? X : 0);
  const int B = (s == 3 || s == 4) ? V : ((s == 2 || s == 5) ? X : 0);
  return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
}

// flow (n, ih, iw, 2) fp32 -> out (n, oh, ow, 3) uint8, src = dst * in // out per axis.  A thread owns 4 consecutive pixels of a
// row (VEC: ow % 4 == 0, three 4-byte stores) or one pixel.
template <bool VEC>
__global__ void __launch_bounds__(THREADS) flow_wheel_kernel(const float* __restrict__ flow, uint8_t* __restrict__ out, int64_t items,
                                                             int ih, int iw, int oh, int ow) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= items) return;
  constexpr int PER = VEC ? 4 : 1;
  const int per_row = ow / PER;
  const int x0 = (int)(idx % per_row) * PER, y = (int)((idx / per_row) % oh);
  const int64_t n = idx / ((int64_t)per_row * oh);
  const int sy = (int)((int64_t)y * ih / oh);
  const float* row = flow + ((n * ih + sy) * (int64_t)iw) * 2;
  uint32_t c[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int sx = (int)((int64_t)(x0 + e) * iw / ow);
    const float2 v = *reinterpret_cast<const float2*>(row + 2 * sx);
    c[e] = wheel_rgb(v.x, v.y);
  }
  uint8_t* dst = out + ((n * oh + y) * (int64_t)ow + x0) * 3;
  if (VEC) {
    uint32_t* w = reinterpret_cast<uint32_t*>(dst);
    w[0] = c[0] | (c[PER > 1 ? 1 : 0] << 24);
    w[1] = (c[PER > 1 ? 1 : 0] >> 8) | (c[PER > 2 ? 2 : 0] << 16);
    w[2] = (c[PER > 2 ? 2 : 0] >> 16) | (c[PER > 3 ? 3 : 0] << 8);
  } else {
    dst[0] = (uint8_t)c[0]; dst[1] = (uint8_t)(c[0] >> 8); dst[2] = (uint8_t)(c[0] >> 16);
  }
}

// one token's own verdict: the means of its f^2 dx and f^2 dy in fp32 (summed in channel order, times 1 / f^2), dx^2 + dy^2 > thr^2
__device__ __forceinline__ bool token_moves(const bf16_t* __restrict__ tok, int ff, float inv, float thr2) {
  float sx = 0.f, sy = 0.f;
  for (int k = 0; k < ff; ++k) { sx += bf2f(tok[k]); sy += bf2f(tok[ff + k]); }
  sx *= inv; sy *= inv;
  return sx * sx + sy * sy > thr2;
}

// pred (n, g g, 2 f^2) bf16 -> mask (n, g, g) uint8 in {0, 1}; dilate: the OR over the 3 x 3 neighbourhood inside the grid
__global__ void __launch_bounds__(THREADS) motion_mask_kernel(const bf16_t* __restrict__ pred, uint8_t* __restrict__ mask,
                                                              int64_t tokens, int g, int ff, float thr, int dilate) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= tokens) return;
  const int x = (int)(idx % g), y = (int)((idx / g) % g);
  const int64_t n = idx / ((int64_t)g * g);
  const float inv = 1.0f / (float)ff, thr2 = thr * thr;
  const bf16_t* base = pred + n * g * g * (2 * ff);
  bool on = false;
  const int r = dilate ? 1 : 0;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy < 0 || yy >= g || xx < 0 || xx >= g) continue;
      on = on || token_moves(base + ((int64_t)yy * g + xx) * (2 * ff), ff, inv, thr2);
    }
  mask[idx] = on ? 1 : 0;
}

// cur (n, 3, H, W) bf16 CLIP-normalised, mask (n, g, g) -> out (n, H, W, 3) uint8: render_u8_kernel's de-normalisation
// u8(rint(255 clamp(x std + mean, 0, 1))) (csrc/dream.hip, the same expression), then inside masked cells
// (v (256 - a) + tint a + 128) >> 8.  A thread owns 4 consecutive pixels of a row: three 8-byte loads, three 4-byte stores.
__global__ void __launch_bounds__(THREADS) motion_overlay_kernel(const bf16_t* __restrict__ cur, const uint8_t* __restrict__ mask,
                                                                 uint8_t* __restrict__ out, int64_t items, int H, int W, int g,
                                                                 float m0, float m1, float m2, float s0, float s1, float s2,
                                                                 int t0, int t1, int t2, int alpha) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= items) return;
  const int per_row = W / 4;
  const int x0 = (int)(idx % per_row) * 4, y = (int)((idx / per_row) % H);
  const int64_t n = idx / ((int64_t)per_row * H);
  const int cell_h = H / g, cell_w = W / g;
  const uint8_t* mrow = mask + (n * g + y / cell_h) * g;
  uint32_t b[12];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const uint2 raw = *reinterpret_cast<const uint2*>(cur + ((n * 3 + ch) * H + y) * (int64_t)W + x0);
    const float f[4] = {__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u), __uint_as_float(raw.y << 16),
                        __uint_as_float(raw.y & 0xffff0000u)};
    const float cm = ch == 0 ? m0 : (ch == 1 ? m1 : m2), cs = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
    const int tint = ch == 0 ? t0 : (ch == 1 ? t1 : t2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = __builtin_fmaf(f[e], cs, cm);          // render_u8_kernel's `xs * cs + cm` compiles to one fma: said here outright
      t = fminf(fmaxf(t, 0.f), 1.f);
      int v = (int)rintf(t * 255.0f);
      if (mrow[(x0 + e) / cell_w]) v = (v * (256 - alpha) + tint * alpha + 128) >> 8;
      b[3 * e + ch] = (uint32_t)v;
    }
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + ((n * H + y) * (int64_t)W + x0) * 3);
#pragma unroll
  for (int w = 0; w < 3; ++w) dst[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
}

// feat (n g g, D) bf16, Wm (D, 3) fp32 -> out (n, oh, ow, 3) uint8.  One wave per token: lane l takes the 8 features 8 (l + 64 i)
// .. + 7 (one 16-byte load) with their 24 weights (six 16-byte loads), three fp32 accumulators, three wave sums; every lane then
// holds the token's colour and the lanes store the token's block of pixels -- the pixels y, x with y g // oh, x g // ow = the token.
__global__ void __launch_bounds__(THREADS) feature_render_kernel(const bf16_t* __restrict__ feat, const float* __restrict__ Wm,
                                                                 uint8_t* __restrict__ out, int64_t tokens, int g, int D, int oh, int ow,
                                                                 float b0, float b1, float b2, float lo0, float lo1, float lo2,
                                                                 float hi0, float hi1, float hi2) {
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (tok >= tokens) return;                         // wave-uniform
  const bf16_t* x = feat + tok * D;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int d = lane * 8; d < D; d += 64 * 8) {
    const uint4 raw = *reinterpret_cast<const uint4*>(x + d);
    const float4* wp = reinterpret_cast<const float4*>(Wm + (int64_t)d * 3);
    const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3], w4 = wp[4], w5 = wp[5];
    const float f0 = __uint_as_float(raw.x << 16), f1 = __uint_as_float(raw.x & 0xffff0000u);
    const float f2 = __uint_as_float(raw.y << 16), f3 = __uint_as_float(raw.y & 0xffff0000u);
    const float f4 = __uint_as_float(raw.z << 16), f5 = __uint_as_float(raw.z & 0xffff0000u);
    const float f6 = __uint_as_float(raw.w << 16), f7 = __uint_as_float(raw.w & 0xffff0000u);
    a0 += f0 * w0.x; a1 += f0 * w0.y; a2 += f0 * w0.z;
    a0 += f1 * w0.w; a1 += f1 * w1.x; a2 += f1 * w1.y;
    a0 += f2 * w1.z; a1 += f2 * w1.w; a2 += f2 * w2.x;
    a0 += f3 * w2.y; a1 += f3 * w2.z; a2 += f3 * w2.w;
    a0 += f4 * w3.x; a1 += f4 * w3.y; a2 += f4 * w3.z;
    a0 += f5 * w3.w; a1 += f5 * w4.x; a2 += f5 * w4.y;
    a0 += f6 * w4.z; a1 += f6 * w4.w; a2 += f6 * w5.x;
    a0 += f7 * w5.y; a1 += f7 * w5.z; a2 += f7 * w5.w;
  }
  a0 = wave_sum(a0) + b0; a1 = wave_sum(a1) + b1; a2 = wave_sum(a2) + b2;
  const uint8_t c0 = (uint8_t)level_u8(a0, lo0, hi0), c1 = (uint8_t)level_u8(a1, lo1, hi1), c2 = (uint8_t)level_u8(a2, lo2, hi2);
  const int per = g * g;
  const int64_t n = tok / per;
  const int t = (int)(tok % per);
  const int ty = t / g, tx = t % g;
  // y g // oh == ty  <=>  ceil(ty oh / g) <= y < ceil((ty + 1) oh / g)
  const int y0 = (int)(((int64_t)ty * oh + g - 1) / g), y1 = (int)(((int64_t)(ty + 1) * oh + g - 1) / g);
  const int x0 = (int)(((int64_t)tx * ow + g - 1) / g), x1 = (int)(((int64_t)(tx + 1) * ow + g - 1) / g);
  const int bw = x1 - x0, count = (y1 - y0) * bw;
  for (int i = lane; i < count; i += 64) {
    uint8_t* dst = out + ((n * oh + y0 + i / bw) * (int64_t)ow + x0 + i % bw) * 3;
    dst[0] = c0; dst[1] = c1; dst[2] = c2;
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool grid_ok(int64_t blocks) { return blocks <= (int64_t)0x7fffffff; }
inline bool byte_ok(int32_t v) { return v >= 0 && v <= 255; }
inline int isqrt_exact(int64_t v) {                   // the side of a square grid of v cells, or -1
  if (v < 1 || v > (int64_t)1 << 30) return -1;
  int s = (int)(sqrt((double)v) + 0.5);
  return (int64_t)s * s == v ? s : -1;
}

}  // namespace

extern "C" int64_t dvla_depth_range_partial_len(int64_t n, int32_t height, int32_t width) {
  if (n < 0 || height < 1 || width < 1) return 0;
  const int64_t hw = (int64_t)height * width;
  const int chunk = range_chunk(hw);
  return n * ((hw + chunk - 1) / chunk) * 2;
}

extern "C" int dvla_depth_colorize(const float* depth, uint8_t* out, int64_t n, int32_t height, int32_t width,
                                   const uint8_t* palette, int32_t own_range, float lo, float hi, int32_t nan_r, int32_t nan_g,
                                   int32_t nan_b, void* partial, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!depth || !out || !palette || n < 0 || height < 1 || width < 1 || !byte_ok(nan_r) || !byte_ok(nan_g) || !byte_ok(nan_b))
    return DVLA_ERR_ARG;
  if (own_range ? !partial : !(lo <= hi && fabsf(lo) < INFINITY && fabsf(hi) < INFINITY)) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (misaligned(depth, 4) || (own_range && misaligned(partial, 4)) || n > 65535) return DVLA_ERR_UNSUPPORTED;
  const int64_t hw = (int64_t)height * width;
  const int chunk = range_chunk(hw);
  const int64_t chunks = (hw + chunk - 1) / chunk;
  const int64_t blocks = (hw + THREADS * 4 - 1) / (THREADS * 4);
  if (!grid_ok(blocks) || !grid_ok(chunks)) return DVLA_ERR_UNSUPPORTED;
  float* part = own_range ? reinterpret_cast<float*>(partial) : nullptr;
  if (own_range) {
    hipLaunchKernelGGL(depth_range_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(THREADS), 0, stream, depth, part, hw, chunk,
                       (int)chunks);
    if (dvla_check_launch() != DVLA_OK) return DVLA_ERR_LAUNCH;
  }
  const uint32_t nan_rgb = (uint32_t)nan_r | ((uint32_t)nan_g << 8) | ((uint32_t)nan_b << 16);
  const dim3 grid((unsigned)blocks, (unsigned)n), block(THREADS);
  if (hw % 4 == 0 && !misaligned(depth, 16) && !misaligned(out, 4))
    hipLaunchKernelGGL(depth_colorize_kernel<true>, grid, block, 0, stream, depth, out, palette, part, hw, (int)chunks, lo, hi, nan_rgb);
  else
    hipLaunchKernelGGL(depth_colorize_kernel<false>, grid, block, 0, stream, depth, out, palette, part, hw, (int)chunks, lo, hi, nan_rgb);
  return dvla_check_launch();
}

extern "C" int dvla_flow_unshuffle(const void* pred, float* flow, int64_t n, int32_t tokens, int32_t factor, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!pred || !flow || n < 0 || tokens < 1 || factor < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  const int g = isqrt_exact(tokens);
  if (g < 0 || (factor != 1 && factor != 2 && factor != 4) || misaligned(pred, 2) || misaligned(flow, 8)) return DVLA_ERR_UNSUPPORTED;
  const int64_t cells = n * tokens * factor * factor;
  const int64_t blocks = (cells + THREADS - 1) / THREADS;
  if (!grid_ok(blocks)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(flow_unshuffle_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, reinterpret_cast<const bf16_t*>(pred),
                     flow, cells, g, (int)factor);
  return dvla_check_launch();
}

extern "C" int dvla_flow_wheel(const float* flow, uint8_t* out, int64_t n, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                               void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!flow || !out || n < 0 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (misaligned(flow, 8)) return DVLA_ERR_UNSUPPORTED;
  const bool vec = out_w % 4 == 0 && !misaligned(out, 4);
  const int64_t items = n * out_h * (int64_t)(vec ? out_w / 4 : out_w);
  const int64_t blocks = (items + THREADS - 1) / THREADS;
  if (!grid_ok(blocks)) return DVLA_ERR_UNSUPPORTED;
  if (vec)
    hipLaunchKernelGGL(flow_wheel_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, stream, flow, out, items, in_h, in_w, out_h, out_w);
  else
    hipLaunchKernelGGL(flow_wheel_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, stream, flow, out, items, in_h, in_w, out_h, out_w);
  return dvla_check_launch();
}

extern "C" int dvla_motion_mask(const void* pred, uint8_t* mask, int64_t n, int32_t tokens, int32_t factor, float thr, int32_t dilate,
                                void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!pred || !mask || n < 0 || tokens < 1 || factor < 1 || !(thr >= 0.f) || !(thr < INFINITY)) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  const int g = isqrt_exact(tokens);
  if (g < 0 || (factor != 1 && factor != 2 && factor != 4) || misaligned(pred, 2)) return DVLA_ERR_UNSUPPORTED;
  const int64_t total = n * tokens;
  const int64_t blocks = (total + THREADS - 1) / THREADS;
  if (!grid_ok(blocks)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(motion_mask_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, reinterpret_cast<const bf16_t*>(pred), mask,
                     total, g, (int)(factor * factor), thr, dilate ? 1 : 0);
  return dvla_check_launch();
}

extern "C" int dvla_motion_overlay(const uint8_t* mask, const void* current, uint8_t* out, int64_t n, int32_t grid, int32_t height,
                                   int32_t width, float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b,
                                   int32_t tint_r, int32_t tint_g, int32_t tint_b, int32_t alpha, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!mask || !current || !out || n < 0 || grid < 1 || height < 1 || width < 1 || !byte_ok(tint_r) || !byte_ok(tint_g) ||
      !byte_ok(tint_b) || alpha < 0 || alpha > 256)
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (height % grid || width % grid || width % 4 || misaligned(current, 8) || misaligned(out, 4)) return DVLA_ERR_UNSUPPORTED;
  const int64_t items = n * height * (int64_t)(width / 4);
  const int64_t blocks = (items + THREADS - 1) / THREADS;
  if (!grid_ok(blocks)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(motion_overlay_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, reinterpret_cast<const bf16_t*>(current),
                     mask, out, items, height, width, grid, mean_r, mean_g, mean_b, std_r, std_g, std_b, tint_r, tint_g, tint_b, alpha);
  return dvla_check_launch();
}

extern "C" int dvla_feature_render(const void* feat, const float* proj, uint8_t* out, int64_t n, int32_t tokens, int32_t dim,
                                   int32_t out_h, int32_t out_w, float b0, float b1, float b2, float lo0, float lo1, float lo2,
                                   float hi0, float hi1, float hi2, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!feat || !proj || !out || n < 0 || tokens < 1 || dim < 1 || out_h < 1 || out_w < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  const int g = isqrt_exact(tokens);
  if (g < 0 || dim % 8 != 0 || misaligned(feat, 16) || misaligned(proj, 16)) return DVLA_ERR_UNSUPPORTED;
  const int64_t total = n * tokens;
  const int64_t blocks = (total + THREADS / 64 - 1) / (THREADS / 64);
  if (!grid_ok(blocks)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(feature_render_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, reinterpret_cast<const bf16_t*>(feat), proj,
                     out, total, g, (int)dim, (int)out_h, (int)out_w, b0, b1, b2, lo0, lo1, lo2, hi0, hi1, hi2);
  return dvla_check_launch();
}
