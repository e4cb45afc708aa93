// dream.hip -- the policy's dreams at evaluation: the executed window position's query rows out of the trunk output, and the
// dream heads' patch predictions as displayable frames.  The mirror image of input_pipeline.hip (uint8 HWC -> normalised bf16 CHW).
//
// The image head is trained toward `normalize_patchfied_image(patchify(future frame))` (utils/train_utils.py:37-57, 783-799):
// patchify = 'nchpwq->nhwpqc' (the P*P*3 values of a patch in (p, q, c) order, channel last), then per patch
// (x - mean) / sqrt(var + 1e-6) with the unbiased variance over those values.  The future frame's statistics do not exist at
// evaluation; the render inverts the normalisation with the statistics of the SAME patch of the CURRENT frame (the model's own
// CLIP-normalised input), then inverts CLIP's Normalize, clamps to [0, 1], scales by 255 and rounds half-to-even:
//
//   x[c, y, x]   = pred[patch, (p, q, c)] * sqrt(var_cur(patch) + 1e-6) + mean_cur(patch)
//   out[y, x, c] = u8(rint(255 * clamp(x * std[c] + mean[c], 0, 1)))
//
// One wave per patch of 16 x 16 pixels: lane l owns the 4 pixels q = 4 (l % 4) .. + 3 of patch row p = l / 4, i.e. 4 C
// CONSECUTIVE values of the prediction (8-byte loads) and 4 C consecutive bytes of the HWC output row (4-byte stores); the
// current frame is read as 8-byte pieces of its CHW rows.  Both statistics are wave reductions over values held in registers
// (mean first, then the centred squares): nothing but the frame is written to HBM.
// HBM-bound: 2 B (pred) + 2 B (current) read and 1 B written per value.
#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int PATCH = 16;

__device__ __forceinline__ void unpack4(uint2 v, float (&f)[4]) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
}

// out[b, t, :] = x[b, sel[b], t0 + t, :]      x (B, S, T, H) bf16 contiguous, out (B, count, H); one thread per 8 values
__global__ void gather_positions_kernel(const bf16_t* __restrict__ x, const int64_t* __restrict__ sel, bf16_t* __restrict__ out,
                                        int B, int S, int T, int H, int t0, int count) {
  const int h8 = H / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * count * h8) return;
  const int c = (int)(idx % h8);
  const int t = (int)((idx / h8) % count);
  const int b = (int)(idx / ((int64_t)h8 * count));
  int64_t s = sel[b];
  s = s < 0 ? 0 : (s >= S ? S - 1 : s);           // an index outside the window never leaves the tensor
  const uint4 v = *reinterpret_cast<const uint4*>(x + (((int64_t)b * S + s) * T + t0 + t) * H + c * 8);
  *reinterpret_cast<uint4*>(out + ((int64_t)b * count + t) * H + c * 8) = v;
}

// pred (n, gh * gw, 768) bf16, cur (n, 3, 16 gh, 16 gw) bf16 -> out (n, 16 gh, 16 gw, 3) uint8
__global__ void __launch_bounds__(256) render_u8_kernel(const bf16_t* __restrict__ pred, const bf16_t* __restrict__ cur,
                                                        uint8_t* __restrict__ out, int64_t patches, int gh, int gw,
                                                        float m0, float m1, float m2, float s0, float s1, float s2) {
  const int lane = threadIdx.x & 63;
  const int64_t patch = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (patch >= patches) return;                     // wave-uniform
  const int per = gh * gw;
  const int64_t n = patch / per;
  const int g = (int)(patch % per);
  const int py = g / gw, px = g % gw;
  const int W = gw * PATCH, Hh = gh * PATCH;
  const int p = lane >> 2, q0 = (lane & 3) * 4;
  const int y = py * PATCH + p, x0 = px * PATCH + q0;

  float c[3][4];                                    // current frame: [channel][pixel]
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    unpack4(*reinterpret_cast<const uint2*>(cur + ((n * 3 + ch) * Hh + y) * (int64_t)W + x0), c[ch]);
  float part = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int e = 0; e < 4; ++e) part += c[ch][e];
  const float mean = wave_sum(part) * (1.0f / (PATCH * PATCH * 3));
  part = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = c[ch][e] - mean; part += d * d; }
  const float var = wave_sum(part) * (1.0f / (PATCH * PATCH * 3 - 1));      // torch.var: unbiased
  const float sd = sqrtf(var + 1.e-6f);

  float v[12];                                      // prediction: (pixel, channel), channel fastest
  const bf16_t* src = pred + patch * (PATCH * PATCH * 3) + lane * 12;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float f[4];
    unpack4(*reinterpret_cast<const uint2*>(src + 4 * j), f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * j + e] = f[e];
  }
  uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const int ch = i % 3;
    const float xs = v[i] * sd + mean;                                        // the frame in the model's input space
    const float cm = ch == 0 ? m0 : (ch == 1 ? m1 : m2), cs = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
    float t = xs * cs + cm;                                                   // CLIP Normalize inverted: [0, 1]
    t = fminf(fmaxf(t, 0.f), 1.f);
    w[i >> 2] |= (uint32_t)rintf(t * 255.0f) << (8 * (i & 3));
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + ((n * Hh + y) * (int64_t)W + x0) * 3);
  dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
}

// un-patchify only: pred (n, gh * gw, 256 C) bf16 in (p, q, c) order -> out (n, C, 16 gh, 16 gw) fp32
template <int C>
__global__ void __launch_bounds__(256) unpatchify_f32_kernel(const bf16_t* __restrict__ pred, float* __restrict__ out,
                                                             int64_t patches, int gh, int gw) {
  const int lane = threadIdx.x & 63;
  const int64_t patch = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (patch >= patches) return;
  const int per = gh * gw;
  const int64_t n = patch / per;
  const int g = (int)(patch % per);
  const int py = g / gw, px = g % gw;
  const int W = gw * PATCH, Hh = gh * PATCH;
  const int p = lane >> 2, q0 = (lane & 3) * 4;
  const int y = py * PATCH + p, x0 = px * PATCH + q0;
  float v[4 * C];
  const bf16_t* src = pred + patch * (PATCH * PATCH * C) + lane * (4 * C);
#pragma unroll
  for (int j = 0; j < C; ++j) {
    float f[4];
    unpack4(*reinterpret_cast<const uint2*>(src + 4 * j), f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * j + e] = f[e];
  }
#pragma unroll
  for (int ch = 0; ch < C; ++ch)
    *reinterpret_cast<float4*>(out + ((n * C + ch) * Hh + y) * (int64_t)W + x0) =
        make_float4(v[ch], v[C + ch], v[2 * C + ch], v[3 * C + ch]);
}

}  // namespace

extern "C" int dvla_gather_positions(const void* x, const int64_t* sel, void* out, int32_t B, int32_t S, int32_t T, int32_t H,
                                     int32_t tok_begin, int32_t tok_count, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!x || !sel || !out || B < 0 || S < 1 || T < 1 || H < 1 || tok_begin < 0 || tok_count < 0 || tok_begin + (int64_t)tok_count > T)
    return DVLA_ERR_ARG;
  if (B == 0 || tok_count == 0) return DVLA_OK;
  if (H % 8 != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15)) return DVLA_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)B * tok_count * (H / 8);
  hipLaunchKernelGGL(gather_positions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const bf16_t*>(x), sel, reinterpret_cast<bf16_t*>(out), B, S, T, H, tok_begin, tok_count);
  return dvla_check_launch();
}

extern "C" int dvla_dream_render(const void* pred, const void* current, void* out, int64_t n, int32_t grid_h, int32_t grid_w,
                                 int32_t patch, int32_t channels, const float* mean3, const float* std3, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!pred || !out || n < 0 || grid_h < 1 || grid_w < 1 || patch < 1 || channels < 1 || (current && (!mean3 || !std3)))
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  // one wave per 16 x 16 patch, RGB or one channel; the frame with its statistics is RGB only
  if (patch != PATCH || (channels != 1 && channels != 3) || (current && channels != 3)) return DVLA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(pred) & 7) || (reinterpret_cast<uintptr_t>(out) & 15) ||
      (current && (reinterpret_cast<uintptr_t>(current) & 7)))
    return DVLA_ERR_UNSUPPORTED;
  const int64_t patches = n * grid_h * (int64_t)grid_w;
  if (patches > (int64_t)0x7fffffff * 4) return DVLA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((patches + 3) / 4)), block(256);
  const bf16_t* p = reinterpret_cast<const bf16_t*>(pred);
  if (current) {
    hipLaunchKernelGGL(render_u8_kernel, grid, block, 0, stream, p, reinterpret_cast<const bf16_t*>(current),
                       reinterpret_cast<uint8_t*>(out), patches, grid_h, grid_w, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                       std3[2]);
  } else if (channels == 3) {
    hipLaunchKernelGGL(unpatchify_f32_kernel<3>, grid, block, 0, stream, p, reinterpret_cast<float*>(out), patches, grid_h, grid_w);
  } else {
    hipLaunchKernelGGL(unpatchify_f32_kernel<1>, grid, block, 0, stream, p, reinterpret_cast<float*>(out), patches, grid_h, grid_w);
  }
  return dvla_check_launch();
}
