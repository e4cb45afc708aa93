// image_resize.hip -- raw camera frames: Resize(n_px, BICUBIC) + CenterCrop(n_px) of CLIP's image transform on uint8 HWC frames,
// byte for byte what Pillow's 8-bit resample produces.
//
// Pillow resamples 8-bit images in fixed point: per axis and per (input size, output size) a table of bounds (first tap, tap count)
// and 22-bit integer coefficients, then per output byte  clip8((2^21 + sum_t in[first + t] * k[t]) >> 22)  in a signed 32-bit
// accumulator, the horizontal pass first, ITS RESULT ROUNDED TO uint8, the vertical pass on those bytes.  The tables are built on the
// host in float64 (dreamvla_amd/preprocess.py: bicubic_tables) and arrive here as int32; this file holds integer multiply-add, shift
// and clamp only -- no floating point on the device -- so the result is Pillow's by construction, not to a tolerance.  A pass whose
// input and output size are equal is skipped by Pillow; the caller hands this kernel the identity table for it (one tap of 2^22,
// which the arithmetic above maps to the input byte exactly).
//
// One launch; the horizontally resampled rows never leave the CU.  A workgroup (4 waves) owns `tile` output rows of one frame:
//   phase 1  each wave takes source rows r0 + wave, r0 + wave + 4, ... of the rows the tile's vertical taps touch: it copies the
//            row's needed column segment into its own LDS staging buffer (16-byte global loads on the aligned body of the segment,
//            byte loads on the up to 15 bytes in front of and behind it: a 200 x 200 x 3 row is 600 bytes, so a row starts at any
//            alignment; the segment is placed at the same offset mod 16 in LDS, which keeps the 16-byte LDS stores aligned), then
//            one lane per output pixel runs the horizontal taps on the staged bytes and writes 3 bytes of the row's image in `mid`;
//   phase 2  after one barrier, a thread produces 16 consecutive bytes of an output row from 16-byte LDS reads of the `mid` rows
//            under its vertical taps and stores them with one 16-byte store (byte stores when the output rows are not 16-byte
//            aligned).
// LDS = rows x align16(3 n_px) for `mid` + 4 staging buffers; `rows` is bounded through the tile height (16 output rows, halved
// until the plan fits 64 KiB), not by the source size.
#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int RS_THREADS = 256, RS_WAVES = RS_THREADS / 64;
constexpr int RS_TILE = 16;                 // output rows per workgroup (halved while the LDS plan exceeds RS_LDS_MAX)
constexpr int RS_LDS_MAX = 64 * 1024;       // dynamic LDS a launch may ask for without a function attribute

struct ResizeArgs {
  const uint8_t* src; uint8_t* out;
  const int32_t *bx, *kx, *by, *ky;         // bounds (res, 2) and coefficients (res, ksize) of the two axes
  int32_t src_h, src_w, ksx, ksy, left, top, n_px;
  int32_t tile, tiles, rows_cap, cols_cap, mid_stride, stage_stride, vec_out;
};

__device__ __forceinline__ int clip8(int acc) {
  acc >>= 22;                               // arithmetic shift of the signed accumulator
  return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

__global__ __launch_bounds__(RS_THREADS) void image_resize_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int64_t frame = blockIdx.x / a.tiles;
  const int y0 = (int)(blockIdx.x % a.tiles) * a.tile;
  const int y1 = y0 + a.tile < a.n_px ? y0 + a.tile : a.n_px;
  // the source rows under this tile's vertical taps and the source columns under the cropped row's horizontal taps
  int r0 = a.src_h, r1 = 0;
  for (int y = y0; y < y1; ++y) {
    const int b = a.by[2 * (a.top + y)], e = b + a.by[2 * (a.top + y) + 1];
    r0 = b < r0 ? b : r0;
    r1 = e > r1 ? e : r1;
  }
  int c0 = a.bx[2 * a.left];
  int c1 = a.bx[2 * (a.left + a.n_px - 1)] + a.bx[2 * (a.left + a.n_px - 1) + 1];
  r0 = r0 < 0 ? 0 : r0;  r1 = r1 > a.src_h ? a.src_h : r1;
  c0 = c0 < 0 ? 0 : c0;  c1 = c1 > a.src_w ? a.src_w : c1;
  // tables that do not belong to these sizes (more rows / columns than the launch's LDS plan holds): write nothing
  if (r1 <= r0 || c1 <= c0 || r1 - r0 > a.rows_cap || c1 - c0 > a.cols_cap) return;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* st = lds + a.rows_cap * a.mid_stride + wave * a.stage_stride;
  const int seg = (c1 - c0) * 3;
  for (int r = r0 + wave; r < r1; r += RS_WAVES) {
    const uint8_t* g = a.src + ((frame * a.src_h + r) * (int64_t)a.src_w + c0) * 3;
    const int o = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    int head = (16 - o) & 15;
    head = head > seg ? seg : head;
    const int body = (seg - head) >> 4, tail0 = head + (body << 4);
    if (lane < head) st[o + lane] = g[lane];
    for (int v = lane; v < body; v += 64)
      *reinterpret_cast<uint4*>(st + o + head + 16 * v) = *reinterpret_cast<const uint4*>(g + head + 16 * v);
    if (lane < seg - tail0) st[o + tail0 + lane] = g[tail0 + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the staged row is read by other lanes of this wave only
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint8_t* m = lds + (r - r0) * a.mid_stride;
    for (int x = lane; x < a.n_px; x += 64) {
      const int2 b = *reinterpret_cast<const int2*>(a.bx + 2 * (a.left + x));
      const int32_t* k = a.kx + (int64_t)(a.left + x) * a.ksx;
      const uint8_t* p = st + o + (b.x - c0) * 3;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int t = 0; t < b.y; ++t) {
        const int c = k[t];
        s0 += (int)p[3 * t] * c;
        s1 += (int)p[3 * t + 1] * c;
        s2 += (int)p[3 * t + 2] * c;
      }
      m[3 * x] = (uint8_t)clip8(s0);
      m[3 * x + 1] = (uint8_t)clip8(s1);
      m[3 * x + 2] = (uint8_t)clip8(s2);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next row overwrites the staging buffer
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  const int chunks = a.mid_stride >> 4, row_bytes = a.n_px * 3;
  const int items = (y1 - y0) * chunks;
  for (int it = threadIdx.x; it < items; it += RS_THREADS) {
    const int y = y0 + it / chunks, ch = it % chunks;
    const int2 b = *reinterpret_cast<const int2*>(a.by + 2 * (a.top + y));
    const int32_t* k = a.ky + (int64_t)(a.top + y) * a.ksy;
    const uint8_t* col = lds + (b.x - r0) * a.mid_stride + ch * 16;
    int s[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 1 << 21;
    for (int t = 0; t < b.y; ++t) {
      const uint4 v = *reinterpret_cast<const uint4*>(col + t * a.mid_stride);
      const int c = k[t];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] += (int)((w[i >> 2] >> (8 * (i & 3))) & 255u) * c;
    }
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      q[i] = (uint32_t)clip8(s[4 * i]) | ((uint32_t)clip8(s[4 * i + 1]) << 8) | ((uint32_t)clip8(s[4 * i + 2]) << 16) |
             ((uint32_t)clip8(s[4 * i + 3]) << 24);
    uint8_t* dst = a.out + (frame * a.n_px + y) * (int64_t)row_bytes + ch * 16;
    if (a.vec_out) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (ch * 16 + i < row_bytes) dst[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
    }
  }
}

}  // namespace

extern "C" int dvla_image_resize_u8(const uint8_t* src, uint8_t* out, int64_t n, int32_t src_h, int32_t src_w, int32_t res_h,
                                    int32_t res_w, const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x,
                                    const int32_t* bounds_y, const int32_t* coef_y, int32_t ksize_y, int32_t crop_left,
                                    int32_t crop_top, int32_t n_px, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!src || !out || !bounds_x || !coef_x || !bounds_y || !coef_y || n < 0 || src_h < 1 || src_w < 1 || res_h < 1 || res_w < 1 ||
      ksize_x < 1 || ksize_y < 1 || n_px < 1 || crop_left < 0 || crop_top < 0 || (int64_t)crop_left + n_px > res_w ||
      (int64_t)crop_top + n_px > res_h)
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (src_h > (1 << 20) || src_w > (1 << 20) || n_px > (1 << 14) || ksize_x > (1 << 20) || ksize_y > (1 << 20)) return DVLA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(bounds_x) & 7) || (reinterpret_cast<uintptr_t>(bounds_y) & 7)) return DVLA_ERR_UNSUPPORTED;   // read as (first, count) pairs
  ResizeArgs a;
  a.src = src; a.out = out; a.bx = bounds_x; a.kx = coef_x; a.by = bounds_y; a.ky = coef_y;
  a.src_h = src_h; a.src_w = src_w; a.ksx = ksize_x; a.ksy = ksize_y; a.left = crop_left; a.top = crop_top; a.n_px = n_px;
  a.mid_stride = (n_px * 3 + 15) & ~15;
  // the taps of n_px output columns (of `tile` output rows) span at most ceil((count - 1) * scale) + ksize input columns (rows):
  // first tap >= centre - support - 1/2, last tap < centre + support + 1/2, ksize >= 2 support + 1
  const int64_t cols = ((int64_t)(n_px - 1) * src_w + res_w - 1) / res_w + ksize_x;
  a.cols_cap = (int32_t)(cols < src_w ? cols : src_w);
  a.stage_stride = (a.cols_cap * 3 + 16 + 15) & ~15;          // + 16: the segment sits at its global address mod 16
  int64_t lds = 0;
  for (a.tile = RS_TILE; a.tile >= 1; a.tile >>= 1) {
    const int64_t rows = ((int64_t)(a.tile - 1) * src_h + res_h - 1) / res_h + ksize_y;
    a.rows_cap = (int32_t)(rows < src_h ? rows : src_h);
    lds = (int64_t)a.rows_cap * a.mid_stride + (int64_t)RS_WAVES * a.stage_stride;
    if (lds <= RS_LDS_MAX) break;
  }
  if (a.tile < 1) return DVLA_ERR_UNSUPPORTED;
  a.tiles = (n_px + a.tile - 1) / a.tile;
  if (n * a.tiles > 0x7fffffffLL) return DVLA_ERR_UNSUPPORTED;
  a.vec_out = ((n_px * 3) % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(image_resize_kernel, dim3((unsigned)(n * a.tiles)), dim3(RS_THREADS), (size_t)lds, stream, a);
  return dvla_check_launch();
}
