// image_resized_crop.hip -- MAE pretraining from raw frames: RandomResizedCrop(n_px, BICUBIC) + RandomHorizontalFlip (+ ToTensor +
// Normalize + the bf16 cast) on uint8 HWC frames, one crop box PER FRAME, byte for byte what Pillow's crop -> resize -> transpose
// produces.
//
// The arithmetic is image_resize.hip's: Pillow's fixed point on Pillow's float64-built tables -- per output byte
// clip8((2^21 + sum_t in[first + t] * k[t]) >> 22)  in a signed 32-bit accumulator, the horizontal pass first, its result rounded to
// uint8, the vertical pass on those bytes; integer multiply-add, shift and clamp only on the resample path.  What differs is the
// geometry: the crop is cut out FIRST (the taps clip at the crop's edge, as torchvision's resized_crop on a PIL image does), so a
// frame with a (ch, cw) crop takes the tables of the size pairs (cw -> n_px) and (ch -> n_px), and every frame of a launch has its own.
// The tables of EVERY input size 1 .. max_size live in one device-resident store the caller builds once
// (dreamvla_amd/preprocess.py: _crop_table_store):
//   store[2 s], store[2 s + 1]   = (offset, ksize) of size s, s = 0 .. max_size (offset in int32 words from the store's base, even)
//   store[offset ..]             = bounds (n_px, 2) int32 = (first input index, tap count), then coefficients (n_px, ksize) int32
// and a frame's descriptor (top, left, ch, cw, flip) indexes it with ch and cw.  A size equal to n_px has the identity table.
//
// One launch.  A workgroup (4 waves) owns `tile` output rows of one frame, as in image_resize.hip:
//   phase 1  each wave takes crop rows r0 + wave, r0 + wave + 4, ... of the rows the tile's vertical taps touch: it copies the row's
//            needed column segment into its own LDS staging buffer (16-byte global loads on the aligned body, byte loads on the up
//            to 15 bytes in front of and behind it; a frame's `left` moves the segment to any alignment, so it is placed at its
//            global address mod 16 in LDS), then one lane per output pixel runs the horizontal taps and writes 3 bytes of the row's
//            image in `mid` -- at column n_px - 1 - x when the frame is flipped, so phase 2 knows nothing of the flip;
//   phase 2  after one barrier, the vertical taps from wide LDS reads of the `mid` rows:
//            uint8 HWC   a thread produces 16 consecutive bytes of an output row (one 16-byte store, byte stores when the output
//                        rows are not 16-byte aligned);
//            bf16 CHW    a thread produces 8 consecutive pixels of an output row, all three channels (24 bytes of `mid` per tap as
//                        three 8-byte reads: lanes 24 bytes apart cover all 64 banks once per 32 lanes), normalises them as
//                        preprocess_kernel does -- fp32: byte / 255, - mean, / std, one rounding to bf16 -- and stores 16 bytes
//                        per channel plane.
// LDS = rows x align16(3 n_px) for `mid` + 4 staging buffers, planned on the host for the LARGEST crop of the launch (the tile height
// is halved until the plan fits 64 KiB).  A frame whose box leaves the source, or whose crop is larger than the plan was made for,
// writes nothing.
#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int RC_THREADS = 256, RC_WAVES = RC_THREADS / 64;
constexpr int RC_TILE = 16;                 // output rows per workgroup (halved while the LDS plan exceeds RC_LDS_MAX)
constexpr int RC_LDS_MAX = 64 * 1024;       // dynamic LDS a launch may ask for without a function attribute

struct CropArgs {
  const uint8_t* src; void* out;
  const int32_t *crops, *store;
  int32_t src_h, src_w, max_size, n_px, out_bf16;
  int32_t tile, tiles, rows_cap, cols_cap, mid_stride, stage_stride, vec_out;
  float m0, m1, m2, s0, s1, s2;
};

__device__ __forceinline__ int clip8(int acc) {
  acc >>= 22;                               // arithmetic shift of the signed accumulator
  return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

__device__ __forceinline__ float normalise(int byte, float mean, float stdv) {
  const float t = (float)byte / 255.0f;     // ToTensor
  return (t - mean) / stdv;                 // Normalize: sub_, div_
}

__global__ __launch_bounds__(RC_THREADS) void image_resized_crop_kernel(const CropArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int64_t frame = blockIdx.x / a.tiles;
  const int y0 = (int)(blockIdx.x % a.tiles) * a.tile;
  const int y1 = y0 + a.tile < a.n_px ? y0 + a.tile : a.n_px;
  const int32_t* d = a.crops + frame * 5;
  const int top = d[0], left = d[1], ch = d[2], cw = d[3], flip = d[4];
  // a box that leaves the source, or a crop the store has no table for: write nothing
  if (top < 0 || left < 0 || ch < 1 || cw < 1 || ch > a.max_size || cw > a.max_size || ch > a.src_h - top || cw > a.src_w - left) return;
  const int32_t* bx = a.store + a.store[2 * cw];
  const int32_t* by = a.store + a.store[2 * ch];
  const int ksx = a.store[2 * cw + 1], ksy = a.store[2 * ch + 1];
  const int32_t *kx = bx + 2 * a.n_px, *ky = by + 2 * a.n_px;
  // the crop's rows under this tile's vertical taps and the crop's columns under the horizontal taps
  int r0 = ch, r1 = 0;
  for (int y = y0; y < y1; ++y) {
    const int b = by[2 * y], e = b + by[2 * y + 1];
    r0 = b < r0 ? b : r0;
    r1 = e > r1 ? e : r1;
  }
  int c0 = bx[0];
  int c1 = bx[2 * (a.n_px - 1)] + bx[2 * (a.n_px - 1) + 1];
  r0 = r0 < 0 ? 0 : r0;  r1 = r1 > ch ? ch : r1;
  c0 = c0 < 0 ? 0 : c0;  c1 = c1 > cw ? cw : c1;
  // more rows / columns than the launch's LDS plan holds (a crop larger than the plan's): write nothing
  if (r1 <= r0 || c1 <= c0 || r1 - r0 > a.rows_cap || c1 - c0 > a.cols_cap) return;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* st = lds + a.rows_cap * a.mid_stride + wave * a.stage_stride;
  const int seg = (c1 - c0) * 3;
  for (int r = r0 + wave; r < r1; r += RC_WAVES) {
    const uint8_t* g = a.src + ((frame * a.src_h + top + r) * (int64_t)a.src_w + left + c0) * 3;
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
      const int2 b = *reinterpret_cast<const int2*>(bx + 2 * x);
      const int32_t* k = kx + (int64_t)x * ksx;
      const uint8_t* p = st + o + (b.x - c0) * 3;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int t = 0; t < b.y; ++t) {
        const int c = k[t];
        s0 += (int)p[3 * t] * c;
        s1 += (int)p[3 * t + 1] * c;
        s2 += (int)p[3 * t + 2] * c;
      }
      const int xo = flip ? a.n_px - 1 - x : x;
      m[3 * xo] = (uint8_t)clip8(s0);
      m[3 * xo + 1] = (uint8_t)clip8(s1);
      m[3 * xo + 2] = (uint8_t)clip8(s2);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next row overwrites the staging buffer
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  if (!a.out_bf16) {
    uint8_t* out = reinterpret_cast<uint8_t*>(a.out);
    const int chunks = a.mid_stride >> 4, row_bytes = a.n_px * 3;
    const int items = (y1 - y0) * chunks;
    for (int it = threadIdx.x; it < items; it += RC_THREADS) {
      const int y = y0 + it / chunks, cx = it % chunks;
      const int2 b = *reinterpret_cast<const int2*>(by + 2 * y);
      const int32_t* k = ky + (int64_t)y * ksy;
      const uint8_t* col = lds + (b.x - r0) * a.mid_stride + cx * 16;
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
      uint8_t* dst = out + (frame * a.n_px + y) * (int64_t)row_bytes + cx * 16;
      if (a.vec_out) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (cx * 16 + i < row_bytes) dst[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
      }
    }
  } else {
    bf16_t* out = reinterpret_cast<bf16_t*>(a.out);
    const int octets = a.n_px >> 3;           // n_px % 8 == 0
    const int items = (y1 - y0) * octets;
    const int64_t plane = (int64_t)a.n_px * a.n_px;
    for (int it = threadIdx.x; it < items; it += RC_THREADS) {
      const int y = y0 + it / octets, ox = it % octets;
      const int2 b = *reinterpret_cast<const int2*>(by + 2 * y);
      const int32_t* k = ky + (int64_t)y * ksy;
      const uint8_t* col = lds + (b.x - r0) * a.mid_stride + ox * 24;
      int s[24];
#pragma unroll
      for (int i = 0; i < 24; ++i) s[i] = 1 << 21;
      for (int t = 0; t < b.y; ++t) {
        const uint2* p = reinterpret_cast<const uint2*>(col + t * a.mid_stride);
        const uint2 v0 = p[0], v1 = p[1], v2 = p[2];
        const int c = k[t];
        const uint32_t w[6] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y};
#pragma unroll
        for (int i = 0; i < 24; ++i) s[i] += (int)((w[i >> 2] >> (8 * (i & 3))) & 255u) * c;
      }
      bf16_t* dst = out + (frame * 3 * a.n_px + y) * (int64_t)a.n_px + ox * 8;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float mean = c == 0 ? a.m0 : (c == 1 ? a.m1 : a.m2), stdv = c == 0 ? a.s0 : (c == 1 ? a.s1 : a.s2);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = normalise(clip8(s[3 * e + c]), mean, stdv);
        *reinterpret_cast<uint4*>(dst + c * plane) =
            make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
      }
    }
  }
}

}  // namespace

extern "C" int dvla_image_resized_crop(const uint8_t* src, void* out, const int32_t* crops, const int32_t* table_store, int64_t n,
                                       int32_t src_h, int32_t src_w, int32_t max_size, int32_t max_ch, int32_t max_cw, int32_t n_px,
                                       int32_t out_kind, const float* mean3, const float* std3, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!src || !out || !crops || !table_store || n < 0 || src_h < 1 || src_w < 1 || max_size < 1 || max_ch < 1 || max_cw < 1 || n_px < 1 ||
      max_ch > src_h || max_cw > src_w || max_ch > max_size || max_cw > max_size ||
      (out_kind != DVLA_CROP_OUT_U8 && out_kind != DVLA_CROP_OUT_BF16) || (out_kind == DVLA_CROP_OUT_BF16 && (!mean3 || !std3)))
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (src_h > (1 << 20) || src_w > (1 << 20) || n_px > (1 << 14)) return DVLA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(table_store) & 7) || (reinterpret_cast<uintptr_t>(crops) & 3)) return DVLA_ERR_UNSUPPORTED;   // bounds are read as (first, count) pairs
  if (out_kind == DVLA_CROP_OUT_BF16 && (n_px % 8 != 0 || (reinterpret_cast<uintptr_t>(out) & 15))) return DVLA_ERR_UNSUPPORTED;
  CropArgs a;
  a.src = src; a.out = out; a.crops = crops; a.store = table_store;
  a.src_h = src_h; a.src_w = src_w; a.max_size = max_size; a.n_px = n_px; a.out_bf16 = out_kind == DVLA_CROP_OUT_BF16 ? 1 : 0;
  a.m0 = a.m1 = a.m2 = 0.f; a.s0 = a.s1 = a.s2 = 1.f;
  if (a.out_bf16) { a.m0 = mean3[0]; a.m1 = mean3[1]; a.m2 = mean3[2]; a.s0 = std3[0]; a.s1 = std3[1]; a.s2 = std3[2]; }
  a.mid_stride = (n_px * 3 + 15) & ~15;
  a.cols_cap = max_cw;                                         // the horizontal taps of a whole output row span the whole crop row
  a.stage_stride = (a.cols_cap * 3 + 16 + 15) & ~15;           // + 16: the segment sits at its global address mod 16
  // the vertical taps of `tile` output rows of a crop `ch` rows high span at most ceil((tile - 1) ch / n_px) + ksize(ch) crop rows,
  // ksize(ch) = 2 ceil(2 max(ch / n_px, 1)) + 1; both terms grow with ch, so the launch's largest crop bounds every frame's
  const int64_t ks = 2 * (max_ch > n_px ? (2 * (int64_t)max_ch + n_px - 1) / n_px : 2) + 1;
  int64_t lds = 0;
  for (a.tile = RC_TILE; a.tile >= 1; a.tile >>= 1) {
    const int64_t rows = ((int64_t)(a.tile - 1) * max_ch + n_px - 1) / n_px + ks;
    a.rows_cap = (int32_t)(rows < max_ch ? rows : max_ch);
    lds = (int64_t)a.rows_cap * a.mid_stride + (int64_t)RC_WAVES * a.stage_stride;
    if (lds <= RC_LDS_MAX) break;
  }
  if (a.tile < 1) return DVLA_ERR_UNSUPPORTED;
  a.tiles = (n_px + a.tile - 1) / a.tile;
  if (n * a.tiles > 0x7fffffffLL) return DVLA_ERR_UNSUPPORTED;
  a.vec_out = ((n_px * 3) % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(image_resized_crop_kernel, dim3((unsigned)(n * a.tiles)), dim3(RC_THREADS), (size_t)lds, stream, a);
  return dvla_check_launch();
}
