// depth_pipeline.hip -- depth labels: raw fp32 depth maps -> nearest resize -> RandomShiftsAug -> bf16 / fp32 (n, out_h, out_w),
// one pass.  The depth sibling of input_pipeline.hip.
//
// The reference does this on the host, frame by frame, in the collator: `depth_image_fn` (utils/data_utils.py:3588-3607) stacks
// the maps and resizes them with torchvision's Resize(NEAREST) on a tensor = F.interpolate(mode="nearest"); on the traj_cons path
// RandomShiftsAug follows (a pure gather, see input_pipeline.hip) and the training loop uploads 200 KB of fp32 per frame and casts.
// Here the raw map (160 KB / 28 KB per CALVIN frame) is what crosses PCIe and everything after it is this kernel:
//
//   out[i, y, x] = cast(src[i, ry(clamp(y + sy_i - pad, 0, out_h - 1)), rx(clamp(x + sx_i - pad, 0, out_w - 1))])
//   ry(j) = min(int(floorf(j * (float(src_h) / out_h))), src_h - 1), rx likewise: ATen's nearest source index, in fp32
//
// A gather composed with a gather: no arithmetic touches the values, the bf16 cast is the hardware's round-to-nearest-even.
// The two index tables (out_h + out_w entries) are computed once per workgroup into LDS; a workgroup then walks over
// (frame, block of rows) units, a thread producing 16 bytes (8 bf16 / 4 fp32 consecutive x) of one output row per item.  When the
// output rows are not 16-byte aligned (out_w not a multiple of the vector width, or `out` itself off a 16-byte boundary) every row
// gets a scalar head up to its first aligned element, the vector body, and a scalar tail.
#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_ITEMS = 1024;              // items (16-byte pieces) of one unit of work: four per thread
constexpr int DP_MAX_BLOCKS = 4096;         // the grid cap of the elementwise kernels (grid_for); the units beyond it are strided over
constexpr int DP_LDS_MAX = 64 * 1024;

struct DepthArgs {
  const float* src; const int32_t* shift; void* out;
  int64_t n, units;
  int32_t src_h, src_w, out_h, out_w, pad;
  int32_t rows_per_unit, tiles, chunks, lead, base_mod;   // lead = 1: rows have a scalar head (chunk 0); base_mod = (out / elem) % V
};

template <bool BF16>
__global__ __launch_bounds__(DP_THREADS) void depth_preprocess_kernel(const DepthArgs a) {
  constexpr int V = BF16 ? 8 : 4;
  extern __shared__ __attribute__((aligned(16))) int32_t tab[];
  int32_t* ry = tab;
  int32_t* rx = tab + a.out_h;
  {
    const float sy = (float)a.src_h / (float)a.out_h, sx = (float)a.src_w / (float)a.out_w;
    for (int j = threadIdx.x; j < a.out_h; j += DP_THREADS) {
      const int s = (int)floorf((float)j * sy);
      ry[j] = s < a.src_h - 1 ? s : a.src_h - 1;
    }
    for (int j = threadIdx.x; j < a.out_w; j += DP_THREADS) {
      const int s = (int)floorf((float)j * sx);
      rx[j] = s < a.src_w - 1 ? s : a.src_w - 1;
    }
  }
  __syncthreads();
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t frame = u / a.tiles;
    const int y0 = (int)(u - frame * a.tiles) * a.rows_per_unit;
    const int rows = y0 + a.rows_per_unit < a.out_h ? a.rows_per_unit : a.out_h - y0;
    int dx = 0, dy = 0;                       // no augmentation: the identity gather
    if (a.shift && a.pad > 0) { dx = a.shift[2 * frame] - a.pad; dy = a.shift[2 * frame + 1] - a.pad; }
    const float* img = a.src + frame * ((int64_t)a.src_h * a.src_w);
    const int items = rows * a.chunks;
    for (int it = threadIdx.x; it < items; it += DP_THREADS) {
      const int r = it / a.chunks, c = it - r * a.chunks;
      const int y = y0 + r;
      const int64_t row = frame * a.out_h + y;                 // output row index over all frames
      const int64_t row_elem = row * (int64_t)a.out_w;
      // elements in front of the row's first 16-byte aligned one
      const int head = a.lead ? (int)((V - (int)((a.base_mod + row_elem) % V)) % V) : 0;
      const int x0 = head + (c - a.lead) * V;
      int yy = y + dy; yy = yy < 0 ? 0 : (yy >= a.out_h ? a.out_h - 1 : yy);
      const float* line = img + (int64_t)ry[yy] * a.src_w;
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        int xx = x0 + e + dx; xx = xx < 0 ? 0 : (xx >= a.out_w ? a.out_w - 1 : xx);
        v[e] = line[rx[xx]];
      }
      const int lo = x0 < 0 ? 0 : x0, hi = x0 + V < a.out_w ? x0 + V : a.out_w;
      if constexpr (BF16) {
        bf16_t* dst = reinterpret_cast<bf16_t*>(a.out) + row_elem;
        if (hi - lo == V) {
          *reinterpret_cast<uint4*>(dst + x0) =
              make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (x0 + e >= lo && x0 + e < hi) dst[x0 + e] = f2bf(v[e]);
        }
      } else {
        float* dst = reinterpret_cast<float*>(a.out) + row_elem;
        if (hi - lo == V) {
          *reinterpret_cast<float4*>(dst + x0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (x0 + e >= lo && x0 + e < hi) dst[x0 + e] = v[e];
        }
      }
    }
  }
}

}  // namespace

extern "C" int dvla_depth_preprocess(const float* src, const int32_t* shift, void* out, int64_t n, int32_t src_h, int32_t src_w,
                                     int32_t out_h, int32_t out_w, int32_t pad, int32_t out_dtype, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!src || !out || n < 0 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || pad < 0) return DVLA_ERR_ARG;
  if (out_dtype != DVLA_DT_BF16 && out_dtype != DVLA_DT_F32) return DVLA_ERR_UNSUPPORTED;
  if (n == 0) return DVLA_OK;
  const int bf = out_dtype == DVLA_DT_BF16;
  const int V = bf ? 8 : 4, esize = bf ? 2 : 4;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(out);
  // both tables live in LDS; ATen forms the source index from float(size) and float(index): exact below 2^24; src / out
  // aligned to their element
  if (((int64_t)out_h + out_w) * 4 > DP_LDS_MAX || src_h > (1 << 24) || src_w > (1 << 24)) return DVLA_ERR_UNSUPPORTED;
  if ((addr & (esize - 1)) || (reinterpret_cast<uintptr_t>(src) & 3)) return DVLA_ERR_UNSUPPORTED;
  DepthArgs a;
  a.src = src; a.shift = shift; a.out = out; a.n = n;
  a.src_h = src_h; a.src_w = src_w; a.out_h = out_h; a.out_w = out_w; a.pad = pad;
  a.lead = (out_w % V == 0 && (addr & 15) == 0) ? 0 : 1;
  a.base_mod = (int32_t)((addr / esize) % V);
  a.chunks = a.lead ? (out_w + V - 1) / V + 1 : out_w / V;    // + 1: the head and the tail of a row are two partial pieces at most
  int rows = DP_ITEMS / a.chunks;
  rows = rows < 1 ? 1 : (rows > out_h ? out_h : rows);
  a.rows_per_unit = rows;
  a.tiles = (out_h + rows - 1) / rows;
  a.units = n * a.tiles;
  const int64_t blocks = a.units < DP_MAX_BLOCKS ? a.units : DP_MAX_BLOCKS;
  const size_t lds = ((size_t)out_h + out_w) * 4;
  if (bf)
    hipLaunchKernelGGL(depth_preprocess_kernel<true>, dim3((unsigned)blocks), dim3(DP_THREADS), lds, stream, a);
  else
    hipLaunchKernelGGL(depth_preprocess_kernel<false>, dim3((unsigned)blocks), dim3(DP_THREADS), lds, stream, a);
  return dvla_check_launch();
}
