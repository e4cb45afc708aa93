// optimizer.hip -- gradient-norm clipping + AdamW over flat buffers (gfx950), HBM-bound.
//
// Replaces `torch.nn.utils.clip_grad_norm_` + `torch.optim.AdamW.step` of the training step (train.py / utils/train_utils.py in
// the reference: the caller's optimizer step).  Parameters, gradients and both moments live in flat
// buffers (the gradient buffers are the data-parallel communication buckets), so the whole step is a norm pass and one step
// launch per bucket instead of ~80 multi-tensor launches.
//
// The norm: dvla_sumsq_bf16 / _f32, a deterministic two-stage fp32 sum of squares into one device scalar (one clip norm can span
// bf16 and fp32 buckets) or into one slot per bucket; dvla_step_verdict (one wave) adds the slots, decides whether the step is
// applied (the total is finite), counts, and picks the bias-correction scalars of the step count that is then current from a
// table the host derived (dvla_step_candidates) for every count still possible.
//
// The step: one kernel template per precision; every dvla_adamw_* entry point launches an instance.
//   adamw_kernel<GUARD, EMA, MAP, CLIP, SR>     bf16 parameters, gradients and moments, math in fp32: torch's fused AdamW with
//       bf16 parameters and clip_grad_norm_ (the scaled gradient rounded to bf16); 2 (g) + 3 x (2 + 2) (p, m, v) = 14 B / parameter
//   adamw_master_kernel<GUARD, EMA, MAP, CLIP>  fp32 masters (the shipped `--precision fp32` runs): clip in fp32 + torch's foreach
//       AdamW restated operation for operation, and the bf16 compute shadow of the new master: 4 + 3 x (4 + 4) + 2 = 30 B / parameter
//   A flag that is off folds away with `if constexpr`, and its arguments do not travel to the kernel:
//     GUARD  verdict and step-dependent scalars come from the dvla_step_state; a skipped step moves no byte
//     EMA    one more fp32 stream, e <- lerp(e, p, w) on the parameter as stored (ATen's lerp, bit for bit): + 8 B / parameter
//     MAP    a group map gives every vector of 8 elements its group's lr and weight decay (one byte; 255, or any id >= n_groups:
//            nothing of the vector is read or written); without it one group covers all n elements
//     CLIP   (with MAP) a clip coefficient per group from the groups' sums of squares, instead of one per launch
//     SR     (bf16) the three stores rounded stochastically from counter-based random bits instead of to nearest
//   An element's arithmetic does not depend on the flags: one element function per precision (adam_one, master_one) with every
//   rounding written out, so every instance gives the plain instance's bits wherever their inputs agree.
//
// Around it: dvla_ema_swap_f32 / _bf16 (the EMA becomes the weights and back, for evaluation) and dvla_sr_cast_f32_to_bf16.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "../../include/dvla.h"

namespace {

constexpr int SS_BLOCKS = 1024;

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const bf16_t* __restrict__ x, int64_t n, float* __restrict__ partial) {
  __shared__ float red[4];
  const int64_t nvec = n >> 3;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const uint4 u = reinterpret_cast<const uint4*>(x)[i];
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = bf2f((bf16_t)(w[k] & 0xffff)), b = bf2f((bf16_t)(w[k] >> 16));
      s = fmaf(a, a, s); s = fmaf(b, b, s);
    }
  }
  if (blockIdx.x == 0)   // ragged tail (n % 8 elements)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < n; i += 256) { const float a = bf2f(x[i]); s = fmaf(a, a, s); }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ out,
                                                          int accumulate) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = red[0] + red[1] + red[2] + red[3];
    out[0] = accumulate ? out[0] + t : t;
  }
}

__global__ __launch_bounds__(256) void sumsq_f32_partial_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ partial) {
  __shared__ float red[4];
  const int64_t nvec = n >> 2;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const float4 u = reinterpret_cast<const float4*>(x)[i];
    s = fmaf(u.x, u.x, s); s = fmaf(u.y, u.y, s); s = fmaf(u.z, u.z, s); s = fmaf(u.w, u.w, s);
  }
  if (blockIdx.x == 0)   // ragged tail (n % 4 elements)
    for (int64_t i = (nvec << 2) + threadIdx.x; i < n; i += 256) { const float a = x[i]; s = fmaf(a, a, s); }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the verdict of a guarded step (dvla.h: dvla_step_state) ----------------------------------------------------------------
struct VerdictArgs {
  const float* slots; int n; float* out; dvla_step_state* st; int64_t confirmed; int n_cand;
  dvla_step_scalars c[DVLA_STEP_MAX_CANDIDATES];      // by value: no upload, no pointer to chase
};

// One wave.  Lane 0 adds the per-bucket sums in index order (the order of the `accumulate` chain of dvla_sumsq_*, so the
// total has the same bits), decides, picks the candidate scalars and moves the counters; all lanes latch the slots of a skip.
__global__ __launch_bounds__(64) void step_verdict_kernel(VerdictArgs a) {
  __shared__ float slot[DVLA_STEP_MAX_BUCKETS];
  __shared__ int verdict;
  for (int i = threadIdx.x; i < a.n; i += 64) slot[i] = a.slots[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = slot[0];
    for (int i = 1; i < a.n; ++i) t = t + slot[i];
    int ok = (__float_as_uint(t) & 0x7f800000u) != 0x7f800000u;      // finite: exponent not all ones
    const int64_t j = a.st->applied - a.confirmed;
    dvla_step_scalars s = a.c[0];
#pragma unroll
    for (int k = 1; k < DVLA_STEP_MAX_CANDIDATES; ++k)               // compare-and-select: a.c[j] would go through scratch
      if (j == k) s = a.c[k];
    if (j < 0 || j >= a.n_cand) {                                    // the host's window does not cover this step
      ok = 0;
      a.st->faults += 1;
    } else {
      a.st->cand = (int32_t)j;
      a.st->inv_bc1 = s.inv_bc1; a.st->inv_bc2_sqrt = s.inv_bc2_sqrt; a.st->bc2_sqrt = s.bc2_sqrt; a.st->step_size = s.step_size;
    }
    a.out[0] = t;
    a.st->sumsq = t;
    a.st->ok = ok;
    a.st->applied += ok;
    a.st->skipped += !ok;
    if (!ok) { a.st->n_latched = a.n; a.st->latched_step = a.st->applied + a.st->skipped; }
    verdict = ok;
  }
  __syncthreads();
  if (!verdict)
    for (int i = threadIdx.x; i < a.n; i += 64) a.st->skipped_bucket_sumsq[i] = slot[i];
}

// ---- kernel arguments: a core per precision + one part per flag ---------------------------------------------------------------
struct AdamArgs {      // bf16; lr and wd: the one group's (MAP: from the table instead)
  bf16_t* p; const bf16_t* g; bf16_t* m; bf16_t* v; int64_t n;
  float lr, beta1, beta2, eps, wd, inv_bc1, inv_bc2_sqrt;      // GUARD: inv_bc1 and inv_bc2_sqrt come from the state
  const float* sumsq; float max_norm;                          // the one clip of the launch; sumsq null: none
};

// fp32 masters.  Scalars derived on the host exactly as torch/optim/adam.py derives them from the Python (double)
// hyper-parameters, then handed to the element-wise ops as fp32 (the foreach kernels' opmath scalars).
struct MasterArgs {
  float* p; const float* g; float* m; float* v; bf16_t* sh; int64_t n;
  float decay;        // 1 - lr * wd                      (_foreach_mul_(params, 1 - lr * weight_decay))     MAP: from the table
  float w1;           // 1 - beta1                        (_foreach_lerp_(exp_avgs, grads, 1 - beta1))
  int w1_small;       // |w1| < 0.5: ATen lerp's branch
  float beta2, omb2;  // beta2, 1 - beta2                 (_foreach_mul_(exp_avg_sqs, beta2); _foreach_addcmul_(.., g, g, 1 - beta2))
  float bc2_sqrt;     // sqrt(1 - beta2^step)             (_foreach_div_(sqrt(v), bc2_sqrt))                 GUARD: from the state
  float eps;          //                                  (_foreach_add_(.., eps))
  float step_size;    // -lr / (1 - beta1^step)           (_foreach_addcdiv_(params, m, denom, step_size))   GUARD / MAP: state / table
  const float* sumsq; float max_norm;
};

struct GuardPart { const dvla_step_state* st; };
// the EMA weights of every step count still possible, by value like VerdictArgs::c; the verdict's row (st->cand) is used
struct EmaTable { float w[DVLA_STEP_MAX_CANDIDATES]; };
template <bool GUARD> struct EmaPart { float* e; float w; };
template <> struct EmaPart<true> { float* e; EmaTable wt; };
// What depends on the group travels by value, as VerdictArgs::c does; wave 0 puts one row per group into LDS (constant indices
// only: a lane-varying index into a by-value array goes through scratch; the candidate row is wave-uniform and picked by
// compare-and-select), and every vector looks its row up by its map byte.
template <int NC>
struct MapPart {                    // master: x = decay, y = step_size per candidate count.  bf16: x = lr, y[0] = wd (NC = 1)
  const uint8_t* map; int n_groups;
  float x[DVLA_STEP_MAX_GROUPS], y[NC][DVLA_STEP_MAX_GROUPS];
};

// the groups' sums of squares stay in device memory, their max_norm travel by value (<= 0 or NaN: the group is not clipped)
struct ClipPart { const float* group_sumsq; float group_max_norm[DVLA_STEP_MAX_GROUPS]; };
struct SrPart { uint64_t seed; int64_t step, base; uint32_t bucket; };      // step: unguarded; base: the index of element 0

// A part whose flag is off is an empty base class and takes no room in the argument block.
template <bool ON, class T> struct Opt : T {};
template <class T> struct Opt<false, T> {};
template <class Core, int NC, bool GUARD, bool EMA, bool MAP, bool CLIP, bool SR>
struct StepArgs : Core, Opt<GUARD, GuardPart>, Opt<EMA, EmaPart<GUARD>>, Opt<MAP, MapPart<NC>>, Opt<CLIP, ClipPart>,
                  Opt<SR, SrPart> {
  static_assert(MAP || !CLIP, "a coefficient per group needs the group map");
};
template <bool GUARD, bool EMA, bool MAP, bool CLIP, bool SR> using Bf16StepArgs = StepArgs<AdamArgs, 1, GUARD, EMA, MAP, CLIP, SR>;
template <bool GUARD, bool EMA, bool MAP, bool CLIP>
using MasterStepArgs = StepArgs<MasterArgs, GUARD ? DVLA_STEP_MAX_CANDIDATES : 1, GUARD, EMA, MAP, CLIP, false>;
static_assert(sizeof(Bf16StepArgs<false, false, false, false, false>) == sizeof(AdamArgs) &&
              sizeof(MasterStepArgs<false, false, false, false>) == sizeof(MasterArgs), "the plain instances carry the core alone");

// ---- what the two kernels share ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float clip_coef(const float* sumsq, float max_norm) {
  if (!sumsq) return 1.0f;
  const float c = max_norm / (sqrtf(sumsq[0]) + 1e-6f);
  return c < 1.0f ? c : 1.0f;
}

template <int NC>
__device__ __forceinline__ float2 group_row(const MapPart<NC>& t, int cand) {      // the row of group threadIdx.x
  float x = 0.f, y = 0.f;
#pragma unroll
  for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) {
    if (g >= t.n_groups) break;                                      // uniform: two or three groups cost two or three rounds
    float yg = t.y[0][g];
#pragma unroll
    for (int k = 1; k < NC; ++k)
      if (cand == k) yg = t.y[k][g];
    if ((int)threadIdx.x == g) { x = t.x[g]; y = yg; }
  }
  return make_float2(x, y);
}

// the coefficient of group threadIdx.x; `off` for a group that is not clipped (its sum is not read)
__device__ __forceinline__ float group_coef(const ClipPart& c, int n_groups, float off) {
  float mx = 0.f;
#pragma unroll
  for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) {
    if (g >= n_groups) break;                                        // uniform, as in group_row
    if ((int)threadIdx.x == g) mx = c.group_max_norm[g];
  }
  return mx > 0.f ? clip_coef(c.group_sumsq + threadIdx.x, mx) : off;
}

// e <- lerp(e, p, w) as ATen's lerp computes it (the expression master_one restates for exp_avg)
struct Ema { float* e; float w, omw; int w_small; };        // omw = 1 - w in fp32, w_small = |w| < 0.5: lerp's branch
__device__ __forceinline__ float ema_pick(const EmaTable& t, int cand) {
  float w = t.w[0];
#pragma unroll
  for (int k = 1; k < DVLA_STEP_MAX_CANDIDATES; ++k)                 // compare-and-select: t.w[cand] would go through scratch
    if (cand == k) w = t.w[k];
  return w;
}
__device__ __forceinline__ Ema ema_of(const EmaPart<false>& a, int) { return {a.e, a.w, 1.0f - a.w, fabsf(a.w) < 0.5f}; }
__device__ __forceinline__ Ema ema_of(const EmaPart<true>& a, int cand) {
  const float w = ema_pick(a.wt, cand);
  return {a.e, w, 1.0f - w, fabsf(w) < 0.5f};
}
__device__ __forceinline__ void ema_one(float& e, float p, const Ema& x) {
  const float d = __fsub_rn(p, e);
  e = x.w_small ? fmaf(x.w, d, e) : fmaf(-d, x.omw, p);
}

// The generator and the rounding of SR as dvla.h states them (tests/sr_ref.py restates both in integer arithmetic): 16 random bits
// per stored value from two hashes per element, keyed by (seed, applied step count, bucket) and the element's index in its bucket.
__device__ __forceinline__ uint32_t sr_bf16(uint32_t u, uint32_t r) {      // u: the fp32 bits, r: 16 random bits -> the bf16 bits
  if ((u & 0x7f800000u) == 0x7f800000u) return (u >> 16) | ((u & 0x007fffffu) ? 0x0040u : 0u);      // inf stays, NaN stays NaN
  return (u + r) >> 16;
}
__device__ __forceinline__ uint32_t sr_key(uint64_t seed, uint64_t step, uint32_t bucket) {
  uint32_t k = hash32((uint32_t)seed ^ 0x243F6A88u);
  k = hash32(k ^ (uint32_t)(seed >> 32));
  k = hash32(k ^ (uint32_t)step);
  k = hash32(k ^ (uint32_t)(step >> 32));
  return hash32(k ^ bucket);
}
__device__ __forceinline__ uint32_t sr_hash(uint32_t key, int64_t i) {
  return hash32((key ^ ((uint32_t)((uint64_t)i >> 32) * 0x85EBCA6Bu)) + (uint32_t)i * 0x9E3779B9u);
}
__device__ __forceinline__ uint32_t sr_draw(uint32_t h, int stream) {      // stream 0: param, 1: exp_avg, 2: exp_avg_sq
  return stream == 0 ? h >> 16 : stream == 1 ? h & 0xffffu : hash32(h ^ 0x5BD1E995u) >> 16;
}
// the three stores of element i
__device__ __forceinline__ void sr_round3(float p, float m, float v, uint32_t key, int64_t i, uint32_t& pb, uint32_t& mb,
                                          uint32_t& vb) {
  const uint32_t h = sr_hash(key, i);
  pb = sr_bf16(__float_as_uint(p), sr_draw(h, 0));
  mb = sr_bf16(__float_as_uint(m), sr_draw(h, 1));
  vb = sr_bf16(__float_as_uint(v), sr_draw(h, 2));
}

__global__ __launch_bounds__(256) void sr_cast_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int64_t n, uint64_t seed,
                                                      uint64_t step, uint32_t bucket, int stream, int64_t base) {
  const uint32_t key = sr_key(seed, step, bucket);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = (bf16_t)sr_bf16(__float_as_uint(x[i]), sr_draw(sr_hash(key, base + i), stream));
}

// ---- the bf16 step ------------------------------------------------------------------------------------------------------------
// One bf16 element, every rounding written out (nothing is contracted inside this function, so it gives the same bits wherever
// the compiler places it).  The two forms are what the first shipped kernel, plain C++ under the compiler's own contraction,
// computed in its vector loop and in its ragged-tail loop; checkpoints continue bit for bit across both:
//   vector loop: decay = fma(-lr, wd, 1), v = fma(beta2, v, ((1 - beta2) g) g), p = fma(decay, p, -((lr inv_bc1) (m / denom)))
//   tail loop:   decay = 1 - lr wd,       v = beta2 v + ((1 - beta2) g) g,     p = decay p - (lr inv_bc1) (m / denom)
// and in both g = bf16(g coef) (clip_grad_norm_ scales the bf16 gradient in place; coef 1 without a clip),
// m = fma(1 - beta1, g - m, m) (exp_avg.lerp_), denom = fma(sqrt(v), inv_bc2_sqrt, eps).
template <bool TAIL>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float lr, float wd, float coef) {
#pragma clang fp contract(off)
  g = bf2f(f2bf(g * coef));
  const float gg = ((1.0f - a.beta2) * g) * g, step = lr * a.inv_bc1;
  v = TAIL ? a.beta2 * v + gg : fmaf(a.beta2, v, gg);
  m = fmaf(1.0f - a.beta1, g - m, m);
  const float q = step * (m / fmaf(sqrtf(v), a.inv_bc2_sqrt, a.eps));
  p = TAIL ? (1.0f - lr * wd) * p - q : fmaf(fmaf(-lr, wd, 1.0f), p, -q);
}

// 8 elements per thread: 16 B of each bf16 stream, 2 x 16 B of the EMA.  MAP: the map byte of the next round is fetched before
// this round's streams, so the dependent load is off the critical path; the ragged tail (n % 8 elements) belongs to the last
// map byte.  CLIP: the coefficient is the group's, 1 for a group that is not clipped.
template <bool GUARD, bool EMA, bool MAP, bool CLIP, bool SR>
__global__ __launch_bounds__(256) void adamw_kernel(const Bf16StepArgs<GUARD, EMA, MAP, CLIP, SR> a) {
  __shared__ float2 rows[MAP ? DVLA_STEP_MAX_GROUPS : 1];
  __shared__ float coefs[CLIP ? DVLA_STEP_MAX_GROUPS : 1];
  AdamArgs c = a;      // the core alone: writing to `a` would put its tables into scratch
  int cand = 0;
  if constexpr (GUARD) {
    if (a.st->ok == 0) return;
    c.inv_bc1 = a.st->inv_bc1; c.inv_bc2_sqrt = a.st->inv_bc2_sqrt;
    cand = a.st->cand;
  }
  uint32_t key = 0;
  if constexpr (SR) {      // keyed by the count of applied steps this step becomes
    if constexpr (GUARD) key = sr_key(a.seed, (uint64_t)a.st->applied, a.bucket);
    else key = sr_key(a.seed, (uint64_t)a.step, a.bucket);
  }
  if constexpr (MAP) {
    if (threadIdx.x < DVLA_STEP_MAX_GROUPS) {
      rows[threadIdx.x] = group_row(a, 0);
      if constexpr (CLIP) coefs[threadIdx.x] = group_coef(a, a.n_groups, 1.0f);
    }
    __syncthreads();
  }
  Ema x = {};
  if constexpr (EMA) x = ema_of(a, cand);
  float coef0 = 1.0f;
  if constexpr (!CLIP) coef0 = clip_coef(c.sumsq, c.max_norm);
  // lr, wd and clip coefficient of a vector's group; false: the vector is left alone
  auto group = [&](unsigned id, float& lr, float& wd, float& coef) {
    lr = c.lr; wd = c.wd; coef = coef0;
    if constexpr (MAP) {
      if (id >= (unsigned)a.n_groups) return false;
      const float2 r = rows[id];
      lr = r.x; wd = r.y;
      if constexpr (CLIP) coef = coefs[id];
    }
    return true;
  };
  const int64_t nvec = c.n >> 3, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned id = 0;
  if constexpr (MAP) id = i < nvec ? a.map[i] : 255u;
  while (i < nvec) {
    const int64_t nx = i + stride;
    unsigned id_nx = 0;
    if constexpr (MAP) id_nx = nx < nvec ? a.map[nx] : 255u;
    float lr, wd, coef;
    if (group(id, lr, wd, coef)) {
      const uint4 up = reinterpret_cast<const uint4*>(c.p)[i], ug = reinterpret_cast<const uint4*>(c.g)[i];
      const uint4 um = reinterpret_cast<const uint4*>(c.m)[i], uv = reinterpret_cast<const uint4*>(c.v)[i];
      const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
      const uint32_t wm[4] = {um.x, um.y, um.z, um.w}, wv[4] = {uv.x, uv.y, uv.z, uv.w};
      uint32_t op[4], om[4], ov[4];
      float e[8];
      if constexpr (EMA) {
        const float4 e0 = reinterpret_cast<const float4*>(x.e)[2 * i], e1 = reinterpret_cast<const float4*>(x.e)[2 * i + 1];
        e[0] = e0.x; e[1] = e0.y; e[2] = e0.z; e[3] = e0.w; e[4] = e1.x; e[5] = e1.y; e[6] = e1.z; e[7] = e1.w;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float p0 = bf2f((bf16_t)(wp[k] & 0xffff)), p1 = bf2f((bf16_t)(wp[k] >> 16));
        float m0 = bf2f((bf16_t)(wm[k] & 0xffff)), m1 = bf2f((bf16_t)(wm[k] >> 16));
        float v0 = bf2f((bf16_t)(wv[k] & 0xffff)), v1 = bf2f((bf16_t)(wv[k] >> 16));
        adam_one<false>(p0, bf2f((bf16_t)(wg[k] & 0xffff)), m0, v0, c, lr, wd, coef);
        adam_one<false>(p1, bf2f((bf16_t)(wg[k] >> 16)), m1, v1, c, lr, wd, coef);
        if constexpr (SR) {
          const int64_t el = a.base + (i << 3) + 2 * k;
          uint32_t pb0, mb0, vb0, pb1, mb1, vb1;
          sr_round3(p0, m0, v0, key, el, pb0, mb0, vb0);
          sr_round3(p1, m1, v1, key, el + 1, pb1, mb1, vb1);
          op[k] = pb0 | (pb1 << 16); om[k] = mb0 | (mb1 << 16); ov[k] = vb0 | (vb1 << 16);
        } else {
          op[k] = pack2bf(p0, p1); om[k] = pack2bf(m0, m1); ov[k] = pack2bf(v0, v1);
        }
        if constexpr (EMA) {      // the EMA follows the bf16 value that is written
          ema_one(e[2 * k], bf2f((bf16_t)(op[k] & 0xffff)), x);
          ema_one(e[2 * k + 1], bf2f((bf16_t)(op[k] >> 16)), x);
        }
      }
      reinterpret_cast<uint4*>(c.p)[i] = make_uint4(op[0], op[1], op[2], op[3]);
      reinterpret_cast<uint4*>(c.m)[i] = make_uint4(om[0], om[1], om[2], om[3]);
      reinterpret_cast<uint4*>(c.v)[i] = make_uint4(ov[0], ov[1], ov[2], ov[3]);
      if constexpr (EMA) {
        reinterpret_cast<float4*>(x.e)[2 * i] = make_float4(e[0], e[1], e[2], e[3]);
        reinterpret_cast<float4*>(x.e)[2 * i + 1] = make_float4(e[4], e[5], e[6], e[7]);
      }
    }
    i = nx; id = id_nx;
  }
  if (blockIdx.x == 0 && (nvec << 3) < c.n) {
    unsigned idt = 0;
    if constexpr (MAP) idt = a.map[nvec];
    float lr, wd, coef;
    if (group(idt, lr, wd, coef))
      for (int64_t j = (nvec << 3) + threadIdx.x; j < c.n; j += 256) {
        float p = bf2f(c.p[j]), m = bf2f(c.m[j]), v = bf2f(c.v[j]);
        adam_one<true>(p, bf2f(c.g[j]), m, v, c, lr, wd, coef);
        uint32_t pb, mb, vb;
        if constexpr (SR) sr_round3(p, m, v, key, a.base + j, pb, mb, vb);
        else { pb = f2bf(p); mb = f2bf(m); vb = f2bf(v); }
        c.p[j] = (bf16_t)pb; c.m[j] = (bf16_t)mb; c.v[j] = (bf16_t)vb;
        if constexpr (EMA) { float e = x.e[j]; ema_one(e, bf2f((bf16_t)pb), x); x.e[j] = e; }
      }
  }
}

// ---- the fp32-master step -----------------------------------------------------------------------------------------------------
// One element.  Every torch foreach op is a separate kernel, so its result is rounded to fp32 before the next op sees it
// (explicit _rn intrinsics: the compiler must not contract across them); WITHIN one ATen element function the expression is
// compiled as written (a + b * c contracts to one fma: lerp, addcmul, addcdiv).  clipped false: no clip, the gradient as it is.
__device__ __forceinline__ void master_one(float& p, float g, float& m, float& v, const MasterArgs& a, float decay, float step_size,
                                           float coef) {
  if (!(coef < 0.f)) g = __fmul_rn(g, coef);                          // clip_grad_norm_: _foreach_mul_(grads, clip_coef), fp32
  p = __fmul_rn(p, decay);                                      // decoupled weight decay
  const float d = __fsub_rn(g, m);                              // exp_avg.lerp_(grad, w1)
  m = a.w1_small ? fmaf(a.w1, d, m) : fmaf(-d, 1.0f - a.w1, g);
  v = __fmul_rn(v, a.beta2);                                    // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  v = fmaf(a.omb2, __fmul_rn(g, g), v);
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);   // (sqrt(v) / bc2_sqrt) + eps
  p = fmaf(step_size, __fdiv_rn(m, denom), p);                  // p.addcdiv_(m, denom, -lr / bc1)
}

// 8 elements per thread: 2 x 16 B of each fp32 stream (EMA: five of them), 16 B of shadow.  GUARD, EMA, MAP and the map's
// prefetch and tail as in adamw_kernel.  CLIP: a group that is not clipped has a negative coefficient in LDS.
template <bool GUARD, bool EMA, bool MAP, bool CLIP>
__global__ __launch_bounds__(256) void adamw_master_kernel(const MasterStepArgs<GUARD, EMA, MAP, CLIP> a) {
  __shared__ float2 rows[MAP ? DVLA_STEP_MAX_GROUPS : 1];
  __shared__ float coefs[CLIP ? DVLA_STEP_MAX_GROUPS : 1];
  MasterArgs c = a;      // the core alone, as in adamw_kernel
  int cand = 0;
  if constexpr (GUARD) {
    if (a.st->ok == 0) return;
    c.bc2_sqrt = a.st->bc2_sqrt;
    if constexpr (!MAP) c.step_size = a.st->step_size;
    cand = a.st->cand;
  }
  if constexpr (MAP) {
    if (threadIdx.x < DVLA_STEP_MAX_GROUPS) {
      rows[threadIdx.x] = group_row(a, cand);
      if constexpr (CLIP) coefs[threadIdx.x] = group_coef(a, a.n_groups, -1.0f);
    }
    __syncthreads();
  }
  Ema x = {};
  if constexpr (EMA) x = ema_of(a, cand);
  float coef0 = -1.0f;
  if constexpr (!CLIP) { if (c.sumsq) coef0 = clip_coef(c.sumsq, c.max_norm); }
  // decay, step_size and clip of a vector's group; false: the vector is left alone
  auto group = [&](unsigned id, float& decay, float& step_size, float& coef) {
    decay = c.decay; step_size = c.step_size; coef = coef0;
    if constexpr (MAP) {
      if (id >= (unsigned)a.n_groups) return false;
      const float2 r = rows[id];
      decay = r.x; step_size = r.y;
      if constexpr (CLIP) coef = coefs[id];
    }
    return true;
  };
  const int64_t nvec = c.n >> 3, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned id = 0;
  if constexpr (MAP) id = i < nvec ? a.map[i] : 255u;
  while (i < nvec) {
    const int64_t nx = i + stride;
    unsigned id_nx = 0;
    if constexpr (MAP) id_nx = nx < nvec ? a.map[nx] : 255u;
    float decay, step_size, coef;
    if (group(id, decay, step_size, coef)) {
      float4 p4[2], g4[2], m4[2], v4[2], e4[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        p4[h] = reinterpret_cast<const float4*>(c.p)[2 * i + h]; g4[h] = reinterpret_cast<const float4*>(c.g)[2 * i + h];
        m4[h] = reinterpret_cast<const float4*>(c.m)[2 * i + h]; v4[h] = reinterpret_cast<const float4*>(c.v)[2 * i + h];
        if constexpr (EMA) e4[h] = reinterpret_cast<const float4*>(x.e)[2 * i + h];
      }
      uint32_t sh[4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        master_one(p4[h].x, g4[h].x, m4[h].x, v4[h].x, c, decay, step_size, coef);
        master_one(p4[h].y, g4[h].y, m4[h].y, v4[h].y, c, decay, step_size, coef);
        master_one(p4[h].z, g4[h].z, m4[h].z, v4[h].z, c, decay, step_size, coef);
        master_one(p4[h].w, g4[h].w, m4[h].w, v4[h].w, c, decay, step_size, coef);
        sh[2 * h] = pack2bf(p4[h].x, p4[h].y); sh[2 * h + 1] = pack2bf(p4[h].z, p4[h].w);
        if constexpr (EMA) {
          ema_one(e4[h].x, p4[h].x, x); ema_one(e4[h].y, p4[h].y, x); ema_one(e4[h].z, p4[h].z, x); ema_one(e4[h].w, p4[h].w, x);
        }
        reinterpret_cast<float4*>(c.p)[2 * i + h] = p4[h];
        reinterpret_cast<float4*>(c.m)[2 * i + h] = m4[h];
        reinterpret_cast<float4*>(c.v)[2 * i + h] = v4[h];
        if constexpr (EMA) reinterpret_cast<float4*>(x.e)[2 * i + h] = e4[h];
      }
      if (c.sh) reinterpret_cast<uint4*>(c.sh)[i] = make_uint4(sh[0], sh[1], sh[2], sh[3]);
    }
    i = nx; id = id_nx;
  }
  if (blockIdx.x == 0 && (nvec << 3) < c.n) {
    unsigned idt = 0;
    if constexpr (MAP) idt = a.map[nvec];
    float decay, step_size, coef;
    if (group(idt, decay, step_size, coef))
      for (int64_t j = (nvec << 3) + threadIdx.x; j < c.n; j += 256) {
        float p = c.p[j], m = c.m[j], v = c.v[j];
        master_one(p, c.g[j], m, v, c, decay, step_size, coef);
        c.p[j] = p; c.m[j] = m; c.v[j] = v;
        if constexpr (EMA) { float e = x.e[j]; ema_one(e, p, x); x.e[j] = e; }
        if (c.sh) c.sh[j] = f2bf(p);
      }
  }
}

// param <-> ema, and the bf16 shadow of the new param in the same pass (pack2bf / f2bf: the bits of dvla_cast_f32_to_bf16)
__global__ __launch_bounds__(256) void ema_swap_f32_kernel(float* __restrict__ p, float* __restrict__ e, bf16_t* __restrict__ sh,
                                                           int64_t n) {
  const int64_t nvec = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float4 p4[2], e4[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      p4[h] = reinterpret_cast<const float4*>(p)[2 * i + h]; e4[h] = reinterpret_cast<const float4*>(e)[2 * i + h];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      reinterpret_cast<float4*>(p)[2 * i + h] = e4[h]; reinterpret_cast<float4*>(e)[2 * i + h] = p4[h];
    }
    if (sh)
      reinterpret_cast<uint4*>(sh)[i] = make_uint4(pack2bf(e4[0].x, e4[0].y), pack2bf(e4[0].z, e4[0].w),
                                                   pack2bf(e4[1].x, e4[1].y), pack2bf(e4[1].z, e4[1].w));
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < n; i += 256) {
      const float a = p[i], b = e[i];
      p[i] = b; e[i] = a;
      if (sh) sh[i] = f2bf(b);
    }
}

// bf16 parameters cannot hold the fp32 EMA and come back: they are stashed while the rounded EMA stands in for them
__global__ __launch_bounds__(256) void ema_swap_bf16_kernel(bf16_t* __restrict__ p, const float* __restrict__ e,
                                                            bf16_t* __restrict__ stash, int64_t n, int restore) {
  const int64_t nvec = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    if (restore) {
      reinterpret_cast<uint4*>(p)[i] = reinterpret_cast<const uint4*>(stash)[i];
    } else {
      const float4 e0 = reinterpret_cast<const float4*>(e)[2 * i], e1 = reinterpret_cast<const float4*>(e)[2 * i + 1];
      reinterpret_cast<uint4*>(stash)[i] = reinterpret_cast<const uint4*>(p)[i];
      reinterpret_cast<uint4*>(p)[i] = make_uint4(pack2bf(e0.x, e0.y), pack2bf(e0.z, e0.w), pack2bf(e1.x, e1.y), pack2bf(e1.z, e1.w));
    }
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < n; i += 256) {
      if (restore) { p[i] = stash[i]; } else { stash[i] = p[i]; p[i] = f2bf(e[i]); }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// The step-dependent scalars from the 1-based step count: shared with dvla_step_candidates, so a guarded step runs on the same floats
inline void bf16_step_scalars(float beta1, float beta2, int64_t step, float* inv_bc1, float* inv_bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  *inv_bc1 = (float)(1.0 / bc1); *inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}
// the scalars as torch/optim/adam.py (_multi_tensor_adam, capturable=False) computes them in Python floats
inline float master_decay(double lr, double weight_decay) { return (float)(1.0 - lr * weight_decay); }
inline void master_step_scalars(double lr, double beta1, double beta2, int64_t step, float* bc2_sqrt, float* step_size) {
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  *bc2_sqrt = (float)pow(bc2, 0.5);
  *step_size = (float)((lr / bc1) * -1.0);
}

inline unsigned step_blocks(int64_t n) {      // 8 elements per thread, at most 4096 blocks (grid-stride beyond)
  return (unsigned)std::min<int64_t>(std::max<int64_t>((n / 8 + 255) / 256, 1), 4096);
}

// runtime booleans -> template arguments: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <class F> int with_flags(F f) { return f(); }
template <class F, class... Bs> int with_flags(F f, bool b, Bs... rest) {
  return b ? with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
           : with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// What a step launch takes besides the core arguments of its precision; a null pointer turns the part's flag off.
struct GroupClip { const float* sumsq; const float* max_norm; };      // the per-group clip of the `_clip` entry points
struct StepOpts {
  const dvla_step_state* state = nullptr;
  float* ema = nullptr; const float* ema_w = nullptr; int32_t n_cand = 1;      // ema_w[j]: the weight at the j-th candidate count
  const uint8_t* map = nullptr; int32_t n_groups = 1;
  const GroupClip* clip = nullptr;
  const SrPart* sr = nullptr;
};

// the checks every step entry point makes before the n == 0 and alignment ones (lr, wd: one value per group)
inline int step_opts_ok(bool streams, int64_t n, int64_t step, const void* lr, const void* wd, const StepOpts& o) {
  if (!streams || !lr || !wd || n < 0 || step < 1 || o.n_groups < 1 || o.n_groups > DVLA_STEP_MAX_GROUPS) return DVLA_ERR_ARG;
  if (!o.map && (o.n_groups != 1 || o.clip)) return DVLA_ERR_ARG;      // without a map there is one group
  if (o.clip && (!o.clip->sumsq || !o.clip->max_norm)) return DVLA_ERR_ARG;
  if (o.ema && !o.ema_w) return DVLA_ERR_ARG;
  if (o.state && (o.n_cand < 1 || o.n_cand > DVLA_STEP_MAX_CANDIDATES)) return DVLA_ERR_ARG;
  if (o.sr && o.sr->base < 0) return DVLA_ERR_ARG;
  return DVLA_OK;
}

// the parts of an instance's argument block; gx, gy: MapPart::x and ::y (gy in rows of DVLA_STEP_MAX_GROUPS) of the n_groups groups
template <class Args, bool GUARD, bool EMA, bool MAP, bool CLIP, bool SR, int NC>
void fill_parts(Args& a, const StepOpts& o, const float* gx, const float* gy) {
  const int n_cand = o.state ? o.n_cand : 1;
  if constexpr (GUARD) a.st = o.state;
  if constexpr (EMA) {
    a.e = o.ema;
    if constexpr (GUARD) { for (int j = 0; j < DVLA_STEP_MAX_CANDIDATES; ++j) a.wt.w[j] = o.ema_w[j < n_cand ? j : n_cand - 1]; }
    else a.w = o.ema_w[0];
  }
  if constexpr (MAP) {
    a.map = o.map; a.n_groups = o.n_groups;
    for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) {
      const int r = g < o.n_groups ? g : o.n_groups - 1;
      a.x[g] = gx[r];
      for (int k = 0; k < NC; ++k) a.y[k][g] = gy[k * DVLA_STEP_MAX_GROUPS + r];
    }
  }
  if constexpr (CLIP) {
    a.group_sumsq = o.clip->sumsq;
    for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) a.group_max_norm[g] = g < o.n_groups ? o.clip->max_norm[g] : 0.f;
  }
  if constexpr (SR) static_cast<SrPart&>(a) = *o.sr;
}

// Every bf16 step entry point: validates, builds the arguments and launches the instance the options select.  lr, wd: n_groups
// doubles, rounded to float here as dvla_adamw_bf16 receives its one pair (whose floats pass through a double unchanged).
// Guarded: `step` only has to be >= 1.
int bf16_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, const double* lr, const double* wd,
              float beta1, float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm, const StepOpts& o,
              void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int rc = step_opts_ok(param && grad && exp_avg && exp_avg_sq, n, step, lr, wd, o);
  if (rc != DVLA_OK) return rc;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (o.ema && !al16(o.ema)) || (o.state && !al16(o.state)))
    return DVLA_ERR_UNSUPPORTED;
  float lrf[DVLA_STEP_MAX_GROUPS], wdf[DVLA_STEP_MAX_GROUPS];
  for (int g = 0; g < o.n_groups; ++g) { lrf[g] = (float)lr[g]; wdf[g] = (float)wd[g]; }
  AdamArgs core;
  core.p = reinterpret_cast<bf16_t*>(param); core.g = reinterpret_cast<const bf16_t*>(grad);
  core.m = reinterpret_cast<bf16_t*>(exp_avg); core.v = reinterpret_cast<bf16_t*>(exp_avg_sq); core.n = n;
  core.lr = lrf[0]; core.wd = wdf[0]; core.beta1 = beta1; core.beta2 = beta2; core.eps = eps;
  core.inv_bc1 = core.inv_bc2_sqrt = 0.f;           // guarded: the kernel takes both from the state
  if (!o.state) bf16_step_scalars(beta1, beta2, step, &core.inv_bc1, &core.inv_bc2_sqrt);
  core.sumsq = o.state ? (max_norm > 0.f ? &o.state->sumsq : nullptr) : grad_sumsq; core.max_norm = max_norm;
  return with_flags([&](auto G, auto E, auto M, auto C, auto S) {
    constexpr bool g = G.value, e = E.value, m = M.value, c = C.value, s = S.value;
    if constexpr (c && !m) {
      return (int)DVLA_ERR_ARG;                     // (step_opts_ok has refused it)
    } else {
      Bf16StepArgs<g, e, m, c, s> a;
      static_cast<AdamArgs&>(a) = core;
      fill_parts<decltype(a), g, e, m, c, s, 1>(a, o, lrf, wdf);
      hipLaunchKernelGGL((adamw_kernel<g, e, m, c, s>), dim3(step_blocks(n)), dim3(256), 0, stream, a);
      return dvla_check_launch();
    }
  }, o.state != nullptr, o.ema != nullptr, o.map != nullptr, o.clip != nullptr, o.sr != nullptr);
}

// Every fp32-master step entry point.  lr, wd: n_groups doubles (torch's Python floats).
int master_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t n, const double* lr,
                const double* wd, double beta1, double beta2, double eps, int64_t step, const float* grad_sumsq, float max_norm,
                const StepOpts& o, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc = step_opts_ok(param && grad && exp_avg && exp_avg_sq, n, step, lr, wd, o);
  if (rc != DVLA_OK) return rc;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (shadow_bf16 && !al16(shadow_bf16)) ||
      (o.ema && !al16(o.ema)) || (o.state && !al16(o.state)))
    return DVLA_ERR_UNSUPPORTED;
  MasterArgs core;
  core.p = param; core.g = grad; core.m = exp_avg; core.v = exp_avg_sq; core.sh = reinterpret_cast<bf16_t*>(shadow_bf16); core.n = n;
  core.decay = master_decay(lr[0], wd[0]);
  core.w1 = (float)(1.0 - beta1); core.w1_small = fabsf(core.w1) < 0.5f;
  core.beta2 = (float)beta2; core.omb2 = (float)(1.0 - beta2); core.eps = (float)eps;
  master_step_scalars(lr[0], beta1, beta2, step, &core.bc2_sqrt, &core.step_size);      // guarded: the kernel takes the state's
  core.sumsq = o.state ? (max_norm > 0.f ? &o.state->sumsq : nullptr) : grad_sumsq; core.max_norm = max_norm;
  float gx[DVLA_STEP_MAX_GROUPS], gy[DVLA_STEP_MAX_CANDIDATES][DVLA_STEP_MAX_GROUPS];
  if (o.map) {
    dvla_group_row rows[DVLA_STEP_MAX_GROUPS];
    rc = dvla_group_scalars(lr, wd, o.n_groups, beta1, beta2, step, o.state ? o.n_cand : 1, rows);
    if (rc != DVLA_OK) return rc;
    for (int g = 0; g < o.n_groups; ++g) {
      gx[g] = rows[g].decay;
      for (int k = 0; k < DVLA_STEP_MAX_CANDIDATES; ++k) gy[k][g] = rows[g].step_size[k];
    }
  }
  return with_flags([&](auto G, auto E, auto M, auto C) {
    constexpr bool g = G.value, e = E.value, m = M.value, c = C.value;
    if constexpr (c && !m) {
      return (int)DVLA_ERR_ARG;                     // (step_opts_ok has refused it)
    } else {
      MasterStepArgs<g, e, m, c> a;
      static_cast<MasterArgs&>(a) = core;
      fill_parts<decltype(a), g, e, m, c, false, g ? DVLA_STEP_MAX_CANDIDATES : 1>(a, o, gx, &gy[0][0]);
      hipLaunchKernelGGL((adamw_master_kernel<g, e, m, c>), dim3(step_blocks(n)), dim3(256), 0, stream, a);
      return dvla_check_launch();
    }
  }, o.state != nullptr, o.ema != nullptr, o.map != nullptr, o.clip != nullptr);
}

// the two-stage sum of squares: `partial` one float per block of stage 1 (VEC elements per thread and round)
template <int VEC, class T>
int sumsq(void (*stage1)(const T*, int64_t, float*), const void* x, int64_t n, float* partial, float* out, int32_t accumulate,
          void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!x || !partial || !out || n < 0) return DVLA_ERR_ARG;
  if (!al16(x)) return DVLA_ERR_UNSUPPORTED;
  int64_t blocks = (n / VEC + 255) / 256;
  if (blocks > SS_BLOCKS) blocks = SS_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(stage1, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const T*>(x), n, partial);
  int rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, partial, (int)blocks, out, (int)accumulate);
  return dvla_check_launch();
}

}  // namespace

extern "C" int64_t dvla_sumsq_partial_len(void) { return SS_BLOCKS; }
extern "C" int dvla_sumsq_bf16(const void* x, int64_t n, float* partial, float* out, int32_t accumulate, void* stream) {
  return sumsq<8, bf16_t>(sumsq_partial_kernel, x, n, partial, out, accumulate, stream);
}
extern "C" int dvla_sumsq_f32(const float* x, int64_t n, float* partial, float* out, int32_t accumulate, void* stream) {
  return sumsq<4, float>(sumsq_f32_partial_kernel, x, n, partial, out, accumulate, stream);
}

// ---- the tables the host derives ----------------------------------------------------------------------------------------------
extern "C" int dvla_step_candidates(double lr, double beta1, double beta2, int64_t base, int32_t n_cand, dvla_step_scalars* out) {
  if (!out || base < 1 || n_cand < 1 || n_cand > DVLA_STEP_MAX_CANDIDATES) return DVLA_ERR_ARG;
  for (int32_t j = 0; j < n_cand; ++j) {      // the bf16 kernel's betas are floats (dvla_adamw_bf16's arguments)
    bf16_step_scalars((float)beta1, (float)beta2, base + j, &out[j].inv_bc1, &out[j].inv_bc2_sqrt);
    master_step_scalars(lr, beta1, beta2, base + j, &out[j].bc2_sqrt, &out[j].step_size);
  }
  return DVLA_OK;
}

extern "C" int dvla_step_verdict(const float* bucket_sumsq, int32_t n, float* grad_sumsq, dvla_step_state* state,
                                 int64_t confirmed_applied, int32_t n_cand, const dvla_step_scalars* cand, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!bucket_sumsq || !grad_sumsq || !state || !cand || n < 0 || confirmed_applied < 0 || n_cand < 1 ||
      n_cand > DVLA_STEP_MAX_CANDIDATES)
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (n > DVLA_STEP_MAX_BUCKETS || !al16(state)) return DVLA_ERR_UNSUPPORTED;
  VerdictArgs a;
  a.slots = bucket_sumsq; a.n = n; a.out = grad_sumsq; a.st = state; a.confirmed = confirmed_applied; a.n_cand = n_cand;
  for (int j = 0; j < DVLA_STEP_MAX_CANDIDATES; ++j) a.c[j] = cand[j < n_cand ? j : n_cand - 1];
  hipLaunchKernelGGL(step_verdict_kernel, dim3(1), dim3(64), 0, stream, a);
  return dvla_check_launch();
}

extern "C" int dvla_ema_weights(double decay, int32_t warmup, int64_t base, int32_t n, float* out) {
  if (!out || !(decay > 0.0 && decay < 1.0) || base < 1 || n < 0 || n > DVLA_STEP_MAX_CANDIDATES) return DVLA_ERR_ARG;
  for (int32_t j = 0; j < n; ++j) {
    const double t = (double)(base + j);      // the 1-based count of applied steps
    double d = decay;
    if (warmup) {
      const double ramp = (1.0 + t) / (10.0 + t);
      if (ramp < d) d = ramp;
    }
    out[j] = (float)(1.0 - d);
  }
  return DVLA_OK;
}

extern "C" int dvla_group_scalars(const double* lr, const double* weight_decay, int32_t n_groups, double beta1, double beta2,
                                  int64_t base, int32_t n_cand, dvla_group_row* out) {
  if (!lr || !weight_decay || !out || n_groups < 1 || n_groups > DVLA_STEP_MAX_GROUPS || base < 1 || n_cand < 1 ||
      n_cand > DVLA_STEP_MAX_CANDIDATES)
    return DVLA_ERR_ARG;
  for (int32_t g = 0; g < n_groups; ++g) {
    out[g].decay = master_decay(lr[g], weight_decay[g]);
    out[g].lr = (float)lr[g]; out[g].weight_decay = (float)weight_decay[g];      // as dvla_adamw_bf16 receives them
    float bc2_sqrt;                                                               // common to all groups: not kept here
    for (int32_t j = 0; j < DVLA_STEP_MAX_CANDIDATES; ++j)
      master_step_scalars(lr[g], beta1, beta2, base + (j < n_cand ? j : n_cand - 1), &bc2_sqrt, &out[g].step_size[j]);
  }
  return DVLA_OK;
}

// ---- the step entry points: each states what it requires and hands the rest to bf16_step / master_step -------------------------
// one group, no map; a guarded one has no step count of its own (1 passes the check)
extern "C" int dvla_adamw_bf16(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int64_t step, const float* grad_sumsq, float max_norm,
                               void* stream) {
  const double l = lr, w = weight_decay;
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, &l, &w, beta1, beta2, eps, step, grad_sumsq, max_norm, {}, stream);
}
extern "C" int dvla_adamw_f32_master(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                     int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                     int64_t step, const float* grad_sumsq, float max_norm, void* stream) {
  return master_step(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, &lr, &weight_decay, beta1, beta2, eps, step, grad_sumsq,
                     max_norm, {}, stream);
}

extern "C" int dvla_adamw_bf16_guarded(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                       const dvla_step_state* state, void* stream) {
  if (!state) return DVLA_ERR_ARG;
  const double l = lr, w = weight_decay;
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, &l, &w, beta1, beta2, eps, 1, nullptr, max_norm, {state}, stream);
}
extern "C" int dvla_adamw_f32_master_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                             int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                             float max_norm, const dvla_step_state* state, void* stream) {
  if (!state) return DVLA_ERR_ARG;
  return master_step(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, &lr, &weight_decay, beta1, beta2, eps, 1, nullptr,
                     max_norm, {state}, stream);
}

extern "C" int dvla_adamw_bf16_ema(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* grad_sumsq,
                                   float max_norm, float ema_w, void* stream) {
  if (!ema) return DVLA_ERR_ARG;
  const double l = lr, w = weight_decay;
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, &l, &w, beta1, beta2, eps, step, grad_sumsq, max_norm,
                   {nullptr, ema, &ema_w}, stream);
}
extern "C" int dvla_adamw_f32_master_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                         float* ema, int64_t n, double lr, double beta1, double beta2, double eps,
                                         double weight_decay, int64_t step, const float* grad_sumsq, float max_norm, float ema_w,
                                         void* stream) {
  if (!ema) return DVLA_ERR_ARG;
  return master_step(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, &lr, &weight_decay, beta1, beta2, eps, step, grad_sumsq,
                     max_norm, {nullptr, ema, &ema_w}, stream);
}

extern "C" int dvla_adamw_bf16_ema_guarded(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                           float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                           const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream) {
  if (!ema || !state) return DVLA_ERR_ARG;
  const double l = lr, w = weight_decay;
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, &l, &w, beta1, beta2, eps, 1, nullptr, max_norm,
                   {state, ema, ema_w, n_cand}, stream);
}
extern "C" int dvla_adamw_f32_master_ema_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                 void* shadow_bf16, float* ema, int64_t n, double lr, double beta1, double beta2,
                                                 double eps, double weight_decay, float max_norm, const dvla_step_state* state,
                                                 const float* ema_w, int32_t n_cand, void* stream) {
  if (!ema || !state) return DVLA_ERR_ARG;
  return master_step(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, &lr, &weight_decay, beta1, beta2, eps, 1, nullptr,
                     max_norm, {state, ema, ema_w, n_cand}, stream);
}

extern "C" int dvla_ema_swap_f32(float* param, float* ema, void* shadow_bf16, int64_t n, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !ema || n < 0) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(ema) || (shadow_bf16 && !al16(shadow_bf16))) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ema_swap_f32_kernel, dim3(step_blocks(n)), dim3(256), 0, stream, param, ema,
                     reinterpret_cast<bf16_t*>(shadow_bf16), n);
  return dvla_check_launch();
}

extern "C" int dvla_ema_swap_bf16(void* param, const float* ema, void* stash, int64_t n, int32_t restore, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !ema || !stash || n < 0) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(ema) || !al16(stash)) return DVLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ema_swap_bf16_kernel, dim3(step_blocks(n)), dim3(256), 0, stream, reinterpret_cast<bf16_t*>(param), ema,
                     reinterpret_cast<bf16_t*>(stash), n, (int)(restore != 0));
  return dvla_check_launch();
}

// with a group map (required), the guard and the EMA by their pointers; `_clip`: a clip per group instead of the launch's one
extern "C" int dvla_adamw_bf16_grouped(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                       const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                       float beta1, float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm,
                                       const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream) {
  if (!group_map) return DVLA_ERR_ARG;
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, lr, weight_decay, beta1, beta2, eps, step, grad_sumsq, max_norm,
                   {state, ema, ema_w, n_cand, group_map, n_groups}, stream);
}
extern "C" int dvla_adamw_f32_master_grouped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                             float* ema, int64_t n, const uint8_t* group_map, int32_t n_groups, const double* lr,
                                             const double* weight_decay, double beta1, double beta2, double eps, int64_t step,
                                             const float* grad_sumsq, float max_norm, const dvla_step_state* state,
                                             const float* ema_w, int32_t n_cand, void* stream) {
  if (!group_map) return DVLA_ERR_ARG;
  return master_step(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, lr, weight_decay, beta1, beta2, eps, step, grad_sumsq,
                     max_norm, {state, ema, ema_w, n_cand, group_map, n_groups}, stream);
}

extern "C" int dvla_adamw_bf16_grouped_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                            const uint8_t* group_map, int32_t n_groups, const double* lr,
                                            const double* weight_decay, float beta1, float beta2, float eps, int64_t step,
                                            const float* group_sumsq, const float* max_norm, const dvla_step_state* state,
                                            const float* ema_w, int32_t n_cand, void* stream) {
  if (!group_map) return DVLA_ERR_ARG;
  const GroupClip clip = {group_sumsq, max_norm};
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, lr, weight_decay, beta1, beta2, eps, step, nullptr, 0.f,
                   {state, ema, ema_w, n_cand, group_map, n_groups, &clip}, stream);
}
extern "C" int dvla_adamw_f32_master_grouped_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                  void* shadow_bf16, float* ema, int64_t n, const uint8_t* group_map,
                                                  int32_t n_groups, const double* lr, const double* weight_decay, double beta1,
                                                  double beta2, double eps, int64_t step, const float* group_sumsq,
                                                  const float* max_norm, const dvla_step_state* state, const float* ema_w,
                                                  int32_t n_cand, void* stream) {
  if (!group_map) return DVLA_ERR_ARG;
  const GroupClip clip = {group_sumsq, max_norm};
  return master_step(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, lr, weight_decay, beta1, beta2, eps, step, nullptr, 0.f,
                     {state, ema, ema_w, n_cand, group_map, n_groups, &clip}, stream);
}

// ---- stochastic rounding ----------------------------------------------------------------------------------------------------------
extern "C" int dvla_sr_cast_f32_to_bf16(const float* x, void* out, int64_t n, uint64_t seed, uint64_t step, int32_t bucket,
                                        int32_t stream_id, int64_t index_base, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!x || !out || n < 0 || stream_id < 0 || stream_id > 2) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(sr_cast_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, reinterpret_cast<bf16_t*>(out), n, seed, step,
                     (uint32_t)bucket, (int)stream_id, index_base);
  return dvla_check_launch();
}

// the grouped entry points' arguments; the map may be null: one group (n_groups 1) over a range of a bucket
extern "C" int dvla_adamw_bf16_sr(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                  const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                  float beta1, float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm,
                                  const dvla_step_state* state, const float* ema_w, int32_t n_cand, uint64_t sr_seed,
                                  int32_t sr_bucket, int64_t sr_index_base, void* stream) {
  const SrPart sr = {sr_seed, step, sr_index_base, (uint32_t)sr_bucket};
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, lr, weight_decay, beta1, beta2, eps, step, grad_sumsq, max_norm,
                   {state, ema, ema_w, n_cand, group_map, n_groups, nullptr, &sr}, stream);
}

extern "C" int dvla_adamw_bf16_sr_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                       const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                       float beta1, float beta2, float eps, int64_t step, const float* group_sumsq,
                                       const float* max_norm, const dvla_step_state* state, const float* ema_w, int32_t n_cand,
                                       uint64_t sr_seed, int32_t sr_bucket, int64_t sr_index_base, void* stream) {
  const GroupClip clip = {group_sumsq, max_norm};
  const SrPart sr = {sr_seed, step, sr_index_base, (uint32_t)sr_bucket};
  return bf16_step(param, grad, exp_avg, exp_avg_sq, n, lr, weight_decay, beta1, beta2, eps, step, nullptr, 0.f,
                   {state, ema, ema_w, n_cand, group_map, n_groups, &clip, &sr}, stream);
}
