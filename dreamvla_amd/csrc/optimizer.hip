// optimizer.hip -- gradient-norm clipping + AdamW over flat bf16 buffers (gfx950), HBM-bound.
//
// Replaces `torch.nn.utils.clip_grad_norm_` + `torch.optim.AdamW.step` of the training step (train.py /
// utils/train_utils.py in the reference: the caller's optimizer step).  Parameters, gradients
// and both moments live in flat bf16 buffers (the gradient buffers are the data-parallel communication buckets), so
// the whole step is two kernels per bucket instead of ~80 multi-tensor launches:
//   dvla_sumsq_bf16 : sum of squares (fp32, deterministic two-stage reduction) accumulated into a device scalar
//   dvla_adamw_bf16 : clip coefficient from that scalar, then the AdamW update, all math in fp32 per element,
//                     one read-modify-write pass: 2 B (g) + 3 x (2 + 2) B (p, m, v) = 14 B / parameter.
// Element-wise semantics follow torch's fused AdamW with bf16 parameters (state in the parameter dtype) and
// clip_grad_norm_ (the gradient is rounded to bf16 after scaling, as the in-place `grad.mul_(coef)` does).
//
// fp32 masters (the shipped `--precision fp32` runs: parameters, gradients and both moments fp32):
//   dvla_sumsq_f32        : the fp32 twin of dvla_sumsq_bf16, same two-stage reduction, same device scalar (one clip norm
//                           can span bf16 and fp32 buckets)
//   dvla_adamw_f32_master : clip (in fp32) + AdamW restating torch's foreach AdamW on fp32 parameters operation for
//                           operation, and the bf16 compute shadow of the new master written in the same pass:
//                           4 B (g) + 3 x (4 + 4) B (p, m, v) + 2 B (shadow) = 30 B / parameter.
//
// guarded step (an addition; dvla.h): the per-bucket sums go into one slot each,
//   dvla_step_verdict             : one wave adds them, decides whether the step is applied (the total is finite), counts, and
//                                   picks the bias-correction scalars of the step count that is then current from a table the
//                                   host derived (dvla_step_candidates) for every count still possible
//   dvla_adamw_*_guarded          : the two AdamW kernels reading verdict and scalars from that state; a skipped step moves no byte
//
// EMA of the weights (an addition; dvla.h): one more fp32 stream through the step,
//   dvla_adamw_*_ema(_guarded)    : the four AdamW kernels + e <- lerp(e, p, w) on the parameter just written (ATen's lerp, bit for
//                                   bit): 30 + 8 = 38 B / parameter on fp32 masters, 14 + 8 = 22 B on bf16; w from dvla_ema_weights
//   dvla_ema_swap_f32 / _bf16     : the EMA becomes the weights and back (evaluation), the bf16 shadow written in the same pass
//
// stochastic rounding (an addition; dvla.h): pure bf16 with round-to-nearest stores cannot train,
//   dvla_adamw_bf16_sr            : the bf16 step -- plain, guarded, with the EMA, grouped -- with parameter and both moments rounded
//                                   up with a probability equal to the discarded fraction, from counter-based random bits: 14 B still
//   dvla_sr_cast_f32_to_bf16      : the same rounding and bits as a stand-alone cast
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

struct AdamArgs {
  bf16_t* p; const bf16_t* g; bf16_t* m; bf16_t* v; int64_t n;
  float lr, beta1, beta2, eps, wd, inv_bc1, inv_bc2_sqrt;
  const float* sumsq; float max_norm;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float coef) {
  g = bf2f(f2bf(g * coef));                        // clip_grad_norm_ scales the bf16 gradient in place
  p *= (1.0f - a.lr * a.wd);                       // decoupled weight decay
  m = m + (g - m) * (1.0f - a.beta1);              // exp_avg.lerp_(grad, 1 - beta1)
  v = a.beta2 * v + (1.0f - a.beta2) * g * g;
  const float denom = sqrtf(v) * a.inv_bc2_sqrt + a.eps;
  p -= (a.lr * a.inv_bc1) * (m / denom);
}

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
  float coef = 1.0f;
  if (a.sumsq) {
    const float c = a.max_norm / (sqrtf(a.sumsq[0]) + 1e-6f);
    coef = c < 1.0f ? c : 1.0f;
  }
  const int64_t nvec = a.n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const uint4 up = reinterpret_cast<const uint4*>(a.p)[i], ug = reinterpret_cast<const uint4*>(a.g)[i];
    const uint4 um = reinterpret_cast<const uint4*>(a.m)[i], uv = reinterpret_cast<const uint4*>(a.v)[i];
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
    const uint32_t wm[4] = {um.x, um.y, um.z, um.w}, wv[4] = {uv.x, uv.y, uv.z, uv.w};
    uint32_t op[4], om[4], ov[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float p0 = bf2f((bf16_t)(wp[k] & 0xffff)), p1 = bf2f((bf16_t)(wp[k] >> 16));
      float m0 = bf2f((bf16_t)(wm[k] & 0xffff)), m1 = bf2f((bf16_t)(wm[k] >> 16));
      float v0 = bf2f((bf16_t)(wv[k] & 0xffff)), v1 = bf2f((bf16_t)(wv[k] >> 16));
      adam_one(p0, bf2f((bf16_t)(wg[k] & 0xffff)), m0, v0, a, coef);
      adam_one(p1, bf2f((bf16_t)(wg[k] >> 16)), m1, v1, a, coef);
      op[k] = pack2bf(p0, p1); om[k] = pack2bf(m0, m1); ov[k] = pack2bf(v0, v1);
    }
    reinterpret_cast<uint4*>(a.p)[i] = make_uint4(op[0], op[1], op[2], op[3]);
    reinterpret_cast<uint4*>(a.m)[i] = make_uint4(om[0], om[1], om[2], om[3]);
    reinterpret_cast<uint4*>(a.v)[i] = make_uint4(ov[0], ov[1], ov[2], ov[3]);
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < a.n; i += 256) {
      float p = bf2f(a.p[i]), m = bf2f(a.m[i]), v = bf2f(a.v[i]);
      adam_one(p, bf2f(a.g[i]), m, v, a, coef);
      a.p[i] = f2bf(p); a.m[i] = f2bf(m); a.v[i] = f2bf(v);
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

// Scalars derived on the host exactly as torch/optim/adam.py derives them from the Python (double) hyper-parameters, then
// handed to the element-wise ops as fp32 (the foreach kernels' opmath scalars).
struct MasterArgs {
  float* p; const float* g; float* m; float* v; bf16_t* sh; int64_t n;
  float decay;        // 1 - lr * wd                      (_foreach_mul_(params, 1 - lr * weight_decay))
  float w1;           // 1 - beta1                        (_foreach_lerp_(exp_avgs, grads, 1 - beta1))
  int w1_small;       // |w1| < 0.5: ATen lerp's branch
  float beta2, omb2;  // beta2, 1 - beta2                 (_foreach_mul_(exp_avg_sqs, beta2); _foreach_addcmul_(.., g, g, 1 - beta2))
  float bc2_sqrt;     // sqrt(1 - beta2^step)             (_foreach_div_(sqrt(v), bc2_sqrt))
  float eps;          //                                  (_foreach_add_(.., eps))
  float step_size;    // -lr / (1 - beta1^step)           (_foreach_addcdiv_(params, m, denom, step_size))
  const float* sumsq; float max_norm;
};

// One element.  Every torch foreach op is a separate kernel, so its result is rounded to fp32 before the next op sees it
// (explicit _rn intrinsics: the compiler must not contract across them); WITHIN one ATen element function the expression is
// compiled as written (a + b * c contracts to one fma: lerp, addcmul, addcdiv).
__device__ __forceinline__ void master_one(float& p, float g, float& m, float& v, const MasterArgs& a, float coef) {
  if (a.sumsq) g = __fmul_rn(g, coef);                          // clip_grad_norm_: _foreach_mul_(grads, clip_coef), fp32
  p = __fmul_rn(p, a.decay);                                    // decoupled weight decay
  const float d = __fsub_rn(g, m);                              // exp_avg.lerp_(grad, w1)
  m = a.w1_small ? fmaf(a.w1, d, m) : fmaf(-d, 1.0f - a.w1, g);
  v = __fmul_rn(v, a.beta2);                                    // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  v = fmaf(a.omb2, __fmul_rn(g, g), v);
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);   // (sqrt(v) / bc2_sqrt) + eps
  p = fmaf(a.step_size, __fdiv_rn(m, denom), p);                // p.addcdiv_(m, denom, -lr / bc1)
}

// the whole of adamw_master_kernel: the guarded kernel runs the same body on an applied step
__device__ __forceinline__ void adamw_master_body(MasterArgs a) {
  float coef = 1.0f;
  if (a.sumsq) {
    const float c = a.max_norm / (sqrtf(a.sumsq[0]) + 1e-6f);
    coef = c < 1.0f ? c : 1.0f;
  }
  const int64_t nvec = a.n >> 3;      // 8 elements per thread: 2 x 16 B of each fp32 stream, 16 B of shadow
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float4 p4[2], g4[2], m4[2], v4[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      p4[h] = reinterpret_cast<const float4*>(a.p)[2 * i + h]; g4[h] = reinterpret_cast<const float4*>(a.g)[2 * i + h];
      m4[h] = reinterpret_cast<const float4*>(a.m)[2 * i + h]; v4[h] = reinterpret_cast<const float4*>(a.v)[2 * i + h];
    }
    uint32_t sh[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      master_one(p4[h].x, g4[h].x, m4[h].x, v4[h].x, a, coef);
      master_one(p4[h].y, g4[h].y, m4[h].y, v4[h].y, a, coef);
      master_one(p4[h].z, g4[h].z, m4[h].z, v4[h].z, a, coef);
      master_one(p4[h].w, g4[h].w, m4[h].w, v4[h].w, a, coef);
      sh[2 * h] = pack2bf(p4[h].x, p4[h].y); sh[2 * h + 1] = pack2bf(p4[h].z, p4[h].w);
      reinterpret_cast<float4*>(a.p)[2 * i + h] = p4[h];
      reinterpret_cast<float4*>(a.m)[2 * i + h] = m4[h];
      reinterpret_cast<float4*>(a.v)[2 * i + h] = v4[h];
    }
    if (a.sh) reinterpret_cast<uint4*>(a.sh)[i] = make_uint4(sh[0], sh[1], sh[2], sh[3]);
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < a.n; i += 256) {
      float p = a.p[i], m = a.m[i], v = a.v[i];
      master_one(p, a.g[i], m, v, a, coef);
      a.p[i] = p; a.m[i] = m; a.v[i] = v;
      if (a.sh) a.sh[i] = f2bf(p);
    }
}

__global__ __launch_bounds__(256) void adamw_master_kernel(MasterArgs a) { adamw_master_body(a); }

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The step-dependent scalars of the two AdamW kernels, from the 1-based step count.  dvla_adamw_bf16 / dvla_adamw_f32_master
// and dvla_step_candidates all derive them here, so a guarded step that selects candidate `step` runs on the same floats.
inline void bf16_step_scalars(float beta1, float beta2, int64_t step, float* inv_bc1, float* inv_bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  *inv_bc1 = (float)(1.0 / bc1); *inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}
inline float master_decay(double lr, double weight_decay) { return (float)(1.0 - lr * weight_decay); }
inline void master_fixed_scalars(MasterArgs& a, double lr, double beta1, double beta2, double eps, double weight_decay) {
  a.decay = master_decay(lr, weight_decay);
  a.w1 = (float)(1.0 - beta1);
  a.w1_small = fabsf(a.w1) < 0.5f;
  a.beta2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
}
inline void master_step_scalars(double lr, double beta1, double beta2, int64_t step, float* bc2_sqrt, float* step_size) {
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  *bc2_sqrt = (float)pow(bc2, 0.5);
  *step_size = (float)((lr / bc1) * -1.0);
}

// ---- guarded step: the verdict of one step and the AdamW kernels that obey it (dvla.h: dvla_step_state) ---------------------
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

// adamw_kernel / adamw_master_kernel under a verdict: nothing is read or written on a skipped step; on an applied one the
// step-dependent scalars come from the state and the twin's loop runs.  a.sumsq is &st->sumsq or null.
// The bf16 loop is restated here (every element still goes through adam_one): moved into a function shared with adamw_kernel
// it compiles adamw_kernel to a different instruction stream, and the unguarded kernels are to stay as they are; the master
// kernels share adamw_master_body, which leaves adamw_master_kernel's instructions unchanged.
__global__ __launch_bounds__(256) void adamw_guarded_kernel(AdamArgs a, const dvla_step_state* __restrict__ st) {
  if (st->ok == 0) return;
  a.inv_bc1 = st->inv_bc1; a.inv_bc2_sqrt = st->inv_bc2_sqrt;
  float coef = 1.0f;
  if (a.sumsq) {
    const float c = a.max_norm / (sqrtf(a.sumsq[0]) + 1e-6f);
    coef = c < 1.0f ? c : 1.0f;
  }
  const int64_t nvec = a.n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const uint4 up = reinterpret_cast<const uint4*>(a.p)[i], ug = reinterpret_cast<const uint4*>(a.g)[i];
    const uint4 um = reinterpret_cast<const uint4*>(a.m)[i], uv = reinterpret_cast<const uint4*>(a.v)[i];
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
    const uint32_t wm[4] = {um.x, um.y, um.z, um.w}, wv[4] = {uv.x, uv.y, uv.z, uv.w};
    uint32_t op[4], om[4], ov[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float p0 = bf2f((bf16_t)(wp[k] & 0xffff)), p1 = bf2f((bf16_t)(wp[k] >> 16));
      float m0 = bf2f((bf16_t)(wm[k] & 0xffff)), m1 = bf2f((bf16_t)(wm[k] >> 16));
      float v0 = bf2f((bf16_t)(wv[k] & 0xffff)), v1 = bf2f((bf16_t)(wv[k] >> 16));
      adam_one(p0, bf2f((bf16_t)(wg[k] & 0xffff)), m0, v0, a, coef);
      adam_one(p1, bf2f((bf16_t)(wg[k] >> 16)), m1, v1, a, coef);
      op[k] = pack2bf(p0, p1); om[k] = pack2bf(m0, m1); ov[k] = pack2bf(v0, v1);
    }
    reinterpret_cast<uint4*>(a.p)[i] = make_uint4(op[0], op[1], op[2], op[3]);
    reinterpret_cast<uint4*>(a.m)[i] = make_uint4(om[0], om[1], om[2], om[3]);
    reinterpret_cast<uint4*>(a.v)[i] = make_uint4(ov[0], ov[1], ov[2], ov[3]);
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < a.n; i += 256) {
      float p = bf2f(a.p[i]), m = bf2f(a.m[i]), v = bf2f(a.v[i]);
      adam_one(p, bf2f(a.g[i]), m, v, a, coef);
      a.p[i] = f2bf(p); a.m[i] = f2bf(m); a.v[i] = f2bf(v);
    }
}
__global__ __launch_bounds__(256) void adamw_master_guarded_kernel(MasterArgs a, const dvla_step_state* __restrict__ st) {
  if (st->ok == 0) return;
  a.bc2_sqrt = st->bc2_sqrt; a.step_size = st->step_size;
  adamw_master_body(a);
}

// ---- EMA of the weights inside the step (additive; dvla.h) ------------------------------------------------------
// One more fp32 stream through the loops above: e <- lerp(e, p, w) on the parameter the step has just produced, as ATen's lerp
// computes it (the expression master_one restates for exp_avg).  The loops are restated, not shared with the kernels above,
// whose instruction streams are to stay as they are; every element still goes through adam_one / master_one.
struct EmaArgs { float* e; float w, omw; int w_small; };        // omw = 1 - w in fp32, w_small = |w| < 0.5: lerp's branch

__device__ __forceinline__ EmaArgs ema_args(float* e, float w) {
  EmaArgs x;
  x.e = e; x.w = w; x.omw = 1.0f - w; x.w_small = fabsf(w) < 0.5f;
  return x;
}
__device__ __forceinline__ void ema_one(float& e, float p, const EmaArgs& x) {
  const float d = __fsub_rn(p, e);
  e = x.w_small ? fmaf(x.w, d, e) : fmaf(-d, x.omw, p);
}

__device__ __forceinline__ void adamw_master_ema_body(MasterArgs a, EmaArgs x) {
  float coef = 1.0f;
  if (a.sumsq) {
    const float c = a.max_norm / (sqrtf(a.sumsq[0]) + 1e-6f);
    coef = c < 1.0f ? c : 1.0f;
  }
  const int64_t nvec = a.n >> 3;      // 8 elements per thread: 2 x 16 B of each of the five fp32 streams, 16 B of shadow
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float4 p4[2], g4[2], m4[2], v4[2], e4[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      p4[h] = reinterpret_cast<const float4*>(a.p)[2 * i + h]; g4[h] = reinterpret_cast<const float4*>(a.g)[2 * i + h];
      m4[h] = reinterpret_cast<const float4*>(a.m)[2 * i + h]; v4[h] = reinterpret_cast<const float4*>(a.v)[2 * i + h];
      e4[h] = reinterpret_cast<const float4*>(x.e)[2 * i + h];
    }
    uint32_t sh[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      master_one(p4[h].x, g4[h].x, m4[h].x, v4[h].x, a, coef);
      master_one(p4[h].y, g4[h].y, m4[h].y, v4[h].y, a, coef);
      master_one(p4[h].z, g4[h].z, m4[h].z, v4[h].z, a, coef);
      master_one(p4[h].w, g4[h].w, m4[h].w, v4[h].w, a, coef);
      ema_one(e4[h].x, p4[h].x, x); ema_one(e4[h].y, p4[h].y, x); ema_one(e4[h].z, p4[h].z, x); ema_one(e4[h].w, p4[h].w, x);
      sh[2 * h] = pack2bf(p4[h].x, p4[h].y); sh[2 * h + 1] = pack2bf(p4[h].z, p4[h].w);
      reinterpret_cast<float4*>(a.p)[2 * i + h] = p4[h];
      reinterpret_cast<float4*>(a.m)[2 * i + h] = m4[h];
      reinterpret_cast<float4*>(a.v)[2 * i + h] = v4[h];
      reinterpret_cast<float4*>(x.e)[2 * i + h] = e4[h];
    }
    if (a.sh) reinterpret_cast<uint4*>(a.sh)[i] = make_uint4(sh[0], sh[1], sh[2], sh[3]);
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nvec << 3) + threadIdx.x; i < a.n; i += 256) {
      float p = a.p[i], m = a.m[i], v = a.v[i], e = x.e[i];
      master_one(p, a.g[i], m, v, a, coef);
      ema_one(e, p, x);
      a.p[i] = p; a.m[i] = m; a.v[i] = v; x.e[i] = e;
      if (a.sh) a.sh[i] = f2bf(p);
    }
}

// The bf16 loop with the EMA (the EMA follows the bf16 value that is written: the parameter as every later reader sees it).
// adam_one is plain C++, and which of its products the compiler fuses into an fma depends on where the loop stands: inside a
// function that takes AdamArgs -- shared by the two kernels below -- LLVM's reassociation pass orders the two products of the
// exp_avg_sq line the other way round than it does in adamw_kernel, the other one is fused, and 2 elements in a million come
// out one bf16 ulp away.  So the loop is expanded in each kernel body, on the kernel's own argument `a`, where it compiles to
// adamw_kernel's arithmetic (tests/test_ema_step_gpu.py compares 8 million elements with dvla_adamw_bf16, bit for bit).
// a: AdamArgs, x: EmaArgs, both kernel-local.  8 elements per thread: 16 B of each bf16 stream, 2 x 16 B of the EMA.
#define DVLA_ADAMW_EMA_LOOP(a, x)                                                                                              \
  {                                                                                                                            \
    float coef = 1.0f;                                                                                                         \
    if (a.sumsq) {                                                                                                             \
      const float c = a.max_norm / (sqrtf(a.sumsq[0]) + 1e-6f);                                                                \
      coef = c < 1.0f ? c : 1.0f;                                                                                              \
    }                                                                                                                          \
    const int64_t nvec = a.n >> 3;                                                                                             \
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {                       \
      const uint4 up = reinterpret_cast<const uint4*>(a.p)[i], ug = reinterpret_cast<const uint4*>(a.g)[i];                    \
      const uint4 um = reinterpret_cast<const uint4*>(a.m)[i], uv = reinterpret_cast<const uint4*>(a.v)[i];                    \
      const float4 e0 = reinterpret_cast<const float4*>(x.e)[2 * i], e1 = reinterpret_cast<const float4*>(x.e)[2 * i + 1];     \
      const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};                                       \
      const uint32_t wm[4] = {um.x, um.y, um.z, um.w}, wv[4] = {uv.x, uv.y, uv.z, uv.w};                                       \
      uint32_t op[4], om[4], ov[4];                                                                                            \
      float e[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};                                                           \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                          \
        float p0 = bf2f((bf16_t)(wp[k] & 0xffff)), p1 = bf2f((bf16_t)(wp[k] >> 16));                                           \
        float m0 = bf2f((bf16_t)(wm[k] & 0xffff)), m1 = bf2f((bf16_t)(wm[k] >> 16));                                           \
        float v0 = bf2f((bf16_t)(wv[k] & 0xffff)), v1 = bf2f((bf16_t)(wv[k] >> 16));                                           \
        adam_one(p0, bf2f((bf16_t)(wg[k] & 0xffff)), m0, v0, a, coef);                                                         \
        adam_one(p1, bf2f((bf16_t)(wg[k] >> 16)), m1, v1, a, coef);                                                            \
        op[k] = pack2bf(p0, p1); om[k] = pack2bf(m0, m1); ov[k] = pack2bf(v0, v1);                                             \
        ema_one(e[2 * k], bf2f((bf16_t)(op[k] & 0xffff)), x);                                                                  \
        ema_one(e[2 * k + 1], bf2f((bf16_t)(op[k] >> 16)), x);                                                                 \
      }                                                                                                                        \
      reinterpret_cast<uint4*>(a.p)[i] = make_uint4(op[0], op[1], op[2], op[3]);                                               \
      reinterpret_cast<uint4*>(a.m)[i] = make_uint4(om[0], om[1], om[2], om[3]);                                               \
      reinterpret_cast<uint4*>(a.v)[i] = make_uint4(ov[0], ov[1], ov[2], ov[3]);                                               \
      reinterpret_cast<float4*>(x.e)[2 * i] = make_float4(e[0], e[1], e[2], e[3]);                                             \
      reinterpret_cast<float4*>(x.e)[2 * i + 1] = make_float4(e[4], e[5], e[6], e[7]);                                         \
    }                                                                                                                          \
    if (blockIdx.x == 0)                                                                                                       \
      for (int64_t i = (nvec << 3) + threadIdx.x; i < a.n; i += 256) {                                                         \
        float p = bf2f(a.p[i]), m = bf2f(a.m[i]), v = bf2f(a.v[i]), e = x.e[i];                                                \
        adam_one(p, bf2f(a.g[i]), m, v, a, coef);                                                                              \
        const bf16_t pb = f2bf(p);                                                                                             \
        ema_one(e, bf2f(pb), x);                                                                                               \
        a.p[i] = pb; a.m[i] = f2bf(m); a.v[i] = f2bf(v); x.e[i] = e;                                                           \
      }                                                                                                                        \
  }

__global__ __launch_bounds__(256) void adamw_master_ema_kernel(MasterArgs a, float* ema, float w) {
  adamw_master_ema_body(a, ema_args(ema, w));
}
__global__ __launch_bounds__(256) void adamw_ema_kernel(AdamArgs a, float* ema, float w) {
  const EmaArgs x = ema_args(ema, w);
  DVLA_ADAMW_EMA_LOOP(a, x)
}

// the weights of every step count still possible, by value like VerdictArgs::c; the verdict's row (st->cand) is used
struct EmaTable { float w[DVLA_STEP_MAX_CANDIDATES]; };

__device__ __forceinline__ float ema_pick(const EmaTable& t, int cand) {
  float w = t.w[0];
#pragma unroll
  for (int k = 1; k < DVLA_STEP_MAX_CANDIDATES; ++k)                 // compare-and-select: t.w[cand] would go through scratch
    if (cand == k) w = t.w[k];
  return w;
}

__global__ __launch_bounds__(256) void adamw_master_ema_guarded_kernel(MasterArgs a, float* ema, EmaTable t,
                                                                       const dvla_step_state* __restrict__ st) {
  if (st->ok == 0) return;
  a.bc2_sqrt = st->bc2_sqrt; a.step_size = st->step_size;
  adamw_master_ema_body(a, ema_args(ema, ema_pick(t, st->cand)));
}
__global__ __launch_bounds__(256) void adamw_ema_guarded_kernel(AdamArgs a, float* ema, EmaTable t,
                                                                const dvla_step_state* __restrict__ st) {
  if (st->ok == 0) return;
  a.inv_bc1 = st->inv_bc1; a.inv_bc2_sqrt = st->inv_bc2_sqrt;
  const EmaArgs x = ema_args(ema, ema_pick(t, st->cand));
  DVLA_ADAMW_EMA_LOOP(a, x)
}
#undef DVLA_ADAMW_EMA_LOOP

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

// ---- parameter groups: per-group lr and weight decay in one launch per bucket (additive; dvla.h) ----------------
// A group map gives every vector of 8 elements its group (one byte; 255, or any id >= n_groups: the vector is left alone, nothing
// of it read or written).  What depends on the group travels by value in the kernel arguments, as VerdictArgs::c does; wave 0
// puts one row per group into LDS (constant indices only: a lane-varying index into a by-value array goes through scratch; the
// candidate row is wave-uniform and picked by compare-and-select), and every vector looks its row up by its map byte.  The
// map byte of the next round is fetched before this round's streams, so the dependent load is off the critical path.
template <int NC>
struct GroupTab {                   // master: x = decay, y = step_size per candidate count.  bf16: x = lr, y[0] = wd (NC = 1)
  float x[DVLA_STEP_MAX_GROUPS];
  float y[NC][DVLA_STEP_MAX_GROUPS];
};

template <int NC>
__device__ __forceinline__ float2 group_row(const GroupTab<NC>& t, int n_groups, int cand) {      // the row of group threadIdx.x
  float x = 0.f, y = 0.f;
#pragma unroll
  for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) {
    if (g >= n_groups) break;                                        // uniform: two or three groups cost two or three rounds
    float yg = t.y[0][g];
#pragma unroll
    for (int k = 1; k < NC; ++k)
      if (cand == k) yg = t.y[k][g];
    if ((int)threadIdx.x == g) { x = t.x[g]; y = yg; }
  }
  return make_float2(x, y);
}

__device__ __forceinline__ float clip_coef(const float* sumsq, float max_norm) {
  if (!sumsq) return 1.0f;
  const float c = max_norm / (sqrtf(sumsq[0]) + 1e-6f);
  return c < 1.0f ? c : 1.0f;
}

// Per-group clipping (CLIP; dvla.h: dvla_adamw_*_clip): the groups' sums of squares stay in device memory, their max_norm travel by
// value, and wave 0 puts one coefficient per group -- clip_coef itself on (&sumsq[g], max_norm[g]) -- into LDS next to the group's
// row.  Without CLIP the struct is empty and the LAST kernel argument, and every `if (CLIP)` folds away: the kernels of the
// entry points without `_clip` keep their instruction streams.
template <bool CLIP> struct ClipTab {};
template <> struct ClipTab<true> { const float* sumsq; float max_norm[DVLA_STEP_MAX_GROUPS]; };

// the coefficient of group threadIdx.x; `off` for a group that is not clipped (max_norm <= 0 or NaN: its sum is not read)
__device__ __forceinline__ float group_coef(const ClipTab<true>& c, int n_groups, float off) {
  float mx = 0.f;
#pragma unroll
  for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) {
    if (g >= n_groups) break;                                        // uniform, as in group_row
    if ((int)threadIdx.x == g) mx = c.max_norm[g];
  }
  return mx > 0.f ? clip_coef(c.sumsq + threadIdx.x, mx) : off;
}
__device__ __forceinline__ float group_coef(const ClipTab<false>&, int, float off) { return off; }

// GUARD: the verdict and the step-dependent scalars come from *st (adamw_master_guarded_kernel); EMA: + ema_one on the
// parameter just written (adamw_master_ema_body).  Every element goes through master_one, on a copy of the arguments that
// carries its group's decay and step_size -- CLIP: and its group's clip, sumsq null for a group that is not clipped (coefficient
// < 0 in LDS), as the one-group entry point gets it.
template <bool GUARD, bool EMA, bool CLIP = false>
__global__ __launch_bounds__(256) void adamw_master_grouped_kernel(MasterArgs a, const uint8_t* __restrict__ map, int n_groups,
                                                                   GroupTab<GUARD ? DVLA_STEP_MAX_CANDIDATES : 1> t, float* ema,
                                                                   EmaTable wt, const dvla_step_state* __restrict__ st,
                                                                   ClipTab<CLIP> ct) {
  __shared__ float2 rows[DVLA_STEP_MAX_GROUPS];
  __shared__ float coefs[CLIP ? DVLA_STEP_MAX_GROUPS : 1];
  int cand = 0;
  if (GUARD) {
    if (st->ok == 0) return;
    a.bc2_sqrt = st->bc2_sqrt;
    cand = st->cand;
  }
  if (threadIdx.x < DVLA_STEP_MAX_GROUPS) rows[threadIdx.x] = group_row(t, n_groups, cand);
  if (CLIP) {
    if (threadIdx.x < DVLA_STEP_MAX_GROUPS) coefs[threadIdx.x] = group_coef(ct, n_groups, -1.0f);
  }
  __syncthreads();
  const EmaArgs x = ema_args(ema, EMA ? ema_pick(wt, cand) : 0.f);
  float coef = 1.0f;
  if (!CLIP) coef = clip_coef(a.sumsq, a.max_norm);
  const int64_t nvec = a.n >> 3, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned id = i < nvec ? map[i] : 255u;
  while (i < nvec) {
    const int64_t nx = i + stride;
    const unsigned id_nx = nx < nvec ? map[nx] : 255u;
    if (id < (unsigned)n_groups) {
      const float2 r = rows[id];
      MasterArgs b = a;
      b.decay = r.x; b.step_size = r.y;
      if constexpr (CLIP) { coef = coefs[id]; b.sumsq = coef < 0.f ? nullptr : ct.sumsq; }
      float4 p4[2], g4[2], m4[2], v4[2], e4[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        p4[h] = reinterpret_cast<const float4*>(a.p)[2 * i + h]; g4[h] = reinterpret_cast<const float4*>(a.g)[2 * i + h];
        m4[h] = reinterpret_cast<const float4*>(a.m)[2 * i + h]; v4[h] = reinterpret_cast<const float4*>(a.v)[2 * i + h];
        if (EMA) e4[h] = reinterpret_cast<const float4*>(x.e)[2 * i + h];
      }
      uint32_t sh[4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        master_one(p4[h].x, g4[h].x, m4[h].x, v4[h].x, b, coef);
        master_one(p4[h].y, g4[h].y, m4[h].y, v4[h].y, b, coef);
        master_one(p4[h].z, g4[h].z, m4[h].z, v4[h].z, b, coef);
        master_one(p4[h].w, g4[h].w, m4[h].w, v4[h].w, b, coef);
        sh[2 * h] = pack2bf(p4[h].x, p4[h].y); sh[2 * h + 1] = pack2bf(p4[h].z, p4[h].w);
        reinterpret_cast<float4*>(a.p)[2 * i + h] = p4[h];
        reinterpret_cast<float4*>(a.m)[2 * i + h] = m4[h];
        reinterpret_cast<float4*>(a.v)[2 * i + h] = v4[h];
        if (EMA) {
          ema_one(e4[h].x, p4[h].x, x); ema_one(e4[h].y, p4[h].y, x); ema_one(e4[h].z, p4[h].z, x); ema_one(e4[h].w, p4[h].w, x);
          reinterpret_cast<float4*>(x.e)[2 * i + h] = e4[h];
        }
      }
      if (a.sh) reinterpret_cast<uint4*>(a.sh)[i] = make_uint4(sh[0], sh[1], sh[2], sh[3]);
    }
    i = nx; id = id_nx;
  }
  if (blockIdx.x == 0 && (nvec << 3) < a.n) {      // the ragged tail (n % 8 elements) belongs to the last map byte
    const unsigned idt = map[nvec];
    if (idt < (unsigned)n_groups) {
      const float2 r = rows[idt];
      MasterArgs b = a;
      b.decay = r.x; b.step_size = r.y;
      if constexpr (CLIP) { coef = coefs[idt]; b.sumsq = coef < 0.f ? nullptr : ct.sumsq; }
      for (int64_t j = (nvec << 3) + threadIdx.x; j < a.n; j += 256) {
        float p = a.p[j], m = a.m[j], v = a.v[j];
        master_one(p, a.g[j], m, v, b, coef);
        a.p[j] = p; a.m[j] = m; a.v[j] = v;
        if (EMA) { float e = x.e[j]; ema_one(e, p, x); x.e[j] = e; }
        if (a.sh) a.sh[j] = f2bf(p);
      }
    }
  }
}

// The bf16 element function with its roundings written out.  adam_one is plain C++ and the compiler decides which of its
// products to fuse, differently in adamw_kernel's vector loop and in its ragged-tail loop; with lr and wd per vector instead of
// per launch it would decide once more.  So both forms are restated here as adamw_kernel's instructions have them (nothing is
// contracted inside these two functions; tests/test_param_groups_gpu.py compares 9 million elements with dvla_adamw_bf16):
//   vector loop: decay = fma(-lr, wd, 1), v = fma(beta2, v, ((1 - beta2) g) g), p = fma(decay, p, -((lr inv_bc1) (m / denom)))
//   tail loop:   decay = 1 - lr wd,       v = beta2 v + ((1 - beta2) g) g,     p = decay p - (lr inv_bc1) (m / denom)
// and in both m = fma(1 - beta1, g - m, m), denom = fma(sqrt(v), inv_bc2_sqrt, eps).
template <bool TAIL>
__device__ __forceinline__ void adam_group_one(float& p, float g, float& m, float& v, const AdamArgs& a, float lr, float wd,
                                               float coef) {
#pragma clang fp contract(off)
  g = bf2f(f2bf(g * coef));
  const float gg = ((1.0f - a.beta2) * g) * g, step = lr * a.inv_bc1;
  v = TAIL ? a.beta2 * v + gg : fmaf(a.beta2, v, gg);
  m = fmaf(1.0f - a.beta1, g - m, m);
  const float q = step * (m / fmaf(sqrtf(v), a.inv_bc2_sqrt, a.eps));
  p = TAIL ? (1.0f - lr * wd) * p - q : fmaf(fmaf(-lr, wd, 1.0f), p, -q);
}

// CLIP: the coefficient is the group's (1 for a group that is not clipped: adam_one multiplies by 1 without a clip as well).
template <bool GUARD, bool EMA, bool CLIP = false>
__global__ __launch_bounds__(256) void adamw_grouped_kernel(AdamArgs a, const uint8_t* __restrict__ map, int n_groups, GroupTab<1> t,
                                                            float* ema, EmaTable wt, const dvla_step_state* __restrict__ st,
                                                            ClipTab<CLIP> ct) {
  __shared__ float2 rows[DVLA_STEP_MAX_GROUPS];
  __shared__ float coefs[CLIP ? DVLA_STEP_MAX_GROUPS : 1];
  int cand = 0;
  if (GUARD) {
    if (st->ok == 0) return;
    a.inv_bc1 = st->inv_bc1; a.inv_bc2_sqrt = st->inv_bc2_sqrt;
    cand = st->cand;
  }
  if (threadIdx.x < DVLA_STEP_MAX_GROUPS) rows[threadIdx.x] = group_row(t, n_groups, 0);
  if (CLIP) {
    if (threadIdx.x < DVLA_STEP_MAX_GROUPS) coefs[threadIdx.x] = group_coef(ct, n_groups, 1.0f);
  }
  __syncthreads();
  const EmaArgs x = ema_args(ema, EMA ? ema_pick(wt, cand) : 0.f);
  float coef = 1.0f;
  if (!CLIP) coef = clip_coef(a.sumsq, a.max_norm);
  const int64_t nvec = a.n >> 3, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned id = i < nvec ? map[i] : 255u;
  while (i < nvec) {
    const int64_t nx = i + stride;
    const unsigned id_nx = nx < nvec ? map[nx] : 255u;
    if (id < (unsigned)n_groups) {
      const float2 r = rows[id];      // lr, wd
      if (CLIP) coef = coefs[id];
      const uint4 up = reinterpret_cast<const uint4*>(a.p)[i], ug = reinterpret_cast<const uint4*>(a.g)[i];
      const uint4 um = reinterpret_cast<const uint4*>(a.m)[i], uv = reinterpret_cast<const uint4*>(a.v)[i];
      float4 e0, e1;
      if (EMA) { e0 = reinterpret_cast<const float4*>(x.e)[2 * i]; e1 = reinterpret_cast<const float4*>(x.e)[2 * i + 1]; }
      const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
      const uint32_t wm[4] = {um.x, um.y, um.z, um.w}, wv[4] = {uv.x, uv.y, uv.z, uv.w};
      uint32_t op[4], om[4], ov[4];
      float e[8];
      if (EMA) { e[0] = e0.x; e[1] = e0.y; e[2] = e0.z; e[3] = e0.w; e[4] = e1.x; e[5] = e1.y; e[6] = e1.z; e[7] = e1.w; }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float p0 = bf2f((bf16_t)(wp[k] & 0xffff)), p1 = bf2f((bf16_t)(wp[k] >> 16));
        float m0 = bf2f((bf16_t)(wm[k] & 0xffff)), m1 = bf2f((bf16_t)(wm[k] >> 16));
        float v0 = bf2f((bf16_t)(wv[k] & 0xffff)), v1 = bf2f((bf16_t)(wv[k] >> 16));
        adam_group_one<false>(p0, bf2f((bf16_t)(wg[k] & 0xffff)), m0, v0, a, r.x, r.y, coef);
        adam_group_one<false>(p1, bf2f((bf16_t)(wg[k] >> 16)), m1, v1, a, r.x, r.y, coef);
        op[k] = pack2bf(p0, p1); om[k] = pack2bf(m0, m1); ov[k] = pack2bf(v0, v1);
        if (EMA) {      // the EMA follows the bf16 value that is written
          ema_one(e[2 * k], bf2f((bf16_t)(op[k] & 0xffff)), x);
          ema_one(e[2 * k + 1], bf2f((bf16_t)(op[k] >> 16)), x);
        }
      }
      reinterpret_cast<uint4*>(a.p)[i] = make_uint4(op[0], op[1], op[2], op[3]);
      reinterpret_cast<uint4*>(a.m)[i] = make_uint4(om[0], om[1], om[2], om[3]);
      reinterpret_cast<uint4*>(a.v)[i] = make_uint4(ov[0], ov[1], ov[2], ov[3]);
      if (EMA) {
        reinterpret_cast<float4*>(x.e)[2 * i] = make_float4(e[0], e[1], e[2], e[3]);
        reinterpret_cast<float4*>(x.e)[2 * i + 1] = make_float4(e[4], e[5], e[6], e[7]);
      }
    }
    i = nx; id = id_nx;
  }
  if (blockIdx.x == 0 && (nvec << 3) < a.n) {      // the ragged tail (n % 8 elements) belongs to the last map byte
    const unsigned idt = map[nvec];
    if (idt < (unsigned)n_groups) {
      const float2 r = rows[idt];
      if (CLIP) coef = coefs[idt];
      for (int64_t j = (nvec << 3) + threadIdx.x; j < a.n; j += 256) {
        float p = bf2f(a.p[j]), m = bf2f(a.m[j]), v = bf2f(a.v[j]);
        adam_group_one<true>(p, bf2f(a.g[j]), m, v, a, r.x, r.y, coef);
        const bf16_t pb = f2bf(p);
        a.p[j] = pb; a.m[j] = f2bf(m); a.v[j] = f2bf(v);
        if (EMA) { float e = x.e[j]; ema_one(e, bf2f(pb), x); x.e[j] = e; }
      }
    }
  }
}

// ---- stochastic rounding of the bf16 stores (additive; dvla.h) --------------------------------------------------
// The generator and the rounding as dvla.h states them (tests/sr_ref.py restates both in integer arithmetic): 16 random bits per
// stored value from two hashes per element, keyed by (seed, applied step count, bucket) and the element's index in its bucket.
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

struct SrArgs { uint64_t seed; int64_t step, base; uint32_t bucket; };      // step: unguarded; base: the index of element 0

// adamw_grouped_kernel with the three final conversions rounded stochastically: the same element function (adam_group_one, so
// the fp32 values are those of every other bf16 step kernel), the same guard, EMA (on the parameter as stored) and map.
// MAP false: no map, one group (row 0 of the table) over all n elements -- the one-group step over a range of a bucket.
// CLIP (with MAP only): the coefficient per group, as in adamw_grouped_kernel.
template <bool GUARD, bool EMA, bool MAP, bool CLIP = false>
__global__ __launch_bounds__(256) void adamw_sr_kernel(AdamArgs a, const uint8_t* __restrict__ map, int n_groups, GroupTab<1> t,
                                                       float* ema, EmaTable wt, const dvla_step_state* __restrict__ st, SrArgs sr,
                                                       ClipTab<CLIP> ct) {
  static_assert(MAP || !CLIP, "a coefficient per group needs the group map");
  __shared__ float2 rows[DVLA_STEP_MAX_GROUPS];
  __shared__ float coefs[CLIP ? DVLA_STEP_MAX_GROUPS : 1];
  int cand = 0;
  if (GUARD) {
    if (st->ok == 0) return;
    a.inv_bc1 = st->inv_bc1; a.inv_bc2_sqrt = st->inv_bc2_sqrt;
    cand = st->cand;
  }
  const uint32_t key = sr_key(sr.seed, GUARD ? (uint64_t)st->applied : (uint64_t)sr.step, sr.bucket);
  if (MAP) {
    if (threadIdx.x < DVLA_STEP_MAX_GROUPS) rows[threadIdx.x] = group_row(t, n_groups, 0);
    if (CLIP) {
      if (threadIdx.x < DVLA_STEP_MAX_GROUPS) coefs[threadIdx.x] = group_coef(ct, n_groups, 1.0f);
    }
    __syncthreads();
  }
  const float2 r0 = make_float2(t.x[0], t.y[0][0]);
  const EmaArgs x = ema_args(ema, EMA ? ema_pick(wt, cand) : 0.f);
  float coef = 1.0f;
  if (!CLIP) coef = clip_coef(a.sumsq, a.max_norm);
  const int64_t nvec = a.n >> 3, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned id = 0;
  if (MAP) id = i < nvec ? map[i] : 255u;
  while (i < nvec) {
    const int64_t nx = i + stride;
    unsigned id_nx = 0;
    if (MAP) id_nx = nx < nvec ? map[nx] : 255u;
    if (id < (unsigned)n_groups) {
      const float2 r = MAP ? rows[id] : r0;      // lr, wd
      if (CLIP) coef = coefs[id];
      const uint4 up = reinterpret_cast<const uint4*>(a.p)[i], ug = reinterpret_cast<const uint4*>(a.g)[i];
      const uint4 um = reinterpret_cast<const uint4*>(a.m)[i], uv = reinterpret_cast<const uint4*>(a.v)[i];
      float4 e0, e1;
      if (EMA) { e0 = reinterpret_cast<const float4*>(x.e)[2 * i]; e1 = reinterpret_cast<const float4*>(x.e)[2 * i + 1]; }
      const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
      const uint32_t wm[4] = {um.x, um.y, um.z, um.w}, wv[4] = {uv.x, uv.y, uv.z, uv.w};
      uint32_t op[4], om[4], ov[4];
      float e[8];
      if (EMA) { e[0] = e0.x; e[1] = e0.y; e[2] = e0.z; e[3] = e0.w; e[4] = e1.x; e[5] = e1.y; e[6] = e1.z; e[7] = e1.w; }
      const int64_t el = sr.base + (i << 3);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float p0 = bf2f((bf16_t)(wp[k] & 0xffff)), p1 = bf2f((bf16_t)(wp[k] >> 16));
        float m0 = bf2f((bf16_t)(wm[k] & 0xffff)), m1 = bf2f((bf16_t)(wm[k] >> 16));
        float v0 = bf2f((bf16_t)(wv[k] & 0xffff)), v1 = bf2f((bf16_t)(wv[k] >> 16));
        adam_group_one<false>(p0, bf2f((bf16_t)(wg[k] & 0xffff)), m0, v0, a, r.x, r.y, coef);
        adam_group_one<false>(p1, bf2f((bf16_t)(wg[k] >> 16)), m1, v1, a, r.x, r.y, coef);
        uint32_t pb0, mb0, vb0, pb1, mb1, vb1;
        sr_round3(p0, m0, v0, key, el + 2 * k, pb0, mb0, vb0);
        sr_round3(p1, m1, v1, key, el + 2 * k + 1, pb1, mb1, vb1);
        op[k] = pb0 | (pb1 << 16); om[k] = mb0 | (mb1 << 16); ov[k] = vb0 | (vb1 << 16);
        if (EMA) {      // the EMA follows the bf16 value that is written
          ema_one(e[2 * k], bf2f((bf16_t)pb0), x);
          ema_one(e[2 * k + 1], bf2f((bf16_t)pb1), x);
        }
      }
      reinterpret_cast<uint4*>(a.p)[i] = make_uint4(op[0], op[1], op[2], op[3]);
      reinterpret_cast<uint4*>(a.m)[i] = make_uint4(om[0], om[1], om[2], om[3]);
      reinterpret_cast<uint4*>(a.v)[i] = make_uint4(ov[0], ov[1], ov[2], ov[3]);
      if (EMA) {
        reinterpret_cast<float4*>(x.e)[2 * i] = make_float4(e[0], e[1], e[2], e[3]);
        reinterpret_cast<float4*>(x.e)[2 * i + 1] = make_float4(e[4], e[5], e[6], e[7]);
      }
    }
    i = nx; id = id_nx;
  }
  if (blockIdx.x == 0 && (nvec << 3) < a.n) {      // the ragged tail (n % 8 elements) belongs to the last map byte
    const unsigned idt = MAP ? map[nvec] : 0u;
    if (idt < (unsigned)n_groups) {
      const float2 r = MAP ? rows[idt] : r0;
      if (CLIP) coef = coefs[idt];
      for (int64_t j = (nvec << 3) + threadIdx.x; j < a.n; j += 256) {
        float p = bf2f(a.p[j]), m = bf2f(a.m[j]), v = bf2f(a.v[j]);
        adam_group_one<true>(p, bf2f(a.g[j]), m, v, a, r.x, r.y, coef);
        uint32_t pb, mb, vb;
        sr_round3(p, m, v, key, sr.base + j, pb, mb, vb);
        a.p[j] = (bf16_t)pb; a.m[j] = (bf16_t)mb; a.v[j] = (bf16_t)vb;
        if (EMA) { float e = x.e[j]; ema_one(e, bf2f((bf16_t)pb), x); x.e[j] = e; }
      }
    }
  }
}

inline unsigned step_blocks(int64_t n) {      // 8 elements per thread, at most 4096 blocks (grid-stride beyond)
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
inline void ema_table(EmaTable& t, const float* w, int n_cand) {
  for (int j = 0; j < DVLA_STEP_MAX_CANDIDATES; ++j) t.w[j] = w[j < n_cand ? j : n_cand - 1];
}

}  // namespace

extern "C" int64_t dvla_sumsq_partial_len(void) { return SS_BLOCKS; }

extern "C" int dvla_sumsq_bf16(const void* x, int64_t n, float* partial, float* out, int32_t accumulate, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!x || !partial || !out || n < 0) return DVLA_ERR_ARG;
  if (!al16(x)) return DVLA_ERR_UNSUPPORTED;
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > SS_BLOCKS) blocks = SS_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const bf16_t*>(x), n, partial);
  int rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, partial, (int)blocks, out, (int)accumulate);
  return dvla_check_launch();
}

extern "C" int dvla_adamw_bf16(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int64_t step, const float* grad_sumsq, float max_norm,
                               void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq)) return DVLA_ERR_UNSUPPORTED;
  AdamArgs a;
  a.p = reinterpret_cast<bf16_t*>(param); a.g = reinterpret_cast<const bf16_t*>(grad);
  a.m = reinterpret_cast<bf16_t*>(exp_avg); a.v = reinterpret_cast<bf16_t*>(exp_avg_sq); a.n = n;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  bf16_step_scalars(beta1, beta2, step, &a.inv_bc1, &a.inv_bc2_sqrt);
  a.sumsq = grad_sumsq; a.max_norm = max_norm;
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return dvla_check_launch();
}

extern "C" int dvla_sumsq_f32(const float* x, int64_t n, float* partial, float* out, int32_t accumulate, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!x || !partial || !out || n < 0) return DVLA_ERR_ARG;
  if (!al16(x)) return DVLA_ERR_UNSUPPORTED;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > SS_BLOCKS) blocks = SS_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sumsq_f32_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, partial);
  int rc = dvla_check_launch();
  if (rc != DVLA_OK) return rc;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, partial, (int)blocks, out, (int)accumulate);
  return dvla_check_launch();
}

extern "C" int dvla_adamw_f32_master(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                     int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                     int64_t step, const float* grad_sumsq, float max_norm, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (shadow_bf16 && !al16(shadow_bf16)))
    return DVLA_ERR_UNSUPPORTED;
  MasterArgs a;
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.sh = reinterpret_cast<bf16_t*>(shadow_bf16); a.n = n;
  // the scalars as torch/optim/adam.py (_multi_tensor_adam, capturable=False) computes them in Python floats
  master_fixed_scalars(a, lr, beta1, beta2, eps, weight_decay);
  master_step_scalars(lr, beta1, beta2, step, &a.bc2_sqrt, &a.step_size);
  a.sumsq = grad_sumsq; a.max_norm = max_norm;
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_master_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return dvla_check_launch();
}

// ---- guarded step (additive, ABI 9) -----------------------------------------------------------------------------------------
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

extern "C" int dvla_adamw_bf16_guarded(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                       const dvla_step_state* state, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || !state || n < 0) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || !al16(state)) return DVLA_ERR_UNSUPPORTED;
  AdamArgs a;
  a.p = reinterpret_cast<bf16_t*>(param); a.g = reinterpret_cast<const bf16_t*>(grad);
  a.m = reinterpret_cast<bf16_t*>(exp_avg); a.v = reinterpret_cast<bf16_t*>(exp_avg_sq); a.n = n;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.inv_bc1 = a.inv_bc2_sqrt = 0.f;           // the kernel takes both from the state
  a.sumsq = max_norm > 0.f ? &state->sumsq : nullptr; a.max_norm = max_norm;
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, state);
  return dvla_check_launch();
}

extern "C" int dvla_adamw_f32_master_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                             int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                             float max_norm, const dvla_step_state* state, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || !state || n < 0) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (shadow_bf16 && !al16(shadow_bf16)) || !al16(state))
    return DVLA_ERR_UNSUPPORTED;
  MasterArgs a;
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.sh = reinterpret_cast<bf16_t*>(shadow_bf16); a.n = n;
  master_fixed_scalars(a, lr, beta1, beta2, eps, weight_decay);
  a.bc2_sqrt = a.step_size = 0.f;             // the kernel takes both from the state
  a.sumsq = max_norm > 0.f ? &state->sumsq : nullptr; a.max_norm = max_norm;
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_master_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, state);
  return dvla_check_launch();
}

// ---- EMA of the weights (additive, ABI 9) -----------------------------------------------------------------------------------
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

extern "C" int dvla_adamw_bf16_ema(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* grad_sumsq,
                                   float max_norm, float ema_w, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || n < 0 || step < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || !al16(ema)) return DVLA_ERR_UNSUPPORTED;
  AdamArgs a;
  a.p = reinterpret_cast<bf16_t*>(param); a.g = reinterpret_cast<const bf16_t*>(grad);
  a.m = reinterpret_cast<bf16_t*>(exp_avg); a.v = reinterpret_cast<bf16_t*>(exp_avg_sq); a.n = n;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  bf16_step_scalars(beta1, beta2, step, &a.inv_bc1, &a.inv_bc2_sqrt);
  a.sumsq = grad_sumsq; a.max_norm = max_norm;
  hipLaunchKernelGGL(adamw_ema_kernel, dim3(step_blocks(n)), dim3(256), 0, stream, a, ema, ema_w);
  return dvla_check_launch();
}

extern "C" int dvla_adamw_f32_master_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                         float* ema, int64_t n, double lr, double beta1, double beta2, double eps,
                                         double weight_decay, int64_t step, const float* grad_sumsq, float max_norm, float ema_w,
                                         void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || n < 0 || step < 1) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (shadow_bf16 && !al16(shadow_bf16)) || !al16(ema))
    return DVLA_ERR_UNSUPPORTED;
  MasterArgs a;
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.sh = reinterpret_cast<bf16_t*>(shadow_bf16); a.n = n;
  master_fixed_scalars(a, lr, beta1, beta2, eps, weight_decay);
  master_step_scalars(lr, beta1, beta2, step, &a.bc2_sqrt, &a.step_size);
  a.sumsq = grad_sumsq; a.max_norm = max_norm;
  hipLaunchKernelGGL(adamw_master_ema_kernel, dim3(step_blocks(n)), dim3(256), 0, stream, a, ema, ema_w);
  return dvla_check_launch();
}

extern "C" int dvla_adamw_bf16_ema_guarded(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                           float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                           const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || !state || !ema_w || n < 0 || n_cand < 1 ||
      n_cand > DVLA_STEP_MAX_CANDIDATES)
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || !al16(ema) || !al16(state)) return DVLA_ERR_UNSUPPORTED;
  AdamArgs a;
  a.p = reinterpret_cast<bf16_t*>(param); a.g = reinterpret_cast<const bf16_t*>(grad);
  a.m = reinterpret_cast<bf16_t*>(exp_avg); a.v = reinterpret_cast<bf16_t*>(exp_avg_sq); a.n = n;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.inv_bc1 = a.inv_bc2_sqrt = 0.f;           // the kernel takes both from the state
  a.sumsq = max_norm > 0.f ? &state->sumsq : nullptr; a.max_norm = max_norm;
  EmaTable t;
  ema_table(t, ema_w, n_cand);
  hipLaunchKernelGGL(adamw_ema_guarded_kernel, dim3(step_blocks(n)), dim3(256), 0, stream, a, ema, t, state);
  return dvla_check_launch();
}

extern "C" int dvla_adamw_f32_master_ema_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                 void* shadow_bf16, float* ema, int64_t n, double lr, double beta1, double beta2,
                                                 double eps, double weight_decay, float max_norm, const dvla_step_state* state,
                                                 const float* ema_w, int32_t n_cand, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || !state || !ema_w || n < 0 || n_cand < 1 ||
      n_cand > DVLA_STEP_MAX_CANDIDATES)
    return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (shadow_bf16 && !al16(shadow_bf16)) || !al16(ema) ||
      !al16(state))
    return DVLA_ERR_UNSUPPORTED;
  MasterArgs a;
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.sh = reinterpret_cast<bf16_t*>(shadow_bf16); a.n = n;
  master_fixed_scalars(a, lr, beta1, beta2, eps, weight_decay);
  a.bc2_sqrt = a.step_size = 0.f;             // the kernel takes both from the state
  a.sumsq = max_norm > 0.f ? &state->sumsq : nullptr; a.max_norm = max_norm;
  EmaTable t;
  ema_table(t, ema_w, n_cand);
  hipLaunchKernelGGL(adamw_master_ema_guarded_kernel, dim3(step_blocks(n)), dim3(256), 0, stream, a, ema, t, state);
  return dvla_check_launch();
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

// ---- parameter groups (additive, ABI 9) -------------------------------------------------------------------------------------
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

namespace {

// what the grouped entry points check alike; returns DVLA_OK when the launch is to go ahead
inline int grouped_args(bool streams, int64_t n, const void* map, int32_t n_groups, const double* lr, const double* wd, int64_t step,
                        const dvla_step_state* state, const float* ema, const float* ema_w, int32_t n_cand) {
  if (!streams || !map || !lr || !wd || n < 0 || step < 1 || n_groups < 1 || n_groups > DVLA_STEP_MAX_GROUPS) return DVLA_ERR_ARG;
  if (ema && !ema_w) return DVLA_ERR_ARG;
  if (state && (n_cand < 1 || n_cand > DVLA_STEP_MAX_CANDIDATES)) return DVLA_ERR_ARG;
  return DVLA_OK;
}

template <int NC>
inline void group_tab(GroupTab<NC>& t, const dvla_group_row* rows, int32_t n_groups, bool master) {
  for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) {
    const dvla_group_row& r = rows[g < n_groups ? g : n_groups - 1];
    t.x[g] = master ? r.decay : r.lr;
    for (int k = 0; k < NC; ++k) t.y[k][g] = master ? r.step_size[k] : r.weight_decay;
  }
}

// the per-group clip of the `_clip` entry points: null (the entry points without it: one coefficient per launch) or both given
struct GroupClip { const float* sumsq; const float* max_norm; };

inline void clip_tab(ClipTab<true>& c, const GroupClip& clip, int32_t n_groups) {
  c.sumsq = clip.sumsq;
  for (int g = 0; g < DVLA_STEP_MAX_GROUPS; ++g) c.max_norm[g] = g < n_groups ? clip.max_norm[g] : 0.f;
}

// dvla_adamw_bf16_grouped and, with `clip`, dvla_adamw_bf16_grouped_clip
int bf16_grouped(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n, const uint8_t* group_map,
                 int32_t n_groups, const double* lr, const double* weight_decay, float beta1, float beta2, float eps, int64_t step,
                 const float* grad_sumsq, float max_norm, const GroupClip* clip, const dvla_step_state* state, const float* ema_w,
                 int32_t n_cand, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc = grouped_args(param && grad && exp_avg && exp_avg_sq, n, group_map, n_groups, lr, weight_decay, step, state, ema, ema_w,
                        n_cand);
  if (rc != DVLA_OK) return rc;
  if (clip && (!clip->sumsq || !clip->max_norm)) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (ema && !al16(ema)) || (state && !al16(state)))
    return DVLA_ERR_UNSUPPORTED;
  if (!state) n_cand = 1;
  dvla_group_row rows[DVLA_STEP_MAX_GROUPS];
  rc = dvla_group_scalars(lr, weight_decay, n_groups, beta1, beta2, step, n_cand, rows);
  if (rc != DVLA_OK) return rc;
  AdamArgs a;
  a.p = reinterpret_cast<bf16_t*>(param); a.g = reinterpret_cast<const bf16_t*>(grad);
  a.m = reinterpret_cast<bf16_t*>(exp_avg); a.v = reinterpret_cast<bf16_t*>(exp_avg_sq); a.n = n;
  a.lr = a.wd = 0.f;                          // per group: the kernel takes both from its table
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.inv_bc1 = a.inv_bc2_sqrt = 0.f;           // guarded: the kernel takes both from the state
  if (!state) bf16_step_scalars(beta1, beta2, step, &a.inv_bc1, &a.inv_bc2_sqrt);
  a.sumsq = state ? (max_norm > 0.f ? &state->sumsq : nullptr) : grad_sumsq; a.max_norm = max_norm;
  GroupTab<1> t;
  group_tab(t, rows, n_groups, false);
  EmaTable w;
  if (ema) ema_table(w, ema_w, n_cand); else for (float& x : w.w) x = 0.f;
  const dim3 grid(step_blocks(n)), block(256);
#define DVLA_GROUPED_LAUNCH(G, E, C, ct)                                                                                       \
  hipLaunchKernelGGL((adamw_grouped_kernel<G, E, C>), grid, block, 0, stream, a, group_map, n_groups, t, ema, w, state, ct)
  if (clip) {
    ClipTab<true> c;
    clip_tab(c, *clip, n_groups);
    if (state && ema) DVLA_GROUPED_LAUNCH(true, true, true, c);
    else if (state) DVLA_GROUPED_LAUNCH(true, false, true, c);
    else if (ema) DVLA_GROUPED_LAUNCH(false, true, true, c);
    else DVLA_GROUPED_LAUNCH(false, false, true, c);
  } else {
    const ClipTab<false> c{};
    if (state && ema) DVLA_GROUPED_LAUNCH(true, true, false, c);
    else if (state) DVLA_GROUPED_LAUNCH(true, false, false, c);
    else if (ema) DVLA_GROUPED_LAUNCH(false, true, false, c);
    else DVLA_GROUPED_LAUNCH(false, false, false, c);
  }
#undef DVLA_GROUPED_LAUNCH
  return dvla_check_launch();
}

// dvla_adamw_f32_master_grouped and, with `clip`, dvla_adamw_f32_master_grouped_clip
int master_grouped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, float* ema, int64_t n,
                   const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay, double beta1,
                   double beta2, double eps, int64_t step, const float* grad_sumsq, float max_norm, const GroupClip* clip,
                   const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc = grouped_args(param && grad && exp_avg && exp_avg_sq, n, group_map, n_groups, lr, weight_decay, step, state, ema, ema_w,
                        n_cand);
  if (rc != DVLA_OK) return rc;
  if (clip && (!clip->sumsq || !clip->max_norm)) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (shadow_bf16 && !al16(shadow_bf16)) ||
      (ema && !al16(ema)) || (state && !al16(state)))
    return DVLA_ERR_UNSUPPORTED;
  if (!state) n_cand = 1;
  dvla_group_row rows[DVLA_STEP_MAX_GROUPS];
  rc = dvla_group_scalars(lr, weight_decay, n_groups, beta1, beta2, step, n_cand, rows);
  if (rc != DVLA_OK) return rc;
  MasterArgs a;
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.sh = reinterpret_cast<bf16_t*>(shadow_bf16); a.n = n;
  master_fixed_scalars(a, lr[0], beta1, beta2, eps, weight_decay[0]);      // decay and step_size: per group, from the table
  master_step_scalars(lr[0], beta1, beta2, step, &a.bc2_sqrt, &a.step_size);      // guarded: the kernel takes bc2_sqrt from the state
  a.sumsq = state ? (max_norm > 0.f ? &state->sumsq : nullptr) : grad_sumsq; a.max_norm = max_norm;
  EmaTable w;
  if (ema) ema_table(w, ema_w, n_cand); else for (float& x : w.w) x = 0.f;
  const dim3 grid(step_blocks(n)), block(256);
  ClipTab<true> c;
  if (clip) clip_tab(c, *clip, n_groups);
  const ClipTab<false> none{};
#define DVLA_MASTER_LAUNCH(G, E)                                                                                               \
  if (clip) hipLaunchKernelGGL((adamw_master_grouped_kernel<G, E, true>), grid, block, 0, stream, a, group_map, n_groups, t, ema, w, \
                               state, c);                                                                                      \
  else hipLaunchKernelGGL((adamw_master_grouped_kernel<G, E, false>), grid, block, 0, stream, a, group_map, n_groups, t, ema, w,  \
                          state, none)
  if (state) {
    GroupTab<DVLA_STEP_MAX_CANDIDATES> t;
    group_tab(t, rows, n_groups, true);
    if (ema) { DVLA_MASTER_LAUNCH(true, true); } else { DVLA_MASTER_LAUNCH(true, false); }
  } else {
    GroupTab<1> t;
    group_tab(t, rows, n_groups, true);
    if (ema) { DVLA_MASTER_LAUNCH(false, true); } else { DVLA_MASTER_LAUNCH(false, false); }
  }
#undef DVLA_MASTER_LAUNCH
  return dvla_check_launch();
}

}  // namespace

extern "C" int dvla_adamw_bf16_grouped(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                       const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                       float beta1, float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm,
                                       const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream) {
  return bf16_grouped(param, grad, exp_avg, exp_avg_sq, ema, n, group_map, n_groups, lr, weight_decay, beta1, beta2, eps, step,
                      grad_sumsq, max_norm, nullptr, state, ema_w, n_cand, stream);
}

extern "C" int dvla_adamw_f32_master_grouped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                             float* ema, int64_t n, const uint8_t* group_map, int32_t n_groups, const double* lr,
                                             const double* weight_decay, double beta1, double beta2, double eps, int64_t step,
                                             const float* grad_sumsq, float max_norm, const dvla_step_state* state,
                                             const float* ema_w, int32_t n_cand, void* stream) {
  return master_grouped(param, grad, exp_avg, exp_avg_sq, shadow_bf16, ema, n, group_map, n_groups, lr, weight_decay, beta1, beta2,
                        eps, step, grad_sumsq, max_norm, nullptr, state, ema_w, n_cand, stream);
}

// ---- per-group clipping (additive, ABI 9) -----------------------------------------------------------------------------------
extern "C" int dvla_adamw_bf16_grouped_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                            const uint8_t* group_map, int32_t n_groups, const double* lr,
                                            const double* weight_decay, float beta1, float beta2, float eps, int64_t step,
                                            const float* group_sumsq, const float* max_norm, const dvla_step_state* state,
                                            const float* ema_w, int32_t n_cand, void* stream) {
  const GroupClip clip = {group_sumsq, max_norm};
  return bf16_grouped(param, grad, exp_avg, exp_avg_sq, ema, n, group_map, n_groups, lr, weight_decay, beta1, beta2, eps, step,
                      nullptr, 0.f, &clip, state, ema_w, n_cand, stream);
}

extern "C" int dvla_adamw_f32_master_grouped_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                  void* shadow_bf16, float* ema, int64_t n, const uint8_t* group_map,
                                                  int32_t n_groups, const double* lr, const double* weight_decay, double beta1,
                                                  double beta2, double eps, int64_t step, const float* group_sumsq,
                                                  const float* max_norm, const dvla_step_state* state, const float* ema_w,
                                                  int32_t n_cand, void* stream) {
  const GroupClip clip = {group_sumsq, max_norm};
  return master_grouped(param, grad, exp_avg, exp_avg_sq, shadow_bf16, ema, n, group_map, n_groups, lr, weight_decay, beta1, beta2,
                        eps, step, nullptr, 0.f, &clip, state, ema_w, n_cand, stream);
}

// ---- stochastic rounding (additive, ABI 9) ----------------------------------------------------------------------------------
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

namespace {

// dvla_adamw_bf16_sr and, with `clip` (and a map), dvla_adamw_bf16_sr_clip
int bf16_sr(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n, const uint8_t* group_map,
            int32_t n_groups, const double* lr, const double* weight_decay, float beta1, float beta2, float eps, int64_t step,
            const float* grad_sumsq, float max_norm, const GroupClip* clip, const dvla_step_state* state, const float* ema_w,
            int32_t n_cand, uint64_t sr_seed, int32_t sr_bucket, int64_t sr_index_base, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  static const uint8_t no_map = 0;      // grouped_args wants a map; without one there is one group
  if (!group_map && (n_groups != 1 || clip)) return DVLA_ERR_ARG;
  if (clip && (!clip->sumsq || !clip->max_norm)) return DVLA_ERR_ARG;
  int rc = grouped_args(param && grad && exp_avg && exp_avg_sq, n, group_map ? group_map : &no_map, n_groups, lr, weight_decay, step,
                        state, ema, ema_w, n_cand);
  if (rc != DVLA_OK) return rc;
  if (sr_index_base < 0) return DVLA_ERR_ARG;
  if (n == 0) return DVLA_OK;
  if (!al16(param) || !al16(grad) || !al16(exp_avg) || !al16(exp_avg_sq) || (ema && !al16(ema)) || (state && !al16(state)))
    return DVLA_ERR_UNSUPPORTED;
  if (!state) n_cand = 1;
  dvla_group_row rows[DVLA_STEP_MAX_GROUPS];
  rc = dvla_group_scalars(lr, weight_decay, n_groups, beta1, beta2, step, n_cand, rows);
  if (rc != DVLA_OK) return rc;
  AdamArgs a;
  a.p = reinterpret_cast<bf16_t*>(param); a.g = reinterpret_cast<const bf16_t*>(grad);
  a.m = reinterpret_cast<bf16_t*>(exp_avg); a.v = reinterpret_cast<bf16_t*>(exp_avg_sq); a.n = n;
  a.lr = a.wd = 0.f;                          // per group: the kernel takes both from its table
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.inv_bc1 = a.inv_bc2_sqrt = 0.f;           // guarded: the kernel takes both from the state
  if (!state) bf16_step_scalars(beta1, beta2, step, &a.inv_bc1, &a.inv_bc2_sqrt);
  a.sumsq = state ? (max_norm > 0.f ? &state->sumsq : nullptr) : grad_sumsq; a.max_norm = max_norm;
  GroupTab<1> t;
  group_tab(t, rows, n_groups, false);
  EmaTable w;
  if (ema) ema_table(w, ema_w, n_cand); else for (float& x : w.w) x = 0.f;
  SrArgs sr;
  sr.seed = sr_seed; sr.step = step; sr.base = sr_index_base; sr.bucket = (uint32_t)sr_bucket;
  const dim3 grid(step_blocks(n)), block(256);
  const ClipTab<false> none{};
#define DVLA_SR_LAUNCH(G, E, M, C, ct)                                                                                         \
  hipLaunchKernelGGL((adamw_sr_kernel<G, E, M, C>), grid, block, 0, stream, a, group_map, n_groups, t, ema, w, state, sr, ct)
  if (clip) {
    ClipTab<true> c;
    clip_tab(c, *clip, n_groups);
    switch ((state ? 4 : 0) | (ema ? 2 : 0)) {
      case 0: DVLA_SR_LAUNCH(false, false, true, true, c); break;
      case 2: DVLA_SR_LAUNCH(false, true, true, true, c); break;
      case 4: DVLA_SR_LAUNCH(true, false, true, true, c); break;
      default: DVLA_SR_LAUNCH(true, true, true, true, c); break;
    }
    return dvla_check_launch();
  }
  switch ((state ? 4 : 0) | (ema ? 2 : 0) | (group_map ? 1 : 0)) {
    case 0: DVLA_SR_LAUNCH(false, false, false, false, none); break;
    case 1: DVLA_SR_LAUNCH(false, false, true, false, none); break;
    case 2: DVLA_SR_LAUNCH(false, true, false, false, none); break;
    case 3: DVLA_SR_LAUNCH(false, true, true, false, none); break;
    case 4: DVLA_SR_LAUNCH(true, false, false, false, none); break;
    case 5: DVLA_SR_LAUNCH(true, false, true, false, none); break;
    case 6: DVLA_SR_LAUNCH(true, true, false, false, none); break;
    default: DVLA_SR_LAUNCH(true, true, true, false, none); break;
  }
#undef DVLA_SR_LAUNCH
  return dvla_check_launch();
}

}  // namespace

extern "C" int dvla_adamw_bf16_sr(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                  const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                  float beta1, float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm,
                                  const dvla_step_state* state, const float* ema_w, int32_t n_cand, uint64_t sr_seed,
                                  int32_t sr_bucket, int64_t sr_index_base, void* stream) {
  return bf16_sr(param, grad, exp_avg, exp_avg_sq, ema, n, group_map, n_groups, lr, weight_decay, beta1, beta2, eps, step, grad_sumsq,
                 max_norm, nullptr, state, ema_w, n_cand, sr_seed, sr_bucket, sr_index_base, stream);
}

extern "C" int dvla_adamw_bf16_sr_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                       const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                       float beta1, float beta2, float eps, int64_t step, const float* group_sumsq,
                                       const float* max_norm, const dvla_step_state* state, const float* ema_w, int32_t n_cand,
                                       uint64_t sr_seed, int32_t sr_bucket, int64_t sr_index_base, void* stream) {
  const GroupClip clip = {group_sumsq, max_norm};
  return bf16_sr(param, grad, exp_avg, exp_avg_sq, ema, n, group_map, n_groups, lr, weight_decay, beta1, beta2, eps, step, nullptr,
                 0.f, &clip, state, ema_w, n_cand, sr_seed, sr_bucket, sr_index_base, stream);
}
