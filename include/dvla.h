/* dvla.h -- C ABI of libdvla_hip.so: the hand-written CDNA4 (gfx950) kernels under DreamVLA's
 * transformer hot path.
 *
 * The reference (Zhangwenyao1/DreamVLA) has no native code and no FFI: every "kernel" on this path is
 * an ATen / F.scaled_dot_product_attention call issued from eager Python.  Each
 * entry point below therefore cites the reference *call sites* whose ATen op(s) it replaces; the
 * Python-side binding (ctypes) is dreamvla_amd/_lib.py and the drop-in nn.Module surface is
 * models/dreamvla_model.py.
 *
 * Conventions: plain pointers + sizes, no torch types.  All tensors are device pointers.  bf16 is the
 * raw 16-bit pattern.  Every function enqueues work on `stream` (a hipStream_t passed as void*),
 * never synchronises, is re-entrant per stream, and returns 0 on success or a negative DVLA_ERR_* code (no
 * exceptions cross the ABI).  Workspaces are the caller's (torch's caching allocator) with ONE exception: the
 * stream-K schedules of dvla_gemm_bf16 keep a 64-MiB slab area + flags per (device, stream), hipMalloc'ed at the
 * first launch that uses it (never during stream capture) and kept for the life of the process -- see
 * dvla_set_gemm_variant / dvla_set_gemm_schedule.  dtype codes: 0 = bf16, 1 = fp32.
 */
#ifndef DVLA_H_
#define DVLA_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DVLA_DT_BF16 0
#define DVLA_DT_F32 1

/* activation codes (applied in fp32 on the accumulator) */
#define DVLA_ACT_NONE 0
#define DVLA_ACT_GELU_ERF 1   /* timm Mlp nn.GELU():            models/vit_mae.py:73, dreamvla_model.py:349 */
#define DVLA_ACT_GELU_TANH 2  /* HF ACT2FN["gelu_new"]:         models/gpt2.py:292-301; DiT approx_gelu models.py:133 */
#define DVLA_ACT_RELU 3       /* action MLP head / depth pred:  dreamvla_model.py:458-471,842 */
#define DVLA_ACT_SILU 4       /* DiT TimestepEmbedder:          action_model/models.py:34 */
#define DVLA_ACT_QUICK_GELU 5 /* CLIP text tower QuickGELU (openai/CLIP model.py) */
#define DVLA_ACT_TANH 6
#define DVLA_ACT_SIGMOID 7

/* ABI revision of this header; dreamvla_amd/_lib.py refuses a library that reports another one (a stale prebuilt .so then fails
 * with a clear message instead of a missing-symbol error).  3 = round 3 (dvla_last_gemm_variant, variant 10, ...); 4 = k-sums on the
 * weight-gradient GEMM (ksum_* fields of dvla_gemm_params); 5 = dvla_ddim_cfg_step, dvla_act_bwd_colsum, a_layernorm,
 * GEMM configuration 11; 6 = dvla_dit_sample (the evaluation sampler as one persistent kernel); 7 = round 5: the sampler's
 * status word no longer carries over to the next launch (workspace words 33 / 34), dvla_dit_sample_inject_timeouts;
 * 9 = the three entry points that were aliases of a general form with fixed arguments (plain LayerNorm forward / backward, fp32
 * column sum) are removed: call dvla_layernorm_fwd_rows, dvla_layernorm_bwd_add and dvla_colsum_dt. */
#define DVLA_ABI_VERSION 9
int dvla_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue( A[M,K] * B[N,K]^T )     bf16 operands, fp32 MFMA accumulate
 *   a_trans = 0: A(m,k) at A[m*lda + k]      a_trans = 1: A(m,k) at A[k*lda + m]
 *   b_trans = 0: B(n,k) at B[n*ldb + k]  (nn.Linear weight (out,in))
 *   b_trans = 1: B(n,k) at B[k*ldb + n]  (HF Conv1D weight (in,out), models/gpt2.py:53-54,291-292)
 * epilogue, in order: v = acc; v += bias[n]; preact[m,n] = v; v = act(v); v *= act'(dact_aux[m,n]) (dact);
 *   v = dropout(v) (p, seed; element (m,n)); v += residual[m,n]; C = v (or C += v when accumulate, fp32 C).
 * Replaces: nn.Linear / Conv1D / timm PatchEmbed-as-GEMM + bias + GELU + dropout + residual add at
 *   models/vit_mae.py:188-203 (via timm Block), models/gpt2.py:160,172-173,296-301,329-339,
 *   models/perceiver_resampler.py:11-18,49-51,61, models/dreamvla_model.py:652-664,718-724,800-809,
 *   models/action_model/models.py:34-41,128-141,158-160, and their autograd backward GEMMs.
 * split_k > 1: K is cut in split_k slices written to `workspace` (split_k*M*N fp32) and reduced by a
 *   second kernel.  Plain epilogue, fp32 C and `accumulate` (the weight gradients), or bias / activation / residual applied by
 *   the reduction pass (forward GEMMs with few hundred rows and a long K); never with preact, dact_aux or dropout
 *   (DVLA_ERR_ARG).
 *
 * Addressing.  Every matrix has its own leading dimension (lda, ldb, ldc, ld_preact, ld_dact, ld_res, in elements) and may be a
 *   view into a wider buffer; the library writes the M x N windows of C and preact and nothing else.  residual with
 *   res_rows > 0 is a table of res_rows rows, row m % res_rows added to output row m.  bias is bf16 or fp32 (bias_dtype).
 *   * Vector paths (16-byte accesses) need, per matrix: a 16-byte aligned base and a leading dimension that is a multiple of
 *     8 elements (fp32 C: of 4); for the bias: a 16-byte aligned base.  Ragged sizes are fine for configuration 2 and 11; the
 *     ring / phase configurations (4, 6, 7, 8, 9, 10) additionally need N % 64 == 0 and whole K-tiles.
 *   * A call in which any of A, B, C, preact, dact_aux, residual or bias misses that is not taken by configurations 4 - 10:
 *     it runs on configuration 2 (register-staged kernel, element-wise guarded epilogue) whatever was forced, with the same
 *     values.  Configuration 11 needs A and B vectorisable only; a misaligned C / preact / dact_aux / residual / bias selects
 *     its element-wise epilogue.
 *   * An explicit split_k > 1 with bias / activation / residual needs N % 8 == 0 and vectorisable C, bias and residual:
 *     DVLA_ERR_UNSUPPORTED before any launch otherwise.
 *   * Stride bounds of configurations 4 - 10 (32-bit byte offsets inside a tile; wider views run on configuration 2, which
 *     addresses in 64 bits): for a k-contiguous operand (tile rows - 1) * ld * 2 + 2 * K-tile < 2^32, for an r-contiguous one
 *     (K-tile - 1) * ld * 2 + 2 * tile rows < 2^32; the phase kernel (8, 9, 10) also needs rows * ld * 2 < 2^32 for the whole
 *     of A and of B; and for C, preact, dact_aux and a residual with res_rows == 0: 127 * ld * element size + 64 * element
 *     size < 2^32, i.e. ld below about 16.9 M bf16 elements.
 */
typedef struct dvla_gemm_params {
  const void* A; int64_t lda; int32_t a_trans;
  const void* B; int64_t ldb; int32_t b_trans;
  void* C; int64_t ldc; int32_t c_dtype;
  int64_t M, N, K;
  const void* bias; int32_t bias_dtype;
  int32_t act;
  void* preact; int64_t ld_preact;
  const void* dact_aux; int64_t ld_dact; int32_t dact;
  float dropout_p; uint32_t seed_lo; uint32_t seed_hi;
  const void* residual; int64_t ld_res; int64_t res_rows; /* >0: residual row = m % res_rows (broadcast tables) */
  int32_t accumulate;
  int32_t split_k; void* workspace;
  /* (ABI 4) k-sums of one operand, computed by the GEMM that streams it anyway -- the bias gradient db = sum_m dz[m, :] of a
   * weight-gradient GEMM dW = dz^T x (utils/train_utils.py:599-608 leaves it to autograd's sum kernel):
   *   ksum_operand 0: none; 1: ksum[i] = sum_k A(i, k), i < M; 2: ksum[j] = sum_k B(j, k), j < N   (fp32 accumulation of the
   *   bf16 operand values, result in ksum_dtype = DVLA_DT_F32 / DVLA_DT_BF16).
   *   ksum_workspace: dvla_gemm_ksum_partial_rows(split_k) x (M or N) floats.
   * The ring kernels sum the fragments they feed to the matrix pipe (one v_dot2c_f32_bf16 per dword, in the MFMA
   * shadow); since ABI 7 the phase kernel sums too (both operands r-contiguous: the weight-gradient layout), in the slack of its
   * fragment-read segments, the sum of a tile row spread over up to four of its tiles -- dvla_gemm_ksum_partial_rows() accounts
   * for their partial rows.  A configuration without that code runs the column-sum kernel on the operand instead, which needs
   * the operand stored k-major (a_trans / b_trans = 1); otherwise DVLA_ERR_UNSUPPORTED. */
  void* ksum; int32_t ksum_dtype; int32_t ksum_operand; float* ksum_workspace;
  /* (ABI 5) a_layernorm != 0: the rows of A are layer-normalised on their way into the product -- A'(m, :) = (A(m, :) - mean_m) *
   * rsqrt(var_m + a_ln_eps), no affine parameters, rounded to bf16 like the output of dvla_layernorm_fwd_rows -- i.e. the GEMM computes
   * Linear(LayerNorm(x)) from x.  The DiT blocks' parameter-free LayerNorms in front of qkv / fc1 / the output layer
   * (models/action_model/models.py:129-141,158-160) at evaluation: 250 launches of a control step less.  Few-rows kernel only
   * (configuration 11: M <= 512, k-contiguous operands, 512 <= K <= 1536); DVLA_ERR_UNSUPPORTED otherwise. */
  int32_t a_layernorm; float a_ln_eps;
} dvla_gemm_params;
int64_t dvla_gemm_ksum_partial_rows(int32_t split_k);
int dvla_gemm_bf16(const dvla_gemm_params* p, void* stream);
/* tuning hook: 0 = automatic kernel choice by the built-in cost model (default; env DVLA_GEMM_VARIANT overrides at load);
 * 11 = the few-rows kernel (M <= 512, both operands k-contiguous, K % 16 == 0: one 32 x 32 tile of C per workgroup, K split over
 * its four or eight waves, fragments straight from global memory -- the evaluation-time shapes; what 0 picks for such problems);
 * 2 = register-staged 128x128 kernel; 4 / 6 / 7 = LDS-DMA ring kernels 256x256 / 128x128 / 256x128 (K-tile 64); 8 = phase
 * kernel (256x256, K-tile 64, two wave groups in ping-pong); 9 = the phase kernel under the stream-K hybrid schedule (whole
 * rounds one tile per CU; the last, partial rounds as equal K-iteration ranges per group of 16 CUs, the two halves of a
 * shared tile combined in-kernel through a 256-KiB fp32 slab); 11 = the few-rows kernel (M <= 512).  A configuration that does
 * not take a shape, and any number not named here, falls back to the register-staged kernel inside the library
 * (dvla_last_gemm_variant() then reports 2).  All differ only in fp32 summation order.  89 = the timeline build of the phase
 * kernel (s_memtime stamps into the workspace; only in a library built with DVLA_ABLATIONS=1, tests/probes/gemm_probe.cpp --stamps).
 * Stream-K scratch: 64 MiB + flags per (device, stream), hipMalloc'ed on the first launch that uses it (never while the
 * stream is being captured -- such launches take the plain schedule) and kept; DVLA_GEMM_STREAMK=0 turns the schedule off. */
enum {                                  /* the numbers above, by name (dvla_set_gemm_variant takes them, dvla_last_gemm_variant reports them) */
  DVLA_GEMM_CFG_AUTO = 0,
  DVLA_GEMM_CFG_REG = 2,                /* register-staged 128x128 */
  DVLA_GEMM_CFG_RING_256 = 4,           /* LDS-DMA ring 256x256 */
  DVLA_GEMM_CFG_RING_128 = 6,           /* LDS-DMA ring 128x128 */
  DVLA_GEMM_CFG_RING_256X128 = 7,       /* LDS-DMA ring 256x128, K-tile 64 */
  DVLA_GEMM_CFG_PHASE = 8,              /* phase kernel, plain schedule */
  DVLA_GEMM_CFG_PHASE_STREAMK = 9,      /* ... stream-K hybrid schedule */
  DVLA_GEMM_CFG_PHASE_STREAMK_FULL = 10,/* ... full stream-K schedule */
  DVLA_GEMM_CFG_FEW_ROWS = 11,
  DVLA_GEMM_CFG_PHASE_STAMPS = 89       /* timeline build of the phase kernel (DVLA_ABLATIONS=1 libraries only) */
};
void dvla_set_gemm_variant(int variant);
/* 10 = the phase kernel under the FULL stream-K schedule: every tile belongs to the K-iteration ranges, so the groups' tile
 * boundaries (epilogue write bursts) fall at different times for the whole launch instead of in lockstep rounds.
 * What the last dvla_gemm_bf16 call of this process launched: 2 / 4 / 6 / 7 / 8 as above, 9 / 10 only when the stream-K
 * schedule actually ENGAGED (otherwise 8: the plain schedule of the same kernel); 0 before the first call.  Tests use it to
 * assert that a forced configuration ran instead of falling back. */
int dvla_last_gemm_variant(void);
/* How the persistent kernels spread tiles over the CUs (process-wide; env DVLA_GEMM_OVERSUBSCRIBE / DVLA_GEMM_STREAMK at load).
 *   oversubscribe = 1 (default): one workgroup per CU slot walks a fixed share of the tiles; the stream-K schedule may apply.
 *     Fastest on a GPU that runs nothing else (the default bench: 165 ms / step against 176 with k = 8).
 *   oversubscribe = k > 1: up to k times as many, shorter-lived workgroups with equal tile counts, handed out by the hardware
 *     dispatcher as slots free up.  For callers whose GEMMs run for long stretches next to another stream's kernel that holds
 *     CUs: with a fixed share per CU a launch waits for the workgroups that could not start (measured +65 % per launch for
 *     16 of 256 CUs taken; k = 8: +0 ... +9 %; profiles/r02_gemm_cu_contention.txt).  The data-parallel path keeps k = 1: its
 *     bucket all-reduces (0.99 GB per step) occupy CUs for a few milliseconds of a 165-ms step.
 *   stream_k = 0 / 1: forbid / allow the stream-K schedule (needs every workgroup co-resident); -1 / oversubscribe < 1: keep. */
void dvla_set_gemm_schedule(int oversubscribe, int stream_k);
/* the schedule in force (either pointer may be NULL).  dreamvla_amd.ddp.GradBucketReducer switches to (8, 0) -- equal-sized,
 * short-lived workgroups, no co-residency assumption -- while its RCCL all-reduces are outstanding (their kernels hold CUs for
 * the whole transfer) and back afterwards. */
void dvla_get_gemm_schedule(int* oversubscribe, int* stream_k);

/* ---------------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (rows x cols, bf16 in/out, fp32 statistics).
 * gamma/beta may be NULL (DiT elementwise_affine=False, action_model/models.py:129-131,148).
 * Replaces nn.LayerNorm at models/vit_mae.py:77,202-204 (eps 1e-6), models/gpt2.py:312-315,437
 * (eps 1e-5), models/dreamvla_model.py:279,352,374,393,412,433, models/perceiver_resampler.py:14,28-29,101.
 * fwd writes mean/rstd (fp32, one per row) when they are non-NULL (needed by bwd).
 * bwd: dx (NULL, round 6: the input needs no gradient -- parameter gradients only); dgamma/dbeta (fp32, cols) when non-NULL, using
 *      `partial` = fp32 workspace of
 *      2 * dvla_layernorm_bwd_partial_rows() * cols floats.
 * Forward over all rows of a buffer: dvla_layernorm_fwd_rows with grp = gstride = goff = map_output = 0 (below).
 */
/* backward, plus the gradient of the residual stream that bypassed the LayerNorm (pre-LN blocks: h = x + f(LN(x)), so
 * dL/dx = dL/dh + LN'(...)): dx = dres + LN-backward(dy), one bf16 rounding -- replaces the separate autograd
 * accumulation add after every norm1 / norm2 / ln_1 / ln_2 backward (models/gpt2.py:312-339, timm Block).  dres must
 * not overlap dx; dres == NULL gives plain LayerNorm backward.  dgamma / dbeta are written in `grad_dtype` (0 = bf16:
 * the parameters' dtype, no cast kernel afterwards; 1 = fp32). */
int dvla_layernorm_bwd_add(const void* dy, const void* x, const void* gamma, int32_t param_dtype,
                           const float* mean, const float* rstd, const void* dres, void* dx, void* dgamma,
                           void* dbeta, int32_t grad_dtype, float* partial, int64_t rows, int64_t cols, void* stream);
int64_t dvla_layernorm_bwd_partial_rows(void);
/* (ABI 8) LayerNorm over the LAST `grp` rows of every `gstride`-row sequence of a (n_seq * gstride, cols) buffer, `goff` = gstride - grp
 * rows skipped in front of each group -- the dream-head decoders normalise only their mask-token rows before the prediction layer
 * (`x = self.image_decoder_norm(x[:, -n_mask:, :])`, models/dreamvla_model.py:812-816 and the depth / dino / sam / trajectory twins):
 * the slice is strided across sequences, and as an ATen copy (+ a zero-fill and a copy-back in backward) it was six launches and ~0.5 ms
 * per step.  rows = n_seq * grp logical rows; y, mean, rstd, dy are contiguous over them; x is read, and dx (the gradient of the WHOLE
 * buffer: zeros outside the groups, written by the kernel) is stored, in the buffer's rows.  General in goff: 0 <= goff, goff + grp <= gstride.
 * map_output != 0 is the mirror image: x (and dx) contiguous over the logical rows, the OUTPUT y (forward) and the incoming gradient dy
 * (backward) in the buffer's rows, nothing zero-filled -- two LayerNorms writing the two row ranges of one buffer replace
 * `torch.cat((norm_media(x), norm_latents(latents)), dim=-2)` of the PerceiverResampler (models/perceiver_resampler.py:44-49) and, in
 * backward, the copies of the cat's strided gradient slices. */
int dvla_layernorm_fwd_rows(const void* x, const void* gamma, const void* beta, int32_t param_dtype, void* y,
                            float* mean, float* rstd, int64_t rows, int64_t cols, float eps,
                            int32_t grp, int32_t gstride, int32_t goff, int32_t map_output, void* stream);
int dvla_layernorm_bwd_rows(const void* dy, const void* x, const void* gamma, int32_t param_dtype,
                            const float* mean, const float* rstd, void* dx, void* dgamma, void* dbeta,
                            int32_t grad_dtype, float* partial, int64_t rows, int64_t cols,
                            int32_t grp, int32_t gstride, int32_t goff, int32_t map_output, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Fused multi-head attention, head_dim = 64 (ViT 768/12, trunk 1024/16, dream-head decoders 1024/16, DiT 768/12,
 * perceiver dim_head 64, CLIP text 512/8).  Other head widths (models of another hidden_dim or head count, and the
 * 16-head dream-head decoders of any hidden_dim != 1024) take dvla_attn_hd_fwd / dvla_attn_hd_bwd below.
 *   O[b,i,h,:] = sum_j drop( softmax_j( scale * q[b,i,h,:].k[b,j,h,:] + mask[i,j] ) ) * v[b,j,h,:]
 * q/k/v/o element (b, token, head, d) lives at ptr[b*stride_b + token*stride_t + head*stride_h + d], so
 * the fused (B,N,3,h,d) timm qkv buffer, the GPT-2 c_attn (B,L,3H) buffer and the perceiver q / kv
 * buffers are read in place (no head-split copies).
 * Masks: the reference only ever builds 0 / -inf additive masks (generate_attention_mask,
 * models/dreamvla_model.py:25-66; CLIP's causal mask).  The host converts such a mask once into
 *   mask_bits_q (Lq x ceil(Lk/32) uint32): bit j of [i][kt] set <=> key 32*kt+j is visible to query i
 *   mask_bits_k (Lk x ceil(Lq/32) uint32): bit i of [j][qt] set <=> query 32*qt+i sees key j   (backward)
 *   tile_map    (ceil(Lq/32) x ceil(Lk/32) uint8): 0 = all -inf (tile skipped), 1 = all visible, 2 = mixed
 * so masked tiles cost nothing (64-81 % of the trunk's score matrix) and a mixed tile
 * costs one 32-bit load per lane.  key_index (Lk int32, optional) names the k/v (and dk/dv) token row that
 * holds key j (any order, every entry < 2^18): keys that no query can see are dropped from the key axis without
 * copying K/V, and the caller is free to ORDER the kept keys so that keys with the same audience share 32-key tiles
 * (dreamvla_amd.ops.build_mask_tables does); dk/dv rows that are not indexed are NOT written (the caller zero-fills them).
 * Without key_index EVERY dk/dv row is written, the rows of keys that no query sees with zeros.
 * ANY 0 / -inf pattern is a valid mask, Lq != Lk included (mask_bits_q has ceil(Lk/32) words per query, mask_bits_k ceil(Lq/32)
 * per key).  A query that sees NO key gets o = 0 and lse = +inf; in the backward pass its dq is 0 and it contributes nothing to
 * dk or dv, whatever its dout holds (tests/test_attention_masks_gpu.py holds the kernels to all of this).
 * lse (B*H*Lq fp32, natural-log-sum-exp of the scaled+masked scores) is written when non-NULL.
 * Replaces: F.scaled_dot_product_attention in timm Attention (vit_mae.py:202-203, dreamvla_model.py:806-904,
 * action_model/models.py:137), GPT2Attention._attn / GPT2SdpaAttention (models/gpt2.py:61-84,267-274),
 * PerceiverAttention einsum-softmax-einsum (models/perceiver_resampler.py:55-60).
 */
typedef struct dvla_attn_params {
  const void* q; const void* k; const void* v; void* o;
  int64_t q_stride_b, q_stride_t, q_stride_h;
  int64_t k_stride_b, k_stride_t, k_stride_h;
  int64_t v_stride_b, v_stride_t, v_stride_h;
  int64_t o_stride_b, o_stride_t, o_stride_h;
  int32_t B, H, Lq, Lk;
  float scale;
  const int32_t* key_index;
  const uint32_t* mask_bits_q;
  const uint32_t* mask_bits_k;
  const uint8_t* tile_map;
  float dropout_p; uint32_t seed_lo; uint32_t seed_hi;
  float* lse;
  /* backward only */
  const void* dout; int64_t do_stride_b, do_stride_t, do_stride_h;
  float* delta; /* workspace B*H*Lq fp32: rowsum(dO * O) */
  void* dq; void* dk; void* dv;
  int64_t dq_stride_b, dq_stride_t, dq_stride_h;
  int64_t dk_stride_b, dk_stride_t, dk_stride_h;
  int64_t dv_stride_b, dv_stride_t, dv_stride_h;
} dvla_attn_params;
int dvla_attn_fwd(const dvla_attn_params* p, void* stream);
int dvla_attn_bwd(const dvla_attn_params* p, void* stream);
/* The same attention for SHORT sequences (Lq == Lk <= 64) with ANY head_dim <= 128 (multiple of 8), no mask, no dropout: one
 * wave per (batch, head).  Further limits (DVLA_ERR_UNSUPPORTED from both entry points): B <= 65535, and the backward kernel's
 * LDS, (4 L (head_dim + 1) + 2 L (L + 1)) * 4 bytes, must fit 160 KiB -- L = 64 with head_dim 128 does not (L <= 63 does).  The only head_dim != 64 the reference can produce is the DiT-S action head (models/action_model/
 * action_model.py:12-14: 384 / 4 = 96) on 6-token sequences.  Same parameter block; `delta` is not used. */
int dvla_attn_small_fwd(const dvla_attn_params* p, int32_t head_dim, void* stream);
int dvla_attn_small_bwd(const dvla_attn_params* p, int32_t head_dim, void* stream);
/* (additive, ABI 8) The same attention as dvla_attn_fwd / dvla_attn_bwd -- same parameter block, masks, key_index, dropout keep
 * mask, lse and delta -- for head_dim a multiple of 8 with 8 <= head_dim <= 128 and head_dim != 64 (DVLA_ERR_UNSUPPORTED
 * otherwise).  The kernels run at head_dim rounded up to a multiple of 32 with the extra d columns zero; columns >= head_dim of
 * o / dq / dk / dv are not written.  q / k / v / dout (and o in backward) need 16-byte aligned rows, o / dq / dk / dv 8-byte. */
int dvla_attn_hd_fwd(const dvla_attn_params* p, int32_t head_dim, void* stream);
int dvla_attn_hd_bwd(const dvla_attn_params* p, int32_t head_dim, void* stream);
/* (additive, still ABI 9) Attention probe: the softmax probabilities of R selected query rows of every sequence over all keys --
 * what the kernels above apply and never store.  An evaluation instrument with no counterpart in the reference.
 * Of the parameter block it reads q, k and their strides, B, H, Lq, Lk, scale, key_index and mask_bits_q (NULL = no mask;
 * key_index NULL = keys in place, Lk == Lk_full); v, o, dropout and everything after are ignored.  head_dim: a multiple of 8 from
 * 8 to 128, 64 included.  rows: (B, R) int32 on the device, 1 <= R <= DVLA_PROBE_MAX_ROWS (DVLA_ERR_UNSUPPORTED otherwise, before
 * any launch); an entry < 0 or >= Lq gives a zero row.
 * out (fp32): per_head != 0: (B, H, R, Lk_full);  per_head == 0: (B, R, Lk_full), the mean over heads = (sum over h ascending) / H,
 * and workspace must hold B * H * R * Lk_full floats.  Columns are ORIGINAL key numbers (key_index is undone on the store).  Every
 * element of out is written: a key the row cannot see, and a row that sees no key, get exactly 0.0f.
 * p = exp(s - max s) / sum exp(s - max s) over the visible keys, s = scale * <q, k> accumulated in fp32.  No atomics, no host
 * synchronisation; a sequence's result does not depend on B or on its place in the batch and is the same bits on every run. */
#define DVLA_PROBE_MAX_ROWS 32
int dvla_attn_probe(const dvla_attn_params* p, const int32_t* rows, int32_t R, int32_t head_dim, int32_t Lk_full, int32_t per_head,
                    float* out, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Small HBM-bound helpers (bf16 unless noted).
 */
/* out[n] = sum_m x[m,n]  (bias gradients), written in out_dtype (0 = bf16: the bias gradient in the parameter's dtype, no cast
 * kernel; 1 = fp32); `partial` = fp32 workspace of dvla_colsum_partial_rows() * cols floats. */
int dvla_colsum_dt(const void* x, int64_t ld, int64_t rows, int64_t cols, void* out, int32_t out_dtype, float* partial,
                   void* stream);
int64_t dvla_colsum_partial_rows(void);
/* y = dropout(x) * 1/(1-p) with the stateless hash RNG; rows x cols, row stride = cols.
 * GPT2Model.drop (models/gpt2.py:459) and its backward (same call on the gradient). */
int dvla_dropout(const void* x, void* y, int64_t rows, int64_t cols, float p, uint32_t seed_lo, uint32_t seed_hi,
                 void* stream);
/* dz = dy * act'(preact) (optionally after dropout mask of dy): backward of a fused activation. */
int dvla_act_bwd(const void* dy, const void* preact, void* dz, int64_t rows, int64_t cols, int32_t act,
                 float dropout_p, uint32_t seed_lo, uint32_t seed_hi, void* stream);
/* The same dz, plus colsum[c] = sum_r dz[r, c] (fp32 sums of the stored bf16 values, written as colsum_dtype) from the same pass:
 * the bias gradient of `y = dropout(act(x W + b))` (models/gpt2.py:160,172-173,329-339: c_proj and the MLP's second Conv1D),
 * which otherwise costs either a column-sum pass over dz or the summing code inside the weight-gradient GEMM.  partial:
 * dvla_colsum_partial_rows() x cols floats.  cols % 8 == 0 and 16-byte aligned operands, else DVLA_ERR_UNSUPPORTED. */
int dvla_act_bwd_colsum(const void* dy, const void* preact, void* dz, int64_t rows, int64_t cols, int32_t act, float dropout_p,
                        uint32_t seed_lo, uint32_t seed_hi, void* colsum, int32_t colsum_dtype, float* partial, void* stream);
/* y = act(x) */
int dvla_act_fwd(const void* x, void* y, int64_t n, int32_t act, void* stream);
/* One step of the action sampler's algebra, evaluation path (models/dreamvla_model.py:935-987): classifier-free guidance
 * (action_model/models.py:253-268: eps = uncond + s (cond - uncond), evaluated in the model dtype like the tensor expression
 * it replaces: three bf16 roundings) followed by the eta = 0 DDIM update (gaussian_diffusion.py:522-569):
 *     pred_x0 = a x - b eps;   eps' = (a x - pred_x0) / b;   x_next = pred_x0 sqrt_acp_prev + sqrt_1m_acp_prev eps'
 * in fp32, operation by operation (no contraction) -- ~20 elementwise ATen launches on (bs, 3, 7) tensors become one.
 * model_out: bf16, sample i of the guided half at model_out + i * sample_stride, of the unguided half at
 * model_out + (bs + i) * sample_stride, per_sample contiguous values each; x, x_next: fp32 (bs, per_sample) contiguous. */
int dvla_ddim_cfg_step(const void* model_out, int64_t sample_stride, const float* x, float* x_next, int64_t bs, int64_t per_sample,
                       float cfg_scale, float a, float b, float sqrt_acp_prev, float sqrt_1m_acp_prev, void* stream);
/* One step of the flow-matching head's evaluation sampler (models/action_model/respace.py:118-191 FMDiffusion over
 * forward_with_cfg): the same guidance as dvla_ddim_cfg_step (three bf16 roundings) followed by the Euler update
 *     x_next = x + delta u
 * in fp32, one multiply and one add (no contraction).  Arguments and layouts as dvla_ddim_cfg_step. */
int dvla_fm_cfg_step(const void* model_out, int64_t sample_stride, const float* x, float* x_next, int64_t bs, int64_t per_sample,
                     float cfg_scale, float delta, void* stream);
/* The WHOLE evaluation sampler of the DiT action head in one launch (models/dreamvla_model.py:935-987: ddim_sample_loop over
 * net.forward_with_cfg, eta = 0; models/action_model/models.py:162-268 DiT.forward / forward_with_cfg; gaussian_diffusion.py:
 * 522-569 ddim_sample): `steps` x { token embedding, `depth` DiT blocks, final layer, guidance + DDIM update } on 2 bs sequences
 * of 2 tokens tokens (the guided and the unguided half of every sample), as a persistent kernel on the 32 CUs of one XCD whose
 * workgroups exchange activations through that XCD's L2 (csrc/dit_team.hip; tests/probes/sync_probe.cpp has the measurements
 * behind the design).  Same arithmetic and rounding points as the launch-by-launch path (ActionModel.sample_ddim_cfg: few-rows
 * GEMMs with LayerNorm on the fly, flash attention, dvla_ddim_cfg_step), other fp32 summation order inside the products.
 *   blocks     device array of `depth` entries: bf16 weights in nn.Linear layout (out, in), bf16 biases
 *   xemb_*     x_embedder Linear(channels -> hidden); final_*: final_layer.linear (hidden -> channels); pos (2 tokens, hidden)
 *   cond       (steps, 2 bs, tokens, hidden) bf16: z_embedder([cond ; uncondition]) + t_embedder(timestep of step j), j = 0 the
 *              FIRST sampler step (the largest timestep)
 *   coef       (steps, 4) fp32 on the device: a, b, sqrt_acp_prev, sqrt_1m_acp_prev of dvla_ddim_cfg_step per sampler step
 *   noise/out  (bs, tokens, channels) fp32: start noise / samples (NaN if a wait inside the kernel timed out)
 *   workspace  dvla_dit_sample_workspace_bytes(hidden) bytes, 16-byte aligned, ZERO-INITIALISED by the caller once (the kernel
 *              leaves its counters at zero); 32-bit word 33 = number of launches so far in which a wait timed out (their outputs
 *              are NaN; the launch retires its own status word 32, so a timeout does not carry over to the next launch), word 34 =
 *              the last non-zero status, words 64 .. 95 = the XCC id each of the 32 team members ran on in the last launch (all
 *              equal = the fast case), valid after a launch
 * DVLA_ERR_UNSUPPORTED unless hidden = 768 (DiT-B), head_dim 64, 2 tokens <= 8, 4 bs tokens <= 16 rows (one episode),
 * channels <= 16, on a device with 256 CUs: the caller then runs the launch-by-launch sampler (which is the faster one for two
 * row blocks and for hidden 1024: profiles/r04_dit_team_perf.jsonl). */
typedef struct dvla_dit_block_weights {
  const void *qkv_w, *qkv_b, *proj_w, *proj_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} dvla_dit_block_weights;
typedef struct dvla_dit_sample_params {
  const dvla_dit_block_weights* blocks;
  const void *xemb_w, *xemb_b, *final_w, *final_b, *pos, *cond;
  const float* coef;
  const float* noise;
  float* out;
  void* workspace;
  int64_t workspace_bytes;
  float cfg_scale, ln_eps;
  int32_t depth, hidden, heads, channels, tokens, bs, steps, reserved;
} dvla_dit_sample_params;
int64_t dvla_dit_sample_workspace_bytes(int32_t hidden);
int dvla_dit_sample(const dvla_dit_sample_params* p, void* stream);
/* The flow-matching head's evaluation sampler (FMDiffusion over forward_with_cfg: models/action_model/respace.py:118-191) as the
 * same persistent kernel: the same exchange schedule, shape gate, workspace, timeout contract (word 33 / 34, NaN output, the
 * launch retires its own status) and test hooks as dvla_dit_sample, with the Euler update of dvla_fm_cfg_step in place of the
 * DDIM update.  The fields of p mean what they mean there, except
 *   cond       (steps, 2 bs, tokens, hidden) bf16: z_embedder([cond ; uncondition]) + t_embedder(j / steps), j = 0 the first step
 *   coef       (steps) fp32 on the device: the Euler step size delta of each sampler step (1 / steps upstream) */
int dvla_dit_sample_fm(const dvla_dit_sample_params* p, void* stream);
/* measurement: a device buffer of 2 x 8 x (steps x (1 + 5 depth) + 1) uint64 that later launches fill with wall-clock stamps
 * (100 MHz) of team members 0 and 17 -- per exchange: weights requested, producers arrived, operands landed, partial tiles in
 * LDS, results stored; NULL (the default) switches it off */
void dvla_dit_sample_set_stamps(void* device_buffer);
/* test hook: the next n dvla_dit_sample launches behave as if a wait inside the kernel had timed out (NaN output, workspace word 33
 * incremented); a launch captured into a hipGraph while the hook is armed times out on every replay */
void dvla_dit_sample_inject_timeouts(int32_t n);
/* dst(bf16) = src(fp32) / dst(fp32) = src(bf16) */
int dvla_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int dvla_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* out = a + b (bf16, n elements); b_period > 0 broadcasts b with period b_period elements */
int dvla_add(const void* a, const void* b, void* out, int64_t n, int64_t b_period, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Optimizer step over flat bf16 buffers (the caller's `clip_grad_norm_` + `torch.optim.AdamW.step`, reference
 * train.py:253-262 / utils/train_utils.py:600-608).
 * dvla_sumsq_bf16: out[0] (+)= sum x[i]^2 in fp32; `partial` holds dvla_sumsq_partial_len() floats.
 * dvla_adamw_bf16: one AdamW step on n elements; math in fp32, parameters and both moments stored in bf16 (torch's
 *   fused AdamW with bf16 parameters).  If grad_sumsq != NULL the gradient is first scaled by
 *   min(1, max_norm / (sqrt(*grad_sumsq) + 1e-6)) and rounded to bf16 (clip_grad_norm_ semantics; the scalar stays on
 *   the device, no host synchronisation).  `step` is the 1-based step count (bias corrections). */
int64_t dvla_sumsq_partial_len(void);
int dvla_sumsq_bf16(const void* x, int64_t n, float* partial, float* out, int32_t accumulate, void* stream);
int dvla_adamw_bf16(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int64_t step, const float* grad_sumsq, float max_norm,
                    void* stream);
/* fp32 masters (`--precision fp32`: parameters, gradients and both moments fp32).
 * dvla_sumsq_f32: the fp32 twin of dvla_sumsq_bf16 (same reduction, same `partial` / `out` contract): calls on bf16 and
 *   fp32 buffers can accumulate into one device scalar.
 * dvla_adamw_f32_master: one clip + AdamW step on n fp32 elements, restating torch's foreach AdamW for fp32 parameters
 *   operation for operation (decoupled weight decay; each torch op rounded to fp32): the clip coefficient
 *   min(1, max_norm / (sqrt(*grad_sumsq) + 1e-6)) scales the gradient in fp32 (grad_sumsq NULL: no clipping).  The
 *   hyper-parameters are doubles (the Python floats torch derives its scalars from).  If shadow_bf16 != NULL it receives
 *   the round-to-nearest-even bf16 copy of the new parameter (bit-identical to dvla_cast_f32_to_bf16 of it).  Every
 *   pointer is 16-byte aligned; `step` is the 1-based step count. */
int dvla_sumsq_f32(const float* x, int64_t n, float* partial, float* out, int32_t accumulate, void* stream);
int dvla_adamw_f32_master(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t n,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                          const float* grad_sumsq, float max_norm, void* stream);
/* (additive, ABI 9) The guarded step: the same two AdamW kernels under a verdict taken on the device, so that a step whose
 * gradient is not finite changes nothing and is counted, with no host synchronisation.  The bias corrections
 * depend on the number of steps APPLIED so far, which the host -- running ahead of the device -- does not know; it keeps
 * deriving them in doubles (dvla_step_candidates, the expressions of dvla_adamw_bf16 / dvla_adamw_f32_master) for every count
 * that is still possible and hands the table to dvla_step_verdict by value; the device picks the row.
 * dvla_step_scalars: what depends on the step count -- inv_bc1 = 1 / (1 - beta1^t) and inv_bc2_sqrt = 1 / sqrt(1 - beta2^t)
 *   (dvla_adamw_bf16's kernel), bc2_sqrt = sqrt(1 - beta2^t) and step_size = -lr / (1 - beta1^t) (dvla_adamw_f32_master's).
 * dvla_step_state: device memory, 16-byte aligned, zeroed once by the caller (or set to a resumed run's counts).  The first
 *   32 bytes are what a caller reads back per step: the counters, the verdict and the norm.
 *     applied / skipped: steps applied / skipped so far.  faults: steps whose applied count lay outside the caller's table (the
 *     caller lost track; such a step is skipped too, and the caller must treat faults != 0 as an error).
 *     ok: the current step's verdict.  sumsq: its total sum of squares (what *grad_sumsq receives).
 *     cand: the row chosen, and the row itself (inv_bc1 ... step_size).
 *     skipped_bucket_sumsq[0 .. n_latched): the per-bucket sums of the LAST skipped step (which bucket went non-finite), and
 *     latched_step: that step's 1-based number (applied + skipped after it).
 *   At most DVLA_STEP_MAX_BUCKETS buckets (more: DVLA_ERR_UNSUPPORTED), at most DVLA_STEP_MAX_CANDIDATES rows.
 * dvla_step_candidates: no launch.  out[j], j < n_cand, = the scalars of step count base + j (base >= 1) from the double
 *   hyper-parameters; the bf16 pair from the betas rounded to float, as dvla_adamw_bf16 receives them.
 * dvla_step_verdict: one launch of one wave.  bucket_sumsq[i], i < n, is bucket i's sum of squares (dvla_sumsq_bf16 /
 *   dvla_sumsq_f32 with accumulate = 0 into slot i).  The slots are added in index order -- the order of the `accumulate` chain,
 *   so the total has the same bits -- and written to *grad_sumsq and state->sumsq; ok = the total is finite (one non-finite
 *   element, or a norm that overflows fp32, makes it not).  j = state->applied - confirmed_applied selects cand[j] (a HOST
 *   table, copied into the kernel arguments); j outside [0, n_cand) forces ok = 0 and counts a fault.  Then applied += ok,
 *   skipped += !ok, and a skipped step latches its slots.
 * dvla_adamw_bf16_guarded / dvla_adamw_f32_master_guarded: their twins without `step` and `grad_sumsq` -- both come from the
 *   state (one uniform load per workgroup).  state->ok == 0: the kernel returns before it reads or writes param, exp_avg,
 *   exp_avg_sq or the shadow.  Otherwise each element goes through the twin's own element function: bit-identical results
 *   for the same scalars.  max_norm <= 0: no clipping.
 * DVLA_ERR_ARG: a null pointer, a negative size or count, base < 1, n_cand outside 1 .. DVLA_STEP_MAX_CANDIDATES.
 * DVLA_ERR_UNSUPPORTED: a base that is not 16-byte aligned, n > DVLA_STEP_MAX_BUCKETS.  n == 0: DVLA_OK, nothing launched. */
#define DVLA_STEP_MAX_BUCKETS 256
#define DVLA_STEP_MAX_CANDIDATES 9
typedef struct dvla_step_scalars { float inv_bc1, inv_bc2_sqrt, bc2_sqrt, step_size; } dvla_step_scalars;
typedef struct dvla_step_state {
  int64_t applied, skipped, faults;
  int32_t ok;
  float sumsq;
  int32_t cand, n_latched;
  float inv_bc1, inv_bc2_sqrt, bc2_sqrt, step_size;
  int64_t latched_step;
  float skipped_bucket_sumsq[DVLA_STEP_MAX_BUCKETS];
} __attribute__((aligned(16))) dvla_step_state;
int dvla_step_candidates(double lr, double beta1, double beta2, int64_t base, int32_t n_cand, dvla_step_scalars* out);
int dvla_step_verdict(const float* bucket_sumsq, int32_t n, float* grad_sumsq, dvla_step_state* state,
                      int64_t confirmed_applied, int32_t n_cand, const dvla_step_scalars* cand, void* stream);
int dvla_adamw_bf16_guarded(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, float max_norm, const dvla_step_state* state,
                            void* stream);
int dvla_adamw_f32_master_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                  int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                  float max_norm, const dvla_step_state* state, void* stream);
/* (additive, ABI 9) EMA of the weights inside the step.  The EMA buffer is fp32 whatever the parameter dtype
 * (a bf16 EMA with 1 - decay below a bf16 ulp would never move), at the parameter's offsets.  After an element's AdamW update
 * has produced the STORED parameter p (the fp32 master; the bf16 value that is written, widened), e <- lerp(e, p, w) as ATen
 * computes it: diff = p - e (rounded), then fma(w, diff, e) if |w| < 0.5 else fma(-diff, 1 - w, p).  Parameters, moments and
 * shadows come out bit-identical to the step without `ema`: the AdamW part is the twin's element function on the same scalars.
 * dvla_ema_weights: no launch; the one place the weight is derived.  out[j], j < n, = (float)(1 - d(base + j)) formed in
 *   double, where t = base + j is the 1-based count of applied steps and d(t) = decay, or with warmup != 0
 *   d(t) = min(decay, (1 + t) / (10 + t)) (the timm / diffusers warm-up).  0 < decay < 1, base >= 1,
 *   0 <= n <= DVLA_STEP_MAX_CANDIDATES, out not NULL: DVLA_ERR_ARG otherwise.
 * dvla_adamw_bf16_ema / dvla_adamw_f32_master_ema: dvla_adamw_bf16 / dvla_adamw_f32_master + `ema` (n floats, 16-byte
 *   aligned, not NULL) and its weight `ema_w` (dvla_ema_weights of `step`).
 * dvla_adamw_bf16_ema_guarded / dvla_adamw_f32_master_ema_guarded: the guarded twins + `ema` and `ema_w`, a HOST table of
 *   n_cand weights (dvla_ema_weights(decay, warmup, base, n_cand) for the `base` and n_cand given to dvla_step_candidates /
 *   dvla_step_verdict), copied into the kernel arguments; row state->cand is used.  state->ok == 0: nothing is read or
 *   written, the EMA included, so a skipped step neither moves the EMA nor advances its warm-up.
 * dvla_ema_swap_f32: param[i] <-> ema[i] for i < n, and, if shadow_bf16 != NULL, shadow[i] = the RNE bf16 of the new param[i]
 *   (dvla_cast_f32_to_bf16's bits).  Twice in a row restores everything.
 * dvla_ema_swap_bf16: restore == 0: stash[i] = param[i], then param[i] = the RNE bf16 of ema[i]; restore != 0:
 *   param[i] = stash[i].  The EMA is only read.
 * Every pointer 16-byte aligned (DVLA_ERR_UNSUPPORTED otherwise); n == 0: DVLA_OK, nothing launched. */
int dvla_ema_weights(double decay, int32_t warmup, int64_t base, int32_t n, float* out);
int dvla_adamw_bf16_ema(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* grad_sumsq,
                        float max_norm, float ema_w, void* stream);
int dvla_adamw_f32_master_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, float* ema,
                              int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                              const float* grad_sumsq, float max_norm, float ema_w, void* stream);
int dvla_adamw_bf16_ema_guarded(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n, float lr,
                                float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream);
int dvla_adamw_f32_master_ema_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                      float* ema, int64_t n, double lr, double beta1, double beta2, double eps,
                                      double weight_decay, float max_norm, const dvla_step_state* state, const float* ema_w,
                                      int32_t n_cand, void* stream);
int dvla_ema_swap_f32(float* param, float* ema, void* shadow_bf16, int64_t n, void* stream);
int dvla_ema_swap_bf16(void* param, const float* ema, void* stash, int64_t n, int32_t restore, void* stream);
/* (additive, ABI 9) Parameter groups: per-group lr and weight decay in ONE launch per bucket whatever the number
 * of groups; betas, eps and the clip coefficient stay common.  A parameter of group g comes out bit-identical to that
 * parameter under the one-group entry points called with (lr[g], weight_decay[g]).
 * group_map: device memory, one byte per vector of 8 elements, (n + 7) / 8 bytes: a group id 0 .. n_groups - 1, or 255 = leave
 *   this vector alone (nothing of it is read or written: parameter, moments, shadow and EMA keep their bits).  The n % 8 ragged
 *   tail belongs to the last byte.  Ids in n_groups .. 254 are the caller's error (check them where the map is built); the
 *   kernels treat them as 255.
 * lr, weight_decay: HOST arrays of n_groups doubles.  The kernels receive floats derived from them by value (no upload):
 * dvla_group_scalars: no launch; the one place they are derived, with the expressions of the one-group entry points.
 *   out[g].decay = (float)(1 - lr weight_decay) and out[g].step_size[j] = (float)((lr / (1 - beta1^(base + j))) * -1.0), j < n_cand
 *   (dvla_adamw_f32_master's; step_size[j] is what dvla_step_candidates(lr[g], ...) gives; rows j >= n_cand repeat the last);
 *   out[g].lr, out[g].weight_decay = the doubles rounded to float (dvla_adamw_bf16's arguments).
 * dvla_adamw_bf16_grouped / dvla_adamw_f32_master_grouped: the streams of dvla_adamw_bf16 / dvla_adamw_f32_master, + `ema`
 *   (n floats, or NULL: no EMA) and `state` (or NULL: no guard).
 *   state == NULL: `step` is the 1-based step count, grad_sumsq as in the twin, ema_w[0] the EMA weight; n_cand is ignored.
 *   state != NULL: the guarded step.  `step` is the `base` and n_cand the count given to dvla_step_candidates / dvla_step_verdict,
 *     ema_w the host table of n_cand weights; the gradient is clipped on state->sumsq iff max_norm > 0 (grad_sumsq is ignored);
 *     state->ok == 0: nothing is read or written.
 * DVLA_ERR_ARG: a null pointer (ema_w with ema != NULL included), n < 0, step < 1, n_groups outside 1 .. DVLA_STEP_MAX_GROUPS,
 *   n_cand outside 1 .. DVLA_STEP_MAX_CANDIDATES.  DVLA_ERR_UNSUPPORTED: a base that is not 16-byte aligned (the map may sit at
 *   any address).  n == 0: DVLA_OK, nothing launched. */
#define DVLA_STEP_MAX_GROUPS 64
typedef struct dvla_group_row { float decay, lr, weight_decay; float step_size[DVLA_STEP_MAX_CANDIDATES]; } dvla_group_row;
int dvla_group_scalars(const double* lr, const double* weight_decay, int32_t n_groups, double beta1, double beta2, int64_t base,
                       int32_t n_cand, dvla_group_row* out);
int dvla_adamw_bf16_grouped(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                            const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay, float beta1,
                            float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm,
                            const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream);
int dvla_adamw_f32_master_grouped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, float* ema,
                                  int64_t n, const uint8_t* group_map, int32_t n_groups, const double* lr,
                                  const double* weight_decay, double beta1, double beta2, double eps, int64_t step,
                                  const float* grad_sumsq, float max_norm, const dvla_step_state* state, const float* ema_w,
                                  int32_t n_cand, void* stream);
/* (additive, ABI 9) Stochastic rounding of the bf16 stores: a stored value equals its fp32 value in expectation,
 * so updates below half a bf16 spacing land with the right frequency instead of never.
 * The rounding, on the 32 bits u of the fp32 value and 16 random bits r (all integer arithmetic):
 *     exponent all ones, mantissa zero (+-inf):  u >> 16
 *     exponent all ones, mantissa not zero (NaN): (u >> 16) | 0x0040
 *     anything else:                              (u + r) >> 16
 *   A value that is a bf16 already (low 16 bits zero) comes back unchanged for every r; otherwise the magnitude goes up with
 *   probability low16 / 65536 (negative values and denormals alike, -0 stays -0); a finite value above the largest bf16 may
 *   become inf, as it does under round-to-nearest.
 * The random bits are counter-based and stateless: a pure function of (seed: 64 bits, step: 64 bits, bucket: 32 bits,
 * stream: 0 = param, 1 = exp_avg, 2 = exp_avg_sq, element index i: 64 bits), whatever the grid, the split of a bucket into ranges
 * or the rank.  With hash32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32 arithmetic):
 *     k = hash32(lo32(seed) ^ 0x243F6A88); k = hash32(k ^ hi32(seed)); k = hash32(k ^ lo32(step)); k = hash32(k ^ hi32(step));
 *     k = hash32(k ^ bucket)                                                          -- the launch key
 *     h = hash32((k ^ (hi32(i) * 0x85EBCA6B)) + lo32(i) * 0x9E3779B9)                 -- per element
 *     r[0] = h >> 16,  r[1] = h & 0xffff,  r[2] = hash32(h ^ 0x5BD1E995) >> 16        -- per stream
 *   (tests/sr_ref.py restates generator and rounding in integer arithmetic).
 * dvla_sr_cast_f32_to_bf16: out[j] = the rounding of x[j] with r[stream] of element index index_base + j, j < n.  x and out need
 *   no more than their elements' own alignment.  DVLA_ERR_ARG: a null pointer, n < 0, stream outside 0 .. 2.  n == 0: DVLA_OK, nothing launched.
 * dvla_adamw_bf16_sr: dvla_adamw_bf16_grouped (its arguments, its fp32 arithmetic element for element, its guard and EMA) with
 *   the three final conversions of param, exp_avg and exp_avg_sq rounded as above instead of to nearest; the rounding of the
 *   clipped gradient stays round-to-nearest, and the EMA follows the parameter as stored.  group_map may be NULL: then n_groups
 *   must be 1 and every element is stepped with (lr[0], weight_decay[0]) -- the one-group step, plain, guarded, with or without
 *   the EMA.  Element j of the launch has index sr_index_base + j (a launch over a range of a bucket passes the range's offset:
 *   a bucket stepped in several ranges draws the bits of one stepped whole).  The key's step is the count of APPLIED steps this
 *   step becomes: `step` with state == NULL, state->applied (as dvla_step_verdict left it) otherwise, so a skipped step draws
 *   nothing and does not advance the key.  Errors as dvla_adamw_bf16_grouped, + DVLA_ERR_ARG for group_map == NULL with
 *   n_groups != 1 and for sr_index_base < 0. */
int dvla_sr_cast_f32_to_bf16(const float* x, void* out, int64_t n, uint64_t seed, uint64_t step, int32_t bucket, int32_t stream,
                             int64_t index_base, void* hip_stream);
int dvla_adamw_bf16_sr(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                       const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay, float beta1,
                       float beta2, float eps, int64_t step, const float* grad_sumsq, float max_norm,
                       const dvla_step_state* state, const float* ema_w, int32_t n_cand, uint64_t sr_seed, int32_t sr_bucket,
                       int64_t sr_index_base, void* stream);
/* (additive, ABI 9) Per-parameter reductions over the flat optimizer buffers: every parameter of a bucket is a
 * segment of the gradient, parameter and moment buffers at the same element offsets.  Stage 1 (one launch per bucket and buffer)
 * reduces chunks of segments into records, stage 2 (dvla_segment_combine: one launch for all buckets) adds every segment's
 * records: no atomics, no host synchronisation, nothing the step kernels do changes.
 * The chunk table (host-built; dreamvla_amd/optim.py: build_chunk_table): every segment is cut into chunks of DVLA_STATS_CHUNK
 *   elements counted from the segment's OWN first element, the last one shorter; segments start on multiples of 8 elements.
 *     chunks[2 c], chunks[2 c + 1]   element offset in the buffer and length (<= DVLA_STATS_CHUNK) of chunk c of a bucket; the
 *                                    chunks of a segment are consecutive rows, in order
 *     segs[3 j .. 3 j + 2]           first record, number of records (0 for an empty segment) and output index of segment j
 *   Both live in device memory.  partial: device scratch of DVLA_STATS_PARTIAL_BYTES per chunk; stage 1 writes record c of its
 *   bucket at partial + c * DVLA_STATS_PARTIAL_BYTES, so the buckets of one optimizer pass consecutive regions of one scratch
 *   and segs counts records from its start.  A row that does not lie inside the buffer (n elements), the records (n_chunks)
 *   or the outputs (n_out) is not followed: nothing is read or written for it (a chunk row: a record of zeros).
 *   A segment's results depend on its own elements and on nothing else -- not on the grid, the other segments, the bucket or the
 *   segment's offset -- and two calls give the same bits.  Elements outside every chunk (alignment gaps) are never read.
 * dvla_segment_stats_bf16 / _f32: per chunk the sum of x^2, the largest |x| over the elements that are not NaN and the number of
 *   NaN / +-inf elements.  dvla_segment_adam_bf16 / _f32: per chunk the sum of r^2, r = exp_avg / denom(exp_avg_sq) with the step
 *   kernels' own expressions,
 *     fp32 masters:  denom = rn(rn(rn(sqrt(v)) / bc2_sqrt) + eps), r = rn(m / denom)          (dvla_adamw_f32_master)
 *     bf16:          denom = fma(sqrt(v), inv_bc2_sqrt, eps),       r = m / denom, on the stored moments widened to fp32
 *   and bc2_sqrt / inv_bc2_sqrt those of dvla_step_candidates for `step` (the count of the step that wrote the moments).  No lr
 *   enters: lr / (1 - beta1^step) * sqrt(sum r^2) is the norm of the Adam term that step added to the parameter.
 * dvla_segment_combine: for segment j, at output index o = segs[3 j + 2], its records added in order (the sum in double),
 *     sumsq[o]      the sum, fp32 (error bound: DESIGN.md 4.3); NaN / inf if the segment holds one
 *     absmax[o]     max |x| over the elements that are not NaN (fmaxf; an inf gives inf); 0 for an empty or all-NaN segment
 *     nonfinite[o]  the number of NaN and +-inf elements, exact
 *   absmax and nonfinite may be NULL (the Adam term has neither).
 * DVLA_ERR_ARG: a null pointer, a negative count, step < 1.  n_chunks == 0 (stage 1) or n_segs == 0 (stage 2): DVLA_OK, nothing
 * launched.  DVLA_ERR_UNSUPPORTED: a buffer, chunk table or scratch base that is not 16-byte aligned.  All of these return
 * before anything touches the device. */
#define DVLA_STATS_CHUNK 8192
#define DVLA_STATS_PARTIAL_BYTES 16
int dvla_segment_stats_bf16(const void* x, int64_t n, const int64_t* chunks, int64_t n_chunks, void* partial, void* stream);
int dvla_segment_stats_f32(const float* x, int64_t n, const int64_t* chunks, int64_t n_chunks, void* partial, void* stream);
int dvla_segment_adam_bf16(const void* exp_avg, const void* exp_avg_sq, int64_t n, const int64_t* chunks, int64_t n_chunks,
                           void* partial, float beta2, float eps, int64_t step, void* stream);
int dvla_segment_adam_f32(const float* exp_avg, const float* exp_avg_sq, int64_t n, const int64_t* chunks, int64_t n_chunks,
                          void* partial, double beta2, double eps, int64_t step, void* stream);
int dvla_segment_combine(const void* partial, int64_t n_chunks, const int64_t* segs, int32_t n_segs, float* sumsq, float* absmax,
                         int64_t* nonfinite, int64_t n_out, void* stream);
/* (additive, ABI 9) Per-group gradient clipping: every parameter group has its own clip norm and its own
 * max_norm, inside the one launch per bucket of the grouped step.  A parameter of group g comes out bit-identical to that
 * parameter under the one-group entry points called with (lr[g], weight_decay[g]), grad_sumsq = &group_sumsq[g] and
 * max_norm[g] -- grad_sumsq = NULL for a group that is not clipped --, and depends on no other group's gradient.
 * dvla_group_sumsq: one launch of one wave, behind dvla_segment_stats_* over the gradient buckets and dvla_segment_combine.
 *   param_sumsq[i], i < n_params, is parameter i's sum of squares and group_of[i] its group (one byte; an id >= n_groups: the
 *   parameter is in no sum).  group_sumsq[g], g < n_groups, = the sum of the group's parameters in index order, accumulated in
 *   double and rounded to fp32 once (a non-finite term reaches its own group only: nothing is multiplied by a mask); a group
 *   without parameters gets 0.  total (may be NULL) receives group_sumsq[0] + group_sumsq[1] + ... added in fp32 in index
 *   order, the chain of dvla_step_verdict over the same slots, so the guarded and the unguarded step see the same total.  No
 *   atomics, and two calls give the same bits; with per-parameter terms from the segmented reduction the result does not
 *   depend on how the parameters are laid out in buckets.
 *   DVLA_ERR_ARG: a null pointer (total excepted), n_params < 0, n_groups outside 1 .. DVLA_STEP_MAX_GROUPS.
 * dvla_adamw_bf16_grouped_clip / dvla_adamw_f32_master_grouped_clip / dvla_adamw_bf16_sr_clip: dvla_adamw_bf16_grouped /
 *   dvla_adamw_f32_master_grouped / dvla_adamw_bf16_sr with the clip coefficient per group instead of per launch:
 *   group_sumsq: device memory, n_groups floats (dvla_group_sumsq's), read by the kernel -- no host synchronisation;
 *   max_norm:    a HOST array of n_groups floats, copied into the kernel arguments; max_norm[g] > 0: group g's gradient is
 *                scaled by min(1, max_norm[g] / (sqrt(group_sumsq[g]) + 1e-6)), the one-group kernels' expression; anything
 *                else (<= 0, NaN): group g is not clipped and group_sumsq[g] is not read.
 *   state != NULL: the guarded step; the verdict is dvla_step_verdict's over the group sums (one verdict per step, not per
 *   group) and state->sumsq is not used for clipping.  dvla_adamw_bf16_sr_clip needs a group_map (the one-group step has one
 *   clip norm: dvla_adamw_bf16_sr).
 *   Errors as the entry point without `_clip`, + DVLA_ERR_ARG for group_sumsq == NULL, max_norm == NULL and, for
 *   dvla_adamw_bf16_sr_clip, group_map == NULL.  All of these return before anything touches the device. */
int dvla_group_sumsq(const float* param_sumsq, const uint8_t* group_of, int32_t n_params, int32_t n_groups, float* group_sumsq,
                     float* total, void* stream);
int dvla_adamw_bf16_grouped_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                                 const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay,
                                 float beta1, float beta2, float eps, int64_t step, const float* group_sumsq, const float* max_norm,
                                 const dvla_step_state* state, const float* ema_w, int32_t n_cand, void* stream);
int dvla_adamw_f32_master_grouped_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                       float* ema, int64_t n, const uint8_t* group_map, int32_t n_groups, const double* lr,
                                       const double* weight_decay, double beta1, double beta2, double eps, int64_t step,
                                       const float* group_sumsq, const float* max_norm, const dvla_step_state* state,
                                       const float* ema_w, int32_t n_cand, void* stream);
int dvla_adamw_bf16_sr_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, float* ema, int64_t n,
                            const uint8_t* group_map, int32_t n_groups, const double* lr, const double* weight_decay, float beta1,
                            float beta2, float eps, int64_t step, const float* group_sumsq, const float* max_norm,
                            const dvla_step_state* state, const float* ema_w, int32_t n_cand, uint64_t sr_seed, int32_t sr_bucket,
                            int64_t sr_index_base, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Token assembly (models/dreamvla_model.py:739-759): out[b, s, t, :] = part_k[b, s, t - tok_begin_k, :] + pos[s, :]
 * for the part k that owns token t -- the per-frame conditioning tokens (text, state, resampled image tokens, cls tokens)
 * and the learned prediction-query tokens (stride_b = stride_s = 0: broadcast parameters) -- replacing torch.cat + the
 * window-position add.  Parts cover [0, T) in order; element strides; every base 16-byte aligned; H % 8 == 0.
 * pos may be NULL (no add) and is read at pos + s * pos_stride_s.  bf16.
 */
#define DVLA_MAX_TOKEN_SRCS 16
typedef struct dvla_token_src { const void* base; int64_t stride_b; int64_t stride_s; int32_t tok_begin; int32_t tok_count; } dvla_token_src;
int dvla_assemble_tokens(const dvla_token_src* srcs, int32_t n_src, const void* pos, int64_t pos_stride_s, void* out,
                         int32_t B, int32_t S, int32_t T, int32_t H, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Training-loss reductions (the caller-side loss block of the reference, utils/train_utils.py:172-450 + utils/sigloss.py:
 * patchify -> per-patch normalise -> (flow mask) -> MSE; 1 - cosine_similarity; SiLog on un-patchified depth).  bf16 data,
 * fp32 arithmetic, deterministic two-stage sums.  Tensors are addressed per FRAME through a view so the caller's slices
 * (prediction[:, view, 0], label[:, future : future + T]) are read in place: frame f lives at
 *   base + (f / T) * stride_b + (f % T) * stride_t          (element strides; the inner block of a frame is contiguous).
 * fwd: out2[0] = loss (fp32 scalar), out2[1] = auxiliary (SiLog: mean d, needed by bwd); `partial` = fp32 workspace of
 *      dvla_loss_partial_len() floats.   bwd: dpred (bf16, same addressing as pred) = grad_out[0] * dLoss/dpred.
 */
typedef struct dvla_frame_view { const void* base; int64_t stride_b; int64_t stride_t; int32_t T; } dvla_frame_view;
int64_t dvla_loss_partial_len(void);
/* pred frames (196, 768); image frames (3, 224, 224); patch_mask NULL or fp32 (n_frames, 196) of {0,1} */
int dvla_patch_mse_fwd(const dvla_frame_view* pred, const dvla_frame_view* image, const float* patch_mask, int64_t n_frames,
                       float* out2, float* partial, void* stream);
int dvla_patch_mse_bwd(const dvla_frame_view* pred, const dvla_frame_view* image, const float* patch_mask, int64_t n_frames,
                       const float* grad_out, const dvla_frame_view* dpred, void* stream);
/* pred / label frames (rows_per_frame, cols); cols % 8 == 0, cols <= 1024, and every view 16-byte aligned (base, and both
 * strides multiples of 8 elements): rows are read as 16-byte vectors.  DVLA_ERR_UNSUPPORTED otherwise, before any launch. */
int dvla_cosine_loss_fwd(const dvla_frame_view* pred, const dvla_frame_view* label, int32_t rows_per_frame, int32_t cols,
                         int64_t n_frames, float* out2, float* partial, void* stream);
int dvla_cosine_loss_bwd(const dvla_frame_view* pred, const dvla_frame_view* label, int32_t rows_per_frame, int32_t cols,
                         int64_t n_frames, const float* grad_out, const dvla_frame_view* dpred, void* stream);
/* pred frames (196, 256) = 16x16 depth patches; depth frames (1, 224, 224) */
int dvla_silog_loss_fwd(const dvla_frame_view* pred, const dvla_frame_view* depth, int64_t n_frames, float lambd, float* out2,
                        float* partial, void* stream);
int dvla_silog_loss_bwd(const dvla_frame_view* pred, const dvla_frame_view* depth, int64_t n_frames, float lambd, const float* out2,
                        const float* grad_out, const dvla_frame_view* dpred, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Attention-mask tables from the block-mask RULE, on the device.
 * Replaces the per-step host regeneration + upload of the (L, L) additive mask in the pretrain phase
 * (models/dreamvla_model.py:610-628 calling generate_attention_mask, 25-66) and the host-side derivation of the
 * kernels' tables from it.  `rule` are generate_attention_mask's own arguments; `drop` (device, [K][n_drop] int32) are
 * the obs-token indices that `mask_l_obs_ratio` drew for each window step with numpy's RNG on the host (n_drop =
 * int(ratio * num_obs); the draw stays on the host so the stream is consumed exactly as the reference consumes it).
 * Outputs (device, caller-allocated): key_index (Lk int32), bits_q (L x ceil(Lk/32) uint32), bits_k (Lk x ceil(L/32)),
 * tile_map (ceil(L/32) x ceil(Lk/32) uint8), where L = K (num_A + num_B) and Lk = K (num_A + kept obs columns) --
 * exactly the tables dvla_attn_fwd / dvla_attn_bwd take.  No host synchronisation, capturable. */
typedef struct dvla_mask_rule {
  int32_t K, num_A, num_B, num_obs, action_pred_steps;
  int32_t atten_goal, atten_goal_state, atten_only_obs, attn_robot_proprio_state;
  int32_t n_drop;
} dvla_mask_rule;
int dvla_mask_tables(const dvla_mask_rule* rule, const int32_t* drop, int32_t* key_index, uint32_t* bits_q, uint32_t* bits_k,
                     uint8_t* tile_map, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Camera-frame input pipeline on the device: uint8 HWC frames (already resized to the model's
 * resolution on the host) -> ToTensor (/255) -> CLIP Normalize (mean3 / std3, fp32, torch's operation order) ->
 * RandomShiftsAug as the integer-shift gather it is -> bf16 CHW.  Replaces, per frame, clip's `_transform` tail
 * (ToTensor + Normalize: utils/data_utils.py:175-178 via image_processor), RandomShiftsAug.forward / forward_traj
 * (utils/data_utils.py:326-383, applied by the collaters at 1337-1353) and the fp32 upload + cast of
 * utils/train_utils.py:118-123.  src: (n, H, W, 3) uint8; shift: (n, 2) int32 (sx, sy) in [0, 2 pad] or NULL (no
 * augmentation); out: (n, 3, H, W) bf16, 16-byte aligned; W % 8 == 0. */
int dvla_image_preprocess(const uint8_t* src, const int32_t* shift, void* out, int64_t n, int32_t height, int32_t width,
                          int32_t pad, const float* mean3, const float* std3, void* stream);
/* (additive, ABI 8) The head of that transform, Resize(n_px, BICUBIC) + CenterCrop(n_px), on raw uint8 frames, byte for byte what
 * Pillow's 8-bit resample gives: integer arithmetic on tables the CALLER builds in float64 exactly as Pillow does
 * (dreamvla_amd/preprocess.py: bicubic_tables).  src: (n, src_h, src_w, 3) uint8, contiguous, any alignment.
 * The frame is resampled to res_h x res_w -- horizontally first, that result rounded to uint8, then vertically -- of which
 * out (n, n_px, n_px, 3) uint8 is the window at (crop_top, crop_left); only that window is computed.  Per axis: bounds (res, 2)
 * int32 = (first input index, tap count <= ksize) of every output index, 8-byte aligned; coef (res, ksize) int32 = the taps'
 * coefficients at 22 fractional bits;  output byte = clamp((2^21 + sum_t in[first + t] * coef[t]) >> 22, 0, 255)  in a signed 32-bit
 * accumulator.  An axis whose input and output size are equal is NOT resampled by Pillow: pass the identity table for it (bounds
 * (i, 1), coef 2^22, ksize 1).  One launch; the intermediate rows stay in LDS.
 * DVLA_ERR_ARG: a null pointer, a size < 1, a crop window outside res_h x res_w.  DVLA_ERR_UNSUPPORTED: the LDS plan of ONE
 * output row -- ksize_y rows of align16(3 n_px) bytes plus four staging buffers of 3 (min(src_w, ceil((n_px - 1) src_w / res_w) +
 * ksize_x)) + 31 bytes -- exceeds 64 KiB (at n_px = 224: sources up to 10 x n_px on their shorter side all fit, whatever the
 * longer side; 84 x 84, 200 x 200, 480 x 640 and 720 x 1280 run at 16 output rows per workgroup), src_h or src_w > 2^20,
 * n_px > 2^14, or more than 2^31 - 1 workgroups (n x ceil(n_px / rows per workgroup)). */
int dvla_image_resize_u8(const uint8_t* src, uint8_t* out, int64_t n, int32_t src_h, int32_t src_w, int32_t res_h, int32_t res_w,
                         const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x, const int32_t* bounds_y,
                         const int32_t* coef_y, int32_t ksize_y, int32_t crop_left, int32_t crop_top, int32_t n_px, void* stream);
/* (additive, ABI 8) MAE pretraining from raw frames: torchvision's resized_crop(frame, top, left, ch, cw, (n_px, n_px),
 * BICUBIC) followed by an optional horizontal flip, with ONE BOX PER FRAME, byte for byte what Pillow's crop -> resize -> transpose
 * gives: the arithmetic of dvla_image_resize_u8 on the tables of the size pairs (cw -> n_px) horizontally and (ch -> n_px) vertically,
 * the taps clipped at the crop's edge.  src: (n, src_h, src_w, 3) uint8, contiguous, any alignment.
 * crops: (n, 5) int32 on the device = (top, left, ch, cw, flip) per frame; flip != 0 writes output column x to n_px - 1 - x.
 * table_store: int32 on the device, 8-byte aligned, built by the CALLER (dreamvla_amd/preprocess.py: _crop_table_store) for every input
 * size s = 0 .. max_size:  store[2 s] = offset (even, in int32 words from the base) of size s's tables, store[2 s + 1] = their ksize;
 * at the offset bounds (n_px, 2) = (first input index, tap count <= ksize) and behind them coefficients (n_px, ksize) at 22 fractional
 * bits (the identity table -- bounds (i, 1), coefficient 2^22, ksize 1 -- for s == n_px; size 0 is never read).
 * max_ch, max_cw: the largest ch and cw among the n descriptors (the host knows them: it drew the boxes); the launch's LDS plan is
 * made for them.  A frame whose box leaves the source, has ch or cw < 1, or exceeds max_ch / max_cw rows / columns WRITES NOTHING.
 * out_kind DVLA_CROP_OUT_U8: out (n, n_px, n_px, 3) uint8 at any address; mean3 / std3 unused (may be NULL).
 * out_kind DVLA_CROP_OUT_BF16: out (n, 3, n_px, n_px) bf16 = dvla_image_preprocess (no shift) of the uint8 kind, bit for bit: fp32
 * byte / 255, - mean3[c], / std3[c], one rounding to bf16; n_px % 8 == 0 and out 16-byte aligned, else DVLA_ERR_UNSUPPORTED.
 * n == 0: DVLA_OK.  DVLA_ERR_ARG: a null pointer, a size < 1, max_ch > min(src_h, max_size), max_cw > min(src_w, max_size), another
 * out_kind.  DVLA_ERR_UNSUPPORTED: the LDS plan of ONE output row -- min(max_ch, ksize(max_ch)) rows of align16(3 n_px) bytes plus
 * four staging buffers of 3 max_cw + 31 bytes -- exceeds 64 KiB, src_h or src_w > 2^20, n_px > 2^14, a misaligned table_store or
 * crops, or more than 2^31 - 1 workgroups. */
#define DVLA_CROP_OUT_U8 0
#define DVLA_CROP_OUT_BF16 1
int dvla_image_resized_crop(const uint8_t* src, void* out, const int32_t* crops, const int32_t* table_store, int64_t n, int32_t src_h,
                            int32_t src_w, int32_t max_size, int32_t max_ch, int32_t max_cw, int32_t n_px, int32_t out_kind,
                            const float* mean3, const float* std3, void* stream);
/* (additive, ABI 8) Depth labels on the device: raw fp32 depth maps -> the collator's nearest resize
 * (`depth_image_fn`, utils/data_utils.py:3588-3607 = F.interpolate(mode="nearest")) -> RandomShiftsAug as the integer-shift gather
 * -> cast, one launch:
 *   out[i, y, x] = cast(src[i, ry(clamp(y + sy_i - pad, 0, out_h - 1)), rx(clamp(x + sx_i - pad, 0, out_w - 1))])
 *   ry(j) = min((int)floorf(j * ((float)src_h / out_h)), src_h - 1), rx(j) likewise with the widths (ATen's source index, fp32).
 * src: (n, src_h, src_w) fp32, contiguous; shift: (n, 2) int32 (sx, sy) in [0, 2 pad] or NULL; shift == NULL or pad == 0: no shift.
 * out: (n, out_h, out_w) contiguous, out_dtype DVLA_DT_BF16 (round to nearest even) or DVLA_DT_F32 (the bits of src), at any
 * element-aligned address: rows that are not 16-byte aligned get scalar stores in front of and behind their 16-byte body.
 * n == 0: DVLA_OK.  DVLA_ERR_ARG: src or out null, a size < 1, n < 0, pad < 0.  DVLA_ERR_UNSUPPORTED: another out_dtype,
 * out_h + out_w > 16384 (the two index tables live in 64 KiB of LDS), src_h or src_w > 2^24, src or out not aligned to its element. */
int dvla_depth_preprocess(const float* src, const int32_t* shift, void* out, int64_t n, int32_t src_h, int32_t src_w, int32_t out_h,
                          int32_t out_w, int32_t pad, int32_t out_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Dreams at evaluation (an addition: the reference decodes its image / depth / feature predictions in mode="train" only).
 * dvla_gather_positions: out[b, t, :] = x[b, sel[b], tok_begin + t, :] -- the query rows of ONE window position per sequence
 *   (the position the evaluation wrapper executes) out of the trunk output x (B, S, T, H), read in place.  bf16, contiguous,
 *   16-byte aligned, H % 8 == 0; sel (B,) int64 on the device, clamped to [0, S).  out (B, tok_count, H).
 * dvla_dream_render: patch predictions -> frames, one launch, nothing but the frame written.  pred (n, grid_h * grid_w,
 *   patch * patch * channels) bf16 in the reference's patch layout (utils/train_utils.py:37-50 'nchpwq->nhwpqc': the values of
 *   a patch in (p, q, c) order).
 *   current == NULL: un-patchify only (utils/train_utils.py:783-799) -> out (n, channels, patch grid_h, patch grid_w) fp32;
 *     channels 3 (the image head, in the normalised space it was trained in) or 1 (the depth head).
 *   current != NULL (channels == 3): the model's own input frame (n, 3, patch grid_h, patch grid_w) bf16, CLIP-normalised.  The
 *     head's target is normalize_patchfied_image of the future frame (utils/train_utils.py:52-57); it is inverted with the mean
 *     and the unbiased variance of the SAME patch of `current` (x = pred * sqrt(var + 1e-6) + mean), then CLIP's Normalize is
 *     inverted with mean3 / std3 (x * std + mean), clamped to [0, 1], scaled by 255, rounded half-to-even
 *     -> out (n, patch grid_h, patch grid_w, 3) uint8.  fp32 arithmetic.
 *   patch == 16 (one wave per patch); anything else, or a misaligned base (pred / current 8, out 16 bytes):
 *   DVLA_ERR_UNSUPPORTED. */
int dvla_gather_positions(const void* x, const int64_t* sel, void* out, int32_t B, int32_t S, int32_t T, int32_t H,
                          int32_t tok_begin, int32_t tok_count, void* stream);
int dvla_dream_render(const void* pred, const void* current, void* out, int64_t n, int32_t grid_h, int32_t grid_w, int32_t patch,
                      int32_t channels, const float* mean3, const float* std3, void* stream);
/* (additive, ABI 8) Scoring a dream against the frame that arrived (an addition; csrc/dream_score.hip).
 * Both are two launches -- partials of one tile / chunk each into `partial`, then one workgroup per image adding them in a fixed
 * order -- without atomics: an image's results are bit-identical from run to run, whatever n and its place in the batch.
 * `partial`: 4-byte aligned workspace of dvla_*_quality_partial_len(n, height, width) 4-byte words, every word written before read.
 * dvla_image_quality: a, b (n, height, width, 3) uint8 contiguous at any address.  sse[i] (int64) = the sum of squared byte
 *   differences of image i, exact.  mse_psnr_ssim (n, 3) fp32 = sse / (3 height width); 10 log10(255^2 / mse), +inf when sse = 0;
 *   the mean SSIM (Wang et al. 2004): 11 x 11 Gaussian window of sigma 1.5 normalised to sum 1, C1 = (0.01 * 255)^2, C2 =
 *   (0.03 * 255)^2, population (co)variances, evaluated at the (height - 10) x (width - 10) positions whose window lies inside the
 *   image, per channel, averaged over positions and channels.  fp32 moments of the pixels centred at 128, the sums of the map
 *   in float64.  height < 11 or width < 11, or more than 2^31 - 1 tiles: DVLA_ERR_UNSUPPORTED.
 * dvla_depth_quality: pred, target (n, height, width) fp32 contiguous.  Over the pixels with target > 0, with p = max(pred, 0):
 *   valid[i] (int64) = their number; metrics4 (n, 4) fp32 = mean |p - t| / t; sqrt(mean (p - t)^2); SiLog with the training loss's
 *   constants, d = log(t + 1e-6) - log(p + 1e-6), sqrt(mean d^2 - 0.5 mean(d)^2); the share with max(p / t, t / p) < 1.25.
 *   valid[i] == 0: the four metrics are NaN.
 * Both: n == 0: DVLA_OK, nothing launched.  DVLA_ERR_ARG: a null pointer, n < 0, a size < 1. */
int64_t dvla_image_quality_partial_len(int64_t n, int32_t height, int32_t width);
int dvla_image_quality(const uint8_t* a, const uint8_t* b, int64_t n, int32_t height, int32_t width, int64_t* sse,
                       float* mse_psnr_ssim, void* partial, void* stream);
int64_t dvla_depth_quality_partial_len(int64_t n, int32_t height, int32_t width);
int dvla_depth_quality(const float* pred, const float* target, int64_t n, int32_t height, int32_t width, int64_t* valid,
                       float* metrics4, void* partial, void* stream);
/* (additive, ABI 9) The depth, motion and feature dreams as pictures (an addition, DESIGN.md section 5 item 26;
 * csrc/dream_view.hip).  uint8 HWC out, no atomics, a frame's bytes do not depend on the batch.  All of them: n == 0: DVLA_OK,
 * nothing launched; DVLA_ERR_ARG: a null pointer, n < 0, a size < 1, a colour outside 0 .. 255; DVLA_ERR_UNSUPPORTED as listed.
 * level(v, lo, hi), shared by the depth and feature pictures, in fp32 with one rounding per operation (no FMA):
 *   s = v - lo; r = hi - lo; t = s / r; t = (r > 0 and t > 0) ? min(t, 1) : 0 (hi == lo, a NaN quotient: 0); rint(255 * t), half to even.
 * dvla_depth_colorize: depth (n, height, width) fp32 -> out (n, height, width, 3) = palette[level(d, lo, hi)], palette (256, 3)
 *   uint8 on the device; a non-finite pixel gets (nan_r, nan_g, nan_b).  own_range == 0: lo <= hi, both finite (else
 *   DVLA_ERR_ARG).  own_range != 0: lo / hi are per map the min / max over its finite pixels, two launches through `partial`
 *   (dvla_depth_range_partial_len(n, height, width) 4-byte words, every word written before it is read).  n > 65535: unsupported.
 * dvla_flow_unshuffle: pred (n, tokens, 2 factor^2) bf16, channel = c factor^2 + i factor + j (F.pixel_unshuffle's order, the
 *   trajectory head's target) -> flow (n, g factor, g factor, 2) fp32, flow[y factor + i, x factor + j, c]; exact.  tokens = g^2,
 *   factor in {1, 2, 4}, flow 8-byte aligned, else unsupported.
 * dvla_flow_wheel: flow (n, in_h, in_w, 2) fp32, 8-byte aligned -> out (n, out_h, out_w, 3), nearest (src = dst * in / out, integer
 *   division): angle = atan2(dy, dx) in degrees in [0, 360), Hh = trunc(angle / 2), V = trunc(min(32 |flow|, 255)), S = 255;
 *   s = Hh / 30, X = (V (30 - |Hh % 60 - 30|) + 15) / 30, (R, G, B) = (V,X,0) (X,V,0) (0,V,X) (0,X,V) (X,0,V) (V,0,X) for s = 0 .. 5.
 *   A non-finite flow is black.
 * dvla_motion_mask: pred as dvla_flow_unshuffle takes it -> mask (n, g, g) uint8 in {0, 1}: mx, my = the fp32 means of the token's
 *   factor^2 dx / dy; mx^2 + my^2 > thr^2; dilate != 0: the OR over the 3 x 3 neighbourhood inside the grid.  thr >= 0, finite.
 * dvla_motion_overlay: current (n, 3, height, width) bf16, CLIP-normalised (dvla_dream_render's `current`), 8-byte aligned ->
 *   out (n, height, width, 3) 4-byte aligned: v = rint(255 clamp(x std + mean, 0, 1)) as dvla_dream_render de-normalises, and in
 *   the cells of mask (n, grid, grid) that are non-zero (v (256 - alpha) + tint alpha + 128) >> 8, 0 <= alpha <= 256.  height and
 *   width multiples of grid, width % 4 == 0, else unsupported.
 * dvla_feature_render: feat (n, tokens, dim) bf16, proj (dim, 3) fp32, both 16-byte aligned, dim % 8 == 0, tokens = g^2 (else
 *   unsupported) -> out (n, out_h, out_w, 3): per token p_k = sum_d x_d proj[d, k] + b_k (fp32), byte k = level(p_k, lo_k, hi_k),
 *   written to the pixels y, x with y g / out_h, x g / out_w (integer division) = the token. */
int64_t dvla_depth_range_partial_len(int64_t n, int32_t height, int32_t width);
int dvla_depth_colorize(const float* depth, uint8_t* out, int64_t n, int32_t height, int32_t width, const uint8_t* palette,
                        int32_t own_range, float lo, float hi, int32_t nan_r, int32_t nan_g, int32_t nan_b, void* partial, void* stream);
int dvla_flow_unshuffle(const void* pred, float* flow, int64_t n, int32_t tokens, int32_t factor, void* stream);
int dvla_flow_wheel(const float* flow, uint8_t* out, int64_t n, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, void* stream);
int dvla_motion_mask(const void* pred, uint8_t* mask, int64_t n, int32_t tokens, int32_t factor, float thr, int32_t dilate, void* stream);
int dvla_motion_overlay(const uint8_t* mask, const void* current, uint8_t* out, int64_t n, int32_t grid, int32_t height, int32_t width,
                        float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, int32_t tint_r,
                        int32_t tint_g, int32_t tint_b, int32_t alpha, void* stream);
int dvla_feature_render(const void* feat, const float* proj, uint8_t* out, int64_t n, int32_t tokens, int32_t dim, int32_t out_h,
                        int32_t out_w, float b0, float b1, float b2, float lo0, float lo1, float lo2, float hi0, float hi1, float hi2,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------
 * MAE pretraining (models/vit_mae.py:129-256): random masking, the decoder's token un-shuffle and the patch-MSE loss, each
 * one pass instead of the reference's argsort / gather / cat / add / patchify / mean / var chains.  Deterministic: no float
 * atomics, fixed-order two-stage sums.  bf16 activations, fp32 arithmetic; all tensors contiguous unless a stride is given,
 * every bf16 row base 16-byte aligned.
 *
 * dvla_mae_mask_fwd: per sample n, ids_shuffle = the ascending order of noise[n, :] with ties broken by index (exactly
 * torch.argsort(noise, dim=1, stable=True)); ids_restore[n, ids_shuffle[r]] = r (int64); mask[n, l] = (ids_restore[n, l] >=
 * len_keep) in {0, 1} fp32; out (N, c + len_keep, D) = [cls_row ; x[n, ids_shuffle[n, :len_keep]]] where c = 1, or c = 0 and no
 * cls row when cls_row is NULL.  noise (N, L) fp32, x (N, L, D) bf16, cls_row (D,) bf16.  L <= 1024, 0 < len_keep <= L,
 * D % 8 == 0, else DVLA_ERR_UNSUPPORTED.
 * dvla_mae_mask_bwd: dx (N, L, D) = dout's row c + ids_restore[n, l] where that is a kept row, else 0 (the cls row's gradient
 * is the caller's column sum of dout[:, 0, :]).  ids_restore outside [0, L) reads as removed. */
int dvla_mae_mask_fwd(const float* noise, const void* x, const void* cls_row, int32_t N, int32_t L, int32_t D, int32_t len_keep,
                      int64_t* ids_restore, float* mask, void* out, void* stream);
int dvla_mae_mask_bwd(const int64_t* ids_restore, const void* dout, int32_t has_cls, int32_t N, int32_t L, int32_t D,
                      int32_t len_keep, void* dx, void* stream);
/* dvla_mae_unshuffle_fwd (models/vit_mae.py:213-219): out (N, 1 + L, D) with out[n, 0] = y[n, 0] + pos[0] and out[n, 1 + l] =
 * (r = ids_restore[n, l] in [0, len_keep) ? y[n, 1 + r] : mask_token) + pos[1 + l], each element one fp32 add of the bf16
 * operands rounded once (ATen's bf16 add).  y (N, 1 + len_keep, D), mask_token (D,), pos (1 + L, D), all bf16.
 * dvla_mae_unshuffle_bwd: dy (N, 1 + len_keep, D) bf16 = the gather of dout's cls row and kept rows (rows of dy that no
 * ids_restore entry names are zero); dmask_token (D,) in dmask_dtype = the fp32 sum over all removed rows of all samples in a
 * fixed order, rounded once.  `partial` = 4 * N * D floats of workspace.  D % 8 == 0 and D <= 2048, L <= 1024, N <= 65535 (also
 * for dvla_mae_mask_bwd). */
int dvla_mae_unshuffle_fwd(const void* y, const void* mask_token, const int64_t* ids_restore, const void* pos, int32_t N, int32_t L,
                           int32_t D, int32_t len_keep, void* out, void* stream);
int dvla_mae_unshuffle_bwd(const void* dout, const int64_t* ids_restore, int32_t N, int32_t L, int32_t D, int32_t len_keep, void* dy,
                           void* dmask_token, int32_t dmask_dtype, float* partial, void* stream);
/* dvla_mae_loss_fwd / _bwd (models/vit_mae.py:129-141,234-250): forward_loss fused with patchify.  Sample n's L = (H / p) (W / p)
 * patch predictions are the bf16 rows pred + n * pred_stride_n + (row0 + l) * pred_stride_r, P = 3 p^2 contiguous elements
 * each; element e = (py p + px) 3 + c of patch l = ph (W / p) + pw is imgs[n, c, ph p + py, pw p + px] ('nchpwq->nhwpqc').
 * norm_pix != 0: the target is (t - mean) / sqrt(var + 1e-6) per patch, var unbiased.  mask (N, L) fp32.
 * fwd: out2[0] = sum(mask * mean_P((pred - target)^2)) / sum(mask), out2[1] = sum(mask); partial = dvla_mae_loss_partial_len()
 * floats.  bwd: dpred (N, row0 + L, P) bf16 contiguous = grad_out[0] * dloss/dpred (out2[1] from the forward), rows < row0
 * zero.  p <= 16, imgs_dtype fp32 or bf16, H and W multiples of p, else DVLA_ERR_UNSUPPORTED. */
typedef struct dvla_mae_loss_params {
  const void* pred; int64_t pred_stride_n; int64_t pred_stride_r; int32_t row0; int32_t patch;
  const void* imgs; int32_t imgs_dtype; int32_t norm_pix; int32_t H; int32_t W;
  const float* mask; int64_t N;
} dvla_mae_loss_params;
int64_t dvla_mae_loss_partial_len(void);
int dvla_mae_loss_fwd(const dvla_mae_loss_params* p, float* out2, float* partial, void* stream);
int dvla_mae_loss_bwd(const dvla_mae_loss_params* p, const float* out2, const float* grad_out, void* dpred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVLA_H_ */
