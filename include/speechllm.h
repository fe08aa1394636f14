/*
 * speechllm.h — C ABI of libspeechllm.so: the MI355X (gfx950) hot path of the speech-prompted LLM
 * pipeline (HuBERT encoder -> pooled projector -> Llama prefill + KV-cached greedy decode).
 *
 * The reference (wonjune-kang/llm-speech-summarization) has no native code and no FFI: its hot path
 * is Python calling HuggingFace `transformers` modules.  Each entry point below therefore cites the
 * reference / HF call it replaces (ref: = /root/reference, hf: = site-packages/transformers).  The
 * Python host mirror of the reference classes (the .py files of llm-speech-summarization_amd/) binds these with
 * ctypes; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no C++ / torch types cross this boundary.
 *   - Every device buffer (weights, activations, KV cache, workspace) is allocated and owned by the
 *     caller.  The library never allocates or frees device memory.  Per-op entry points (sl_gemm*, sl_attn_*,
 *     norms, losses, the KD tape stacks ...) only enqueue launches on `stream` and never synchronise.
 *     The whole-model entry points that take HOST descriptor arrays synchronise as follows:
 *       sl_hubert_forward, sl_whisper_forward, sl_llama_prefill — ONE hipStreamSynchronize(stream) after uploading the
 *         batch descriptors (row offsets / group records built from the host arrays), before the first compute launch;
 *       sl_greedy_generate — that of its prefill, one every `check_every` steps when EOS is enabled, and ONE at the end
 *         behind the asynchronous copy of the ids to the host (the call returns host results).
 *     Nothing synchronises the device or touches the null stream.
 *   - Return value: 0 on success, a negative sl_status otherwise; sl_last_error() gives the text.
 *   - dtype: SL_F32 (exact-fp32 MFMA, the parity mode), SL_BF16 (bf16 storage, fp32 accumulate) or SL_F16
 *     (fp16 storage, fp32 accumulate; norms and softmax statistics in fp32, as for bf16; values beyond the fp16
 *     range become +-inf, no clamping).  SL_F16 is an inference dtype: the forward entry points take it, the
 *     training-only entry points (attention backward, the tapes, post_op / colsum_out / transposed products,
 *     the AdamW dst_dtype, sl_allreduce_sum) return SL_ERR_ARG for it.
 *   - Layouts: activations row-major (tokens, channels); Linear weights in nn.Linear layout
 *     (out_features, in_features); conv weights re-laid out by the host as documented per call.
 */
#ifndef SPEECHLLM_H
#define SPEECHLLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sl_stream; /* hipStream_t */

enum sl_dtype { SL_F32 = 0, SL_BF16 = 1, SL_F16 = 2 };
enum sl_status {
  SL_OK = 0,
  SL_ERR_ARG = -1,      /* bad shape / alignment / enum */
  SL_ERR_LAUNCH = -2,   /* HIP launch or runtime error */
  SL_ERR_UNSUPPORTED = -3
};
enum sl_act { SL_ACT_NONE = 0, SL_ACT_GELU = 1, SL_ACT_SILU_MUL = 2, SL_ACT_ROPE_KV = 3 };
enum sl_w_layout { SL_W_ROWMAJOR = 0, SL_W_PACKED = 1 };
#define SL_W_PACKED_E4M3 2                       /* sl_gemm_args.w_layout: an e4m3 weight image (sl_pack_weight_e4m3) */
#define SL_W_PACKED_MXFP4 4                      /* sl_gemm_args.w_layout: an MXFP4 weight image (sl_pack_weight_mxfp4); 3 is not a layout */

const char* sl_last_error(void);       /* thread-local, never NULL */
#define SL_ABI_VERSION 7
int sl_version(void);                  /* == SL_ABI_VERSION of the header the library was built from; bumps on any signature change */
int sl_device_arch(char* buf, int n);  /* gcnArchName of the current device, e.g. "gfx950:sramecc+:xnack-" */
/* Tuning switches (SL_* environment variables, documented in csrc/common.h) are read once, at first use; tools that change
 * them inside one process call this to re-read them.  Not needed in normal operation. */
int sl_tuning_reload(void);

/* ---------------------------------------------------------------------------------------------
 * GEMM  C[b] = act(A[b] . W[b]^T + bias[b]) + residual[b]        (TN: both operands K-contiguous)
 * Replaces every nn.Linear / F.linear on the path (hf:models/hubert/modeling_hubert.py:229,
 * 293-300,340,360-365; hf:models/llama/modeling_llama.py:174-176,254-256,280; lm_head
 * ref:model/audio_llama.py:67) and, through lda < K (overlapping rows), the strided Conv1d layers
 * 1..6 of the HuBERT feature extractor (hf:...hubert.py:141) and the grouped positional conv
 * (hf:...hubert.py:47-53) as implicit GEMMs without an im2col buffer.
 *   A: (M, K) row stride lda;  W: (N, K) row stride ldw;  C: (M, Nout) row stride ldc
 *   act == SL_ACT_SILU_MUL: W rows come in blocks of 16 gate rows followed by 16 up rows;
 *     Nout = N/2, C[m][16p+c] = silu(gate) * up  (hf:...llama.py:175).  Otherwise Nout = N.
 *   bias (N) and residual (M, Nout; row stride ldr) may be NULL.  Order: +bias, act, +residual.
 *   out_f32 != 0 writes C as float regardless of dtype (logits).
 *   Requirements: K % 8 == 0 (bf16) / K % 4 == 0 (f32); A, W 16-byte aligned rows.
 *   M <= 64 with row-major weights dispatches to the weight-streaming (HBM-bound) skinny kernel; packed weights
 *   (sl_pack_weight) run the skinny kernel up to 32 rows and the LDS-staged streaming kernel (gemm_stream.hip) above.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const void* A; int64_t lda; int64_t strideA;
  const void* W; int64_t ldw; int64_t strideW;
  void* C; int64_t ldc; int64_t strideC;
  const void* bias; int64_t strideBias;
  const void* residual; int64_t ldr; int64_t strideR;
  int32_t M, N, K, batch;
  int32_t dtype, act, out_f32, w_layout;
} sl_gemm_args;
int sl_gemm(const sl_gemm_args* a, sl_stream stream);

/* Fragment-major weight packing for the decode weight-streaming kernels:
 *   dst[f][s][lane][e] = src[16 f + (lane & 15)][KSTEP s + VEC (lane >> 4) + e],  VEC = 8 (bf16) / 4 (f32),
 *   KSTEP = 4 VEC, f < ceil(N/16) (rows past N are zero), so one wave-level weight load is 1 KiB contiguous
 *   (+25..45 % HBM throughput over 16 x 64-byte row segments, tools/tune_skinny.hip).  K %% KSTEP == 0.
 *   dst holds ceil(N/16)*16*K elements.  Pass it to sl_gemm with w_layout = SL_W_PACKED. */
int sl_pack_weight(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream);

/* Weight-only fp8 for the decode step of small batches: the "e4m3 weight image" of a bf16 / fp16 weight W (N, K), K % 64 == 0,
 * Np = ceil(N/16)*16.  One fp32 scale per output row, s[n] = max_k |W[n][k]| / 448 (a correctly rounded division; 1 for an all-zero
 * row and for the padding rows n >= N), and one OCP e4m3fn byte per element, b[n][k] = q8(float(W[n][k]) / s[n]) with the K/V
 * cache's quantiser (round to nearest even, saturating at +-448: no byte is 0x7F / 0xFF); padding rows are zero bytes.  Bytes are
 * fragment-major over PAIRS of 32-wide MFMA k-steps, so a lane load is still 16 bytes and a wave load 1 KiB contiguous:
 *   img[f][j][lane][0..7]  = b[16 f + (lane & 15)][64 j + 8 (lane >> 4) + e]
 *   img[f][j][lane][8..15] = b[16 f + (lane & 15)][64 j + 32 + 8 (lane >> 4) + e],      f < Np/16, j < K/64
 * and the Np scales follow the bytes in the same buffer, at byte offset Np*K: one pointer names a whole weight.
 *   sl_w8_image_bytes       Np*K + 4*Np; 0 on a bad argument (N <= 0, K <= 0, K % 64 != 0)
 *   sl_pack_weight_e4m3     src (N, K) row stride ld_src on the device -> dst (16-byte aligned, sl_w8_image_bytes) on the device
 *   sl_pack_weight_e4m3_host the same routine on host memory (no GPU needed)
 *   sl_w8_max_rows          largest row count the e4m3 skinny kernels take (the packed skinny range: SL_STREAM_MIN_M, 26 by default)
 * SL_F32 is SL_ERR_UNSUPPORTED, K % 64 != 0 is SL_ERR_ARG.  sl_gemm / sl_gemm_fused_decode take the image with
 * w_layout = SL_W_PACKED_E4M3 for up to sl_w8_max_rows() rows (more: SL_ERR_UNSUPPORTED, nothing is launched): activations, the
 * accumulation and the output stay as they are; the fp32 sum of output row n is multiplied by s[n] before bias, the fuse_rms row
 * factor and the pair epilogues.  fuse_rms may take rstd_in here.  GELU, batches, transposes and groups are not built. */
size_t sl_w8_image_bytes(int32_t N, int32_t K);
int sl_pack_weight_e4m3(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream);
int sl_pack_weight_e4m3_host(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype);
int32_t sl_w8_max_rows(void);

/* Weight-only 4-bit for the decode step of small batches: the "MXFP4 weight image" of a bf16 / fp16 weight W (N, K), K % 128 == 0,
 * Np = ceil(N/16)*16.  The OCP MX format: e2m1 elements in blocks of 32 consecutive k of one row, one e8m0 scale byte per block.
 *   Block scale: amax = max |w| of the block (NaN elements skipped); e = the smallest integer with amax <= 6 * 2^e, clamped to
 *   [-13, 13]; an all-zero block and every padding row take e = 0; the byte is e + 127.  With the clamp every dequantised value
 *   (0.5 * 2^-13 .. 6 * 2^13) is a normal number in fp16 as well as in bf16: one image serves both model dtypes.
 *   Elements: float(w) / 2^e rounded to the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6}, to nearest with ties to the even code, saturating
 *   at +-6 (inf included; a NaN element becomes code 0); the sign is bit 3; a value that rounds to zero is code 0x0 (no negative zero).
 *   Layout: fragment-major over QUADS of 32-wide MFMA k-steps, img[f][j][lane][16 B], f < Np/16, j < K/128, 64 lanes.  Dword d (0..3)
 *   of a lane's 16 bytes holds the 8 elements k = 128 j + 32 d + 8 (lane >> 4) + i of row 16 f + (lane & 15); element 2b is the low
 *   nibble of byte b, element 2b+1 the high nibble.  A lane load is 16 bytes, a wave load 1 KiB contiguous, and one dword is the A
 *   fragment of one 16x16x32 MFMA after four v_cvt_scalef32_pk_{bf16,f16}_fp4 (byte select 0..3).
 *   Scales: behind the elements, at byte offset Np*K/2, as sc[f][j][r][d]: one byte for row 16 f + r, block 4 j + d, so a lane reads
 *   its four scales as one dword at ((f * K/128 + j) * 16 + (lane & 15)) * 4.  One pointer names a whole weight.
 *   sl_w4_image_bytes        Np*K/2 + Np*K/32; 0 on a bad argument (N <= 0, K <= 0, K % 128 != 0)
 *   sl_pack_weight_mxfp4     src (N, K) row stride ld_src on the device -> dst (16-byte aligned, sl_w4_image_bytes) on the device
 *   sl_pack_weight_mxfp4_host the same routines on host memory (no GPU needed): the same bits
 *   sl_w4_max_rows           largest row count the MXFP4 skinny kernels take: sl_w8_max_rows()
 * SL_F32 is SL_ERR_UNSUPPORTED, K % 128 != 0 is SL_ERR_ARG.  sl_gemm / sl_gemm_fused_decode take the image with
 * w_layout = SL_W_PACKED_MXFP4 for up to sl_w4_max_rows() rows (more: SL_ERR_UNSUPPORTED, nothing is launched).  The MFMA operands are
 * exactly the dequantised values e2m1 * 2^e (the scale is applied by the conversion), so the product is the 16-bit kernel's on
 * dq(W): no scale multiply follows the reduction.  fuse_rms may take rstd_in.  GELU, batches, transposes and groups are not built. */
size_t sl_w4_image_bytes(int32_t N, int32_t K);
int sl_pack_weight_mxfp4(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream);
int sl_pack_weight_mxfp4_host(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype);
int32_t sl_w4_max_rows(void);

/* Block-scaled ("MX") linears, opt-in (sl_llama_model.reserved = SL_WDEC_MX_LINEAR): MXFP8 activations x MXFP4 weights on
 * v_mfma_scale_f32_16x16x128_f8f6f4 -> fp32 -> model dtype, at every row count.
 *
 * The "MX weight image" of a bf16 / fp16 weight W (N, K), K % 128 == 0, Np = ceil(N/16)*16.  Element codes and scale bytes are
 * EXACTLY those of the MXFP4 weight image above (block scale rule, clamp of e to [-13, 13], e2m1 rounding, saturation, NaN and
 * zero handling; padding rows are zero codes with scale byte 127); only the arrangement differs, because the scaled MFMA wants,
 * per lane, 32 CONSECUTIVE k of one row and ONE scale:
 *   Elements: img[f][j][lane][16 B], f < Np/16, j < K/128, 64 lanes.  A lane's 16 bytes are one whole 32-element block: byte b
 *   holds the elements k = 128 j + 32 (lane >> 4) + 2 b (low nibble) and + 2 b + 1 (high nibble) of row 16 f + (lane & 15).
 *   A lane load is 16 bytes, a wave load 1 KiB contiguous, and the 16 bytes are the low four operand registers of one
 *   v_mfma_scale_f32_16x16x128_f8f6f4 with the e2m1 operand format.
 *   Scales: behind the elements, at byte offset Np*K/2, as sc[f][j][lane]: one byte, the scale of that lane's block (row
 *   16 f + (lane & 15), block 4 j + (lane >> 4)), so a lane reads its own scale with one byte load at (f * K/128 + j) * 64 + lane.
 *   One pointer names a whole weight.
 *   sl_mx_weight_image_bytes  Np*K/2 + Np*K/32; 0 on a bad argument (N <= 0, K <= 0, K % 128 != 0)
 *   sl_pack_weight_mx         src (N, K) row stride ld_src on the device -> dst (16-byte aligned) on the device
 *   sl_pack_weight_mx_host    the same routines on host memory (no GPU needed): the same bits
 * SL_F32 is SL_ERR_UNSUPPORTED, K % 128 != 0 is SL_ERR_ARG.
 *
 * "MXFP8 activation rows" of x (M, K) bf16 / fp16, row stride ldx, K % 32 == 0: q (M, K) bytes, row-major, OCP e4m3fn, and
 * scales (M, K/32) e8m0 bytes, row-major, one per 32 consecutive k of one row.
 *   Block scale: amax = max |x| over the FINITE elements of the block; e = the smallest integer with amax <= 448 * 2^e, clamped
 *   to [-127, 127]; a block without a nonzero finite element takes e = 0; the byte is e + 127.
 *   Elements: x / 2^e rounded to e4m3, to nearest with ties to even, subnormals (multiples of 2^-9) included, saturating at
 *   +-448: with this rule no finite element is ever clipped, +-inf becomes +-448 (0x7E / 0xFE) and NaN becomes 0x7F.  The sign bit
 *   is the element's own: a negative value that rounds to zero, and -0, are 0x80.
 *   sl_mxfp8_quantize_rows_host is the definition (host memory, no GPU needed); sl_mxfp8_quantize_rows gives the same bytes
 *   on the device (q 16-byte aligned).  SL_F32 is SL_ERR_UNSUPPORTED, K % 32 != 0 is SL_ERR_ARG.
 *
 * sl_gemm_mx: C = act(dq(Aq) . dq(W)^T) + residual, dq(.) = element * 2^(scale byte - 127), accumulated in fp32.
 *   Aq (M, K) e4m3 bytes with row stride lda (a multiple of 16, 16-byte aligned), a_scales (M, K/32), W an MX weight image of
 *   (N, K); any M >= 1, any N >= 1 (the image's padding rows produce columns that are not stored), K % 128 == 0.
 *   act: SL_ACT_NONE, or SL_ACT_SILU_MUL with sl_gemm's 16 gate / 16 up row interleave (N % 32 == 0, N/2 output columns).
 *   residual (M, Nout; row stride ldr; may be C itself) is of the output type `dtype` (SL_BF16 / SL_F16); out_f32 != 0 writes
 *   C as float.  A row's result does not depend on M: no K split, one accumulation chain per output. */
size_t sl_mx_weight_image_bytes(int32_t N, int32_t K);
int sl_pack_weight_mx(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream);
int sl_pack_weight_mx_host(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype);
int sl_mxfp8_quantize_rows(const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype, sl_stream stream);
int sl_mxfp8_quantize_rows_host(const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype);
typedef struct {
  const void* Aq; int64_t lda; const void* a_scales;
  const void* W;
  void* C; int64_t ldc;
  const void* residual; int64_t ldr;
  int32_t M, N, K;
  int32_t dtype, act, out_f32;
} sl_gemm_mx_args;
int sl_gemm_mx(const sl_gemm_mx_args* a, sl_stream stream);

/* Decode-only fusions on top of sl_gemm (packed weights; M <= 16 rows run the skinny kernel, more rows the
 * LDS-staged streaming kernel of gemm_stream.hip):
 *   fuse_rms  — the consuming Linear absorbs the preceding LlamaRMSNorm (hf:...llama.py:62-67): the
 *               gain is pre-multiplied into W on the host and out[m] *= rsqrt(mean(x[m]^2) + rms_eps),
 *               with the mean taken from the activation fragments the kernel streams anyway;
 *   act == SL_ACT_ROPE_KV — N = (n_heads + 2 n_kv) * 128 fused q|k|v rows whose q/k heads are stored
 *               in 16-row blocks alternating the two rotate_half halves ([0:16],[64:80],[16:32],...):
 *               the epilogue applies RoPE (hf:...llama.py:130-160), writes q to C (row stride ldc,
 *               natural head layout) and k, v straight into the cache at [tok_seq][head][tok_pos]
 *               (replaces sl_rope_kv_append + the qkv round trip). */
typedef struct {
  int32_t fuse_rms; float rms_eps;
  const float* rope_cos; const float* rope_sin;
  const int32_t* tok_pos; const int32_t* tok_seq;
  void* k_cache; void* v_cache;
  int32_t n_heads, n_kv_heads, max_ctx, reserved;   /* reserved: the caches' K/V format (SL_KV_MODEL_DTYPE / SL_KV_FP8_E4M3, see sl_kv_cache) */
  /* optional scratch for K-split partial sums (M > 16 rows against few weight rows cannot fill 256 CUs
   * otherwise): sl_gemm_split_workspace_bytes(M, N, K, dtype) bytes, or NULL to disable the split.
   * Its first 8192 bytes are arrival counters for the optional in-kernel reduce (SL_STREAM_FIXUP=1: above 384 rows the
   * block that finishes a tile last sums the partial records itself): zero them once when the buffer is created; every
   * call leaves them zero again, in stream order.  One buffer per call chain — two streams must not share it. */
  void* split_ws; size_t split_ws_bytes;
  /* RMSNorm statistics handed from one GEMM to the next (streaming path only):
   *   rstd_out — with the plain epilogue and a K-split, the reduce kernel also writes, per output row,
   *              rsqrt(mean(row^2) + rms_eps) of the values it stores (N <= 4096);
   *   rstd_in  — with fuse_rms, multiply by rstd_in[m] instead of recomputing the statistics of A's rows. */
  const float* rstd_in; float* rstd_out;
  /* with rstd_out: the reduce pass also writes the RMS-normalised rows themselves (hf:models/llama/modeling_llama.py:60-71:
   * weight * (x * rsqrt(mean(x^2) + eps)).to(dtype)) to norm_out (row stride N, the output's type), gain = norm_gain (N values) —
   * for a consumer that runs on the row-major tiled kernels and therefore wants its input normalised (decode steps above ~900 rows:
   * gate/up on the 256 x 256 tiles).  Both NULL: off. */
  void* norm_out; const void* norm_gain;
} sl_gemm_fused;
size_t sl_gemm_split_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t dtype);
/* K splits sl_gemm_fused_decode will use for this shape when split_ws is supplied (1: no reduce pass, so no rstd_out) */
int32_t sl_gemm_split_count(int32_t M, int32_t N, int32_t K, int32_t dtype);
int sl_gemm_fused_decode(const sl_gemm_args* a, const sl_gemm_fused* fx, sl_stream stream);

/* Backward-pass forms of sl_gemm (training; always the tiled MFMA kernel):
 *   trans_a: A is stored as (K, M) with row stride lda  — C = A^T-stored . W^T   (e.g. dW = dY^T X)
 *   trans_w: W is stored as (K, N) with row stride ldw  — C = A . W-stored       (e.g. dX = dY W)
 *            transposed operands are read in 16-byte chunks along the OUTPUT index: lda/ldw must be
 *            multiples of 8 (bf16) / 4 (f32) and each stored row readable up to that multiple.
 *            What the loader requires of lda / ldw: a chunk is loaded whole when its FIRST element lies inside
 *            the extent, so with M (N) no multiple of the chunk, each of the K stored rows is read up to the
 *            next multiple of 8 / 4 elements: M rounded up must fit in lda, or in the buffer behind the last
 *            row.  The elements read behind the extent land in tile rows that no epilogue stores, so their
 *            values never matter; rows K and beyond are never read.  A row stride below the extent
 *            (overlapping rows: the implicit-GEMM conv windows) is allowed for W.  The token-major kernel
 *            (both transposed, bf16, M and N multiples of 128) reads exactly M x K and N x K elements.
 *   aux_out: also store the pre-activation (after bias, before act) — what GELU's backward needs.
 *   residual_f32: with out_f32, the residual is float: C = residual + A.W^T accumulates fp32 gradients.
 *   groups / w_mod: see below. */
typedef struct {
  int32_t trans_a, trans_w, residual_f32, w_mod;
  void* aux_out;
  /* grouped (ragged) batch: device array of `batch` records {M, a_off, c_off, r_off} (int64, element offsets).
   * Batch z computes its own M rows from A + a_off into C + c_off (residual + r_off); W and bias are taken
   * at index z % w_mod (strideW / strideBias).  args->M is the LARGEST group (sizes the grid).  One launch
   * then covers e.g. a conv layer of every utterance of a ragged batch (hf:...hubert.py:141). */
  const int64_t* groups;
  /* groups_ext != 0: records are 8 int64 wide, {M, a_off, c_off, r_off, w_off, N, K, 0}: every group also has its own
   * weight offset, column count and reduction length (args->N / args->K are then the LARGEST ones).  One launch covers
   * e.g. one product of the attention backward over every (sequence, head) of a ragged batch.
   * groups_ext == 2: as 1, and the caller vouches that every group's K is a multiple of 64 bf16 / 32 f32 elements
   * (whole 128-byte slabs), which admits the LDS-DMA tiled kernel. */
  int32_t groups_ext, reserved;
  /* Fused row-wise top-1 in place of the store (greedy decode: lm_head + argmax, hf:generation/utils.py:2911-2925 over the logits
   * of ref:model/audio_llama.py:67): when both are set, C is NOT written; instead, for every row m and every group g of 64
   * output columns, amax_val[g * M + m] = max over columns [64 g, 64 g + 64) of (A.W^T + bias)[m][.] and amax_idx[g * M + m] =
   * its column (the lowest one on a tie; -inf / 0x7fffffff when every value is NaN).  ceil(N / 64) * M entries each.
   * Plain epilogue only (act NONE, no residual), one un-grouped row-major product, M > 64.  sl_greedy_select_partial finishes
   * the argmax over the groups: together they give bit for bit the token sl_gemm(out_f32) + sl_greedy_select give. */
  float* amax_val; int32_t* amax_idx;
  /* LayerNorm folded into the Linears around it (hf:models/hubert/modeling_hubert.py:515-517,612 stable-LN layer: x -> LN -> Linear;
   * bf16, plain row-major un-grouped products with N % 64 == 0, any row count (a product carrying these fields stays on the tiled
   * kernels even below 65 rows, so a short utterance alone gets the bits it gets inside a batch) — sl_gemm_ln_fold_ok()):
   *   producer side, stats_out: besides storing C, write for every row m and 64-column segment s the pair {sum, sum of squares} of
   *     the values AS STORED (after bias / act / residual, rounded to the output type) at stats_out[(m * (N / 64) + s) * 2];
   *     sl_layernorm_stats_finalize turns the N / 64 pairs of a row into {mean, rstd};
   *   consumer side, ln_mr / ln_u / ln_c: A holds the un-normalised rows x; W is the Linear's weight with the LayerNorm gain
   *     multiplied into its columns, ln_u[n] = sum_k W[n][k] (of the stored, rounded W), ln_c[n] = sum_k W0[n][k] beta[k] + bias[n];
   *     with {mean, rstd} = ln_mr[2 m], ln_mr[2 m + 1]:  out[m][n] = rstd * ((x W^T)[m][n] - mean * ln_u[n]) + ln_c[n], then act /
   *     residual as usual (bias must be NULL: it is inside ln_c).  Equals Linear(LayerNorm(x)) without the LayerNorm pass over x. */
  const float* ln_mr; const float* ln_u; const float* ln_c; float* stats_out;
  /* Stream-K workspace (optional).  Products whose 256 x 256 output tiles do not fill the chip evenly — the KD step's windows of a few
   * thousand rows (ref:trainer.py:270-384 at grad_accum_interval 16), its per-rank share under data parallelism, weight gradients of a
   * few dozen tiles under a long reduction — are cut along K as well: every CU takes an equal run of (tile, K slab) units, tiles
   * shared by two or three CUs are summed through this workspace inside the launch (fp32, fixed order: reproducible, not bit-equal
   * to the unsplit product).  The same workspace carries the PLAIN K runs of products of few tiles (S batched runs of whole slabs + a
   * fixed-order reduce launch; round 6: at most one 128 x 128 tile per CU runs on the ring form of the tile kernel, and a 256-tile
   * product that fills 50-66 % of one round is cut into three runs of uneven length).  Caller-owned, sl_gemm_streamk_workspace_bytes()
   * bytes (1 KiB of flags + 128 MiB of fp32 partial tiles), 16-byte aligned, ZEROED ONCE before its first
   * use and not shared by launches that may run concurrently (one per stream).  NULL, a shape the rule does not take, transposed /
   * grouped operands or the ln_* / stats_out / amax_* / aux_out forms: the product runs one block per tile as without it. */
  void* sk_ws; size_t sk_ws_bytes;
  /* Training-tape epilogue fusions (ABI 7; ref:trainer.py:270-384 runs these as separate torch ops around every Linear).  Plain
   * un-grouped row-major products on the tiled kernels only (no trans_*, groups, ln_*, stats_out, amax_*); all in the epilogue, with
   * the roundings of the unfused launch sequence reproduced (bf16: the value is rounded to the storage type where the unfused
   * sequence stored it), so fused and unfused tapes give the same bits.
   *   post_op = SL_POST_DROPOUT:  C = residual + dropout(act(A.W^T + bias))      (hf HubertEncoderLayerStableLayerNorm: h = h + dropout(sublayer))
   *             keep(i) as sl_dropout with seed drop_seed at element index i = row * drop_ld + col, kept values scaled by 1 / (1 - drop_p);
   *             aux_out (the pre-activation) is stored before act as usual.
   *   post_op = SL_POST_GELU_BWD: C = gelu'(post_in) * dropout(A.W^T)            (d pre = gelu'(pre) . d mid: sl_dropout + sl_gelu_bwd behind the
   *             data-gradient product; post_in = the saved pre-activation, (M, N) with row stride post_ld; drop_p = 0: no mask)
   *   post_op = SL_POST_SILU_MUL_BWD: C (M, 2 N) in the interleaved [16 gate | 16 up] layout = sl_silu_mul_bwd(post_in = gu (M, 2 N) with row
   *             stride post_ld, d mid = A.W^T); ldc is the row stride of the 2 N-wide output.
   *   colsum_out (any post_op incl. NONE): fp32 (N) += column sums of the values AS STORED in C (bias gradients: db = colsum(dY)),
   *             float atomics, a few dozen adders per column. */
  int32_t post_op, post_reserved;
  float drop_p; float post_reserved_f;
  uint64_t drop_seed;
  int64_t drop_ld;
  const void* post_in; int64_t post_ld;
  float* colsum_out;
  /* deferred_splits (host pointer, optional; plain un-grouped product with sk_ws, no bias / residual / post_op, output in the storage type): if the
   * product is cut into K runs (the few-tile rule of sk_ws), the reduce pass is NOT launched: *deferred_splits = S >= 2 and the S fp32 partial
   * products stay in sk_ws at byte offset 1024, S slabs of M x N floats (row stride N) — for a consumer that sums them itself while loading
   * (the norm-backward kernels of the training tapes: C = round(sum over runs, in run order) is what the reduce pass would have stored, and C is
   * NOT written).  Otherwise *deferred_splits = 0 and C is written as usual.  The partials live until the next product that uses sk_ws. */
  int32_t* deferred_splits;
} sl_gemm_ex_args;
enum { SL_POST_NONE = 0, SL_POST_DROPOUT = 1, SL_POST_GELU_BWD = 2, SL_POST_SILU_MUL_BWD = 3 };
int sl_gemm_ex(const sl_gemm_args* a, const sl_gemm_ex_args* ex, sl_stream stream);
size_t sl_gemm_streamk_workspace_bytes(void);
/* 1 when sl_gemm_ex takes ln_* / stats_out for a plain (M, N, K) product of this dtype, else 0 */
int32_t sl_gemm_ln_fold_ok(int32_t M, int32_t N, int32_t K, int32_t dtype);
/* The weight side of that fold for one Linear W (N, K) behind LayerNorm(gain, beta) (hf:models/hubert/modeling_hubert.py:515-517,612):
 * Wf = W with the gain multiplied into its columns, rounded to the storage type once; u[n] = sum_k Wf[n][k] (of the rounded values);
 * c[n] = sum_k W[n][k] beta[k] + bias[n] (bias may be NULL) — the ln_u / ln_c vectors and the weight a consumer GEMM takes. */
int sl_layernorm_fold_build(const void* W, const void* gain, const void* beta, const void* bias, void* Wf, float* u, float* c, int32_t N,
                            int32_t K, int32_t dtype, sl_stream stream);
/* {mean, rstd} per row from the per-segment {sum, sum of squares} a stats_out GEMM left ([rows][segs][2] floats, cols = 64 * segs
 * elements per row): mr[2 m] = mean, mr[2 m + 1] = rsqrt(max(E[x^2] - mean^2, 0) + eps); segments summed in order. */
int sl_layernorm_stats_finalize(const float* stats, int32_t segs, int64_t rows, int32_t cols, float eps, float* mr, sl_stream stream);
/* The same pair straight from the rows of x (rows, cols) — two-pass mean / variance, one wave per row — for a row set no GEMM
 * has just produced (the first layer's input). */
int sl_layernorm_stats(const void* x, int64_t rows, int32_t cols, float eps, float* mr, int32_t dtype, sl_stream stream);

/* LayerNorm over the last dim, optional fused GELU (conv layers: hf:...hubert.py:144-150;
 * encoder LNs hf:...hubert.py:515,517,612; feature projection :226).  In-place allowed. */
int sl_layernorm(const void* x, void* y, const void* gamma, const void* beta, int64_t rows, int32_t cols,
                 float eps, int32_t gelu, int32_t dtype, sl_stream stream);

/* LlamaRMSNorm (hf:models/llama/modeling_llama.py:62-67): y = w * (x * rsqrt(mean(x^2)+eps)). */
int sl_rmsnorm(const void* x, void* y, const void* w, int64_t rows, int32_t cols, float eps, int32_t dtype,
               sl_stream stream);

/* HuBERT conv layer 0: Conv1d(1 -> C, k, stride) + LayerNorm(C) + GELU fused, channel-last output
 * (hf:...hubert.py:141-150 for layer_id 0).  wave: (n_samples) float32 (always fp32 on input:
 * ref:inference.py:166);  w: (C, k) float32;  out: (L, C) dtype, L = (n_samples-k)/stride+1.
 * C must be 64*{1,2,4,8}. */
int sl_hubert_conv0(const float* wave, int64_t n_samples, const float* w, const float* bias,
                    const float* gamma, const float* beta, void* out, int32_t C, int32_t k, int32_t stride,
                    float eps, int32_t dtype, sl_stream stream);

/* Positional-conv input staging: x (T, H) -> xg (groups, T + k, H/groups), zero halo of k/2 rows
 * on both sides, so each group's conv window is one contiguous GEMM row (hf:...hubert.py:47-53). */
int sl_posconv_stage(const void* x, void* xg, int64_t T, int32_t H, int32_t groups, int32_t k,
                     int32_t dtype, sl_stream stream);

/* AvgPool1d(kernel, stride) over time on channel-last rows (ref:model/audio_encoder.py:59-63):
 * y[p] = mean(x[p*stride .. p*stride+kernel)).  Also serves ctc_pool via explicit ranges
 * (ref:model/audio_encoder.py:78-82): ranges = int32 (P,2) device array or NULL. */
int sl_avgpool_rows(const void* x, void* y, int64_t T, int32_t H, int32_t kernel, int32_t stride,
                    const int32_t* ranges, int64_t P, int32_t dtype, sl_stream stream);

/* Whole-ragged-batch forms of the three front-end / head stages (one launch for every utterance of a packed batch; the
 * encoder runtime and the KD tape use these: a single 10 s clip is only ~1 300 waves of conv0 work).
 *   sl_hubert_conv0_batch: utterance u has samples [sample_offsets[u], sample_offsets[u+1]) of `waves` and writes rows
 *     [row_offsets[u], row_offsets[u+1]) of out (both int64 device arrays of n_utt + 1 entries); max_L = longest output.
 *   sl_posconv_stage_batch: frames cu[u] .. cu[u] + klen[u] of x; utterance u's staged (groups, T_u + k, H/groups) block
 *     starts (cu[u] + u k) * H elements into xg.
 *   sl_avgpool_batch: rec = int64 (n_utt, 4) device records {pooled rows P_u, element offset of the utterance's rows in y, -, -};
 *     frames cu[u] .. of x (ref:model/audio_encoder.py:59-63). */
int sl_hubert_conv0_batch(const float* waves, const int64_t* sample_offsets_dev, const int64_t* row_offsets_dev, int32_t n_utt,
                          int64_t max_L, const float* w, const float* bias, const float* gamma, const float* beta, void* out, int32_t C,
                          int32_t k, int32_t stride, float eps, int32_t dtype, sl_stream stream);
int sl_posconv_stage_batch(const void* x, void* xg, const int32_t* cu, const int32_t* klen, int32_t n_utt, int64_t max_T, int32_t H,
                           int32_t groups, int32_t k, int32_t dtype, sl_stream stream);
int sl_avgpool_batch(const void* x, void* y, const int32_t* cu, const int32_t* klen, const int64_t* rec, int32_t n_utt, int64_t max_P,
                     int32_t H, int32_t kernel, int32_t stride, int32_t dtype, sl_stream stream);

/* The other two downsamples of the reference (ref:model/audio_encoder.py:65-85) on a packed ragged batch, one launch each, fp32 / bf16 / fp16,
 * fp32 accumulation, 16-byte accesses (H a multiple of 4 in fp32, 8 in 16 bits), no atomics, device tables only (additive to ABI 7).
 *   sl_segment_mean_batch (ctc_pool): ranges_dev = int64 (n_ranges, 2) records {first row, end row} in PACKED-row coordinates of x (n_rows, H);
 *     y[r] = mean of x[first_r .. end_r) (n_ranges, H).  The rows of one range are spread over eight row slices of a block and 32-chunk tiles of H.
 *   sl_stack_rows_batch (stack): desc_dev = n_utt int64 records {P_u, first frame row of the utterance in x, first stacked row in y, -}; stacked row p
 *     of y (sum P_u, factor * H) is frames factor p .. factor p + factor - 1 side by side; P_u = T_u / factor (T_u % factor == 0 keeps every frame,
 *     SURVEY.md section 9 Q5), P_u = 0 gives no rows; max_P sizes the grid (0: nothing to do).
 * Host side of ctc_pool (no device, no stream):
 *   sl_segment_ranges_host: utterance-relative (start, end) pairs as the dataset stores them (counts[u] of them for utterance u of frames[u] frames,
 *     concatenated) -> packed_out records.  Each pair is clamped to the utterance the way a tensor slice clamps it (a negative position counts from the
 *     end); a pair that is empty afterwards is SL_ERR_ARG, the message naming the utterance and the range (the reference would average nothing into a
 *     NaN row there).
 *   sl_segment_csr_host: the inverse index frame -> covering ranges of a packed table, in CSR form: row_ptr (n_rows + 1) is always written; cols (range
 *     numbers, those of frame t at row_ptr[t] .. row_ptr[t + 1], in table order) when cols is not NULL and cols_cap >= row_ptr[n_rows] (the sum of the
 *     lengths).  Ranges may overlap, repeat, be unsorted and leave gaps; one that is empty or leaves [0, n_rows) is SL_ERR_ARG. */
int sl_segment_mean_batch(const void* x, void* y, const int64_t* ranges_dev, int64_t n_ranges, int64_t n_rows, int32_t H, int32_t dtype,
                          sl_stream stream);
int sl_stack_rows_batch(const void* x, void* y, const int64_t* desc_dev, int32_t n_utt, int64_t max_P, int32_t H, int32_t factor, int32_t dtype,
                        sl_stream stream);
int sl_segment_ranges_host(const int64_t* ranges_rel, const int32_t* counts, const int64_t* frames, int32_t n_utt, int64_t* packed_out);
int sl_segment_csr_host(const int64_t* ranges, int64_t n_ranges, int64_t n_rows, int64_t* row_ptr, int32_t* cols, int64_t cols_cap);

/* Embedding row gather (hf:...llama.py:380-381; ref:utils.py:63-64). ids int32 on device. */
int sl_embed_gather(const void* table, const int32_t* ids, void* out, int64_t n, int32_t cols,
                    int32_t dtype, sl_stream stream);

/* Flash-style attention forward, variable-length packed sequences.
 *   head_dim 64, non-causal: HuBERT (hf:...hubert.py:234-259);  head_dim 128, causal GQA: Llama
 *   prefill (hf:...llama.py:191-213).  softmax in fp32, scores scaled by `scale`.
 *   q/out: token t of sequence s is row cu_q[s] + t;   k/v: row cu_k[s] + t.
 *   element address = base + row*row_stride + head*head_stride (strides in elements).
 *   Causal: key j visible to query i iff j <= i + (klen - qlen). */
typedef struct {
  const void* q; int64_t q_row_stride, q_head_stride;
  const void* k; int64_t k_row_stride, k_head_stride;
  const void* v; int64_t v_row_stride, v_head_stride;
  void* out; int64_t o_row_stride, o_head_stride;
  const int32_t* cu_q;   /* (nseq+1) device */
  const int32_t* cu_k;   /* (nseq)   device: first k/v row of each sequence */
  const int32_t* klen;   /* (nseq)   device: number of keys of each sequence */
  int32_t nseq, max_qlen, n_heads, n_kv_heads, head_dim, causal, dtype, reserved;
  float scale;
  /* training mode (hf HubertAttention: dropout on the attention probabilities): probability (0 = off) and the seed of
   * the counter-based mask of sl_dropout; the element index of probability (query row t of the packed batch, head h,
   * key j of its sequence) is ((t * n_heads + h) << 16) | j, so sequences are limited to 65 536 keys in this mode.
   * The softmax normaliser is the undropped sum. */
  float dropout_p;
  uint64_t dropout_seed;
  /* training: when non-NULL receives the log-sum-exp of every (query row, head) of the packed batch — float
   * [n_tok_q][n_heads], natural log of sum_j exp(scale * q.k_j) over the visible keys (undropped) — which sl_attn_bwd
   * recomputes the probabilities from. */
  float* lse;
} sl_attn_args;
int sl_attn_fwd(const sl_attn_args* a, sl_stream stream);
/* Causal head_dim 128 prefill attention of CONTINUED sequences (bf16 / fp16): the keys of sequence s come in two segments.
 *   keys [0, past_s)                 rows of its K/V cache slot: k_past / v_past are ONE layer's cache, (slots, n_kv, max_ctx, D), elements of
 *                                    a->dtype (kv_format = SL_KV_MODEL_DTYPE) or e4m3 bytes (SL_KV_FP8_E4M3), which are widened on the way
 *                                    into the LDS tiles by the exact conversion the decode kernels use; past_row0_dev[s] is the first cache
 *                                    row of the sequence's slot, slot * n_kv * max_ctx (the kv head adds head * max_ctx rows), and
 *                                    past_len_dev[s] = past_s in [0, max_ctx], not a multiple of anything.
 *   keys [past_s, past_s + klen_s)   a->k / a->v rows cu_k[s] + t, unquantised; a->klen holds the NEW key counts.
 * Causal shift as in sl_attn_fwd with klen = past_s + klen_s: key j visible to query i iff j <= i + past_s + klen_s - qlen_s.
 * Tiles, products and softmax are sl_attn_fwd's 16-bit kernel: with kv_format = SL_KV_MODEL_DTYPE the output is bit for bit what
 * sl_attn_fwd gives over a cache the new rows were appended to.  SL_F32, head_dim != 128, non-causal, dropout and lse are
 * SL_ERR_UNSUPPORTED; a format code other than 0 / 1 is SL_ERR_ARG; nothing is launched on either. */
int sl_attn_fwd_past(const sl_attn_args* a, const void* k_past, const void* v_past, const int32_t* past_len_dev, const int32_t* past_row0_dev,
                     int32_t max_ctx, int32_t kv_format, sl_stream stream);

/* Flash-style attention BACKWARD for the same packed layouts (the KD step's data gradients through the frozen Llama,
 * data + parameter gradients through the HuBERT / Whisper encoder; autograd of hf:...hubert.py:234-259 /
 * hf:...llama.py:191-213 in the reference, ref:trainer.py:373-374).  Given q, k, v, the forward output `out`, its
 * gradient `d_out` and the forward's `lse`, writes dq (q's layout: rows cu_q[s]+t), dk and dv (k / v's layout: rows
 * cu_k[s]+t, n_kv_heads heads — the query heads of a GQA group are summed inside the kernel).  The S x S probabilities are
 * recomputed per tile and never stored; no atomics (results are bitwise reproducible).  `delta` is a float
 * [n_tok_q][n_heads] workspace (rowsum(d_out * out), filled by the call).  dropout_p / dropout_seed must equal the forward's.
 * Strides in elements; dq rows / heads must start on 4-element boundaries. */
typedef struct {
  const void* q; int64_t q_row_stride, q_head_stride;
  const void* k; int64_t k_row_stride, k_head_stride;
  const void* v; int64_t v_row_stride, v_head_stride;
  const void* out; int64_t o_row_stride, o_head_stride;
  const void* d_out; int64_t do_row_stride, do_head_stride;
  void* dq; int64_t dq_row_stride, dq_head_stride;
  void* dk; int64_t dk_row_stride, dk_head_stride;
  void* dv; int64_t dv_row_stride, dv_head_stride;
  const float* lse;
  float* delta;
  const int32_t* cu_q;   /* (nseq+1) device */
  const int32_t* cu_k;   /* (nseq)   device */
  const int32_t* klen;   /* (nseq)   device */
  int64_t n_tok_q;       /* rows of q / out / d_out / dq (= cu_q[nseq]) */
  int32_t nseq, max_qlen, max_klen, n_heads, n_kv_heads, head_dim, causal, dtype;
  float scale;
  float dropout_p;
  uint64_t dropout_seed;
} sl_attn_bwd_args;
int sl_attn_bwd(const sl_attn_bwd_args* a, sl_stream stream);

/* Backward-side companion of sl_attn_args.dropout_p for the explicit-probability backward: for every score matrix
 * z = seq * n_kv + kv_head of a packed batch ((n_mat, smax, ld) buffers, dims[z] valid rows / columns, query head
 * kv_head * rep + r) writes p_dropped = keep * p / (1-p) and masks the fp32 d(probabilities) in place. */
int sl_attn_dropout_bwd(const void* p, void* p_dropped, float* d_p, int64_t n_mat, int32_t smax, const int32_t* dims, int32_t ld,
                        const int32_t* cu_q, int32_t n_heads, int32_t n_kv_heads, int32_t r, float dropout_p, uint64_t seed, int32_t dtype,
                        sl_stream stream);

/* RoPE (rotate_half form, hf:...llama.py:130-160) on the q and k slices of a fused QKV activation,
 * then KV-cache append (hf:cache_utils.py:127-145 restated as write-at-position).
 *   qkv: (n_tok, (n_heads + 2 n_kv) * D);  q is rotated in place;
 *   k,v -> cache (n_seq_slots, n_kv, max_ctx, D) at [tok_seq[t]][:, tok_pos[t]].
 *   cos/sin: (rope_len, D/2) float32 tables computed on the host exactly as HF does. */
int sl_rope_kv_append(void* qkv, void* k_cache, void* v_cache, const int32_t* tok_seq, const int32_t* tok_pos,
                      const float* cos, const float* sin, int64_t n_tok, int32_t n_heads, int32_t n_kv,
                      int32_t D, int32_t max_ctx, int32_t dtype, sl_stream stream);
/* K/V cache formats (sl_kv_cache.reserved, sl_gemm_fused.reserved, the kv_format argument of the *_ex entries):
 *   SL_KV_MODEL_DTYPE — rows of D elements in the model dtype;
 *   SL_KV_FP8_E4M3    — rows of D bytes, OCP e4m3fn, unscaled: a value is first rounded to the model dtype (what the 16-bit cache
 *                       would hold), clamped to +-448 and rounded to nearest even, so no byte is ever 0x7F / 0xFF (NaN) and
 *                       reading a byte back into bf16 / fp16 is exact.  Built for SL_BF16 / SL_F16 and head_dim 128: SL_F32 or
 *                       another head_dim is SL_ERR_UNSUPPORTED; any other format code is SL_ERR_ARG. */
#define SL_KV_MODEL_DTYPE 0
#define SL_KV_FP8_E4M3 1
/* sl_rope_kv_append with the cache format chosen by the caller.  kv_format = SL_KV_MODEL_DTYPE: exactly sl_rope_kv_append.
 * SL_KV_FP8_E4M3: k, v go to the cache as e4m3 bytes AND the rotated k rows are written back into qkv in place (as q is), so that
 * a prefill can attend the unquantised keys straight from qkv. */
int sl_rope_kv_append_ex(void* qkv, void* k_cache, void* v_cache, const int32_t* tok_seq, const int32_t* tok_pos,
                         const float* cos, const float* sin, int64_t n_tok, int32_t n_heads, int32_t n_kv,
                         int32_t D, int32_t max_ctx, int32_t dtype, int32_t kv_format, sl_stream stream);

/* One-token GQA attention against the KV cache (decode; hf:...llama.py:191-213 with q_len 1).
 *   q: row b of (B, n_heads*D) with row stride q_stride;  ctx_len[b] keys are attended (the
 *   current token must already be appended).  out: (B, n_heads*D).  K/V rows are read from
 *   cache (slots, n_kv, max_ctx, D). */
int sl_attn_decode(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out,
                   const int32_t* ctx_len, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D,
                   int32_t max_ctx, float scale, int32_t dtype, sl_stream stream);

/* Flash-decoding form of sl_attn_decode: the context is split into 64-key blocks (grid = n_kv x B x
 * ceil(max_ctx/64)) whose fp32 partial (O, max, sum) records are merged by a second kernel, so batch 1
 * fills the chip too.  workspace: sl_attn_decode_workspace_bytes(B, n_heads, n_kv, max_ctx). */
size_t sl_attn_decode_workspace_bytes(int32_t B, int32_t n_heads, int32_t n_kv, int32_t max_ctx);
int sl_attn_decode_split(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out,
                         void* workspace, const int32_t* ctx_len, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D,
                         int32_t max_ctx, float scale, int32_t dtype, sl_stream stream);
/* sl_attn_decode_split on a cache of either format.  shared_prefix = P: positions [0, P) are read from slot 0 for every sequence
 * (sl_kv_cache.shared_prefix; the single-pass form honours it in both formats, the split forms on e4m3 rows).  kv_format =
 * SL_KV_MODEL_DTYPE and P = 0: exactly sl_attn_decode_split. */
int sl_attn_decode_split_ex(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out,
                            void* workspace, const int32_t* ctx_len, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D,
                            int32_t max_ctx, float scale, int32_t dtype, int32_t kv_format, int32_t shared_prefix, sl_stream stream);

/* Grouped decode attention: rows that share a prompt (several sampled answers per prompt, sl_generate_n) read its K / V rows once.
 * Row b attends positions [0, prefix_len[b]) of its record's prefix_slot and [prefix_len[b], ctx_len[b]) of slot row_slot0 + b (both
 * slot indices into k_cache / v_cache; ctx_len[b] >= prefix_len[b], an empty tail is allowed).  A row with prefix_len 0 is in no record
 * and attends its own slot only.  Two launches: a prefix pass, one block per (record, kv head), whose 16-row matrix-core tile carries the
 * n_heads / n_kv query heads of up to floor(16 / (n_heads / n_kv)) sibling rows and which leaves an fp32 {O[128], max, sum} record per
 * (row, head) in the workspace; and a tail pass, one block per (row, kv head), that starts its online softmax from that record.  No
 * merge launch, no atomics.  The grid of the prefix pass is B records whatever the plan used (hipGraph-capturable: groups_dev is read
 * at run time); a record with n_rows = 0 exits at once.  Rows of a record need not be adjacent.
 * Built for SL_BF16 / SL_F16 (SL_F32: SL_ERR_UNSUPPORTED), D = 128, n_heads / n_kv in 1..4, both K / V formats.
 * sl_attn_group_plan_host is a pure host routine (no GPU): rows with the same (prefix_slot, prefix_len > 0) share records, in row
 * order, floor(16 / rep) rows per record; it always writes B records (the unused ones with n_rows = 0) and *n_used = the used count. */
typedef struct { int32_t prefix_slot, prefix_len, n_rows, reserved; int32_t rows[16]; } sl_attn_group;
int sl_attn_group_plan_host(const int32_t* prefix_slot, const int32_t* prefix_len, int32_t B, int32_t rep, sl_attn_group* out, int32_t* n_used);
size_t sl_attn_decode_grouped_workspace_bytes(int32_t B, int32_t n_heads);
int sl_attn_decode_grouped(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                           const int32_t* ctx_len, const int32_t* prefix_len, const sl_attn_group* groups_dev, int32_t B,
                           int32_t row_slot0, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale,
                           int32_t dtype, int32_t kv_format, sl_stream stream);

/* Greedy token selection (hf:generation/utils.py:2894,2925-2936): argmax over fp32 logits (lowest index
 * on ties), pad finished rows, EOS check, append to out_ids[b][gen_count[b]], advance gen_count and
 * ctx_len.  logits (B, V) float; eos_ids is a HOST array of at most 8 ids (passed by value to the
 * kernel).  Device state, all int32 (B): unfinished (1 until the row emits EOS), ctx_len, gen_count,
 * finish_len (gen_count at the row's EOS), next_ids (fed to the next embedding gather);
 * out_ids (B, max_new) int32. */
int sl_greedy_select(const float* logits, int32_t B, int32_t V, const int32_t* eos_ids_host, int32_t n_eos,
                     int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count,
                     int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, sl_stream stream);
/* sl_greedy_select over the per-group partial maxima of a fused lm_head (sl_gemm_ex_args.amax_val / amax_idx, n_groups =
 * ceil(V / 64), layout [group][B]): same token, same EOS / pad / finished-row bookkeeping, 1/64 of the bytes. */
int sl_greedy_select_partial(const float* amax_val, const int32_t* amax_idx, int32_t n_groups, int32_t B, const int32_t* eos_ids_host,
                             int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t advance_ctx, int32_t* unfinished, int32_t* ctx_len,
                             int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, sl_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Knowledge-distillation step (ref:trainer.py:270-374): backward and loss kernels.  GEMM-shaped
 * backward work (dgrad, wgrad, attention products) runs on sl_gemm_ex.
 * ------------------------------------------------------------------------------------------- */
/* dx = dy * gelu'(pre)  (pre = aux_out of the forward GEMM). */
int sl_gelu_bwd(const void* dy, const void* pre, void* dx, int64_t n, int32_t dtype, sl_stream stream);
/* y = a*x + b*y (gradient accumulation at residual joins). */
int sl_axpby(const void* x, void* y, float a, float b, int64_t n, int32_t dtype, sl_stream stream);

/* torch.optim.AdamW.step() for every trainable tensor of the encoder in ONE launch (ref:trainer.py:97-105 builds the optimizer,
 * :380-383 steps it; arithmetic of torch/optim/adamw.py _multi_tensor_adamw, amsgrad off, maximize off: decay, lerp of exp_avg,
 * exp_avg_sq, bias corrections formed in double on the host, addcdiv), and — where `dst` is set — the kernel-layout copy of the
 * updated weight in the compute dtype written in the same pass (what AudioEncoder.refresh_weights would otherwise re-derive).
 * tensors_dev: device array of n_tensors records; first_block_dev: device array of n_tensors int64, first_block[t] = sum over
 * u < t of sl_adamw_blocks(n_u); total_blocks = that sum over all tensors.  p / g / m / v are fp32, caller-owned; `step` is the
 * 1-based count of this update (state['step'] after the increment).  The hyper-parameters are doubles because torch forms
 * 1 - beta, the bias corrections and lr / bias_correction1 from python floats before rounding them to fp32 once (1 - 0.999 in
 * fp32 is off by 1.3e-5).  Launches on `stream`, never synchronises. */
typedef struct sl_adamw_tensor {
  float* p;            /* fp32 master weight, updated in place */
  const float* g;      /* fp32 gradient */
  float* m;            /* exp_avg */
  float* v;            /* exp_avg_sq */
  void* dst;           /* NULL, or where the compute-dtype copy of p goes (same element order) */
  int64_t n;           /* elements */
  int32_t dst_dtype;   /* SL_F32 / SL_BF16 (not SL_F16: training is fp32 / bf16) */
  int32_t reserved;
} sl_adamw_tensor;
size_t sl_adamw_blocks(int64_t n);
int sl_adamw_step(const sl_adamw_tensor* tensors_dev, const int64_t* first_block_dev, int32_t n_tensors, int64_t total_blocks, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int64_t step, sl_stream stream);

/* y (cols, ld_out) = x (rows, cols)^T with columns rows..ld_out-1 zero-filled (row strides ldx / ldy in elements): the
 * K-contiguous operand copies of the backward products (torch's autograd transposes implicitly inside its GEMM calls,
 * hf training under ref:trainer.py:374-378 loss.backward()). */
int sl_transpose_pad(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, int32_t ld_out, int32_t dtype,
                     sl_stream stream);

/* Training-mode dropout (hf:models/hubert/modeling_hubert.py feature-projection / hidden / activation dropouts of the
 * encoder the reference puts in train() mode, ref:trainer.py:258):  y = (residual ? residual : 0) + keep(i) * x / (1 - p).
 * keep(i) is a counter-based hash of (element index, seed) — no mask tensor; the backward pass calls the same entry
 * point on the gradient with the same seed.  n must be a multiple of 16 bytes' worth of elements; in place allowed. */
int sl_dropout(const void* x, const void* residual, void* y, int64_t n, float p, uint64_t seed, int32_t dtype, sl_stream stream);
/* SwiGLU on the 16-row interleaved gate/up activation gu (M, 2F): out (M, F) = silu(g)*u; backward
 * writes d gu in the same interleaved layout (hf:models/llama/modeling_llama.py:175). */
int sl_silu_mul(const void* gu, void* out, int64_t M, int32_t F, int32_t dtype, sl_stream stream);
int sl_silu_mul_bwd(const void* gu, const void* dy, void* dgu, int64_t M, int32_t F, int32_t dtype, sl_stream stream);
/* RoPE in place on the first n_rot heads of (n_tok, heads*D) rows; inverse != 0 applies the transposed
 * rotation (the backward of apply_rotary_pos_emb, hf:...llama.py:130-160). */
int sl_rope_inplace(void* x, const int32_t* tok_pos, const float* cos, const float* sin, int64_t n_tok, int32_t heads,
                    int32_t n_rot, int32_t D, int32_t inverse, int32_t dtype, sl_stream stream);
/* LayerNorm backward, optionally through a fused GELU (HuBERT conv layers): dx (may alias dy) and
 * fp32 dgamma/dbeta ACCUMULATED into the given buffers (may be NULL for input-only gradients). */
int sl_layernorm_bwd(const void* x, const void* gamma, const void* beta, const void* dy, void* dx, float* dgamma,
                     float* dbeta, int64_t rows, int32_t cols, float eps, int32_t gelu, int32_t dtype, sl_stream stream);
/* The same with a scratch buffer of sl_layernorm_bwd_ws_bytes(rows, cols) bytes: the blocks' column partials of dgamma / dbeta go to
 * per-block records summed by a second launch instead of colliding in atomics on 2 x cols addresses (7 984 x 1 024: 79 -> ~20 us).
 * A NULL / too small workspace, or rows wider than 1 024 elements, fall back to the form above. */
size_t sl_layernorm_bwd_ws_bytes(int64_t rows, int32_t cols);
int sl_layernorm_bwd_ws(const void* x, const void* gamma, const void* beta, const void* dy, void* dx, float* dgamma, float* dbeta,
                        int64_t rows, int32_t cols, float eps, int32_t gelu, int32_t dtype, void* workspace, size_t workspace_bytes,
                        sl_stream stream);
/* LlamaRMSNorm backward, data gradient only (the LLM is frozen, ref:trainer.py:63-64). */
int sl_rmsnorm_bwd(const void* x, const void* w, const void* dy, void* dx, int64_t rows, int32_t cols, float eps,
                   int32_t dtype, sl_stream stream);
/* Weight-norm backward of the positional conv (hf:models/hubert/modeling_hubert.py:50-68, weight_norm(dim = 2): W[h][j][t] =
 * g[t] v[h][j][t] / ||v[:, :, t]||; ref:trainer.py:373-384 steps on g and v).  dW_khg: the tape's gradient of the folded weight in
 * the kernel layout (H, k, Hg) fp32; v (H, Hg, k), g (k) fp32 masters; writes dg (k) and dv (H, Hg, k).  workspace:
 * sl_weight_norm_bwd_workspace_bytes(k) bytes.  Fixed summation order (reproducible). */
size_t sl_weight_norm_bwd_workspace_bytes(int32_t k);
int sl_weight_norm_bwd(const float* dW_khg, const float* v, const float* g, float* dg, float* dv, float* workspace, int32_t H, int32_t Hg,
                       int32_t k, sl_stream stream);
/* out[c] += sum_r x[r][c]  (bias gradients), fp32 accumulate. */
int sl_colsum(const void* x, int64_t ld, float* out, int64_t rows, int32_t cols, int32_t dtype, sl_stream stream);
/* Explicit softmax over rows of fp32 scores (n_mats matrices of rows x cols, row stride ld):
 * P = softmax(scale*S [+ causal mask: column j visible to row i iff j <= i + cols - rows]); columns
 * [cols, ld) of P are zeroed.  Backward: dS = scale * P * (dP - rowsum(dP*P)). */
int sl_softmax_rows(const float* S, void* P, int64_t n_mats, int32_t rows, int32_t cols, int64_t ld, float scale,
                    int32_t causal, int32_t dtype, sl_stream stream);
int sl_softmax_bwd(const void* P, const float* dP, void* dS, int64_t nrows, int32_t cols, int64_t ld, float scale,
                   int32_t dtype, sl_stream stream);
/* The same over n_mats square matrices of different sizes stored at a common pitch (rows_per_mat rows of ld elements
 * each): matrix i is mat_dim[i] x mat_dim[i]; rows / columns past it are left alone / written as zeros. */
int sl_softmax_rows_var(const float* S, void* P, int64_t n_mats, int32_t rows_per_mat, const int32_t* mat_dim, int64_t ld, float scale,
                        int32_t causal, int32_t dtype, sl_stream stream);
int sl_softmax_bwd_var(const void* P, const float* dP, void* dS, int64_t n_mats, int32_t rows_per_mat, const int32_t* mat_dim, int64_t ld,
                       float scale, int32_t dtype, sl_stream stream);
/* Losses over rows of fp32 logits; *loss += coef * sum_rows(...), d logits (+)= coef * grad (dtype T):
 *   ce:      lse(s) - s[label]                    (ref:model/audio_llama.py:72-101 with coef = w/(n-1))
 *   soft-ce: -sum softmax(t) * log_softmax(s)     (ref:utils.py:167-178 with coef = w/n)
 *   mse:     mean((a-b)^2)                        (ref:trainer.py:358-370)
 * sl_ce_loss: every labels[r] must be in [0, V) — the kernel reads logits[r][labels[r]] unconditionally.  Its one caller hands it the
 * response's own token ids (ref:model/audio_llama.py:84-98: labels exist for the response portion only, no ignore index reaches the
 * loss); rows without a next-token term belong to sl_kd_logit_losses, which skips labels < 0. */
int sl_ce_loss(const float* logits, const int32_t* labels, int64_t rows, int32_t V, float coef, float* loss, void* dlogits,
               int32_t accumulate, int32_t dtype, sl_stream stream);
int sl_soft_ce_loss(const float* student, const float* teacher, int64_t rows, int32_t V, float coef, float* loss,
                    void* dstudent, int32_t accumulate, int32_t dtype, sl_stream stream);
int sl_mse_loss(const void* a, const void* b, int64_t n, float coef, float* loss, void* da, int32_t accumulate,
                int32_t dtype, sl_stream stream);
/* The KD step's losses for a whole accumulation window in single launches (ref:trainer.py:325-370; what the per-utterance
 * forms above do one utterance and one term at a time):
 *   sl_kd_logit_losses: row r of the packed tail logits (student / teacher: float (rows, V)) carries
 *     labels[r] (int32, < 0: no next-token term), row_coef[r] = {ce loss, ce grad, soft-ce loss, soft-ce grad} weights and
 *     row_slot[r] = its utterance; losses (n_slots, loss_ld) float: [slot][0] += ce, [slot][1] += soft-ce;
 *     dstudent (rows, V) of `dtype` is OVERWRITTEN with the summed gradient.  teacher may be NULL (no soft-ce).
 *   sl_kd_mse_rows: feature-distillation MSE of one hidden-state tap: row_coef[r] = {loss weight on sum_h d^2, gradient
 *     weight on d}; losses[slot][loss_col] += ...; da (rows, H) overwritten with the gradient (may be NULL). */
int sl_kd_logit_losses(const float* student, const float* teacher, const int32_t* labels, const float* row_coef, const int32_t* row_slot,
                       int64_t rows, int32_t V, float* losses, int32_t loss_ld, void* dstudent, int32_t dtype, sl_stream stream);
int sl_kd_mse_rows(const void* a, const void* b, const float* row_coef, const int32_t* row_slot, int64_t rows, int32_t H, float* losses,
                   int32_t loss_ld, int32_t loss_col, void* da, int32_t dtype, sl_stream stream);
/* HuBERT front-end backward: AvgPool1d, strided-conv data gradient (col2im of the dgrad GEMM output),
 * fused conv0 (recomputes conv+LN, accumulates fp32 grads of w (C,k), bias, gamma, beta). */
int sl_avgpool_bwd(const void* dy, void* dx, int64_t T, int32_t H, int32_t kernel, int32_t stride, int64_t P, int32_t dtype,
                   sl_stream stream);
int sl_col2im(const void* dcol, void* dx, int64_t Lin, int64_t Lout, int32_t C, int32_t k, int32_t s, int32_t dtype,
              sl_stream stream);
/* The same two for every utterance of a packed (ragged) batch in ONE launch (ABI 7; ref:trainer.py:270-384 loops over utterances):
 * desc_dev = n_utt device records of four int64 {source rows (Lout / P), destination rows (Lin / T), first source row, first destination row}
 * into the packed source / destination buffers; max_Lin / max_T = the largest destination row count (sizes the grid). */
int sl_col2im_batch(const void* dcol, void* dx, const int64_t* desc_dev, int32_t n_utt, int64_t max_Lin, int32_t C, int32_t k, int32_t s,
                    int32_t dtype, sl_stream stream);
int sl_avgpool_bwd_batch(const void* dy, void* dx, const int64_t* desc_dev, int32_t n_utt, int64_t max_T, int32_t H, int32_t kernel,
                         int32_t stride, int32_t dtype, sl_stream stream);
/* Backward of the ctc_pool / stack downsamples (additive to ABI 7; fp32 / bf16 / fp16).  Every row of dx is written (the caller does no memset), nothing
 * is accumulated atomically: the result is a function of the tables alone.
 *   sl_segment_mean_bwd_batch: dx[t] = sum over the ranges r covering frame t of dy[r] / len_r, gathered through the CSR index of sl_segment_csr_host
 *     (row_ptr_dev int64 (n_rows + 1), cols_dev int32) in table order; frames nothing covers get zeros.
 *   sl_stack_rows_bwd_batch: desc_dev = n_utt int64 records {P_u, T_u, first stacked row in dy, first frame row in dx}; the T_u % factor cropped frames
 *     get zeros; max_T sizes the grid. */
int sl_segment_mean_bwd_batch(const void* dy, void* dx, const int64_t* ranges_dev, const int64_t* row_ptr_dev, const int32_t* cols_dev, int64_t n_ranges,
                              int64_t n_rows, int32_t H, int32_t dtype, sl_stream stream);
int sl_stack_rows_bwd_batch(const void* dy, void* dx, const int64_t* desc_dev, int32_t n_utt, int64_t max_T, int32_t H, int32_t factor, int32_t dtype,
                            sl_stream stream);
int sl_hubert_conv0_bwd(const float* wave, int64_t n_samples, const float* w, const float* bias, const float* gamma,
                        const float* beta, const void* dy, int32_t C, int32_t k, int32_t stride, float eps, float* dw,
                        float* dbias, float* dgamma, float* dbeta, int32_t dtype, sl_stream stream);

/* sl_hubert_conv0_bwd for a whole ragged batch in one launch: utterance u has samples [sample_offsets[u], sample_offsets[u+1])
 * of `waves`, rows [row_offsets[u], row_offsets[u+1]) of dy, and strips strip_prefix[u] .. strip_prefix[u+1]-1 of 24 time
 * steps (all three arrays on the device, n_utt + 1 entries).  A fixed grid walks the strips and flushes its sums once. */
int sl_hubert_conv0_bwd_batch(const float* waves, const int64_t* sample_offsets_dev, const int64_t* row_offsets_dev,
                              const int64_t* strip_prefix_dev, int32_t n_utt, int64_t total_strips, const float* w, const float* bias,
                              const float* gamma, const float* beta, const void* dy, int32_t C, int32_t k, int32_t stride, float eps,
                              float* dw, float* dbias, float* dgamma, float* dbeta, int32_t dtype, sl_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-model entry points (C++ host runtime inside the library: layer loops, workspace carving,
 * hipGraph capture of the decode step).  Weight tables are plain structs of device pointers.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const void *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
} sl_hubert_layer;

/* Optional per-layer copies for the inference path's LayerNorm fold (bf16; sl_gemm_ex_args.ln_*): the two LayerNorms of a stable-LN
 * layer (hf:models/hubert/modeling_hubert.py:515-517) disappear into the q|k|v and FFN1 Linears —
 *   wqkv_f = wqkv with ln1's gain multiplied into its columns, uqkv[n] = sum_k wqkv_f[n][k], cqkv[n] = (wqkv . ln1_b)[n] + bqkv[n];
 *   w1_f / u1 / c1 likewise from ln2, w1, b1.  The row statistics come out of the out_proj / FFN2 epilogues (stats_out). */
typedef struct {
  const void* wqkv_f; const float* uqkv; const float* cqkv;
  const void* w1_f; const float* u1; const float* c1;
} sl_hubert_fold;

typedef struct {
  int32_t dtype, n_conv, hidden, n_layers, n_heads, ffn, pos_k, pos_groups;
  int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
  float ln_eps;   /* encoder / feature-projection LayerNorm eps; conv LayerNorms use 1e-5 */
  int32_t pool_kernel, pool_stride, llm_dim, reserved;   /* reserved: 0 = HuBERT front end, 1 = Whisper (see sl_whisper_forward) */
  const float *conv0_w, *conv0_b, *conv0_g, *conv0_beta;       /* fp32: (C,k), (C), (C), (C) */
  const void *conv_w[8], *conv_b[8], *conv_g[8], *conv_beta[8]; /* i>=1: (C_out, k*C_in) tap-major */
  const void *fp_ln_g, *fp_ln_b, *fp_w, *fp_b;                  /* feature projection */
  const void *pos_w, *pos_b;          /* (groups, H/groups, k*H/groups) weight-norm folded; (H) */
  const sl_hubert_layer* layers;      /* host array, n_layers entries */
  const void *final_ln_g, *final_ln_b;
  const void *proj_w, *proj_b;        /* embed_projection (llm_dim, hidden) */
  const sl_hubert_fold* fold;         /* NULL, or host array of n_layers entries: LayerNorms folded into the Linears (bf16 inference) */
} sl_hubert_model;

/* AudioEncoder.forward with the `pool` downsample for a batch of utterances
 * (ref:model/audio_encoder.py:56-63,87).  Every utterance is encoded at its own length (no padding,
 * so results equal the reference's batch-size-1 behaviour): the conv feature extractor
 * and positional conv run per utterance, the 24 transformer layers run on all frames packed together
 * with variable-length attention.
 *   waves: device fp32, utterances concatenated; sample_offsets_host: (n_utt+1) host int64.
 *   out: rows of out_ld elements; utterance u's P_u rows go to row out_row_offsets_host[u] (so the
 *   encoder writes straight into the LLM prompt buffer, ref:utils.py:66-72), or packed if NULL.
 *   last_hidden: optional (sum T_u, hidden) packed encoder output before pooling. */
size_t sl_hubert_workspace_bytes(const sl_hubert_model* m, const int64_t* sample_offsets_host, int32_t n_utt);
int sl_hubert_num_frames(const sl_hubert_model* m, int64_t n_samples);
int sl_hubert_forward(const sl_hubert_model* m, const float* waves, const int64_t* sample_offsets_host, int32_t n_utt,
                      void* out, int64_t out_ld, const int64_t* out_row_offsets_host, void* last_hidden,
                      void* workspace, size_t workspace_bytes, sl_stream stream);

/* The same forward with the `stack` or `ctc_pool` downsample (ref:model/audio_encoder.py:65-85) between the final LayerNorm and the projection (additive
 * to ABI 7; sl_hubert_forward itself is unchanged and stays the `pool` entry).  The model's own proj_w / proj_b are not read: the projection comes with the
 * descriptor, since its input width depends on the method.
 *   stack: utterance u gives P_u = T_u / factor rows; the projection (llm_dim, factor * hidden) reads the frames in place (row stride factor * hidden),
 *     no copy is made.  ctc_pool: P_u = range_counts_host[u] rows, the means of its ranges (sl_segment_mean_batch), ranges_dev holding the packed-row
 *     records of all utterances in order (sl_segment_ranges_host); the projection is (llm_dim, hidden).
 *   Utterance u's P_u rows go to row out_row_offsets_host[u] of out (packed if NULL), as in sl_hubert_forward.
 * SL_ERR_ARG before any launch: a NULL descriptor / projection / table, a method other than these two, factor < 1, proj_in != factor * hidden (stack) or
 * != hidden (ctc_pool), range counts that do not add up to n_ranges. */
#define SL_DS_POOL 0
#define SL_DS_STACK 1
#define SL_DS_CTC_POOL 2
typedef struct {
  int32_t method;                      /* SL_DS_STACK or SL_DS_CTC_POOL */
  int32_t factor;                      /* downsample_factor (>= 1; ctc_pool does not read it further) */
  int32_t proj_in;                     /* input features of the projection */
  int32_t reserved;
  int64_t n_ranges;                    /* ctc_pool: records in ranges_dev */
  const int64_t* ranges_dev;           /* ctc_pool: (n_ranges, 2) {first row, end row} in packed frame rows */
  const int32_t* range_counts_host;    /* ctc_pool: n_utt counts, adding up to n_ranges */
  const void *proj_w, *proj_b;         /* embed_projection (llm_dim, proj_in), (llm_dim) */
} sl_downsample_desc;
size_t sl_hubert_workspace_bytes_ds(const sl_hubert_model* m, const int64_t* sample_offsets_host, int32_t n_utt, const sl_downsample_desc* ds);
int sl_hubert_forward_ds(const sl_hubert_model* m, const float* waves, const int64_t* sample_offsets_host, int32_t n_utt, void* out, int64_t out_ld,
                         const int64_t* out_row_offsets_host, void* last_hidden, const sl_downsample_desc* ds, void* workspace,
                         size_t workspace_bytes, sl_stream stream);

/* CTC word segmentation on the device: what lies between a CTC model's last hidden state and a table of ctc_pool ranges that sl_segment_mean_batch /
 * sl_hubert_forward_ds accept (ref:preprocess_data/utils.py:127-188 does this per utterance on the host).  Additive to ABI 7.
 *   sl_ctc_greedy_batch: ids[m] = the lowest column v that attains max_v (x[m] . w[v] + bias[v]); x (n_rows, H) packed frames, w (V, H), bias (V) or
 *     NULL, all in `dtype` (fp32 / bf16 / fp16); fp32 accumulation in a fixed order per row, the logits are never written, and ids[m] depends on row m
 *     alone.  1 <= V <= 64 and H a positive multiple of 8, otherwise SL_ERR_ARG before any launch.  n_rows = 0 does nothing.
 *   sl_ctc_pool_ranges_batch: ids (n_rows) packed, row_offsets_dev (n_utt + 1) int64 on the device, utterance u holding rows row_offsets[u] ..
 *     row_offsets[u + 1].  Words (HF's Wav2Vec2CTCTokenizer word offsets, group_tokens = True, skip_special_tokens = False): inside every maximal stretch
 *     of frames without delim_id, [first frame whose id is not blank_id, last such frame + 1); a stretch without such a frame has no word; every id other
 *     than blank_id / delim_id counts as a letter.  Ranges (ref:preprocess_data/utils.py:155-188), for the words (s_i, e_i) in order: (0, s_0); for
 *     every word the chunks (s_i + k pr, s_i + k pr + pr) while s_i + k pr < e_i, pr = pool_range; (e_i, s_i+1) between words; (e_last, e_last + 2 pr).
 *     SL_CTC_RANGES_RAW: exactly that list, utterance-relative, unclamped, empty pairs kept (what the reference stores).
 *     SL_CTC_RANGES_PACKED: each pair clamped to [0, T_u), pairs that are empty afterwards dropped, row_offsets[u] added: {first row, end row} records
 *       in packed frame rows, none of which leaves its utterance.
 *     An utterance without a word gives the one range (0, T_u) in both modes (the reference raises IndexError); with T_u = 0 packed mode gives none.
 *     ranges_out: int64 (ranges_cap, 2), the utterances' records contiguous and in utterance order; counts_out: n_utt int32 on the device.
 *     words_out / word_counts_out: both NULL, or the int64 (words_cap, 2) utterance-relative word table (same order) and its n_utt int32 counts.
 *     CAPACITY: an utterance of T frames gives at most T + 2 ranges and (T + 1) / 2 words, so ranges_cap >= sl_ctc_pool_ranges_capacity(n_rows, n_utt) =
 *     n_rows + 2 n_utt and words_cap >= sl_ctc_words_capacity(n_rows, n_utt) = (n_rows + n_utt) / 2 are required (less: SL_ERR_ARG) and never exceeded.
 *     Two launches (count, emit), integer arithmetic only, nothing crosses to the host.
 *   SL_ERR_ARG before any launch: NULL ids / offsets / range table / counts, a word table without word counts or the reverse, n_utt < 1,
 *   blank_id == delim_id, pool_range < 1, an unknown mode, a capacity below the bound. */
#define SL_CTC_RANGES_PACKED 0
#define SL_CTC_RANGES_RAW 1
int sl_ctc_greedy_batch(const void* x, const void* w, const void* bias, int32_t* ids, int64_t n_rows, int32_t H, int32_t V, int32_t dtype,
                        sl_stream stream);
size_t sl_ctc_pool_ranges_capacity(int64_t n_rows, int32_t n_utt);
size_t sl_ctc_words_capacity(int64_t n_rows, int32_t n_utt);
int sl_ctc_pool_ranges_batch(const int32_t* ids, const int64_t* row_offsets_dev, int32_t n_utt, int64_t n_rows, int32_t blank_id, int32_t delim_id,
                             int32_t pool_range, int32_t mode, int64_t* ranges_out, int64_t ranges_cap, int32_t* counts_out, int64_t* words_out,
                             int64_t words_cap, int32_t* word_counts_out, sl_stream stream);

/* Whisper path (BASELINE configs[3]; ref:model/audio_encoder.py:10-13, ref:trainer.py:168-199, 280-291).
 * sl_whisper_logmel: WhisperFeatureExtractor's torch path (hf:models/whisper/feature_extraction_whisper.py:135-168)
 *   for one utterance: zero-pad/trim to n_frames*hop samples, reflect pad, Hann STFT as an fp32 GEMM against
 *   dft_basis ((n_fft/2+1)*2 rows [cos | sin] x n_fft, window folded in), power, mel_w (n_mel x roundup4(n_fft/2+1),
 *   slaney), log10, max(x, max-8), (x+4)/4.  mel_out: (n_frames, n_mel) channel-last, dtype T.
 * sl_whisper_forward: WhisperEncoder (hf:models/whisper/modeling_whisper.py:592-646) + AvgPool + projection for
 *   n_utt mel inputs of exactly 2*max_source_positions frames each.  The model struct is sl_hubert_model with
 *   reserved = 1, conv_dim[0] = n_mel, conv_w/b[1] = conv1 and conv_w/b[2] = conv2 (tap-major (C_out, 3*C_in)),
 *   pos_w = embed_positions (pos_k = max_source_positions rows), layers' bqkv carrying zeros for the bias-less k_proj. */
size_t sl_whisper_logmel_workspace_bytes(int32_t n_fft, int32_t hop, int32_t n_frames, int32_t n_mel);
int sl_whisper_logmel(const float* audio, int64_t n_samples, const float* dft_basis, const float* mel_w, void* mel_out,
                      int32_t n_fft, int32_t hop, int32_t n_frames, int32_t n_mel, void* workspace, size_t workspace_bytes,
                      int32_t dtype, sl_stream stream);
size_t sl_whisper_workspace_bytes(const sl_hubert_model* m, int32_t n_utt);
int sl_whisper_forward(const sl_hubert_model* m, const void* mel, int32_t n_utt, void* out, int64_t out_ld,
                       const int64_t* out_row_offsets_host, void* last_hidden, void* workspace, size_t workspace_bytes,
                       sl_stream stream);

typedef struct {
  const void *norm1, *wqkv, *wo, *norm2, *wgu, *wdown;   /* row-major (prefill); wgu: 16-row gate/up interleave */
  /* decode copies, fragment-packed (sl_pack_weight); NULL -> decode falls back to the row-major set.
   * wqkv_dec rows: q/k heads in rotate_half pair order (see sl_gemm_fused); if dec_fused_norm the
   * RMSNorm gains are pre-multiplied into wqkv_dec / wgu_dec (and final_norm into lm_head_dec). */
  const void *wqkv_dec, *wo_dec, *wgu_dec, *wdown_dec;
} sl_llama_layer;

typedef struct {
  int32_t dtype, hidden, n_layers, n_heads, n_kv_heads, head_dim, ffn, vocab;
  float rms_eps; int32_t rope_len;
  const void *embed, *lm_head, *final_norm;
  const float *rope_cos, *rope_sin;      /* (rope_len, head_dim/2) */
  const sl_llama_layer* layers;          /* host array */
  const void* lm_head_dec;               /* packed (gain-folded if dec_fused_norm) or NULL */
  /* reserved: the format of the five *_dec weights (wqkv_dec / wo_dec / wgu_dec / wdown_dec of every layer, lm_head_dec).
   * SL_WDEC_E4M3: they are e4m3 weight images (sl_pack_weight_e4m3) of the same rows, in the same order and with the same gain fold,
   * as the 16-bit decode copies; dec_fused_norm must be 1.  The decode step then runs the skinny structure on
   * w_layout = SL_W_PACKED_E4M3 with the unfused lm_head + sl_greedy_select, for up to sl_w8_max_rows() rows: more rows, SL_F32 or a
   * reduction length that is no multiple of 64 are SL_ERR_UNSUPPORTED before any launch.  Prefill ignores the field.
   * SL_WDEC_MXFP4: the same with MXFP4 weight images (sl_pack_weight_mxfp4), w_layout = SL_W_PACKED_MXFP4, sl_w4_max_rows() and
   * reduction lengths that are multiples of 128.  2 and 3 are not formats.
   * SL_WDEC_MX_LINEAR (opt-in MX linears): the ROW-MAJOR pointers wqkv / wo / wgu / wdown of every layer are MX weight images
   * (sl_pack_weight_mx) of the same rows, and the four *_dec pointers of every layer must be NULL.  embed, lm_head, lm_head_dec,
   * final_norm and the layers' norms are what the 16-bit struct holds, and the lm_head part of every path runs as it does for that
   * struct.  The four products of every layer (qkv, o, gate/up + SiLU.mul, down) then run as sl_mxfp8_quantize_rows of the input
   * rows + sl_gemm_mx, at every row count: sl_llama_prefill, sl_llama_prefill_cont, sl_llama_decode_step and the sl_generate family
   * (sl_generate, _lp, _sc, _cont, sl_greedy_generate, sl_sample_generate).  Embedding, RMSNorm, RoPE, attention, the K/V cache
   * (both formats), lm_head, sampling, logits processors and scores stay as they are.  sl_llama_workspace_bytes and the
   * sl_generate_workspace_bytes family grow by the quantised-row buffer, n_tok * Kmax * (1 + 1/32) bytes + alignment,
   * Kmax = max(hidden, n_heads * head_dim, ffn), for this format only.  SL_F32, a reduction length that is no multiple of 128 and a
   * non-null *_dec pointer are refused before any launch; sl_beam_generate*, sl_generate_n with several answers and sl_llama_score
   * return SL_ERR_UNSUPPORTED for this format. */
  int32_t dec_fused_norm, reserved;
} sl_llama_model;
#define SL_WDEC_MODEL_DTYPE 0
#define SL_WDEC_E4M3        1
#define SL_WDEC_MXFP4       4
#define SL_WDEC_MX_LINEAR   5
/* The rules of weight format `code`, from the library's one table of them: the multiple every reduction length must be (1 for the model
 * dtype), the most decode rows the format runs (sl_w8_max_rows() / sl_w4_max_rows(); 0 = no limit) and the w_layout its *_dec images are
 * read with (-1: the format has no *_dec images).  Any out pointer may be NULL.  A code that is no format (2, 3, 6, negatives, ...) is
 * SL_ERR_ARG and the message lists the four formats. */
int sl_weight_format_info(int32_t code, int32_t* k_multiple, int32_t* max_rows, int32_t* w_layout);

typedef struct {
  void* k_cache; void* v_cache;  /* (n_layers, slots, n_kv, max_ctx, D) each: elements of the model dtype, or bytes (reserved = SL_KV_FP8_E4M3) */
  int32_t slots, max_ctx;
  /* shared_prefix = P > 0 is the caller's promise that the first P prompt positions of EVERY sequence of a generate call carry the
   * same input rows (one prompt template in front of the audio, ref:inference.py:95-113 builds it per call): prefill then leaves
   * bit-identical K/V rows at positions [0, P) of every slot, and the batched decode attention reads those positions from slot 0
   * (out of L2 instead of once per sequence from HBM).  0 = no promise.  P <= every prompt length (checked). */
  int32_t shared_prefix, reserved;       /* reserved: the K/V format, SL_KV_MODEL_DTYPE (0) or SL_KV_FP8_E4M3 (1) */
} sl_kv_cache;
/* bytes of ONE of the two caches (k_cache or v_cache) for `slots` x `max_ctx` positions in the given format; 0 on a bad argument */
size_t sl_kv_cache_bytes(const sl_llama_model* m, int32_t slots, int32_t max_ctx, int32_t kv_format);
/* The SL_KV_FP8_E4M3 quantiser on HOST memory (no GPU needed): out[i] = the byte the kernels store for the value x[i] (already
 * rounded to the model dtype by the caller).  The kernels and this entry run the same routine; it exists so that the format can be
 * checked exhaustively without a device. */
int sl_kv_quantize_e4m3_host(const float* x, uint8_t* out, int64_t n);

/* LlamaModel.forward over packed prompt embeddings + last-token logits
 * (hf:...llama.py:367-417 + ref:model/audio_llama.py:67 with logits for the last position only).
 *   x: (n_tok, hidden) packed prompts (overwritten: the residual stream runs in it, and its contents on return
 *   are unspecified — without hidden_taps the final layer computes its o / FFN part for each sequence's last row
 *   only, in the workspace);  cu_seqlens (nseq+1)
 *   host array.  Writes K/V for positions [0, len) of slot s, logits (nseq, vocab) fp32, and
 *   ctx_len[s] = len (device int32).  hidden_taps, if non-NULL, receives the (n_layers+1) hidden
 *   states (each (n_tok, hidden), last one post-norm) like output_hidden_states=True. */
size_t sl_llama_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq);
int sl_llama_prefill(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host,
                     int32_t nseq, float* logits, int32_t* ctx_len_dev, void* hidden_taps, void* workspace,
                     size_t workspace_bytes, sl_stream stream);

/* One KV-cached decode step for B sequences: embeds next_ids, runs all layers with M = B, writes
 * logits (B, vocab) fp32 (B <= SL_MAX_DECODE_BATCH).  The new token's K/V are appended at position ctx_len[b] and
 * ctx_len[b]+1 keys are attended; ctx_len itself is advanced by sl_greedy_select.  Reads/writes only
 * device state, so the call is hipGraph-capturable.  Workspace: sl_llama_workspace_bytes(m, B, B) + B*hidden. */
int sl_llama_decode_step(const sl_llama_model* m, const sl_kv_cache* kv, const int32_t* next_ids_dev,
                         const int32_t* ctx_len_dev, int32_t B, float* logits, void* workspace,
                         size_t workspace_bytes, sl_stream stream);

/* GenerationMixin._sample in greedy mode from prompt embeddings (ref:inference.py:60-66):
 * prefill + up to max_new_tokens decode steps replayed from one captured hipGraph.  out_ids_host
 * (nseq, max_new_tokens) int32 receives new tokens only; *n_steps_host the number of columns
 * produced (all rows finished => early stop, checked every `check_every` steps).  This call
 * synchronises `stream` (it returns host data).
 * LIMIT: nseq <= SL_MAX_DECODE_BATCH (2048) sequences per call — the row count the decode GEMMs, the single-pass attention grid and
 * the 288 GB of HBM are sized for (a KV cache of 2 048 slots x 393 positions of Llama-3.2-3B is 92 GB); a larger batch is rejected with
 * SL_ERR_ARG (split it: sequences are independent — the Python surface does, inference.generate_audio_responses).
 * The captured decode graph is cached per calling thread, keyed by every buffer, limit, the device and a hash of the model's
 * and every layer's fields; sl_decode_graph_cache_clear() destroys the calling thread's cached graphs (returns how many) —
 * call it after re-laying-out weights in place behind unchanged struct contents, or before unloading the library. */
#define SL_MAX_DECODE_BATCH 2048
int sl_decode_graph_cache_clear(void);
size_t sl_generate_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens);
int sl_greedy_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host,
                       int32_t nseq, int32_t max_new_tokens, const int32_t* eos_ids_host, int32_t n_eos,
                       int32_t pad_id, int32_t use_eos, int32_t check_every, int32_t* out_ids_host,
                       int32_t* n_steps_host, float* timings_ms_host /* [prefill, decode] or NULL */,
                       void* workspace, size_t workspace_bytes, sl_stream stream);

/* sl_generate (ABI version 6): the general form of the two calls around it — same prefill, same captured decode step, same HF
 * semantics (hf:generation/utils.py:2928-2942: a finished row emits pad_id, generation ends at the step where the last row
 * finished) — plus what a batch whose answers have different lengths needs:
 *   row_limits_host : NULL, or one token budget per sequence in [1, max_new_tokens] (a per-request max_new_tokens): a row that
 *                     has produced its budget is finished exactly like a row that emitted EOS.  Implies use_eos semantics.
 *   compact         : 1 = at a `check_every` synchronisation, once the live rows fit the next lower rung of a fixed ladder of
 *                     row counts (multiples of 64 from 128 up; 96, 64, 48, 32, 24, 16, 12, 8, 6, 4, 3, 2, 1 below), the batch is COMPACTED: finished
 *                     sequences are written out, the live rows above the rung take the places of finished rows below it — their
 *                     state, output ids and K / V cache slot move with them — and decoding continues with that many rows (one
 *                     cached graph per rung).  Per sequence the result is what compact = 0 gives: identical ids in SL_F32 (every
 *                     kernel family is bit-exact there); in SL_BF16 the row count selects the GEMM family, so a logit near-tie
 *                     may resolve differently after a compaction, as it may between two batch sizes.  The K / V cache is
 *                     re-ordered in place: after the call slot j no longer belongs to sequence j.
 *   sample          : 0 = greedy argmax; 1 = temperature / top_k / top_p / seed as in sl_sample_generate (the draw of a
 *                     sequence depends on (seed, the sequence's index in THIS call, step) only, compacted or not).
 * out_ids_host (nseq, max_new_tokens) is indexed by the caller's sequence order whatever moved.  stats may be NULL. */
typedef struct {
  const int32_t* eos_ids_host;     /* n_eos ids (<= 8) */
  const int32_t* row_limits_host;  /* NULL or nseq budgets */
  uint64_t seed;
  int32_t max_new_tokens;
  int32_t n_eos;
  int32_t pad_id;
  int32_t use_eos;
  int32_t check_every;             /* host check of the finished flags every this many steps (<= 0: 16) */
  int32_t sample;
  float temperature;
  int32_t top_k;
  float top_p;
  int32_t compact;
} sl_generate_opts;
typedef struct {
  int64_t row_steps;        /* sum over decode launches of the rows the launch ran (nseq x launches without compaction) */
  int32_t n_steps;          /* columns of out_ids_host produced */
  int32_t decode_launches;
  int32_t compactions;
  int32_t final_rows;       /* rows of the last decode launch */
  float prefill_ms;
  float decode_ms;
} sl_generate_stats;
int sl_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace,
                size_t workspace_bytes, sl_stream stream);

/* Sampled generation (hf:generation/utils.py:2911-2923 with do_sample = True — what the hub's generation_config.json of
 * Llama-3.2-3B-Instruct asks for when a caller does not force greedy): HF's logits warpers in HF's order —
 * temperature (scores / T), top-k (keep scores >= the k-th largest; 0 = off; HF's default is 50), top-p over the
 * top-k-filtered distribution (drop a token iff the mass ranked above it is >= top_p; 1.0 = off) — then one draw per row from
 * the renormalised survivors by inverse CDF in index order at u = hash(seed, row, step): reproducible for a given seed (HF's
 * own stream is torch.multinomial on the global CUDA generator, which no other implementation can reproduce).
 * sl_sample_select is sl_greedy_select with the draw in place of the argmax (choice_ws: B int32 scratch);
 * sl_sample_generate is sl_greedy_generate with it (same workspace size, same synchronisation points). */
int sl_sample_select(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                     const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len,
                     int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, int32_t* choice_ws,
                     sl_stream stream);
int sl_sample_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                       int32_t max_new_tokens, const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos,
                       int32_t check_every, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t* out_ids_host,
                       int32_t* n_steps_host, float* timings_ms_host, void* workspace, size_t workspace_bytes, sl_stream stream);

/* Beam search (hf:generation/utils.py _beam_search with do_sample = False, prompts given as embeddings: decoder_prompt_len = 0,
 * max_length = max_new_tokens; additive to ABI 7).  K = num_beams, E = the EOS ids in use, M = max(2, 1 + E) * K candidates per step.
 * Per sequence: K running beams (token histories + scores, initialised to [0, -1e9, ...]), a finished set of K hypotheses (scores
 * initialised to -1e9, flags, lengths) and `open` (HF's is_early_stop_heuristic_unsatisfied).  Step t (0-based):
 *   1. acc[j][v] = log_softmax(logits of beam j)[v] + running_score[j]            (only beam 0 exists at t = 0)
 *   2. candidates = the M largest acc over (j, v): larger value first, then lower flat index j * V + v
 *   3. hit[c] = candidate c's token is an EOS id, or t + 1 == max_new_tokens
 *   4. next running beams = the first K, in candidate order, of score + (hit ? -1e9 : 0); their source beams re-order the K/V cache
 *   5. finished set = top-K of [old K | M candidates], concatenation order on ties; a candidate's score is score / (t+1)^length_penalty,
 *      with -1e9 added once for each of: all K flags set and early_stopping == 1; !open; c >= K or !hit[c]
 *   6. open &= running_score[0] / L^length_penalty > worst;  L = max_new_tokens if early_stopping == 2 and length_penalty > 0, else t + 1;
 *      worst = min(finished scores) if all K flags are set, else -1e9
 *   7. the sequence is done when !open, or early_stopping == 1 and all K flags are set, or t + 1 == max_new_tokens.
 * All score arithmetic is fp32; (t+1)^length_penalty is formed in double on the host and rounded once (sl_beam_state.len_pen).
 * Decode rows: row s * K + j is beam j of sequence s and owns cache slot s * K + j, during and after the call.  Each prompt is
 * prefilled ONCE (into slot s * K) and its K/V rows are copied to the K - 1 sibling slots.  There is no compaction: a done sequence
 * keeps its rows, its finished set frozen by the rules above, until every sequence is done (checked every `check_every` steps).
 * LIMITS (SL_ERR_ARG / SL_ERR_UNSUPPORTED before any launch): 1 <= num_beams <= 8; M <= 64 and M <= vocab; nseq * num_beams <=
 * SL_MAX_DECODE_BATCH and <= kv->slots; 1 <= num_return_sequences <= num_beams; length_penalty finite; prompt + max_new_tokens <= max_ctx;
 * e4m3 decode weights up to sl_w8_max_rows() rows, counted as nseq * num_beams. */
typedef struct {
  const int32_t* eos_ids_host;     /* n_eos ids (<= 8) */
  int32_t n_eos, pad_id, use_eos, max_new_tokens, check_every;
  int32_t num_beams, num_return_sequences;
  int32_t early_stopping;          /* 0 = False, 1 = True, 2 = "never" */
  float length_penalty;
} sl_beam_opts;
/* Device state of sl_beam_step; R = nseq * num_beams rows, all arrays caller-owned.  Initial values: run_score [0, -1e9, ...] per
 * sequence, fin_score -1e9, fin_flag / fin_len / seq_done / step 0, open 1, ctx_len = the prompt lengths; fin_score must stay
 * sorted (descending) per sequence, as the kernel leaves it. */
typedef struct {
  float* run_score;       /* (R) */
  int32_t* next_ids;      /* (R) token each row feeds to the next decode step */
  int32_t* src_row;       /* (R) global row index of the beam a row continues (the cache re-ordering of the step) */
  int32_t* ctx_len;       /* (R) advanced by one per step, except by the first */
  int32_t* hist[2];       /* two (R, max_new_tokens) token histories: step t reads hist[t & 1] and writes hist[(t + 1) & 1] */
  float* fin_score;       /* (R) */
  int32_t* fin_ids;       /* (R, max_new_tokens) */
  int32_t* fin_flag;      /* (R) */
  int32_t* fin_len;       /* (R) */
  int32_t* open;          /* (nseq) */
  int32_t* seq_done;      /* (nseq) */
  int32_t* step;          /* (nseq) t of the next step; advanced by the kernel (a step with t >= max_new_tokens does nothing) */
  const float* len_pen;   /* (max_new_tokens) len_pen[t] = (float)pow((double)(t + 1), length_penalty) */
} sl_beam_state;
size_t sl_beam_generate_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq, const sl_kv_cache* kv, const sl_beam_opts* opts);
/* out_ids_host (nseq, R, max_new_tokens): hypothesis r of sequence s, pad_id past its length (an EOS that ended it is included);
 * out_scores_host / out_lens_host (nseq, R).  stats (may be NULL): n_steps = steps run, decode_launches = replays of the captured
 * step (decode on nseq * K rows -> top-M per row -> beam step -> cache gather -> scatter), cached per thread like sl_generate's. */
int sl_beam_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                     const sl_beam_opts* opts, int32_t* out_ids_host, float* out_scores_host, int32_t* out_lens_host,
                     sl_generate_stats* stats, void* workspace, size_t workspace_bytes, sl_stream stream);
/* Kernel-level entries (the tests, callers with their own loop).
 * sl_beam_topk: per row of fp32 logits (rows, V) the M (<= 64, <= V) largest log_softmax(row) + row_score[row] (row_score NULL: 0) with
 *   their tokens, in the order of step 2; NaN logits count as -inf.  cand_score / cand_token: (rows, M).
 * sl_beam_step: steps 2-7 for nseq sequences from the rows' lists.  first != 0: step 0 — sequence s has ONE list, at list row s
 *   (the prefill logits), and ctx_len is not advanced; otherwise list row s * K + j belongs to beam j.
 * sl_kv_beam_reorder: for every row with src_row[row] != row, positions [prompt_len[row], ctx_len[row]) (at most max_span of them) of
 *   slot src_row[row] replace those of slot row in every layer and KV head, in two launches through `staging`
 *   (sl_kv_beam_staging_bytes = 2 * rows * n_layers * n_kv_heads * max_span * bytes of one K row).  Either K/V format. */
int sl_beam_topk(const float* logits, int32_t rows, int32_t V, const float* row_score, int32_t M, float* cand_score, int32_t* cand_token,
                 sl_stream stream);
int sl_beam_step(const sl_beam_state* state, const float* cand_score, const int32_t* cand_token, int32_t nseq, int32_t num_beams, int32_t M,
                 int32_t first, const sl_beam_opts* opts, sl_stream stream);
size_t sl_kv_beam_staging_bytes(const sl_kv_cache* kv, const sl_llama_model* m, int32_t rows, int32_t max_span);
int sl_kv_beam_reorder(const sl_kv_cache* kv, const sl_llama_model* m, const int32_t* src_row_dev, const int32_t* prompt_len_dev,
                       const int32_t* ctx_len_dev, int32_t rows, int32_t max_span, void* staging, size_t staging_bytes, sl_stream stream);

/* Logits processors (hf:generation/utils.py _get_logits_processor; classes in hf:generation/logits_process.py; additive to ABI 7): what a
 * caller of HF's generate reaches for when an answer loops — repetition_penalty, no_repeat_ngram_size — and min_new_tokens, in HF's order,
 * on the fp32 logits of every step, the prefill's included, before the argmax / the sampling warpers / the beam selection.
 * A row's history is the tokens it has GENERATED: the prompt is embeddings (the reference's input_ids start empty) and is never penalised.
 *   repetition_penalty p   every token of the history: s < 0 ? s * p : s / p, once however often it occurs (IEEE fp32 division)
 *   no_repeat_ngram_size g with n >= g history tokens: every token that followed an occurrence of the last g - 1 tokens is set to -inf
 *                          (g = 1: every generated token); runs after the penalty, so a ban overrides it
 *   min_new_tokens         while n < min_new_tokens the EOS ids in use are set to -inf (nothing without EOS ids)
 * LIMITS (SL_ERR_ARG before any launch): repetition_penalty finite and > 0; no_repeat_ngram_size >= 0; 0 <= min_new_tokens <=
 * max_new_tokens; at most 8 EOS ids.
 * COST: with any processor on, every step is lm_head -> fp32 logits -> sl_logits_process -> select: above 64 rows a greedy step gives up
 * the lm_head's fused per-64-column top-1 and pays the logits round trip (2 x rows x vocab x 4 bytes, about 1 GB at 1 024 rows of
 * Llama-3.2-3B).  With lp NULL or all three off, sl_generate_lp / sl_beam_generate_lp ARE sl_generate / sl_beam_generate: the same
 * launches, captured graphs and bits, and the workspace sizes are the same. */
typedef struct {
  float repetition_penalty;      /* 1.0 = off; must be finite and > 0 */
  int32_t no_repeat_ngram_size;  /* 0 = off */
  int32_t min_new_tokens;        /* 0 = off; <= max_new_tokens */
  int32_t reserved;
} sl_logits_opts;
/* In place on logits (rows, V), one block per row.  hist (rows, hist_ld) int32 with hist_len[row] valid entries (clamped to [0, hist_ld];
 * ids outside [0, V) are ignored); unfinished NULL or (rows): a row with 0 is left untouched (the select kernels emit pad_id for it).
 * log_softmax != 0: the row is first rewritten as (x - max) - log(sum exp(x - max)), NaN counted as -inf — bit for bit what sl_beam_topk
 * forms — and sl_beam_topk_ex(is_logprob = 1) then selects from it.  scratch: rows * hist_ld floats, read and written only when
 * repetition_penalty != 1 (may be NULL otherwise).  Deterministic: no float atomics. */
int sl_logits_process(float* logits, int32_t rows, int32_t V, const int32_t* hist, int64_t hist_ld, const int32_t* hist_len,
                      const int32_t* unfinished, const sl_logits_opts* lp, const int32_t* eos_ids_host, int32_t n_eos, int32_t log_softmax,
                      float* scratch, sl_stream stream);
/* sl_beam_topk; with is_logprob != 0 the max / log-sum-exp passes are skipped: acc = x + row_score */
int sl_beam_topk_ex(const float* logits, int32_t rows, int32_t V, const float* row_score, int32_t M, float* cand_score, int32_t* cand_token,
                    sl_stream stream, int32_t is_logprob);
/* sl_generate / sl_beam_generate with the processors (lp may be NULL).  History: the row's output ids (greedy, sampling: it moves with the
 * row when the batch is compacted) / the running beam's tokens.  The workspace grows by the penalty's scratch only when it is on. */
size_t sl_generate_workspace_bytes_lp(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp);
int sl_generate_lp(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                   const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                   sl_stream stream, const sl_logits_opts* lp);
size_t sl_beam_generate_workspace_bytes_lp(const sl_llama_model* m, int64_t n_tok, int32_t nseq, const sl_kv_cache* kv, const sl_beam_opts* opts,
                                           const sl_logits_opts* lp);
int sl_beam_generate_lp(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                        const sl_beam_opts* opts, int32_t* out_ids_host, float* out_scores_host, int32_t* out_lens_host,
                        sl_generate_stats* stats, void* workspace, size_t workspace_bytes, sl_stream stream, const sl_logits_opts* lp);

/* ---------------------------------------------------------------------------------------------
 * Token log-probabilities (HF generate(output_scores=True) + compute_transition_scores(normalize_logits=True)); additive to ABI 7.
 * For row b and step t, with y the chosen token and s the fp32 score row the selection saw (after the logits processors, and after the
 * temperature / top-k / top-p warpers when sampling: filtered tokens at -inf):  logprob[b][t] = log_softmax(s)[y].
 * NaN counts as -inf, the arithmetic is fp32 in one fixed order (no float atomics); positions at or after a row's finish (pad tokens)
 * hold 0.0f; a row whose scores have no finite maximum yields a non-finite value.
 *
 * sl_gemm_top1_lse: sl_gemm_ex with amax_val / amax_idx set (same argument checks, same two planes bit for bit) plus a third plane
 * amax_sum[g * M + m] = sum over the valid columns of group g of expf(v - amax_val[g * M + m]), v the value the top-1 compared; 0 for a
 * group whose maximum is -inf.  sl_greedy_select_partial_sc turns the three planes into the token and -log(sum_g amax_sum[g] *
 * expf(amax_val[g] - row max)) (the chosen token is the maximum); sl_greedy_select_sc forms (best - m) - log(sum exp(x - m)) over the
 * fp32 row, through the row reduce sl_beam_topk and sl_logits_process use; sl_sample_select_sc writes log(p_chosen / mass of the
 * survivors), the p and the mass of its own draw.  logprob_out: (B, max_new) floats on the device, written at [b][gen_count[b]];
 * token and bookkeeping are bit for bit those of the entries without _sc.
 *
 * sl_generate_sc: sl_generate_lp (lp may be NULL) + out_logprobs_host (nseq, max_new_tokens) floats; with out_logprobs_host NULL /
 * scores 0 they ARE sl_generate_lp / sl_generate_workspace_bytes_lp: same launches, captured graphs, workspace layout and bits.
 * The device buffer is carved behind every other piece of generation state and moves with its row when the batch is compacted.
 * Above 64 rows a greedy step keeps the lm_head's fused top-1: the third plane sits behind the other two in the idle logits buffer. */
int sl_gemm_top1_lse(const sl_gemm_args* args, const sl_gemm_ex_args* ex, float* amax_sum, sl_stream stream);
int sl_greedy_select_sc(const float* logits, int32_t B, int32_t V, const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos,
                        int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids,
                        int32_t max_new, float* logprob_out, sl_stream stream);
int sl_greedy_select_partial_sc(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t B,
                                const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t advance_ctx,
                                int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count, int32_t* finish_len, int32_t* next_ids,
                                int32_t* out_ids, int32_t max_new, float* logprob_out, sl_stream stream);
int sl_sample_select_sc(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                        const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len,
                        int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, int32_t* choice_ws,
                        float* logprob_out, sl_stream stream);
size_t sl_generate_workspace_bytes_sc(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp,
                                      int32_t scores);
int sl_generate_sc(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                   const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                   sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host);

/* sl_generate_n: sl_generate_sc with N = num_return_sequences sampled answers per prompt (HF's do_sample = True,
 * num_return_sequences = N).  N = 1 IS sl_generate_sc: same launches, captured graphs, workspace layout and bits.  N > 1 needs
 * opts->sample = 1 (HF refuses greedy with several return sequences too), nseq * N <= SL_MAX_DECODE_BATCH decode rows and
 * kv->slots >= nseq * (N + 1): the nseq prompts are prefilled ONCE into slots [0, nseq), which are never written again, and row
 * s * N + j (answer j of prompt s) appends its own tokens to slot nseq + s * N + j.  out_ids_host / out_logprobs_host are
 * (nseq * N, max_new_tokens), prompt-major; row_limits_host, when given, has nseq * N entries.  The draw of answer j of prompt s is
 * that of sequence index s * N + j of an sl_generate_sc call in which every prompt is repeated N times, compacted or not.
 * Decode attention: where the grouped kernels are built and the switch SL_GEN_GROUP_ATTN allows it (0 = never, 1 = wherever built,
 * -1 = default rule), a row reads its prompt from the prompt slot through sl_attn_decode_grouped and its row slot holds positions
 * >= the prompt length only; otherwise the prompt's K / V rows are copied to the N row slots once and the attention of sl_generate_sc
 * runs on them.  sl_generate_last_attn_path(): what the calling thread's last sl_generate_n call ran — 0 = N was 1, 1 = the copy,
 * 2 = the grouped kernels. */
size_t sl_generate_workspace_bytes_n(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp,
                                     int32_t scores, int32_t num_return_sequences);
int sl_generate_n(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                  const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                  sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host, int32_t num_return_sequences);
int32_t sl_generate_last_attn_path(void);

/* Multi-turn sessions: generation that CONTINUES on a K/V cache the caller keeps between calls.
 *
 * sl_llama_prefill_cont: sl_llama_prefill for sequences that already hold a past.  Sequence s lives in cache slot slot_host[s]
 * (slot_host NULL: slot s); positions [0, past_len_host[s]) of that slot hold its K/V.  The new rows are rotated at positions
 * past_s + t and appended there, attend [0, past_s + len_s), the last row's logits are written and ctx_len[s] = past_s + len_s.
 * Checked before any launch: past_s >= 0, past_s + len_s <= max_ctx (<= rope_len), slots distinct and < kv->slots, and, when any
 * past is > 0, kv->shared_prefix <= every past: the new rows are never deduplicated, the promise then only says that cache
 * positions [0, shared_prefix) of every slot are equal, which the first call made true.  past_len_host NULL or all zero with
 * slot_host NULL IS sl_llama_prefill, bit for bit and launch for launch.  hidden_taps are not offered.
 * 16-bit / fp32 cache: the rows are appended first and sl_attn_fwd attends the cache (klen = past + len).  e4m3 cache: the past
 * keys exist only as bytes, so sl_attn_fwd_past attends the dequantised past and the unquantised new rows — a continued e4m3
 * prefill is therefore NOT bit-equal to a one-shot prefill of the same text, which attends every key unquantised.
 *
 * sl_generate_cont / sl_generate_workspace_bytes_cont: sl_generate_sc (greedy / sampling, row_limits, logits processors,
 * optional log-probabilities) + past_len_host + slot_host; the decode loop is sl_generate_sc's.  past + prompt + max_new_tokens
 * <= max_ctx per sequence.  The logits processors' history starts EMPTY at this call's first generated token (as HF's would over
 * input_ids of the new tokens only): tokens of earlier turns are neither penalised nor counted into n-grams or min_new_tokens.
 * opts->compact must be 0 when past_len_host is non-NULL (SL_ERR_ARG): compaction moves live rows into the slots of finished rows
 * and destroys the K/V the caller wants to keep.  The decode loop keeps row b in slot b, so slot_host must be NULL or the identity
 * (SL_ERR_UNSUPPORTED otherwise).  NULL / all-zero pasts and NULL slots give exactly sl_generate_sc.
 * What is valid afterwards is the caller's bookkeeping: finished rows of the uncompacted batch go on appending pad tokens, so
 * after a call in which sequence s generated g_s tokens (its last one counted) its valid length is past_s + len_s + g_s - 1;
 * everything above is overwritten by the next call.  The last generated token was never fed back: the next call's rows begin
 * with its embedding. */
int sl_llama_prefill_cont(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, const int32_t* past_len_host,
                          const int32_t* slot_host, int32_t nseq, float* logits, int32_t* ctx_len_dev, void* workspace, size_t workspace_bytes,
                          sl_stream stream);
size_t sl_generate_workspace_bytes_cont(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp,
                                        int32_t scores);
int sl_generate_cont(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                     const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                     sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host, const int32_t* past_len_host, const int32_t* slot_host);

/* ---------------------------------------------------------------------------------------------
 * HF's four further logits warpers in the device sampler; additive to ABI 7, no struct above changes its size.
 * They run behind temperature / top-k / top-p in HF's order: min_p, typical_p, epsilon_cutoff, eta_cutoff.  S is the survivor set
 * entering a stage, p the softmax of the scores / T over S, H = -sum_S p ln p (natural log); equal scores always share their fate:
 *   min_p           in [0, 1], 0 = off:   keep i iff p_i >= min_p * max_S p            (the maximum and its ties always stay)
 *   typical_p       in (0, 1], 1 = off:   d_i = |-ln p_i - H|; drop i iff the mass of the tokens of S with a strictly smaller d is
 *                                         >= typical_p  (HF's rule; a band in score: the row maximum itself may be dropped)
 *   epsilon_cutoff  in [0, 1), 0 = off:   keep i iff p_i >= epsilon or x_i is the largest score in S
 *   eta_cutoff      in [0, 1), 0 = off:   eta = min(epsilon, sqrt(epsilon) * exp(-H)); keep i iff p_i >= eta or x_i is the largest in S
 * The draw (u = hash(seed, row, step), inverse CDF in index order, never a token of mass zero), the log-probability log(p / z) and the
 * row without a finite logit (token 0, -inf) are sl_sample_select_sc's over the final survivors.  A value outside its range or NaN is
 * SL_ERR_ARG before any launch, with the value in sl_last_error.  warp NULL, or every field at its off value, gives exactly the call
 * without it: bit for bit and launch for launch, the same captured graphs.  No workspace grows: sl_generate_workspace_bytes_n /
 * _cont / _sc sizes hold for sl_generate_w, and choice_ws is B int32 as before (the warped kernel keeps its state in LDS and registers).
 *
 * sl_sample_select_w: sl_sample_select_sc (logprob_out may be NULL: then sl_sample_select) + warp.
 * sl_generate_w: ONE entry for the plain, scored, several-answers and continued forms — sl_generate_sc's arguments, then
 * num_return_sequences (sl_generate_n; 1 = one answer), past_len_host / slot_host (sl_generate_cont; NULL = a fresh cache), then warp.
 * Without opts->sample the warp values are checked and otherwise ignored, as temperature is. */
typedef struct { float min_p, typical_p, epsilon_cutoff, eta_cutoff; } sl_warp_opts;
int sl_sample_select_w(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                       const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len,
                       int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, int32_t* choice_ws,
                       float* logprob_out, sl_stream stream, const sl_warp_opts* warp);
int sl_generate_w(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                  const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                  sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host, int32_t num_return_sequences,
                  const int32_t* past_len_host, const int32_t* slot_host, const sl_warp_opts* warp);

/* ---------------------------------------------------------------------------------------------
 * Teacher-forced scoring: the log-probability of GIVEN tokens, batched; additive to ABI 7.
 * For a scored row with hidden state h and label y:  logprob = log_softmax(lm_head(final_norm(h)))[y] in fp32, NaN counted as -inf, one
 * fixed order of additions (no float atomics).  A label outside [0, vocab) (HF's -100) marks an IGNORED position: its logprob is 0.0f, it
 * is counted in no sum, and nothing is read at its place.  top1 = the row's first maximum (sl_greedy_select's rule: the larger value, then
 * the lower column; NaN never wins).  A row without a finite maximum yields a non-finite logprob.
 *
 * sl_gemm_top1_lse_tgt: sl_gemm_top1_lse (same checks, same three planes bit for bit) plus tgt_val[m] = the value at (m, tgt_col[m]) — the
 * acc + bias value the top-1 compared, stored by the one lane that holds that element.  A row whose tgt_col lies outside [0, N) is written
 * by nobody: tgt_val[m] keeps what it held.  tgt_col (M int32) and tgt_val (M floats) are device pointers and come both or neither
 * (neither: this IS sl_gemm_top1_lse).
 *
 * sl_score_finalize: the three planes ([g][rows], n_groups = ceil(vocab / 64)) and tgt_val -> logprob_out[r] = (tgt_val[r] - m) -
 * logf(sum_g amax_sum[g] * expf(amax_val[g] - m)), m the row maximum, and top1_out[r] (may be NULL).  tgt_val[r] is not read for an
 * ignored label.  Groups are added in index order within each of 32 stripes (g mod 32), the stripes in order.
 * sl_score_rows: the same two outputs from fp32 logits (rows, vocab) of pitch ld, one block per row through the row reduce of
 * sl_greedy_select_sc / sl_logits_process; logits[r][label] is not read for an ignored label.
 * sl_score_segment_sums: per sequence s over rows [row_offsets[s], row_offsets[s + 1]) (device, nseq + 1 entries): sum_logprob[s], n_counted[s]
 * (rows that are not ignored) and n_top1[s] (counted rows whose top1 equals the label; top1 and n_top1 come both or neither).
 *
 * sl_llama_score: sl_llama_prefill's layers over the packed sequences of x (modified in place, K/V left in slots [0, nseq) like prefill;
 * no generation state, captured graph or session is touched), then row score_start_host[s] + j of sequence s is scored against
 * labels_dev[off_s + j], off_s = sum of n_score_host below s; logprob_dev / top1_dev (may be NULL) have sum n_score entries in that
 * order; seq_sum_dev / seq_counted_dev / seq_top1_dev (nseq each, all three or none) take sl_score_segment_sums' results.  The final
 * layer computes nothing behind attention except for the scored rows; the lm_head runs in passes of opts->row_chunk rows (0 = 2 048): a
 * pass of more than 64 rows through sl_gemm_top1_lse_tgt + sl_score_finalize (no logit is written), a pass of at most 64 rows — a short
 * remainder included — through fp32 logits + sl_score_rows.  force_path: 0 = that rule, 1 = always fp32 logits + sl_score_rows, 2 = fused
 * wherever a pass has more than 64 rows.  The shared-prefix prefill is not used (kv->shared_prefix is ignored).  The e4m3 K/V format is
 * accepted: prefill under it attends the unquantised rows and that path is the one prefill runs.  One host synchronisation, as in prefill.
 * Checked before any launch: SL_ERR_ARG for null pointers, n_score < 0, start < 0, start + n > length, sum n_score == 0, the per-sequence
 * outputs given partly, row_chunk < 0, a workspace below sl_llama_score_workspace_bytes (0 on a bad argument); SL_ERR_UNSUPPORTED for a
 * cache with fewer than nseq slots or a sequence longer than max_ctx.  sl_llama_score_last_paths(): what the calling thread's last
 * sl_llama_score ran — bit 0 = fp32 logits + sl_score_rows, bit 1 = the fused planes. */
typedef struct {
  int32_t row_chunk;   /* lm_head rows per pass; 0 = default */
  int32_t force_path;  /* 0 = rule above, 1 = always fp32 logits + sl_score_rows, 2 = fused wherever M > 64 */
  int32_t reserved[6];
} sl_score_opts;
int sl_gemm_top1_lse_tgt(const sl_gemm_args* args, const sl_gemm_ex_args* ex, float* amax_sum, const int32_t* tgt_col, float* tgt_val, sl_stream stream);
int sl_score_finalize(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t vocab, const float* tgt_val,
                      const int32_t* labels, int32_t rows, float* logprob_out, int32_t* top1_out, sl_stream stream);
int sl_score_rows(const float* logits, int64_t ld, const int32_t* labels, int32_t rows, int32_t vocab, float* logprob_out, int32_t* top1_out,
                  sl_stream stream);
int sl_score_segment_sums(const float* logprob, const int32_t* labels, const int32_t* top1, const int32_t* row_offsets, int32_t nseq, int32_t vocab,
                          float* sum_logprob, int32_t* n_counted, int32_t* n_top1, sl_stream stream);
size_t sl_llama_score_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int64_t n_rows, const sl_score_opts* opts);
int sl_llama_score(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                   const int32_t* score_start_host, const int32_t* n_score_host, const int32_t* labels_dev, float* logprob_dev, int32_t* top1_dev,
                   float* seq_sum_dev, int32_t* seq_counted_dev, int32_t* seq_top1_dev, const sl_score_opts* opts, void* workspace,
                   size_t workspace_bytes, sl_stream stream);
int32_t sl_llama_score_last_paths(void);

/* ---------------------------------------------------------------------------------------------
 * KD step, layer stacks (C++ host runtime of the training tape: one call issues the launches of a whole stack of layers
 * over a packed ragged batch; ref:trainer.py:270-384 runs the same arithmetic through autograd, one utterance at a time).
 * Saved activations, hidden states and fp32 gradient accumulators are caller-owned; temporaries come from `workspace`.
 *
 * Encoder (HuBERT stable-LN layer hf:models/hubert/modeling_hubert.py:504-547; Whisper hf:models/whisper/modeling_whisper.py:
 * 360-414; head_dim 64, bidirectional): train()-mode regularisers as sl_dropout / sl_attn_args.dropout_p, LayerDrop via `skip`.
 *   seeds: HOST array (n_layers, 4) = {attention-probability, attention-output, activation, ffn-output} dropout seeds.
 *   fwd: layer l reads its input (x_in or the previous layer's x_out), fills saved[l] (and records the input pointer in
 *        saved[l].x); *x_out = the stack's output.  bwd: layers layer_end-1 .. layer_begin; dx holds d(output of layer
 *        layer_end-1) on entry and d(input of layer layer_begin) on return; parameter gradients ACCUMULATE into grads[l]
 *        (kernel layouts: wqkv (3H, H), w1 (F, H), w2 (H, F), ...).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t dtype, hidden, n_heads, ffn, n_layers, nseq, max_len, reserved;
  int64_t n_tok;
  float ln_eps, p_hidden, p_act, p_attn;
  const int32_t* cu;       /* (nseq+1) device: first packed row of each sequence */
  const int32_t* klen;     /* (nseq) device */
  const uint8_t* skip;     /* (n_layers) HOST: 1 = LayerDrop skips the layer */
  const uint64_t* seeds;   /* (n_layers, 4) HOST */
} sl_enc_stack_cfg;
typedef struct {
  const void* x;                                            /* layer input, recorded by the forward */
  void *ln1, *qkv, *att, *x_mid, *ln2, *pre1, *mid, *x_out; /* (n_tok, H | 3H | H | H | H | F | F | H) */
  float* lse;                                               /* (n_tok, n_heads) */
} sl_enc_layer_saved;
typedef struct {
  float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
} sl_enc_layer_grads;
size_t sl_encoder_stack_train_workspace_bytes(const sl_enc_stack_cfg* c);
int sl_encoder_stack_train_fwd(const sl_hubert_layer* layers, const sl_enc_stack_cfg* c, const void* x_in, sl_enc_layer_saved* saved,
                               const void** x_out, void* workspace, size_t workspace_bytes, sl_stream stream);
int sl_encoder_stack_train_bwd(const sl_hubert_layer* layers, const sl_enc_stack_cfg* c, const sl_enc_layer_saved* saved,
                               const sl_enc_layer_grads* grads, int32_t layer_begin, int32_t layer_end, void* dx, void* workspace,
                               size_t workspace_bytes, sl_stream stream);

/* Frozen Llama decoder (hf:models/llama/modeling_llama.py:284-324; head_dim 128, causal GQA) over packed sequences:
 *   hidden: HOST array of n_layers + 1 device buffers (n_tok, H): hidden[0] = input embeddings (caller-filled),
 *           hidden[l + 1] = output of layer l (written by fwd) — these are HF's `hidden_states` taps before the final norm.
 *   fwd:    saved == NULL keeps nothing else (teacher pass, torch.no_grad in ref:trainer.py:337-344); otherwise saved[l]
 *           receives what the data-gradient backward needs.
 *   bwd:    dx = d(hidden[n_layers]) on entry, d(hidden[0]) on return; d_tap (HOST array of n_layers pointers or NULL):
 *           d_tap[l] != NULL is added to the gradient of hidden[l] (feature-distillation terms, ref:trainer.py:358-370).
 *   pos: (n_tok) device position ids; layers[l].*_t: transposed copies (in, out) of the frozen weights for the dgrad GEMMs. */
typedef struct {
  int32_t dtype, hidden, n_heads, n_kv_heads, head_dim, ffn, n_layers, nseq, max_len, reserved;
  int64_t n_tok;
  float rms_eps;
  const int32_t* cu;
  const int32_t* klen;
  const int32_t* pos;
  const float* rope_cos;
  const float* rope_sin;
} sl_llama_stack_cfg;
typedef struct {
  const void *norm1, *wqkv, *wo, *norm2, *wgu, *wdown;   /* nn.Linear layouts; gate/up interleaved in 16-row blocks */
  const void *wqkv_t, *wo_t, *wgu_t, *wdown_t;           /* (in, out) copies; only the backward reads them */
} sl_llama_train_layer;
typedef struct {
  void *qkv, *x2, *gu, *att;   /* (n_tok, (nh+2nkv)D | H | 2F | nh D) */
  float* lse;                  /* (n_tok, n_heads) */
} sl_llama_layer_saved;
size_t sl_llama_stack_train_workspace_bytes(const sl_llama_stack_cfg* c);
int sl_llama_stack_train_fwd(const sl_llama_train_layer* layers, const sl_llama_stack_cfg* c, void* const* hidden,
                             const sl_llama_layer_saved* saved, void* workspace, size_t workspace_bytes, sl_stream stream);
int sl_llama_stack_train_bwd(const sl_llama_train_layer* layers, const sl_llama_stack_cfg* c, void* const* hidden,
                             const sl_llama_layer_saved* saved, void* const* d_tap, void* dx, void* workspace, size_t workspace_bytes,
                             sl_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Collective (group 11): the ONE exchange of the hot path — the in-place sum of the encoder's fp32 gradient arena over the ranks
 * of a data-parallel KD step.  The reference has none (ref:README.md:86: "only supports training on a single GPU with a batch size
 * of 1"); its accumulation boundary ref:trainer.py:373-384 is where the sum goes.  RCCL over xGMI, one process per GPU; librccl is
 * bound at run time (a host without it gets SL_ERR_UNSUPPORTED from these calls and everything else keeps working).
 *   sl_comm_unique_id : rank 0 draws the 128-byte RCCL id; the caller carries it to the other ranks over whatever channel launched
 *                       them (torchrun's store, MPI, a file) — the library opens no sockets of its own.
 *   sl_comm_init      : collective over `world` processes, each on its own current device; the communicator belongs to that device.
 *   sl_allreduce_sum  : in place on `count` elements (SL_F32 / SL_BF16) of caller-owned device memory, asynchronous on `stream`
 *                       (the KD step passes a side stream behind an event on the kernels' stream); same call order on all ranks.
 *   sl_comm_destroy   : collective; the caller has synchronised the streams it used.
 *   sl_comm_abort     : LOCAL tear-down (ncclCommAbort): for a communicator whose peers may never have made theirs — a start-up the
 *                       ranks voted to abandon, or one obtained after this rank had given up waiting (ABI version 6).
 * --------------------------------------------------------------------------------------------- */
#define SL_COMM_ID_BYTES 128
typedef struct sl_comm_s* sl_comm;
int sl_comm_unique_id(void* id_out /* SL_COMM_ID_BYTES */);
int sl_comm_init(sl_comm* comm_out, const void* unique_id /* SL_COMM_ID_BYTES */, int32_t rank, int32_t world);
int sl_allreduce_sum(sl_comm comm, void* buf, int64_t count, int32_t dtype, sl_stream stream);
int sl_comm_destroy(sl_comm comm);
int sl_comm_abort(sl_comm comm);
int32_t sl_comm_rank(sl_comm comm);    /* -1: not a communicator */
int32_t sl_comm_world(sl_comm comm);

#ifdef __cplusplus
}
#endif
#endif /* SPEECHLLM_H */
