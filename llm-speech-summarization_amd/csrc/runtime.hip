// runtime.hip — C++ host runtime above the kernels: HuBERT encoder forward over a batch of utterances,
// Llama prefill / decode step / generation.  The decode step is captured once into a hipGraph and replayed, all per-step state lives on
// the device.  Two host loops, generate_impl (greedy / sampling, per-row budgets, compaction, token log-probabilities) and
// sl_beam_generate_lp, share decode_graph_get — scratch reset, the one key constructor, capture, instantiate, cache — and hand it what
// follows the lm_head as a callable; HF's logits processors (logits_proc.hip) sit between the lm_head's fp32 logits and the selection in
// both.  generate_impl's per-row state is one RowTable.  Workspace is carved from one caller-owned buffer.
#include <cmath>
#include <vector>

#include "common.h"
#include "gemm_internal.h"
#include "wformat.h"

int sl_attn_decode_impl(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, const int32_t* ctx_len,
                        int ctx_add, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale, int32_t dtype,
                        hipStream_t st);
int sl_logits_opts_check(const char* who, const sl_logits_opts* lp, int max_new_tokens);
int sl_logits_process_impl(float* logits, int32_t rows, int32_t V, const int32_t* hist, const int32_t* hist_odd, int64_t hist_ld, const int32_t* hist_len,
                           const int32_t* unfinished, const sl_logits_opts* lp, const int32_t* eos_ids_host, int32_t n_eos, int32_t log_softmax,
                           float* scratch, hipStream_t st);

int sl_attn_decode_split_zero_counters(void* workspace, int B, int n_heads, int n_kv, int max_ctx, hipStream_t st);
int sl_attn_decode_split_impl(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                              const int32_t* ctx_len, int ctx_add, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx,
                              float scale, int32_t dtype, hipStream_t st, int counters, int shared_prefix, int kv_format);
size_t sl_attn_decode_split_ws(int B, int n_heads, int n_kv, int max_ctx);
int sl_attn_decode_grouped_impl(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                                const int32_t* ctx_len, int ctx_add, const int32_t* prefix_len, const sl_attn_group* groups_dev, int32_t B,
                                int32_t row_slot0, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale, int32_t dtype,
                                int32_t kv_format, hipStream_t st);
bool sl_attn_decode_grouped_built(int n_heads, int n_kv, int D, int dtype, int kv_format);
int sl_rmsnorm_rstd_impl(const void* x, void* y, const void* w, float* rstd_out, int64_t rows, int32_t cols, float eps, int32_t dtype, hipStream_t st);
int sl_gemm_impl(const sl_gemm_args* a, const sl_gemm_fused* fx, const sl_gemm_ex_args* ex, hipStream_t st);
int sl_gemm_top1_lse_impl(const sl_gemm_args* a, const sl_gemm_ex_args* ex, float* amax_sum, hipStream_t st);
int sl_gemm_top1_lse_tgt_impl(const sl_gemm_args* a, const sl_gemm_ex_args* ex, float* amax_sum, const int32_t* tgt_col, float* tgt_val, hipStream_t st);
int sl_score_finalize_impl(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t V, const float* tgt_val,
                           const int32_t* labels, int32_t rows, float* logprob_out, int32_t* top1_out, hipStream_t st);
int sl_score_rows_impl(const float* logits, int64_t ld, const int32_t* labels, int32_t rows, int32_t V, float* logprob_out, int32_t* top1_out, hipStream_t st);
int sl_score_segment_sums_impl(const float* logprob, const int32_t* labels, const int32_t* top1, const int32_t* row_offsets, int32_t nseq, int32_t V,
                               float* sum_logprob, int32_t* n_counted, int32_t* n_top1, hipStream_t st);

namespace {

struct Carver {
  unsigned char* base;
  size_t off = 0, cap;
  Carver(void* b, size_t c) : base((unsigned char*)b), cap(c) {}
  void* take(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
  bool ok() const { return off <= cap; }
};

int gemm(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const void* bias, const void* res,
         int64_t ldr, int M, int N, int K, int act, int out_f32, hipStream_t st) {
  sl_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.bias = bias; a.residual = res; a.ldr = ldr;
  a.M = M; a.N = N; a.K = K; a.batch = 1; a.dtype = dtype; a.act = act; a.out_f32 = out_f32;
  return sl_gemm(&a, (sl_stream)st);
}

inline unsigned char* bptr(void* p) { return (unsigned char*)p; }

}  // namespace

// ================================================================================================
// HuBERT
// ================================================================================================
extern "C" int sl_hubert_num_frames(const sl_hubert_model* m, int64_t n_samples) {
  int64_t L = n_samples;
  for (int i = 0; i < m->n_conv; ++i) {
    if (L < m->conv_kernel[i]) return 0;
    L = (L - m->conv_kernel[i]) / m->conv_stride[i] + 1;
  }
  return (int)L;
}

struct HubertPlan {
  int64_t max_conv_elems = 0;  // largest conv activation (elements) over layers and utterances
  int64_t total_T = 0, max_T = 0, total_P = 0;
  int64_t conv_elems[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int64_t> T, P, tok0;
};

static int hubert_plan(const sl_hubert_model* m, const int64_t* offs, int n_utt, HubertPlan& pl) {
  pl.T.resize(n_utt); pl.P.resize(n_utt); pl.tok0.resize(n_utt + 1);
  for (int u = 0; u < n_utt; ++u) {
    int64_t L = offs[u + 1] - offs[u];
    for (int i = 0; i < m->n_conv; ++i) {
      SL_CHECK_ARG(L >= m->conv_kernel[i], "sl_hubert_forward: utterance %d too short (%lld samples)", u, (long long)(offs[u + 1] - offs[u]));
      L = (L - m->conv_kernel[i]) / m->conv_stride[i] + 1;
      pl.conv_elems[i] += L * m->conv_dim[i];   // conv activations of the whole batch are packed per layer
      if (pl.conv_elems[i] > pl.max_conv_elems) pl.max_conv_elems = pl.conv_elems[i];
    }
    pl.T[u] = L;
    SL_CHECK_ARG(L >= m->pool_kernel, "sl_hubert_forward: utterance %d gives %lld frames < pool kernel %d", u, (long long)L, m->pool_kernel);
    pl.P[u] = (L - m->pool_kernel) / m->pool_stride + 1;
    pl.tok0[u] = pl.total_T;
    pl.total_T += L;
    pl.total_P += pl.P[u];
    if (L > pl.max_T) pl.max_T = L;
  }
  pl.tok0[n_utt] = pl.total_T;
  return 0;
}

struct HubertWs {
  void *convA, *convB, *feat, *x, *ln, *qkv, *att, *mid, *xg, *pooled;
  int32_t *cu, *cuk, *klen;
  int64_t* desc;
  int64_t* c0desc;  // n_utt + 1 sample offsets, then n_utt + 1 row offsets of the conv0 output (batched conv0 launch)
  int64_t* pdesc;   // per utterance {pooled rows, element offset into `pooled`, element offset into `out`, 0}: AvgPool + grouped projector
  float* ln_stats;  // LayerNorm fold: [frames][hidden / 64][2] partial {sum, sum of squares} out of the out_proj / FFN2 epilogues
  float* ln_mr;     //                 [frames][2] {mean, rstd}
};

// pooled_rows: rows of the downsampled frames ahead of the projection (default: the AvgPool's; ctc_pool: one per range)
static size_t hubert_carve(const sl_hubert_model* m, const HubertPlan& pl, int n_utt, void* base, size_t cap, HubertWs& w, int64_t pooled_rows = -1) {
  const size_t sz = sl_dtype_size(m->dtype);
  const int H = m->hidden;
  Carver c(base, cap);
  w.convA = c.take(pl.max_conv_elems * sz);
  w.convB = c.take(pl.max_conv_elems * sz);
  w.feat = c.take(pl.total_T * m->conv_dim[m->n_conv - 1] * sz);
  w.x = c.take(pl.total_T * H * sz);
  w.ln = c.take(pl.total_T * H * sz);
  w.qkv = c.take(pl.total_T * 3 * H * sz);
  w.att = c.take(pl.total_T * H * sz);
  w.mid = c.take(pl.total_T * (int64_t)m->ffn * sz);
  w.xg = c.take((pl.total_T + (int64_t)n_utt * m->pos_k) * H * sz);
  w.desc = (int64_t*)c.take((size_t)((m->n_conv - 1) * n_utt + n_utt * m->pos_groups) * 4 * sizeof(int64_t));
  w.pooled = c.take((pooled_rows < 0 ? pl.total_P : pooled_rows) * H * sz);
  w.pdesc = (int64_t*)c.take((size_t)n_utt * 4 * sizeof(int64_t));
  w.c0desc = (int64_t*)c.take((size_t)(n_utt + 1) * 2 * sizeof(int64_t));
  w.cu = (int32_t*)c.take((n_utt + 1) * sizeof(int32_t));
  w.cuk = (int32_t*)c.take(n_utt * sizeof(int32_t));
  w.klen = (int32_t*)c.take(n_utt * sizeof(int32_t));
  w.ln_stats = (float*)c.take((size_t)pl.total_T * (size_t)((H + 63) / 64) * 2 * sizeof(float));
  w.ln_mr = (float*)c.take((size_t)pl.total_T * 2 * sizeof(float));
  return c.off + 256;
}

// records of the pooled rows / projector output rows of every utterance (see HubertWs::pdesc)
static void proj_records(const sl_hubert_model* m, const HubertPlan& pl, int n_utt, int64_t out_ld, const int64_t* out_row_offsets_host,
                         std::vector<int64_t>& rec) {
  rec.assign((size_t)n_utt * 4, 0);
  int64_t prow = 0;
  for (int u = 0; u < n_utt; ++u) {
    rec[4 * u] = pl.P[u];
    rec[4 * u + 1] = prow * m->hidden;
    rec[4 * u + 2] = (out_row_offsets_host ? out_row_offsets_host[u] : prow) * out_ld;
    prow += pl.P[u];
  }
}

// rows each utterance gives the projection under a stack / ctc_pool descriptor
static int64_t ds_rows(const sl_downsample_desc* ds, const HubertPlan& pl, int u) {
  return ds->method == SL_DS_STACK ? pl.T[u] / ds->factor : ds->range_counts_host[u];
}

// stack / ctc_pool records of the grouped projector GEMM, one per utterance that has rows (a group without rows is left out):
// {rows, element offset of its first A row, element offset into `out`, 0}.  stack: A is the final LayerNorm's output read with lda = f H
// (row p = frames f p .. f p + f - 1, contiguous), ctc_pool: the range means.  Returns the number of records.
static int ds_records(const sl_hubert_model* m, const sl_downsample_desc* ds, const HubertPlan& pl, int n_utt, int64_t out_ld,
                      const int64_t* out_row_offsets_host, std::vector<int64_t>& rec, int64_t* max_rows) {
  rec.clear();
  int64_t prow = 0, mx = 0;
  for (int u = 0; u < n_utt; ++u) {
    const int64_t P = ds_rows(ds, pl, u);
    if (P > 0) {
      rec.push_back(P);
      rec.push_back((ds->method == SL_DS_STACK ? pl.tok0[u] : prow) * m->hidden);
      rec.push_back((out_row_offsets_host ? out_row_offsets_host[u] : prow) * out_ld);
      rec.push_back(0);
      if (P > mx) mx = P;
    }
    prow += P;
  }
  if (max_rows) *max_rows = mx;
  return (int)(rec.size() / 4);
}

// transformer layers on the packed frames of the batch (varlen attention), final LayerNorm, downsample (AvgPool, or the descriptor's stack / ctc_pool) + projection.
// Shared by the HuBERT and Whisper front ends (both are 16x64 pre-LN encoders: hf:...hubert.py:504-547,
// hf:models/whisper/modeling_whisper.py:360-414).
static int encoder_tail(const sl_hubert_model* m, HubertWs& w, const HubertPlan& pl, int n_utt, void* out, int64_t out_ld,
                        const int64_t* out_row_offsets_host, void* last_hidden, hipStream_t st, const sl_downsample_desc* ds = nullptr) {
  sl_stream stream = (sl_stream)st;
  const int dt = m->dtype, H = m->hidden, NT = (int)pl.total_T;
  const size_t sz = sl_dtype_size(dt);
  // LayerNorm fold (bf16 inference, weights prepared by the caller: m->fold): no LayerNorm pass over the frames inside the layers.
  // x -> [q|k|v Linear with ln1 folded in, row statistics applied in its epilogue] -> attention -> out_proj (+ bias + residual;
  // its epilogue leaves the row statistics of the new x) -> [FFN1 with ln2 folded in, GELU] -> FFN2 (+ bias + residual, statistics
  // again).  Two LayerNorm launches per layer (160 us each at 255 k frames, HBM-bound) become two 8 us finalize launches.
  const bool fold = m->fold != nullptr && sl_is16(dt) && !sl_env().no_ln_fold && H % 64 == 0 && m->ffn % 64 == 0 &&
                    sl_gemm_rows_epilogue_ok(NT, 3 * H, H, dt) && sl_gemm_rows_epilogue_ok(NT, H, H, dt) &&
                    sl_gemm_rows_epilogue_ok(NT, m->ffn, H, dt) && sl_gemm_rows_epilogue_ok(NT, H, m->ffn, dt);
  auto gemm_x = [&](const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const void* bias, const void* res, int N, int K, int act,
                    const float* ln_u, const float* ln_c, bool stats) -> int {
    sl_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.bias = bias; a.residual = res; a.ldr = res ? ldc : 0;
    a.M = NT; a.N = N; a.K = K; a.batch = 1; a.dtype = dt; a.act = act;
    sl_gemm_ex_args ex;
    memset(&ex, 0, sizeof(ex));
    ex.w_mod = 1;
    if (ln_u) { ex.ln_mr = w.ln_mr; ex.ln_u = ln_u; ex.ln_c = ln_c; }
    if (stats) ex.stats_out = w.ln_stats;
    return sl_gemm_impl(&a, nullptr, &ex, st);
  };
  if (fold) SL_TRY(sl_layernorm_stats(w.x, NT, H, m->ln_eps, w.ln_mr, dt, stream));       // the first layer's input comes out of the positional conv
  for (int l = 0; l < m->n_layers; ++l) {
    const sl_hubert_layer& L = m->layers[l];
    if (fold) {
      const sl_hubert_fold& F = m->fold[l];
      SL_TRY(gemm_x(w.x, H, F.wqkv_f, H, w.qkv, 3 * H, nullptr, nullptr, 3 * H, H, SL_ACT_NONE, F.uqkv, F.cqkv, false));
    } else {
      SL_TRY(sl_layernorm(w.x, w.ln, L.ln1_g, L.ln1_b, NT, H, m->ln_eps, 0, dt, stream));
      SL_TRY(gemm(dt, w.ln, H, L.wqkv, H, w.qkv, 3 * H, L.bqkv, nullptr, 0, NT, 3 * H, H, SL_ACT_NONE, 0, st));
    }
    sl_attn_args a;
    memset(&a, 0, sizeof(a));
    a.q = w.qkv; a.q_row_stride = 3 * H; a.q_head_stride = 64;
    a.k = bptr(w.qkv) + (size_t)H * sz; a.k_row_stride = 3 * H; a.k_head_stride = 64;
    a.v = bptr(w.qkv) + (size_t)2 * H * sz; a.v_row_stride = 3 * H; a.v_head_stride = 64;
    a.out = w.att; a.o_row_stride = H; a.o_head_stride = 64;
    a.cu_q = w.cu; a.cu_k = w.cuk; a.klen = w.klen;
    a.nseq = n_utt; a.max_qlen = (int)pl.max_T; a.n_heads = m->n_heads; a.n_kv_heads = m->n_heads; a.head_dim = 64; a.causal = 0;
    a.dtype = dt; a.scale = 0.125f;
    SL_TRY(sl_attn_fwd(&a, stream));
    if (fold) {
      const sl_hubert_fold& F = m->fold[l];
      SL_TRY(gemm_x(w.att, H, L.wo, H, w.x, H, L.bo, w.x, H, H, SL_ACT_NONE, nullptr, nullptr, true));
      SL_TRY(sl_layernorm_stats_finalize(w.ln_stats, H / 64, NT, H, m->ln_eps, w.ln_mr, stream));
      SL_TRY(gemm_x(w.x, H, F.w1_f, H, w.mid, m->ffn, nullptr, nullptr, m->ffn, H, SL_ACT_GELU, F.u1, F.c1, false));
      const bool more = l + 1 < m->n_layers;       // the final LayerNorm keeps its own kernel (its output is the product)
      SL_TRY(gemm_x(w.mid, m->ffn, L.w2, m->ffn, w.x, H, L.b2, w.x, H, m->ffn, SL_ACT_NONE, nullptr, nullptr, more));
      if (more) SL_TRY(sl_layernorm_stats_finalize(w.ln_stats, H / 64, NT, H, m->ln_eps, w.ln_mr, stream));
      continue;
    }
    SL_TRY(gemm(dt, w.att, H, L.wo, H, w.x, H, L.bo, w.x, H, NT, H, H, SL_ACT_NONE, 0, st));
    SL_TRY(sl_layernorm(w.x, w.ln, L.ln2_g, L.ln2_b, NT, H, m->ln_eps, 0, dt, stream));
    SL_TRY(gemm(dt, w.ln, H, L.w1, H, w.mid, m->ffn, L.b1, nullptr, 0, NT, m->ffn, H, SL_ACT_GELU, 0, st));
    SL_TRY(gemm(dt, w.mid, m->ffn, L.w2, m->ffn, w.x, H, L.b2, w.x, H, NT, H, m->ffn, SL_ACT_NONE, 0, st));
  }
  void* lh = last_hidden ? last_hidden : w.ln;
  SL_TRY(sl_layernorm(w.x, lh, m->final_ln_g, m->final_ln_b, NT, H, m->ln_eps, 0, dt, stream));
  if (ds) {
    // ---- stack / ctc_pool + projection into the caller's (prompt) buffer: at most one downsample launch (stack needs none) and one grouped GEMM
    std::vector<int64_t> rec;
    int64_t max_rows = 0;
    const int n_grp = ds_records(m, ds, pl, n_utt, out_ld, out_row_offsets_host, rec, &max_rows);     // the same records the caller uploaded to w.pdesc
    if (n_grp == 0) return 0;
    const bool stack = ds->method == SL_DS_STACK;
    if (!stack) SL_TRY(sl_segment_mean_batch(lh, w.pooled, ds->ranges_dev, ds->n_ranges, NT, H, dt, stream));
    const int Kp = stack ? ds->factor * H : H;
    sl_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = stack ? lh : w.pooled; a.lda = Kp;
    a.W = ds->proj_w; a.ldw = Kp;
    a.C = out; a.ldc = out_ld;
    a.bias = ds->proj_b;
    a.M = (int)max_rows; a.N = m->llm_dim; a.K = Kp; a.batch = n_grp; a.dtype = dt; a.act = SL_ACT_NONE;
    sl_gemm_ex_args ex;
    memset(&ex, 0, sizeof(ex));
    ex.groups = w.pdesc; ex.w_mod = 1;
    return sl_gemm_impl(&a, nullptr, &ex, st);
  }
  // ---- AvgPool over time + projection into the caller's (prompt) buffer
  if (!m->proj_w) return 0;  // stack / ctc_pool through sl_hubert_forward: the host finishes from last_hidden
  // one AvgPool launch and one grouped projector GEMM for the whole ragged batch (records uploaded by the caller: w.pdesc)
  int64_t max_P = 0;
  for (int u = 0; u < n_utt; ++u) max_P = pl.P[u] > max_P ? pl.P[u] : max_P;
  SL_TRY(sl_avgpool_batch(lh, w.pooled, w.cu, w.klen, w.pdesc, n_utt, max_P, H, m->pool_kernel, m->pool_stride, dt, stream));
  sl_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.A = w.pooled; a.lda = H;
  a.W = m->proj_w; a.ldw = H;
  a.C = out; a.ldc = out_ld;
  a.bias = m->proj_b;
  a.M = (int)max_P; a.N = m->llm_dim; a.K = H; a.batch = n_utt; a.dtype = dt; a.act = SL_ACT_NONE;
  sl_gemm_ex_args ex;
  memset(&ex, 0, sizeof(ex));
  ex.groups = w.pdesc; ex.w_mod = 1;
  SL_TRY(sl_gemm_impl(&a, nullptr, &ex, st));
  return 0;
}

extern "C" size_t sl_hubert_workspace_bytes(const sl_hubert_model* m, const int64_t* sample_offsets_host, int32_t n_utt) {
  HubertPlan pl;
  if (hubert_plan(m, sample_offsets_host, n_utt, pl) != 0) return 0;
  HubertWs w;
  return hubert_carve(m, pl, n_utt, nullptr, 0, w);
}

// ds == nullptr: sl_hubert_forward (pool, or last_hidden only); otherwise a checked stack / ctc_pool descriptor (sl_hubert_forward_ds)
static int hubert_forward_impl(const sl_hubert_model* m, const float* waves, const int64_t* sample_offsets_host, int32_t n_utt, void* out, int64_t out_ld,
                               const int64_t* out_row_offsets_host, void* last_hidden, void* workspace, size_t workspace_bytes, sl_stream stream,
                               const sl_downsample_desc* ds) {
  SL_CHECK_ARG(m && waves && sample_offsets_host && workspace && n_utt > 0, "sl_hubert_forward: bad arguments");
  SL_CHECK_ARG(ds || (m->proj_w && out) || (!m->proj_w && last_hidden), "sl_hubert_forward: need `out` (pool) or `last_hidden` (host-side downsample)");
  SL_CHECK_ARG(m->n_conv >= 2 && m->n_conv <= 8 && m->hidden % m->n_heads == 0 && m->hidden / m->n_heads == 64,
               "sl_hubert_forward: need 2..8 conv layers and head_dim 64 (hidden=%d heads=%d)", m->hidden, m->n_heads);
  hipStream_t st = (hipStream_t)stream;
  const int dt = m->dtype;
  const int H = m->hidden;
  HubertPlan pl;
  SL_TRY(hubert_plan(m, sample_offsets_host, n_utt, pl));
  HubertWs w;
  const size_t need = hubert_carve(m, pl, n_utt, workspace, workspace_bytes, w, ds && ds->method == SL_DS_CTC_POOL ? ds->n_ranges : -1);
  SL_CHECK_ARG(need <= workspace_bytes, "sl_hubert_forward: workspace %zu B < required %zu B", workspace_bytes, need);
  const int Cl = m->conv_dim[m->n_conv - 1];

  // ---- descriptors of the ragged batch: row offsets of every utterance in each packed conv activation,
  //      grouped-GEMM records {M, a_off, c_off, r_off} for conv layers 1.. and for the positional conv
  const int nc = m->n_conv, G = m->pos_groups, Hg = H / G, kpos = m->pos_k;
  std::vector<std::vector<int64_t>> row0(nc, std::vector<int64_t>(n_utt + 1, 0)), Lc(nc, std::vector<int64_t>(n_utt, 0));
  for (int u = 0; u < n_utt; ++u) {
    int64_t L = sample_offsets_host[u + 1] - sample_offsets_host[u];
    for (int i = 0; i < nc; ++i) { L = (L - m->conv_kernel[i]) / m->conv_stride[i] + 1; Lc[i][u] = L; }
  }
  for (int i = 0; i < nc; ++i)
    for (int u = 0; u < n_utt; ++u) row0[i][u + 1] = row0[i][u] + Lc[i][u];
  std::vector<int64_t> desc((size_t)((nc - 1) * n_utt + n_utt * G) * 4);
  std::vector<int64_t> max_rows(nc, 0);
  for (int i = 1; i < nc; ++i)
    for (int u = 0; u < n_utt; ++u) {
      int64_t* d = &desc[(size_t)((i - 1) * n_utt + u) * 4];
      d[0] = Lc[i][u]; d[1] = row0[i - 1][u] * m->conv_dim[i - 1]; d[2] = row0[i][u] * m->conv_dim[i]; d[3] = 0;
      if (Lc[i][u] > max_rows[i]) max_rows[i] = Lc[i][u];
    }
  std::vector<int64_t> xg_off(n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) xg_off[u + 1] = xg_off[u] + (pl.T[u] + kpos) * H;
  const size_t pos_desc0 = (size_t)(nc - 1) * n_utt * 4;
  for (int u = 0; u < n_utt; ++u)
    for (int g = 0; g < G; ++g) {
      int64_t* d = &desc[pos_desc0 + (size_t)(u * G + g) * 4];
      d[0] = pl.T[u]; d[1] = xg_off[u] + (int64_t)g * (pl.T[u] + kpos) * Hg; d[2] = pl.tok0[u] * H + (int64_t)g * Hg; d[3] = d[2];
    }
  {
    std::vector<int32_t> cu(n_utt + 1), kl(n_utt);
    for (int u = 0; u <= n_utt; ++u) cu[u] = (int32_t)pl.tok0[u];
    for (int u = 0; u < n_utt; ++u) kl[u] = (int32_t)pl.T[u];
    SL_HIP(hipMemcpyAsync(w.cu, cu.data(), (n_utt + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipMemcpyAsync(w.cuk, cu.data(), n_utt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipMemcpyAsync(w.klen, kl.data(), n_utt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipMemcpyAsync(w.desc, desc.data(), desc.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    std::vector<int64_t> prec;
    if (ds) ds_records(m, ds, pl, n_utt, out_ld, out_row_offsets_host, prec, nullptr);
    else proj_records(m, pl, n_utt, out_ld, out_row_offsets_host, prec);
    if (!prec.empty()) SL_HIP(hipMemcpyAsync(w.pdesc, prec.data(), prec.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    std::vector<int64_t> c0(2 * (size_t)(n_utt + 1));
    for (int u = 0; u <= n_utt; ++u) { c0[u] = sample_offsets_host[u] - sample_offsets_host[0]; c0[n_utt + 1 + u] = row0[0][u]; }
    SL_HIP(hipMemcpyAsync(w.c0desc, c0.data(), c0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipStreamSynchronize(st));  // host vectors go out of scope; pageable copies are staged but be explicit
  }
  // ---- conv feature extractor: layer 0 per utterance (fused conv+LN+GELU), layers 1.. as ONE grouped implicit GEMM
  //      + ONE LayerNorm+GELU over the packed rows of the whole batch
  void* cur = w.convA;
  {
    int64_t max_L0 = 0;
    for (int u = 0; u < n_utt; ++u) max_L0 = Lc[0][u] > max_L0 ? Lc[0][u] : max_L0;
    SL_TRY(sl_hubert_conv0_batch(waves + sample_offsets_host[0], w.c0desc, w.c0desc + n_utt + 1, n_utt, max_L0, m->conv0_w, m->conv0_b, m->conv0_g,
                                 m->conv0_beta, cur, m->conv_dim[0], m->conv_kernel[0], m->conv_stride[0], 1e-5f, dt, stream));
  }
  for (int i = 1; i < nc; ++i) {
    const int Cin = m->conv_dim[i - 1], Cout = m->conv_dim[i], k = m->conv_kernel[i], s = m->conv_stride[i];
    void* dst = (i == nc - 1) ? w.feat : (cur == w.convA ? w.convB : w.convA);
    sl_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = cur; a.lda = (int64_t)s * Cin;   // implicit GEMM: output row t reads the k*Cin contiguous elements from input row t*s
    a.W = m->conv_w[i]; a.ldw = (int64_t)k * Cin;
    a.C = dst; a.ldc = Cout; a.bias = m->conv_b[i];
    a.M = (int)max_rows[i]; a.N = Cout; a.K = k * Cin; a.batch = n_utt; a.dtype = dt; a.act = SL_ACT_NONE;
    sl_gemm_ex_args ex;
    memset(&ex, 0, sizeof(ex));
    ex.groups = w.desc + (size_t)(i - 1) * n_utt * 4; ex.w_mod = 1;
    SL_TRY(sl_gemm_impl(&a, nullptr, &ex, st));
    SL_TRY(sl_layernorm(dst, dst, m->conv_g[i], m->conv_beta[i], row0[i][n_utt], Cout, 1e-5f, 1, dt, stream));
    cur = dst;
  }
  // ---- feature projection on the packed tokens
  const int NT = (int)pl.total_T;
  SL_TRY(sl_layernorm(w.feat, w.feat, m->fp_ln_g, m->fp_ln_b, NT, Cl, m->ln_eps, 0, dt, stream));
  SL_TRY(gemm(dt, w.feat, Cl, m->fp_w, Cl, w.x, H, m->fp_b, nullptr, 0, NT, H, Cl, SL_ACT_NONE, 0, st));
  // ---- positional conv embedding: x += gelu(grouped_conv(x)); every (utterance, group) is one record of ONE grouped GEMM
  {
    SL_TRY(sl_posconv_stage_batch(w.x, w.xg, w.cu, w.klen, n_utt, pl.max_T, H, G, kpos, dt, stream));
    sl_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = w.xg; a.lda = Hg;
    a.W = m->pos_w; a.ldw = (int64_t)kpos * Hg; a.strideW = (int64_t)Hg * kpos * Hg;
    a.C = w.ln; a.ldc = H;
    a.bias = m->pos_b; a.strideBias = Hg;
    a.residual = w.x; a.ldr = H;
    a.M = (int)pl.max_T; a.N = Hg; a.K = kpos * Hg; a.batch = n_utt * G; a.dtype = dt; a.act = SL_ACT_GELU;
    sl_gemm_ex_args ex;
    memset(&ex, 0, sizeof(ex));
    ex.groups = w.desc + pos_desc0; ex.w_mod = G;
    SL_TRY(sl_gemm_impl(&a, nullptr, &ex, st));
    void* t = w.x; w.x = w.ln; w.ln = t;
  }
  return encoder_tail(m, w, pl, n_utt, out, out_ld, out_row_offsets_host, last_hidden, st, ds);
}

extern "C" int sl_hubert_forward(const sl_hubert_model* m, const float* waves, const int64_t* sample_offsets_host, int32_t n_utt,
                                 void* out, int64_t out_ld, const int64_t* out_row_offsets_host, void* last_hidden, void* workspace,
                                 size_t workspace_bytes, sl_stream stream) {
  return hubert_forward_impl(m, waves, sample_offsets_host, n_utt, out, out_ld, out_row_offsets_host, last_hidden, workspace, workspace_bytes, stream, nullptr);
}

// every check of a stack / ctc_pool descriptor that needs no device; `who` names the entry point in the message
static int ds_check(const char* who, const sl_hubert_model* m, const sl_downsample_desc* ds, int32_t n_utt) {
  SL_CHECK_ARG(m && ds && n_utt > 0, "%s: null model / descriptor or no utterances", who);
  SL_CHECK_ARG(ds->method == SL_DS_STACK || ds->method == SL_DS_CTC_POOL, "%s: method %d: 1 (stack) or 2 (ctc_pool); `pool` goes through sl_hubert_forward", who,
               ds->method);
  SL_CHECK_ARG(ds->factor >= 1, "%s: downsample factor %d must be at least 1", who, ds->factor);
  SL_CHECK_ARG(ds->proj_w && ds->proj_b, "%s: null projection", who);
  if (ds->method == SL_DS_STACK) {
    SL_CHECK_ARG(ds->proj_in == ds->factor * m->hidden, "%s: stack: the projection reads %d features, factor x hidden = %d x %d", who, ds->proj_in, ds->factor,
                 m->hidden);
    return 0;
  }
  SL_CHECK_ARG(ds->proj_in == m->hidden, "%s: ctc_pool: the projection reads %d features, hidden = %d", who, ds->proj_in, m->hidden);
  SL_CHECK_ARG(ds->range_counts_host && (ds->ranges_dev || ds->n_ranges == 0) && ds->n_ranges >= 0, "%s: ctc_pool: null range table / counts", who);
  int64_t total = 0;
  for (int u = 0; u < n_utt; ++u) {
    SL_CHECK_ARG(ds->range_counts_host[u] >= 0, "%s: ctc_pool: utterance %d has %d ranges", who, u, ds->range_counts_host[u]);
    total += ds->range_counts_host[u];
  }
  SL_CHECK_ARG(total == ds->n_ranges, "%s: ctc_pool: the utterances' range counts add up to %lld, the table holds %lld", who, (long long)total,
               (long long)ds->n_ranges);
  return 0;
}

extern "C" size_t sl_hubert_workspace_bytes_ds(const sl_hubert_model* m, const int64_t* sample_offsets_host, int32_t n_utt, const sl_downsample_desc* ds) {
  if (!sample_offsets_host || ds_check("sl_hubert_workspace_bytes_ds", m, ds, n_utt) != 0) {
    if (!sample_offsets_host) sl_set_error("sl_hubert_workspace_bytes_ds: null sample offsets");
    return 0;
  }
  HubertPlan pl;
  if (hubert_plan(m, sample_offsets_host, n_utt, pl) != 0) return 0;
  HubertWs w;
  return hubert_carve(m, pl, n_utt, nullptr, 0, w, ds->method == SL_DS_CTC_POOL ? ds->n_ranges : -1);
}

extern "C" int sl_hubert_forward_ds(const sl_hubert_model* m, const float* waves, const int64_t* sample_offsets_host, int32_t n_utt, void* out, int64_t out_ld,
                                    const int64_t* out_row_offsets_host, void* last_hidden, const sl_downsample_desc* ds, void* workspace,
                                    size_t workspace_bytes, sl_stream stream) {
  SL_TRY(ds_check("sl_hubert_forward_ds", m, ds, n_utt));
  SL_CHECK_ARG(out && out_ld >= m->llm_dim, "sl_hubert_forward_ds: need `out` with rows of at least llm_dim = %d elements", m->llm_dim);
  return hubert_forward_impl(m, waves, sample_offsets_host, n_utt, out, out_ld, out_row_offsets_host, last_hidden, workspace, workspace_bytes, stream, ds);
}

// ================================================================================================
// Whisper encoder (hf:models/whisper/modeling_whisper.py:592-646): conv1(k3,p1)+GELU, conv2(k3,s2,p1)+GELU as implicit
// GEMMs over zero-haloed channel-last rows, + positional table, then the shared transformer tail.
// Model struct reuse: conv_dim[0] = n_mel, conv_w/b[1] = conv1, conv_w/b[2] = conv2 (tap-major), pos_w = embed_positions
// (pos_k rows = max_source_positions), frontend = 1.
// ================================================================================================
static int whisper_plan(const sl_hubert_model* m, int n_utt, HubertPlan& pl) {
  const int64_t T = m->pos_k;
  pl.T.assign(n_utt, T); pl.P.resize(n_utt); pl.tok0.resize(n_utt + 1);
  SL_CHECK_ARG(T >= m->pool_kernel, "sl_whisper_forward: %lld frames < pool kernel %d", (long long)T, m->pool_kernel);
  for (int u = 0; u < n_utt; ++u) { pl.P[u] = (T - m->pool_kernel) / m->pool_stride + 1; pl.tok0[u] = (int64_t)u * T; pl.total_P += pl.P[u]; }
  pl.tok0[n_utt] = (int64_t)n_utt * T;
  pl.total_T = (int64_t)n_utt * T; pl.max_T = T;
  // conv buffers: haloed mel (2T+2, n_mel) and haloed conv1 output (2T+2, H) per utterance
  pl.max_conv_elems = (int64_t)n_utt * (2 * T + 2) * (m->hidden > m->conv_dim[0] ? m->hidden : m->conv_dim[0]);
  return 0;
}

extern "C" size_t sl_whisper_workspace_bytes(const sl_hubert_model* m, int32_t n_utt) {
  HubertPlan pl;
  if (whisper_plan(m, n_utt, pl) != 0) return 0;
  HubertWs w;
  return hubert_carve(m, pl, n_utt, nullptr, 0, w);
}

extern "C" int sl_whisper_forward(const sl_hubert_model* m, const void* mel, int32_t n_utt, void* out, int64_t out_ld,
                                  const int64_t* out_row_offsets_host, void* last_hidden, void* workspace, size_t workspace_bytes,
                                  sl_stream stream) {
  SL_CHECK_ARG(m && mel && workspace && n_utt > 0, "sl_whisper_forward: bad arguments");
  SL_CHECK_ARG(m->reserved == 1, "sl_whisper_forward: model struct is not a Whisper front end");
  SL_CHECK_ARG((m->proj_w && out) || (!m->proj_w && last_hidden), "sl_whisper_forward: need `out` (pool) or `last_hidden`");
  SL_CHECK_ARG(m->hidden % m->n_heads == 0 && m->hidden / m->n_heads == 64, "sl_whisper_forward: head_dim must be 64");
  hipStream_t st = (hipStream_t)stream;
  const int dt = m->dtype, H = m->hidden, n_mel = m->conv_dim[0];
  const size_t sz = sl_dtype_size(dt);
  const int64_t T = m->pos_k, F = 2 * T;   // F mel frames in, T positions out
  HubertPlan pl;
  SL_TRY(whisper_plan(m, n_utt, pl));
  HubertWs w;
  const size_t need = hubert_carve(m, pl, n_utt, workspace, workspace_bytes, w);
  SL_CHECK_ARG(need <= workspace_bytes, "sl_whisper_forward: workspace %zu B < required %zu B", workspace_bytes, need);
  {
    std::vector<int32_t> cu(n_utt + 1), kl(n_utt, (int32_t)T);
    for (int u = 0; u <= n_utt; ++u) cu[u] = (int32_t)(u * T);
    SL_HIP(hipMemcpyAsync(w.cu, cu.data(), (n_utt + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipMemcpyAsync(w.cuk, cu.data(), n_utt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipMemcpyAsync(w.klen, kl.data(), n_utt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    std::vector<int64_t> prec;
    proj_records(m, pl, n_utt, out_ld, out_row_offsets_host, prec);
    SL_HIP(hipMemcpyAsync(w.pdesc, prec.data(), prec.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SL_HIP(hipStreamSynchronize(st));
  }
  // haloed inputs: one zero row before and after each utterance's frames (Conv1d padding=1)
  SL_HIP(hipMemsetAsync(w.convA, 0, (size_t)n_utt * (F + 2) * n_mel * sz, st));
  SL_HIP(hipMemsetAsync(w.convB, 0, (size_t)n_utt * (F + 2) * H * sz, st));
  SL_HIP(hipMemcpy2DAsync(bptr(w.convA) + (size_t)n_mel * sz, (size_t)(F + 2) * n_mel * sz, mel, (size_t)F * n_mel * sz, (size_t)F * n_mel * sz, n_utt,
                          hipMemcpyDeviceToDevice, st));
  sl_gemm_args a;
  memset(&a, 0, sizeof(a));   // conv1: out row t reads the 3*n_mel contiguous elements from haloed row t
  a.A = w.convA; a.lda = n_mel; a.strideA = (F + 2) * n_mel;
  a.W = m->conv_w[1]; a.ldw = 3 * n_mel;
  a.C = bptr(w.convB) + (size_t)H * sz; a.ldc = H; a.strideC = (F + 2) * H;
  a.bias = m->conv_b[1];
  a.M = (int)F; a.N = H; a.K = 3 * n_mel; a.batch = n_utt; a.dtype = dt; a.act = SL_ACT_GELU;
  SL_TRY(sl_gemm_impl(&a, nullptr, nullptr, st));
  memset(&a, 0, sizeof(a));   // conv2 (stride 2): out row t reads haloed rows 2t .. 2t+2; + positional table after GELU
  a.A = w.convB; a.lda = 2 * (int64_t)H; a.strideA = (F + 2) * H;
  a.W = m->conv_w[2]; a.ldw = 3 * (int64_t)H;
  a.C = w.x; a.ldc = H; a.strideC = T * H;
  a.bias = m->conv_b[2];
  a.residual = m->pos_w; a.ldr = H; a.strideR = 0;
  a.M = (int)T; a.N = H; a.K = 3 * H; a.batch = n_utt; a.dtype = dt; a.act = SL_ACT_GELU;
  SL_TRY(sl_gemm_impl(&a, nullptr, nullptr, st));
  return encoder_tail(m, w, pl, n_utt, out, out_ld, out_row_offsets_host, last_hidden, st);
}

// ================================================================================================
// Llama
// ================================================================================================
// SL_MAX_DECODE_BATCH (speechllm.h): rows of one decode step (M of the weight-streaming GEMMs)

struct LlamaWs {
  void *h, *qkv, *att, *mid, *last, *part, *split;
  void *mxq = nullptr, *mxs = nullptr;   // SL_WDEC_MX_LINEAR only: the MXFP8 rows (bytes, scales) of the product being fed
  size_t split_bytes;
  float *rstd_a, *rstd_b;   // RMSNorm scales handed from the o / down projection's reduce pass to the next fused GEMM
  int32_t *tok_seq, *tok_pos, *cu, *cuk, *klen;
  int32_t* last_row;        // prefill: row of every sequence's last token (the rows lm_head reads)
};

static size_t llama_carve(const sl_llama_model* m, int64_t n_tok, int nseq, void* base, size_t cap, LlamaWs& w) {
  const size_t sz = sl_dtype_size(m->dtype);
  const int qkv_w = (m->n_heads + 2 * m->n_kv_heads) * m->head_dim;
  Carver c(base, cap);
  w.h = c.take(n_tok * m->hidden * sz);
  w.qkv = c.take(n_tok * qkv_w * sz);
  w.att = c.take(n_tok * (int64_t)m->n_heads * m->head_dim * sz);
  w.mid = c.take(n_tok * (int64_t)m->ffn * sz);
  w.last = c.take((size_t)nseq * m->hidden * sz);
  w.part = c.take(sl_attn_decode_split_ws(nseq, m->n_heads, m->n_kv_heads, m->rope_len));  // rope_len >= max_ctx
  {  // K-split partial sums of the decode GEMMs (batches above the skinny kernel's range)
    size_t sb = 0;
    const int shapes[5][2] = {{qkv_w, m->hidden}, {m->hidden, m->n_heads * m->head_dim}, {2 * m->ffn, m->hidden}, {m->hidden, m->ffn}, {m->vocab, m->hidden}};
    for (auto& sh : shapes) {
      const size_t b = sl_gemm_split_workspace_bytes(nseq, sh[0], sh[1], m->dtype);
      if (b > sb) sb = b;
    }
    w.split_bytes = sb;
    w.split = c.take(sb);
  }
  w.rstd_a = (float*)c.take((size_t)nseq * sizeof(float));
  w.rstd_b = (float*)c.take((size_t)nseq * sizeof(float));
  w.tok_seq = (int32_t*)c.take(n_tok * sizeof(int32_t));
  w.tok_pos = (int32_t*)c.take(n_tok * sizeof(int32_t));
  w.cu = (int32_t*)c.take((nseq + 2) * sizeof(int32_t));     // + 1: the shared prompt prefix is one more attention sequence in prefill
  w.cuk = (int32_t*)c.take((nseq + 1) * sizeof(int32_t));
  w.klen = (int32_t*)c.take((nseq + 1) * sizeof(int32_t));
  w.last_row = (int32_t*)c.take((size_t)nseq * sizeof(int32_t));
  if (sl_wformat_code(m) == SL_WDEC_MX_LINEAR) {      // behind everything else: the other formats keep their layout and their byte count
    int kmax = m->hidden;
    if (m->n_heads * m->head_dim > kmax) kmax = m->n_heads * m->head_dim;
    if (m->ffn > kmax) kmax = m->ffn;
    w.mxq = c.take((size_t)n_tok * kmax);
    w.mxs = c.take((size_t)n_tok * (kmax / 32));
  }
  return c.off + 256;
}

extern "C" size_t sl_llama_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq) {
  LlamaWs w;
  return llama_carve(m, n_tok, nseq, nullptr, 0, w);
}

static int llama_check(const sl_llama_model* m, const sl_kv_cache* kv) {
  SL_CHECK_ARG(m && kv && m->layers && m->embed && m->lm_head && m->final_norm && m->rope_cos && m->rope_sin, "llama: null model field");
  if (sl_kv_format(kv) != SL_KV_MODEL_DTYPE) SL_TRY(sl_kv_format_check("llama (sl_kv_cache.reserved)", sl_kv_format(kv), m->dtype, m->head_dim));
  SL_CHECK_ARG(m->head_dim == 128, "llama: head_dim %d not built (128)", m->head_dim);
  SL_CHECK_ARG(kv->k_cache && kv->v_cache && kv->slots > 0 && kv->max_ctx > 0, "llama: bad kv cache");
  SL_CHECK_ARG(kv->shared_prefix >= 0 && kv->shared_prefix <= kv->max_ctx, "llama: kv cache shared_prefix %d outside [0, max_ctx=%d]", kv->shared_prefix, kv->max_ctx);
  SL_CHECK_ARG(kv->max_ctx <= m->rope_len, "llama: max_ctx %d exceeds the rope table (%d)", kv->max_ctx, m->rope_len);
  return 0;
}

// MX linears (gemm_mx.hip)
int sl_gemm_mx_impl(const sl_gemm_mx_args* a, hipStream_t st);
int sl_mxfp8_quantize_rows_impl(const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype, hipStream_t st);

// one product of a decoder layer on the row-major weight set: C = act(A . W^T) + res.  Format 5: quantise the M input rows (one launch), then the MX product
// on the weight image; every other format: the call it always was, launch for launch.
static int layer_gemm(const sl_llama_model* m, const LlamaWs& w, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const void* res,
                      int64_t ldr, int M, int N, int K, int act, hipStream_t st) {
  if (sl_wformat_code(m) != SL_WDEC_MX_LINEAR) return gemm(m->dtype, A, lda, W, ldw, C, ldc, nullptr, res, ldr, M, N, K, act, 0, st);
  SL_TRY(sl_mxfp8_quantize_rows_impl(A, lda, w.mxq, w.mxs, M, K, m->dtype, st));
  sl_gemm_mx_args a;
  memset(&a, 0, sizeof(a));
  a.Aq = w.mxq; a.lda = K; a.a_scales = w.mxs; a.W = W; a.C = C; a.ldc = ldc; a.residual = res; a.ldr = ldr;
  a.M = M; a.N = N; a.K = K; a.dtype = m->dtype; a.act = act; a.out_f32 = 0;
  return sl_gemm_mx_impl(&a, st);
}

// The model's weight format against what `entry` (SL_ENTRY_*) runs: checked by every entry of the runtime at the point it always was, before any launch.
// rows: the rows of the entry's decode steps; 0 where it runs none (prefill, scoring) — those read the row-major weights, so the decode-image
// formats, and a code that names no format, pass.  MX linears are checked at every row count: their images ARE the row-major weights.
static int llama_wformat_check(const char* who, const sl_llama_model* m, int rows, unsigned entry) {
  const SlWFormat* f = sl_wformat(sl_wformat_code(m));
  if (f && !(f->runs & entry)) {
    sl_set_error("%s: MX linears (sl_llama_model.reserved = 5, format 5) are not built for this entry: prefill, decode step and sl_generate* run them", who);
    return SL_ERR_UNSUPPORTED;
  }
  if (rows <= 0 && (!f || f->dec_images)) return 0;
  SL_CHECK_ARG(f, "%s: unknown decode-weight format %d (sl_llama_model.reserved: " SL_WFORMAT_LIST ")", who, sl_wformat_code(m));
  if (f->code == SL_WDEC_MODEL_DTYPE) return 0;
  const char* kind = f->dec_images ? " decode weights" : "";
  if (m->dtype == SL_F32) {
    sl_set_error("%s: %s%s are built for bf16 / fp16 models, not float32 (the parity mode)", who, f->name, kind);
    return SL_ERR_UNSUPPORTED;
  }
  if (f->dec_images) SL_CHECK_ARG(m->dec_fused_norm == 1 && m->lm_head_dec, "%s: %s decode weights need dec_fused_norm = 1 and lm_head_dec", who, f->name);
  else SL_CHECK_ARG(sl_is16(m->dtype), "%s: unknown dtype %d", who, m->dtype);
  for (int l = 0; l < m->n_layers; ++l) {
    const sl_llama_layer& L = m->layers[l];
    const bool dec = L.wqkv_dec && L.wo_dec && L.wgu_dec && L.wdown_dec, no_dec = !L.wqkv_dec && !L.wo_dec && !L.wgu_dec && !L.wdown_dec;
    if (f->dec_images) SL_CHECK_ARG(dec, "%s: %s decode weights: layer %d has a null *_dec image", who, f->name, l);
    else {
      SL_CHECK_ARG(L.wqkv && L.wo && L.wgu && L.wdown, "%s: %s: layer %d has a null weight image", who, f->name, l);
      SL_CHECK_ARG(no_dec, "%s: %s: layer %d has a non-null *_dec pointer (the four must be NULL)", who, f->name, l);
    }
  }
  const int ks[3] = {m->hidden, m->n_heads * m->head_dim, m->ffn};
  for (int k : ks)
    if (k % f->k_multiple != 0) {
      sl_set_error("%s: %s%s need every reduction length to be a multiple of %d (hidden=%d, n_heads*head_dim=%d, ffn=%d)", who, f->name, kind, f->k_multiple, ks[0], ks[1], ks[2]);
      return SL_ERR_UNSUPPORTED;
    }
  if (f->max_rows && sl_family_rows(rows) > f->max_rows()) {
    sl_set_error("%s: %s decode weights run up to %s() = %d rows per decode step, not %d (use the 16-bit decode copies)", who, f->name, f->max_rows_name, f->max_rows(),
                 sl_family_rows(rows));
    return SL_ERR_UNSUPPORTED;
  }
  return 0;
}

// K / V rows are head_dim elements of the cache's own element size: 1 byte in the e4m3 format, the model dtype's otherwise
static inline size_t kv_elem_bytes(const sl_llama_model* m, const sl_kv_cache* kv) { return sl_kv_elem_size(sl_kv_format(kv), m->dtype); }
static inline size_t kv_layer_bytes(const sl_llama_model* m, const sl_kv_cache* kv) {
  return (size_t)kv->slots * m->n_kv_heads * kv->max_ctx * m->head_dim * kv_elem_bytes(m, kv);
}

extern "C" size_t sl_kv_cache_bytes(const sl_llama_model* m, int32_t slots, int32_t max_ctx, int32_t kv_format) {
  if (!m || slots <= 0 || max_ctx <= 0 || m->n_layers <= 0) { sl_set_error("sl_kv_cache_bytes: bad arguments"); return 0; }
  if (sl_kv_format_check("sl_kv_cache_bytes", kv_format, m->dtype, m->head_dim) != 0) return 0;
  return (size_t)m->n_layers * slots * m->n_kv_heads * max_ctx * m->head_dim * sl_kv_elem_size(kv_format, m->dtype);
}

// ---- shared prompt prefix in prefill (sl_kv_cache.shared_prefix = P): the P rows every sequence opens with are computed once ----
// rows of the packed prompt buffer gathered by an index list (16-byte pieces; dst and src do not overlap)
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int32_t* __restrict__ map,
                                                          int64_t n_rows, int row_vec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows * row_vec) return;
  const int64_t r = i / row_vec;
  const int c = (int)(i - r * row_vec);
  dst[i] = src[(int64_t)map[r] * row_vec + c];
}
static int gather_rows(const void* src, void* dst, const int32_t* map, int64_t n_rows, size_t row_bytes, hipStream_t st) {
  const int row_vec = (int)(row_bytes / 16);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n_rows * row_vec + 255) / 256)), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, map, n_rows, row_vec);
  SL_CHECK_LAUNCH("gather_rows");
  return 0;
}
// K / V rows [0, P) of slot 0 copied to slots 1 .. nseq-1 of one layer's cache: grid (P, n_kv, nseq - 1); lanes 0..31 move the K row,
// 32..63 the V row, 16 bytes each (rows of 256 B in bf16, 512 B in fp32)
__global__ __launch_bounds__(64) void kv_prefix_broadcast_kernel(uint4* __restrict__ kc, uint4* __restrict__ vc, int nkv, int max_ctx, int row_vec) {
  const int pos = blockIdx.x, h = blockIdx.y, s = blockIdx.z + 1;
  uint4* c = threadIdx.x < 32 ? kc : vc;
  const int lane = threadIdx.x & 31;
  if (lane >= row_vec) return;
  const int64_t src = ((int64_t)h * max_ctx + pos) * row_vec + lane;
  c[((int64_t)s * nkv * max_ctx) * row_vec + src] = c[src];
}

// ---- weight prefetch beside the decode chain (small batches) ----
// At batch 1 a decode step is a chain of ~140 dependent launches that each stream their weights once: HBM idles through every ramp, tail and
// launch gap (r04: lm_head reads at 6.6 TB/s, qkv at 3.0, o at 3.4; 0.53 of the HBM ceiling end to end).  The captured graph therefore carries
// a second branch: while the consumer of weight matrix k runs, a prefetch kernel streams matrix k + 1 through the memory side into the
// 256 MiB Infinity Cache (plain loads allocate there; guide: a table stays resident while table + traffic between uses < 256 MiB, and is
// then read at ~8.6 TB/s against ~6.1 from HBM).  The branch is a hint: it writes nothing, nothing waits for it except the end of the graph,
// and the lead is two matrices (<= 150 MB at Llama-3.2-3B).
// MEASURED (profiles/r06_j_decode_prefetch_ab.txt): the step takes 3.3 ms with the branch against 1.50 ms without, at every batch 1..26, with
// non-temporal and with default-policy weight loads alike — the second branch of the graph does not run beside the chain for free (its long-lived
// blocks and the chain's short launches share one dispatcher, and the bytes are fetched twice).  Kept behind SL_DECODE_PREFETCH=1 (default 0) as the
// record of the experiment.
__global__ __launch_bounds__(256) void weight_prefetch_kernel(const uint4* __restrict__ w, size_t n16, uint32_t* __restrict__ sink) {
  uint32_t acc = 0;
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 7 * stride < n16; i += 8 * stride) {       // eight 16-byte loads in flight per lane
    uint4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = w[i + u * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
  }
  for (; i < n16; i += stride) { const uint4 v = w[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
  if (acc == 0x9e3779b9u && sink) *sink = acc;          // (practically never: keeps the loads alive)
}

struct DecodePrefetch {
  hipStream_t main = nullptr, side = nullptr;
  hipEvent_t ev = nullptr;
  uint32_t* sink = nullptr;
  bool on = false;
  // called right before the consumer of the CURRENT matrix is launched on `main`: the prefetch of `next` starts when everything launched so far has
  // completed, i.e. together with that consumer
  int ahead(const void* next, size_t bytes) {
    if (!on || !next || bytes < (1u << 20)) return 0;
    SL_HIP(hipEventRecord(ev, main));
    SL_HIP(hipStreamWaitEvent(side, ev, 0));
    const size_t n16 = bytes / 16;
    int blocks = (int)((n16 + 256 * 8 - 1) / (256 * 8));
    blocks = blocks > 512 ? 512 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(weight_prefetch_kernel, dim3(blocks), dim3(256), 0, side, (const uint4*)next, n16, sink);
    SL_CHECK_LAUNCH("weight_prefetch");
    return 0;
  }
  int join() {
    if (!on) return 0;
    SL_HIP(hipEventRecord(ev, side));
    SL_HIP(hipStreamWaitEvent(main, ev, 0));
    return 0;
  }
};
static thread_local DecodePrefetch* g_prefetch = nullptr;      // set by sl_generate around the capture of a small-batch decode graph

// Where a decode step's rows keep their K / V (sl_generate_n with several answers per prompt; all zero for every other caller): the rows' slots
// start at slot row_slot0 of the cache — the K / V append, the attention's "own slot" and compaction all work on the per-layer base
// shifted by that many slots — and, with `groups` set, a row's positions below prefix_len[row] are read from its record's prompt slot
// by the grouped attention (sl_attn_decode_grouped) instead of from a copy in its own slot.
struct DecodeAttn {
  int row_slot0 = 0;
  const sl_attn_group* groups = nullptr;      // device, B records rebuilt at every compaction (NULL: the copy path)
  const int32_t* prefix_len = nullptr;        // device, per row
  void* gws = nullptr;                        // the grouped attention's records
};

// one decoder layer over `n` token rows; attention chosen by `decode`
// decode GEMM on the fragment-packed weights, optionally absorbing the preceding RMSNorm / RoPE+KV-append
static int dec_gemm(const sl_llama_model* m, const LlamaWs& w, const void* A, int64_t lda, const void* Wp, void* C, int64_t ldc, const void* res,
                    int M, int N, int K, int act, int out_f32, const sl_gemm_fused* fx_in, hipStream_t st, const float* rstd_in = nullptr,
                    float* rstd_out = nullptr, void* norm_out = nullptr, const void* norm_gain = nullptr) {
  sl_gemm_fused fxl;
  if (fx_in) fxl = *fx_in; else memset(&fxl, 0, sizeof(fxl));
  fxl.split_ws = w.split; fxl.split_ws_bytes = w.split_bytes;
  fxl.rstd_in = rstd_in; fxl.rstd_out = rstd_out; fxl.rms_eps = m->rms_eps;
  fxl.norm_out = norm_out; fxl.norm_gain = norm_gain;
  const sl_gemm_fused* fx = &fxl;
  sl_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.lda = lda; a.W = Wp; a.ldw = K; a.C = C; a.ldc = ldc; a.residual = res; a.ldr = ldc;
  a.M = M; a.N = N; a.K = K; a.batch = 1; a.dtype = m->dtype; a.act = act; a.out_f32 = out_f32;
  const SlWFormat* f = sl_wformat(sl_wformat_code(m));
  a.w_layout = f && f->w_layout >= 0 ? f->w_layout : SL_W_PACKED;      // a format without *_dec images of its own decodes lm_head on the 16-bit lm_head_dec
  return sl_gemm_impl(&a, fx, nullptr, st);
}

// one decoder layer over `n` token rows; attention chosen by `decode`
// rstd_chain (decode): the o / down projections run K-split, so their reduce passes emit the RMSNorm scale of the rows
// they store and the next fused GEMM (gate/up, next layer's qkv, lm_head) takes it instead of recomputing it per block;
// rstd_qkv = scale of x on entry (NULL: this layer's qkv takes its own statistics)
// prefix_bcast = P > 0 (prefill with a shared prompt prefix): the P prefix rows were appended to slot 0 only and are copied to the other
// bcast_slots - 1 slots before attention, in which the prefix is one more sequence (nseq counts it)
// tail_rows (prefill's final layer, n_tail device indices): the only rows of this layer's output that anything reads.  Norm, qkv, RoPE /
// append and attention run over all n rows (the cache needs every K / V row); the n_tail rows of the attention output and of x are then
// gathered, and o + residual, norm, gate/up and down + residual run on those alone, their result left in w.last (x is not updated).
// The products stay pinned to the family of n rows, so a row goes through the kernel — and the K order — it goes through in the full pass.
static int llama_layer(const sl_llama_model* m, const sl_kv_cache* kv, int l, void* x, int64_t n, LlamaWs& w, bool decode, int nseq,
                       int max_qlen, const int32_t* ctx_len_dev, hipStream_t st, bool rstd_chain = false, const float* rstd_qkv = nullptr,
                       int prefix_bcast = 0, int bcast_slots = 0, bool rstd_pass = false, const int32_t* tail_rows = nullptr, int n_tail = 0,
                       const DecodeAttn* da = nullptr, const int32_t* past_len_dev = nullptr) {
  const sl_llama_layer& L = m->layers[l];
  const int dt = m->dtype, H = m->hidden, D = m->head_dim, nh = m->n_heads, nkv = m->n_kv_heads;
  const int qkv_w = (nh + 2 * nkv) * D;
  void* kc = bptr(kv->k_cache) + (size_t)l * kv_layer_bytes(m, kv);
  void* vc = bptr(kv->v_cache) + (size_t)l * kv_layer_bytes(m, kv);
  const void *kc0 = kc, *vc0 = vc;       // slot 0 of the layer: the grouped attention's prompt slots are indexed from here
  if (decode && da && da->row_slot0 > 0) {
    const size_t off = (size_t)da->row_slot0 * nkv * kv->max_ctx * D * kv_elem_bytes(m, kv);
    kc = bptr(kc) + off; vc = bptr(vc) + off;
  }
  const float scale = 1.0f / sqrtf((float)D);
  auto decode_attn = [&](int64_t q_stride) -> int {
    if (da && da->groups)
      return sl_attn_decode_grouped_impl(w.qkv, q_stride, kc0, vc0, w.att, da->gws, ctx_len_dev, 1, da->prefix_len, da->groups, (int)n, da->row_slot0, nh, nkv,
                                         D, kv->max_ctx, scale, dt, sl_kv_format(kv), st);
    return sl_attn_decode_split_impl(w.qkv, q_stride, kc, vc, w.att, w.part, ctx_len_dev, 1, (int)n, nh, nkv, D, kv->max_ctx, scale, dt, st, 1, kv->shared_prefix, sl_kv_format(kv));
  };
  if (decode && L.wqkv_dec && L.wo_dec && L.wgu_dec && L.wdown_dec) {
    // 5-6 launches per layer: [norm+]qkv+rope+append | attention (split + merge) | o+res | [norm+]gate/up+silu.mul | down+res
    sl_gemm_fused fx;
    memset(&fx, 0, sizeof(fx));
    fx.fuse_rms = m->dec_fused_norm; fx.rms_eps = m->rms_eps;
    fx.rope_cos = m->rope_cos; fx.rope_sin = m->rope_sin; fx.tok_pos = ctx_len_dev; fx.tok_seq = w.tok_seq;
    fx.k_cache = kc; fx.v_cache = vc; fx.n_heads = nh; fx.n_kv_heads = nkv; fx.max_ctx = kv->max_ctx; fx.reserved = sl_kv_format(kv);
    // small-batch graphs: the prefetch branch runs two matrices ahead of the chain (DecodePrefetch): released where a consumer is launched
    DecodePrefetch* pf = g_prefetch;
    const size_t esz = sl_dtype_size(dt);
    const SlWFormat* wf = sl_wformat(sl_wformat_code(m));
    auto wbytes = [&](int N, int K) -> size_t { return sl_wformat_bytes(wf, N, K, esz); };      // weight images: elements + scales
    const size_t b_qkv = wbytes(qkv_w, H), b_o = wbytes(H, nh * D), b_gu = wbytes(2 * m->ffn, H), b_down = wbytes(H, m->ffn);
    const sl_llama_layer* Ln = (l + 1 < m->n_layers) ? &m->layers[l + 1] : nullptr;
    if (pf && l == 0) { SL_TRY(pf->ahead(L.wqkv_dec, b_qkv)); SL_TRY(pf->ahead(L.wo_dec, b_o)); }
    if (pf) SL_TRY(pf->ahead(L.wgu_dec, b_gu));                       // ... while qkv, attention and o run
    const void* a_in = x;
    if (!m->dec_fused_norm) { SL_TRY(sl_rmsnorm(x, w.h, L.norm1, n, H, m->rms_eps, dt, (sl_stream)st)); a_in = w.h; }
    // rstd_pass (rows whose o / down projections run unsplit: no reduce pass forms the RMSNorm scales): one read of x leaves them, so
    // that the gain-folded products stay on the 256 x 128 streaming blocks instead of taking the statistics per block themselves
    if (rstd_pass) { SL_TRY(sl_rmsnorm_rstd_impl(x, nullptr, nullptr, w.rstd_b, n, H, m->rms_eps, dt, st)); rstd_qkv = w.rstd_b; }
    SL_TRY(dec_gemm(m, w, a_in, H, L.wqkv_dec, w.qkv, (int64_t)nh * D, nullptr, (int)n, qkv_w, H, SL_ACT_ROPE_KV, 0, &fx, st, rstd_qkv));
    SL_TRY(decode_attn((int64_t)nh * D));
    // Above ~900 rows gate/up runs on the row-major 256 x 256 tiles (the prefill kernel): at 1 024 rows it is 4 x 64 = 256 tiles, one per
    // CU, 78-81 us against 99 us on the 256 x 128 streaming block (tools/time_decode_tiled.py; in the graph: profiles/r04_l_*).  Its input
    // must then be normalised: the o projection's reduce pass, which already forms each row's RMSNorm scale, writes the normalised rows
    // beside x (sl_gemm_fused.norm_out) — a separate sl_rmsnorm launch costs 11.5 us per layer in the graph and ate the gain, and o itself
    // stays on the streaming form (27 + 11 us against 47 us on the 128 x 128 tiles its 48 big tiles fall back to).  SL_DECODE_TILED=0: off.
    if (pf) SL_TRY(pf->ahead(L.wdown_dec, b_down));                   // ... while o and gate/up run
    if (rstd_pass) {
      SL_TRY(dec_gemm(m, w, w.att, (int64_t)nh * D, L.wo_dec, x, H, x, (int)n, H, nh * D, SL_ACT_NONE, 0, nullptr, st));
      if (L.wgu && sl_env().decode_tiled) {     // gate/up on the row-major 256 x 256 tiles (2 048 rows: 512 tiles = two whole rounds of the chip)
        SL_TRY(sl_rmsnorm(x, w.h, L.norm2, n, H, m->rms_eps, dt, (sl_stream)st));
        SL_TRY(gemm(dt, w.h, H, L.wgu, H, w.mid, m->ffn, nullptr, nullptr, 0, (int)n, 2 * m->ffn, H, SL_ACT_SILU_MUL, 0, st));
      } else {
        SL_TRY(sl_rmsnorm_rstd_impl(x, nullptr, nullptr, w.rstd_a, n, H, m->rms_eps, dt, st));
        sl_gemm_fused fn;
        memset(&fn, 0, sizeof(fn));
        fn.fuse_rms = 1; fn.rms_eps = m->rms_eps;
        SL_TRY(dec_gemm(m, w, x, H, L.wgu_dec, w.mid, m->ffn, nullptr, (int)n, 2 * m->ffn, H, SL_ACT_SILU_MUL, 0, &fn, st, w.rstd_a));
      }
    } else if (sl_family_rows((int)n) > 896 && sl_is16(dt) && L.wgu && rstd_chain && sl_env().decode_tiled) {
      SL_TRY(dec_gemm(m, w, w.att, (int64_t)nh * D, L.wo_dec, x, H, x, (int)n, H, nh * D, SL_ACT_NONE, 0, nullptr, st, nullptr, w.rstd_a, w.h, L.norm2));
      SL_TRY(gemm(dt, w.h, H, L.wgu, H, w.mid, m->ffn, nullptr, nullptr, 0, (int)n, 2 * m->ffn, H, SL_ACT_SILU_MUL, 0, st));
    } else {
      SL_TRY(dec_gemm(m, w, w.att, (int64_t)nh * D, L.wo_dec, x, H, x, (int)n, H, nh * D, SL_ACT_NONE, 0, nullptr, st, nullptr,
                      rstd_chain ? w.rstd_a : nullptr));
      sl_gemm_fused fn;
      memset(&fn, 0, sizeof(fn));
      fn.fuse_rms = m->dec_fused_norm; fn.rms_eps = m->rms_eps;
      a_in = x;
      if (pf && Ln) SL_TRY(pf->ahead(Ln->wqkv_dec, b_qkv));           // ... while gate/up and down run
      if (!m->dec_fused_norm) { SL_TRY(sl_rmsnorm(x, w.h, L.norm2, n, H, m->rms_eps, dt, (sl_stream)st)); a_in = w.h; }
      SL_TRY(dec_gemm(m, w, a_in, H, L.wgu_dec, w.mid, m->ffn, nullptr, (int)n, 2 * m->ffn, H, SL_ACT_SILU_MUL, 0, &fn, st,
                      rstd_chain ? w.rstd_a : nullptr));
    }
    if (pf && Ln) SL_TRY(pf->ahead(Ln->wo_dec, b_o));
    SL_TRY(dec_gemm(m, w, w.mid, m->ffn, L.wdown_dec, x, H, x, (int)n, H, m->ffn, SL_ACT_NONE, 0, nullptr, st, nullptr,
                    rstd_chain ? w.rstd_b : nullptr));
    return 0;
  }
  SL_TRY(sl_rmsnorm(x, w.h, L.norm1, n, H, m->rms_eps, dt, (sl_stream)st));
  SL_TRY(layer_gemm(m, w, w.h, H, L.wqkv, H, w.qkv, qkv_w, nullptr, 0, (int)n, qkv_w, H, SL_ACT_NONE, st));
  SL_TRY(sl_rope_kv_append_ex(w.qkv, kc, vc, w.tok_seq, decode ? ctx_len_dev : w.tok_pos, m->rope_cos, m->rope_sin, n, nh, nkv, D, kv->max_ctx,
                              dt, sl_kv_format(kv), (sl_stream)st));
  if (decode) {
    SL_TRY(decode_attn(qkv_w));
  } else {
    if (prefix_bcast > 0 && bcast_slots > 1) {     // (not reached with e4m3 rows: sl_llama_prefill switches the dedupe off there; the row size is the cache's all the same)
      const int row_vec = (int)(D * kv_elem_bytes(m, kv) / 16);
      SL_CHECK_ARG(row_vec <= 32 && (D * kv_elem_bytes(m, kv)) % 16 == 0, "llama: shared prefix broadcast needs K / V rows of <= 512 bytes");
      hipLaunchKernelGGL(kv_prefix_broadcast_kernel, dim3(prefix_bcast, nkv, bcast_slots - 1), dim3(64), 0, st, (uint4*)kc, (uint4*)vc, nkv, kv->max_ctx, row_vec);
      SL_CHECK_LAUNCH("kv_prefix_broadcast");
    }
    sl_attn_args a;
    memset(&a, 0, sizeof(a));
    a.q = w.qkv; a.q_row_stride = qkv_w; a.q_head_stride = D;
    a.k = kc; a.k_row_stride = D; a.k_head_stride = (int64_t)kv->max_ctx * D;
    a.v = vc; a.v_row_stride = D; a.v_head_stride = (int64_t)kv->max_ctx * D;
    a.out = w.att; a.o_row_stride = (int64_t)nh * D; a.o_head_stride = D;
    a.cu_q = w.cu; a.cu_k = w.cuk; a.klen = w.klen;
    if (sl_kv_format(kv) == SL_KV_FP8_E4M3) {
      // e4m3 cache: the prompt attends the unquantised keys — the rotated K rows sl_rope_kv_append_ex left in qkv and the V rows beside
      // them (same values, same key order as the 16-bit cache gives: the prefill logits are those of the 16-bit mode, bit for bit)
      const size_t esz = sl_dtype_size(dt);
      a.k = bptr(w.qkv) + (size_t)nh * D * esz; a.k_row_stride = qkv_w; a.k_head_stride = D;
      a.v = bptr(w.qkv) + (size_t)(nh + nkv) * D * esz; a.v_row_stride = qkv_w; a.v_head_stride = D;
      a.cu_k = w.cu;
    }
    a.nseq = nseq; a.max_qlen = max_qlen; a.n_heads = nh; a.n_kv_heads = nkv; a.head_dim = D; a.causal = 1; a.dtype = dt; a.scale = scale;
    // continued prefill on an e4m3 cache (past_len_dev set, w.klen = the NEW key counts, w.cuk = each slot's first cache row): the past keys exist
    // only as the cache's bytes — the values decode reads — and the new ones are attended unquantised out of qkv, as above
    if (sl_kv_format(kv) == SL_KV_FP8_E4M3 && past_len_dev) SL_TRY(sl_attn_fwd_past(&a, kc, vc, past_len_dev, w.cuk, kv->max_ctx, sl_kv_format(kv), (sl_stream)st));
    else SL_TRY(sl_attn_fwd(&a, (sl_stream)st));
  }
  if (tail_rows && !decode) {
    const size_t esz = sl_dtype_size(dt);
    void* att_t = w.qkv;      // q / k / v are consumed: the gathered attention rows take their place, the normalised rows take w.h
    SL_TRY(gather_rows(w.att, att_t, tail_rows, n_tail, (size_t)nh * D * esz, st));
    SL_TRY(gather_rows(x, w.last, tail_rows, n_tail, (size_t)H * esz, st));
    SlFamilyPin pin((int)n);
    SL_TRY(layer_gemm(m, w, att_t, (int64_t)nh * D, L.wo, (int64_t)nh * D, w.last, H, w.last, H, n_tail, H, nh * D, SL_ACT_NONE, st));
    SL_TRY(sl_rmsnorm(w.last, w.h, L.norm2, n_tail, H, m->rms_eps, dt, (sl_stream)st));
    SL_TRY(layer_gemm(m, w, w.h, H, L.wgu, H, w.mid, m->ffn, nullptr, 0, n_tail, 2 * m->ffn, H, SL_ACT_SILU_MUL, st));
    SL_TRY(layer_gemm(m, w, w.mid, m->ffn, L.wdown, m->ffn, w.last, H, w.last, H, n_tail, H, m->ffn, SL_ACT_NONE, st));
    return 0;
  }
  SL_TRY(layer_gemm(m, w, w.att, (int64_t)nh * D, L.wo, (int64_t)nh * D, x, H, x, H, (int)n, H, nh * D, SL_ACT_NONE, st));
  SL_TRY(sl_rmsnorm(x, w.h, L.norm2, n, H, m->rms_eps, dt, (sl_stream)st));
  SL_TRY(layer_gemm(m, w, w.h, H, L.wgu, H, w.mid, m->ffn, nullptr, 0, (int)n, 2 * m->ffn, H, SL_ACT_SILU_MUL, st));
  SL_TRY(layer_gemm(m, w, w.mid, m->ffn, L.wdown, m->ffn, x, H, x, H, (int)n, H, m->ffn, SL_ACT_NONE, st));
  return 0;
}

static inline const char* cont_name(const int32_t* past_host, const int32_t* slot_host) { return (past_host || slot_host) ? "sl_llama_prefill_cont" : "sl_llama_prefill"; }
// slot_stride: sequence s is written to cache slot s * slot_stride (1 for every public caller; the beam search prefills each prompt once,
// into the slot of its first beam — without the shared-prefix dedupe, whose broadcast assumes consecutive slots)
static int llama_prefill_impl(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                              float* logits, int32_t* ctx_len_dev, void* hidden_taps, void* workspace, size_t workspace_bytes,
                              sl_stream stream, int slot_stride, const int32_t* past_host = nullptr, const int32_t* slot_host = nullptr) {
  SL_TRY(llama_check(m, kv));
  SL_TRY(llama_wformat_check(cont_name(past_host, slot_host), m, 0, SL_ENTRY_PREFILL));
  // continued prefill (sl_llama_prefill_cont): sequence s already holds positions [0, past_host[s]) of cache slot slot_host[s].  All-zero pasts on
  // the identity slots ARE the plain call: every line below then runs as it did
  if (past_host && nseq > 0) {
    bool any = false;
    for (int s = 0; s < nseq; ++s) {
      SL_CHECK_ARG(past_host[s] >= 0, "sl_llama_prefill_cont: past length %d of sequence %d is negative", past_host[s], s);
      any = any || past_host[s] > 0;
    }
    if (!any) past_host = nullptr;
  }
  const bool cont = past_host || slot_host;
  if (cont) SL_CHECK_ARG(!hidden_taps && slot_stride == 1, "sl_llama_prefill_cont: hidden_taps are not offered");
  SL_CHECK_ARG(x && cu_seqlens_host && logits && ctx_len_dev && workspace && nseq > 0 && slot_stride >= 1 && (int64_t)nseq * slot_stride <= kv->slots,
               "sl_llama_prefill: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_tok = cu_seqlens_host[nseq];
  const int dt = m->dtype, H = m->hidden;
  const size_t sz = sl_dtype_size(dt);
  LlamaWs w;
  const size_t need = llama_carve(m, n_tok, nseq, workspace, workspace_bytes, w);
  SL_CHECK_ARG(need <= workspace_bytes, "sl_llama_prefill: workspace %zu B < required %zu B", workspace_bytes, need);
  SL_CHECK_ARG(((size_t)H * sz) % 16 == 0, "sl_llama_prefill: hidden rows must be a multiple of 16 bytes");
  std::vector<int32_t> tseq(n_tok), tpos(n_tok), cuk(nseq + 1), kl(nseq + 1), ctx(nseq), cuq(nseq + 2), last_row(nseq);
  int max_q = 0;
  // Shared prompt prefix (sl_kv_cache.shared_prefix = P, the caller's promise that rows [0, P) of every sequence are the same rows): they
  // are computed ONCE — the batch becomes [P prefix rows | tail of sequence 0 | tail of sequence 1 | ...], the prefix's K / V rows are
  // appended to slot 0 and copied to the other slots in every layer, and attention sees the prefix as one more sequence while a tail's
  // queries attend [prefix + tail] keys of their own slot (causal with klen > qlen).  Every row-wise product, RoPE at the row's own
  // position and attention over the same keys in the same order give the bits the unshared pass gives (asserted on the cache and the
  // logits).  Not with hidden_taps (they are per row of the caller's layout) or when a sequence is nothing but the prefix.
  // Not with e4m3 rows either: that prefill reads K / V from its own qkv rows, not from the cache, so there is nothing to broadcast
  // (decode still reads the positions below shared_prefix from slot 0).
  int P = (kv->shared_prefix > 0 && nseq > 1 && !hidden_taps && sl_env().prefill_share_prefix && sl_kv_format(kv) != SL_KV_FP8_E4M3 && slot_stride == 1) ? kv->shared_prefix : 0;
  if (cont) P = 0;      // the new rows are never deduplicated: the promise then only says that cache positions [0, shared_prefix) are equal, which the first call made true
  for (int s = 0; s < nseq; ++s) {
    const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
    SL_CHECK_ARG(len > 0 && len <= kv->max_ctx, "sl_llama_prefill: sequence %d length %d outside (0, max_ctx=%d]", s, len, kv->max_ctx);
    if (past_host) {      // (max_ctx <= rope_len: llama_check)
      SL_CHECK_ARG((int64_t)past_host[s] + len <= kv->max_ctx, "sl_llama_prefill_cont: sequence %d: past %d + %d new rows exceed max_ctx %d", s, past_host[s], len, kv->max_ctx);
      SL_CHECK_ARG(kv->shared_prefix <= past_host[s], "sl_llama_prefill_cont: kv cache shared_prefix %d exceeds the past length %d of sequence %d", kv->shared_prefix,
                   past_host[s], s);
    } else {
      SL_CHECK_ARG(kv->shared_prefix <= len, "sl_llama_prefill: kv cache shared_prefix %d exceeds sequence %d (%d tokens)", kv->shared_prefix, s, len);
    }
    if (len <= P) P = 0;
  }
  if (slot_host) {
    std::vector<char> used(kv->slots, 0);
    for (int s = 0; s < nseq; ++s) {
      SL_CHECK_ARG(slot_host[s] >= 0 && slot_host[s] < kv->slots, "sl_llama_prefill_cont: slot %d of sequence %d outside [0, %d)", slot_host[s], s, kv->slots);
      SL_CHECK_ARG(!used[slot_host[s]], "sl_llama_prefill_cont: slot %d is given to two sequences", slot_host[s]);
      used[slot_host[s]] = 1;
    }
  }
  std::vector<int32_t> pastv;      // cont: per sequence, for the e4m3 attention
  int64_t n_run = n_tok;       // rows the layers run over
  int nseq_attn = nseq;
  if (P > 0) {
    std::vector<int32_t> map;
    map.reserve(n_tok);
    for (int t = 0; t < P; ++t) { map.push_back(cu_seqlens_host[0] + t); }
    cuq[0] = 0; cuq[1] = P; cuk[0] = 0; kl[0] = P;
    for (int t = 0; t < P; ++t) { tseq[t] = 0; tpos[t] = t; }
    max_q = P;
    for (int s = 0; s < nseq; ++s) {
      const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s], tail = len - P;
      const int r0 = (int)map.size();
      for (int t = 0; t < tail; ++t) { map.push_back(cu_seqlens_host[s] + P + t); tseq[r0 + t] = s; tpos[r0 + t] = P + t; }
      cuq[s + 2] = r0 + tail;
      cuk[s + 1] = s * m->n_kv_heads * kv->max_ctx;
      kl[s + 1] = len; ctx[s] = len;
      last_row[s] = r0 + tail - 1;
      if (tail > max_q) max_q = tail;
    }
    n_run = (int64_t)map.size();
    nseq_attn = nseq + 1;
    // x -> compact rows: gathered into the (still unused) FFN scratch, then copied back to the head of x
    SL_HIP(hipMemcpyAsync(w.tok_pos, map.data(), n_run * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SL_TRY(gather_rows(x, w.mid, w.tok_pos, n_run, (size_t)H * sz, st));
    SL_HIP(hipMemcpyAsync(x, w.mid, (size_t)n_run * H * sz, hipMemcpyDeviceToDevice, st));
    SL_HIP(hipStreamSynchronize(st));      // `map` leaves scope / tok_pos is rewritten below
  } else if (cont) {
    // rows rotated at and appended to positions past + t of their slot.  16-bit / fp32 cache: attention over the cache, klen = past + len > qlen,
    // as the shared-prefix tails above.  e4m3: sl_attn_fwd_past takes the new key counts and the pasts apart (llama_layer)
    const bool kv8 = sl_kv_format(kv) == SL_KV_FP8_E4M3;
    pastv.resize(nseq);
    for (int s = 0; s < nseq; ++s) {
      const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s], past = past_host ? past_host[s] : 0, slot = slot_host ? slot_host[s] : s;
      for (int t = 0; t < len; ++t) { tseq[cu_seqlens_host[s] + t] = slot; tpos[cu_seqlens_host[s] + t] = past + t; }
      cuk[s] = slot * m->n_kv_heads * kv->max_ctx;
      kl[s] = kv8 ? len : past + len; ctx[s] = past + len; pastv[s] = past;
      cuq[s] = cu_seqlens_host[s];
      last_row[s] = cu_seqlens_host[s + 1] - 1;
      if (len > max_q) max_q = len;
    }
    cuq[nseq] = cu_seqlens_host[nseq];
  } else {
    for (int s = 0; s < nseq; ++s) {
      const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
      for (int t = 0; t < len; ++t) { tseq[cu_seqlens_host[s] + t] = s * slot_stride; tpos[cu_seqlens_host[s] + t] = t; }
      cuk[s] = s * slot_stride * m->n_kv_heads * kv->max_ctx;  // first cache row of the sequence (rows of D elements, head-major inside)
      kl[s] = len; ctx[s] = len;
      cuq[s] = cu_seqlens_host[s];
      last_row[s] = cu_seqlens_host[s + 1] - 1;
      if (len > max_q) max_q = len;
    }
    cuq[nseq] = cu_seqlens_host[nseq];
  }
  SL_HIP(hipMemcpyAsync(w.tok_seq, tseq.data(), n_run * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.tok_pos, tpos.data(), n_run * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.cu, cuq.data(), (nseq_attn + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.cuk, cuk.data(), nseq_attn * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.klen, kl.data(), nseq_attn * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(ctx_len_dev, ctx.data(), nseq * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.last_row, last_row.data(), nseq * sizeof(int32_t), hipMemcpyHostToDevice, st));
  // the pasts ride in the decode chain's RMSNorm-scale array, nseq 4-byte entries no prefill touches
  int32_t* past_dev = (cont && sl_kv_format(kv) == SL_KV_FP8_E4M3) ? (int32_t*)w.rstd_a : nullptr;
  if (past_dev) SL_HIP(hipMemcpyAsync(past_dev, pastv.data(), nseq * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipStreamSynchronize(st));
  // Only each sequence's last row is read after the final layer (lm_head below): without hidden_taps that layer runs everything behind
  // attention on those nseq rows alone (llama_layer tail_rows) — at 137-row prompts, 136 of 137 rows of o / gate/up / down of one layer
  // in 28.  SL_PREFILL_PRUNE_LAST=0 restores the full layer (same logits and cache, bit for bit: tests/test_prefill_prune_gpu.py).
  const bool prune = !hidden_taps && m->n_layers > 0 && sl_env().prefill_prune_last != 0;
  for (int l = 0; l < m->n_layers; ++l) {
    if (hidden_taps) SL_HIP(hipMemcpyAsync(bptr(hidden_taps) + (size_t)l * n_tok * H * sz, x, n_tok * H * sz, hipMemcpyDeviceToDevice, st));
    const bool tail = prune && l == m->n_layers - 1;
    SL_TRY(llama_layer(m, kv, l, x, n_run, w, false, nseq_attn, max_q, nullptr, st, false, nullptr, P, nseq, false, tail ? w.last_row : nullptr, nseq, nullptr, past_dev));
  }
  if (hidden_taps) {
    SL_TRY(sl_rmsnorm(x, bptr(hidden_taps) + (size_t)m->n_layers * n_tok * H * sz, m->final_norm, n_tok, H, m->rms_eps, dt, stream));
  }
  // last-token rows (one gather launch; the pruned final layer has left them in w.last already) -> final norm -> lm_head (fp32 logits)
  if (!prune) SL_TRY(gather_rows(x, w.last, w.last_row, nseq, (size_t)H * sz, st));
  SL_TRY(sl_rmsnorm(w.last, w.last, m->final_norm, nseq, H, m->rms_eps, dt, stream));
  SL_TRY(gemm(dt, w.last, H, m->lm_head, H, logits, m->vocab, nullptr, nullptr, 0, nseq, m->vocab, H, SL_ACT_NONE, 1, st));
  return 0;
}

extern "C" int sl_llama_prefill(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                                float* logits, int32_t* ctx_len_dev, void* hidden_taps, void* workspace, size_t workspace_bytes,
                                sl_stream stream) {
  return llama_prefill_impl(m, kv, x, cu_seqlens_host, nseq, logits, ctx_len_dev, hidden_taps, workspace, workspace_bytes, stream, 1);
}

extern "C" int sl_llama_prefill_cont(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, const int32_t* past_len_host,
                                     const int32_t* slot_host, int32_t nseq, float* logits, int32_t* ctx_len_dev, void* workspace, size_t workspace_bytes,
                                     sl_stream stream) {
  return llama_prefill_impl(m, kv, x, cu_seqlens_host, nseq, logits, ctx_len_dev, nullptr, workspace, workspace_bytes, stream, 1, past_len_host, slot_host);
}

// ---- teacher-forced scoring: log_softmax(lm_head(final_norm(h)))[label] for rows [start, start + n) of every sequence ----
// The prefill body without hidden_taps and without the shared-prefix dedupe (every sequence runs its own rows: a scored batch shares no
// promised prefix): the final layer runs everything behind attention on the scored rows alone (llama_layer tail_rows = all of them), the
// final RMSNorm runs over those gathered rows, and the lm_head runs in passes of row_chunk rows.  A pass of more than 64 rows leaves
// the three planes and the labels' logits (sl_gemm_top1_lse_tgt) and sl_score_finalize turns them into log-probabilities; a pass of at most
// 64 rows — a short remainder included — writes fp32 logits and sl_score_rows reads them.  The remainder of a chunked call stays pinned
// to the family of a full pass (SlFamilyPin), so its logits come out of the tiled kernel, and the K order, the full passes went through.
constexpr int SL_SCORE_ROW_CHUNK = 2048;      // default rows per lm_head pass: planes of 2 048 x 2 004 groups x 12 B = 49.3 MB at vocab 128 256
constexpr int SL_SCORE_UNFUSED_MAX = 64;      // the fused top-1 lives in the tiled kernels: sl_family_rows(M) > 64 (gemm.hip)

struct ScoreWs {
  LlamaWs w;
  void* last;            // (n_rows, H): the scored rows behind the final layer
  int32_t *rows, *offs;  // scored row of the packed batch per label; first label of each sequence (nseq + 1)
  int32_t* top1;         // (n_rows) when the caller keeps none
  float *planes, *tgt;   // [3][n_groups][pass rows] and the labels' logits of one pass
  float* logits;         // fp32 logits of one unfused pass
  int chunk, plane_rows, logit_rows;
};

static thread_local int g_score_paths = 0;      // sl_llama_score_last_paths: 1 = fp32 logits + sl_score_rows ran, 2 = the fused planes ran

static size_t score_carve(const sl_llama_model* m, int64_t n_tok, int nseq, int64_t n_rows, const sl_score_opts* o, void* base, size_t cap, ScoreWs& s) {
  const size_t sz = sl_dtype_size(m->dtype);
  const int force = o ? o->force_path : 0;
  const int64_t chunk = (o && o->row_chunk > 0) ? o->row_chunk : SL_SCORE_ROW_CHUNK;
  const int64_t pass = chunk < n_rows ? chunk : n_rows;      // the longest pass
  s.chunk = (int)chunk;
  s.plane_rows = (force != 1 && pass > SL_SCORE_UNFUSED_MAX) ? (int)pass : 0;
  s.logit_rows = force == 1 ? (int)pass : (int)(n_rows < SL_SCORE_UNFUSED_MAX ? n_rows : SL_SCORE_UNFUSED_MAX);
  const size_t head = (llama_carve(m, n_tok, nseq, base, cap, s.w) + 255) & ~(size_t)255;      // the pieces below keep the base's 256-byte alignment
  Carver c(base ? bptr(base) + head : nullptr, cap > head ? cap - head : 0);
  const int64_t ng = (m->vocab + 63) / 64;
  s.last = c.take((size_t)n_rows * m->hidden * sz);
  s.rows = (int32_t*)c.take((size_t)n_rows * sizeof(int32_t));
  s.offs = (int32_t*)c.take((size_t)(nseq + 1) * sizeof(int32_t));
  s.top1 = (int32_t*)c.take((size_t)n_rows * sizeof(int32_t));
  s.planes = (float*)c.take((size_t)3 * ng * s.plane_rows * sizeof(float));
  s.tgt = (float*)c.take((size_t)s.plane_rows * sizeof(float));
  s.logits = (float*)c.take((size_t)s.logit_rows * m->vocab * sizeof(float));
  return head + c.off + 256;
}

static bool score_opts_ok(const sl_score_opts* o) { return !o || (o->row_chunk >= 0 && o->force_path >= 0 && o->force_path <= 2); }

extern "C" size_t sl_llama_score_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int64_t n_rows, const sl_score_opts* opts) {
  if (!m || n_tok <= 0 || nseq <= 0 || n_rows <= 0 || n_rows > n_tok || n_tok > 0x7fffffff || !score_opts_ok(opts)) {
    sl_set_error("sl_llama_score_workspace_bytes: bad arguments (n_tok=%lld nseq=%d n_rows=%lld row_chunk=%d force_path=%d)", (long long)n_tok, nseq, (long long)n_rows,
                 opts ? opts->row_chunk : 0, opts ? opts->force_path : 0);
    return 0;
  }
  ScoreWs s;
  return score_carve(m, n_tok, nseq, n_rows, opts, nullptr, 0, s);
}

extern "C" int32_t sl_llama_score_last_paths(void) { return g_score_paths; }

extern "C" int sl_llama_score(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                              const int32_t* score_start_host, const int32_t* n_score_host, const int32_t* labels_dev, float* logprob_dev, int32_t* top1_dev,
                              float* seq_sum_dev, int32_t* seq_counted_dev, int32_t* seq_top1_dev, const sl_score_opts* opts, void* workspace,
                              size_t workspace_bytes, sl_stream stream) {
  // every check comes before the first launch
  SL_TRY(llama_check(m, kv));
  SL_TRY(llama_wformat_check("sl_llama_score", m, 0, SL_ENTRY_SCORE));
  SL_CHECK_ARG(x && cu_seqlens_host && score_start_host && n_score_host && labels_dev && logprob_dev && workspace, "sl_llama_score: null pointer");
  SL_CHECK_ARG(nseq > 0, "sl_llama_score: nseq=%d", nseq);
  SL_CHECK_ARG((seq_sum_dev != nullptr) == (seq_counted_dev != nullptr) && (seq_sum_dev != nullptr) == (seq_top1_dev != nullptr),
               "sl_llama_score: seq_sum_dev, seq_counted_dev and seq_top1_dev come all three or none (%s, %s, %s)", seq_sum_dev ? "set" : "NULL",
               seq_counted_dev ? "set" : "NULL", seq_top1_dev ? "set" : "NULL");
  SL_CHECK_ARG(!opts || opts->row_chunk >= 0, "sl_llama_score: row_chunk %d is negative", opts ? opts->row_chunk : 0);
  SL_CHECK_ARG(!opts || (opts->force_path >= 0 && opts->force_path <= 2), "sl_llama_score: force_path %d outside [0, 2]", opts ? opts->force_path : 0);
  if (nseq > kv->slots) {
    sl_set_error("sl_llama_score: %d sequences need %d cache slots, the kv cache has %d", nseq, nseq, kv->slots);
    return SL_ERR_UNSUPPORTED;
  }
  int64_t n_rows = 0;
  int max_q = 0;
  for (int s = 0; s < nseq; ++s) {
    const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
    SL_CHECK_ARG(len > 0, "sl_llama_score: sequence %d length %d outside (0, max_ctx=%d]", s, len, kv->max_ctx);
    if (len > kv->max_ctx) {
      sl_set_error("sl_llama_score: sequence %d length %d outside (0, max_ctx=%d]", s, len, kv->max_ctx);
      return SL_ERR_UNSUPPORTED;
    }
    const int st0 = score_start_host[s], ns = n_score_host[s];
    SL_CHECK_ARG(ns >= 0, "sl_llama_score: n_score %d of sequence %d is negative", ns, s);
    SL_CHECK_ARG(st0 >= 0, "sl_llama_score: score_start %d of sequence %d is negative", st0, s);
    SL_CHECK_ARG((int64_t)st0 + ns <= len, "sl_llama_score: sequence %d: rows [%d, %d + %d) leave its %d rows", s, st0, st0, ns, len);
    n_rows += ns;
    if (len > max_q) max_q = len;
  }
  SL_CHECK_ARG(n_rows > 0, "sl_llama_score: nothing to score (sum of n_score is 0)");
  const int64_t n_tok = cu_seqlens_host[nseq];
  const int dt = m->dtype, H = m->hidden, V = m->vocab;
  const size_t sz = sl_dtype_size(dt);
  SL_CHECK_ARG(((size_t)H * sz) % 16 == 0, "sl_llama_score: hidden rows must be a multiple of 16 bytes");
  ScoreWs sw;
  const size_t need = score_carve(m, n_tok, nseq, n_rows, opts, workspace, workspace_bytes, sw);
  SL_CHECK_ARG(need <= workspace_bytes, "sl_llama_score: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  LlamaWs& w = sw.w;
  g_score_paths = 0;
  std::vector<int32_t> tseq(n_tok), tpos(n_tok), cuk(nseq), kl(nseq), cuq(nseq + 1), rows(n_rows), offs(nseq + 1);
  int64_t at = 0;
  for (int s = 0; s < nseq; ++s) {
    const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
    for (int t = 0; t < len; ++t) { tseq[cu_seqlens_host[s] + t] = s; tpos[cu_seqlens_host[s] + t] = t; }
    cuk[s] = s * m->n_kv_heads * kv->max_ctx;
    kl[s] = len;
    cuq[s] = cu_seqlens_host[s];
    offs[s] = (int32_t)at;
    for (int j = 0; j < n_score_host[s]; ++j) rows[at++] = cu_seqlens_host[s] + score_start_host[s] + j;
  }
  cuq[nseq] = cu_seqlens_host[nseq];
  offs[nseq] = (int32_t)at;
  SL_HIP(hipMemcpyAsync(w.tok_seq, tseq.data(), n_tok * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.tok_pos, tpos.data(), n_tok * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.cu, cuq.data(), (nseq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.cuk, cuk.data(), nseq * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(w.klen, kl.data(), nseq * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(sw.rows, rows.data(), n_rows * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(sw.offs, offs.data(), (nseq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipStreamSynchronize(st));      // the one host synchronisation prefill has too: the host vectors leave scope
  w.last = sw.last;                       // the tail of the final layer holds every scored row, not one per sequence
  for (int l = 0; l < m->n_layers; ++l) {
    const bool tail = l == m->n_layers - 1;
    SL_TRY(llama_layer(m, kv, l, x, n_tok, w, false, nseq, max_q, nullptr, st, false, nullptr, 0, nseq, false, tail ? sw.rows : nullptr, (int)n_rows));
  }
  if (m->n_layers == 0) SL_TRY(gather_rows(x, sw.last, sw.rows, n_rows, (size_t)H * sz, st));
  SL_TRY(sl_rmsnorm(sw.last, sw.last, m->final_norm, n_rows, H, m->rms_eps, dt, stream));
  int32_t* top1 = top1_dev ? top1_dev : (seq_top1_dev ? sw.top1 : nullptr);
  const int force = opts ? opts->force_path : 0;
  const int64_t ng = (V + 63) / 64;
  for (int64_t r0 = 0; r0 < n_rows; r0 += sw.chunk) {
    const int M = (int)(n_rows - r0 < sw.chunk ? n_rows - r0 : sw.chunk);
    const void* A = bptr(sw.last) + (size_t)r0 * H * sz;
    if (force != 1 && M > SL_SCORE_UNFUSED_MAX) {
      sl_gemm_args a;
      memset(&a, 0, sizeof(a));
      a.A = A; a.lda = H; a.W = m->lm_head; a.ldw = H; a.C = nullptr; a.ldc = V;
      a.M = M; a.N = V; a.K = H; a.batch = 1; a.dtype = dt; a.act = SL_ACT_NONE; a.out_f32 = 1; a.w_layout = SL_W_ROWMAJOR;
      sl_gemm_ex_args ex;
      memset(&ex, 0, sizeof(ex));
      ex.w_mod = 1;
      ex.amax_val = sw.planes;
      ex.amax_idx = (int32_t*)(sw.planes + ng * M);
      float* psum = sw.planes + 2 * ng * M;
      SL_TRY(sl_gemm_top1_lse_tgt_impl(&a, &ex, psum, labels_dev + r0, sw.tgt, st));
      SL_TRY(sl_score_finalize_impl(ex.amax_val, ex.amax_idx, psum, (int)ng, V, sw.tgt, labels_dev + r0, M, logprob_dev + r0, top1 ? top1 + r0 : nullptr, st));
      g_score_paths |= 2;
    } else {
      SlFamilyPin pin(n_rows > sw.chunk ? sw.chunk : sl_family_rows(0));      // (sl_family_rows(0) = the caller's pin: unchanged)
      SL_TRY(gemm(dt, A, H, m->lm_head, H, sw.logits, V, nullptr, nullptr, 0, M, V, H, SL_ACT_NONE, 1, st));
      SL_TRY(sl_score_rows_impl(sw.logits, V, labels_dev + r0, M, V, logprob_dev + r0, top1 ? top1 + r0 : nullptr, st));
      g_score_paths |= 1;
    }
  }
  if (seq_sum_dev) SL_TRY(sl_score_segment_sums_impl(logprob_dev, labels_dev, top1, sw.offs, nseq, V, seq_sum_dev, seq_counted_dev, seq_top1_dev, st));
  return 0;
}

// decode-step state carved from the tail of the workspace by sl_greedy_generate, or supplied by the caller
// rows from which the lm_head of a greedy decode step leaves per-64-column partial maxima instead of fp32 logits (the tiled
// kernels' fused top-1): the logits round trip is B x vocab x 8 bytes per step, 1 GB at 1 024 rows
constexpr int SL_FUSED_ARGMAX_MIN_B = 256;

// = the steps whose lm_head runs on the tiled kernels (below: packed weights stream through dec_gemm up to 255 rows)
static bool decode_fuses_argmax(const sl_llama_model* m, int B) { B = sl_family_rows(B); return B > 64 && !(m->lm_head_dec && B < SL_FUSED_ARGMAX_MIN_B); }

// fused_top1: the caller will run sl_greedy_select_partial_impl over `logits` reinterpreted as [n_groups][B] floats followed by
// [n_groups][B] int32 (n_groups = ceil(vocab / 64)) — only honoured where decode_fuses_argmax() says so.  top1_sum (token log-probabilities):
// a third plane of [n_groups][B] floats behind the two, the groups' sum exp(v - group max) (3 ceil(V / 64) B <= B0 V floats always holds)
static int decode_step(const sl_llama_model* m, const sl_kv_cache* kv, const int32_t* next_ids, const int32_t* ctx_len, int B, float* logits,
                       void* x, LlamaWs& w, hipStream_t st, bool fused_top1 = false, bool top1_sum = false, const DecodeAttn* da = nullptr) {
  const int dt = m->dtype, H = m->hidden;
  SL_TRY(sl_embed_gather(m->embed, next_ids, x, B, H, dt, (sl_stream)st));
  // hand RMSNorm scales along the chain when every o / down projection has a reduce pass to compute them in
  bool chain = m->dec_fused_norm && m->lm_head_dec && H / 16 * 4 <= 1024 && H % 16 == 0 &&
               sl_gemm_split_count(B, H, m->n_heads * m->head_dim, dt) > 1 && sl_gemm_split_count(B, H, m->ffn, dt) > 1 && w.split != nullptr;
  for (int l = 0; l < m->n_layers && chain; ++l) {
    const sl_llama_layer& L = m->layers[l];
    chain = L.wqkv_dec && L.wo_dec && L.wgu_dec && L.wdown_dec;
  }
  // rows whose o / down projections run UNSPLIT on the 256 x 128 blocks (from ~1 500 rows at Llama-3.2-3B's widths: 8 x 24 = 192 blocks
  // at 2 048): no reduce pass exists to take the RMSNorm scales in, a one-read pass in front of qkv and gate/up leaves them instead
  bool rstd_pass = !chain && sl_is16(dt) && m->dec_fused_norm && sl_family_rows(B) > 384 && sl_gemm_split_count(B, H, m->n_heads * m->head_dim, dt) == 1 &&
                   sl_gemm_split_count(B, H, m->ffn, dt) == 1;
  for (int l = 0; l < m->n_layers && rstd_pass; ++l) {
    const sl_llama_layer& L = m->layers[l];
    rstd_pass = L.wqkv_dec && L.wo_dec && L.wgu_dec && L.wdown_dec;
  }
  for (int l = 0; l < m->n_layers; ++l)
    SL_TRY(llama_layer(m, kv, l, x, B, w, true, B, 1, ctx_len, st, chain, (chain && l > 0) ? w.rstd_b : nullptr, 0, 0, rstd_pass, nullptr, 0, da));
  // lm_head: above ~256 rows the 128-tile MFMA kernel on the row-major matrix beats the streaming kernel on the packed one
  // (M=512: 439 vs 632 us; the 263 MB of fp32 logits dominate either way)
  if (m->lm_head_dec && sl_family_rows(B) < SL_FUSED_ARGMAX_MIN_B) {
    sl_gemm_fused fx;
    memset(&fx, 0, sizeof(fx));
    fx.fuse_rms = m->dec_fused_norm; fx.rms_eps = m->rms_eps;
    const void* a_in = x;
    if (!m->dec_fused_norm) { SL_TRY(sl_rmsnorm(x, w.last, m->final_norm, B, H, m->rms_eps, dt, (sl_stream)st)); a_in = w.last; }
    return dec_gemm(m, w, a_in, H, m->lm_head_dec, logits, m->vocab, nullptr, B, m->vocab, H, SL_ACT_NONE, 1, &fx, st,
                    (chain && m->n_layers > 0) ? w.rstd_b : nullptr);
  }
  SL_TRY(sl_rmsnorm(x, w.last, m->final_norm, B, H, m->rms_eps, dt, (sl_stream)st));
  if (fused_top1 && decode_fuses_argmax(m, B)) {
    const int64_t ng = (m->vocab + 63) / 64;
    sl_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = w.last; a.lda = H; a.W = m->lm_head; a.ldw = H; a.C = nullptr; a.ldc = m->vocab;
    a.M = B; a.N = m->vocab; a.K = H; a.batch = 1; a.dtype = dt; a.act = SL_ACT_NONE; a.out_f32 = 1; a.w_layout = SL_W_ROWMAJOR;
    sl_gemm_ex_args ex;
    memset(&ex, 0, sizeof(ex));
    ex.w_mod = 1;
    ex.amax_val = logits;
    ex.amax_idx = (int32_t*)(logits + ng * B);
    if (top1_sum) return sl_gemm_top1_lse_impl(&a, &ex, logits + 2 * ng * B, st);
    return sl_gemm_impl(&a, nullptr, &ex, st);
  }
  SL_TRY(gemm(dt, w.last, H, m->lm_head, H, logits, m->vocab, nullptr, nullptr, 0, B, m->vocab, H, SL_ACT_NONE, 1, st));
  return 0;
}

__global__ void iota_kernel(int32_t* p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = i;
}

// what a decode step expects of its scratch before its first launch, per captured graph: the K-split fix-up's counters (sl_gemm_fused.split_ws)
// and the split attention's arrival counters (merged in-launch) at zero, tok_seq = the slot index list
static int decode_scratch_reset(const sl_llama_model* m, const sl_kv_cache* kv, const LlamaWs& w, int rows, hipStream_t st) {
  if (w.split && w.split_bytes >= 8192) SL_HIP(hipMemsetAsync(w.split, 0, 8192, st));
  SL_TRY(sl_attn_decode_split_zero_counters(w.part, rows, m->n_heads, m->n_kv_heads, kv->max_ctx, st));
  hipLaunchKernelGGL(iota_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, w.tok_seq, rows);
  SL_CHECK_LAUNCH("iota");
  return 0;
}

extern "C" int sl_llama_decode_step(const sl_llama_model* m, const sl_kv_cache* kv, const int32_t* next_ids_dev, const int32_t* ctx_len_dev,
                                    int32_t B, float* logits, void* workspace, size_t workspace_bytes, sl_stream stream) {
  SL_TRY(llama_check(m, kv));
  SL_CHECK_ARG(next_ids_dev && ctx_len_dev && logits && workspace && B > 0 && B <= kv->slots && B <= SL_MAX_DECODE_BATCH, "sl_llama_decode_step: bad arguments (B<=%d)", SL_MAX_DECODE_BATCH);
  SL_TRY(llama_wformat_check("sl_llama_decode_step", m, B, SL_ENTRY_DECODE));
  hipStream_t st = (hipStream_t)stream;
  LlamaWs w;
  Carver c(workspace, workspace_bytes);
  void* x = c.take((size_t)B * m->hidden * sl_dtype_size(m->dtype));
  c.take(0);
  const size_t off = c.off;
  SL_CHECK_ARG(off <= workspace_bytes, "sl_llama_decode_step: workspace too small");
  const size_t need = off + llama_carve(m, B, B, bptr(workspace) + off, workspace_bytes - off, w);
  SL_CHECK_ARG(need <= workspace_bytes, "sl_llama_decode_step: workspace %zu B < required %zu B", workspace_bytes, need);
  SL_TRY(decode_scratch_reset(m, kv, w, B, st));
  return decode_step(m, kv, next_ids_dev, ctx_len_dev, B, logits, x, w, st);
}

// ---- instantiated decode graphs, cached per thread (see sl_generate)
struct DecodeGraphKey {
  const void *model, *layers, *w0, *lm, *embed, *kc, *vc, *ws;
  size_t ws_bytes;
  uint64_t content;        // FNV-1a over the model struct and every layer struct: all weight / norm / rope pointers and dimensions
  int device;
  int B, B0, max_new, use_eos, n_eos, pad, max_ctx, slots, shared_prefix, dtype, n_layers, vocab, fused, limits;
  int eos[8];
  int sample, top_k;
  float temperature, top_p;
  float min_p, typical_p, epsilon_cutoff, eta_cutoff;   // the warped sampler (all 0 in a graph without it)
  uint64_t seed;
  int beam_k, beam_m, beam_es;     // beam search (0 in every other graph: a beam graph and a greedy graph never share a key)
  float beam_lp;
  float lp_penalty;                // logits processors (all 0 when off: the graph without them): a changed value never replays a stale graph
  int lp_ngram, lp_min_new;
  int scores;                      // token log-probabilities on: other select kernels, a third lm_head plane — never the graph of a call without them
  int n_ret, row_slot0, grouped;   // sl_generate_n: answers per prompt (1 in every other generate graph, 0 in a beam graph), first row slot, attention path
  const void* groups;              // ... and the device records the grouped attention reads
};
struct DecodeGraphEntry { DecodeGraphKey key; hipGraph_t graph; hipGraphExec_t exec; uint64_t stamp; };
static thread_local std::vector<DecodeGraphEntry> g_graphs;
static thread_local uint64_t g_graph_clock = 0;
constexpr size_t SL_GRAPH_CACHE = 64;      // a generation that compacts its batch walks down a ladder of row counts: one graph per rung

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

// Everything a captured decode step bakes in that the caller could change behind the same host addresses: the model struct's
// fields (dimensions, eps, embed / norm / rope / lm_head pointers) and EVERY layer's pointers.  A caller that rebuilds its
// weights and gets the same struct addresses back from malloc therefore misses the cache instead of replaying stale pointers.
static uint64_t model_content_hash(const sl_llama_model* m) {
  uint64_t h = fnv1a(1469598103934665603ull, m, sizeof(*m));
  if (m->layers && m->n_layers > 0) h = fnv1a(h, m->layers, sizeof(m->layers[0]) * (size_t)m->n_layers);
  return h;
}

extern "C" int sl_decode_graph_cache_clear(void) {
  for (auto& e : g_graphs) { (void)hipGraphExecDestroy(e.exec); (void)hipGraphDestroy(e.graph); }
  const int n = (int)g_graphs.size();
  g_graphs.clear();
  return n;
}

static hipGraphExec_t decode_graph_lookup(const DecodeGraphKey& k) {
  for (auto& e : g_graphs)
    if (memcmp(&e.key, &k, sizeof(k)) == 0) { e.stamp = ++g_graph_clock; return e.exec; }
  return nullptr;
}

static void decode_graph_store(const DecodeGraphKey& k, hipGraph_t g, hipGraphExec_t x) {
  if (g_graphs.size() >= SL_GRAPH_CACHE) {   // evict the least recently used
    size_t lru = 0;
    for (size_t i = 1; i < g_graphs.size(); ++i)
      if (g_graphs[i].stamp < g_graphs[lru].stamp) lru = i;
    (void)hipGraphExecDestroy(g_graphs[lru].exec);
    (void)hipGraphDestroy(g_graphs[lru].graph);
    g_graphs.erase(g_graphs.begin() + lru);
  }
  g_graphs.push_back(DecodeGraphEntry{k, g, x, ++g_graph_clock});
}

// the logits processors a call runs: none with lp NULL or all three off (min_new_tokens acts through the EOS ids: off without any)
struct LpPlan {
  bool on = false, penalty = false;
  sl_logits_opts o{1.0f, 0, 0, 0};
};
static LpPlan lp_plan(const sl_logits_opts* lp, int n_eos) {
  LpPlan p;
  if (!lp) return p;
  p.o = *lp;
  p.o.reserved = 0;
  if (n_eos <= 0) p.o.min_new_tokens = 0;
  p.penalty = p.o.repetition_penalty != 1.0f;
  p.on = p.penalty || p.o.no_repeat_ngram_size > 0 || p.o.min_new_tokens > 0;
  return p;
}

extern "C" size_t sl_generate_workspace_bytes_lp(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp) {
  size_t a = sl_generate_workspace_bytes(m, n_tok, nseq, max_new_tokens);
  if (lp && lp->repetition_penalty != 1.0f) a += (size_t)nseq * max_new_tokens * sizeof(float) + 256;      // the penalty's gather scratch
  return a;
}

extern "C" size_t sl_generate_workspace_bytes_sc(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp,
                                                 int32_t scores) {
  size_t a = sl_generate_workspace_bytes_lp(m, n_tok, nseq, max_new_tokens, lp);
  if (scores) a += (size_t)nseq * max_new_tokens * sizeof(float) + 256;      // the (nseq, max_new_tokens) log-probabilities
  return a;
}

extern "C" size_t sl_generate_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens) {
  LlamaWs w;
  size_t a = llama_carve(m, n_tok > nseq ? n_tok : nseq, nseq, nullptr, 0, w);
  a += (size_t)nseq * m->hidden * sl_dtype_size(m->dtype) + 256;    // decode x
  a += (size_t)nseq * m->vocab * sizeof(float) + 256;               // logits
  a += ((size_t)nseq * (8 + max_new_tokens)) * sizeof(int32_t) + 11 * 256;
  return a;
}

// ---- compaction of a batch whose rows finish at different steps (sl_generate_opts.compact) ----
// K / V rows [first, len) of slot `src` copied to slot `dst` in every layer: grid (pair, layer * n_kv); src >= every dst (the movers sit
// above the rows that stay), so no block reads what another writes.  first > 0: a row slot of the grouped path, which holds no prompt rows
struct KvMove { int32_t src, dst, len, first; };
__global__ __launch_bounds__(256) void kv_move_kernel(uint4* __restrict__ kc, uint4* __restrict__ vc, const KvMove* __restrict__ mv, int nkv, int slots,
                                                      int max_ctx, int row_vec) {
  const KvMove m = mv[blockIdx.x];
  const int l = blockIdx.y / nkv, h = blockIdx.y - l * nkv;
  const int64_t lay = (int64_t)l * slots * nkv * max_ctx * row_vec;
  const int64_t s0 = lay + ((int64_t)m.src * nkv + h) * max_ctx * row_vec, d0 = lay + ((int64_t)m.dst * nkv + h) * max_ctx * row_vec;
  const int n = m.len * row_vec;
  for (int i = m.first * row_vec + threadIdx.x; i < n; i += 256) {
    kc[d0 + i] = kc[s0 + i];
    vc[d0 + i] = vc[s0 + i];
  }
}

// rungs of the row-count ladder a compacting generation steps down: each is a row count some kernel family runs at full blocks, and
// each costs one captured graph (kept in the per-thread cache)
static int compact_rung(int n_live) {
  // every 64 rows from 128 up (a captured graph per rung costs ~1 ms once and is cached; padding rows cost a step's per-row time every step:
  // with steps of 128 above 512 rows the synthetic stop mix of bench.py ran 6.2 % more rows x steps than useful tokens), powers of two and
  // their 1.5-multiples below
  static const int small[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128};
  for (int r : small)
    if (n_live <= r) return r;
  return (n_live + 63) / 64 * 64;
}

struct SampleOpts { float temperature; int top_k; float top_p; uint64_t seed; sl_warp_opts warp; bool warped; };   // warped: some option of warp is on

// the three timing events of a generate call, destroyed on every way out of it
struct Events3 {
  hipEvent_t e[3] = {};
  int create() { for (auto& x : e) SL_HIP(hipEventCreate(&x)); return 0; }
  ~Events3() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// ---- the decode graph of both generation loops (sl_generate, sl_beam_generate) ----
// What a loop knows when it asks for the captured step of B rows.  Everything the captured launches bake in is in here, and decode_graph_key
// turns ALL of it into the cache key: a field a mode adds goes into this struct and into that one function.
struct GraphCtx {
  const char* who;
  const sl_llama_model* m;
  const sl_kv_cache* kv;
  void *ws, *scratch;                 // the caller's workspace (its pointer stands for the layout of every state array) and the decode scratch inside it
  size_t ws_bytes, scratch_bytes;
  float* logits;                      // decode_step's arguments: the rows' ids and context lengths in, fp32 logits (or the top-1 planes) out
  void* xdec;
  const int32_t *next_ids, *ctx_len;
  hipStream_t st;                     // the caller's stream: the scratch reset runs here, the capture on a private one
  int B0, max_new, use_eos, n_eos, pad;
  const int32_t* eos;                 // host
  int pin_rows, limits, scores;       // sl_generate only: family pin of a compacting call, per-row budgets, token log-probabilities
  const SampleOpts* smp;              // ... and sampling (NULL = greedy)
  const LpPlan* lp;
  int beam_k, beam_m, beam_es;        // sl_beam_generate only (0 elsewhere: a beam graph and a greedy graph never share a key)
  float beam_lp;
  int n_ret;                          // sl_generate only: answers per prompt
  const DecodeAttn* da;               // ... and, above 1, where the rows keep their K / V (NULL otherwise)
};

// The capture stream of every device, per thread (a stream belongs to the device that was current when it was made), and the prefetch
// branch's side stream and event.  At file scope, NOT inside decode_graph_get: a function template has one set of local statics per
// specialisation, and each loop's tail is a closure type of its own.
static thread_local hipStream_t cap_by_dev[SL_MAX_DEVICES] = {};
static thread_local hipStream_t cap2_by_dev[SL_MAX_DEVICES] = {};
static thread_local hipEvent_t pev_by_dev[SL_MAX_DEVICES] = {};

// the ONLY writer of DecodeGraphKey's fields
static int decode_graph_key(const GraphCtx& g, int B, DecodeGraphKey& key) {
  const sl_llama_model* m = g.m;
  const sl_kv_cache* kv = g.kv;
  memset(&key, 0, sizeof(key));
  key.model = m; key.layers = m->layers; key.w0 = m->n_layers > 0 ? m->layers[0].wqkv_dec : nullptr; key.lm = m->lm_head_dec ? m->lm_head_dec : m->lm_head;
  key.embed = m->embed; key.kc = kv->k_cache; key.vc = kv->v_cache; key.ws = g.ws; key.ws_bytes = g.ws_bytes;
  key.B = B; key.B0 = g.B0; key.max_new = g.max_new; key.use_eos = g.use_eos; key.n_eos = g.n_eos; key.pad = g.pad; key.max_ctx = kv->max_ctx;
  key.slots = kv->slots; key.shared_prefix = kv->shared_prefix; key.dtype = m->dtype; key.n_layers = m->n_layers; key.vocab = m->vocab;
  // + the switches that shape the captured launches
  key.fused = m->dec_fused_norm | (sl_env().decode_tiled << 8) | ((sl_env().attn_decode_ks & 127) << 9) | ((g.pin_rows ? 1 : 0) << 16) |
              ((sl_env().decode_prefetch ? 1 : 0) << 17) | ((sl_kv_format(kv) & 3) << 18) | ((sl_wformat_code(m) & 7) << 20);
  key.limits = g.limits;
  key.content = model_content_hash(m);
  SL_HIP(hipGetDevice(&key.device));
  for (int i = 0; i < g.n_eos && i < 8; ++i) key.eos[i] = g.eos[i];
  if (g.smp) { key.sample = 1; key.temperature = g.smp->temperature; key.top_k = g.smp->top_k; key.top_p = g.smp->top_p; key.seed = g.smp->seed; }
  if (g.smp && g.smp->warped) { key.min_p = g.smp->warp.min_p; key.typical_p = g.smp->warp.typical_p; key.epsilon_cutoff = g.smp->warp.epsilon_cutoff; key.eta_cutoff = g.smp->warp.eta_cutoff; }
  key.beam_k = g.beam_k; key.beam_m = g.beam_m; key.beam_es = g.beam_es; key.beam_lp = g.beam_lp;
  if (g.lp->on) { key.lp_penalty = g.lp->o.repetition_penalty; key.lp_ngram = g.lp->o.no_repeat_ngram_size; key.lp_min_new = g.lp->o.min_new_tokens; }
  key.scores = g.scores;
  key.n_ret = g.n_ret;
  if (g.da) { key.row_slot0 = g.da->row_slot0; key.grouped = g.da->groups ? 1 : 0; key.groups = g.da->groups; }
  return 0;
}

// The decode step for `B` rows: captured ONCE per (model, cache, workspace, row count, mode) and kept in a small per-thread
// cache — a second call with the same buffers (the usual case: a serving loop reusing its KV cache and workspace) replays it
// without re-capturing.  Every pointer the captured launches were recorded with is part of the key (the state arrays and the
// scratch layout follow from the workspace pointer, the ORIGINAL batch B0 and the row count B), so a changed buffer can never
// replay a stale graph.  Also resets the per-graph scratch (decode_scratch_reset).
// tail(cap, B, top1) records on the capture stream everything behind the layers' lm_head; top1: the lm_head left per-64-column
// maxima instead of fp32 logits (greedy without a logits processor — which edits the logits the fused form never writes — at a
// batch the tiled lm_head serves).
template <class Tail>
static int decode_graph_get(const GraphCtx& g, int B, Tail&& tail, hipGraphExec_t* exec_out) {
  const sl_llama_model* m = g.m;
  SlFamilyPin pin(g.pin_rows);
  LlamaWs w;
  llama_carve(m, B, B, g.scratch, g.scratch_bytes, w);
  SL_TRY(decode_scratch_reset(m, g.kv, w, B, g.st));
  DecodeGraphKey key;
  SL_TRY(decode_graph_key(g, B, key));
  hipGraphExec_t exec = decode_graph_lookup(key);
  if (!exec) {
    hipGraph_t graph = nullptr;
    // Capture on a private stream (the caller's may be the legacy null stream, which cannot capture);
    // capturing records the launches without running them, the graph is then replayed on `st`.
    SL_CHECK_ARG(key.device >= 0 && key.device < SL_MAX_DEVICES, "%s: device index %d", g.who, key.device);
    hipStream_t& cap = cap_by_dev[key.device];
    if (!cap) SL_HIP(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    SL_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    const bool top1 = !g.beam_k && !g.smp && !g.lp->on && decode_fuses_argmax(m, B);
    // small batches (the skinny kernels: every matrix read once per step by a chain of short launches): a prefetch branch beside the chain
    DecodePrefetch pf;
    if (!g.beam_k && sl_env().decode_prefetch && B <= sl_env().stream_min_m && m->dtype == SL_BF16) {
      hipStream_t& cap2 = cap2_by_dev[key.device];
      hipEvent_t& pev = pev_by_dev[key.device];
      if (!cap2) SL_HIP(hipStreamCreateWithFlags(&cap2, hipStreamNonBlocking));
      if (!pev) SL_HIP(hipEventCreateWithFlags(&pev, hipEventDisableTiming));
      pf.main = cap; pf.side = cap2; pf.ev = pev; pf.sink = (uint32_t*)w.tok_pos; pf.on = true;      // (the sink is never written: see the kernel)
      g_prefetch = &pf;
    }
    int rc = decode_step(m, g.kv, g.next_ids, g.ctx_len, B, g.logits, g.xdec, w, cap, top1, top1 && g.scores, g.da);
    g_prefetch = nullptr;
    if (pf.on) { const int rj = pf.join(); if (rc == 0) rc = rj; }       // the branch joins the chain before the capture ends
    if (rc == 0) rc = tail(cap, B, top1);
    const hipError_t ce = hipStreamEndCapture(cap, &graph);
    if (rc != 0) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ce != hipSuccess) { sl_set_error("hipStreamEndCapture: %s", hipGetErrorString(ce)); return SL_ERR_LAUNCH; }
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (ie != hipSuccess) (void)hipGraphDestroy(graph);
    SL_HIP(ie);
    decode_graph_store(key, graph, exec);
  }
  *exec_out = exec;
  return 0;
}

// ---- sl_generate's per-row state: each array listed ONCE, in carve order (the workspace layout is part of the graph key through the
// workspace pointer).  Elements are 4 bytes (int32, or float for the two log-probability arrays).  Carve, initial upload, the pulls at a
// check / compaction / the end, the move of a row into a hole and the push back all walk this list.
struct RowTable {
  enum { UNF, CTX, CNT, FIN, NEXT, OUT, CHOICE, LIM, ROW, LPS, LP, PSLOT, PLEN, NCOL };
  // unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, the sampler's drawn tokens, row_limit, row_id (the caller's index of the
  // sequence a row holds), the repetition penalty's gather scratch, the token log-probabilities, and — several answers per prompt — the
  // slot that holds the row's prompt and the positions the row reads from it (0 on the copy path: the row's own slot holds them)
  static constexpr unsigned bit(int i) { return 1u << i; }
  static constexpr unsigned ALL = (1u << NCOL) - 1;
  struct Col {
    size_t row_bytes = 4;
    bool carved = true;             // LPS / LP are carved only when on: the layout without them is unchanged
    bool on = true;                 // state that travels with the row in THIS call (never the two scratch arrays)
    unsigned char* dev = nullptr;
    std::vector<unsigned char> host;
  };
  Col col[NCOL];
  RowTable(int B0, int max_new, bool limits, bool penalty, bool scores, bool prefixes) {
    for (int i : {OUT, LPS, LP}) col[i].row_bytes = (size_t)max_new * 4;
    col[CHOICE].on = col[LPS].on = false;
    col[LIM].on = limits;
    col[LPS].carved = penalty;
    col[LP].carved = col[LP].on = scores;
    for (int i : {PSLOT, PLEN}) col[i].carved = col[i].on = prefixes;      // carved only with several answers per prompt: the layout without them is unchanged
    for (auto& a : col)
      if (a.on) a.host.assign((size_t)B0 * a.row_bytes, 0);
  }
  void carve(Carver& c, int B0) {
    for (auto& a : col)
      if (a.carved) a.dev = (unsigned char*)c.take((size_t)B0 * a.row_bytes);
  }
  template <class T> T* d(int i) const { return (T*)col[i].dev; }
  template <class T> T* h(int i) { return (T*)col[i].host.data(); }
  // rows [0, B) of the arrays in `mask` that this call carries, queued on st
  int copy(unsigned mask, int B, hipMemcpyKind kind, hipStream_t st) {
    for (int i = 0; i < NCOL; ++i) {
      Col& a = col[i];
      if (!a.on || !(mask & bit(i))) continue;
      const bool down = kind == hipMemcpyDeviceToHost;
      SL_HIP(hipMemcpyAsync(down ? (void*)a.host.data() : (void*)a.dev, down ? (const void*)a.dev : (const void*)a.host.data(), (size_t)B * a.row_bytes, kind, st));
    }
    return 0;
  }
  int pull(unsigned mask, int B, hipStream_t st) { return copy(mask, B, hipMemcpyDeviceToHost, st); }
  int push(unsigned mask, int B, hipStream_t st) { return copy(mask, B, hipMemcpyHostToDevice, st); }
  void move(int hole, int r) {
    for (auto& a : col)
      if (a.on) memcpy(a.host.data() + hole * a.row_bytes, a.host.data() + r * a.row_bytes, a.row_bytes);
  }
  // every row unfinished, nothing generated, row r holds sequence r; ctx_len and next_ids are the prefill's and the first select's to write
  int init(const int32_t* limits, int B0, hipStream_t st) {
    for (int b = 0; b < B0; ++b) { h<int32_t>(UNF)[b] = 1; h<int32_t>(ROW)[b] = b; }
    if (limits) memcpy(h<int32_t>(LIM), limits, (size_t)B0 * 4);
    SL_TRY(push(bit(UNF) | bit(CNT) | bit(FIN) | bit(LIM) | bit(ROW) | bit(PSLOT) | bit(PLEN), B0, st));
    for (int i : {OUT, LP})
      if (col[i].on) SL_HIP(hipMemsetAsync(col[i].dev, 0, (size_t)B0 * col[i].row_bytes, st));
    return 0;
  }
};

// fp32 logits row s of `src` (nseq rows) -> rows s * N .. s * N + N - 1 of `dst`: grid (ceil(V / 1024), nseq * N)
__global__ __launch_bounds__(256) void logits_fanout_kernel(const float* __restrict__ src, float* __restrict__ dst, int V, int N) {
  const int b = blockIdx.y;
  const float* s = src + (int64_t)(b / N) * V;
  float* d = dst + (int64_t)b * V;
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < V && i < (int)(blockIdx.x + 1) * 1024; i += 256) d[i] = s[i];
}

// SL_GEN_GROUP_ATTN = -1: where a decode step with the grouped attention was measured no slower than with the prompt rows copied to every
// row slot (tools/bench_sample_n.py, profiles/sample_n_ab.txt; Llama-3.2-3B, bf16, 137-row prompts, N = 4): 16-bit K / V rows
// from 256 rows up (4.87 against 4.99 ms per step at 256 rows, 11.29 against 12.04 at 1 024; 3.02 against 2.84 at 64: two launches per
// layer against one, both launch-bound).  Never on e4m3 rows: 1.01-1.08 of the copy path's step at every row count measured — half the
// bytes to save, the same two launches.
static bool gen_group_attn_rule(int rows, int kv_format) { return kv_format == SL_KV_MODEL_DTYPE && rows >= 256; }

// what generate_impl carves behind the row table when N > 1 (one list for the size query and the carve)
struct SampleNWs {
  sl_attn_group* groups;      // B0 records
  void* gws;                  // the grouped attention's (row, head) records
  float* logits_stage;        // the prefill's nseq logits rows, fanned out to the B0 rows' buffer
  KvMove* fan;                // the copy path's prompt -> row slot moves
  void carve(Carver& c, const sl_llama_model* m, int nseq, int B0) {
    groups = (sl_attn_group*)c.take((size_t)B0 * sizeof(sl_attn_group));
    gws = c.take(sl_attn_decode_grouped_workspace_bytes(B0, m->n_heads));
    logits_stage = (float*)c.take((size_t)nseq * m->vocab * sizeof(float));
    fan = (KvMove*)c.take((size_t)B0 * sizeof(KvMove));
  }
};

static thread_local int g_last_attn_path = 0;
extern "C" int32_t sl_generate_last_attn_path(void) { return g_last_attn_path; }

extern "C" size_t sl_generate_workspace_bytes_n(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp,
                                                int32_t scores, int32_t num_return_sequences) {
  const int N = num_return_sequences;
  if (N == 1) return sl_generate_workspace_bytes_sc(m, n_tok, nseq, max_new_tokens, lp, scores);
  if (!m || N < 1 || nseq <= 0 || (int64_t)nseq * N > SL_MAX_DECODE_BATCH) {
    sl_set_error("sl_generate_workspace_bytes_n: nseq %d x num_return_sequences %d rows outside (0, %d]", nseq, N, SL_MAX_DECODE_BATCH);
    return 0;
  }
  const int B0 = nseq * N;
  size_t a = sl_generate_workspace_bytes_sc(m, n_tok, B0, max_new_tokens, lp, scores);      // every per-row piece, for B0 rows
  a += 2 * ((size_t)B0 * sizeof(int32_t) + 256);                                                // the row table's prefix_slot / prefix_len
  Carver c(nullptr, 0);
  SampleNWs sw;
  sw.carve(c, m, nseq, B0);
  return a + c.off + 512;
}

static int generate_impl(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                         const sl_generate_opts* o, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                         sl_stream stream, const sl_logits_opts* lp_opts = nullptr, float* out_lp_host = nullptr, int N = 1, const int32_t* past_host = nullptr,
                         const int32_t* slot_host = nullptr, const sl_warp_opts* warp = nullptr) {
  SL_CHECK_ARG(o != nullptr, "sl_generate: null options");
  SL_TRY(sl_warp_opts_check("sl_generate_w", warp));      // a value out of range is refused first, and named
  // sl_generate_cont: the caller keeps the cache.  Refused before anything is launched: compaction (it moves live rows into the slots of finished
  // ones and destroys their K / V), several answers per prompt, and slots other than the identity (a decode row's slot is its row index)
  bool past_any = false;      // some sequence continues: the shared-prefix promise is then about the cache ([0, P) below every past)
  if (past_host)
    for (int s = 0; s < nseq; ++s) past_any = past_any || past_host[s] > 0;
  if (past_host) {
    SL_CHECK_ARG(o->compact == 0,"sl_generate_cont: compact must be 0 when the caller keeps the cache (past_len_host is set)");
    SL_CHECK_ARG(N == 1, "sl_generate_cont: one answer per sequence");
    for (int s = 0; s < nseq; ++s) SL_CHECK_ARG(past_host[s] >= 0, "sl_generate_cont: past length %d of sequence %d is negative", past_host[s], s);
  }
  if (slot_host)
    for (int s = 0; s < nseq; ++s)
      if (slot_host[s] != s) {
        sl_set_error("sl_generate_cont: sequence %d in slot %d: the decode loop keeps row b in slot b, pass the sequences in slot order (or NULL)", s, slot_host[s]);
        return SL_ERR_UNSUPPORTED;
      }
  SL_TRY(sl_logits_opts_check("sl_generate", lp_opts, o->max_new_tokens));
  SL_TRY(llama_check(m, kv));
  // several answers per prompt: refused before anything is launched
  SL_CHECK_ARG(N >= 1, "sl_generate_n: num_return_sequences %d < 1", N);
  if (N > 1) {
    SL_TRY(llama_wformat_check("sl_generate_n", m, 0, SL_ENTRY_GENERATE_N));
    SL_CHECK_ARG(o->sample != 0, "sl_generate_n: num_return_sequences %d > 1 needs sample = 1 (greedy answers of one prompt are all the same)", N);
    SL_CHECK_ARG(nseq > 0 && (int64_t)nseq * N <= SL_MAX_DECODE_BATCH, "sl_generate_n: nseq %d x num_return_sequences %d decode rows outside (0, %d]", nseq, N,
                 SL_MAX_DECODE_BATCH);
    SL_CHECK_ARG((int64_t)kv->slots >= (int64_t)nseq * (N + 1), "sl_generate_n: kv->slots %d < nseq * (num_return_sequences + 1) = %lld (nseq prompt slots + a slot per row)",
                 kv->slots, (long long)nseq * (N + 1));
  }
  // use_eos = 0: the EOS ids are ignored even when the caller left them in the struct — rows then finish on their budgets only
  const int max_new_tokens = o->max_new_tokens, n_eos = o->use_eos ? o->n_eos : 0, pad_id = o->pad_id;
  const int32_t* eos_ids_host = o->eos_ids_host;
  const int use_eos = (o->use_eos || o->row_limits_host) ? 1 : 0;       // per-row budgets finish rows the way EOS does
  SL_CHECK_ARG(x && cu_seqlens_host && out_ids_host && workspace && nseq > 0 && nseq <= SL_MAX_DECODE_BATCH && max_new_tokens > 0,
               "sl_generate: bad arguments (nseq<=%d)", SL_MAX_DECODE_BATCH);
  const int B0 = nseq * N;         // decode rows: row s * N + j is answer j of prompt s
  SL_TRY(llama_wformat_check("sl_generate", m, B0, SL_ENTRY_DECODE));      // compaction only moves down the row ladder: a call that starts within the e4m3 range stays within it
  SL_CHECK_ARG(n_eos >= 0 && n_eos <= 8 && (n_eos == 0 || eos_ids_host != nullptr), "sl_generate: 0..8 eos ids");
  SampleOpts smp_s{o->temperature, o->top_k, o->top_p, o->seed, {0.f, 1.0f, 0.f, 0.f}, sl_warp_opts_on(warp)};
  if (smp_s.warped) smp_s.warp = *warp;
  const SampleOpts* smp = o->sample ? &smp_s : nullptr;
  if (smp) SL_CHECK_ARG(smp->temperature > 0.f && smp->top_p > 0.f && smp->top_p <= 1.0f && smp->top_k >= 0, "sl_generate: sampling needs temperature > 0, 0 < top_p <= 1, top_k >= 0");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_tok = cu_seqlens_host[nseq];
  for (int s = 0; s < nseq; ++s)
    SL_CHECK_ARG((int64_t)(past_host ? past_host[s] : 0) + cu_seqlens_host[s + 1] - cu_seqlens_host[s] + max_new_tokens <= kv->max_ctx,
                 "sl_generate: prompt %d (%d tokens) + %d new tokens exceeds max_ctx %d", s,
                 (past_host ? past_host[s] : 0) + cu_seqlens_host[s + 1] - cu_seqlens_host[s], max_new_tokens, kv->max_ctx);
  for (int s = 0; s < nseq; ++s)
    SL_CHECK_ARG(kv->shared_prefix <= (past_any ? past_host[s] : cu_seqlens_host[s + 1] - cu_seqlens_host[s]),
                 "sl_generate: kv cache shared_prefix %d exceeds prompt %d (%d tokens)", kv->shared_prefix, s,
                 past_any ? past_host[s] : cu_seqlens_host[s + 1] - cu_seqlens_host[s]);
  if (o->row_limits_host)
    for (int s = 0; s < B0; ++s)
      SL_CHECK_ARG(o->row_limits_host[s] >= 1 && o->row_limits_host[s] <= max_new_tokens, "sl_generate: row limit %d of sequence %d outside [1, max_new_tokens=%d]",
                   o->row_limits_host[s], s, max_new_tokens);
  const LpPlan lp = lp_plan(lp_opts, n_eos);
  const int scores = out_lp_host ? 1 : 0;
  SL_CHECK_ARG(sl_generate_workspace_bytes_n(m, n_tok, nseq, max_new_tokens, lp.on ? &lp.o : nullptr, scores, N) <= workspace_bytes,
               "sl_generate: workspace %zu B < required %zu B", workspace_bytes,
               sl_generate_workspace_bytes_n(m, n_tok, nseq, max_new_tokens, lp.on ? &lp.o : nullptr, scores, N));
  // N > 1: prompts in slots [0, nseq), rows from slot nseq on.  Grouped: a row reads its prompt from the prompt slot; copy: from its own slot
  DecodeAttn da;
  da.row_slot0 = N > 1 ? nseq : 0;
  const int rep_heads = m->n_kv_heads > 0 ? m->n_heads / m->n_kv_heads : 0;
  const bool grouped = N > 1 && sl_attn_decode_grouped_built(m->n_heads, m->n_kv_heads, m->head_dim, m->dtype, sl_kv_format(kv)) &&
                       (sl_env().gen_group_attn == 1 || (sl_env().gen_group_attn < 0 && gen_group_attn_rule(B0, sl_kv_format(kv))));
  g_last_attn_path = N == 1 ? 0 : (grouped ? 2 : 1);
  // carve: generation state first, then the prefill/decode scratch
  Carver c(workspace, workspace_bytes);
  float* logits = (float*)c.take((size_t)B0 * m->vocab * sizeof(float));
  void* xdec = c.take((size_t)B0 * m->hidden * sl_dtype_size(m->dtype));
  using RT = RowTable;
  RT tab(B0, max_new_tokens, o->row_limits_host != nullptr, lp.penalty, scores != 0, N > 1);
  tab.carve(c, B0);
  SampleNWs sn{};
  std::vector<int32_t> ctx0;
  std::vector<KvMove> fan;
  std::vector<sl_attn_group> recs;
  if (N > 1) {
    sn.carve(c, m, nseq, B0);
    ctx0.resize(B0); recs.resize(B0);
    for (int b = 0; b < B0; ++b) {
      const int s = b / N, len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
      ctx0[b] = len;
      tab.h<int32_t>(RT::PSLOT)[b] = s;
      tab.h<int32_t>(RT::PLEN)[b] = grouped ? len : 0;
      if (!grouped) fan.push_back(KvMove{s, nseq + b, len, 0});
    }
    if (grouped) { da.groups = sn.groups; da.prefix_len = tab.d<int32_t>(RT::PLEN); da.gws = sn.gws; }
  }
  c.take(0);
  void* scratch = bptr(workspace) + c.off;
  const size_t scratch_bytes = workspace_bytes - c.off;
  SL_TRY(tab.init(o->row_limits_host, B0, st));
  // what every select of this call reads and advances (advance_ctx: off for the prefill's token, on inside the captured step)
  SlRowState rs{tab.d<int32_t>(RT::UNF), tab.d<int32_t>(RT::CTX), tab.d<int32_t>(RT::CNT), tab.d<int32_t>(RT::FIN), tab.d<int32_t>(RT::NEXT), tab.d<int32_t>(RT::OUT),
                max_new_tokens, o->row_limits_host ? tab.d<int32_t>(RT::LIM) : nullptr, tab.d<float>(RT::LP), eos_ids_host, n_eos, pad_id, use_eos, 0};

  Events3 ev;
  SL_TRY(ev.create());
  SL_HIP(hipEventRecord(ev.e[0], st));
  SL_TRY(llama_prefill_impl(m, kv, x, cu_seqlens_host, nseq, N > 1 ? sn.logits_stage : logits, rs.ctx_len, nullptr, scratch, scratch_bytes, stream, 1, past_host,
                            slot_host));
  const int kv_row_vec = (int)(m->head_dim * kv_elem_bytes(m, kv) / 16);
  if (N > 1) {
    // each prompt was prefilled once: its logits row and its length go to its N rows; then either the group records (grouped) or a
    // copy of its K / V rows to the N row slots (sources below nseq, destinations from nseq on: disjoint)
    hipLaunchKernelGGL(logits_fanout_kernel, dim3((m->vocab + 1023) / 1024, B0), dim3(256), 0, st, sn.logits_stage, logits, m->vocab, N);
    SL_CHECK_LAUNCH("logits_fanout");
    SL_HIP(hipMemcpyAsync(rs.ctx_len, ctx0.data(), (size_t)B0 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (grouped) {
      int32_t n_used = 0;
      SL_TRY(sl_attn_group_plan_host(tab.h<int32_t>(RT::PSLOT), tab.h<int32_t>(RT::PLEN), B0, rep_heads, recs.data(), &n_used));
      SL_HIP(hipMemcpyAsync(sn.groups, recs.data(), (size_t)B0 * sizeof(sl_attn_group), hipMemcpyHostToDevice, st));
    } else {
      SL_HIP(hipMemcpyAsync(sn.fan, fan.data(), fan.size() * sizeof(KvMove), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(kv_move_kernel, dim3((unsigned)fan.size(), m->n_layers * m->n_kv_heads), dim3(256), 0, st, (uint4*)kv->k_cache, (uint4*)kv->v_cache,
                         sn.fan, m->n_kv_heads, kv->slots, kv->max_ctx, kv_row_vec);
      SL_CHECK_LAUNCH("kv_move (prompt fan-out)");
    }
  }
  // With a processor on, every step — this first one included — is lm_head -> fp32 logits -> sl_logits_process -> select.  The history is
  // the row's own output ids (out_ids, gen_count): both move with the row at a compaction, so nothing else does.
  auto select = [&](int B, hipStream_t s_) -> int {
    if (lp.on)
      SL_TRY(sl_logits_process_impl(logits, B, m->vocab, rs.out_ids, nullptr, max_new_tokens, rs.gen_count, rs.unfinished, &lp.o, eos_ids_host, n_eos, 0,
                                    tab.d<float>(RT::LPS), s_));
    if (smp)
      return sl_sample_select_impl(logits, B, m->vocab, smp->temperature, smp->top_k, smp->top_p, smp->seed, tab.d<int32_t>(RT::CHOICE), tab.d<int32_t>(RT::ROW), rs, s_,
                                   smp->warped ? &smp->warp : nullptr);
    return sl_greedy_select_impl(logits, B, m->vocab, rs, s_);
  };
  SL_TRY(select(B0, st));
  rs.advance_ctx = 1;
  SL_HIP(hipEventRecord(ev.e[1], st));

  // The decode step for `B` rows comes from decode_graph_get.  A compacting generation keeps the kernel family of the batch it started with
  // (common.h sl_family_rows): measured at full depth in bf16, 819 of 1 024 random-init sequences changed ids when each rung picked its own
  // family (near-ties flip between the families' rounding orders) — pinned, a sequence's ids are those of the uncompacted batch, bit for bit.
  // SL_COMPACT_PIN=0: the old behaviour (A/B only).
  GraphCtx g{};
  g.who = "sl_generate"; g.m = m; g.kv = kv; g.ws = workspace; g.ws_bytes = workspace_bytes; g.scratch = scratch; g.scratch_bytes = scratch_bytes;
  g.logits = logits; g.xdec = xdec; g.next_ids = rs.next_ids; g.ctx_len = rs.ctx_len; g.st = st;
  g.B0 = B0; g.max_new = max_new_tokens; g.use_eos = use_eos; g.n_eos = n_eos; g.pad = pad_id; g.eos = eos_ids_host; g.lp = &lp; g.smp = smp;
  g.pin_rows = (o->compact && use_eos && sl_env().compact_pin) ? B0 : 0; g.limits = rs.row_limit ? 1 : 0; g.scores = scores;
  g.n_ret = N; g.da = N > 1 ? &da : nullptr;
  // behind the lm_head: the select above, or — top1: the lm_head left per-group maxima — the pass that reads 1/64 of the bytes
  auto tail = [&](hipStream_t cap, int B, bool top1) -> int {
    if (!top1) return select(B, cap);
    const int64_t ng = (m->vocab + 63) / 64;
    return sl_greedy_select_partial_impl(logits, (const int32_t*)(logits + ng * B), scores ? logits + 2 * ng * B : nullptr, (int)ng, B, rs, cap);
  };

  // host copies of the per-row state live in the table, filled at a check; `done[s]`: sequence s (caller's index) has been written to out_ids_host
  int32_t *h_unf = tab.h<int32_t>(RT::UNF), *h_fin = tab.h<int32_t>(RT::FIN), *orig = tab.h<int32_t>(RT::ROW);
  std::vector<char> done(B0, 0);
  std::vector<int32_t> fin_of(B0, 0), unf_of(B0, 1);
  int steps_done = 1, B = B0, compactions = 0, launches = 0;
  int64_t row_steps = 0;
  bool all_done = false;
  // rows [0, B) -> the caller's output rows, for the sequences not written yet (a retired sequence's row may live on as padding of
  // the compacted batch: its pads are not written again)
  auto retire = [&](bool only_finished) {
    for (int r = 0; r < B; ++r) {
      const int s = orig[r];
      if (done[s] || (only_finished && h_unf[r] != 0)) continue;
      memcpy(out_ids_host + (size_t)s * max_new_tokens, tab.h<int32_t>(RT::OUT) + (size_t)r * max_new_tokens, (size_t)max_new_tokens * sizeof(int32_t));
      if (scores) memcpy(out_lp_host + (size_t)s * max_new_tokens, tab.h<float>(RT::LP) + (size_t)r * max_new_tokens, (size_t)max_new_tokens * sizeof(float));
      fin_of[s] = h_fin[r]; unf_of[s] = h_unf[r];
      done[s] = 1;
    }
  };
  if (max_new_tokens > 1) {
    hipGraphExec_t exec = nullptr;
    SL_TRY(decode_graph_get(g, B, tail, &exec));
    const int check_every = o->check_every > 0 ? o->check_every : 16;
    while (steps_done < max_new_tokens) {
      SL_HIP(hipGraphLaunch(exec, st));
      ++steps_done; ++launches; row_steps += B;
      if (!(use_eos && (steps_done % check_every == 0) && steps_done < max_new_tokens)) continue;
      SL_TRY(tab.pull(RT::bit(RT::UNF), B, st));
      SL_HIP(hipStreamSynchronize(st));
      int n_live = 0;
      for (int b = 0; b < B; ++b) n_live += (h_unf[b] != 0);
      if (n_live == 0) { all_done = true; break; }
      const int rung = compact_rung(n_live);
      if (!o->compact || rung >= B) continue;
      // ---- compact: the live rows that sit at or above `rung` (the movers) take the places of finished rows below it; live rows
      // below it and the remaining finished ones (padding of the rung) stay where they are.  Finished sequences are written to the
      // caller's buffer first.  Everything per-row moves with the row: the table's arrays (through the host: a few KB) and
      // the row's K / V slot (on the device).
      SL_TRY(tab.pull(RT::ALL & ~(RT::bit(RT::UNF) | RT::bit(RT::ROW)), B, st));      // (unfinished is here already, the row ids are the host's to say)
      SL_HIP(hipStreamSynchronize(st));
      retire(true);
      std::vector<KvMove> moves;
      int hole = 0;
      for (int r = rung; r < B; ++r) {
        if (h_unf[r] == 0) continue;
        while (h_unf[hole] != 0) ++hole;          // exists: at most `rung` rows are live
        moves.push_back(KvMove{da.row_slot0 + r, da.row_slot0 + hole, tab.h<int32_t>(RT::CTX)[r], N > 1 ? tab.h<int32_t>(RT::PLEN)[r] : 0});
        tab.move(hole, r);
        ++hole;
      }
      if (!moves.empty()) {
        KvMove* mv_dev = (KvMove*)logits;         // the logits buffer is idle between steps (>= B0 * vocab floats)
        SL_CHECK_ARG(moves.size() * sizeof(KvMove) <= (size_t)B0 * m->vocab * sizeof(float), "sl_generate: move list does not fit");
        SL_HIP(hipMemcpyAsync(mv_dev, moves.data(), moves.size() * sizeof(KvMove), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(kv_move_kernel, dim3((unsigned)moves.size(), m->n_layers * m->n_kv_heads), dim3(256), 0, st, (uint4*)kv->k_cache, (uint4*)kv->v_cache,
                           mv_dev, m->n_kv_heads, kv->slots, kv->max_ctx, kv_row_vec);
        SL_CHECK_LAUNCH("kv_move");
      }
      B = rung;
      SL_TRY(tab.push(RT::ALL, B, st));
      if (grouped) {      // the rows moved: their records are planned again over the rung's rows
        int32_t n_used = 0;
        SL_TRY(sl_attn_group_plan_host(tab.h<int32_t>(RT::PSLOT), tab.h<int32_t>(RT::PLEN), B, rep_heads, recs.data(), &n_used));
        SL_HIP(hipMemcpyAsync(sn.groups, recs.data(), (size_t)B * sizeof(sl_attn_group), hipMemcpyHostToDevice, st));
      }
      SL_HIP(hipStreamSynchronize(st));           // the host arrays above are reused / the move list is overwritten by the next step's logits
      SL_TRY(decode_graph_get(g, B, tail, &exec));
      ++compactions;
    }
  }
  SL_HIP(hipEventRecord(ev.e[2], st));
  // results: queued behind the last step on the caller's stream, ONE synchronisation for the whole call (plus one per check above)
  SL_TRY(tab.pull(RT::bit(RT::UNF) | RT::bit(RT::FIN) | RT::bit(RT::OUT) | RT::bit(RT::LP), B, st));
  SL_HIP(hipStreamSynchronize(st));
  retire(false);
  int n_cols = steps_done;
  if (use_eos) {
    all_done = true;
    int mx = 0;
    for (int s = 0; s < B0; ++s) { all_done = all_done && unf_of[s] == 0; if (fin_of[s] > mx) mx = fin_of[s]; }
    if (all_done) n_cols = mx;  // HF stops at the step where the last row emitted its EOS
    // a sequence retired at a compaction has pads up to the step of its retirement only: pad the rest of its row, as the uncompacted
    // batch would have (hf:generation/utils.py:2928-2929)
    for (int s = 0; s < B0; ++s)
      if (unf_of[s] == 0)
        for (int t = fin_of[s]; t < max_new_tokens; ++t) {
          out_ids_host[(size_t)s * max_new_tokens + t] = pad_id;
          if (scores) out_lp_host[(size_t)s * max_new_tokens + t] = 0.f;
        }
  }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->n_steps = n_cols; stats->decode_launches = launches; stats->compactions = compactions; stats->final_rows = B; stats->row_steps = row_steps;
    SL_HIP(hipEventElapsedTime(&stats->prefill_ms, ev.e[0], ev.e[1]));
    SL_HIP(hipEventElapsedTime(&stats->decode_ms, ev.e[1], ev.e[2]));
  }
  return 0;
}

extern "C" int sl_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                           const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                           sl_stream stream) {
  return generate_impl(m, kv, x, cu_seqlens_host, nseq, opts, out_ids_host, stats, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int sl_generate_lp(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                              const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                              sl_stream stream, const sl_logits_opts* lp) {
  return generate_impl(m, kv, x, cu_seqlens_host, nseq, opts, out_ids_host, stats, workspace, workspace_bytes, stream, lp);
}

extern "C" int sl_generate_sc(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                              const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                              sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host) {
  return generate_impl(m, kv, x, cu_seqlens_host, nseq, opts, out_ids_host, stats, workspace, workspace_bytes, stream, lp, out_logprobs_host);
}

/* sl_generate_cont: sl_generate_sc on a cache the caller keeps (speechllm.h) */
extern "C" size_t sl_generate_workspace_bytes_cont(const sl_llama_model* m, int64_t n_tok, int32_t nseq, int32_t max_new_tokens, const sl_logits_opts* lp,
                                                   int32_t scores) {
  return sl_generate_workspace_bytes_sc(m, n_tok, nseq, max_new_tokens, lp, scores);
}
extern "C" int sl_generate_cont(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                                const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                                sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host, const int32_t* past_len_host, const int32_t* slot_host) {
  return generate_impl(m, kv, x, cu_seqlens_host, nseq, opts, out_ids_host, stats, workspace, workspace_bytes, stream, lp, out_logprobs_host, 1, past_len_host,
                       slot_host);
}

extern "C" int sl_generate_n(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                             const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                             sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host, int32_t num_return_sequences) {
  return generate_impl(m, kv, x, cu_seqlens_host, nseq, opts, out_ids_host, stats, workspace, workspace_bytes, stream, lp, out_logprobs_host,
                       num_return_sequences);
}

extern "C" int sl_generate_w(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                             const sl_generate_opts* opts, int32_t* out_ids_host, sl_generate_stats* stats, void* workspace, size_t workspace_bytes,
                             sl_stream stream, const sl_logits_opts* lp, float* out_logprobs_host, int32_t num_return_sequences,
                             const int32_t* past_len_host, const int32_t* slot_host, const sl_warp_opts* warp) {
  return generate_impl(m, kv, x, cu_seqlens_host, nseq, opts, out_ids_host, stats, workspace, workspace_bytes, stream, lp, out_logprobs_host,
                       num_return_sequences, past_len_host, slot_host, warp);
}

static int generate_compat(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq, sl_generate_opts& o,
                           int32_t* out_ids_host, int32_t* n_steps_host, float* timings_ms_host, void* workspace, size_t workspace_bytes, sl_stream stream) {
  SL_CHECK_ARG(n_steps_host != nullptr, "sl_greedy_generate: null n_steps");
  sl_generate_stats stt;
  SL_TRY(generate_impl(m, kv, x, cu_seqlens_host, nseq, &o, out_ids_host, &stt, workspace, workspace_bytes, stream));
  *n_steps_host = stt.n_steps;
  if (timings_ms_host) { timings_ms_host[0] = stt.prefill_ms; timings_ms_host[1] = stt.decode_ms; }
  return 0;
}

extern "C" int sl_greedy_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                                  int32_t max_new_tokens, const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos,
                                  int32_t check_every, int32_t* out_ids_host, int32_t* n_steps_host, float* timings_ms_host,
                                  void* workspace, size_t workspace_bytes, sl_stream stream) {
  sl_generate_opts o;
  memset(&o, 0, sizeof(o));
  o.max_new_tokens = max_new_tokens; o.eos_ids_host = eos_ids_host; o.n_eos = n_eos; o.pad_id = pad_id; o.use_eos = use_eos; o.check_every = check_every;
  return generate_compat(m, kv, x, cu_seqlens_host, nseq, o, out_ids_host, n_steps_host, timings_ms_host, workspace, workspace_bytes, stream);
}

extern "C" int sl_sample_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                                  int32_t max_new_tokens, const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id, int32_t use_eos,
                                  int32_t check_every, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t* out_ids_host,
                                  int32_t* n_steps_host, float* timings_ms_host, void* workspace, size_t workspace_bytes, sl_stream stream) {
  SL_CHECK_ARG(temperature > 0.f && top_p > 0.f && top_p <= 1.0f && top_k >= 0, "sl_sample_generate: need temperature > 0, 0 < top_p <= 1, top_k >= 0");
  sl_generate_opts o;
  memset(&o, 0, sizeof(o));
  o.max_new_tokens = max_new_tokens; o.eos_ids_host = eos_ids_host; o.n_eos = n_eos; o.pad_id = pad_id; o.use_eos = use_eos; o.check_every = check_every;
  o.sample = 1; o.temperature = temperature; o.top_k = top_k; o.top_p = top_p; o.seed = seed;
  return generate_compat(m, kv, x, cu_seqlens_host, nseq, o, out_ids_host, n_steps_host, timings_ms_host, workspace, workspace_bytes, stream);
}

// ================================================================================================
// Beam search (speechllm.h sl_beam_generate; kernels in beam.hip)
// ================================================================================================
int sl_beam_topk_impl(const float* logits, int32_t rows, int32_t V, const float* row_score, int32_t M, float* cand_score, int32_t* cand_token,
                      hipStream_t st, int is_logprob);
int sl_beam_step_impl(const sl_beam_state* s, const float* cand_score, const int32_t* cand_token, int32_t nseq, int32_t K, int32_t M, int32_t first,
                      const sl_beam_opts* o, hipStream_t st);
int sl_beam_m(int num_beams, int n_eos);
size_t sl_kv_beam_staging_bytes_impl(const sl_kv_cache* kv, const sl_llama_model* m, int32_t rows, int32_t max_span);
int sl_kv_beam_reorder_impl(const sl_kv_cache* kv, const sl_llama_model* m, const int32_t* src_row, const int32_t* prompt_len, const int32_t* ctx_len,
                            int32_t rows, int32_t max_span, void* staging, size_t staging_bytes, hipStream_t st);

struct BeamWs {
  float *logits, *cand_score, *zero_score, *len_pen;
  void* xdec;
  int32_t *cand_token, *prompt_len;
  KvMove* moves;
  sl_beam_state st;
  void* staging;
  size_t staging_bytes;
  void* scratch;
  size_t scratch_off;
  int32_t* hist_len;      // logits processors on: (R) length of every row's history (= the sequence's step), refreshed inside the captured step
  float* lp_scratch;      // ... and the repetition penalty's gather scratch (R, max_new)
};

// hist_len[r] = step of the sequence row r belongs to (sl_beam_state.step): the running beams of a sequence all hold `step` tokens
__global__ void beam_hist_len_kernel(const int32_t* __restrict__ step, int K, int R, int32_t* __restrict__ hist_len) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < R) hist_len[r] = step[r / K];
}

// generation state first, then the staging area of the cache re-ordering, then the prefill / decode scratch
static size_t beam_carve(const sl_llama_model* m, const sl_kv_cache* kv, int64_t n_tok, int nseq, int K, int M, int max_new, void* base, size_t cap, BeamWs& b,
                         const LpPlan& lp) {
  const size_t R = (size_t)nseq * K;
  Carver c(base, cap);
  b.logits = (float*)c.take(R * m->vocab * sizeof(float));
  b.xdec = c.take(R * m->hidden * sl_dtype_size(m->dtype));
  b.cand_score = (float*)c.take(R * M * sizeof(float));
  b.cand_token = (int32_t*)c.take(R * M * sizeof(int32_t));
  b.zero_score = (float*)c.take((size_t)nseq * sizeof(float));
  b.len_pen = (float*)c.take((size_t)max_new * sizeof(float));
  b.prompt_len = (int32_t*)c.take(R * sizeof(int32_t));
  b.moves = (KvMove*)c.take(R * sizeof(KvMove));
  b.st.run_score = (float*)c.take(R * sizeof(float));
  b.st.next_ids = (int32_t*)c.take(R * sizeof(int32_t));
  b.st.src_row = (int32_t*)c.take(R * sizeof(int32_t));
  b.st.ctx_len = (int32_t*)c.take(R * sizeof(int32_t));
  b.st.hist[0] = (int32_t*)c.take(R * max_new * sizeof(int32_t));
  b.st.hist[1] = (int32_t*)c.take(R * max_new * sizeof(int32_t));
  b.st.fin_score = (float*)c.take(R * sizeof(float));
  b.st.fin_ids = (int32_t*)c.take(R * max_new * sizeof(int32_t));
  b.st.fin_flag = (int32_t*)c.take(R * sizeof(int32_t));
  b.st.fin_len = (int32_t*)c.take(R * sizeof(int32_t));
  b.st.open = (int32_t*)c.take((size_t)nseq * sizeof(int32_t));
  b.st.seq_done = (int32_t*)c.take((size_t)nseq * sizeof(int32_t));
  b.st.step = (int32_t*)c.take((size_t)nseq * sizeof(int32_t));
  b.st.len_pen = b.len_pen;
  b.staging_bytes = K > 1 ? sl_kv_beam_staging_bytes_impl(kv, m, (int)R, max_new) : 0;
  b.staging = c.take(b.staging_bytes);
  b.hist_len = lp.on ? (int32_t*)c.take(R * sizeof(int32_t)) : nullptr;          // carved only when on: the layout without them is unchanged
  b.lp_scratch = lp.penalty ? (float*)c.take(R * max_new * sizeof(float)) : nullptr;
  c.take(0);
  b.scratch_off = c.off;
  b.scratch = base ? (unsigned char*)base + c.off : nullptr;
  LlamaWs w;
  return c.off + llama_carve(m, n_tok > (int64_t)R ? n_tok : (int64_t)R, (int)R, nullptr, 0, w) + 256;
}

// every limit of sl_beam_generate, before any launch (also what sl_beam_generate_workspace_bytes refuses)
static int beam_check(const char* who, const sl_llama_model* m, const sl_kv_cache* kv, int nseq, const sl_beam_opts* o, int* M_out) {
  SL_CHECK_ARG(m && kv && o, "%s: null model, cache or options", who);
  SL_CHECK_ARG(o->num_beams >= 1 && o->num_beams <= 8, "%s: num_beams %d outside [1, 8]", who, o->num_beams);
  const int n_eos = o->use_eos ? o->n_eos : 0;
  SL_CHECK_ARG(n_eos >= 0 && n_eos <= 8 && (n_eos == 0 || o->eos_ids_host != nullptr), "%s: 0..8 eos ids", who);
  const int M = sl_beam_m(o->num_beams, n_eos);
  if (M > 64) {
    sl_set_error("%s: max(2, 1 + n_eos) * num_beams = %d candidates per step, the kernels keep 64 (num_beams %d, %d eos ids)", who, M, o->num_beams, n_eos);
    return SL_ERR_UNSUPPORTED;
  }
  SL_CHECK_ARG(M <= m->vocab, "%s: %d candidates per step exceed the vocabulary (%d)", who, M, m->vocab);
  SL_CHECK_ARG(nseq > 0 && (int64_t)nseq * o->num_beams <= SL_MAX_DECODE_BATCH, "%s: nseq * num_beams = %lld rows outside (0, %d]", who,
               (long long)nseq * o->num_beams, SL_MAX_DECODE_BATCH);
  SL_CHECK_ARG((int64_t)nseq * o->num_beams <= kv->slots, "%s: nseq * num_beams = %lld rows need as many cache slots (kv->slots = %d)", who,
               (long long)nseq * o->num_beams, kv->slots);
  SL_CHECK_ARG(o->num_return_sequences >= 1 && o->num_return_sequences <= o->num_beams, "%s: num_return_sequences %d outside [1, num_beams = %d]", who,
               o->num_return_sequences, o->num_beams);
  SL_CHECK_ARG(std::isfinite(o->length_penalty), "%s: length_penalty must be finite", who);
  SL_CHECK_ARG(o->early_stopping >= 0 && o->early_stopping <= 2, "%s: early_stopping %d (0 = False, 1 = True, 2 = \"never\")", who, o->early_stopping);
  SL_CHECK_ARG(o->max_new_tokens > 0 && o->max_new_tokens <= kv->max_ctx, "%s: max_new_tokens %d outside (0, max_ctx = %d]", who, o->max_new_tokens, kv->max_ctx);
  *M_out = M;
  return 0;
}

extern "C" size_t sl_beam_generate_workspace_bytes_lp(const sl_llama_model* m, int64_t n_tok, int32_t nseq, const sl_kv_cache* kv, const sl_beam_opts* o,
                                                      const sl_logits_opts* lp) {
  int M = 0;
  if (beam_check("sl_beam_generate_workspace_bytes", m, kv, nseq, o, &M) != 0) return 0;
  if (sl_logits_opts_check("sl_beam_generate_workspace_bytes", lp, o->max_new_tokens) != 0) return 0;
  BeamWs b;
  return beam_carve(m, kv, n_tok, nseq, o->num_beams, M, o->max_new_tokens, nullptr, 0, b, lp_plan(lp, o->use_eos ? o->n_eos : 0));
}

extern "C" size_t sl_beam_generate_workspace_bytes(const sl_llama_model* m, int64_t n_tok, int32_t nseq, const sl_kv_cache* kv, const sl_beam_opts* o) {
  return sl_beam_generate_workspace_bytes_lp(m, n_tok, nseq, kv, o, nullptr);
}

extern "C" int sl_beam_generate_lp(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                                   const sl_beam_opts* o, int32_t* out_ids_host, float* out_scores_host, int32_t* out_lens_host,
                                   sl_generate_stats* stats, void* workspace, size_t workspace_bytes, sl_stream stream, const sl_logits_opts* lp_opts) {
  int M = 0;
  SL_TRY(beam_check("sl_beam_generate", m, kv, nseq, o, &M));
  SL_TRY(sl_logits_opts_check("sl_beam_generate", lp_opts, o->max_new_tokens));
  SL_TRY(llama_check(m, kv));
  SL_CHECK_ARG(x && cu_seqlens_host && out_ids_host && out_scores_host && out_lens_host && workspace, "sl_beam_generate: null buffer");
  const int K = o->num_beams, R = nseq * K, Rn = o->num_return_sequences, max_new = o->max_new_tokens;
  const int n_eos = o->use_eos ? o->n_eos : 0;
  SL_TRY(llama_wformat_check("sl_beam_generate", m, R, SL_ENTRY_BEAM));
  for (int s = 0; s < nseq; ++s) {
    const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
    SL_CHECK_ARG(len > 0 && len + max_new <= kv->max_ctx, "sl_beam_generate: prompt %d (%d tokens) + %d new tokens exceeds max_ctx %d", s, len, max_new, kv->max_ctx);
    SL_CHECK_ARG(kv->shared_prefix <= len, "sl_beam_generate: kv cache shared_prefix %d exceeds prompt %d (%d tokens)", kv->shared_prefix, s, len);
  }
  const int64_t n_tok = cu_seqlens_host[nseq];
  BeamWs b;
  const LpPlan lp = lp_plan(lp_opts, n_eos);
  const size_t need = beam_carve(m, kv, n_tok, nseq, K, M, max_new, workspace, workspace_bytes, b, lp);
  SL_CHECK_ARG(need <= workspace_bytes, "sl_beam_generate: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const size_t scratch_bytes = workspace_bytes - b.scratch_off;
  sl_beam_opts oo = *o;           // the options the kernels see: EOS ids only when in use
  oo.n_eos = n_eos; oo.use_eos = n_eos > 0 ? 1 : 0;

  // ---- initial state
  std::vector<float> run0(R, -1.0e9f), fin0(R, -1.0e9f), lpen(max_new);
  std::vector<int32_t> ctx0(R), ones(nseq, 1);
  std::vector<KvMove> moves;
  for (int s = 0; s < nseq; ++s) {
    const int len = cu_seqlens_host[s + 1] - cu_seqlens_host[s];
    run0[(size_t)s * K] = 0.f;
    for (int j = 0; j < K; ++j) {
      ctx0[(size_t)s * K + j] = len;
      if (j > 0) moves.push_back(KvMove{s * K, s * K + j, len, 0});
    }
  }
  for (int t = 0; t < max_new; ++t) lpen[t] = (float)pow((double)(t + 1), (double)o->length_penalty);
  Events3 ev;
  SL_TRY(ev.create());
  SL_HIP(hipEventRecord(ev.e[0], st));
  // prefill: each prompt once, into the slot of its first beam (it writes nseq context lengths: overwritten below with the rows')
  SL_TRY(llama_prefill_impl(m, kv, x, cu_seqlens_host, nseq, b.logits, b.st.ctx_len, nullptr, b.scratch, scratch_bytes, stream, K));
  SL_HIP(hipMemcpyAsync(b.st.run_score, run0.data(), R * sizeof(float), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(b.st.fin_score, fin0.data(), R * sizeof(float), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(b.st.ctx_len, ctx0.data(), R * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(b.prompt_len, ctx0.data(), R * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(b.len_pen, lpen.data(), max_new * sizeof(float), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemcpyAsync(b.st.open, ones.data(), nseq * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SL_HIP(hipMemsetAsync(b.zero_score, 0, nseq * sizeof(float), st));
  SL_HIP(hipMemsetAsync(b.st.seq_done, 0, nseq * sizeof(int32_t), st));
  SL_HIP(hipMemsetAsync(b.st.step, 0, nseq * sizeof(int32_t), st));
  SL_HIP(hipMemsetAsync(b.st.fin_flag, 0, R * sizeof(int32_t), st));
  SL_HIP(hipMemsetAsync(b.st.fin_len, 0, R * sizeof(int32_t), st));
  SL_HIP(hipMemsetAsync(b.st.hist[0], 0, (size_t)R * max_new * sizeof(int32_t), st));
  SL_HIP(hipMemsetAsync(b.st.hist[1], 0, (size_t)R * max_new * sizeof(int32_t), st));
  SL_HIP(hipMemsetAsync(b.st.fin_ids, 0, (size_t)R * max_new * sizeof(int32_t), st));
  if (!moves.empty()) {      // the prompt's K / V rows to the K - 1 sibling slots: sources (s * K) and destinations are disjoint
    const int row_vec = (int)(m->head_dim * kv_elem_bytes(m, kv) / 16);
    SL_HIP(hipMemcpyAsync(b.moves, moves.data(), moves.size() * sizeof(KvMove), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kv_move_kernel, dim3((unsigned)moves.size(), m->n_layers * m->n_kv_heads), dim3(256), 0, st, (uint4*)kv->k_cache, (uint4*)kv->v_cache,
                       b.moves, m->n_kv_heads, kv->slots, kv->max_ctx, row_vec);
    SL_CHECK_LAUNCH("kv_move (beam prompt)");
  }
  // step 0: the prefill logits are beam 0's.  With a logits processor on, HF's order: log_softmax, the processors on the log-probabilities
  // (every history is empty here: only min_new_tokens can act), then the running score and the selection.
  if (lp.on) {
    SL_HIP(hipMemsetAsync(b.hist_len, 0, (size_t)R * sizeof(int32_t), st));
    SL_TRY(sl_logits_process_impl(b.logits, nseq, m->vocab, b.st.hist[0], b.st.hist[1], max_new, b.hist_len, nullptr, &lp.o, o->eos_ids_host, n_eos, 1,
                                  b.lp_scratch, st));
  }
  SL_TRY(sl_beam_topk_impl(b.logits, nseq, m->vocab, b.zero_score, M, b.cand_score, b.cand_token, st, lp.on ? 1 : 0));
  SL_TRY(sl_beam_step_impl(&b.st, b.cand_score, b.cand_token, nseq, K, M, 1, &oo, st));
  SL_HIP(hipEventRecord(ev.e[1], st));
  SL_HIP(hipStreamSynchronize(st));     // the host vectors above leave scope only after their copies ran

  int steps_done = 1, launches = 0;
  std::vector<int32_t> h_done(nseq, 0);
  if (max_new > 1) {
    GraphCtx g{};
    g.who = "sl_beam_generate"; g.m = m; g.kv = kv; g.ws = workspace; g.ws_bytes = workspace_bytes; g.scratch = b.scratch; g.scratch_bytes = scratch_bytes;
    g.logits = b.logits; g.xdec = b.xdec; g.next_ids = b.st.next_ids; g.ctx_len = b.st.ctx_len; g.st = st;
    g.B0 = nseq; g.max_new = max_new; g.use_eos = oo.use_eos; g.n_eos = n_eos; g.pad = o->pad_id; g.eos = o->eos_ids_host; g.lp = &lp;
    g.beam_k = K; g.beam_m = M; g.beam_es = o->early_stopping; g.beam_lp = o->length_penalty;
    // behind the lm_head's fp32 logits: row s * K + j holds the history of running beam j, `step` tokens long, in hist[step & 1]
    auto tail = [&](hipStream_t cap, int, bool) -> int {
      if (lp.on) {
        hipLaunchKernelGGL(beam_hist_len_kernel, dim3((R + 255) / 256), dim3(256), 0, cap, b.st.step, K, R, b.hist_len);
        SL_CHECK_LAUNCH("beam_hist_len");
        SL_TRY(sl_logits_process_impl(b.logits, R, m->vocab, b.st.hist[0], b.st.hist[1], max_new, b.hist_len, nullptr, &lp.o, o->eos_ids_host, n_eos, 1,
                                      b.lp_scratch, cap));
      }
      SL_TRY(sl_beam_topk_impl(b.logits, R, m->vocab, b.st.run_score, M, b.cand_score, b.cand_token, cap, lp.on ? 1 : 0));
      SL_TRY(sl_beam_step_impl(&b.st, b.cand_score, b.cand_token, nseq, K, M, 0, &oo, cap));
      return K > 1 ? sl_kv_beam_reorder_impl(kv, m, b.st.src_row, b.prompt_len, b.st.ctx_len, R, max_new, b.staging, b.staging_bytes, cap) : 0;
    };
    hipGraphExec_t exec = nullptr;
    SL_TRY(decode_graph_get(g, R, tail, &exec));
    const int check_every = o->check_every > 0 ? o->check_every : 16;
    while (steps_done < max_new) {
      SL_HIP(hipGraphLaunch(exec, st));
      ++steps_done; ++launches;
      if (steps_done % check_every != 0 || steps_done >= max_new) continue;
      SL_HIP(hipMemcpyAsync(h_done.data(), b.st.seq_done, nseq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      SL_HIP(hipStreamSynchronize(st));
      bool all = true;
      for (int s = 0; s < nseq; ++s) all = all && h_done[s] != 0;
      if (all) break;
    }
  }
  SL_HIP(hipEventRecord(ev.e[2], st));
  std::vector<int32_t> h_ids((size_t)R * max_new), h_len(R);
  std::vector<float> h_sc(R);
  SL_HIP(hipMemcpyAsync(h_ids.data(), b.st.fin_ids, h_ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SL_HIP(hipMemcpyAsync(h_len.data(), b.st.fin_len, R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SL_HIP(hipMemcpyAsync(h_sc.data(), b.st.fin_score, R * sizeof(float), hipMemcpyDeviceToHost, st));
  SL_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < nseq; ++s)
    for (int r = 0; r < Rn; ++r) {
      const size_t src = (size_t)s * K + r, dst = (size_t)s * Rn + r;
      int len = h_len[src];
      len = len < 0 ? 0 : (len > max_new ? max_new : len);
      for (int t = 0; t < max_new; ++t) out_ids_host[dst * max_new + t] = t < len ? h_ids[src * max_new + t] : o->pad_id;
      out_scores_host[dst] = h_sc[src];
      out_lens_host[dst] = len;
    }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->n_steps = steps_done; stats->decode_launches = launches; stats->final_rows = R; stats->row_steps = (int64_t)launches * R;
    SL_HIP(hipEventElapsedTime(&stats->prefill_ms, ev.e[0], ev.e[1]));
    SL_HIP(hipEventElapsedTime(&stats->decode_ms, ev.e[1], ev.e[2]));
  }
  return 0;
}

extern "C" int sl_beam_generate(const sl_llama_model* m, const sl_kv_cache* kv, void* x, const int32_t* cu_seqlens_host, int32_t nseq,
                                const sl_beam_opts* o, int32_t* out_ids_host, float* out_scores_host, int32_t* out_lens_host,
                                sl_generate_stats* stats, void* workspace, size_t workspace_bytes, sl_stream stream) {
  return sl_beam_generate_lp(m, kv, x, cu_seqlens_host, nseq, o, out_ids_host, out_scores_host, out_lens_host, stats, workspace, workspace_bytes, stream, nullptr);
}
