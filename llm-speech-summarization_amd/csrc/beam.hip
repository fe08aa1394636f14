// beam.hip — beam search on the device (hf:generation/utils.py _beam_search and its helpers, restated in tests/beam_ref.py):
//   beam_topk_kernel        one block per decode row: log-softmax + the row's running score, the row's M largest with their tokens
//                           (is_logprob: the row already holds processed log-probabilities, logits_proc.hip; the softmax passes are skipped)
//   beam_step_kernel        one block per sequence: merge of the K rows' lists into M candidates, next running beams, finished set,
//                           early-stop heuristic, done flag, token histories
//   kv_beam_gather / scatter  the K/V cache re-ordered by the chosen source beams, through a staging area (a slot is source AND destination)
// No float atomics anywhere: a row's / a sequence's output is the same on every run.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t beam_ord_key(float x) {      // order-preserving 32-bit image of a float (select.hip ord_key)
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct BeamEos { int n; int ids[8]; };

constexpr int BEAM_MAX_M = 64;
constexpr int BEAM_MAX_K = 8;
constexpr int TOPK_THREADS = 1024;

// ----------------------------------------------------------------------------------------------
// Row `b`: acc[v] = (x[v] - max) - log(sum exp(x - max)) + row_score[b]  (torch.log_softmax's form), NaN logits count as -inf;
// is_logprob: the row holds log-probabilities already, acc[v] = x[v] + row_score[b].
// Output: the M largest acc in the order (larger value, then lower v).  The threshold is the M-th largest ord_key(acc) by a 4-pass
// radix selection (integer LDS histograms), keys above it are collected, the equal ones in index order, the <= M survivors ranked in LDS.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TOPK_THREADS) void beam_topk_kernel(const float* __restrict__ logits, int V, const float* __restrict__ row_score, int M,
                                                                 float* __restrict__ cand_score, int32_t* __restrict__ cand_token, int is_logprob) {
  __shared__ float redf[16];
  __shared__ int hcnt[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_above, s_n;
  __shared__ int part[TOPK_THREADS];
  __shared__ float sv[BEAM_MAX_M];
  __shared__ int si[BEAM_MAX_M];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (int64_t)b * V;
  const SlRowScan<TOPK_THREADS> scan(row, V, tid);
  auto clean = [](float x) { return SlRowScan<TOPK_THREADS>::clean(x); };
  auto for_each = [&](auto&& f) { scan.each(f); };
  // row maximum and log-sum-exp (common.h sl_row_max_lse, shared with logits_proc.hip); a row that already holds log-probabilities
  // (is_logprob: sl_logits_process(log_softmax = 1) formed them, and the processors edited them) keeps its values: (x - 0) - 0 = x
  float m = 0.f, ls = 0.f;
  if (!is_logprob) sl_row_max_lse<TOPK_THREADS>(scan, redf, m, ls);
  const float rs = row_score ? row_score[b] : 0.f;
  auto acc = [&](float x) { const float a = ((x - m) - ls) + rs; return a != a ? -INFINITY : a; };

  // radix selection of the M-th largest key
  uint32_t prefix = 0;
  int above = 0;         // keys larger than every key matching the current prefix
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int i = tid; i < 256; i += TOPK_THREADS) hcnt[i] = 0;
    __syncthreads();
    for_each([&](int, float x) {
      const uint32_t k = beam_ord_key(acc(x));
      if ((k & hi_mask) == prefix) atomicAdd(&hcnt[(k >> shift) & 255], 1);
    });
    __syncthreads();
    if (tid == 0) {
      int run = above, sel = 0;
      for (int bin = 255; bin >= 0; --bin) {
        if (run + hcnt[bin] >= M) { sel = bin; break; }      // exists: M <= V keys match the prefix in total
        run += hcnt[bin];
      }
      s_prefix = prefix | ((uint32_t)sel << shift);
      s_above = run;
    }
    __syncthreads();
    prefix = s_prefix;
    above = s_above;
    __syncthreads();
  }
  const uint32_t kth = prefix;          // `above` (< M) keys are larger; at least M - above are equal
  if (tid == 0) s_n = 0;
  __syncthreads();
  for_each([&](int i, float x) {
    const float a = acc(x);
    if (beam_ord_key(a) > kth) {
      const int p = atomicAdd(&s_n, 1);        // arrival order is free: the survivors are ranked below
      if (p < BEAM_MAX_M) { sv[p] = a; si[p] = i; }
    }
  });
  // the equal keys, lowest indices first: thread t owns the contiguous slice [t * Cn, (t + 1) * Cn)
  const int Cn = (V + TOPK_THREADS - 1) / TOPK_THREADS;
  const int i0 = tid * Cn < V ? tid * Cn : V, i1 = (i0 + Cn) < V ? (i0 + Cn) : V;
  int eq = 0;
  for (int i = i0; i < i1; ++i) eq += beam_ord_key(acc(clean(row[i]))) == kth;
  part[tid] = eq;
  __syncthreads();
  const int need = M - above;
  if (eq > 0) {
    int before = 0;
    for (int t = 0; t < tid && before < need; ++t) before += part[t];
    if (before < need) {
      for (int i = i0; i < i1 && before < need; ++i) {
        const float a = acc(clean(row[i]));
        if (beam_ord_key(a) != kth) continue;
        const int p = above + before;
        if (p < BEAM_MAX_M) { sv[p] = a; si[p] = i; }
        ++before;
      }
    }
  }
  __syncthreads();
  // rank the M survivors: larger value first, lower index on ties
  if (tid < M) {
    const float a = sv[tid];
    const int idx = si[tid];
    int r = 0;
    for (int q = 0; q < M; ++q) r += (sv[q] > a) || (sv[q] == a && si[q] < idx);
    cand_score[(int64_t)b * M + r] = a;
    cand_token[(int64_t)b * M + r] = idx;
  }
}

// ----------------------------------------------------------------------------------------------
// One block per sequence: steps 2-7 of the beam search on device state (speechllm.h sl_beam_state).
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_step_kernel(sl_beam_state st, const float* __restrict__ cand_score, const int32_t* __restrict__ cand_token,
                                                        int K, int M, int first, BeamEos eos, int max_new, int early_stopping, int never_len) {
  __shared__ float in_sc[BEAM_MAX_K * BEAM_MAX_M];
  __shared__ int in_j[BEAM_MAX_K * BEAM_MAX_M], in_v[BEAM_MAX_K * BEAM_MAX_M];
  __shared__ float c_sc[BEAM_MAX_M];
  __shared__ int c_j[BEAM_MAX_M], c_v[BEAM_MAX_M];
  __shared__ int run_src[BEAM_MAX_K], fin_from[BEAM_MAX_K];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int t = st.step[s];
  if (t < 0 || t >= max_new) return;          // a replay past the budget touches nothing
  const int nl = first ? 1 : K, N = nl * M;
  for (int i = tid; i < N; i += 256) {
    const int l = i / M, c = i - l * M;
    const int64_t lr = first ? s : (int64_t)s * K + l;
    in_sc[i] = cand_score[lr * M + c]; in_j[i] = l; in_v[i] = cand_token[lr * M + c];
  }
  if (tid < M) { c_sc[tid] = -INFINITY; c_j[tid] = 0; c_v[tid] = 0; }
  __syncthreads();
  // the M best of the N list entries: larger score, then lower flat index (beam, token)
  for (int i = tid; i < N; i += 256) {
    const float a = in_sc[i];
    const int j = in_j[i], v = in_v[i];
    int r = 0;
    for (int q = 0; q < N; ++q) {
      const float bq = in_sc[q];
      r += (bq > a) || (bq == a && (in_j[q] < j || (in_j[q] == j && in_v[q] < v)));
    }
    if (r < M) { c_sc[r] = a; c_j[r] = j; c_v[r] = v; }
  }
  __syncthreads();
  const int64_t r0 = (int64_t)s * K;
  if (tid == 0) {
    const bool last = (t + 1 == max_new);
    uint64_t hit = 0;
    for (int c = 0; c < M; ++c) {
      bool h = last;
      for (int e = 0; e < eos.n; ++e) h = h || (c_v[c] == eos.ids[e]);
      if (h) hit |= 1ull << c;
    }
    // next running beams: top-K of score + (hit ? -1e9 : 0), candidate order on ties
    float new_run[BEAM_MAX_K];
    uint64_t used = 0;
    for (int k = 0; k < K; ++k) {
      int best = -1;
      float bv = 0.f;
      for (int c = 0; c < M; ++c) {
        if ((used >> c) & 1) continue;
        const float rv = c_sc[c] + (((hit >> c) & 1) ? -1.0e9f : 0.f);
        if (best < 0 || rv > bv) { best = c; bv = rv; }
      }
      used |= 1ull << best;
      run_src[k] = best; new_run[k] = bv;
    }
    // finished set: top-K of [old K | M candidates], concatenation order on ties
    bool allfin = true;
    float old_fs[BEAM_MAX_K];
    int old_flag[BEAM_MAX_K], old_len[BEAM_MAX_K];
    for (int i = 0; i < K; ++i) { old_fs[i] = st.fin_score[r0 + i]; old_flag[i] = st.fin_flag[r0 + i]; old_len[i] = st.fin_len[r0 + i]; allfin = allfin && old_flag[i] != 0; }
    const bool full = allfin && early_stopping == 1;
    bool opn = st.open[s] != 0;
    const float lp = st.len_pen[t];
    float new_fs[BEAM_MAX_K];
    int new_flag[BEAM_MAX_K], new_len[BEAM_MAX_K];
    uint64_t usedc = 0;
    uint32_t usedo = 0;
    for (int p = 0; p < K; ++p) {
      int best = -1;
      float bv = 0.f;
      for (int i = 0; i < K + M; ++i) {
        float v;
        if (i < K) {
          if ((usedo >> i) & 1) continue;
          v = old_fs[i];
        } else {
          const int c = i - K;
          if ((usedc >> c) & 1) continue;
          v = c_sc[c] / lp;
          v += full ? -1.0e9f : 0.f;
          v += !opn ? -1.0e9f : 0.f;
          v += !(c < K && ((hit >> c) & 1)) ? -1.0e9f : 0.f;
        }
        if (best < 0 || v > bv) { best = i; bv = v; }
      }
      fin_from[p] = best; new_fs[p] = bv;
      if (best < K) { usedo |= 1u << best; new_flag[p] = old_flag[best]; new_len[p] = old_len[best]; }
      else { const int c = best - K; usedc |= 1ull << c; new_flag[p] = (c < K && ((hit >> c) & 1)) ? 1 : 0; new_len[p] = t + 1; }
    }
    bool allnew = true;
    float worst = new_fs[0];
    for (int p = 0; p < K; ++p) {
      st.fin_score[r0 + p] = new_fs[p]; st.fin_flag[r0 + p] = new_flag[p]; st.fin_len[r0 + p] = new_len[p];
      allnew = allnew && new_flag[p] != 0;
      worst = fminf(worst, new_fs[p]);
    }
    if (!allnew) worst = -1.0e9f;
    const float lpo = never_len ? st.len_pen[max_new - 1] : lp;
    opn = opn && (new_run[0] / lpo > worst);
    st.open[s] = opn ? 1 : 0;
    if (!opn || (early_stopping == 1 && allnew) || last) st.seq_done[s] = 1;
    for (int k = 0; k < K; ++k) {
      const int c = run_src[k];
      st.run_score[r0 + k] = new_run[k];
      st.next_ids[r0 + k] = c_v[c];
      st.src_row[r0 + k] = (int32_t)(r0 + c_j[c]);
      if (!first) st.ctx_len[r0 + k] += 1;
    }
    st.step[s] = t + 1;
  }
  __syncthreads();
  const int32_t* ho = (t & 1) ? st.hist[1] : st.hist[0];
  int32_t* hn = (t & 1) ? st.hist[0] : st.hist[1];
  for (int k = 0; k < K; ++k) {
    const int c = run_src[k];
    const int32_t* src = ho + (r0 + c_j[c]) * max_new;
    int32_t* dst = hn + (r0 + k) * max_new;
    for (int i = tid; i <= t; i += 256) dst[i] = i < t ? src[i] : c_v[c];
  }
  // finished histories, in place: an old entry only ever moves down (the set stays sorted), so walking the places from the last to the
  // first never reads a row that was already rewritten
  for (int p = K - 1; p >= 0; --p) {
    const int from = fin_from[p];
    int32_t* dst = st.fin_ids + (r0 + p) * max_new;
    if (from < K) {
      if (from != p) {
        const int32_t* src = st.fin_ids + (r0 + from) * max_new;
        for (int i = tid; i < max_new; i += 256) dst[i] = src[i];
      }
    } else {
      const int c = from - K;
      const int32_t* src = ho + (r0 + c_j[c]) * max_new;
      for (int i = tid; i <= t; i += 256) dst[i] = i < t ? src[i] : c_v[c];
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------
// Cache re-ordering: grid (row, layer * n_kv).  Positions [prompt_len[row], ctx_len[row]) of slot src_row[row] -> staging (gather), then
// staging -> slot row (scatter).  Rows that keep their slot do nothing.  16-byte units of the cache's own bytes (either K/V format).
// ----------------------------------------------------------------------------------------------
template <bool GATHER>
__global__ __launch_bounds__(256) void kv_beam_move_kernel(uint4* __restrict__ kc, uint4* __restrict__ vc, uint4* __restrict__ stage_k, uint4* __restrict__ stage_v,
                                                           const int32_t* __restrict__ src_row, const int32_t* __restrict__ prompt_len,
                                                           const int32_t* __restrict__ ctx_len, int rows, int nkv, int n_lh, int slots, int max_ctx,
                                                           int row_vec, int max_span) {
  const int r = blockIdx.x, lh = blockIdx.y;
  const int src = src_row[r];
  if (src == r || src < 0 || src >= rows) return;
  const int p0 = prompt_len[r];
  int span = ctx_len[r] - p0;
  if (p0 < 0 || span <= 0) return;
  if (span > max_span) span = max_span;
  if (span > max_ctx - p0) span = max_ctx - p0;
  if (span <= 0) return;
  const int l = lh / nkv, h = lh - l * nkv;
  const int slot = GATHER ? src : r;
  const int64_t c0 = ((((int64_t)l * slots + slot) * nkv + h) * max_ctx + p0) * row_vec;
  const int64_t s0 = ((int64_t)r * n_lh + lh) * max_span * row_vec;
  const int n = span * row_vec;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (GATHER) { stage_k[s0 + i] = kc[c0 + i]; stage_v[s0 + i] = vc[c0 + i]; }
    else { kc[c0 + i] = stage_k[s0 + i]; vc[c0 + i] = stage_v[s0 + i]; }
  }
}

}  // namespace

int sl_beam_topk_impl(const float* logits, int32_t rows, int32_t V, const float* row_score, int32_t M, float* cand_score, int32_t* cand_token,
                      hipStream_t st, int is_logprob) {
  SL_CHECK_ARG(logits && cand_score && cand_token && rows > 0 && V > 0, "sl_beam_topk: bad arguments");
  SL_CHECK_ARG(M >= 1 && M <= BEAM_MAX_M && M <= V, "sl_beam_topk: M = %d outside [1, min(%d, V = %d)]", M, BEAM_MAX_M, V);
  hipLaunchKernelGGL(beam_topk_kernel, dim3(rows), dim3(TOPK_THREADS), 0, st, logits, V, row_score, M, cand_score, cand_token, is_logprob ? 1 : 0);
  SL_CHECK_LAUNCH("beam_topk");
  return 0;
}

// M of a beam search: max(2, 1 + n_eos) * num_beams candidates kept per step
int sl_beam_m(int num_beams, int n_eos) { return (n_eos + 1 > 2 ? n_eos + 1 : 2) * num_beams; }

int sl_beam_step_impl(const sl_beam_state* s, const float* cand_score, const int32_t* cand_token, int32_t nseq, int32_t K, int32_t M, int32_t first,
                      const sl_beam_opts* o, hipStream_t st) {
  SL_CHECK_ARG(s && cand_score && cand_token && o && nseq > 0, "sl_beam_step: bad arguments");
  SL_CHECK_ARG(s->run_score && s->next_ids && s->src_row && s->ctx_len && s->hist[0] && s->hist[1] && s->fin_score && s->fin_ids && s->fin_flag &&
               s->fin_len && s->open && s->seq_done && s->step && s->len_pen, "sl_beam_step: null state field");
  SL_CHECK_ARG(K >= 1 && K <= BEAM_MAX_K && K == o->num_beams, "sl_beam_step: num_beams %d outside [1, %d] (opts say %d)", K, BEAM_MAX_K, o->num_beams);
  SL_CHECK_ARG(M >= K && M <= BEAM_MAX_M, "sl_beam_step: M = %d outside [num_beams = %d, %d]", M, K, BEAM_MAX_M);
  SL_CHECK_ARG(o->max_new_tokens > 0 && o->early_stopping >= 0 && o->early_stopping <= 2, "sl_beam_step: max_new_tokens > 0, early_stopping in {0, 1, 2}");
  const int n_eos = o->use_eos ? o->n_eos : 0;
  SL_CHECK_ARG(n_eos >= 0 && n_eos <= 8 && (n_eos == 0 || o->eos_ids_host), "sl_beam_step: 0..8 eos ids");
  BeamEos e;
  e.n = n_eos;
  for (int i = 0; i < 8; ++i) e.ids[i] = i < n_eos ? o->eos_ids_host[i] : -1;
  hipLaunchKernelGGL(beam_step_kernel, dim3(nseq), dim3(256), 0, st, *s, cand_score, cand_token, K, M, first ? 1 : 0, e, o->max_new_tokens, o->early_stopping,
                     (o->early_stopping == 2 && o->length_penalty > 0.f) ? 1 : 0);
  SL_CHECK_LAUNCH("beam_step");
  return 0;
}

size_t sl_kv_beam_staging_bytes_impl(const sl_kv_cache* kv, const sl_llama_model* m, int32_t rows, int32_t max_span) {
  const size_t row_bytes = (size_t)m->head_dim * sl_kv_elem_size(kv->reserved, m->dtype);
  return 2 * (size_t)rows * m->n_layers * m->n_kv_heads * (size_t)max_span * row_bytes;
}

int sl_kv_beam_reorder_impl(const sl_kv_cache* kv, const sl_llama_model* m, const int32_t* src_row, const int32_t* prompt_len, const int32_t* ctx_len,
                            int32_t rows, int32_t max_span, void* staging, size_t staging_bytes, hipStream_t st) {
  SL_CHECK_ARG(kv && m && src_row && prompt_len && ctx_len && staging && kv->k_cache && kv->v_cache, "sl_kv_beam_reorder: bad arguments");
  SL_CHECK_ARG(rows > 0 && rows <= kv->slots && max_span > 0 && max_span <= kv->max_ctx, "sl_kv_beam_reorder: rows %d outside (0, slots = %d] or max_span %d outside (0, max_ctx = %d]",
               rows, kv->slots, max_span, kv->max_ctx);
  if (kv->reserved != SL_KV_MODEL_DTYPE) SL_TRY(sl_kv_format_check("sl_kv_beam_reorder (sl_kv_cache.reserved)", kv->reserved, m->dtype, m->head_dim));
  const size_t row_bytes = (size_t)m->head_dim * sl_kv_elem_size(kv->reserved, m->dtype);
  SL_CHECK_ARG(row_bytes % 16 == 0 && m->n_layers > 0 && m->n_kv_heads > 0, "sl_kv_beam_reorder: K / V rows must be a multiple of 16 bytes");
  SL_CHECK_ARG((((uintptr_t)staging) & 15) == 0, "sl_kv_beam_reorder: staging must be 16-byte aligned");
  const size_t need = sl_kv_beam_staging_bytes_impl(kv, m, rows, max_span);
  SL_CHECK_ARG(staging_bytes >= need, "sl_kv_beam_reorder: staging %zu B < required %zu B", staging_bytes, need);
  const int n_lh = m->n_layers * m->n_kv_heads, row_vec = (int)(row_bytes / 16);
  uint4* sk = (uint4*)staging;
  uint4* sv = (uint4*)((unsigned char*)staging + need / 2);
  const dim3 grid(rows, n_lh);
  hipLaunchKernelGGL(kv_beam_move_kernel<true>, grid, dim3(256), 0, st, (uint4*)kv->k_cache, (uint4*)kv->v_cache, sk, sv, src_row, prompt_len, ctx_len, rows,
                     m->n_kv_heads, n_lh, kv->slots, kv->max_ctx, row_vec, max_span);
  SL_CHECK_LAUNCH("kv_beam_gather");
  hipLaunchKernelGGL(kv_beam_move_kernel<false>, grid, dim3(256), 0, st, (uint4*)kv->k_cache, (uint4*)kv->v_cache, sk, sv, src_row, prompt_len, ctx_len, rows,
                     m->n_kv_heads, n_lh, kv->slots, kv->max_ctx, row_vec, max_span);
  SL_CHECK_LAUNCH("kv_beam_scatter");
  return 0;
}

extern "C" int sl_beam_topk(const float* logits, int32_t rows, int32_t V, const float* row_score, int32_t M, float* cand_score, int32_t* cand_token,
                            sl_stream stream) {
  return sl_beam_topk_impl(logits, rows, V, row_score, M, cand_score, cand_token, (hipStream_t)stream, 0);
}

extern "C" int sl_beam_topk_ex(const float* logits, int32_t rows, int32_t V, const float* row_score, int32_t M, float* cand_score, int32_t* cand_token,
                               sl_stream stream, int32_t is_logprob) {
  return sl_beam_topk_impl(logits, rows, V, row_score, M, cand_score, cand_token, (hipStream_t)stream, is_logprob);
}

extern "C" int sl_beam_step(const sl_beam_state* state, const float* cand_score, const int32_t* cand_token, int32_t nseq, int32_t num_beams, int32_t M,
                            int32_t first, const sl_beam_opts* opts, sl_stream stream) {
  return sl_beam_step_impl(state, cand_score, cand_token, nseq, num_beams, M, first, opts, (hipStream_t)stream);
}

extern "C" size_t sl_kv_beam_staging_bytes(const sl_kv_cache* kv, const sl_llama_model* m, int32_t rows, int32_t max_span) {
  if (!kv || !m || rows <= 0 || max_span <= 0) { sl_set_error("sl_kv_beam_staging_bytes: bad arguments"); return 0; }
  return sl_kv_beam_staging_bytes_impl(kv, m, rows, max_span);
}

extern "C" int sl_kv_beam_reorder(const sl_kv_cache* kv, const sl_llama_model* m, const int32_t* src_row_dev, const int32_t* prompt_len_dev,
                                  const int32_t* ctx_len_dev, int32_t rows, int32_t max_span, void* staging, size_t staging_bytes, sl_stream stream) {
  return sl_kv_beam_reorder_impl(kv, m, src_row_dev, prompt_len_dev, ctx_len_dev, rows, max_span, staging, staging_bytes, (hipStream_t)stream);
}
