// score.hip — teacher-forced scoring: the log-probability of a GIVEN token per row, from the planes a fused lm_head left
// (sl_gemm_top1_lse_tgt -> sl_score_finalize) or from fp32 logits (sl_score_rows), and the per-sequence sums (sl_score_segment_sums).
// A label outside [0, V) marks an ignored position (HF's -100): its log-probability is 0.0f, it is counted nowhere, and nothing is read
// at its place — neither tgt_val[row] nor logits[row][label].  NaN counts as -inf; every sum has one fixed order, no float atomics.
#include "common.h"

// ----------------------------------------------------------------------------------------------
// planes -> log-probability and top-1.  The layout of greedy_select_partial_kernel (select.hip): block = 32 rows x 32 group stripes,
// eight groups in flight per thread, the stripes meet in LDS in stripe order; compare rule: larger value, then lower column.
//   m = max_g val_g, total = sum_g sum_g * expf(val_g - m) (a stripe's groups in index order, then the stripes in order),
//   logprob = (tgt - m) - logf(total)
// A row without a finite maximum gives a non-finite value (m = -inf: total = 0).
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void score_finalize_kernel(const float* __restrict__ pv, const int32_t* __restrict__ pi, const float* __restrict__ ps,
                                                              int n_groups, int V, const float* __restrict__ tgt_val, const int32_t* __restrict__ labels,
                                                              int rows, float* __restrict__ logprob_out, int32_t* __restrict__ top1_out) {
  constexpr int ROWS = 32, STRIPES = 32, U = 8;
  __shared__ float sv[STRIPES][ROWS];
  __shared__ int si[STRIPES][ROWS];
  __shared__ float ss[STRIPES][ROWS];
  const int lr = threadIdx.x & (ROWS - 1), stripe = threadIdx.x / ROWS;
  const int b = blockIdx.x * ROWS + lr;
  const int bc = b < rows ? b : rows - 1;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int g0 = stripe; g0 < n_groups; g0 += STRIPES * U) {
    float v[U];
    int ix[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int g = g0 + u * STRIPES;
      const int64_t at = (int64_t)(g < n_groups ? g : n_groups - 1) * rows + bc;
      v[u] = pv[at];
      ix[u] = pi[at];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (g0 + u * STRIPES >= n_groups) continue;
      if (v[u] > best || (v[u] == best && ix[u] < bi)) { best = v[u]; bi = ix[u]; }
    }
  }
  sv[stripe][lr] = best;
  si[stripe][lr] = bi;
  __syncthreads();
  float mx = sv[0][lr];
  for (int s2 = 1; s2 < STRIPES; ++s2) mx = fmaxf(mx, sv[s2][lr]);
  float acc = 0.f;
  for (int g0 = stripe; g0 < n_groups; g0 += STRIPES * U) {
    float v[U], sg[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int g = g0 + u * STRIPES;
      const int64_t at = (int64_t)(g < n_groups ? g : n_groups - 1) * rows + bc;
      v[u] = pv[at];
      sg[u] = ps[at];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (g0 + u * STRIPES >= n_groups) continue;
      if (v[u] != -INFINITY) acc += sg[u] * expf(v[u] - mx);      // a group of nothing but -inf / NaN holds sum 0 and takes no part
    }
  }
  ss[stripe][lr] = acc;
  __syncthreads();
  if (stripe != 0 || b >= rows) return;
  float total = 0.f;
  for (int s2 = 0; s2 < STRIPES; ++s2) total += ss[s2][lr];
  for (int s2 = 1; s2 < STRIPES; ++s2)
    if (sv[s2][lr] > best || (sv[s2][lr] == best && si[s2][lr] < bi)) { best = sv[s2][lr]; bi = si[s2][lr]; }
  if (bi == 0x7fffffff) bi = 0;
  if (top1_out) top1_out[b] = bi;
  const int lab = labels[b];
  float lp = 0.f;
  if (lab >= 0 && lab < V) {      // an ignored label reads nothing: tgt_val[b] is whatever it was
    float t = tgt_val[b];
    if (t != t) t = -INFINITY;
    lp = (t - mx) - logf(total);
  }
  logprob_out[b] = lp;
}

// ----------------------------------------------------------------------------------------------
// fp32 logits -> log-probability and top-1: one block per row.  The top-1 is greedy_select_kernel's scan (raw values: NaN never wins, the
// first maximum wins, -inf columns included); the log-softmax goes through the row reduce sl_greedy_select_sc / sl_logits_process use
// (common.h sl_row_max_lse): logprob = (x[label] - m) - ls.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void score_rows_kernel(const float* __restrict__ logits, int64_t ld, int V, const int32_t* __restrict__ labels,
                                                          float* __restrict__ logprob_out, int32_t* __restrict__ top1_out) {
  __shared__ float smax[16];
  __shared__ int sidx[16];
  __shared__ float redf[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (int64_t)b * ld;
  const SlRowScan<1024> scan(row, V, tid);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  auto upd = [&](float v, int i) {
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  };
  if (scan.vec) {
    const float4* row4 = (const float4*)row;
    for (int i = tid; i < (V >> 2); i += 1024) {
      const float4 v = row4[i];
      upd(v.x, 4 * i); upd(v.y, 4 * i + 1); upd(v.z, 4 * i + 2); upd(v.w, 4 * i + 3);
    }
  } else {
    for (int i = tid; i < V; i += 1024) upd(row[i], i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { smax[wave] = best; sidx[wave] = bi; }
  __syncthreads();
  float row_m = 0.f, row_ls = 0.f;
  sl_row_max_lse<1024>(scan, redf, row_m, row_ls);
  if (tid != 0) return;
  for (int w = 1; w < 16; ++w)
    if (smax[w] > best || (smax[w] == best && sidx[w] < bi)) { best = smax[w]; bi = sidx[w]; }
  if (bi == 0x7fffffff) bi = 0;
  if (top1_out) top1_out[b] = bi;
  const int lab = labels[b];
  float lp = 0.f;
  if (lab >= 0 && lab < V) {      // an ignored label reads nothing at its place
    const float t = SlRowScan<1024>::clean(row[lab]);
    lp = (t - row_m) - row_ls;
  }
  logprob_out[b] = lp;
}

// ----------------------------------------------------------------------------------------------
// per-sequence sums over rows [row_offsets[s], row_offsets[s + 1]): one block of 256 threads per sequence.  A thread adds its rows
// (t, t + 256, ...) in order, the xor butterfly inside the wave, the four waves in order: one fixed order.  Ignored rows (label outside
// [0, V)) count in neither the sum nor the counters; the counters are exact integers.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_segment_sums_kernel(const float* __restrict__ logprob, const int32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ top1, const int32_t* __restrict__ row_offsets, int V,
                                                                 float* __restrict__ sum_logprob, int32_t* __restrict__ n_counted, int32_t* __restrict__ n_top1) {
  __shared__ float sf[4];
  __shared__ int sc[4], st1[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = row_offsets[s], r1 = row_offsets[s + 1];
  float sum = 0.f;
  int cnt = 0, hit = 0;
  for (int r = r0 + tid; r < r1; r += 256) {
    const int lab = labels[r];
    if (lab < 0 || lab >= V) continue;
    sum += logprob[r];
    cnt += 1;
    if (top1 && top1[r] == lab) hit += 1;
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); hit += __shfl_xor(hit, o, 64); }
  if (lane == 0) { sf[wave] = sum; sc[wave] = cnt; st1[wave] = hit; }
  __syncthreads();
  if (tid != 0) return;
  float t = 0.f;
  int c = 0, h = 0;
  for (int w = 0; w < 4; ++w) { t += sf[w]; c += sc[w]; h += st1[w]; }
  sum_logprob[s] = t;
  n_counted[s] = c;
  if (n_top1) n_top1[s] = h;
}

int sl_score_finalize_impl(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t V, const float* tgt_val,
                           const int32_t* labels, int32_t rows, float* logprob_out, int32_t* top1_out, hipStream_t st) {
  SL_CHECK_ARG(amax_val && amax_idx && amax_sum && tgt_val && labels && logprob_out, "sl_score_finalize: null pointer");
  SL_CHECK_ARG(rows > 0 && n_groups > 0 && V > 0, "sl_score_finalize: bad shape rows=%d n_groups=%d V=%d", rows, n_groups, V);
  SL_CHECK_ARG(n_groups == (V + 63) / 64, "sl_score_finalize: n_groups=%d is not ceil(V / 64) for V=%d", n_groups, V);
  hipLaunchKernelGGL(score_finalize_kernel, dim3((rows + 31) / 32), dim3(1024), 0, st, amax_val, amax_idx, amax_sum, n_groups, V, tgt_val, labels, rows, logprob_out,
                     top1_out);
  SL_CHECK_LAUNCH("score_finalize");
  return 0;
}

int sl_score_rows_impl(const float* logits, int64_t ld, const int32_t* labels, int32_t rows, int32_t V, float* logprob_out, int32_t* top1_out, hipStream_t st) {
  SL_CHECK_ARG(logits && labels && logprob_out, "sl_score_rows: null pointer");
  SL_CHECK_ARG(rows > 0 && V > 0 && ld >= V, "sl_score_rows: bad shape rows=%d V=%d ld=%lld", rows, V, (long long)ld);
  hipLaunchKernelGGL(score_rows_kernel, dim3(rows), dim3(1024), 0, st, logits, ld, V, labels, logprob_out, top1_out);
  SL_CHECK_LAUNCH("score_rows");
  return 0;
}

int sl_score_segment_sums_impl(const float* logprob, const int32_t* labels, const int32_t* top1, const int32_t* row_offsets, int32_t nseq, int32_t V,
                               float* sum_logprob, int32_t* n_counted, int32_t* n_top1, hipStream_t st) {
  SL_CHECK_ARG(logprob && labels && row_offsets && sum_logprob && n_counted, "sl_score_segment_sums: null pointer");
  SL_CHECK_ARG((top1 != nullptr) == (n_top1 != nullptr), "sl_score_segment_sums: top1 and n_top1 come together");
  SL_CHECK_ARG(nseq > 0 && V > 0, "sl_score_segment_sums: bad shape nseq=%d V=%d", nseq, V);
  hipLaunchKernelGGL(score_segment_sums_kernel, dim3(nseq), dim3(256), 0, st, logprob, labels, top1, row_offsets, V, sum_logprob, n_counted, n_top1);
  SL_CHECK_LAUNCH("score_segment_sums");
  return 0;
}

extern "C" int sl_score_finalize(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t vocab, const float* tgt_val,
                                 const int32_t* labels, int32_t rows, float* logprob_out, int32_t* top1_out, sl_stream stream) {
  return sl_score_finalize_impl(amax_val, amax_idx, amax_sum, n_groups, vocab, tgt_val, labels, rows, logprob_out, top1_out, (hipStream_t)stream);
}

extern "C" int sl_score_rows(const float* logits, int64_t ld, const int32_t* labels, int32_t rows, int32_t vocab, float* logprob_out, int32_t* top1_out,
                             sl_stream stream) {
  return sl_score_rows_impl(logits, ld, labels, rows, vocab, logprob_out, top1_out, (hipStream_t)stream);
}

extern "C" int sl_score_segment_sums(const float* logprob, const int32_t* labels, const int32_t* top1, const int32_t* row_offsets, int32_t nseq, int32_t vocab,
                                     float* sum_logprob, int32_t* n_counted, int32_t* n_top1, sl_stream stream) {
  return sl_score_segment_sums_impl(logprob, labels, top1, row_offsets, nseq, vocab, sum_logprob, n_counted, n_top1, (hipStream_t)stream);
}
