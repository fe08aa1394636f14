// logits_proc.hip — HF's logits processors on the device (hf:generation/utils.py _get_logits_processor, classes in
// hf:generation/logits_process.py; restated in tests/logits_proc_ref.py), in HF's order, in place on the fp32 logits of a decode step:
//   0. (beam search) log_softmax of the row: HF's _beam_search hands the processors log-probabilities, not raw logits
//   1. RepetitionPenaltyLogitsProcessor     every token of the row's history: s < 0 ? s * p : s / p, once however often it occurs
//   2. NoRepeatNGramLogitsProcessor         every token that would complete an n-gram the history already holds: -inf
//   3. MinNewTokensLengthLogitsProcessor    the EOS ids while the history is shorter than min_new_tokens: -inf
// One block per decode row.  A row's history is hist[row][0 .. hist_len[row]): the tokens it has GENERATED (the prompt is embeddings and is
// never penalised, as in the reference, whose input_ids start empty).  No float atomics: a row's output is the same on every run.
#include <cmath>

#include "common.h"

namespace {

struct LpEos { int n; int ids[8]; };

constexpr int LP_THREADS_RAW = 256;        // raw logits: the work is a few passes over the history
constexpr int LP_THREADS_LSM = 1024;       // log_softmax first: beam_topk_kernel's block, so that both reduce the row in one order

template <int THREADS, bool LSM>
__global__ __launch_bounds__(THREADS) void logits_process_kernel(float* __restrict__ logits, int V, const int32_t* __restrict__ hist_even,
                                                                 const int32_t* __restrict__ hist_odd, int64_t hist_ld,
                                                                 const int32_t* __restrict__ hist_len, const int32_t* __restrict__ unfinished,
                                                                 float penalty, int ngram, int min_new, LpEos eos, float* __restrict__ scratch) {
  __shared__ float redf[THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (unfinished && unfinished[b] == 0) return;        // the select kernels emit pad_id for the row whatever its logits are
  float* row = logits + (int64_t)b * V;
  int n = hist_len[b];
  n = n < 0 ? 0 : (n > hist_ld ? (int)hist_ld : n);
  // the beam search keeps two histories and swaps them every step: a history of odd length lives in the second (sl_beam_state.hist)
  const int32_t* h = ((n & 1) && hist_odd ? hist_odd : hist_even) + (int64_t)b * hist_ld;

  if constexpr (LSM) {
    const SlRowScan<THREADS> scan(row, V, tid);
    float m, ls;
    sl_row_max_lse<THREADS>(scan, redf, m, ls);
    // each thread rewrites exactly the elements it read (the barriers inside sl_row_max_lse separate the last read of the raw row)
    scan.each([&](int i, float x) {
      const float a = (x - m) - ls;
      row[i] = a != a ? -INFINITY : a;
    });
    __syncthreads();
  }

  // 1. repetition penalty: gather the originals of every history entry, barrier, scatter f(original) — a token that occurs twice is
  //    written twice with the same value (HF gathers, then scatters), never penalised twice
  if (penalty != 1.0f && n > 0) {
    float* orig = scratch + (int64_t)b * hist_ld;
    for (int j = tid; j < n; j += THREADS) {
      const int tok = h[j];
      if (tok >= 0 && tok < V) orig[j] = row[tok];
    }
    __syncthreads();
    for (int j = tid; j < n; j += THREADS) {
      const int tok = h[j];
      if (tok >= 0 && tok < V) {
        const float s = orig[j];
        row[tok] = s < 0.f ? s * penalty : s / penalty;      // IEEE division: never a reciprocal multiply
      }
    }
    __syncthreads();          // a ban below overrides a penalty
  }

  // 2. no-repeat n-gram: window starts i in [0, n - g]; the last g - 1 tokens are the prefix (empty for g = 1: every token is banned)
  if (ngram > 0 && n >= ngram) {
    const int g = ngram, p0 = n - g + 1;
    for (int i = tid; i <= n - g; i += THREADS) {
      bool same = true;
      for (int k = 0; k < g - 1 && same; ++k) same = h[i + k] == h[p0 + k];
      if (same) {
        const int tok = h[i + g - 1];
        if (tok >= 0 && tok < V) row[tok] = -INFINITY;       // several windows may ban one token: they all write the same value
      }
    }
  }

  // 3. min_new_tokens: no EOS yet
  if (n < min_new && tid < eos.n) {
    const int tok = eos.ids[tid];
    if (tok >= 0 && tok < V) row[tok] = -INFINITY;
  }
}

}  // namespace

int sl_logits_opts_check(const char* who, const sl_logits_opts* lp, int max_new_tokens) {
  if (!lp) return 0;
  SL_CHECK_ARG(std::isfinite(lp->repetition_penalty) && lp->repetition_penalty > 0.f, "%s: repetition_penalty %g must be finite and > 0 (1.0 = off)", who,
               (double)lp->repetition_penalty);
  SL_CHECK_ARG(lp->no_repeat_ngram_size >= 0, "%s: no_repeat_ngram_size %d must be >= 0 (0 = off)", who, lp->no_repeat_ngram_size);
  SL_CHECK_ARG(lp->min_new_tokens >= 0, "%s: min_new_tokens %d must be >= 0 (0 = off)", who, lp->min_new_tokens);
  SL_CHECK_ARG(max_new_tokens < 0 || lp->min_new_tokens <= max_new_tokens, "%s: min_new_tokens %d exceeds max_new_tokens %d", who, lp->min_new_tokens,
               max_new_tokens);
  return 0;
}

// hist_odd: NULL, or the history buffer of the rows whose history has an odd length (the beam search's second buffer)
int sl_logits_process_impl(float* logits, int32_t rows, int32_t V, const int32_t* hist, const int32_t* hist_odd, int64_t hist_ld, const int32_t* hist_len,
                           const int32_t* unfinished, const sl_logits_opts* lp, const int32_t* eos_ids_host, int32_t n_eos, int32_t log_softmax,
                           float* scratch, hipStream_t st) {
  SL_CHECK_ARG(lp != nullptr, "sl_logits_process: null options");
  SL_TRY(sl_logits_opts_check("sl_logits_process", lp, -1));
  SL_CHECK_ARG(n_eos >= 0 && n_eos <= 8 && (n_eos == 0 || eos_ids_host != nullptr), "sl_logits_process: 0..8 eos ids (n_eos = %d)", n_eos);
  SL_CHECK_ARG(logits && hist_len && rows > 0 && V > 0 && hist_ld >= 0, "sl_logits_process: bad arguments (logits, hist_len, rows > 0, V > 0, hist_ld >= 0)");
  SL_CHECK_ARG(hist != nullptr || hist_ld == 0, "sl_logits_process: null history with hist_ld = %lld", (long long)hist_ld);
  const bool pen = lp->repetition_penalty != 1.0f;
  SL_CHECK_ARG(!pen || hist_ld == 0 || scratch != nullptr, "sl_logits_process: repetition_penalty needs a scratch of rows * hist_ld floats");
  const int min_new = n_eos > 0 ? lp->min_new_tokens : 0;
  if (!log_softmax && !pen && lp->no_repeat_ngram_size == 0 && min_new == 0) return 0;       // nothing to do: no launch
  LpEos e;
  e.n = n_eos;
  for (int i = 0; i < 8; ++i) e.ids[i] = i < n_eos ? eos_ids_host[i] : -1;
  if (log_softmax) {
    hipLaunchKernelGGL((logits_process_kernel<LP_THREADS_LSM, true>), dim3(rows), dim3(LP_THREADS_LSM), 0, st, logits, V, hist, hist_odd, hist_ld, hist_len,
                       unfinished, lp->repetition_penalty, lp->no_repeat_ngram_size, min_new, e, scratch);
  } else {
    hipLaunchKernelGGL((logits_process_kernel<LP_THREADS_RAW, false>), dim3(rows), dim3(LP_THREADS_RAW), 0, st, logits, V, hist, hist_odd, hist_ld, hist_len,
                       unfinished, lp->repetition_penalty, lp->no_repeat_ngram_size, min_new, e, scratch);
  }
  SL_CHECK_LAUNCH("logits_process");
  return 0;
}

extern "C" int sl_logits_process(float* logits, int32_t rows, int32_t V, const int32_t* hist, int64_t hist_ld, const int32_t* hist_len,
                                 const int32_t* unfinished, const sl_logits_opts* lp, const int32_t* eos_ids_host, int32_t n_eos, int32_t log_softmax,
                                 float* scratch, sl_stream stream) {
  return sl_logits_process_impl(logits, rows, V, hist, nullptr, hist_ld, hist_len, unfinished, lp, eos_ids_host, n_eos, log_softmax, scratch,
                                (hipStream_t)stream);
}
