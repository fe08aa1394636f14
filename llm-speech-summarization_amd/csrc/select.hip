// select.hip — token selection, one block per sequence row: greedy (over fp32 logits, and over the partial maxima a fused lm_head left),
// the sampler and the bookkeeping every select ends with.  HBM/latency-bound; fp32 math.
#include "common.h"

struct EosList { int ids[8]; int n; };

// The bookkeeping every select ends with, by the one thread that holds row b's token: pad for a finished row (hf:generation/utils.py:2928-2929),
// out_ids[b][gen_count], the counters, EOS / the row's own budget (a spent budget finishes the row like an EOS), the context.
// SC: the token's log-probability `lp` goes to logprob_out[b][gen_count], 0 for a finished row; LP = false (sampling: the draw left it there
// already) only writes that 0.
// rs travels to every kernel by value: the state pointers and scalars are the device's to read, rs.eos_ids is a HOST pointer (the ids come in
// an EosList) — never read rs.eos_ids / rs.n_eos in device code.
template <bool SC, bool LP = true>
__device__ __forceinline__ void select_commit(const SlRowState& rs, const EosList& eos, int b, int tok, float lp = 0.f) {
  const int unf = rs.unfinished[b];
  if (rs.use_eos) tok = unf ? tok : rs.pad_id;
  const int n = rs.gen_count[b];
  if constexpr (SC) {
    if (n < rs.max_new && (LP || (rs.use_eos && !unf))) rs.logprob_out[(int64_t)b * rs.max_new + n] = (rs.use_eos && !unf) ? 0.f : lp;
  }
  if (n < rs.max_new) rs.out_ids[(int64_t)b * rs.max_new + n] = tok;
  rs.gen_count[b] = n + 1;
  rs.next_ids[b] = tok;
  if (rs.use_eos && unf) {
    bool is_eos = false;
    for (int e = 0; e < eos.n; ++e) is_eos |= (tok == eos.ids[e]);
    if (rs.row_limit) is_eos |= (n + 1 >= rs.row_limit[b]);
    if (is_eos) { rs.unfinished[b] = 0; rs.finish_len[b] = n + 1; }
  }
  if (rs.advance_ctx) rs.ctx_len[b] += 1;
}

// The sampler's second launch: row b commits choice[b], the token its draw left there.  With SC the draw has also left the token's
// log-probability in place; the commit only zeroes it for a finished row.
template <bool SC>
__global__ __launch_bounds__(64) void select_commit_kernel(EosList eos, SlRowState rs, const int32_t* __restrict__ choice) {
  if (threadIdx.x == 0) select_commit<SC, false>(rs, eos, blockIdx.x, choice[blockIdx.x]);
}

// ----------------------------------------------------------------------------------------------
// greedy selection: one block per sequence row
// SC (token log-probabilities): logprob_out[b][gen_count] = log_softmax(row)[token] through the row reduce beam search and the
// logits processors use (common.h sl_row_max_lse), 0 for a finished row.  SC = false is the kernel as it was.
// ----------------------------------------------------------------------------------------------
template <bool SC>
__global__ __launch_bounds__(1024) void greedy_select_kernel(const float* __restrict__ logits, int V, EosList eos, SlRowState rs) {
  __shared__ float smax[16];
  __shared__ int sidx[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (int64_t)b * V;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  auto upd = [&](float v, int i) {
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }   // NaN never wins, like a strict '>' scan
  };
  if ((V & 3) == 0) {  // 16-byte loads, four in flight per thread: the scan is latency-bound otherwise
    const float4* row4 = (const float4*)row;
    const int n4 = V >> 2;
    for (int i0 = tid; i0 < n4; i0 += 4096) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * 1024;
        v[u] = i < n4 ? row4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i0 + u * 1024 >= n4) continue;
        const int i = (i0 + u * 1024) * 4;
        upd(v[u].x, i); upd(v[u].y, i + 1); upd(v[u].z, i + 2); upd(v[u].w, i + 3);
      }
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
  if constexpr (SC) {
    __shared__ float redf[16];
    const SlRowScan<1024> scan(row, V, tid);
    sl_row_max_lse<1024>(scan, redf, row_m, row_ls);
  }
  if (tid == 0) {
    for (int w = 1; w < 16; ++w)
      if (smax[w] > best || (smax[w] == best && sidx[w] < bi)) { best = smax[w]; bi = sidx[w]; }
    if (bi == 0x7fffffff) bi = 0;
    select_commit<SC>(rs, eos, b, bi, (best - row_m) - row_ls);
  }
}

// the state arrays every select needs, and the EOS ids as the kernels take them
static bool row_state_ok(const SlRowState& rs) {
  return rs.unfinished && rs.ctx_len && rs.gen_count && rs.finish_len && rs.next_ids && rs.out_ids;
}
static EosList eos_list(const SlRowState& rs) {
  EosList e;
  e.n = rs.n_eos;
  for (int i = 0; i < 8; ++i) e.ids[i] = i < rs.n_eos ? rs.eos_ids[i] : -1;
  return e;
}

int sl_greedy_select_impl(const float* logits, int32_t B, int32_t V, const SlRowState& rs, hipStream_t st) {
  SL_CHECK_ARG(logits && row_state_ok(rs) && B > 0 && V > 0, "sl_greedy_select: bad arguments");
  SL_CHECK_ARG(rs.n_eos >= 0 && rs.n_eos <= 8, "sl_greedy_select: at most 8 eos ids");
  auto* kern = rs.logprob_out ? greedy_select_kernel<true> : greedy_select_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(1024), 0, st, logits, V, eos_list(rs), rs);
  SL_CHECK_LAUNCH("greedy_select");
  return 0;
}

// greedy selection over the [group][B] partial maxima a fused lm_head left (gemm.hip tile_argmax): block = 32 rows x 32 group
// stripes (a wave = two stripes of 32 consecutive rows: two 128-byte segments per load), eight groups' values and columns in
// flight per thread — the scan is latency-bound (2 004 groups of 8 bytes per row at vocab 128 256), not bandwidth-bound; the
// stripes meet in LDS in stripe order and select_commit follows.  Compare rule everywhere: larger
// value, then lower column.
// SC (token log-probabilities): ps holds the third plane, sum_g = sum exp(v - max_g) per group.  With the row maximum Mx (every
// thread folds the 32 stripe maxima of its row, in stripe order) a second pass forms sum_g * exp(max_g - Mx) per stripe in group order, the
// stripes are added in stripe order, and logprob_out[b][gen_count] = -log(total): the chosen token IS the maximum.  0 for a finished row.
// SC = false is the kernel as it was.
template <bool SC>
__global__ __launch_bounds__(1024) void greedy_select_partial_kernel(const float* __restrict__ pv, const int32_t* __restrict__ pi, int n_groups, int B,
                                                                     EosList eos, SlRowState rs, const float* __restrict__ ps) {
  constexpr int ROWS = 32, STRIPES = 32, U = 8;
  __shared__ float sv[STRIPES][ROWS];
  __shared__ int si[STRIPES][ROWS];
  const int lr = threadIdx.x & (ROWS - 1), stripe = threadIdx.x / ROWS;
  const int b = blockIdx.x * ROWS + lr;
  const int bc = b < B ? b : B - 1;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int g0 = stripe; g0 < n_groups; g0 += STRIPES * U) {
    float v[U];
    int ix[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int g = g0 + u * STRIPES;
      const int64_t at = (int64_t)(g < n_groups ? g : n_groups - 1) * B + bc;
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
  float total = 0.f;
  if constexpr (SC) {
    __shared__ float ss[STRIPES][ROWS];
    float mx = sv[0][lr];
    for (int s2 = 1; s2 < STRIPES; ++s2) mx = fmaxf(mx, sv[s2][lr]);
    float acc = 0.f;
    for (int g0 = stripe; g0 < n_groups; g0 += STRIPES * U) {
      float v[U], sg[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + u * STRIPES;
        const int64_t at = (int64_t)(g < n_groups ? g : n_groups - 1) * B + bc;
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
    if (stripe == 0)
      for (int s2 = 0; s2 < STRIPES; ++s2) total += ss[s2][lr];
  }
  if (stripe != 0 || b >= B) return;
  for (int s2 = 1; s2 < STRIPES; ++s2)
    if (sv[s2][lr] > best || (sv[s2][lr] == best && si[s2][lr] < bi)) { best = sv[s2][lr]; bi = si[s2][lr]; }
  if (bi == 0x7fffffff) bi = 0;
  select_commit<SC>(rs, eos, b, bi, SC ? -logf(total) : 0.f);
}

int sl_greedy_select_partial_impl(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t B, const SlRowState& rs,
                                  hipStream_t st) {
  SL_CHECK_ARG(amax_val && amax_idx && row_state_ok(rs) && B > 0 && n_groups > 0, "sl_greedy_select_partial: bad arguments");
  SL_CHECK_ARG(rs.n_eos >= 0 && rs.n_eos <= 8, "sl_greedy_select_partial: at most 8 eos ids");
  SL_CHECK_ARG((amax_sum != nullptr) == (rs.logprob_out != nullptr), "sl_greedy_select_partial_sc: amax_sum and logprob_out come together");
  auto* kern = rs.logprob_out ? greedy_select_partial_kernel<true> : greedy_select_partial_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((B + 31) / 32), dim3(1024), 0, st, amax_val, amax_idx, n_groups, B, eos_list(rs), rs, amax_sum);
  SL_CHECK_LAUNCH("greedy_select_partial");
  return 0;
}

// ----------------------------------------------------------------------------------------------
// sampled selection (hf:generation/utils.py:2911-2923 with do_sample: logits processors then multinomial):
//   TemperatureLogitsWarper (scores / T), TopKLogitsWarper (keep scores >= the k-th largest), TopPLogitsWarper (on the
//   top-k-filtered distribution: drop token i iff the probability mass of the tokens ranked ABOVE it is >= top_p; at least
//   one token survives), then one draw from the renormalised survivors.  One block per row; thresholds by 4-pass radix
//   selection over the order-preserving 32-bit image of the logits (by count for top-k, by probability mass for top-p), so no
//   sort and no O(V) scratch; the draw is the inverse CDF in INDEX order at u = hash(seed, row, step) — reproducible, and the
//   test restates it on the host.  Tokens of equal logit share their fate (all kept or all dropped).  NaN counts as -inf wherever the
//   row is read; a row without a finite logit commits token 0 (tests/select_ref.py).
//
// WARP: HF's four further warpers behind top-p, in HF's order — min_p, typical_p, epsilon_cutoff, eta_cutoff.  With
// a = (x - m) / T the warped score relative to the row maximum, a survivor is a token with
//   ord_key(x) >= keep_key   (top-k / top-p)
//   a >= a_lo                (min_p: ln min_p;  the cutoffs: min(ln(eta Z), largest a in S), so the largest score in S always stays)
//   |a - c| <= d_hi          (typical_p: c = sum_S p a / Z is ln Z - H, so |a - c| IS |-ln p - H|; a band in score that may drop m)
// d_hi comes from the by-mass radix selection run on the inverted bits of |a - c| (a float >= 0 orders as its bits do): dropped iff the
// mass of the strictly smaller distances is >= typical_p Z.  Every stage that needs Z, sum p a or the largest a of its S takes them in
// ONE pass over the row (stage_stats); min_p takes none.  Masses stay relative to m: a survivor of a band that dropped m still holds at
// least V^-2, far above what fp32 and the 2^-40 histogram lose.
// One body, two kernels: everything named in the WARP paragraph sits behind `if constexpr (WARP)`, so sample_rows_kernel (WARP = false,
// what every call without those options launches) neither computes nor stores any of it, and the two share the row read, the radix
// selection, the statistics pass, the draw and the log-probability statement for statement.
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ord_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct WarpArgs { float ln_min_p, typical_p, eps, eta; };    // ln_min_p = -inf, typical_p = 1, eps = eta = 0: off

// bits of |a - c|, never contracted with the product that made a: the selection's histogram and the survivor predicate must see the SAME
// distance for a token, or the token on the boundary could be binned on one side and tested on the other
__device__ __forceinline__ uint32_t dist_bits(float a, float c) {
#pragma clang fp contract(off)
  return __float_as_uint(fabsf(a - c));
}

template <bool WARP>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const float* __restrict__ logits, int V, float inv_temp, int top_k, float top_p, uint64_t seed,
                                                           const int32_t* __restrict__ gen_count, int32_t* __restrict__ choice,
                                                           const int32_t* __restrict__ row_ids, float* __restrict__ logprob_out, int max_new, WarpArgs wa) {
  __shared__ float redf[WARP ? 3 : 1][16];
  __shared__ int hcnt[256];
  __shared__ unsigned long long hmass_fx[256];   // probability mass per bin in 2^-40 fixed point: integer adds commute, so the
                                                 // bin totals (and the threshold compare below) are the same on every run
  __shared__ uint32_t s_prefix;
  __shared__ float s_above;
  __shared__ float part[1024];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* rowp = logits + (int64_t)b * V;
  auto row = [&](int i) { const float x = rowp[i]; return x != x ? -INFINITY : x; };   // NaN counts as -inf: no seat, no mass
  // row maximum (numerical stability of the exponentials)
  float m = -INFINITY;
  for (int i = tid; i < V; i += 1024) m = fmaxf(m, row(i));
  m = wave_max(m);
  if (lane == 0) redf[0][wave] = m;
  __syncthreads();
  m = redf[0][0];
  for (int w = 1; w < 16; ++w) m = fmaxf(m, redf[0][w]);
  __syncthreads();
  if (m == -INFINITY) {   // no finite logit (m is the block's, so every thread leaves here): token 0 as greedy gives, log-probability -inf
    if (tid == 0) {
      choice[b] = 0;
      const int step = gen_count[b];
      if (logprob_out && step < max_new) logprob_out[(int64_t)b * max_new + step] = -INFINITY;
    }
    return;
  }
  auto score = [&](float x) { return (x - m) * inv_temp; };
  auto prob = [&](float x) { return __expf((x - m) * inv_temp); };   // the one mass expression

  // the survivor predicate: what every later stage and the draw see.  Without WARP it is ord_key(x) >= keep_key and nothing else.
  uint32_t keep_key = 0, d_hi = 0xFFFFFFFFu;
  float a_lo = -INFINITY, c = 0.f;
  auto alive = [&](float x) {
    if (ord_key(x) < keep_key) return false;
    if constexpr (WARP) { const float a = score(x); return a >= a_lo && dist_bits(a, c) <= d_hi; }
    return true;
  };
  auto score_key = [&](float x) { return ord_key(x); };
  auto dist_key = [&](float x) { return ~dist_bits(score(x), c); };   // larger key = closer to the expected -ln p

  // radix selection over key_of(x), among the tokens alive now: mode 0 = by count (the k-th largest key), mode 1 = by mass (the first key,
  // from the top, at which the mass of the strictly larger keys is still < limit).  Returns the selected key.
  auto radix_select = [&](int mode, float limit, auto key_of) -> uint32_t {
    uint32_t prefix = 0;
    float above = 0.f;     // count / mass of keys larger than every key matching the current prefix
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
      for (int i = tid; i < 256; i += 1024) { hcnt[i] = 0; hmass_fx[i] = 0ull; }
      __syncthreads();
      for (int i = tid; i < V; i += 1024) {
        const float x = row(i);
        if (!alive(x)) continue;
        const uint32_t k = key_of(x);
        if ((k & hi_mask) != prefix) continue;
        const int bin = (k >> shift) & 255;
        if (mode == 0) atomicAdd(&hcnt[bin], 1);
        else atomicAdd(&hmass_fx[bin], (unsigned long long)(prob(x) * 1099511627776.0f));   // prob <= 1: < 2^57 over a 128 k row
      }
      __syncthreads();
      if (tid == 0) {
        float run = above;
        int sel = -1;
        for (int bin = 255; bin >= 0; --bin) {
          const float w = mode == 0 ? (float)hcnt[bin] : (float)hmass_fx[bin] * (1.0f / 1099511627776.0f);
          if (mode == 0 ? (hcnt[bin] > 0 && run + w >= limit) : (hmass_fx[bin] > 0ull && run + w >= limit)) { sel = bin; break; }
          run += w;
        }
        if (sel < 0) {           // the limit is never reached (rounding / k >= candidates): take the smallest populated bin
          for (int bin = 255; bin >= 0; --bin)
            if (mode == 0 ? hcnt[bin] > 0 : hmass_fx[bin] > 0ull) sel = bin;
          run = above;
          for (int bin = 255; bin > sel; --bin) run += mode == 0 ? (float)hcnt[bin] : (float)hmass_fx[bin] * (1.0f / 1099511627776.0f);
          if (sel < 0) sel = 0;
        }
        s_prefix = prefix | ((uint32_t)sel << shift);
        s_above = run;
      }
      __syncthreads();
      prefix = s_prefix;
      above = s_above;
      __syncthreads();
    }
    return prefix;
  };

  // one pass over the survivors: z = sum p, each thread over its elements strided by 1024, then the wave butterfly, then the 16 waves in
  // order.  WARP adds s1 = sum p a (a token of mass zero adds nothing to either) and amax = the largest a in the same pass.
  float z, s1, amax;
  auto stage_stats = [&]() {
    float lz = 0.f, ls = 0.f, la = -INFINITY;
    for (int i = tid; i < V; i += 1024) {
      const float x = row(i);
      if (!alive(x)) continue;
      const float a = score(x), p = __expf(a);
      if constexpr (WARP) { la = fmaxf(la, a); if (p > 0.f) { lz += p; ls += p * a; } }
      else lz += p;
    }
    lz = wave_sum(lz);
    if constexpr (WARP) { ls = wave_sum(ls); la = wave_max(la); }
    __syncthreads();
    if (lane == 0) { redf[0][wave] = lz; if constexpr (WARP) { redf[1][wave] = ls; redf[2][wave] = la; } }
    __syncthreads();
    z = 0.f; s1 = 0.f; amax = -INFINITY;
    for (int w = 0; w < 16; ++w) { z += redf[0][w]; if constexpr (WARP) { s1 += redf[1][w]; amax = fmaxf(amax, redf[2][w]); } }
  };

  if (top_k > 0 && top_k < V) keep_key = radix_select(0, (float)top_k, score_key);
  if (top_p < 1.0f) {
    stage_stats();
    const uint32_t kp = radix_select(1, top_p * z, score_key);
    keep_key = kp > keep_key ? kp : keep_key;
  }
  if constexpr (WARP) {
    a_lo = wa.ln_min_p;                                  // the largest score of S is m here (a = 0 >= ln min_p): it and its ties stay
    if (wa.typical_p < 1.0f) {
      stage_stats();
      c = s1 / z;
      d_hi = ~radix_select(1, wa.typical_p * z, dist_key);
    }
    if (wa.eps > 0.f) {
      stage_stats();
      a_lo = fmaxf(a_lo, fminf(logf(wa.eps * z), amax));
    }
    if (wa.eta > 0.f) {
      stage_stats();
      const float lnz = logf(z), h = lnz - s1 / z, le = logf(wa.eta);
      a_lo = fmaxf(a_lo, fminf(fminf(le, 0.5f * le - h) + lnz, amax));
    }
  }
  // the draw, inverse CDF in index order: thread t owns the contiguous slice [t * C, (t + 1) * C)
  const int Cn = (V + 1023) / 1024;
  const int i0 = tid * Cn, i1 = (i0 + Cn) < V ? (i0 + Cn) : V;
  float loc = 0.f;
  for (int i = i0; i < i1; ++i) { const float x = row(i); if (alive(x)) loc += prob(x); }
  part[tid] = loc;
  __syncthreads();
  if (tid == 0) {
    float zt = 0.f;
    for (int t = 0; t < 1024; ++t) zt += part[t];
    const uint32_t step = (uint32_t)gen_count[b];
    const uint32_t rid = row_ids ? (uint32_t)row_ids[b] : (uint32_t)b;    // the sequence's index in the caller's batch (rows move when a batch is compacted)
    const uint32_t h = lowbias32(step ^ lowbias32(rid ^ (uint32_t)seed) ^ (uint32_t)(seed >> 32));
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
    const float target = u * zt;
    float run = 0.f;
    int t = 0;
    for (; t < 1023; ++t) { if (run + part[t] > target) break; run += part[t]; }
    // walk the slice; the LAST survivor of mass above zero seen is the fallback when rounding leaves target >= the total (a -inf token
    // passes keep_key = 0 and must never be returned)
    int pick = -1, last = -1;
    const int j0 = t * Cn, j1 = (j0 + Cn) < V ? (j0 + Cn) : V;
    for (int i = j0; i < j1; ++i) {
      const float x = row(i);
      if (!alive(x)) continue;
      const float p = prob(x);
      if (p > 0.f) last = i;
      run += p;
      if (run > target) { pick = i; break; }
    }
    if (pick < 0) pick = last;
    if (pick < 0) {   // empty slice (cannot happen with zt > 0): the first survivor of mass above zero
      for (int i = 0; i < V; ++i) { const float x = row(i); if (alive(x) && prob(x) > 0.f) { pick = i; break; } }
    }
    choice[b] = pick < 0 ? 0 : pick;
    // token log-probabilities: the drawn token under the renormalised survivors, log(p / z) with the p and the z of the draw
    if (logprob_out && (int)step < max_new) logprob_out[(int64_t)b * max_new + step] = logf(prob(row(pick < 0 ? 0 : pick)) / zt);
  }
}

// NULL or every option at its off value: no warped form
bool sl_warp_opts_on(const sl_warp_opts* w) {
  return w && (w->min_p != 0.f || w->typical_p != 1.0f || w->epsilon_cutoff != 0.f || w->eta_cutoff != 0.f);
}
// the `!(..)` forms refuse NaN
int sl_warp_opts_check(const char* who, const sl_warp_opts* w) {
  if (!w) return 0;
  SL_CHECK_ARG(w->min_p >= 0.f && w->min_p <= 1.0f, "%s: min_p %f outside [0, 1]", who, (double)w->min_p);
  SL_CHECK_ARG(w->typical_p > 0.f && w->typical_p <= 1.0f, "%s: typical_p %f outside (0, 1]", who, (double)w->typical_p);
  SL_CHECK_ARG(w->epsilon_cutoff >= 0.f && w->epsilon_cutoff < 1.0f, "%s: epsilon_cutoff %f outside [0, 1)", who, (double)w->epsilon_cutoff);
  SL_CHECK_ARG(w->eta_cutoff >= 0.f && w->eta_cutoff < 1.0f, "%s: eta_cutoff %f outside [0, 1)", who, (double)w->eta_cutoff);
  return 0;
}

int sl_sample_select_impl(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t* choice_ws,
                          const int32_t* row_ids, const SlRowState& rs, hipStream_t st, const sl_warp_opts* warp) {
  SL_CHECK_ARG(logits && row_state_ok(rs) && choice_ws && B > 0 && V > 0, "sl_sample_select: bad arguments");
  SL_CHECK_ARG(temperature > 0.f && top_p > 0.f && top_p <= 1.0f && top_k >= 0, "sl_sample_select: need temperature > 0, 0 < top_p <= 1, top_k >= 0 (got %f, %f, %d)",
               (double)temperature, (double)top_p, top_k);
  SL_CHECK_ARG(rs.n_eos >= 0 && rs.n_eos <= 8, "sl_sample_select: at most 8 eos ids");
  SL_TRY(sl_warp_opts_check("sl_sample_select_w", warp));
  const bool on = sl_warp_opts_on(warp);       // off: the unwarped instantiation, which never reads wa
  const WarpArgs wa = on ? WarpArgs{warp->min_p > 0.f ? logf(warp->min_p) : -INFINITY, warp->typical_p, warp->epsilon_cutoff, warp->eta_cutoff} : WarpArgs{};
  hipLaunchKernelGGL(on ? sample_rows_kernel<true> : sample_rows_kernel<false>, dim3(B), dim3(1024), 0, st, logits, V, 1.0f / temperature, top_k, top_p, seed,
                     rs.gen_count, choice_ws, row_ids, rs.logprob_out, rs.max_new, wa);
  SL_CHECK_LAUNCH("sample_rows");
  auto* commit = rs.logprob_out ? select_commit_kernel<true> : select_commit_kernel<false>;
  hipLaunchKernelGGL(commit, dim3(B), dim3(64), 0, st, eos_list(rs), rs, (const int32_t*)choice_ws);
  SL_CHECK_LAUNCH("sample_commit");
  return 0;
}

// ---- the C entries: each fills the row state from its flat argument list
static SlRowState entry_state(int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids,
                              int32_t max_new, float* logprob_out, const int32_t* eos_ids, int32_t n_eos, int32_t pad_id, int32_t use_eos,
                              int32_t advance_ctx = 1) {
  SlRowState rs{};                              // no per-row budgets through these entries: row_limit stays NULL
  rs.unfinished = unfinished; rs.ctx_len = ctx_len; rs.gen_count = gen_count; rs.finish_len = finish_len; rs.next_ids = next_ids;
  rs.out_ids = out_ids; rs.max_new = max_new; rs.logprob_out = logprob_out;
  rs.eos_ids = eos_ids; rs.n_eos = n_eos; rs.pad_id = pad_id; rs.use_eos = use_eos; rs.advance_ctx = advance_ctx;
  return rs;
}

extern "C" int sl_greedy_select(const float* logits, int32_t B, int32_t V, const int32_t* eos_ids, int32_t n_eos, int32_t pad_id,
                                int32_t use_eos, int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count, int32_t* finish_len,
                                int32_t* next_ids, int32_t* out_ids, int32_t max_new, sl_stream stream) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, nullptr, eos_ids, n_eos, pad_id, use_eos);
  return sl_greedy_select_impl(logits, B, V, rs, (hipStream_t)stream);
}

extern "C" int sl_greedy_select_sc(const float* logits, int32_t B, int32_t V, const int32_t* eos_ids, int32_t n_eos, int32_t pad_id,
                                   int32_t use_eos, int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count, int32_t* finish_len,
                                   int32_t* next_ids, int32_t* out_ids, int32_t max_new, float* logprob_out, sl_stream stream) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, logprob_out, eos_ids, n_eos, pad_id, use_eos);
  return sl_greedy_select_impl(logits, B, V, rs, (hipStream_t)stream);
}

extern "C" int sl_greedy_select_partial(const float* amax_val, const int32_t* amax_idx, int32_t n_groups, int32_t B, const int32_t* eos_ids, int32_t n_eos,
                                        int32_t pad_id, int32_t use_eos, int32_t advance_ctx, int32_t* unfinished, int32_t* ctx_len, int32_t* gen_count,
                                        int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, sl_stream stream) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, nullptr, eos_ids, n_eos, pad_id, use_eos, advance_ctx);
  return sl_greedy_select_partial_impl(amax_val, amax_idx, nullptr, n_groups, B, rs, (hipStream_t)stream);
}

extern "C" int sl_greedy_select_partial_sc(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t B,
                                           const int32_t* eos_ids, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t advance_ctx, int32_t* unfinished,
                                           int32_t* ctx_len, int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new,
                                           float* logprob_out, sl_stream stream) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, logprob_out, eos_ids, n_eos, pad_id, use_eos, advance_ctx);
  return sl_greedy_select_partial_impl(amax_val, amax_idx, amax_sum, n_groups, B, rs, (hipStream_t)stream);
}

extern "C" int sl_sample_select(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                const int32_t* eos_ids, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len,
                                int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, int32_t* choice_ws,
                                sl_stream stream) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, nullptr, eos_ids, n_eos, pad_id, use_eos);
  return sl_sample_select_impl(logits, B, V, temperature, top_k, top_p, seed, choice_ws, nullptr, rs, (hipStream_t)stream);
}

extern "C" int sl_sample_select_sc(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                   const int32_t* eos_ids, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len,
                                   int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, int32_t* choice_ws,
                                   float* logprob_out, sl_stream stream) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, logprob_out, eos_ids, n_eos, pad_id, use_eos);
  return sl_sample_select_impl(logits, B, V, temperature, top_k, top_p, seed, choice_ws, nullptr, rs, (hipStream_t)stream);
}

extern "C" int sl_sample_select_w(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                  const int32_t* eos_ids, int32_t n_eos, int32_t pad_id, int32_t use_eos, int32_t* unfinished, int32_t* ctx_len,
                                  int32_t* gen_count, int32_t* finish_len, int32_t* next_ids, int32_t* out_ids, int32_t max_new, int32_t* choice_ws,
                                  float* logprob_out, sl_stream stream, const sl_warp_opts* warp) {
  const SlRowState rs = entry_state(unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, max_new, logprob_out, eos_ids, n_eos, pad_id, use_eos);
  return sl_sample_select_impl(logits, B, V, temperature, top_k, top_p, seed, choice_ws, nullptr, rs, (hipStream_t)stream, warp);
}
