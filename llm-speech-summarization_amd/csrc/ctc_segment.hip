// ctc_segment.hip — CTC word segmentation of a packed ragged batch on the device (additive to ABI 7):
//   sl_ctc_greedy_batch      frames (n_rows, H) x CTC head (V, H) -> greedy ids, the argmax taken in the accumulator registers
//   sl_ctc_pool_ranges_batch greedy ids -> HF word offsets -> the reference's pool ranges (ref:preprocess_data/utils.py:155-188)
#include "common.h"

// ----------------------------------------------------------------------------------------------
// CTC head + argmax.  The product is one streaming read of x against a (V <= 64, H) weight that stays in LDS, so the kernel is
// frame-major: a block of 8 waves walks slabs of 128 rows, wave w owning rows 16 w .. 16 w + 15 of the slab; its A operand comes
// straight from global memory (every element of x is read once, by one lane), its B operands from the LDS image of w, NT = ceil(V / 16)
// accumulator tiles per wave.  The weight image is (16 NT) rows of KC elements plus one 16-byte pad slot (odd row stride in slots);
// rows >= V and columns >= H are zeros.  KC = H rounded up to the MFMA step when that fits SL_CTC_LDS_BYTES (32 x 1024 in 16 bits
// does: staged once per block), otherwise the largest multiple of the step that does, and the image is re-staged per slab and chunk.
// A row's logits are the fixed chain of MFMA steps k = 0, KSTEP, ... whatever slab, wave or batch the row sits in, the bias is added
// in fp32 afterwards, and the argmax orders (value, column) pairs totally (greater value, then lower column), so ids[m] is a
// function of row m alone.  Accumulator layout (common.h): lane (c = l & 15, q = l >> 4) holds D[row 4 q + i][col c].
// ----------------------------------------------------------------------------------------------
#define SL_CTC_LDS_BYTES (96 * 1024)
#define SL_CTC_THREADS 512
#define SL_CTC_SLAB 128

template <typename T, int NT>
__global__ __launch_bounds__(SL_CTC_THREADS) void ctc_greedy_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ bias,
                                                                    int32_t* __restrict__ ids, int64_t n_rows, int H, int V, int KC) {
  constexpr int VEC = Vec16<T>::VEC, KSTEP = MMA<T>::KSTEP;
  extern __shared__ __attribute__((aligned(16))) uint4 wimg[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int cpr = KC / VEC, RS = cpr + 1;      // 16-byte slots per image row, row stride
  const int n_chunks = (H + KC - 1) / KC;
  const int64_t n_slabs = (n_rows + SL_CTC_SLAB - 1) / SL_CTC_SLAB;

  float bv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bv[t] = (bias && 16 * t + r < V) ? to_f32(bias[16 * t + r]) : 0.f;

  bool staged = false;
  for (int64_t slab = blockIdx.x; slab < n_slabs; slab += gridDim.x) {
    const int64_t row0 = slab * SL_CTC_SLAB + wave * 16;
    int64_t row_a = row0 + r;                  // rows past the end read the last row; their results are not stored
    if (row_a >= n_rows) row_a = n_rows - 1;
    const T* xa = x + row_a * (int64_t)H;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < n_chunks; ++c) {
      const int k0 = c * KC;
      if (n_chunks > 1 || !staged) {
        if (staged) __syncthreads();           // every wave is done with the previous image
        for (int i = tid; i < NT * 16 * cpr; i += SL_CTC_THREADS) {
          const int row = i / cpr, ch = i - row * cpr, k = k0 + ch * VEC;
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (row < V && k < H) v = *(const uint4*)(w + (int64_t)row * H + k);
          wimg[row * RS + ch] = v;
        }
        __syncthreads();
        staged = true;
      }
      if (row0 < n_rows) {
        const int klen = (H - k0 < KC) ? H - k0 : KC;
        for (int kk = 0; kk < klen; kk += 4 * KSTEP) {      // four 16-byte loads of x in flight per lane, then their MFMA steps in k order
          uint4 a[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int k = k0 + kk + s * KSTEP + q * VEC;
            a[s] = make_uint4(0u, 0u, 0u, 0u);
            if (kk + s * KSTEP < klen && k < H) a[s] = ld_nt16(xa + k);
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int ks = kk + s * KSTEP;
            if (ks < klen) {
#pragma unroll
              for (int t = 0; t < NT; ++t) MMA<T>::step(acc[t], a[s], wimg[(16 * t + r) * RS + ks / VEC + q]);
            }
          }
        }
      }
    }
    if (row0 >= n_rows) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float best = -INFINITY;                  // this lane's columns r, 16 + r, ... in ascending order; 0x7fffffff: none below V yet
      int bi = 0x7fffffff;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = 16 * t + r;
        const float v = acc[t][i] + bv[t];
        if (col < V && (bi == 0x7fffffff || v > best)) { best = v; bi = col; }
      }
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {       // the 16 lanes of one q group hold the 16 column residues of rows 4 q + i
        const float ov = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
      }
      const int64_t row = row0 + 4 * q + i;
      if (r == 0 && row < n_rows) ids[row] = bi;
    }
  }
}

template <typename T, int NT>
static int launch_ctc_greedy(const void* x, const void* w, const void* bias, int32_t* ids, int64_t n_rows, int H, int V, hipStream_t st) {
  constexpr int VEC = Vec16<T>::VEC, KSTEP = MMA<T>::KSTEP;
  const int Hp = (H + KSTEP - 1) / KSTEP * KSTEP;
  int KC = ((SL_CTC_LDS_BYTES / (16 * NT)) - 16) / (int)sizeof(T) / KSTEP * KSTEP;      // elements per image row that fit the budget
  if (KC > Hp) KC = Hp;
  const size_t lds = (size_t)16 * NT * (KC / VEC + 1) * 16;
  auto kern = ctc_greedy_kernel<T, NT>;
  if (lds > 64 * 1024) SL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t n_slabs = ceil_div64(n_rows, SL_CTC_SLAB);
  const unsigned grid = (unsigned)(n_slabs < 256 ? n_slabs : 256);      // one block per CU: the image takes most of its LDS
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SL_CTC_THREADS), lds, st, (const T*)x, (const T*)w, (const T*)bias, ids, n_rows, H, V, KC);
  SL_CHECK_LAUNCH("ctc_greedy_batch");
  return 0;
}

extern "C" int sl_ctc_greedy_batch(const void* x, const void* w, const void* bias, int32_t* ids, int64_t n_rows, int32_t H, int32_t V, int32_t dtype,
                                   sl_stream stream) {
  SL_CHECK_ARG(x && w && ids, "sl_ctc_greedy_batch: null x, w or ids");
  SL_CHECK_ARG(n_rows >= 0 && n_rows <= 0x7fffffffLL, "sl_ctc_greedy_batch: n_rows=%lld out of range", (long long)n_rows);
  SL_CHECK_ARG(V >= 1 && V <= 64, "sl_ctc_greedy_batch: V=%d must be in 1..64 (a CTC letter vocabulary)", V);
  SL_CHECK_ARG(H >= 8 && H % 8 == 0, "sl_ctc_greedy_batch: H=%d must be a positive multiple of 8", H);
  SL_CHECK_ARG(dtype == SL_F32 || dtype == SL_BF16 || dtype == SL_F16, "sl_ctc_greedy_batch: unknown dtype %d", dtype);
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int nt = (V + 15) / 16;
  SL_DISPATCH_DTYPE_INF(dtype, T, {
    switch (nt) {
      case 1: return launch_ctc_greedy<T, 1>(x, w, bias, ids, n_rows, H, V, st);
      case 2: return launch_ctc_greedy<T, 2>(x, w, bias, ids, n_rows, H, V, st);
      case 3: return launch_ctc_greedy<T, 3>(x, w, bias, ids, n_rows, H, V, st);
      default: return launch_ctc_greedy<T, 4>(x, w, bias, ids, n_rows, H, V, st);
    }
  });
  return 0;
}

// ----------------------------------------------------------------------------------------------
// ids -> words -> pool ranges.  One block of 256 threads per utterance walks its T_u + 1 positions (the position T_u acts as a
// closing delimiter) in tiles of 256, forward only, carrying four positions between tiles:
//   last delimiter, last letter (any id other than blank / delimiter), start of the open word, end of the last closed word.
// Inside a tile the four waves ballot their letter / delimiter flags into LDS; "the last set position below p" and "how many set
// below p" are then a count-leading-zeros / popcount over at most four 64-bit masks.  A word closes at a delimiter position p that
// has a letter since the previous delimiter: (s, e) = (start of the open word, last letter + 1).  The closing position emits, in list
// order, the gap before its word (e of the previous word or 0, s) and the word's chunks (s + k pr, s + k pr + pr); an exclusive scan
// of the item counts over the tile's closed words gives every item its place, and the items are then written one per thread (a
// binary search over the scanned offsets finds the word), so a 1 500-frame word is 375 parallel stores, not a serial walk.  The
// final gap (e_last, e_last + 2 pr), or the one range (0, T_u) of an utterance without a word, is written after the last tile.
// The kernel runs twice: a counting pass (counts / word_counts), then the emitting pass, in which block u first adds up counts[0 .. u)
// to find its place in the table, so that the utterances' ranges are contiguous and in utterance order without a workspace.
// Capacity: an utterance of T frames yields at most T + 2 ranges (each word costs ceil(len / pr) + 1 <= len + 1 items, the words and
// the delimiters between them fit in T, plus the first gap) and at most (T + 1) / 2 words; every store is checked against the
// caller's capacity all the same.
// ----------------------------------------------------------------------------------------------
#define SL_SEG_THREADS 256
#define SL_SEG_WAVES 4

// last set position < p (0 <= p <= 256) in four 64-bit masks, or -1
__device__ __forceinline__ int seg_last_below(const unsigned long long* m, int p) {
  int wv = p >> 6;
  if (wv < SL_SEG_WAVES) {
    const int b = p & 63;
    const unsigned long long mm = b ? (m[wv] & (~0ull >> (64 - b))) : 0ull;
    if (mm) return wv * 64 + 63 - __clzll((long long)mm);
  }
  for (--wv; wv >= 0; --wv)
    if (wv < SL_SEG_WAVES && m[wv]) return wv * 64 + 63 - __clzll((long long)m[wv]);
  return -1;
}

// number of set positions < p (0 <= p <= 256)
__device__ __forceinline__ int seg_count_below(const unsigned long long* m, int p) {
  int n = 0;
  const int wv = p >> 6, b = p & 63;
  for (int i = 0; i < SL_SEG_WAVES; ++i) {
    if (i < wv) n += __popcll(m[i]);
    else if (i == wv && b) n += __popcll(m[i] & (~0ull >> (64 - b)));
  }
  return n;
}

__global__ __launch_bounds__(SL_SEG_THREADS) void ctc_pool_ranges_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ row_offsets,
                                                                         int64_t n_rows, int blank_id, int delim_id, int pr, int raw, int emit,
                                                                         int64_t* __restrict__ ranges, int64_t ranges_cap, int32_t* __restrict__ counts,
                                                                         int64_t* __restrict__ words, int64_t words_cap,
                                                                         int32_t* __restrict__ word_counts) {
  __shared__ unsigned long long mL[SL_SEG_WAVES], mD[SL_SEG_WAVES], mS[SL_SEG_WAVES], mE[SL_SEG_WAVES];
  __shared__ int evS[SL_SEG_THREADS], evE[SL_SEG_THREADS], evP[SL_SEG_THREADS], evOff[SL_SEG_THREADS + 1];
  __shared__ long long red[SL_SEG_WAVES * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = blockIdx.x;
  int64_t tok0 = row_offsets[u], tok1 = row_offsets[u + 1];
  if (tok0 < 0) tok0 = 0;                      // a bad offset table must still stay inside ids
  if (tok1 > n_rows) tok1 = n_rows;
  const int T = tok1 > tok0 ? (int)(tok1 - tok0) : 0;
  const int64_t add = raw ? 0 : tok0;

  // place of this utterance in the tables: the sums of the counts of the utterances before it (emitting pass only)
  int64_t rbase = 0, wbase = 0;
  if (emit) {
    long long a = 0, b = 0;
    for (int v = tid; v < u; v += SL_SEG_THREADS) {
      a += counts[v];
      b += word_counts ? word_counts[v] : 0;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      a += __shfl_xor(a, m, 64);
      b += __shfl_xor(b, m, 64);
    }
    if (lane == 0) { red[2 * wave] = a; red[2 * wave + 1] = b; }
    __syncthreads();
    for (int i = 0; i < SL_SEG_WAVES; ++i) { rbase += red[2 * i]; wbase += red[2 * i + 1]; }
  }

  int cD = -1, cL = -2, cS = -1, cE = 0;       // carried positions: last delimiter, last letter, start of the open word, end of the last closed word
  int n_items = 0, n_words = 0;                // items / words of the tiles so far
  const int n_tiles = (T + 1 + SL_SEG_THREADS - 1) / SL_SEG_THREADS;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int g0 = tile * SL_SEG_THREADS, g = g0 + tid;
    bool isL = false, isD = false;
    if (g < T) {
      const int id = ids[tok0 + g];
      isD = id == delim_id;
      isL = !isD && id != blank_id;
    } else if (g == T) {
      isD = true;
    }
    const unsigned long long bl = __ballot(isL), bd = __ballot(isD);
    __syncthreads();                           // the previous tile's readers of the masks and event arrays are done
    if (lane == 0) { mL[wave] = bl; mD[wave] = bd; }
    __syncthreads();
    int p;
    p = seg_last_below(mD, tid);
    const int prevD = p >= 0 ? g0 + p : cD;
    p = seg_last_below(mL, tid);
    const int prevL = p >= 0 ? g0 + p : cL;
    const bool isS = isL && prevL < prevD;     // the first letter since the last delimiter opens a word
    const bool isE = isD && prevL > prevD;     // a delimiter with a letter since the previous one closes it
    const unsigned long long bs = __ballot(isS), be = __ballot(isE);
    if (lane == 0) { mS[wave] = bs; mE[wave] = be; }
    __syncthreads();
    const int n_ev = seg_count_below(mE, SL_SEG_THREADS);
    int items = 0, j = 0;
    if (isE) {
      p = seg_last_below(mS, tid);
      const int s = p >= 0 ? g0 + p : cS, e = prevL + 1;
      int pe = cE;                             // end of the previous word: the last letter before the previous closing position
      p = seg_last_below(mE, tid);
      if (p >= 0) {
        const int pl = seg_last_below(mL, p);
        pe = (pl >= 0 ? g0 + pl : cL) + 1;
      }
      j = seg_count_below(mE, tid);
      evS[j] = s; evE[j] = e; evP[j] = pe;
      items = ((raw || s > pe) ? 1 : 0) + (e - s + pr - 1) / pr;
      if (emit && words) {
        const int64_t o = wbase + n_words + j;
        if (o < words_cap) { words[2 * o] = s; words[2 * o + 1] = e; }
      }
    }
    // exclusive scan of the item counts over the tile's closing positions, in position order
    int incl = items;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    int wpre = 0, total = 0;
    for (int i = 0; i < SL_SEG_WAVES; ++i) {
      if (i < wave) wpre += (int)red[i];
      total += (int)red[i];
    }
    if (isE) evOff[j] = wpre + incl - items;
    if (tid == 0) evOff[n_ev] = total;
    __syncthreads();
    if (emit) {
      for (int it = tid; it < total; it += SL_SEG_THREADS) {
        int lo = 0, hi = n_ev - 1;             // the last closed word whose first item is at or before `it`
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (evOff[mid] <= it) lo = mid; else hi = mid - 1;
        }
        const int s = evS[lo], pe = evP[lo];
        const int has_gap = (raw || s > pe) ? 1 : 0;
        int k = it - evOff[lo];
        int64_t a, b;
        if (has_gap && k == 0) {
          a = pe; b = s;
        } else {
          k -= has_gap;
          a = s + (int64_t)k * pr; b = a + pr;
          if (!raw && b > T) b = T;            // a chunk never reaches into the next utterance's rows
        }
        const int64_t o = rbase + n_items + it;
        if (o < ranges_cap) { ranges[2 * o] = a + add; ranges[2 * o + 1] = b + add; }
      }
    }
    // carries, the same in every thread
    p = seg_last_below(mD, SL_SEG_THREADS);
    if (p >= 0) cD = g0 + p;
    const int pe_ = seg_last_below(mE, SL_SEG_THREADS);
    if (pe_ >= 0) {
      const int pl = seg_last_below(mL, pe_);
      cE = (pl >= 0 ? g0 + pl : cL) + 1;
    }
    p = seg_last_below(mS, SL_SEG_THREADS);
    if (p >= 0) cS = g0 + p;
    p = seg_last_below(mL, SL_SEG_THREADS);
    if (p >= 0) cL = g0 + p;
    n_items += total;
    n_words += n_ev;
  }
  if (tid != 0) return;
  int64_t a = 0, b = 0;
  bool last = true;
  if (n_words == 0) {                          // no word: the one range (0, T_u) (the reference raises IndexError here)
    a = 0; b = T;
    last = raw || T > 0;
  } else {                                     // final gap (e_last, e_last + 2 pr)
    a = cE; b = (int64_t)cE + 2 * pr;
    if (!raw) {
      if (b > T) b = T;
      last = b > a;
    }
  }
  if (last) {
    const int64_t o = rbase + n_items;
    if (emit && o < ranges_cap) { ranges[2 * o] = a + add; ranges[2 * o + 1] = b + add; }
    ++n_items;
  }
  if (!emit) {
    counts[u] = n_items;
    if (word_counts) word_counts[u] = n_words;
  }
}

extern "C" int sl_ctc_pool_ranges_batch(const int32_t* ids, const int64_t* row_offsets_dev, int32_t n_utt, int64_t n_rows, int32_t blank_id,
                                        int32_t delim_id, int32_t pool_range, int32_t mode, int64_t* ranges_out, int64_t ranges_cap,
                                        int32_t* counts_out, int64_t* words_out, int64_t words_cap, int32_t* word_counts_out, sl_stream stream) {
  SL_CHECK_ARG(ids && row_offsets_dev && ranges_out && counts_out, "sl_ctc_pool_ranges_batch: null ids, row offsets, range table or counts");
  SL_CHECK_ARG(n_utt > 0 && n_rows >= 0 && n_rows <= (1LL << 30), "sl_ctc_pool_ranges_batch: n_utt=%d, n_rows=%lld (at most 2^30)", n_utt,
               (long long)n_rows);
  SL_CHECK_ARG(blank_id != delim_id, "sl_ctc_pool_ranges_batch: blank_id and delim_id are both %d", blank_id);
  SL_CHECK_ARG(pool_range >= 1 && pool_range <= (1 << 20), "sl_ctc_pool_ranges_batch: pool_range=%d must be at least 1", pool_range);
  SL_CHECK_ARG(mode == SL_CTC_RANGES_PACKED || mode == SL_CTC_RANGES_RAW, "sl_ctc_pool_ranges_batch: unknown mode %d", mode);
  SL_CHECK_ARG(ranges_cap >= (int64_t)sl_ctc_pool_ranges_capacity(n_rows, n_utt),
               "sl_ctc_pool_ranges_batch: the range table holds %lld records, %lld rows in %d utterances can give %lld (n_rows + 2 n_utt)",
               (long long)ranges_cap, (long long)n_rows, n_utt, (long long)sl_ctc_pool_ranges_capacity(n_rows, n_utt));
  SL_CHECK_ARG(!words_out == !word_counts_out, "sl_ctc_pool_ranges_batch: the word table and the word counts come together");
  SL_CHECK_ARG(!words_out || words_cap >= (int64_t)sl_ctc_words_capacity(n_rows, n_utt),
               "sl_ctc_pool_ranges_batch: the word table holds %lld records, %lld rows in %d utterances can give %lld ((n_rows + n_utt) / 2)",
               (long long)words_cap, (long long)n_rows, n_utt, (long long)sl_ctc_words_capacity(n_rows, n_utt));
  hipStream_t st = (hipStream_t)stream;
  const int raw = mode == SL_CTC_RANGES_RAW;
  for (int emit = 0; emit < 2; ++emit) {
    hipLaunchKernelGGL(ctc_pool_ranges_kernel, dim3((unsigned)n_utt), dim3(SL_SEG_THREADS), 0, st, ids, row_offsets_dev, n_rows, (int)blank_id,
                       (int)delim_id, (int)pool_range, raw, emit, ranges_out, ranges_cap, counts_out, words_out, words_cap, word_counts_out);
    SL_CHECK_LAUNCH("ctc_pool_ranges_batch");
  }
  return 0;
}

extern "C" size_t sl_ctc_pool_ranges_capacity(int64_t n_rows, int32_t n_utt) { return n_rows < 0 || n_utt < 0 ? 0 : (size_t)(n_rows + 2 * (int64_t)n_utt); }
extern "C" size_t sl_ctc_words_capacity(int64_t n_rows, int32_t n_utt) { return n_rows < 0 || n_utt < 0 ? 0 : (size_t)((n_rows + (int64_t)n_utt) / 2); }
