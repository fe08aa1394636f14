// llama_ops.hip — the small Llama-side kernels: embedding gather, RoPE + KV-cache append, one-token GQA
// attention against the cache, the weight packers (token selection: select.hip).  All HBM/latency-bound; 16-byte accesses, fp32 math.
#include <stdlib.h>

#include <map>
#include <type_traits>
#include <utility>

#include "common.h"
#include "wformat.h"

// ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_gather_kernel(const T* __restrict__ table, const int32_t* __restrict__ ids,
                                                           T* __restrict__ out, int64_t n, int cols) {
  constexpr int VEC = Vec16<T>::VEC;
  const int cpr = cols / VEC;
  const int64_t total = n * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / cpr;
    const int ch = (int)(i % cpr);
    *(uint4*)(out + row * cols + ch * VEC) = *(const uint4*)(table + (int64_t)ids[row] * cols + ch * VEC);
  }
}

extern "C" int sl_embed_gather(const void* table, const int32_t* ids, void* out, int64_t n, int32_t cols, int32_t dtype,
                               sl_stream stream) {
  SL_CHECK_ARG(table && ids && out && n >= 0 && cols > 0, "sl_embed_gather: bad arguments");
  const int vec = dtype == SL_F32 ? 4 : 8;
  SL_CHECK_ARG(cols % vec == 0, "sl_embed_gather: cols=%d must be a multiple of %d", cols, vec);
  if (n == 0) return 0;
  const int64_t total = n * (cols / vec);
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 4096 ? ceil_div64(total, 256) : 4096);
  SL_DISPATCH_DTYPE_INF(dtype, T, {
    hipLaunchKernelGGL((embed_gather_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)table, ids, (T*)out, n, cols);
  });
  SL_CHECK_LAUNCH("embed_gather");
  return 0;
}

// ----------------------------------------------------------------------------------------------
// RoPE + KV append.  One thread owns chunk j of the first half of a head and the matching chunk of the
// second half (rotate_half pairs d with d + D/2).
// ----------------------------------------------------------------------------------------------
// KV8 (SL_KV_FP8_E4M3): the caches hold one e4m3 byte per element, quantised from the value rounded to T (sl_q8_e4m3), and the
// rotated K rows also go back into qkv in place, where the fp8-mode prefill attention reads them unquantised.
template <typename T, bool KV8 = false>
__global__ __launch_bounds__(256) void rope_kv_append_kernel(T* __restrict__ qkv, std::conditional_t<KV8, uint8_t, T>* __restrict__ kc,
                                                             std::conditional_t<KV8, uint8_t, T>* __restrict__ vc,
                                                             const int32_t* __restrict__ tok_seq, const int32_t* __restrict__ tok_pos,
                                                             const float* __restrict__ cosT, const float* __restrict__ sinT, int64_t n_tok,
                                                             int nh, int nkv, int D, int max_ctx) {
  constexpr int VEC = Vec16<T>::VEC;
  const int half = D / 2, cph = half / VEC;  // chunks per half head
  const int heads = nh + 2 * nkv;
  const int64_t total = n_tok * heads * cph;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % cph);
    const int h = (int)((i / cph) % heads);
    const int64_t t = i / ((int64_t)cph * heads);
    T* src = qkv + t * (int64_t)heads * D + (int64_t)h * D + j * VEC;
    const int pos = tok_pos[t];
    uint4 u1 = *(const uint4*)src, u2 = *(const uint4*)(src + half);
    if (h < nh + nkv) {
      float a[VEC], b[VEC], c[VEC], s[VEC], o1[VEC], o2[VEC];
      Vec16<T>::unpack(u1, a);
      Vec16<T>::unpack(u2, b);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        c[e] = cosT[(int64_t)pos * half + j * VEC + e];
        s[e] = sinT[(int64_t)pos * half + j * VEC + e];
        o1[e] = a[e] * c[e] - b[e] * s[e];  // x*cos + rotate_half(x)*sin, first half: -x2*sin
        o2[e] = b[e] * c[e] + a[e] * s[e];  // second half: +x1*sin
      }
      u1 = Vec16<T>::pack(o1);
      u2 = Vec16<T>::pack(o2);
    }
    if (h < nh) {
      *(uint4*)src = u1;
      *(uint4*)(src + half) = u2;
    } else {
      const bool isk = h < nh + nkv;
      const int kvh = isk ? h - nh : h - nh - nkv;
      auto* dst = (isk ? kc : vc) + (((int64_t)tok_seq[t] * nkv + kvh) * max_ctx + pos) * D + j * VEC;
      if constexpr (KV8) {
        static_assert(sizeof(T) == 2, "e4m3 K/V rows are built for the 16-bit types");
        if (isk) {
          *(uint4*)src = u1;
          *(uint4*)(src + half) = u2;
        }
        float f1[VEC], f2[VEC];
        Vec16<T>::unpack(u1, f1);
        Vec16<T>::unpack(u2, f2);
        *(uint2*)dst = make_uint2(sl_q8x4(f1[0], f1[1], f1[2], f1[3]), sl_q8x4(f1[4], f1[5], f1[6], f1[7]));
        *(uint2*)(dst + half) = make_uint2(sl_q8x4(f2[0], f2[1], f2[2], f2[3]), sl_q8x4(f2[4], f2[5], f2[6], f2[7]));
      } else {
        *(uint4*)dst = u1;
        *(uint4*)(dst + half) = u2;
      }
    }
  }
}

extern "C" int sl_rope_kv_append_ex(void* qkv, void* k_cache, void* v_cache, const int32_t* tok_seq, const int32_t* tok_pos,
                                    const float* cos, const float* sin, int64_t n_tok, int32_t n_heads, int32_t n_kv, int32_t D,
                                    int32_t max_ctx, int32_t dtype, int32_t kv_format, sl_stream stream) {
  if (kv_format == SL_KV_MODEL_DTYPE)
    return sl_rope_kv_append(qkv, k_cache, v_cache, tok_seq, tok_pos, cos, sin, n_tok, n_heads, n_kv, D, max_ctx, dtype, stream);
  SL_CHECK_ARG(qkv && k_cache && v_cache && tok_seq && tok_pos && cos && sin, "sl_rope_kv_append_ex: null pointer");
  SL_TRY(sl_kv_format_check("sl_rope_kv_append_ex", kv_format, dtype, D));
  if (n_tok == 0) return 0;
  const int64_t total = n_tok * (n_heads + 2 * n_kv) * (D / 2 / 8);
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 8192 ? ceil_div64(total, 256) : 8192);
  if (dtype == SL_BF16)
    hipLaunchKernelGGL((rope_kv_append_kernel<bf16_t, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv, (uint8_t*)k_cache,
                       (uint8_t*)v_cache, tok_seq, tok_pos, cos, sin, n_tok, n_heads, n_kv, D, max_ctx);
  else
    hipLaunchKernelGGL((rope_kv_append_kernel<f16_t, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (f16_t*)qkv, (uint8_t*)k_cache,
                       (uint8_t*)v_cache, tok_seq, tok_pos, cos, sin, n_tok, n_heads, n_kv, D, max_ctx);
  SL_CHECK_LAUNCH("rope_kv_append_fp8");
  return 0;
}

extern "C" int sl_rope_kv_append(void* qkv, void* k_cache, void* v_cache, const int32_t* tok_seq, const int32_t* tok_pos,
                                 const float* cos, const float* sin, int64_t n_tok, int32_t n_heads, int32_t n_kv, int32_t D,
                                 int32_t max_ctx, int32_t dtype, sl_stream stream) {
  SL_CHECK_ARG(qkv && k_cache && v_cache && tok_seq && tok_pos && cos && sin, "sl_rope_kv_append: null pointer");
  const int vec = dtype == SL_F32 ? 4 : 8;
  SL_CHECK_ARG(D % (2 * vec) == 0, "sl_rope_kv_append: head_dim=%d must be a multiple of %d", D, 2 * vec);
  if (n_tok == 0) return 0;
  const int64_t total = n_tok * (n_heads + 2 * n_kv) * (D / 2 / vec);
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 8192 ? ceil_div64(total, 256) : 8192);
  SL_DISPATCH_DTYPE_INF(dtype, T, {
    hipLaunchKernelGGL((rope_kv_append_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (T*)qkv, (T*)k_cache, (T*)v_cache,
                       tok_seq, tok_pos, cos, sin, n_tok, n_heads, n_kv, D, max_ctx);
  });
  SL_CHECK_LAUNCH("rope_kv_append");
  return 0;
}

// ----------------------------------------------------------------------------------------------
// One-token attention against the cache (decode).  Block = (kv head, sequence); the REP query heads
// that share the kv head are processed together so K and V are streamed once.
//   phase 1: scores  — a 16-lane group per key, each lane D/16 dims, xor-shuffle reduce
//   phase 2: softmax — one wave per query head over the LDS score row
//   phase 3: P.V     — 16 key groups x 16 dim chunks, LDS reduce over key groups
// ----------------------------------------------------------------------------------------------
template <typename T, int D, int REP>
__global__ __launch_bounds__(256) void attn_decode_kernel(const T* __restrict__ q, int64_t q_stride, const T* __restrict__ kc,
                                                          const T* __restrict__ vc, T* __restrict__ out, const int32_t* __restrict__ ctx_len,
                                                          int ctx_add, int nh, int nkv, int max_ctx, float scale) {
  constexpr int VEC = Vec16<T>::VEC;
  constexpr int EPL = D / 16;       // elements per lane of a 16-lane group (8 for D=128)
  constexpr int CPLN = EPL / VEC;   // 16-byte chunks per lane: 1 (bf16) or 2 (f32)
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int kvh = blockIdx.x, b = blockIdx.y;
  const int n_keys = ctx_len[b] + ctx_add;
  float* sc = dsm;                          // [REP][max_ctx]
  float* red = dsm + REP * max_ctx;         // [16][REP][D]
  float* inv_sum = red + 16 * REP * D;      // [REP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 4, gl = lane & 15;

  const T* kbase = kc + ((int64_t)b * nkv + kvh) * max_ctx * D;
  const T* vbase = vc + ((int64_t)b * nkv + kvh) * max_ctx * D;

  // phase 1
  float qr[REP][EPL];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    const T* qp = q + (int64_t)b * q_stride + (int64_t)(kvh * REP + h) * D + gl * EPL;
#pragma unroll
    for (int c = 0; c < CPLN; ++c) Vec16<T>::unpack(*(const uint4*)(qp + c * VEC), &qr[h][c * VEC]);
  }
  for (int key0 = 0; key0 < n_keys; key0 += 16) {
    const int key = key0 + wave * 4 + grp;
    const int kk = key < n_keys ? key : n_keys - 1;
    float kf[EPL];
#pragma unroll
    for (int c = 0; c < CPLN; ++c) Vec16<T>::unpack(*(const uint4*)(kbase + (int64_t)kk * D + gl * EPL + c * VEC), &kf[c * VEC]);
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) d = fmaf(qr[h][e], kf[e], d);
      d += __shfl_xor(d, 8, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 1, 64);
      if (gl == 0 && key < n_keys) sc[h * max_ctx + key] = d * scale;
    }
  }
  __syncthreads();
  // phase 2
  for (int h = wave; h < REP; h += 4) {
    float m = -INFINITY;
    for (int k = lane; k < n_keys; k += 64) m = fmaxf(m, sc[h * max_ctx + k]);
    m = wave_max(m);
    float s = 0.f;
    for (int k = lane; k < n_keys; k += 64) {
      const float p = __expf(sc[h * max_ctx + k] - m);
      sc[h * max_ctx + k] = p;
      s += p;
    }
    s = wave_sum(s);
    if (lane == 0) inv_sum[h] = 1.0f / s;
  }
  __syncthreads();
  // phase 3
  {
    const int kg = tid >> 4, dc = tid & 15;
    float acc[REP][EPL];
#pragma unroll
    for (int h = 0; h < REP; ++h)
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[h][e] = 0.f;
    for (int key = kg; key < n_keys; key += 16) {
      float vf[EPL];
#pragma unroll
      for (int c = 0; c < CPLN; ++c) Vec16<T>::unpack(*(const uint4*)(vbase + (int64_t)key * D + dc * EPL + c * VEC), &vf[c * VEC]);
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        // bf16 mode: probabilities are rounded to the storage dtype before P.V as HF eager does
        const float p = to_f32(from_f32<T>(sc[h * max_ctx + key] * inv_sum[h]));
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[h][e] = fmaf(p, vf[e], acc[h][e]);
      }
    }
#pragma unroll
    for (int h = 0; h < REP; ++h)
#pragma unroll
      for (int e = 0; e < EPL; ++e) red[(kg * REP + h) * D + dc * EPL + e] = acc[h][e];
  }
  __syncthreads();
  for (int o = tid; o < REP * D; o += 256) {
    const int h = o / D, d = o % D;
    float s = 0.f;
#pragma unroll
    for (int kg = 0; kg < 16; ++kg) s += red[(kg * REP + h) * D + d];
    out[(int64_t)b * nh * D + (int64_t)(kvh * REP + h) * D + d] = from_f32<T>(s);
  }
}

template <typename T, int REP>
static int launch_attn_decode(const void* q, int64_t q_stride, const void* kc, const void* vc, void* out, const int32_t* ctx_len,
                              int ctx_add, int B, int nh, int nkv, int max_ctx, float scale, hipStream_t st) {
  constexpr int D = 128;
  const size_t lds = ((size_t)REP * max_ctx + 16 * REP * D + REP) * sizeof(float);
  SL_CHECK_ARG(lds <= 160 * 1024, "sl_attn_decode: max_ctx=%d needs %zu B of LDS (> 160 KiB)", max_ctx, lds);
  auto kern = attn_decode_kernel<T, D, REP>;
  if (lds > 64 * 1024) SL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(nkv, B), dim3(256), lds, st, (const T*)q, q_stride, (const T*)kc, (const T*)vc, (T*)out, ctx_len, ctx_add,
                     nh, nkv, max_ctx, scale);
  SL_CHECK_LAUNCH("attn_decode");
  return 0;
}

int sl_attn_decode_impl(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, const int32_t* ctx_len,
                        int ctx_add, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale, int32_t dtype,
                        hipStream_t st) {
  SL_CHECK_ARG(q && k_cache && v_cache && out && ctx_len && B > 0, "sl_attn_decode: bad arguments");
  SL_CHECK_ARG(D == 128, "sl_attn_decode: head_dim %d not built (Llama family uses 128)", D);
  SL_CHECK_ARG(n_kv > 0 && n_heads % n_kv == 0, "sl_attn_decode: n_heads %% n_kv != 0");
  const int rep = n_heads / n_kv;
  SL_DISPATCH_DTYPE_INF(dtype, T, {
    switch (rep) {
      case 1: return launch_attn_decode<T, 1>(q, q_stride, k_cache, v_cache, out, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st);
      case 2: return launch_attn_decode<T, 2>(q, q_stride, k_cache, v_cache, out, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st);
      case 3: return launch_attn_decode<T, 3>(q, q_stride, k_cache, v_cache, out, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st);
      case 4: return launch_attn_decode<T, 4>(q, q_stride, k_cache, v_cache, out, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st);
      default: sl_set_error("sl_attn_decode: n_heads/n_kv=%d not built (1..4)", rep); return SL_ERR_UNSUPPORTED;
    }
  });
}

extern "C" int sl_attn_decode(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out,
                              const int32_t* ctx_len, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale,
                              int32_t dtype, sl_stream stream) {
  return sl_attn_decode_impl(q, q_stride, k_cache, v_cache, out, ctx_len, 0, B, n_heads, n_kv, D, max_ctx, scale, dtype, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------------------
// fragment-major weight packing (see sl_pack_weight in speechllm.h)
// ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_weight_kernel(const T* __restrict__ src, int64_t ld, T* __restrict__ dst, int N, int K) {
  constexpr int VEC = Vec16<T>::VEC;
  constexpr int KSTEP = 4 * VEC;
  const int nks = K / KSTEP;
  const int64_t total = (int64_t)((N + 15) / 16) * nks * 64;  // one 16-byte chunk per (fragment, k-step, lane)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int lane = (int)(i & 63);
    const int64_t fs = i >> 6;
    const int s = (int)(fs % nks);
    const int64_t f = fs / nks;
    const int64_t row = f * 16 + (lane & 15);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < N) v = *(const uint4*)(src + row * ld + (int64_t)s * KSTEP + (lane >> 4) * VEC);
    *(uint4*)(dst + i * VEC) = v;
  }
}

extern "C" int sl_pack_weight(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream) {
  SL_CHECK_ARG(src && dst && N > 0 && K > 0, "sl_pack_weight: bad arguments");
  const int vec = dtype == SL_F32 ? 4 : 8;
  SL_CHECK_ARG(K % (4 * vec) == 0 && ld_src % vec == 0, "sl_pack_weight: K=%d must be a multiple of %d", K, 4 * vec);
  const int64_t total = (int64_t)((N + 15) / 16) * (K / (4 * vec)) * 64;
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 16384 ? ceil_div64(total, 256) : 16384);
  SL_DISPATCH_DTYPE_INF(dtype, T, {
    hipLaunchKernelGGL((pack_weight_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)src, ld_src, (T*)dst, N, K);
  });
  SL_CHECK_LAUNCH("pack_weight");
  return 0;
}

// ----------------------------------------------------------------------------------------------
// e4m3 weight images (speechllm.h sl_pack_weight_e4m3): scales first (one wave per row: a maximum does not depend on the order it
// is taken in), then one thread per 16-byte chunk.  Both kernels and the host entry run the routines of common.h.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void w8_scales_kernel(const uint16_t* __restrict__ src, int64_t ld, float* __restrict__ scales, int N, int Np, int K, int dtype) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Np) return;
  const float m = wave_max(row < N ? sl_w8_absmax(src + (int64_t)row * ld, K, dtype, lane, 64) : 0.f);
  if (lane == 0) scales[row] = sl_w8_scale(m);
}
__global__ __launch_bounds__(256) void w8_pack_kernel(const uint16_t* __restrict__ src, int64_t ld, const float* __restrict__ scales, uint4* __restrict__ dst, int N,
                                                      int Np, int K, int dtype) {
  const int nkp = K / 64;
  const int64_t total = (int64_t)(Np / 16) * nkp * 64;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t fj = i >> 6;
    uint32_t o[4];
    sl_w8_chunk(src, ld, scales, N, dtype, fj / nkp, (int)(fj % nkp), (int)(i & 63), o);
    dst[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

static int w8_pack_check(const char* who, const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype) {
  SL_CHECK_ARG(src && dst && N > 0 && K > 0, "%s: bad arguments", who);
  if (dtype == SL_F32) {
    sl_set_error("%s: e4m3 weight images are built for bf16 / fp16 weights, not float32 (the parity mode)", who);
    return SL_ERR_UNSUPPORTED;
  }
  SL_CHECK_ARG(sl_is16(dtype), "%s: unknown dtype %d", who, dtype);
  SL_CHECK_ARG(K % 64 == 0, "%s: K=%d must be a multiple of 64 (pairs of 32-wide k-steps)", who, K);
  SL_CHECK_ARG(ld_src >= K, "%s: ld_src=%lld < K=%d", who, (long long)ld_src, K);
  SL_CHECK_ARG(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 1) == 0, "%s: dst must be 16-byte aligned", who);
  return 0;
}

extern "C" size_t sl_w8_image_bytes(int32_t N, int32_t K) {
  if (N <= 0 || K <= 0 || K % 64 != 0) { sl_set_error("sl_w8_image_bytes: N=%d K=%d (K must be a positive multiple of 64)", N, K); return 0; }
  const size_t Np = ((size_t)N + 15) / 16 * 16;
  return Np * (size_t)K + 4 * Np;
}

extern "C" int32_t sl_w8_max_rows(void) {
  const int r = sl_env().stream_min_m;      // the packed skinny range; the e4m3 kernels are built for MT 1 and 2 (<= 32 rows)
  return r < 32 ? r : 32;
}

extern "C" int sl_pack_weight_e4m3_host(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype) {
  SL_TRY(w8_pack_check("sl_pack_weight_e4m3_host", src, ld_src, dst, N, K, dtype));
  const int64_t Np = ((int64_t)N + 15) / 16 * 16;
  const int nkp = K / 64;
  const uint16_t* s = (const uint16_t*)src;
  float* scales = (float*)((unsigned char*)dst + Np * K);
  for (int64_t n = 0; n < Np; ++n) scales[n] = sl_w8_scale(n < N ? sl_w8_absmax(s + n * ld_src, K, dtype, 0, 1) : 0.f);
  uint32_t* out = (uint32_t*)dst;
  for (int64_t f = 0; f < Np / 16; ++f)
    for (int j = 0; j < nkp; ++j)
      for (int lane = 0; lane < 64; ++lane) sl_w8_chunk(s, ld_src, scales, N, dtype, f, j, lane, out + ((f * nkp + j) * 64 + lane) * 4);
  return 0;
}

extern "C" int sl_pack_weight_e4m3(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream) {
  SL_TRY(w8_pack_check("sl_pack_weight_e4m3", src, ld_src, dst, N, K, dtype));
  const int Np = (N + 15) / 16 * 16;
  float* scales = (float*)((unsigned char*)dst + (int64_t)Np * K);
  hipLaunchKernelGGL(w8_scales_kernel, dim3((Np + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, ld_src, scales, N, Np, K, dtype);
  SL_CHECK_LAUNCH("w8_scales");
  const int64_t total = (int64_t)(Np / 16) * (K / 64) * 64;
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 16384 ? ceil_div64(total, 256) : 16384);
  hipLaunchKernelGGL(w8_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, ld_src, scales, (uint4*)dst, N, Np, K, dtype);
  SL_CHECK_LAUNCH("w8_pack");
  return 0;
}

// ----------------------------------------------------------------------------------------------
// MXFP4 weight images (speechllm.h sl_pack_weight_mxfp4): the scale bytes first (one thread per 32-element block, in the order the
// bytes are stored in), then one thread per 16-byte chunk, which reads its four scale bytes as the dword the GEMM reads.  Both kernels
// and the host entry run the routines of common.h.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void w4_scales_kernel(const uint16_t* __restrict__ src, int64_t ld, uint8_t* __restrict__ sc, int N, int Np, int K, int dtype) {
  const int nkq = K / 128;
  const int64_t total = (int64_t)Np * (K / 32);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t fj = i >> 6;      // sc[f][j][r][d]
    sc[i] = (uint8_t)sl_w4_scale_byte(src, ld, N, dtype, (fj / nkq) * 16 + ((i >> 2) & 15), (int)(fj % nkq) * 4 + (int)(i & 3));
  }
}
__global__ __launch_bounds__(256) void w4_pack_kernel(const uint16_t* __restrict__ src, int64_t ld, const uint32_t* __restrict__ sc, uint4* __restrict__ dst, int N, int Np,
                                                      int K, int dtype) {
  const int nkq = K / 128;
  const int64_t total = (int64_t)(Np / 16) * nkq * 64;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t fj = i >> 6;
    uint32_t o[4];
    sl_w4_chunk(src, ld, sc[fj * 16 + (i & 15)], N, dtype, fj / nkq, (int)(fj % nkq), (int)(i & 63), o);
    dst[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

static int w4_pack_check(const char* who, const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype) {
  SL_CHECK_ARG(src && dst && N > 0 && K > 0, "%s: bad arguments", who);
  if (dtype == SL_F32) {
    sl_set_error("%s: MXFP4 weight images are built for bf16 / fp16 weights, not float32 (the parity mode)", who);
    return SL_ERR_UNSUPPORTED;
  }
  SL_CHECK_ARG(sl_is16(dtype), "%s: unknown dtype %d", who, dtype);
  SL_CHECK_ARG(K % 128 == 0, "%s: K=%d must be a multiple of 128 (quads of 32-wide k-steps)", who, K);
  SL_CHECK_ARG(ld_src >= K, "%s: ld_src=%lld < K=%d", who, (long long)ld_src, K);
  SL_CHECK_ARG(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 1) == 0, "%s: dst must be 16-byte aligned", who);
  return 0;
}

extern "C" size_t sl_w4_image_bytes(int32_t N, int32_t K) {
  if (N <= 0 || K <= 0 || K % 128 != 0) { sl_set_error("sl_w4_image_bytes: N=%d K=%d (K must be a positive multiple of 128)", N, K); return 0; }
  const size_t Np = ((size_t)N + 15) / 16 * 16;
  return Np * (size_t)K / 2 + Np * (size_t)K / 32;
}

extern "C" int32_t sl_w4_max_rows(void) { return sl_w8_max_rows(); }      // the same skinny structures (MT 1 and 2)

// the rules of a weight format (wformat.h), for callers that would otherwise restate them
extern "C" int sl_weight_format_info(int32_t code, int32_t* k_multiple, int32_t* max_rows, int32_t* w_layout) {
  const SlWFormat* f = sl_wformat(code);
  SL_CHECK_ARG(f, "sl_weight_format_info: unknown weight format %d (" SL_WFORMAT_LIST ")", code);
  if (k_multiple) *k_multiple = f->k_multiple;
  if (max_rows) *max_rows = f->max_rows ? f->max_rows() : 0;
  if (w_layout) *w_layout = f->w_layout;
  return 0;
}

extern "C" int sl_pack_weight_mxfp4_host(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype) {
  SL_TRY(w4_pack_check("sl_pack_weight_mxfp4_host", src, ld_src, dst, N, K, dtype));
  const int64_t Np = ((int64_t)N + 15) / 16 * 16;
  const int nkq = K / 128;
  const uint16_t* s = (const uint16_t*)src;
  uint8_t* sc = (uint8_t*)dst + Np * K / 2;      // a multiple of 16 bytes behind dst: the dword reads below are aligned
  for (int64_t f = 0; f < Np / 16; ++f)
    for (int j = 0; j < nkq; ++j)
      for (int r = 0; r < 16; ++r)
        for (int d = 0; d < 4; ++d) sc[((f * nkq + j) * 16 + r) * 4 + d] = (uint8_t)sl_w4_scale_byte(s, ld_src, N, dtype, f * 16 + r, 4 * j + d);
  uint32_t* out = (uint32_t*)dst;
  for (int64_t f = 0; f < Np / 16; ++f)
    for (int j = 0; j < nkq; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        const uint8_t* b = sc + ((f * nkq + j) * 16 + (lane & 15)) * 4;
        const uint32_t sc4 = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        sl_w4_chunk(s, ld_src, sc4, N, dtype, f, j, lane, out + ((f * nkq + j) * 64 + lane) * 4);
      }
  return 0;
}

extern "C" int sl_pack_weight_mxfp4(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream) {
  SL_TRY(w4_pack_check("sl_pack_weight_mxfp4", src, ld_src, dst, N, K, dtype));
  const int Np = (N + 15) / 16 * 16;
  uint8_t* sc = (uint8_t*)dst + (int64_t)Np * K / 2;
  const int64_t nsc = (int64_t)Np * (K / 32);
  const unsigned grid_s = (unsigned)(ceil_div64(nsc, 256) < 16384 ? ceil_div64(nsc, 256) : 16384);
  hipLaunchKernelGGL(w4_scales_kernel, dim3(grid_s), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, ld_src, sc, N, Np, K, dtype);
  SL_CHECK_LAUNCH("w4_scales");
  const int64_t total = (int64_t)(Np / 16) * (K / 128) * 64;
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 16384 ? ceil_div64(total, 256) : 16384);
  hipLaunchKernelGGL(w4_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, ld_src, (const uint32_t*)sc, (uint4*)dst, N, Np, K, dtype);
  SL_CHECK_LAUNCH("w4_pack");
  return 0;
}

// ----------------------------------------------------------------------------------------------
// Flash-decoding: one-token attention split over the context so that small batches still fill the chip.
//   grid (kv head, sequence, split); each block owns 64 keys: scores -> local softmax -> partial P.V,
//   and leaves (O[REP][128], m[REP], l[REP]) in fp32; a second tiny kernel merges the splits.
//   (Tried for batches that fill the chip on their own, B * n_kv >= 1024: one block per (sequence, kv head) walking the
//   context in 64-key chunks with an online softmax and the next chunk prefetched — no partial records, no merge launch —
//   was 20 % slower than split + merge at B = 128 and 256: the serial chunk chain exposes three barriers per 32 KiB.)
// ----------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_ptr3_t;
// K / V cache rows are read exactly once per decode step (one block per sequence and kv head): non-temporal loads keep them from
// displacing what other kernels re-read in L2 / the Infinity Cache and land sooner (MI355X_MICROARCH.md, nt-weights).  Measured
// (tools/time_decode_attn.py, bf16, 8 kv heads, profiles/r03_l_attn_nt.txt): 1 024 sequences x 264 keys 194.1 -> 178.3 us
// (5.77 -> 6.28 TB/s = 0.785 of the 8 TB/s peak, the rate a plain copy reaches on this chip), x 393 keys 286.5 -> 260.8 us, 512
// sequences 102.3 -> 92.1 us, 64 sequences 17.3 -> 16.1 us.
#ifndef SL_KV_NT
#define SL_KV_NT 1
#endif
#if SL_KV_NT
#define SL_KV_LOAD(ptr) __builtin_nontemporal_load((const u32x4_t*)(ptr))
#define SL_KV_LOAD8(ptr) __builtin_nontemporal_load((const u32x2_t*)(ptr))
#else
#define SL_KV_LOAD(ptr) (*(const u32x4_t*)(ptr))
#define SL_KV_LOAD8(ptr) (*(const u32x2_t*)(ptr))
#endif
// e4m3 K/V rows (KVT = uint8_t; 16-bit T only): a thread's 8-element chunk of a row is 8 bytes instead of 16, held as loaded and
// widened to T (exactly: sl_dq8x8) where the 16-bit kernels copy their registers to LDS.  Everything behind that copy — tile
// images, MFMA steps, softmax, records — is the 16-bit kernel's.
template <typename T, typename KVT> struct KvRow {
  using raw_t = u32x4_t;
  static __device__ __forceinline__ raw_t load(const KVT* p) { return SL_KV_LOAD(p); }
  static __device__ __forceinline__ u32x4_t widen(const raw_t& r) { return r; }
};
template <typename T> struct KvRow<T, uint8_t> {
  using raw_t = u32x2_t;
  static __device__ __forceinline__ raw_t load(const uint8_t* p) { return SL_KV_LOAD8(p); }
  static __device__ __forceinline__ u32x4_t widen(const raw_t& r) { return sl_dq8x8<T>(r); }
};
// floats per partial record (REP x 128 outputs, REP maxima, REP sums), rounded up to whole 128-byte lines so that the records of
// different (sequence, kv head, split) blocks never share a line (the in-launch merge hands them between workgroups with sc1 stores)
constexpr int split_record_floats(int rep) { return (rep * 128 + 2 * rep + 31) / 32 * 32; }
constexpr int DSPLIT = 64;  // keys per block (KS = 128 for batches that fill the chip anyway: half the records to merge)

// Partial records handed from the split blocks to the block that merges them INSIDE the launch (cnt != nullptr): every record
// word is stored with sc1 (agent scope: through the XCD's non-coherent L2 to the memory side), drained with s_waitcnt before the
// arrival counter is bumped, and re-read with sc1 loads by the block whose add came last (MI355X_MICROARCH.md, Correctness
// boundaries; the same hand-off as gemm_stream.hip's K-split fix-up).  The merge is attn_decode_combine_kernel's arithmetic in
// its order (splits ascending), so both forms give the same bits.
__device__ __forceinline__ void st_rec(float* p, float v, bool sc1) {
  if (sc1) asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  else *p = v;
}
// agent-scope relaxed load = global_load_dword ... sc1: re-reads a word another workgroup of this launch stored with sc1; the compiler
// keeps several in flight (an asm load + wait per word serialised ~28 memory-side round trips per merge)
__device__ __forceinline__ float ld_rec_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the last of a (sequence, kv head)'s `nsplit` blocks to arrive merges their records and writes the REP heads' outputs
template <typename T, int REP>
__device__ __forceinline__ void split_arrive_and_merge(float* __restrict__ part, int32_t* __restrict__ cnt, T* __restrict__ out, int b, int kvh, int nkv,
                                                        int nsplit) {
  constexpr int D = 128, PSTRIDE = split_record_floats(REP), U = 8;
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's record stores have reached the memory side
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = atomicAdd(&cnt[b * nkv + kvh], 1);
    s_last = old == nsplit - 1;
    if (old == nsplit - 1) cnt[b * nkv + kvh] = 0;     // leave the counter as it was found: zero between launches
  }
  __syncthreads();
  if (!s_last) return;
  const float* base = part + ((int64_t)b * nkv + kvh) * nsplit * PSTRIDE;
  for (int o = threadIdx.x; o < REP * D; o += 256) {
    const int h = o / D, d = o % D;
    float M = -INFINITY;
    for (int s0 = 0; s0 < nsplit; s0 += U) {
      float mv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int sp2 = s0 + u < nsplit ? s0 + u : nsplit - 1;
        mv[u] = ld_rec_sc1(base + (int64_t)sp2 * PSTRIDE + REP * D + h);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) M = fmaxf(M, mv[u]);
    }
    float Lsum = 0.f, acc = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += U) {
      float mv[U], lv[U], ov[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int sp2 = s0 + u < nsplit ? s0 + u : nsplit - 1;
        const float* rec = base + (int64_t)sp2 * PSTRIDE;
        mv[u] = ld_rec_sc1(rec + REP * D + h);
        lv[u] = ld_rec_sc1(rec + REP * D + REP + h);
        ov[u] = ld_rec_sc1(rec + h * D + d);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (s0 + u >= nsplit || mv[u] == -INFINITY) continue;
        const float w = __expf(mv[u] - M);
        Lsum += w * lv[u];
        acc += w * ov[u];
      }
    }
    out[((int64_t)b * nkv * REP + kvh * REP + h) * D + d] = from_f32<T>(Lsum > 0.f ? acc / Lsum : 0.f);
  }
}

// KVT = uint8_t: e4m3 rows (KvRow).  Those instances also read positions below shared_prefix from slot 0, as the single-pass form
// does; the 16-bit instances ignore shared_prefix as before (every slot holds the prefix rows there, so the results agree).
template <typename T, int REP, int KS, typename KVT = T>
__global__ __launch_bounds__(256) void attn_decode_split_kernel(const T* __restrict__ q, int64_t q_stride, const KVT* __restrict__ kc,
                                                                const KVT* __restrict__ vc, float* __restrict__ part,
                                                                const int32_t* __restrict__ ctx_len, int ctx_add, int nkv, int max_ctx,
                                                                float scale, int32_t* __restrict__ cnt, T* __restrict__ out, int shared_prefix) {
  constexpr int D = 128;
  constexpr bool KV8 = !std::is_same_v<KVT, T>;
  static_assert(!KV8 || sizeof(T) == 2, "e4m3 K/V rows are built for the 16-bit types");
  using Row = KvRow<T, KVT>;
  constexpr int VEC = Vec16<T>::VEC;
  constexpr int EPL = D / 16, CPLN = EPL / VEC;
  constexpr int PSTRIDE = split_record_floats(REP);  // floats per partial record
  constexpr int NPS = KS / 16;   // passes of 16 keys
  constexpr bool MFMA_QK = sizeof(T) == 2;   // bf16: scores on the matrix core (the VALU form was ~75 % VALU-busy at B = 256)
  constexpr int KT_BYTES = MFMA_QK ? KS * D * (int)sizeof(T) : 16, RED_BYTES = 16 * REP * D * (int)sizeof(float);
  __shared__ float sc[REP][KS];
  // bf16: K tile of the score MFMAs ([KS rows][256 B], chunk c of row r at c ^ (r & 15)), then — same bytes — the V tile of
  // the P.V MFMAs ([KS rows][256 B], chunk c of row r at voff()); fp32: the cross-thread reduction buffer of the VALU form
  __shared__ __attribute__((aligned(16))) unsigned char un[KT_BYTES > RED_BYTES ? KT_BYTES : RED_BYTES];
  constexpr int PROW = KS * 2 + 16;   // bytes per row of the bf16 probability tile (padded: rows land on different banks)
  __shared__ __attribute__((aligned(16))) unsigned char pt[MFMA_QK ? 16 * PROW : 16];
  float (*red)[REP][D] = (float (*)[REP][D])un;
  const int kvh = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, gl = lane & 15;
  const int n_keys = ctx_len[b] + ctx_add;
  const int k0 = sp * KS;
  float* rec = part + (((int64_t)b * nkv + kvh) * nsplit + sp) * PSTRIDE;
  const bool fuse = cnt != nullptr;      // merge inside this launch (no combine kernel)
  if (k0 >= n_keys) {  // empty split: neutral record
    if (tid < REP) { st_rec(rec + REP * D + tid, -INFINITY, fuse); st_rec(rec + REP * D + REP + tid, 0.f, fuse); }
    if (fuse) split_arrive_and_merge<T, REP>(part, cnt, out, b, kvh, nkv, nsplit);
    return;
  }
  const int nk = (n_keys - k0) < KS ? (n_keys - k0) : KS;
  const KVT* kbase = kc + (((int64_t)b * nkv + kvh) * max_ctx + k0) * D;
  const KVT* vbase = vc + (((int64_t)b * nkv + kvh) * max_ctx + k0) * D;
  const KVT* kbase0 = kc + ((int64_t)kvh * max_ctx + k0) * D;   // slot 0 (KV8: positions below shared_prefix)
  const KVT* vbase0 = vc + ((int64_t)kvh * max_ctx + k0) * D;

  // phase 1: scores; every K and V row of the split is requested up front (16-byte chunks, 256-byte rows coalesced)
  typename Row::raw_t kraw[NPS][CPLN];   // ext-vector type: HIP's uint4 struct copies to LDS went through scratch
#pragma unroll
  for (int ps = 0; ps < NPS; ++ps) {
    int key = ps * 16 + wave * 4 + grp;
    key = key < nk ? key : nk - 1;
#pragma unroll
    for (int c = 0; c < CPLN; ++c) kraw[ps][c] = Row::load(((KV8 && k0 + key < shared_prefix) ? kbase0 : kbase) + (int64_t)key * D + gl * EPL + c * VEC);
  }
  // V rows for phase 3 are requested now: their HBM latency hides behind the score / softmax phases
  const int kg = tid >> 4, dc = tid & 15;
  typename Row::raw_t vraw[NPS][CPLN];
#pragma unroll
  for (int ps = 0; ps < NPS; ++ps) {
    int key = kg + 16 * ps;
    key = key < nk ? key : nk - 1;
#pragma unroll
    for (int c = 0; c < CPLN; ++c) vraw[ps][c] = Row::load(((KV8 && k0 + key < shared_prefix) ? vbase0 : vbase) + (int64_t)key * D + dc * EPL + c * VEC);
  }
  if constexpr (MFMA_QK) {
    // S[head][key] = Q . K^T on the matrix core: A = the REP query heads of this kv head (rows REP..15 zero), B = 16 keys
    // from the LDS tile; wave w scores keys [w KS/4, (w+1) KS/4).  Lanes 0..15 end up holding heads 0..3 of their key.
    const int r = lane & 15, q4 = lane >> 4;
    uint4 qf[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
      qf[s4] = r < REP ? *(const uint4*)(q + (int64_t)b * q_stride + (int64_t)(kvh * REP + r) * D + 32 * s4 + 8 * q4) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      const int kl = ps * 16 + wave * 4 + grp;
      *(u32x4_t*)(un + kl * 256 + ((gl ^ (kl & 15)) << 4)) = Row::widen(kraw[ps][0]);
    }
    __syncthreads();
    constexpr int NF = KS / 64;
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      const int rowbase = wave * (KS / 4) + n * 16;
      f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const uint4 kf = *(const uint4*)(un + (rowbase + r) * 256 + (((4 * s4 + q4) ^ r) << 4));
        MMA<T>::step(sacc, qf[s4], kf);
      }
      if (q4 == 0) {
        const int key = rowbase + r;
#pragma unroll
        for (int h = 0; h < REP; ++h) sc[h][key] = key < nk ? sacc[h] * scale : -INFINITY;
      }
    }
  } else {
    float qr[REP][EPL];
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      const T* qp = q + (int64_t)b * q_stride + (int64_t)(kvh * REP + h) * D + gl * EPL;
#pragma unroll
      for (int c = 0; c < CPLN; ++c) Vec16<T>::unpack(*(const uint4*)(qp + c * VEC), &qr[h][c * VEC]);
    }
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      const int key = ps * 16 + wave * 4 + grp;
      float kf[EPL];
#pragma unroll
      for (int c = 0; c < CPLN; ++c) {
        const u32x4_t kr = Row::widen(kraw[ps][c]);
        Vec16<T>::unpack(make_uint4(kr.x, kr.y, kr.z, kr.w), &kf[c * VEC]);
      }
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) d = fmaf(qr[h][e], kf[e], d);
        d += __shfl_xor(d, 8, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 1, 64);
        if (gl == 0) sc[h][key] = key < nk ? d * scale : -INFINITY;
      }
    }
  }
  __syncthreads();
  // phase 2: local softmax, one wave per head, one key per lane
  for (int h = wave; h < REP; h += 4) {
    float sv[KS / 64], m = -INFINITY;
#pragma unroll
    for (int j = 0; j < KS / 64; ++j) { sv[j] = sc[h][lane + 64 * j]; m = fmaxf(m, sv[j]); }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < KS / 64; ++j) {
      const float p = __expf(sv[j] - m);  // masked keys: exp(-inf) = 0
      if constexpr (MFMA_QK) *(T*)(pt + h * PROW + (lane + 64 * j) * 2) = from_f32<T>(p);   // P rounded to bf16, as HF eager does
      else sc[h][lane + 64 * j] = p;
      l += p;
    }
    l = wave_sum(l);
    if (lane == 0) { st_rec(rec + REP * D + h, m, fuse); st_rec(rec + REP * D + REP + h, l, fuse); }
  }
  if constexpr (MFMA_QK) {
    // phase 3 on the matrix core: O[head][dim] = P . V with V consumed column-wise by ds_read_b64_tr_b16 (a 16-lane group
    // reads a 4-key x 16-dim block and receives it transposed: lane i gets the 4 keys of dim i).  V tile image: chunk c of
    // row r at c ^ (((r & 3) << 2) | ((r >> 2) & 3)) — conflict-free for these reads (guide T10, image (b)).
    auto voff = [](int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); };
    for (int o = tid; o < (16 - REP) * (KS / 8); o += 256)   // zero the padding rows of P (heads REP..15)
      *(uint4*)(pt + (REP + o / (KS / 8)) * PROW + (o % (KS / 8)) * 16) = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) *(u32x4_t*)(un + voff(kg + 16 * ps, dc)) = Row::widen(vraw[ps][0]);   // K tile is dead: scores are in sc
    __syncthreads();
    const int r = lane & 15, q4 = lane >> 4, qq = r >> 2, pp = r & 3;
    const uint32_t ub = (uint32_t)(uintptr_t)(lds_ptr3_t)un;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int df = 2 * wave + j;   // 16-dim fragment of the head dimension
      f32x4 oacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS / 32; ++ks) {
        const uint4 pa = *(const uint4*)(pt + r * PROW + (32 * ks + 8 * q4) * 2);
        const int r0 = 32 * ks + 8 * q4 + qq;
        u32x2_t lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(ub + (uint32_t)(voff(r0, 2 * df + (pp >> 1)) + 8 * (pp & 1))) : "memory");
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(ub + (uint32_t)(voff(r0 + 4, 2 * df + (pp >> 1)) + 8 * (pp & 1))) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo), "+v"(hi));
        MMA<T>::step(oacc, pa, make_uint4(lo.x, lo.y, hi.x, hi.y));
      }
      if (q4 == 0) {
#pragma unroll
        for (int h = 0; h < REP; ++h) st_rec(rec + h * D + df * 16 + r, oacc[h], fuse);
      }
    }
    if (fuse) split_arrive_and_merge<T, REP>(part, cnt, out, b, kvh, nkv, nsplit);
    return;
  }
  __syncthreads();
  // phase 3: partial P.V
  {
    float acc[REP][EPL];
#pragma unroll
    for (int h = 0; h < REP; ++h)
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[h][e] = 0.f;
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      const int key = kg + 16 * ps;
      float vf[EPL];
#pragma unroll
      for (int c = 0; c < CPLN; ++c) {
        const u32x4_t vr = Row::widen(vraw[ps][c]);
        Vec16<T>::unpack(make_uint4(vr.x, vr.y, vr.z, vr.w), &vf[c * VEC]);
      }
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float p = sc[h][key];  // 0 for keys past nk
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[h][e] = fmaf(p, vf[e], acc[h][e]);
      }
    }
#pragma unroll
    for (int h = 0; h < REP; ++h)
#pragma unroll
      for (int e = 0; e < EPL; ++e) red[kg][h][dc * EPL + e] = acc[h][e];
  }
  __syncthreads();
  for (int o = tid; o < REP * D; o += 256) {
    const int h = o / D, d = o % D;
    float s = 0.f;
#pragma unroll
    for (int kg = 0; kg < 16; ++kg) s += red[kg][h][d];
    st_rec(rec + h * D + d, s, fuse);
  }
  if (fuse) split_arrive_and_merge<T, REP>(part, cnt, out, b, kvh, nkv, nsplit);
}

// Single-pass form (bf16, B * n_kv >= 32): one block per (sequence, kv head)
// walks the context in 128-key chunks with an online softmax, all products on the matrix core as in the split kernel.  No
// partial records, no merge launch.  PREFETCH = false (used): a chunk's K rows are requested at its start and its V rows as
// soon as the K registers are free (138 VGPRs, 3 blocks per CU, other blocks cover the latency): 97 us per layer at B = 512;
// PREFETCH = true holds the next chunk's K and V rows in a second register set (239 VGPRs, 2 blocks per CU): 104 us.
// Four blocks per CU (query fragments and a shared zero row in LDS: 128 VGPRs + 16 B of scratch, 36 KiB) would make 4096 blocks exactly
// four rounds instead of 5.33 on 768 slots, but measured 117 us: the extra LDS reads per MFMA and the fourth block's traffic cost more
// than the idle third of the last round.
// KS_ = keys per chunk.  128 (default): the measurements above.  64: 19.4 KiB of LDS and ~100 VGPRs per block instead of 38 KiB / 138 —
// small enough to sit on a CU BESIDE a 256 x 256 GEMM block of another stream (130 of the 160 KiB of LDS, half the register file):
// the HBM-bound attention of one in-flight batch can then run under the matrix-core-bound encode / prefill of the other
// (SL_ATTN_DECODE_KS=64; DESIGN §8.10 has what it measured).
// KVT = uint8_t: e4m3 rows (KvRow): 8-byte loads, the K / V registers hold half the dwords, the LDS images are unchanged.
// TAIL = true (sl_attn_decode_grouped's second pass; rec / prefix_len are NULL and unread otherwise): the walk starts at key prefix_len[b]
// instead of 0, and the running maximum, sum and output start from the fp32 record {O[128], m, l} the prefix pass left for every
// (row, head) instead of -inf / 0 / 0 — the row's prompt keys live in another slot and were folded in there.
constexpr int GROUP_REC_FLOATS = 136;      // O[128], m, l, padded to whole 32-byte sectors
template <typename T, int REP, bool PREFETCH, int KS_ = 128, typename KVT = T, bool TAIL = false>
__global__ __launch_bounds__(256) void attn_decode_full_kernel(const T* __restrict__ q, int64_t q_stride, const KVT* __restrict__ kc,
                                                               const KVT* __restrict__ vc, T* __restrict__ out,
                                                               const int32_t* __restrict__ ctx_len, int ctx_add, int nh, int nkv, int max_ctx,
                                                               float scale, int shared_prefix, const float* __restrict__ rec,
                                                               const int32_t* __restrict__ prefix_len) {
  static_assert(sizeof(T) == 2, "the single-pass form is built for the 16-bit types (bf16 / fp16)");
  constexpr int D = 128, KS = KS_, NPS = KS / 16;
  static_assert(KS == 64 || KS == 128, "chunks of 64 or 128 keys");
  constexpr int PROW = KS * 2 + 16;
  __shared__ float sc[REP][KS];
  __shared__ float alpha[4], linv[4];
  __shared__ __attribute__((aligned(16))) unsigned char un[KS * D * 2];   // K tile, then V tile
  __shared__ __attribute__((aligned(16))) unsigned char pt[16 * PROW];
  const int kvh = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, gl = lane & 15;
  const int kg = tid >> 4, dc = tid & 15;
  const int r = lane & 15, q4 = lane >> 4, qq = r >> 2, pp = r & 3;
  const int n_keys = ctx_len[b] + ctx_add;
  int k_begin = 0;
  if constexpr (TAIL) k_begin = prefix_len[b];
  using Row = KvRow<T, KVT>;
  const KVT* kbase = kc + ((int64_t)b * nkv + kvh) * max_ctx * D;
  const KVT* vbase = vc + ((int64_t)b * nkv + kvh) * max_ctx * D;
  // positions below shared_prefix hold the same rows in every slot (the caller's promise: one prompt prefix for the whole batch);
  // every block reads them from slot 0, so they come out of L2 instead of HBM.  Measured (tools/time_decode_step.py 1024 with
  // SHARED_PREFIX=9, three A/B rounds on one box, profiles/r04_w_shared_prefix.txt): decode step 11.08 -> 10.82 ms; the same rows
  // through plain (not non-temporal) loads behind a per-load branch: 11.30 ms, slower than no sharing.
  const KVT* kbase0 = kc + (int64_t)kvh * max_ctx * D;
  const KVT* vbase0 = vc + (int64_t)kvh * max_ctx * D;
  auto voff = [](int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); };

  uint4 qf[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4)
    qf[s4] = r < REP ? *(const uint4*)(q + (int64_t)b * q_stride + (int64_t)(kvh * REP + r) * D + 32 * s4 + 8 * q4) : make_uint4(0, 0, 0, 0);
  for (int o = tid; o < (16 - REP) * (KS / 8); o += 256)   // padding rows of P (heads REP..15) stay zero
    *(uint4*)(pt + (REP + o / (KS / 8)) * PROW + (o % (KS / 8)) * 16) = make_uint4(0, 0, 0, 0);

  typename Row::raw_t kraw[PREFETCH ? 2 : 1][NPS], vraw[PREFETCH ? 2 : 1][NPS];
  auto fetch_k = [&](int buf, int k0) {   // rows past the context are clamped (their scores are masked)
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      int key = k0 + ps * 16 + wave * 4 + grp; key = key < n_keys ? key : n_keys - 1;
      kraw[buf][ps] = Row::load((key < shared_prefix ? kbase0 : kbase) + (int64_t)key * D + gl * 8);
    }
  };
  auto fetch_v = [&](int buf, int k0) {
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      int key = k0 + kg + 16 * ps; key = key < n_keys ? key : n_keys - 1;
      vraw[buf][ps] = Row::load((key < shared_prefix ? vbase0 : vbase) + (int64_t)key * D + dc * 8);
    }
  };
  auto fetch = [&](int buf, int k0) { fetch_k(buf, k0); fetch_v(buf, k0); };
  f32x4 oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float m_run = -INFINITY, l_run = 0.f;   // live in wave h (< REP), replicated over its lanes
  const uint32_t ub = (uint32_t)(uintptr_t)(lds_ptr3_t)un;
  if constexpr (TAIL) {
    if (k_begin > 0) {
      const float* rb = rec + ((int64_t)b * nh + kvh * REP) * GROUP_REC_FLOATS;
      if (wave < REP) { m_run = rb[wave * GROUP_REC_FLOATS + D]; l_run = rb[wave * GROUP_REC_FLOATS + D + 1]; }
      if (q4 == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int h = 0; h < REP; ++h) oacc[j][h] = rb[h * GROUP_REC_FLOATS + (2 * wave + j) * 16 + r];
      }
    }
  }
  const int nchunk = (n_keys - k_begin + KS - 1) / KS;
  if constexpr (PREFETCH) fetch(0, k_begin);
  for (int c0 = 0; c0 < nchunk; c0 += 2) {
#pragma unroll
    for (int u2 = 0; u2 < 2; ++u2) {
      constexpr int dummy = 0; (void)dummy;
      const int u = PREFETCH ? u2 : 0;
      const int ci = c0 + u2;
      if (ci >= nchunk) break;
      const int k0 = k_begin + ci * KS;
      if constexpr (PREFETCH) { if (ci + 1 < nchunk) fetch(u ^ 1, k0 + KS); }
      else fetch_k(0, k0);
      // K tile -> LDS -> scores on the matrix core
#pragma unroll
      for (int ps = 0; ps < NPS; ++ps) {
        const int kl = ps * 16 + wave * 4 + grp;
        *(u32x4_t*)(un + kl * 256 + ((gl ^ (kl & 15)) << 4)) = Row::widen(kraw[u][ps]);
      }
      if constexpr (!PREFETCH) fetch_v(0, k0);   // K registers are free again: V rows fly under the score / softmax phases
      __syncthreads();
#pragma unroll
      for (int n = 0; n < KS / 64; ++n) {
        const int rowbase = wave * (KS / 4) + n * 16;
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const uint4 kf = *(const uint4*)(un + (rowbase + r) * 256 + (((4 * s4 + q4) ^ r) << 4));
          MMA<T>::step(sacc, qf[s4], kf);
        }
        if (q4 == 0) {
          const int key = rowbase + r;
#pragma unroll
          for (int h = 0; h < REP; ++h) sc[h][key] = (k0 + key) < n_keys ? sacc[h] * scale : -INFINITY;
        }
      }
      __syncthreads();
      // online softmax: wave h owns head h (two keys per lane); P rounded to bf16 as HF eager does
      if (wave < REP) {
        const float s0 = sc[wave][lane], s1 = KS == 128 ? sc[wave][(lane + 64) & (KS - 1)] : -INFINITY;
        const float m_new = fmaxf(m_run, wave_max(fmaxf(s0, s1)));   // finite: key k0 is inside the context
        const float p0 = __expf(s0 - m_new), p1 = KS == 128 ? __expf(s1 - m_new) : 0.f;
        const float a = __expf(m_run - m_new);                        // first chunk: exp(-inf) = 0
        l_run = l_run * a + wave_sum(p0 + p1);
        m_run = m_new;
        *(T*)(pt + wave * PROW + lane * 2) = from_f32<T>(p0);
        if constexpr (KS == 128) *(T*)(pt + wave * PROW + (lane + 64) * 2) = from_f32<T>(p1);
        if (lane == 0) alpha[wave] = a;
      }
      // V tile over the (dead) K tile
#pragma unroll
      for (int ps = 0; ps < NPS; ++ps) *(u32x4_t*)(un + voff(kg + 16 * ps, dc)) = Row::widen(vraw[u][ps]);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int df = 2 * wave + j;
#pragma unroll
        for (int h = 0; h < REP; ++h) oacc[j][h] *= alpha[h];
#pragma unroll
        for (int ks = 0; ks < KS / 32; ++ks) {
          const uint4 pa = *(const uint4*)(pt + r * PROW + (32 * ks + 8 * q4) * 2);
          const int r0 = 32 * ks + 8 * q4 + qq;
          u32x2_t lo, hi;
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(ub + (uint32_t)(voff(r0, 2 * df + (pp >> 1)) + 8 * (pp & 1))) : "memory");
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(ub + (uint32_t)(voff(r0 + 4, 2 * df + (pp >> 1)) + 8 * (pp & 1))) : "memory");
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo), "+v"(hi));
          MMA<T>::step(oacc[j], pa, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
      }
      __syncthreads();   // un / pt / sc / alpha are rewritten by the next chunk
    }
  }
  if (wave < REP && lane == 0) linv[wave] = l_run > 0.f ? 1.0f / l_run : 0.f;
  __syncthreads();
  if (q4 == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int h = 0; h < REP; ++h)
        out[(int64_t)b * nh * D + (int64_t)(kvh * REP + h) * D + (2 * wave + j) * 16 + r] = from_f32<T>(oacc[j][h] * linv[h]);
  }
}

template <typename T>
__global__ __launch_bounds__(128) void attn_decode_combine_kernel(const float* __restrict__ part, T* __restrict__ out, int nh, int nkv,
                                                                  int nsplit) {
  constexpr int D = 128;
  const int b = blockIdx.y, head = blockIdx.x, d = threadIdx.x;
  const int rep = nh / nkv, kvh = head / rep, h = head % rep;
  const int pstride = split_record_floats(rep);
  const float* base = part + ((int64_t)b * nkv + kvh) * nsplit * pstride;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[(int64_t)s * pstride + rep * D + h]);
  float L = 0.f, o = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* rec = base + (int64_t)s * pstride;
    const float m = rec[rep * D + h];
    if (m == -INFINITY) continue;
    const float w = __expf(m - M);
    L += w * rec[rep * D + rep + h];
    o += w * rec[h * D + d];
  }
  out[((int64_t)b * nh + head) * D + d] = from_f32<T>(L > 0.f ? o / L : 0.f);
}

// workspace = the partial records, then (256-byte aligned) one arrival counter per (sequence, kv head) for the in-launch merge
static size_t attn_split_records_bytes(int B, int n_heads, int n_kv, int max_ctx) {
  const int rep = n_heads / n_kv, nsplit = (max_ctx + DSPLIT - 1) / DSPLIT;   // sized for the finer split
  return ((size_t)B * n_kv * nsplit * split_record_floats(rep) * sizeof(float) + 255) & ~(size_t)255;
}
size_t sl_attn_decode_split_ws(int B, int n_heads, int n_kv, int max_ctx) {
  return attn_split_records_bytes(B, n_heads, n_kv, max_ctx) + (((size_t)B * n_kv * sizeof(int32_t) + 255) & ~(size_t)255);
}
// The counters must be zero when a launch starts; every launch leaves them zero.  The owner of the workspace zeroes them once
// (the decode runtime: at the start of a generate / decode-step call, outside the captured graph).
int sl_attn_decode_split_zero_counters(void* workspace, int B, int n_heads, int n_kv, int max_ctx, hipStream_t st) {
  SL_HIP(hipMemsetAsync((unsigned char*)workspace + attn_split_records_bytes(B, n_heads, n_kv, max_ctx), 0, (size_t)B * n_kv * sizeof(int32_t), st));
  return 0;
}

template <typename T, int REP, typename KVT = T>
static int launch_attn_decode_split(const void* q, int64_t q_stride, const void* kc, const void* vc, void* out, float* part,
                                    const int32_t* ctx_len, int ctx_add, int B, int nh, int nkv, int max_ctx, float scale, hipStream_t st,
                                    int32_t* cnt, int shared_prefix) {
  constexpr bool KV8 = !std::is_same_v<KVT, T>;
  if constexpr (sizeof(T) == 2) {
    const int64_t full_min = sl_env().attn_full_min;   // tuning switch: (sequence, kv head) pairs from which the single-pass form runs; measured faster than split + merge from B = 4 up (9.1 vs 11.4 us), 97 vs 127 us at B = 512
    // ... except long caches at batches that leave the chip under-filled: a block of the single-pass form walks its whole context in
    // 128-key chunks one after the other (16 sequences x 8 kv heads = 128 blocks, up to 14 chunks each at 1 800 keys), the split
    // form spreads the same keys over (sequence, kv head, 64 keys) blocks: long-form leg of bench.py (16 utterances of 30-120 s,
    // contexts up to 1 782) decode 680 -> 627 ms; at contexts of a few hundred keys the single pass stays ahead (1.88 vs 1.94 ms
    // per step at 16 sequences, 709 vs 743 ms for the Whisper leg's 32 sequences)
    const int64_t Bf = sl_family_rows(B);              // the form follows the pinned family's rows (common.h sl_family_rows)
    const bool long_thin = max_ctx >= 1024 && Bf * nkv < 768;
    if (Bf * nkv >= full_min && !long_thin && !sl_env().attn_force_split) {
      if constexpr (KV8)     // e4m3 rows: the 128-key form only (SL_ATTN_DECODE_KS is a 16-bit experiment)
        hipLaunchKernelGGL((attn_decode_full_kernel<T, REP, false, 128, KVT>), dim3(nkv, B), dim3(256), 0, st, (const T*)q, q_stride, (const KVT*)kc,
                           (const KVT*)vc, (T*)out, ctx_len, ctx_add, nh, nkv, max_ctx, scale, shared_prefix, nullptr, nullptr);
      else if (sl_env().attn_decode_ks == 65)        // 64-key chunks with the NEXT chunk's K / V rows held in a second register set (twice the bytes in flight per block)
        hipLaunchKernelGGL((attn_decode_full_kernel<T, REP, true, 64>), dim3(nkv, B), dim3(256), 0, st, (const T*)q, q_stride, (const T*)kc,
                           (const T*)vc, (T*)out, ctx_len, ctx_add, nh, nkv, max_ctx, scale, shared_prefix, nullptr, nullptr);
      else if (sl_env().attn_decode_ks == 64)
        hipLaunchKernelGGL((attn_decode_full_kernel<T, REP, false, 64>), dim3(nkv, B), dim3(256), 0, st, (const T*)q, q_stride, (const T*)kc,
                           (const T*)vc, (T*)out, ctx_len, ctx_add, nh, nkv, max_ctx, scale, shared_prefix, nullptr, nullptr);
      else
        hipLaunchKernelGGL((attn_decode_full_kernel<T, REP, false>), dim3(nkv, B), dim3(256), 0, st, (const T*)q, q_stride, (const T*)kc,
                           (const T*)vc, (T*)out, ctx_len, ctx_add, nh, nkv, max_ctx, scale, shared_prefix, nullptr, nullptr);
      SL_CHECK_LAUNCH("attn_decode_full");
      return 0;
    }
  }
  int nsplit;
  if ((int64_t)sl_family_rows(B) * nkv >= 512) {
    nsplit = (max_ctx + 127) / 128;
    hipLaunchKernelGGL((attn_decode_split_kernel<T, REP, 128, KVT>), dim3(nkv, B, nsplit), dim3(256), 0, st, (const T*)q, q_stride, (const KVT*)kc,
                       (const KVT*)vc, part, ctx_len, ctx_add, nkv, max_ctx, scale, cnt, (T*)out, shared_prefix);
  } else {
    nsplit = (max_ctx + DSPLIT - 1) / DSPLIT;
    hipLaunchKernelGGL((attn_decode_split_kernel<T, REP, DSPLIT, KVT>), dim3(nkv, B, nsplit), dim3(256), 0, st, (const T*)q, q_stride, (const KVT*)kc,
                       (const KVT*)vc, part, ctx_len, ctx_add, nkv, max_ctx, scale, cnt, (T*)out, shared_prefix);
  }
  SL_CHECK_LAUNCH("attn_decode_split");
  if (cnt) return 0;   // the last block of every (sequence, kv head) merged its records
  hipLaunchKernelGGL((attn_decode_combine_kernel<T>), dim3(nh, B), dim3(128), 0, st, part, (T*)out, nh, nkv, nsplit);
  SL_CHECK_LAUNCH("attn_decode_combine");
  return 0;
}

// counters: 0 = separate combine launch; 1 = merge inside the split launch, the caller has zeroed the counters
// (sl_attn_decode_split_zero_counters) on this stream; 2 = the same, zeroing them here first (one memset per call)
int sl_attn_decode_split_impl(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                              const int32_t* ctx_len, int ctx_add, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx,
                              float scale, int32_t dtype, hipStream_t st, int counters, int shared_prefix, int kv_format) {
  SL_CHECK_ARG(q && k_cache && v_cache && out && workspace && ctx_len && B > 0, "sl_attn_decode_split: bad arguments");
  SL_TRY(sl_kv_format_check("sl_attn_decode_split", kv_format, dtype, D));
  SL_CHECK_ARG(D == 128, "sl_attn_decode_split: head_dim %d not built (128)", D);
  SL_CHECK_ARG(n_kv > 0 && n_heads % n_kv == 0, "sl_attn_decode_split: n_heads %% n_kv != 0");
  SL_CHECK_ARG(shared_prefix >= 0 && shared_prefix <= max_ctx, "sl_attn_decode_split: shared_prefix %d outside [0, max_ctx=%d]", shared_prefix, max_ctx);
  float* part = (float*)workspace;
  const int rep = n_heads / n_kv;
  // Measured (tools/time_decode_step.py, Llama-3.2-3B, 128 new tokens, 7 splits x 8 kv heads): merged in-launch 1.5725 / 1.5884 / 1.5922 ms
  // per step at batch 1 / 2 / 3 against 1.6136 / 1.6213 / 1.6303 ms with the separate combine launch (the merge costs an arrival-counter
  // round trip plus two batches of sc1 re-reads, ~3 us, the launch boundary + combine kernel ~4.5 us).  A first version that waited
  // for every sc1 load on its own was SLOWER than the combine launch (1.778 vs 1.640 ms per token).  Default: merge where the split
  // path serves small batches (B * n_kv <= 32); large fp32 batches keep the combine launch (one counter per (sequence, kv head)).
  // SL_ATTN_SPLIT_MERGE = 0 / 1 forces it off / on.
  const int mode = sl_env().attn_split_merge;
  if (mode == 0 || (mode < 0 && (int64_t)sl_family_rows(B) * n_kv > 32)) counters = 0;
  int32_t* cnt = counters ? (int32_t*)((unsigned char*)workspace + attn_split_records_bytes(B, n_heads, n_kv, max_ctx)) : nullptr;
  if (counters == 2) SL_TRY(sl_attn_decode_split_zero_counters(workspace, B, n_heads, n_kv, max_ctx, st));
#define SL_ATTN8_CASE(T_, R_) \
  case R_: return launch_attn_decode_split<T_, R_, uint8_t>(q, q_stride, k_cache, v_cache, out, part, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st, cnt, shared_prefix)
  if (kv_format == SL_KV_FP8_E4M3) {
    if (dtype == SL_BF16) {
      switch (rep) { SL_ATTN8_CASE(bf16_t, 1); SL_ATTN8_CASE(bf16_t, 2); SL_ATTN8_CASE(bf16_t, 3); SL_ATTN8_CASE(bf16_t, 4); default: break; }
    } else {
      switch (rep) { SL_ATTN8_CASE(f16_t, 1); SL_ATTN8_CASE(f16_t, 2); SL_ATTN8_CASE(f16_t, 3); SL_ATTN8_CASE(f16_t, 4); default: break; }
    }
    sl_set_error("sl_attn_decode_split: n_heads/n_kv=%d not built (1..4)", rep);
    return SL_ERR_UNSUPPORTED;
  }
#undef SL_ATTN8_CASE
  SL_DISPATCH_DTYPE_INF(dtype, T, {
    switch (rep) {
      case 1: return launch_attn_decode_split<T, 1>(q, q_stride, k_cache, v_cache, out, part, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st, cnt, shared_prefix);
      case 2: return launch_attn_decode_split<T, 2>(q, q_stride, k_cache, v_cache, out, part, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st, cnt, shared_prefix);
      case 3: return launch_attn_decode_split<T, 3>(q, q_stride, k_cache, v_cache, out, part, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st, cnt, shared_prefix);
      case 4: return launch_attn_decode_split<T, 4>(q, q_stride, k_cache, v_cache, out, part, ctx_len, ctx_add, B, n_heads, n_kv, max_ctx, scale, st, cnt, shared_prefix);
      default: sl_set_error("sl_attn_decode_split: n_heads/n_kv=%d not built (1..4)", rep); return SL_ERR_UNSUPPORTED;
    }
  });
}

extern "C" size_t sl_attn_decode_workspace_bytes(int32_t B, int32_t n_heads, int32_t n_kv, int32_t max_ctx) {
  return sl_attn_decode_split_ws(B, n_heads, n_kv, max_ctx);
}

extern "C" int sl_attn_decode_split(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                                    const int32_t* ctx_len, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale,
                                    int32_t dtype, sl_stream stream) {
  return sl_attn_decode_split_impl(q, q_stride, k_cache, v_cache, out, workspace, ctx_len, 0, B, n_heads, n_kv, D, max_ctx, scale, dtype,
                                   (hipStream_t)stream, 2, 0, SL_KV_MODEL_DTYPE);
}

extern "C" int sl_attn_decode_split_ex(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                                       const int32_t* ctx_len, int32_t B, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale,
                                       int32_t dtype, int32_t kv_format, int32_t shared_prefix, sl_stream stream) {
  return sl_attn_decode_split_impl(q, q_stride, k_cache, v_cache, out, workspace, ctx_len, 0, B, n_heads, n_kv, D, max_ctx, scale, dtype,
                                   (hipStream_t)stream, 2, shared_prefix, kv_format);
}

// ----------------------------------------------------------------------------------------------
// Grouped decode attention (speechllm.h sl_attn_decode_grouped): rows that share a prompt read its K / V once.
// Pass 1, attn_decode_prefix_kernel: one block per (group record, kv head).  The single-pass kernel's 16-row MFMA tile carries REP live
// rows there; here tile row t holds head t % REP of the record's sibling t / REP (up to 16 / REP siblings), so the C / D rows
// 4 * (lane >> 4) + reg of every 16-lane group are live, each wave runs the online softmax of four tile rows, and the block walks keys
// [0, prefix_len) of prefix_slot in 128-key chunks — the single-pass kernel's loads, LDS images and MFMA steps.  It leaves the fp32
// record {O[128] (unnormalised), m, l} of every (row, head) in the workspace.
// Pass 2, attn_decode_full_kernel<.., TAIL = true>: one block per (row, kv head) starts from that record and walks the row's own slot from
// prefix_len on.  No merge launch, no atomics; a record with n_rows = 0 exits at once (the grid is B records whatever the plan used).
// ----------------------------------------------------------------------------------------------
template <typename T, int REP, typename KVT = T>
__global__ __launch_bounds__(256) void attn_decode_prefix_kernel(const T* __restrict__ q, int64_t q_stride, const KVT* __restrict__ kc,
                                                                 const KVT* __restrict__ vc, float* __restrict__ rec,
                                                                 const sl_attn_group* __restrict__ groups, int B, int nh, int nkv, int max_ctx,
                                                                 float scale) {
  static_assert(sizeof(T) == 2, "the grouped form is built for the 16-bit types (bf16 / fp16)");
  constexpr int D = 128, KS = 128, NPS = KS / 16, PROW = KS * 2 + 16, NSIB = 16 / REP;
  __shared__ float sc[16][KS];
  __shared__ float alpha[16];
  __shared__ int32_t s_row[16];        // tile row -> batch row (-1: padding)
  __shared__ __attribute__((aligned(16))) unsigned char un[KS * D * 2];   // K tile, then V tile
  __shared__ __attribute__((aligned(16))) unsigned char pt[16 * PROW];
  const int kvh = blockIdx.x;
  const sl_attn_group* g = groups + blockIdx.y;
  const int n_rows = g->n_rows < NSIB ? g->n_rows : NSIB;
  const int n_keys = g->prefix_len < max_ctx ? g->prefix_len : max_ctx;
  if (n_rows <= 0 || n_keys <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, gl = lane & 15;
  const int kg = tid >> 4, dc = tid & 15;
  const int r = lane & 15, q4 = lane >> 4, qq = r >> 2, pp = r & 3;
  using Row = KvRow<T, KVT>;
  const KVT* kbase = kc + ((int64_t)g->prefix_slot * nkv + kvh) * max_ctx * D;
  const KVT* vbase = vc + ((int64_t)g->prefix_slot * nkv + kvh) * max_ctx * D;
  auto voff = [](int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); };
  auto row_of = [&](int t) {      // batch row of tile row t; a row index outside the batch is padding
    if (t >= n_rows * REP) return -1;
    const int b = g->rows[t / REP];
    return (b >= 0 && b < B) ? b : -1;
  };
  if (tid < 16) { s_row[tid] = row_of(tid); alpha[tid] = 1.0f; }
  uint4 qf[4];
  {
    const int b = row_of(r);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
      qf[s4] = b >= 0 ? *(const uint4*)(q + (int64_t)b * q_stride + (int64_t)(kvh * REP + r % REP) * D + 32 * s4 + 8 * q4) : make_uint4(0, 0, 0, 0);
  }
  for (int o = tid; o < 16 * (KS / 8); o += 256)   // P rows of padding tile rows stay zero
    *(uint4*)(pt + (o / (KS / 8)) * PROW + (o % (KS / 8)) * 16) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  typename Row::raw_t kraw[NPS], vraw[NPS];
  f32x4 oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float m_run[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, l_run[4] = {0.f, 0.f, 0.f, 0.f};   // tile rows 4 * wave + i
  const uint32_t ub = (uint32_t)(uintptr_t)(lds_ptr3_t)un;
  const int nchunk = (n_keys + KS - 1) / KS;
  for (int ci = 0; ci < nchunk; ++ci) {
    const int k0 = ci * KS;
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {   // rows past the prefix are clamped (their scores are masked)
      int key = k0 + ps * 16 + wave * 4 + grp; key = key < n_keys ? key : n_keys - 1;
      kraw[ps] = Row::load(kbase + (int64_t)key * D + gl * 8);
    }
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      const int kl = ps * 16 + wave * 4 + grp;
      *(u32x4_t*)(un + kl * 256 + ((gl ^ (kl & 15)) << 4)) = Row::widen(kraw[ps]);
    }
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      int key = k0 + kg + 16 * ps; key = key < n_keys ? key : n_keys - 1;
      vraw[ps] = Row::load(vbase + (int64_t)key * D + dc * 8);
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < KS / 64; ++n) {
      const int rowbase = wave * (KS / 4) + n * 16;
      f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const uint4 kf = *(const uint4*)(un + (rowbase + r) * 256 + (((4 * s4 + q4) ^ r) << 4));
        MMA<T>::step(sacc, qf[s4], kf);
      }
      const int key = rowbase + r;
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[4 * q4 + e][key] = (k0 + key) < n_keys ? sacc[e] * scale : -INFINITY;
    }
    __syncthreads();
    // online softmax: wave w owns tile rows 4 w .. 4 w + 3 (two keys per lane); P rounded to 16 bits as in the single-pass form
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = 4 * wave + i;
      if (t >= n_rows * REP) break;
      const float s0 = sc[t][lane], s1 = sc[t][lane + 64];
      const float m_new = fmaxf(m_run[i], wave_max(fmaxf(s0, s1)));   // finite: key k0 is inside the prefix
      const float p0 = __expf(s0 - m_new), p1 = __expf(s1 - m_new);
      const float a = __expf(m_run[i] - m_new);
      l_run[i] = l_run[i] * a + wave_sum(p0 + p1);
      m_run[i] = m_new;
      *(T*)(pt + t * PROW + lane * 2) = from_f32<T>(p0);
      *(T*)(pt + t * PROW + (lane + 64) * 2) = from_f32<T>(p1);
      if (lane == 0) alpha[t] = a;
    }
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) *(u32x4_t*)(un + voff(kg + 16 * ps, dc)) = Row::widen(vraw[ps]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int df = 2 * wave + j;
#pragma unroll
      for (int e = 0; e < 4; ++e) oacc[j][e] *= alpha[4 * q4 + e];
#pragma unroll
      for (int ks = 0; ks < KS / 32; ++ks) {
        const uint4 pa = *(const uint4*)(pt + r * PROW + (32 * ks + 8 * q4) * 2);
        const int r0 = 32 * ks + 8 * q4 + qq;
        u32x2_t lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(ub + (uint32_t)(voff(r0, 2 * df + (pp >> 1)) + 8 * (pp & 1))) : "memory");
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(ub + (uint32_t)(voff(r0 + 4, 2 * df + (pp >> 1)) + 8 * (pp & 1))) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo), "+v"(hi));
        MMA<T>::step(oacc[j], pa, make_uint4(lo.x, lo.y, hi.x, hi.y));
      }
    }
    __syncthreads();   // un / pt / sc / alpha are rewritten by the next chunk
  }
  // records: (m, l) from the wave that ran the row's softmax, O from every wave's two 16-dim fragments
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = 4 * wave + i, b = s_row[t];
      if (b < 0) continue;
      float* p = rec + ((int64_t)b * nh + kvh * REP + t % REP) * GROUP_REC_FLOATS;
      p[D] = m_run[i]; p[D + 1] = l_run[i];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int t = 4 * q4 + e, b = s_row[t];
    if (b < 0) continue;
    float* p = rec + ((int64_t)b * nh + kvh * REP + t % REP) * GROUP_REC_FLOATS;
#pragma unroll
    for (int j = 0; j < 2; ++j) p[(2 * wave + j) * 16 + r] = oacc[j][e];
  }
}

extern "C" int sl_attn_group_plan_host(const int32_t* prefix_slot, const int32_t* prefix_len, int32_t B, int32_t rep, sl_attn_group* out, int32_t* n_used) {
  SL_CHECK_ARG(prefix_slot && prefix_len && out && n_used, "sl_attn_group_plan_host: null prefix_slot, prefix_len, out or n_used");
  SL_CHECK_ARG(B > 0 && B <= SL_MAX_DECODE_BATCH, "sl_attn_group_plan_host: B %d outside (0, %d]", B, SL_MAX_DECODE_BATCH);
  SL_CHECK_ARG(rep >= 1 && rep <= 16, "sl_attn_group_plan_host: rep %d outside [1, 16]", rep);
  const int per = 16 / rep;
  memset(out, 0, (size_t)B * sizeof(sl_attn_group));
  std::map<std::pair<int32_t, int32_t>, int> open;      // (slot, len) -> its record that still has room
  int used = 0;
  for (int b = 0; b < B; ++b) {
    if (prefix_len[b] <= 0) continue;
    const auto key = std::make_pair(prefix_slot[b], prefix_len[b]);
    auto it = open.find(key);
    if (it == open.end() || out[it->second].n_rows == per) {
      out[used].prefix_slot = key.first; out[used].prefix_len = key.second;
      open[key] = used++;
      it = open.find(key);
    }
    sl_attn_group& g = out[it->second];
    g.rows[g.n_rows++] = b;
  }
  *n_used = used;
  return 0;
}

extern "C" size_t sl_attn_decode_grouped_workspace_bytes(int32_t B, int32_t n_heads) {
  if (B <= 0 || n_heads <= 0) { sl_set_error("sl_attn_decode_grouped_workspace_bytes: B=%d n_heads=%d", B, n_heads); return 0; }
  return ((size_t)B * n_heads * GROUP_REC_FLOATS * sizeof(float) + 255) & ~(size_t)255;
}

// what the grouped kernels are built for (the generation runtime asks before it chooses the path)
bool sl_attn_decode_grouped_built(int n_heads, int n_kv, int D, int dtype, int kv_format) {
  return sl_is16(dtype) && D == 128 && n_kv > 0 && n_heads % n_kv == 0 && n_heads / n_kv >= 1 && n_heads / n_kv <= 4 &&
         (kv_format == SL_KV_MODEL_DTYPE || kv_format == SL_KV_FP8_E4M3);
}

template <typename T, int REP, typename KVT>
static int launch_attn_decode_grouped(const void* q, int64_t q_stride, const void* kc, const void* vc, void* out, float* rec, const int32_t* ctx_len,
                                      int ctx_add, const int32_t* prefix_len, const sl_attn_group* groups, int B, int row_slot0, int nh, int nkv,
                                      int max_ctx, float scale, hipStream_t st) {
  hipLaunchKernelGGL((attn_decode_prefix_kernel<T, REP, KVT>), dim3(nkv, B), dim3(256), 0, st, (const T*)q, q_stride, (const KVT*)kc, (const KVT*)vc, rec,
                     groups, B, nh, nkv, max_ctx, scale);
  SL_CHECK_LAUNCH("attn_decode_prefix");
  const int64_t slot0 = (int64_t)row_slot0 * nkv * max_ctx * 128;      // the rows' own slots start here
  hipLaunchKernelGGL((attn_decode_full_kernel<T, REP, false, 128, KVT, true>), dim3(nkv, B), dim3(256), 0, st, (const T*)q, q_stride,
                     (const KVT*)kc + slot0, (const KVT*)vc + slot0, (T*)out, ctx_len, ctx_add, nh, nkv, max_ctx, scale, 0, rec, prefix_len);
  SL_CHECK_LAUNCH("attn_decode_tail");
  return 0;
}

int sl_attn_decode_grouped_impl(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                                const int32_t* ctx_len, int ctx_add, const int32_t* prefix_len, const sl_attn_group* groups_dev, int32_t B,
                                int32_t row_slot0, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale, int32_t dtype,
                                int32_t kv_format, hipStream_t st) {
  SL_CHECK_ARG(q && k_cache && v_cache && out && workspace && ctx_len && prefix_len && groups_dev, "sl_attn_decode_grouped: null q, k_cache, v_cache, out, workspace, ctx_len, prefix_len or groups_dev");
  SL_CHECK_ARG(B > 0 && B <= SL_MAX_DECODE_BATCH, "sl_attn_decode_grouped: B %d outside (0, %d]", B, SL_MAX_DECODE_BATCH);
  SL_CHECK_ARG(row_slot0 >= 0, "sl_attn_decode_grouped: row_slot0 %d < 0", row_slot0);
  SL_CHECK_ARG(max_ctx > 0, "sl_attn_decode_grouped: max_ctx %d", max_ctx);
  if (dtype == SL_F32) {
    sl_set_error("sl_attn_decode_grouped: dtype float32 not built (bf16 / fp16; the generation runtime copies the prompt rows there)");
    return SL_ERR_UNSUPPORTED;
  }
  SL_CHECK_ARG(sl_is16(dtype), "sl_attn_decode_grouped: unknown dtype %d", dtype);
  SL_TRY(sl_kv_format_check("sl_attn_decode_grouped", kv_format, dtype, D));
  SL_CHECK_ARG(D == 128, "sl_attn_decode_grouped: head_dim D %d not built (128)", D);
  SL_CHECK_ARG(n_kv > 0 && n_heads % n_kv == 0, "sl_attn_decode_grouped: n_heads %% n_kv != 0");
  const int rep = n_heads / n_kv;
  float* rec = (float*)workspace;
#define SL_ATTNG_CASE(T_, KVT_, R_) \
  case R_: return launch_attn_decode_grouped<T_, R_, KVT_>(q, q_stride, k_cache, v_cache, out, rec, ctx_len, ctx_add, prefix_len, groups_dev, B, row_slot0, n_heads, n_kv, max_ctx, scale, st)
#define SL_ATTNG_REPS(T_, KVT_) switch (rep) { SL_ATTNG_CASE(T_, KVT_, 1); SL_ATTNG_CASE(T_, KVT_, 2); SL_ATTNG_CASE(T_, KVT_, 3); SL_ATTNG_CASE(T_, KVT_, 4); default: break; }
  if (kv_format == SL_KV_FP8_E4M3) {
    if (dtype == SL_BF16) SL_ATTNG_REPS(bf16_t, uint8_t) else SL_ATTNG_REPS(f16_t, uint8_t)
  } else {
    if (dtype == SL_BF16) SL_ATTNG_REPS(bf16_t, bf16_t) else SL_ATTNG_REPS(f16_t, f16_t)
  }
#undef SL_ATTNG_REPS
#undef SL_ATTNG_CASE
  sl_set_error("sl_attn_decode_grouped: n_heads/n_kv=%d not built (1..4)", rep);
  return SL_ERR_UNSUPPORTED;
}

extern "C" int sl_attn_decode_grouped(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, void* out, void* workspace,
                                      const int32_t* ctx_len, const int32_t* prefix_len, const sl_attn_group* groups_dev, int32_t B,
                                      int32_t row_slot0, int32_t n_heads, int32_t n_kv, int32_t D, int32_t max_ctx, float scale, int32_t dtype,
                                      int32_t kv_format, sl_stream stream) {
  return sl_attn_decode_grouped_impl(q, q_stride, k_cache, v_cache, out, workspace, ctx_len, 0, prefix_len, groups_dev, B, row_slot0, n_heads, n_kv, D,
                                     max_ctx, scale, dtype, kv_format, (hipStream_t)stream);
}
