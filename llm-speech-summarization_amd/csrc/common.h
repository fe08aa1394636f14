// common.h — shared device/host helpers for libspeechllm (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/speechllm.h"

// ----------------------------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------------------------
void sl_set_error(const char* fmt, ...);

#define SL_CHECK_ARG(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      sl_set_error(__VA_ARGS__);     \
      return SL_ERR_ARG;             \
    }                                \
  } while (0)

#define SL_CHECK_LAUNCH(what)                                                        \
  do {                                                                               \
    hipError_t e__ = hipGetLastError();                                              \
    if (e__ != hipSuccess) {                                                         \
      sl_set_error("%s: %s", what, hipGetErrorString(e__));                          \
      return SL_ERR_LAUNCH;                                                          \
    }                                                                                \
  } while (0)

#define SL_HIP(call)                                                                 \
  do {                                                                               \
    hipError_t e__ = (call);                                                         \
    if (e__ != hipSuccess) {                                                         \
      sl_set_error("%s failed: %s", #call, hipGetErrorString(e__));                  \
      return SL_ERR_LAUNCH;                                                          \
    }                                                                                \
  } while (0)

#define SL_TRY(call)            \
  do {                          \
    int r__ = (call);           \
    if (r__ != 0) return r__;   \
  } while (0)

// ----------------------------------------------------------------------------------------------
// element types.  bf16 is carried as its 16 raw bits; conversion f32->bf16 is a plain cast so hipcc
// emits v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN-preserving: MI355X_MICROARCH "Correctness").
// fp16 (f16_t) likewise: f32->fp16 through v_cvt_pk_f16_f32 (round-to-nearest-even; values beyond 65 504
// become +-inf, as torch's .half() does — no clamping), fp16->f32 through v_cvt_f32_f16 (exact).
// Code that is written once for both 16-bit types tests sizeof(T) == 2 and moves elements through the
// type-generic helpers below (to_f32 / from_f32 / Vec16 / MMA / pack2 / unpack2); kernels built for bf16
// only (the training tapes) say so with a static_assert on sl_is_bf16<T>.
// ----------------------------------------------------------------------------------------------
struct bf16_t {
  uint16_t bits;
};
struct f16_t {
  uint16_t bits;
};
template <typename T> inline constexpr bool sl_is_bf16 = false;
template <> inline constexpr bool sl_is_bf16<bf16_t> = true;
template <typename T> inline constexpr bool sl_is_f16 = false;
template <> inline constexpr bool sl_is_f16<f16_t> = true;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// 16-byte streaming load with the non-temporal hint (weights read once per token: guide nt-weights)
__device__ __forceinline__ uint4 ld_nt16(const void* p) {
#ifdef SL_W_PLAIN      // A/B builds only (tools/ab): default-policy weight loads
  return *(const uint4*)p;
#else
  u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)p);
  return make_uint4(v.x, v.y, v.z, v.w);
#endif
}

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t b) { return __builtin_bit_cast(float, b << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
// one v_cvt_pk_bf16_f32 (converting the halves separately and OR-ing them costs four instructions per pair)
__device__ __forceinline__ uint32_t pack2_bf16(float lo, float hi) {
  const bf16x2_t v = __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t);
  return __builtin_bit_cast(uint32_t, v);
}

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
__device__ __forceinline__ float f16_bits_to_f32(uint32_t b) { return (float)__builtin_bit_cast(_Float16, (uint16_t)b); }
__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) {
  _Float16 h = (_Float16)f;
  return __builtin_bit_cast(uint16_t, h);
}
// one v_cvt_pk_f16_f32
__device__ __forceinline__ uint32_t pack2_f16(float lo, float hi) {
  const f16x2_t v = __builtin_convertvector(f32x2_t{lo, hi}, f16x2_t);
  return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return bf16_bits_to_f32(v.bits); }
__device__ __forceinline__ float to_f32(f16_t v) { return f16_bits_to_f32(v.bits); }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return bf16_t{f32_to_bf16_bits(v)}; }
template <> __device__ __forceinline__ f16_t from_f32<f16_t>(float v) { return f16_t{f32_to_f16_bits(v)}; }

// two 16-bit elements <-> one 32-bit word (element 0 in the low half)
template <typename T> __device__ __forceinline__ uint32_t pack2(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack2<bf16_t>(float lo, float hi) { return pack2_bf16(lo, hi); }
template <> __device__ __forceinline__ uint32_t pack2<f16_t>(float lo, float hi) { return pack2_f16(lo, hi); }
template <typename T> __device__ __forceinline__ f32x2_t unpack2(uint32_t w);
template <> __device__ __forceinline__ f32x2_t unpack2<bf16_t>(uint32_t w) {
  return f32x2_t{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
}
template <> __device__ __forceinline__ f32x2_t unpack2<f16_t>(uint32_t w) {
  return __builtin_convertvector(__builtin_bit_cast(f16x2_t, w), f32x2_t);
}

// 16-byte vector of T: 4 floats or 8 bf16.  VEC = elements per 16 bytes.
template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    f[0] = __builtin_bit_cast(float, u.x); f[1] = __builtin_bit_cast(float, u.y);
    f[2] = __builtin_bit_cast(float, u.z); f[3] = __builtin_bit_cast(float, u.w);
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    return make_uint4(__builtin_bit_cast(uint32_t, f[0]), __builtin_bit_cast(uint32_t, f[1]),
                      __builtin_bit_cast(uint32_t, f[2]), __builtin_bit_cast(uint32_t, f[3]));
  }
};
template <> struct Vec16<bf16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    f[0] = bf16_bits_to_f32(u.x & 0xffffu); f[1] = bf16_bits_to_f32(u.x >> 16);
    f[2] = bf16_bits_to_f32(u.y & 0xffffu); f[3] = bf16_bits_to_f32(u.y >> 16);
    f[4] = bf16_bits_to_f32(u.z & 0xffffu); f[5] = bf16_bits_to_f32(u.z >> 16);
    f[6] = bf16_bits_to_f32(u.w & 0xffffu); f[7] = bf16_bits_to_f32(u.w >> 16);
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    return make_uint4(pack2_bf16(f[0], f[1]), pack2_bf16(f[2], f[3]), pack2_bf16(f[4], f[5]),
                      pack2_bf16(f[6], f[7]));
  }
};
template <> struct Vec16<f16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2_t v = unpack2<f16_t>(w[i]);
      f[2 * i] = v[0]; f[2 * i + 1] = v[1];
    }
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    return make_uint4(pack2_f16(f[0], f[1]), pack2_f16(f[2], f[3]), pack2_f16(f[4], f[5]), pack2_f16(f[6], f[7]));
  }
};

// ----------------------------------------------------------------------------------------------
// fp8 K/V cache rows (SL_KV_FP8_E4M3: OCP e4m3fn, unscaled).
// sl_q8_e4m3: fp32 -> byte.  |x| >= 448 (inf and NaN included) gives the largest finite value, so 0x7F / 0xFF are never
// produced; below that, round to nearest even on the 20 dropped mantissa bits; below 2^-6 the subnormal grid (multiples of
// 2^-9) through one fp32 add, whose own rounding is the tie rule.  Integer and fp32-add arithmetic only: the same bits on the
// host and on the device, whatever the hardware conversion does with saturation and subnormals.  The callers pass a value
// already rounded to the model dtype, so the byte is quantise(what the 16-bit cache would hold).
// ----------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t sl_q8_e4m3(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  const uint32_t sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7fffffffu;
  if (a >= 0x43E00000u) return sign | 0x7Eu;                                   // 448.0f and above
  if (a < 0x3C800000u)                                                          // below 2^-6: ulp(2^14) = 2^-9
    return sign | (__builtin_bit_cast(uint32_t, __builtin_bit_cast(float, a) + 16384.0f) - 0x46800000u);
  a += 0x7FFFFu + ((a >> 20) & 1u);
  return sign | ((a - 0x3C000000u) >> 20);                                      // exponent bias 127 -> 7
}
// 4 / 8 values -> 4 / 8 consecutive bytes
__device__ __forceinline__ uint32_t sl_q8x4(float a, float b, float c, float d) {
  return sl_q8_e4m3(a) | (sl_q8_e4m3(b) << 8) | (sl_q8_e4m3(c) << 16) | (sl_q8_e4m3(d) << 24);
}
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
// 8 e4m3 bytes -> 8 elements of T (every finite e4m3 value is exact in bf16 and in fp16): four v_cvt_scalef32_pk_*_fp8 at scale 1
template <typename T> __device__ __forceinline__ u32x4_t sl_dq8x8(u32x2_t w);
template <> __device__ __forceinline__ u32x4_t sl_dq8x8<bf16_t>(u32x2_t w) {
  return u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.x, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.x, 1.0f, true)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.y, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.y, 1.0f, true))};
}
template <> __device__ __forceinline__ u32x4_t sl_dq8x8<f16_t>(u32x2_t w) {
  return u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.0f, true)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.0f, true))};
}

// ----------------------------------------------------------------------------------------------
// e4m3 weight images (speechllm.h sl_pack_weight_e4m3): the routines the device packer and the host entry both run.
// Values come in as the 16 raw bits of a bf16 / fp16 element; every step is an exact conversion, a comparison or ONE fp32 division,
// so host and device give the same scale and the same bytes.
// ----------------------------------------------------------------------------------------------
__host__ __device__ inline float sl_w8_elem_f32(uint16_t bits, int dtype) {
  if (dtype == SL_BF16) return __builtin_bit_cast(float, (uint32_t)bits << 16);
  return (float)__builtin_bit_cast(_Float16, bits);
}
// max |W[row][k]| over k = k0, k0 + kstride, ... < K (NaN elements are skipped by the comparison)
__host__ __device__ inline float sl_w8_absmax(const uint16_t* row, int K, int dtype, int k0, int kstride) {
  float m = 0.f;
  for (int k = k0; k < K; k += kstride) {
    const float a = __builtin_fabsf(sl_w8_elem_f32(row[k], dtype));
    m = a > m ? a : m;
  }
  return m;
}
__host__ __device__ inline float sl_w8_scale(float amax) { return amax == 0.f ? 1.0f : amax / 448.0f; }
// the 16-byte chunk (fragment f, pair step j, lane) of the image: two runs of 8 bytes, 32 columns apart
__host__ __device__ inline void sl_w8_chunk(const uint16_t* src, int64_t ld, const float* scales, int N, int dtype, int64_t f, int j, int lane, uint32_t out[4]) {
  const int64_t row = f * 16 + (lane & 15);
  out[0] = out[1] = out[2] = out[3] = 0u;
  if (row >= N) return;
  const float s = scales[row];
  const uint16_t* p = src + row * ld + (int64_t)j * 64 + 8 * (lane >> 4);
  for (int h = 0; h < 2; ++h)
    for (int e = 0; e < 8; ++e) out[2 * h + (e >> 2)] |= sl_q8_e4m3(sl_w8_elem_f32(p[32 * h + e], dtype) / s) << (8 * (e & 3));
}

// ----------------------------------------------------------------------------------------------
// MXFP4 weight images (speechllm.h sl_pack_weight_mxfp4): the routines the device packer and the host entry both run.  Integer
// arithmetic on the fp32 bits, one exact multiplication by a power of two and comparisons against exact thresholds: the same bits on
// the host and on the device.  No hardware f32 -> fp4 conversion and no log2f.
// ----------------------------------------------------------------------------------------------
// the block exponent: the smallest e with amax <= 6 * 2^e = 1.5 * 2^(e+2), clamped to [-13, 13]; 0 for an all-zero block.  With
// amax = m * 2^E, 1 <= m < 2 (the fp32 exponent field): e = E - 2 where m <= 1.5, E - 1 above.  inf clamps to 13, fp32 subnormals to -13.
__host__ __device__ inline int sl_w4_exp(float amax) {
  const uint32_t u = __builtin_bit_cast(uint32_t, amax) & 0x7fffffffu;
  if (u == 0u) return 0;
  const int e = (int)(u >> 23) - 127 - 2 + ((u & 0x7fffffu) > 0x400000u ? 1 : 0);
  return e < -13 ? -13 : (e > 13 ? 13 : e);
}
// fp32 -> e2m1 code of x * 2^-e: round to nearest, ties to the even code (.25 -> 0, .75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4,
// 5 -> 4), saturating at 6 (inf included); NaN fails every comparison and becomes 0; the sign is bit 3 and never set on code 0.
__host__ __device__ inline uint32_t sl_q4_e2m1(float x, int e) {
  const float v = x * __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);      // exact (or a flush far below .25, or inf)
  const float a = __builtin_fabsf(v);
  const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) + (uint32_t)(a > 2.5f) +
                     (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return (c != 0u && (__builtin_bit_cast(uint32_t, v) >> 31)) ? (c | 8u) : c;
}
// the scale byte (e + 127) of row `row`, 32-wide block `blk` (NaN elements are skipped by the comparison, as in sl_w8_absmax)
__host__ __device__ inline uint32_t sl_w4_scale_byte(const uint16_t* src, int64_t ld, int N, int dtype, int64_t row, int blk) {
  if (row >= N) return 127u;
  return (uint32_t)(sl_w4_exp(sl_w8_absmax(src + row * ld + (int64_t)blk * 32, 32, dtype, 0, 1)) + 127);
}
// the 16-byte chunk (fragment f, quad step j, lane) of the image; sc4 = the lane's four scale bytes, sc[f][j][lane & 15][0..3], as one dword
__host__ __device__ inline void sl_w4_chunk(const uint16_t* src, int64_t ld, uint32_t sc4, int N, int dtype, int64_t f, int j, int lane, uint32_t out[4]) {
  const int64_t row = f * 16 + (lane & 15);
  out[0] = out[1] = out[2] = out[3] = 0u;
  if (row >= N) return;
  const uint16_t* p = src + row * ld + (int64_t)j * 128 + 8 * (lane >> 4);
  for (int d = 0; d < 4; ++d) {
    const int e = (int)((sc4 >> (8 * d)) & 0xffu) - 127;
    for (int i = 0; i < 8; ++i) out[d] |= sl_q4_e2m1(sl_w8_elem_f32(p[32 * d + i], dtype), e) << (4 * i);
  }
}
// 8 e2m1 nibbles (one dword of the image) -> 8 elements of T, each times the block scale: four v_cvt_scalef32_pk_*_fp4, byte select
// 0..3, every result exact (e2m1 * 2^e is a normal number of both 16-bit types for e in [-13, 13])
template <typename T> __device__ __forceinline__ u32x4_t sl_dq4x8(uint32_t w, float s);
template <> __device__ __forceinline__ u32x4_t sl_dq4x8<bf16_t>(uint32_t w, float s) {
  return u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0)), __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2)), __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3))};
}
template <> __device__ __forceinline__ u32x4_t sl_dq4x8<f16_t>(uint32_t w, float s) {
  return u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 0)), __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 1)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 2)), __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 3))};
}

// ----------------------------------------------------------------------------------------------
// MFMA 16x16 tile step, dtype-generic.  One "k-step" consumes 64 bytes of K per operand row:
//   bf16: 32 k  -> one v_mfma_f32_16x16x32_bf16
//   fp16: 32 k  -> one v_mfma_f32_16x16x32_f16 (same operand / accumulator layout, same cycles)
//   f32 : 16 k  -> four v_mfma_f32_16x16x4_f32 (exact fp32 fma chain)
// Lane l = (r = l & 15, q = l >> 4) supplies, for BOTH operands, the 16 bytes at k-offset q*VEC of
// row r of its operand tile (A: output row, B: output column).  For f32 the four MFMAs take element
// s of each lane's float4, i.e. k = 4q + s: a k-permutation shared by A and B, so the sum is exact.
// Accumulator (C/D) layout: lane (c = l & 15, q = l >> 4) holds D[row 4q + i][col c], i = 0..3.
// ----------------------------------------------------------------------------------------------
template <typename T> struct MMA;
template <> struct MMA<bf16_t> {
  static constexpr int KSTEP = 32;
  static __device__ __forceinline__ void step(f32x4& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                  acc, 0, 0, 0);
  }
};
template <> struct MMA<f16_t> {
  static constexpr int KSTEP = 32;
  static __device__ __forceinline__ void step(f32x4& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
  }
};
template <> struct MMA<float> {
  static constexpr int KSTEP = 16;
  static __device__ __forceinline__ void step(f32x4& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.y), __builtin_bit_cast(float, b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.z), __builtin_bit_cast(float, b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.w), __builtin_bit_cast(float, b.w), acc, 0, 0, 0);
  }
};

// ----------------------------------------------------------------------------------------------
// math
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// GELU for the bf16 instantiations: erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far inside bf16's 4e-3 output
// rounding) — rcp + exp2 + 7 fma instead of libm's branchy erff; erf evaluations were ~11 % of an encoder pass
// (conv stack LayerNorm+GELU, 24 x FFN1).  gelu(x) = x - x*w for x >= 0 and x*w for x < 0, w = 0.5 erfc(|x|/sqrt 2).
__device__ __forceinline__ float gelu_fast(float x) {
  // 20 issue slots per value (two of them quarter rate) instead of 23: 0.5 folded into the polynomial, and the two branches x - x w (x >= 0) /
  // x w (x < 0) written as max(x, 0) - |x| w — one v_max and one v_fma with source modifiers instead of multiply, compare, select, subtract
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, z, 1.0f));
  float pl = __builtin_fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
  pl = __builtin_fmaf(pl, t, 0.5f * 1.421413741f);
  pl = __builtin_fmaf(pl, t, 0.5f * -0.284496736f);
  pl = __builtin_fmaf(pl, t, 0.5f * 0.254829592f);
  const float w = pl * t * __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);     // 0.5 erfc(|x| / sqrt 2)
  return __builtin_fmaf(-fabsf(x), w, fmaxf(x, 0.f));
}
// counter-based dropout mask shared by sl_dropout, the attention kernels and sl_attn_dropout_bwd (train_ops.hip has the story)
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ bool dropout_keep(int64_t i, uint64_t seed, uint32_t thr24) {
  const uint32_t h = lowbias32((uint32_t)i ^ lowbias32((uint32_t)((uint64_t)i >> 32) ^ (uint32_t)seed) ^ (uint32_t)(seed >> 32));
  return (h >> 8) >= thr24;
}
// the same mask in two steps, for loops in which the upper half of the index takes one or two values: inner = drop_inner(hi, seed) once,
// then dropout_keep_lo(lo, inner, thr) per element (a 32-bit integer multiply is a quarter-rate instruction: lowbias32 costs ~56 cycles)
__device__ __forceinline__ uint32_t drop_inner(uint32_t hi, uint64_t seed) { return lowbias32(hi ^ (uint32_t)seed) ^ (uint32_t)(seed >> 32); }
__device__ __forceinline__ bool dropout_keep_lo(uint32_t lo, uint32_t inner, uint32_t thr24) { return (lowbias32(lo ^ inner) >> 8) >= thr24; }
template <typename T> __device__ __forceinline__ float gelu_act(float x) {
  if constexpr (sizeof(T) == 2) return gelu_fast(x);      // bf16 and fp16 (1.5e-7 is also far inside fp16's 4.9e-4 rounding)
  else return gelu_erf(x);
}
__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }
// d gelu(u) / du (exact erf form, hf:activations.py GELUActivation): sl_gelu_bwd and the GEMM epilogue's SL_POST_GELU_BWD
__device__ __forceinline__ float gelu_grad(float u) {
  const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * __expf(-0.5f * u * u);
  return cdf + u * pdf;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One block of THREADS threads over one row of fp32 logits: every element once, in a fixed per-thread order (16-byte loads when the row
// allows them), NaN counted as -inf.  Shared by beam_topk_kernel (beam.hip) and logits_process_kernel (logits_proc.hip): the two form
// the same log-softmax, bit for bit, because they walk the row and reduce through this one piece of code.
template <int THREADS>
struct SlRowScan {
  const float* row;
  int V, tid;
  bool vec;
  __device__ __forceinline__ SlRowScan(const float* r, int v, int t) : row(r), V(v), tid(t), vec((v & 3) == 0 && (((uintptr_t)r) & 15) == 0) {}
  static __device__ __forceinline__ float clean(float x) { return x != x ? -INFINITY : x; }
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
    if (vec) {
      const float4* r4 = (const float4*)row;
      for (int i = tid; i < (V >> 2); i += THREADS) {
        const float4 q = r4[i];
        f(4 * i, clean(q.x)); f(4 * i + 1, clean(q.y)); f(4 * i + 2, clean(q.z)); f(4 * i + 3, clean(q.w));
      }
    } else {
      for (int i = tid; i < V; i += THREADS) f(i, clean(row[i]));
    }
  }
};
// Row maximum m (0 for a row of nothing but -inf / NaN, so that every x - m stays -inf and not NaN) and ls = log(sum exp(x - m)):
// per-thread partials in index order, xor-butterfly inside the wave, the waves combined in order — one fixed order, no atomics.
// redf: THREADS / 64 floats of LDS.  Ends with a barrier: redf may be reused at once.
template <int THREADS>
__device__ __forceinline__ void sl_row_max_lse(const SlRowScan<THREADS>& sc, float* redf, float& m_out, float& ls_out) {
  constexpr int WAVES = THREADS / 64;
  const int lane = sc.tid & 63, wave = sc.tid >> 6;
  float m = -INFINITY;
  sc.each([&](int, float x) { m = fmaxf(m, x); });
  m = wave_max(m);
  if (lane == 0) redf[wave] = m;
  __syncthreads();
  m = redf[0];
  for (int w = 1; w < WAVES; ++w) m = fmaxf(m, redf[w]);
  __syncthreads();
  if (m == -INFINITY) m = 0.f;
  float sum = 0.f;
  sc.each([&](int, float x) { sum += expf(x - m); });
  sum = wave_sum(sum);
  if (lane == 0) redf[wave] = sum;
  __syncthreads();
  sum = 0.f;
  for (int w = 0; w < WAVES; ++w) sum += redf[w];
  __syncthreads();
  m_out = m;
  ls_out = logf(sum);
}

constexpr int SL_MAX_DEVICES = 64;      // per-thread, per-device helper objects (capture streams, side streams) are kept in arrays of this size

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// dtype dispatch on the host.  SL_DISPATCH_DTYPE: fp32 / bf16 (every entry point, the training ones included);
// SL_DISPATCH_DTYPE_INF adds fp16 for the inference entry points only, so that the training kernels are not
// instantiated a third time.
#define SL_DISPATCH_DTYPE_INF(dtype, T, ...)                  \
  do {                                                        \
    if ((dtype) == SL_F32) {                                  \
      using T = float;                                        \
      __VA_ARGS__;                                            \
    } else if ((dtype) == SL_BF16) {                          \
      using T = bf16_t;                                       \
      __VA_ARGS__;                                            \
    } else if ((dtype) == SL_F16) {                           \
      using T = f16_t;                                        \
      __VA_ARGS__;                                            \
    } else {                                                  \
      sl_set_error("unknown dtype %d", (int)(dtype));         \
      return SL_ERR_ARG;                                      \
    }                                                         \
  } while (0)
#define SL_DISPATCH_DTYPE(dtype, T, ...)                      \
  do {                                                        \
    if ((dtype) == SL_F32) {                                  \
      using T = float;                                        \
      __VA_ARGS__;                                            \
    } else if ((dtype) == SL_BF16) {                          \
      using T = bf16_t;                                       \
      __VA_ARGS__;                                            \
    } else {                                                  \
      sl_set_error("unknown dtype %d", (int)(dtype));         \
      return SL_ERR_ARG;                                      \
    }                                                         \
  } while (0)

static inline size_t sl_dtype_size(int dtype) { return dtype == SL_F32 ? 4 : 2; }
// a 16-bit storage type (bf16 or fp16): both run the same kernel families
static inline bool sl_is16(int dtype) { return dtype == SL_BF16 || dtype == SL_F16; }
// K/V cache format of an entry point (speechllm.h SL_KV_*): unknown codes are SL_ERR_ARG; e4m3 rows are built for the 16-bit
// model dtypes and head_dim 128 only (SL_ERR_UNSUPPORTED otherwise).  0 = fine.
static inline int sl_kv_format_check(const char* who, int kv_format, int dtype, int head_dim) {
  if (kv_format != SL_KV_MODEL_DTYPE && kv_format != SL_KV_FP8_E4M3) {
    sl_set_error("%s: unknown K/V cache format %d (0 = model dtype, 1 = fp8 e4m3)", who, kv_format);
    return SL_ERR_ARG;
  }
  if (kv_format == SL_KV_FP8_E4M3 && !sl_is16(dtype)) {
    sl_set_error("%s: the fp8 K/V cache is built for bf16 / fp16 models, not dtype %d (float32 is the parity mode)", who, dtype);
    return SL_ERR_UNSUPPORTED;
  }
  if (kv_format == SL_KV_FP8_E4M3 && head_dim != 128) {
    sl_set_error("%s: the fp8 K/V cache is built for head_dim 128, not %d", who, head_dim);
    return SL_ERR_UNSUPPORTED;
  }
  return 0;
}
// bytes of one K/V element in the cache
static inline size_t sl_kv_elem_size(int kv_format, int dtype) { return kv_format == SL_KV_FP8_E4M3 ? 1 : sl_dtype_size(dtype); }

// ----------------------------------------------------------------------------------------------
// tuning switches: environment variables read ONCE (first use) into this table, never on a dispatch path;
// sl_tuning_reload() (api.hip, exported for tools/tune_*.py) re-reads them for in-process A/B runs
// ----------------------------------------------------------------------------------------------
struct SlEnv {
  int attn_fwd_st;         // SL_ATTN_FWD_ST       (default 1; 2 measured equal, profiles/r06_l_attn_fwd_st_ab.txt) head_dim-64 attention forward: 64-key tiles per staged block
  int conv0_fold;          // SL_CONV0_FOLD        (default 1) conv0 backward of a batch: the block's four waves fold their sums through LDS and flush once, >= 4 strips per wave; 0 = a flush per wave of a 512-block grid (A/B)
  int enc_wt_ahead;        // SL_ENC_WT_AHEAD      (default 1) encoder tape: the layers' transposed weights for the data-gradient products are made in one batched launch on a side stream beside the forward; 0 = a transpose in front of each product
  int glds_ring;           // SL_GLDS_RING         (default 4) bf16 products of <= 256 tiles of 128 x 128 (one block per CU) run the ring form of the 128-tile kernel (gemm128.hip): 4 / 3 = stages of 32 KiB, 104 = four stages without the software-pipelined fragment reads, 0 = the two-stage kernel (A/B)
  int tt_batched;          // SL_TT_BATCHED        (default 1) batched both-transposed products of 64 or 128 k output rows (the positional conv's weight gradient) run on the token-major kernel, batch index on blockIdx.z (0: the register-staged loader — A/B)
  int wgrad_stream_min_tok; // SL_WGRAD_STREAM_MIN_TOK (default 0 = 512; 2 048 until round 6) encoder tape: from this many token rows the parameter-gradient products run on the library's side stream (tuning)
  int attn_bwd_both;       // SL_ATTN_BWD_BOTH     (default 1) attention backward: dK / dV and dQ blocks in ONE launch where neither pass fills the chip (<= 1 024 blocks together: the per-rank KD window); 0 = two launches (A/B, same bits)
  int ring_max_tiles;      // SL_GLDS_RING_MAX_TILES (default 0 = the CU count) most 128 x 128 tiles (x batch) of a product the ring form of the 128-tile kernel takes; above the CU count its blocks run in two rounds (tuning)
  int split_k256;          // SL_SPLIT_K256        (default 1) 256-tile products that fill 50-66 % of one round and hand their K runs to the consumer (deferred_splits) are cut into S uneven runs of whole slabs (gemm.hip splitk256_runs); 0 = off (A/B)
  int ln_colred_inkernel;  // SL_LN_COLRED_INKERNEL (default 0: measured SLOWER, per-rank KD window 30.8 against 29.7 ms — one block pulls every record through one CU behind an atomic round trip; profiles/r06_am_*) 1 = training tapes: the LayerNorm backward's last-arriving block sums the per-block dgamma / dbeta records itself (52 launches fewer per window, same bits)
  int tt_ring;             // SL_TT_RING           (default 1) token-major weight-gradient launches of <= 256 blocks run the ring form of gemm_tiled_tt_kernel (0: the two-stage kernel — A/B)
  int glds_dmab;           // SL_GLDS_DMAB         (default 0: measured equal to -6 % at two blocks per CU, profiles/r06_ah_*) 1 = the two-stage 128-tile kernel issues the next slab's DMA requests between the MFMAs of the current one (0: in a burst at the top of the iteration)
  int splitk_slots;        // SL_SPLITK_SLOTS      (default 0 = rule) block slots the plain split-K rule fills with K runs: 256 = one block per CU (ring form), 512 = two (two-stage kernel)
  int rms_bwd_lean;        // SL_RMSBWD_LEAN       (default 2) RMSNorm backward: x / dy kept as loaded 16-byte vectors (no float copies: ~130 registers instead of 256, 3 waves per SIMD instead of 1); 2 = and four rows per block at every row count, 3 = eight; 0 = the float-copy form
  int decode_prefetch;     // SL_DECODE_PREFETCH   (default 0: measured 2.2 x SLOWER, profiles/r06_j_decode_prefetch_ab.txt) small-batch decode graphs with a weight-prefetch branch two matrices ahead of the chain (runtime.hip DecodePrefetch)
  int attn_bwd_kf;         // SL_ATTN_BWD_KF       (default 0 = by shape) 16-row fragments per wave in the attention-backward kernels: 1 / 2 force a form
  int tape_fuse;           // SL_TAPE_FUSE         (default 1) training tapes: dropout / GELU' / SwiGLU' / bias-gradient passes inside the GEMM and norm-backward kernels (0: the unfused launch sequence, A/B + parity tests)
  int compact_pin;         // SL_COMPACT_PIN       (default 1) a compacting generation keeps the kernel family of its first batch (0: each rung picks its own — A/B only)
  int gen_group_attn;      // SL_GEN_GROUP_ATTN    sl_generate_n with several answers per prompt: 1 = decode attention reads the prompt's K / V once per group of sibling rows (sl_attn_decode_grouped) wherever built, 0 = the prompt rows are copied to every row slot, -1 (default) = by the measured rule (runtime.hip gen_group_attn_rule: 16-bit K / V rows from 256 decode rows up)
  int stream_min_m;        // SL_STREAM_MIN_M      (default 26) packed-weight products with more rows than this take the LDS-staged streaming kernels
  int disable_t256;        // SL_DISABLE_T256
  int t256_min_tiles;      // SL_T256_MIN_TILES    (default 512)
  int t256_min_k;          // SL_T256_MIN_K        (default 1024)
  int t256_by_rounds_pad;  // SL_T256_BY_ROUNDS_PAD 1 (default) = a product chosen for the 256-tile kernel by whole rounds of tiles may pad its rows to 256 freely (634 rows -> 768), 0 = round-4 rule (<= 1/8 more rows than the 128-row padding)
  int t256_phased;         // SL_T256_PHASED       1 (default) = the 256-tile GEMM runs the staggered two-phase main loop, 0 = the round-3 one-barrier-per-slab loop (A/B)
  int disable_glds;        // SL_DISABLE_GLDS      0 / 1 / 2
  int direct_epilogue;     // SL_DIRECT_EPILOGUE
  int gemm_gm;             // SL_GEMM_GM           (default 8)
  int attn_full_min;       // SL_ATTN_FULL_MIN     (default 32)
  int attn_force_split;    // SL_ATTN_FORCE_SPLIT
  int attn_decode_ks;      // SL_ATTN_DECODE_KS    keys per chunk of the single-pass decode attention: 128 (default) or 64 (a block small enough to share a CU with a 256-tile GEMM block of another stream)
  int attn_split_merge;    // SL_ATTN_SPLIT_MERGE    split attention merges its partial records inside the split launch: -1 (default) = where B * n_kv <= 32, 0 = never, 1 = always
  int attn_generic;        // SL_ATTN_GENERIC
  int attn_qt;             // SL_ATTN_QT
  int norm_single_row;     // SL_NORM_SINGLE_ROW
  int no_ln_fold;          // SL_NO_LN_FOLD        1 = the encoder runs its LayerNorm kernels even when folded weights are supplied (A/B)
  int no_wgrad_stream;     // SL_NO_WGRAD_STREAM   1 = the encoder backward keeps its parameter-gradient products on the caller's stream (A/B)
  int gemm_log;            // SL_GEMM_LOG          1 = every sl_gemm* call prints its shape and flags on stderr (`SLGEMM ...`, shape census for tuning) and, on the tiled path, the plan the
                           //                      dispatcher chose (`SLPLAN fam= form= tm= tn= grid= S= krun= close=`: kernel family and form, tiles, grid, K runs and what closes them; gemm.hip plan_tiled);
                           //                      2 = dry run: both lines, then return 0 before any HIP call — nothing is launched, no pointer is dereferenced, the plan assumes 256 CUs (tests/test_gemm_plan_cpu.py)
  int no_swap_epilogue;    // SL_NO_SWAP_EPILOGUE  1 = the 256-tile GEMM keeps the LDS-turned rows epilogue where the swapped-operand form applies (A/B)
  int decode_tiled;        // SL_DECODE_TILED      1 (default) = decode steps above ~900 rows run o and gate/up on the row-major 256-tile kernels, 0 = streaming forms
  int prefill_share_prefix; // SL_PREFILL_SHARE_PREFIX 1 (default) = prefill computes a shared prompt prefix (sl_kv_cache.shared_prefix) once per batch, 0 = per sequence (A/B)
  int prefill_prune_last;  // SL_PREFILL_PRUNE_LAST 1 (default) = prefill's final layer runs o / FFN on each sequence's last row only (the one row lm_head reads), 0 = on every row (A/B, same bits)
  int skinny_alt;          // SL_SKINNY_ALT        1 = o / down at M <= 8 keep the two-steps-in-flight structure of the larger row counts (A/B)
  int tt_max_splits;       // SL_TT_MAX_SPLITS     8 (default): most K runs of a token-major weight-gradient product (tuning)
  int lnbwd_nw;            // SL_LNBWD_NW          16 (default) | 8 | 4: waves per block of the LayerNorm backward for rows <= 1 024 elements (tuning)
  int wgrad_tr;            // SL_WGRAD_TR          1 (default) = weight gradients read dY and X as stored (gemm_tiled_tt_kernel), 0 = through K-contiguous transposed copies (A/B)
  int split_k;             // SL_SPLIT_K           1 (default) = products of few tiles whose caller supplies a workspace (sk_ws) run as S batched K runs + a fixed-order reduce launch, 0 = off (A/B)
  int stream_k;            // SL_STREAM_K          stream-K form of the 256-tile GEMM when a workspace is supplied: 0 = never, 1 = by rule (default), 2 = whenever the form allows
  int gemm_ko;             // SL_GEMM_KO           debug builds (-DSL_GEMM_DEBUG): knock-out bits of the phased 256-tile GEMM (1 reads, 2 DMA, 4 MFMAs)
  unsigned long long gemm_stamp_ptr;   // SL_GEMM_STAMP_PTR  device address (hex) of a uint32 buffer: the phased 256-tile GEMM launches its instrumented build and
                                       // leaves in-kernel cycle stamps there (tools/gemm_stamps.py); 0 = off
  int stream_splits, stream_nwv, stream_mt;   // SL_STREAM_CFG "splits,nwv[,mt]" (0 = not set)
  int stream_wide;         // SL_STREAM_WIDE       0 = never use the 256 x 128 streaming block, 1 = default rule, 2 = whenever it applies
  int stream_wsplits;      // SL_STREAM_WSPLITS    K splits of the 256 x 128 form when its blocks do not cover the CUs (0 = rule)
  int stream_fixup;        // SL_STREAM_FIXUP      1 = K splits of the 256 x 128 form are closed inside the kernel (default 0: reduce launch, faster)
  int stream_nl;           // SL_STREAM_NL         loader waves of the 128-row streaming GEMM blocks (0 = default)
};
const SlEnv& sl_env();

// Kernel-family pin (api.hip).  Every choice of the decode step that depends on the row count — skinny / streaming / tiled GEMM form,
// K-split counts, the RMSNorm-scale chain, single-pass or split attention, fused lm_head top-1 — is made on sl_family_rows(M) =
// max(M, pinned rows of the calling thread).  A compacting generation pins the rows of the batch it STARTED with (sl_generate): the
// live rows shrink, the arithmetic each row goes through does not change, so a sequence's bf16 ids cannot depend on when its
// neighbours finish (tests/test_fullsize_gpu.py::test_configs1_compacted_batch_ids_equal_uncompacted_at_bench_stop_mix).
// train_ops.hip: y (cols, ld_out) = x (rows, cols)^T for a list of matrices in one launch per SL_TRANSPOSE_BATCH records (sl_transpose_pad's
// argument rules per record; tiles_r is filled by the launcher)
#define SL_TRANSPOSE_BATCH 64
struct SlTransposeRec {
  const void* x; void* y;
  int64_t ldx, ldy;
  int32_t rows, cols, ld_out, tiles_r;
};
struct SlTransposeBatch {
  SlTransposeRec rec[SL_TRANSPOSE_BATCH];
  int32_t first_block[SL_TRANSPOSE_BATCH];
  int32_t n, pad;
};
int sl_transpose_pad_batch_impl(const SlTransposeRec* recs, int n, int32_t dtype, sl_stream stream);
int sl_family_rows(int rows);
int sl_family_pin(int rows);      // returns the previous pin (0 = none)
struct SlFamilyPin {
  int prev;
  explicit SlFamilyPin(int rows) : prev(sl_family_pin(rows)) {}
  ~SlFamilyPin() { sl_family_pin(prev); }
};

// Per-row generation state a select pass reads and advances (select.hip), all device arrays of B rows unless noted: the one argument
// of the three selects below, which the extern "C" entries and the generation loop (runtime.hip) fill.
struct SlRowState {
  int32_t *unfinished, *ctx_len, *gen_count, *finish_len, *next_ids;
  int32_t* out_ids;               // (B, max_new)
  int32_t max_new;
  const int32_t* row_limit;       // per-row token budgets, NULL = none
  float* logprob_out;             // (B, max_new) token log-probabilities, NULL = off
  const int32_t* eos_ids;         // HOST, n_eos <= 8 ids
  int32_t n_eos, pad_id, use_eos, advance_ctx;
};
int sl_greedy_select_impl(const float* logits, int32_t B, int32_t V, const SlRowState& rs, hipStream_t st);
// amax_sum (the third plane) and rs.logprob_out come together
int sl_greedy_select_partial_impl(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int32_t n_groups, int32_t B, const SlRowState& rs,
                                  hipStream_t st);
int sl_sample_select_impl(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t* choice_ws,
                          const int32_t* row_ids, const SlRowState& rs, hipStream_t st, const sl_warp_opts* warp = nullptr);
// the ranges of speechllm.h's sl_warp_opts (NULL passes); refused values land in sl_last_error
int sl_warp_opts_check(const char* who, const sl_warp_opts* w);
bool sl_warp_opts_on(const sl_warp_opts* w);      // some option is on (NULL: none)
