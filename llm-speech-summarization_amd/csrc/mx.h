// mx.h — the OCP MX formats of the block-scaled linears (speechllm.h "MX weight image", "MXFP8 activation rows"): the routines the
// device kernels and the host entries both run.  As in common.h's e4m3 / MXFP4 routines, every step is an exact conversion, a
// comparison, integer arithmetic on the fp32 bits or ONE exact multiplication by a power of two, so host and device give the same
// bytes.  No hardware f32 -> fp8 / fp4 conversion (v_cvt_scalef32_pk_fp8_*) is used: its treatment of saturation and of non-finite
// inputs would have to be selected around, and the quantise launch is bound by its loads, not by these few VALU operations.
#pragma once
#include "common.h"

// ----------------------------------------------------------------------------------------------
// MX weight image: values and scale bytes are those of the MXFP4 weight image (sl_w4_scale_byte, sl_q4_e2m1); only the place differs.
// Lane `lane` of fragment f, slab j owns ONE 32-element block — row 16 f + (lane & 15), columns 128 j + 32 (lane >> 4) + [0, 32) —
// as 16 bytes (element 2b in the low nibble of byte b), and that block's scale byte.
// ----------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t sl_mx_chunk(const uint16_t* src, int64_t ld, int N, int dtype, int64_t f, int j, int lane, uint32_t out[4]) {
  const int64_t row = f * 16 + (lane & 15);
  const int blk = 4 * j + (lane >> 4);
  out[0] = out[1] = out[2] = out[3] = 0u;
  const uint32_t sb = sl_w4_scale_byte(src, ld, N, dtype, row, blk);
  if (row >= N) return sb;
  const int e = (int)sb - 127;
  const uint16_t* p = src + row * ld + (int64_t)blk * 32;
  for (int d = 0; d < 4; ++d)
    for (int i = 0; i < 8; ++i) out[d] |= sl_q4_e2m1(sl_w8_elem_f32(p[8 * d + i], dtype), e) << (4 * i);
  return sb;
}

// ----------------------------------------------------------------------------------------------
// MXFP8 activation rows.  The block exponent: the smallest e with amax <= 448 * 2^e = 1.75 * 2^(e + 8), clamped to [-127, 127]; 0 for a
// block without a nonzero finite element.  With amax = m * 2^E, 1 <= m < 2 (the fp32 exponent field): e = E - 8 where m <= 1.75, E - 7
// above.  An fp32 subnormal amax (a bf16 subnormal) has field 0: E = -127, clamped to -127 like its true exponent would be.
// ----------------------------------------------------------------------------------------------
__host__ __device__ inline int sl_mx8_exp(float amax) {
  const uint32_t u = __builtin_bit_cast(uint32_t, amax) & 0x7fffffffu;
  if (u == 0u) return 0;
  const int e = (int)(u >> 23) - 127 - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// max |x| over the FINITE elements of one 32-element block (inf and NaN are skipped: an inf saturates whatever the scale)
__host__ __device__ inline float sl_mx8_absmax32(const uint16_t* blk, int dtype) {
  float m = 0.f;
  for (int k = 0; k < 32; ++k) {
    const float a = __builtin_fabsf(sl_w8_elem_f32(blk[k], dtype));
    m = (a < __builtin_inff() && a > m) ? a : m;
  }
  return m;
}
// one element: x / 2^e -> e4m3 byte.  NaN -> 0x7F; +-inf -> +-448 (0x7E / 0xFE) through sl_q8_e4m3's saturation; otherwise round to
// nearest even, subnormals included.  127 - e lies in [7, 254] for every e a 16-bit input can produce (e <= 120), so 2^-e is a normal
// fp32 number and the multiplication is exact unless the result is an fp32 subnormal — far below half the smallest e4m3 step, zero
// either way.
__host__ __device__ inline uint32_t sl_mx8_elem(float x, int e) {
  if (x != x) return 0x7Fu;
  return sl_q8_e4m3(x * __builtin_bit_cast(float, (uint32_t)(127 - e) << 23));
}
// one block: 32 elements -> 8 dwords of bytes; returns the scale byte
__host__ __device__ inline uint32_t sl_mx8_block(const uint16_t* blk, int dtype, uint32_t out[8]) {
  const int e = sl_mx8_exp(sl_mx8_absmax32(blk, dtype));
  for (int d = 0; d < 8; ++d) {
    uint32_t w = 0u;
    for (int i = 0; i < 4; ++i) w |= sl_mx8_elem(sl_w8_elem_f32(blk[4 * d + i], dtype), e) << (8 * i);
    out[d] = w;
  }
  return (uint32_t)(e + 127);
}
