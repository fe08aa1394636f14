// gemm_mx.hip — the block-scaled product of the opt-in MX linears: C = act(dq(Aq) . dq(Wimg)^T) + residual with
// MXFP8 (e4m3 + e8m0 per 32 k) activation rows and an MX weight image (e2m1 + e8m0 per 32 k), on v_mfma_scale_f32_16x16x128_f8f6f4;
// and the two launches that produce its operands (sl_mxfp8_quantize_rows, sl_pack_weight_mx) with their host definitions.
//
// Operand map of the scaled MFMA, as the chip has it (pinned by tests/test_mx_gpu.py::test_operand_map_probe; the first form of this
// kernel assumed 32 consecutive k per lane for BOTH operands and the probe refuted it for the 8-bit one).  Lane l = (r = l & 15,
// q = l >> 4) supplies row (A) / column (B) r.
//   e2m1 (16 bytes, the low 4 operand VGPRs): the 32 consecutive k [32 q, 32 q + 32), element 2b in the low nibble of byte b.
//   e4m3 (32 bytes, 8 VGPRs): TWO runs of 16 — VGPRs 0-3 hold k [16 q, 16 q + 16), VGPRs 4-7 hold k [64 + 16 q, 64 + 16 q + 16).
//   scales: ONE e8m0 byte per operand and lane (byte 0 of the scale VGPR with op_sel 0); the byte of lane (r, q) applies to row /
//   column r and the k block [32 q, 32 q + 32) — one MX block — WHICHEVER lanes hold that block's elements.  For e2m1 that is the
//   lane's own data; for e4m3 block q sits in VGPRs 0-3 (q < 2) or 4-7 (q >= 2) of lanes (r, 2 (q & 1)) and (r, 2 (q & 1) + 1).
//   The accumulator is the usual 16x16 one: lane (c = r, q) holds D[4q + i][c].
//
// One tile structure: 128 x 128 outputs per block, 2 x 2 waves of 64 x 64, BK = 128 = one MFMA deep.  A slab is 16 KiB of A bytes and
// 8 KiB of W nibbles (the bf16 128^2 tile moves 32 KiB for a quarter of the K), brought in by 16-byte LDS-DMA pieces into two stages.
// The LDS image is lane-linear per wave (the DMA's only form), so the order is made on the SOURCE address: piece (fragment, half,
// lane) of A is read from row 16 fragment + (lane & 15), byte 16 (lane >> 4) + 64 half of the slab — the weight image already IS that
// order — and a fragment read is ds_read_b128 at lane * 16: no bank conflict, no swizzle arithmetic.  The scale bytes (under 1 KiB per
// slab) go from global memory to registers, one slab ahead.
// No K split and no cross-block hand-off: an output row's sum is the chain slab 0, 1, ... of one accumulator whatever M is, so a row
// has the same bits alone and inside a batch (test_row_independence).
#include "common.h"
#include "gemm_internal.h"
#include "gemm_epilogue.h"
#include "mx.h"

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

struct MxP {
  const uint8_t* Aq; int64_t lda;      // (M, K) e4m3 bytes, row stride lda
  const uint8_t* As;                   // (M, K/32) e8m0 bytes
  const uint8_t* W;                    // MX weight image: elements
  const uint8_t* Ws;                   // ... its scales
  void* C; int64_t ldc;
  const void* res; int64_t ldr;
  int M, N, Np, K, out_f32, tiles_m, tiles_n;
};

constexpr int MX_BM = 128, MX_BN = 128, MX_A_BYTES = 16384, MX_STAGE = 24576;

template <typename T, int ACT>
__global__ __launch_bounds__(256, 2) void gemm_mx_kernel(MxP p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][MX_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, q = lane >> 4;
  int bm, bn;
  tile_patch_coords(xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n), p.tiles_m, p.tiles_n, 8, bm, bn);
  const int nk = p.K >> 7, nfrag = p.Np >> 4, nsb = p.K >> 5;

  // DMA piece idx = 4 i + wave: A piece (fragment idx >> 1, half idx & 1), W fragment idx.  Rows / fragments past the end are clamped
  // to the last one: what they produce lands in outputs no epilogue stores.
  const uint8_t* ga[4];
  const uint8_t* gw[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = 4 * i + wave;
    int row = bm * MX_BM + (idx >> 1) * 16 + r;
    row = row < p.M ? row : p.M - 1;
    ga[i] = p.Aq + (int64_t)row * p.lda + 16 * q + 64 * (idx & 1);      // k [16 q, +16) for VGPRs 0-3, [64 + 16 q, +16) for VGPRs 4-7
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int f = bn * 8 + 4 * i + wave;
    f = f < nfrag ? f : nfrag - 1;
    gw[i] = p.W + ((int64_t)f * nk * 64 + lane) * 16;
  }
  // the lane's scale bytes: A fragment m -> row of that fragment, block 4 kt + q; W fragment n -> byte `lane` of (fragment, slab)
  const uint8_t* gsa[4];
  const uint8_t* gsw[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    int row = bm * MX_BM + (wm * 4 + m) * 16 + r;
    row = row < p.M ? row : p.M - 1;
    gsa[m] = p.As + (int64_t)row * nsb + q;
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    int f = bn * 8 + wn * 4 + n;
    f = f < nfrag ? f : nfrag - 1;
    gsw[n] = p.Ws + (int64_t)f * nk * 64 + lane;
  }
  const int wave_lds = __builtin_amdgcn_readfirstlane(wave) * 1024;

  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) __builtin_amdgcn_global_load_lds((glb_ptr_t)(ga[i] + (int64_t)kt * 128), (lds_ptr_t)(&smem[buf][i * 4096 + wave_lds]), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(gw[i] + (int64_t)kt * 1024), (lds_ptr_t)(&smem[buf][MX_A_BYTES + i * 4096 + wave_lds]), 16, 0, 0);
  };
  int sa_n[4], sw_n[4];
  auto scales = [&](int kt) {
#pragma unroll
    for (int m = 0; m < 4; ++m) sa_n[m] = gsa[m][4 * kt];
#pragma unroll
    for (int n = 0; n < 4; ++n) sw_n[n] = gsw[n][(int64_t)kt * 64];
  };

  issue(0, 0);
  scales(0);
  const uint32_t sb0 = (uint32_t)(uintptr_t)(lds_ptr_t)(&smem[0][0]);
  const uint32_t ra0 = sb0 + (uint32_t)(wm * 8192 + lane * 16), rb0 = sb0 + (uint32_t)(MX_A_BYTES + wn * 4096 + lane * 16);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    // behind the wait + barrier: slab kt is in LDS, and every wave has retired its fragment reads of slab kt - 1, whose stage the DMA
    // of slab kt + 1 (requested next, running under this slab's MFMAs) overwrites
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int sa[4], sw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { sa[i] = sa_n[i]; sw[i] = sw_n[i]; }
    if (kt + 1 < nk) { issue(kt + 1, buf ^ 1); scales(kt + 1); }
    const uint32_t ra = ra0 + (uint32_t)(buf * MX_STAGE), rb = rb0 + (uint32_t)(buf * MX_STAGE);
    u32x4_t a0[4], a1[4], b[4];
    SL_LDS_RD(a0[0], ra, 0);    SL_LDS_RD(a1[0], ra, 1024);
    SL_LDS_RD(b[0], rb, 0);     SL_LDS_RD(b[1], rb, 1024); SL_LDS_RD(b[2], rb, 2048); SL_LDS_RD(b[3], rb, 3072);
    SL_LDS_RD(a0[1], ra, 2048); SL_LDS_RD(a1[1], ra, 3072);
    SL_LDS_RD(a0[2], ra, 4096); SL_LDS_RD(a1[2], ra, 5120);
    SL_LDS_RD(a0[3], ra, 6144); SL_LDS_RD(a1[3], ra, 7168);
    lds_wait8<0>(a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]);
    asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));      // the wait above covers them; volatile keeps this behind it, the uses behind this
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const i32x8_t av = {(int)a0[m].x, (int)a0[m].y, (int)a0[m].z, (int)a0[m].w, (int)a1[m].x, (int)a1[m].y, (int)a1[m].z, (int)a1[m].w};
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const i32x8_t bv = {(int)b[n].x, (int)b[n].y, (int)b[n].z, (int)b[n].w, 0, 0, 0, 0};
        // A: e4m3 (cbsz 0), B: e2m1 (blgp 4); each operand's scale is byte 0 of its scale register
        acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc[m][n], 0, 4, 0, sa[m], 0, sw[n]);
      }
    }
  }

  // direct epilogue: lane (r, q) holds rows 4q .. 4q + 3 of column r of each 16 x 16 fragment
  const int row0 = bm * MX_BM + wm * 64 + 4 * q;
  const int colb = bn * MX_BN + wn * 64;
  auto put = [&](int row, int col, float v) {
    if (p.res) v += to_f32(((const T*)p.res)[(int64_t)row * p.ldr + col]);
    if (p.out_f32) ((float*)p.C)[(int64_t)row * p.ldc + col] = v;
    else ((T*)p.C)[(int64_t)row * p.ldc + col] = from_f32<T>(v);
  };
  if constexpr (ACT == SL_ACT_SILU_MUL) {
    const int nout = p.N >> 1;      // fragments 2 pr / 2 pr + 1 are 16 gate rows and their 16 up rows: one lane holds both values of an output
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int ocol = (colb >> 1) + pr * 16 + r;
      if (ocol >= nout) continue;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + m * 16 + i;
          if (row < p.M) put(row, ocol, silu(acc[m][2 * pr][i]) * acc[m][2 * pr + 1][i]);
        }
    }
  } else {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = colb + n * 16 + r;
      if (col >= p.N) continue;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + m * 16 + i;
          if (row < p.M) put(row, col, acc[m][n][i]);
        }
    }
  }
}

static int mx16_check(const char* who, const char* what, int32_t dtype) {
  if (dtype == SL_F32) {
    sl_set_error("%s: %s are built for bf16 / fp16 models, not float32 (the parity mode)", who, what);
    return SL_ERR_UNSUPPORTED;
  }
  SL_CHECK_ARG(sl_is16(dtype), "%s: unknown dtype %d", who, dtype);
  return 0;
}

int sl_gemm_mx_impl(const sl_gemm_mx_args* a, hipStream_t st) {
  SL_CHECK_ARG(a && a->Aq && a->a_scales && a->W && a->C, "sl_gemm_mx: null argument");
  SL_TRY(mx16_check("sl_gemm_mx", "MX products", a->dtype));
  SL_CHECK_ARG(a->M >= 1 && a->N >= 1 && a->K >= 128 && a->K % 128 == 0, "sl_gemm_mx: M=%d N=%d K=%d (K must be a positive multiple of 128)", a->M, a->N, a->K);
  SL_CHECK_ARG(a->act == SL_ACT_NONE || a->act == SL_ACT_SILU_MUL, "sl_gemm_mx: act %d not built (SL_ACT_NONE, SL_ACT_SILU_MUL)", a->act);
  SL_CHECK_ARG(a->act != SL_ACT_SILU_MUL || a->N % 32 == 0, "sl_gemm_mx: SL_ACT_SILU_MUL needs N=%d to be a multiple of 32 (16 gate rows + 16 up rows)", a->N);
  SL_CHECK_ARG(a->lda >= a->K && a->lda % 16 == 0 && ((uintptr_t)a->Aq & 15) == 0 && ((uintptr_t)a->W & 15) == 0,
               "sl_gemm_mx: Aq and W must be 16-byte aligned, lda=%lld a multiple of 16 and >= K", (long long)a->lda);
  const int nout = a->act == SL_ACT_SILU_MUL ? a->N / 2 : a->N;
  SL_CHECK_ARG(a->ldc >= nout && (!a->residual || a->ldr >= nout), "sl_gemm_mx: ldc / ldr below the %d output columns", nout);
  MxP p;
  p.Aq = (const uint8_t*)a->Aq; p.lda = a->lda; p.As = (const uint8_t*)a->a_scales;
  p.M = a->M; p.N = a->N; p.K = a->K; p.Np = (a->N + 15) / 16 * 16;
  p.W = (const uint8_t*)a->W; p.Ws = p.W + (int64_t)p.Np * a->K / 2;
  p.C = a->C; p.ldc = a->ldc; p.res = a->residual; p.ldr = a->ldr; p.out_f32 = a->out_f32;
  p.tiles_m = (a->M + MX_BM - 1) / MX_BM; p.tiles_n = (a->N + MX_BN - 1) / MX_BN;
  const dim3 grid((unsigned)(p.tiles_m * p.tiles_n));
  if (a->dtype == SL_BF16) {
    if (a->act == SL_ACT_SILU_MUL) hipLaunchKernelGGL((gemm_mx_kernel<bf16_t, SL_ACT_SILU_MUL>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_mx_kernel<bf16_t, SL_ACT_NONE>), grid, dim3(256), 0, st, p);
  } else {
    if (a->act == SL_ACT_SILU_MUL) hipLaunchKernelGGL((gemm_mx_kernel<f16_t, SL_ACT_SILU_MUL>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_mx_kernel<f16_t, SL_ACT_NONE>), grid, dim3(256), 0, st, p);
  }
  SL_CHECK_LAUNCH("gemm_mx");
  return 0;
}
extern "C" int sl_gemm_mx(const sl_gemm_mx_args* a, sl_stream stream) { return sl_gemm_mx_impl(a, (hipStream_t)stream); }

// ----------------------------------------------------------------------------------------------
// MXFP8 activation rows: one thread per 32-element block (64 bytes in, 32 bytes + 1 scale byte out)
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mx8_quant_kernel(const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ qo, uint8_t* __restrict__ sc, int64_t M, int K,
                                                        int dtype, int vec) {
  const int nb = K >> 5;
  const int64_t total = M * nb;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / nb;
    const int b = (int)(i - row * nb);
    const uint16_t* src = x + row * ldx + (int64_t)b * 32;
    uint16_t e[32];
    if (vec) {      // 16-byte aligned rows: four 16-byte loads
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint4 u = ((const uint4*)src)[v];
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { e[8 * v + 2 * j] = (uint16_t)(w[j] & 0xffffu); e[8 * v + 2 * j + 1] = (uint16_t)(w[j] >> 16); }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 32; ++k) e[k] = src[k];
    }
    uint32_t o[8];
    const uint32_t sbyte = sl_mx8_block(e, dtype, o);
    uint4* dst = (uint4*)(qo + row * K + (int64_t)b * 32);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    sc[i] = (uint8_t)sbyte;
  }
}

static int mx8_quant_check(const char* who, const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype) {
  SL_CHECK_ARG(x && q && scales && M >= 1 && K > 0, "%s: bad arguments", who);
  SL_TRY(mx16_check(who, "MXFP8 activation rows", dtype));
  SL_CHECK_ARG(K % 32 == 0, "%s: K=%d must be a multiple of 32 (one scale per 32 elements)", who, K);
  SL_CHECK_ARG(ldx >= K, "%s: ldx=%lld < K=%d", who, (long long)ldx, K);
  SL_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 1) == 0, "%s: q must be 16-byte aligned", who);
  return 0;
}

int sl_mxfp8_quantize_rows_impl(const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype, hipStream_t st) {
  SL_TRY(mx8_quant_check("sl_mxfp8_quantize_rows", x, ldx, q, scales, M, K, dtype));
  const int64_t total = M * (K / 32);
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 65536 ? ceil_div64(total, 256) : 65536);
  const int vec = (((uintptr_t)x & 15) == 0 && ldx % 8 == 0) ? 1 : 0;
  hipLaunchKernelGGL(mx8_quant_kernel, dim3(grid), dim3(256), 0, st, (const uint16_t*)x, ldx, (uint8_t*)q, (uint8_t*)scales, M, K, dtype, vec);
  SL_CHECK_LAUNCH("mxfp8_quantize_rows");
  return 0;
}
extern "C" int sl_mxfp8_quantize_rows(const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype, sl_stream stream) {
  return sl_mxfp8_quantize_rows_impl(x, ldx, q, scales, M, K, dtype, (hipStream_t)stream);
}

extern "C" int sl_mxfp8_quantize_rows_host(const void* x, int64_t ldx, void* q, void* scales, int64_t M, int32_t K, int32_t dtype) {
  SL_TRY(mx8_quant_check("sl_mxfp8_quantize_rows_host", x, ldx, q, scales, M, K, dtype));
  const int nb = K / 32;
  for (int64_t row = 0; row < M; ++row)
    for (int b = 0; b < nb; ++b) {
      uint32_t o[8];
      ((uint8_t*)scales)[row * nb + b] = (uint8_t)sl_mx8_block((const uint16_t*)x + row * ldx + (int64_t)b * 32, dtype, o);
      memcpy((uint8_t*)q + row * K + (int64_t)b * 32, o, 32);
    }
  return 0;
}

// ----------------------------------------------------------------------------------------------
// MX weight images (speechllm.h sl_pack_weight_mx): one thread per (fragment, slab, lane) = one 32-element block: its scale byte and its
// 16 bytes of nibbles, both by common.h's MXFP4 routines
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mx_pack_kernel(const uint16_t* __restrict__ src, int64_t ld, uint4* __restrict__ dst, uint8_t* __restrict__ sc, int N, int Np, int K,
                                                      int dtype) {
  const int nk = K / 128;
  const int64_t total = (int64_t)(Np / 16) * nk * 64;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t fj = i >> 6;
    uint32_t o[4];
    sc[i] = (uint8_t)sl_mx_chunk(src, ld, N, dtype, fj / nk, (int)(fj % nk), (int)(i & 63), o);
    dst[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

static int mx_pack_check(const char* who, const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype) {
  SL_CHECK_ARG(src && dst && N > 0 && K > 0, "%s: bad arguments", who);
  SL_TRY(mx16_check(who, "MX weight images", dtype));
  SL_CHECK_ARG(K % 128 == 0, "%s: K=%d must be a multiple of 128 (one scaled MFMA is 128 deep)", who, K);
  SL_CHECK_ARG(ld_src >= K, "%s: ld_src=%lld < K=%d", who, (long long)ld_src, K);
  SL_CHECK_ARG(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 1) == 0, "%s: dst must be 16-byte aligned", who);
  return 0;
}

extern "C" size_t sl_mx_weight_image_bytes(int32_t N, int32_t K) {
  if (N <= 0 || K <= 0 || K % 128 != 0) { sl_set_error("sl_mx_weight_image_bytes: N=%d K=%d (K must be a positive multiple of 128)", N, K); return 0; }
  const size_t Np = ((size_t)N + 15) / 16 * 16;
  return Np * (size_t)K / 2 + Np * (size_t)K / 32;
}

extern "C" int sl_pack_weight_mx_host(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype) {
  SL_TRY(mx_pack_check("sl_pack_weight_mx_host", src, ld_src, dst, N, K, dtype));
  const int64_t Np = ((int64_t)N + 15) / 16 * 16;
  const int nk = K / 128;
  uint8_t* sc = (uint8_t*)dst + Np * K / 2;
  for (int64_t f = 0; f < Np / 16; ++f)
    for (int j = 0; j < nk; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        uint32_t o[4];
        const int64_t i = (f * nk + j) * 64 + lane;
        sc[i] = (uint8_t)sl_mx_chunk((const uint16_t*)src, ld_src, N, dtype, f, j, lane, o);
        memcpy((uint8_t*)dst + i * 16, o, 16);
      }
  return 0;
}

extern "C" int sl_pack_weight_mx(const void* src, int64_t ld_src, void* dst, int32_t N, int32_t K, int32_t dtype, sl_stream stream) {
  SL_TRY(mx_pack_check("sl_pack_weight_mx", src, ld_src, dst, N, K, dtype));
  const int Np = (N + 15) / 16 * 16;
  const int64_t total = (int64_t)(Np / 16) * (K / 128) * 64;
  const unsigned grid = (unsigned)(ceil_div64(total, 256) < 16384 ? ceil_div64(total, 256) : 16384);
  hipLaunchKernelGGL(mx_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, ld_src, (uint4*)dst, (uint8_t*)dst + (int64_t)Np * K / 2, N, Np, K, dtype);
  SL_CHECK_LAUNCH("pack_weight_mx");
  return 0;
}
