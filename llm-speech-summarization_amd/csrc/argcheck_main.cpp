// argcheck_main.cpp — sanitizer driver for the HOST side of libspeechllm (the reference has no sanitizer runs).
// Built by `make asan` against a host-ASan + UBSan build of the library (device code is not instrumented: GPU ASan needs
// xnack+, which this pool does not offer) and run on a machine WITHOUT a GPU: every call below must be rejected or answered by
// host code alone — argument validation, shape / workspace arithmetic, the tuning-switch parser — before any HIP call, with
// the right status and a non-empty error string, and without the sanitizers reporting anything.
#include <initializer_list>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/speechllm.h"

static int g_fail = 0;
#define EXPECT(cond, what)                                                         \
  do {                                                                             \
    if (!(cond)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, what); ++g_fail; } \
  } while (0)
#define EXPECT_ARG_ERROR(call)                                                      \
  do {                                                                              \
    const int rc__ = (call);                                                        \
    EXPECT(rc__ == SL_ERR_ARG || rc__ == SL_ERR_UNSUPPORTED, #call " must be rejected"); \
    EXPECT(sl_last_error()[0] != 0, #call " must leave an error message");         \
  } while (0)

// ... and the message names the reason: a case refused by an EARLIER check would pass EXPECT_ARG_ERROR all the same
#define EXPECT_ARG_ERROR_SAYS(call, needle)                                         \
  do {                                                                              \
    EXPECT_ARG_ERROR(call);                                                         \
    EXPECT(strstr(sl_last_error(), needle) != nullptr, #call " must name " needle); \
  } while (0)

static void fill_hubert(sl_hubert_model* m, sl_hubert_layer* layers, int n_layers) {
  memset(m, 0, sizeof(*m));
  m->dtype = SL_BF16; m->n_conv = 7; m->hidden = 1024; m->n_layers = n_layers; m->n_heads = 16; m->ffn = 4096; m->pos_k = 128; m->pos_groups = 16;
  const int k[7] = {10, 3, 3, 3, 3, 2, 2}, s[7] = {5, 2, 2, 2, 2, 2, 2};
  for (int i = 0; i < 7; ++i) { m->conv_dim[i] = 512; m->conv_kernel[i] = k[i]; m->conv_stride[i] = s[i]; }
  m->ln_eps = 1e-5f; m->pool_kernel = 8; m->pool_stride = 4; m->llm_dim = 3072;
  m->layers = layers;
}

int main() {
  EXPECT(sl_version() == SL_ABI_VERSION && SL_ABI_VERSION == 7, "ABI version");
  EXPECT(sl_last_error() != nullptr, "error string never NULL");

  // ---- tuning switches: parser under the sanitizers, garbage included
  setenv("SL_STREAM_CFG", "4,2,16", 1);
  setenv("SL_STREAM_MIN_M", "-7", 1);
  setenv("SL_T256_MIN_TILES", "99999999999999999999", 1);
  setenv("SL_DISABLE_GLDS", "2", 1);
  EXPECT(sl_tuning_reload() == 0, "tuning reload");
  setenv("SL_STREAM_CFG", ",,,;;", 1);
  EXPECT(sl_tuning_reload() == 0, "tuning reload (garbage)");
  unsetenv("SL_STREAM_CFG"); unsetenv("SL_STREAM_MIN_M"); unsetenv("SL_T256_MIN_TILES"); unsetenv("SL_DISABLE_GLDS");
  EXPECT(sl_tuning_reload() == 0, "tuning reload (defaults)");

  // ---- GEMM family
  EXPECT_ARG_ERROR(sl_gemm(nullptr, nullptr));
  sl_gemm_args g;
  memset(&g, 0, sizeof(g));
  EXPECT_ARG_ERROR(sl_gemm(&g, nullptr));                       // M = N = K = 0
  g.M = 4; g.N = 8; g.K = 8; g.batch = 1; g.dtype = 7;
  EXPECT_ARG_ERROR(sl_gemm(&g, nullptr));                       // unknown dtype
  g.dtype = SL_BF16; g.K = 12;
  EXPECT_ARG_ERROR(sl_gemm(&g, nullptr));                       // K % 8
  EXPECT_ARG_ERROR(sl_gemm_ex(nullptr, nullptr, nullptr));
  EXPECT_ARG_ERROR(sl_gemm_fused_decode(nullptr, nullptr, nullptr));
  EXPECT_ARG_ERROR(sl_pack_weight(nullptr, 0, nullptr, 16, 32, SL_BF16, nullptr));
  for (int M : {1, 16, 33, 64, 128, 129, 512, 1024})
    for (int N : {48, 3072, 5120, 16384, 128256})
      for (int K : {64, 3072, 8192}) {
        const size_t b = sl_gemm_split_workspace_bytes(M, N, K, SL_BF16);
        const int sp = sl_gemm_split_count(M, N, K, SL_BF16);
        EXPECT(sp >= 1 && sp <= 64, "split count in range");
        EXPECT(b < ((size_t)1 << 40), "split workspace sane");
      }

  // ---- attention
  EXPECT_ARG_ERROR(sl_attn_fwd(nullptr, nullptr));
  sl_attn_args a;
  memset(&a, 0, sizeof(a));
  EXPECT_ARG_ERROR(sl_attn_fwd(&a, nullptr));
  int dummy[4] = {0, 1, 2, 3};
  a.q = a.k = a.v = dummy; a.out = dummy; a.cu_q = a.cu_k = a.klen = dummy;
  a.nseq = 1; a.max_qlen = 4; a.n_heads = 3; a.n_kv_heads = 2; a.head_dim = 64; a.dtype = SL_BF16;
  EXPECT_ARG_ERROR(sl_attn_fwd(&a, nullptr));                   // heads not a multiple of kv heads
  a.n_heads = 4; a.dropout_p = 1.5f;
  EXPECT_ARG_ERROR(sl_attn_fwd(&a, nullptr));                   // dropout_p outside [0, 1)
  a.dropout_p = 0.f; a.q_row_stride = 3;
  EXPECT_ARG_ERROR(sl_attn_fwd(&a, nullptr));                   // misaligned strides
  EXPECT_ARG_ERROR(sl_attn_bwd(nullptr, nullptr));
  sl_attn_bwd_args ab;
  memset(&ab, 0, sizeof(ab));
  EXPECT_ARG_ERROR(sl_attn_bwd(&ab, nullptr));
  EXPECT_ARG_ERROR(sl_attn_decode(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 1.f, SL_BF16, nullptr));
  EXPECT(sl_attn_decode_workspace_bytes(512, 24, 8, 448) > 0, "decode attention workspace");
  {  // K/V cache formats: an unknown code, e4m3 rows with fp32, e4m3 rows with head_dim 64 (pointers are never dereferenced)
    void* fk = (void*)(uintptr_t)(1 << 20);
    const int32_t* fi = (const int32_t*)fk;
    const float* ff = (const float*)fk;
    EXPECT_ARG_ERROR(sl_rope_kv_append_ex(fk, fk, fk, fi, fi, ff, ff, 4, 4, 2, 128, 64, SL_BF16, 2, nullptr));
    EXPECT_ARG_ERROR(sl_rope_kv_append_ex(fk, fk, fk, fi, fi, ff, ff, 4, 4, 2, 128, 64, SL_F32, SL_KV_FP8_E4M3, nullptr));
    EXPECT_ARG_ERROR(sl_rope_kv_append_ex(fk, fk, fk, fi, fi, ff, ff, 4, 4, 2, 64, 64, SL_F16, SL_KV_FP8_E4M3, nullptr));
    EXPECT_ARG_ERROR(sl_attn_decode_split_ex(fk, 512, fk, fk, fk, fk, fi, 2, 4, 2, 128, 64, 0.1f, SL_BF16, 2, 0, nullptr));
    EXPECT_ARG_ERROR(sl_attn_decode_split_ex(fk, 512, fk, fk, fk, fk, fi, 2, 4, 2, 128, 64, 0.1f, SL_F32, SL_KV_FP8_E4M3, 0, nullptr));
    EXPECT_ARG_ERROR(sl_attn_decode_split_ex(fk, 512, fk, fk, fk, fk, fi, 2, 4, 2, 64, 64, 0.1f, SL_BF16, SL_KV_FP8_E4M3, 0, nullptr));
    EXPECT_ARG_ERROR(sl_attn_decode_split_ex(fk, 512, fk, fk, fk, fk, fi, 2, 4, 2, 128, 64, 0.1f, SL_BF16, SL_KV_FP8_E4M3, 65, nullptr));   // shared_prefix > max_ctx
    sl_llama_layer kl[2];
    memset(kl, 0, sizeof(kl));
    sl_llama_model km;
    memset(&km, 0, sizeof(km));
    km.dtype = SL_BF16; km.hidden = 256; km.n_layers = 2; km.n_heads = 4; km.n_kv_heads = 2; km.head_dim = 128; km.ffn = 512; km.vocab = 1000;
    km.layers = kl;
    EXPECT(sl_kv_cache_bytes(&km, 3, 448, SL_KV_FP8_E4M3) == (size_t)2 * 3 * 2 * 448 * 128, "e4m3 cache bytes");
    EXPECT(sl_kv_cache_bytes(&km, 3, 448, SL_KV_MODEL_DTYPE) == (size_t)2 * 2 * 3 * 2 * 448 * 128, "16-bit cache bytes");
    EXPECT(sl_kv_cache_bytes(&km, 3, 448, 2) == 0 && sl_last_error()[0] != 0, "unknown format: 0 bytes and a message");
    km.dtype = SL_F32;
    EXPECT(sl_kv_cache_bytes(&km, 3, 448, SL_KV_FP8_E4M3) == 0, "e4m3 with fp32: 0 bytes");
    // the quantiser on the host: ties to even, the subnormal grid, the clamp, signed zero; never 0x7F / 0xFF
    const float qx[] = {0.f, -0.f, 1.f, -1.f, 448.f, 449.f, 60000.f, -1e30f, 0.001953125f, 0.0009765625f, 0.0029296875f, 17.f, 19.f, 0.015625f, 432.f, 1.0625f, 1.1875f};
    const uint8_t qw[] = {0x00, 0x80, 0x38, 0xB8, 0x7E, 0x7E, 0x7E, 0xFE, 0x01, 0x00, 0x02, 0x58, 0x5A, 0x08, 0x7E, 0x38, 0x3A};
    uint8_t qo[sizeof(qx) / sizeof(qx[0])];
    EXPECT(sl_kv_quantize_e4m3_host(qx, qo, (int64_t)(sizeof(qx) / sizeof(qx[0]))) == 0, "quantiser runs on the host");
    for (size_t i = 0; i < sizeof(qx) / sizeof(qx[0]); ++i) EXPECT(qo[i] == qw[i], "e4m3 byte of a known value");
    EXPECT_ARG_ERROR(sl_kv_quantize_e4m3_host(nullptr, qo, 1));
  }
  {   // e4m3 weight images: the host packer under the sanitizers on a (40, 192) bf16 weight read with a row stride of 200 out of an
      // exactly-sized allocation into an exactly-sized image (a read or write past either end is a report), and the refusals
    const int N = 40, K = 192, ld = 200;
    const size_t bytes = sl_w8_image_bytes(N, K);
    EXPECT(bytes == (size_t)48 * 192 + 4 * 48, "e4m3 image bytes");
    EXPECT(sl_w8_image_bytes(N, 96) == 0 && sl_w8_image_bytes(0, 64) == 0, "e4m3 image bytes of a bad shape");
    uint16_t* src = (uint16_t*)malloc(((size_t)(N - 1) * ld + K) * sizeof(uint16_t));
    unsigned char* img = (unsigned char*)aligned_alloc(16, (bytes + 15) / 16 * 16);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) src[(size_t)n * ld + k] = n == 7 ? 0 : (uint16_t)(0x3C00 + ((n * 131 + k * 17) & 0x3FF) + ((k & 1) << 15));   // bf16 bits, row 7 all zero
    EXPECT(sl_pack_weight_e4m3_host(src, ld, img, N, K, SL_BF16) == 0, "host packer runs");
    const float* sc = (const float*)(img + (size_t)48 * K);
    EXPECT(sc[7] == 1.0f && sc[40] == 1.0f && sc[47] == 1.0f && sc[0] > 0.f, "scales: 1 for the zero row and the padding rows");
    bool nan_byte = false, pad_zero = true;
    for (size_t i = 0; i < (size_t)48 * K; ++i) nan_byte = nan_byte || (img[i] & 0x7F) == 0x7F;
    for (int j = 0; j < K / 64; ++j)
      for (int lane = 0; lane < 64; ++lane)
        if ((lane & 15) >= 8)
          for (int e = 0; e < 16; ++e) pad_zero = pad_zero && img[(((size_t)2 * (K / 64) + j) * 64 + lane) * 16 + e] == 0;      // fragment 2: rows 40..47
    EXPECT(!nan_byte && pad_zero, "no 0x7F / 0xFF byte; padding rows are zero bytes");
    EXPECT(sl_pack_weight_e4m3_host(src, ld, img, N, K, SL_F32) == SL_ERR_UNSUPPORTED, "e4m3 image of a float32 weight");
    EXPECT_ARG_ERROR(sl_pack_weight_e4m3_host(src, ld, img, N, 96, SL_BF16));
    EXPECT_ARG_ERROR(sl_pack_weight_e4m3(src, ld, img, N, 96, SL_F16, nullptr));
    EXPECT(sl_w8_max_rows() == 26, "the e4m3 skinny range");
    sl_gemm_args wa;
    memset(&wa, 0, sizeof(wa));
    wa.A = img; wa.W = img; wa.C = img; wa.lda = wa.ldw = 256; wa.ldc = 256; wa.M = 27; wa.N = 256; wa.K = 256; wa.batch = 1; wa.dtype = SL_BF16; wa.w_layout = SL_W_PACKED_E4M3;
    EXPECT(sl_gemm(&wa, nullptr) == SL_ERR_UNSUPPORTED, "e4m3 layout above sl_w8_max_rows()");
    wa.w_layout = 3;
    EXPECT_ARG_ERROR(sl_gemm(&wa, nullptr));
    free(src); free(img);
  }
  {   // MXFP4 weight images: the host packer under the sanitizers on a (40, 384) bf16 weight read with a row stride of 392 out of an
      // exactly-sized allocation into an exactly-sized image, and the refusals
    const int N = 40, K = 384, ld = 392;
    const size_t bytes = sl_w4_image_bytes(N, K);
    EXPECT(bytes == (size_t)48 * 192 + 48 * 12, "MXFP4 image bytes");
    EXPECT(sl_w4_image_bytes(N, 192) == 0 && sl_w4_image_bytes(0, 128) == 0, "MXFP4 image bytes of a bad shape");
    uint16_t* src = (uint16_t*)malloc(((size_t)(N - 1) * ld + K) * sizeof(uint16_t));
    unsigned char* img = (unsigned char*)aligned_alloc(16, bytes);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) src[(size_t)n * ld + k] = n == 7 ? 0 : (uint16_t)(0x3C00 + ((n * 131 + k * 17) & 0x3FF) + ((k & 1) << 15));   // bf16 bits, row 7 all zero
    src[(size_t)3 * ld + 5] = 0x7F80; src[(size_t)3 * ld + 40] = 0x7FC0; src[(size_t)4 * ld + 9] = 0x0001;      // +inf, a NaN, the smallest subnormal
    EXPECT(sl_pack_weight_mxfp4_host(src, ld, img, N, K, SL_BF16) == 0, "host packer runs");
    const unsigned char* sc = img + (size_t)48 * K / 2;
    bool range = true, pad = true, neg_zero = false;
    for (size_t i = 0; i < (size_t)48 * K / 32; ++i) range = range && sc[i] >= 127 - 13 && sc[i] <= 127 + 13;
    for (int j = 0; j < K / 128; ++j) {
      for (int d = 0; d < 4; ++d) pad = pad && sc[(((size_t)0 * (K / 128) + j) * 16 + 7) * 4 + d] == 127;      // the all-zero row 7: e = 0
      for (int r = 8; r < 16; ++r)
        for (int d = 0; d < 4; ++d) pad = pad && sc[(((size_t)2 * (K / 128) + j) * 16 + r) * 4 + d] == 127;    // fragment 2: rows 40..47
      for (int lane = 0; lane < 64; ++lane)
        if ((lane & 15) >= 8)
          for (int e = 0; e < 16; ++e) pad = pad && img[(((size_t)2 * (K / 128) + j) * 64 + lane) * 16 + e] == 0;
    }
    for (size_t i = 0; i < (size_t)48 * K / 2; ++i) neg_zero = neg_zero || (img[i] & 0x0F) == 0x08 || (img[i] & 0xF0) == 0x80;
    EXPECT(range && pad && !neg_zero, "scale bytes within the clamp; zero and padding rows: e = 0, zero codes; no negative zero");
    EXPECT(sl_pack_weight_mxfp4_host(src, ld, img, N, K, SL_F32) == SL_ERR_UNSUPPORTED, "MXFP4 image of a float32 weight");
    EXPECT_ARG_ERROR(sl_pack_weight_mxfp4_host(src, ld, img, N, 192, SL_BF16));
    EXPECT_ARG_ERROR(sl_pack_weight_mxfp4_host(src, K - 1, img, N, K, SL_BF16));
    EXPECT_ARG_ERROR(sl_pack_weight_mxfp4(src, ld, img, N, 192, SL_F16, nullptr));
    EXPECT(sl_w4_max_rows() == 26, "the MXFP4 skinny range");
    int32_t kmul = 0, rows = -1, layout = 0;
    EXPECT(sl_weight_format_info(SL_WDEC_MXFP4, &kmul, &rows, &layout) == 0 && kmul == 128 && rows == sl_w4_max_rows() && layout == SL_W_PACKED_MXFP4, "MXFP4 format row");
    EXPECT(sl_weight_format_info(SL_WDEC_E4M3, &kmul, &rows, &layout) == 0 && kmul == 64 && rows == sl_w8_max_rows() && layout == SL_W_PACKED_E4M3, "e4m3 format row");
    EXPECT(sl_weight_format_info(SL_WDEC_MX_LINEAR, &kmul, &rows, nullptr) == 0 && kmul == 128 && rows == 0, "MX linears format row");
    EXPECT(sl_weight_format_info(SL_WDEC_MODEL_DTYPE, &kmul, &rows, &layout) == 0 && kmul == 1 && rows == 0 && layout == SL_W_PACKED, "model dtype format row");
    EXPECT_ARG_ERROR(sl_weight_format_info(3, &kmul, &rows, &layout));
    sl_gemm_args wa;
    memset(&wa, 0, sizeof(wa));
    wa.A = img; wa.W = img; wa.C = img; wa.lda = wa.ldw = 256; wa.ldc = 256; wa.M = 27; wa.N = 256; wa.K = 256; wa.batch = 1; wa.dtype = SL_BF16; wa.w_layout = SL_W_PACKED_MXFP4;
    EXPECT(sl_gemm(&wa, nullptr) == SL_ERR_UNSUPPORTED, "MXFP4 layout above sl_w4_max_rows()");
    wa.M = 4; wa.K = 192; wa.lda = wa.ldw = 192;
    EXPECT_ARG_ERROR(sl_gemm(&wa, nullptr));
    free(src); free(img);
  }
  {   // MX linears: the host packer and the host activation quantiser under the sanitizers, strided sources out of exactly-sized
      // allocations into exactly-sized outputs; the MX image holds the MXFP4 image's scale bytes, rearranged; and the refusals
    const int N = 40, K = 384, ld = 392, M = 5;
    const size_t bytes = sl_mx_weight_image_bytes(N, K);
    EXPECT(bytes == (size_t)48 * 192 + 48 * 12 && bytes == sl_w4_image_bytes(N, K), "MX image bytes");
    EXPECT(sl_mx_weight_image_bytes(N, 192) == 0 && sl_mx_weight_image_bytes(0, 128) == 0, "MX image bytes of a bad shape");
    uint16_t* src = (uint16_t*)malloc(((size_t)(N - 1) * ld + K) * sizeof(uint16_t));
    unsigned char* img = (unsigned char*)aligned_alloc(16, bytes);
    unsigned char* img4 = (unsigned char*)aligned_alloc(16, bytes);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) src[(size_t)n * ld + k] = n == 7 ? 0 : (uint16_t)(0x3C00 + ((n * 131 + k * 17) & 0x3FF) + ((k & 1) << 15));
    src[(size_t)3 * ld + 5] = 0x7F80; src[(size_t)3 * ld + 40] = 0x7FC0; src[(size_t)4 * ld + 9] = 0x0001;      // +inf, a NaN, the smallest subnormal
    EXPECT(sl_pack_weight_mx_host(src, ld, img, N, K, SL_BF16) == 0 && sl_pack_weight_mxfp4_host(src, ld, img4, N, K, SL_BF16) == 0, "host packers run");
    bool same = true;
    const unsigned char *sc = img + (size_t)48 * K / 2, *sc4 = img4 + (size_t)48 * K / 2;
    for (int f = 0; f < 3; ++f)
      for (int j = 0; j < K / 128; ++j)
        for (int lane = 0; lane < 64; ++lane)       // sc[f][j][lane] against the MXFP4 image's sc[f][j][r][d], r = lane & 15, d = lane >> 4
          same = same && sc[((size_t)f * (K / 128) + j) * 64 + lane] == sc4[(((size_t)f * (K / 128) + j) * 16 + (lane & 15)) * 4 + (lane >> 4)];
    EXPECT(same, "MX image scale bytes = the MXFP4 image's");
    EXPECT(sl_pack_weight_mx_host(src, ld, img, N, K, SL_F32) == SL_ERR_UNSUPPORTED, "MX image of a float32 weight");
    EXPECT_ARG_ERROR(sl_pack_weight_mx_host(src, ld, img, N, 192, SL_BF16));
    EXPECT_ARG_ERROR(sl_pack_weight_mx_host(src, K - 1, img, N, K, SL_BF16));
    EXPECT_ARG_ERROR(sl_pack_weight_mx(src, ld, img, N, 192, SL_F16, nullptr));
    unsigned char* q = (unsigned char*)aligned_alloc(16, (size_t)M * K);
    unsigned char* qs = (unsigned char*)malloc((size_t)M * (K / 32));
    EXPECT(sl_mxfp8_quantize_rows_host(src, ld, q, qs, M, K, SL_BF16) == 0, "host quantiser runs");
    EXPECT(q[(size_t)3 * K + 5] == 0x7E && q[(size_t)3 * K + 40] == 0x7F, "+inf -> 448, NaN -> 0x7F");
    EXPECT(sl_mxfp8_quantize_rows_host(src, ld, q, qs, M, K, SL_F32) == SL_ERR_UNSUPPORTED, "MXFP8 rows of float32 activations");
    EXPECT_ARG_ERROR(sl_mxfp8_quantize_rows_host(src, ld, q, qs, M, 48, SL_BF16));
    EXPECT_ARG_ERROR(sl_mxfp8_quantize_rows(src, K - 1, q, qs, M, K, SL_F16, nullptr));
    sl_gemm_mx_args ma;
    memset(&ma, 0, sizeof(ma));
    ma.Aq = q; ma.lda = K; ma.a_scales = qs; ma.W = img; ma.C = img4; ma.ldc = N; ma.M = M; ma.N = N; ma.K = 192; ma.dtype = SL_BF16;
    EXPECT_ARG_ERROR(sl_gemm_mx(&ma, nullptr));
    ma.K = K; ma.dtype = SL_F32;
    EXPECT(sl_gemm_mx(&ma, nullptr) == SL_ERR_UNSUPPORTED, "MX product in float32");
    ma.dtype = SL_BF16; ma.act = SL_ACT_GELU;
    EXPECT_ARG_ERROR(sl_gemm_mx(&ma, nullptr));
    free(src); free(img); free(img4); free(q); free(qs);
  }

  // ---- norms / element-wise / losses
  EXPECT_ARG_ERROR(sl_layernorm(nullptr, nullptr, nullptr, nullptr, 4, 1024, 1e-5f, 0, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_rmsnorm(nullptr, nullptr, nullptr, 4, 3072, 1e-5f, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_embed_gather(nullptr, nullptr, nullptr, 4, 3072, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_kd_logit_losses(nullptr, nullptr, nullptr, nullptr, nullptr, 4, 1000, nullptr, 3, nullptr, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_kd_mse_rows(nullptr, nullptr, nullptr, nullptr, 4, 3072, nullptr, 3, 2, nullptr, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_ce_loss(nullptr, nullptr, 4, 1000, 1.f, nullptr, nullptr, 0, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_hubert_conv0(nullptr, 16000, nullptr, nullptr, nullptr, nullptr, nullptr, 512, 10, 5, 1e-5f, SL_BF16, nullptr));
  float w1[1] = {0.f};
  EXPECT_ARG_ERROR(sl_hubert_conv0(w1, 16000, w1, w1, w1, w1, w1, 512, 3, 2, 1e-5f, SL_BF16, nullptr));   // geometry not built
  EXPECT_ARG_ERROR(sl_hubert_conv0(w1, 5, w1, w1, w1, w1, w1, 512, 10, 5, 1e-5f, SL_BF16, nullptr));      // shorter than the kernel

  // ---- HuBERT runtime: frame arithmetic and plan validation are host code
  sl_hubert_layer hl[24];
  memset(hl, 0, sizeof(hl));
  sl_hubert_model hm;
  fill_hubert(&hm, hl, 24);
  EXPECT(sl_hubert_num_frames(&hm, 160000) == 499, "10 s -> 499 frames");
  EXPECT(sl_hubert_num_frames(&hm, 16000) == 49, "1 s -> 49 frames");
  EXPECT(sl_hubert_num_frames(&hm, 300) == 0, "too short -> 0");
  int64_t offs[4] = {0, 160000, 160000 + 32000, 160000 + 32000 + 1920000};
  EXPECT(sl_hubert_workspace_bytes(&hm, offs, 3) > 0, "encoder workspace");
  int64_t short_offs[2] = {0, 200};
  EXPECT(sl_hubert_workspace_bytes(&hm, short_offs, 1) == 0, "too-short utterance -> 0 workspace + error");
  float wave[16] = {0};
  char ws[256];
  hm.proj_w = w1;
  EXPECT_ARG_ERROR(sl_hubert_forward(&hm, wave, short_offs, 1, ws, 3072, nullptr, nullptr, ws, sizeof(ws), nullptr));
  EXPECT_ARG_ERROR(sl_hubert_forward(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, ws, sizeof(ws), nullptr));     // workspace too small
  EXPECT_ARG_ERROR(sl_hubert_forward(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr));
  sl_hubert_model wm = hm;
  EXPECT_ARG_ERROR(sl_whisper_forward(&wm, wave, 1, ws, 3072, nullptr, nullptr, ws, sizeof(ws), nullptr));          // not a Whisper struct

  // ---- stack / ctc_pool head: descriptor checks, range clamping and the inverse index are host code
  {
    sl_downsample_desc ds;
    memset(&ds, 0, sizeof(ds));
    int32_t cnt3[3] = {2, 1, 3};
    ds.method = SL_DS_STACK; ds.factor = 4; ds.proj_in = 4 * hm.hidden; ds.proj_w = w1; ds.proj_b = w1;
    EXPECT(sl_hubert_workspace_bytes_ds(&hm, offs, 3, &ds) > 0, "stack workspace");
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, nullptr, ws, sizeof(ws), nullptr));   // no descriptor
    ds.factor = 0;
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, &ds, ws, sizeof(ws), nullptr));       // factor < 1
    ds.factor = 4; ds.proj_in = hm.hidden;
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, &ds, ws, sizeof(ws), nullptr));       // width != f H
    ds.method = SL_DS_CTC_POOL;
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, &ds, ws, sizeof(ws), nullptr));       // null tables
    ds.range_counts_host = cnt3; ds.ranges_dev = (const int64_t*)ws; ds.n_ranges = 5;
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, &ds, ws, sizeof(ws), nullptr));       // counts add up to 6
    ds.n_ranges = 6;
    EXPECT(sl_hubert_workspace_bytes_ds(&hm, offs, 3, &ds) > 0, "ctc_pool workspace");
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, &ds, ws, sizeof(ws), nullptr));       // workspace too small
    ds.method = SL_DS_POOL;
    EXPECT_ARG_ERROR(sl_hubert_forward_ds(&hm, wave, offs, 3, ws, 3072, nullptr, nullptr, &ds, ws, sizeof(ws), nullptr));       // pool has its own entry
    const int64_t rel[12] = {0, 4, 4, 9, -3, 100, 2, 3, 0, 1, 6, 8};
    const int64_t frames[3] = {5, 49, 8};
    int64_t packed[12];
    EXPECT(sl_segment_ranges_host(rel, cnt3, frames, 3, packed) == 0, "ranges pack");
    EXPECT(packed[2] == 4 && packed[3] == 5 && packed[4] == 5 + 46 && packed[5] == 5 + 49 && packed[10] == 54 + 6 && packed[11] == 54 + 8, "clamped and offset");
    const int64_t rel_bad[12] = {0, 4, 5, 9, 0, 1, 2, 3, 0, 1, 6, 8};        // (5, 9) of a 5-frame utterance: empty after clamping
    EXPECT_ARG_ERROR(sl_segment_ranges_host(rel_bad, cnt3, frames, 3, packed));
    EXPECT(strstr(sl_last_error(), "utterance 0") && strstr(sl_last_error(), "range 1"), "the message names utterance and range");
    int64_t row_ptr[63];
    int32_t cols[64];
    EXPECT(sl_segment_ranges_host(rel, cnt3, frames, 3, packed) == 0 && sl_segment_csr_host(packed, 6, 62, row_ptr, nullptr, 0) == 0, "csr count");
    EXPECT(row_ptr[62] == 4 + 1 + 3 + 1 + 1 + 2, "csr size");
    EXPECT_ARG_ERROR(sl_segment_csr_host(packed, 6, 62, row_ptr, cols, 3));            // cols too small
    EXPECT(sl_segment_csr_host(packed, 6, 62, row_ptr, cols, 64) == 0 && cols[row_ptr[4]] == 0 + 1 && row_ptr[5] - row_ptr[4] == 1, "csr fill");
    EXPECT_ARG_ERROR(sl_segment_csr_host(packed, 6, 61, row_ptr, nullptr, 0));          // a range past the rows
    EXPECT_ARG_ERROR(sl_segment_mean_batch(ws, ws, (const int64_t*)ws, 4, 100, 130, SL_BF16, nullptr));                            // H not a multiple of 8
    EXPECT_ARG_ERROR(sl_segment_mean_bwd_batch(ws, ws, (const int64_t*)ws, nullptr, nullptr, 4, 100, 128, SL_BF16, nullptr));     // no index
    EXPECT_ARG_ERROR(sl_stack_rows_batch(ws, ws, (const int64_t*)ws, 2, 10, 128, 0, SL_BF16, nullptr));                           // factor < 1
    EXPECT_ARG_ERROR(sl_stack_rows_bwd_batch(ws, ws, (const int64_t*)ws, 2, 10, 130, 4, SL_F16, nullptr));                        // H not a multiple of 8
    // CTC segmentation: the head and the ids -> ranges entry, every refusal before any launch
    int32_t* idp = (int32_t*)ws;
    EXPECT_ARG_ERROR(sl_ctc_greedy_batch(ws, ws, nullptr, nullptr, 100, 1024, 32, SL_BF16, nullptr));                              // null ids
    EXPECT_ARG_ERROR(sl_ctc_greedy_batch(ws, ws, nullptr, idp, 100, 1024, 65, SL_BF16, nullptr));                                  // V > 64
    EXPECT_ARG_ERROR(sl_ctc_greedy_batch(ws, ws, nullptr, idp, 100, 1028, 32, SL_F32, nullptr));                                   // H not a multiple of 8
    EXPECT(sl_ctc_greedy_batch(ws, ws, nullptr, idp, 0, 1024, 32, SL_F16, nullptr) == 0, "no rows: nothing to do");
    EXPECT(sl_ctc_pool_ranges_capacity(100, 3) == 106 && sl_ctc_words_capacity(100, 3) == 51, "capacity bounds");
    const int64_t* ro = (const int64_t*)ws;
    int64_t* tab = (int64_t*)ws;
    EXPECT_ARG_ERROR(sl_ctc_pool_ranges_batch(idp, ro, 3, 100, 0, 4, 4, SL_CTC_RANGES_PACKED, nullptr, 106, idp, nullptr, 0, nullptr, nullptr));   // null table
    EXPECT_ARG_ERROR(sl_ctc_pool_ranges_batch(idp, ro, 3, 100, 4, 4, 4, SL_CTC_RANGES_PACKED, tab, 106, idp, nullptr, 0, nullptr, nullptr));       // blank == delimiter
    EXPECT_ARG_ERROR(sl_ctc_pool_ranges_batch(idp, ro, 3, 100, 0, 4, 0, SL_CTC_RANGES_RAW, tab, 106, idp, nullptr, 0, nullptr, nullptr));          // pool_range < 1
    EXPECT_ARG_ERROR(sl_ctc_pool_ranges_batch(idp, ro, 3, 100, 0, 4, 4, SL_CTC_RANGES_PACKED, tab, 105, idp, nullptr, 0, nullptr, nullptr));       // capacity below the bound
    EXPECT_ARG_ERROR(sl_ctc_pool_ranges_batch(idp, ro, 3, 100, 0, 4, 4, SL_CTC_RANGES_PACKED, tab, 106, idp, tab, 50, idp, nullptr));             // word capacity below the bound
    EXPECT_ARG_ERROR(sl_ctc_pool_ranges_batch(idp, ro, 3, 100, 0, 4, 4, 2, tab, 106, idp, nullptr, 0, nullptr, nullptr));                          // unknown mode
  }

  // ---- Llama runtime
  sl_llama_layer ll[28];
  memset(ll, 0, sizeof(ll));
  sl_llama_model lm;
  memset(&lm, 0, sizeof(lm));
  lm.dtype = SL_BF16; lm.hidden = 3072; lm.n_layers = 28; lm.n_heads = 24; lm.n_kv_heads = 8; lm.head_dim = 128; lm.ffn = 8192; lm.vocab = 128256;
  lm.rms_eps = 1e-5f; lm.rope_len = 448; lm.layers = ll;
  EXPECT(sl_llama_workspace_bytes(&lm, 512 * 137, 512) > 0, "prefill workspace");
  EXPECT(sl_generate_workspace_bytes(&lm, 512 * 137, 512, 256) > sl_llama_workspace_bytes(&lm, 512 * 137, 512), "generate workspace");
  sl_kv_cache kv;
  memset(&kv, 0, sizeof(kv));
  int32_t cu[2] = {0, 137};
  float logits[1];
  int32_t ctx[1];
  EXPECT_ARG_ERROR(sl_llama_prefill(&lm, &kv, ws, cu, 1, logits, ctx, nullptr, ws, sizeof(ws), nullptr));            // null model fields
  lm.embed = lm.lm_head = lm.final_norm = w1; lm.rope_cos = lm.rope_sin = w1;
  EXPECT_ARG_ERROR(sl_llama_prefill(&lm, &kv, ws, cu, 1, logits, ctx, nullptr, ws, sizeof(ws), nullptr));            // bad kv cache
  kv.k_cache = kv.v_cache = ws; kv.slots = 1; kv.max_ctx = 4096;
  EXPECT_ARG_ERROR(sl_llama_prefill(&lm, &kv, ws, cu, 1, logits, ctx, nullptr, ws, sizeof(ws), nullptr));            // max_ctx beyond the rope table
  kv.max_ctx = 256;
  int32_t out_ids[8], n_steps = 0;
  int32_t eos[3] = {128001, 128008, 128009};
  EXPECT_ARG_ERROR(sl_greedy_generate(&lm, &kv, ws, cu, 1, 256, eos, 3, 128001, 1, 16, out_ids, &n_steps, nullptr, ws, sizeof(ws), nullptr));   // prompt + new > max_ctx
  EXPECT_ARG_ERROR(sl_greedy_generate(&lm, &kv, ws, cu, 4096, 8, eos, 3, 128001, 1, 16, out_ids, &n_steps, nullptr, ws, sizeof(ws), nullptr));  // batch above the limit
  kv.shared_prefix = 200;
  EXPECT_ARG_ERROR(sl_greedy_generate(&lm, &kv, ws, cu, 1, 8, eos, 3, 128001, 1, 16, out_ids, &n_steps, nullptr, ws, sizeof(ws), nullptr));     // shared prefix longer than the prompt
  kv.shared_prefix = 0;
  {   // sl_generate (ABI 6): options checked before anything is launched
    sl_generate_opts go;
    memset(&go, 0, sizeof(go));
    sl_generate_stats gs;
    go.max_new_tokens = 8; go.eos_ids_host = eos; go.n_eos = 3; go.pad_id = 128001; go.use_eos = 1; go.compact = 1;
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, 1, nullptr, out_ids, &gs, ws, sizeof(ws), nullptr));                 // no options
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, SL_MAX_DECODE_BATCH + 1, &go, out_ids, &gs, ws, sizeof(ws), nullptr));   // batch above the limit
    go.n_eos = 9;
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, sizeof(ws), nullptr));                      // more than 8 eos ids
    go.n_eos = 3;
    int32_t lim[1] = {9};
    go.row_limits_host = lim;
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, sizeof(ws), nullptr));                      // budget above max_new_tokens
    lim[0] = 0;
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, sizeof(ws), nullptr));                      // budget below 1
    go.row_limits_host = nullptr;
    go.sample = 1; go.temperature = 0.f; go.top_p = 1.f;
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, sizeof(ws), nullptr));                      // temperature 0
    go.sample = 0;
    EXPECT_ARG_ERROR(sl_generate(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, 64, nullptr));                              // workspace too small
  }
  {   // the generation loops' own limits, with a model and a cache that pass every earlier check: refused before any device call
    sl_generate_opts go;
    memset(&go, 0, sizeof(go));
    sl_generate_stats gs;
    go.max_new_tokens = 8; go.eos_ids_host = eos; go.n_eos = 3; go.pad_id = 128001; go.use_eos = 1; go.compact = 1;
    float* lps = (float*)ws;
    const size_t need = sl_generate_workspace_bytes_sc(&lm, 137, 1, 8, nullptr, 1);
    EXPECT(need > 0, "generate workspace with scores");
    EXPECT_ARG_ERROR_SAYS(sl_generate_sc(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, need - 1, nullptr, nullptr, lps), "workspace");       // workspace one byte short
    go.max_new_tokens = 128;
    EXPECT_ARG_ERROR_SAYS(sl_generate_sc(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, need, nullptr, nullptr, lps), "max_ctx");           // 137 + 128 > max_ctx = 256
    go.max_new_tokens = 8;
    int32_t lim[1] = {0};
    go.row_limits_host = lim;
    EXPECT_ARG_ERROR_SAYS(sl_generate_sc(&lm, &kv, ws, cu, 1, &go, out_ids, &gs, ws, need, nullptr, nullptr, lps), "row limit");           // row limit 0
    go.row_limits_host = nullptr;
    {   // teacher-forced scoring: sl_llama_score refuses before any device call; the workspace arithmetic
      int32_t start[1] = {130}, nsc[1] = {7};
      const int32_t* lab = (const int32_t*)ws;
      int32_t* iws = (int32_t*)ws;
      const size_t sneed = sl_llama_score_workspace_bytes(&lm, 137, 1, 7, nullptr);
      EXPECT(sneed > sl_llama_workspace_bytes(&lm, 137, 1), "score workspace above the prefill workspace");
      EXPECT(sl_llama_score_workspace_bytes(&lm, 137, 1, 138, nullptr) == 0, "more scored rows than rows");
      EXPECT_ARG_ERROR_SAYS(sl_llama_score(&lm, &kv, ws, cu, 1, start, nsc, lab, lps, iws, nullptr, nullptr, nullptr, nullptr, ws, sneed - 1, nullptr), "workspace");
      nsc[0] = 8;
      EXPECT_ARG_ERROR_SAYS(sl_llama_score(&lm, &kv, ws, cu, 1, start, nsc, lab, lps, iws, nullptr, nullptr, nullptr, nullptr, ws, sneed, nullptr), "leave its 137 rows");
      nsc[0] = 0;
      EXPECT_ARG_ERROR_SAYS(sl_llama_score(&lm, &kv, ws, cu, 1, start, nsc, lab, lps, iws, nullptr, nullptr, nullptr, nullptr, ws, sneed, nullptr), "nothing to score");
      nsc[0] = 7;
      EXPECT_ARG_ERROR_SAYS(sl_llama_score(&lm, &kv, ws, cu, 1, start, nsc, lab, lps, iws, lps, nullptr, iws, nullptr, ws, sneed, nullptr), "all three or none");
      sl_score_opts so;
      memset(&so, 0, sizeof(so));
      so.row_chunk = -1;
      EXPECT_ARG_ERROR_SAYS(sl_llama_score(&lm, &kv, ws, cu, 1, start, nsc, lab, lps, iws, nullptr, nullptr, nullptr, &so, ws, sneed, nullptr), "row_chunk");
    }
    {   // multi-turn sessions: sl_llama_prefill_cont / sl_generate_cont refuse before any device call
      sl_kv_cache kvs = kv;
      kvs.slots = 3;
      const size_t pneed = sl_llama_workspace_bytes(&lm, 137, 1);
      const size_t pneed2 = sl_llama_workspace_bytes(&lm, 20, 2);
      int32_t cu2[3] = {0, 10, 20};
      int32_t past[2] = {-1, 0}, slot[2] = {0, 1};
      EXPECT_ARG_ERROR_SAYS(sl_llama_prefill_cont(&lm, &kvs, ws, cu2, past, nullptr, 2, logits, ctx, ws, pneed2, nullptr), "negative");
      past[0] = 120;
      EXPECT_ARG_ERROR_SAYS(sl_llama_prefill_cont(&lm, &kvs, ws, cu, past, nullptr, 1, logits, ctx, ws, pneed, nullptr), "exceed max_ctx");      // 120 + 137 > 256
      past[0] = 100; past[1] = 30;
      kvs.shared_prefix = 31;
      EXPECT_ARG_ERROR_SAYS(sl_llama_prefill_cont(&lm, &kvs, ws, cu2, past, nullptr, 2, logits, ctx, ws, pneed2, nullptr), "shared_prefix");    // above the shortest past
      kvs.shared_prefix = 0;
      slot[0] = 1;
      EXPECT_ARG_ERROR_SAYS(sl_llama_prefill_cont(&lm, &kvs, ws, cu2, past, slot, 2, logits, ctx, ws, pneed2, nullptr), "two sequences");       // slot 1 twice
      slot[0] = 3;
      EXPECT_ARG_ERROR_SAYS(sl_llama_prefill_cont(&lm, &kvs, ws, cu2, nullptr, slot, 2, logits, ctx, ws, pneed2, nullptr), "outside");          // slot 3 of 3
      slot[0] = 0;
      EXPECT(sl_generate_workspace_bytes_cont(&lm, 137, 1, 8, nullptr, 1) == need, "cont workspace = sc workspace");
      past[0] = 50;
      EXPECT_ARG_ERROR_SAYS(sl_generate_cont(&lm, &kvs, ws, cu, 1, &go, out_ids, &gs, ws, need, nullptr, nullptr, lps, past, nullptr), "compact");   // compact = 1 on a kept cache
      go.compact = 0;
      past[0] = 112;
      EXPECT_ARG_ERROR_SAYS(sl_generate_cont(&lm, &kvs, ws, cu, 1, &go, out_ids, &gs, ws, need, nullptr, nullptr, lps, past, nullptr), "max_ctx");   // 112 + 137 + 8 > 256
      past[0] = -2;
      EXPECT_ARG_ERROR_SAYS(sl_generate_cont(&lm, &kvs, ws, cu, 1, &go, out_ids, &gs, ws, need, nullptr, nullptr, lps, past, nullptr), "negative");
      past[0] = 50; slot[0] = 2;
      EXPECT_ARG_ERROR_SAYS(sl_generate_cont(&lm, &kvs, ws, cu, 1, &go, out_ids, &gs, ws, need, nullptr, nullptr, lps, past, slot), "slot order");   // a row's slot is its index
      go.compact = 1;
      // sl_attn_fwd_past: the forms that are not built, and a format code that is none
      sl_attn_args pa;
      memset(&pa, 0, sizeof(pa));
      void* fk = (void*)(uintptr_t)(1 << 20);
      const int32_t* fi = (const int32_t*)fk;
      pa.q = pa.k = pa.v = fk; pa.out = fk; pa.cu_q = pa.cu_k = pa.klen = fi;
      pa.nseq = 1; pa.max_qlen = 4; pa.n_heads = 4; pa.n_kv_heads = 2; pa.head_dim = 128; pa.causal = 1; pa.dtype = SL_BF16;
      pa.q_row_stride = pa.k_row_stride = pa.v_row_stride = pa.o_row_stride = 1024; pa.q_head_stride = pa.k_head_stride = pa.v_head_stride = pa.o_head_stride = 128;
      EXPECT(sl_attn_fwd_past(&pa, fk, fk, fi, fi, 64, 2, nullptr) == SL_ERR_ARG, "format code 2 is SL_ERR_ARG");
      EXPECT(sl_attn_fwd_past(&pa, fk, fk, fi, fi, 64, -1, nullptr) == SL_ERR_ARG, "format code -1 is SL_ERR_ARG");
      EXPECT(sl_attn_fwd_past(&pa, nullptr, fk, fi, fi, 64, 1, nullptr) == SL_ERR_ARG, "null cache");
      pa.dtype = SL_F32;
      EXPECT(sl_attn_fwd_past(&pa, fk, fk, fi, fi, 64, 1, nullptr) == SL_ERR_UNSUPPORTED, "fp32 is SL_ERR_UNSUPPORTED");
      pa.dtype = SL_F16; pa.head_dim = 64;
      EXPECT(sl_attn_fwd_past(&pa, fk, fk, fi, fi, 64, 0, nullptr) == SL_ERR_UNSUPPORTED, "head_dim 64 is SL_ERR_UNSUPPORTED");
      pa.head_dim = 128; pa.causal = 0;
      EXPECT(sl_attn_fwd_past(&pa, fk, fk, fi, fi, 64, 0, nullptr) == SL_ERR_UNSUPPORTED, "non-causal is SL_ERR_UNSUPPORTED");
    }
    go.row_limits_host = lim;
    sl_kv_cache kv4 = kv;
    kv4.slots = 4;
    sl_beam_opts bo;
    memset(&bo, 0, sizeof(bo));
    bo.eos_ids_host = eos; bo.n_eos = 3; bo.use_eos = 1; bo.max_new_tokens = 8; bo.num_beams = 2; bo.num_return_sequences = 1; bo.length_penalty = 1.0f;
    sl_logits_opts lp = {1.2f, 0, 0, 0};
    float sc[2];
    int32_t ln[2];
    const size_t bneed = sl_beam_generate_workspace_bytes_lp(&lm, 137, 1, &kv4, &bo, &lp);
    EXPECT(bneed > 0, "beam workspace with the penalty on");
    EXPECT_ARG_ERROR_SAYS(sl_beam_generate_lp(&lm, &kv4, ws, cu, 1, &bo, out_ids, sc, ln, &gs, ws, bneed - 1, nullptr, &lp), "workspace");   // workspace one byte short
    bo.num_beams = 9;
    EXPECT_ARG_ERROR_SAYS(sl_beam_generate_lp(&lm, &kv4, ws, cu, 1, &bo, out_ids, sc, ln, &gs, ws, bneed, nullptr, &lp), "num_beams");       // num_beams 9
  }
  EXPECT(sl_comm_abort(nullptr) == 0, "aborting no communicator is a no-op");
  kv.shared_prefix = -1;
  EXPECT_ARG_ERROR(sl_llama_prefill(&lm, &kv, ws, cu, 1, logits, ctx, nullptr, ws, sizeof(ws), nullptr));            // negative shared prefix
  kv.shared_prefix = 0;
  lm.head_dim = 96;
  EXPECT_ARG_ERROR(sl_llama_prefill(&lm, &kv, ws, cu, 1, logits, ctx, nullptr, ws, sizeof(ws), nullptr));            // head_dim not built
  EXPECT_ARG_ERROR(sl_llama_decode_step(&lm, &kv, nullptr, nullptr, 1, logits, ws, sizeof(ws), nullptr));

  // ---- KD tape runtime
  sl_enc_stack_cfg ec;
  memset(&ec, 0, sizeof(ec));
  ec.dtype = SL_BF16; ec.hidden = 1024; ec.n_heads = 16; ec.ffn = 4096; ec.n_layers = 24; ec.nseq = 16; ec.max_len = 499; ec.n_tok = 16 * 499;
  EXPECT(sl_encoder_stack_train_workspace_bytes(&ec) > 0, "encoder tape workspace");
  EXPECT_ARG_ERROR(sl_encoder_stack_train_fwd(nullptr, &ec, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
  EXPECT_ARG_ERROR(sl_encoder_stack_train_bwd(nullptr, &ec, nullptr, nullptr, 0, 24, nullptr, nullptr, 0, nullptr));
  sl_llama_stack_cfg lc;
  memset(&lc, 0, sizeof(lc));
  lc.dtype = SL_BF16; lc.hidden = 3072; lc.n_heads = 24; lc.n_kv_heads = 8; lc.head_dim = 128; lc.ffn = 8192; lc.n_layers = 28; lc.nseq = 16; lc.max_len = 200;
  lc.n_tok = 3200;
  EXPECT(sl_llama_stack_train_workspace_bytes(&lc) > 0, "llama tape workspace");
  EXPECT_ARG_ERROR(sl_llama_stack_train_fwd(nullptr, &lc, nullptr, nullptr, nullptr, 0, nullptr));
  EXPECT_ARG_ERROR(sl_llama_stack_train_bwd(nullptr, &lc, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));

  // ---- round-3 entry points
  EXPECT_ARG_ERROR(sl_adamw_step(nullptr, nullptr, 0, 0, 5e-5, 0.9, 0.999, 1e-8, 0.01, 1, nullptr));
  EXPECT_ARG_ERROR(sl_adamw_step((const sl_adamw_tensor*)ws, (const int64_t*)ws, 1, 1, 5e-5, 1.5, 0.999, 1e-8, 0.01, 1, nullptr));    // beta1 >= 1
  EXPECT_ARG_ERROR(sl_adamw_step((const sl_adamw_tensor*)ws, (const int64_t*)ws, 1, 1, 5e-5, 0.9, 0.999, 1e-8, 0.01, 0, nullptr));    // step counts from 1
  EXPECT(sl_adamw_blocks(0) == 0 && sl_adamw_blocks(1) == 1 && sl_adamw_blocks(4096) == 1 && sl_adamw_blocks(4097) == 2, "adamw block count");
  EXPECT(sl_layernorm_bwd_ws_bytes(7984, 1024) > 0 && sl_layernorm_bwd_ws_bytes(7984, 2048) == 0 && sl_layernorm_bwd_ws_bytes(0, 1024) == 0, "layernorm backward scratch size");
  EXPECT_ARG_ERROR(sl_layernorm_bwd_ws(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 16, 1024, 1e-5f, 0, SL_BF16, nullptr, 0, nullptr));
  EXPECT_ARG_ERROR(sl_greedy_select_partial(nullptr, nullptr, 2004, 1024, eos, 3, 128001, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 8, nullptr));
  EXPECT_ARG_ERROR(sl_greedy_select_partial((const float*)ws, (const int32_t*)ws, 2004, 8, eos, 9, 128001, 1, 1, ctx, ctx, ctx, ctx, ctx, out_ids, 8, nullptr));   // > 8 eos ids
  {
    sl_gemm_args ga;
    memset(&ga, 0, sizeof(ga));
    ga.A = ws; ga.W = ws; ga.lda = 64; ga.ldw = 64; ga.M = 32; ga.N = 128; ga.K = 64; ga.batch = 1; ga.dtype = SL_BF16; ga.out_f32 = 1;
    sl_gemm_ex_args gx;
    memset(&gx, 0, sizeof(gx));
    gx.w_mod = 1; gx.amax_val = (float*)ws;                         // amax_idx missing
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.amax_idx = (int32_t*)ws;                                     // M <= 64: the fused top-1 lives in the tiled kernels
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    // training-tape epilogue fusions (ABI 7): every refused combination comes back as an argument error, before any launch
    memset(&gx, 0, sizeof(gx));
    gx.w_mod = 1; ga.M = 256; ga.out_f32 = 0; ga.C = ws; ga.ldc = 128;
    gx.post_op = 9;                                                 // unknown post-op
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.post_op = SL_POST_DROPOUT; gx.drop_p = 0.1f; gx.drop_ld = 0; // a mask needs its index stride
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.drop_ld = 128; gx.drop_p = 1.5f;                             // p outside [0, 1)
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.drop_p = 0.1f; gx.trans_w = 1;                               // transposed operands keep the plain epilogue
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.trans_w = 0; gx.post_op = SL_POST_GELU_BWD; gx.post_in = nullptr;   // GELU' without the saved pre-activation
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.post_op = SL_POST_SILU_MUL_BWD; gx.post_in = ws; gx.post_ld = 256; gx.drop_p = 0.f;     // ldc must span the 2 N-wide output
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.post_op = SL_POST_NONE; gx.colsum_out = (float*)ws; ga.M = 32;      // M <= 64: post-ops / colsum_out live in the tiled kernels
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
    gx.trans_a = gx.trans_w = 1; ga.M = 192; ga.N = 128; ga.K = 512;        // the bias-gradient rider needs the token-major kernel's shapes (M % 128)
    EXPECT_ARG_ERROR(sl_gemm_ex(&ga, &gx, nullptr));
  }
  {   // SL_GEMM_LOG=2, the dispatcher's dry run: plan_tiled under the sanitizers (every rule, the recursion of the 128-tile split, the token-major
      // runs), the plan printed, 0 returned before any HIP call — the operand pointers are never read
    setenv("SL_GEMM_LOG", "2", 1);
    EXPECT(sl_tuning_reload() == 0, "tuning reload (dry run)");
    sl_gemm_args ga;
    memset(&ga, 0, sizeof(ga));
    alignas(16) static char ops[64];      // stands for every operand: 16-byte aligned as the argument checks ask, never read
    ga.A = ops; ga.W = ops; ga.C = ops; ga.batch = 1; ga.dtype = SL_BF16;
    sl_gemm_ex_args gx;
    memset(&gx, 0, sizeof(gx));
    gx.w_mod = 1; gx.sk_ws = ops; gx.sk_ws_bytes = sl_gemm_streamk_workspace_bytes();
    int32_t runs = -1;
    const int shapes[][3] = {{300, 256, 200}, {2048, 2048, 512}, {5072, 3072, 3072}, {634, 3072, 8192}, {634, 3072, 16384}, {3200, 3072, 16384}, {400, 3072, 16384}, {16, 3072, 3072}};
    for (const auto& s : shapes) {
      ga.M = s[0]; ga.N = s[1]; ga.K = s[2]; ga.lda = ga.ldw = s[2]; ga.ldc = s[1];
      for (int dt : {SL_BF16, SL_F32}) {
        ga.dtype = dt;
        EXPECT(sl_gemm(&ga, nullptr) == 0, "dry run: plain product");
        EXPECT(sl_gemm_ex(&ga, &gx, nullptr) == 0, "dry run: product with a workspace");
      }
    }
    ga.dtype = SL_BF16; ga.M = 3200; ga.N = 3072; ga.K = 16384; ga.lda = ga.ldw = 16384; ga.ldc = 3072;
    gx.deferred_splits = &runs;
    EXPECT(sl_gemm_ex(&ga, &gx, nullptr) == 0 && runs == 0, "dry run: deferred K runs are planned, not handed over");
    gx.deferred_splits = nullptr;
    gx.trans_a = gx.trans_w = 1; ga.M = 1024; ga.N = 1024; ga.K = 7984; ga.lda = ga.ldw = ga.ldc = 1024;
    EXPECT(sl_gemm_ex(&ga, &gx, nullptr) == 0, "dry run: token-major product in K runs");
    unsetenv("SL_GEMM_LOG");
    EXPECT(sl_tuning_reload() == 0, "tuning reload (defaults)");
  }
  EXPECT_ARG_ERROR(sl_col2im_batch(nullptr, nullptr, nullptr, 4, 100, 64, 3, 2, SL_BF16, nullptr));
  EXPECT_ARG_ERROR(sl_col2im_batch(ws, ws, (const int64_t*)ws, 4, 100, 60, 3, 2, SL_BF16, nullptr));            // C not a multiple of 8
  EXPECT_ARG_ERROR(sl_avgpool_bwd_batch(ws, ws, (const int64_t*)ws, 0, 100, 128, 8, 4, SL_BF16, nullptr));      // no utterances
  EXPECT_ARG_ERROR(sl_avgpool_bwd_batch(ws, ws, (const int64_t*)ws, 2, 100, 130, 8, 4, SL_BF16, nullptr));      // H not a multiple of 8
  EXPECT(sl_decode_graph_cache_clear() == 0, "nothing cached on this thread");

  {   // collective group: argument checks only (no device here)
    sl_comm c = nullptr;
    unsigned char id[SL_COMM_ID_BYTES] = {0};
    EXPECT(sl_comm_unique_id(nullptr) == SL_ERR_ARG, "sl_comm_unique_id(null)");
    EXPECT(sl_comm_init(nullptr, id, 0, 1) == SL_ERR_ARG, "sl_comm_init(null out)");
    EXPECT(sl_comm_init(&c, id, 2, 2) == SL_ERR_ARG && c == nullptr, "sl_comm_init(rank >= world)");
    EXPECT(sl_allreduce_sum(nullptr, id, 4, SL_F32, nullptr) == SL_ERR_ARG, "sl_allreduce_sum(no communicator)");
    EXPECT(sl_comm_destroy(nullptr) == 0 && sl_comm_rank(nullptr) == -1 && sl_comm_world(nullptr) == -1, "sl_comm_destroy(null) is a no-op");
  }
  {   // beam search: every limit is answered before any launch, and the workspace arithmetic runs under the sanitizers
    sl_llama_model bm;
    memset(&bm, 0, sizeof(bm));
    bm.dtype = SL_BF16; bm.hidden = 3072; bm.n_layers = 28; bm.n_heads = 24; bm.n_kv_heads = 8; bm.head_dim = 128; bm.ffn = 8192; bm.vocab = 128256; bm.rope_len = 448;
    sl_kv_cache bkv;
    memset(&bkv, 0, sizeof(bkv));
    bkv.slots = 1024; bkv.max_ctx = 448;
    const int32_t eos[3] = {1, 2, 3};
    sl_beam_opts bo;
    memset(&bo, 0, sizeof(bo));
    bo.eos_ids_host = eos; bo.n_eos = 3; bo.use_eos = 1; bo.max_new_tokens = 256; bo.num_beams = 4; bo.num_return_sequences = 1; bo.length_penalty = 1.0f;
    const size_t need = sl_beam_generate_workspace_bytes(&bm, 137 * 256, 256, &bkv, &bo);
    const size_t stage = sl_kv_beam_staging_bytes(&bkv, &bm, 1024, 256);
    EXPECT(stage == (size_t)2 * 1024 * 28 * 8 * 256 * 128 * 2 && need > stage, "beam workspace holds the staging area");
    bo.num_beams = 9;
    EXPECT(sl_beam_generate_workspace_bytes(&bm, 137, 1, &bkv, &bo) == 0 && sl_last_error()[0] != 0, "num_beams 9");
    EXPECT_ARG_ERROR(sl_beam_generate(&bm, &bkv, nullptr, nullptr, 1, &bo, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    bo.num_beams = 8; bo.n_eos = 8;                                                                            // M = 72 > 64
    EXPECT(sl_beam_generate(&bm, &bkv, nullptr, nullptr, 1, &bo, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SL_ERR_UNSUPPORTED, "M > 64");
    bo.n_eos = 3; bo.num_return_sequences = 9;
    EXPECT_ARG_ERROR(sl_beam_generate(&bm, &bkv, nullptr, nullptr, 1, &bo, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    bo.num_return_sequences = 1;
    EXPECT_ARG_ERROR(sl_beam_generate(&bm, &bkv, nullptr, nullptr, 129, &bo, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));      // 1 032 rows > 1 024 slots
    EXPECT_ARG_ERROR(sl_beam_topk((const float*)ws, 4, 100, nullptr, 65, (float*)ws, (int32_t*)ws, nullptr));
    sl_beam_state bs;
    memset(&bs, 0, sizeof(bs));
    EXPECT_ARG_ERROR(sl_beam_step(&bs, (const float*)ws, (const int32_t*)ws, 2, 8, 32, 0, &bo, nullptr));     // null state fields
    EXPECT_ARG_ERROR(sl_kv_beam_reorder(&bkv, &bm, (const int32_t*)ws, (const int32_t*)ws, (const int32_t*)ws, 8, 16, ws, 16, nullptr));   // null cache
    // logits processors: options are checked before anything else; off / NULL options leave the workspace sizes alone
    bo.num_beams = 4;
    sl_logits_opts lp = {1.0f, 0, 0, 0};
    EXPECT(sl_beam_generate_workspace_bytes_lp(&bm, 137 * 256, 256, &bkv, &bo, &lp) == need, "processors off: the beam workspace is unchanged");
    EXPECT(sl_generate_workspace_bytes_lp(&bm, 137 * 256, 256, 256, nullptr) == sl_generate_workspace_bytes(&bm, 137 * 256, 256, 256), "NULL options: unchanged");
    lp.repetition_penalty = 1.2f;
    EXPECT(sl_generate_workspace_bytes_lp(&bm, 137 * 256, 256, 256, &lp) == sl_generate_workspace_bytes(&bm, 137 * 256, 256, 256) + (size_t)256 * 256 * 4 + 256,
           "penalty on: + the gather scratch");
    EXPECT(sl_beam_generate_workspace_bytes_lp(&bm, 137 * 256, 256, &bkv, &bo, &lp) > need, "penalty on: the beam workspace grows");
    sl_generate_opts go;
    memset(&go, 0, sizeof(go));
    go.max_new_tokens = 16;
    const float bad_p[4] = {0.f, -1.f, INFINITY, NAN};
    for (float p : bad_p) {
      lp.repetition_penalty = p;
      EXPECT_ARG_ERROR(sl_generate_lp(nullptr, nullptr, nullptr, nullptr, 1, &go, nullptr, nullptr, nullptr, 0, nullptr, &lp));
      EXPECT_ARG_ERROR(sl_beam_generate_lp(&bm, &bkv, nullptr, nullptr, 1, &bo, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &lp));
      EXPECT_ARG_ERROR(sl_logits_process((float*)ws, 4, 100, (const int32_t*)ws, 8, (const int32_t*)ws, nullptr, &lp, eos, 3, 0, (float*)ws, nullptr));
    }
    lp.repetition_penalty = 1.2f; lp.no_repeat_ngram_size = -1;
    EXPECT_ARG_ERROR(sl_generate_lp(nullptr, nullptr, nullptr, nullptr, 1, &go, nullptr, nullptr, nullptr, 0, nullptr, &lp));
    lp.no_repeat_ngram_size = 2; lp.min_new_tokens = 17;                                                       // > max_new_tokens = 16
    EXPECT_ARG_ERROR(sl_generate_lp(nullptr, nullptr, nullptr, nullptr, 1, &go, nullptr, nullptr, nullptr, 0, nullptr, &lp));
    lp.min_new_tokens = 4;
    EXPECT_ARG_ERROR(sl_logits_process((float*)ws, 4, 100, (const int32_t*)ws, 8, (const int32_t*)ws, nullptr, &lp, eos, 9, 0, (float*)ws, nullptr));   // 9 eos ids
    EXPECT_ARG_ERROR(sl_logits_process((float*)ws, 4, 100, (const int32_t*)ws, 8, (const int32_t*)ws, nullptr, &lp, eos, 3, 0, nullptr, nullptr));     // no scratch
    EXPECT_ARG_ERROR(sl_beam_topk_ex((const float*)ws, 4, 100, nullptr, 65, (float*)ws, (int32_t*)ws, nullptr, 1));
  }
  {
    // token log-probabilities (additive to ABI 7): the third plane rides on the fused top-1 and is refused with it
    sl_gemm_args ga;
    memset(&ga, 0, sizeof(ga));
    ga.A = ws; ga.W = ws; ga.lda = 64; ga.ldw = 64; ga.M = 128; ga.N = 128; ga.K = 64; ga.batch = 1; ga.dtype = SL_BF16; ga.out_f32 = 1;
    sl_gemm_ex_args gx;
    memset(&gx, 0, sizeof(gx));
    gx.w_mod = 1;
    EXPECT_ARG_ERROR(sl_gemm_top1_lse(&ga, nullptr, (float*)ws, nullptr));                    // no ex args
    EXPECT_ARG_ERROR(sl_gemm_top1_lse(&ga, &gx, (float*)ws, nullptr));                        // the third plane without the first two
    gx.amax_val = (float*)ws;
    EXPECT_ARG_ERROR(sl_gemm_top1_lse(&ga, &gx, (float*)ws, nullptr));                        // ... without amax_idx
    gx.amax_idx = (int32_t*)ws;
    EXPECT_ARG_ERROR(sl_gemm_top1_lse(&ga, &gx, nullptr, nullptr));                           // no third plane
    ga.M = 64;                                                                                // M <= 64: no tiled kernel, no fused top-1
    EXPECT_ARG_ERROR(sl_gemm_top1_lse(&ga, &gx, (float*)ws, nullptr));
    EXPECT_ARG_ERROR(sl_greedy_select_sc(nullptr, 4, 100, eos, 3, 0, 1, ctx, ctx, ctx, ctx, ctx, out_ids, 8, (float*)ws, nullptr));
    EXPECT_ARG_ERROR(sl_greedy_select_partial_sc((const float*)ws, (const int32_t*)ws, nullptr, 16, 128, eos, 3, 0, 1, 1, ctx, ctx, ctx, ctx, ctx, out_ids, 8,
                                                 (float*)ws, nullptr));                     // log-probabilities without the third plane
    EXPECT_ARG_ERROR(sl_greedy_select_partial_sc((const float*)ws, (const int32_t*)ws, (const float*)ws, 16, 128, eos, 3, 0, 1, 1, ctx, ctx, ctx, ctx, ctx, out_ids,
                                                 8, nullptr, nullptr));                     // ... and the reverse
    EXPECT_ARG_ERROR(sl_sample_select_sc((const float*)ws, 4, 100, 0.f, 0, 1.f, 1, eos, 3, 0, 1, ctx, ctx, ctx, ctx, ctx, out_ids, 8, ctx, (float*)ws, nullptr));   // temperature 0
    sl_llama_model sm;
    memset(&sm, 0, sizeof(sm));
    sm.dtype = SL_BF16; sm.hidden = 256; sm.n_layers = 2; sm.n_heads = 2; sm.n_kv_heads = 2; sm.head_dim = 128; sm.ffn = 384; sm.vocab = 1000; sm.rope_len = 64;
    EXPECT(sl_generate_workspace_bytes_sc(&sm, 40, 4, 16, nullptr, 0) == sl_generate_workspace_bytes(&sm, 40, 4, 16), "scores off: the workspace is unchanged");
    EXPECT(sl_generate_workspace_bytes_sc(&sm, 40, 4, 16, nullptr, 1) == sl_generate_workspace_bytes(&sm, 40, 4, 16) + (size_t)4 * 16 * 4 + 256,
           "scores on: + the (nseq, max_new_tokens) log-probabilities");
    sl_generate_opts go;
    memset(&go, 0, sizeof(go));
    go.max_new_tokens = 16;
    EXPECT_ARG_ERROR(sl_generate_sc(nullptr, nullptr, nullptr, nullptr, 1, &go, nullptr, nullptr, nullptr, 0, nullptr, nullptr, (float*)ws));
    // min_p / typical_p / epsilon_cutoff / eta_cutoff: a value outside its range is refused before any launch, by both entries
    const sl_warp_opts bad[] = {{-0.1f, 1.f, 0.f, 0.f}, {1.5f, 1.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 1.5f, 0.f, 0.f}, {0.f, 1.f, 1.f, 0.f},
                                {0.f, 1.f, -0.1f, 0.f}, {0.f, 1.f, 0.f, 1.f}, {0.f, 1.f, 0.f, NAN}, {NAN, 1.f, 0.f, 0.f}};
    for (const sl_warp_opts& w : bad) {
      EXPECT_ARG_ERROR(sl_sample_select_w((const float*)ws, 4, 100, 1.f, 0, 1.f, 1, eos, 3, 0, 1, ctx, ctx, ctx, ctx, ctx, out_ids, 8, ctx, (float*)ws, nullptr, &w));
      EXPECT_ARG_ERROR(sl_generate_w(nullptr, nullptr, nullptr, nullptr, 1, &go, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, &w));
    }
    EXPECT(sizeof(sl_warp_opts) == 16, "sl_warp_opts is four floats");
  }
  if (g_fail == 0) printf("argcheck ok\n");
  return g_fail == 0 ? 0 : 1;
}
