// wformat.h — the weight formats of a Llama model (speechllm.h SL_WDEC_*), one row each: what a format's rules are is written here and
// nowhere else in the library.  sl_weight_format_info (llama_ops.hip) hands the numbers to the Python side.
#pragma once
#include "common.h"

// the entries of the Llama runtime, as bits of SlWFormat::runs
enum { SL_ENTRY_PREFILL = 1, SL_ENTRY_DECODE = 2, SL_ENTRY_GENERATE_N = 4, SL_ENTRY_BEAM = 8, SL_ENTRY_SCORE = 16, SL_ENTRY_ALL = 31 };

struct SlWFormat {
  int code;                                      // SL_WDEC_*
  const char* name;                              // in messages
  int k_multiple;                                // every reduction length is a multiple of this
  int w_layout;                                  // what the *_dec pointers are read with; -1: the format has no *_dec images
  int32_t (*max_rows)(void);                     // most decode rows it runs; NULL: no limit
  const char* max_rows_name;
  size_t (*image_bytes)(int32_t N, int32_t K);   // NULL: N * K elements of the model dtype
  bool dec_images;                               // true: the five *_dec pointers hold its images and only decoding reads them;
                                                 // false: its images replace the layers' row-major pointers, for every row count
  unsigned runs;                                 // SL_ENTRY_* that run it; the others refuse it before any launch
};

static const SlWFormat sl_wformats[] = {
    {SL_WDEC_MODEL_DTYPE, "model dtype", 1, SL_W_PACKED, nullptr, nullptr, nullptr, true, SL_ENTRY_ALL},
    {SL_WDEC_E4M3, "e4m3", 64, SL_W_PACKED_E4M3, sl_w8_max_rows, "sl_w8_max_rows", sl_w8_image_bytes, true, SL_ENTRY_ALL},
    {SL_WDEC_MXFP4, "MXFP4", 128, SL_W_PACKED_MXFP4, sl_w4_max_rows, "sl_w4_max_rows", sl_w4_image_bytes, true, SL_ENTRY_ALL},
    {SL_WDEC_MX_LINEAR, "MX linears (format 5)", 128, -1, nullptr, nullptr, sl_mx_weight_image_bytes, false, SL_ENTRY_PREFILL | SL_ENTRY_DECODE},
};
#define SL_WFORMAT_LIST "0 = model dtype, 1 = e4m3 weight images, 4 = MXFP4 weight images, 5 = MX linears"

// NULL for what is no format: 2, 3, 6, negatives and the rest
static inline const SlWFormat* sl_wformat(int code) {
  for (const SlWFormat& f : sl_wformats)
    if (f.code == code) return &f;
  return nullptr;
}
// the quantised decode-image format a sl_gemm_args.w_layout names (SL_W_PACKED_E4M3, SL_W_PACKED_MXFP4); NULL for the 16-bit layouts
static inline const SlWFormat* sl_wformat_of_layout(int w_layout) {
  for (const SlWFormat& f : sl_wformats)
    if (f.max_rows && f.w_layout == w_layout) return &f;
  return nullptr;
}
static inline size_t sl_wformat_bytes(const SlWFormat* f, int N, int K, size_t elem_size) { return f->image_bytes ? f->image_bytes(N, K) : (size_t)N * K * elem_size; }

// The public structs carry their format codes in the field named `reserved`: sl_llama_model.reserved is the weight format (SL_WDEC_*),
// sl_kv_cache.reserved and sl_gemm_fused.reserved are the K/V cache format (SL_KV_*).  The library reads the field through these.
static inline int sl_wformat_code(const sl_llama_model* m) { return m->reserved; }
static inline int sl_kv_format(const sl_kv_cache* kv) { return kv->reserved; }
static inline int sl_kv_format(const sl_gemm_fused* fx) { return fx->reserved; }
