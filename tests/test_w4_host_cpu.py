"""CPU: the host side of the opt-in MXFP4 (e2m1 elements, e8m0 block scales) decode weights.  The header names the new layout and the
decode-weight format as code 4 without an ABI bump, the new entries are mirrored in the ctypes table, the host packer (the routines
the device packer runs) is held byte for byte against the format written here in torch FROM ITS DEFINITION — block exponent as the
smallest e of the clamped range with amax <= 6 * 2^e, elements by nearest grid point in fp64 with ties to the even code, layout by
index arithmetic — and every entry refuses what is not built (float32, K % 128 != 0, more rows than sl_w4_max_rows(), GELU) before any
device work, so all of this runs without a GPU.  The reference never calls the C routine."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import pkg

L = pkg("_lib")
ops = pkg("ops")
cfgm = pkg("config")
weights = pkg("weights")
llama_mod = pkg("audio_llama")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(1 << 20)          # a non-null, 16-byte aligned pointer the argument checks never dereference
ERR_ARG, ERR_UNSUPPORTED = -1, -3
F16, BF16 = torch.float16, torch.bfloat16
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _err():
    return L.lib().sl_last_error().decode()


def test_header_defines_the_two_codes_as_4_and_keeps_abi_7():
    h = open(os.path.join(REPO, "include", "speechllm.h")).read()
    assert re.search(r"#define SL_W_PACKED_MXFP4 4\b", h)
    assert re.search(r"#define SL_WDEC_MXFP4\s+4\b", h)
    assert re.search(r"#define SL_W_PACKED_E4M3 2\b", h) and re.search(r"#define SL_WDEC_E4M3\s+1\b", h)
    assert re.search(r"#define SL_ABI_VERSION 7\b", h)
    assert L.lib().sl_version() == 7
    assert L.W_PACKED_MXFP4 == 4 and L.WDEC_MXFP4 == 4
    assert (L.W_ROWMAJOR, L.W_PACKED, L.W_PACKED_E4M3) == (0, 1, 2) and (L.WDEC_MODEL_DTYPE, L.WDEC_E4M3) == (0, 1)


def test_new_exports_are_mirrored():
    for name in ("sl_w4_image_bytes", "sl_pack_weight_mxfp4", "sl_pack_weight_mxfp4_host", "sl_w4_max_rows"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().sl_w4_max_rows() == 26 == L.lib().sl_w8_max_rows()          # the packed skinny range (SL_STREAM_MIN_M unset)


def test_image_bytes():
    lib = L.lib()
    assert lib.sl_w4_image_bytes(16, 128) == 16 * 64 + 16 * 4
    assert lib.sl_w4_image_bytes(40, 384) == 48 * 192 + 48 * 12
    assert lib.sl_w4_image_bytes(1000, 256) == 1008 * 128 + 1008 * 8
    assert lib.sl_w4_image_bytes(128256, 3072) == 128256 * 1536 + 128256 * 96
    for n, k in ((16, 64), (0, 128), (16, 0), (16, 192), (-1, 128)):
        assert lib.sl_w4_image_bytes(n, k) == 0 and "sl_w4_image_bytes" in _err()


# ------------------------------------------------------------------------------------------------------------------------------
# the format, written out from its definition
# ------------------------------------------------------------------------------------------------------------------------------
def ref_quantise(w):
    """(N, K) bf16 / fp16 -> (codes (N, K) uint8, exponents (N, K/32) int64), from the definition, in fp64"""
    N, K = w.shape
    v = w.double().view(N, K // 32, 32)
    a = torch.where(torch.isnan(v), torch.zeros_like(v), v.abs())
    amax = a.amax(-1)                                                   # NaN elements skipped
    e = torch.full(amax.shape, 13, dtype=torch.int64)                   # nothing in the range holds amax: the top of the clamp
    for cand in range(12, -14, -1):                                     # ... else the smallest e of [-13, 13] with amax <= 6 * 2^e
        e = torch.where(amax <= 6.0 * 2.0 ** cand, torch.full_like(e, cand), e)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    x = v / torch.exp2(e.double())[:, :, None]                          # exact in fp64
    ax = torch.where(torch.isnan(x), torch.zeros_like(x), x.abs().clamp(max=6.0))      # saturation (inf included); NaN -> 0
    lo = (torch.searchsorted(GRID, ax.contiguous(), right=True) - 1).clamp(0, 7)
    hi = (lo + 1).clamp(max=7)
    dl, dh = ax - GRID[lo], GRID[hi] - ax
    even = torch.where(lo % 2 == 0, lo, hi)
    code = torch.where(hi == lo, lo, torch.where(dl < dh, lo, torch.where(dl > dh, hi, even)))
    code = torch.where((x < 0) & (code != 0), code + 8, code)           # sign in bit 3; no negative zero
    return code.view(N, K).to(torch.uint8), e


def ref_image(w):
    """-> (element bytes of the image (Np*K/2,), scale bytes (Np*K/32,), natural-order codes (Np, K), scale bytes (Np, K/32)) on the CPU"""
    N, K = w.shape
    Np = (N + 15) // 16 * 16
    code = torch.zeros(Np, K, dtype=torch.uint8)
    sc = torch.full((Np, K // 32), 127, dtype=torch.uint8)              # padding rows: e = 0
    c, e = ref_quantise(w)
    code[:N], sc[:N] = c, (e + 127).to(torch.uint8)
    f = torch.arange(Np // 16)[:, None, None, None, None]
    j = torch.arange(K // 128)[None, :, None, None, None]
    lane = torch.arange(64)[None, None, :, None, None]
    d = torch.arange(4)[None, None, None, :, None]
    b = torch.arange(4)[None, None, None, None, :]
    rows, cols = 16 * f + (lane & 15), 128 * j + 32 * d + 8 * (lane >> 4) + 2 * b
    img = code[rows, cols] | (code[rows, cols + 1] << 4)                # (Np/16, K/128, 64, 4, 4): element 2b low nibble, 2b+1 high
    f4, j4 = torch.arange(Np // 16)[:, None, None, None], torch.arange(K // 128)[None, :, None, None]
    r4, d4 = torch.arange(16)[None, None, :, None], torch.arange(4)[None, None, None, :]
    sci = sc[16 * f4 + r4, 4 * j4 + d4]                                 # sc[f][j][r][d]: row 16 f + r, block 4 j + d
    return img.reshape(-1), sci.reshape(-1), code, sc


def dequantise(code, sc):
    """codes (R, K), scale bytes (R, K/32) -> fp64 values e2m1 * 2^e"""
    g = torch.cat([GRID, -GRID])[code.long()]
    return (g.view(code.shape[0], -1, 32) * torch.exp2(sc.double() - 127)[:, :, None]).view(code.shape)


def split_image(img, N, K):
    Np = (N + 15) // 16 * 16
    return img[:Np * K // 2], img[Np * K // 2:]


def weight_rows(N, K, dt, seed=0):
    """(N, K) test weight in dt: magnitudes vary by 2^((block + row) % 9 - 4) along K and across rows; row 0 all zero; row 1 walks the
    grid values at scale 1; row 2 one outlier among tiny values; row 3 holds an all-zero block inside a non-zero row."""
    g = torch.Generator().manual_seed(2000 + seed)
    mag = 2.0 ** ((torch.arange(K // 32)[None, :] + torch.arange(N)[:, None]) % 9 - 4).float()
    w = torch.randn(N, K // 32, 32, generator=g) * mag[:, :, None]
    w = w.view(N, K)
    w[0] = 0
    vals = torch.cat([GRID, -GRID]).float()
    w[1] = vals[torch.randint(0, 16, (K,), generator=g)]
    w[1, ::32] = 6.0
    w[2] = torch.randn(K, generator=g) * 3e-5
    w[2, K // 2] = -7.0
    w[3, 32:64] = 0
    return w.to(dt)


SHAPES = [(16, 128), (40, 384), (1000, 256)]


def _check(w):
    N, K = w.shape
    want_b, want_s, nat, sc = ref_image(w)
    img = ops.pack_weight_mxfp4(w)                     # CPU tensor: sl_pack_weight_mxfp4_host
    assert img.numel() == L.lib().sl_w4_image_bytes(N, K)
    got_b, got_s = split_image(img, N, K)
    assert torch.equal(got_s, want_s), f"{int((got_s != want_s).sum())} scale bytes differ"
    assert torch.equal(got_b, want_b), f"{int((got_b != want_b).sum())} element bytes differ"
    c2, s2 = ops.w4_image_parts(img, N, K)              # the inverse the Python surface uses
    assert torch.equal(c2, nat) and torch.equal(s2, sc)
    assert not bool((c2 == 8).any()), "a negative zero (code 0x8) in the image"
    assert int(s2.min()) >= 127 - 13 and int(s2.max()) <= 127 + 13
    assert bool((c2[N:] == 0).all()) and bool((s2[N:] == 127).all()), "padding rows: zero codes, e = 0"
    assert torch.equal(ops.w4_dequantise(img, N, K), dequantise(nat, sc)[:N])
    return c2, s2


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_host_packer_matches_the_format_byte_for_byte(dt, N, K):
    w = weight_rows(N, K, dt)
    c, s = _check(w)
    assert bool((c[0] == 0).all()) and bool((s[0] == 127).all()), "the all-zero row"
    assert bool((s[1] == 127).all()) and torch.equal(dequantise(c[1:2], s[1:2])[0], w[1].double()), "amax = 6: e = 0, grid values unchanged"
    assert int(c[2, K // 2]) == 0xE and int(s[2, K // 64]) == 127 + 1, "the outlier -7: e = 1, -3.5 ties to the even code 6 (-4)"
    assert bool((c[3, 32:64] == 0).all()) and int(s[3, 1]) == 127 and int(c[3].count_nonzero()) > K // 2, "an all-zero block inside a non-zero row"


def test_host_packer_reads_a_strided_source_with_poison_in_the_pad_columns():
    w = weight_rows(40, 384, BF16, seed=3)
    wide = torch.full((40, 512), 3e4, dtype=BF16)
    wide[:, :384] = w
    assert torch.equal(ops.pack_weight_mxfp4(wide[:, :384]), ops.pack_weight_mxfp4(w))


def _next_up(x, dt):
    """one ulp above a positive value of dt"""
    t = torch.tensor([x], dtype=dt)
    return float((t.view(torch.int16) + 1).view(dt)[0])


@pytest.mark.parametrize("dt", [BF16, F16])
def test_host_packer_on_rows_built_to_hit_the_edges(dt):
    """every block below is built for one edge of the definition; the image must equal the reference and, where the definition gives
    the answer outright, the stated codes and exponents"""
    K = 256
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    tie_codes = [0, 2, 2, 4, 4, 6, 6]                                     # ties go to the even code
    exps = [-13, -6, -1, 0, 1, 5, 12, 13]          # 6 * 2^13 = 49 152 is a finite fp16 too
    rows, expect = [], []                                                 # expect: (row, block, e or None, {k in block: code})

    def row():
        rows.append(torch.zeros(K))
        return len(rows) - 1, rows[-1]

    for e in exps:
        s = 2.0 ** e
        # amax exactly 6 * 2^e (mantissa exactly 1.5) with every tie point of both signs; negative .25 rounds to zero: code 0x0
        n, r = row()
        r[0] = 6 * s
        r[1:8], r[8:15] = ties * s, -ties * s
        expect.append((n, 0, e, dict([(0, 7)] + [(1 + i, c) for i, c in enumerate(tie_codes)] + [(8 + i, c + 8 if c else 0) for i, c in enumerate(tie_codes)])))
        # amax one ulp above 6 * 2^e (mantissa one ulp above 1.5): the next exponent, 6.x / 2 -> 3; at the top of the clamp it saturates
        r[32] = _next_up(6 * s, dt)
        r[33] = -0.2 * s
        expect.append((n, 1, min(e + 1, 13), {0: 7 if e == 13 else 5, 1: 0}))
        # amax with mantissa exactly 1.0 (4 * 2^e), of either sign
        r[64] = 4 * s
        expect.append((n, 2, e, {0: 6}))
        r[96] = -4 * s
        r[97] = 3 * s
        expect.append((n, 3, e, {0: 14, 1: 5}))
    # an all-zero block inside a non-zero row
    n, r = row()
    r[:32] = torch.linspace(-3, 3, 32)
    r[64:] = 0.01
    expect.append((n, 1, 0, {i: 0 for i in range(32)}))
    # a block above 6 * 2^13 (saturates at +-6, e = 13), with an inf
    n, r = row()
    big = 60000.0 if dt == F16 else 3.0e6
    r[0], r[1], r[2], r[3] = big, -big, float("inf"), 2.0 ** 12
    expect.append((n, 0, 13, {0: 7, 1: 15, 2: 7, 3: 1}))
    r[32], r[33] = float("-inf"), 1.0
    expect.append((n, 1, 13, {0: 15, 1: 0}))
    # a block below 2^-14 (clamped exponent: e = -13, values round on the 2^-14 grid or to zero)
    tiny = 2.0 ** -15
    r[64], r[65], r[66], r[67] = tiny, 3 * tiny, -tiny, -0.4 * tiny
    expect.append((n, 2, -13, {0: 0, 1: 2, 2: 0, 3: 0}))                   # 2^-15 = .25 * 2^-13 -> tie to 0; 3 * 2^-15 = .75 * 2^-13 -> tie to 1.0
    # a NaN element: skipped by the block maximum, code 0
    r[96], r[97], r[98] = float("nan"), 3.0, -0.5
    expect.append((n, 3, -1, {0: 0, 1: 7, 2: 10}))
    # a block that is NaN only
    r[128:160] = float("nan")
    expect.append((n, 4, 0, {i: 0 for i in range(32)}))
    w = torch.stack(rows).to(dt)
    c, s = _check(w)
    for n, blk, e, codes in expect:
        assert int(s[n, blk]) - 127 == e, (n, blk, int(s[n, blk]) - 127, e)
        for k, code in codes.items():
            assert int(c[n, 32 * blk + k]) == code, (n, blk, k, int(c[n, 32 * blk + k]), code)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals, without a device
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [True, False])
def test_packer_refuses_float32_ragged_k_null_pointers_and_a_short_stride(host):
    lib = L.lib()

    def call(N, K, dtype, src=FAKE, dst=FAKE, ld=None):
        ld = K if ld is None else ld
        if host:
            return lib.sl_pack_weight_mxfp4_host(src, ld, dst, N, K, dtype)
        return lib.sl_pack_weight_mxfp4(src, ld, dst, N, K, dtype, None)

    assert call(16, 128, L.SL_F32) == ERR_UNSUPPORTED and "float32" in _err()
    assert call(16, 64, L.SL_BF16) == ERR_ARG and "multiple of 128" in _err()
    assert call(16, 192, L.SL_F16) == ERR_ARG and "multiple of 128" in _err()
    assert call(16, 128, 7) == ERR_ARG and "dtype" in _err()
    assert call(0, 128, L.SL_F16) == ERR_ARG
    assert call(16, 128, L.SL_BF16, src=None) == ERR_ARG and call(16, 128, L.SL_BF16, dst=None) == ERR_ARG
    assert call(16, 128, L.SL_BF16, ld=127) == ERR_ARG and "ld_src" in _err()


def _gemm_args(M, N, K, dtype, w_layout):
    a = L.GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = FAKE.value, K, FAKE.value, K, FAKE.value, N
    a.M, a.N, a.K, a.batch, a.dtype, a.act, a.w_layout = M, N, K, 1, dtype, L.ACT_NONE, w_layout
    return a


def test_gemm_refuses_what_the_mxfp4_kernels_do_not_take():
    lib = L.lib()
    rows = lib.sl_w4_max_rows()
    W4 = L.W_PACKED_MXFP4
    a = _gemm_args(rows + 1, 256, 256, L.SL_BF16, W4)
    assert lib.sl_gemm(C.byref(a), None) == ERR_UNSUPPORTED and "sl_w4_max_rows" in _err() and str(rows + 1) in _err()
    f = L.GemmFused()
    assert lib.sl_gemm_fused_decode(C.byref(a), C.byref(f), None) == ERR_UNSUPPORTED and "rows" in _err()
    a = _gemm_args(4, 256, 256, L.SL_F32, W4)
    assert lib.sl_gemm(C.byref(a), None) == ERR_UNSUPPORTED and "float32" in _err()
    a = _gemm_args(4, 256, 192, L.SL_F16, W4)
    assert lib.sl_gemm(C.byref(a), None) == ERR_ARG and "K % 128" in _err()
    a = _gemm_args(4, 256, 256, L.SL_BF16, 3)                              # still not a layout
    assert lib.sl_gemm(C.byref(a), None) == ERR_ARG and "w_layout 3" in _err()
    a = _gemm_args(4, 256, 256, L.SL_BF16, W4)
    a.act = L.ACT_GELU
    assert lib.sl_gemm(C.byref(a), None) == ERR_ARG and "GELU" in _err()


def _model(dtype=L.SL_BF16, hidden=256, ffn=512, n_layers=2, reserved=L.WDEC_MXFP4):
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab = dtype, hidden, n_layers, 4, 2, 128, ffn, 1000
    m.rms_eps, m.rope_len = 1e-5, 512
    layers = (L.LlamaLayer * n_layers)()
    for lay in layers:
        for name, _ in L.LlamaLayer._fields_:
            setattr(lay, name, FAKE.value)
    m.layers = layers
    m._keep = layers
    for f in ("embed", "lm_head", "final_norm", "rope_cos", "rope_sin", "lm_head_dec"):
        setattr(m, f, FAKE.value)
    m.dec_fused_norm, m.reserved = 1, reserved
    return m


def _kv(slots):
    kv = L.KVCache()
    kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx = FAKE.value, FAKE.value, slots, 64
    return kv


def _step(m, B):
    kv = _kv(64)
    return L.lib().sl_llama_decode_step(C.byref(m), C.byref(kv), FAKE, FAKE, B, FAKE, FAKE, 1 << 40, None)


def _generate(m, B):
    kv = _kv(64)
    cu = (C.c_int32 * (B + 1))(*range(0, 4 * (B + 1), 4))
    o = L.GenerateOpts()
    o.max_new_tokens = 4
    out = (C.c_int32 * (4 * B))()
    return L.lib().sl_generate(C.byref(m), C.byref(kv), FAKE, cu, B, C.byref(o), out, None, FAKE, 1 << 40, None)


@pytest.mark.parametrize("entry", [_step, _generate], ids=["sl_llama_decode_step", "sl_generate"])
def test_mxfp4_model_is_refused_before_any_launch(entry):
    rows = L.lib().sl_w4_max_rows()
    assert entry(_model(dtype=L.SL_F32), 2) == ERR_UNSUPPORTED and "float32" in _err() and "MXFP4" in _err()
    assert entry(_model(), rows + 1) == ERR_UNSUPPORTED and "sl_w4_max_rows" in _err() and str(rows + 1) in _err()
    assert entry(_model(ffn=576), 2) == ERR_UNSUPPORTED and "multiple of 128" in _err() and "576" in _err()      # a multiple of 64: the e4m3 format takes it
    assert entry(_model(ffn=576, reserved=L.WDEC_E4M3), rows + 1) == ERR_UNSUPPORTED and "sl_w8_max_rows" in _err()
    for bad in (2, 3):
        assert entry(_model(reserved=bad), 2) == ERR_ARG and f"format {bad}" in _err()
    m = _model()
    m.dec_fused_norm = 0
    assert entry(m, 2) == ERR_ARG and "dec_fused_norm" in _err()
    m = _model()
    m.layers[1].wgu_dec = None
    assert entry(m, 2) == ERR_ARG and "null *_dec image" in _err() and "layer 1" in _err()


# ------------------------------------------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_weight_format_code_config_helper_and_shipped_configs():
    assert L.weight_format_code("mxfp4") == L.WDEC_MXFP4 == L.weight_format_code("fp4") == 4
    assert L.weight_format_code("fp8") == L.WDEC_E4M3 and L.weight_format_code(None) == L.WDEC_MODEL_DTYPE
    for bad in ("int8", "model", "int4", "mxfp8", torch.float8_e5m2, torch.float16, torch.uint8):
        with pytest.raises(L.SpeechLLMError):
            L.weight_format_code(bad)
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="mxfp4")))) == "mxfp4"
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="fp4")))) == "mxfp4"
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="fp8")))) == "fp8"
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="model")))) is None
    with pytest.raises(ValueError):
        cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="int4"))))
    for f in ("llama3_hubert", "llama3_whisper", "minichat_hubert", "minichat_whisper"):      # the option is off by default
        assert cfgm.runtime_weight_dtype(cfgm.load_config(os.path.join(REPO, "config", f + ".yaml"))) is None


def test_constructor_refusals_and_the_default_format():
    arch = weights.LlamaArch(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=512,
                             vocab_size=100)
    mk = lambda a=arch, **kw: llama_mod.AudioLlamaForCausalLM(a, {}, **kw)
    assert mk(torch_dtype=BF16, weight_dtype="mxfp4").weight_format == L.WDEC_MXFP4
    assert mk(torch_dtype=F16, weight_dtype="fp4", kv_cache_dtype="fp8").weight_format == L.WDEC_MXFP4
    assert mk(torch_dtype=BF16).weight_format == L.WDEC_MODEL_DTYPE           # option unset: as before
    with pytest.raises(L.SpeechLLMError, match="float32"):
        mk(torch_dtype=torch.float32, weight_dtype="mxfp4")
    with pytest.raises(L.SpeechLLMError, match="pack_decode"):
        mk(torch_dtype=BF16, weight_dtype="mxfp4", pack_decode=False)
    odd = weights.LlamaArch(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=576,
                            vocab_size=100)
    with pytest.raises(L.SpeechLLMError, match="multiple of 128"):
        mk(odd, torch_dtype=BF16, weight_dtype="mxfp4")
    assert mk(odd, torch_dtype=BF16, weight_dtype="fp8").weight_format == L.WDEC_E4M3      # 576 is a multiple of 64
    llm = mk(torch_dtype=torch.float32)
    with pytest.raises(L.SpeechLLMError):
        llm.set_weight_dtype("mxfp4")
    assert llm.weight_format == L.WDEC_MODEL_DTYPE


def test_weight_bytes_per_token_of_llama_3b():
    """the issue's table: 1.61 GB of elements + 0.10 GB of scales, 4.25 bits per weight, against 6.43 GB of 16-bit weights"""
    w = weights.LlamaDeviceWeights.__new__(weights.LlamaDeviceWeights)
    w.arch = weights.LlamaArch(hidden_size=3072, num_hidden_layers=28, num_attention_heads=24, num_key_value_heads=8, head_dim=128, intermediate_size=8192,
                               vocab_size=128256)
    w.dtype = BF16
    n4, n16 = w.weight_bytes_per_token("mxfp4"), w.weight_bytes_per_token()
    per_layer = (5120 * 3072 + 3072 * 3072 + 3 * 8192 * 3072)
    elems = 28 * per_layer + 128256 * 3072
    assert n4 == elems // 2 + elems // 32 and w.weight_bytes_per_token("fp4") == n4
    assert abs(n4 / 1e9 - 1.71) < 0.01 and abs(n16 / 1e9 - 6.43) < 0.01
