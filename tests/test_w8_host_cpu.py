"""CPU: the host side of the opt-in fp8 (e4m3) decode weights.  The header names the new layout and the decode-weight formats without
an ABI bump, the new entries are mirrored in the ctypes table, the host packer (the routine the device packer runs) is held byte for
byte against a reference written here in torch — scales, bytes, layout, padding — and every entry refuses what is not built (float32,
K % 64 != 0, an unknown layout, more rows than sl_w8_max_rows()) before any device work, so all of this runs without a GPU."""
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
F8 = torch.float8_e4m3fn
F16, BF16 = torch.float16, torch.bfloat16


def _err():
    return L.lib().sl_last_error().decode()


def test_header_defines_the_layout_and_the_formats_and_keeps_abi_7():
    h = open(os.path.join(REPO, "include", "speechllm.h")).read()
    assert re.search(r"#define SL_W_PACKED_E4M3 2\b", h)
    assert re.search(r"#define SL_WDEC_MODEL_DTYPE 0\b", h) and re.search(r"#define SL_WDEC_E4M3\s+1\b", h)
    assert re.search(r"#define SL_ABI_VERSION 7\b", h)
    assert L.lib().sl_version() == 7
    assert (L.W_ROWMAJOR, L.W_PACKED, L.W_PACKED_E4M3) == (0, 1, 2) and (L.WDEC_MODEL_DTYPE, L.WDEC_E4M3) == (0, 1)


def test_new_exports_are_mirrored():
    for name in ("sl_w8_image_bytes", "sl_pack_weight_e4m3", "sl_pack_weight_e4m3_host", "sl_w8_max_rows"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().sl_w8_max_rows() == 26          # the packed skinny range (SL_STREAM_MIN_M unset)


def test_image_bytes():
    lib = L.lib()
    assert lib.sl_w8_image_bytes(16, 64) == 16 * 64 + 4 * 16
    assert lib.sl_w8_image_bytes(40, 192) == 48 * 192 + 4 * 48
    assert lib.sl_w8_image_bytes(1000, 256) == 1008 * 256 + 4 * 1008
    assert lib.sl_w8_image_bytes(128256, 3072) == 128256 * 3072 + 4 * 128256
    for n, k in ((0, 64), (16, 0), (16, 96), (-1, 64)):
        assert lib.sl_w8_image_bytes(n, k) == 0 and "sl_w8_image_bytes" in _err()


# ------------------------------------------------------------------------------------------------------------------------------
# the packer against the format's definition
# ------------------------------------------------------------------------------------------------------------------------------
def weight_rows(N, K, dt, seed=0):
    """(N, K) test weight in dt: rows scaled by 2^(n % 9 - 4); row 0 all zero; row 1 holds every finite e4m3 value it has room for
    with amax exactly 448 (scale exactly 1: the values survive unchanged); row 2 one outlier among tiny values (the rest goes to
    e4m3 subnormals or zero); row 3, fp16 only, values near 65 504."""
    g = torch.Generator().manual_seed(1000 + seed)
    w = torch.randn(N, K, generator=g) * (2.0 ** (torch.arange(N) % 9 - 4).float())[:, None]
    w[0] = 0
    fin = torch.tensor([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=torch.uint8).view(F8).float()
    fin = fin[torch.randperm(fin.numel(), generator=g)]
    w[1] = fin.repeat((K + fin.numel() - 1) // fin.numel())[:K]
    w[1, 5] = 448.0
    w[2] = torch.randn(K, generator=g) * 3e-5
    w[2, K // 2] = -7.0
    if dt == F16:
        w[3] = 65504.0 - 32.0 * torch.randint(0, 64, (K,), generator=g).float()
        w[3, 1] = -65504.0
    return w.to(dt)


def ref_image(w):
    """the format, written out: (bytes of the image (Np*K,), scales (Np,), natural-order bytes (Np, K)) on the CPU"""
    N, K = w.shape
    Np = (N + 15) // 16 * 16
    amax = w.float().abs().amax(1)
    s = torch.ones(Np, dtype=torch.float32)
    s[:N] = torch.where(amax == 0, torch.ones_like(amax), amax / 448)
    b = torch.zeros(Np, K, dtype=torch.uint8)
    b[:N] = (w.float() / s[:N, None]).clamp(-448, 448).to(F8).view(torch.uint8)
    f = torch.arange(Np // 16)[:, None, None, None]
    j = torch.arange(K // 64)[None, :, None, None]
    lane = torch.arange(64)[None, None, :, None]
    e = torch.arange(8)[None, None, None, :]
    rows, cols = 16 * f + (lane & 15), 64 * j + 8 * (lane >> 4) + e
    img = torch.cat([b[rows, cols], b[rows, cols + 32]], dim=-1)          # (Np/16, K/64, 64, 16)
    return img.reshape(-1), s, b


def split_image(img, N, K):
    Np = (N + 15) // 16 * 16
    return img[:Np * K], img[Np * K:].clone().view(torch.float32)


SHAPES = [(16, 64), (40, 192), (1000, 256)]


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_host_packer_matches_the_format_byte_for_byte(dt, N, K):
    w = weight_rows(N, K, dt)
    want_b, want_s, nat = ref_image(w)
    img = ops.pack_weight_e4m3(w)                       # CPU tensor: sl_pack_weight_e4m3_host
    assert img.numel() == L.lib().sl_w8_image_bytes(N, K)
    got_b, got_s = split_image(img, N, K)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)), "scales differ (bit for bit)"
    assert torch.equal(got_b, want_b), f"{int((got_b != want_b).sum())} image bytes differ"
    assert not bool(((got_b & 0x7F) == 0x7F).any()), "a NaN byte (0x7F / 0xFF) in the image"
    Np = (N + 15) // 16 * 16
    b2, s2 = ops.w8_image_parts(img, N, K)               # the inverse the Python surface uses
    assert torch.equal(b2, nat) and torch.equal(s2, want_s)
    assert bool((b2[N:] == 0).all()) and bool((s2[N:] == 1).all()), "padding rows: zero bytes, scale 1"
    assert float(got_s[0]) == 1.0 and bool((b2[0] == 0).all()), "the all-zero row"
    assert float(got_s[1]) == 1.0 and torch.equal(b2[1].view(F8).float(), w[1].float()), "amax = 448: scale 1, values unchanged"
    assert int((b2[2] != 0).sum()) >= 1 and int(((b2[2] & 0x78) == 0).sum()) > K // 2, "outlier row: the rest is subnormal or zero"
    assert int(b2[2, K // 2]) == 0xFE                      # the outlier itself: -448
    if dt == F16:
        assert float(got_s[3]) == float(torch.tensor(65504.0) / 448) and int(b2[3, 1]) == 0xFE


def test_host_packer_reads_a_strided_source():
    w = weight_rows(40, 192, BF16, seed=3)
    wide = torch.zeros(40, 256, dtype=BF16)
    wide[:, :192] = w
    assert torch.equal(ops.pack_weight_e4m3(wide[:, :192]), ops.pack_weight_e4m3(w))


# ------------------------------------------------------------------------------------------------------------------------------
# refusals, without a device
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [True, False])
def test_packer_refuses_float32_and_ragged_k(host):
    lib = L.lib()

    def call(N, K, dtype):
        if host:
            return lib.sl_pack_weight_e4m3_host(FAKE, K, FAKE, N, K, dtype)
        return lib.sl_pack_weight_e4m3(FAKE, K, FAKE, N, K, dtype, None)

    assert call(16, 64, L.SL_F32) == ERR_UNSUPPORTED and "float32" in _err()
    assert call(16, 96, L.SL_BF16) == ERR_ARG and "multiple of 64" in _err()
    assert call(16, 64, 7) == ERR_ARG and "dtype" in _err()
    assert call(0, 64, L.SL_F16) == ERR_ARG


def _gemm_args(M, N, K, dtype, w_layout):
    a = L.GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = FAKE.value, K, FAKE.value, K, FAKE.value, N
    a.M, a.N, a.K, a.batch, a.dtype, a.act, a.w_layout = M, N, K, 1, dtype, L.ACT_NONE, w_layout
    return a


def test_gemm_refuses_what_the_e4m3_kernels_do_not_take():
    lib = L.lib()
    rows = lib.sl_w8_max_rows()
    a = _gemm_args(rows + 1, 256, 256, L.SL_BF16, L.W_PACKED_E4M3)
    assert lib.sl_gemm(C.byref(a), None) == ERR_UNSUPPORTED and "sl_w8_max_rows" in _err() and str(rows + 1) in _err()
    f = L.GemmFused()
    assert lib.sl_gemm_fused_decode(C.byref(a), C.byref(f), None) == ERR_UNSUPPORTED and "rows" in _err()
    a = _gemm_args(4, 256, 256, L.SL_F32, L.W_PACKED_E4M3)
    assert lib.sl_gemm(C.byref(a), None) == ERR_UNSUPPORTED and "float32" in _err()
    a = _gemm_args(4, 256, 96, L.SL_F16, L.W_PACKED_E4M3)
    assert lib.sl_gemm(C.byref(a), None) == ERR_ARG and "K % 64" in _err()
    a = _gemm_args(4, 256, 256, L.SL_BF16, 3)
    assert lib.sl_gemm(C.byref(a), None) == ERR_ARG and "w_layout 3" in _err()
    a = _gemm_args(4, 256, 256, L.SL_BF16, L.W_PACKED_E4M3)
    a.act = L.ACT_GELU
    assert lib.sl_gemm(C.byref(a), None) == ERR_ARG and "GELU" in _err()


def _model(dtype=L.SL_BF16, hidden=256, ffn=512, n_layers=2, reserved=L.WDEC_E4M3):
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
def test_e4m3_model_is_refused_before_any_launch(entry):
    rows = L.lib().sl_w8_max_rows()
    assert entry(_model(dtype=L.SL_F32), 2) == ERR_UNSUPPORTED and "float32" in _err()
    assert entry(_model(), rows + 1) == ERR_UNSUPPORTED and "rows" in _err() and str(rows + 1) in _err()
    assert entry(_model(ffn=544), 2) == ERR_UNSUPPORTED and "multiple of 64" in _err() and "544" in _err()
    assert entry(_model(reserved=2), 2) == ERR_ARG and "format 2" in _err()
    m = _model()
    m.dec_fused_norm = 0
    assert entry(m, 2) == ERR_ARG and "dec_fused_norm" in _err()


# ------------------------------------------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_runtime_weight_dtype_helper_and_shipped_configs():
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="fp8")))) == "fp8"
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="model")))) is None
    assert cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(kv_dtype="fp8")))) is None
    assert cfgm.runtime_weight_dtype(cfgm.from_dict({})) is None
    with pytest.raises(ValueError):
        cfgm.runtime_weight_dtype(cfgm.from_dict(dict(runtime=dict(weight_dtype="int8"))))
    for f in ("llama3_hubert", "llama3_whisper", "minichat_hubert", "minichat_whisper"):
        assert cfgm.runtime_weight_dtype(cfgm.load_config(os.path.join(REPO, "config", f + ".yaml"))) is None
    assert L.weight_format_code("fp8") == L.WDEC_E4M3 == L.weight_format_code(F8) and L.weight_format_code(None) == L.WDEC_MODEL_DTYPE
    for bad in ("int8", "model", torch.float8_e5m2, torch.float16):
        with pytest.raises(L.SpeechLLMError):
            L.weight_format_code(bad)


def test_constructor_refusals():
    arch = weights.LlamaArch(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=512,
                             vocab_size=100)
    mk = lambda a=arch, **kw: llama_mod.AudioLlamaForCausalLM(a, {}, **kw)
    assert mk(torch_dtype=BF16, weight_dtype="fp8").weight_format == L.WDEC_E4M3
    assert mk(torch_dtype=F16, weight_dtype=F8, kv_cache_dtype="fp8").weight_format == L.WDEC_E4M3
    assert mk(torch_dtype=BF16).weight_format == L.WDEC_MODEL_DTYPE
    with pytest.raises(L.SpeechLLMError, match="float32"):
        mk(torch_dtype=torch.float32, weight_dtype="fp8")
    with pytest.raises(L.SpeechLLMError, match="pack_decode"):
        mk(torch_dtype=BF16, weight_dtype="fp8", pack_decode=False)
    odd = weights.LlamaArch(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=544,
                            vocab_size=100)
    with pytest.raises(L.SpeechLLMError, match="multiple of 64"):
        mk(odd, torch_dtype=BF16, weight_dtype="fp8")
    with pytest.raises(L.SpeechLLMError):
        mk(torch_dtype=BF16, weight_dtype="int8")
    llm = mk(torch_dtype=torch.float32)
    with pytest.raises(L.SpeechLLMError):
        llm.set_weight_dtype("fp8")
