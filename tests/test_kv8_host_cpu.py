"""CPU: the host side of the opt-in fp8 (e4m3) K/V cache.  The header names the two formats without an ABI bump, the new entries
are mirrored in the ctypes table, `runtime.kv_dtype` maps to the `kv_cache_dtype` keyword, sl_kv_cache_bytes counts bytes, and the
argument checks refuse what is not built (an unknown format code, fp8 with SL_F32, fp8 with head_dim 64) before any device work —
so all of this runs without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import pkg

L = pkg("_lib")
cfgm = pkg("config")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(1 << 20)          # a non-null pointer the argument checks never dereference
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _err():
    return L.lib().sl_last_error().decode()


def test_header_defines_the_kv_formats_and_keeps_abi_7():
    h = open(os.path.join(REPO, "include", "speechllm.h")).read()
    assert re.search(r"#define SL_KV_MODEL_DTYPE 0\b", h) and re.search(r"#define SL_KV_FP8_E4M3 1\b", h)
    assert re.search(r"#define SL_ABI_VERSION 7\b", h)
    assert L.lib().sl_version() == 7
    assert (L.KV_MODEL_DTYPE, L.KV_FP8_E4M3) == (0, 1)


def test_new_exports_are_mirrored():
    for name in ("sl_kv_cache_bytes", "sl_rope_kv_append_ex", "sl_attn_decode_split_ex"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)


def test_kv_format_code():
    assert L.kv_format_code(None) == L.KV_MODEL_DTYPE
    assert L.kv_format_code("fp8") == L.KV_FP8_E4M3 == L.kv_format_code(torch.float8_e4m3fn)
    for bad in ("int8", "e5m2", "model", torch.float8_e5m2, torch.float16):
        with pytest.raises(L.SpeechLLMError):
            L.kv_format_code(bad)


def test_runtime_kv_dtype_helper_and_shipped_configs():
    assert cfgm.runtime_kv_dtype(cfgm.from_dict(dict(runtime=dict(kv_dtype="fp8")))) == "fp8"
    assert cfgm.runtime_kv_dtype(cfgm.from_dict(dict(runtime=dict(kv_dtype="model")))) is None
    assert cfgm.runtime_kv_dtype(cfgm.from_dict(dict(runtime=dict(dtype="fp16")))) is None
    assert cfgm.runtime_kv_dtype(cfgm.from_dict({})) is None
    with pytest.raises(ValueError):
        cfgm.runtime_kv_dtype(cfgm.from_dict(dict(runtime=dict(kv_dtype="int8"))))
    for f in ("llama3_hubert", "llama3_whisper", "minichat_hubert", "minichat_whisper"):
        assert cfgm.runtime_kv_dtype(cfgm.load_config(os.path.join(REPO, "config", f + ".yaml"))) is None
    assert L.kv_format_code(cfgm.runtime_kv_dtype(cfgm.from_dict(dict(runtime=dict(kv_dtype="fp8"))))) == L.KV_FP8_E4M3


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_quantiser_matches_torch_on_every_16bit_value(dt):
    """sl_kv_quantize_e4m3_host runs the routine the kernels store with (one __host__ __device__ function).  Every one of the 65 536
    bit patterns of the dtype: finite values and +-inf give torch's clamp(-448, 448) -> float8_e4m3fn byte (round to nearest even,
    subnormals kept, signed zero); NaN gives the largest finite value of its sign; no byte is 0x7F / 0xFF."""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt).float().contiguous()
    out = torch.empty(65536, dtype=torch.uint8)
    assert L.lib().sl_kv_quantize_e4m3_host(x.data_ptr(), out.data_ptr(), 65536) == 0
    nan = torch.isnan(x)
    want = x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(out[~nan], want[~nan]), int((out[~nan] != want[~nan]).sum())
    assert bool(((out[nan] & 0x7F) == 0x7E).all()) and not bool(((out & 0x7F) == 0x7F).any())
    assert len(torch.unique(out)) == 254


def _model(dtype=L.SL_BF16, head_dim=128, n_layers=3, n_kv=2):
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab = dtype, 256, n_layers, 2 * n_kv, n_kv, head_dim, 512, 1000
    m.rms_eps, m.rope_len = 1e-5, 512
    layers = (L.LlamaLayer * n_layers)()
    m.layers = layers
    m._keep = layers
    for f in ("embed", "lm_head", "final_norm", "rope_cos", "rope_sin"):
        setattr(m, f, FAKE.value)
    return m


def test_kv_cache_bytes():
    lib = L.lib()
    m = _model()
    slots, ctx = 7, 448
    n = m.n_layers * slots * m.n_kv_heads * ctx * m.head_dim
    assert lib.sl_kv_cache_bytes(C.byref(m), slots, ctx, L.KV_FP8_E4M3) == n
    assert lib.sl_kv_cache_bytes(C.byref(m), slots, ctx, L.KV_MODEL_DTYPE) == 2 * n
    m16 = _model(dtype=L.SL_F16)
    assert lib.sl_kv_cache_bytes(C.byref(m16), slots, ctx, L.KV_FP8_E4M3) == n
    m32 = _model(dtype=L.SL_F32)
    assert lib.sl_kv_cache_bytes(C.byref(m32), slots, ctx, L.KV_MODEL_DTYPE) == 4 * n
    assert lib.sl_kv_cache_bytes(C.byref(m32), slots, ctx, L.KV_FP8_E4M3) == 0 and "float32" in _err()
    assert lib.sl_kv_cache_bytes(C.byref(m), slots, ctx, 2) == 0 and "format 2" in _err()
    assert lib.sl_kv_cache_bytes(C.byref(_model(head_dim=64)), slots, ctx, L.KV_FP8_E4M3) == 0 and "head_dim" in _err()
    # more than 2^32 bytes: 2 048 slots x 448 positions of Llama-3.2-3B (28 layers, 8 kv heads)
    big = _model(n_layers=28, n_kv=8)
    assert lib.sl_kv_cache_bytes(C.byref(big), 2048, 448, L.KV_FP8_E4M3) == 28 * 2048 * 8 * 448 * 128


CASES = [("format 2", L.SL_BF16, 128, 2, ERR_ARG, "format 2"),
         ("fp8 with SL_F32", L.SL_F32, 128, 1, ERR_UNSUPPORTED, "float32"),
         ("fp8 with head_dim 64", L.SL_BF16, 64, 1, ERR_UNSUPPORTED, "head_dim")]


@pytest.mark.parametrize("what,dtype,D,fmt,rc,word", CASES, ids=[c[0] for c in CASES])
def test_rope_kv_append_ex_refuses(what, dtype, D, fmt, rc, word):
    got = L.lib().sl_rope_kv_append_ex(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 4, 2, D, 64, dtype, fmt, None)
    assert got == rc and word in _err(), (got, _err())


@pytest.mark.parametrize("what,dtype,D,fmt,rc,word", CASES, ids=[c[0] for c in CASES])
def test_attn_decode_split_ex_refuses(what, dtype, D, fmt, rc, word):
    got = L.lib().sl_attn_decode_split_ex(FAKE, 512, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 4, 2, D, 64, C.c_float(0.1), dtype, fmt, 0, None)
    assert got == rc and word in _err(), (got, _err())


@pytest.mark.parametrize("what,dtype,D,fmt,rc,word", CASES, ids=[c[0] for c in CASES])
def test_llama_decode_step_refuses(what, dtype, D, fmt, rc, word):
    m = _model(dtype=dtype, head_dim=D)
    kv = L.KVCache()
    kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx, kv.shared_prefix, kv.reserved = FAKE.value, FAKE.value, 4, 64, 0, fmt
    got = L.lib().sl_llama_decode_step(C.byref(m), C.byref(kv), FAKE, FAKE, 2, FAKE, FAKE, 1 << 20, None)
    assert got == rc and word in _err(), (got, _err())


@pytest.mark.parametrize("what,dtype,D,fmt,rc,word", CASES[:2], ids=[c[0] for c in CASES[:2]])
def test_gemm_rope_kv_epilogue_refuses(what, dtype, D, fmt, rc, word):
    """sl_gemm_fused.reserved carries the same code for the SL_ACT_ROPE_KV epilogue (its head_dim is 128 by construction)"""
    a = L.GemmArgs()
    a.A = a.W = a.C = FAKE.value
    a.M, a.N, a.K, a.batch, a.dtype, a.act, a.w_layout = 4, (4 + 2 * 2) * 128, 256, 1, dtype, L.ACT_ROPE_KV, L.W_PACKED
    a.lda = a.ldw = 256
    a.ldc = 4 * 128
    f = L.GemmFused()
    for name in ("rope_cos", "rope_sin", "tok_pos", "tok_seq", "k_cache", "v_cache"):
        setattr(f, name, FAKE.value)
    f.n_heads, f.n_kv_heads, f.max_ctx, f.reserved = 4, 2, 64, fmt
    got = L.lib().sl_gemm_fused_decode(C.byref(a), C.byref(f), None)
    assert got == rc and word in _err(), (got, _err())


def test_model_constructor_refuses_fp8_with_float32():
    llama_mod, weights = pkg("audio_llama"), pkg("weights")
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128)
    with pytest.raises(L.SpeechLLMError, match="float32"):
        llama_mod.AudioLlamaForCausalLM(arch, {}, torch_dtype=torch.float32, kv_cache_dtype="fp8")
    m = llama_mod.AudioLlamaForCausalLM(arch, {}, torch_dtype=torch.bfloat16, kv_cache_dtype=torch.float8_e4m3fn)
    assert m.kv_format == L.KV_FP8_E4M3
    assert llama_mod.AudioLlamaForCausalLM(arch, {}, torch_dtype=torch.float16).kv_format == L.KV_MODEL_DTYPE
