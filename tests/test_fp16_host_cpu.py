"""CPU: the host side of the fp16 compute mode (SL_F16).  The C header names the dtype without an ABI bump, the Python layer maps
torch.float16 / `runtime.dtype: fp16` to it, training refuses it at construction, and the training-only C entries refuse it in
their argument checks (before any device work, so this runs without a GPU)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import pkg

L = pkg("_lib")
cfgm = pkg("config")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(1 << 20)          # a non-null pointer the argument checks never dereference


def test_header_has_sl_f16_and_keeps_abi_7():
    h = open(os.path.join(REPO, "include", "speechllm.h")).read()
    assert re.search(r"enum sl_dtype \{ SL_F32 = 0, SL_BF16 = 1, SL_F16 = 2 \};", h)
    assert re.search(r"#define SL_ABI_VERSION 7\b", h)
    assert L.lib().sl_version() == 7
    assert L.SL_F16 == 2


def test_dtype_code_maps_float16():
    assert L.dtype_code(torch.float16) == 2 == L.SL_F16
    assert L.dtype_code(torch.bfloat16) == L.SL_BF16 and L.dtype_code(torch.float32) == L.SL_F32
    with pytest.raises(L.SpeechLLMError):
        L.dtype_code(torch.float64)
    assert L.is16(torch.float16) and L.is16(torch.bfloat16) and not L.is16(torch.float32)


@pytest.mark.parametrize("name,dt", [("fp16", torch.float16), ("bf16", torch.bfloat16), ("fp32", torch.float32)])
def test_runtime_dtype_helper(name, dt):
    assert cfgm.runtime_dtype(cfgm.from_dict(dict(runtime=dict(dtype=name)))) == dt


def test_runtime_dtype_default_and_shipped_configs():
    assert cfgm.runtime_dtype(cfgm.from_dict({})) == torch.bfloat16
    with pytest.raises(ValueError):
        cfgm.runtime_dtype(cfgm.from_dict(dict(runtime=dict(dtype="half"))))
    for f in ("llama3_hubert", "llama3_whisper", "minichat_hubert", "minichat_whisper"):
        assert cfgm.runtime_dtype(cfgm.load_config(os.path.join(REPO, "config", f + ".yaml"))) == torch.bfloat16


def test_trainer_refuses_float16_at_construction():
    trainer_mod = pkg("trainer")
    args = SimpleNamespace(run_name="fp16", gpu_idx=0)
    with pytest.raises(L.SpeechLLMError, match="loss scaler"):
        trainer_mod.Trainer(args, cfgm.from_dict({}), torch.device("cpu"), dtype=torch.float16)
    training = pkg("training")
    with pytest.raises(L.SpeechLLMError):
        training.check_training_dtype(torch.float16)
    training.check_training_dtype(torch.bfloat16)
    training.check_training_dtype(torch.float32)


def _err():
    return L.lib().sl_last_error().decode()


def test_gemm_accepts_f16_in_its_argument_checks():
    a = L.GemmArgs()
    a.M, a.N, a.K, a.batch, a.dtype = 4, 4, 12, 1, L.SL_F16     # K not a multiple of 8: the shape check, not the dtype check, refuses it
    assert L.lib().sl_gemm(C.byref(a), None) == -1 and "multiple of 8" in _err()


@pytest.mark.parametrize("feature", ["trans_a", "trans_w", "post_op", "colsum_out", "aux_out"])
def test_gemm_ex_training_features_refuse_f16(feature):
    a = L.GemmArgs()
    a.M, a.N, a.K, a.batch, a.dtype = 128, 128, 128, 1, L.SL_F16
    a.lda = a.ldw = a.ldc = 128
    ex = L.GemmEx()
    ex.w_mod = 1
    if feature in ("trans_a", "trans_w", "post_op"):
        setattr(ex, feature, 1)
    else:
        setattr(ex, feature, FAKE.value)
    assert L.lib().sl_gemm_ex(C.byref(a), C.byref(ex), None) == -1
    assert "SL_F16" in _err()


def test_attention_backward_refuses_f16():
    a = L.AttnBwdArgs()
    for f in ("q", "k", "v", "out", "d_out", "dq", "dk", "dv", "lse", "delta", "cu_q", "cu_k", "klen"):
        setattr(a, f, FAKE.value)
    a.nseq, a.max_qlen, a.max_klen, a.n_tok_q, a.n_heads, a.n_kv_heads, a.head_dim, a.dtype = 1, 8, 8, 8, 2, 2, 64, L.SL_F16
    assert L.lib().sl_attn_bwd(C.byref(a), None) == -1
    assert "training dtype" in _err()


def test_training_tapes_refuse_f16():
    lib = L.lib()
    ec = L.EncStackCfg()
    ec.dtype, ec.hidden, ec.n_heads, ec.ffn, ec.n_layers = L.SL_F16, 128, 2, 256, 1
    ec.cu = ec.klen = ec.skip = ec.seeds = FAKE.value
    layers, saved, grads = (L.HubertLayer * 1)(), (L.EncLayerSaved * 1)(), (L.EncLayerGrads * 1)()
    x_out = C.c_void_p()
    assert lib.sl_encoder_stack_train_fwd(layers, C.byref(ec), FAKE, saved, C.byref(x_out), FAKE, 1 << 20, None) == -1
    assert "training dtype" in _err()
    assert lib.sl_encoder_stack_train_bwd(layers, C.byref(ec), saved, grads, 0, 1, FAKE, FAKE, 1 << 20, None) == -1
    assert "training dtype" in _err()
    lc = L.LlamaStackCfg()
    lc.dtype, lc.hidden, lc.n_heads, lc.n_kv_heads, lc.head_dim, lc.ffn, lc.n_layers = L.SL_F16, 256, 2, 1, 128, 512, 1
    lc.cu = lc.klen = lc.pos = lc.rope_cos = lc.rope_sin = FAKE.value
    llayers, lsaved = (L.LlamaTrainLayer * 1)(), (L.LlamaLayerSaved * 1)()
    hidden = (C.c_void_p * 2)(FAKE.value, FAKE.value)
    assert lib.sl_llama_stack_train_fwd(llayers, C.byref(lc), hidden, lsaved, FAKE, 1 << 20, None) == -1
    assert "training dtype" in _err()
    assert lib.sl_llama_stack_train_bwd(llayers, C.byref(lc), hidden, lsaved, hidden, FAKE, FAKE, 1 << 20, None) == -1
    assert "training dtype" in _err()


@pytest.mark.parametrize("entry", ["sl_gelu_bwd", "sl_axpby"])
def test_elementwise_training_entries_refuse_f16(entry):
    lib = L.lib()
    if entry == "sl_gelu_bwd":
        rc = lib.sl_gelu_bwd(FAKE, FAKE, FAKE, 64, L.SL_F16, None)
    else:
        rc = lib.sl_axpby(FAKE, FAKE, C.c_float(1.0), C.c_float(1.0), 64, L.SL_F16, None)
    assert rc == -1 and "dtype" in _err()
