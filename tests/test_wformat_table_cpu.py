"""CPU: the weight formats' one table.  sl_weight_format_info gives, for the four SL_WDEC_* codes, the reduction-length multiple, the row
limit and the w_layout that the library's own checks run on, and refuses every other code naming the four; the Python table
(_lib.WEIGHT_FORMATS) has those four codes, takes its numbers from the C side, and maps every option spelling to the code it always
mapped to; weight_bytes_per_token of a quantised format is the sum of the library's own image-byte functions."""
import ctypes as C

import pytest
import torch

from conftest import pkg

L = pkg("_lib")
weights = pkg("weights")
ERR_ARG = -1


def _info(code):
    k, rows, layout = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rc = L.lib().sl_weight_format_info(code, C.byref(k), C.byref(rows), C.byref(layout))
    return rc, (k.value, rows.value, layout.value)


def test_format_info_of_the_four_codes():
    lib = L.lib()
    want = {L.WDEC_MODEL_DTYPE: (1, 0, L.W_PACKED), L.WDEC_E4M3: (64, lib.sl_w8_max_rows(), L.W_PACKED_E4M3),
            L.WDEC_MXFP4: (128, lib.sl_w4_max_rows(), L.W_PACKED_MXFP4), L.WDEC_MX_LINEAR: (128, 0, -1)}
    assert sorted(want) == [0, 1, 4, 5]
    for code, row in want.items():
        assert _info(code) == (0, row), code
    assert lib.sl_weight_format_info(L.WDEC_MXFP4, None, None, None) == 0      # any out pointer may be NULL


@pytest.mark.parametrize("code", [-1, 2, 3, 6])
def test_format_info_refuses_what_is_no_format(code):
    rc, out = _info(code)
    assert rc == ERR_ARG and out == (-7, -7, -7)
    msg = L.lib().sl_last_error().decode()
    for needle in ("0 = model dtype", "1 = e4m3", "4 = MXFP4", "5 = MX linears"):
        assert needle in msg, msg


def test_python_table_has_the_four_codes_and_the_c_numbers():
    assert sorted(L.WEIGHT_FORMATS) == [0, 1, 4, 5]
    for code, f in L.WEIGHT_FORMATS.items():
        assert f.code == code and (f.k_multiple, f.max_rows, f.w_layout) == _info(code)[1]


def test_option_spellings_map_to_the_codes_they_always_did():
    for spelling, code in ((None, 0), ("fp8", 1), (torch.float8_e4m3fn, 1), ("mxfp4", 4), ("fp4", 4)):
        assert L.weight_format_code(spelling) == code
    for spelling, code in ((None, 0), ("mx", 5), ("mxfp8_mxfp4", 5)):
        assert L.linear_format_code(spelling) == code
    for bad in ("mx", "mxfp8_mxfp4", "int8", "model", torch.float8_e5m2, torch.float16, 1):
        with pytest.raises(L.SpeechLLMError):
            L.weight_format_code(bad)
    for bad in ("fp8", "mxfp4", "fp4", "int8", torch.float8_e4m3fn, 5):
        with pytest.raises(L.SpeechLLMError):
            L.linear_format_code(bad)


@pytest.mark.parametrize("fmt,fn", [("fp8", "sl_w8_image_bytes"), ("mxfp4", "sl_w4_image_bytes")])
def test_weight_bytes_per_token_is_the_sum_of_the_c_image_bytes(fmt, fn):
    w = weights.LlamaDeviceWeights.__new__(weights.LlamaDeviceWeights)
    w.arch = weights.LlamaArch(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=512,
                               vocab_size=320)
    w.dtype = torch.bfloat16
    img = getattr(L.lib(), fn)
    layer = img(3 * 256, 256) + img(256, 256) + img(2 * 512, 256) + img(256, 512)      # qkv, o, gate/up, down
    assert layer > 0 and w.weight_bytes_per_token(fmt) == 2 * layer + img(320, 256)
