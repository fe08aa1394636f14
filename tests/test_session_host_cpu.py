"""No GPU: the host side of multi-turn sessions — the new exports and their ctypes signatures, KVSession's bookkeeping from synthetic id
matrices, the follow-up templates against the committed tokenizers, and the refusals that need no device."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch

from conftest import GOLDEN, REPO, pkg

L = pkg("_lib")
utils = pkg("utils")
llama_mod = pkg("audio_llama")
weights = pkg("weights")
KVSession = llama_mod.KVSession

NEW_EXPORTS = ["sl_attn_fwd_past", "sl_llama_prefill_cont", "sl_generate_workspace_bytes_cont", "sl_generate_cont"]
HDR = open(os.path.join(REPO, "include", "speechllm.h")).read()


def test_exports_signatures_and_version():
    lib = L.lib()
    for name in NEW_EXPORTS:
        assert name in L.EXPORTS and getattr(lib, name).argtypes is not None
        assert re.search(r"\b%s\(" % name, HDR), name
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_EXPORTS:
        assert re.search(r" T %s$" % name, out, re.M), name
    # the entries are additions: no signature changed, so the version stays where every other suite pins it (the header: "bumps on any signature change")
    assert lib.sl_version() == 7 and re.search(r"#define SL_ABI_VERSION 7\b", HDR)
    assert len(lib.sl_generate_cont.argtypes) == len(lib.sl_generate_sc.argtypes) + 2
    assert len(lib.sl_llama_prefill_cont.argtypes) == 12 and len(lib.sl_attn_fwd_past.argtypes) == 8
    for words in ("history starts EMPTY", "compact must be 0", "past_s + len_s + g_s - 1"):
        assert words in HDR, words


def test_refusals_of_the_entries_without_a_device():
    lib = L.lib()
    a = L.AttnArgs()
    fake = 1 << 20
    a.q = a.k = a.v = a.out = a.cu_q = a.cu_k = a.klen = fake
    a.nseq, a.max_qlen, a.n_heads, a.n_kv_heads, a.head_dim, a.causal, a.dtype = 1, 4, 4, 2, 128, 1, L.SL_BF16
    a.q_row_stride = a.k_row_stride = a.v_row_stride = a.o_row_stride = 1024
    a.q_head_stride = a.k_head_stride = a.v_head_stride = a.o_head_stride = 128
    assert lib.sl_attn_fwd_past(C.byref(a), fake, fake, fake, fake, 64, 2, None) == -1 and b"format" in lib.sl_last_error()
    a.dtype = L.SL_F32
    assert lib.sl_attn_fwd_past(C.byref(a), fake, fake, fake, fake, 64, 1, None) == -3
    a.dtype, a.head_dim = L.SL_F16, 64
    assert lib.sl_attn_fwd_past(C.byref(a), fake, fake, fake, fake, 64, 0, None) == -3
    a.head_dim, a.causal = 128, 0
    assert lib.sl_attn_fwd_past(C.byref(a), fake, fake, fake, fake, 64, 0, None) == -3
    # sl_generate_cont: compaction on a kept cache, a slot that is not the row's index
    o = L.GenerateOpts()
    o.max_new_tokens, o.compact = 4, 1
    past, slot, cu = (C.c_int32 * 1)(5), (C.c_int32 * 1)(2), (C.c_int32 * 2)(0, 3)
    m, kv = L.LlamaModel(), L.KVCache()
    assert lib.sl_generate_cont(C.byref(m), C.byref(kv), fake, cu, 1, C.byref(o), None, None, fake, 0, None, None, None, past, None) == -1
    assert b"compact" in lib.sl_last_error()
    o.compact = 0
    assert lib.sl_generate_cont(C.byref(m), C.byref(kv), fake, cu, 1, C.byref(o), None, None, fake, 0, None, None, None, past, slot) == -3
    assert b"slot" in lib.sl_last_error()
    past[0] = -1
    assert lib.sl_generate_cont(C.byref(m), C.byref(kv), fake, cu, 1, C.byref(o), None, None, fake, 0, None, None, None, past, None) == -1
    assert b"negative" in lib.sl_last_error()


EOS, PAD = 9, 0


@pytest.mark.parametrize("name,row,budget,g", [
    ("eos mid-row", [4, 5, EOS, PAD, PAD, PAD], None, 3),
    ("eos in the first column", [EOS, PAD, PAD, PAD, PAD, PAD], None, 1),
    ("budget exhausted without eos", [4, 5, 6, 7, 8, 3], None, 6),
    ("row limit without eos, pads behind it", [4, 5, 6, 7, PAD, PAD], 4, 4),
    ("all-pad tail where the pad is the eos", [4, EOS, EOS, EOS, EOS, EOS], None, 2),
    ("eos at the row limit", [4, 5, EOS, PAD, PAD, PAD], 3, 3),
])
def test_kvsession_bookkeeping(name, row, budget, g):
    s = KVSession(2, 64)
    assert s.fresh and s.pending_id == [None, None] and s.k is None
    s.valid_len = [10, 0]
    other = [1, 2, 3, 4, 5, 6]
    s.advance([5, 7], torch.tensor([row, other]), eos_ids=[EOS], budgets=None if budget is None else [budget, 6])
    assert s.valid_len == [10 + 5 + g - 1, 0 + 7 + 6 - 1], name
    assert s.pending_id == [row[g - 1], 6] and s.turns == 1 and not s.fresh
    s.advance([3, 3])      # a forward(): rows only, nothing pending
    assert s.valid_len == [10 + 5 + g - 1 + 3, 15] and s.pending_id == [None, None]
    with pytest.raises(L.SpeechLLMError):
        s.advance([1], torch.tensor([row]))
    with pytest.raises(L.SpeechLLMError):
        s.check_room([64, 1])
    with pytest.raises(L.SpeechLLMError):
        s.check_room([1, 1], 64)
    s.check_room([1, 1], 8)


def _tokenizer(family):
    transformers = pytest.importorskip("transformers")
    name = {"llama3": "Llama-3.2-3B-Instruct", "minichat": "MiniChat-2-3B"}[family]
    return transformers.AutoTokenizer.from_pretrained(os.path.join(GOLDEN, "tokenizers", name), use_fast=(family == "llama3"))


@pytest.mark.parametrize("family,llm_type", [("llama3", utils.LLAMA_ID), ("minichat", utils.MINICHAT_ID)])
def test_follow_up_template_ids(family, llm_type):
    text = "what did she say about the budget?"
    eot, header, suffix = {"llama3": ("<|eot_id|>", "<|start_header_id|>user<|end_header_id|>\n\n", utils.LLAMA_PROMPT_SUFFIX),
                           "minichat": ("</s>", "[|User|]", utils.MINICHAT_PROMPT_SUFFIX)}[family]
    assert utils.follow_up_prompt(llm_type, text) == eot + header + text + suffix
    assert utils.follow_up_prompt(llm_type, text, drop_eot=True) == header + text + suffix
    tok = _tokenizer(family)
    full = utils.follow_up_ids(tok, llm_type, text).tolist()
    cut = utils.follow_up_ids(tok, llm_type, text, drop_eot=True).tolist()
    eot_id = tok.convert_tokens_to_ids(eot)
    bos = tok.bos_token_id
    assert bos is not None and bos not in full and bos not in cut, "a turn in the middle of a sequence carries no BOS"
    assert full[0] == eot_id and full[1] != eot_id, "the template opens with exactly one eot"
    assert cut[0] != eot_id, "pending eot: the template's own is dropped"
    # behind the leading eot the two are the same ids, and they end with the ids of the prompt suffix (the suffix's own BOS dropped)
    suf = tok(suffix, return_tensors="pt").input_ids[0].tolist()
    suf = suf[1:] if suf[0] == bos else suf
    assert full[-len(suf):] == suf and cut[-len(suf):] == suf
    if family == "llama3":
        assert full[1:] == cut
    rec = json.load(open(os.path.join(GOLDEN, "tokenizers", "tokenizer_ids.json")))[family]
    assert tok(rec["strings"]["suffix"], return_tensors="pt").input_ids[0].tolist() == rec["ids"]["suffix"]


def test_python_refusals_without_a_device():
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
    llm = llama_mod.AudioLlamaForCausalLM(arch, {}, torch_dtype=torch.bfloat16, max_ctx=32)
    sess = KVSession(2, 32, L.KV_MODEL_DTYPE, torch.zeros(1, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.bfloat16))
    x = torch.zeros((8, 256), dtype=torch.bfloat16)
    with pytest.raises(L.SpeechLLMError, match="num_beams"):
        llm.generate(inputs_embeds=x.view(2, 4, 256), max_new_tokens=4, past_key_values=sess, num_beams=2)
    with pytest.raises(L.SpeechLLMError, match="num_return_sequences"):
        llm.generate(inputs_embeds=x.view(2, 4, 256), max_new_tokens=4, past_key_values=sess, do_sample=True, num_return_sequences=2)
    with pytest.raises(L.SpeechLLMError, match="compact"):
        llm.generate_packed(x, [4, 4], 4, session=sess, compact=True)
    with pytest.raises(L.SpeechLLMError, match="max_ctx"):
        llm.generate_packed(x, [4, 4], 29, session=sess)
    sess.valid_len = [20, 3]
    with pytest.raises(L.SpeechLLMError, match="max_ctx"):      # 20 past + 4 rows + 9 new tokens > 32
        llm.generate_packed(x, [4, 4], 9, session=sess)
    with pytest.raises(L.SpeechLLMError, match="KVSession"):
        llm.generate_packed(x, [4, 4], 4, session=object())
    with pytest.raises(L.SpeechLLMError, match="sequences"):
        llm.generate_packed(x[:4], [4], 4, session=sess)
    with pytest.raises(L.SpeechLLMError, match="kv_cache_dtype"):
        llm.generate_packed(x, [4, 4], 4, session=KVSession(2, 32, L.KV_FP8_E4M3, torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8)))
