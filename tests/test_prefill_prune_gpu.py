"""sl_llama_prefill's final layer computes o / FFN for each sequence's last row only (runtime.hip llama_layer tail_rows); with
SL_PREFILL_PRUNE_LAST=0 it computes them for every row.  Both forms must leave the same logits and the same K / V cache, bit for bit."""
import ctypes as C

import pytest
import torch

from conftest import pkg
from oracle.golden_cfgs import TINY_LLAMA, TINY_MHA

pytestmark = pytest.mark.gpu

ri = pkg("random_init")
llama_mod = pkg("audio_llama")
weights = pkg("weights")
utils = pkg("utils")
L = pkg("_lib")

DEV = "cuda:0"


@pytest.fixture
def tuning(monkeypatch):
    """Set an SL_* tuning switch and re-read the library's table; restored in the finalizer."""
    def set_(name, value):
        monkeypatch.setenv(name, value)
        L.lib().sl_tuning_reload()

    yield set_
    monkeypatch.undo()
    L.lib().sl_tuning_reload()


def llama_arch(c):
    return weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                             c.intermediate_size, c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling,
                             c.tie_word_embeddings, tuple(c.eos_token_ids), c.pad_token_id)


def prefill(llm, x, lens, shared_prefix):
    """Last-position fp32 logits and the K / V cache after sl_llama_prefill over a packed prompt buffer (x is consumed)."""
    w, lib, B = llm._dev(), L.lib(), len(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    if llm._kv is not None:
        llm._kv[0].zero_(); llm._kv[1].zero_()
    kv = llm._kv_cache(B, shared_prefix)
    ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(w.struct), x.shape[0], B, 1))
    logits = torch.zeros((B, llm.arch.vocab_size), device=DEV, dtype=torch.float32)
    ctx = torch.zeros(B, device=DEV, dtype=torch.int32)
    L.check(lib.sl_llama_prefill(C.byref(w.struct), C.byref(kv), x.data_ptr(), (C.c_int32 * (B + 1))(*cu), B, logits.data_ptr(), ctx.data_ptr(),
                                 None, ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
    torch.cuda.synchronize()
    return logits.clone(), ctx.clone(), llm._kv[0].clone(), llm._kv[1].clone()


def both_forms_agree(llm, prompts, shared_prefix, tuning):
    lens = [int(p.shape[0]) for p in prompts]
    x = torch.cat(prompts).to(DEV, llm.dtype).contiguous()
    got = {}
    for mode in ("0", "1"):
        tuning("SL_PREFILL_PRUNE_LAST", mode)
        got[mode] = prefill(llm, x.clone(), lens, shared_prefix)
    full, pruned = got["0"], got["1"]
    assert torch.isfinite(full[0]).all() and float(full[0].abs().max()) > 0
    assert torch.equal(pruned[1].cpu(), torch.tensor(lens, dtype=torch.int32))
    nd = int((pruned[0] != full[0]).sum())
    print(f"B={len(lens)} rows={sum(lens)} prefix={shared_prefix} {llm.dtype}: {nd} logits differ")
    assert torch.equal(pruned[0], full[0])
    assert torch.equal(pruned[2], full[2]) and torch.equal(pruned[3], full[3])


@pytest.mark.parametrize("shared_prefix", [0, 11])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("cfg", [TINY_LLAMA, TINY_MHA], ids=["tiny_gqa", "tiny_mha"])
def test_pruned_final_layer_tiny_model(cfg, dtype, shared_prefix, tuning):
    """Ragged lengths from 1 tail row to 140, 40 sequences (tiled GEMM range) and 3 sequences (skinny range), with and without a
    shared prompt prefix."""
    llm = llama_mod.AudioLlamaForCausalLM(llama_arch(cfg), dict(ri.llama_state_dict(cfg, seed=35)), torch_dtype=dtype, device=DEV, max_ctx=256)
    gen = torch.Generator().manual_seed(12)
    pre = torch.randn(11, cfg.hidden_size, generator=gen) * 0.05
    tails = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in (9, 140, 14, 5, 77, 30, 21, 1)]
    for B in (40, 3):
        prompts = [torch.cat([pre, tails[b % len(tails)] * (1.0 + 0.01 * (b // len(tails)))]) for b in range(B)]
        both_forms_agree(llm, prompts, shared_prefix, tuning)


@pytest.mark.parametrize("shared_prefix", [0, 9])
def test_pruned_final_layer_full_depth_llama32_3b(shared_prefix, tuning):
    """Llama-3.2-3B shape at full depth in bf16 (the benchmark's weights): 130 ragged prompts of 21 to 137 rows, about 9 000 rows, so
    the full pass runs its products on the 256 x 256 tiles and the pruned one must be held to them by the family pin."""
    import bench
    larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
    sd = bench.gpu_llama_state_dict(larch, 0, torch.device(DEV))
    llm = llama_mod.AudioLlamaForCausalLM(larch, sd, torch_dtype=torch.bfloat16, device=DEV, max_ctx=192, max_batch=130)
    del sd
    gen = torch.Generator().manual_seed(21)
    pre = torch.randn(9, larch.hidden_size, generator=gen) * 0.02
    tail_lens = (128, 51, 16, 90, 12, 70)
    prompts = [torch.cat([pre, torch.randn(tail_lens[b % len(tail_lens)], larch.hidden_size, generator=gen) * 0.02]) for b in range(130)]
    both_forms_agree(llm, prompts, shared_prefix, tuning)
    del llm
    torch.cuda.empty_cache()
