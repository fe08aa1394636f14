"""GPU: min_p / typical_p / epsilon_cutoff / eta_cutoff end to end on TINY_LLAMA in fp32, 32 new tokens: the
greedy-degenerate settings return the greedy ids, seeds reproduce, the off values are the call without the options (ids and launches),
generate() equals a Python loop over sl_llama_decode_step + ops.sample_select_w in every form the runtime has — plain, with scores, a
compacting batch with per-row budgets, three answers per prompt, a second session turn — and a graph captured for one min_p is never
replayed for another."""
import copy
import ctypes as C

import pytest
import torch

from conftest import pkg
from oracle.golden_cfgs import TINY_LLAMA
from test_kv8_gpu import _make_llama

pytestmark = pytest.mark.gpu
L = pkg("_lib")
ops = pkg("ops")
DEV = "cuda:0"
NEW = 32
LENS = (9, 14, 5, 11)
_LLM = {}
# one non-degenerate setting of each option, and all four together
SETTINGS = {"min_p": dict(min_p=0.05), "typical_p": dict(typical_p=0.9), "epsilon_cutoff": dict(epsilon_cutoff=1e-3), "eta_cutoff": dict(eta_cutoff=2e-3),
            "all": dict(min_p=0.02, typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=1e-3)}


def _llm():
    if "llm" not in _LLM:
        llm, _ = _make_llama(TINY_LLAMA, 61, torch.float32, max_ctx=128)
        _LLM["llm"] = llm
    llm = _LLM["llm"]
    llm.generation_config.eos_token_id = None
    llm.generation_config.pad_token_id = TINY_LLAMA.pad_token_id
    return llm


def _prompts(seed=7, lens=LENS):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, TINY_LLAMA.hidden_size, generator=gen) * 0.05 for n in lens]


def _sample(seed, temperature=0.9, top_k=0, top_p=1.0, **warp):
    return dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, **warp)


def _packed(llm, prompts, sample, **kw):
    x = torch.cat(prompts).to(DEV).contiguous()
    return llm.generate_packed(x, [int(p.shape[0]) for p in prompts], NEW, use_eos=False, sample=sample, **kw)


# ------------------------------------------------------------------------------------------------ the Python loop
def _loop(llm, sample, prompts=None, first=None, scores=False, n_new=NEW):
    """sl_llama_prefill (or `first` = (logits, ctx, kv struct) of a continued call), then n_new - 1 x (sl_llama_decode_step,
    ops.sample_select_w) -> (ids (B, n_new) int32, log-probabilities or None), on the host"""
    w, lib = llm._dev(), L.lib()
    warp = {k: sample.get(k) for k in L.WARP_OFF}
    if first is None:
        B = len(prompts)
        x = torch.cat([p.to(DEV) for p in prompts]).contiguous()
        cu = [0]
        for p in prompts:
            cu.append(cu[-1] + p.shape[0])
        kv = llm._kv_cache(B)
        ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(w.struct), x.shape[0], B, 1))
        logits = torch.empty((B, llm.arch.vocab_size), device=DEV, dtype=torch.float32)
        ctx = torch.empty(B, device=DEV, dtype=torch.int32)
        L.check(lib.sl_llama_prefill(C.byref(w.struct), C.byref(kv), x.data_ptr(), (C.c_int32 * (B + 1))(*cu), B, logits.data_ptr(), ctx.data_ptr(),
                                     None, ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
    else:
        logits, ctx, kv = first
        B = logits.shape[0]
        ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(w.struct), B, B, 1))
    i32 = dict(dtype=torch.int32, device=DEV)
    unf, gen, fin, nxt = torch.ones(B, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
    out = torch.full((B, n_new), -1, **i32)
    lps = torch.zeros((B, n_new), dtype=torch.float32, device=DEV) if scores else None
    a = (sample["temperature"], sample["top_k"], sample["top_p"], sample["seed"], [], 0, False, unf)
    ops.sample_select_w(logits, *a, ctx.clone(), gen, fin, nxt, out, lps, warp)          # the prefill's token: the context length stays
    for _ in range(n_new - 1):
        L.check(lib.sl_llama_decode_step(C.byref(w.struct), C.byref(kv), nxt.data_ptr(), ctx.data_ptr(), B, logits.data_ptr(), ws.data_ptr(),
                                         ws.numel(), L.stream_ptr()), "sl_llama_decode_step")
        ops.sample_select_w(logits, *a, ctx, gen, fin, nxt, out, lps, warp)              # ... and advances here
    torch.cuda.synchronize()
    return out.cpu(), None if lps is None else lps.cpu()


# ------------------------------------------------------------------------------------------------ the tests
def test_greedy_degenerate_settings_return_the_greedy_ids():
    """fails on a build whose generate() swallows the keyword: it then samples from the whole distribution"""
    llm = _llm()
    x = torch.nn.utils.rnn.pad_sequence([p.flip(0) for p in _prompts()], batch_first=True).flip(1).to(DEV)
    mask = torch.tensor([[0] * (max(LENS) - n) + [1] * n for n in LENS], device=DEV)
    kw = dict(inputs_embeds=x, attention_mask=mask, max_new_tokens=NEW, use_eos=False)
    greedy = llm.generate(**kw)
    assert greedy.shape == (len(LENS), NEW)
    for opt in (dict(min_p=1.0), dict(epsilon_cutoff=0.999)):
        got = llm.generate(do_sample=True, seed=11, **opt, **kw)
        assert torch.equal(got, greedy), opt
    assert not torch.equal(llm.generate(do_sample=True, seed=11, **kw), greedy)      # the seed does sample where nothing cuts


@pytest.mark.parametrize("name", list(SETTINGS))
def test_seeds_reproduce_and_differ(name):
    llm, prompts = _llm(), _prompts()
    a, _ = _packed(llm, prompts, _sample(21, **SETTINGS[name]))
    b, _ = _packed(llm, prompts, _sample(21, **SETTINGS[name]))
    c, _ = _packed(llm, prompts, _sample(22, **SETTINGS[name]))
    assert torch.equal(a, b) and not torch.equal(a, c), name


def test_off_values_are_the_call_without_the_options():
    llm, prompts = _llm(), _prompts()
    base, _ = _packed(llm, prompts, _sample(31, top_k=40, top_p=0.9))
    launches = llm.last_generate_stats["decode_launches"]
    for off in (dict(L.WARP_OFF), dict(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None), dict(typical_p=1.0)):
        got, _ = _packed(llm, prompts, _sample(31, top_k=40, top_p=0.9, **off))
        assert torch.equal(got, base) and llm.last_generate_stats["decode_launches"] == launches == NEW - 1, off


@pytest.mark.parametrize("name", list(SETTINGS))
def test_generate_equals_the_step_loop_plain_and_with_scores(name):
    llm, prompts = _llm(), _prompts()
    s = _sample(41, top_k=200, **SETTINGS[name])
    want, want_lp = _loop(llm, s, prompts, scores=True)
    ids, _ = _packed(llm, prompts, s)
    assert torch.equal(ids, want), name
    ids_s, _, lps = _packed(llm, prompts, s, scores=True)
    assert torch.equal(ids_s, want) and torch.equal(lps.view(torch.int32), want_lp.view(torch.int32)), name
    assert bool((lps <= 0).all()) and bool(torch.isfinite(lps).all())


def test_a_compacting_batch_with_row_limits_equals_the_step_loop():
    """budgets finish rows one after the other and the batch walks down its ladder of row counts; a row's draws follow its index in the
    caller's batch (row_ids), so every row holds the loop's ids up to its budget and pads behind"""
    llm = _llm()
    prompts = _prompts(8, lens=(9, 14, 5, 11, 7, 6, 12, 10))
    limits = [3, 32, 5, 9, 32, 2, 17, 4]
    s = _sample(51, **SETTINGS["all"])
    want, _ = _loop(llm, s, prompts)
    ids, n_cols = _packed(llm, prompts, s, row_limits=limits, compact=True, check_every=2)
    assert llm.last_generate_stats["compactions"] >= 2 and n_cols == NEW
    pad = TINY_LLAMA.pad_token_id
    for b, n in enumerate(limits):
        assert ids[b, :n].tolist() == want[b, :n].tolist() and ids[b, n:].tolist() == [pad] * (NEW - n), b


def test_three_answers_per_prompt_are_the_draws_of_the_prompt_repeated():
    llm = _llm()
    prompts = _prompts(9, lens=(9, 14))
    s = _sample(61, **SETTINGS["min_p"])
    want, _ = _loop(llm, s, [p for p in prompts for _ in range(3)])
    ids, _ = _packed(llm, prompts, s, num_return=3)
    assert ids.shape == (6, NEW) and torch.equal(ids, want)
    assert len({tuple(r) for r in ids[:3].tolist()}) > 1                              # the answers of one prompt differ


def test_a_second_session_turn_equals_the_step_loop():
    llm = _llm()
    prompts, follow = _prompts(10, lens=(9, 14, 5)), _prompts(12, lens=(4, 4, 4))
    s1, s2 = _sample(71, **SETTINGS["typical_p"]), _sample(72, **SETTINGS["all"])
    sess = llm.new_session(3)
    _packed(llm, prompts, s1, session=sess)
    probe = copy.copy(sess)
    probe.k, probe.v, probe.valid_len, probe.pending_id = sess.k.clone(), sess.v.clone(), list(sess.valid_len), list(sess.pending_id)
    logits = llm(inputs_embeds=[f.to(DEV) for f in follow], use_cache=True, past_key_values=probe).logits[:, 0].float().contiguous()
    ctx = torch.tensor(probe.valid_len, dtype=torch.int32, device=DEV)
    want, _ = _loop(llm, s2, first=(logits, ctx, probe.kv_struct()))
    ids, _ = _packed(llm, follow, s2, session=sess)
    assert sess.turns == 2 and torch.equal(ids, want)


def test_a_graph_captured_for_one_min_p_is_not_replayed_for_another():
    """the same model, cache, workspace, seed and row count, min_p alone differs: 1.0 must give the greedy ids, 0.05 the loop's"""
    llm, prompts = _llm(), _prompts()
    loose = _sample(81, min_p=0.05)
    want, _ = _loop(llm, loose, prompts)
    greedy, _ = _packed(llm, prompts, None)
    assert not torch.equal(want, greedy)
    for sample, ref in ((loose, want), (_sample(81, min_p=1.0), greedy), (loose, want)):
        got, _ = _packed(llm, prompts, sample)
        assert torch.equal(got, ref), sample
