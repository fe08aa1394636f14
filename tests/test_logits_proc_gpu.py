"""GPU: HF's logits processors — sl_logits_process against tests/logits_proc_ref.py, sl_beam_topk_ex against sl_beam_topk, and generate()
with repetition_penalty / no_repeat_ngram_size / min_new_tokens end to end against what the reference class returned
(tests/golden/logits_proc_tiny.npz)."""
import ctypes as C

import pytest
import torch

from conftest import golden, pkg, t
from oracle.golden_cfgs import TINY_LLAMA, TINY_MHA

import logits_proc_ref as lpr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = pkg("_lib")
ri = pkg("random_init")
weights = pkg("weights")
llama_mod = pkg("audio_llama")

KINDS = ["rep13", "ngram2", "minnew6", "all3", "beam_k3"]
CASES = [f"{m}_{k}" for m in ("tiny_mha", "tiny_gqa") for k in KINDS]
CFG = {"tiny_mha": TINY_MHA, "tiny_gqa": TINY_LLAMA}
GUARD = 12345.0
HIST_LD = 304

_LLMS = {}


def _llm(model, seed, norm_mul, dtype, max_ctx=64):
    key = (model, seed, norm_mul, dtype, max_ctx)
    if key not in _LLMS:
        c = CFG[model]
        arch = weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size,
                                 c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling, c.tie_word_embeddings, tuple(c.eos_token_ids), c.pad_token_id)
        sd = dict(ri.llama_state_dict(c, seed=seed))
        sd["model.norm.weight"] = sd["model.norm.weight"] * float(norm_mul)
        _LLMS[key] = llama_mod.AudioLlamaForCausalLM(arch, sd, torch_dtype=dtype, device=DEV, max_ctx=max_ctx)
    return _LLMS[key]


def _set_eos(llm, eos, pad):
    llm.generation_config.eos_token_id = list(eos) if len(eos) else None
    llm.generation_config.pad_token_id = int(pad)


def _lp(p=1.0, g=0, mn=0):
    lp = L.LogitsOpts()
    lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = p, g, mn
    return lp


# ------------------------------------------------------------------------------------------------ sl_logits_process
def _run_kernel(logits, hists, unfinished, p, g, mn, eos, log_softmax):
    """-> processed (rows, V) on the host; guard words behind the logits and the scratch are checked"""
    rows, V = logits.shape
    buf = torch.full((rows * V + 16,), GUARD, device=DEV)
    buf[:rows * V] = logits.reshape(-1).to(DEV)
    scratch = torch.full((rows * HIST_LD + 16,), GUARD, device=DEV)
    hist = torch.randint(0, V, (rows, HIST_LD), generator=torch.Generator().manual_seed(V), dtype=torch.int32)      # entries past a row's length: never read
    for r, h in enumerate(hists):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hist_d = hist.to(DEV)
    len_d = torch.tensor([len(h) for h in hists], dtype=torch.int32).to(DEV)
    unf_d = None if unfinished is None else torch.tensor(unfinished, dtype=torch.int32).to(DEV)
    lp = _lp(p, g, mn)
    eos_c = (C.c_int32 * 8)(*(list(eos) + [0] * (8 - len(eos))))
    L.check(L.lib().sl_logits_process(buf.data_ptr(), rows, V, hist_d.data_ptr(), HIST_LD, len_d.data_ptr(), L.ptr(unf_d), C.byref(lp), eos_c, len(eos),
                                      int(log_softmax), scratch.data_ptr(), L.stream_ptr()), "sl_logits_process")
    torch.cuda.synchronize()
    assert bool((buf[rows * V:] == GUARD).all()) and bool((scratch[rows * HIST_LD:] == GUARD).all()), "guard words were written"
    return buf[:rows * V].view(rows, V).cpu()


def _histories(V, lengths, seed):
    """small alphabets (every n-gram repeats), ids 0 and V - 1 among them, and in a row of 300 one token 40 times in a row"""
    gen = torch.Generator().manual_seed(seed)
    alphabet = torch.tensor([0, V - 1, 7, 11, V // 2, V // 3])
    out = []
    for n in lengths:
        h = alphabet[torch.randint(0, len(alphabet), (n,), generator=gen)].tolist()
        if n >= 300:
            wide = torch.randint(0, V, (n,), generator=gen).tolist()         # most of the long row is spread over the vocabulary
            h = [w if i % 3 else a for i, (w, a) in enumerate(zip(wide, h))]
            h[100:140] = [11] * 40
            h[0], h[-1] = 0, V - 1
        out.append(h)
    return out


PROCESSORS = {"penalty": dict(p=1.3, g=0, mn=0), "penalty_below_1": dict(p=0.7, g=0, mn=0), "ngram3": dict(p=1.0, g=3, mn=0), "ngram1": dict(p=1.0, g=1, mn=0),
              "min_new": dict(p=1.0, g=0, mn=40), "all": dict(p=1.3, g=2, mn=40)}


@pytest.mark.parametrize("V", [777, 1000, 128256])
@pytest.mark.parametrize("which", list(PROCESSORS))
def test_logits_process_matches_the_restatement(V, which):
    kw = PROCESSORS[which]
    p, g, mn = kw["p"], kw["g"], kw["mn"]
    gl = g if g > 0 else 3
    eos = [5, V - 1, 11]
    gen = torch.Generator().manual_seed(V + len(which))
    # two assignments of the lengths 0, 1, g - 1, g, 37, 300 to the five rows; the second has a finished row (left untouched)
    for lengths, unfinished in (([0, 1, gl - 1, gl, 300], None), ([37, 300, gl, 300, 1], [1, 0, 1, 1, 1])):
        hists = _histories(V, lengths, seed=V + sum(lengths))
        logits = torch.randn(5, V, generator=gen)
        logits[:, torch.randint(0, V, (9,), generator=gen)] = float("-inf")
        logits[:, 0], logits[:, V - 1] = -1.5, 2.25                           # a negative and a positive score under history tokens
        live = [r for r in range(5) if unfinished is None or unfinished[r]]
        # raw logits: bit for bit
        got = _run_kernel(logits, hists, unfinished, p, g, mn, eos, 0)
        want = lpr.process(logits, hists, p, g, mn, eos)
        for r in range(5):
            assert torch.equal(got[r], want[r] if r in live else logits[r]), (which, V, lengths, r)
        assert torch.equal(_run_kernel(logits, hists, unfinished, p, g, mn, eos, 0), got)          # the same bits on every run
        # log_softmax first: within 1e-5 of the double-precision log_softmax followed by the processors, the same -inf set
        got = _run_kernel(logits, hists, unfinished, p, g, mn, eos, 1)
        want = lpr.process(torch.log_softmax(logits.double(), dim=-1), hists, p, g, mn, eos)
        for r in live:
            inf = torch.isinf(want[r])
            assert torch.equal(torch.isinf(got[r]), inf) and not bool(torch.isnan(got[r]).any()), (which, V, lengths, r)
            err = float((got[r][~inf].double() - want[r][~inf]).abs().max())
            print(f"{which} V={V} row {r} (n={lengths[r]}): log_softmax mode max |err| {err:.3e}")
            assert err <= 1e-5, (which, V, lengths, r, err)
        for r in range(5):
            if r not in live:
                assert torch.equal(got[r], logits[r])
        assert torch.equal(_run_kernel(logits, hists, unfinished, p, g, mn, eos, 1), got)


def test_all_processors_off_leaves_raw_logits_alone():
    logits = torch.randn(3, 1000, generator=torch.Generator().manual_seed(1))
    hists = _histories(1000, [5, 37, 300], seed=2)
    assert torch.equal(_run_kernel(logits, hists, None, 1.0, 0, 0, [5], 0), logits)
    assert torch.equal(_run_kernel(logits, hists, None, 1.0, 0, 7, [], 0), logits)            # min_new_tokens without EOS ids: nothing to ban


# ------------------------------------------------------------------------------------------------ sl_beam_topk_ex
def _topk(fn, logits_d, score_d, M, *extra):
    rows, V = logits_d.shape
    val = torch.full((rows * M + 16,), float("nan"), device=DEV)
    tok = torch.full((rows * M + 16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    val[rows * M:] = GUARD
    L.check(fn(logits_d.data_ptr(), rows, V, score_d.data_ptr(), M, val.data_ptr(), tok.data_ptr(), L.stream_ptr(), *extra), "sl_beam_topk")
    torch.cuda.synchronize()
    assert bool((val[rows * M:] == GUARD).all()) and bool((tok[rows * M:] == 0x5A5A5A5A).all())
    return val[:rows * M].view(rows, M).cpu(), tok[:rows * M].view(rows, M).cpu()


@pytest.mark.parametrize("V", [777, 1000, 128256])
def test_topk_of_the_processed_log_probabilities_equals_topk_of_the_raw_logits_bit_for_bit(V):
    lib = L.lib()
    gen = torch.Generator().manual_seed(V)
    rows, M = 5, 8
    logits = torch.randn(rows, V, generator=gen) * 2.0
    logits[1, torch.randint(0, V, (20,), generator=gen)] = float("-inf")
    logits[2, 3] = float("nan")
    logits[4] = float("-inf")                                               # a row of nothing: every value -inf, never NaN
    score = (-torch.rand(rows, generator=gen) * 5.0).to(DEV)
    raw = logits.to(DEV)
    val0, tok0 = _topk(lib.sl_beam_topk, raw, score, M)
    lsm = raw.clone()
    zero = torch.zeros(rows, dtype=torch.int32, device=DEV)
    lp = _lp()
    L.check(lib.sl_logits_process(lsm.data_ptr(), rows, V, None, 0, zero.data_ptr(), None, C.byref(lp), None, 0, 1, None, L.stream_ptr()), "sl_logits_process")
    val1, tok1 = _topk(lib.sl_beam_topk_ex, lsm, score, M, 1)
    assert torch.equal(tok0, tok1) and torch.equal(val0.view(torch.int32), val1.view(torch.int32))
    assert not bool(torch.isnan(lsm).any())
    # is_logprob = 0 is sl_beam_topk itself
    val2, tok2 = _topk(lib.sl_beam_topk_ex, raw, score, M, 0)
    assert torch.equal(tok0, tok2) and torch.equal(val0.view(torch.int32), val2.view(torch.int32))


# ------------------------------------------------------------------------------------------------ end to end, fp32
def _case(name):
    g = golden("logits_proc_tiny")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def _case_inputs(c, dtype=torch.float32):
    model = str(c["model"])
    llm = _llm(model, int(c["weight_seed"]), float(c["norm_mul"]), dtype)
    _set_eos(llm, c["eos"].tolist(), int(c["pad"]))
    x = torch.randn(int(c["batch"]), int(c["S"]), CFG[model].hidden_size, generator=torch.Generator().manual_seed(int(c["input_seed"]))) * 0.05
    proc = dict(repetition_penalty=float(c["repetition_penalty"]), no_repeat_ngram_size=int(c["no_repeat_ngram_size"]), min_new_tokens=int(c["min_new_tokens"]))
    return llm, x, proc


def _check_against_fixture(llm, c, ids, tag):
    if int(c["K"]) > 1:
        lens, want = t(c[f"{tag}lens"]).long(), t(c[f"{tag}ids"]).long()
        assert torch.equal(llm.last_beam_lengths.long(), lens)
        assert ids.shape == (want.shape[0], int(lens.max())) and torch.equal(ids, want[:, :ids.shape[1]])
        got, ref = llm.last_beam_scores.double(), t(c[f"{tag}scores"]).double()
        print("scores", got.tolist(), "reference", ref.tolist())
        assert bool(((got - ref).abs() <= 1e-4 * ref.abs().clamp(min=1.0)).all())
    else:
        want = t(c[f"{tag}ids"]).long()[:, :int(c[f"{tag}n_cols"])]
        assert ids.shape == want.shape and torch.equal(ids, want), (ids, want)


@pytest.mark.parametrize("name", CASES)
def test_generate_with_the_processors_reproduces_the_reference_class(name):
    """fails on a build that ignores the keywords: every case's processed ids differ from its plain ids"""
    c = _case(name)
    llm, x, proc = _case_inputs(c)
    kw = dict(max_new_tokens=int(c["max_new"]))
    if int(c["K"]) > 1:
        kw.update(num_beams=int(c["K"]), num_return_sequences=1, length_penalty=1.0, early_stopping=False)
    ids = llm.generate(inputs_embeds=x.to(DEV), **kw, **proc).cpu()
    assert ids.dtype == torch.int64
    _check_against_fixture(llm, c, ids, "")
    plain = llm.generate(inputs_embeds=x.to(DEV), **kw).cpu()
    _check_against_fixture(llm, c, plain, "plain_")


# ------------------------------------------------------------------------------------------------ compaction
def test_compacted_and_uncompacted_batches_give_the_same_ids_with_processors_on():
    llm = _llm("tiny_gqa", 31, 32, torch.float32)
    lens = [9, 21, 14, 5, 17, 11, 8, 13, 19, 6, 10, 15]
    budgets = [2, 2, 3, 3, 4, 4, 5, 20, 20, 20, 20, 20]                       # six rows are finished at the first check (step 4): 12 -> the 6-row rung
    max_new = 20
    x = (torch.randn(sum(lens), TINY_LLAMA.hidden_size, generator=torch.Generator().manual_seed(77)) * 0.05).to(DEV)
    logits = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    _set_eos(llm, [], TINY_LLAMA.pad_token_id)
    free, _ = llm.generate_packed(x.clone(), lens, max_new, use_eos=False, compact=False, logits=logits)
    _set_eos(llm, [int(free[8, 12])], TINY_LLAMA.pad_token_id)               # an EOS id the ninth row meets at step 12 at the latest
    out = {}
    for compact in (False, True):
        ids, n_cols = llm.generate_packed(x.clone(), lens, max_new, row_limits=budgets, compact=compact, logits=logits)
        out[compact] = (ids.clone(), n_cols, dict(llm.last_generate_stats))
    assert out[True][2]["compactions"] >= 1 and out[False][2]["compactions"] == 0
    assert out[True][1] == out[False][1] and torch.equal(out[True][0], out[False][0])
    eos = int(free[8, 12])
    for b, n in enumerate(budgets):                                          # and the processors held in every row
        row = out[True][0][b, :n].tolist()
        if eos in row:
            row = row[:row.index(eos) + 1]
        assert not lpr.has_repeated_ngram(row, 2), (b, row)


# ------------------------------------------------------------------------------------------------ 16-bit and sampling: invariants of the output
@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_and_sampled_outputs_keep_the_processors_invariants(dtype, sampling):
    llm = _llm("tiny_gqa", 31, 8, dtype)
    B, S, max_new, mn = 16, 12, 24, 5
    x = (torch.randn(B, S, TINY_LLAMA.hidden_size, generator=torch.Generator().manual_seed(9)) * 0.05).to(dtype).to(DEV)
    mode = dict(do_sample=True, temperature=1.0, top_k=20, top_p=0.95, seed=7) if sampling else {}
    _set_eos(llm, [], TINY_LLAMA.pad_token_id)
    free = llm.generate(inputs_embeds=x.clone(), max_new_tokens=max_new, **mode).cpu()
    eos = int(torch.mode(free.reshape(-1)).values)                            # the token the plain run emits most: an EOS id that matters
    _set_eos(llm, [eos], TINY_LLAMA.pad_token_id)
    plain = llm.generate(inputs_embeds=x.clone(), max_new_tokens=max_new, **mode).cpu()
    st_plain = dict(llm.last_generate_stats)
    off = llm.generate(inputs_embeds=x.clone(), max_new_tokens=max_new, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, **mode).cpu()
    assert torch.equal(off, plain) and dict(llm.last_generate_stats) == st_plain          # the off switch really is off
    ids = llm.generate(inputs_embeds=x.clone(), max_new_tokens=max_new, repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=mn, **mode).cpu()
    assert ids.shape[0] == B and ids.shape[1] >= mn
    for b in range(B):
        row = ids[b].tolist()
        assert eos not in row[:mn], (b, row)                                  # no EOS before min_new_tokens
        if eos in row:
            row = row[:row.index(eos) + 1]
        assert not lpr.has_repeated_ngram(row, 2), (b, row)                   # no 2-gram twice before the row's EOS


# ------------------------------------------------------------------------------------------------ graph cache
def test_a_changed_penalty_never_replays_the_other_graph():
    c = _case("tiny_mha_rep13")
    llm, x, proc = _case_inputs(c)
    B, S, max_new = x.shape[0], x.shape[1], int(c["max_new"])
    xp = x.reshape(B * S, -1).to(DEV)
    on = dict(repetition_penalty=1.3, no_repeat_ngram_size=0, min_new_tokens=0)
    llm.generate_packed(xp.clone(), [S] * B, max_new, logits=on)             # sizes the workspace: the calls below share one buffer
    L.lib().sl_decode_graph_cache_clear()
    got = []
    for logits in (on, dict(on, repetition_penalty=1.0), on, None):
        ids, n_cols = llm.generate_packed(xp.clone(), [S] * B, max_new, logits=logits)
        got.append(ids[:, :n_cols].long())
    want_on, want_off = t(c["ids"]).long(), t(c["plain_ids"]).long()
    assert torch.equal(got[0], want_on) and torch.equal(got[1], want_off) and torch.equal(got[2], want_on) and torch.equal(got[3], want_off)
    assert L.lib().sl_decode_graph_cache_clear() == 2                        # one graph with the penalty, one without: the repeats replayed them
