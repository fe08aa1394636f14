"""CPU (no GPU): the token log-probability surface — header / ctypes mirror / exports, the fp64 restatement
(tests/token_scores_ref.py) against transformers' compute_transition_scores(normalize_logits=True), the rounding bound against fp32 numpy
emulations of the two summation orders, the conditions the fixture (tests/golden/token_scores_tiny.npz, written by
tools/gen_token_scores_golden.py) must meet, and the keyword plumbing of generate()."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO, golden, pkg, t

import logits_proc_ref as lpr
import token_scores_ref as tsr

L = pkg("_lib")
llama_mod = pkg("audio_llama")

NEW_EXPORTS = ["sl_gemm_top1_lse", "sl_greedy_select_sc", "sl_greedy_select_partial_sc", "sl_sample_select_sc", "sl_generate_workspace_bytes_sc",
               "sl_generate_sc"]
CASES = ["greedy", "rep13", "ngram2", "minnew6", "eos_all", "eos_one", "batch1", "batch1_eos", "ragged3", "ragged3_eos"]
HDR = open(os.path.join(REPO, "include", "speechllm.h")).read()


# ------------------------------------------------------------------------------------------------ header, exports
def test_header_declares_the_new_entries_and_the_abi_stays_7():
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", HDR))
    assert set(NEW_EXPORTS) <= declared and set(NEW_EXPORTS) <= set(L.EXPORTS)
    lib = L.lib()
    assert lib.sl_version() == 7
    for name in NEW_EXPORTS:
        getattr(lib, name)
    assert "SL_ABI_VERSION 7" in re.sub(r"\s+", " ", HDR)


def _c_params(name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", HDR, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW_EXPORTS)
def test_argtypes_match_the_header(name):
    res, args = L._PROTOS[name]
    params = _c_params(name)
    assert len(params) == len(args), (name, params)
    assert res is (L.c_sz if re.search(r"\bsize_t\s+" + name, HDR) else L.c_i32)
    scalars = {"int32_t": L.c_i32, "int64_t": L.c_i64, "size_t": L.c_sz, "float": L.c_f32, "uint64_t": C.c_uint64}
    structs = {"sl_logits_opts": L.LogitsOpts, "sl_generate_opts": L.GenerateOpts, "sl_llama_model": L.LlamaModel, "sl_kv_cache": L.KVCache,
               "sl_generate_stats": L.GenerateStats, "sl_gemm_args": L.GemmArgs, "sl_gemm_ex_args": L.GemmEx}
    for p, a in zip(params, args):
        if "*" in p or p.startswith("sl_stream"):
            base = re.sub(r"\bconst\b", "", p).split("*")[0].strip()
            if base in structs:
                assert a is C.POINTER(structs[base]), (name, p)
            else:
                assert a is L.c_vp or (isinstance(a, type) and issubclass(a, C._Pointer)), (name, p)
        else:
            assert a is scalars[p.split()[0]], (name, p)


def test_the_new_entries_refuse_bad_arguments_without_a_gpu_and_off_is_the_old_workspace():
    lib = L.lib()
    a, ex = L.GemmArgs(), L.GemmEx()
    a.A, a.W, a.lda, a.ldw, a.M, a.N, a.K, a.batch, a.dtype, a.out_f32 = 4096, 4096, 64, 64, 128, 128, 64, 1, L.SL_BF16, 1
    ex.w_mod = 1
    assert lib.sl_gemm_top1_lse(C.byref(a), C.byref(ex), 4096, None) == -1 and b"amax_val" in lib.sl_last_error()      # the third plane alone
    ex.amax_val, ex.amax_idx = 4096, 4096
    assert lib.sl_gemm_top1_lse(C.byref(a), C.byref(ex), None, None) == -1
    a.M = 64
    assert lib.sl_gemm_top1_lse(C.byref(a), C.byref(ex), 4096, None) == -1 and b"M > 64" in lib.sl_last_error()
    eos = (C.c_int32 * 8)(*range(8))
    assert lib.sl_greedy_select_partial_sc(4096, 4096, None, 16, 128, eos, 1, 0, 1, 1, 4096, 4096, 4096, 4096, 4096, 4096, 8, 4096, None) == -1
    assert b"come together" in lib.sl_last_error()
    assert lib.sl_greedy_select_sc(None, 4, 100, eos, 1, 0, 1, 4096, 4096, 4096, 4096, 4096, 4096, 8, 4096, None) == -1
    assert lib.sl_sample_select_sc(4096, 4, 100, 0.0, 0, 1.0, 1, eos, 1, 0, 1, 4096, 4096, 4096, 4096, 4096, 4096, 8, 4096, 4096, None) == -1
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab, m.rope_len = L.SL_F32, 256, 2, 2, 2, 128, 384, 1000, 64
    base = lib.sl_generate_workspace_bytes(C.byref(m), 40, 4, 16)
    assert lib.sl_generate_workspace_bytes_sc(C.byref(m), 40, 4, 16, None, 0) == base
    assert lib.sl_generate_workspace_bytes_sc(C.byref(m), 40, 4, 16, None, 1) == base + 4 * 16 * 4 + 256
    lp = L.LogitsOpts()
    lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = 1.2, 0, 0
    assert lib.sl_generate_workspace_bytes_sc(C.byref(m), 40, 4, 16, C.byref(lp), 0) == lib.sl_generate_workspace_bytes_lp(C.byref(m), 40, 4, 16, C.byref(lp))
    # the third plane always fits behind the other two in the idle logits buffer: 3 ceil(V / 64) B <= B V
    for V in (1, 2, 3, 63, 64, 65, 777, 1000, 128256):
        assert 3 * ((V + 63) // 64) <= V or V < 3          # (a vocabulary below 3 takes no tiled lm_head: K and N limits refuse it first)


# ------------------------------------------------------------------------------------------------ the restatement against transformers
def _hf_transition_scores(sequences, scores):
    from transformers.generation.utils import GenerationMixin
    stub = SimpleNamespace(config=SimpleNamespace(vocab_size=scores[0].shape[-1], is_encoder_decoder=False, get_text_config=None))
    stub.config.get_text_config = lambda *a, **k: stub.config
    return GenerationMixin.compute_transition_scores(stub, sequences, tuple(scores), normalize_logits=True)


@pytest.mark.parametrize("mode", ["plain", "processors", "topk", "topp", "topk_topp_temp"])
def test_restatement_equals_transformers_compute_transition_scores(mode):
    import transformers.generation.logits_process as lp_mod
    B, V, T = 4, 200, 6
    gen = torch.Generator().manual_seed(17)
    eos = [3]
    hist = [[] for _ in range(B)]
    scores, toks, mine = [], [], []
    for step in range(T):
        raw = torch.randn(B, V, generator=gen) * 3.0
        raw[:, 5] = float("-inf")
        ids = torch.tensor(hist, dtype=torch.long).view(B, step)
        s, s_mine = raw.clone(), raw.clone()
        if mode == "processors":
            s = lp_mod.RepetitionPenaltyLogitsProcessor(penalty=1.3)(ids, s)
            s = lp_mod.NoRepeatNGramLogitsProcessor(2)(ids, s)
            s = lp_mod.MinNewTokensLengthLogitsProcessor(0, 3, eos, device="cpu")(ids, s)
            s_mine = lpr.process(raw, hist, 1.3, 2, 3, eos)
        if mode in ("topk", "topp", "topk_topp_temp"):
            temp, k, p = (0.7, 20, 0.9) if mode == "topk_topp_temp" else ((1.0, 20, 1.0) if mode == "topk" else (1.0, 0, 0.8))
            if temp != 1.0:
                s = lp_mod.TemperatureLogitsWarper(temp)(ids, s)
            if k:
                s = lp_mod.TopKLogitsWarper(k)(ids, s)
            if p < 1.0:
                s = lp_mod.TopPLogitsWarper(p)(ids, s)
            s_mine = tsr.warp(raw, temp, k, p)
            assert torch.equal(torch.isinf(s_mine), torch.isinf(s)), (mode, step)        # the same survivors
        tok = torch.multinomial(torch.softmax(s, dim=-1), 1, generator=gen)[:, 0]
        scores.append(s)
        mine.append(s_mine)
        toks.append(tok)
        for b in range(B):
            hist[b].append(int(tok[b]))
    seq = torch.stack(toks, dim=1)
    want = _hf_transition_scores(seq, scores).double()
    got = torch.stack([tsr.transition_logprobs(m_, seq[:, i]) for i, m_ in enumerate(mine)], dim=1)
    assert bool(torch.isfinite(got).all()) and bool((got <= 0).all())
    assert float((got - want).abs().max()) < 2e-6, float((got - want).abs().max())          # transformers works in fp32, the restatement in fp64


def test_nan_counts_as_minus_inf_and_a_row_without_a_finite_maximum_is_not_finite():
    s = torch.tensor([[1.0, float("nan"), 2.0, float("-inf")], [float("-inf")] * 4, [float("nan")] * 4])
    lp = tsr.transition_logprobs(s, torch.tensor([2, 0, 1]))
    assert abs(float(lp[0]) - (2.0 - np.log(np.exp(1.0) + np.exp(2.0)))) < 1e-12
    assert not np.isfinite(float(lp[1])) and not np.isfinite(float(lp[2]))
    for x in (np.array([-np.inf] * 70, dtype=np.float32), np.array([np.nan] * 70, dtype=np.float32)):
        gmax, gsum = tsr.group_planes_f32(x)
        assert (gsum == 0).all() and (gmax == -np.inf).all()
        assert not np.isfinite(tsr.partial_logprob_f32(gmax, gsum)) and not np.isfinite(tsr.row_logprob_f32(x, 0))


# ------------------------------------------------------------------------------------------------ the rounding bound
BOUND_SHAPES = [64, 65, 777, 1000, 4096, 128256]


def _bound_rows(V):
    gen = np.random.default_rng(V)
    rows = [gen.standard_normal(V).astype(np.float32) * s for s in (0.05, 1.0, 4.0, 12.0)]
    rows.append((gen.standard_normal(V) * 3.0 + 100.0).astype(np.float32))              # a large common offset: exp(x) alone overflows
    flat = np.zeros(V, dtype=np.float32)                                                 # every term 1: the longest chains at full weight
    rows.append(flat)
    holes = (gen.standard_normal(V) * 2.0).astype(np.float32)
    holes[: min(V - 1, 64)] = -np.inf                                                    # a whole group of -inf (a banned range)
    holes[V // 2] = np.nan
    rows.append(holes)
    return rows


@pytest.mark.parametrize("V", BOUND_SHAPES)
def test_bound_holds_for_both_summation_orders_and_rejects_two_wrong_forms(V):
    """The bound of DESIGN 3.5 against fp32 numpy emulations of the row scan (sl_row_max_lse) and of the group / stripe order (tile_argmax
    + greedy_select_partial_kernel) at every vocabulary the GPU tests use and the product's 128 256.  Worst err / bound over all shapes
    and rows as measured when this was written: row scan 0.13, group / stripe 0.14 (both at V = 4 096); on the GPU the kernels reach 0.14 /
    0.10 and the third plane 0.23 of its own bound (tests/test_token_scores_gpu.py prints them).  The bound refuses the sum taken without subtracting the maximum (overflows on the offset rows: err = inf) and the group
    maximum used in place of the row maximum (off by about log(number of groups))."""
    worst = dict(row=0.0, partial=0.0)
    rejected = dict(no_max=0, group_max=0)
    for x in _bound_rows(V):
        clean = np.where(np.isnan(x), -np.inf, x).astype(np.float64)
        tok = int(np.argmax(clean))
        ref = float(tsr.transition_logprobs(torch.from_numpy(x)[None], torch.tensor([tok]))[0])
        b_row, b_part = tsr.bound_row(x, tok), tsr.bound_partial(x)
        got_row = float(tsr.row_logprob_f32(x, tok))
        gmax, gsum = tsr.group_planes_f32(x)
        got_part = float(tsr.partial_logprob_f32(gmax, gsum))
        print(f"V={V} row err {abs(got_row - ref):.3e} / {b_row:.3e}  partial err {abs(got_part - ref):.3e} / {b_part:.3e}")
        assert abs(got_row - ref) <= b_row and abs(got_part - ref) <= b_part
        worst["row"] = max(worst["row"], abs(got_row - ref) / b_row)
        worst["partial"] = max(worst["partial"], abs(got_part - ref) / b_part)
        # the group sums, per element, against their own bound
        pad = np.full(len(gmax) * 64, -np.inf)
        pad[:V] = clean
        for g, grp in enumerate(pad.reshape(-1, 64)):
            if np.isfinite(grp.max()):
                want = float(np.exp(grp - grp.max()).sum())
                assert abs(float(gsum[g]) - want) <= tsr.bound_group_sum(grp) * want
        # two wrong emulations the bound must refuse
        bad1 = float(tsr.row_logprob_f32(x, tok, subtract_max=False))
        bad2 = float(tsr.partial_logprob_f32(gmax, gsum, rescale=False))
        rejected["no_max"] += int(not abs(bad1 - ref) <= b_row)
        rejected["group_max"] += int(not abs(bad2 - ref) <= b_part)
    print("worst err / bound", worst, "rejected", rejected)
    assert rejected["no_max"] >= 1 and rejected["group_max"] >= (1 if V > 64 else 0)


# ------------------------------------------------------------------------------------------------ the fixture
def _case(name):
    g = golden("token_scores_tiny")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def test_fixture_holds_the_cases_and_data_only():
    g = golden("token_scores_tiny")
    assert list(g["cases"]) == CASES
    assert all(v.dtype.kind in "iufbU" for v in g.values())
    assert (int(g["cfg.vocab_size"]), int(g["cfg.num_hidden_layers"])) == (1000, 2)


@pytest.mark.parametrize("name", CASES)
def test_fixture_meets_its_own_conditions(name):
    c = _case(name)
    ids, lps, lens = t(c["ids"]).long(), t(c["logprobs"]), c["lens"].tolist()
    B, max_new = ids.shape
    assert lps.shape == ids.shape and lps.dtype == torch.float32 and len(c["prompt_lens"]) == B
    assert float(c["min_margin"]) >= 1e-3
    assert bool((lps <= 0).all()) and bool(torch.isfinite(lps).all())
    eos = set(c["eos"].tolist())
    for b in range(B):
        n = lens[b]
        assert bool((lps[b, n:] == 0).all()) and bool((ids[b, n:] == 0).all())            # zeros / pads at and after the finish
        assert bool((lps[b, :n] < 0).all())
        assert not (set(ids[b, :n - 1].tolist()) & eos)
        assert n == max_new or int(ids[b, n - 1]) in eos
    assert int(c["n_cols"]) == max(lens)
    if name == "minnew6":
        assert min(lens) >= 6
    if name == "ngram2":
        assert not any(lpr.has_repeated_ngram(ids[b, :lens[b]].tolist(), 2) for b in range(B))
    if name in ("rep13", "ngram2"):
        assert not torch.equal(ids, t(_case("greedy")["ids"]).long())                    # the processor changed the path


# ------------------------------------------------------------------------------------------------ keyword plumbing
def _tiny_llm():
    from oracle.golden_cfgs import TINY_MHA as LC
    weights = pkg("weights")
    larch = weights.LlamaArch(LC.hidden_size, LC.num_hidden_layers, LC.num_attention_heads, LC.num_key_value_heads, LC.head_dim,
                              LC.intermediate_size, LC.vocab_size, LC.rms_norm_eps, LC.rope_theta, LC.rope_scaling,
                              LC.tie_word_embeddings, tuple(LC.eos_token_ids), LC.pad_token_id)
    return llama_mod.AudioLlamaForCausalLM(larch, {}, torch_dtype=torch.float32, max_ctx=64)


class _Recorder:
    """stands in for generate_packed: keeps what generate() hands over, answers with recognisable values"""

    def __init__(self, llm):
        self.calls = []
        llm._w = object()
        llm._dev = lambda: llm._w
        llm.generate_packed = self

    def __call__(self, x, lens, max_new_tokens, **kw):
        self.calls.append(kw)
        ids = torch.arange(len(lens) * max_new_tokens, dtype=torch.int32).view(len(lens), max_new_tokens)
        if kw.get("scores"):
            return ids, max_new_tokens - 1, -torch.ones(len(lens), max_new_tokens)
        return ids, max_new_tokens - 1


def test_generate_on_a_cpu_model_fails_as_loudly_as_before():
    llm = _tiny_llm()
    for kw in (dict(), dict(return_dict_in_generate=True, output_scores=True)):
        with pytest.raises(L.SpeechLLMError, match="not on the GPU"):
            llm.generate(inputs_embeds=torch.zeros(1, 4, 256), max_new_tokens=4, **kw)
    with pytest.raises(L.SpeechLLMError, match="not on the GPU"):
        llm.generate_packed(torch.zeros(4, 256), [4], 4, scores=True)


def test_return_dict_in_generate_and_output_scores_are_no_longer_swallowed():
    """fails on a build that drops the two keywords into **unused: the call then returns the bare tensor"""
    llm = _tiny_llm()
    rec = _Recorder(llm)
    x = torch.zeros(2, 4, 256)
    plain = llm.generate(inputs_embeds=x, max_new_tokens=8)
    assert torch.is_tensor(plain) and plain.shape == (2, 7) and "scores" not in rec.calls[-1]           # neither set: the tensor, the old call
    out = llm.generate(inputs_embeds=x, max_new_tokens=8, return_dict_in_generate=True, output_scores=True)
    assert isinstance(out, llama_mod.GenerateOutput) and rec.calls[-1]["scores"] is True
    assert torch.equal(out.sequences, plain) and out.sequences.dtype == torch.int64
    assert out.token_logprobs.shape == (2, 7) and out.token_logprobs.dtype == torch.float32
    assert out.sequences_scores.tolist() == [-7.0, -7.0]
    out = llm.generate(inputs_embeds=x, max_new_tokens=8, return_dict_in_generate=True)
    assert isinstance(out, llama_mod.GenerateOutput) and out.token_logprobs is None and out.sequences_scores is None and "scores" not in rec.calls[-1]
    llm.last_token_logprobs = None
    ids = llm.generate(inputs_embeds=x, max_new_tokens=8, output_scores=True)                           # HF ignores the flag here; the attribute costs nothing
    assert torch.is_tensor(ids) and llm.last_token_logprobs.shape == (2, 7)
    llm.generation_config.return_dict_in_generate, llm.generation_config.output_scores = True, True      # generation_config is the fallback
    out = llm.generate(inputs_embeds=x, max_new_tokens=8)
    assert isinstance(out, llama_mod.GenerateOutput) and out.token_logprobs is not None
    assert torch.is_tensor(llm.generate(inputs_embeds=x, max_new_tokens=8, return_dict_in_generate=False, output_scores=False))
    out = llm.generate(inputs_embeds=x, max_new_tokens=8, do_sample=True, seed=3)
    assert rec.calls[-1]["scores"] is True and rec.calls[-1]["sample"]["seed"] == 3


def test_beam_search_with_output_scores_raises_and_sequences_scores_are_the_beam_scores():
    llm = _tiny_llm()
    rec = _Recorder(llm)
    x = torch.zeros(2, 4, 256)
    with pytest.raises(L.SpeechLLMError, match="output_scores"):
        llm.generate(inputs_embeds=x, max_new_tokens=8, num_beams=3, output_scores=True)
    with pytest.raises(L.SpeechLLMError, match="output_scores"):
        llm.generate(inputs_embeds=x, max_new_tokens=8, num_beams=3, output_scores=True, return_dict_in_generate=True)
    llm.last_beam_scores = torch.tensor([-1.5, -2.5])
    out = llm.generate(inputs_embeds=x, max_new_tokens=8, num_beams=3, return_dict_in_generate=True)
    assert out.token_logprobs is None and out.sequences_scores.tolist() == [-1.5, -2.5] and rec.calls[-1]["beams"]["num_beams"] == 3


def test_inference_return_scores_gives_one_mean_log_probability_per_answer():
    inference = pkg("inference")
    llm = _tiny_llm()
    rec = _Recorder(llm)
    llm.generation_config.eos_token_id = [10]                       # row 1 of the recorder's ids (8 .. 14) meets it at its third token
    inf = inference.LLMSpeechTextInference.__new__(inference.LLMSpeechTextInference)       # the constructor needs a GPU: the plumbing does not
    inf.llm, inf.beams, inf.logits = llm, None, None
    inf.llm_tokenizer = type("Tok", (), {"batch_decode": staticmethod(lambda ids, **kw: ["" for _ in ids])})()
    texts = inf.generate_llm_response(torch.zeros(2, 4, 256), max_new_tokens=8)
    assert texts == ["", ""] and "scores" not in rec.calls[-1]
    texts, scores = inf.generate_llm_response(torch.zeros(2, 4, 256), max_new_tokens=8, return_scores=True)
    assert texts == ["", ""] and scores == [-1.0, -1.0] and rec.calls[-1]["scores"] is True
    lps = torch.tensor([[-1.0, -3.0, 0.0, 0.0], [-2.0, -2.0, -2.0, -6.0]])
    assert inf._mean_logprobs(torch.tensor([[4, 10, 0, 0], [1, 2, 3, 4]]), lps) == [-2.0, -3.0]
