"""CPU (no GPU): the logits-processor surface — header / exports / struct mirror, every limit reported before any launch, the plain-torch
restatement (tests/logits_proc_ref.py) against transformers' own processors, the conditions the fixture
(tests/golden/logits_proc_tiny.npz, written by tools/gen_logits_proc_golden.py) must meet, and the config / keyword plumbing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import REPO, golden, pkg, t

import logits_proc_ref as lpr

L = pkg("_lib")
cfgm = pkg("config")

NEW_EXPORTS = ["sl_logits_process", "sl_beam_topk_ex", "sl_generate_workspace_bytes_lp", "sl_generate_lp", "sl_beam_generate_workspace_bytes_lp",
               "sl_beam_generate_lp"]
KINDS = ["rep13", "ngram2", "minnew6", "all3", "beam_k3"]
CASES = [f"{m}_{k}" for m in ("tiny_mha", "tiny_gqa") for k in KINDS]
HDR = open(os.path.join(REPO, "include", "speechllm.h")).read()


# ------------------------------------------------------------------------------------------------ header, exports, struct
def test_header_declares_the_new_entries_and_the_abi_stays_7():
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", HDR))
    assert set(NEW_EXPORTS) <= declared and set(NEW_EXPORTS) <= set(L.EXPORTS)
    lib = L.lib()
    assert lib.sl_version() == 7
    for name in NEW_EXPORTS:
        getattr(lib, name)
    assert "unfused" in HDR or "gives up" in HDR          # the header states what a processors-on step costs


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
    structs = {"sl_logits_opts": L.LogitsOpts, "sl_generate_opts": L.GenerateOpts, "sl_beam_opts": L.BeamOpts, "sl_llama_model": L.LlamaModel,
               "sl_kv_cache": L.KVCache, "sl_generate_stats": L.GenerateStats}
    for p, a in zip(params, args):
        if "*" in p or p.startswith("sl_stream"):
            base = re.sub(r"\bconst\b", "", p).split("*")[0].strip()
            if base in structs:
                assert a is C.POINTER(structs[base]), (name, p)
            else:
                assert a is L.c_vp or (isinstance(a, type) and issubclass(a, C._Pointer)), (name, p)
        else:
            assert a is scalars[p.split()[0]], (name, p)


def test_struct_mirror_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "sl_logits_opts", L.LogitsOpts
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "speechllm.h")}"', 'int main(void) {',
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[cname]) == C.sizeof(cls) == 16
    for fname, _ in cls._fields_:
        assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


# ------------------------------------------------------------------------------------------------ limits, before any device work
def _lp(p=1.0, g=0, mn=0):
    lp = L.LogitsOpts()
    lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = p, g, mn
    return lp


BAD = [("penalty 0", dict(p=0.0), b"repetition_penalty"), ("penalty < 0", dict(p=-1.5), b"repetition_penalty"),
       ("penalty inf", dict(p=float("inf")), b"repetition_penalty"), ("penalty nan", dict(p=float("nan")), b"repetition_penalty"),
       ("ngram < 0", dict(g=-1), b"no_repeat_ngram_size"), ("min_new < 0", dict(mn=-2), b"min_new_tokens")]


@pytest.mark.parametrize("what,kw,needle", BAD)
def test_bad_options_are_refused_by_every_entry_without_a_gpu(what, kw, needle):
    lib = L.lib()
    lp = _lp(**kw)
    eos = (C.c_int32 * 8)(*range(8))
    # (the pointers are never dereferenced: the options are checked first)
    assert lib.sl_logits_process(1, 4, 100, 1, 8, 1, None, C.byref(lp), eos, 1, 0, 1, None) == -1 and needle in lib.sl_last_error(), (what, lib.sl_last_error())
    o = L.GenerateOpts()
    o.max_new_tokens = 8
    assert lib.sl_generate_lp(None, None, None, None, 2, C.byref(o), None, None, None, 0, None, C.byref(lp)) == -1
    assert needle in lib.sl_last_error(), (what, lib.sl_last_error())
    m, kv, bo = L.LlamaModel(), L.KVCache(), L.BeamOpts()
    m.vocab, kv.slots, kv.max_ctx = 1000, 64, 48
    bo.num_beams, bo.num_return_sequences, bo.max_new_tokens = 2, 1, 8
    cu = (C.c_int32 * 3)(0, 10, 20)
    assert lib.sl_beam_generate_lp(C.byref(m), C.byref(kv), None, cu, 2, C.byref(bo), None, None, None, None, None, 0, None, C.byref(lp)) == -1
    assert needle in lib.sl_last_error(), (what, lib.sl_last_error())
    assert lib.sl_beam_generate_workspace_bytes_lp(C.byref(m), 20, 2, C.byref(kv), C.byref(bo), C.byref(lp)) == 0 and needle in lib.sl_last_error()


def test_min_new_tokens_above_the_budget_and_too_many_eos_ids_are_refused():
    lib = L.lib()
    lp = _lp(mn=9)
    o = L.GenerateOpts()
    o.max_new_tokens = 8
    assert lib.sl_generate_lp(None, None, None, None, 2, C.byref(o), None, None, None, 0, None, C.byref(lp)) == -1
    assert b"min_new_tokens 9 exceeds max_new_tokens 8" in lib.sl_last_error(), lib.sl_last_error()
    m, kv, bo = L.LlamaModel(), L.KVCache(), L.BeamOpts()
    m.vocab, kv.slots, kv.max_ctx = 1000, 64, 48
    bo.num_beams, bo.num_return_sequences, bo.max_new_tokens = 2, 1, 8
    cu = (C.c_int32 * 3)(0, 10, 20)
    assert lib.sl_beam_generate_lp(C.byref(m), C.byref(kv), None, cu, 2, C.byref(bo), None, None, None, None, None, 0, None, C.byref(lp)) == -1
    assert b"exceeds max_new_tokens" in lib.sl_last_error()
    eos = (C.c_int32 * 9)(*range(9))
    ok = _lp(p=1.2)
    assert lib.sl_logits_process(1, 4, 100, 1, 8, 1, None, C.byref(ok), eos, 9, 0, 1, None) == -1 and b"eos ids" in lib.sl_last_error()
    assert lib.sl_logits_process(1, 4, 100, 1, 8, 1, None, C.byref(ok), eos, -1, 0, 1, None) == -1
    assert lib.sl_logits_process(1, 4, 100, 1, 8, 1, None, None, eos, 1, 0, 1, None) == -1 and b"null options" in lib.sl_last_error()
    assert lib.sl_logits_process(None, 4, 100, 1, 8, 1, None, C.byref(ok), eos, 1, 0, 1, None) == -1
    assert lib.sl_logits_process(1, 0, 100, 1, 8, 1, None, C.byref(ok), eos, 1, 0, 1, None) == -1
    assert lib.sl_logits_process(1, 4, 100, 1, -1, 1, None, C.byref(ok), eos, 1, 0, 1, None) == -1
    assert lib.sl_logits_process(1, 4, 100, 1, 8, 1, None, C.byref(ok), eos, 1, 0, None, None) == -1 and b"scratch" in lib.sl_last_error()
    assert lib.sl_beam_topk_ex(1, 4, 100, None, 65, 1, 1, None, 1) == -1 and b"M = 65" in lib.sl_last_error()


def test_workspace_grows_by_the_scratch_only_when_the_penalty_is_on():
    lib = L.lib()
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab, m.rope_len = L.SL_F32, 256, 2, 2, 2, 128, 384, 1000, 64
    base = lib.sl_generate_workspace_bytes(C.byref(m), 40, 4, 16)
    assert lib.sl_generate_workspace_bytes_lp(C.byref(m), 40, 4, 16, None) == base
    assert lib.sl_generate_workspace_bytes_lp(C.byref(m), 40, 4, 16, C.byref(_lp())) == base
    assert lib.sl_generate_workspace_bytes_lp(C.byref(m), 40, 4, 16, C.byref(_lp(g=3, mn=2))) == base
    assert lib.sl_generate_workspace_bytes_lp(C.byref(m), 40, 4, 16, C.byref(_lp(p=1.2))) == base + 4 * 16 * 4 + 256
    kv, bo = L.KVCache(), L.BeamOpts()
    kv.slots, kv.max_ctx = 64, 48
    bo.num_beams, bo.num_return_sequences, bo.max_new_tokens = 2, 1, 8
    b0 = lib.sl_beam_generate_workspace_bytes(C.byref(m), 40, 4, C.byref(kv), C.byref(bo))
    assert b0 > 0 and lib.sl_beam_generate_workspace_bytes_lp(C.byref(m), 40, 4, C.byref(kv), C.byref(bo), None) == b0
    assert lib.sl_beam_generate_workspace_bytes_lp(C.byref(m), 40, 4, C.byref(kv), C.byref(bo), C.byref(_lp())) == b0
    assert lib.sl_beam_generate_workspace_bytes_lp(C.byref(m), 40, 4, C.byref(kv), C.byref(bo), C.byref(_lp(p=1.2, g=2))) > b0


# ------------------------------------------------------------------------------------------------ the restatement against transformers
def _histories(V, gen):
    """token lists with duplicates (one token 40 times), lengths around g, ids 0 and V - 1"""
    hs = [[], [5], [0, V - 1], [7, 7, 7], [3, 4, 3, 4, 3]]
    long = torch.randint(0, V, (60,), generator=gen).tolist()
    long[10:50] = [11] * 40
    hs.append(long)
    rep = torch.randint(0, 6, (37,), generator=gen).tolist()          # a six-token alphabet: every n-gram repeats
    hs.append(rep)
    return hs


@pytest.mark.parametrize("g", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("p", [1.0, 1.3, 0.7])
def test_restatement_equals_the_transformers_processors(p, g):
    import transformers.generation.logits_process as lp_mod
    V, eos, min_new = 50, [2, 9], 4
    gen = torch.Generator().manual_seed(100 * g + int(10 * p))
    for hist in _histories(V, gen):
        scores = torch.randn(V, generator=gen) * 3.0                     # negative and positive
        scores[torch.randint(0, V, (5,), generator=gen)] = float("-inf")
        scores[0], scores[V - 1] = -1.25, 2.5
        ids = torch.tensor([hist], dtype=torch.long)
        want = scores[None].clone()
        if p != 1.0:
            want = lp_mod.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, want)
        if g > 0:
            want = lp_mod.NoRepeatNGramLogitsProcessor(g)(ids, want)
        want = lp_mod.MinNewTokensLengthLogitsProcessor(0, min_new, eos, device="cpu")(ids, want)
        got = lpr.process_row(scores, hist, p, g, min_new, eos)
        assert torch.equal(got, want[0]), (p, g, hist)
        assert torch.equal(torch.isinf(got), torch.isinf(want[0]))


def test_a_duplicated_token_is_penalised_once_and_a_ban_overrides_the_penalty():
    s = torch.tensor([2.0, -2.0, 1.0, 4.0])
    out = lpr.process_row(s, [0, 0, 1, 1, 0], p=2.0)
    assert out.tolist() == [1.0, -4.0, 1.0, 4.0]
    out = lpr.process_row(s, [0, 3, 0], p=2.0, g=2)                    # ... 0 was followed by 3: banned, although penalised first
    assert out.tolist() == [1.0, -2.0, 1.0, float("-inf")]
    assert lpr.process_row(s, [0], g=2).tolist() == s.tolist()            # n < g: nothing
    assert lpr.process_row(s, [2, 1], g=1).tolist() == [2.0, float("-inf"), float("-inf"), 4.0]


# ------------------------------------------------------------------------------------------------ the fixture
def _case(name):
    g = golden("logits_proc_tiny")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def test_fixture_holds_the_cases_and_data_only():
    g = golden("logits_proc_tiny")
    assert list(g["cases"]) == CASES
    assert all(v.dtype.kind in "iufbU" for v in g.values())


@pytest.mark.parametrize("name", CASES)
def test_fixture_meets_the_conditions_the_generator_asserted(name):
    c = _case(name)
    ids, plain, lens, plens = t(c["ids"]).long(), t(c["plain_ids"]).long(), c["lens"].tolist(), c["plain_lens"].tolist()
    assert not torch.equal(ids, plain)
    assert float(c["min_margin"]) >= 1e-3 and float(c["plain_min_margin"]) >= 1e-3
    B = int(c["batch"])
    g, mn = int(c["no_repeat_ngram_size"]), int(c["min_new_tokens"])
    if g > 0:
        assert not any(lpr.has_repeated_ngram(ids[b, :lens[b]].tolist(), g) for b in range(B))
        if mn == 0:
            assert any(lpr.has_repeated_ngram(plain[b, :plens[b]].tolist(), 2) for b in range(B))
    if mn > 0:
        eos = set(c["eos"].tolist())
        assert len(eos) > 0 and max(plens) < 6 and min(lens) >= mn
        for b in range(B):
            assert not (set(ids[b, :mn].tolist()) & eos)
            assert int(plain[b, plens[b] - 1]) in eos
    kind = name.split("_", 2)[2]
    want = dict(rep13=(1.3, 0, 0, 1), ngram2=(1.0, 2, 0, 1), minnew6=(1.0, 0, 6, 1), all3=(1.3, 2, 6, 1), beam_k3=(1.2, 2, 0, 3))[kind]
    assert (round(float(c["repetition_penalty"]), 6), g, mn, int(c["K"])) == want


# ------------------------------------------------------------------------------------------------ config and keyword plumbing
def test_runtime_logits_parsing_and_the_shipped_yamls_are_off():
    for name in sorted(os.listdir(os.path.join(REPO, "config"))):
        if name.endswith(".yaml"):
            conf = cfgm.load_config(os.path.join(REPO, "config", name))
            assert cfgm.runtime_logits(conf) is None, name
            assert (conf.runtime.repetition_penalty, conf.runtime.no_repeat_ngram_size, conf.runtime.min_new_tokens) == (1.0, 0, 0)
    assert cfgm.runtime_logits(cfgm.from_dict(dict(model={}))) is None
    assert cfgm.runtime_logits(cfgm.from_dict(dict(runtime=dict(repetition_penalty=1.2)))) == dict(repetition_penalty=1.2, no_repeat_ngram_size=0, min_new_tokens=0)
    assert cfgm.runtime_logits(cfgm.from_dict(dict(runtime=dict(no_repeat_ngram_size=3, min_new_tokens=4)))) == dict(repetition_penalty=1.0, no_repeat_ngram_size=3,
                                                                                                                   min_new_tokens=4)
    for bad in (dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty="x"), dict(repetition_penalty=float("inf")),
                dict(repetition_penalty=True), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.5), dict(min_new_tokens=-3), dict(min_new_tokens=True)):
        with pytest.raises(ValueError):
            cfgm.runtime_logits(cfgm.from_dict(dict(runtime=bad)))


def _tiny_llm():
    from oracle.golden_cfgs import TINY_MHA as LC
    weights = pkg("weights")
    larch = weights.LlamaArch(LC.hidden_size, LC.num_hidden_layers, LC.num_attention_heads, LC.num_key_value_heads, LC.head_dim,
                              LC.intermediate_size, LC.vocab_size, LC.rms_norm_eps, LC.rope_theta, LC.rope_scaling,
                              LC.tie_word_embeddings, tuple(LC.eos_token_ids), LC.pad_token_id)
    return pkg("audio_llama").AudioLlamaForCausalLM(larch, {}, torch_dtype=torch.float32, max_ctx=64)


class _Recorder:
    """stands in for generate_packed: keeps what generate() hands over"""

    def __init__(self, llm):
        self.calls = []
        llm._w = object()
        llm._dev = lambda: llm._w
        llm.generate_packed = self

    def __call__(self, x, lens, max_new_tokens, **kw):
        self.calls.append(kw)
        return torch.zeros(len(lens), max_new_tokens, dtype=torch.int32), max_new_tokens


def test_generate_keywords_reach_generate_packed_and_the_defaults_build_none():
    llm = _tiny_llm()
    g = llm.generation_config
    assert (g.repetition_penalty, g.no_repeat_ngram_size, g.min_new_tokens) == (1.0, 0, 0)      # HF's defaults
    rec = _Recorder(llm)
    x = torch.zeros(2, 4, 256)
    llm.generate(inputs_embeds=x, max_new_tokens=8)
    assert rec.calls[-1]["logits"] is None
    llm.generate(inputs_embeds=x, max_new_tokens=8, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    assert rec.calls[-1]["logits"] is None
    llm.generate(inputs_embeds=x, max_new_tokens=8, repetition_penalty=1.2)
    assert rec.calls[-1]["logits"] == dict(repetition_penalty=1.2, no_repeat_ngram_size=0, min_new_tokens=0)
    llm.generate(inputs_embeds=x, max_new_tokens=8, no_repeat_ngram_size=3, min_new_tokens=5, num_beams=2)
    assert rec.calls[-1]["logits"] == dict(repetition_penalty=1.0, no_repeat_ngram_size=3, min_new_tokens=5) and rec.calls[-1]["beams"]["num_beams"] == 2
    g.repetition_penalty = 1.1                                     # generation_config is the fallback of a keyword left at None
    llm.generate(inputs_embeds=x, max_new_tokens=8)
    assert rec.calls[-1]["logits"]["repetition_penalty"] == 1.1
    llm.generate(inputs_embeds=x, max_new_tokens=8, repetition_penalty=1.0)
    assert rec.calls[-1]["logits"] is None
    assert llm._logits_struct(None, 8) is None and llm._logits_struct(dict(repetition_penalty=1.0), 8) is None
    lp = llm._logits_struct(dict(repetition_penalty=1.5, min_new_tokens=2), 8)
    assert (round(lp.repetition_penalty, 6), lp.no_repeat_ngram_size, lp.min_new_tokens) == (1.5, 0, 2)


def test_values_outside_the_limits_raise_with_the_limit_in_the_text():
    llm = _tiny_llm()
    _Recorder(llm)
    x = torch.zeros(1, 4, 256)
    for kw, needle in ((dict(repetition_penalty=0.0), "> 0"), (dict(repetition_penalty=float("nan")), "finite"), (dict(no_repeat_ngram_size=-1), ">= 0"),
                       (dict(min_new_tokens=-1), ">= 0"), (dict(min_new_tokens=9), "max_new_tokens=8"), (dict(no_repeat_ngram_size=2.5), "integer")):
        with pytest.raises(L.SpeechLLMError, match=needle):
            llm.generate(inputs_embeds=x, max_new_tokens=8, **kw)
    with pytest.raises(L.SpeechLLMError, match="unknown keys"):
        llm._logits_struct(dict(penalty=1.2), 8)


def test_a_yaml_with_runtime_repetition_penalty_reaches_generate_packed(tmp_path):
    inference = pkg("inference")
    path = tmp_path / "conf.yaml"
    path.write_text(open(os.path.join(REPO, "config", "llama3_hubert.yaml")).read().replace("repetition_penalty: 1.0", "repetition_penalty: 1.25")
                    .replace("min_new_tokens: 0", "min_new_tokens: 3"))
    conf = cfgm.load_config(str(path))
    llm = _tiny_llm()
    rec = _Recorder(llm)
    inf = inference.LLMSpeechTextInference.__new__(inference.LLMSpeechTextInference)       # the constructor needs a GPU: the plumbing does not
    inf.llm, inf.beams, inf.logits = llm, cfgm.runtime_beams(conf), cfgm.runtime_logits(conf)
    inf.llm_tokenizer = type("Tok", (), {"batch_decode": staticmethod(lambda ids, **kw: ["" for _ in ids])})()
    inf.generate_llm_response(torch.zeros(1, 4, 256), max_new_tokens=8)
    assert rec.calls[-1]["logits"] == dict(repetition_penalty=1.25, no_repeat_ngram_size=0, min_new_tokens=3)
    inf.generate_llm_response(torch.zeros(1, 4, 256), max_new_tokens=8, repetition_penalty=1.0, min_new_tokens=0)      # a keyword overrides the config
    assert rec.calls[-1]["logits"] is None
