"""CPU (no GPU): the host side of teacher-forced scoring — header / ctypes mirror / exports, the argument refusals of
sl_llama_score and sl_gemm_top1_lse_tgt (they return before any launch), the workspace arithmetic, score()'s host bookkeeping against a
brute-force restatement, the Python refusals, and the Trainer's opt-in switch."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO, pkg

L = pkg("_lib")
llama_mod = pkg("audio_llama")
cfgm = pkg("config")
trainer_mod = pkg("trainer")

NEW_EXPORTS = ["sl_gemm_top1_lse_tgt", "sl_score_finalize", "sl_score_rows", "sl_score_segment_sums", "sl_llama_score_workspace_bytes", "sl_llama_score",
               "sl_llama_score_last_paths"]
HDR = open(os.path.join(REPO, "include", "speechllm.h")).read()
FAKE = 1 << 20          # a non-null, 16-byte aligned pointer the argument checks never dereference
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _err():
    return L.lib().sl_last_error().decode()


# ------------------------------------------------------------------------------------------------ header, exports
def test_header_declares_the_new_entries_and_the_abi_stays_7():
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", HDR))
    assert set(NEW_EXPORTS) <= declared and set(NEW_EXPORTS) <= set(L.EXPORTS)
    lib = L.lib()
    assert lib.sl_version() == 7 and "SL_ABI_VERSION 7" in re.sub(r"\s+", " ", HDR)
    for name in NEW_EXPORTS:
        getattr(lib, name)
    m = re.search(r"typedef struct \{([^}]*)\}\s*sl_score_opts;", HDR)
    assert m and re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split() == ["int32_t", "row_chunk;", "int32_t", "force_path;", "int32_t", "reserved[6];"]
    assert C.sizeof(L.ScoreOpts) == 32 and [f[0] for f in L.ScoreOpts._fields_] == ["row_chunk", "force_path", "reserved"]


def _c_params(name):
    m = re.search(r"\b(?:int|size_t|int32_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", HDR, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
    return [] if body == "void" else [p.strip() for p in body.split(",")]


@pytest.mark.parametrize("name", NEW_EXPORTS)
def test_argtypes_match_the_header(name):
    res, args = L._PROTOS[name]
    params = _c_params(name)
    assert len(params) == len(args), (name, params)
    assert res is (L.c_sz if re.search(r"\bsize_t\s+" + name + r"\s*\(", HDR) else L.c_i32)
    scalars = {"int32_t": L.c_i32, "int64_t": L.c_i64, "size_t": L.c_sz, "float": L.c_f32}
    structs = {"sl_llama_model": L.LlamaModel, "sl_kv_cache": L.KVCache, "sl_gemm_args": L.GemmArgs, "sl_gemm_ex_args": L.GemmEx, "sl_score_opts": L.ScoreOpts}
    for p, a in zip(params, args):
        if "*" in p or p.startswith("sl_stream"):
            base = re.sub(r"\bconst\b", "", p).split("*")[0].strip()
            if base in structs:
                assert a is C.POINTER(structs[base]), (name, p)
            else:
                assert a is L.c_vp or (isinstance(a, type) and issubclass(a, C._Pointer)), (name, p)
        else:
            assert a is scalars[p.split()[0]], (name, p)


# ------------------------------------------------------------------------------------------------ refusals of the C entries
def test_gemm_top1_lse_tgt_refuses_half_a_pair_and_keeps_the_older_checks():
    lib = L.lib()
    a, ex = L.GemmArgs(), L.GemmEx()
    a.A, a.W, a.lda, a.ldw, a.M, a.N, a.K, a.batch, a.dtype, a.out_f32 = FAKE, FAKE, 64, 64, 128, 128, 64, 1, L.SL_BF16, 1
    ex.w_mod = 1
    assert lib.sl_gemm_top1_lse_tgt(C.byref(a), None, FAKE, FAKE, FAKE, None) == ERR_ARG                       # no ex args
    assert lib.sl_gemm_top1_lse_tgt(C.byref(a), C.byref(ex), FAKE, FAKE, FAKE, None) == ERR_ARG and "amax_val" in _err()      # planes missing
    ex.amax_val, ex.amax_idx = FAKE, FAKE
    assert lib.sl_gemm_top1_lse_tgt(C.byref(a), C.byref(ex), None, FAKE, FAKE, None) == ERR_ARG                # no third plane
    assert lib.sl_gemm_top1_lse_tgt(C.byref(a), C.byref(ex), FAKE, FAKE, None, None) == ERR_ARG
    assert "come together" in _err() and "tgt_val NULL" in _err()
    assert lib.sl_gemm_top1_lse_tgt(C.byref(a), C.byref(ex), FAKE, None, FAKE, None) == ERR_ARG
    assert "come together" in _err() and "tgt_col NULL" in _err()
    a.M = 64
    assert lib.sl_gemm_top1_lse_tgt(C.byref(a), C.byref(ex), FAKE, FAKE, FAKE, None) == ERR_ARG and "M > 64" in _err() and "M=64" in _err()


def _model(dtype=L.SL_F32, hidden=256, ffn=384, n_layers=2, vocab=1000):
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab = dtype, hidden, n_layers, 2, 2, 128, ffn, vocab
    m.rms_eps, m.rope_len = 1e-5, 512
    layers = (L.LlamaLayer * n_layers)()
    for lay in layers:
        for name, _ in L.LlamaLayer._fields_:
            setattr(lay, name, FAKE)
    m.layers = layers
    m._keep = layers
    for f in ("embed", "lm_head", "final_norm", "rope_cos", "rope_sin"):
        setattr(m, f, FAKE)
    return m


def _kv(slots=8, max_ctx=64):
    kv = L.KVCache()
    kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx = FAKE, FAKE, slots, max_ctx
    return kv


def _score(m=None, kv=None, lens=(10, 12), start=(3, 0), n=(4, 12), opts=None, ws_bytes=1 << 40, **ptr):
    m, kv = m or _model(), kv or _kv()
    nseq = len(lens)
    cu = [0]
    for v in lens:
        cu.append(cu[-1] + v)
    p = dict(x=FAKE, labels=FAKE, logprob=FAKE, top1=FAKE, ssum=FAKE, scnt=FAKE, shit=FAKE, ws=FAKE)
    p.update(ptr)
    return L.lib().sl_llama_score(C.byref(m), C.byref(kv), p["x"], (C.c_int32 * (nseq + 1))(*cu), nseq, (C.c_int32 * nseq)(*start), (C.c_int32 * nseq)(*n),
                                  p["labels"], p["logprob"], p["top1"], p["ssum"], p["scnt"], p["shit"], None if opts is None else C.byref(opts), p["ws"],
                                  ws_bytes, None)


def test_llama_score_refuses_bad_arguments_before_any_launch():
    for name in ("x", "labels", "logprob", "ws"):
        assert _score(**{name: None}) == ERR_ARG and "null pointer" in _err(), name
    assert _score(n=(4, -2)) == ERR_ARG and "n_score -2 of sequence 1" in _err()
    assert _score(start=(-1, 0)) == ERR_ARG and "score_start -1 of sequence 0" in _err()
    assert _score(start=(7, 0)) == ERR_ARG and "sequence 0" in _err() and "[7, 7 + 4)" in _err() and "10 rows" in _err()
    assert _score(n=(0, 0)) == ERR_ARG and "nothing to score" in _err()
    assert _score(ssum=None) == ERR_ARG and "all three or none" in _err() and "(NULL, set, set)" in _err()
    assert _score(shit=None) == ERR_ARG and "(set, set, NULL)" in _err()
    o = L.ScoreOpts()
    o.row_chunk = -5
    assert _score(opts=o) == ERR_ARG and "row_chunk -5" in _err()
    o.row_chunk, o.force_path = 0, 3
    assert _score(opts=o) == ERR_ARG and "force_path 3" in _err()
    need = L.lib().sl_llama_score_workspace_bytes(C.byref(_model()), 22, 2, 16, None)
    assert need > 0
    assert _score(ws_bytes=need - 1) == ERR_ARG and f"workspace {need - 1} B < required {need} B" in _err()
    # the cache: too few slots, too small a max_ctx
    assert _score(kv=_kv(slots=1)) == ERR_UNSUPPORTED and "2 sequences" in _err() and "has 1" in _err()
    assert _score(kv=_kv(max_ctx=11)) == ERR_UNSUPPORTED and "sequence 1 length 12 outside (0, max_ctx=11]" in _err()
    assert _score(lens=(10, 0), start=(3, 0), n=(4, 0)) == ERR_ARG and "sequence 1 length 0" in _err()
    m = _model()
    m.lm_head = None
    assert _score(m=m) == ERR_ARG and "null model field" in _err()
    # the e4m3 K/V format is for 16-bit models only: refused for float32 in the words every llama entry uses
    kv8 = _kv()
    kv8.reserved = L.KV_FP8_E4M3
    assert _score(kv=kv8) == ERR_UNSUPPORTED


def test_workspace_is_monotone_zero_on_bad_arguments_and_the_planes_stop_growing():
    lib = L.lib()
    m = _model(L.SL_BF16, vocab=128256, hidden=3072, ffn=8192)

    def ws(n_tok, n_rows, chunk=0, force=0, nseq=4):
        o = L.ScoreOpts()
        o.row_chunk, o.force_path = chunk, force
        return lib.sl_llama_score_workspace_bytes(C.byref(m), n_tok, nseq, n_rows, C.byref(o))

    assert ws(8000, 100) == lib.sl_llama_score_workspace_bytes(C.byref(m), 8000, 4, 100, None) > lib.sl_llama_workspace_bytes(C.byref(m), 8000, 4)
    for bad in (dict(n_tok=0, n_rows=1), dict(n_tok=100, n_rows=0), dict(n_tok=100, n_rows=101), dict(n_tok=100, n_rows=10, chunk=-1),
                dict(n_tok=100, n_rows=10, force=3), dict(n_tok=100, n_rows=10, nseq=0)):
        assert ws(**bad) == 0 and "sl_llama_score_workspace_bytes" in _err(), bad
    assert lib.sl_llama_score_workspace_bytes(None, 100, 4, 10, None) == 0
    rows = [1, 63, 64, 65, 100, 2047, 2048, 2049, 5000, 8000]
    for force in (0, 1, 2):
        sizes = [ws(8000, r, force=force) for r in rows]
        assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])), (force, sizes)
        toks = [ws(t_, 1000, force=force) for t_ in (1000, 1001, 4000, 8000)]
        assert all(b >= a for a, b in zip(toks, toks[1:]))
        chunks = [ws(8000, 5000, chunk=c, force=force) for c in (1, 32, 64, 65, 128, 1000, 2048, 4096, 5000, 6000)]
        assert all(b >= a for a, b in zip(chunks, chunks[1:])), (force, chunks)
    assert ws(8000, 5000) == ws(8000, 5000, chunk=2048)                          # 0 = the default of 2 048 rows
    # once n_rows > row_chunk the planes (and the fp32 logits of the unfused remainder) are as large as they get: what still grows is the
    # per-row share — the gathered hidden rows, the row list and the top-1 scratch
    per_row = 3072 * 2 + 4 + 4
    for chunk in (128, 2048):
        a, b = ws(8000, chunk + 1, chunk=chunk), ws(8000, 8000, chunk=chunk)
        assert abs((b - a) - (8000 - chunk - 1) * per_row) <= 3 * 256, (chunk, a, b)      # three pieces, each rounded up to 256 B
    ng = (128256 + 63) // 64
    assert ng == 2004
    planes = ws(8000, 3000, chunk=2048) - ws(8000, 3000, chunk=64)               # chunk 64: no pass is fused, no planes
    assert abs(planes - 2048 * (12 * ng + 4)) <= 3 * 256                           # 12 B x 2 004 groups per row + the target logit: 49.3 MB
    assert ws(8000, 3000, chunk=2048, force=1) - ws(8000, 3000, chunk=2048) > 2048 * 128256 * 4 - 2048 * (12 * ng + 4) - 64 * 128256 * 4 - 1024


# ------------------------------------------------------------------------------------------------ score(): host bookkeeping
def _brute(prompt_lens, targets, cap, pad):
    """the same plan restated token by token"""
    calls, cur = [], None
    for b, (P, tg) in enumerate(zip(prompt_lens, targets)):
        if cur is None or len(cur["seqs"]) == cap:
            cur = dict(seqs=[], lens=[], score_start=[], n_score=[], labels=[], input_ids=[])
            calls.append(cur)
        cur["seqs"].append(b)
        rows = ["p"] * P                      # the sequence, row by row: prompt rows, then one row per fed target token
        for j, tok in enumerate(tg):
            cur["labels"].append(tok)         # ... row P - 1 + j predicts target[j]
            if j + 1 < len(tg):
                rows.append(tok if tok >= 0 else pad)
        cur["input_ids"] += rows[P:]
        cur["lens"].append(len(rows))
        cur["score_start"].append(P - 1)
        cur["n_score"].append(len(tg))
    return calls


def test_score_plan_matches_a_brute_force_restatement_on_ragged_inputs():
    gen = torch.Generator().manual_seed(3)
    prompt_lens = [9, 21, 14, 1, 30, 7, 12]
    tlens = [5, 1, 13, 4, 2, 9, 6]                      # sequence 1: a one-token target
    targets = [torch.randint(0, 1000, (n,), generator=gen).tolist() for n in tlens]
    targets[2][0], targets[2][5], targets[2][12] = -100, -100, -100      # ignored positions: first, inside, last
    targets[5][3] = -1
    for cap in (1, 3, 7, 100):
        plan = llama_mod.score_plan(prompt_lens, targets, 64, cap, pad_id=11)
        assert plan == _brute(prompt_lens, targets, cap, 11), cap
        assert [len(c["seqs"]) for c in plan] == [min(cap, 7 - i) for i in range(0, 7, cap)]
        for c in plan:
            assert sum(c["n_score"]) == len(c["labels"]) and sum(c["lens"]) - sum(prompt_lens[b] for b in c["seqs"]) == len(c["input_ids"])
            assert all(s + n <= ln for s, n, ln in zip(c["score_start"], c["n_score"], c["lens"]))
            assert all(v >= 0 for v in c["input_ids"])
    one = llama_mod.score_plan(prompt_lens, targets, 64, 100, pad_id=11)[0]
    assert one["lens"][1] == 21 and one["n_score"][1] == 1                                   # a one-token target appends nothing
    assert one["labels"][5 + 1:5 + 1 + 13][0] == -100 and 11 in one["input_ids"]


def test_score_refuses_before_any_device_work():
    arch = SimpleNamespace(vocab_size=1000, hidden_size=256, num_hidden_layers=1, eos_token_ids=(), pad_token_id=0)
    llm = llama_mod.AudioLlamaForCausalLM(arch, {}, torch_dtype=torch.float32, max_ctx=16)      # weights never leave the host: _dev() would raise
    p = [torch.zeros(4, 256)]
    with pytest.raises(L.SpeechLLMError, match="empty target"):
        llm.score(p, [torch.zeros(0, dtype=torch.long)])
    with pytest.raises(L.SpeechLLMError, match="zero rows"):
        llm.score([torch.zeros(0, 256)], [torch.tensor([1, 2])])
    with pytest.raises(L.SpeechLLMError, match="exceed max_ctx=16"):
        llm.score(p, [torch.arange(14)])
    with pytest.raises(L.SpeechLLMError, match="1 prompts for 2 targets"):
        llm.score(p, [torch.tensor([1]), torch.tensor([2])])
    with pytest.raises(L.SpeechLLMError, match="row_chunk=-1"):
        llm.score(p, [torch.tensor([1, 2])], row_chunk=-1)
    with pytest.raises(L.SpeechLLMError, match="force_path=5"):
        llm.score(p, [torch.tensor([1, 2])], force_path=5)
    with pytest.raises(L.SpeechLLMError, match="not on the GPU"):      # a well-formed call gets as far as the device check and no further
        llm.score(p, [torch.arange(13)])
    # a left-padded (B, S, H) tensor with its mask is taken apart like generate()'s
    with pytest.raises(L.SpeechLLMError, match="sequence 1: .*exceed max_ctx=16"):
        llm.score(torch.zeros(2, 8, 256), [torch.arange(3), torch.arange(14)], attention_mask=torch.tensor([[0] * 4 + [1] * 4, [0] * 4 + [1] * 4]))


def test_score_output_reductions():
    out = llama_mod.ScoreOutput([torch.tensor([-1.0, -2.0]), torch.tensor([-3.0, 0.0, -1.0])], torch.tensor([-3.0, -4.0]), torch.tensor([2, 2]))
    assert out.nll.tolist() == [1.5, 2.0]
    assert abs(out.perplexity() - math.exp(1.75)) < 1e-12


# ------------------------------------------------------------------------------------------------ Trainer: opt-in only
class _StubLLM:
    def __init__(self):
        self.model = SimpleNamespace(embed_tokens=lambda ids: torch.zeros(*ids.shape, 8))
        self.forward_calls, self.score_calls = 0, []

    def __call__(self, inputs_embeds=None, labels=None):
        self.forward_calls += 1
        return SimpleNamespace(loss=torch.tensor(0.5 * self.forward_calls))

    def score(self, prompts, targets):
        self.score_calls.append((len(prompts), [int(p.shape[0]) for p in prompts], [t_.tolist() for t_ in targets]))
        n = len(prompts)
        return llama_mod.ScoreOutput([None] * n, -torch.ones(n) * 3.0, torch.full((n,), 2))


def _stub_trainer(log):
    tr = object.__new__(trainer_mod.Trainer)
    tr.llm = _StubLLM()
    tr.device, tr.rank, tr.world, tr.dist, tr.step = torch.device("cpu"), 1, 2, None, 0      # rank 1 of 2: no generation, no checkpoint
    tr.prefix_ids, tr.suffix_ids = torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long)
    tr.val_dataset = list(range(7))
    tr.config = cfgm.from_dict(dict(log=log))
    tr._val_sample = lambda i: (torch.zeros(1, 5 + i, 8), torch.arange(4), torch.arange(10, 16 + i), f"t{i}")
    tr._rng_states = lambda: {}
    return tr


def test_trainer_without_the_key_never_calls_score_and_with_it_batches_the_samples():
    tr = _stub_trainer(dict(num_generate_samples=0))

    def boom(*a, **k):
        raise AssertionError("score() called without log.validation_batch_size")

    tr.llm.score = boom
    out = tr.validate(0)
    assert tr.llm.forward_calls == 6                                  # samples 1, 3, 5 of this rank, audio and text prompt each
    assert abs(out["validation/audio_perplexity"] - math.exp((0.5 + 1.5 + 2.5) / 3)) < 1e-12
    assert abs(out["validation/text_perplexity"] - math.exp((1.0 + 2.0 + 3.0) / 3)) < 1e-12
    tr = _stub_trainer(dict(num_generate_samples=0, validation_batch_size=2))
    out = tr.validate(0)
    assert tr.llm.forward_calls == 0
    # batches of [1, 3] and [5], the audio then the text prompt; prompt rows = prefix 3 + (5 + i | 4) + suffix[1:] 2; targets = resp[1:]
    assert [c[0] for c in tr.llm.score_calls] == [2, 2, 1, 1]
    assert tr.llm.score_calls[0][1] == [3 + 6 + 2, 3 + 8 + 2] and tr.llm.score_calls[1][1] == [9, 9]
    assert tr.llm.score_calls[0][2] == [list(range(11, 17)), list(range(11, 19))] and tr.llm.score_calls[2][2] == [list(range(11, 21))]
    assert abs(out["validation/audio_perplexity"] - math.exp(1.5)) < 1e-12 and abs(out["validation/text_perplexity"] - math.exp(1.5)) < 1e-12
