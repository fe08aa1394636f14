"""GPU: beam search — the selection, step and cache re-ordering kernels against torch / tests/beam_ref.py, and sl_beam_generate end to
end against what the reference class returned (tests/golden/beam_tiny.npz)."""
import ctypes as C
import itertools

import pytest
import torch

from conftest import golden, pkg, t
from oracle.golden_cfgs import TINY_LLAMA, TINY_MHA

import beam_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = pkg("_lib")
ri = pkg("random_init")
weights = pkg("weights")
llama_mod = pkg("audio_llama")

CASES = ["mha_k2_eos", "mha_k3_eos_early", "mha_k3_eos_lp2", "mha_k4", "gqa_k2_eos_lp2", "gqa_k4", "mha_k3_eos_never", "mha_k3_eos_r3"]
ES = {0: False, 1: True, 2: "never"}
CFG = {"tiny_mha": TINY_MHA, "tiny_gqa": TINY_LLAMA}
GUARD = 0x5A5A5A5A
# |score * len**length_penalty - sum of the chosen tokens' log-probabilities recomputed by forward()|, largest over the returned hypotheses
# of test_16bit_scores_are_the_sums_of_the_chosen_log_probabilities, as measured on an MI355X; the test asserts 2x these
SUM_LOGPROB_DIFF_MEASURED = {torch.float32: 8.799e-06, torch.bfloat16: 4.540e-02, torch.float16: 1.282e-02}

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


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sl_beam_topk
def _topk(logits, score, M):
    rows, V = logits.shape
    val = torch.full((rows * M + 16,), float("nan"), device=DEV)
    tok = torch.full((rows * M + 16,), GUARD, dtype=torch.int32, device=DEV)
    val[rows * M:] = 12345.0
    L.check(L.lib().sl_beam_topk(logits.data_ptr(), rows, V, L.ptr(score), M, val.data_ptr(), tok.data_ptr(), L.stream_ptr()), "sl_beam_topk")
    _sync()
    assert bool((val[rows * M:] == 12345.0).all()) and bool((tok[rows * M:] == GUARD).all()), "guard words after the outputs were written"
    return val[:rows * M].view(rows, M).cpu(), tok[:rows * M].view(rows, M).cpu().long()


@pytest.mark.parametrize("V", [777, 1000, 128256])
@pytest.mark.parametrize("M", [2, 8, 64])
def test_beam_topk_matches_torch_topk_of_log_softmax_plus_score(V, M):
    g = torch.Generator().manual_seed(V + M)
    rows = 5
    logits = torch.stack([(torch.arange(V, dtype=torch.float32) * 1e-2)[torch.randperm(V, generator=g)] for _ in range(rows)])
    score = -torch.rand(rows, generator=g) * 5.0
    val, tok = _topk(logits.to(DEV), score.to(DEV), M)
    want = torch.topk(torch.log_softmax(logits.double(), dim=-1) + score.double()[:, None], M, dim=-1)
    assert torch.equal(tok, want.indices)
    assert float((val.double() - want.values).abs().max()) <= 1e-5
    # the same row gives the same output on every run (no float atomics, one summation order)
    val2, tok2 = _topk(logits.to(DEV), score.to(DEV), M)
    assert torch.equal(val, val2) and torch.equal(tok, tok2)


def test_beam_topk_tie_rule_minus_infinity_and_nan():
    V, M = 1000, 8
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(4, V, generator=g)
    logits[0] = 0.25                                              # all equal: the lowest indices, in order
    logits[1, :] = float("-inf")
    finite = torch.tensor([900, 17, 333, 4, 512])
    logits[1, finite] = torch.tensor([3.0, 2.0, 1.0, 0.5, 0.0])   # five finite entries, M = 8: then -inf entries by index
    top = int(logits[2].argmax())
    logits[2, top] = float("nan")                                 # a NaN where the maximum was
    logits[3, 5] = float("nan")
    logits[3, 6] = float("-inf")
    val, tok = _topk(logits.to(DEV), None, M)
    assert tok[0].tolist() == list(range(M)) and bool((val[0] == val[0, 0]).all())
    assert tok[1, :5].tolist() == finite.tolist() and tok[1, 5:].tolist() == [0, 1, 2] and bool(torch.isinf(val[1, 5:]).all())
    assert not bool(torch.isnan(val).any())
    assert top not in tok[2].tolist() and 5 not in tok[3].tolist()
    clean = torch.where(torch.isnan(logits), torch.tensor(float("-inf")), logits)
    for r in (2, 3):
        want = torch.topk(torch.log_softmax(clean[r].double(), dim=-1), M)
        assert torch.equal(tok[r], want.indices) and float((val[r].double() - want.values).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ sl_beam_step
class _DevBeam:
    """device state of sl_beam_step, initialised as the header says"""

    def __init__(self, nseq, K, max_new, lp, prompt_len=7):
        R = nseq * K
        i32 = dict(dtype=torch.int32, device=DEV)
        self.nseq, self.K, self.max_new = nseq, K, max_new
        self.run_score = torch.full((R,), -1.0e9, device=DEV)
        self.run_score[::K] = 0.0
        self.next_ids = torch.zeros(R, **i32)
        self.src_row = torch.zeros(R, **i32)
        self.ctx_len = torch.full((R,), prompt_len, **i32)
        self.hist = [torch.zeros((R, max_new), **i32), torch.zeros((R, max_new), **i32)]
        self.fin_score = torch.full((R,), -1.0e9, device=DEV)
        self.fin_ids = torch.zeros((R, max_new), **i32)
        self.fin_flag = torch.zeros(R, **i32)
        self.fin_len = torch.zeros(R, **i32)
        self.open = torch.ones(nseq, **i32)
        self.seq_done = torch.zeros(nseq, **i32)
        self.step = torch.zeros(nseq, **i32)
        self.len_pen = torch.tensor([float(i + 1) ** lp for i in range(max_new)], dtype=torch.float32).to(DEV)
        s = L.BeamState()
        for f in ("run_score", "next_ids", "src_row", "ctx_len", "fin_score", "fin_ids", "fin_flag", "fin_len", "open", "seq_done", "step", "len_pen"):
            setattr(s, f, getattr(self, f).data_ptr())
        s.hist[0], s.hist[1] = self.hist[0].data_ptr(), self.hist[1].data_ptr()
        self.struct = s


def _rel_close(a, b, tol=1e-6):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= tol * b.abs().clamp(min=1e-30)).all()) or torch.equal(a, b)


def _compare_step_state(d, ref, tstep, prompt_len, what):
    nseq, K = d.nseq, d.K
    _sync()
    assert _rel_close(d.run_score.cpu().view(nseq, K), ref.run_score), what
    assert torch.equal(d.next_ids.cpu().view(nseq, K).long(), ref.next_ids), what
    assert torch.equal(d.src_row.cpu().view(nseq, K).long(), ref.src_beam + torch.arange(nseq)[:, None] * K), what
    assert bool((d.ctx_len.cpu() == prompt_len + tstep).all()), what
    cur = d.hist[(tstep + 1) & 1].cpu().view(nseq, K, -1).long()
    assert torch.equal(cur[:, :, :tstep + 1], ref.run_hist[:, :, :tstep + 1]), what
    assert _rel_close(d.fin_score.cpu().view(nseq, K), ref.fin_score), what
    assert torch.equal(d.fin_flag.cpu().view(nseq, K) != 0, ref.fin_flag), what
    assert torch.equal(d.fin_len.cpu().view(nseq, K).long(), ref.fin_len), what
    fi = d.fin_ids.cpu().view(nseq, K, -1).long()
    mask = torch.arange(d.max_new)[None, None, :] < ref.fin_len[:, :, None]
    assert torch.equal(fi[mask], ref.fin_hist[mask]), what
    assert (d.open.cpu() != 0).tolist() == ref.open and (d.seq_done.cpu() != 0).tolist() == ref.done, what
    assert d.step.cpu().tolist() == ref.t, what


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_beam_step_matches_the_restatement(K):
    """Synthetic candidate lists on a grid of spacing 1e-2 (no two candidates of a sequence closer), tokens drawn from a small vocabulary
    that holds the EOS ids: every E, early_stopping and length_penalty.  At step 2 every beam's best continuations are the EOS ids, which
    leaves the fewest un-hit candidates that rows of distinct tokens allow (M is sized so that K remain); once beams have died their
    lists collapse to ties at -1e9 and fewer than K live candidates remain; step 5 is the last (everything hits); sequences that become
    done are stepped on and must stay frozen."""
    nseq, max_new, V, prompt_len = 3, 6, 40, 7
    lib = L.lib()
    early_seen = False
    for E, es, lp in itertools.product((0, 1, 3), (False, True, "never"), (0.0, 1.0, 2.0)):
        eos = [3, 11, 29][:E]
        M = beam_ref.n_candidates(K, E)
        g = torch.Generator().manual_seed(1000 * K + 100 * E + 10 * int(lp) + L.early_stopping_code(es))
        ref = beam_ref.BeamRef(nseq, K, max_new, eos, lp, es)
        d = _DevBeam(nseq, K, max_new, lp, prompt_len)
        o = L.BeamOpts()
        eos_c = (C.c_int32 * 8)(*(eos + [0] * (8 - E)))
        o.eos_ids_host, o.n_eos, o.use_eos, o.max_new_tokens, o.num_beams, o.num_return_sequences = eos_c, E, int(E > 0), max_new, K, 1
        o.early_stopping, o.length_penalty = L.early_stopping_code(es), lp
        for step in range(max_new):
            what = (K, E, es, lp, step)
            # distinct grid values per sequence, each beam's list descending; dead beams (running score -1e9) collapse to ties at -1e9 in fp32
            acc = torch.empty(nseq, K, M)
            tok = torch.empty(nseq, K, M, dtype=torch.int64)
            for s in range(nseq):
                grid = -(torch.randperm(K * M * 2, generator=g)[:K * M].float() + 1.0) * 1e-2 - step
                for j in range(K):
                    acc[s, j] = grid[j * M:(j + 1) * M].sort(descending=True).values + (ref.run_score[s, j] if ref.run_score[s, j] < -1e8 else 0.0)
                    tok[s, j] = torch.randperm(V, generator=g)[:M]
                    if step == 2 and E > 0:                      # every beam's best E continuations are the EOS ids: K * E candidates hit
                        rest = [v for v in torch.randperm(V, generator=g).tolist() if v not in eos][:M - E]
                        tok[s, j] = torch.tensor(eos + rest)
            first = step == 0
            if first:
                acc[:, 1:] = acc[:, :1] + beam_ref.NEG
                tok[:, 1:] = tok[:, :1]
                lists_v, lists_t = acc[:, 0].contiguous(), tok[:, 0].contiguous()
            else:
                lists_v, lists_t = acc.view(nseq * K, M), tok.view(nseq * K, M)
            dv, dt_ = lists_v.to(DEV), lists_t.to(torch.int32).to(DEV)
            L.check(lib.sl_beam_step(C.byref(d.struct), dv.data_ptr(), dt_.data_ptr(), nseq, K, M, int(first), C.byref(o), L.stream_ptr()), "sl_beam_step")
            ref.step_acc(acc, tok)
            _compare_step_state(d, ref, step, prompt_len, what)
            if step == 2 and E > 0:
                early_seen = early_seen or bool(ref.fin_flag.any())      # the EOS step finished hypotheses before the budget
        assert ref.all_done()
        # a step past the budget touches nothing
        before = d.fin_score.clone()
        L.check(lib.sl_beam_step(C.byref(d.struct), dv.data_ptr(), dt_.data_ptr(), nseq, K, M, 0, C.byref(o), L.stream_ptr()), "sl_beam_step")
        _sync()
        assert torch.equal(before, d.fin_score) and d.step.cpu().tolist() == [max_new] * nseq
    assert early_seen


# ------------------------------------------------------------------------------------------------ sl_kv_beam_reorder
@pytest.mark.parametrize("fmt", ["float32", "bfloat16", "fp8"])
@pytest.mark.parametrize("perm", ["identity", "cycle", "fanout"])
def test_kv_beam_reorder_moves_the_generated_span_and_nothing_else(fmt, perm):
    lib = L.lib()
    n_layers, n_kv, D, max_ctx, rows, K = 2, 2, 128, 48, 6, 3
    m = L.LlamaModel()
    m.dtype = {"float32": L.SL_F32, "bfloat16": L.SL_BF16, "fp8": L.SL_BF16}[fmt]
    m.n_layers, m.n_kv_heads, m.head_dim, m.n_heads, m.hidden = n_layers, n_kv, D, 2, 256
    esz = {"float32": 4, "bfloat16": 2, "fp8": 1}[fmt]
    src = {"identity": [0, 1, 2, 3, 4, 5], "cycle": [1, 2, 0, 4, 5, 3], "fanout": [0, 0, 0, 3, 3, 3]}[perm]
    prompt = [5, 5, 5, 9, 9, 9]
    g = torch.Generator().manual_seed(11)
    for span in (0, 1, 7):
        k0 = torch.randint(0, 256, (n_layers, rows + 1, n_kv, max_ctx, D * esz), dtype=torch.uint8, generator=g)       # one slot more than rows: untouched
        v0 = torch.randint(0, 256, k0.shape, dtype=torch.uint8, generator=g)
        k, v = k0.to(DEV), v0.to(DEV)
        kv = L.KVCache()
        kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx, kv.reserved = k.data_ptr(), v.data_ptr(), rows + 1, max_ctx, int(fmt == "fp8")
        need = lib.sl_kv_beam_staging_bytes(C.byref(kv), C.byref(m), rows, 7)
        assert need == 2 * rows * n_layers * n_kv * 7 * D * esz
        staging = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
        staging[need:] = 0xA5
        i32 = lambda x: torch.tensor(x, dtype=torch.int32).to(DEV)
        src_d, p_d, c_d = i32(src), i32(prompt), i32([p + span for p in prompt])
        L.check(lib.sl_kv_beam_reorder(C.byref(kv), C.byref(m), src_d.data_ptr(), p_d.data_ptr(), c_d.data_ptr(), rows, 7, staging.data_ptr(), need,
                                       L.stream_ptr()), "sl_kv_beam_reorder")
        _sync()
        for got, orig in ((k.cpu(), k0), (v.cpu(), v0)):
            want = orig.clone()
            for r in range(rows):
                p0 = prompt[r]
                want[:, r, :, p0:p0 + span] = orig[:, src[r], :, p0:p0 + span]
            assert torch.equal(got, want), (fmt, perm, span)
        assert bool((staging[need:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ end to end, fp32
def _case(name):
    g = golden("beam_tiny")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def _case_inputs(c, dtype=torch.float32):
    model = str(c["model"])
    llm = _llm(model, int(c["weight_seed"]), float(c["norm_mul"]), dtype)
    _set_eos(llm, c["eos"].tolist(), int(c["pad"]))
    x = torch.randn(int(c["batch"]), int(c["S"]), CFG[model].hidden_size, generator=torch.Generator().manual_seed(int(c["input_seed"]))) * 0.05
    kw = dict(max_new_tokens=int(c["max_new"]), num_beams=int(c["K"]), num_return_sequences=int(c["R"]), length_penalty=float(c["length_penalty"]),
              early_stopping=ES[int(c["early_stopping"])])
    return llm, x, kw


def _score_close(got, want):
    got, want = got.double(), want.double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().clamp(min=1.0)).all())


@pytest.mark.parametrize("name", CASES)
def test_generate_reproduces_the_reference_class(name):
    c = _case(name)
    llm, x, kw = _case_inputs(c)
    ids = llm.generate(inputs_embeds=x.to(DEV), **kw).cpu()
    lens, want_ids = t(c["lens"]).long(), t(c["ids"]).long()
    print(name, "scores", llm.last_beam_scores.tolist(), "reference", c["scores"].tolist())
    assert torch.equal(llm.last_beam_lengths.long(), lens)
    assert ids.shape == (want_ids.shape[0], int(lens.max())) and ids.dtype == torch.int64
    assert torch.equal(ids, want_ids[:, :ids.shape[1]])
    assert _score_close(llm.last_beam_scores, t(c["scores"]))
    assert llm.last_generate_stats["rows"] == int(c["batch"]) * int(c["K"]) and llm.last_generate_stats["num_beams"] == int(c["K"])


@pytest.mark.parametrize("name", ["mha_k3_eos_lp2", "gqa_k4"])
def test_generate_packed_with_a_shared_prefix_equals_the_unshared_call(name):
    c = _case(name)
    llm, x, kw = _case_inputs(c)
    x[:, :5] = x[0, :5]                                           # the first five rows of every prompt are the same rows
    B, S = x.shape[0], x.shape[1]
    beams = dict(num_beams=kw["num_beams"], num_return_sequences=kw["num_beams"], length_penalty=kw["length_penalty"], early_stopping=kw["early_stopping"])
    out = []
    for P in (0, 5):
        ids, n_cols = llm.generate_packed(x.reshape(B * S, -1).to(DEV).clone(), [S] * B, kw["max_new_tokens"], shared_prefix=P, beams=beams)
        out.append((ids.clone(), n_cols, llm.last_beam_scores.clone(), llm.last_beam_lengths.clone()))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])


def test_num_return_sequences_equal_to_num_beams_gives_descending_distinct_hypotheses():
    c = _case("mha_k3_eos_r3")
    llm, x, kw = _case_inputs(c)
    ids = llm.generate(inputs_embeds=x.to(DEV), **kw).cpu()
    K, B = kw["num_beams"], x.shape[0]
    sc = llm.last_beam_scores.view(B, K)
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())
    for b in range(B):
        hyps = {tuple(ids[b * K + r, :int(llm.last_beam_lengths[b * K + r])].tolist()) for r in range(K)}
        assert len(hyps) == K


# ------------------------------------------------------------------------------------------------ num_beams = 1 is the greedy loop
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_beam_generate_with_one_beam_returns_the_greedy_ids_bit_for_bit(dtype):
    llm = _llm("tiny_gqa", 31, 1, dtype)
    lens = [9, 21, 14, 5]
    x = (torch.randn(sum(lens), TINY_LLAMA.hidden_size, generator=torch.Generator().manual_seed(5)) * 0.05).to(dtype).to(DEV)
    greedy, n_cols = llm.generate_packed(x.clone(), lens, 10, use_eos=False, compact=False)
    assert n_cols == 10
    beam, n_beam = llm.generate_packed(x.clone(), lens, 10, use_eos=False, beams=dict(num_beams=1))
    assert n_beam == 10 and torch.equal(beam, greedy)
    assert bool((llm.last_beam_lengths == 10).all()) and bool(torch.isfinite(llm.last_beam_scores).all())


# ------------------------------------------------------------------------------------------------ 16-bit: scores are sums of log-probabilities
def _sum_logprob_diff(dtype):
    """K = 4 on TINY_LLAMA, five ragged prompts, 16 new tokens: largest |score * len**lp - sum of the chosen tokens' log-probabilities|, the
    log-probabilities recomputed by forward() on the prompt plus the returned ids"""
    llm = _llm("tiny_gqa", 31, 8, dtype, max_ctx=64)
    _set_eos(llm, [], TINY_LLAMA.pad_token_id)
    lens, K, max_new, lp = [9, 21, 14, 5, 33], 4, 16, 1.0
    g = torch.Generator().manual_seed(21)
    prompts = [(torch.randn(n, TINY_LLAMA.hidden_size, generator=g) * 0.05).to(dtype).to(DEV) for n in lens]
    ids = llm.generate(inputs_embeds=[p.clone() for p in prompts], max_new_tokens=max_new, num_beams=K, num_return_sequences=K, length_penalty=lp).cpu()
    sc, ln = llm.last_beam_scores.view(len(lens), K), llm.last_beam_lengths.view(len(lens), K)
    assert bool(torch.isfinite(sc).all()) and bool((sc[:, :-1] >= sc[:, 1:]).all())
    worst = 0.0
    for b, p in enumerate(prompts):
        for r in range(K):
            n = int(ln[b, r])
            toks = ids[b * K + r, :n]
            seq = torch.cat([p, llm.model.embed_tokens(toks[:-1].to(DEV))]) if n > 1 else p
            logits = llm.forward(inputs_embeds=seq[None]).logits[0, lens[b] - 1:].float().cpu()
            lps = torch.log_softmax(logits.double(), dim=-1)[torch.arange(n), toks]
            worst = max(worst, abs(float(sc[b, r]) * float(n) ** lp - float(lps.sum())))
    return worst


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_scores_are_the_sums_of_the_chosen_log_probabilities(dtype):
    floor = _sum_logprob_diff(torch.float32)
    got = _sum_logprob_diff(dtype)
    print(f"sum-of-log-probabilities difference: float32 {floor:.3e}, {dtype} {got:.3e}")
    rec = SUM_LOGPROB_DIFF_MEASURED[dtype]
    assert rec is not None, "no recorded figure: run once, record it in DESIGN §8.15 and above"
    assert rec >= floor, "the recorded 16-bit figure is below what float32 itself shows"
    assert got <= 2 * rec, (got, rec, floor)


# ------------------------------------------------------------------------------------------------ graph replay, no aliasing with greedy
def test_second_call_replays_the_cached_graph_and_a_greedy_call_in_between_keeps_its_own():
    lib = L.lib()
    c = _case("mha_k3_eos_lp2")
    llm, x, kw = _case_inputs(c)
    B, S = x.shape[0], x.shape[1]
    beams = dict(num_beams=kw["num_beams"], length_penalty=kw["length_penalty"], early_stopping=kw["early_stopping"])
    xp = x.reshape(B * S, -1).to(DEV)
    llm.generate_packed(xp.clone(), [S] * B, 12, beams=beams)          # sizes the workspace and the cache for both modes
    lib.sl_decode_graph_cache_clear()
    greedy0, _ = llm.generate_packed(xp.clone(), [S] * B, 12, use_eos=False, compact=False)
    ids1, _ = llm.generate_packed(xp.clone(), [S] * B, 12, beams=beams)
    st1 = dict(llm.last_generate_stats)
    greedy1, _ = llm.generate_packed(xp.clone(), [S] * B, 12, use_eos=False, compact=False)
    ids2, _ = llm.generate_packed(xp.clone(), [S] * B, 12, beams=beams)
    st2 = dict(llm.last_generate_stats)
    greedy2, _ = llm.generate_packed(xp.clone(), [S] * B, 12, use_eos=False, compact=False)
    assert torch.equal(ids1, ids2) and st1 == st2 and st1["decode_launches"] >= 1
    assert torch.equal(greedy0, greedy1) and torch.equal(greedy1, greedy2)
    assert torch.equal(ids1[:, :int(llm.last_beam_lengths.max())], t(c["ids"])[:, :int(llm.last_beam_lengths.max())].to(torch.int32))
    assert lib.sl_decode_graph_cache_clear() == 2                     # one beam graph + one greedy graph: the second calls replayed them


def test_decode_graph_census():
    """One graph per mode and not one more: greedy, greedy + scores, sampling, greedy + repetition penalty, beams, beams + no-repeat n-grams on
    the same buffers each capture once (their keys differ in scores / sample / lp_* / beam_*), the second round replays all six and returns
    what the first did.  Then a budgeted greedy call that compacts once: 3 -> 2 rows, ids those of the uncompacted call."""
    lib = L.lib()
    llm = _llm("tiny_gqa", 31, 1, torch.float32)
    _set_eos(llm, TINY_LLAMA.eos_token_ids, TINY_LLAMA.pad_token_id)          # the model's own: whatever an earlier test left is not this test's
    lens, max_new = [5, 9, 7], 6
    x = (torch.randn(sum(lens), TINY_LLAMA.hidden_size, generator=torch.Generator().manual_seed(9)) * 0.05).to(DEV)
    modes = [dict(), dict(scores=True), dict(sample=dict(temperature=0.8, top_k=20, top_p=0.9, seed=1234)), dict(logits=dict(repetition_penalty=1.3)),
             dict(beams=dict(num_beams=2)), dict(beams=dict(num_beams=2), logits=dict(no_repeat_ngram_size=2))]

    def run(kw):
        r = llm.generate_packed(x.clone(), lens, max_new, use_eos=False, compact=False, **kw)
        extra = llm.last_beam_scores.clone() if "beams" in kw else (r[2].clone() if kw.get("scores") else None)
        return r[0].clone(), extra

    for kw in modes:                                   # sizes the workspace and the cache for the largest mode: the rounds below share one buffer
        run(kw)
    lib.sl_decode_graph_cache_clear()
    first = [run(kw) for kw in modes]
    second = [run(kw) for kw in modes]
    for kw, a, b in zip(modes, first, second):
        assert torch.equal(a[0], b[0]), kw
        assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1]), kw
    assert lib.sl_decode_graph_cache_clear() == 6
    out = {}
    for compact in (False, True):
        ids, n_cols = llm.generate_packed(x.clone(), lens, max_new, use_eos=True, row_limits=[2, 6, 6], check_every=2, compact=compact)
        out[compact] = (ids.clone(), n_cols, dict(llm.last_generate_stats))
    assert out[True][2]["compactions"] == 1 and out[True][2]["final_rows"] == 2, out[True][2]
    assert torch.equal(out[True][0], out[False][0]) and out[True][1] == out[False][1]
