"""GPU: token log-probabilities — the lm_head epilogue's third plane per element, the three select kernels against the fp64
restatement (tests/token_scores_ref.py) within the bound counted there, generate() end to end against what the reference class and
transformers' compute_transition_scores returned (tests/golden/token_scores_tiny.npz), every branch of the fused / unfused gate,
compaction, scores off, and the 16-bit modes."""
import numpy as np
import pytest
import torch

from conftest import golden, pkg, t
from oracle.llama_oracle import LlamaCfg

import token_scores_ref as tsr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = pkg("_lib")
ops = pkg("ops")
ri = pkg("random_init")
weights = pkg("weights")
llama_mod = pkg("audio_llama")

# tests/test_models_gpu.py: F32_TOL = 1e-4 (fp32 logits against the oracle, relative to the logits' norm; also what
# test_llama_decode_step_large_batch_matches_small_batch allows between two kernel families) and BF16_TOL = 3e-2 (16-bit logits).  A
# log-probability is a logit minus a log-sum-exp of logits: the tolerance is taken twice, times the logits' root mean square.
F32_TOL, BF16_TOL = 1e-4, 3e-2
GUARD = 12345.0
CASES = ["greedy", "rep13", "ngram2", "minnew6", "eos_all", "eos_one", "batch1", "batch1_eos", "ragged3", "ragged3_eos"]
DT = [torch.float32, torch.bfloat16, torch.float16]


def rnd(*shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _guarded(n, dtype, fill):
    """n elements with 64 guard words on either side -> (whole buffer, the view)"""
    buf = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
    return buf, buf[64:64 + n]


def _guards_intact(buf, n, fill):
    return bool((buf[:64] == fill).all()) and bool((buf[64 + n:] == fill).all())


# ------------------------------------------------------------------------------------------------ the fused epilogue, per element
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M", [65, 77, 300])
@pytest.mark.parametrize("N,K", [(1000, 64), (1000, 192), (64, 64), (64, 192)])
def test_fused_epilogue_third_plane_per_element(dt, M, N, K):
    """sl_gemm_top1_lse: the two existing planes bit for bit those of sl_gemm_ex, the third within bound_group_sum of the fp64 sum over the
    fp32 logits the same kernel stores (bitwise the values the epilogue saw: the maxima are asserted equal), a whole group of -inf bias and
    an all-NaN row at 0, nothing written outside the planes."""
    A, W = rnd(M, K, seed=11 + M), rnd(N, K, seed=12 + N, std=2.0 * K ** -0.5)
    A[M // 3] = float("nan")                                        # one all-NaN row: every product is NaN
    bias = rnd(N, seed=13)
    if N > 192:
        bias[128:192] = float("-inf")                              # a whole group
        bias[70:75] = float("-inf")
    else:
        bias[0:32] = float("-inf")
    Ad, Wd = A.to(DEV, dt), W.to(DEV, dt)
    ng = (N + 63) // 64
    for b in (None, bias.to(DEV, dt)):
        logits = ops.gemm(Ad, Wd, bias=b, out_f32=True)
        val0, idx0 = ops.gemm_top1(Ad, Wd, bias=b)
        bufs = [_guarded(ng * M, torch.float32, GUARD), _guarded(ng * M, torch.int32, 12345), _guarded(ng * M, torch.float32, GUARD)]
        val, idx, ssum = ops.gemm_top1_lse(Ad, Wd, bias=b, out=tuple(v.view(ng, M) for _, v in bufs))
        torch.cuda.synchronize()
        assert _guards_intact(bufs[0][0], ng * M, GUARD) and _guards_intact(bufs[1][0], ng * M, 12345) and _guards_intact(bufs[2][0], ng * M, GUARD)
        assert torch.equal(val.view(torch.int32), val0.view(torch.int32)) and torch.equal(idx, idx0)
        # the fp32 logits are the values the epilogue saw: every group's maximum of them is the first plane, bit for bit
        cl = torch.where(torch.isnan(logits), torch.full_like(logits, float("-inf")), logits)
        gmax = torch.cat([cl, torch.full((M, ng * 64 - N), float("-inf"), device=DEV)], 1).view(M, ng, 64).max(dim=2).values
        assert torch.equal(val.T.contiguous(), gmax)
        S, rel, dead = tsr.group_sums_reference(logits)
        got = ssum.double()
        assert bool((got[dead] == 0).all()) and bool(dead[:, M // 3].all())
        if b is not None and N > 192:
            assert bool(dead[2].all())
        live = ~dead
        assert bool(torch.isfinite(got[live]).all()) and bool((got[live] >= 1.0 - 1e-6).all())        # the maximum itself contributes exp(0)
        err = ((got - S).abs() / S.clamp(min=1e-300))[live]
        print(f"dt={dt} M={M} N={N} K={K} bias={b is not None}: worst err / bound {float((err / rel[live]).max()):.3f}")
        assert bool((err <= rel[live]).all())


# ------------------------------------------------------------------------------------------------ the select kernels
def _state(B, max_new, gen):
    return dict(unfinished=torch.ones(B, dtype=torch.int32, device=DEV), ctx=torch.arange(B, dtype=torch.int32, device=DEV),
                gen=torch.tensor(gen, dtype=torch.int32, device=DEV), fin=torch.zeros(B, dtype=torch.int32, device=DEV),
                nxt=torch.zeros(B, dtype=torch.int32, device=DEV), out=torch.full((B, max_new), -1, dtype=torch.int32, device=DEV))


def _same_state(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("V", [1000, 777, 64, 4100])
def test_row_and_partial_select_agree_with_the_restatement_and_keep_token_and_bookkeeping(V):
    """V = 777: the scalar row scan and a last group of 9; 4 100: more than one 16-byte group per thread and 65 groups (three per stripe).
    B = 70: three blocks of the partial kernel, the last with 6 rows."""
    B, max_new = 70, 3
    logits = rnd(B, V, seed=V) * 3.0
    logits[:, 5] = float("-inf")
    logits[3, 7] = float("nan")
    logits[4] = float("-inf")                                       # no finite maximum: the value must not be finite, nothing may fault
    if V > 128:
        logits[5, 64:128] = float("-inf")                          # a dead group
    logits[6] += 100.0
    ng = (V + 63) // 64
    clean = torch.where(torch.isnan(logits), torch.full_like(logits, float("-inf")), logits)
    grp = torch.cat([clean, torch.full((B, ng * 64 - V), float("-inf"))], 1).view(B, ng, 64)
    gmax = grp.max(dim=2).values
    first = (grp == gmax[:, :, None]).float().argmax(dim=2) + torch.arange(ng)[None, :] * 64
    first[torch.isinf(gmax) & (gmax < 0)] = 0x7fffffff
    gsum = torch.exp(grp.double() - torch.where(torch.isinf(gmax), torch.zeros_like(gmax), gmax).double()[:, :, None]).sum(dim=2)
    gsum[torch.isinf(gmax)] = 0.0
    val, idx, ssum = gmax.T.contiguous().to(DEV), first.T.contiguous().to(torch.int32).to(DEV), gsum.T.contiguous().float().to(DEV)
    gen = [b % max_new for b in range(B)]
    eos = [int(clean[0].argmax()), 3]
    ld = logits.to(DEV)
    runs = {}
    for kind in ("row", "row_sc", "partial", "partial_sc"):
        s = _state(B, max_new, gen)
        s["unfinished"][B // 2] = 0
        s["unfinished"][9] = 0
        buf, lp = _guarded(B * max_new, torch.float32, GUARD)
        a = (eos, 7, True, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"])
        if kind == "row":
            ops.greedy_select(ld, *a)
        elif kind == "row_sc":
            ops.greedy_select_sc(ld, *a, lp.view(B, max_new))
        elif kind == "partial":
            ops.greedy_select_partial(val, idx, *a)
        else:
            ops.greedy_select_partial_sc(val, idx, ssum, *a, lp.view(B, max_new))
        torch.cuda.synchronize()
        assert _guards_intact(buf, B * max_new, GUARD)
        runs[kind] = ({k: v.cpu() for k, v in s.items()}, lp.view(B, max_new).cpu())
    assert _same_state(runs["row"][0], runs["row_sc"][0]) and _same_state(runs["partial"][0], runs["partial_sc"][0])
    assert _same_state(runs["row"][0], runs["partial"][0])
    tok = clean.argmax(dim=1)
    ref = tsr.transition_logprobs(logits, tok)
    worst = [0.0, 0.0]
    for b in range(B):
        for j, kind in enumerate(("row_sc", "partial_sc")):
            lp = runs[kind][1][b]
            others = [c for c in range(max_new) if c != gen[b]]
            assert bool((lp[others] == GUARD).all())               # one element per row
            got = float(lp[gen[b]])
            if b in (B // 2, 9):
                assert got == 0.0                                     # a finished row (the pad was emitted)
            elif b == 4:
                assert not np.isfinite(got)
            else:
                bound = tsr.bound_row(logits[b].numpy(), int(tok[b])) if j == 0 else tsr.bound_partial(logits[b].numpy())
                if j == 1:
                    bound += tsr.U * 1.01                             # the host-made third plane above: one more rounding per group sum
                assert abs(got - float(ref[b])) <= bound, (kind, b, got, float(ref[b]), bound)
                worst[j] = max(worst[j], abs(got - float(ref[b])) / bound)
    print(f"V={V}: worst err / bound row {worst[0]:.3f} partial {worst[1]:.3f}")


SAMPLING = {"topk": (1.0, 20, 1.0), "topp": (1.0, 0, 0.8), "both": (0.7, 20, 0.9)}


@pytest.mark.parametrize("mode", list(SAMPLING))
def test_sampled_log_probability_is_the_warped_renormalised_one(mode):
    temp, k, p = SAMPLING[mode]
    B, V, max_new = 8, 1000, 4
    logits = rnd(B, V, seed=300) * 3.0
    logits[:, 11] = float("-inf")
    warped = tsr.warp(logits, temp, k, p)
    if p < 1.0:
        # the inputs leave the top-p boundary clear of rounding: mass above the last survivor and above the first dropped token are 1e-3 away from p
        full = tsr.warp(logits, temp, k, 1.0)
        probs = torch.softmax(full, dim=-1)
        for b in range(B):
            srt = torch.sort(probs[b], descending=True).values
            above = torch.cat([torch.zeros(1, dtype=torch.float64), srt.cumsum(0)[:-1]])
            n_keep = int(torch.isfinite(warped[b]).sum())
            assert float(above[n_keep - 1]) < p - 1e-3 and float(above[n_keep]) > p + 1e-3, (b, float(above[n_keep - 1]), float(above[n_keep]))
    ld = logits.to(DEV)
    got = {}
    for sc in (False, True):
        s = _state(B, max_new, [b % max_new for b in range(B)])
        s["unfinished"][2] = 0
        buf, lp = _guarded(B * max_new, torch.float32, GUARD)
        a = (temp, k, p, 99, [3], 7, True, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"])
        if sc:
            ops.sample_select_sc(ld, *a, lp.view(B, max_new))
        else:
            ops.sample_select(ld, *a)
        torch.cuda.synchronize()
        assert _guards_intact(buf, B * max_new, GUARD)
        got[sc] = ({k_: v.cpu() for k_, v in s.items()}, lp.view(B, max_new).cpu())
    assert _same_state(got[False][0], got[True][0])
    nxt, lps = got[True][0]["nxt"], got[True][1]
    worst = 0.0
    for b in range(B):
        v = float(lps[b, b % max_new])
        if b == 2:
            assert v == 0.0 and int(nxt[b]) == 7
            continue
        tok = int(nxt[b])
        assert bool(torch.isfinite(warped[b, tok]))                  # a survivor was drawn
        ref = float(tsr.transition_logprobs(warped[b:b + 1], torch.tensor([tok]))[0])
        bound = tsr.bound_sample(warped[b].numpy(), tok)
        assert v <= 0.0 and abs(v - ref) <= bound, (b, v, ref, bound)
        worst = max(worst, abs(v - ref) / bound)
    print(f"{mode}: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ end to end
_LLMS = {}


def _cfg():
    g = golden("token_scores_tiny")
    kw = {k[4:]: g[k].item() for k in g if k.startswith("cfg.") and k[4:] not in ("weight_seed", "norm_mul", "max_new")}
    return LlamaCfg(rope_scaling=None, eos_token_ids=(), **kw), int(g["cfg.weight_seed"]), float(g["cfg.norm_mul"]), int(g["cfg.max_new"])


def _llm(dtype=torch.float32, pack_decode=True):
    key = (dtype, pack_decode)
    if key not in _LLMS:
        c, seed, norm_mul, _ = _cfg()
        arch = weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size,
                                 c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling, c.tie_word_embeddings, (), c.pad_token_id)
        sd = dict(ri.llama_state_dict(c, seed=seed))
        sd["model.norm.weight"] = sd["model.norm.weight"] * norm_mul
        _LLMS[key] = llama_mod.AudioLlamaForCausalLM(arch, sd, torch_dtype=dtype, device=DEV, max_ctx=64, pack_decode=pack_decode)
    return _LLMS[key]


def _case(name):
    g = golden("token_scores_tiny")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def _prompts(c, hidden=256):
    """the generator's prompts: row b of a case is its own draw"""
    seed = int(c["input_seed"])
    return [torch.randn(int(n), hidden, generator=torch.Generator().manual_seed(seed * 100 + b)) * 0.05 for b, n in enumerate(c["prompt_lens"].tolist())]


def _set_eos(llm, eos, pad=0):
    llm.generation_config.eos_token_id = list(eos) if len(eos) else None
    llm.generation_config.pad_token_id = int(pad)


_RMS = {}


def _logit_rms(prompts):
    """root mean square of the fp32 logits at the prompts' last positions (what F32_TOL / BF16_TOL are relative to)"""
    key = tuple(int(p.shape[0]) for p in prompts) + (float(prompts[0][0, 0]),)
    if key not in _RMS:
        llm = _llm()
        vals = [llm(inputs_embeds=p[None].to(DEV)).logits[0, -1].double() for p in prompts]
        _RMS[key] = float(torch.stack(vals).pow(2).mean().sqrt())
    return _RMS[key]


@pytest.mark.parametrize("name", CASES)
def test_generate_returns_the_reference_ids_and_transition_scores(name):
    c = _case(name)
    llm = _llm()
    _set_eos(llm, c["eos"].tolist())
    prompts = _prompts(c)
    max_new = _cfg()[3]
    out = llm.generate(inputs_embeds=[p.to(DEV) for p in prompts], max_new_tokens=max_new, return_dict_in_generate=True, output_scores=True,
                       repetition_penalty=float(c["repetition_penalty"]), no_repeat_ngram_size=int(c["no_repeat_ngram_size"]), min_new_tokens=int(c["min_new_tokens"]))
    n_cols = int(c["n_cols"])
    want_ids, want_lp, lens = t(c["ids"]).long()[:, :n_cols], t(c["logprobs"])[:, :n_cols].double(), c["lens"].tolist()
    assert torch.equal(out.sequences.cpu(), want_ids)
    got = out.token_logprobs.double()
    assert got.shape == want_lp.shape and out.token_logprobs.dtype == torch.float32
    tol = 2 * F32_TOL * _logit_rms(prompts)
    print(f"{name}: worst |diff| {float((got - want_lp).abs().max()):.3e}, tolerance {tol:.3e}")
    assert bool(((got - want_lp).abs() <= tol).all())
    for b, n in enumerate(lens):
        assert bool((got[b, n:] == 0).all()) and bool((got[b, :n] < 0).all())
    assert bool(((out.sequences_scores.double() - want_lp.sum(dim=1)).abs() <= tol * n_cols).all())
    assert torch.equal(llm.last_token_logprobs, out.token_logprobs)


def _tiled(c, rows):
    prompts = _prompts(c)
    lens = [int(prompts[i % len(prompts)].shape[0]) for i in range(rows)]
    x = torch.cat([prompts[i % len(prompts)] for i in range(rows)], 0)
    return x, lens, len(prompts)


def test_every_branch_of_the_fused_gate_gives_each_sequence_the_same_log_probabilities():
    """decode_fuses_argmax: <= 64 rows (row form); 65-255 with the packed lm_head (row form) and without (fused, 128-row tiles at 66, 130); >= 256
    (fused, either packing).  The prompts are the fixture's ragged three, tiled.
    Bare bound (bound_greedy_any: the two summation orders, nothing else) wherever the two sides saw the same logits: every fused branch
    against the same call forced through the row form (a logits processor that can never act: the same tiled lm_head, storing its
    accumulators instead of reducing them), and the fused branches that share a kernel family (66 / 130 / 258 rows unpacked) against each other.
    Across kernel families the logits themselves differ (other accumulation orders in every layer), which no bound on the log-sum-exp covers:
    there the tolerance adds 2 x F32_TOL x rms, what tests/test_models_gpu.py allows fp32 logits of two families."""
    c = _case("ragged3")
    want = t(c["ids"]).long()
    max_new = _cfg()[3]
    base, family = None, None
    bare = tsr.bound_greedy_any(1000)
    tol = 2 * F32_TOL * _logit_rms(_prompts(c)) + bare
    never = dict(repetition_penalty=1.0, no_repeat_ngram_size=max_new + 8, min_new_tokens=0)
    for pack, rows, fused in ((True, 3, False), (True, 64, False), (True, 66, False), (False, 66, True), (False, 130, True), (True, 255, False),
                              (True, 256, True), (False, 258, True)):
        llm = _llm(pack_decode=pack)
        _set_eos(llm, [])
        x, lens, n = _tiled(c, rows)
        ids, n_cols, lps = llm.generate_packed(x.to(DEV), lens, max_new, scores=True)
        assert n_cols == max_new and bool(torch.isfinite(lps).all()) and bool((lps < 0).all())
        for r in range(rows):
            assert torch.equal(ids[r].long(), want[r % n]), (pack, rows, r)
        if base is None:
            base = lps[:n].double()
        diff = float((lps.double() - base.repeat((rows + n - 1) // n, 1)[:rows]).abs().max())
        print(f"pack_decode={pack} rows={rows}: worst |diff| to the 3-row call {diff:.3e}, tolerance {tol:.3e}")
        assert diff <= tol
        if fused:
            ids_u, _, lps_u = llm.generate_packed(x.to(DEV), lens, max_new, scores=True, logits=never)
            d_u = float((lps.double() - lps_u.double()).abs().max())
            print(f"    fused against the row form on the same logits: worst |diff| {d_u:.3e}, bound {bare:.3e}")
            assert torch.equal(ids_u, ids) and d_u <= bare
        if fused and not pack:
            if family is None:
                family = lps[:n].double()
            d_f = float((lps.double() - family.repeat((rows + n - 1) // n, 1)[:rows]).abs().max())
            print(f"    against the 66-row unpacked call: worst |diff| {d_f:.3e}, bound {bare:.3e}")
            assert d_f <= bare


@pytest.mark.parametrize("pack,rows,dtype", [(True, 12, torch.float32), (False, 132, torch.float32), (False, 132, torch.bfloat16)])
def test_compacted_and_uncompacted_calls_give_the_same_log_probabilities(pack, rows, dtype):
    """budgets that retire half the rows by the first check (step 4) and half of the rest by the second (step 8): two compactions, down the
    ladder of row counts 12 -> 6 -> 3 and 132 -> 96 -> 48 (66 and 33 live rows; with the fused planes, the family pinned).  fp32: bit for bit.
    bf16: the ids are those of the uncompacted call (the pin), the log-probabilities within the bare bound.  Retired rows are zero beyond
    their budget."""
    c = _case("ragged3")
    llm = _llm(dtype, pack_decode=pack)
    _set_eos(llm, [])
    x, lens, n = _tiled(c, rows)
    cycle = [2, 20, 3, 6, 4, 20, 2, 7, 3, 20, 4, 8]
    budgets = [cycle[r % 12] for r in range(rows)]
    out = {}
    for compact in (False, True):
        ids, n_cols, lps = llm.generate_packed(x.to(dtype).to(DEV), lens, 20, row_limits=budgets, compact=compact, scores=True)
        out[compact] = (ids.clone(), n_cols, lps.clone(), dict(llm.last_generate_stats))
    assert out[True][3]["compactions"] == 2 and out[False][3]["compactions"] == 0, out[True][3]
    assert out[True][3]["final_rows"] == (3 if rows == 12 else 48) and out[False][3]["final_rows"] == rows
    assert out[True][1] == out[False][1] and torch.equal(out[True][0], out[False][0])
    if dtype == torch.float32:
        assert torch.equal(out[True][2].view(torch.int32), out[False][2].view(torch.int32))
    else:
        d = float((out[True][2].double() - out[False][2].double()).abs().max())
        print(f"{dtype}: worst |diff| compacted against uncompacted {d:.3e}, bound {tsr.bound_greedy_any(1000):.3e}")
        assert d <= tsr.bound_greedy_any(1000)
    for r, n_ in enumerate(budgets):
        assert bool((out[True][2][r, n_:] == 0).all()) and bool((out[True][2][r, :n_] < 0).all())


@pytest.mark.parametrize("rows", [12, 96])
def test_one_compaction_moves_ids_and_log_probabilities_together_on_both_sides_of_the_fused_gate(rows):
    """12 rows with the packed lm_head (row form: fp32 logits, greedy_select_kernel) and 96 without (fused top-1: three planes,
    greedy_select_partial_kernel; the family stays pinned at 96 after the compaction).  Even rows have a budget of 3, so half the batch is
    finished at the first check (step 4): one compaction, to the rung of rows / 2 live rows (6 and 48), in which every surviving row changes
    its slot — out_ids and the log-probabilities travel through the same per-row table.  fp32: both equal the uncompacted call bit for bit."""
    c = _case("ragged3")
    llm = _llm(pack_decode=rows == 12)
    _set_eos(llm, [])
    x, lens, n = _tiled(c, rows)
    max_new = 8
    budgets = [3 if r % 2 == 0 else max_new for r in range(rows)]
    out = {}
    for compact in (False, True):
        ids, n_cols, lps = llm.generate_packed(x.to(DEV), lens, max_new, row_limits=budgets, compact=compact, check_every=4, scores=True)
        out[compact] = (ids.clone(), n_cols, lps.clone(), dict(llm.last_generate_stats))
    assert out[True][3]["compactions"] == 1 and out[True][3]["final_rows"] == rows // 2, out[True][3]
    assert out[False][3]["compactions"] == 0 and out[False][3]["final_rows"] == rows
    assert out[True][1] == out[False][1] == max_new
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][2].view(torch.int32), out[False][2].view(torch.int32))
    for r, n_ in enumerate(budgets):
        assert bool((out[True][2][r, n_:] == 0).all()) and bool((out[True][2][r, :n_] < 0).all())


def test_scores_off_is_the_call_without_them_and_on_never_replays_the_other_graph():
    c = _case("greedy")
    lib = L.lib()
    for pack, rows in ((True, 3), (False, 66)):
        llm = _llm(pack_decode=pack)
        _set_eos(llm, [])
        x, lens, n = _tiled(c, rows)
        max_new = _cfg()[3]
        xd = x.to(DEV)
        llm.generate_packed(xd.clone(), lens, max_new, scores=True)                 # sizes the workspace: the calls below share one buffer
        lib.sl_decode_graph_cache_clear()
        ids0, cols0 = llm.generate_packed(xd.clone(), lens, max_new)                # sl_generate_lp
        st0 = dict(llm.last_generate_stats)
        assert lib.sl_decode_graph_cache_clear() == 1
        # the same call through sl_generate_sc with a NULL buffer / sl_generate_workspace_bytes_sc with scores 0
        lp_fn, ws_fn = lib.sl_generate_lp, lib.sl_generate_workspace_bytes_lp
        seen = []
        try:
            lib.sl_generate_lp = lambda *a: lib.sl_generate_sc(*a, None)
            lib.sl_generate_workspace_bytes_lp = lambda *a: seen.append((ws_fn(*a), lib.sl_generate_workspace_bytes_sc(*a, 0))) or seen[-1][1]
            ids1, cols1 = llm.generate_packed(xd.clone(), lens, max_new)
        finally:
            lib.sl_generate_lp, lib.sl_generate_workspace_bytes_lp = lp_fn, ws_fn
        assert seen and seen[0][0] == seen[0][1]
        assert torch.equal(ids0, ids1) and cols0 == cols1 and dict(llm.last_generate_stats) == st0
        assert st0["decode_launches"] == max_new - 1
        assert lib.sl_decode_graph_cache_clear() == 1
        got = []
        for scores in (False, True, False, True):
            r = llm.generate_packed(xd.clone(), lens, max_new, scores=scores)
            got.append(r)
            assert torch.equal(r[0], ids0)
        assert torch.equal(got[1][2], got[3][2])
        assert lib.sl_decode_graph_cache_clear() == 2                               # one graph without scores, one with: the repeats replayed them


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_log_probabilities_are_finite_and_close_to_the_fp32_run(dtype):
    c = _case("ragged3")
    max_new = _cfg()[3]
    tol = 2 * BF16_TOL * _logit_rms(_prompts(c))
    for pack, rows in ((True, 3), (False, 66)):
        x, lens, n = _tiled(c, rows)
        res = {}
        for dt in (torch.float32, dtype):
            llm = _llm(dt, pack)
            _set_eos(llm, [])
            res[dt] = llm.generate_packed(x.to(dt).to(DEV), lens, max_new, scores=True)
        ids32, _, lp32 = res[torch.float32]
        ids16, _, lp16 = res[dtype]
        assert bool(torch.isfinite(lp16).all()) and bool((lp16 <= 0).all())
        same = ((ids32 == ids16).int().cumprod(dim=1)).bool()                       # steps up to a row's first differing token saw the same history
        assert int(same[:, 0].sum()) > 0
        diff = (lp16.double() - lp32.double()).abs()[same]
        print(f"{dtype} pack_decode={pack} rows={rows}: {int(same.sum())} comparable steps, worst |diff| {float(diff.max()):.3e}, tolerance {tol:.3e}")
        assert bool((diff <= tol).all())
