"""GPU: several sampled answers per prompt.  The grouped decode attention per element against a poisoned cache (prompt
slots and row slots, scrambled rows, records that overflow), sl_generate_n against today's call on every prompt repeated N times (fp32,
bit for bit), the grouped path against the copy path in 16 bits, and N = 1 as sl_generate_sc."""
import ctypes as C

import pytest
import torch

from conftest import pkg
from oracle.golden_cfgs import TINY_LLAMA, TINY_MHA
from edge_helpers import BF16, BIG, DEV, F16, F32, FILL, gauss, operand, tuning  # noqa: F401
from test_kernel_edges_gpu import attn_bounds, check_attn

pytestmark = pytest.mark.gpu
L = pkg("_lib")
ops = pkg("ops")
ri = pkg("random_init")
weights = pkg("weights")
llama_mod = pkg("audio_llama")
F8 = torch.float8_e4m3fn

# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels, per element
# ------------------------------------------------------------------------------------------------------------------------------
# 14 rows in scrambled order: a group of 7 (two records at REP 3 and 4), one of 5, one of 1, and a row without a prefix
GROUP_OF_ROW = [0, 1, 0, 3, 0, 1, 2, 0, 1, 0, 1, 0, 1, 0]          # 0: the 7, 1: the 5, 2: the single row, 3: no prefix
TAILS = [0, 1, 63, 64, 65, 130]
PREFIX_SETS = [(129, 200, 1), (63, 64, 65), (128, 65, 64)]            # prefix length of group 0, 1, 2 (= of prompt slot 0, 1, 2)
ROW_SLOT0, MAX_CTX, D = 3, 448, 128


def _cache(x64, dt, fmt):
    """fp64 -> (device cache in the format, its exact stored values in fp64): e4m3 rows are q8(what the 16-bit cache would hold)"""
    d = x64.float().to(dt)
    if fmt == L.KV_FP8_E4M3:
        d8 = d.float().clamp(-448.0, 448.0).to(F8)
        return d8.view(torch.uint8).to(DEV), d8.float().double()
    return d.to(DEV), d.double()


@pytest.mark.parametrize("prefixes", PREFIX_SETS, ids=lambda p: "p" + "_".join(map(str, p)))
@pytest.mark.parametrize("nh,nkv", [(6, 2), (4, 1), (2, 2)])
@pytest.mark.parametrize("fmt", [L.KV_MODEL_DTYPE, L.KV_FP8_E4M3], ids=["kv16", "kv8"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_grouped_decode_attention_mask_probe_and_gaussian(dt, fmt, nh, nkv, prefixes):
    """Row b attends [0, P) of its prompt slot and [P, n) of slot 3 + b.  Poison (K 8.0, V large) sits at positions < P of every row slot,
    >= P of every prompt slot and >= n of every row slot: the state of a reused cache.  V once as the one-hot probe (an output no visible
    key feeds must be exactly 0, every other one is a single probability) and once Gaussian; reference and bound are the edge suite's
    (attn_bounds / check_attn) over cat(prompt slot[:P], own slot[P:n]).  The output buffer is guarded above and below."""
    B, n_slots = len(GROUP_OF_ROW), ROW_SLOT0 + len(GROUP_OF_ROW)
    scale = D ** -0.5
    pslot = [g if g < 3 else 0 for g in GROUP_OF_ROW]
    plen = [prefixes[g] if g < 3 else 0 for g in GROUP_OF_ROW]
    tails = [TAILS[(b + 2 * g) % len(TAILS)] if g < 3 else 65 for b, g in enumerate(GROUP_OF_ROW)]
    assert set(t_ for t_, g in zip(tails, GROUP_OF_ROW) if g == 0) >= {0, 1, 63, 64, 65, 130}
    ctx = [p + t_ for p, t_ in zip(plen, tails)]
    assert max(ctx) <= MAX_CTX
    q, q64 = operand(gauss((B, nh * D), 900 + nh), dt)
    k64 = gauss((n_slots, nkv, MAX_CTX, D), 901)
    vg64 = gauss((n_slots, nkv, MAX_CTX, D), 902)
    vp64 = torch.zeros_like(vg64)
    j = torch.arange(MAX_CTX)
    vp64[:, :, j, j % D] = 1.0
    for t64, poison in ((k64, 8.0), (vg64, BIG[dt]), (vp64, BIG[dt])):
        for s in range(3):
            t64[s, :, prefixes[s]:] = poison
        for b in range(B):
            t64[ROW_SLOT0 + b, :, :plen[b]] = poison
            t64[ROW_SLOT0 + b, :, ctx[b]:] = poison
    kc, k64 = _cache(k64, dt, fmt)
    ctx_d = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    for cls, v64_ in (("P", vp64), ("G", vg64)):
        vc, v64 = _cache(v64_, dt, fmt)
        obuf = torch.full((B + 2, nh * D), FILL, device=DEV, dtype=dt)
        out = obuf[1:B + 1]
        ops.attn_decode_grouped(q, q.stride(0), kc, vc, ctx_d, pslot, plen, ROW_SLOT0, nh, nkv, D, MAX_CTX, scale, kv_format=fmt, out=out)
        assert bool((obuf[0] == FILL).all()) and bool((obuf[B + 1] == FILL).all())
        for b in range(B):
            P, n = plen[b], ctx[b]
            kk = torch.cat([k64[pslot[b], :, :P], k64[ROW_SLOT0 + b, :, P:n]], dim=1)
            vv = torch.cat([v64[pslot[b], :, :P], v64[ROW_SLOT0 + b, :, P:n]], dim=1)
            ref, tol, zero = attn_bounds(q64[b].view(nh, 1, D), kk, vv, torch.ones(1, n, dtype=torch.bool), scale, dt)
            check_attn(out[b:b + 1], ref, tol, zero, dt, f"{cls} row {b}: prefix {P} of slot {pslot[b]} + tail {n - P}")


# ------------------------------------------------------------------------------------------------------------------------------
# 2-4. model level
# ------------------------------------------------------------------------------------------------------------------------------
LENS = (9, 21, 14, 5, 33)
SAMPLE = dict(temperature=0.9, top_k=40, top_p=0.95, seed=123)
_LLMS = {}


def _llm(cfg, dtype, kv=None):
    key = (id(cfg), dtype, kv)
    if key not in _LLMS:
        arch = weights.LlamaArch(cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim,
                                 cfg.intermediate_size, cfg.vocab_size, cfg.rms_norm_eps, cfg.rope_theta, cfg.rope_scaling, cfg.tie_word_embeddings,
                                 tuple(cfg.eos_token_ids), cfg.pad_token_id)
        _LLMS[key] = llama_mod.AudioLlamaForCausalLM(arch, dict(ri.llama_state_dict(cfg, seed=41)), torch_dtype=dtype, device=DEV, max_ctx=96,
                                                     kv_cache_dtype=kv)
    return _LLMS[key]


def _prompts(cfg):
    gen = torch.Generator().manual_seed(77)
    return [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in LENS]


def _packed(prompts, dtype, times=1):
    rows = [p for p in prompts for _ in range(times)]
    return torch.cat(rows).to(dtype).to(DEV).contiguous(), [int(p.shape[0]) for p in rows]


@pytest.mark.parametrize("cfg", [TINY_LLAMA, TINY_MHA], ids=["gqa", "mha"])
def test_fp32_answers_equal_the_call_on_repeated_prompts_bit_for_bit(cfg):
    """fp32 (the copy path: the grouped kernels are 16-bit): ids, n_cols and log-probabilities of generate_packed(num_return=3) are those of
    today's call on the 15 repeated prompts, with EOS on; with row budgets that finish rows early, compacted or not; one prefill of 5."""
    llm, N, max_new = _llm(cfg, F32), 3, 24
    prompts = _prompts(cfg)
    x5, lens5 = _packed(prompts, F32)
    x15, lens15 = _packed(prompts, F32, N)
    want = llm.generate_packed(x15.clone(), lens15, max_new, sample=SAMPLE, scores=True, compact=False)
    assert "prefill_seqs" not in llm.last_generate_stats
    got = llm.generate_packed(x5.clone(), lens5, max_new, sample=SAMPLE, scores=True, compact=False, num_return=N)
    st = llm.last_generate_stats
    assert (st["prefill_seqs"], st["rows"], st["num_return_sequences"], st["attn_path"]) == (5, 15, N, "copy")
    assert got[1] == want[1] and torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert got[0].shape == (15, max_new)
    assert len({tuple(r) for r in got[0][:N].tolist()}) > 1, "the answers of one prompt are different draws"
    limits = [3 + (5 * b) % 20 for b in range(15)]
    want_l = llm.generate_packed(x15.clone(), lens15, max_new, sample=SAMPLE, scores=True, compact=False, row_limits=limits)
    for compact in (False, True):
        got_l = llm.generate_packed(x5.clone(), lens5, max_new, sample=SAMPLE, scores=True, compact=compact, check_every=2, row_limits=limits, num_return=N)
        st = llm.last_generate_stats
        assert (st["compactions"] >= 1) == compact and st["prefill_seqs"] == 5
        assert got_l[1] == want_l[1] and torch.equal(got_l[0], want_l[0]) and torch.equal(got_l[2], want_l[2]), compact


def _teacher_forced_error(llm, prompts, ids, lps, N):
    """max |returned log-probability - log_softmax(forward(prompt + returned ids))[id]| over every token"""
    worst = 0.0
    emb = llm.model.embed_tokens
    for s, p in enumerate(prompts):
        rows = ids[s * N:(s + 1) * N].to(torch.int64).to(DEV)                      # (N, T)
        T = rows.shape[1]
        x = torch.cat([p.to(llm.dtype).to(DEV)[None].expand(N, -1, -1), emb(rows[:, :-1]).to(llm.dtype)], dim=1)
        logits = llm.forward(inputs_embeds=x).logits.float()[:, p.shape[0] - 1:p.shape[0] - 1 + T]
        ref = torch.log_softmax(logits, dim=-1).gather(-1, rows[..., None])[..., 0].cpu()
        worst = max(worst, float((ref - lps[s * N:(s + 1) * N]).abs().max()))
    return worst


@pytest.mark.parametrize("kv", [None, "fp8"], ids=["kv16", "kv8"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_16bit_grouped_path_is_as_close_to_forward_as_the_copy_path(dt, kv, tuning):
    """N = 5, plain sampling (temperature 1, top_k 0, top_p 1), EOS off, 16 tokens: e = max |returned log-probability - log_softmax of
    forward on prompt + returned ids|, once on the copy path (the existing attention kernels: the yardstick) and once on the grouped
    path; e_grouped <= 2 e_copy (both do the same arithmetic with different rescale points; 2 covers the scatter of a maximum over 400
    tokens).  Then a compacting grouped run against its uncompacted run.
    Measured (MI355X): see DESIGN 8.16."""
    cfg, N, max_new = TINY_LLAMA, 5, 16
    llm = _llm(cfg, dt, kv)
    prompts = _prompts(cfg)
    x5, lens5 = _packed(prompts, dt)
    smp = dict(temperature=1.0, top_k=0, top_p=1.0, seed=321)
    e = {}
    for name, sw in (("copy", "0"), ("grouped", "1")):
        tuning("SL_GEN_GROUP_ATTN", sw)
        ids, n_cols, lps = llm.generate_packed(x5.clone(), lens5, max_new, use_eos=False, sample=smp, scores=True, num_return=N)
        assert llm.last_generate_stats["attn_path"] == name and llm.last_generate_stats["prefill_seqs"] == 5
        assert n_cols == max_new and ids.shape == (25, max_new) and bool(torch.isfinite(lps).all()) and bool((lps <= 0).all())
        e[name] = _teacher_forced_error(llm, prompts, ids, lps, N)
    print(f"{dt} kv={kv}: e_copy {e['copy']:.4e}  e_grouped {e['grouped']:.4e}")
    assert e["grouped"] <= 2 * e["copy"], e
    limits = [2 + (7 * b) % 15 for b in range(25)]
    runs = {}
    for compact in (False, True):
        runs[compact] = llm.generate_packed(x5.clone(), lens5, max_new, use_eos=False, sample=smp, scores=True, num_return=N, row_limits=limits,
                                            compact=compact, check_every=2)
        st = llm.last_generate_stats
        assert st["attn_path"] == "grouped" and (st["compactions"] >= 1) == compact
    assert runs[True][1] == runs[False][1] and torch.equal(runs[True][0], runs[False][0])


def test_n_1_is_sl_generate_sc_and_reuses_its_graph():
    cfg, max_new = TINY_LLAMA, 12
    llm = _llm(cfg, BF16)
    lib = L.lib()
    prompts = _prompts(cfg)
    B = len(prompts)
    cu = [0]
    for p in prompts:
        cu.append(cu[-1] + p.shape[0])
    cu_c = (C.c_int32 * (B + 1))(*cu)
    struct, _ = llm._struct_for(B)
    kv = llm._kv_cache(B)
    o = L.GenerateOpts()
    o.max_new_tokens, o.check_every, o.sample, o.temperature, o.top_k, o.top_p, o.seed = max_new, 4, 1, 0.9, 40, 0.95, 5
    nbytes = lib.sl_generate_workspace_bytes_sc(C.byref(struct), cu[-1], B, max_new, None, 1)
    assert lib.sl_generate_workspace_bytes_n(C.byref(struct), cu[-1], B, max_new, None, 1, 1) == nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def run(n_entry):
        x, _ = _packed(prompts, BF16)
        out, lps, st = (C.c_int32 * (B * max_new))(), (C.c_float * (B * max_new))(), L.GenerateStats()
        args = (C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(), L.stream_ptr(), None, lps)
        L.check(lib.sl_generate_n(*args, 1) if n_entry else lib.sl_generate_sc(*args), "generate")
        return list(out), list(lps)

    lib.sl_decode_graph_cache_clear()
    want = run(False)
    n_sc = lib.sl_decode_graph_cache_clear()
    assert n_sc >= 1
    assert run(False) == want
    got = run(True)
    assert lib.sl_generate_last_attn_path() == 0
    assert got == want
    assert lib.sl_decode_graph_cache_clear() == n_sc, "sl_generate_n(.., 1) captured a graph of its own"
