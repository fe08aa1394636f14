"""GPU: multi-turn sessions — generation continued on a kept K/V cache (KVSession, sl_llama_prefill_cont, sl_generate_cont) on TINY_LLAMA.

fp32 on the model-dtype cache: the ids of a second turn equal the ids of ONE generate over [prompt | fed answer tokens | follow-up] from an
empty cache, and the first-step logits agree within the fp32 tolerance of tests/test_models_gpu.py; the CPU oracle's top-1 / top-2 margins at
every compared step are asserted to exceed what that tolerance can move a logit by, so a near-tie cannot hide behind "ids differ".
bf16 / fp16 on both cache formats: the first-step logits of the continued call against the oracle on the cache the session actually holds
(dequantised for e4m3), with the bounds of tests/test_kv8_gpu.py's decode-step test."""
import ctypes as C
import copy

import pytest
import torch

from conftest import pkg, rel_err
from oracle import llama_oracle as lo
from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA
from test_kv8_gpu import TOL16, _make_llama, dq8, q8

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ri = pkg("random_init")
utils = pkg("utils")
inf_mod = pkg("inference")
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F32_TOL = 1e-4                      # tests/test_models_gpu.py: prefill logits, fp32
LENS, FOLLOW, NEW = (9, 14, 5), 4, 6
SEED = 3                            # chosen on the CPU: the oracle's margins below hold at every compared step


def _prompts(cfg, seed, P=2):
    gen = torch.Generator().manual_seed(seed)
    pre = torch.randn(P, cfg.hidden_size, generator=gen) * 0.05
    prompts = [torch.cat([pre, torch.randn(n - P, cfg.hidden_size, generator=gen) * 0.05]) for n in LENS]
    follow = [torch.randn(FOLLOW, cfg.hidden_size, generator=gen) * 0.05 for _ in LENS]
    return prompts, follow


def _oracle_steps(sd, cfg, x, n, eos):
    """greedy ids of one sequence with per-step (margin, logits norm); stops after the first id in `eos`"""
    embed = sd["model.embed_tokens.weight"].float()
    out = lo.llama_forward(sd, cfg, x[None], last_logits_only=True)
    ids, marg = [], []
    for step in range(n):
        lg = out["logits"][0, -1].float()
        top = lg.topk(2).values
        ids.append(int(lg.argmax()))
        marg.append((float(top[0] - top[1]), float(lg.norm())))
        if ids[-1] in eos or step + 1 == n:
            break
        out = lo.llama_forward(sd, cfg, embed[ids[-1]][None, None], past=out["past"], last_logits_only=True)
    return ids, marg


def _clone(sess):
    c = copy.copy(sess)
    c.k, c.v, c.valid_len, c.pending_id = sess.k.clone(), sess.v.clone(), list(sess.valid_len), list(sess.pending_id)
    return c


@pytest.mark.parametrize("P", [0, 2])
def test_second_turn_equals_one_generate_over_the_concatenation_fp32(P):
    cfg = TINY_LLAMA
    llm, sd = _make_llama(cfg, 41, F32, max_ctx=64)
    prompts, follow = _prompts(cfg, SEED)
    embed = sd["model.embed_tokens.weight"].float()
    # an EOS the oracle is known to emit: the third token of sequence 0's free-running answer, so that row finishes before its budget
    free = [_oracle_steps(sd, cfg, p, NEW, ())[0] for p in prompts]
    eos = free[0][2]
    llm.generation_config.eos_token_id = [eos]
    llm.generation_config.pad_token_id = cfg.pad_token_id
    want1 = [_oracle_steps(sd, cfg, p, NEW, (eos,)) for p in prompts]
    assert len({len(w[0]) for w in want1}) > 1 and len(want1[0][0]) <= 3, "one row must finish by EOS before the others"
    concat = [torch.cat([p, embed[torch.tensor(w[0])], f]) for p, w, f in zip(prompts, want1, follow)]
    want2 = [_oracle_steps(sd, cfg, c, NEW, (eos,)) for c in concat]
    for ids_, marg in want1 + want2:       # the margin a logit pair needs against a relative-L2 error of F32_TOL on either side
        for m, norm in marg:
            assert m > 2 * F32_TOL * norm, (m, norm)
    sess = llm.new_session(len(LENS))
    x1 = torch.cat(prompts).to(DEV)
    ids1, n1 = llm.generate_packed(x1.clone(), list(LENS), NEW, shared_prefix=P, session=sess)
    for s, (w, _) in enumerate(want1):
        assert ids1[s, :len(w)].tolist() == w and sess.pending_id[s] == w[-1] and sess.valid_len[s] == LENS[s] + len(w) - 1, (s, ids1[s], w)
    assert sess.shared_prefix == P
    # first-step logits of the continued call (on a copy of the session) against the one-shot prefill of the concatenation
    probe = _clone(sess)
    got = llm(inputs_embeds=[f.to(DEV) for f in follow], use_cache=True, past_key_values=probe).logits[:, 0].cpu()
    assert probe.valid_len == [v + 1 + FOLLOW for v in sess.valid_len] and probe.pending_id == [None] * 3
    for s, c in enumerate(concat):
        ref = llm(inputs_embeds=c[None].to(DEV)).logits[0, -1].cpu()
        orc = lo.llama_forward(sd, cfg, c[None], last_logits_only=True)["logits"][0, -1]
        assert rel_err(got[s], ref) < F32_TOL and rel_err(got[s], orc) < F32_TOL, (s, rel_err(got[s], ref), rel_err(got[s], orc))
    # turn 2 against ONE generate over the concatenation from an empty cache
    ids2, n2 = llm.generate_packed(torch.cat(follow).to(DEV), [FOLLOW] * 3, NEW, session=sess)
    ref2, nr = llm.generate_packed(torch.cat(concat).to(DEV), [int(c.shape[0]) for c in concat], NEW, shared_prefix=P, compact=False)
    assert n2 == nr and torch.equal(ids2, ref2), (ids2, ref2)
    for s, (w, _) in enumerate(want2):
        assert ids2[s, :len(w)].tolist() == w, (s, ids2[s], w)
    assert sess.turns == 2 and sess.valid_len == [int(c.shape[0]) + len(w[0]) - 1 for c, w in zip(concat, want2)]
    with pytest.raises(L.SpeechLLMError):      # 64 positions: a third turn of 40 new tokens does not fit, refused before any launch
        llm.generate_packed(torch.cat(follow).to(DEV), [FOLLOW] * 3, 40, session=sess)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("kvd", [None, "fp8"])
def test_continued_prefill_logits_against_the_oracle_on_the_session_cache(dt, kvd):
    cfg = TINY_LLAMA
    llm, sd = _make_llama(cfg, 43, dt, kv_cache_dtype=kvd, max_ctx=64)
    llm.generation_config.eos_token_id = None
    prompts, follow = _prompts(cfg, 11)
    sdq = {k: v.to(dt).float() for k, v in sd.items()}
    embed = sdq["model.embed_tokens.weight"]
    sess = llm.new_session(3)
    ids1, _ = llm.generate_packed(torch.cat(prompts).to(DEV, dt), list(LENS), NEW, use_eos=False, session=sess)
    assert sess.valid_len == [n + NEW - 1 for n in LENS] and sess.pending_id == ids1[:, NEW - 1].tolist()
    held = (sess.k.cpu(), sess.v.cpu())
    valid = list(sess.valid_len)
    got = llm(inputs_embeds=[f.to(DEV, dt) for f in follow], use_cache=True, past_key_values=sess).logits[:, 0].cpu()
    for s in range(3):
        n = valid[s]
        rows = torch.cat([embed[int(ids1[s, NEW - 1])][None], follow[s].to(dt).float()])[None]      # the pending token, then the follow-up rows
        conv = (lambda t_: dq8(t_).float()) if kvd else (lambda t_: t_.float())
        past = [(conv(held[0][l, s, :, :n])[None], conv(held[1][l, s, :, :n])[None]) for l in range(cfg.num_hidden_layers)]
        ref = lo.llama_forward(sdq, cfg, rows, past=past, last_logits_only=True)["logits"][0, -1]
        bound = TOL16[dt]
        if kvd:      # d8 from the oracle alone (tests/test_kv8_gpu.py): its logits with its exact past against those with q8 of that past
            fed = torch.cat([prompts[s].to(dt).float(), embed[ids1[s, :NEW - 1].long()]])[None]
            exact = lo.llama_forward(sdq, cfg, fed, last_logits_only=True)["past"]
            a = lo.llama_forward(sdq, cfg, rows, past=exact, last_logits_only=True)["logits"][0, -1]
            pq = [(dq8(q8(k)).float(), dq8(q8(v)).float()) for k, v in exact]
            b = lo.llama_forward(sdq, cfg, rows, past=pq, last_logits_only=True)["logits"][0, -1]
            bound += rel_err(b, a)
        e = rel_err(got[s], ref)
        print(f"continued prefill {dt} kv={kvd} sequence {s}: rel err {e:.3e}, bound {bound:.3e}")
        assert e < bound, (s, e, bound)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_fp8_session_bytes_are_q8_of_the_16bit_session(dt):
    """two forward() turns with the same rows into a 16-bit and an e4m3 session: the first turn is the one-shot prefill (every layer's bytes are
    q8 of the 16-bit rows); the second turn's rows at [past, past + len) are q8 of the 16-bit session's in layer 0, whose K/V depend on the input
    rows alone (deeper layers attend the quantised past and legitimately differ)"""
    cfg = TINY_LLAMA
    prompts, follow = _prompts(cfg, 12)
    caches = {}
    for kvd in (None, "fp8"):
        llm, _ = _make_llama(cfg, 43, dt, kv_cache_dtype=kvd, max_ctx=64)
        sess = llm.new_session(3)
        llm(inputs_embeds=[p.to(DEV, dt) for p in prompts], use_cache=True, past_key_values=sess)
        llm(inputs_embeds=[f.to(DEV, dt) for f in follow], use_cache=True, past_key_values=sess)
        assert sess.valid_len == [n + FOLLOW for n in LENS]
        caches[kvd] = (sess.k.cpu(), sess.v.cpu())
        del llm
    for which in (0, 1):
        c16, c8 = caches[None][which], caches["fp8"][which]
        for s, n in enumerate(LENS):
            assert torch.equal(c8[:, s, :, :n], q8(c16[:, s, :, :n].float())), ("first turn", which, s)
            assert torch.equal(c8[0, s, :, n:n + FOLLOW], q8(c16[0, s, :, n:n + FOLLOW].float())), ("second turn, layer 0", which, s)
            assert bool((c8[:, s, :, n + FOLLOW:] == 0).all()), "cache written behind the second turn"


def _direct(llm, entry, x, lens, past, kv, max_new, sample=None, logits=None, scores=True):
    """sl_generate_sc / sl_generate_cont called by hand with generate_packed's options -> (ids, logprobs, decode_launches)"""
    lib = L.lib()
    B = len(lens)
    cu_c, eos_c, n_eos, use_eos, pad = llm._generate_preamble(lens, max_new, True, 0)
    o = L.GenerateOpts()
    o.eos_ids_host, o.n_eos, o.pad_id, o.use_eos = eos_c, n_eos, int(pad), int(use_eos)
    o.max_new_tokens, o.check_every, o.compact = max_new, 4, 0
    if sample is not None:
        o.sample, o.temperature, o.top_k, o.top_p, o.seed = 1, sample["temperature"], sample["top_k"], sample["top_p"], sample["seed"]
    lp = llm._logits_struct(logits, max_new)
    lp_ref = C.byref(lp) if lp is not None else None
    struct, _ = llm._struct_for(B)
    out, lps, st = (C.c_int32 * (B * max_new))(), (C.c_float * (B * max_new))(), L.GenerateStats()
    ws = llm._workspace(lib.sl_generate_workspace_bytes_sc(C.byref(struct), x.shape[0], B, max_new, lp_ref, 1))
    assert lib.sl_generate_workspace_bytes_cont(C.byref(struct), x.shape[0], B, max_new, lp_ref, 1) == lib.sl_generate_workspace_bytes_sc(C.byref(struct), x.shape[0], B, max_new, lp_ref, 1)
    args = (C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(), L.stream_ptr(), lp_ref, lps)
    if entry == "sc":
        L.check(lib.sl_generate_sc(*args), "sl_generate_sc")
    else:
        L.check(lib.sl_generate_cont(*args, (C.c_int32 * B)(*past), None), "sl_generate_cont")
    return (torch.frombuffer(out, dtype=torch.int32).clone().view(B, max_new), torch.frombuffer(lps, dtype=torch.float32).clone().view(B, max_new),
            int(st.decode_launches))


def test_generate_cont_with_zero_pasts_is_generate_sc():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 44, BF16, max_ctx=64)
    llm.generation_config.eos_token_id = None
    prompts, _ = _prompts(cfg, 13)
    x = torch.cat(prompts).to(DEV, BF16)
    sess = llm.new_session(3)
    a = _direct(llm, "sc", x.clone(), list(LENS), None, sess.kv_struct(), NEW)
    ka = sess.k.clone()
    sess.k.zero_(); sess.v.zero_()
    b = _direct(llm, "cont", x.clone(), list(LENS), [0, 0, 0], sess.kv_struct(), NEW)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and a[2] == b[2] == NEW - 1
    assert torch.equal(ka, sess.k)


def test_plain_generate_between_turns_and_sampling_pass_through():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 45, BF16, max_ctx=64)
    llm.generation_config.eos_token_id = None
    prompts, follow = _prompts(cfg, 14)
    x, xf = torch.cat(prompts).to(DEV, BF16), torch.cat(follow).to(DEV, BF16)
    runs = []
    for disturb in (False, True):
        sess = llm.new_session(3)
        i1 = llm.generate(inputs_embeds=[p.to(DEV, BF16) for p in prompts], max_new_tokens=NEW, past_key_values=sess)
        if disturb:      # a call without a session runs in the model's own buffer
            llm.generate(inputs_embeds=[f.to(DEV, BF16) for f in follow[::-1]], max_new_tokens=9)
        i2 = llm.generate(inputs_embeds=[f.to(DEV, BF16) for f in follow], max_new_tokens=NEW, past_key_values=sess)
        runs.append((i1, i2, sess))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert llm._kv is not None and llm._kv[0].data_ptr() != runs[1][2].k.data_ptr()
    # a sampled third turn with a repetition penalty through the session against the direct sl_generate_cont call with the same options
    sess = runs[0][2]
    twin = _clone(sess)
    smp = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7)
    got = llm.generate(inputs_embeds=[f.to(DEV, BF16) for f in follow], max_new_tokens=NEW, past_key_values=sess, do_sample=True, seed=7, temperature=0.8,
                       top_k=20, top_p=0.9, repetition_penalty=1.2, output_scores=True)
    rows, lens = llm._session_rows(twin, xf.clone(), [FOLLOW] * 3)
    want = _direct(llm, "cont", rows, lens, twin.valid_len, twin.kv_struct(), NEW, sample=smp, logits=dict(repetition_penalty=1.2))
    assert torch.equal(got.cpu(), want[0].long()) and torch.equal(llm.last_token_logprobs.view(torch.int32), want[1].view(torch.int32))
    with pytest.raises(L.SpeechLLMError):
        llm.generate(inputs_embeds=[f.to(DEV, BF16) for f in follow], max_new_tokens=2, past_key_values=sess, num_beams=2)
    with pytest.raises(L.SpeechLLMError):
        llm.generate(inputs_embeds=[f.to(DEV, BF16) for f in follow], max_new_tokens=2, past_key_values=sess, do_sample=True, num_return_sequences=2)
    with pytest.raises(L.SpeechLLMError):
        llm.generate_packed(xf.clone(), [FOLLOW] * 3, 2, session=sess, compact=True)


class _Tok:
    """text -> ids by table (the pipeline's stub tokenizer, tests/test_models_gpu.py)"""
    bos_token_id = None

    def __init__(self, table):
        self.table = table

    def __call__(self, text, return_tensors="pt"):
        from types import SimpleNamespace
        return SimpleNamespace(input_ids=self.table[text].clone())

    def batch_decode(self, ids, **kw):
        return [" ".join(str(int(i)) for i in row) for row in ids]


def test_conversation_equals_generate_over_the_hand_built_prompt_fp32():
    """start_conversation / ask on the tiny pipeline: the follow-up answers equal those of one generate_packed over
    [first prompt | fed answer | follow-up template] built by hand"""
    from conftest import golden, t
    from test_models_gpu import make_encoder, make_llama
    g = golden("pipeline_tiny")
    cfg = TINY_LLAMA
    enc, _ = make_encoder(TINY_HUBERT, cfg.hidden_size, int(g["enc_seed"]), F32)
    llm, _ = make_llama(cfg, int(g["llm_seed"]), F32)
    V = cfg.vocab_size
    q_ids = torch.tensor([[5 % V, 77 % V, 130 % V, 9 % V, 41 % V]])
    q_ids_noeot = q_ids[:, 1:]
    table = {utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"]),
             utils.follow_up_prompt(utils.LLAMA_ID, "WHY"): q_ids, utils.follow_up_prompt(utils.LLAMA_ID, "WHY", drop_eot=True): q_ids_noeot}
    conf = enc.config
    inf = inf_mod.LLMSpeechTextInference(conf, None, DEV, tokenizer=_Tok(table), llm=llm, audio_encoder=enc, dtype=F32)
    waves = [ri.synthetic_waveform(int(g["n_samples"]), seed=int(g["wave_seed"])).numpy(), ri.synthetic_waveform(21000, seed=77).numpy()]
    first, conv = inf.start_conversation(waves, max_new_tokens=8)
    ids1 = conv.last_generate_ids.cpu()
    assert first == inf.generate_audio_responses(waves, max_new_tokens=8) and torch.equal(ids1, inf.last_generate_ids.cpu())
    eos = set(llm.generation_config.eos_token_id)
    pend = list(conv.session.pending_id)
    texts2 = conv.ask("WHY", max_new_tokens=8)
    ids2 = conv.last_generate_ids.cpu()
    # by hand: the packed first prompts again (the chunk builder, one utterance at a time), the fed answer, the follow-up ids
    emb = llm.model.embed_tokens
    rows = []
    for s, w in enumerate(waves):
        cap = {}
        keep = llm.generate_packed
        llm.generate_packed = lambda x, lens, *a, **k: cap.update(x=x.clone()) or keep(x, lens, *a, **k)
        try:
            inf._generate_chunk([w], [""], 1)
        finally:
            llm.generate_packed = keep
        gl = next((i + 1 for i, tok in enumerate(ids1[s].tolist()) if tok in eos), ids1.shape[1])
        fu = q_ids_noeot if pend[s] in eos else q_ids
        rows.append(torch.cat([cap["x"], emb(ids1[s, :gl].to(DEV)), emb(fu[0].to(DEV))]))
    ref, n_ref = llm.generate_packed(torch.cat(rows), [int(r.shape[0]) for r in rows], 8, compact=False)
    assert torch.equal(ids2, ref[:, :n_ref].long()), (ids2, ref)
    assert texts2 == [" ".join(str(int(i)) for i in row) for row in ref[:, :n_ref]]
