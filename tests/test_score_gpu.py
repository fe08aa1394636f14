"""GPU, model level (tiny shapes): AudioLlamaForCausalLM.score() — teacher-forced log-probabilities through sl_llama_score —
against the reference's own numbers (tests/golden/token_scores_tiny.npz: greedy answers; tests/golden/score_tiny.npz, written by
tools/gen_score_golden.py: random answers that are not the argmax), against the per-sample forward(labels=) path on the device, across
lm_head chunkings and raggedness, and the promise that nothing else moves (generate()'s ids and captured graphs, a live session, the
Trainer without its opt-in key).

Tolerances: 2 x F32_TOL x rms of the logits (tests/test_token_scores_gpu.py: a log-probability is a logit minus a log-sum-exp of logits,
the tolerance tests/test_models_gpu.py allows fp32 logits taken twice), 2 x BF16_TOL x rms in the 16-bit modes; where two runs saw the
same logits, twice the per-token rounding bound of tests/token_scores_ref.py (bound_row + bound_partial, as in
tests/test_score_kernels_gpu.py)."""
import numpy as np
import pytest
import torch

from conftest import golden, pkg, t

import token_scores_ref as tsr
from test_token_scores_gpu import BF16_TOL, F32_TOL, _case, _cfg, _llm, _logit_rms, _prompts, _set_eos

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = pkg("_lib")
llama_mod = pkg("audio_llama")

UNPROCESSED = ["greedy", "eos_all", "eos_one", "batch1", "batch1_eos", "ragged3", "ragged3_eos"]
MIN_MARGIN = 1e-3          # tools/gen_token_scores_golden.py: the recorded ids are the argmax with at least this margin


def _room(llm, slots=32):
    """score() never replaces the model's K/V cache: give it the slots these batches need"""
    llm._kv_cache(slots)
    return llm


def _recorded(name):
    c = _case(name)
    assert float(c["min_margin"]) >= MIN_MARGIN
    lens = c["lens"].tolist()
    ids, lps = t(c["ids"]).long(), t(c["logprobs"]).double()
    return _prompts(c), [ids[b, :n] for b, n in enumerate(lens)], [lps[b, :n] for b, n in enumerate(lens)]


# ------------------------------------------------------------------------------------------------ the reference's numbers in the tree
@pytest.mark.parametrize("name", UNPROCESSED)
def test_score_returns_the_recorded_log_probabilities_of_the_greedy_answers(name):
    """each case alone: at most 36 rows, the unfused path"""
    prompts, targets, want = _recorded(name)
    llm = _room(_llm())
    out = llm.score([p.to(DEV) for p in prompts], targets, return_top1=True)
    assert out.paths == {"rows"}
    tol = 2 * F32_TOL * _logit_rms(prompts)
    for b, w in enumerate(want):
        got = out.token_logprobs[b].double().cpu()
        assert out.token_logprobs[b].dtype == torch.float32 and got.shape == w.shape
        assert bool(((got - w).abs() <= tol).all()), (name, b, float((got - w).abs().max()), tol)
        assert bool(out.top1_match[b].all())
        assert abs(float(out.sequence_logprobs[b]) - float(w.sum())) <= tol * len(w) and int(out.n_tokens[b]) == len(w)
    nll = torch.stack([-w.mean() for w in want])
    assert bool(((out.nll.cpu() - nll).abs() <= tol).all())
    assert abs(out.perplexity() - float(torch.exp(nll.mean()))) <= 2 * tol * float(torch.exp(nll.mean()))


def test_all_seven_cases_in_one_call_take_the_fused_path():
    """17 sequences, more than 64 rows in one lm_head pass: sl_gemm_top1_lse_tgt + sl_score_finalize (asserted through the paths the call reports)"""
    prompts, targets, want = [], [], []
    for name in UNPROCESSED:
        p, tg, w = _recorded(name)
        prompts, targets, want = prompts + p, targets + tg, want + w
    assert len(prompts) == 17 and sum(len(w) for w in want) > 64
    llm = _room(_llm())
    out = llm.score([p.to(DEV) for p in prompts], targets, return_top1=True)
    assert out.paths == {"fused"}
    assert out.sequence_logprobs.shape == (17,) and out.n_tokens.tolist() == [len(w) for w in want]
    worst = 0.0
    for b, w in enumerate(want):
        tol = 2 * F32_TOL * _logit_rms(prompts[b:b + 1])
        d = float((out.token_logprobs[b].double().cpu() - w).abs().max())
        assert d <= tol, (b, d, tol)
        assert bool(out.top1_match[b].all())
        worst = max(worst, d / tol)
    print(f"17 sequences fused: worst |diff| / tolerance {worst:.3f}")
    forced = llm.score([p.to(DEV) for p in prompts], targets, force_path=1)
    assert forced.paths == {"rows"}


# ------------------------------------------------------------------------------------------------ targets that are not the argmax
def _score_tiny(n):
    g = golden("score_tiny")
    seed = int(g[f"n{n}.input_seed"])
    prompts = [torch.randn(int(P), 256, generator=torch.Generator().manual_seed(seed * 100 + b)) * 0.05 for b, P in enumerate(g["prompt_lens"].tolist())]
    return prompts, t(g[f"n{n}.targets"]).long(), t(g[f"n{n}.logprobs"]).double(), t(g[f"n{n}.loss"]).double()


@pytest.mark.parametrize("n", [1, 2, 13])
def test_random_targets_match_the_reference_class(n):
    """tests/golden/score_tiny.npz: the reference class's per-token log_softmax gather (fp64) and its forward(labels=).loss per sample, for
    seeded random targets at the ragged prompt lengths 9 / 21 / 14"""
    prompts, targets, want, loss = _score_tiny(n)
    llm = _room(_llm())
    out = llm.score([p.to(DEV) for p in prompts], [targets[b] for b in range(3)], return_top1=True)
    tol = 2 * F32_TOL * _logit_rms(prompts)
    for b in range(3):
        got = out.token_logprobs[b].double().cpu()
        assert got.shape == (n,) and bool(((got - want[b]).abs() <= tol).all()), (n, b, got, want[b], tol)
    assert bool(((out.nll.cpu() - loss).abs() <= tol).all()), (out.nll, loss)          # the labels[1:] convention: loss = the mean over the targets
    assert not bool(torch.cat(out.top1_match).all())                                      # random ids are not the argmax


# ------------------------------------------------------------------------------------------------ against the per-sample path on the device
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_nll_equals_the_loss_of_forward_with_labels(dtype):
    """forward(inputs_embeds=[prompt | embed(resp[1:])], labels=[resp]).loss (the path Trainer.validate loops over) against score(prompt,
    resp[1:]).nll for the same sample"""
    prompts, targets, _, _ = _score_tiny(13)
    llm = _room(_llm(dtype))
    emb = llm.model.embed_tokens
    tol = 2 * (F32_TOL if dtype == torch.float32 else BF16_TOL) * _logit_rms(prompts)
    out = llm.score([p.to(DEV, dtype) for p in prompts], [targets[b] for b in range(3)])
    for b in range(3):
        resp = torch.cat([torch.zeros(1, dtype=torch.long), targets[b]]).to(DEV)
        seq = torch.cat([prompts[b].to(DEV, dtype), emb(resp[1:])], 0)
        loss = float(llm(inputs_embeds=seq[None], labels=[resp]).loss)
        print(f"{dtype} sample {b}: loss {loss:.6f} nll {float(out.nll[b]):.6f} tolerance {tol:.3e}")
        assert abs(loss - float(out.nll[b])) <= tol


# ------------------------------------------------------------------------------------------------ chunking, raggedness
def _chunk_batch():
    """12 sequences of 25 targets = 300 scored rows; ignored positions at the edges of the 128-row passes, inside one and at the very end"""
    gen = torch.Generator().manual_seed(77)
    plens = [9, 21, 14, 30, 5, 17, 1, 26, 11, 33, 8, 19]
    prompts = [torch.randn(P, 256, generator=torch.Generator().manual_seed(9000 + b)) * 0.05 for b, P in enumerate(plens)]
    targets = torch.randint(0, 1000, (12, 25), generator=gen)
    flat = targets.view(-1)
    ignored = [0, 127, 128, 200, 255, 256, 299]
    for r in ignored:
        flat[r] = -100
    return prompts, targets, ignored


def test_nothing_depends_on_the_chunk_a_row_falls_in():
    """row_chunk=128 on 300 rows: passes of 128, 128 (fused) and 44 rows (fp32 logits, pinned to the family of a full pass), against one
    fused pass of 300 (row_chunk=0) and against fp32 logits everywhere (force_path=1): the same logits, so twice the per-token bound"""
    prompts, targets, ignored = _chunk_batch()
    llm = _room(_llm())
    pd = [p.to(DEV) for p in prompts]
    tg = [targets[b] for b in range(12)]
    runs = {"chunk128": llm.score(pd, tg, row_chunk=128, return_top1=True), "one_pass": llm.score(pd, tg, row_chunk=0, return_top1=True),
            "rows_only": llm.score(pd, tg, force_path=1, return_top1=True), "rows_chunk128": llm.score(pd, tg, row_chunk=128, force_path=1)}
    assert runs["chunk128"].paths == {"fused", "rows"} and runs["one_pass"].paths == {"fused"}
    assert runs["rows_only"].paths == {"rows"} and runs["rows_chunk128"].paths == {"rows"}
    # the per-token bound from the model's own fp32 logits at the scored rows (the unchanged forward())
    emb = llm.model.embed_tokens
    bound = []
    for b in range(12):
        ids = targets[b].clamp(min=0)
        seq = torch.cat([pd[b], emb(ids[:-1].to(DEV))], 0)
        P = prompts[b].shape[0]
        lg = llm(inputs_embeds=seq[None]).logits[0, P - 1:P - 1 + 25].cpu().numpy()
        bound.append([2 * (tsr.bound_row(lg[j], int(ids[j])) + tsr.bound_partial(lg[j])) for j in range(25)])
    bound = torch.tensor(bound, dtype=torch.float64)
    base = torch.stack([x.double().cpu() for x in runs["one_pass"].token_logprobs])
    flat_ig = torch.zeros(300, dtype=torch.bool)
    flat_ig[ignored] = True
    for name, out in runs.items():
        got = torch.stack([x.double().cpu() for x in out.token_logprobs])
        assert bool((got.view(-1)[flat_ig] == 0).all()), name                              # ignored positions: exactly 0.0
        assert bool((got.view(-1)[~flat_ig] < 0).all()), name
        assert out.n_tokens.tolist() == [25 - int(flat_ig.view(12, 25)[b].sum()) for b in range(12)], name      # ... and uncounted
        d = (got - base).abs()
        print(f"{name}: worst |diff| to the single fused pass / bound {float((d / bound).max()):.3f}")
        assert bool((d <= bound).all()), (name, float((d / bound).max()))
        if out.top1_match is not None:
            assert all(torch.equal(a, b) for a, b in zip(out.top1_match, runs["one_pass"].top1_match)), name
        ssum = torch.stack([x.double().sum() for x in out.token_logprobs]).cpu()
        assert bool(((out.sequence_logprobs.double().cpu() - ssum).abs() <= bound.sum(dim=1)).all()), name


def test_each_sequence_alone_equals_its_rows_in_the_ragged_batch():
    prompts, targets, want, _ = _score_tiny(13)
    llm = _room(_llm())
    tol = 2 * F32_TOL * _logit_rms(prompts)          # what the existing tests allow two kernel families
    batch = llm.score([p.to(DEV) for p in prompts], [targets[b] for b in range(3)])
    for b in range(3):
        alone = llm.score([prompts[b].to(DEV)], [targets[b]])
        d = float((alone.token_logprobs[0].double() - batch.token_logprobs[b].double()).abs().max())
        assert d <= tol, (b, d, tol)
    # a left-padded (B, S, H) tensor with its mask is the same call
    S = max(p.shape[0] for p in prompts)
    x = torch.zeros(3, S, 256)
    mask = torch.zeros(3, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        x[b, S - p.shape[0]:] = p
        mask[b, S - p.shape[0]:] = 1
    padded = llm.score(x.to(DEV), [targets[b] for b in range(3)], attention_mask=mask.to(DEV))
    for b in range(3):
        assert torch.equal(padded.token_logprobs[b], batch.token_logprobs[b])


def test_a_batch_beyond_the_cache_slots_is_split_into_calls():
    prompts, targets, _, _ = _score_tiny(13)
    big = llm = _room(_llm())
    whole = big.score([p.to(DEV) for p in prompts], [targets[b] for b in range(3)])
    small = llama_mod.AudioLlamaForCausalLM(llm.arch, None, torch_dtype=torch.float32, max_ctx=64, max_batch=2)
    small._w, small.device = llm._w, llm.device          # the same device weights, a cache of its own with two slots
    split = small.score([p.to(DEV) for p in prompts], [targets[b] for b in range(3)])
    assert small._kv[0].shape[1] == 2 and split.sequence_logprobs.shape == (3,)
    tol = 2 * F32_TOL * _logit_rms(prompts)
    for b in range(3):
        assert float((split.token_logprobs[b].double() - whole.token_logprobs[b].double()).abs().max()) <= tol


# ------------------------------------------------------------------------------------------------ nothing else moves
def test_generate_keeps_its_ids_and_its_captured_graph_around_a_score_call():
    c = _case("ragged3")
    prompts, targets, _ = _recorded("ragged3")
    llm = _room(_llm())
    _set_eos(llm, [])
    lib = L.lib()
    max_new = _cfg()[3]
    pd = [p.to(DEV) for p in prompts]
    llm.generate(inputs_embeds=pd, max_new_tokens=max_new)                           # sizes generate()'s workspace
    lib.sl_decode_graph_cache_clear()
    ids0 = llm.generate(inputs_embeds=pd, max_new_tokens=max_new)
    assert torch.equal(ids0.cpu(), t(c["ids"]).long())
    ws_ptr, kv_ptr = llm._ws.data_ptr(), llm._kv[0].data_ptr()
    out = llm.score(pd, targets)
    assert llm._ws.data_ptr() == ws_ptr and llm._kv[0].data_ptr() == kv_ptr
    ids1 = llm.generate(inputs_embeds=pd, max_new_tokens=max_new)
    assert torch.equal(ids0, ids1)
    assert lib.sl_decode_graph_cache_clear() == 1                                    # the second call replayed the first one's graph
    assert bool(torch.isfinite(out.sequence_logprobs).all())


def test_a_live_session_is_untouched_by_a_score_call():
    prompts, targets, _ = _recorded("ragged3")
    follow = [torch.randn(4, 256, generator=torch.Generator().manual_seed(600 + b)) * 0.05 for b in range(3)]
    llm = _room(_llm())
    _set_eos(llm, [])
    res = {}
    for with_score in (False, True):
        sess = llm.new_session(3)
        i1 = llm.generate(inputs_embeds=[p.to(DEV) for p in prompts], max_new_tokens=6, past_key_values=sess)
        valid = list(sess.valid_len)
        if with_score:
            llm.score([p.to(DEV) for p in prompts], targets)
            assert sess.valid_len == valid
        i2 = llm.generate(inputs_embeds=[f.to(DEV) for f in follow], max_new_tokens=6, past_key_values=sess)
        res[with_score] = (i1.cpu(), i2.cpu(), list(sess.valid_len))
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1]) and res[False][2] == res[True][2]


# ------------------------------------------------------------------------------------------------ Trainer.validate
# the parent commit's own tree and build on an MI355X, first of two fresh processes (the second: 1041.7122024911778 / 1101.7240161887835)
PARENT_AUDIO_PPL = 1041.712500527472          # 0x1.046d999bcff80p+10
PARENT_TEXT_PPL = 1101.7239111201989          # 0x1.136e548f4e9dcp+10


def _val_trainer(tmp_path, run, **log_extra):
    from types import SimpleNamespace
    from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA
    from test_models_gpu import StubTokenizer, make_encoder, make_llama
    cfgm, ri, utils, trainer_mod = pkg("config"), pkg("random_init"), pkg("utils"), pkg("trainer")
    g, v = golden("pipeline_tiny"), golden("validation_tiny")
    gen = torch.Generator().manual_seed(int(v["gen_seed"]))
    V = TINY_LLAMA.vocab_size
    val_ds = []
    for i, n in enumerate(v["n_samples"]):
        text_ids = torch.randint(1, V, (6 - i % 2,), generator=gen)
        resp_ids = torch.randint(1, V, (7 + i % 3,), generator=gen)
        bos = torch.zeros(1, dtype=torch.long)
        val_ds.append({"audio": {"array": ri.synthetic_waveform(int(n), seed=int(n))}, "text": f"utt{n}", "text_input_ids": torch.cat([bos, text_ids]),
                       "response_input_ids": torch.cat([bos, resp_ids])[None], "pool_ranges_4": []})
    conf = cfgm.from_dict(dict(seed_everything=1234, audio=dict(sampling_rate=16000),
                               model=dict(audio_encoder=dict(base="hubert", type="synthetic", downsample_method="pool", downsample_factor=4,
                                                             pooling=dict(kernel_size=8, stride=4)),
                                          llm_embedding_channels=TINY_LLAMA.hidden_size, llm_type=utils.LLAMA_ID),
                               train=dict(optimizer=dict(lr=5e-5, beta1=0.9, beta2=0.999), batch_size=1, grad_accum_interval=4, epochs=1,
                                          use_ld_loss=True, use_fd_loss=True, ntp_loss_weight=0.5, ld_loss_weight=0.5, fd_loss_weight=1.0,
                                          fd_loss_connector_layers=[0, 1, 3]),
                               log=dict(checkpoint_dir=str(tmp_path / "ckpt"), log_dir=str(tmp_path / "logs"), log_interval=4,
                                        validation_interval=1000, num_generate_samples=0, **log_extra)))
    enc, _ = make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, int(v["enc_seed"]), torch.float32)
    llm, _ = make_llama(TINY_LLAMA, int(v["llm_seed"]), torch.float32)
    tok = StubTokenizer({utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"])})
    return trainer_mod.Trainer(SimpleNamespace(run_name=run, checkpoint_path=None, gpu_idx=0), conf, DEV, tokenizer=tok, llm=llm, audio_encoder=enc,
                               train_dataset=val_ds, val_dataset=val_ds, dtype=torch.float32), v


def test_validate_with_the_key_batches_through_score_and_without_it_is_the_parent(tmp_path):
    """Trainer.validate on the 5-sample fixture of tests/test_train_models_gpu.py (tests/golden/validation_tiny.npz, fp32).

    The parent's figures, recorded by running the parent commit's own tree and build on an MI355X in two fresh processes:
        audio 1041.712500527472 (0x1.046d999bcff80p+10) and 1041.7122024911778 (0x1.046d94b9c1ef4p+10)
        text  1101.7239111201989 (0x1.136e548f4e9dcp+10) and 1101.7240161887835 (0x1.136e5647ff266p+10)
    The parent does not return the same bits twice: forward(labels=) sums a sample's rows into ONE fp32 word with atomicAdd (train_ops.hip
    logit_loss_kernel, one block per row), in arrival order.  Two fresh processes of this tree gave 1041.7124011820315 / 1041.712599872922
    and 1101.723595914504 / 1101.7237009830592, the same spread.  So "without the key = the parent" is asserted in two parts: the loop runs
    exactly the parent's calls (two forward(labels=) per sample, score() never — also tests/test_score_host_cpu.py), and the two values
    equal the recorded ones within what the arrival order can move them: a sample's loss is a sum of r <= 8 terms coef x ce (one rounding
    of the product, r - 1 of the additions, each at most U x the loss), in the recorded run and in this one; ln(perplexity) is the mean
    of the losses, so |ln ppl - ln ppl_parent| <= 2 x 1.01 x U x 8 x the largest sample loss of the fixture (7.28: about 7e-6; the two
    parent runs differ by 3e-7).

    With log.validation_batch_size: 2 (batches of 2, 2 and 1 through llm.score()) the values agree with the parent's within the fp32
    tolerance test_validate_perplexities_match_reference_fixture allows against the reference's values, 1e-4 relative."""
    import math
    tr, v = _val_trainer(tmp_path, "plain")
    calls = []
    tr.llm.score = lambda *a, **k: calls.append("score")
    plain = tr.validate(0)
    assert calls == []
    a0, t0 = plain["validation/audio_perplexity"], plain["validation/text_perplexity"]
    print(f"without the key: audio {a0!r} ({float(a0).hex()}) text {t0!r} ({float(t0).hex()})")
    rows = max(int(s_["response_input_ids"].shape[1]) - 2 for s_ in tr.val_dataset)          # BOS stripped, then logits[-n:-1] against labels[1:]
    assert rows == 8
    arrival = 2 * tsr.HIGHER_ORDER * tsr.U * rows * float(max(v["audio_nll"].max(), v["text_nll"].max()))      # rows - 1 additions + the product by coef
    print(f"|d ln ppl| audio {abs(math.log(a0) - math.log(PARENT_AUDIO_PPL)):.3e} text {abs(math.log(t0) - math.log(PARENT_TEXT_PPL)):.3e} bound {arrival:.3e}")
    assert abs(math.log(a0) - math.log(PARENT_AUDIO_PPL)) <= arrival and abs(math.log(t0) - math.log(PARENT_TEXT_PPL)) <= arrival
    tr2, _ = _val_trainer(tmp_path, "batched", validation_batch_size=2)
    inner = tr2.llm.score
    tr2.llm.score = lambda prompts, targets, **kw: calls.append(len(prompts)) or inner(prompts, targets, **kw)
    batched = tr2.validate(0)
    a1, t1 = batched["validation/audio_perplexity"], batched["validation/text_perplexity"]
    print(f"validation_batch_size=2: audio {a1!r} text {t1!r}")
    assert calls == [2, 2, 2, 2, 1, 1]
    assert abs(a1 - PARENT_AUDIO_PPL) < 1e-4 * PARENT_AUDIO_PPL and abs(t1 - PARENT_TEXT_PPL) < 1e-4 * PARENT_TEXT_PPL
    assert abs(a1 - float(v["audio_perplexity"])) < 1e-4 * float(v["audio_perplexity"])
    assert abs(t1 - float(v["text_perplexity"])) < 1e-4 * float(v["text_perplexity"])


# ------------------------------------------------------------------------------------------------ the inference class
class _ScoreTok:
    """text -> ids by table; strings asked for without special tokens come back as a plain id list, as a tokenizer returns them"""
    bos_token_id = None

    def __init__(self, table):
        self.table = table

    def __call__(self, text, return_tensors=None, add_special_tokens=True):
        from types import SimpleNamespace
        ids = self.table[text]
        return SimpleNamespace(input_ids=ids.clone() if return_tensors == "pt" else ids.reshape(-1).tolist())

    def batch_decode(self, ids, **kw):
        return [" ".join(str(int(i)) for i in row) for row in ids]


def test_score_audio_and_text_responses_build_the_prompts_generation_builds():
    """strings are tokenised without BOS and end with the end-of-turn token; the prompts are generate_audio_responses' / generate_text_response's:
    scoring under them equals llm.score() under the hand-built [prefix | audio | suffix[1:]] within the fp32 tolerance"""
    from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA
    from test_models_gpu import make_encoder, make_llama
    utils, ri, inf_mod = pkg("utils"), pkg("random_init"), pkg("inference")
    g = golden("pipeline_tiny")
    enc, _ = make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, int(g["enc_seed"]), torch.float32)
    llm, _ = make_llama(TINY_LLAMA, int(g["llm_seed"]), torch.float32)
    V = TINY_LLAMA.vocab_size
    ra, rb = torch.tensor([[17 % V, 230 % V, 5 % V, 99 % V]]), torch.tensor([[41 % V, 7 % V]])
    user = torch.tensor([[0, 12 % V, 77 % V, 3 % V]])
    table = {utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"]), "answer a": ra, "answer b": rb}
    inf = inf_mod.LLMSpeechTextInference(enc.config, None, DEV, tokenizer=_ScoreTok(table), llm=llm, audio_encoder=enc, dtype=torch.float32)
    table[f"{inf.prompt_prefix} what{inf.prompt_suffix} "] = user
    e = llm.generation_config.eos_token_id
    eos = list(e) if isinstance(e, (list, tuple)) else ([] if e is None else [e])
    assert eos, "the tiny model names an end-of-turn id"
    want_ids = [ra[0].tolist() + [int(eos[0])], rb[0].tolist() + [int(eos[0])]]
    assert inf._response_ids(["answer a", "answer b"]) == want_ids and inf._response_ids(want_ids) == want_ids
    waves = [ri.synthetic_waveform(int(g["n_samples"]), seed=int(g["wave_seed"])).numpy(), ri.synthetic_waveform(21000, seed=77).numpy()]
    by_text = inf.score_audio_responses(waves, ["answer a", "answer b"], return_top1=True)
    by_ids = inf.score_audio_responses(waves, want_ids)
    assert [int(x.shape[0]) for x in by_text.token_logprobs] == [5, 3] and by_text.n_tokens.tolist() == [5, 3]
    for a, b in zip(by_text.token_logprobs, by_ids.token_logprobs):
        assert torch.equal(a, b)
    emb = llm.model.embed_tokens
    pre, suf = emb(t(g["prefix_ids"]).to(DEV))[0], emb(t(g["suffix_ids"]).to(DEV))[0, 1:]
    prompts = [torch.cat([pre, enc(torch.as_tensor(w)[None].to(DEV))[0], suf], 0) for w in waves]
    rms = float(torch.stack([llm(inputs_embeds=p[None]).logits[0, -1].double() for p in prompts]).pow(2).mean().sqrt())
    hand = llm.score(prompts, [torch.tensor(v) for v in want_ids])
    for a, b in zip(by_text.token_logprobs, hand.token_logprobs):
        assert float((a.double() - b.double()).abs().max()) <= 2 * F32_TOL * rms
    txt = inf.score_text_responses(["what"], ["answer a"])
    hand_t = llm.score([emb(user.to(DEV))[0]], [torch.tensor(want_ids[0])])
    assert torch.equal(txt.token_logprobs[0], hand_t.token_logprobs[0]) and abs(txt.perplexity() - hand_t.perplexity()) == 0.0
