"""GPU: the `stack` and `ctc_pool` downsamples through every layer above the kernels, on the tiny configs of oracle/golden_cfgs.py —
AudioEncoder.encode_packed on ragged batches (sl_hubert_forward_ds), the batched inference entry point, the KD step (EncoderTape head forward
and backward) against autograd through the CPU oracle, and the Trainer loop with a dataset that carries `pool_ranges_4`.  `pool` must stay what
it was: the last test holds a KD window and a generate_audio_responses call to bits recorded on the commit before this feature."""
import hashlib
import json
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN, golden, pkg, rel_err, t
from oracle import hubert_oracle as ho
from oracle import kd_oracle as ko
from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA
from test_models_gpu import BF16_TOL, DEV, F32_TOL, StubTokenizer, make_encoder, make_llama
from test_train_models_gpu import kd_config

pytestmark = pytest.mark.gpu

ri = pkg("random_init")
cfgm = pkg("config")
training = pkg("training")
inf_mod = pkg("inference")
utils = pkg("utils")
L = pkg("_lib")

LENS = (9000, 16720, 24000)                 # T = 27, 52, 74 frames: T % 4 = 3, 0, 2


def frames(n):
    return TINY_HUBERT.num_frames(n)


def ranges_for(T):
    """word-chunk-like ranges of a T-frame utterance: (7, 11) overlaps (9, 14) the way the reference's recipe lets a word's last chunk run into the
    gap range that follows, frames 14 .. 19 are covered by nothing, and the last range ends past T (clamped, as a slice clamps)"""
    return [(0, 3), (3, 7), (7, 11), (9, 14), (20, T - 5), (T - 5, T + 3)]


def oracle_kwargs(method, T):
    return dict(method="stack", factor=4, fix_stack_quirk=True) if method == "stack" else dict(method="ctc_pool", ctc_pool_ranges=[ranges_for(T)])


@pytest.mark.parametrize("dtype,tol", [(torch.float32, F32_TOL), (torch.bfloat16, BF16_TOL), (torch.float16, BF16_TOL)], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("method", ["stack", "ctc_pool"])
def test_encode_packed_ragged_batch_equals_oracle_and_the_one_utterance_forward(method, dtype, tol):
    enc, sd = make_encoder(TINY_HUBERT, 256, 12, dtype, method=method)
    waves = [ri.synthetic_waveform(n, seed=n) for n in LENS]
    T = [frames(n) for n in LENS]
    assert [t_ % 4 for t_ in T] == [3, 0, 2]
    ranges = [ranges_for(t_) for t_ in T] if method == "ctc_pool" else None
    out, P, _, T_got = enc.encode_packed(waves, ctc_pool_ranges=ranges)
    assert T_got == T and P == ([t_ // 4 for t_ in T] if method == "stack" else [6, 6, 6]) and out.shape[0] == sum(P)
    if dtype != torch.float32:      # the same rounded weights on the oracle side (conv0 stays fp32 in the kernel)
        sd = {k: (v if "conv_layers.0." in k else v.to(dtype).float()) for k, v in sd.items()}
    r0 = 0
    for w, p, t_, rng in zip(waves, P, T, ranges or [None] * 3):
        ref = ho.audio_encoder_forward(sd, TINY_HUBERT, w[None], **oracle_kwargs(method, t_))[0]
        assert ref.shape[0] == p and rel_err(out[r0:r0 + p].float().cpu(), ref) < tol, (w.numel(), rel_err(out[r0:r0 + p].float().cpu(), ref))
        alone = enc(w[None].to(DEV), None if rng is None else [rng])[0]            # this build's one-utterance path (host-composed head)
        assert alone.shape[0] == p and rel_err(out[r0:r0 + p].float().cpu(), alone.float().cpu()) < tol
        r0 += p
    # rows land where the caller says (the prompt builder's use), nothing else is written
    buf = torch.full((sum(P) + 7, 256), -1504.0, device=DEV, dtype=dtype)
    offs = [5 + sum(P[1:]), 1, 3 + P[1]]       # utterance 1 first, a hole, utterance 2, a hole, utterance 0
    enc.encode_packed(waves, out=buf, out_row_offsets=offs, ctc_pool_ranges=ranges)
    seen = torch.zeros(buf.shape[0], dtype=torch.bool)
    r0 = 0
    for o, p in zip(offs, P):
        assert torch.equal(buf[o:o + p], out[r0:r0 + p])
        seen[o:o + p] = True
        r0 += p
    assert bool((buf[~seen.to(DEV)] == -1504.0).all())


def test_encode_packed_stack_utterance_shorter_than_one_row_gives_no_rows():
    enc, sd = make_encoder(TINY_HUBERT, 256, 12, torch.float32, method="stack")
    short = ri.synthetic_waveform(1200, seed=1)              # 3 frames: P = 0
    assert frames(1200) == 3
    waves = [ri.synthetic_waveform(9000, seed=9000), short, ri.synthetic_waveform(16720, seed=16720)]
    out, P, _, _ = enc.encode_packed(waves)
    assert P == [6, 0, 13]
    both = enc.encode_packed([waves[0], waves[2]])[0]
    assert rel_err(out.cpu(), both.cpu()) < 1e-6
    out0, P0, _, _ = enc.encode_packed([short])
    assert P0 == [0] and out0.shape[0] == 0


def test_ctc_pool_ranges_are_checked_on_the_host():
    enc, _ = make_encoder(TINY_HUBERT, 256, 13, torch.float32, method="ctc_pool")
    w = ri.synthetic_waveform(16000, seed=3)
    with pytest.raises(L.SpeechLLMError, match=r"utterance 0, range 1 \(60, 70\)"):
        enc.encode_packed([w], ctc_pool_ranges=[[(0, 4), (60, 70)]])
    with pytest.raises(L.SpeechLLMError, match="ctc_pool_ranges"):
        enc.encode_packed([w])
    with pytest.raises(L.SpeechLLMError, match="batch size 1"):          # forward() above one utterance: what it raised before
        enc(torch.stack([w, w]).to(DEV), [[(0, 4)], [(0, 4)]])


@pytest.mark.parametrize("method", ["stack", "ctc_pool"])
def test_generate_audio_responses_batched_ids_equal_per_utterance_calls_fp32(method):
    g = golden("pipeline_tiny")
    cfg = TINY_LLAMA
    enc, _ = make_encoder(TINY_HUBERT, cfg.hidden_size, int(g["enc_seed"]), torch.float32, method=method)
    llm, _ = make_llama(cfg, int(g["llm_seed"]), torch.float32)
    tok = StubTokenizer({utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"]), "EXTRA": t(g["text_prompt_ids"])})
    inf = inf_mod.LLMSpeechTextInference(enc.config, None, DEV, tokenizer=tok, llm=llm, audio_encoder=enc, dtype=torch.float32)
    waves = [ri.synthetic_waveform(n, seed=n).numpy() for n in LENS]
    texts = ["", "EXTRA", ""]
    ranges = [ranges_for(frames(n)) for n in LENS] if method == "ctc_pool" else None
    singles = []
    for i, w in enumerate(waves):
        inf.generate_audio_response(w, additional_text_prompt=texts[i], max_new_tokens=24, ctc_pool_ranges=None if ranges is None else ranges[i])
        singles.append(inf.last_generate_ids.cpu()[0])
    out = inf.generate_audio_responses(waves, texts, max_new_tokens=24, ctc_pool_ranges=ranges)
    ids = inf.last_generate_ids.cpu()
    assert len(out) == 3 and ids.shape[0] == 3
    for row, ref in zip(ids, singles):
        assert torch.equal(row[:ref.shape[0]], ref) and bool((row[ref.shape[0]:] == cfg.pad_token_id).all())
    if method == "ctc_pool":      # without ranges: the reference's AttributeError, on both entry points
        with pytest.raises(AttributeError, match="get_ctc_pool_ranges"):
            inf.generate_audio_responses(waves, texts, max_new_tokens=24)
        with pytest.raises(AttributeError, match="get_ctc_pool_ranges"):
            inf.generate_audio_response(waves[0], max_new_tokens=24)
        with pytest.raises(ValueError):
            inf.generate_audio_responses(waves, texts, max_new_tokens=24, ctc_pool_ranges=ranges[:2])


# ------------------------------------------------------------------------------------------------------------------------------
# KD step
# ------------------------------------------------------------------------------------------------------------------------------
KD_LENS = (16000, 16720)        # T = 49 (T % 4 = 1: one frame cropped by stack) and 52 (T % 4 = 0: every frame kept)


def kd_inputs():
    gen = torch.Generator().manual_seed(91)
    waves = [ri.synthetic_waveform(n, seed=n) for n in KD_LENS]
    texts = [torch.randint(1, TINY_LLAMA.vocab_size, (k,), generator=gen) for k in (9, 6)]
    resps = [torch.randint(1, TINY_LLAMA.vocab_size, (k,), generator=gen) for k in (7, 8)]
    return waves, texts, resps


def kd_build(method, dtype, g):
    enc, enc_sd = make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, int(g["enc_seed"]), dtype, method=method)
    llm, llm_sd = make_llama(TINY_LLAMA, int(g["llm_seed"]), dtype)
    tr = training.KDTrainer(kd_config(taps=(0, 1, 3)), enc, llm, t(g["prefix_ids"]), t(g["suffix_ids"]))
    return tr, enc_sd, llm_sd


def oracle_step(method, g, enc_sd, llm_sd, waves, texts, resps):
    """autograd through the CPU oracle over the two utterances of the micro-batch, each loss divided by the 16 of the accumulation window"""
    sd = {k: v.clone().requires_grad_(k != "encoder.masked_spec_embed") for k, v in enc_sd.items()}
    losses = []
    for w, tx, rs in zip(waves, texts, resps):
        audio = ho.audio_encoder_forward(sd, TINY_HUBERT, w[None], **oracle_kwargs(method, frames(w.numel())))
        l_ = ko.kd_losses(llm_sd, TINY_LLAMA, audio, tx, rs, t(g["prefix_ids"]), t(g["suffix_ids"]), connector_layers=(0, 1, 3))
        (l_["total"] / 16).backward()
        losses.append({k: float(v.detach()) for k, v in l_.items()})
    return sd, losses


@pytest.fixture(scope="module")
def kd_oracle():
    """the oracle's losses and gradients of both methods, computed once and shared by the fp32 and bf16 tests"""
    g = golden("pipeline_tiny")
    waves, texts, resps = kd_inputs()
    out = {}
    for method in ("stack", "ctc_pool"):
        enc_sd = ri.hubert_encoder_state_dict(TINY_HUBERT, TINY_LLAMA.hidden_size, seed=int(g["enc_seed"]), downsample=method)
        llm_sd = ri.llama_state_dict(TINY_LLAMA, seed=int(g["llm_seed"]))
        sd, losses = oracle_step(method, g, enc_sd, llm_sd, waves, texts, resps)
        out[method] = ({k: v.grad for k, v in sd.items() if v.grad is not None}, losses)
    return out


@pytest.mark.parametrize("method", ["stack", "ctc_pool"])
def test_kd_micro_batch_losses_and_every_encoder_gradient_match_oracle_autograd_fp32(kd_oracle, method):
    g = golden("pipeline_tiny")
    waves, texts, resps = kd_inputs()
    tr, enc_sd, _ = kd_build(method, torch.float32, g)
    ranges = [ranges_for(frames(n)) for n in KD_LENS] if method == "ctc_pool" else None
    got = tr.micro_batch(waves, texts, resps, pool_ranges=ranges)
    ref_grads, ref_losses = kd_oracle[method]
    for a, b in zip(got, ref_losses):
        for k, kr in (("ntp_loss", "ntp"), ("ld_loss", "ld"), ("fd_loss", "fd"), ("total", "total")):
            assert abs(a[k] - b[kr]) < 1e-4 * max(1.0, abs(b[kr])), (k, a[k], b[kr])
    grads = training.kernel_grads_to_state_dict(tr.enc, tr.grads, tr.master)
    assert tuple(grads["embed_projection.weight"].shape) == (TINY_LLAMA.hidden_size, TINY_HUBERT.hidden_size * (4 if method == "stack" else 1))
    total = torch.stack([ref_grads[k].norm() for k in tr.trainable]).norm()
    worst = 0.0
    for k in tr.trainable:      # the limits of test_every_encoder_parameter_gradient_matches_oracle_autograd_fp32
        ref = ref_grads[k]
        err = float((grads[k].cpu().reshape(ref.shape).double() - ref.double()).norm())
        bound = 2e-3 * float(ref.norm()) + 1e-6 * float(total)
        worst = max(worst, err / (float(ref.norm()) + 1e-6 * float(total)))
        assert err < bound, (k, err, float(ref.norm()))
    print(method, "worst relative gradient error", worst)


@pytest.mark.parametrize("method", ["stack", "ctc_pool"])
def test_kd_micro_batch_bf16_runs_and_tracks_fp32(kd_oracle, method):
    g = golden("pipeline_tiny")
    waves, texts, resps = kd_inputs()
    tr, _, _ = kd_build(method, torch.bfloat16, g)
    ranges = [ranges_for(frames(n)) for n in KD_LENS] if method == "ctc_pool" else None
    got = tr.micro_batch(waves, texts, resps, pool_ranges=ranges)
    ref_grads, ref_losses = kd_oracle[method]
    for a, b in zip(got, ref_losses):
        for k, kr in (("ntp_loss", "ntp"), ("ld_loss", "ld")):
            assert abs(a[k] - b[kr]) < 3e-2 * abs(b[kr]), (k, a[k], b[kr])
    grads = training.kernel_grads_to_state_dict(tr.enc, tr.grads, tr.master)
    gn, ref = float(grads["embed_projection.weight"].norm()), float(ref_grads["embed_projection.weight"].norm())
    assert abs(gn - ref) < 0.15 * ref, (gn, ref)


def test_kd_refusals_on_the_device_path():
    g = golden("pipeline_tiny")
    waves, texts, resps = kd_inputs()
    tr, _, _ = kd_build("ctc_pool", torch.float32, g)
    with pytest.raises(L.SpeechLLMError, match="micro_batch needs pool_ranges"):
        tr.micro_batch(waves, texts, resps)
    with pytest.raises(L.SpeechLLMError, match=r"utterance 1, range 0 \(52, 60\)"):
        tr.micro_batch(waves, texts, resps, pool_ranges=[[(0, 4)], [(52, 60)]])
    assert tr.micro == 0 and tr.micro_batches == 0          # refused before anything ran
    tr2, _, _ = kd_build("stack", torch.float32, g)
    with pytest.raises(L.SpeechLLMError, match="ctc_pool downsample only"):
        tr2.micro_batch(waves, texts, resps, pool_ranges=[[(0, 4)], [(0, 4)]])


# ------------------------------------------------------------------------------------------------------------------------------
# Trainer
# ------------------------------------------------------------------------------------------------------------------------------
def test_trainer_epoch_with_ctc_pool_ranges_validate_and_checkpoint_roundtrip(tmp_path):
    trainer_mod = pkg("trainer")
    g = golden("pipeline_tiny")
    gen = torch.Generator().manual_seed(5)
    V = TINY_LLAMA.vocab_size

    def row(n, nt, nr):      # the reference's preprocessed-row schema (tests/hf_dirs.py write_kd_dataset), pool_ranges_4 filled for this utterance
        return {"audio": {"array": ri.synthetic_waveform(n, seed=n)}, "text": f"utt{n}",
                "text_input_ids": torch.cat([torch.zeros(1, dtype=torch.long), torch.randint(1, V, (nt,), generator=gen)]),
                "response_input_ids": torch.cat([torch.zeros(1, dtype=torch.long), torch.randint(1, V, (nr,), generator=gen)])[None],
                "pool_ranges_4": torch.tensor(ranges_for(frames(n)))}

    train_ds = [row(16000 + 1000 * i, 5 + i % 3, 6 + i % 4) for i in range(8)]
    val_ds = [row(20000, 6, 7), row(24000, 4, 5)]
    conf = cfgm.from_dict(dict(seed_everything=1234, audio=dict(sampling_rate=16000),
                               model=dict(audio_encoder=dict(base="hubert", type="synthetic", downsample_method="ctc_pool", downsample_factor=4,
                                                             pooling=dict(kernel_size=8, stride=4)),
                                          llm_embedding_channels=TINY_LLAMA.hidden_size, llm_type=utils.LLAMA_ID),
                               train=dict(optimizer=dict(lr=5e-5, beta1=0.9, beta2=0.999), batch_size=1, grad_accum_interval=4, epochs=1,
                                          use_ld_loss=True, use_fd_loss=True, ntp_loss_weight=0.5, ld_loss_weight=0.5, fd_loss_weight=1.0,
                                          fd_loss_connector_layers=[0, 1, 3]),
                               log=dict(checkpoint_dir=str(tmp_path / "ckpt"), log_dir=str(tmp_path / "logs"), log_interval=4,
                                        validation_interval=1000, num_generate_samples=1)))
    tok = StubTokenizer({utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"])})
    llm, _ = make_llama(TINY_LLAMA, 52, torch.float32)

    def trainer(name, ckpt=None):
        enc, _ = make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, 51, torch.float32, method="ctc_pool")
        args = SimpleNamespace(run_name=name, checkpoint_path=ckpt, gpu_idx=0, no_regularizers=True)
        return trainer_mod.Trainer(args, conf, DEV, tokenizer=tok, llm=llm, audio_encoder=enc, train_dataset=train_ds, val_dataset=val_ds, dtype=torch.float32)

    tr = trainer("t")
    calls = []
    inner = tr.kd.micro_batch

    def recording(waves, text_ids, resp_ids, **kw):
        losses = inner(waves, text_ids, resp_ids, **kw)
        calls.append((waves, text_ids, resp_ids, kw, losses))
        return losses

    tr.kd.micro_batch = recording
    tr.train()
    assert tr.step == 8 and len(calls) == 2
    for _, _, _, kw, losses in calls:
        assert kw["pool_ranges"] is not None and len(kw["pool_ranges"]) == 4
        assert all(all(abs(v) < 1e4 and v == v for v in l_.values()) for l_ in losses), losses          # finite
    lines = [json.loads(l_) for l_ in open(tmp_path / "logs" / "t" / "metrics.jsonl")]
    val = [l_ for l_ in lines if "validation/audio_perplexity" in l_]
    assert val and all(0 < l_["validation/audio_perplexity"] < float("inf") for l_ in val)
    # the first window against a direct KDTrainer.micro_batch call on the same initial weights with the same ranges
    enc0, _ = make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, 51, torch.float32, method="ctc_pool")
    kd = training.KDTrainer(conf, enc0, llm, tr.prefix_ids, tr.suffix_ids, total_optimizer_steps=2)
    waves, text_ids, resp_ids, kw, losses = calls[0]
    direct = kd.micro_batch(waves, text_ids, resp_ids, pool_ranges=kw["pool_ranges"])
    # (equal up to the last bits: two runs of one KD window do not give bit-identical loss sums, with any downsample method)
    assert len(direct) == len(losses) == 4
    for a, b in zip(direct, losses):
        assert all(abs(a[k] - b[k]) <= 1e-5 * abs(b[k]) for k in b), (a, b)
    # checkpoint round trip: bit-identical masters
    ck_path = tmp_path / "ckpt" / "t" / "epoch_0_step_8.pt"
    tr2 = trainer("t2", str(ck_path))
    assert tr2.step == 8 and set(tr2.kd.master) == set(tr.kd.master)
    for k, v in tr.kd.master.items():
        assert torch.equal(tr2.kd.master[k], v), k


# ------------------------------------------------------------------------------------------------------------------------------
# pool stays bit for bit what it was
# ------------------------------------------------------------------------------------------------------------------------------
def sha(*tensors):
    h = hashlib.sha256()
    for x in tensors:
        h.update(x.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def pool_bits():
    """The `pool` encoder of a KD window — the tape's forward (the audio embeddings the LLM gets) and the head's backward (the gradient handed to the
    layer stack, and the projection's and the final LayerNorm's parameter gradients) for a fixed upstream gradient, fp32 and bf16 — and a `pool`
    generate_audio_responses call (ids and packed audio embeddings), hashed.  The KD window as a whole is not hashed: two runs of it differ in the
    last bits of the loss sums and of some gradients, on the commit before this feature as well."""
    g = golden("pipeline_tiny")
    waves, texts, resps = kd_inputs()
    out = {}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        tr, _, _ = kd_build("pool", dtype, g)
        audio, tape = tr.enc_tape.forward(waves)
        d_out = torch.randn(audio.shape, generator=torch.Generator().manual_seed(3)).to(DEV, dtype)
        dx = tr.enc_tape._head_backward(tape, d_out, tr.grads, lambda names: None)
        torch.cuda.synchronize()
        out[f"kd_forward_{name}"] = sha(audio)
        out[f"kd_head_backward_{name}"] = sha(dx, *[tr.grads[k] for k in ("proj_w", "proj_b", "final_ln_g", "final_ln_b")])
        losses = tr.micro_batch(waves, texts, resps)                      # the whole window still runs
        assert all(v == v for l_ in losses for v in l_.values())
    enc, _ = make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, int(g["enc_seed"]), torch.float32)
    llm, _ = make_llama(TINY_LLAMA, int(g["llm_seed"]), torch.float32)
    tok = StubTokenizer({utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"]), "EXTRA": t(g["text_prompt_ids"])})
    inf = inf_mod.LLMSpeechTextInference(enc.config, None, DEV, tokenizer=tok, llm=llm, audio_encoder=enc, dtype=torch.float32)
    inf.generate_audio_responses([ri.synthetic_waveform(n, seed=n).numpy() for n in LENS], ["", "EXTRA", ""], max_new_tokens=24)
    out["generate_fp32"] = sha(inf.last_generate_ids, enc.encode_packed([ri.synthetic_waveform(n, seed=n) for n in LENS])[0])
    return out


def test_pool_kd_window_and_batched_generate_give_the_bits_of_the_parent_commit():
    """tests/golden/downsample_pool_bits.json was recorded by running pool_bits() on the commit before the stack / ctc_pool feature, in a process
    of its own — and that is how it is compared: what a process ran before (tuning switches reloaded, cached plans and transposed weights) moves
    the last bits of the fp32 head backward, so inside the suite's process the hashes are not those of a fresh start.  Three fresh runs gave the
    same hashes on the parent commit and on this one."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import json, sys; sys.path.insert(0, '.'); import conftest, test_downsample_models_gpu as m; print('BITS ' + json.dumps(m.pool_bits()))"
    r = subprocess.run([sys.executable, "-c", code], cwd=here, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(next(l_ for l_ in r.stdout.splitlines() if l_.startswith("BITS "))[5:])
    want = json.load(open(os.path.join(GOLDEN, "downsample_pool_bits.json")))
    assert got == want
