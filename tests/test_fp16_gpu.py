"""GPU: the fp16 compute mode (SL_F16: fp16 storage, fp32 accumulate, norms and softmax statistics in fp32) — the reference's
torch_dtype=float16 regime (ref:inference.py:47-51).

Kernel level: every GEMM family (skinny packed, streaming packed split / unsplit, streaming wide, tiled 256, 128 ring), attention,
decode attention, norms, RoPE, silu_mul, the conv feature extractor and pooling against fp64 math on the SAME fp16-rounded inputs.
An op with one output rounding must land within 5e-4 relative L2: fp16 output rounding alone is ~1.4e-4 rms, bf16 ~1.1e-3, so a
stage that still rounds through bf16 fails.  The shapes here are aligned and the data N(0, 1): one pass per family.  The edge
shapes of every form (ragged M / N, 1-3 K slabs, odd N, lda > K, ring stages, split-K / stream-K, fix-up, RoPE / KV, 64-key
chunks, split + merge), per element, with exact integer data, fp16 overflow / subnormals, guard bands and poisoned padding, are
in tests/test_kernel_edges_gpu.py.  Model level: the tiny fixtures of test_models_gpu.py at BF16_TOL / 4, and the full
depth run against the reference's own fp16-autocast outputs.
"""
import os

import pytest
import torch

from conftest import golden, pkg, rel_err, t
from oracle import hubert_oracle as ho
from oracle import llama_oracle as lo
from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA, TINY_MHA, WIDE_HUBERT, WIDE_LLAMA

pytestmark = pytest.mark.gpu

ops = pkg("ops")
L = pkg("_lib")
ri = pkg("random_init")
cfgm = pkg("config")
enc_mod = pkg("audio_encoder")
llama_mod = pkg("audio_llama")
weights = pkg("weights")
utils = pkg("utils")

DEV = "cuda:0"
F16 = torch.float16
ONE_ROUNDING = 5e-4          # ops with a single fp16 output rounding
BF16_TOL = 3e-2              # test_models_gpu.py's bf16 tolerance
MODEL_TOL = BF16_TOL / 4
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(*shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def h16(x):
    """an fp16 device tensor and its exact fp64 value"""
    x16 = x.to(DEV, F16).contiguous()
    return x16, x16.double()


def silu_mul_ref(y):
    """gate / up in 16-row blocks of W: [16 gate | 16 up] per 32 output rows"""
    M, N2 = y.shape
    y = y.view(M, N2 // 32, 2, 16)
    g, u = y[:, :, 0], y[:, :, 1]
    return (g * torch.sigmoid(g) * u).reshape(M, N2 // 2)


def gelu_ref(y):
    return 0.5 * y * (1.0 + torch.erf(y / 2 ** 0.5))


# ------------------------------------------------------------------------------------------------------------------------------
# GEMM families
# ------------------------------------------------------------------------------------------------------------------------------
ACTS = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "silu_mul": L.ACT_SILU_MUL}


def _ref_act(y, act):
    if act == "gelu":
        return gelu_ref(y)
    if act == "silu_mul":
        return silu_mul_ref(y)
    return y


@pytest.mark.parametrize("M,N,K", [(4096, 1024, 1024), (634, 1024, 1024), (200, 512, 512)])     # tiled 256, 128 ring, two-stage tiled
@pytest.mark.parametrize("act", list(ACTS))
def test_fp16_gemm_rowmajor_families(M, N, K, act):
    a, a64 = h16(rnd(M, K, seed=1))
    w, w64 = h16(rnd(N, K, seed=2, std=K ** -0.5))
    b, b64 = h16(rnd(N, seed=3, std=0.1))
    ref = _ref_act(a64 @ w64.T + b64, act)
    res = None
    if act == "none":
        res, r64 = h16(rnd(M, N, seed=4))
        ref = ref + r64
    out = ops.gemm(a, w, bias=b, residual=res, act=ACTS[act])
    assert out.dtype == F16
    assert rel_err(out, ref) < ONE_ROUNDING


@pytest.mark.parametrize("M", [8, 26, 128, 512, 1024])       # skinny packed, streaming packed (128-row blocks), streaming wide
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("act", ["none", "silu_mul"])
def test_fp16_gemm_packed_families(M, split, act):
    K, N = 3072, 5120
    a, a64 = h16(rnd(M, K, seed=5))
    w, w64 = h16(rnd(N, K, seed=6, std=K ** -0.5))
    ref = _ref_act(a64 @ w64.T, act)
    wp = ops.pack_weight(w)
    res = None
    if act == "none":
        res, r64 = h16(rnd(M, N, seed=7))
        ref = ref + r64
    out = ops.gemm_decode(a, wp, N, residual=res, act=ACTS[act], split_k=split)
    assert out.dtype == F16
    assert rel_err(out, ref) < ONE_ROUNDING


def test_fp16_gemm_out_f32_and_fused_argmax():
    M, N, K = 300, 4000, 1024
    a, a64 = h16(rnd(M, K, seed=8))
    w, w64 = h16(rnd(N, K, seed=9, std=K ** -0.5))
    ref = a64 @ w64.T
    out = ops.gemm(a, w, out_f32=True)
    assert out.dtype == torch.float32
    assert rel_err(out, ref) < 1e-5                   # no output rounding: fp32 accumulation only
    val, idx = ops.gemm_top1(a, w)
    best = val.argmax(0)
    top = idx.gather(0, best[None])[0].long()
    assert torch.equal(top.cpu(), ref.argmax(1).cpu())
    assert rel_err(val.max(0).values, ref.max(1).values) < 1e-5


def test_fp16_layernorm_fold_epilogue_wide_encoder():
    """The encoder's LayerNorm-folded products (sl_hubert_fold + the rows epilogue with ln_* / stats_out) run in fp16: a HuBERT-large
    width encoder builds the folded weights and lands within MODEL_TOL of the oracle on the same fp16-rounded weights."""
    g = golden("enc_wide_pool_32000")
    wave = ri.synthetic_waveform(32000, seed=int(g["wave_seed"]))
    enc, sd = _make_encoder(WIDE_HUBERT, 3072, int(g["weight_seed"]), F16)
    out = enc.encode_packed([wave])[0].float().cpu()
    assert getattr(enc.weights, "_fold_t", None) is not None, "fp16 must take the LayerNorm-folded products"
    assert rel_err(out, _hubert_ref(sd, WIDE_HUBERT, wave)) < MODEL_TOL


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, causal, scale):
    """q (nh, S, D), k / v (nkv, S, D) fp64"""
    rep = q.shape[0] // k.shape[0]
    k = k.repeat_interleave(rep, 0)
    v = v.repeat_interleave(rep, 0)
    s = (q @ k.transpose(1, 2)) * scale
    if causal:
        n = q.shape[1]
        s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool, device=s.device), 1), float("-inf"))
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("D,nh,nkv,causal", [(128, 8, 2, True), (64, 4, 4, False)])
def test_fp16_attention_prefill_ragged(D, nh, nkv, causal):
    lens = [37, 300, 129]
    T = sum(lens)
    qkv, q64 = h16(rnd(T, (nh + 2 * nkv) * D, seed=10))
    out = ops.attn_packed_qkv(qkv, lens, nh, nkv, D, causal, D ** -0.5)
    assert out.dtype == F16
    o0 = 0
    for n in lens:
        x = q64[o0:o0 + n]
        q = x[:, :nh * D].view(n, nh, D).transpose(0, 1)
        k = x[:, nh * D:(nh + nkv) * D].view(n, nkv, D).transpose(0, 1)
        v = x[:, (nh + nkv) * D:].view(n, nkv, D).transpose(0, 1)
        ref = _attn_ref(q, k, v, causal, D ** -0.5).transpose(0, 1).reshape(n, nh * D)
        # two roundings: the probabilities enter P.V as fp16 (as the bf16 mode rounds them to bf16), then the output
        assert rel_err(out[o0:o0 + n], ref) < 8e-4, n
        o0 += n


@pytest.mark.parametrize("B,form", [(4, "split"), (20, "full"), (20, "split")])
def test_fp16_decode_attention_split_and_single_pass(B, form):
    nh, nkv, D, max_ctx = 6, 2, 128, 448
    lens = [(1, 64, 65, 393, 200)[b % 5] for b in range(B)]
    kc, k64 = h16(rnd(B, nkv, max_ctx, D, seed=11))
    vc, v64 = h16(rnd(B, nkv, max_ctx, D, seed=12))
    qd, q64 = h16(rnd(B, nh * D, seed=13))
    ctx = torch.tensor(lens, dtype=torch.int32, device=DEV)
    if form == "split":
        out = ops.attn_decode_split(qd, qd.stride(0), kc, vc, ctx, nh, nkv, D, max_ctx, D ** -0.5)
    else:
        out = ops.attn_decode(qd, qd.stride(0), kc, vc, ctx, nh, nkv, D, max_ctx, D ** -0.5)   # B * n_kv >= 32: single-pass form
    assert out.dtype == F16
    for s, n in enumerate(lens):
        ref = _attn_ref(q64[s].view(nh, 1, D), k64[s, :, :n], v64[s, :, :n], False, D ** -0.5).reshape(nh * D)
        assert rel_err(out[s], ref) < 8e-4, (s, n)


# ------------------------------------------------------------------------------------------------------------------------------
# norms, RoPE, silu_mul, conv feature extractor, pooling
# ------------------------------------------------------------------------------------------------------------------------------
def test_fp16_rmsnorm_layernorm_gelu_rope_silu_mul():
    x, x64 = h16(rnd(300, 1024, seed=14))
    w, w64 = h16(1 + rnd(1024, seed=15, std=0.1))
    y = ops.rmsnorm(x, w, 1e-5)
    ref = w64 * (x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + 1e-5))
    assert y.dtype == F16 and rel_err(y, ref) < ONE_ROUNDING
    b, b64 = h16(rnd(1024, seed=16, std=0.1))
    for gelu in (False, True):
        y = ops.layernorm(x, w, b, 1e-5, gelu=gelu)
        ref = torch.nn.functional.layer_norm(x64, (1024,), w64, b64, 1e-5)
        ref = gelu_ref(ref) if gelu else ref
        assert y.dtype == F16 and rel_err(y, ref) < ONE_ROUNDING, gelu
    gu, gu64 = h16(rnd(300, 2048, seed=17))
    y = ops.silu_mul(gu)
    assert y.dtype == F16 and rel_err(y, silu_mul_ref(gu64)) < ONE_ROUNDING
    # RoPE in place on 4 of 6 heads (the Llama tables)
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=6, num_key_value_heads=2, head_dim=128)
    cos, sin = [t_.to(DEV) for t_ in weights.rope_tables(arch, 64)]
    n, heads, n_rot, D = 40, 6, 4, 128
    xr, xr64 = h16(rnd(n, heads * D, seed=18))
    pos = torch.tensor([(5 * i + 1) % 64 for i in range(n)], dtype=torch.int32, device=DEV)
    ops.rope_inplace(xr, pos, cos, sin, heads, n_rot, D)
    v = xr64.view(n, heads, D).clone()
    c, s_ = cos.double()[pos.long()][:, None], sin.double()[pos.long()][:, None]
    a1, a2 = v[:, :n_rot, :D // 2].clone(), v[:, :n_rot, D // 2:].clone()
    v[:, :n_rot, :D // 2] = a1 * c - a2 * s_
    v[:, :n_rot, D // 2:] = a2 * c + a1 * s_
    assert rel_err(xr, v.reshape(n, heads * D)) < ONE_ROUNDING


def test_fp16_conv_feature_extractor_and_pooling():
    """HuBERT conv0 (fp32 waveform and weights, GroupNorm-style LayerNorm + GELU, fp16 output) and average pooling in fp16."""
    k, stride, C = 10, 5, 512
    wave = rnd(16000, seed=19).to(DEV)
    w = rnd(C, k, seed=20, std=k ** -0.5).to(DEV)
    bias = rnd(C, seed=21, std=0.1).to(DEV)
    gamma = (1 + rnd(C, seed=22, std=0.1)).to(DEV)
    beta = rnd(C, seed=23, std=0.1).to(DEV)
    y = ops.hubert_conv0(wave, w, bias, gamma, beta, F16, k=k, stride=stride)
    assert y.dtype == F16
    y32 = ops.hubert_conv0(wave, w, bias, gamma, beta, torch.float32, k=k, stride=stride)
    assert rel_err(y, y32.double()) < ONE_ROUNDING
    x, x64 = h16(rnd(203, 256, seed=24))
    p = ops.avgpool_rows(x, 8, 4)
    ref = torch.nn.functional.avg_pool1d(x64.T[None], 8, 4)[0].T
    assert p.dtype == F16 and rel_err(p, ref) < ONE_ROUNDING


# ------------------------------------------------------------------------------------------------------------------------------
# tiny fixtures (test_models_gpu.py's), BF16_TOL / 4
# ------------------------------------------------------------------------------------------------------------------------------
def _hubert_arch(c):
    return weights.HubertArch(c.conv_dim, c.conv_kernel, c.conv_stride, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                              c.intermediate_size, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, c.layer_norm_eps)


def _llama_arch(c):
    return weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                             c.intermediate_size, c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling, c.tie_word_embeddings,
                             tuple(c.eos_token_ids), c.pad_token_id)


def _make_encoder(c, llm_dim, seed, dtype):
    conf = cfgm.from_dict(dict(model=dict(audio_encoder=dict(base="hubert", type="synthetic", downsample_method="pool", downsample_factor=4,
                                                             pooling=dict(kernel_size=8, stride=4)),
                                          llm_embedding_channels=llm_dim, llm_type=utils.LLAMA_ID)))
    enc = enc_mod.AudioEncoder(conf, DEV, dtype=dtype, arch=_hubert_arch(c))
    sd = ri.hubert_encoder_state_dict(c, llm_dim, seed=seed)
    enc.load_state_dict(sd)
    return enc.eval().to(DEV), sd


def _make_llama(c, seed, dtype, max_ctx=256):
    sd = ri.llama_state_dict(c, seed=seed)
    return llama_mod.AudioLlamaForCausalLM(_llama_arch(c), dict(sd), torch_dtype=dtype, device=DEV, max_ctx=max_ctx), sd


def _hubert_ref(sd, c, wave):
    """the oracle on the fp16-rounded weights (conv0 stays fp32 in the kernel)"""
    sdq = {k: (v if "conv_layers.0." in k else v.to(F16).float()) for k, v in sd.items()}
    return ho.audio_encoder_forward(sdq, c, wave[None])[0]


@pytest.mark.parametrize("n", [16000, 32000])
def test_fp16_encoder_tiny_vs_reference_fixture(n):
    g = golden(f"enc_tiny_pool_{n}")
    enc, _ = _make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, int(g["weight_seed"]), F16)
    wave = ri.synthetic_waveform(n, seed=int(g["wave_seed"]))
    out = enc(wave[None].to(DEV))
    assert out.dtype == F16
    assert rel_err(out.float().cpu(), t(g["audio_embeds"])) < MODEL_TOL


def test_fp16_whisper_tiny_vs_reference_fixture():
    from oracle.golden_cfgs import TINY_WHISPER as WC
    g = golden("whisper_tiny")
    conf = cfgm.from_dict(dict(model=dict(audio_encoder=dict(base="whisper", type="synthetic", downsample_method="pool", downsample_factor=4,
                                                             pooling=dict(kernel_size=8, stride=4)),
                                          llm_embedding_channels=256, llm_type=utils.LLAMA_ID)))
    arch = weights.WhisperArch(WC.d_model, WC.encoder_layers, WC.encoder_attention_heads, WC.encoder_ffn_dim, WC.num_mel_bins, WC.max_source_positions)
    enc = enc_mod.AudioEncoder(conf, DEV, dtype=F16, arch=arch)
    enc.load_state_dict(ri.whisper_encoder_state_dict(WC, 256, seed=int(g["weight_seed"]))).eval().to(DEV)
    waves = [ri.synthetic_waveform(int(n), seed=int(s)).numpy() for n, s in zip(g["n_samples"], g["wave_seeds"])]
    feats = enc.feature_extractor(waves, return_tensors="pt", sampling_rate=16000).input_features
    out = enc(feats)
    assert out.dtype == F16
    assert rel_err(out.float().cpu(), t(g["audio_embeds"])) < MODEL_TOL


def test_fp16_llama_wide_forward_hidden_states_and_logits():
    g = golden("llama_wide")
    cfg = WIDE_LLAMA
    llm, sd = _make_llama(cfg, int(g["weight_seed"]), F16)
    gen = torch.Generator().manual_seed(int(g["embeds_seed"]))
    x = torch.randn(1, int(g["S"]), cfg.hidden_size, generator=gen) * 0.02
    out = llm(inputs_embeds=x.to(DEV), output_hidden_states=True)
    assert out.hidden_states[-1].dtype == F16 and out.logits.dtype == torch.float32
    sdq = {k: v.to(F16).float() for k, v in sd.items()}
    ref = lo.llama_forward(sdq, cfg, x.to(F16).float(), output_hidden_states=True)
    assert rel_err(torch.stack(out.hidden_states).float().cpu(), torch.stack(ref["hidden_states"])) < MODEL_TOL
    assert rel_err(out.logits[:, -1].cpu(), ref["logits"][:, -1]) < MODEL_TOL


@pytest.mark.parametrize("name,cfg", [("tiny_gqa", TINY_LLAMA), ("tiny_mha", TINY_MHA)])
def test_fp16_llama_tiny_forward_loss_and_ids_vs_reference_fixture(name, cfg):
    """logits, hidden states, the list-label loss (sl_ce_loss behind the fp32 logits) and greedy ids against the fp32 fixture"""
    g = golden(f"llama_{name}")
    llm, _ = _make_llama(cfg, int(g["weight_seed"]), F16)
    gen = torch.Generator().manual_seed(int(g["embeds_seed"]))
    x = (torch.randn(1, int(g["S"]), cfg.hidden_size, generator=gen) * 0.05).to(DEV)
    out = llm(inputs_embeds=x, output_hidden_states=True)
    assert out.logits.dtype == torch.float32 and out.hidden_states[0].dtype == F16
    assert rel_err(out.logits.cpu(), t(g["logits"])) < MODEL_TOL
    assert rel_err(torch.stack(out.hidden_states).float().cpu(), t(g["hidden_states"])) < MODEL_TOL
    labels = [t(g["labels"]).to(DEV)]
    loss = llm(inputs_embeds=x, labels=labels).loss
    assert abs(float(loss) - float(g["loss"])) < MODEL_TOL * max(1.0, abs(float(g["loss"])))
    llm.generation_config.eos_token_id = None
    assert torch.equal(llm.generate(inputs_embeds=x, max_new_tokens=32).cpu(), t(g["ids_noeos"]))


def test_fp16_generate_audio_response_pipeline_tiny_ids():
    from test_models_gpu import StubTokenizer
    inf_mod = pkg("inference")
    g = golden("pipeline_tiny")
    enc, _ = _make_encoder(TINY_HUBERT, TINY_LLAMA.hidden_size, int(g["enc_seed"]), F16)
    llm, _ = _make_llama(TINY_LLAMA, int(g["llm_seed"]), F16)
    tok = StubTokenizer({utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"]), "EXTRA": t(g["text_prompt_ids"])})
    inf = inf_mod.LLMSpeechTextInference(enc.config, None, DEV, tokenizer=tok, llm=llm, audio_encoder=enc, dtype=F16)
    wave = ri.synthetic_waveform(int(g["n_samples"]), seed=int(g["wave_seed"])).numpy()
    inf.generate_audio_response(wave, max_new_tokens=40)
    assert torch.equal(inf.last_generate_ids.cpu(), t(g["ids_audio"]))
    inf.generate_audio_response(wave, additional_text_prompt="EXTRA", max_new_tokens=40)
    assert torch.equal(inf.last_generate_ids.cpu(), t(g["ids_text_audio"]))


# ------------------------------------------------------------------------------------------------------------------------------
# generation: compaction, decode-step families, coexistence with a bf16 model
# ------------------------------------------------------------------------------------------------------------------------------
def test_fp16_compacted_generation_equals_uncompacted():
    """sl_generate in fp16, 300 rows with mixed token budgets: the compacting run gives the ids of the run without compaction"""
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 31, F16)
    gen = torch.Generator().manual_seed(6)
    base = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in (9, 21, 14, 5, 30)]
    llm.generation_config.eos_token_id = list(cfg.eos_token_ids)
    B, new = 300, 48
    limits = [3 + (11 * b) % 44 for b in range(B)]
    prompts = [base[b % 5] for b in range(B)]
    lens = [int(p.shape[0]) for p in prompts]
    x = torch.cat(prompts).to(DEV, F16)
    ids_c, n_c = llm.generate_packed(x.clone(), lens, new, use_eos=True, row_limits=limits, compact=True, check_every=4)
    assert llm.last_generate_stats["compactions"] >= 1
    ids_u, n_u = llm.generate_packed(x.clone(), lens, new, use_eos=True, row_limits=limits, compact=False, check_every=4)
    assert n_c == n_u and torch.equal(ids_c[:, :n_c].cpu(), ids_u[:, :n_u].cpu())


def test_fp16_decode_step_large_batch_matches_small_batch():
    from test_models_gpu import _decode_step_logits
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 33, F16)
    gen = torch.Generator().manual_seed(8)
    base = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in (9, 150, 14, 5, 77)]
    nxt = [11, 222, 3, 444, 55]
    small = _decode_step_logits(llm, base, nxt)
    B = 520
    big = _decode_step_logits(llm, [base[b % 5] for b in range(B)], [nxt[b % 5] for b in range(B)])
    for b in range(B):
        assert rel_err(big[b], small[b % 5]) < MODEL_TOL, b


def test_fp16_and_bf16_models_coexist_bf16_bits_unchanged():
    """A bf16 and an fp16 model in one process: the bf16 model's greedy ids and logits are bit-equal before and after the fp16
    model has captured and replayed its decode graph (the graph cache is keyed by dtype)."""
    cfg = TINY_LLAMA
    gen = torch.Generator().manual_seed(50)
    x = torch.randn(1, 30, cfg.hidden_size, generator=gen) * 0.05
    bf, _ = _make_llama(cfg, 51, torch.bfloat16)
    h1, _ = _make_llama(cfg, 51, F16)
    bf.generation_config.eos_token_id = None
    h1.generation_config.eos_token_id = None
    ids0 = bf.generate(inputs_embeds=x.to(DEV, torch.bfloat16), max_new_tokens=16).cpu()
    lg0 = bf(inputs_embeds=x.to(DEV, torch.bfloat16)).logits.cpu()
    for _ in range(2):      # capture, then replay
        ids16 = h1.generate(inputs_embeds=x.to(DEV, F16), max_new_tokens=16).cpu()
    ids1 = bf.generate(inputs_embeds=x.to(DEV, torch.bfloat16), max_new_tokens=16).cpu()
    lg1 = bf(inputs_embeds=x.to(DEV, torch.bfloat16)).logits.cpu()
    assert torch.equal(ids0, ids1) and torch.equal(lg0, lg1)
    assert ids16.shape == ids0.shape


# ------------------------------------------------------------------------------------------------------------------------------
# full depth: HuBERT-large 24 L -> Llama-3.2-3B 28 L against the reference's fp16-autocast outputs
# ------------------------------------------------------------------------------------------------------------------------------
def test_fp16_path_distance_to_the_references_fp16_autocast_regime_full_depth():
    import numpy as np
    h = np.load(os.path.join(REPO, "tests", "golden", "fp16_autocast_full.npz"))
    g = np.load(os.path.join(REPO, "tests", "golden", "full_depth_llama32.npz"))
    harch, larch = weights.KNOWN_HUBERT["facebook/hubert-large-ls960-ft"], weights.KNOWN_LLAMA[utils.LLAMA_ID]
    conf = cfgm.load_config(os.path.join(REPO, "config", "llama3_hubert.yaml"))
    enc_sd = ri.hubert_encoder_state_dict(harch, larch.hidden_size, seed=int(h["enc_seed"]))
    sd = ri.llama_state_dict(larch, seed=int(h["llm_seed"]))
    wave = ri.synthetic_waveform(int(h["n_samples"]), seed=int(h["wave_seed"]))
    a16, l16 = torch.from_numpy(h["audio_embeds_rows"]), torch.from_numpy(h["first_logits_every16"])
    prefix, suffix = torch.from_numpy(g["prefix_ids"]), torch.from_numpy(g["suffix_ids"])
    n_ids = int(g["ids"].shape[1])
    d, firsts, ids = {}, {}, {}
    for dt in (F16, torch.bfloat16):
        enc = enc_mod.AudioEncoder(conf, DEV, dtype=dt, arch=harch)
        enc.load_state_dict(enc_sd).eval().to(DEV)
        llm = llama_mod.AudioLlamaForCausalLM(larch, dict(sd), torch_dtype=dt, device=DEV, max_ctx=256, max_batch=1)
        audio = enc(wave[None].to(DEV))
        emb = llm.model.embed_tokens
        x = torch.cat([emb(prefix.to(DEV))[0], audio[0], emb(suffix.to(DEV))[0, 1:]])[None]
        first = llm(inputs_embeds=x).logits[0, -1].float().cpu()
        if dt == F16:
            llm.generation_config.eos_token_id = None
            ids[dt] = llm.generate(inputs_embeds=x, max_new_tokens=n_ids).cpu()[0]
            assert bool(torch.isfinite(audio.float()).all()) and bool(torch.isfinite(first).all())
        rows = audio[0, ::8, ::4].float().cpu()
        d[dt] = (rel_err(rows, a16), rel_err(first[::16], l16))
        firsts[dt] = first
        del enc, llm, audio, x
        torch.cuda.empty_cache()
    print(f"fp16 path vs fp16-autocast reference: audio {d[F16][0]:.3e}, first-step logits {d[F16][1]:.3e}")
    print(f"bf16 path vs fp16-autocast reference: audio {d[torch.bfloat16][0]:.3e}, first-step logits {d[torch.bfloat16][1]:.3e}")
    assert d[F16][0] < 4e-3 and d[F16][1] < 1.5e-2, d
    assert d[F16][0] < 0.4 * d[torch.bfloat16][0] and d[F16][1] < 0.4 * d[torch.bfloat16][1], d
    assert int(firsts[F16].argmax()) == int(h["argmax"]) == int(g["ids"][0, 0])
    # greedy ids against the fp32 reference on every margin-qualified step (the rule of test_fullsize_gpu._check_ids_against_reference)
    ref_ids, margins = torch.from_numpy(g["ids"])[0], torch.from_numpy(g["margins"])[0]
    top_idx, top_val = torch.from_numpy(g["first_logits_top16_idx"]), torch.from_numpy(g["first_logits_top16"])
    l32 = torch.from_numpy(g["first_logits_every16"])
    gap = max(float((firsts[F16][::16] - l32).abs().max()), float((firsts[F16][top_idx] - top_val).abs().max()))
    qualified = 0
    for k in range(ref_ids.shape[0]):
        if float(margins[k]) <= 50 * gap:
            break
        assert int(ids[F16][k]) == int(ref_ids[k]), (k, ids[F16].tolist(), ref_ids.tolist())
        qualified += 1
    same = int((ids[F16][:ref_ids.shape[0]] == ref_ids).to(torch.int64).cumprod(0).sum())
    print(f"fp16 greedy ids identical to the fp32 reference on {qualified} margin-qualified steps (gap {gap:.2e}); "
          f"leading ids equal: {same} of {ref_ids.shape[0]}")
