"""GPU: the opt-in fp8 (OCP e4m3fn, unscaled) K/V cache — kv_cache_dtype="fp8", sl_kv_cache.reserved = SL_KV_FP8_E4M3.

The format is defined so that the write path is testable exactly: a row is quantised from the value already rounded to the model
dtype, so the fp8 cache holds q8(what the 16-bit cache would hold), with q8(x) = x.clamp(-448, 448).to(torch.float8_e4m3fn) on the
CPU (round to nearest even, never 0x7F / 0xFF).  Reading a byte back into bf16 / fp16 is exact, so the decode attention on e4m3
rows is checked with the edge suite's own bounds (tests/test_kernel_edges_gpu.py: attn_bounds on the dequantised rows in fp64, the
tolerances of the dtype) and nothing wider.  Model level: the cache after a real prefill + decode step, the decode-step logits
against the CPU oracle fed the dequantised cache, and the invariances that hold inside fp8 mode (shared prefix, compaction, a decode
graph captured for the other format is never replayed).
"""
import ctypes as C

import pytest
import torch

from conftest import pkg, rel_err
from oracle import llama_oracle as lo
from oracle.golden_cfgs import TINY_LLAMA
from test_kernel_edges_gpu import BIG, DEV, FILL, _rope_perm, _set, attn_bounds, check_attn, gauss, operand, tuning, vec  # noqa: F401 (tuning: fixture)

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
weights = pkg("weights")
ri = pkg("random_init")
llama_mod = pkg("audio_llama")

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT16 = [F16, BF16]
F8 = torch.float8_e4m3fn
FILL8 = 0x5A                     # cache sentinel byte (a finite e4m3 value)
BF16_TOL = 3e-2                  # tests/test_models_gpu.py
TOL16 = {BF16: BF16_TOL, F16: BF16_TOL / 4}     # tests/test_fp16_gpu.py: BF16_TOL / 4 for fp16


def q8(x):
    """the test's own reference quantiser: CPU tensor (any float dtype) -> e4m3 bytes"""
    return x.detach().cpu().clamp(-448, 448).to(F8).view(torch.uint8)


def dq8(b):
    """e4m3 bytes -> fp64 on the CPU (exact)"""
    return b.detach().cpu().contiguous().view(F8).double()


def no_nan_bytes(b):
    return not bool(((b & 0x7F) == 0x7F).any())


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the quantiser, byte for byte
# ------------------------------------------------------------------------------------------------------------------------------
def _quantiser_rows():
    """rows of 128 values: every finite e4m3 value, every midpoint between neighbours (both signs), +-0, the subnormal range down
    to 2^-10 (half the smallest subnormal: a tie with zero) and values beyond +-448"""
    fin = torch.tensor([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=torch.uint8).view(F8).double()      # 254 values
    pos = fin[fin >= 0].sort().values
    mid = (pos[1:] + pos[:-1]) / 2
    sub = torch.tensor([2.0 ** -10, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -7, 7.5 * 2.0 ** -9, 2.0 ** -6,
                        0.9 * 2.0 ** -10, 1.1 * 2.0 ** -10, 2.0 ** -12, 2.0 ** -20], dtype=torch.float64)
    big = torch.tensor([449.0, 464.0, 1000.0, 60000.0, 448.0, 447.0, 432.0, 440.0], dtype=torch.float64)
    vals = torch.cat([fin, mid, -mid, torch.tensor([0.0, -0.0], dtype=torch.float64), sub, -sub, big, -big])
    n = (vals.numel() + 127) // 128 * 128
    return torch.cat([vals, torch.zeros(n - vals.numel(), dtype=torch.float64)]).view(-1, 128)


@pytest.mark.parametrize("dt", DT16)
def test_rope_kv_append_ex_quantises_byte_for_byte(dt):
    """sl_rope_kv_append_ex, format 1: V heads are not rotated, so their bytes are known exactly (q8 of the 16-bit value); K bytes
    are q8 of the rows the format-0 call leaves in a 16-bit cache, those rotated rows are also written back into qkv, q has the
    bits of the format-0 call, and nothing outside the written positions changes."""
    nh, nkv, D, max_ctx, slots = 6, 2, 128, 40, 3
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=nh, num_key_value_heads=nkv, head_dim=D)
    cos, sin = [t_.to(DEV) for t_ in weights.rope_tables(arch, max_ctx)]
    vrows = _quantiser_rows()                              # (R, 128); two V heads per token
    n_tok = (vrows.shape[0] + nkv - 1) // nkv
    vfull = torch.zeros(n_tok * nkv, D, dtype=torch.float64)
    vfull[:vrows.shape[0]] = vrows
    qkv64 = gauss((n_tok, (nh + 2 * nkv) * D), 900, 3.0)   # std 3: K values reach past the subnormal / normal boundary both ways
    qkv64[:, (nh + nkv) * D:] = vfull.view(n_tok, nkv * D)
    qkv0 = qkv64.float().to(dt).to(DEV)
    seq = torch.tensor([i % slots for i in range(n_tok)], dtype=torch.int32, device=DEV)
    pos = torch.tensor([(3 * (i // slots) + 1) % max_ctx for i in range(n_tok)], dtype=torch.int32, device=DEV)
    assert len({(int(s), int(p)) for s, p in zip(seq.cpu(), pos.cpu())}) == n_tok
    # format 0 through the old entry and through the new one: the same bits
    a = qkv0.clone()
    kc16 = torch.full((slots, nkv, max_ctx, D), FILL, device=DEV, dtype=dt)
    vc16 = torch.full_like(kc16, FILL)
    ops.rope_kv_append(a, kc16, vc16, seq, pos, cos, sin, nh, nkv, D, max_ctx)
    b = qkv0.clone()
    kcb, vcb = torch.full_like(kc16, FILL), torch.full_like(kc16, FILL)
    ops.rope_kv_append_ex(b, kcb, vcb, seq, pos, cos, sin, nh, nkv, D, max_ctx, L.KV_MODEL_DTYPE)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(kcb.view(torch.int16), kc16.view(torch.int16))
    assert torch.equal(vcb.view(torch.int16), vc16.view(torch.int16))
    # format 1
    c = qkv0.clone()
    kc8 = torch.full((slots, nkv, max_ctx, D), FILL8, device=DEV, dtype=torch.uint8)
    vc8 = torch.full_like(kc8, FILL8)
    ops.rope_kv_append_ex(c, kc8, vc8, seq, pos, cos, sin, nh, nkv, D, max_ctx, L.KV_FP8_E4M3)
    torch.cuda.synchronize()
    s_, p_ = seq.long().cpu(), pos.long().cpu()
    got_v = vc8.cpu()[s_, :, p_]                           # (n_tok, nkv, D)
    want_v = q8(qkv0.cpu()[:, (nh + nkv) * D:].view(n_tok, nkv, D))
    assert torch.equal(got_v, want_v), f"V bytes: {int((got_v != want_v).sum())} differ, first at {tuple((got_v != want_v).nonzero()[0].tolist())}"
    got_k = kc8.cpu()[s_, :, p_]
    k16 = kc16.cpu()[s_, :, p_]
    assert torch.equal(got_k, q8(k16)), f"K bytes: {int((got_k != q8(k16)).sum())} differ from q8(16-bit cache)"
    assert no_nan_bytes(kc8.cpu()) and no_nan_bytes(vc8.cpu())
    cq = c.cpu().view(n_tok, nh + 2 * nkv, D)
    assert torch.equal(cq[:, :nh].contiguous().view(torch.int16), a.cpu().view(n_tok, nh + 2 * nkv, D)[:, :nh].contiguous().view(torch.int16)), "q"
    assert torch.equal(cq[:, nh:nh + nkv].contiguous().view(torch.int16), k16.contiguous().view(torch.int16)), "rotated K rows in qkv"
    assert torch.equal(cq[:, nh + nkv:].contiguous().view(torch.int16), qkv0.cpu().view(n_tok, nh + 2 * nkv, D)[:, nh + nkv:].contiguous().view(torch.int16)), "V in qkv"
    for cache in (kc8, vc8):
        chk = cache.cpu().clone()
        chk[s_, :, p_] = FILL8
        assert bool((chk == FILL8).all()), "cache written outside (tok_seq, tok_pos)"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the fused decode write (ACT_ROPE_KV epilogue of the skinny, streaming and wide blocks)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 17, 130, 385, 700])
def test_gemm_rope_kv_epilogue_writes_q8_of_the_16bit_cache(dt, M):
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=6, num_key_value_heads=2, head_dim=128,
                             rope_scaling=dict(factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192))
    nh, nkv, D, H, max_ctx = 6, 2, 128, 256, 64
    N = (nh + 2 * nkv) * D
    cos, sin = [t_.to(DEV) for t_ in weights.rope_tables(arch, max_ctx)]
    x, _ = operand(gauss((M, H), 910), dt)
    w, _ = vec(gauss((N, H), 911, 4.0 * H ** -0.5), dt)        # outputs of std ~4: bytes across the whole e4m3 range
    wp = ops.pack_weight(w[_rope_perm(nh, nkv).to(DEV)].contiguous())
    seq = torch.arange(M, dtype=torch.int32, device=DEV)
    pos = torch.tensor([(7 * i + 3) % max_ctx for i in range(M)], dtype=torch.int32, device=DEV)
    rope = dict(cos=cos, sin=sin, pos=pos, seq=seq, n_heads=nh, n_kv=nkv, max_ctx=max_ctx)
    kc16 = torch.full((M, nkv, max_ctx, D), FILL, device=DEV, dtype=dt)
    vc16 = torch.full_like(kc16, FILL)
    q16 = ops.gemm_decode(x, wp, N, act=L.ACT_ROPE_KV, rope=dict(rope, k_cache=kc16, v_cache=vc16, kv_format=L.KV_MODEL_DTYPE))
    kc8 = torch.full((M, nkv, max_ctx, D), FILL8, device=DEV, dtype=torch.uint8)
    vc8 = torch.full_like(kc8, FILL8)
    q8_ = ops.gemm_decode(x, wp, N, act=L.ACT_ROPE_KV, rope=dict(rope, k_cache=kc8, v_cache=vc8, kv_format=L.KV_FP8_E4M3))
    torch.cuda.synchronize()
    assert torch.equal(q8_.view(torch.int16), q16.view(torch.int16)), "q differs between the two cache formats"
    rows, p_ = torch.arange(M), pos.long().cpu()
    for name, c8, c16 in (("K", kc8, kc16), ("V", vc8, vc16)):
        got, want = c8.cpu()[rows, :, p_], q8(c16.cpu()[rows, :, p_])
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} bytes differ from q8(16-bit cache)"
        assert len(torch.unique(got)) > 60, "the data does not exercise the format"
        chk = c8.cpu().clone()
        chk[rows, :, p_] = FILL8
        assert bool((chk == FILL8).all()), f"{name} cache written outside (tok_seq, tok_pos)"
        assert no_nan_bytes(c8.cpu())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. decode attention on e4m3 rows
# ------------------------------------------------------------------------------------------------------------------------------
CTX = [1, 63, 64, 65, 127, 128, 129, 393, 448]
FORMS8 = {
    "single_pass_128": dict(SL_ATTN_FULL_MIN="1"),
    "split_combine": dict(SL_ATTN_FORCE_SPLIT="1", SL_ATTN_SPLIT_MERGE="0"),
    "split_merge": dict(SL_ATTN_FORCE_SPLIT="1", SL_ATTN_SPLIT_MERGE="1"),
}
_ATTN_DATA = {}


def _attn_data(nh, nkv, shared_prefix):
    """e4m3 caches (bytes) shared by the dtypes and forms: Gaussian K, Gaussian and one-hot-probe V; behind every context, and below
    shared_prefix in every slot but 0, the largest finite bytes (0x7E / 0xFE)"""
    key = (nh, nkv, shared_prefix)
    if key not in _ATTN_DATA:
        D, max_ctx, B = 128, 448, len(CTX)
        k8 = q8(gauss((B, nkv, max_ctx, D), 921).float())
        vg8 = q8(gauss((B, nkv, max_ctx, D), 922).float())
        vp = torch.zeros(B, nkv, max_ctx, D)
        j = torch.arange(max_ctx)
        vp[:, :, j, j % D] = 1.0
        vp8 = q8(vp)
        poison = torch.tensor([0x7E, 0xFE], dtype=torch.uint8).repeat(D // 2)
        true_rows = {}
        for name, c in (("k", k8), ("vg", vg8), ("vp", vp8)):
            for s, n in enumerate(CTX):
                c[s, :, (max(n, shared_prefix) if s == 0 else n):] = poison      # slot 0 keeps real rows at every prefix position
            true_rows[name] = c.clone()                       # what a sequence attends, before the prefix rows are poisoned
            if shared_prefix:
                for s in range(B):
                    true_rows[name][s, :, :shared_prefix] = c[0, :, :shared_prefix]
                c[1:, :, :shared_prefix] = poison
        _ATTN_DATA[key] = (k8, vg8, vp8, true_rows)
    return _ATTN_DATA[key]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("form", list(FORMS8))
@pytest.mark.parametrize("nh,nkv", [(6, 2), (4, 1)])
@pytest.mark.parametrize("shared_prefix", [0, 9])
def test_attention_decode_on_fp8_rows(dt, form, nh, nkv, shared_prefix, tuning):
    """sl_attn_decode_split_ex, format 1, in the three forms.  Reference: attn_bounds on the exactly dequantised rows in fp64 with the
    dtype's existing tolerance (fp8 -> T, the only new step, is exact).  With shared_prefix = 9 slot 0 holds the true prefix rows,
    every other slot holds poison there, and the reference uses slot 0's rows.  A context shorter than the prefix (1) attends slot
    0's row as well: that is the promise the caller made."""
    _set(tuning, FORMS8[form])
    D, max_ctx, B = 128, 448, len(CTX)
    scale = D ** -0.5
    k8, vg8, vp8, true_rows = _attn_data(nh, nkv, shared_prefix)
    q, q64 = operand(gauss((B, nh * D), 920), dt)
    kc = k8.to(DEV)
    ctx = torch.tensor(CTX, dtype=torch.int32, device=DEV)
    k64 = dq8(true_rows["k"])
    for cls, v8, vtrue in (("P", vp8, true_rows["vp"]), ("G", vg8, true_rows["vg"])):
        vc = v8.to(DEV)
        v64 = dq8(vtrue)
        obuf = torch.full((B + 2, nh * D), FILL, device=DEV, dtype=dt)
        out = obuf[1:B + 1]
        ops.attn_decode_split_ex(q, q.stride(0), kc, vc, ctx, nh, nkv, D, max_ctx, scale, L.KV_FP8_E4M3, shared_prefix, out=out)
        assert bool((obuf[0] == FILL).all()) and bool((obuf[B + 1] == FILL).all())
        for s, n in enumerate(CTX):
            ref, tol, zero = attn_bounds(q64[s].view(nh, 1, D), k64[s, :, :n], v64[s, :, :n], torch.ones(1, n, dtype=torch.bool), scale, dt)
            check_attn(out[s:s + 1], ref, tol, zero, dt, f"{cls} context {n}")


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("form", ["split_combine", "split_merge"])
def test_attention_decode_on_fp8_rows_128_key_splits(dt, form, tuning):
    """The split forms take 128-key blocks from 512 (sequence, kv head) pairs up: 256 sequences x 2 kv heads with the split forced
    reach attn_decode_split_kernel<T, REP, 128, uint8_t>, which the 9-sequence cases above (64-key blocks) do not.  Same data rules:
    contexts cycle through CTX, finite poison behind every context and, below shared_prefix = 9, in every slot but 0."""
    _set(tuning, FORMS8[form])
    nh, nkv, D, max_ctx, B, P = 6, 2, 128, 448, 256, 9
    scale = D ** -0.5
    ctxs = [CTX[s % len(CTX)] for s in range(B)]
    ctxs[0] = 448                                      # slot 0 holds real rows at every prefix position
    k8 = q8(gauss((B, nkv, max_ctx, D), 941).float())
    v8 = q8(gauss((B, nkv, max_ctx, D), 942).float())
    poison = torch.tensor([0x7E, 0xFE], dtype=torch.uint8).repeat(D // 2)
    true_k, true_v = k8.clone(), v8.clone()
    for c, tr in ((k8, true_k), (v8, true_v)):
        for s, n in enumerate(ctxs):
            c[s, :, n:] = poison
        tr[:, :, :P] = c[0, :, :P]
        c[1:, :, :P] = poison
    q, q64 = operand(gauss((B, nh * D), 940), dt)
    ctx = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    obuf = torch.full((B + 2, nh * D), FILL, device=DEV, dtype=dt)
    out = obuf[1:B + 1]
    ops.attn_decode_split_ex(q, q.stride(0), k8.to(DEV), v8.to(DEV), ctx, nh, nkv, D, max_ctx, scale, L.KV_FP8_E4M3, P, out=out)
    assert bool((obuf[0] == FILL).all()) and bool((obuf[B + 1] == FILL).all())
    k64, v64 = dq8(true_k), dq8(true_v)
    for s, n in enumerate(ctxs):
        ref, tol, zero = attn_bounds(q64[s].view(nh, 1, D), k64[s, :, :n], v64[s, :, :n], torch.ones(1, n, dtype=torch.bool), scale, dt)
        check_attn(out[s:s + 1], ref, tol, zero, dt, f"sequence {s} context {n}")


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("form", list(FORMS8))
def test_attention_decode_ex_format0_has_the_bits_of_the_old_entry(dt, form, tuning):
    _set(tuning, FORMS8[form])
    nh, nkv, D, max_ctx, B = 6, 2, 128, 448, len(CTX)
    q, _ = operand(gauss((B, nh * D), 930), dt)
    kc, _ = vec(gauss((B, nkv, max_ctx, D), 931), dt)
    vc, _ = vec(gauss((B, nkv, max_ctx, D), 932), dt)
    ctx = torch.tensor(CTX, dtype=torch.int32, device=DEV)
    a = ops.attn_decode_split(q, q.stride(0), kc, vc, ctx, nh, nkv, D, max_ctx, D ** -0.5)
    b = ops.attn_decode_split_ex(q, q.stride(0), kc, vc, ctx, nh, nkv, D, max_ctx, D ** -0.5, L.KV_MODEL_DTYPE, 0)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------
# 4-6. model level (TINY_LLAMA: 3 layers, D = 128, REP = 2)
# ------------------------------------------------------------------------------------------------------------------------------
def _llama_arch(c):
    return weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                             c.intermediate_size, c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling,
                             c.tie_word_embeddings, tuple(c.eos_token_ids), c.pad_token_id)


def _make_llama(c, seed, dtype, kv_cache_dtype=None, max_ctx=256):
    sd = ri.llama_state_dict(c, seed=seed)
    return llama_mod.AudioLlamaForCausalLM(_llama_arch(c), dict(sd), torch_dtype=dtype, device=DEV, max_ctx=max_ctx, kv_cache_dtype=kv_cache_dtype), sd


def _prefill_and_step(llm, prompts, next_ids, shared_prefix=0):
    """prefill + ONE decode step through the C ABI -> (prefill logits, cache after prefill (k, v), decode logits, cache after the step)"""
    w, lib, B = llm._dev(), L.lib(), len(prompts)
    x = torch.cat([p.to(DEV, llm.dtype) for p in prompts]).contiguous()
    cu = [0]
    for p in prompts:
        cu.append(cu[-1] + p.shape[0])
    kv = llm._kv_cache(B, shared_prefix)
    llm._kv[0].zero_(); llm._kv[1].zero_()
    ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(w.struct), x.shape[0], B, 1))
    logits = torch.empty((B, llm.arch.vocab_size), device=DEV, dtype=torch.float32)
    ctx = torch.empty(B, device=DEV, dtype=torch.int32)
    L.check(lib.sl_llama_prefill(C.byref(w.struct), C.byref(kv), x.data_ptr(), (C.c_int32 * (B + 1))(*cu), B, logits.data_ptr(), ctx.data_ptr(),
                                 None, ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
    pre_logits = logits.cpu()
    pre_cache = (llm._kv[0][:, :B].cpu(), llm._kv[1][:, :B].cpu())
    nid = torch.tensor(next_ids, dtype=torch.int32, device=DEV)
    L.check(lib.sl_llama_decode_step(C.byref(w.struct), C.byref(kv), nid.data_ptr(), ctx.data_ptr(), B, logits.data_ptr(), ws.data_ptr(),
                                     ws.numel(), L.stream_ptr()), "sl_llama_decode_step")
    return pre_logits, pre_cache, logits.cpu(), (llm._kv[0][:, :B].cpu(), llm._kv[1][:, :B].cpu())


_BASE_LENS = (9, 150, 14, 5, 77)
_NEXT = [11, 222, 3, 444, 55]


def _batch(cfg, B):
    gen = torch.Generator().manual_seed(8)
    base = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in _BASE_LENS]
    return base, [base[b % 5] for b in range(B)], [_NEXT[b % 5] for b in range(B)]


@pytest.mark.parametrize("B", [5, 520])
def test_fp8_cache_after_prefill_and_decode_step_is_q8_of_the_16bit_cache(B):
    """The same prompts with the 16-bit cache and with fp8 (bf16): the fp8 cache equals q8(16-bit cache) at every prompt position of
    every layer and at the decode-appended position of layer 0 (deeper layers attend quantised keys and legitimately differ); the
    prefill logits are bit-identical, because the fp8-mode prefill attends the unquantised rows."""
    cfg = TINY_LLAMA
    _, prompts, nxt = _batch(cfg, B)
    llm16, _ = _make_llama(cfg, 33, BF16)
    pl16, pc16, _, dc16 = _prefill_and_step(llm16, prompts, nxt)
    del llm16
    llm8, _ = _make_llama(cfg, 33, BF16, kv_cache_dtype="fp8")
    assert llm8._kv is None
    pl8, pc8, _, dc8 = _prefill_and_step(llm8, prompts, nxt)
    assert llm8._kv[0].dtype == torch.uint8 and llm8._kv[0].numel() == cfg.num_hidden_layers * B * cfg.num_key_value_heads * 256 * cfg.head_dim
    assert torch.equal(pl8.view(torch.int32), pl16.view(torch.int32)), "prefill logits differ between the cache formats"
    for which in (0, 1):
        want = q8(pc16[which][:, :, :, :max(_BASE_LENS)].float())       # prompt positions only (the longest prompt has 150)
        for b in range(B):
            n = prompts[b].shape[0]
            assert torch.equal(pc8[which][:, b, :, :n], want[:, b, :, :n]), (which, b)
            assert bool((pc8[which][:, b, :, n:] == 0).all()), "cache written behind the prompt"
            assert torch.equal(dc8[which][0, b, :, n], q8(dc16[which][0, b, :, n].float())), ("decode-appended row of layer 0", which, b)
            assert bool((dc8[which][:, b, :, n + 1:] == 0).all())
            assert torch.equal(dc8[which][:, b, :, :n], pc8[which][:, b, :, :n]), "the decode step rewrote prompt rows"
        assert no_nan_bytes(dc8[which])


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("B", [5, 520])
def test_fp8_decode_step_logits_against_the_oracle_on_the_dequantised_cache(dt, B):
    """Reference: the CPU oracle's next-token logits with `past` = the fp8 cache read back after prefill and dequantised (its own new
    row stays unquantised).  rel_err < TOL16 + d8, with d8 computed per sequence from the oracle alone: the distance between its
    logits with its exact past and with q8 of that past — quantising the one new row among n + 1 keys cannot cost more than
    quantising all of them."""
    cfg = TINY_LLAMA
    base, prompts, nxt = _batch(cfg, B)
    llm, sd = _make_llama(cfg, 33, dt, kv_cache_dtype="fp8")
    _, pc8, logits, _ = _prefill_and_step(llm, prompts, nxt)
    sdq = {k: v.to(dt).float() for k, v in sd.items()}
    embed = sdq["model.embed_tokens.weight"]
    d8, exact = [], []
    for s in range(5):
        out = lo.llama_forward(sdq, cfg, base[s].to(dt).float()[None], last_logits_only=True)
        tok = embed[_NEXT[s]][None, None]
        a = lo.llama_forward(sdq, cfg, tok, past=out["past"], last_logits_only=True)["logits"][0, -1]
        pq = [(dq8(q8(k)).float(), dq8(q8(v)).float()) for k, v in out["past"]]
        bq = lo.llama_forward(sdq, cfg, tok, past=pq, last_logits_only=True)["logits"][0, -1]
        d8.append(rel_err(bq, a))
        exact.append(a)
    refs = {}
    worst = 0.0
    for b in range(B):
        s, n = b % 5, prompts[b].shape[0]
        kb, vb = pc8[0][:, b, :, :n].contiguous(), pc8[1][:, b, :, :n].contiguous()
        key = (s, kb.numpy().tobytes(), vb.numpy().tobytes())
        if key not in refs:
            past = [(dq8(kb[l]).float()[None], dq8(vb[l]).float()[None]) for l in range(cfg.num_hidden_layers)]
            refs[key] = lo.llama_forward(sdq, cfg, embed[_NEXT[s]][None, None], past=past, last_logits_only=True)["logits"][0, -1]
        e = rel_err(logits[b], refs[key])
        worst = max(worst, e / (TOL16[dt] + d8[s]))
        assert e < TOL16[dt] + d8[s], (b, e, TOL16[dt], d8[s])
    print(f"fp8 decode step, {dt}, B={B}: d8 per sequence {['%.2e' % d for d in d8]}, worst err / bound {worst:.3f}, {len(refs)} distinct caches")


def _prefix_batch(cfg, B, P, seed=12):
    gen = torch.Generator().manual_seed(seed)
    pre = torch.randn(P, cfg.hidden_size, generator=gen) * 0.05
    tails = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in (9, 140, 14, 5, 77, 30, 21, 1)]
    prompts = [torch.cat([pre, tails[b % len(tails)] * (1.0 + 0.01 * (b // len(tails)))]) for b in range(B)]
    return prompts, [int(p.shape[0]) for p in prompts]


def test_fp8_shared_prefix_leaves_ids_and_cache_unchanged():
    """inside fp8 mode: shared_prefix = P against 0 — ids and the whole cache bit-identical (40 sequences, bf16)"""
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, kv_cache_dtype=torch.float8_e4m3fn)
    P, B = 11, 40
    prompts, lens = _prefix_batch(cfg, B, P)
    x = torch.cat(prompts).to(DEV, BF16)
    ids0, n0 = llm.generate_packed(x.clone(), lens, 24, use_eos=False)
    assert llm._kv[0].dtype == torch.uint8
    k0, v0 = llm._kv[0].clone(), llm._kv[1].clone()
    for c in (k0, v0):
        assert torch.equal(c[:, :B, :, :P], c[:, :1, :, :P].expand(-1, B, -1, -1, -1)), "prefix rows differ between slots"
    llm._kv[0].zero_(); llm._kv[1].zero_()
    ids1, n1 = llm.generate_packed(x.clone(), lens, 24, use_eos=False, shared_prefix=P)
    assert n0 == n1 and torch.equal(ids0, ids1)
    assert torch.equal(llm._kv[0], k0) and torch.equal(llm._kv[1], v0)


def test_fp8_compaction_moves_128_byte_rows():
    """inside fp8 mode: compact=True against compact=False with mixed row limits — ids identical per sequence (kv_move on rows of 128
    bytes, under the family pin)"""
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, kv_cache_dtype="fp8")
    B, new = 40, 40
    prompts, lens = _prefix_batch(cfg, B, 11)
    x = torch.cat(prompts).to(DEV, BF16)
    limits = [2 + (7 * b) % 37 for b in range(B)]
    limits[0] = 2
    llm.generation_config.eos_token_id = None
    ref, n_ref = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=False)
    ids, n = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=True, check_every=2)
    assert llm.last_generate_stats["compactions"] >= 3
    assert n == n_ref and torch.equal(ids[:, :n], ref[:, :n_ref])


def test_fp8_decode_graph_is_not_replayed_on_a_16bit_cache():
    """The decode-graph key carries the K/V format.  Both formats are run on the SAME storage: one byte buffer per cache, viewed as
    e4m3 rows (its first half) and as bf16 rows (all of it), so model, cache pointers, workspace, batch and every other key field are
    equal and only the format differs.  After the fp8 generation has captured its graph, the 16-bit generation must give the ids of
    a fresh 16-bit instance; replaying the fp8 graph would read and write bytes in bf16 buffers.  And back again."""
    cfg = TINY_LLAMA
    B, new, max_ctx = 40, 16, 256
    prompts, lens = _prefix_batch(cfg, B, 11)
    x = torch.cat(prompts).to(DEV, BF16)
    fresh, _ = _make_llama(cfg, 35, BF16, max_ctx=max_ctx)
    want, n_want = fresh.generate_packed(x.clone(), lens, new, use_eos=False)
    del fresh
    shape = (cfg.num_hidden_layers, B, cfg.num_key_value_heads, max_ctx, cfg.head_dim)
    n = 1
    for d in shape:
        n *= d
    store = [torch.zeros(2 * n, dtype=torch.uint8, device=DEV) for _ in range(2)]
    as8 = tuple(s_[:n].view(shape) for s_ in store)
    as16 = tuple(s_.view(BF16).view(shape) for s_ in store)
    assert as8[0].data_ptr() == as16[0].data_ptr() and as8[1].data_ptr() == as16[1].data_ptr()
    llm, _ = _make_llama(cfg, 35, BF16, kv_cache_dtype="fp8", max_ctx=max_ctx)
    llm._kv = as8
    ids8, _ = llm.generate_packed(x.clone(), lens, new, use_eos=False)
    ws_ptr = llm._ws.data_ptr()
    assert llm._kv[0].data_ptr() == store[0].data_ptr()
    llm.set_kv_cache_dtype(None)
    assert llm._kv is None
    llm._kv = as16
    ids16, n16 = llm.generate_packed(x.clone(), lens, new, use_eos=False)
    assert llm._kv[0].data_ptr() == store[0].data_ptr() and llm._kv[0].dtype == BF16 and llm._ws.data_ptr() == ws_ptr
    assert n16 == n_want and torch.equal(ids16, want)
    llm.set_kv_cache_dtype("fp8")
    llm._kv = as8
    again, _ = llm.generate_packed(x.clone(), lens, new, use_eos=False)
    assert torch.equal(again, ids8)


def test_fp8_cache_with_a_float32_model_raises():
    cfg = TINY_LLAMA
    with pytest.raises(L.SpeechLLMError):
        _make_llama(cfg, 35, F32, kv_cache_dtype="fp8")
    llm, _ = _make_llama(cfg, 35, F32)
    with pytest.raises(L.SpeechLLMError):
        llm.set_kv_cache_dtype("fp8")
    with pytest.raises(L.SpeechLLMError):
        _make_llama(cfg, 35, BF16, kv_cache_dtype="int8")
