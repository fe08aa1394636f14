"""GPU: the opt-in fp8 (e4m3) decode weights — w_layout = SL_W_PACKED_E4M3, sl_llama_model.reserved = SL_WDEC_E4M3, weight_dtype="fp8".

The format is exact in both directions that matter: the packer is held byte for byte against the format's definition written in torch
(tests/test_w8_host_cpu.py), and a byte converts to bf16 / fp16 without rounding.  So the kernel owes what the 16-bit packed kernel
owes against a reference built from the same values — q(A) @ dq(bytes)^T * s in fp64 — and is held to the 16-bit kernel's bounds:
TOL = 1.5e-2 in bf16 (tests/test_kernels_gpu.py) and 5e-4 in fp16 (tests/test_fp16_gpu.py ONE_ROUNDING, the bound of the packed
products there), 2e-5 with fp32 outputs.  Weight rows are scaled by 2^(n % 9 - 4), gate / up rows and the two rotate_half halves
of a head differ by 2^4, so a scale taken from the wrong row — or not applied — misses by orders of magnitude.  Outputs are views
into sentinel-filled buffers and the caches are sentinel-filled.  Model level: TINY_LLAMA against the CPU oracle run on
e4m3_dequantised_state_dict(), with the bounds tests/test_models_gpu.py gives the 16-bit step.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import pkg, rel_err
from oracle import llama_oracle as lo
from oracle.golden_cfgs import TINY_LLAMA
from test_kernel_edges_gpu import DEV, FILL, _rope_perm, gauss, guarded, untouched
from test_w8_host_cpu import ref_image, split_image, weight_rows

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
weights = pkg("weights")
ri = pkg("random_init")
llama_mod = pkg("audio_llama")

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT16 = [BF16, F16]
F8 = torch.float8_e4m3fn
TOL = {BF16: 1.5e-2, F16: 5e-4}          # tests/test_kernels_gpu.py TOL[bf16]; tests/test_fp16_gpu.py ONE_ROUNDING (its packed products)
TOL_F32_OUT = 2e-5
BF16_TOL = 3e-2                          # tests/test_models_gpu.py
TOL16 = {BF16: BF16_TOL, F16: BF16_TOL / 4}
FILL8 = 0x5A
E4 = L.W_PACKED_E4M3


def q8(x):
    return x.detach().cpu().clamp(-448, 448).to(F8).view(torch.uint8)


def quantise(w):
    """the test's own CPU quantisation of a (N, K) weight in its dtype: (fp64 dequantised bytes (N, K), fp64 scales (N,))"""
    _, s, nat = ref_image(w.cpu())
    n = w.shape[0]
    return nat[:n].view(F8).double(), s[:n].double()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the device packer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("N,K", [(16, 64), (40, 192), (1000, 256)])
def test_device_packer_equals_the_host_entry(dt, N, K):
    w = weight_rows(N, K, dt)
    host = ops.pack_weight_e4m3(w)
    dev_img = ops.pack_weight_e4m3(w.to(DEV))
    assert torch.equal(dev_img.cpu(), host), "device packer differs from sl_pack_weight_e4m3_host"
    want_b, want_s, _ = ref_image(w)
    got_b, got_s = split_image(dev_img.cpu(), N, K)
    assert torch.equal(got_b, want_b) and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
    if (N, K) == (40, 192):          # a strided source: ld_src = 256 with poison in the pad columns
        wide = torch.full((N, 256), 3e4, dtype=dt, device=DEV)
        wide[:, :K] = w.to(DEV)
        assert torch.equal(ops.pack_weight_e4m3(wide[:, :K]).cpu(), host)


# ------------------------------------------------------------------------------------------------------------------------------
# 2 + 4. the product, inside guard bands
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _weight(N, K, dt):
    """rows of std K^-1/2 scaled by 2^(n % 9 - 4), one all-zero row; -> (device image, fp64 dequantised bytes, fp64 scales, zero row)"""
    g = torch.Generator().manual_seed(N * 7 + K)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * (2.0 ** (torch.arange(N) % 9 - 4).float())[:, None]
    zero = N // 3
    w[zero] = 0
    w = w.to(dt)
    dq, s = quantise(w)
    return ops.pack_weight_e4m3(w.to(DEV)), dq, s, zero


def _product(M, N, K, dt, out_f32):
    img, dq, s, zero = _weight(N, K, dt)
    a = gauss((M, K), 11 + M).float().to(dt)
    bias = gauss((N,), 12, 0.5).float().to(dt)
    res = gauss((M, N), 13 + M).float().to(dt)
    ref = a.double() @ dq.T * s[None] + bias.double()[None] + res.double()
    buf, out = guarded(M, N, F32 if out_f32 else dt)
    ops.gemm_decode(a.to(DEV), img, N, bias=bias.to(DEV), residual=res.to(DEV), out_f32=out_f32, out=out, w_layout=E4)
    torch.cuda.synchronize()
    got = out.cpu()
    e = rel_err(got, ref)
    print(f"e4m3 product M={M} N={N} K={K} {dt} out_f32={out_f32}: rel_err {e:.3e}")
    assert e < (TOL_F32_OUT if out_f32 else TOL[dt]), e
    # the all-zero weight row: exactly bias + residual (one fp32 add, one rounding)
    want0 = bias[zero].float() + res[:, zero].float()
    assert torch.equal(got[:, zero], want0 if out_f32 else want0.to(dt)), "all-zero weight row"
    assert untouched(buf, M, N), "wrote outside the M x N results"


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 5, 16, 17, 26])
@pytest.mark.parametrize("N,K", [(16, 64), (40, 192), (1000, 1088), (3072, 3072), (40, 4480)])
def test_e4m3_product(dt, M, N, K):
    """single fragment; clamped partial fragment with fewer pair steps than waves; 63 fragments with 17 pair steps under 16 waves
    (tail loop only, one wave takes two); 192 fragments, 3 pair steps per wave (one unrolled iteration, no tail); (40, 4 480): 70 pair
    steps under 16 waves x 4 — an unrolled iteration plus a tail for the first six waves"""
    _product(M, N, K, dt, False)
    _product(M, N, K, dt, True)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("N,K", [(3072, 8192), (33000, 512)])
def test_e4m3_product_long_and_wide(dt, M, N, K):
    """down's reduction length (8 pair steps per wave: two unrolled iterations); 2 063 fragments (the 4-fragment blocks, the last one clamped)"""
    _product(M, N, K, dt, False)
    _product(M, N, K, dt, True)


STRUCTURES = [(16, 16384, 1024), (16, 16384, 768), (16, 4096, 2048), (16, 4096, 3072),          # <= 16 rows: 4 x 4 waves, U 4 / 3; 2 x 8, U 4 / 3
              (17, 16384, 2048), (17, 16384, 1536), (26, 4096, 2048), (26, 4096, 3072)]         # 17..32 rows: 2 x 8, U 4 / 3; 2 x 16, U 2 / 3


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M,N,K", STRUCTURES)
def test_e4m3_product_every_other_structure_of_the_launch_table(dt, M, N, K):
    """the (fragments, waves, unroll) structures of launch_skinny_w8_mt that the shapes above do not reach (those run 1 x 16 waves with
    U 3 and 4 at both row ranges, and 4 x 4 / 2 x 8 in the tail loop only), each with at least one unrolled iteration; (26, 4 096,
    3 072) is Llama-3.2-3B's qkv structure at 17..26 rows"""
    _product(M, N, K, dt, False)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. epilogues
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 16, 26])
@pytest.mark.parametrize("stats", ["kernel", "rstd_in"])
def test_e4m3_fused_rmsnorm_and_silu(dt, M, stats):
    """SILU_MUL + fuse_rms as tests/test_kernels_gpu.py::test_gemm_packed_fused_rmsnorm_and_silu, the gain folded before quantisation,
    up rows 2^4 larger than gate rows.  rstd_in: the row factors are handed in (deliberately not the rows' own statistics)."""
    H, Fd = 512, 1024
    x = gauss((M, H), 34).float().to(dt)
    gain = 1 + gauss((H,), 35, 0.1)
    g, u = gauss((Fd, H), 36, H ** -0.5) * gain[None], gauss((Fd, H), 37, H ** -0.5) * gain[None] * 16.0
    wgu = weights.interleave_gate_up(g.float(), u.float()).to(dt)
    dq, s = quantise(wgu)
    w = (dq * s[:, None]).view(Fd // 16, 2, 16, H)
    wg, wu = w[:, 0].reshape(Fd, H), w[:, 1].reshape(Fd, H)
    x64 = x.double()
    rstd = torch.rsqrt(x64.pow(2).mean(-1) + 1e-5)
    if stats == "rstd_in":
        rstd = rstd * (1.0 + 0.5 * (torch.arange(M) % 2).double())
    normed = x64 * rstd.float().double()[:, None] if stats == "rstd_in" else x64 * rstd[:, None]
    a, b = normed @ wg.T, normed @ wu.T
    ref = a * torch.sigmoid(a) * b
    buf, out = guarded(M, Fd, dt)
    ops.gemm_decode(x.to(DEV), ops.pack_weight_e4m3(wgu.to(DEV)), 2 * Fd, act=L.ACT_SILU_MUL, fuse_rms=True, eps=1e-5, out=out, w_layout=E4,
                    rstd_in=rstd.float().to(DEV) if stats == "rstd_in" else None)
    torch.cuda.synchronize()
    e = rel_err(out.cpu(), ref)
    print(f"e4m3 silu_mul + fuse_rms ({stats}) M={M} {dt}: rel_err {e:.3e}")
    assert e < TOL[dt], e
    assert untouched(buf, M, Fd)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 16, 26])
def test_e4m3_rope_kv_epilogue(dt, M):
    """ROPE_KV with the arch of tests/test_kernels_gpu.py::test_gemm_packed_rope_kv_epilogue_equals_separate_kernels, the second
    rotate_half half of every head 2^4 larger than the first, fuse_rms on: q, and the K / V rows appended to a 16-bit cache, against
    RoPE in fp64 of the dequantised product; the e4m3 cache of a second run holds q8 of the 16-bit run's rows; nothing else in
    either cache or around q changes."""
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=6, num_key_value_heads=2, head_dim=128,
                             rope_scaling=dict(factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192))
    nh, nkv, D, H, max_ctx = 6, 2, 128, 256, 64
    N = (nh + 2 * nkv) * D
    cos, sin = weights.rope_tables(arch, max_ctx)
    x = gauss((M, H), 38).float().to(dt)
    W = gauss((N, H), 39, H ** -0.5)
    W.view(nh + 2 * nkv, 2, 64, H)[:, 1] *= 16.0
    perm = _rope_perm(nh, nkv)
    Wp = W.float().to(dt)[perm].contiguous()
    dq, s = quantise(Wp)
    pos = torch.tensor([(7 * i + 3) % max_ctx for i in range(M)], dtype=torch.int32)
    seq = torch.arange(M, dtype=torch.int32)
    x64 = x.double()
    rstd = torch.rsqrt(x64.pow(2).mean(-1) + 1e-5)
    y = torch.empty(M, N, dtype=torch.float64)
    y[:, perm] = (x64 * rstd[:, None]) @ dq.T * s[None]
    yh = y.view(M, nh + 2 * nkv, 2, 64)
    c, sn = cos.double()[pos.long()][:, None], sin.double()[pos.long()][:, None]          # (M, 1, 64)
    a, b = yh[:, :nh + nkv, 0], yh[:, :nh + nkv, 1]
    rot = torch.stack([a * c - b * sn, b * c + a * sn], dim=2).reshape(M, nh + nkv, D)
    q_ref, k_ref, v_ref = rot[:, :nh].reshape(M, nh * D), rot[:, nh:], y.view(M, nh + 2 * nkv, D)[:, nh + nkv:]
    img = ops.pack_weight_e4m3(Wp.to(DEV))
    rope = dict(cos=cos.to(DEV), sin=sin.to(DEV), pos=pos.to(DEV), seq=seq.to(DEV), n_heads=nh, n_kv=nkv, max_ctx=max_ctx)
    kc16 = torch.full((M, nkv, max_ctx, D), FILL, device=DEV, dtype=dt)
    vc16 = torch.full_like(kc16, FILL)
    buf, out = guarded(M, nh * D, dt)
    ops.gemm_decode(x.to(DEV), img, N, act=L.ACT_ROPE_KV, fuse_rms=True, eps=1e-5, out=out, w_layout=E4,
                    rope=dict(rope, k_cache=kc16, v_cache=vc16, kv_format=L.KV_MODEL_DTYPE))
    kc8 = torch.full((M, nkv, max_ctx, D), FILL8, device=DEV, dtype=torch.uint8)
    vc8 = torch.full_like(kc8, FILL8)
    buf8, out8 = guarded(M, nh * D, dt)
    ops.gemm_decode(x.to(DEV), img, N, act=L.ACT_ROPE_KV, fuse_rms=True, eps=1e-5, out=out8, w_layout=E4,
                    rope=dict(rope, k_cache=kc8, v_cache=vc8, kv_format=L.KV_FP8_E4M3))
    torch.cuda.synchronize()
    s_, p_ = seq.long(), pos.long()
    k16, v16 = kc16.cpu()[s_, :, p_], vc16.cpu()[s_, :, p_]          # (M, nkv, D)
    errs = (rel_err(out.cpu(), q_ref), rel_err(k16, k_ref), rel_err(v16, v_ref))
    print(f"e4m3 rope_kv M={M} {dt}: rel_err q {errs[0]:.3e} k {errs[1]:.3e} v {errs[2]:.3e}")
    assert max(errs) < TOL[dt], errs
    assert torch.equal(out8.cpu().view(torch.int16), out.cpu().view(torch.int16)), "q depends on the cache format"
    assert torch.equal(kc8.cpu()[s_, :, p_], q8(k16.float())) and torch.equal(vc8.cpu()[s_, :, p_], q8(v16.float())), "e4m3 cache != q8(16-bit rows)"
    assert untouched(buf, M, nh * D) and untouched(buf8, M, nh * D)
    for cache, fill in ((kc16, FILL), (vc16, FILL), (kc8, FILL8), (vc8, FILL8)):
        chk = cache.cpu().clone()
        chk[s_, :, p_] = fill
        assert bool((chk == fill).all()), "cache written outside (tok_seq, tok_pos)"


# ------------------------------------------------------------------------------------------------------------------------------
# 5. model level (TINY_LLAMA)
# ------------------------------------------------------------------------------------------------------------------------------
def _llama_arch(c):
    return weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                             c.intermediate_size, c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling,
                             c.tie_word_embeddings, tuple(c.eos_token_ids), c.pad_token_id)


def _make_llama(c, seed, dtype, max_ctx=128, **kw):
    sd = ri.llama_state_dict(c, seed=seed)
    return llama_mod.AudioLlamaForCausalLM(_llama_arch(c), dict(sd), torch_dtype=dtype, device=DEV, max_ctx=max_ctx, **kw), sd


def _prefill_and_step(llm, struct, prompts, next_ids):
    """prefill + ONE decode step of `struct` through the C ABI -> (prefill logits, cache after prefill (k, v), decode logits)"""
    lib, B = L.lib(), len(prompts)
    x = torch.cat([p.to(DEV, llm.dtype) for p in prompts]).contiguous()
    cu = [0]
    for p in prompts:
        cu.append(cu[-1] + p.shape[0])
    kv = llm._kv_cache(B)
    llm._kv[0].zero_(); llm._kv[1].zero_()
    ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(struct), x.shape[0], B, 1))
    logits = torch.empty((B, llm.arch.vocab_size), device=DEV, dtype=torch.float32)
    ctx = torch.empty(B, device=DEV, dtype=torch.int32)
    L.check(lib.sl_llama_prefill(C.byref(struct), C.byref(kv), x.data_ptr(), (C.c_int32 * (B + 1))(*cu), B, logits.data_ptr(), ctx.data_ptr(),
                                 None, ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
    pre_logits = logits.cpu()
    pre_cache = (llm._kv[0][:, :B].cpu(), llm._kv[1][:, :B].cpu())
    nid = torch.tensor(next_ids, dtype=torch.int32, device=DEV)
    L.check(lib.sl_llama_decode_step(C.byref(struct), C.byref(kv), nid.data_ptr(), ctx.data_ptr(), B, logits.data_ptr(), ws.data_ptr(),
                                     ws.numel(), L.stream_ptr()), "sl_llama_decode_step")
    return pre_logits, pre_cache, logits.cpu()


_BASE_LENS = (9, 40, 14, 5, 21)
_NEXT = [11, 222, 3, 444, 55]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B", [1, 3, 26])
def test_e4m3_model_prefill_is_the_16bit_one_and_the_decode_step_matches_the_oracle(dt, B):
    """(a) prefill ignores the decode-weight format: logits and the whole prompt cache bit-identical to the 16-bit struct's.
    (b) the e4m3 decode step against lo.llama_forward on e4m3_dequantised_state_dict(), past = the GPU cache read back after
    prefill, at the 16-bit step's bound (BF16_TOL; a quarter of it for fp16).
    (c) the e4m3 step against the 16-bit step: 2 TOL16 + d, d = the oracle's own distance between the original and the dequantised
    weights on the same past (printed with the worst ratio: the cost of the quantisation at this size)."""
    cfg = TINY_LLAMA
    gen = torch.Generator().manual_seed(8)
    base = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in _BASE_LENS]
    prompts, nxt = [base[b % 5] for b in range(B)], [_NEXT[b % 5] for b in range(B)]
    llm, sd = _make_llama(cfg, 33, dt, weight_dtype="fp8")
    w = llm._dev()
    assert w.struct_e4m3.reserved == L.WDEC_E4M3 and w.struct.reserved == L.WDEC_MODEL_DTYPE
    pl16, pc16, dl16 = _prefill_and_step(llm, w.struct, prompts, nxt)
    pl8, pc8, dl8 = _prefill_and_step(llm, w.struct_e4m3, prompts, nxt)
    assert torch.equal(pl8.view(torch.int32), pl16.view(torch.int32)), "prefill logits differ between the decode-weight formats"
    assert torch.equal(pc8[0].view(torch.int16), pc16[0].view(torch.int16)) and torch.equal(pc8[1].view(torch.int16), pc16[1].view(torch.int16))
    sdq = w.e4m3_dequantised_state_dict()
    sdo = {k: v.to(dt).float() for k, v in sd.items()}
    embed = sdo["model.embed_tokens.weight"]
    assert torch.equal(sdq["model.embed_tokens.weight"], embed)
    worst_b, worst_c, ds = 0.0, 0.0, []
    for b in range(min(B, 5)):
        n = prompts[b].shape[0]
        past = [(pc8[0][l, b, :, :n].float()[None], pc8[1][l, b, :, :n].float()[None]) for l in range(cfg.num_hidden_layers)]
        tok = embed[nxt[b]][None, None]
        ref_q = lo.llama_forward(sdq, cfg, tok, past=past, last_logits_only=True)["logits"][0, -1]
        ref_o = lo.llama_forward(sdo, cfg, tok, past=past, last_logits_only=True)["logits"][0, -1]
        d = rel_err(ref_q, ref_o)
        ds.append(d)
        for r in range(b, B, 5):          # the rows that repeat this sequence hold the same prompt: the same reference
            eb, ec = rel_err(dl8[r], ref_q), rel_err(dl8[r], dl16[r])
            worst_b, worst_c = max(worst_b, eb / TOL16[dt]), max(worst_c, ec / (2 * TOL16[dt] + d))
            assert eb < TOL16[dt], ("e4m3 step against the oracle on the dequantised weights", r, eb)
            assert ec < 2 * TOL16[dt] + d, ("e4m3 step against the 16-bit step", r, ec, d)
    print(f"e4m3 decode step {dt} B={B}: quantisation distance d per sequence {['%.2e' % d for d in ds]}, worst err / bound: oracle {worst_b:.3f}, "
          f"16-bit step {worst_c:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. selection and graphs
# ------------------------------------------------------------------------------------------------------------------------------
def _prompts(cfg, B, seed=12):
    gen = torch.Generator().manual_seed(seed)
    tails = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in (9, 30, 14, 5, 21, 1, 17, 11)]
    prompts = [tails[b % len(tails)] * (1.0 + 0.01 * (b // len(tails))) for b in range(B)]
    return torch.cat(prompts).to(DEV, BF16), [int(p.shape[0]) for p in prompts]


def test_struct_is_chosen_per_call_and_graphs_are_not_shared():
    cfg = TINY_LLAMA
    plain, _ = _make_llama(cfg, 35, BF16)
    x3, l3 = _prompts(cfg, 3)
    x40, l40 = _prompts(cfg, 40)
    want3, _ = plain.generate_packed(x3.clone(), l3, 12, use_eos=False)
    assert plain.last_generate_stats["weight_format"] == "16-bit"
    want40, _ = plain.generate_packed(x40.clone(), l40, 12, use_eos=False)
    del plain
    llm, _ = _make_llama(cfg, 35, BF16, weight_dtype="fp8")
    got, fmts = [], []
    for x, lens in ((x3, l3), (x40, l40), (x3, l3)):
        ids, _ = llm.generate_packed(x.clone(), lens, 12, use_eos=False)
        got.append(ids)
        fmts.append(llm.last_generate_stats["weight_format"])
    assert fmts == ["e4m3", "16-bit", "e4m3"]
    assert torch.equal(got[0], got[2])
    assert torch.equal(got[1], want40), "a batch above sl_w8_max_rows() must run the 16-bit struct"
    ws_ptr = llm._ws.data_ptr()
    llm.set_weight_dtype(None)
    ids, _ = llm.generate_packed(x3.clone(), l3, 12, use_eos=False)
    assert llm.last_generate_stats["weight_format"] == "16-bit" and llm._ws.data_ptr() == ws_ptr
    assert torch.equal(ids, want3), "after set_weight_dtype(None) the ids are those of a model built without the option"
    llm.set_weight_dtype(torch.float8_e4m3fn)
    ids, _ = llm.generate_packed(x3.clone(), l3, 12, use_eos=False)
    assert llm.last_generate_stats["weight_format"] == "e4m3" and torch.equal(ids, got[0])


def test_e4m3_compaction_keeps_every_sequences_ids():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, weight_dtype="fp8")
    B, new = 26, 24
    x, lens = _prompts(cfg, B)
    limits = [2 + (7 * b) % 23 for b in range(B)]
    limits[0] = 2
    llm.generation_config.eos_token_id = None
    ref, n_ref = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=False)
    ids, n = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=True, check_every=2)
    assert llm.last_generate_stats["weight_format"] == "e4m3" and llm.last_generate_stats["compactions"] >= 2
    assert n == n_ref and torch.equal(ids[:, :n], ref[:, :n_ref])


def test_e4m3_weights_with_the_e4m3_kv_cache():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, weight_dtype="fp8", kv_cache_dtype="fp8")
    x, lens = _prompts(cfg, 5)
    a, _ = llm.generate_packed(x.clone(), lens, 16, use_eos=False)
    assert llm._kv[0].dtype == torch.uint8 and llm.last_generate_stats["weight_format"] == "e4m3"
    b, _ = llm.generate_packed(x.clone(), lens, 16, use_eos=False)
    assert torch.equal(a, b)
