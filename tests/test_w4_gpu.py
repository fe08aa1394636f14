"""GPU: the opt-in MXFP4 decode weights — w_layout = SL_W_PACKED_MXFP4, sl_llama_model.reserved = SL_WDEC_MXFP4, weight_dtype="mxfp4".

The packer is held byte for byte against the format's definition written in torch (tests/test_w4_host_cpu.py), and the one-hot probe
below pins what only the chip can say: the fragment layout, the nibble order, the scale indexing and what v_cvt_scalef32_pk_*_fp4 does
with its scale operand.  Every dequantised value e2m1 * 2^e is exact in bf16 and in fp16, so the kernel owes what the 16-bit packed
kernel owes against x @ dq(W)^T in fp64 and is held to its bounds: TOL = 1.5e-2 in bf16 (tests/test_kernels_gpu.py), 5e-4 in fp16
(tests/test_fp16_gpu.py ONE_ROUNDING), 2e-5 with fp32 outputs.  Weights vary by 2^((block + row) % 9 - 4) along K and across rows,
gate / up rows and the two rotate_half halves differ by 2^4: a scale read from the wrong block or row misses by orders of magnitude.
Outputs are views into sentinel-filled buffers.  Model level: TINY_LLAMA against the CPU oracle run on mxfp4_dequantised_state_dict().
Agreement of ids with the 16-bit model is NOT asserted: 4-bit weights are a different model."""
import functools

import pytest
import torch

from conftest import pkg, rel_err
from oracle import llama_oracle as lo
from oracle.golden_cfgs import TINY_LLAMA
from test_kernel_edges_gpu import DEV, FILL, _rope_perm, gauss, guarded, untouched
from test_w4_host_cpu import GRID, SHAPES, ref_image, split_image, weight_rows
from test_w8_gpu import _BASE_LENS, _NEXT, _make_llama, _prefill_and_step, _prompts, q8

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
weights = pkg("weights")

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT16 = [BF16, F16]
TOL = {BF16: 1.5e-2, F16: 5e-4}          # tests/test_kernels_gpu.py TOL[bf16]; tests/test_fp16_gpu.py ONE_ROUNDING (its packed products)
TOL_F32_OUT = 2e-5
BF16_TOL = 3e-2                          # tests/test_models_gpu.py
TOL16 = {BF16: BF16_TOL, F16: BF16_TOL / 4}
FILL8 = 0x5A
W4 = L.W_PACKED_MXFP4


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the device packer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("N,K", SHAPES)
def test_device_packer_equals_the_host_entry(dt, N, K):
    w = weight_rows(N, K, dt)
    host = ops.pack_weight_mxfp4(w)
    dev_img = ops.pack_weight_mxfp4(w.to(DEV))
    assert torch.equal(dev_img.cpu(), host), "device packer differs from sl_pack_weight_mxfp4_host"
    want_b, want_s, _, _ = ref_image(w)
    got_b, got_s = split_image(dev_img.cpu(), N, K)
    assert torch.equal(got_b, want_b) and torch.equal(got_s, want_s)
    if (N, K) == (40, 384):          # a strided source: ld_src = 512 with poison in the pad columns
        wide = torch.full((N, 512), 3e4, dtype=dt, device=DEV)
        wide[:, :K] = w.to(DEV)
        assert torch.equal(ops.pack_weight_mxfp4(wide[:, :K]).cpu(), host)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the one-hot probe
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
def test_one_hot_probe_pins_layout_nibble_order_scale_indexing_and_the_conversion(dt):
    """16 * 27 rows, K = 256: block b of row n has exponent (n // 16 + b) % 27 - 13 — every exponent of the clamp in every block
    position of a quad step — and element k holds value number (n + k) % 15 of the 15 codes (no negative zero), so every block holds
    +-6 (its exponent is the intended one) and every position sees every code.  All of it exact in bf16 and fp16, so dq(W) = W.  x = 16
    one-hot rows k0 .. k0 + 15, fp32 outputs: one product per output, 1 * value, nothing to round — the product must return
    dq(W)[:, k0:k0+16]^T bit for bit, for every k0."""
    N, K = 16 * 27, 256
    vals = torch.cat([GRID, -GRID[1:]])
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    e = (n // 16 + k // 32) % 27 - 13
    w64 = vals[(n + k) % 15] * torch.exp2(e.double())
    w = w64.to(dt)
    assert torch.equal(w.double(), w64), "the probe's weights must be exact in the model dtype"
    img = ops.pack_weight_mxfp4(w.to(DEV))
    dq = ops.w4_dequantise(img, N, K)
    assert torch.equal(dq, w64), "every probe weight is a value of the format: the packer must keep it"
    for k0 in range(0, K, 16):
        x = torch.zeros(16, K, dtype=dt)
        x[torch.arange(16), k0 + torch.arange(16)] = 1.0
        buf, out = guarded(16, N, F32)
        ops.gemm_decode(x.to(DEV), img, N, out_f32=True, out=out, w_layout=W4)
        torch.cuda.synchronize()
        got, want = out.cpu(), dq[:, k0:k0 + 16].T.float()
        bad = (got != want).nonzero()
        assert torch.equal(got, want), f"k0={k0}: {bad.shape[0]} elements differ, first (x row, weight row) {bad[0].tolist()}: got {float(got[tuple(bad[0])])} want {float(want[tuple(bad[0])])}"
        assert untouched(buf, 16, N)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the product, inside guard bands
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _weight(N, K, dt):
    """std K^-1/2 scaled by 2^((block + row) % 9 - 4), one all-zero row -> (device image, fp64 dq(W) of the R base rows, R, zero row).
    Above 1 024 rows (a multiple of it) the weight is its first R = 1 024 rows repeated, so the CPU reference stays small; the row
    pattern has period 9, so neighbouring fragments still differ."""
    R = 1024 if (N > 1024 and N % 1024 == 0) else N
    g = torch.Generator().manual_seed(N * 7 + K)
    mag = 2.0 ** ((torch.arange(K // 32)[None, :] + torch.arange(R)[:, None]) % 9 - 4).float()
    w = (torch.randn(R, K // 32, 32, generator=g) * K ** -0.5 * mag[:, :, None]).view(R, K)
    zero = R // 3
    w[zero] = 0
    w = w.to(dt).to(DEV)
    dq = ops.w4_dequantise(ops.pack_weight_mxfp4(w), R, K)
    return ops.pack_weight_mxfp4(w.repeat(N // R, 1)), dq, R, zero


def _product(M, N, K, dt, out_f32):
    img, dq, R, zero = _weight(N, K, dt)
    a = gauss((M, K), 11 + M).float().to(dt)
    bias = gauss((N,), 12, 0.5).float().to(dt)
    res = gauss((M, N), 13 + M).float().to(dt)
    ref = (a.double() @ dq.T).repeat(1, N // R) + bias.double()[None] + res.double()
    buf, out = guarded(M, N, F32 if out_f32 else dt)
    ops.gemm_decode(a.to(DEV), img, N, bias=bias.to(DEV), residual=res.to(DEV), out_f32=out_f32, out=out, w_layout=W4)
    torch.cuda.synchronize()
    got = out.cpu()
    e = rel_err(got, ref)
    print(f"mxfp4 product M={M} N={N} K={K} {dt} out_f32={out_f32}: rel_err {e:.3e}")
    assert e < (TOL_F32_OUT if out_f32 else TOL[dt]), e
    # the all-zero weight rows: exactly bias + residual (one fp32 add, one rounding)
    zs = torch.arange(zero, N, R)
    want0 = bias[zs].float()[None] + res[:, zs].float()
    assert torch.equal(got[:, zs], want0 if out_f32 else want0.to(dt)), "all-zero weight row"
    assert untouched(buf, M, N), "wrote outside the M x N results"


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 5, 16, 17, 26])
@pytest.mark.parametrize("N,K", [(16, 128), (40, 384), (1000, 2176), (3072, 3072), (40, 8960)])
def test_mxfp4_product(dt, M, N, K):
    """single fragment, one quad step; clamped partial fragment with fewer quad steps (3) than waves; 63 fragments with 17 quad steps
    under 16 waves (tail loop only, one wave takes two); 192 fragments, 24 steps under 16 waves; (40, 8 960): 70 quad steps under
    16 waves x 4 — an unrolled pass plus a tail for the first six waves"""
    _product(M, N, K, dt, False)
    _product(M, N, K, dt, True)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("N,K", [(3072, 8192), (33000, 512)])
def test_mxfp4_product_long_and_wide(dt, M, N, K):
    """down's reduction length (4 quad steps per wave: one unrolled pass, no tail); 2 063 fragments (the 4-fragment blocks, the last one clamped)"""
    _product(M, N, K, dt, False)
    _product(M, N, K, dt, True)


STRUCTURES = [(16, 16384, 2048), (16, 16384, 1536), (16, 4096, 4096), (16, 4096, 3072), (16, 40, 6144),      # <= 16 rows: 4 x 4 waves, U 4 / 3; 2 x 8, U 4 / 3; 1 x 16, U 3
              (17, 16384, 4096), (17, 16384, 3072), (26, 4096, 4096), (26, 4096, 6144), (17, 40, 6144)]      # 17..32 rows: 2 x 8, U 4 / 3; 2 x 16, U 2 / 3; 1 x 16, U 3


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M,N,K", STRUCTURES)
def test_mxfp4_product_every_other_structure_of_the_launch_table(dt, M, N, K):
    """the (fragments, waves, unroll) structures of launch_skinny_w4_mt that the shapes above do not reach (those run 1 x 16 waves with
    U 4 at both row ranges, and 4 x 4 in the tail loop only), each with at least one unrolled pass"""
    _product(M, N, K, dt, False)


# ------------------------------------------------------------------------------------------------------------------------------
# (d) epilogues
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 16, 26])
@pytest.mark.parametrize("stats", ["kernel", "rstd_in"])
def test_mxfp4_fused_rmsnorm_and_silu(dt, M, stats):
    """SILU_MUL + fuse_rms as tests/test_w8_gpu.py::test_e4m3_fused_rmsnorm_and_silu, the gain folded before quantisation, up rows 2^4
    larger than gate rows.  rstd_in: the row factors are handed in (deliberately not the rows' own statistics)."""
    H, Fd = 512, 1024
    x = gauss((M, H), 34).float().to(dt)
    gain = 1 + gauss((H,), 35, 0.1)
    g, u = gauss((Fd, H), 36, H ** -0.5) * gain[None], gauss((Fd, H), 37, H ** -0.5) * gain[None] * 16.0
    wgu = weights.interleave_gate_up(g.float(), u.float()).to(dt)
    img = ops.pack_weight_mxfp4(wgu.to(DEV))
    w = ops.w4_dequantise(img, 2 * Fd, H).view(Fd // 16, 2, 16, H)
    wg, wu = w[:, 0].reshape(Fd, H), w[:, 1].reshape(Fd, H)
    x64 = x.double()
    rstd = torch.rsqrt(x64.pow(2).mean(-1) + 1e-5)
    if stats == "rstd_in":
        rstd = rstd * (1.0 + 0.5 * (torch.arange(M) % 2).double())
    normed = x64 * rstd.float().double()[:, None] if stats == "rstd_in" else x64 * rstd[:, None]
    a, b = normed @ wg.T, normed @ wu.T
    ref = a * torch.sigmoid(a) * b
    buf, out = guarded(M, Fd, dt)
    ops.gemm_decode(x.to(DEV), img, 2 * Fd, act=L.ACT_SILU_MUL, fuse_rms=True, eps=1e-5, out=out, w_layout=W4,
                    rstd_in=rstd.float().to(DEV) if stats == "rstd_in" else None)
    torch.cuda.synchronize()
    e = rel_err(out.cpu(), ref)
    print(f"mxfp4 silu_mul + fuse_rms ({stats}) M={M} {dt}: rel_err {e:.3e}")
    assert e < TOL[dt], e
    assert untouched(buf, M, Fd)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 16, 26])
def test_mxfp4_rope_kv_epilogue(dt, M):
    """ROPE_KV as tests/test_w8_gpu.py::test_e4m3_rope_kv_epilogue: the second rotate_half half of every head 2^4 larger than the first,
    fuse_rms on: q, and the K / V rows appended to a 16-bit cache, against RoPE in fp64 of the dequantised product; the e4m3 cache of a
    second run holds q8 of the 16-bit run's rows; nothing else in either cache or around q changes."""
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
    img = ops.pack_weight_mxfp4(Wp.to(DEV))
    dq = ops.w4_dequantise(img, N, H)
    pos = torch.tensor([(7 * i + 3) % max_ctx for i in range(M)], dtype=torch.int32)
    seq = torch.arange(M, dtype=torch.int32)
    x64 = x.double()
    rstd = torch.rsqrt(x64.pow(2).mean(-1) + 1e-5)
    y = torch.empty(M, N, dtype=torch.float64)
    y[:, perm] = (x64 * rstd[:, None]) @ dq.T
    yh = y.view(M, nh + 2 * nkv, 2, 64)
    c, sn = cos.double()[pos.long()][:, None], sin.double()[pos.long()][:, None]          # (M, 1, 64)
    a, b = yh[:, :nh + nkv, 0], yh[:, :nh + nkv, 1]
    rot = torch.stack([a * c - b * sn, b * c + a * sn], dim=2).reshape(M, nh + nkv, D)
    q_ref, k_ref, v_ref = rot[:, :nh].reshape(M, nh * D), rot[:, nh:], y.view(M, nh + 2 * nkv, D)[:, nh + nkv:]
    rope = dict(cos=cos.to(DEV), sin=sin.to(DEV), pos=pos.to(DEV), seq=seq.to(DEV), n_heads=nh, n_kv=nkv, max_ctx=max_ctx)
    kc16 = torch.full((M, nkv, max_ctx, D), FILL, device=DEV, dtype=dt)
    vc16 = torch.full_like(kc16, FILL)
    buf, out = guarded(M, nh * D, dt)
    ops.gemm_decode(x.to(DEV), img, N, act=L.ACT_ROPE_KV, fuse_rms=True, eps=1e-5, out=out, w_layout=W4,
                    rope=dict(rope, k_cache=kc16, v_cache=vc16, kv_format=L.KV_MODEL_DTYPE))
    kc8 = torch.full((M, nkv, max_ctx, D), FILL8, device=DEV, dtype=torch.uint8)
    vc8 = torch.full_like(kc8, FILL8)
    buf8, out8 = guarded(M, nh * D, dt)
    ops.gemm_decode(x.to(DEV), img, N, act=L.ACT_ROPE_KV, fuse_rms=True, eps=1e-5, out=out8, w_layout=W4,
                    rope=dict(rope, k_cache=kc8, v_cache=vc8, kv_format=L.KV_FP8_E4M3))
    torch.cuda.synchronize()
    s_, p_ = seq.long(), pos.long()
    k16, v16 = kc16.cpu()[s_, :, p_], vc16.cpu()[s_, :, p_]          # (M, nkv, D)
    errs = (rel_err(out.cpu(), q_ref), rel_err(k16, k_ref), rel_err(v16, v_ref))
    print(f"mxfp4 rope_kv M={M} {dt}: rel_err q {errs[0]:.3e} k {errs[1]:.3e} v {errs[2]:.3e}")
    assert max(errs) < TOL[dt], errs
    assert torch.equal(out8.cpu().view(torch.int16), out.cpu().view(torch.int16)), "q depends on the cache format"
    assert torch.equal(kc8.cpu()[s_, :, p_], q8(k16.float())) and torch.equal(vc8.cpu()[s_, :, p_], q8(v16.float())), "e4m3 cache != q8(16-bit rows)"
    assert untouched(buf, M, nh * D) and untouched(buf8, M, nh * D)
    for cache, fill in ((kc16, FILL), (vc16, FILL), (kc8, FILL8), (vc8, FILL8)):
        chk = cache.cpu().clone()
        chk[s_, :, p_] = fill
        assert bool((chk == fill).all()), "cache written outside (tok_seq, tok_pos)"


# ------------------------------------------------------------------------------------------------------------------------------
# (e) model level (TINY_LLAMA)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B", [1, 3, 26])
def test_mxfp4_model_prefill_is_the_16bit_one_and_the_decode_step_matches_the_oracle(dt, B):
    """(a) prefill ignores the decode-weight format: logits and the whole prompt cache bit-identical to the 16-bit struct's.
    (b) the MXFP4 decode step against lo.llama_forward on mxfp4_dequantised_state_dict(), past = the GPU cache read back after
    prefill, at the 16-bit step's bound (BF16_TOL; a quarter of it for fp16).
    Printed, not asserted: d, the oracle's own logit distance between the original and the dequantised weights on the same past — the
    cost of the quantisation at this size (DESIGN §3.8 records it)."""
    cfg = TINY_LLAMA
    gen = torch.Generator().manual_seed(8)
    base = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in _BASE_LENS]
    prompts, nxt = [base[b % 5] for b in range(B)], [_NEXT[b % 5] for b in range(B)]
    llm, sd = _make_llama(cfg, 33, dt, weight_dtype="mxfp4")
    w = llm._dev()
    assert w.struct_mxfp4.reserved == L.WDEC_MXFP4 and w.struct.reserved == L.WDEC_MODEL_DTYPE
    pl16, pc16, _ = _prefill_and_step(llm, w.struct, prompts, nxt)
    pl4, pc4, dl4 = _prefill_and_step(llm, w.struct_mxfp4, prompts, nxt)
    assert torch.equal(pl4.view(torch.int32), pl16.view(torch.int32)), "prefill logits differ between the decode-weight formats"
    assert torch.equal(pc4[0].view(torch.int16), pc16[0].view(torch.int16)) and torch.equal(pc4[1].view(torch.int16), pc16[1].view(torch.int16))
    sdq = w.mxfp4_dequantised_state_dict()
    sdo = {k: v.to(dt).float() for k, v in sd.items()}
    embed = sdo["model.embed_tokens.weight"]
    assert torch.equal(sdq["model.embed_tokens.weight"], embed)
    worst, ds = 0.0, []
    for b in range(min(B, 5)):
        n = prompts[b].shape[0]
        past = [(pc4[0][l, b, :, :n].float()[None], pc4[1][l, b, :, :n].float()[None]) for l in range(cfg.num_hidden_layers)]
        tok = embed[nxt[b]][None, None]
        ref_q = lo.llama_forward(sdq, cfg, tok, past=past, last_logits_only=True)["logits"][0, -1]
        ref_o = lo.llama_forward(sdo, cfg, tok, past=past, last_logits_only=True)["logits"][0, -1]
        ds.append(rel_err(ref_q, ref_o))
        for r in range(b, B, 5):          # the rows that repeat this sequence hold the same prompt: the same reference
            eb = rel_err(dl4[r], ref_q)
            worst = max(worst, eb / TOL16[dt])
            assert eb < TOL16[dt], ("MXFP4 step against the oracle on the dequantised weights", r, eb)
    print(f"mxfp4 decode step {dt} B={B}: quantisation distance d per sequence {['%.2e' % d for d in ds]}, worst err / bound against the oracle {worst:.3f}")


def test_struct_is_chosen_per_call_and_graphs_are_not_shared_between_the_three_formats():
    """26 rows take the MXFP4 struct, 27 rows the 16-bit one.  One model is switched between the three formats on one workspace and one
    cache; each format's ids must be those of a model that never held another format (were a captured graph shared, a format would
    return another's ids).  With the option unset the format reads "16-bit", as before."""
    cfg = TINY_LLAMA
    x3, l3 = _prompts(cfg, 3)
    x26, l26 = _prompts(cfg, 26)
    x27, l27 = _prompts(cfg, 27)
    want = {}
    for name, kw in (("16-bit", {}), ("e4m3", dict(weight_dtype="fp8")), ("mxfp4", dict(weight_dtype="mxfp4"))):
        fresh, _ = _make_llama(cfg, 35, BF16, **kw)
        want[name], _ = fresh.generate_packed(x3.clone(), l3, 12, use_eos=False)
        assert fresh.last_generate_stats["weight_format"] == name
        if name == "16-bit":
            want27, _ = fresh.generate_packed(x27.clone(), l27, 12, use_eos=False)
        del fresh
    llm, _ = _make_llama(cfg, 35, BF16, weight_dtype="mxfp4")
    ids26, _ = llm.generate_packed(x26.clone(), l26, 12, use_eos=False)
    assert llm.last_generate_stats["weight_format"] == "mxfp4"
    ids27, _ = llm.generate_packed(x27.clone(), l27, 12, use_eos=False)
    assert llm.last_generate_stats["weight_format"] == "16-bit"
    assert torch.equal(ids27, want27), "a batch above sl_w4_max_rows() must run the 16-bit struct"
    ws_ptr = None
    for wd, name in (("mxfp4", "mxfp4"), (None, "16-bit"), ("fp8", "e4m3"), ("fp4", "mxfp4"), ("fp8", "e4m3"), (None, "16-bit"), ("mxfp4", "mxfp4")):
        llm.set_weight_dtype(wd)
        ids, _ = llm.generate_packed(x3.clone(), l3, 12, use_eos=False)
        assert llm.last_generate_stats["weight_format"] == name
        assert torch.equal(ids, want[name]), f"{name}: ids differ from those of a model that only ever held this format"
        if ws_ptr is None:
            ws_ptr = llm._ws.data_ptr()
        assert llm._ws.data_ptr() == ws_ptr
    again, _ = llm.generate_packed(x26.clone(), l26, 12, use_eos=False)
    assert torch.equal(again, ids26)


def test_mxfp4_compaction_keeps_every_sequences_ids():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, weight_dtype="mxfp4")
    B, new = 26, 24
    x, lens = _prompts(cfg, B)
    limits = [2 + (7 * b) % 23 for b in range(B)]
    limits[0] = 2
    llm.generation_config.eos_token_id = None
    ref, n_ref = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=False)
    ids, n = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=True, check_every=2)
    assert llm.last_generate_stats["weight_format"] == "mxfp4" and llm.last_generate_stats["compactions"] >= 2
    assert n == n_ref and torch.equal(ids[:, :n], ref[:, :n_ref])


def test_mxfp4_weights_with_the_e4m3_kv_cache():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, weight_dtype="mxfp4", kv_cache_dtype="fp8")
    x, lens = _prompts(cfg, 5)
    a, _ = llm.generate_packed(x.clone(), lens, 16, use_eos=False)
    assert llm._kv[0].dtype == torch.uint8 and llm.last_generate_stats["weight_format"] == "mxfp4"
    b, _ = llm.generate_packed(x.clone(), lens, 16, use_eos=False)
    assert torch.equal(a, b)
