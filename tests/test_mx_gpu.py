"""GPU: the opt-in MX linears — sl_gemm_mx on v_mfma_scale_f32_16x16x128_f8f6f4 (A = e4m3, B = e2m1), the device quantiser and packer,
and sl_llama_model.reserved = SL_WDEC_MX_LINEAR through prefill, the decode step and generate.

The one-hot probes pin what only the chip can say: which k a lane supplies, the nibble order, which scale a lane's block takes and the
accumulator map.  The exact products are integer-valued operands whose every partial sum is exact in fp32, so any summation order must
return the fp64 product bit for bit.  The random products are held to a DERIVED bound: an fp32 accumulation of K terms, each product
exact (an 4-bit times a 2-bit significand), errs by at most (K - 1) roundings of at most 2^-24 of the running sum of magnitudes — and twice
that, K * 2^-23 * sum |a b|, also covers an accumulator that truncates instead of rounding — plus half an ulp of the output type.
Every output is a view into a sentinel-filled buffer."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import pkg, rel_err
from test_mx_host_cpu import E2M1, image_from_codes, weight_rows

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
weights = pkg("weights")

DEV = "cuda:0"
F16, BF16, F32, F8 = torch.float16, torch.bfloat16, torch.float32, torch.float8_e4m3fn
DT16 = [BF16, F16]
FILL = -1504.0                       # output sentinel, exact in bf16 / fp16 / fp32
FILL8 = 0xA5
GRID16 = np.concatenate([E2M1, -E2M1])


def guarded(rows, cols, dtype):
    """(buffer, view): rows x cols inside a sentinel-filled buffer, one row above and below, 8 elements left and at least 8 right"""
    ld = (cols + 7) // 8 * 8 + 16
    buf = torch.full((rows + 2, ld), FILL, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1, 8:8 + cols]


def untouched(buf, rows, cols):
    chk = buf.clone()
    chk[1:rows + 1, 8:8 + cols] = FILL
    return bool((chk == FILL).all())


def guarded_bytes(n, pad=256):
    buf = torch.full((n + 2 * pad,), FILL8, dtype=torch.uint8, device=DEV)
    return buf, buf[pad:pad + n]


def untouched_bytes(buf, n, pad=256):
    return bool((buf[:pad] == FILL8).all()) and bool((buf[pad + n:] == FILL8).all())


def e4m3_bytes(v):
    """fp64 / fp32 values that ARE e4m3 values -> their bytes"""
    b = v.float().to(F8)
    assert torch.equal(b.double(), v.double()), "not e4m3 values"
    return b.view(torch.uint8)


def dq_a(q, s):
    return ops.mxfp8_dequantise(q, s)


def dq_w(code, sc):
    """natural-order codes (N, K), scale bytes (N, K/32) (numpy) -> fp64 (N, K)"""
    N, K = code.shape
    return torch.from_numpy((GRID16[code].reshape(N, K // 32, 32) * np.exp2(sc.astype(np.float64) - 127)[:, :, None]).reshape(N, K))


def image(code, sc):
    """natural-order codes / scale bytes of N rows (numpy) -> the device MX weight image (padding rows: zero codes, byte 127)"""
    N, K = code.shape
    Np = (N + 15) // 16 * 16
    c = np.zeros((Np, K), dtype=np.uint8)
    s = np.full((Np, K // 32), 127, dtype=np.uint8)
    c[:N], s[:N] = code, sc
    b, sb = image_from_codes(c, s)
    return torch.cat([b, sb]).to(DEV)


def run(Aq, As, img, N, dt, out_dtype, **kw):
    """-> (result on the CPU, guard band intact)"""
    M = Aq.shape[0]
    cols = N // 2 if kw.get("act") == L.ACT_SILU_MUL else N
    buf, out = guarded(M, cols, out_dtype)
    ops.gemm_mx(Aq.to(DEV), As.to(DEV), img, N, dtype=dt, out_f32=out_dtype == F32, out=out, **kw)
    torch.cuda.synchronize()
    return out.cpu(), untouched(buf, M, cols)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the operand-map probe
# ------------------------------------------------------------------------------------------------------------------------------
def test_operand_map_probe():
    """M = N = K = 128, one launch each way.  (a) A one-hot: A[m][k] = a_m (k == m), a_m a nonzero e4m3 value that changes with the row,
    scale bytes that change with (row, block); B dense, asymmetric in (n, k), scales changing with (n, block).  One product per output, an
    exact one: C[m][n] must be a_m 2^ea[m][m/32] dq(B)[n][m], bit for bit.  A lane that supplied other k than [32 (l >> 4), +32), a swapped
    nibble, a scale taken from another block, row or byte of the register, or another accumulator map each change some output.
    (b) the roles swapped: B one-hot, A dense."""
    M = N = K = 128
    m, n, k, blk = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :], np.arange(K // 32)[None, :]
    # (a)
    a_byte = (8 + (37 * np.arange(M)) % 111 + 128 * (np.arange(M) % 3 == 1)).astype(np.uint8)           # normal, finite, both signs
    Aq = torch.zeros(M, K, dtype=torch.uint8)
    Aq[torch.arange(M), torch.arange(M)] = torch.from_numpy(a_byte)
    As = torch.from_numpy((127 + (m + 3 * blk) % 9 - 4).astype(np.uint8))
    codeB = ((7 * n + 3 * k + (n * k) // 5) % 15 + 1).astype(np.uint8)                                  # 1 .. 15: every nonzero code, no symmetry
    scB = (127 + (2 * n + 5 * blk) % 11 - 5).astype(np.uint8)
    got, ok = run(Aq, As, image(codeB, scB), N, BF16, F32)
    want = (dq_a(Aq, As) @ dq_w(codeB, scB).T).float()
    a_val = torch.from_numpy(a_byte).view(F8).double() * torch.exp2(As.double() - 127)[torch.arange(M), torch.arange(M) // 32]
    assert torch.equal(want.double(), a_val[:, None] * dq_w(codeB, scB).T[:M]), "the reference itself: one exact product per output"
    bad = (got != want).nonzero()
    assert torch.equal(got, want), f"one-hot A: {bad.shape[0]} outputs differ, first (m, n) {bad[0].tolist()}: got {float(got[tuple(bad[0])])} want {float(want[tuple(bad[0])])}"
    assert ok
    # (b)
    codeB = np.zeros((N, K), dtype=np.uint8)
    codeB[np.arange(N), np.arange(N)] = 1 + (5 * np.arange(N)) % 7 + 8 * (np.arange(N) % 2)             # a nonzero code of either sign
    scB = (127 + (n + 2 * blk) % 7 - 3).astype(np.uint8)
    Aq = torch.from_numpy((8 + (11 * m + 5 * k + (m * k) // 3) % 111 + 128 * ((m + k) % 2)).astype(np.uint8))
    As = torch.from_numpy((127 + (3 * m + blk) % 9 - 4).astype(np.uint8))
    got, ok = run(Aq, As, image(codeB, scB), N, BF16, F32)
    want = (dq_a(Aq, As) @ dq_w(codeB, scB).T).float()
    bad = (got != want).nonzero()
    assert torch.equal(got, want), f"one-hot B: {bad.shape[0]} outputs differ, first (m, n) {bad[0].tolist()}: got {float(got[tuple(bad[0])])} want {float(want[tuple(bad[0])])}"
    assert ok


# ------------------------------------------------------------------------------------------------------------------------------
# 2. device quantiser and device packer against their host entries
# ------------------------------------------------------------------------------------------------------------------------------
def _rows(M, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** ((torch.arange(K // 32)[None, :] * 5 + torch.arange(M)[:, None] * 3) % 31 - 15).float()
    x = (torch.randn(M, K // 32, 32, generator=g) * mag[:, :, None]).view(M, K)
    x[0, 3], x[0, 40], x[0, 70] = float("inf"), float("-inf"), float("nan")
    x[0, 96:128] = 0
    x[M - 1, 0:32] = torch.randn(32, generator=g) * (6e-8 if dt == F16 else 1e-39)      # subnormals of the type
    x[M // 2, 5] = 448.0
    x[M // 2, 37], x[M // 2, 38] = 65504.0 if dt == F16 else 3.0e38, -1.0
    return x.to(dt)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("K", [128, 384, 3072])
@pytest.mark.parametrize("M", [1, 17, 300])
def test_device_quantiser_equals_the_host_entry(dt, M, K):
    x = _rows(M, K, dt, 100 * M + K)
    hq, hs = ops.mxfp8_quantize_rows(x)
    for ld in (K, K + 24):            # ld = K + 24: rows that are not 16-byte aligned, poison in the pad columns
        wide = torch.full((M, ld), 7e4 if dt == BF16 else 6e4, dtype=dt, device=DEV)
        wide[:, :K] = x.to(DEV)
        bq, q = guarded_bytes(M * K)
        bs, s = guarded_bytes(M * (K // 32))
        ops.mxfp8_quantize_rows(wide[:, :K], out=(q, s))
        torch.cuda.synchronize()
        assert torch.equal(s.cpu().view(M, K // 32), hs), f"ld={ld}: {int((s.cpu().view(M, -1) != hs).sum())} scale bytes differ from the host entry"
        assert torch.equal(q.cpu().view(M, K), hq), f"ld={ld}: {int((q.cpu().view(M, K) != hq).sum())} element bytes differ from the host entry"
        assert untouched_bytes(bq, M * K) and untouched_bytes(bs, M * (K // 32))


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("N,K", [(16, 128), (17, 128), (40, 384), (272, 1024), (300, 3072)])
def test_device_packer_equals_the_host_entry(dt, N, K):
    w = weight_rows(N, K, dt)
    host = ops.pack_weight_mx(w)
    for ld in (K, K + 24):
        wide = torch.full((N, ld), 3e4, dtype=dt, device=DEV)
        wide[:, :K] = w.to(DEV)
        buf, img = guarded_bytes(host.numel())
        ops.pack_weight_mx(wide[:, :K], out=img)
        torch.cuda.synchronize()
        assert torch.equal(img.cpu(), host), f"ld={ld}: device packer differs from sl_pack_weight_mx_host"
        assert untouched_bytes(buf, host.numel())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. exact products
# ------------------------------------------------------------------------------------------------------------------------------
MS, NS, KS = [1, 15, 16, 17, 127, 128, 129, 300], [16, 48, 128, 144, 272], [128, 256, 1024]


@functools.lru_cache(maxsize=1)
def _exact_operands():
    """A: integers in [-8, 8] as e4m3 bytes, scale exponents in {0, 1, 2}; W: e2m1 codes, scale exponents in {0, 1, 2}"""
    g = torch.Generator().manual_seed(77)
    M, N, K = max(MS), max(NS), max(KS)
    a = torch.randint(-8, 9, (M, K), generator=g).double()
    Aq = e4m3_bytes(a)
    As = (127 + torch.randint(0, 3, (M, K // 32), generator=g)).to(torch.uint8)
    code = torch.randint(0, 16, (N, K), generator=g).numpy().astype(np.uint8)
    code[code == 8] = 0                                                   # no negative zero
    sc = (127 + torch.randint(0, 3, (N, K // 32), generator=g)).numpy().astype(np.uint8)
    A64, W64 = dq_a(Aq, As), dq_w(code, sc)
    # the precondition: every product is a multiple of .5 (integer x multiple of .5, scales >= 1), and the sum of magnitudes, counted in
    # that step, stays below 2^24 for every output — so every partial sum in ANY order is an integer below 2^24 in that unit: exact in fp32
    assert float((A64.abs() @ W64.abs().T).max()) / 0.5 < 2 ** 24
    assert torch.equal(A64 * 2, (A64 * 2).round()) and torch.equal(W64 * 2, (W64 * 2).round())
    return Aq, As, code, sc, A64, W64


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_exact_products(M, K):
    Aq, As, code, sc, A64, W64 = _exact_operands()
    for N in NS:
        img = image(code[:N, :K], sc[:N, :K // 32])
        ref = A64[:M, :K] @ W64[:N, :K].T
        for dt, out_dtype in ((BF16, F32), (BF16, BF16), (F16, F16)):
            got, ok = run(Aq[:M, :K].contiguous(), As[:M, :K // 32].contiguous(), img, N, dt, out_dtype)
            want = ref.float() if out_dtype == F32 else ref.float().to(out_dtype)      # ref is exact in fp32: ONE rounding to the 16-bit type
            assert torch.equal(got, want), f"M={M} N={N} K={K} {out_dtype}: {int((got != want).sum())} outputs differ from the exact product"
            assert ok, f"M={M} N={N} K={K} {out_dtype}: guard band written"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. random products against fp64, at the derived bound
# ------------------------------------------------------------------------------------------------------------------------------
HALF_ULP = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}     # relative to the binade
MIN_HALF_ULP = {F32: 2.0 ** -150, BF16: 2.0 ** -134, F16: 2.0 ** -25}


def half_ulp(mag, dtype):
    """half an ulp of dtype at magnitude mag (fp64 tensor): 2^floor(log2 mag) * HALF_ULP, not below half the smallest subnormal step"""
    ex = torch.floor(torch.log2(mag.clamp(min=1e-300)))
    return torch.maximum(torch.exp2(ex) * HALF_ULP[dtype], torch.full_like(mag, MIN_HALF_ULP[dtype]))


def acc_bound(A64, W64, K):
    return K * 2.0 ** -23 * (A64.abs() @ W64.abs().T)


@functools.lru_cache(maxsize=8)
def _random_operands(M, N, K, dt):
    g = torch.Generator().manual_seed(M * 13 + N * 7 + K)
    magx = 2.0 ** ((torch.arange(K // 32)[None, :] + torch.arange(M)[:, None]) % 7 - 3).float()
    x = (torch.randn(M, K // 32, 32, generator=g) * magx[:, :, None]).view(M, K).to(dt)
    magw = 2.0 ** ((torch.arange(K // 32)[None, :] * 2 + torch.arange(N)[:, None]) % 9 - 4).float()
    w = (torch.randn(N, K // 32, 32, generator=g) * K ** -0.5 * magw[:, :, None]).view(N, K).to(dt)
    q, s = ops.mxfp8_quantize_rows(x.to(DEV))
    img = ops.pack_weight_mx(w.to(DEV))
    return q, s, img, dq_a(q, s), ops.mx_dequantise(img, N, K)


@pytest.mark.parametrize("M,N,K,dt,out_dtype", [(300, 1040, 3072, BF16, BF16), (129, 272, 1024, F16, F16), (17, 144, 384, BF16, F32), (1, 48, 256, F16, F16),
                                                (128, 128, 128, BF16, BF16)])
def test_random_products_within_the_derived_bound(M, N, K, dt, out_dtype):
    q, s, img, A64, W64 = _random_operands(M, N, K, dt)
    got, ok = run(q, s, img, N, dt, out_dtype)
    ref = A64 @ W64.T
    acc = acc_bound(A64, W64, K)
    bound = acc + half_ulp(ref.abs() + acc, out_dtype)
    err = (got.double() - ref).abs()
    print(f"mx product M={M} N={N} K={K} {out_dtype}: rel_err {rel_err(got, ref):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} outputs beyond the bound, worst ratio {float((err / bound).max()):.3f}"
    assert ok


# ------------------------------------------------------------------------------------------------------------------------------
# 5. epilogues
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [17, 129])
def test_silu_mul_epilogue(dt, M):
    """N = 2 F rows in blocks of 16 gate rows followed by their 16 up rows: C[m][16 p + c] = silu(gate) * up.  The fp64 reference pushed
    through the epilogue: with g, u the fp32 sums (within their product bounds bg, bu of the fp64 ones), |silu'| <= 1.1, the error of
    silu(g) u is at most 1.1 bg (|u| + bu) + |silu(g)| bu, plus the epilogue's own fp32 arithmetic — the hardware exponential of
    g log2(e) errs by about |g| 2^-23 relative, the division and the product by 2^-23 each: (|g| + 4) 2^-23 |v| — plus half an ulp."""
    K, Fd = 384, 144
    q, s, img, A64, W64 = _random_operands(M, 2 * Fd, K, dt)
    W3 = W64.view(Fd // 16, 2, 16, K)
    g, u = A64 @ W3[:, 0].reshape(Fd, K).T, A64 @ W3[:, 1].reshape(Fd, K).T
    full = acc_bound(A64, W64, K).view(M, Fd // 16, 2, 16)
    bg, bu = full[:, :, 0].reshape(M, Fd), full[:, :, 1].reshape(M, Fd)
    sg = g * torch.sigmoid(g)
    ref = sg * u
    tol = 1.1 * bg * (u.abs() + bu) + sg.abs() * bu + (g.abs() + 4) * 2.0 ** -23 * ref.abs()
    for out_dtype in (dt, F32):
        got, ok = run(q, s, img, 2 * Fd, dt, out_dtype, act=L.ACT_SILU_MUL)
        bound = tol + half_ulp(ref.abs() + tol, out_dtype)
        err = (got.double() - ref).abs()
        print(f"mx silu.mul M={M} {out_dtype}: worst err / bound {float((err / bound).max()):.3f}")
        assert got.shape == (M, Fd) and bool((err <= bound).all()), float((err / bound).max())
        assert ok


@pytest.mark.parametrize("dt", DT16)
def test_residual_in_place_and_f32_output(dt):
    M, N, K = 129, 272, 1024
    q, s, img, A64, W64 = _random_operands(M, N, K, dt)
    res = (torch.randn(M, N, generator=torch.Generator().manual_seed(5)) * 2).to(dt)
    ref = A64 @ W64.T + res.double()
    acc = acc_bound(A64, W64, K) + 2.0 ** -23 * ref.abs()                 # + the fp32 addition of the residual
    # in place: C == residual
    buf, out = guarded(M, N, dt)
    out.copy_(res.to(DEV))
    ops.gemm_mx(q, s, img, N, dtype=dt, residual=out, out=out)
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    bound = acc + half_ulp(ref.abs() + acc, dt)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert untouched(buf, M, N)
    # fp32 output with a 16-bit residual held elsewhere (row stride of its own)
    rbuf, rview = guarded(M, N, dt)
    rview.copy_(res.to(DEV))
    got, ok = run(q, s, img, N, dt, F32, residual=rview)
    err = (got.double() - ref).abs()
    bound = acc + half_ulp(ref.abs() + acc, F32)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert ok
    chk = rbuf.clone()
    chk[1:M + 1, 8:8 + N] = FILL
    assert bool((chk == FILL).all()) and torch.equal(rview.cpu(), res), "the residual was written"


# ------------------------------------------------------------------------------------------------------------------------------
# 6. a row's result does not depend on M
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,out_dtype", [(BF16, BF16), (F16, F32)])
def test_row_independence(dt, out_dtype):
    M, N, K = 300, 1040, 3072
    q, s, img, _, _ = _random_operands(M, N, K, BF16)      # the operands are bytes: dt is the output's type only
    full, ok = run(q, s, img, N, dt, out_dtype)
    assert ok
    bits = torch.int32 if out_dtype == F32 else torch.int16
    for r in (0, 127, 128, 299):
        one, ok = run(q[r:r + 1].contiguous(), s[r:r + 1].contiguous(), img, N, dt, out_dtype)
        assert ok and torch.equal(one.view(bits), full[r:r + 1].view(bits)), f"row {r}: alone != inside the batch of {M}"


# ------------------------------------------------------------------------------------------------------------------------------
# 7 - 10. the model (TINY_LLAMA)
# ------------------------------------------------------------------------------------------------------------------------------
from oracle import llama_oracle as lo                                                       # noqa: E402
from oracle.golden_cfgs import TINY_LLAMA                                                   # noqa: E402
from test_w8_gpu import _BASE_LENS, _NEXT, _make_llama, _prefill_and_step, _prompts         # noqa: E402

MAX_CTX = 128


def _ragged_prompts(cfg, B, P=0, seed=8):
    """B prompts of the five base lengths; with P > 0 their first P rows are the same rows"""
    gen = torch.Generator().manual_seed(seed)
    base = [torch.randn(n, cfg.hidden_size, generator=gen) * 0.05 for n in _BASE_LENS]
    out = [base[b % 5].clone() * (1.0 + 0.01 * (b // 5)) for b in range(B)]
    for p in out:
        p[:P] = base[0][:P]
    return out


def _compose_layers(llm, x, kc, vc, tok_seq, tok_pos, attn, last_rows=None):
    """the decoder stack out of the public ops: rmsnorm -> quantise -> MX product -> RoPE / append -> attention -> quantise -> o + residual
    -> rmsnorm -> quantise -> gate/up + SiLU.mul -> quantise -> down + residual; the final layer's tail on last_rows only, like prefill"""
    w, a, dt = llm._dev(), llm.arch, llm.dtype
    H, D, nh, nkv, Fd = a.hidden_size, a.head_dim, a.num_attention_heads, a.num_key_value_heads, a.intermediate_size
    qkv_w = (nh + 2 * nkv) * D
    mx = lambda t, img, N, **kw: ops.gemm_mx(*ops.mxfp8_quantize_rows(t), img, N, dtype=dt, **kw)
    for li in range(a.num_hidden_layers):
        t, imgs = w.layer_t[li], w.mx_images[li]
        qkv = mx(ops.rmsnorm(x, t["norm1"], a.rms_norm_eps), imgs["qkv"], qkv_w)
        ops.rope_kv_append(qkv, kc[li], vc[li], tok_seq, tok_pos, w.rope_cos, w.rope_sin, nh, nkv, D, llm.max_ctx)
        att = attn(li, qkv)
        if last_rows is not None and li == a.num_hidden_layers - 1:
            att, x = att[last_rows].contiguous(), x[last_rows].contiguous()
        x = mx(att, imgs["o"], H, residual=x)
        mid = mx(ops.rmsnorm(x, t["norm2"], a.rms_norm_eps), imgs["gu"], 2 * Fd, act=L.ACT_SILU_MUL)
        x = mx(mid, imgs["down"], H, residual=x)
    return x


def _compose_prefill(llm, prompts):
    """-> (logits (B, vocab) fp32, k cache, v cache) of the composition, on zeroed caches of the model's shape"""
    w, a, dt = llm._dev(), llm.arch, llm.dtype
    D, nh, nkv = a.head_dim, a.num_attention_heads, a.num_key_value_heads
    B, lens = len(prompts), [int(p.shape[0]) for p in prompts]
    x = torch.cat([p.to(DEV, dt) for p in prompts]).contiguous()
    kc, vc = torch.zeros_like(llm._kv[0]), torch.zeros_like(llm._kv[1])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    tok_seq, tok_pos = i32(sum([[s] * n for s, n in enumerate(lens)], [])), i32(sum([list(range(n)) for n in lens], []))
    cu_q, row0, klen = i32(cu), i32([s * nkv * llm.max_ctx for s in range(B)]), i32(lens)
    qkv_w = (nh + 2 * nkv) * D

    def attn(li, qkv):
        out = torch.empty((x.shape[0], nh * D), device=DEV, dtype=dt)
        ops.attn_fwd(qkv, kc[li], vc[li], out, cu_q, row0, klen, q_strides=(qkv_w, D), k_strides=(D, llm.max_ctx * D), v_strides=(D, llm.max_ctx * D),
                     o_strides=(nh * D, D), nseq=B, max_qlen=max(lens), n_heads=nh, n_kv_heads=nkv, head_dim=D, causal=True, scale=D ** -0.5)
        return out

    last = _compose_layers(llm, x, kc, vc, tok_seq, tok_pos, attn, last_rows=torch.tensor([c - 1 for c in cu[1:]], device=DEV))
    logits = ops.gemm(ops.rmsnorm(last, w.final_norm, a.rms_norm_eps), w.lm_head, out_f32=True)
    torch.cuda.synchronize()
    return logits.cpu(), kc[:, :B].cpu(), vc[:, :B].cpu()


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


@pytest.mark.parametrize("dt", DT16)
def test_model_wiring_prefill_and_decode_step_equal_the_composition_of_public_ops(dt):
    """sl_llama_prefill on struct_mx over five ragged prompts, shared_prefix off and on, and one sl_llama_decode_step at B = 1, 3, 27:
    logits and the WHOLE K/V cache bit-identical to the composition of the public ops above.  (pack_decode=False: the lm_head of the
    decode step is then the row-major product the composition can name; the packed lm_head runs in the generation tests.)"""
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 33, dt, max_ctx=MAX_CTX, linear_dtype="mx", pack_decode=False)
    w, a = llm._dev(), llm.arch
    assert w.struct_mx.reserved == L.WDEC_MX_LINEAR and w.struct.reserved == L.WDEC_MODEL_DTYPE
    lib = L.lib()
    for P in (0, 4):
        prompts = _ragged_prompts(cfg, 5, P)
        kv = llm._kv_cache(5, P)
        pl, pc, _ = _prefill_with(llm, w.struct_mx, prompts, kv)
        cl, ck, cv = _compose_prefill(llm, prompts)
        assert torch.equal(_bits(pc[0]), _bits(ck)) and torch.equal(_bits(pc[1]), _bits(cv)), f"shared_prefix={P}: the K/V cache differs from the composition"
        assert torch.equal(_bits(pl), _bits(cl)), f"shared_prefix={P}: prefill logits differ from the composition"
    for B in (1, 3, 27):
        prompts, nxt = _ragged_prompts(cfg, B), [_NEXT[b % 5] for b in range(B)]
        _, pc, dl = _prefill_and_step(llm, w.struct_mx, prompts, nxt)
        after = (llm._kv[0][:, :B].cpu(), llm._kv[1][:, :B].cpu())
        kc, vc = torch.zeros_like(llm._kv[0]), torch.zeros_like(llm._kv[1])
        kc[:, :B], vc[:, :B] = pc[0].to(DEV), pc[1].to(DEV)
        lens = torch.tensor([int(p.shape[0]) for p in prompts], dtype=torch.int32, device=DEV)
        x = ops.embed_gather(w.embed, torch.tensor(nxt, dtype=torch.int32, device=DEV))
        D, nh, nkv = a.head_dim, a.num_attention_heads, a.num_key_value_heads
        qkv_w = (nh + 2 * nkv) * D
        attn = lambda li, qkv: ops.attn_decode_split(qkv, qkv_w, kc[li], vc[li], lens + 1, nh, nkv, D, llm.max_ctx, D ** -0.5)
        last = _compose_layers(llm, x, kc, vc, torch.arange(B, dtype=torch.int32, device=DEV), lens, attn)
        logits = ops.gemm(ops.rmsnorm(last, w.final_norm, a.rms_norm_eps), w.lm_head, out_f32=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(after[0]), _bits(kc[:, :B].cpu())) and torch.equal(_bits(after[1]), _bits(vc[:, :B].cpu())), f"B={B}: cache after the step"
        assert torch.equal(_bits(dl), _bits(logits.cpu())), f"B={B}: decode-step logits differ from the composition"


def _prefill_with(llm, struct, prompts, kv):
    """sl_llama_prefill of `struct` on the cache struct `kv` (zeroed first) -> (logits, (k, v) of the B slots, ctx_len device tensor)"""
    lib, B = L.lib(), len(prompts)
    x = torch.cat([p.to(DEV, llm.dtype) for p in prompts]).contiguous()
    cu = [0]
    for p in prompts:
        cu.append(cu[-1] + p.shape[0])
    llm._kv[0].zero_(); llm._kv[1].zero_()
    ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(struct), x.shape[0], B, 1))
    logits = torch.empty((B, llm.arch.vocab_size), device=DEV, dtype=torch.float32)
    ctx = torch.empty(B, device=DEV, dtype=torch.int32)
    L.check(lib.sl_llama_prefill(C.byref(struct), C.byref(kv), x.data_ptr(), (C.c_int32 * (B + 1))(*cu), B, logits.data_ptr(), ctx.data_ptr(),
                                 None, ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
    torch.cuda.synchronize()
    return logits.cpu(), (llm._kv[0][:, :B].cpu(), llm._kv[1][:, :B].cpu()), ctx


class _MxF:
    """torch.nn.functional with `linear` passing its input through the HOST MXFP8 quantise / dequantise (rounded to the model dtype first, as
    the device rounds what it quantises) when the weight is one of the projection matrices given; every other call is F's"""

    def __init__(self, real, weights_, dt):
        self._real, self._ptrs, self._dt = real, {t.data_ptr() for t in weights_}, dt

    def __getattr__(self, name):
        return getattr(self._real, name)

    def linear(self, x, weight, bias=None):
        if weight.data_ptr() in self._ptrs:
            q, s = ops.mxfp8_quantize_rows(x.reshape(-1, x.shape[-1]).to(self._dt).contiguous())
            x = ops.mxfp8_dequantise(q, s).float().view(x.shape)
        return self._real.linear(x, weight, bias)


# rel_err(GPU decode-step logits, patched oracle), worst over both dtypes, B in {1, 3, 27} and the sequences checked, MEASURED once on the
# MI355X; the assertion is at twice that.  The oracle works in fp32 and the device rounds activations to 16 bits before it quantises
# them, so a few e4m3 roundings flip: the distance is not a rounding bound and is therefore taken from a measurement.
MODEL_ERR_SEEN = 2.582e-2                # bf16, B = 27 (fp16 worst: 1.886e-2); the MX model itself is 1.3e-1 .. 1.4e-1 from the original weights
MODEL_ERR_FACTOR = 2.0


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B", [1, 3, 27])
def test_model_arithmetic_against_the_patched_oracle(dt, B, monkeypatch):
    cfg = TINY_LLAMA
    llm, sd = _make_llama(cfg, 33, dt, max_ctx=MAX_CTX, linear_dtype="mx")
    w = llm._dev()
    prompts, nxt = _ragged_prompts(cfg, B), [_NEXT[b % 5] for b in range(B)]
    _, pc, dl = _prefill_and_step(llm, w.struct_mx, prompts, nxt)
    sdq = w.mx_dequantised_state_dict()
    sdo = {k: v.to(dt).float() for k, v in sd.items()}
    proj = [v for k, v in sdq.items() if k.endswith("_proj.weight")]
    assert len(proj) == 7 * cfg.num_hidden_layers
    embed = sdo["model.embed_tokens.weight"]
    worst, cost = 0.0, []
    for b in range(min(B, 5)):
        n = prompts[b].shape[0]
        past = [(pc[0][l, b, :, :n].float()[None], pc[1][l, b, :, :n].float()[None]) for l in range(cfg.num_hidden_layers)]
        tok = embed[nxt[b]][None, None]
        ref_o = lo.llama_forward(sdo, cfg, tok, past=past, last_logits_only=True)["logits"][0, -1]
        with monkeypatch.context() as mp:
            mp.setattr(lo, "F", _MxF(lo.F, proj, dt))
            ref_q = lo.llama_forward(sdq, cfg, tok, past=past, last_logits_only=True)["logits"][0, -1]
        e, d = rel_err(dl[b], ref_q), rel_err(ref_q, ref_o)
        worst = max(worst, e)
        cost.append(d)
        assert e < 0.25 * d, f"row {b}: the device is {e:.3e} from the MX model and the MX model only {d:.3e} from the original: not THIS model"
    print(f"mx decode step {dt} B={B}: rel_err(GPU, patched oracle) worst {worst:.3e}; rel_err(patched oracle, original weights) {['%.2e' % d for d in cost]}")
    assert MODEL_ERR_SEEN is not None, "the measured distance has not been recorded"
    assert worst < MODEL_ERR_FACTOR * MODEL_ERR_SEEN, worst


def _step_loop(llm, struct, x, lens, n_new, penalty=1.0):
    """greedy ids by sl_llama_prefill + a loop over sl_llama_decode_step on `struct` -> (B, n_new) int32; penalty: HF's repetition penalty
    over each row's generated tokens (tests/logits_proc_ref.py) in front of the argmax"""
    from logits_proc_ref import repetition_penalty

    def select(lg, hist):
        lg = lg.cpu()
        rows = [repetition_penalty(lg[b], [int(t[b]) for t in hist], penalty) for b in range(lg.shape[0])]
        return torch.stack(rows).argmax(-1).to(torch.int32)
    lib, B = L.lib(), len(lens)
    prompts, o = [], 0
    for n in lens:
        prompts.append(x[o:o + n])
        o += n
    kv = llm._kv_cache(B)
    logits, _, ctx = _prefill_with(llm, struct, prompts, kv)
    ws = llm._workspace(0)
    ids = [select(logits, [])]
    dl = torch.empty((B, llm.arch.vocab_size), device=DEV, dtype=torch.float32)
    for _ in range(n_new - 1):
        nid = ids[-1].to(DEV)
        L.check(lib.sl_llama_decode_step(C.byref(struct), C.byref(kv), nid.data_ptr(), ctx.data_ptr(), B, dl.data_ptr(), ws.data_ptr(), ws.numel(),
                                         L.stream_ptr()), "sl_llama_decode_step")
        ctx += 1
        ids.append(select(dl, ids))
    return torch.stack(ids, 1)


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("B", [3, 27])
def test_generate_gives_the_ids_of_the_step_by_step_loop(B, kv_dtype):
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, max_ctx=MAX_CTX, linear_dtype="mx", kv_cache_dtype=kv_dtype)
    x, lens = _prompts(cfg, B)
    new = 10
    want = _step_loop(llm, llm._dev().struct_mx, x.clone(), lens, new)
    ids, _ = llm.generate_packed(x.clone(), lens, new, use_eos=False)
    assert llm.last_generate_stats["weight_format"] == "mx"
    assert torch.equal(ids[:, :new], want), "generate (captured graphs) != the loop over sl_llama_decode_step"
    ids_s, _, lps = llm.generate_packed(x.clone(), lens, new, use_eos=False, scores=True)
    assert torch.equal(ids_s[:, :new], want) and bool((lps[:, :new] <= 0).all()) and bool(torch.isfinite(lps[:, :new]).all())
    want_p = _step_loop(llm, llm._dev().struct_mx, x.clone(), lens, new, penalty=1.3)
    ids_p, _ = llm.generate_packed(x.clone(), lens, new, use_eos=False, logits=dict(repetition_penalty=1.3))
    assert torch.equal(ids_p[:, :new], want_p), "greedy + repetition_penalty != the loop with HF's penalty in front of the argmax"
    assert not torch.equal(want_p, want), "the penalty changed nothing: the case checks nothing"


def test_generate_compaction_and_a_second_session_turn():
    cfg = TINY_LLAMA
    llm, _ = _make_llama(cfg, 35, BF16, max_ctx=MAX_CTX, linear_dtype="mx")
    B, new = 27, 12
    x, lens = _prompts(cfg, B)
    limits = [2 + (7 * b) % 11 for b in range(B)]
    llm.generation_config.eos_token_id = None
    ref, n_ref = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=False)
    ids, n = llm.generate_packed(x.clone(), lens, new, use_eos=False, row_limits=limits, compact=True, check_every=2)
    assert llm.last_generate_stats["weight_format"] == "mx" and llm.last_generate_stats["compactions"] >= 2
    assert n == n_ref and torch.equal(ids[:, :n], ref[:, :n_ref])
    want = _step_loop(llm, llm._dev().struct_mx, x.clone(), lens, new)
    for b in range(B):
        assert torch.equal(ids[b, :limits[b]], want[b, :limits[b]]), b
    # a second turn in a session: the continued call equals one call over the concatenated rows
    x3, l3 = _prompts(cfg, 3)
    sess = llm.new_session(3)
    a1, _ = llm.generate_packed(x3.clone(), l3, 4, use_eos=False, session=sess)
    more = torch.cat([t for t in _ragged_prompts(cfg, 3, seed=21)]).to(DEV, BF16)
    l2 = [int(n) for n in _BASE_LENS[:3]]
    a2, _ = llm.generate_packed(more.clone(), l2, 5, use_eos=False, session=sess)
    assert llm.last_generate_stats["weight_format"] == "mx"
    emb = llm.model.embed_tokens
    parts, o3, o2 = [], 0, 0
    for s in range(3):
        parts += [x3[o3:o3 + l3[s]], emb(a1[s, :4].to(DEV)).to(BF16), more[o2:o2 + l2[s]]]
        o3 += l3[s]
        o2 += l2[s]
    whole = _step_loop(llm, llm._dev().struct_mx, torch.cat(parts).contiguous(), [l3[s] + 4 + l2[s] for s in range(3)], 5)
    assert torch.equal(a2[:, :5], whole), "second turn != the loop over the concatenated rows"


def test_switching_mx_off_and_on_and_the_option_unset():
    """mx -> off -> mx on one model returns the ids of models that never held the other setting (a shared captured graph would not); with
    the option unset _struct_for returns what it returned, and the decode graph captured before the switch is the one replayed after it"""
    cfg = TINY_LLAMA
    x3, l3 = _prompts(cfg, 3)
    want = {}
    for name, kw in (("16-bit", {}), ("mx", dict(linear_dtype="mx"))):
        fresh, _ = _make_llama(cfg, 35, BF16, max_ctx=MAX_CTX, **kw)
        want[name], _ = fresh.generate_packed(x3.clone(), l3, 12, use_eos=False)
        assert fresh.last_generate_stats["weight_format"] == name
        del fresh
    llm, _ = _make_llama(cfg, 35, BF16, max_ctx=MAX_CTX)
    w = llm._dev()
    s0, n0 = llm._struct_for(3)
    assert s0 is w.struct and n0 == "16-bit" and getattr(w, "struct_mx", None) is None
    ids, _ = llm.generate_packed(x3.clone(), l3, 12, use_eos=False)
    assert torch.equal(ids, want["16-bit"])
    ws_ptr, ws_len = llm._ws.data_ptr(), llm._ws.numel()      # the decode graph cache is keyed by the workspace (and the struct): both must survive the switch
    for ld, name in (("mx", "mx"), (None, "16-bit"), ("mxfp8_mxfp4", "mx"), (None, "16-bit")):
        llm.set_linear_dtype(ld)
        s, n = llm._struct_for(3)
        assert n == name and (s is w.struct_mx if name == "mx" else s is w.struct)
        ids, _ = llm.generate_packed(x3.clone(), l3, 12, use_eos=False)
        assert llm.last_generate_stats["weight_format"] == name
        assert torch.equal(ids, want[name]), f"{name}: ids differ from those of a model that only ever held this setting"
        assert (llm._ws.data_ptr(), llm._ws.numel()) == (ws_ptr, ws_len) and llm._struct_for(3)[0] is s, "the 16-bit calls' workspace moved: their captured graph is lost"
    for entry in ("beam", "generate_n", "score"):
        llm.set_linear_dtype("mx")
        with pytest.raises(L.SpeechLLMError, match="linear_dtype='mx' does not run"):
            llm._struct_for(3, entry)
    with pytest.raises(L.SpeechLLMError):
        llm.generate_packed(x3.clone(), l3, 4, use_eos=False, beams=dict(num_beams=2))
