"""GPU: every kernel form in fp16 / bf16 / fp32 at the shapes that break kernels, checked PER ELEMENT.

Four kinds of input ("edge suite"):
  E  exact integers: A, W in {-2..2}, bias in [-8, 8], residual 8 x [-512, 512].  Every partial sum is an integer below 2^17, so fp32
     accumulation is exact in any order, under any K split and through fp32 partial records; the only rounding is the output's
     round-to-nearest-even, which is torch's.  torch.equal.  Two fp16 scalings of E (x 64: overflow to +-inf; x 2^-12: subnormal
     outputs) pin common.h's "as torch's .half() does" on every store path.
  G  Gaussian, against fp64 on the same rounded inputs: |got - ref| <= 2u |ref| + K 2^-24 mag + 2^-24 with u the output type's
     half-ulp (2^-11 fp16, 2^-8 bf16, 2^-24 fp32) and mag = |A| |W|^T + |b| + |R| (twice the output rounding + the worst-case fp32
     accumulation error of any summation order).  GELU / SiLU-mul propagate the accumulation term through the activation.
  P  attention mask probe: V[j, j mod D] = 1, so out[i, d] is the probability mass on the visible keys j = d (mod D): exact zeros
     where no such key is visible, and |got - ref| <= 2u |ref| + 4u (P |V|) + nk 2^-24 elsewhere (P rounded to the storage type,
     the output rounding, subnormal probabilities).
  Guard bands and poison, in every case: outputs are views into sentinel-filled buffers (a row above and below, 8 elements left and
  right) that must come back untouched; A and W are views with lda / ldw > K whose pad columns and trailing rows hold large finite
  values; KV-cache positions behind ctx_len and packed K / V rows behind klen hold 8.0 (K) and a large value (V).  The poison is
  finite: 0 x finite = 0, so this tests predicates and index clamps, not a NaN contract.
  T  attention in training mode (the last section): sl_attn_bwd in every form and sl_attn_fwd's lse / dropout outputs against
     tests/attn_train_ref.py: probes with exact zeros in dV, dQ and out, Gaussian inputs under per-element bounds, the dropout mask
     restated on the host at exactly the indices a case touches, dq / dk / dv in three guarded buffers.
No tolerance here is a measured number - with one exception, stated where it is used: the allowance for the exponential and the logarithm
in the bound on lse - and nothing compares two forms of a kernel with each other only.
"""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import attn_train_ref as R
from conftest import pkg, rel_err
from edge_helpers import (BF16, BIG, DEV, DT16, DTS, E24, F16, F32, FILL, U, _gen, _set, bad, gauss, guarded, ints, operand, to_dt, tuning,  # noqa: F401
                          untouched, vec)

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
weights = pkg("weights")

NONE, GELU, SILU, ROPE = L.ACT_NONE, L.ACT_GELU, L.ACT_SILU_MUL, L.ACT_ROPE_KV


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def halves(y):
    """gate / up of a product against a weight stored in [16 gate | 16 up] row blocks"""
    M, N2 = y.shape
    y = y.reshape(M, N2 // 32, 2, 16)
    return y[:, :, 0].reshape(M, N2 // 2), y[:, :, 1].reshape(M, N2 // 2)


def silu_mul_bound(y, e, u_out):
    """ref and tolerance of silu(g) * u when g and u each carry an absolute error bound e (same layout as y)"""
    g, up = halves(y)
    eg, eu = halves(e)
    s = g * torch.sigmoid(g)
    ref = s * up
    tol = 2 * u_out * ref.abs() + 1.1 * eg * up.abs() + s.abs() * eu + eg * eu + 2e-6 * (1 + ref.abs()) + E24
    return ref, tol


def check_exact(run, M, N, K, dt, seed, bias=True, residual=True, scalings=True):
    """class E through `run(a, w, bias=, res=, out_f32=)`; run returns the output (guard bands already checked)."""
    a, a64 = operand(ints((M, K), -2, 2, seed), dt)
    w, w64 = operand(ints((N, K), -2, 2, seed + 1), dt)
    r, r64 = operand(8 * ints((M, N), -512, 512, seed + 3), dt)
    b, b64 = vec(ints((N,), -8, 8, seed + 2), dt)
    y = a64 @ w64.T
    cases = [("plain", {}, y), ("out_f32", dict(out_f32=True), y)]
    if residual:
        cases.append(("residual", dict(res=r), y + r64))
    if bias:
        cases.append(("bias", dict(bias=b), y + b64))
    if bias and residual:
        cases.append(("bias+residual", dict(bias=b, res=r), y + b64 + r64))
    for name, kw, want in cases:
        got = run(a, w, **kw)
        msg = bad(got, to_dt(want, got.dtype))
        assert not msg, f"E {name} {(M, N, K)}: {msg}"
    if dt == F16 and scalings:
        for name, s in (("overflow", 64.0), ("subnormal", 2.0 ** -12)):
            a2, a264 = operand(a64 * s, dt)
            w2, w264 = operand(w64 * s, dt)
            want = to_dt(a264 @ w264.T, dt)
            if name == "overflow":
                assert bool(want.isinf().any()) and not bool(want.isnan().any())
            else:
                assert float(want.abs().max()) < 2.0 ** -14 and bool((want != 0).any())
            msg = bad(run(a2, w2), want, bits=True)          # the bits of torch's .half(): +-inf with its sign, subnormals kept, +-0
            assert not msg, f"E {name} {(M, N, K)}: {msg}"


def check_gauss(run, M, N, K, dt, seed, gelu=True, silu=True, bias=True):
    """class G through `run(a, w, bias=, res=, act=)`"""
    a, a64 = operand(gauss((M, K), seed), dt)
    w, w64 = operand(gauss((N, K), seed + 1, K ** -0.5), dt)
    r, r64 = operand(gauss((M, N), seed + 3), dt)
    b, b64 = vec(gauss((N,), seed + 2), dt)
    if not bias:
        b, b64 = None, torch.zeros(N, dtype=torch.float64)
    y, mag = a64 @ w64.T, a64.abs() @ w64.abs().T
    u = U[dt]
    ref = y + b64 + r64
    tol = 2 * u * ref.abs() + K * E24 * (mag + b64.abs() + r64.abs()) + E24
    msg = bad(run(a, w, bias=b, res=r), ref, tol)
    assert not msg, f"G bias+residual {(M, N, K)}: {msg}"
    acc = K * E24 * mag + E24
    msg = bad(run(a, w), y, 2 * u * y.abs() + acc)
    assert not msg, f"G plain {(M, N, K)}: {msg}"
    msg = bad(run(a, w, out_f32=True), y, 2 * U[F32] * y.abs() + acc)
    assert not msg, f"G out_f32 {(M, N, K)}: {msg}"
    if bias:
        ref = y + b64
        msg = bad(run(a, w, bias=b), ref, 2 * u * ref.abs() + K * E24 * (mag + b64.abs()) + E24)
        assert not msg, f"G bias {(M, N, K)}: {msg}"
    if gelu:
        pre = y + b64
        ref = gelu64(pre)
        tol = 2 * u * ref.abs() + 1.13 * K * E24 * (mag + b64.abs()) + 2e-6 * (1 + pre.abs()) + E24
        msg = bad(run(a, w, bias=b, act=GELU), ref, tol)
        assert not msg, f"G gelu {(M, N, K)}: {msg}"
    if silu and N % 32 == 0:
        ref, tol = silu_mul_bound(y, K * E24 * mag, u)
        msg = bad(run(a, w, act=SILU), ref, tol)
        assert not msg, f"G silu_mul {(M, N, K)}: {msg}"


def rowmajor(M, N, K, dt, **extra):
    """run() for ops.gemm_ex on guarded outputs"""
    def run(a, w, bias=None, res=None, act=NONE, out_f32=False):
        n_out = N // 2 if act == SILU else N
        buf, out = guarded(M, n_out, F32 if out_f32 else dt)
        ops.gemm_ex(a, w, M=M, N=N, K=K, lda=a.stride(0), ldw=w.stride(0), out=out, ldc=out.stride(0), bias=bias, residual=res,
                    ldr=res.stride(0) if res is not None else 0, act=act, out_f32=out_f32, dtype=dt, **extra)
        assert untouched(buf, M, n_out), "write outside [0:M, 0:n_out]"
        return out
    return run


def pack_strided(w):
    """ops.pack_weight for a view: sl_pack_weight itself takes ldw (the wrapper only accepts contiguous tensors)"""
    n, k = w.shape
    out = torch.empty(((n + 15) // 16 * 16, k), device=w.device, dtype=w.dtype)
    L.check(L.lib().sl_pack_weight(L.ptr(w), w.stride(0), L.ptr(out), n, k, L.dtype_code(w.dtype), L.stream_ptr()), "sl_pack_weight")
    return out


def top1_strided(a_, w_, bias=None):
    """ops.gemm_top1 for views with lda / ldw > K (the same sl_gemm_ex call; the wrapper only accepts contiguous tensors)"""
    (M, K), N = a_.shape, w_.shape[0]
    ng = (N + 63) // 64
    val = torch.empty((ng, M), device=DEV, dtype=F32)
    idx = torch.empty((ng, M), device=DEV, dtype=torch.int32)
    a = L.GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = L.ptr(a_), a_.stride(0), L.ptr(w_), w_.stride(0), None, N
    a.bias = L.ptr(bias)
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.dtype, a.act, a.out_f32 = L.dtype_code(a_.dtype), NONE, 1
    ex = L.GemmEx()
    ex.w_mod, ex.amax_val, ex.amax_idx = 1, L.ptr(val), L.ptr(idx)
    L.check(L.lib().sl_gemm_ex(C.byref(a), C.byref(ex), L.stream_ptr()), "sl_gemm_ex")
    return val, idx


def packed(M, N, K, dt, **extra):
    """run() for ops.gemm_decode (fragment-packed weight) on guarded outputs"""
    cache = {}

    def run(a, w, bias=None, res=None, act=NONE, out_f32=False, **kw):
        assert bias is None
        if id(w) not in cache:
            cache[id(w)] = pack_strided(w)          # w is an operand() view: sl_pack_weight reads it with ldw > K
        n_out = N // 2 if act == SILU else N
        buf, out = guarded(M, n_out, F32 if out_f32 else dt)
        ops.gemm_decode(a, cache[id(w)], N, residual=res, act=act, out_f32=out_f32, out=out, **extra, **kw)
        assert untouched(buf, M, n_out), "write outside [0:M, 0:n_out]"
        return out
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# row-major GEMM
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,M,N,K", [(dt, M, N, K) for dt in DT16 for M, N, K in [(70, 50, 72), (130, 96, 200)]] + [(F32, 70, 50, 36), (F32, 130, 96, 200)])
def test_gemm_register_path_k_not_a_whole_slab(dt, M, N, K):
    """gemm_tiled_kernel: K that is no whole 128-byte slab (16-bit: 72, 200; fp32: 36, 200)"""
    check_exact(rowmajor(M, N, K, dt), M, N, K, dt, seed=100)
    check_gauss(rowmajor(M, N, K, dt), M, N, K, dt, seed=110)


TWO_STAGE = [(129, 136, 64), (130, 96, 192), (257, 200, 128)]          # one, three and two slabs (16-bit)


@pytest.mark.parametrize("dt,dmab", [(F16, "0"), (F16, "1"), (BF16, "0"), (BF16, "1"), (F32, "0")])
@pytest.mark.parametrize("M,N,K", TWO_STAGE)
def test_gemm_two_stage_128_tile(dt, dmab, M, N, K, tuning):
    """gemm_tiled_glds_kernel (SL_GLDS_RING=0), with and without the DMA requests between the MFMAs (SL_GLDS_DMAB, 16-bit only)"""
    _set(tuning, dict(SL_GLDS_RING="0", SL_GLDS_DMAB=dmab))
    check_exact(rowmajor(M, N, K, dt), M, N, K, dt, seed=120)
    check_gauss(rowmajor(M, N, K, dt), M, N, K, dt, seed=130)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("stages", ["4", "3", "104", "204"])
@pytest.mark.parametrize("M,N,K", [(130, 96, 512), (255, 200, 576)])
def test_gemm_ring_forms(dt, stages, M, N, K, tuning):
    """gemm128.hip ring forms (admission: >= 8 slabs)"""
    tuning("SL_GLDS_RING", stages)
    check_exact(rowmajor(M, N, K, dt), M, N, K, dt, seed=140)
    check_gauss(rowmajor(M, N, K, dt), M, N, K, dt, seed=150)


T256 = dict(SL_T256_MIN_TILES="1", SL_T256_MIN_K="64")


@pytest.mark.parametrize("dt,phased,noswap", [(dt, ph, ns) for dt in DTS for ph in "10" for ns in "01" if dt != F32 or ns == "0"])      # the swapped-operand epilogue is 16-bit only
@pytest.mark.parametrize("M,N,K", [(500, 200, 64), (1000, 200, 1024), (500, 196, 128), (1000, 203, 192), (500, 203, 1024), (1000, 196, 64),
                                   (500, 200, 192), (1000, 200, 128), (500, 224, 128)])
def test_gemm_256_tile_at_small_size(dt, phased, noswap, M, N, K, tuning):
    """gemm256.hip forced onto small products: prologue / tail paths (1, 2, 3, 16 slabs), swapped-operand epilogue (N = 200), LDS-turned
    rows epilogue (196, 203; 203 also the scalar tails), phased and one-barrier loops; N = 224 (a multiple of 32) adds the SiLU-mul
    epilogue, which this tile always runs through the rows epilogue"""
    _set(tuning, dict(T256, SL_T256_PHASED=phased, SL_NO_SWAP_EPILOGUE=noswap))
    check_exact(rowmajor(M, N, K, dt), M, N, K, dt, seed=160)
    check_gauss(rowmajor(M, N, K, dt), M, N, K, dt, seed=170)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form,M,N,K", [("splitk", 130, 132, 3072), ("splitk_two_stage", 130, 132, 3072), ("streamk", 257, 256, 8192)])
def test_gemm_split_k_and_stream_k_are_exact(dt, form, M, N, K, tuning):
    """K runs through the workspace (split-K: batched launch + reduce; stream-K: in-launch hand-over): on class E data the result is
    the unsplit bits, launch after launch, and the workspace's flags are left zero."""
    _set(tuning, dict(SL_STREAM_K="2", SL_SPLIT_K="0") if form == "streamk" else dict(SL_STREAM_K="0", SL_SPLIT_K="1"))
    if form == "splitk_two_stage":
        tuning("SL_GLDS_RING", "0")
    ws = ops.streamk_workspace(DEV)
    for rep in range(2):
        check_exact(rowmajor(M, N, K, dt, sk_ws=ws), M, N, K, dt, seed=180 + rep, scalings=rep == 0)
    assert int(ws[:1024].to(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile", ["128", "256"])
def test_gemm_grouped_ragged_batch(dt, tile, tuning):
    """Row counts [130, 1, 257] in one launch.  The 256-tile rule admits a grouped product only if rows padded to 256 stay within 9/8
    of rows padded to 128, which 257 does not: the launch's row bound is 500 there (the groups keep their own counts)."""
    Ms, N, K = [130, 1, 257], 200, 128
    if tile == "256":
        _set(tuning, T256)
    tot = sum(Ms)
    a, a64 = operand(ints((tot, K), -2, 2, 200), dt)
    w, w64 = operand(ints((N, K), -2, 2, 201), dt)
    b, b64 = vec(ints((N,), -8, 8, 202), dt)
    buf, out = guarded(tot, N, dt)
    lda, ldc = a.stride(0), out.stride(0)
    offs = [0, 130, 131]
    grp = torch.tensor([[m, offs[i] * lda, offs[i] * ldc, 0] for i, m in enumerate(Ms)], dtype=torch.int64, device=DEV)
    ops.gemm_ex(a, w, M=500 if tile == "256" else max(Ms), N=N, K=K, lda=lda, ldw=w.stride(0), out=out, ldc=ldc, bias=b, batch=len(Ms), groups=grp,
                w_mod=1, dtype=dt)
    assert untouched(buf, tot, N)
    msg = bad(out, to_dt(a64 @ w64.T + b64, dt))
    assert not msg, msg


@pytest.mark.parametrize("dt", DTS)
def test_gemm_strided_batch_grouped_conv_layout(dt):
    """The positional conv's argument layout (test_posconv_stage_and_grouped_conv) at T = 131: batch of G groups, A rows overlapping
    (lda = Hg < K = k Hg), C / bias / residual strided by Hg inside rows of H.  The last window of a group ends at row T + k - 2:
    every row behind it is poison (A's rows overlap, so it has no pad columns); W has poisoned pad columns (ldw > K)."""
    T, H, G, k = 131, 256, 4, 16
    Hg = H // G
    rows_g = T + k + 2
    xg64 = ints((G, rows_g, Hg), -2, 2, 210)
    xg64[:, T + k - 1:] = BIG[dt]
    xg64[:, T + k - 1:, ::2] *= -1.0
    xg, xg64 = vec(xg64, dt)
    wd, wd64 = operand(ints((G * Hg, k * Hg), -2, 2, 211), dt)
    bd, b64 = vec(ints((H,), -8, 8, 212), dt)
    r, r64 = operand(8 * ints((T, H), -512, 512, 213), dt)
    buf, out = guarded(T, H, dt)
    a = L.GemmArgs()
    a.A, a.lda, a.strideA = xg.data_ptr(), Hg, rows_g * Hg
    a.W, a.ldw, a.strideW = wd.data_ptr(), wd.stride(0), Hg * wd.stride(0)
    a.C, a.ldc, a.strideC = out.data_ptr(), out.stride(0), Hg
    a.bias, a.strideBias = bd.data_ptr(), Hg
    a.residual, a.ldr, a.strideR = r.data_ptr(), r.stride(0), Hg
    a.M, a.N, a.K, a.batch, a.dtype, a.act = T, Hg, k * Hg, G, L.dtype_code(dt), NONE
    ops.gemm_batched(a)
    assert untouched(buf, T, H)
    flat = xg64.reshape(G, rows_g * Hg)
    want = torch.empty(T, H, dtype=torch.float64)
    for g in range(G):
        win = torch.stack([flat[g, t * Hg:t * Hg + k * Hg] for t in range(T)])
        want[:, g * Hg:(g + 1) * Hg] = win @ wd64[g * Hg:(g + 1) * Hg].T
    msg = bad(out, to_dt(want + b64 + r64, dt))
    assert not msg, msg


@pytest.mark.parametrize("dt", DTS)
def test_gemm_implicit_conv_lda_below_k(dt):
    """Conv1d(k = 3, s = 2) on channel-last rows as a GEMM with lda = s C < K = k C; the rows behind the last window are poison"""
    Lin, Cc, C2, k, s = 401, 64, 96, 3, 2
    Lo = (Lin - k) // s + 1
    x64 = torch.cat([ints((Lin, Cc), -2, 2, 220), torch.full((4, Cc), BIG[dt], dtype=torch.float64)])
    x, x64 = vec(x64, dt)
    w, w64 = operand(ints((C2, k * Cc), -2, 2, 221), dt)
    b, b64 = vec(ints((C2,), -8, 8, 222), dt)
    buf, out = guarded(Lo, C2, dt)
    ops.gemm_ex(x, w, M=Lo, N=C2, K=k * Cc, lda=s * Cc, ldw=w.stride(0), out=out, ldc=out.stride(0), bias=b, dtype=dt)
    assert untouched(buf, Lo, C2)
    flat = x64.reshape(-1)
    win = torch.stack([flat[t * s * Cc:t * s * Cc + k * Cc] for t in range(Lo)])
    msg = bad(out, to_dt(win @ w64.T + b64, dt))
    assert not msg, msg


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M,N,K", [(65, 64, 64), (499, 128, 128)])
def test_gemm_row_statistics_and_layernorm_fold(dt, M, N, K):
    """stats_out (per-64-column {sum, sum of squares} of the STORED rows) and the LayerNorm-folded consumer rstd (x W'^T - mean u) + c"""
    a, a64 = operand(gauss((M, K), 230), dt)
    w, w64 = operand(gauss((N, K), 231, K ** -0.5), dt)
    r, r64 = operand(gauss((M, N), 233) + 0.5, dt)
    b, b64 = vec(gauss((N,), 232), dt)
    buf, out = guarded(M, N, dt)
    sbuf = torch.full((M + 2, N // 64, 2), FILL, device=DEV, dtype=F32)
    ops.gemm_ex(a, w, M=M, N=N, K=K, lda=a.stride(0), ldw=w.stride(0), out=out, ldc=out.stride(0), bias=b, residual=r, ldr=r.stride(0), stats_out=sbuf[1:M + 1],
                dtype=dt)
    assert untouched(buf, M, N) and bool((sbuf[0] == FILL).all()) and bool((sbuf[M + 1] == FILL).all())
    ref = a64 @ w64.T + b64 + r64
    mag = a64.abs() @ w64.abs().T + b64.abs() + r64.abs()
    msg = bad(out, ref, 2 * U[dt] * ref.abs() + K * E24 * mag + E24)
    assert not msg, msg
    seg = out.double().cpu().view(M, N // 64, 64)
    st = sbuf[1:M + 1].double().cpu()
    msg = bad(st[..., 0], seg.sum(-1), 64 * E24 * seg.abs().sum(-1) + E24)
    assert not msg, "segment sums: " + msg
    msg = bad(st[..., 1], (seg * seg).sum(-1), 66 * E24 * (seg * seg).sum(-1) + E24)
    assert not msg, "segment sums of squares: " + msg
    # consumer: the fold's own arithmetic in fp64 on the values it is handed
    mr, mr64 = vec(torch.stack([gauss((M,), 234), 0.5 + gauss((M,), 235).abs()], dim=-1), F32)
    uu, u64 = vec(gauss((N,), 236), F32)
    cc, c64 = vec(gauss((N,), 237), F32)
    for act in (NONE, GELU):
        buf2, out2 = guarded(M, N, dt)
        ops.gemm_ex(a, w, M=M, N=N, K=K, lda=a.stride(0), ldw=w.stride(0), out=out2, ldc=out2.stride(0), act=act, ln_mr=mr, ln_u=uu, ln_c=cc, dtype=dt)
        assert untouched(buf2, M, N)
        mean, rstd = mr64[:, :1], mr64[:, 1:]
        pre = rstd * (a64 @ w64.T - mean * u64) + c64
        e = rstd.abs() * (K * E24 * a64.abs() @ w64.abs().T + 4 * E24 * ((a64 @ w64.T).abs() + (mean * u64).abs())) + 4 * E24 * pre.abs()
        if act == GELU:
            ref2 = gelu64(pre)
            tol = 2 * U[dt] * ref2.abs() + 1.13 * e + 2e-6 * (1 + pre.abs()) + E24
        else:
            ref2, tol = pre, 2 * U[dt] * pre.abs() + e + E24
        msg = bad(out2, ref2, tol)
        assert not msg, f"fold act={act}: {msg}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,force256", [(70, 130, 64, False), (260, 1000, 256, True), (500, 1000, 256, True)])
def test_gemm_fused_top1_on_exact_ties(dt, M, N, K, force256, tuning):
    """ops.gemm_top1 on class E data (thousands of exact ties): every (value, column) partial is its 64-column group's maximum at the
    lowest column, and the row's token is argmax of the exact logits (torch's first-maximum rule).  With the 256-tile switches set,
    260 rows still take the 128-tile kernels (512 padded rows exceed 9/8 of 384); 500 rows reach the 256-tile rows epilogue.  A and W
    are views with poisoned pad columns and rows."""
    if force256:
        _set(tuning, T256)
    a, a64 = operand(ints((M, K), -2, 2, 240), dt)
    w, w64 = operand(ints((N, K), -2, 2, 241), dt)
    b, b64 = vec(ints((N,), -8, 8, 242), dt)
    for bias, bb in ((None, 0.0), (b, b64)):
        logits = a64 @ w64.T + bb
        val, idx = top1_strided(a, w, bias=bias)
        if bias is None:          # the wrapper itself, on contiguous copies
            val2, idx2 = ops.gemm_top1(a.contiguous(), w.contiguous())
            assert torch.equal(val2, val) and torch.equal(idx2, idx)
        ng = (N + 63) // 64
        grp = torch.cat([logits, torch.full((M, ng * 64 - N), -1e30, dtype=torch.float64)], 1).view(M, ng, 64)
        gmax = grp.max(dim=2).values
        first = (grp == gmax[:, :, None]).double().argmax(dim=2) + torch.arange(ng)[None, :] * 64
        assert torch.equal(val.T.double().cpu(), gmax)
        assert torch.equal(idx.T.long().cpu(), first)
        best = val.argmax(0)          # first maximum over the groups = lowest column among equals
        tok = idx.gather(0, best[None])[0].long().cpu()
        assert torch.equal(tok, logits.argmax(dim=1))


# ------------------------------------------------------------------------------------------------------------------------------
# packed decode GEMM
# ------------------------------------------------------------------------------------------------------------------------------
def check_fused_rms_silu(run, M, N, K, dt, seed, rstd_in=None):
    """class G for fuse_rms + SiLU-mul: y = rstd (x W^T); the scale is fp32 over K terms, (K + 8) 2^-24 relative"""
    a, a64 = operand(gauss((M, K), seed), dt)
    w, w64 = operand(gauss((N, K), seed + 1, K ** -0.5), dt)
    if rstd_in is None:
        rs = torch.rsqrt((a64 * a64).mean(-1, keepdim=True) + 1e-5)
        kw = {}
    else:
        rs = rstd_in.double().cpu()[:, None]
        kw = dict(rstd_in=rstd_in)
    y, mag = rs * (a64 @ w64.T), rs * (a64.abs() @ w64.abs().T)
    e = (2 * K + 8) * E24 * mag
    ref, tol = silu_mul_bound(y, e, U[dt])
    msg = bad(run(a, w, act=SILU, fuse_rms=True, eps=1e-5, **kw), ref, tol)
    assert not msg, f"G fuse_rms + silu_mul {(M, N, K)}: {msg}"
    tol = 2 * U[dt] * y.abs() + e + E24
    msg = bad(run(a, w, fuse_rms=True, eps=1e-5, **kw), y, tol)
    assert not msg, f"G fuse_rms {(M, N, K)}: {msg}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(M, N, 256) for M in (1, 8, 16, 17, 26) for N in (48, 1000, 4096, 16400)] + [(M, 3072, K) for M in (1, 8) for K in (3072, 8192)])
def test_gemm_packed_skinny(dt, M, N, K):
    """gemm_skinny_kernel on packed weights: MT 1 / 2 / 4, the < 256, >= 256 and >= 1024 fragment structures, the 3- and 4-step o / down
    structures (M <= 8)"""
    check_exact(packed(M, N, K, dt), M, N, K, dt, seed=300, bias=False)
    if K == 256 and N in (1000, 4096):
        check_gauss(packed(M, N, K, dt), M, N, K, dt, seed=310, gelu=False, bias=False, silu=N % 32 == 0)
        if N % 32 == 0:
            check_fused_rms_silu(packed(M, N, K, dt), M, N, K, dt, seed=320)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("M", [27, 128, 129, 384])
@pytest.mark.parametrize("N,K", [(1000, 256), (1000, 448), (1024, 448)])
def test_gemm_packed_streaming_blocks(dt, split, M, N, K):
    """gemm_stream_kernel: 128-row blocks, ragged last fragment group (N = 1000), odd stage count (K = 448), with and without the K split"""
    check_exact(packed(M, N, K, dt, split_k=split), M, N, K, dt, seed=330, bias=False)
    check_gauss(packed(M, N, K, dt, split_k=split), M, N, K, dt, seed=340, gelu=False, bias=False)
    if N % 32 == 0:
        check_fused_rms_silu(packed(M, N, K, dt, split_k=split), M, N, K, dt, seed=350)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("M", [385, 512, 700])
def test_gemm_packed_wide_block(dt, split, M, tuning):
    """gemm_stream_wide_kernel (SL_STREAM_WIDE=2) on shapes the default rule leaves to the 128-row form"""
    N, K = 1000, 448
    tuning("SL_STREAM_WIDE", "2")
    check_exact(packed(M, N, K, dt, split_k=split), M, N, K, dt, seed=360, bias=False)
    check_gauss(packed(M, N, K, dt, split_k=split), M, N, K, dt, seed=370, gelu=False, bias=False, silu=False)
    rstd = (0.5 + gauss((M,), 371).abs()).float().to(DEV)
    check_fused_rms_silu(packed(M, 1024, K, dt, split_k=split), M, 1024, K, dt, seed=372, rstd_in=rstd)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("fixup", ["0", "1"])
@pytest.mark.parametrize("M", [385, 512, 700])
def test_gemm_packed_wide_k_split_fixup_and_reduce_are_exact(dt, fixup, M, tuning):
    """K split of the wide form (K = 2048, N = 512): the separate reduce launch and the in-kernel fix-up each give the exact result"""
    N, K = 512, 2048
    assert L.lib().sl_gemm_split_count(M, N, K, L.dtype_code(dt)) > 1
    tuning("SL_STREAM_FIXUP", fixup)
    for rep in range(2):          # the fix-up's counters are left at zero: a second call on the same workspace
        check_exact(packed(M, N, K, dt), M, N, K, dt, seed=380 + rep, bias=False, scalings=rep == 0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [40, 128, 600])
def test_gemm_packed_rstd_handoff_and_norm_out(dt, M):
    """rstd_out / norm_out ride on the K-split reduce pass; the next fused product takes the scale (rstd_in)"""
    H, K1 = 512, 2048
    assert L.lib().sl_gemm_split_count(M, H, K1, L.dtype_code(dt)) > 1
    a, a64 = operand(gauss((M, K1), 390), dt)
    w, w64 = vec(gauss((H, K1), 391, K1 ** -0.5), dt)
    r, r64 = operand(gauss((M, H), 392), dt)
    g, g64 = vec(1.0 + gauss((H,), 393, 0.1), dt)
    wp = ops.pack_weight(w)
    buf, out = guarded(M, H, dt)
    nbuf = torch.full((M + 2, H), FILL, device=DEV, dtype=dt)          # norm_out is a contiguous (M, N) buffer: row guards only
    h = nbuf[1:M + 1]
    rbuf = torch.full((M + 16,), FILL, device=DEV, dtype=F32)
    ops.gemm_decode(a, wp, H, residual=r, rstd_out=rbuf[8:8 + M], eps=1e-5, out=out, norm_out=None, norm_gain=None)
    rstd = rbuf[8:8 + M].clone()
    assert untouched(buf, M, H) and bool((rbuf[:8] == FILL).all()) and bool((rbuf[8 + M:] == FILL).all())
    ref = a64 @ w64.T + r64
    tol = 2 * U[dt] * ref.abs() + K1 * E24 * (a64.abs() @ w64.abs().T + r64.abs()) + E24
    msg = bad(out, ref, tol)
    assert not msg, msg
    x64 = out.double().cpu()
    want = torch.rsqrt((x64 * x64).mean(-1) + 1e-5)
    msg = bad(rstd, want, (H + 8) * E24 * want)
    assert not msg, "rstd_out (of the stored rows): " + msg
    buf2, out2 = guarded(M, H, dt)
    rstd2 = torch.empty(M, device=DEV, dtype=F32)
    ops.gemm_decode(a, wp, H, residual=r, rstd_out=rstd2, eps=1e-5, out=out2, norm_out=h, norm_gain=g)
    assert untouched(buf2, M, H) and torch.equal(out2, out) and torch.equal(rstd2, rstd)
    href = x64 * want[:, None] * g64
    msg = bad(h, href, 2 * U[dt] * href.abs() + (H + 16) * E24 * href.abs() + E24)
    assert not msg, "norm_out: " + msg
    assert bool((nbuf[0] == FILL).all()) and bool((nbuf[M + 1] == FILL).all())
    check_fused_rms_silu(packed(M, 1024, H, dt), M, 1024, H, dt, seed=394, rstd_in=(0.5 + gauss((M,), 395).abs()).float().to(DEV))


def _rope_perm(nh, nkv):
    blk = torch.arange(16)
    hp = torch.cat([torch.cat([blk + 16 * j, blk + 64 + 16 * j]) for j in range(4)])
    return torch.cat([hp + 128 * h for h in range(nh + nkv)] + [torch.arange((nh + nkv) * 128, (nh + 2 * nkv) * 128)])


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1, 17, 130])
def test_gemm_packed_rope_kv_epilogue(dt, M):
    """ACT_ROPE_KV on class E weights and inputs: V rows are exact copies at (slot, position); at position 0 (cos 1, sin 0) Q and K
    are exact too; at other positions Q and K are within 2u |ref| + K 2^-24 (mag1 + mag2) of the fp64 rotation; the caches are
    untouched everywhere else."""
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=6, num_key_value_heads=2, head_dim=128,
                             rope_scaling=dict(factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192))
    nh, nkv, D, H, max_ctx = 6, 2, 128, 256, 64
    N = (nh + 2 * nkv) * D
    cos, sin = [t_.to(DEV) for t_ in weights.rope_tables(arch, max_ctx)]
    x, x64 = operand(ints((M, H), -2, 2, 400), dt)
    w, w64 = vec(ints((N, H), -2, 2, 401), dt)
    wp = ops.pack_weight(w[_rope_perm(nh, nkv).to(DEV)].contiguous())
    y = (x64 @ w64.T).view(M, nh + 2 * nkv, D)
    mag = (x64.abs() @ w64.abs().T).view(M, nh + 2 * nkv, D)
    seq = torch.arange(M, dtype=torch.int32, device=DEV)
    for pos_list in ([0] * M, [(7 * i + 3) % max_ctx for i in range(M)]):
        pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
        kc = torch.full((M, nkv, max_ctx, D), FILL, device=DEV, dtype=dt)
        vc = torch.full_like(kc, FILL)
        buf, qo = guarded(M, nh * D, dt)
        ops.gemm_decode(x, wp, N, act=ROPE, out=qo, rope=dict(cos=cos, sin=sin, pos=pos, seq=seq, k_cache=kc, v_cache=vc, n_heads=nh, n_kv=nkv, max_ctx=max_ctx))
        assert untouched(buf, M, nh * D)
        c = torch.cat([cos.double().cpu()[pos.long().cpu()]] * 2, -1)[:, None]
        s = torch.cat([sin.double().cpu()[pos.long().cpu()]] * 2, -1)[:, None]
        qk = y[:, :nh + nkv]
        rot = torch.cat([-qk[..., D // 2:], qk[..., :D // 2]], -1)
        ref = qk * c + rot * s
        mg = mag[:, :nh + nkv]
        tol = 2 * U[dt] * ref.abs() + H * E24 * (mg + torch.cat([mg[..., D // 2:], mg[..., :D // 2]], -1)) + E24
        rows = torch.arange(M)
        p_ = pos.long().cpu()
        got_q = qo.double().cpu().view(M, nh, D)
        got_k = kc.cpu()[rows, :, p_].double()          # (M, nkv, D)
        got_v = vc.cpu()[rows, :, p_]
        if all(p == 0 for p in pos_list):
            assert not bad(got_q, to_dt(ref[:, :nh], dt).double()), "Q at position 0: " + bad(got_q, to_dt(ref[:, :nh], dt).double())
            assert not bad(got_k, to_dt(ref[:, nh:], dt).double()), "K at position 0: " + bad(got_k, to_dt(ref[:, nh:], dt).double())
        else:
            msg = bad(got_q, ref[:, :nh], tol[:, :nh])
            assert not msg, "Q: " + msg
            msg = bad(got_k, ref[:, nh:], tol[:, nh:])
            assert not msg, "K: " + msg
        assert not bad(got_v, to_dt(y[:, nh + nkv:], dt)), "V: " + bad(got_v, to_dt(y[:, nh + nkv:], dt))
        for cache in (kc, vc):
            chk = cache.cpu().clone()
            chk[rows, :, p_] = FILL
            assert bool((chk == FILL).all()), "cache written outside (tok_seq, tok_pos)"


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
def attn_bounds(q64, k64, v64, vis, scale, dt):
    """q (nh, nq, D), k / v (nkv, nk, D) fp64, vis (nq, nk) bool -> ref, tol, must_be_zero, each (nq, nh * D)"""
    nh, nq, D = q64.shape
    rep = nh // k64.shape[0]
    k, v = k64.repeat_interleave(rep, 0), v64.repeat_interleave(rep, 0)
    s = (q64 @ k.transpose(1, 2)) * scale
    s = s.masked_fill(~vis[None], float("-inf"))
    p = torch.softmax(s, -1)
    ref = p @ v
    pv = p @ v.abs()
    tol = 2 * U[dt] * ref.abs() + 4 * U[dt] * pv + vis.shape[1] * E24
    zero = (vis.double()[None] @ v.abs()) == 0
    flat = lambda t_: t_.transpose(0, 1).reshape(nq, nh * D)
    return flat(ref), flat(tol), flat(zero)


def check_attn(got, ref, tol, zero, dt, what):
    got = got.double().cpu()
    assert bool((got[zero] == 0).all()), f"{what}: {int((got[zero] != 0).sum())} outputs that no visible key feeds are not zero"
    if dt == F32:
        assert rel_err(got, ref) < 2e-5, what
    else:
        msg = bad(got, ref, tol)
        assert not msg, f"{what}: {msg}"


QL, KL, SLACK = [70, 1, 260, 33, 129], [200, 64, 300, 33, 129], 5


# The rule's own choice ("default") is the generic kernel in fp32 and, in 16 bits, QT = 2 at D = 128 but QT = 4 at D = 64 (max_qlen = 260
# is above 192): there QT = 2 is selected with SL_ATTN_QT=2.  SL_ATTN_FWD_ST=2 is read on the QT = 4 (D = 64) branch only, so it has no
# D = 128 case.
PREFILL_FORMS = {"default": {}, "qt2": dict(SL_ATTN_QT="2"), "qt4": dict(SL_ATTN_QT="4"), "qt4_st2": dict(SL_ATTN_QT="4", SL_ATTN_FWD_ST="2"),
                 "generic": dict(SL_ATTN_GENERIC="1")}
PREFILL_CASES = [(dt, "default", D) for dt in DTS for D in (64, 128)] + \
                [(dt, form, 64) for dt in DT16 for form in ("qt2", "qt4", "qt4_st2", "generic")] + [(dt, "generic", 128) for dt in DT16]


@pytest.mark.parametrize("dt,form,D,nh,nkv", [(dt, form, D) + {64: (4, 4), 128: (6, 2)}[D] for dt, form, D in PREFILL_CASES])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_prefill_mask_probe_and_gaussian(dt, form, causal, D, nh, nkv, tuning):
    """attn_fwd with more keys than queries (causal visibility j <= i + klen - qlen): the transposed-score kernel at both query-tile
    widths (QT = 2, QT = 4) and with SL_ATTN_FWD_ST=2, and the generic kernel (always, in fp32).  Packed K / V keep 5 poisoned rows behind every
    sequence's klen."""
    _set(tuning, PREFILL_FORMS[form])
    scale = D ** -0.5
    nq_tot, rows_k = sum(QL), sum(KL) + SLACK * len(KL)
    q, q64 = operand(gauss((nq_tot, nh * D), 500), dt)
    k64 = torch.full((rows_k, nkv * D), 8.0, dtype=torch.float64)
    vg64 = torch.full((rows_k, nkv * D), BIG[dt], dtype=torch.float64)
    vp64 = vg64.clone()
    cu_k = [0]
    for n in KL:
        o = cu_k[-1]
        k64[o:o + n] = gauss((n, nkv * D), 501 + o)
        vg64[o:o + n] = gauss((n, nkv * D), 601 + o)
        vp64[o:o + n] = 0.0
        j = torch.arange(n)
        for h in range(nkv):
            vp64[o + j, h * D + j % D] = 1.0
        cu_k.append(o + n + SLACK)
    k, k64 = operand(k64, dt)
    cu_q = torch.tensor([0] + list(torch.tensor(QL).cumsum(0)), dtype=torch.int32, device=DEV)
    cu_kd = torch.tensor(cu_k, dtype=torch.int32, device=DEV)
    kl = torch.tensor(KL, dtype=torch.int32, device=DEV)
    for cls, v64_ in (("P", vp64), ("G", vg64)):
        v, v64 = operand(v64_, dt)
        buf, out = guarded(nq_tot, nh * D, dt)
        ops.attn_fwd(q, k, v, out, cu_q, cu_kd, kl, q_strides=(q.stride(0), D), k_strides=(k.stride(0), D), v_strides=(v.stride(0), D),
                     o_strides=(out.stride(0), D), nseq=len(QL), max_qlen=max(QL), n_heads=nh, n_kv_heads=nkv, head_dim=D, causal=causal, scale=scale)
        assert untouched(buf, nq_tot, nh * D)
        q0 = 0
        for i, (nq, nk) in enumerate(zip(QL, KL)):
            k0 = cu_k[i]
            vis = torch.ones(nq, nk, dtype=torch.bool)
            if causal:
                vis = torch.arange(nk)[None, :] <= torch.arange(nq)[:, None] + (nk - nq)
            ref, tol, zero = attn_bounds(q64[q0:q0 + nq].view(nq, nh, D).transpose(0, 1), k64[k0:k0 + nk].view(nk, nkv, D).transpose(0, 1),
                                         v64[k0:k0 + nk].view(nk, nkv, D).transpose(0, 1), vis, scale, dt)
            check_attn(out[q0:q0 + nq], ref, tol, zero, dt, f"{cls} sequence {i} ({nq} q / {nk} k)")
            q0 += nq


CTX = [1, 63, 64, 65, 127, 128, 129, 393, 448]
DECODE_FORMS = {
    "per_sequence": {},
    "single_pass_128": dict(SL_ATTN_FULL_MIN="1"),
    "single_pass_64": dict(SL_ATTN_FULL_MIN="1", SL_ATTN_DECODE_KS="64"),
    "single_pass_65": dict(SL_ATTN_FULL_MIN="1", SL_ATTN_DECODE_KS="65"),
    "split_combine": dict(SL_ATTN_FORCE_SPLIT="1", SL_ATTN_SPLIT_MERGE="0"),
    "split_merge": dict(SL_ATTN_FORCE_SPLIT="1", SL_ATTN_SPLIT_MERGE="1"),
}


@pytest.mark.parametrize("dt,form", [(dt, form) for dt in DTS for form in DECODE_FORMS if dt != F32 or not form.startswith("single_pass")])      # single pass: 16-bit only
@pytest.mark.parametrize("nh,nkv", [(6, 2), (4, 1)])
def test_attention_decode_mask_probe_and_gaussian(dt, form, nh, nkv, tuning):
    """attn_decode (per sequence) and attn_decode_split (single pass with 128- / 64-key chunks, split + combine launch, split + in-launch
    merge) against a cache whose slots behind every context hold poison (K 8.0, V large): the state a reused cache is in."""
    _set(tuning, DECODE_FORMS[form])
    D, max_ctx, B = 128, 448, len(CTX)
    scale = D ** -0.5
    q, q64 = operand(gauss((B, nh * D), 700), dt)
    k64 = gauss((B, nkv, max_ctx, D), 701)
    vg64 = gauss((B, nkv, max_ctx, D), 702)
    vp64 = torch.zeros_like(vg64)
    j = torch.arange(max_ctx)
    vp64[:, :, j, j % D] = 1.0
    for s, n in enumerate(CTX):
        k64[s, :, n:] = 8.0
        vg64[s, :, n:] = BIG[dt]
        vp64[s, :, n:] = BIG[dt]
    kc, k64 = vec(k64, dt)
    ctx = torch.tensor(CTX, dtype=torch.int32, device=DEV)
    for cls, v64_ in (("P", vp64), ("G", vg64)):
        vc, v64 = vec(v64_, dt)
        obuf = torch.full((B + 2, nh * D), FILL, device=DEV, dtype=dt)
        out = obuf[1:B + 1]
        if form == "per_sequence":
            L.check(L.lib().sl_attn_decode(L.ptr(q), q.stride(0), L.ptr(kc), L.ptr(vc), L.ptr(out), L.ptr(ctx), B, nh, nkv, D, max_ctx, scale, L.dtype_code(dt),
                                           L.stream_ptr()), "sl_attn_decode")
        else:
            ops.attn_decode_split(q, q.stride(0), kc, vc, ctx, nh, nkv, D, max_ctx, scale, out=out)
        assert bool((obuf[0] == FILL).all()) and bool((obuf[B + 1] == FILL).all())
        for s, n in enumerate(CTX):
            ref, tol, zero = attn_bounds(q64[s].view(nh, 1, D), k64[s, :, :n], v64[s, :, :n], torch.ones(1, n, dtype=torch.bool), scale, dt)
            check_attn(out[s:s + 1], ref, tol, zero, dt, f"{cls} context {n}")


# ------------------------------------------------------------------------------------------------------------------------------
# small kernels, odd sizes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", [8, 1000, 4096])
def test_rmsnorm_and_layernorm_per_element(dt, cols):
    """norm.hip at its smallest (one 16-bit vector) and largest (4096) column counts and one in between, 37 rows"""
    rows = 37
    x, x64 = vec(gauss((rows, cols), 800) + 0.3, dt)
    g, g64 = vec(1.0 + gauss((cols,), 801, 0.1), dt)
    b, b64 = vec(gauss((cols,), 802, 0.1), dt)
    u = U[dt]
    rs = torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + 1e-5)
    ref = g64 * (x64 * rs)
    msg = bad(ops.rmsnorm(x, g, 1e-5), ref, 2 * u * ref.abs() + (cols + 16) * E24 * ref.abs() + E24)
    assert not msg, "rmsnorm: " + msg
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + 1e-5)
    ref = (x64 - mean) * rstd * g64 + b64
    # the mean carries cols 2^-24 sum|x| / cols; the centred value is scaled by rstd g
    e = (cols + 16) * E24 * (rstd * g64.abs() * (x64.abs() + x64.abs().mean(-1, keepdim=True)) + b64.abs())
    msg = bad(ops.layernorm(x, g, b, 1e-5), ref, 2 * u * ref.abs() + e + E24)
    assert not msg, "layernorm: " + msg
    gref = gelu64(ref)
    msg = bad(ops.layernorm(x, g, b, 1e-5, gelu=True), gref, 2 * u * gref.abs() + 1.13 * e + 2e-6 * (1 + ref.abs()) + E24)
    assert not msg, "layernorm + gelu: " + msg


@pytest.mark.parametrize("dt", DTS)
def test_avgpool_embed_silu_mul_rope_per_element(dt):
    u = U[dt]
    x, x64 = vec(gauss((51, 136), 810), dt)
    ref = torch.stack([x64[4 * i:4 * i + 8].mean(0) for i in range((51 - 8) // 4 + 1)])
    mag = torch.stack([x64[4 * i:4 * i + 8].abs().mean(0) for i in range((51 - 8) // 4 + 1)])
    msg = bad(ops.avgpool_rows(x, 8, 4), ref, 2 * u * ref.abs() + 10 * E24 * mag + E24)
    assert not msg, "avgpool: " + msg
    ranges = [(0, 3), (3, 4), (4, 11), (11, 30), (30, 51)]
    ref = torch.stack([x64[s:e].mean(0) for s, e in ranges])
    mag = torch.stack([x64[s:e].abs().mean(0) for s, e in ranges])
    got = ops.avgpool_rows(x, ranges=torch.tensor(ranges, dtype=torch.int32, device=DEV))
    msg = bad(got, ref, 2 * u * ref.abs() + 24 * E24 * mag + E24)
    assert not msg, "avgpool ranges: " + msg
    table, _ = vec(gauss((1001, 136), 811), dt)
    ids = torch.tensor([[0, 1000, 5, 5, 123, 999, 1]])
    assert torch.equal(ops.embed_gather(table, ids), table[ids.view(-1).to(DEV)])
    gu, gu64 = vec(gauss((37, 2 * 272), 812, 2.0), dt)
    ref, tol = silu_mul_bound(gu64, torch.zeros_like(gu64), u)
    msg = bad(ops.silu_mul(gu), ref, tol)
    assert not msg, "silu_mul: " + msg
    arch = weights.LlamaArch(hidden_size=256, num_attention_heads=6, num_key_value_heads=2, head_dim=128)
    cos, sin = weights.rope_tables(arch, 64)
    n, heads, n_rot, D = 41, 6, 4, 128
    xr, xr64 = vec(gauss((n, heads * D), 813), dt)
    pos = torch.tensor([(5 * i + 1) % 64 for i in range(n)], dtype=torch.int32)
    ops.rope_inplace(xr, pos.to(DEV), cos.to(DEV), sin.to(DEV), heads, n_rot, D)
    v = xr64.view(n, heads, D).clone()
    c, s_ = cos.double()[pos.long()][:, None], sin.double()[pos.long()][:, None]
    a1, a2 = v[:, :n_rot, :D // 2].clone(), v[:, :n_rot, D // 2:].clone()
    v[:, :n_rot, :D // 2] = a1 * c - a2 * s_
    v[:, :n_rot, D // 2:] = a2 * c + a1 * s_
    mag = xr64.view(n, heads, D).abs()
    mag = mag + torch.cat([mag[..., D // 2:], mag[..., :D // 2]], -1)
    msg = bad(xr.view(n, heads, D), v, 2 * u * v.abs() + 4 * E24 * mag + E24)
    assert not msg, "rope_inplace: " + msg
    assert torch.equal(xr.view(n, heads, D)[:, n_rot:].double().cpu(), xr64.view(n, heads, D)[:, n_rot:]), "heads beyond n_rot must be untouched"


# ------------------------------------------------------------------------------------------------------------------------------
# attention, training mode: sl_attn_bwd (every form) and sl_attn_fwd's training outputs (lse, dropout)
# ------------------------------------------------------------------------------------------------------------------------------
# Reference and bounds: tests/attn_train_ref.py (fp64 on the stored inputs; DESIGN.md derives every constant; tests/
# test_attn_train_bounds_cpu.py holds the bounds against an emulation of the kernels' rounding points and four wrong ones).  The backward is
# handed out = the reference O rounded to the storage type and lse = the reference rounded to fp32, so its inputs are known to one
# rounding each and a failure here is the backward's own.  Out of scope: klen < qlen under a causal mask (rows that see no key), which
# no caller produces.
P_DROP, DROP_SEED = 0.25, 0x1_2345_6789          # a seed above 2^32: both words of it are used
TRAIN_SETS = {
    "ragged": (QL, KL, 0),                                                        # straddles TQ 64 / 32 / 16, TK and TK2 64 / 32, 64- and 128-row blocks
    "crossing": ([70], [70], 1000),                                               # with 64 heads (row * 64 + head) passes 65 536 at query 24 of the first tile
    "rule_kf2": ([129 + (127 * i) // 11 for i in range(12)],) * 2 + (0,),         # 129 ... 256: ceil(256 / 128) x 8 kv heads x 12 = 192 blocks
    "rule_split": ([260] * 8,) * 2 + (0,),                                        # 2 x 5 x 16 x 8 = 1 280 blocks > 1 024
}
BWD_FORMS = {"both": {}, "split_kf1": dict(SL_ATTN_BWD_BOTH="0"), "kf2": dict(SL_ATTN_BWD_KF="2"), "fp32": {}}
BWD_DT_FORMS = [(BF16, "both"), (BF16, "split_kf1"), (BF16, "kf2"), (F32, "fp32")]
HEADS = {64: (4, 4), 128: (6, 2)}


@pytest.fixture(scope="module", autouse=True)
def _release_train_cases():
    """the cached cases hold device tensors: they go when this module's tests are done, not when the process ends"""
    yield
    train_case.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=16)
def train_case(set_name, family, D, nh, nkv, causal, drop, dt):
    """Inputs on the device (strided views with poisoned pads), the fp64 reference of every sequence with its bounds, and the reference's
    own out / lse as the backward's inputs.  Computed once per key and left unchanged: the forms of a kernel share it."""
    ql, kl, t0 = TRAIN_SETS[set_name]
    scale, p = D ** -0.5, (P_DROP if drop else 0.0)
    q64, k64, v64, do64, cu_k = R.packed_inputs(family, ql, kl, nh, nkv, D, dt, SLACK, seed=900, t0=t0)
    c = SimpleNamespace(ql=ql, kl=kl, t0=t0, cu_k=cu_k, n_tok=q64.shape[0], rows_k=k64.shape[0], scale=scale, p=p, seqs=[])
    c.q, q64 = operand(q64, dt)
    c.k, k64 = operand(k64, dt)
    c.v, v64 = operand(v64, dt)
    c.do, do64 = operand(do64, dt)
    o64 = gauss((c.n_tok, nh * D), 899, 0.25)                                     # filler rows stay finite: the delta pass reads every row
    lse64 = torch.zeros(c.n_tok, nh, dtype=torch.float64)
    qo = t0
    for i, (nq, nk) in enumerate(zip(ql, kl)):
        keep = R.dropout_keep_at(R.drop_index(qo, nq, nk, nh), p, DROP_SEED) if drop else None        # exactly the indices the case touches
        r = R.attn_train_ref(R.heads(q64[qo:qo + nq], nh), R.heads(k64[cu_k[i]:cu_k[i] + nk], nkv), R.heads(v64[cu_k[i]:cu_k[i] + nk], nkv),
                             R.heads(do64[qo:qo + nq], nh), R.visibility(nq, nk, causal), scale, keep, p, dt=dt)
        o64[qo:qo + nq], lse64[qo:qo + nq] = R.flat(r.O), r.lse.T
        s = SimpleNamespace(q0=qo, k0=cu_k[i], nq=nq, nk=nk, lse=r.lse.T, lse_acc=r.lse_acc.T, lse_ulp=r.lse_ulp.T)
        for name in ("O", "dQ", "dK", "dV"):
            setattr(s, name, (R.flat(getattr(r, name)), R.flat(getattr(r, "tol_" + name)), R.flat(getattr(r, "zero_" + name))))
        c.seqs.append(s)
        qo += nq
    c.out, _ = operand(o64, dt)
    c.lse = lse64.float().to(DEV)
    mk = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    c.cu_q, c.cu_kd, c.klen = mk([t0 + sum(ql[:i]) for i in range(len(ql) + 1)]), mk(cu_k), mk(kl)
    return c


def check_train(got, s, name, dt, what):
    """one sequence's rows of one output against (reference, bound, exact zeros); fp32: the zeros and the forward suite's rel_err"""
    want, tol, zero = getattr(s, name)
    got = got.double().cpu()
    assert bool((got[zero] == 0).all()), f"{what} {name}: {int((got[zero] != 0).sum())} elements that nothing visible feeds are not zero"
    if dt == F32:
        assert rel_err(got, want) < 2e-5, f"{what} {name}: rel err {rel_err(got, want):.3g}"
    else:
        msg = bad(got, want, tol)
        assert not msg, f"{what} {name}: {msg}"


def run_bwd(c, dt, nh, nkv, D, causal):
    """sl_attn_bwd into fresh guarded dq / dk / dv; guards, the rows in front of the first sequence, the rows behind every klen and delta"""
    bq, dq = guarded(c.n_tok, nh * D, dt)
    bk, dk = guarded(c.rows_k, nkv * D, dt)
    bv, dv = guarded(c.rows_k, nkv * D, dt)
    dbuf = torch.full((c.n_tok + 2, nh), float("nan"), device=DEV, dtype=F32)
    dbuf[0], dbuf[-1] = FILL, FILL
    st = lambda x: (x.stride(0), D)
    ops.attn_bwd(c.q, c.k, c.v, c.out, c.do, c.lse, dq, dk, dv, c.cu_q, c.cu_kd, c.klen, q_strides=st(c.q), k_strides=st(c.k), v_strides=st(c.v),
                 o_strides=st(c.out), do_strides=st(c.do), dq_strides=st(dq), dk_strides=st(dk), dv_strides=st(dv), nseq=len(c.ql), max_qlen=max(c.ql),
                 max_klen=max(c.kl), n_tok_q=c.n_tok, n_heads=nh, n_kv_heads=nkv, head_dim=D, causal=causal, scale=c.scale, dropout_p=c.p,
                 dropout_seed=DROP_SEED, delta=dbuf[1:-1])
    assert untouched(bq, c.n_tok, nh * D) and untouched(bk, c.rows_k, nkv * D) and untouched(bv, c.rows_k, nkv * D), "write outside dq / dk / dv"
    assert bool((dq[:c.t0] == FILL).all()), "dq rows in front of the first sequence written"
    for s in c.seqs:
        for g in (dk, dv):
            assert bool((g[s.k0 + s.nk:s.k0 + s.nk + SLACK] == FILL).all()), f"dk / dv rows behind klen = {s.nk} written"
    assert bool((dbuf[0] == FILL).all()) and bool((dbuf[-1] == FILL).all()) and bool(torch.isfinite(dbuf[1:-1]).all()), "delta"
    return dq, dk, dv


def bwd_case(set_name, dt, form, D, nh, nkv, causal, drop, tuning):
    _set(tuning, BWD_FORMS[form])
    for family in "PG":
        c = train_case(set_name, family, D, nh, nkv, causal, drop, dt)
        dq, dk, dv = run_bwd(c, dt, nh, nkv, D, causal)
        for i, s in enumerate(c.seqs):
            what = f"{family} sequence {i} ({s.nq} q / {s.nk} k)"
            check_train(dq[s.q0:s.q0 + s.nq], s, "dQ", dt, what)
            check_train(dk[s.k0:s.k0 + s.nk], s, "dK", dt, what)
            check_train(dv[s.k0:s.k0 + s.nk], s, "dV", dt, what)
        dq2, dk2, dv2 = run_bwd(c, dt, nh, nkv, D, causal)          # no atomics: the same bits, call after call
        assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv), f"{family}: two calls differ"


@pytest.mark.parametrize("dt,form", BWD_DT_FORMS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_backward_probes_and_gaussian(dt, form, D, causal, tuning):
    """sl_attn_bwd with more keys than queries (shift = klen - qlen > 0, and one shift = 0 pair) in each of its forms: both passes in one
    launch, the one-fragment pair, the two-fragment pair, and the fp32 pair"""
    bwd_case("ragged", dt, form, D, *HEADS[D], causal, False, tuning)


@pytest.mark.parametrize("dt,form,D,causal", [(dt, form, 64, False) for dt, form in BWD_DT_FORMS] + [(BF16, "both", 128, True), (F32, "fp32", 128, True)])
def test_attention_backward_with_dropout(dt, form, D, causal, tuning):
    """p = 0.25: the keep mask of exactly the (row, head, key) indices the case touches, restated on the host"""
    bwd_case("ragged", dt, form, D, *HEADS[D], causal, True, tuning)


@pytest.mark.parametrize("dt,form", BWD_DT_FORMS)
def test_attention_backward_dropout_counter_crossing(dt, form, tuning):
    """70 tokens at rows 1000 ... 1069 of a 1070-row buffer, 64 heads: the upper word of the mask counter, (row * 64 + head) >> 16, steps
    from 0 to 1 at query 24, inside the first query tile of every form"""
    bwd_case("crossing", dt, form, 64, 64, 64, False, True, tuning)


@pytest.mark.parametrize("set_name,D,nh,causal", [("rule_kf2", 128, 8, True), ("rule_split", 64, 16, False)])
def test_attention_backward_forms_selected_by_rule(set_name, D, nh, causal, tuning):
    """bf16, no switch set: launch_attn_bwd's rule takes the two-fragment pair (D = 128, 192 blocks of 128 keys) and the stand-alone
    one-fragment pair (1 280 blocks together); which kernels ran is shown by profiles/attn_train_edge_census.txt"""
    bwd_case(set_name, BF16, "both", D, nh, nh, causal, False, tuning)


# lse beyond its derived bound: the error of exp2f / log2f (transposed-score kernel) and __expf / logf (generic kernel), which this project
# states nowhere.  Measured on an MI355X as the worst |lse - fp64 reference| - derived part over the cases below (DESIGN.md records the
# figures), asserted with a factor of 4.
# fp32 roundings after the scores.  attn_fwd_kernel: scale multiply, max-subtract, sum, rescale of the running sum, log, add.  attn_fwd_tr_kernel:
# the constant scale * log2(e), the running maximum's multiply by it, the fma that subtracts it, sum, rescale, log2, add, the multiply by ln 2.
LSE_OPS = {"tr": 8, "generic": 6}
LSE_MEASURED = {"tr": 0.0, "generic": 0.0}
FWD_TRAIN = {          # name: (kernel family, D, causal, dropout, switches)
    "tr_drop": ("tr", 64, False, True, {}),
    "tr_drop_st2": ("tr", 64, False, True, dict(SL_ATTN_FWD_ST="2")),
    "generic_drop": ("generic", 64, False, True, dict(SL_ATTN_GENERIC="1")),          # fp32 takes the generic kernel with or without the switch
    "generic_drop_causal_128": ("generic", 128, True, True, {}),                      # 16-bit: the rule itself falls back to the generic kernel
    "lse_only": ("tr", 64, False, False, {}),
    "lse_only_causal_128": ("tr", 128, True, False, {}),
}
FWD_TRAIN_CASES = [(dt, f) for f in ("tr_drop", "tr_drop_st2") for dt in DT16] + [(F32, "generic_drop"), (BF16, "generic_drop"), (F32, "generic_drop_causal_128"),
                                                                                   (BF16, "generic_drop_causal_128"), (BF16, "lse_only"), (BF16, "lse_only_causal_128"), (F32, "lse_only")]


@pytest.mark.parametrize("dt,form", FWD_TRAIN_CASES)
@pytest.mark.parametrize("set_name", ["ragged", "crossing"])
def test_attention_forward_training_outputs(dt, form, set_name, tuning):
    """sl_attn_fwd with lse and dropout: out against Pd v (exact zeros where the probe's key is dropped or invisible: with klen <= D the
    probe returns keep P / (1 - p) of every (row, head, key) by itself) and lse of EVERY (row, head)"""
    kind, D, causal, drop, switches = FWD_TRAIN[form]
    if dt == F32:
        kind = "generic"
    _set(tuning, switches)
    nh, nkv = HEADS[D] if set_name == "ragged" else (64, 64)
    fails, excess, ratio = [], -1.0, 0.0
    for family in "VG":
        c = train_case(set_name, family, D, nh, nkv, causal, drop, dt)
        buf, out = guarded(c.n_tok, nh * D, dt)
        lbuf = torch.full((c.n_tok + 2, nh), FILL, device=DEV, dtype=F32)
        lse = lbuf[1:-1]
        ops.attn_fwd(c.q, c.k, c.v, out, c.cu_q, c.cu_kd, c.klen, q_strides=(c.q.stride(0), D), k_strides=(c.k.stride(0), D), v_strides=(c.v.stride(0), D),
                     o_strides=(out.stride(0), D), nseq=len(c.ql), max_qlen=max(c.ql), n_heads=nh, n_kv_heads=nkv, head_dim=D, causal=causal, scale=c.scale,
                     dropout_p=c.p, dropout_seed=DROP_SEED, lse=lse)
        assert untouched(buf, c.n_tok, nh * D) and bool((out[:c.t0] == FILL).all()), "out written outside the sequences' rows"
        assert bool((lbuf[0] == FILL).all()) and bool((lbuf[-1] == FILL).all()) and bool((lse[:c.t0] == FILL).all()), "lse written outside the sequences' rows"
        for i, s in enumerate(c.seqs):
            what = f"{family} sequence {i} ({s.nq} q / {s.nk} k)"
            check_train(out[s.q0:s.q0 + s.nq], s, "O", dt, what)
            err = (lse[s.q0:s.q0 + s.nq].double().cpu() - s.lse).abs()
            derived = s.lse_acc + LSE_OPS[kind] * s.lse_ulp
            excess, ratio = max(excess, float((err - derived).max())), max(ratio, float((err / derived).max()))
            msg = bad(lse[s.q0:s.q0 + s.nq], s.lse, derived + 4 * LSE_MEASURED[kind])
            if msg:
                fails.append(f"{what} lse: {msg}")
    print(f"lse [{kind}] worst |err| - derived part over the case: {excess:.3g} (worst |err| / derived part {ratio:.3g})")          # what LSE_MEASURED records
    assert not fails, "; ".join(fails)
