"""GPU: the GEMM side of the backward pass, every form at the smallest shape that selects it, checked PER ELEMENT (the edge suite's
fourth chapter; DESIGN.md, "Edge suite, training GEMMs").

  A  token-major weight gradient (csrc/gemm_tt.hip: gemm_tiled_tt_kernel, gemm_tiled_tt_ring_kernel, the batched launch, K runs through
     the workspace + splitk_reduce_kernel, the bias-gradient rider)
  B  the transposed-operand loader of gemm_tiled_kernel (csrc/gemm.hip p.ta / p.tw) in bf16 and fp32, overlapping conv windows, and the
     sl_transpose_pad route of ops.wgrad_acc
  C  the training epilogue riders of csrc/gemm_epilogue.h (aux_out, SL_POST_DROPOUT, SL_POST_GELU_BWD + colsum_out, SL_POST_SILU_MUL_BWD,
     colsum_out) on the rows, direct, swapped-operand and LDS-turned epilogues and behind split-K in the reduce pass
  D  K runs left to the consumer (deferred_splits) on the 128 tile

Inputs are the suite's classes: E exact integers (operands in {-2 .. 2}, dW0 / residual 8 x [-512, 512], bias and db0 in [-8, 8]: every
partial sum is an integer below 2^24, so any K run, any order and any atomic give the same fp32 value; torch.equal), G Gaussian under the
per-element bounds of tests/train_gemm_ref.py (reductions of at most 1 024 terms), Z zero probes (one non-zero token row: dW = dW0 +
dY[t]^T X[t] and db = db0 + dY[t] exactly, which pins the slab, the run and the half of the tile a token lands in).  Every output is a
`guarded` view checked `untouched` after every launch; every operand a view with a leading dimension above its extent and poisoned pad
columns; a transposed operand has 64 poisoned rows behind its last reduction row, so that a whole slab read past the tail stays inside the
buffer and shows.  dW and db accumulate onto non-zero values.  The form each shape selects is claimed in the case tables of
train_gemm_ref.py and pinned on the CPU by tests/test_train_gemm_ref_cpu.py through the dispatcher's dry run.  Nothing here compares two
forms of a kernel with each other only, and no tolerance is a measured number."""
import ctypes as C
import functools

import pytest
import torch

import train_gemm_ref as G
from conftest import pkg
from edge_helpers import BF16, BIG, DEV, F16, F32, FILL, _set, bad, gauss, guarded, ints, operand, to_dt, tuning, untouched, vec  # noqa: F401

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")

DTS = [F32, BF16]
SEED_HI = 0x5DEECE66D1234567          # a dropout seed above 2^32


def ids(specs):
    return [s["id"] for s in specs]


def t_operand(x64, dt, tail=64, wide=0):
    """x64 (rows, cols), rows = the reduction -> (device view, its stored value in fp64): one poisoned row above, `tail` behind, poisoned pad
    columns; wide: the view is the middle third of a buffer of 3 cols columns (dY as a column slice of d_qkv)"""
    rows, cols = x64.shape
    ld, c0 = (3 * cols, cols) if wide else (G.ld_of(cols), 8)
    buf = torch.full((rows + 1 + tail, ld), BIG[dt], dtype=torch.float64)
    buf[:, ::2] *= -1.0
    buf[1:rows + 1, c0:c0 + cols] = x64
    buf = buf.float().to(dt).to(DEV)
    v = buf[1:rows + 1, c0:c0 + cols]
    return v, v.double().cpu()


def acc_out(x64):
    """a guarded fp32 view holding x64 (dW0 / db0): (buffer, view)"""
    rows, cols = x64.shape
    buf, v = guarded(rows, cols, F32)
    v.copy_(x64.float().to(DEV))
    return buf, v


def launch(s, A, W, out, res=None, bias=None, aux=None, colsum=None, post_in=None, ws=None, defer=None, seed=0, drop_p=None):
    """ops.gemm_ex with every field of the spec the plan depends on; the tensors must have the spec's leading dimensions"""
    g = lambda k, d=0: s.get(k, d)
    assert A.stride(0) == s["lda"] and out.stride(0) == s["ldc"] and (res is None or res.stride(0) == s["ldr"]) and bool(g("ws")) == (ws is not None)
    assert bool(g("colsum")) == (colsum is not None) and bool(g("aux")) == (aux is not None) and bool(g("bias")) == (bias is not None)
    return ops.gemm_ex(A, W, M=s["M"], N=s["N"], K=s["K"], lda=s["lda"], ldw=s["ldw"], out=out, ldc=s["ldc"], bias=bias, residual=res, ldr=g("ldr"),
                       act=g("act"), out_f32=bool(g("out_f32")), trans_a=bool(g("ta")), trans_w=bool(g("tw")), residual_f32=bool(g("res_f32")), aux_out=aux,
                       batch=g("batch", 1), strideA=g("sA"), strideW=g("sW"), strideC=g("sC"), strideR=g("sR"), dtype=s["dt"], sk_ws=ws, post_op=g("post"),
                       drop_p=g("drop_p", 0.0) if drop_p is None else drop_p, drop_seed=seed, drop_ld=g("drop_ld"), post_in=post_in, post_ld=g("post_ld"),
                       colsum_out=colsum, deferred_splits=defer)


def flags_zero(ws):
    return ws is None or int(ws[:1024].to(torch.int32).abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# A. token-major weight gradient
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_data(cls, M, N, K, seed):
    """(dy (K, M), x (K, N), dW0, db0) in fp64 on the CPU, shared by the forms that run the same shape"""
    if cls == "E":
        return ints((K, M), -2, 2, seed), ints((K, N), -2, 2, seed + 1), 8 * ints((M, N), -512, 512, seed + 2), ints((1, M), -8, 8, seed + 3) + 0.0
    return gauss((K, M), seed), gauss((K, N), seed + 1), gauss((M, N), seed + 2), gauss((1, M), seed + 3)


def wgrad_run(s, dyv, xv, dw0, db0, ws, rider):
    """one accumulate launch onto fresh guarded copies of dW0 (residual and output) and db0: (dW, db) on the CPU"""
    M, N = s["M"], s["N"]
    bufw, dw = acc_out(dw0)
    bufb, db = acc_out(db0) if rider else (None, None)
    launch(dict(s, colsum=int(rider)), dyv, xv, dw, res=dw, colsum=db, ws=ws)
    assert untouched(bufw, M, N), "dW: write outside [0:M, 0:N]"
    assert not rider or untouched(bufb, 1, M), "db: write outside [0:M]"
    assert flags_zero(ws), "the flag area in front of the partial tiles is not zero"
    return dw.cpu(), (db.cpu() if rider else None)


def wgrad_check(s, ws=None, rider=True, probes=()):
    """classes E, G (reductions of at most 1 024 terms) and Z of one weight-gradient spec; rider: the spec may carry colsum_out"""
    M, N, K, dt, wide = s["M"], s["N"], s["K"], s["dt"], s["lda"] == 3 * s["M"]
    tag = f"{s['id']} {(M, N, K)}"
    # E
    dy, x, dw0, db0 = wgrad_data("E", M, N, K, 300)
    dyv, dy64 = t_operand(dy, dt, wide=wide)
    xv, x64 = t_operand(x, dt)
    want_w, want_b = (dw0 + dy64.T @ x64).float(), (db0 + dy64.sum(0)).float()
    plain, _ = wgrad_run(s, dyv, xv, dw0, db0, ws, False)
    assert not (msg := bad(plain, want_w)), f"E dW {tag}: {msg}"
    again, _ = wgrad_run(s, dyv, xv, dw0, db0, ws, False)
    assert not (msg := bad(again, plain, bits=True)), f"E dW, second call {tag}: {msg}"
    if rider:
        with_db, db = wgrad_run(s, dyv, xv, dw0, db0, ws, True)
        assert not (msg := bad(with_db, plain, bits=True)), f"E dW with the rider {tag}: {msg}"
        assert not (msg := bad(db, want_b)), f"E db {tag}: {msg}"
    # Z: one token row
    for t in sorted({0, 63, 64, K - 1, *probes}):
        row = dy64[t].clone()
        row[row == 0] = 1.0
        dyv.zero_()
        dyv[t] = row.to(dt).to(DEV)
        assert torch.equal(dyv.double().cpu()[t], row) and float(dyv.double().abs().sum()) == float(row.abs().sum())
        dw, db = wgrad_run(s, dyv, xv, dw0, db0, ws, rider)
        assert not (msg := bad(dw, (dw0 + torch.outer(row, x64[t])).float())), f"Z dW token {t} {tag}: {msg}"
        if rider:
            assert not (msg := bad(db, (db0 + row).float())), f"Z db token {t} {tag}: {msg}"
    # G
    if G.class_g(s):
        dy, x, dw0, db0 = wgrad_data("G", M, N, K, 310)
        dyv, dy64 = t_operand(dy, dt, wide=wide)
        xv, x64 = t_operand(x, dt)
        dw0, db0 = dw0.float().double(), db0.float().double()
        r = G.wgrad_ref(dy64, x64, dw0, db0)
        dw, db = wgrad_run(s, dyv, xv, dw0, db0, ws, rider)
        assert not (msg := bad(dw, r.dw, r.tol_dw)), f"G dW {tag}: {msg}"
        if rider:
            assert not (msg := bad(db, r.db, r.tol_db)), f"G db {tag}: {msg}"
        dw2, _ = wgrad_run(s, dyv, xv, dw0, db0, ws, rider)
        assert not (msg := bad(dw2, dw, bits=True)), f"G dW, second call {tag}: {msg}"


TT = G.tt_cases()


@pytest.mark.parametrize("s", [s for s in TT if not s["ws"]], ids=ids([s for s in TT if not s["ws"]]))
def test_wgrad_token_major_one_run(s, tuning):
    """gemm_tiled_tt_kernel (2 ... 7 slabs, even and odd counts of the double buffer, tails of 1, 63 and 0 rows) and gemm_tiled_tt_ring_kernel
    (8, 9, 10, 16 slabs: the steady loop taken once and several times, the three-slab drain; SL_TT_RING=0: the two-stage kernel on the same
    shapes, against the same reference, hence the same bits in class E), at one tile and at 2 x 3 tiles with dY a column slice of a buffer three
    times as wide.  With and without the bias-gradient rider: dW keeps its bits, the second row tile's rows are written once, only the first
    column tile adds."""
    _set(tuning, s["env"])
    wgrad_check(s)


@pytest.mark.parametrize("s", [s for s in TT if s["ws"]], ids=ids([s for s in TT if s["ws"]]))
def test_wgrad_token_major_k_runs(s, tuning):
    """K runs through the workspace + splitk_reduce_kernel: 2 runs of 13 and 12 slabs, 8 runs with a last one of 6 (the shortest the default
    switches reach), and with SL_TT_MAX_SPLITS=16 thirteen runs whose last has ONE slab and two slabs - the ring kernel's `n <= 3` path; the
    same on the two-stage kernel and under SL_SPLITK_SLOTS=256.  Classes E and Z only (long reductions); probes at the last row of the first
    run and the first row of the last."""
    _set(tuning, s["env"])
    S, krun = int(s["plan"].split("S=")[1].split()[0]), int(s["plan"].split("krun=")[1].split()[0])
    assert s["K"] > G.G_MAX_K
    wgrad_check(s, ws=ops.streamk_workspace(DEV), probes=(krun * G.BK - 1, (S - 1) * krun * G.BK))


@pytest.mark.parametrize("s", G.tt_refused_cases(), ids=ids(G.tt_refused_cases()))
def test_wgrad_shapes_the_token_major_kernel_refuses_stay_right(s):
    """M = 192, K = 127, N = 136 and fp32 do not select the kernel (the dry-run plan says reg128): the product through the register-staged loader.
    (A leading dimension that is no multiple of 8 elements is an argument error of sl_gemm itself.)"""
    wgrad_check(s, rider=False)
    if s["id"] == "ttref-m192":
        dy, x, dw0, db0 = wgrad_data("E", s["M"], s["N"], s["K"], 300)
        dyv, xv = t_operand(dy, BF16)[0], t_operand(x, BF16)[0]
        with pytest.raises(L.SpeechLLMError):          # the rider exists in the token-major kernel only
            wgrad_run(s, dyv, xv, dw0, db0, None, True)
        with pytest.raises(L.SpeechLLMError):          # rows of 8 k + 4 elements: refused before any launch
            ops.gemm_ex(dyv, xv, M=s["M"], N=s["N"], K=s["K"], lda=s["lda"] + 4, ldw=s["ldw"], out=acc_out(dw0)[1], ldc=s["ldc"], out_f32=True, trans_a=True,
                        trans_w=True, dtype=BF16)


@pytest.mark.parametrize("M,batch,K,spaced", [(M, b, K, sp) for M, b, K in G.TTB for sp in (True, False)])
def test_wgrad_token_major_batched(M, batch, K, spaced, tuning):
    """SL_TT_BATCHED (blockIdx.z) with the positional conv's strides (lda 1 024, ldw 2 048, batch strides 64 and 128 columns): at M = 64 the
    upper half of the tile reads the zero constant and rows 64 ... 127 of a batch's C slab keep the sentinel (slabs 128 rows apart) or the
    neighbouring batch's values (slabs back to back).  SL_TT_BATCHED=0: the register-staged loader, against the same references."""
    N, dt = 128, BF16
    rows_per = 128 if spaced else M
    rows = rows_per * (batch - 1) + M
    wa, ww = G.TTB_SA * (batch - 1) + M, G.TTB_SW * (batch - 1) + N
    for off in (False, True):
        s = G.ttb_spec(M, batch, K, spaced, env=dict(SL_TT_BATCHED="0") if off else None)
        tuning("SL_TT_BATCHED", "0" if off else "1")
        for cls in "EG":
            mk = (lambda sh, sd: ints(sh, -2, 2, sd)) if cls == "E" else gauss
            buf_a = torch.full((K + 65, G.TTB_LDA), BIG[dt], dtype=torch.float64)
            buf_w = torch.full((K + 65, G.TTB_LDW), BIG[dt], dtype=torch.float64)
            buf_a[:, ::2] *= -1.0
            buf_w[:, ::2] *= -1.0
            buf_a[1:K + 1, :wa] = mk((K, wa), 320)
            buf_w[1:K + 1, :ww] = mk((K, ww), 321)
            da, dw_ = buf_a.float().to(dt).to(DEV), buf_w.float().to(dt).to(DEV)
            a64, w64 = da[1:K + 1, :wa].double().cpu(), dw_[1:K + 1, :ww].double().cpu()
            dw0 = (8 * ints((rows, N), -512, 512, 322) if cls == "E" else gauss((rows, N), 322)).float().double()
            want = torch.full((rows, N), FILL, dtype=torch.float64)
            tol = torch.zeros((rows, N), dtype=torch.float64)
            init = want.clone()
            for b in range(batch):
                r = G.wgrad_ref(a64[:, G.TTB_SA * b:G.TTB_SA * b + M], w64[:, G.TTB_SW * b:G.TTB_SW * b + N], dw0[rows_per * b:rows_per * b + M])
                want[rows_per * b:rows_per * b + M], tol[rows_per * b:rows_per * b + M] = r.dw, r.tol_dw
                init[rows_per * b:rows_per * b + M] = dw0[rows_per * b:rows_per * b + M]
            bufc, c = acc_out(init)
            launch(s, da[1:], dw_[1:], c, res=c)
            assert untouched(bufc, rows, N), "dW: write outside the batches' rows"
            msg = bad(c, want.float()) if cls == "E" else bad(c, want, tol)
            assert not msg, f"{cls} batched{' off' if off else ''} {(M, batch, K, spaced)}: {msg}"
            if not off:
                bufc2, c2 = acc_out(init)
                launch(s, da[1:], dw_[1:], c2, res=c2)
                assert not (msg := bad(c2, c, bits=True)), f"second call: {msg}"


# ------------------------------------------------------------------------------------------------------------------------------
# B. register-staged transposed loader
# ------------------------------------------------------------------------------------------------------------------------------
def reg_operands(s, a64, w64):
    """a64 (M, K), w64 (N, K) logical -> device views stored as the spec says, and their stored values (logical orientation)"""
    dt = s["dt"]
    if s.get("ta"):
        av, st = t_operand(a64.T.contiguous(), dt)
        a_st = st.T
    else:
        av, a_st = operand(a64, dt)
    if s.get("tw"):
        wv, st = t_operand(w64.T.contiguous(), dt)
        w_st = st.T
    else:
        wv, w_st = operand(w64, dt)
    assert av.stride(0) == s["lda"] and wv.stride(0) == s["ldw"]
    return av, a_st, wv, w_st


def reg_run(s, av, wv, bias=None, res=None):
    buf, out = guarded(s["M"], s["N"], s["dt"])
    launch(dict(s, bias=int(bias is not None), res=int(res is not None)), av, wv, out, res=res, bias=bias)
    assert untouched(buf, s["M"], s["N"]), "write outside [0:M, 0:N]"
    return out


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(G.reg_cases(F32))), ids=ids(G.reg_cases(F32)))
def test_transposed_operand_loader(i, dt):
    """gemm_tiled_kernel with trans_w (dgrad), trans_a, and both: 16-byte chunks run along the OUTPUT index, so M / N = 70, 203 (bf16: 8-element
    chunks; fp32: 4-element chunks) have a last chunk that straddles the extent - its tail elements are the poisoned pad columns and land in
    tile rows that are never stored; K = 8 ... 200 (both transposed: also 1, 63, 65, 129) ends inside a slab, rows behind K are poisoned."""
    s = G.reg_cases(dt)[i]
    M, N, K = s["M"], s["N"], s["K"]
    tag = f"{s['id']} {dt}"
    # E
    av, a64, wv, w64 = reg_operands(s, ints((M, K), -2, 2, 400), ints((N, K), -2, 2, 401))
    r, r64 = operand(8 * ints((M, N), -512, 512, 403), dt)
    b, b64 = vec(ints((N,), -8, 8, 402), dt)
    y = a64 @ w64.T
    assert not (msg := bad(reg_run(s, av, wv), to_dt(y, dt))), f"E plain {tag}: {msg}"
    assert not (msg := bad(reg_run(s, av, wv, bias=b, res=r), to_dt(y + b64 + r64, dt))), f"E bias+residual {tag}: {msg}"
    # Z: one reduction index
    for k in sorted({0, K // 2, K - 1}):
        a1, w1 = torch.zeros_like(a64), torch.zeros_like(w64)
        a1[:, k], w1[:, k] = torch.where(a64[:, k] == 0, 1.0, a64[:, k]), torch.where(w64[:, k] == 0, 1.0, w64[:, k])
        av1, _, wv1, _ = reg_operands(s, a1, w1)
        assert not (msg := bad(reg_run(s, av1, wv1), to_dt(torch.outer(a1[:, k], w1[:, k]), dt))), f"Z k={k} {tag}: {msg}"
    # G
    av, a64, wv, w64 = reg_operands(s, gauss((M, K), 410), gauss((N, K), 411, K ** -0.5))
    r, r64 = operand(gauss((M, N), 413), dt)
    b, b64 = vec(gauss((N,), 412), dt)
    ref = G.plain_ref(a64, w64, dt, bias=b64, res=r64)
    got = reg_run(s, av, wv, bias=b, res=r)
    assert not (msg := bad(got, ref.c, ref.tol_c)), f"G bias+residual {tag}: {msg}"
    assert not (msg := bad(reg_run(s, av, wv, bias=b, res=r), got, bits=True)), f"G second call {tag}: {msg}"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", G.CONV_WINDOWS)
def test_wgrad_over_overlapping_conv_windows_per_element(geom, dt):
    """ldw < N: X (Lin, C) read as Lo overlapping windows of k C elements, row stride s C (the implicit-GEMM conv weight gradient), both
    operands transposed; rows in front of and behind X are poisoned, the last window ends on X's last element"""
    Lin, Cc, k, s_ = geom
    s = G.conv_spec(dt, *geom)
    Lo, M, N = s["K"], s["M"], s["N"]
    assert (Lo - 1) * s_ + k == Lin
    for cls in "EGZ":
        x = ints((Lin, Cc), -2, 2, 420) if cls != "G" else gauss((Lin, Cc), 420)
        dy = ints((Lo, M), -2, 2, 421) if cls != "G" else gauss((Lo, M), 421)
        dw0 = (8 * ints((M, N), -512, 512, 422) if cls != "G" else gauss((M, N), 422)).float().double()
        for t in ([0, Lo - 1] if cls == "Z" else [None]):
            if t is not None:
                keep = torch.zeros(Lo, 1, dtype=torch.float64)
                keep[t] = 1.0
                dy = torch.where(ints((Lo, M), -2, 2, 421) == 0, 1.0, ints((Lo, M), -2, 2, 421)) * keep
            buf = torch.full((Lin + 72, Cc), BIG[dt], dtype=torch.float64)
            buf[::2] *= -1.0
            buf[8:8 + Lin] = x
            xd = buf.float().to(dt).to(DEV)
            x64 = G.windows(xd[8:8 + Lin].double().cpu(), Lo, k, s_)
            dyv, dy64 = t_operand(dy, dt)
            r = G.wgrad_ref(dy64, x64, dw0)
            bufw, dw = acc_out(dw0)
            launch(s, dyv, xd[8:], dw, res=dw)
            assert untouched(bufw, M, N)
            msg = bad(dw, r.dw, r.tol_dw) if cls == "G" else bad(dw, r.dw.float())
            assert not msg, f"{cls} conv windows {geom} {dt} token {t}: {msg}"


def test_both_routes_of_a_doubly_transposed_bf16_product_agree_exactly(tuning):
    """128 x 128 x 200 tokens: the token-major kernel (default) and, under SL_WGRAD_TR=0, the register-staged loader - each against the exact
    integer product, so they agree bit for bit"""
    for s in G.tt_route_cases(BF16):
        tuning("SL_WGRAD_TR", s["env"].get("SL_WGRAD_TR", "1"))
        wgrad_check(s, rider=False)


@pytest.mark.parametrize("dt,T,No,Ni", [(dt, *c) for dt in DTS for c in G.TPAD[dt]])
def test_wgrad_acc_through_transposed_copies(dt, T, No, Ni):
    """ops.wgrad_acc at 256 token rows and more where the token-major kernel does not apply (fp32; bf16 with 192 input columns):
    sl_transpose_pad copies, zero-filled to a whole number of slabs, then the plain LDS-DMA product.  Class E, exact."""
    dy, x, dw0, _ = wgrad_data("E", No, Ni, T, 430)
    dyv, dy64 = t_operand(dy, dt)
    xv, x64 = t_operand(x, dt)
    bufw, dw = acc_out(dw0)
    ops.wgrad_acc(dyv, xv, dw)
    assert untouched(bufw, No, Ni)
    assert not (msg := bad(dw, (dw0 + dy64.T @ x64).float())), f"E wgrad_acc {(T, No, Ni)} {dt}: {msg}"


# ------------------------------------------------------------------------------------------------------------------------------
# C. training epilogue riders
# ------------------------------------------------------------------------------------------------------------------------------
def epi_inputs(s, cls, seed):
    M, N, K, dt = s["M"], s["N"], s["K"], s["dt"]
    if cls == "E":
        a, w = ints((M, K), -2, 2, seed), ints((N, K), -2, 2, seed + 1)
    else:
        a, w = gauss((M, K), seed), gauss((N, K), seed + 1, K ** -0.5)
    av, a64 = operand(a, dt)
    wv, w64 = operand(w, dt)
    assert av.stride(0) == s["lda"] and wv.stride(0) == s["ldw"]
    return av, a64, wv, w64


def epi_db(N, cls, seed):
    db0 = (ints((1, N), -8, 8, seed) + 0.0) if cls == "E" else gauss((1, N), seed).float().double()
    return db0, *acc_out(db0)


def epi_ws(s):
    return ops.streamk_workspace(DEV) if s.get("ws") else None


EPI = [(dt, s) for dt in DTS for s in G.epi_cases(dt)]


def epi_param(feature):
    sel = [(dt, s) for dt, s in EPI if s["feature"].split("+")[0] == feature]
    return pytest.mark.parametrize("dt,s", sel, ids=[f"{s['id']}-{'f32' if dt == F32 else 'bf16'}" for dt, s in sel])


@epi_param("auxgelu")
def test_epilogue_aux_out_with_gelu(dt, s, tuning):
    """aux_out = the pre-activation (exact in class E), C = gelu(pre as computed in fp32)"""
    _set(tuning, s["env"])
    M, N = s["M"], s["N"]
    for cls in ("EG" if G.class_g(s) else "E"):
        av, a64, wv, w64 = epi_inputs(s, cls, 500)
        b, b64 = vec(ints((N,), -8, 8, 502) if cls == "E" else gauss((N,), 502), dt)
        r = G.aux_gelu_ref(a64, w64, b64, dt)
        bufc, c = guarded(M, N, dt)
        bufa, aux = guarded(M, N, dt)
        launch(s, av, wv, c, bias=b, aux=aux)
        assert untouched(bufc, M, N) and untouched(bufa, M, N)
        msg = bad(aux, to_dt(r.aux, dt)) if cls == "E" else bad(aux, r.aux, r.tol_aux)
        assert not msg, f"{cls} aux {s['id']} {dt}: {msg}"
        assert not (msg := bad(c, r.c, r.tol_c)), f"{cls} gelu {s['id']} {dt}: {msg}"


@epi_param("drop")
def test_epilogue_dropout_onto_the_residual(dt, s, tuning):
    """C = R + keep (A W^T + b) / (1 - p) with the mask of ops.dropout_keep_at on row * drop_ld + col (drop_ld differs from N and ldc, the seed
    is above 2^32): p = 0.5 in class E (the scale 2 is exact: torch.equal on the chain of roundings), a zero residual (dropped elements +0
    bit for bit), p = 0.25 in class G"""
    _set(tuning, s["env"])
    M, N = s["M"], s["N"]
    assert s["drop_ld"] not in (N, s["ldc"])
    ws = epi_ws(s)
    for cls, p_ in (("E", 0.5), ("E0", 0.5), ("G", 0.25))[:3 if G.class_g(s) else 2]:
        av, a64, wv, w64 = epi_inputs(s, cls[0], 510)
        b, b64 = vec(ints((N,), -8, 8, 512) if cls != "G" else gauss((N,), 512), dt)
        res = 8 * ints((M, N), -512, 512, 513) if cls == "E" else torch.zeros(M, N, dtype=torch.float64) if cls == "E0" else gauss((M, N), 513)
        rv, r64 = operand(res, dt)
        keep = G.keep_mask(M, N, s["drop_ld"], p_, SEED_HI)
        assert 0.2 < float(keep.double().mean()) < 0.9
        bufc, c = guarded(M, N, dt)
        launch(s, av, wv, c, res=rv, bias=b, ws=ws, seed=SEED_HI, drop_p=p_)
        assert untouched(bufc, M, N) and flags_zero(ws)
        if cls == "G":
            r = G.dropout_ref(a64, w64, b64, r64, keep, p_, dt)
            assert not (msg := bad(c, r.c, r.tol_c)), f"G dropout {s['id']} {dt}: {msg}"
        else:
            want = to_dt(r64 + 2.0 * keep.double() * to_dt(a64 @ w64.T + b64, dt).double(), dt)
            assert not (msg := bad(c, want, bits=cls == "E0")), f"{cls} dropout {s['id']} {dt}: {msg}"


@epi_param("gbwd")
def test_epilogue_gelu_backward(dt, s, tuning):
    """C = gelu'(pre) dropout(dY W): pre = +16 gives dropout(dY W) exactly and pre = -16 zeros (class E, p in {0, 0.5}); Gaussian pre under the
    composed bound (p in {0, 0.25}).  colsum_out, where the spec carries it: db0 + the column sums of the STORED C - exact in class E"""
    _set(tuning, s["env"])
    M, N = s["M"], s["N"]
    ws = epi_ws(s)
    rider = bool(s.get("colsum"))
    for cls, p_ in (("E", 0.0), ("E", 0.5), ("G", 0.0), ("G", 0.25))[:4 if G.class_g(s) else 2]:
        av, a64, wv, w64 = epi_inputs(s, cls, 520)
        keep = G.keep_mask(M, N, s["drop_ld"], p_, SEED_HI + 1) if p_ > 0 else None
        sign = torch.where(ints((M, N), 0, 1, 523) > 0, 1.0, -1.0)
        pre = 16.0 * sign if cls == "E" else gauss((M, N), 523, 2.0)
        pv, pre64 = operand(pre, dt)
        assert pv.stride(0) == s["post_ld"]
        db0, bufb, db = epi_db(N, cls, 524)
        bufc, c = guarded(M, N, dt)
        launch(s, av, wv, c, post_in=pv, colsum=db if rider else None, ws=ws, seed=SEED_HI + 1, drop_p=p_)
        assert untouched(bufc, M, N) and untouched(bufb, 1, N) and flags_zero(ws)
        if cls == "E":
            d = to_dt(a64 @ w64.T, dt).double()
            if p_ > 0:
                d = to_dt(2.0 * keep.double() * d, dt).double()
            msg = bad(c, to_dt(torch.where(sign > 0, d, 0.0), dt))
        else:
            r = G.gelu_bwd_post_ref(a64, w64, pre64, keep, p_, dt)
            msg = bad(c, r.c, r.tol_c)
        assert not msg, f"{cls} gelu_bwd p={p_} {s['id']} {dt}: {msg}"
        if rider:
            rb = G.colsum_ref(c.double().cpu(), db0)
            msg = bad(db, rb.db.float()) if cls == "E" else bad(db, rb.db, rb.tol_db)
            assert not msg, f"{cls} db p={p_} {s['id']} {dt}: {msg}"
        else:
            assert bool((db == db0.float().to(DEV)).all())


@epi_param("silubwd")
def test_epilogue_swiglu_backward(dt, s, tuning):
    """(d gate | d up) in 16-column blocks of an (M, 2 F) output with ldc = post_ld > 2 F: gates at +104 (d u and 104 d exactly) and -104
    (zeros) in class E, Gaussian gates under the composed bound; F = 96, 144, 208 are no multiple of the 64-column wave tile"""
    _set(tuning, s["env"])
    M, F_ = s["M"], s["N"]
    ws = epi_ws(s)
    for cls in ("EG" if G.class_g(s) else "E"):
        av, a64, wv, w64 = epi_inputs(s, cls, 530)
        if cls == "E":
            sign = torch.where(ints((M, F_), 0, 1, 533) > 0, 1.0, -1.0)
            g, up = 104.0 * sign, ints((M, F_), -2, 2, 534) + 0.0
        else:
            g, up = gauss((M, F_), 533, 2.0), gauss((M, F_), 534)
        guv, gu64 = operand(G.interleave(g, up), dt)
        g64, up64 = G.R.deinterleave(gu64)
        assert guv.stride(0) == s["post_ld"] == s["ldc"]
        bufc, c = guarded(M, 2 * F_, dt)
        launch(s, av, wv, c, post_in=guv, ws=ws)
        assert untouched(bufc, M, 2 * F_) and flags_zero(ws)
        dg, du = G.R.deinterleave(c.cpu().contiguous())
        if cls == "E":
            d = to_dt(a64 @ w64.T, dt).double()
            want_g, want_u = to_dt(torch.where(sign > 0, d * up64, 0.0), dt), to_dt(torch.where(sign > 0, d * 104.0, 0.0), dt)
            msg = bad(dg, want_g) or bad(du, want_u)
        else:
            r = G.silu_bwd_post_ref(a64, w64, g64, up64, dt)
            msg = bad(dg, r.dgate, r.tol_dgate) or bad(du, r.dup, r.tol_dup)
        assert not msg, f"{cls} silu_mul_bwd {s['id']} {dt}: {msg}"


@epi_param("db")
def test_epilogue_colsum_alone(dt, s, tuning):
    """colsum_out on a plain product: db0 + the column sums of the stored C"""
    _set(tuning, s["env"])
    M, N = s["M"], s["N"]
    for cls in ("EG" if G.class_g(s) else "E"):
        av, a64, wv, w64 = epi_inputs(s, cls, 540)
        db0, bufb, db = epi_db(N, cls, 544)
        bufc, c = guarded(M, N, dt)
        launch(s, av, wv, c, colsum=db)
        assert untouched(bufc, M, N) and untouched(bufb, 1, N)
        r = G.plain_ref(a64, w64, dt)
        msg = bad(c, to_dt(r.c, dt)) if cls == "E" else bad(c, r.c, r.tol_c)
        assert not msg, f"{cls} C {s['id']} {dt}: {msg}"
        rb = G.colsum_ref(c.double().cpu(), db0)
        msg = bad(db, rb.db.float()) if cls == "E" else bad(db, rb.db, rb.tol_db)
        assert not msg, f"{cls} db {s['id']} {dt}: {msg}"


def test_training_features_are_refused_in_fp16():
    A, W = torch.zeros((128, 64), device=DEV, dtype=F16), torch.zeros((128, 64), device=DEV, dtype=F16)
    out, f32 = torch.empty((128, 128), device=DEV, dtype=F16), torch.zeros((128,), device=DEV, dtype=F32)
    for kw in (dict(trans_a=True), dict(trans_w=True), dict(post_op=L.POST_DROPOUT, drop_p=0.5, drop_ld=128), dict(colsum_out=f32), dict(aux_out=torch.empty_like(out))):
        with pytest.raises(L.SpeechLLMError):
            ops.gemm_ex(A, W, M=128, N=128, K=64, lda=64, ldw=64, out=out, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# D. K runs left to the consumer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_deferred_k_runs_of_the_128_tile(dt):
    """deferred_splits at 130 x 132 under 32 slabs (the rule's lower edge): *deferred_splits = 2, the two fp32 partial products behind the flag
    area sum (on the host, fp64) to exactly the product, C keeps its sentinel everywhere, and a single non-zero K column shows in its own
    run's slab only.  31 slabs: *deferred_splits = 0 and C is written."""
    cut, not_cut = G.defer_cases(dt)
    M, N, K = cut["M"], cut["N"], cut["K"]
    ws = ops.streamk_workspace(DEV)

    def run(s, a64_, w64_):
        av, a64, wv, w64 = (operand(a64_, dt) + operand(w64_, dt))
        S = C.c_int32(-1)
        buf, out = guarded(M, N, dt)
        launch(s, av, wv, out, ws=ws, defer=S)
        assert flags_zero(ws)
        parts = ws[1024:1024 + S.value * M * N * 4].view(F32).view(S.value, M, N).double().cpu() if S.value > 0 else None
        return S.value, buf, out, parts, a64 @ w64.T

    a, w = ints((M, K), -2, 2, 600), ints((N, K), -2, 2, 601)
    S, buf, out, parts, y = run(cut, a, w)
    assert S == 2 and bool((buf == FILL).all()), (S, "C was written")
    assert not (msg := bad(parts.sum(0), y)), f"E sum of the partial products {dt}: {msg}"
    assert not (msg := bad(parts[0], a[:, :K // 2] @ w[:, :K // 2].T)), f"E run 0 {dt}: {msg}"
    for k in (0, K // 2 - 1, K // 2, K - 1):
        a1, w1 = torch.zeros_like(a), torch.zeros_like(w)
        a1[:, k], w1[:, k] = torch.where(a[:, k] == 0, 1.0, a[:, k]), torch.where(w[:, k] == 0, 1.0, w[:, k])
        S, buf, out, parts, y = run(cut, a1, w1)
        z = k // (K // 2)
        assert S == 2 and bool((buf == FILL).all())
        assert not (msg := bad(parts[z], y)), f"Z column {k} in run {z} {dt}: {msg}"
        assert not bool(parts[1 - z].any()), f"Z column {k}: run {1 - z} is not zero"
    K1 = not_cut["K"]
    S, buf, out, parts, y = run(not_cut, a[:, :K1].contiguous(), w[:, :K1].contiguous())
    assert S == 0 and untouched(buf, M, N)
    assert not (msg := bad(out, to_dt(y, dt))), f"E 31 slabs {dt}: {msg}"
