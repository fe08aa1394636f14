"""GPU: the encoder's front end and its ragged-batch forms, checked PER ELEMENT (the edge suite's front-end chapter).

Everything between the waveform and the first transformer layer plus the pooling behind the last one: csrc/conv.hip (conv0 + LayerNorm +
GELU, the positional conv's staging, AvgPool and range means, each alone and as one launch over a ragged batch), csrc/whisper.hip (the
log-mel front end) and the three grouped / strided implicit-convolution launches csrc/runtime.hip builds around them.  Reference and
bounds: tests/frontend_ref.py, fp64 on the same rounded inputs (tests/test_frontend_ref_cpu.py pins them); DESIGN.md, "edge suite",
front end.  As everywhere in the suite: outputs are views into sentinel-filled buffers whose guards must come back untouched (the
wrappers of ops.py allocate their own outputs, so the kernels are called through ctypes), inputs sit between finite poison, no tolerance
is a measured number and nothing compares one kernel form with another alone.
"""
import pytest
import torch

import frontend_ref as R
from conftest import pkg
from edge_helpers import (BF16, BIG, DEV, DTS, E24, F32, FILL, U, bad, gauss, guarded, guarded_flat, ints, operand, operand_flat, to_dt, untouched,
                          untouched_flat, vec)

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
weights = pkg("weights")

GELU = L.ACT_GELU
EPS = 1e-5


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def cumsum0(v):
    out = [0]
    for x in v:
        out.append(out[-1] + int(x))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# conv0 + LayerNorm + GELU, single and batched
# ------------------------------------------------------------------------------------------------------------------------------
CONV0_L = [1, 23, 24, 25, 95, 96, 97, 193]          # around the strip (24 steps per wave) and the block (4 waves = 96 steps)


def conv0_params(Cout, seed, equal_bias=False):
    """fp32 device tensors (the kernel takes fp32 parameters in every output type) and their fp64 values"""
    w, w64 = vec(gauss((Cout, 10), seed, 10 ** -0.5), F32)
    b, b64 = vec(torch.full((Cout,), 0.5, dtype=torch.float64) if equal_bias else gauss((Cout,), seed + 1, 0.5), F32)
    g, g64 = vec(1.0 + gauss((Cout,), seed + 2, 0.1), F32)
    be, be64 = vec(gauss((Cout,), seed + 3, 0.1), F32)
    return (w, b, g, be), (w64, b64, g64, be64)


def conv0_wave(Lout, r, seed, silence=None):
    """n = 5 (Lout - 1) + 10 + r samples, the r tail samples (which no window reaches) +-BIG; silence = (first, end) samples of exact zeros"""
    n = 5 * (Lout - 1) + 10 + r
    x = gauss((n,), seed)
    if silence:
        x[silence[0]:silence[1]] = 0.0
    for i in range(r):
        x[n - 1 - i] = BIG[F32] * (-1.0) ** i
    return x


def conv0_check(got, wave64, p64, dt, what):
    r = R.conv0_ref(wave64, *p64, U[dt], EPS)
    msg = bad(got, r.ref, r.tol)
    assert not msg, f"{what}: {msg}"
    return r


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cout", [64, 128, 256, 512])          # 16-bit: 512 stores 16-byte vectors, the rest scalars; fp32: 256 and 512 / 64 and 128
def test_conv0_single_per_element(dt, Cout):
    dev, p64 = conv0_params(Cout, 900 + Cout)
    for i, Lout in enumerate(CONV0_L):
        r_tail = i % 5                                          # every r in 0..4 appears
        silence = (300, 420) if Lout == 193 else None           # digital silence: rows 60 .. 82 are the bias alone
        wave, wave64 = operand_flat(conv0_wave(Lout, r_tail, 910 + i, silence), F32)
        buf, out = guarded_flat(Lout * Cout, dt)
        L.check(L.lib().sl_hubert_conv0(wave.data_ptr(), wave.numel(), *[t.data_ptr() for t in dev], out.data_ptr(), Cout, 10, 5, EPS, L.dtype_code(dt),
                                        L.stream_ptr()), "sl_hubert_conv0")
        assert untouched_flat(buf, Lout * Cout), f"L = {Lout}: written outside the {Lout} rows"
        r = conv0_check(out.view(Lout, Cout), wave64, p64, dt, f"C = {Cout}, L = {Lout}, r = {r_tail}")
        if silence:
            assert torch.equal(r.pre[60:83], p64[1].expand(23, Cout))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cout", [64, 512])
def test_conv0_zero_variance_gives_gelu_of_beta(dt, Cout):
    """All biases 0.5 and a silent stretch: every channel of those rows is 0.5, sums of 0.5 are exact in any order, so mean = 0.5, the
    variance is exactly 0 and the row is gelu(beta): no 0 x rstd surprise, and only the erf allowance and the output rounding remain"""
    dev, p64 = conv0_params(Cout, 930, equal_bias=True)
    Lout = 49
    wave, wave64 = operand_flat(conv0_wave(Lout, 2, 931, silence=(100, 200)), F32)          # rows 20 .. 38 read zeros only
    buf, out = guarded_flat(Lout * Cout, dt)
    L.check(L.lib().sl_hubert_conv0(wave.data_ptr(), wave.numel(), *[t.data_ptr() for t in dev], out.data_ptr(), Cout, 10, 5, EPS, L.dtype_code(dt),
                                    L.stream_ptr()), "sl_hubert_conv0")
    assert untouched_flat(buf, Lout * Cout)
    r = conv0_check(out.view(Lout, Cout), wave64, p64, dt, "zero variance")
    assert bool((r.var[20:39] == 0).all())
    ref = R.gelu64(p64[3]).expand(19, Cout)
    msg = bad(out.view(Lout, Cout)[20:39], ref, 2 * U[dt] * ref.abs() + R.TRANS * (1 + p64[3].abs()) + E24)
    assert not msg, "silent rows: " + msg


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cout", [64, 512])
def test_conv0_batch_per_utterance(dt, Cout):
    """One launch over lengths [97, 1, 24, 193, 25], then the same utterances in another order (max_L not at index 0); every utterance
    against the reference of that utterance ALONE, so a strip that reads its neighbour's samples or writes its neighbour's rows shows"""
    dev, p64 = conv0_params(Cout, 940 + Cout)
    lens = [97, 1, 24, 193, 25]
    waves = [conv0_wave(Lo, u, 950 + u, (300, 420) if Lo == 193 else None) for u, Lo in enumerate(lens)]          # r = 0 .. 4 tail samples, poisoned
    for order in ([0, 1, 2, 3, 4], [4, 1, 3, 0, 2]):
        ws, ls = [waves[u] for u in order], [lens[u] for u in order]
        flat, flat64 = operand_flat(torch.cat(ws), F32)
        soff, row0 = cumsum0(w.numel() for w in ws), cumsum0(ls)
        desc = i64([soff, row0])
        buf, out = guarded_flat(row0[-1] * Cout, dt)
        L.check(L.lib().sl_hubert_conv0_batch(flat.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(ls), max(ls), *[t.data_ptr() for t in dev],
                                              out.data_ptr(), Cout, 10, 5, EPS, L.dtype_code(dt), L.stream_ptr()), "sl_hubert_conv0_batch")
        assert untouched_flat(buf, row0[-1] * Cout), "written outside the packed rows"
        o = out.view(row0[-1], Cout)
        for u in range(len(ls)):
            conv0_check(o[row0[u]:row0[u + 1]], flat64[soff[u]:soff[u + 1]], p64, dt, f"order {order}, utterance {u} (L = {ls[u]})")


# ------------------------------------------------------------------------------------------------------------------------------
# positional conv staging: a copy, so the bits are compared
# ------------------------------------------------------------------------------------------------------------------------------
def stage_input(T, H, dt, seed):
    x = gauss((T, H), seed)
    x[0, 0], x[T - 1, H - 1] = -0.0, -0.0                                            # a copy keeps the sign of zero
    return operand_flat(x, dt)


def stage_check(got, x, G, k, what):
    """got (G, T + k, Hg) device view: body bit-equal to x, k // 2 leading and k - k // 2 trailing halo rows exactly +0"""
    T = x.shape[0]
    want = R.stage_ref(x.cpu(), G, k)
    msg = bad(got, want, bits=True)
    assert not msg, f"{what}: {msg}"
    halo = torch.cat([got[:, :k // 2], got[:, k // 2 + T:]], 1)
    assert halo.shape[1] == k and not bool(halo.cpu().view(torch.uint8).any()), f"{what}: halo rows are not all-zero bits"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("wide", [False, True])
def test_posconv_stage_single_bits(dt, wide):
    """T in {1, 7, 131} x k in {16, 128} (so T < k / 2 occurs) at one 16-byte vector per staged row and at 64 columns per group"""
    G = 4
    Hg = 64 if wide else (4 if dt == F32 else 8)
    H = G * Hg
    for T in (1, 7, 131):
        for k in (16, 128):
            x, _ = stage_input(T, H, dt, 1000 + T + k)
            n = G * (T + k) * Hg
            buf, xg = guarded_flat(n, dt)
            L.check(L.lib().sl_posconv_stage(x.data_ptr(), xg.data_ptr(), T, H, G, k, L.dtype_code(dt), L.stream_ptr()), "sl_posconv_stage")
            assert untouched_flat(buf, n), f"T = {T}, k = {k}: written outside the staged block"
            stage_check(xg.view(G, T + k, Hg), x, G, k, f"T = {T}, k = {k}, Hg = {Hg}")


@pytest.mark.parametrize("dt", DTS)
def test_posconv_stage_batch_bits(dt):
    """seqlens [1, 131, 7, 600] at H = 256, G = 4, k = 16: the 600-frame utterance has 4 x 616 x 8 (16-bit) or x 16 (fp32) chunks, more than
    the batch form's 64 x 256 threads, so its grid-stride loop runs more than once.  Utterance u's block starts (cu[u] + u k) H elements in."""
    seqlens, H, G, k = [1, 131, 7, 600], 256, 4, 16
    Hg = H // G
    assert G * (max(seqlens) + k) * (Hg // (4 if dt == F32 else 8)) > 64 * 256
    cu = cumsum0(seqlens)
    x, _ = stage_input(cu[-1], H, dt, 1010)
    n = (cu[-1] + len(seqlens) * k) * H
    buf, xg = guarded_flat(n, dt)
    cu_d, len_d = i32(cu), i32(seqlens)          # named: a temporary's memory is handed to the next allocation
    L.check(L.lib().sl_posconv_stage_batch(x.data_ptr(), xg.data_ptr(), cu_d.data_ptr(), len_d.data_ptr(), len(seqlens), max(seqlens), H, G, k,
                                           L.dtype_code(dt), L.stream_ptr()), "sl_posconv_stage_batch")
    assert untouched_flat(buf, n), "written in front of the first or behind the last block"
    for u, T in enumerate(seqlens):
        o = (cu[u] + u * k) * H
        stage_check(xg[o:o + (T + k) * H].view(G, T + k, Hg), x[cu[u]:cu[u + 1]], G, k, f"utterance {u} (T = {T})")


# ------------------------------------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [8, 136])
def test_avgpool_batch_honours_its_records(dt, H):
    """seqlens [8, 9, 51, 12, 600], kernel 8, stride 4.  The records' element offsets leave two guard rows between utterances: rec[4u + 1]
    is honoured and the output is not assumed packed.  Bound: frontend_ref.avgpool_ref (the existing avgpool check's)."""
    seqlens, kernel, stride, gap = [8, 9, 51, 12, 600], 8, 4, 2
    cu = cumsum0(seqlens)
    P = [(t - kernel) // stride + 1 for t in seqlens]
    row0 = [sum(P[:u]) + gap * u for u in range(len(P))]
    rows = row0[-1] + P[-1]
    x, x64 = operand_flat(gauss((cu[-1], H), 1020), dt)
    buf, y = guarded_flat(rows * H, dt)
    rec, cu_d, len_d = i64([[P[u], row0[u] * H, 0, 0] for u in range(len(P))]), i32(cu), i32(seqlens)
    L.check(L.lib().sl_avgpool_batch(x.data_ptr(), y.data_ptr(), cu_d.data_ptr(), len_d.data_ptr(), rec.data_ptr(), len(P), max(P), H, kernel,
                                     stride, L.dtype_code(dt), L.stream_ptr()), "sl_avgpool_batch")
    assert untouched_flat(buf, rows * H)
    y = y.view(rows, H)
    for u in range(len(P)):
        r = R.avgpool_ref(x64[cu[u]:cu[u + 1]], kernel, stride, U[dt])
        msg = bad(y[row0[u]:row0[u] + P[u]], r.ref, r.tol)
        assert not msg, f"utterance {u} (T = {seqlens[u]}): {msg}"
        if u:
            assert bool((y[row0[u] - gap:row0[u]] == FILL).all()), f"guard rows in front of utterance {u} written"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [8, 136])
def test_avgpool_rows_ranges_contract(dt, H):
    """sl_avgpool_rows with a ranges table keeps segment_mean_kernel's contract: start clamped to 0, end clamped to T, a range that is
    empty afterwards writes zeros, and a clamped range is divided by the number of rows it summed.  x is a view with poisoned rows in front
    of and behind it inside one allocation, so a mis-clamp is a wrong value and not an access outside the buffer.
    sl_segment_mean_batch on the same table has to give the same values."""
    T, front, behind = 11, 3, 6
    ranges = [(-2, 3), (T - 1, T + 5), (4, 4), (T + 1, T + 3), (2, 9)]
    assert all(-front <= s and e <= T + behind for s, e in ranges)
    x, x64 = operand_flat(gauss((T, H), 1030), dt, pad=8 * H)
    r = R.range_mean_ref(x64, ranges, U[dt])
    buf, y = guarded_flat(len(ranges) * H, dt)
    rng32, rng64 = i32(ranges), i64(ranges)
    L.check(L.lib().sl_avgpool_rows(x.data_ptr(), y.data_ptr(), T, H, 0, 0, rng32.data_ptr(), len(ranges), L.dtype_code(dt), L.stream_ptr()),
            "sl_avgpool_rows")
    assert untouched_flat(buf, len(ranges) * H)
    y = y.view(len(ranges), H)
    msg = bad(y, r.ref, r.tol)
    assert not msg, "avgpool_rows: " + msg
    assert not bool(y[2].cpu().view(torch.uint8).any()) and not bool(y[3].cpu().view(torch.uint8).any()), "an empty range writes +0"
    buf2, y2 = guarded_flat(len(ranges) * H, dt)
    L.check(L.lib().sl_segment_mean_batch(x.data_ptr(), y2.data_ptr(), rng64.data_ptr(), len(ranges), T, H, L.dtype_code(dt), L.stream_ptr()),
            "sl_segment_mean_batch")
    assert untouched_flat(buf2, len(ranges) * H)
    y2 = y2.view(len(ranges), H)
    msg = bad(y2, r.ref, r.tol)
    assert not msg, "segment_mean_batch: " + msg
    msg = bad(y2, y.double(), r.tol)          # a x (1 / n) here, a / n there: one fp32 rounding apart, inside one tolerance of each other
    assert not msg, "the two pooling kernels disagree: " + msg


# ------------------------------------------------------------------------------------------------------------------------------
# Whisper log-mel: an interval per element
# ------------------------------------------------------------------------------------------------------------------------------
_LOGMEL = {}


def logmel_consts():
    if not _LOGMEL:
        nb, ld_pw = 201, 204
        basis = weights.windowed_dft_basis(400)
        fb = weights.slaney_mel_filters(nb, 80)
        mel = torch.zeros((80, ld_pw), dtype=torch.float32)          # as weights.WhisperDeviceWeights lays it out: (n_mel, nb padded to 4)
        mel[:, :nb] = fb.T
        _LOGMEL.update(basis=basis.to(DEV), mel=mel.to(DEV), basis64=basis.double(), mel64=fb.double())
    return _LOGMEL


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("n_frames,n", R.LOGMEL_CASES)
def test_whisper_logmel_interval(dt, n_frames, n):
    """sl_whisper_logmel (five kernels, two fp32 GEMMs) at n_fft = 400, hop = 160, 80 mel bins.  Samples behind the window are poison and
    must be ignored; the workspace is exactly sl_whisper_logmel_workspace_bytes inside a guarded allocation; every element has to lie in
    frontend_ref.logmel_ref's interval (no element is left out)."""
    c = logmel_consts()
    n_total = n_frames * 160
    a64 = R.logmel_audio(n)
    if n > n_total:
        a64[n_total:] = BIG[F32]
        a64[n_total::2] *= -1.0
    audio, audio64 = operand_flat(a64, F32, pad=256)
    r = R.logmel_ref(audio64, n_frames, c["basis64"], c["mel64"], U[dt])
    nbytes = int(L.lib().sl_whisper_logmel_workspace_bytes(400, 160, n_frames, 80))
    wbuf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)          # 0xA5A5A5A5 is a finite float
    ws = wbuf[256:256 + nbytes]
    buf, out = guarded_flat(n_frames * 80, dt)
    L.check(L.lib().sl_whisper_logmel(audio.data_ptr(), n, c["basis"].data_ptr(), c["mel"].data_ptr(), out.data_ptr(), 400, 160, n_frames, 80,
                                      ws.data_ptr(), nbytes, L.dtype_code(dt), L.stream_ptr()), "sl_whisper_logmel")
    assert untouched_flat(buf, n_frames * 80)
    assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + nbytes:] == 0xA5).all()), "written outside the workspace"
    width = float((r.raw_hi - r.raw_lo).max())
    o = out.view(n_frames, 80).double().cpu()
    print(f"log-mel {n_frames} frames, {n} samples: widest interval {width:.3g}; worst (got - ref) / half width "
          f"{float(((o - r.ref).abs() / ((r.hi - r.lo) / 2)).max()):.3g}")
    msg = R.inside(out.view(n_frames, 80), r.lo, r.hi)
    assert not msg, msg


# ------------------------------------------------------------------------------------------------------------------------------
# the three implicit-convolution launches, as csrc/runtime.hip builds them
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_gemm_grouped_conv_layers_lda_below_k(dt):
    """hubert_forward_impl's conv layers 1..: ONE grouped launch, a record {Lout_u, a_off, c_off, 0} per utterance, over PACKED channel-last
    rows with lda = s Cin < K = k Cin.  Lin = [401, 3, 130], k = 3, s = 2.  The rows behind utterance u's last window are utterance
    u + 1's: they are 8 and 64 times larger and alternate in sign by row, so a window that runs on shows; poison behind the last one.
    Exact integers: torch.equal."""
    Lin, Cin, Cout, k, s = [401, 3, 130], 64, 96, 3, 2
    Lo = [(n - k) // s + 1 for n in Lin]
    parts = []
    for u, n in enumerate(Lin):
        sign = torch.tensor([(-1.0) ** t for t in range(n)], dtype=torch.float64)[:, None]
        parts.append(ints((n, Cin), 1, 2, 1100 + u) * sign * 8 ** u)
    x64 = torch.cat(parts + [torch.full((4, Cin), BIG[dt], dtype=torch.float64)])
    x, x64 = vec(x64, dt)
    w, w64 = operand(ints((Cout, k * Cin), -2, 2, 1104), dt)
    b, b64 = vec(ints((Cout,), -8, 8, 1105), dt)
    in0, out0 = cumsum0(Lin), cumsum0(Lo)
    buf, out = guarded(out0[-1], Cout, dt)
    ldc = out.stride(0)
    grp = i64([[Lo[u], in0[u] * Cin, out0[u] * ldc, 0] for u in range(len(Lin))])
    ops.gemm_ex(x, w, M=max(Lo), N=Cout, K=k * Cin, lda=s * Cin, ldw=w.stride(0), out=out, ldc=ldc, bias=b, batch=len(Lin), groups=grp, w_mod=1, dtype=dt)
    assert untouched(buf, out0[-1], Cout)
    flat = x64.reshape(-1)
    for u in range(len(Lin)):
        win = torch.stack([flat[(in0[u] + t * s) * Cin:(in0[u] + t * s) * Cin + k * Cin] for t in range(Lo[u])])
        msg = bad(out[out0[u]:out0[u + 1]], to_dt(win @ w64.T + b64, dt))
        assert not msg, f"utterance {u} (Lin = {Lin[u]}): {msg}"


def gelu_residual_bound(pre, mag, b64, r64, K, u):
    """The suite's G bound (test_kernel_edges_gpu.py check_gauss) for gelu(A W^T + b) + R: twice the output rounding, the worst-case fp32
    accumulation K 2^-24 (|A| |W|^T + |b|) carried through GELU (slope <= 1.13) with the erf allowance, and the fp32 add of the residual"""
    ref = R.gelu64(pre) + r64
    tol = 2 * u * ref.abs() + R.GELU_SLOPE * K * E24 * (mag + b64.abs()) + R.TRANS * (1 + pre.abs()) + E24 * (ref.abs() + r64.abs()) + E24
    return ref, tol


@pytest.mark.parametrize("dt", DTS)
def test_gemm_grouped_posconv_of_a_ragged_batch(dt):
    """hubert_forward_impl's positional conv: n_utt G records {T_u, a_off, c_off, r_off} of ONE grouped launch, w_mod = G, strideW, strideBias =
    Hg, GELU, the residual taken at the record's offset inside rows of H.  T = [1, 131, 7], H = 256, G = 4, k = 16.  The one staged row of every
    group that no window reaches (T + k - 1) is poison, as is everything behind the last block."""
    Ts, H, G, k = [1, 131, 7], 256, 4, 16
    Hg, K = H // G, k * (H // G)
    tok0 = cumsum0(Ts)
    x64 = gauss((tok0[-1], H), 1110)
    blocks = []
    for u, T in enumerate(Ts):
        blk = R.stage_ref(x64[tok0[u]:tok0[u + 1]], G, k)
        blk[:, T + k - 1] = BIG[dt]
        blk[:, T + k - 1, ::2] *= -1.0
        blocks.append(blk.reshape(-1))
    xg, xg64 = vec(torch.cat(blocks + [torch.full((2 * H,), BIG[dt], dtype=torch.float64)]), dt)
    w, w64 = operand(gauss((H, K), 1111, K ** -0.5), dt)
    b, b64 = vec(gauss((H,), 1112), dt)
    res, res64 = operand(gauss((tok0[-1], H), 1113), dt)
    buf, out = guarded(tok0[-1], H, dt)
    ldc, ldr = out.stride(0), res.stride(0)
    # the records, as hubert_forward_impl builds them (there ldc = ldr = H and c_off = r_off)
    xg_off = cumsum0((T + k) * H for T in Ts)
    grp = i64([[Ts[u], xg_off[u] + g * (Ts[u] + k) * Hg, tok0[u] * ldc + g * Hg, tok0[u] * ldr + g * Hg] for u in range(len(Ts)) for g in range(G)])
    ops.gemm_ex(xg, w, M=max(Ts), N=Hg, K=K, lda=Hg, ldw=w.stride(0), strideW=Hg * w.stride(0), out=out, ldc=ldc, bias=b, strideBias=Hg, residual=res,
                ldr=ldr, act=GELU, batch=len(Ts) * G, groups=grp, w_mod=G, dtype=dt)
    assert untouched(buf, tok0[-1], H)
    for u, T in enumerate(Ts):
        blk = xg64[xg_off[u]:xg_off[u + 1]].view(G, T + k, Hg)
        win = R.stage_windows(blk, k)                                                    # (G, T, K)
        for g in range(G):
            cols = slice(g * Hg, (g + 1) * Hg)
            pre = win[g] @ w64[cols].T + b64[cols]
            mag = win[g].abs() @ w64[cols].abs().T
            ref, tol = gelu_residual_bound(pre, mag, b64[cols], res64[tok0[u]:tok0[u + 1], cols], K, U[dt])
            msg = bad(out[tok0[u]:tok0[u + 1], cols], ref, tol)
            assert not msg, f"utterance {u} (T = {T}), group {g}: {msg}"


@pytest.mark.parametrize("dt", DTS)
def test_gemm_strided_whisper_conv2(dt):
    """sl_whisper_forward's conv2 (k = 3, stride 2, padding 1): a strided batch of 3 over haloed (F + 2, H) blocks with lda = 2H < K = 3H, GELU,
    then the positional table as a residual shared by the whole batch (strideR = 0).  T = 9 positions out of F = 18 frames, H = 64.  Row F + 1
    of a block is read by no window: poison."""
    n_utt, T, H = 3, 9, 64
    F_, K = 2 * T, 3 * H
    a64 = gauss((n_utt, F_ + 2, H), 1120)
    a64[:, F_ + 1] = BIG[dt]
    a64[:, F_ + 1, ::2] *= -1.0
    A, a64 = vec(a64, dt)
    w, w64 = operand(gauss((H, K), 1121, K ** -0.5), dt)
    b, b64 = vec(gauss((H,), 1122), dt)
    pos, pos64 = operand(gauss((T, H), 1123), dt)
    buf, out = guarded(n_utt * T, H, dt)
    a = L.GemmArgs()
    a.A, a.lda, a.strideA = A.data_ptr(), 2 * H, (F_ + 2) * H
    a.W, a.ldw, a.strideW = w.data_ptr(), w.stride(0), 0
    a.C, a.ldc, a.strideC = out.data_ptr(), out.stride(0), T * out.stride(0)
    a.bias, a.strideBias = b.data_ptr(), 0
    a.residual, a.ldr, a.strideR = pos.data_ptr(), pos.stride(0), 0
    a.M, a.N, a.K, a.batch, a.dtype, a.act = T, H, K, n_utt, L.dtype_code(dt), GELU
    ops.gemm_batched(a)
    assert untouched(buf, n_utt * T, H)
    for u in range(n_utt):
        flat = a64[u].reshape(-1)
        win = torch.stack([flat[t * 2 * H:t * 2 * H + K] for t in range(T)])
        ref, tol = gelu_residual_bound(win @ w64.T + b64, win.abs() @ w64.abs().T, b64, pos64, K, U[dt])
        msg = bad(out[u * T:(u + 1) * T], ref, tol)
        assert not msg, f"utterance {u}: {msg}"
