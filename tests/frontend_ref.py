"""The encoder's front end restated in plain torch, fp64, on the CPU (a helper module of the edge suite, not a conftest).

Four restatements, each of the STORED (already rounded) inputs, each with the bound a kernel's result has to keep per element
("edge suite", front end):
  conv0      Conv1d(1 -> C, k = 10, s = 5) + LayerNorm(C) + GELU, channel-last (csrc/conv.hip conv0_strip)
  stage      the positional conv's staged layout (T, H) -> (G, T + k, H / G) with a zero halo (posconv_stage_kernel): a copy
  pooling    AvgPool1d over time and the mean of row ranges, the ranges clamped as segment_mean_kernel states it
  log-mel    Whisper's: zero-pad or trim, reflect-pad, windowed DFT, power, slaney mel, log10 with the 1e-10 floor, the max - 8 clamp,
             (x + 4) / 4 (csrc/whisper.hip), with an INTERVAL per element instead of a tolerance
tests/test_frontend_ref_cpu.py pins each against an independent implementation; tests/test_frontend_edges_gpu.py runs the kernels against
them.  No constant here is a measured number.
"""
import math
from types import SimpleNamespace

import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}        # half an ulp, relative (as in the edge suite)
E24 = 2.0 ** -24
TRANS = 2e-6          # relative allowance of one device transcendental: test_kernel_edges_gpu.py check_gauss (GELU's erf)
GELU_SLOPE = 1.13     # max |gelu'|, as check_gauss carries an error through GELU
LOG_OPS = 6           # fp32 operations from the logarithm on, as the suite's lse bound counts them for the generic kernel (LSE_OPS)


def f32(v):
    """a Python float as the kernels see it: rounded to fp32"""
    return float(torch.tensor(v, dtype=torch.float32))


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


# ------------------------------------------------------------------------------------------------------------------------------
# conv0 + LayerNorm + GELU
# ------------------------------------------------------------------------------------------------------------------------------
def conv0_len(n_samples, k=10, s=5):
    return (n_samples - k) // s + 1


def conv0_ref(wave, w, b, g, beta, u, eps=1e-5, k=10, s=5):
    """wave (n,), w (C, k), b, g, beta (C,) fp64 -> namespace(pre, z, ref, tol): (L, C) each, L = (n - k) // s + 1; the n - (s (L - 1) + k)
    tail samples are not read.  u: half-ulp of the output type."""
    n, C = wave.numel(), w.shape[0]
    L = conv0_len(n, k, s)
    win = torch.stack([wave[t * s:t * s + k] for t in range(L)])          # (L, k)
    pre = win @ w.T + b
    mean = pre.mean(-1, keepdim=True)
    d = pre - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + f32(eps))
    z = d * rstd * g + beta
    ref = gelu64(z)
    # The conv's own accumulation: k fma and the bias, any order: (k + 1) 2^-24 (|w| |x| + |b|) on every pre-norm element.
    e_y = (k + 1) * E24 * (win.abs() @ w.abs().T + b.abs())
    # ... carried through the normalisation to first order: the centred value moves by at most e_y + mean(e_y); the variance by
    # 2 mean(|d| (e_y + mean e_y)), which moves rstd by rstd^3 / 2 of that and the normalised value by |d| g times it.
    e_c = e_y + e_y.mean(-1, keepdim=True)
    d_var = 2.0 * (d.abs() * e_c).mean(-1, keepdim=True)
    e_conv = rstd * g.abs() * e_c + d.abs() * g.abs() * 0.5 * rstd ** 3 * d_var
    # LayerNorm's own roundings, exactly test_rmsnorm_and_layernorm_per_element's e with cols = C: the mean carries C 2^-24 sum|y| / C,
    # the centred value is scaled by rstd g.
    e_norm = (C + 16) * E24 * (rstd * g.abs() * (pre.abs() + pre.abs().mean(-1, keepdim=True)) + beta.abs())
    # GELU (slope <= 1.13, the suite's erf allowance) and twice the output rounding
    tol = 2 * u * ref.abs() + GELU_SLOPE * (e_conv + e_norm) + TRANS * (1 + z.abs()) + E24
    return SimpleNamespace(pre=pre, var=var, z=z, ref=ref, tol=tol)


# ------------------------------------------------------------------------------------------------------------------------------
# positional conv: staged layout
# ------------------------------------------------------------------------------------------------------------------------------
def stage_ref(x, G, k):
    """x (T, H) -> (G, T + k, H / G): group g's columns in rows k // 2 .. k // 2 + T - 1, k // 2 zero rows in front, k - k // 2 behind"""
    T, H = x.shape
    Hg = H // G
    xg = torch.zeros(G, T + k, Hg, dtype=x.dtype)
    xg[:, k // 2:k // 2 + T] = x.view(T, G, Hg).transpose(0, 1)
    return xg


def stage_windows(xg, k):
    """the rows the grouped GEMM reads: window t of group g is the k Hg contiguous elements from staged row t (lda = Hg < K = k Hg)
    -> (G, T, k Hg), T = rows - k"""
    G, rows, Hg = xg.shape
    flat = xg.reshape(G, rows * Hg)
    return torch.stack([torch.stack([flat[g, t * Hg:t * Hg + k * Hg] for t in range(rows - k)]) for g in range(G)])


# ------------------------------------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------------------------------------
def avgpool_ref(x, kernel, stride, u):
    """AvgPool1d over the rows of x (T, H), no padding -> namespace(ref, tol) of (P, H), P = (T - kernel) // stride + 1.
    Bound, as test_avgpool_embed_silu_mul_rope_per_element: twice the output rounding + kernel adds and the multiply by 1 / kernel (itself
    rounded) on the mean magnitude."""
    P = (x.shape[0] - kernel) // stride + 1
    ref = torch.stack([x[stride * i:stride * i + kernel].mean(0) for i in range(P)])
    mag = torch.stack([x[stride * i:stride * i + kernel].abs().mean(0) for i in range(P)])
    return SimpleNamespace(ref=ref, tol=2 * u * ref.abs() + (kernel + 2) * E24 * mag + E24)


def clamp_range(s, e, T):
    """segment_mean_kernel's contract: start clamped to 0, end to T; the range is empty if nothing is left"""
    s, e = max(int(s), 0), min(int(e), T)
    return (s, e) if e > s else (0, 0)


def range_mean_ref(x, ranges, u):
    """mean of rows [s, e) of x (T, H) for every (s, e), clamped as clamp_range; an empty range gives zeros.  The divisor is the number of
    rows summed.  Bound as avgpool_ref with kernel = that number."""
    T, H = x.shape
    ref, tol = torch.zeros(len(ranges), H, dtype=torch.float64), torch.zeros(len(ranges), H, dtype=torch.float64)
    for i, (s, e) in enumerate(ranges):
        s, e = clamp_range(s, e, T)
        if e > s:
            ref[i] = x[s:e].mean(0)
            tol[i] = 2 * u * ref[i].abs() + (e - s + 2) * E24 * x[s:e].abs().mean(0) + E24
    return SimpleNamespace(ref=ref, tol=tol)


# ------------------------------------------------------------------------------------------------------------------------------
# Whisper log-mel
# ------------------------------------------------------------------------------------------------------------------------------
def logmel_frames(audio, n_frames, n_fft=400, hop=160):
    """zero-pad or trim to n_frames hop samples, reflect-pad by n_fft / 2 (torch.stft center=True), cut n_frames frames (the STFT's
    last frame is dropped) -> (n_frames, n_fft).  With ONE frame the padding is longer than the signal and a full reflect-pad does not
    exist; frame 0 itself still reads only once-reflected positions, which is all that is built here."""
    n_total, pad = n_frames * hop, n_fft // 2
    x = torch.zeros(n_total, dtype=torch.float64)
    n = min(audio.numel(), n_total)
    x[:n] = audio[:n]
    j = torch.arange(-pad, (n_frames - 1) * hop + n_fft - pad).abs()
    j = torch.where(j >= n_total, 2 * (n_total - 1) - j, j)
    assert int(j.min()) >= 0 and int(j.max()) < n_total
    padded = x[j]
    return torch.stack([padded[t * hop:t * hop + n_fft] for t in range(n_frames)])


def logmel_ref(audio, n_frames, basis, mel, u, n_fft=400, hop=160):
    """audio (n,), basis (2 nb, n_fft) = [window cos | window sin], mel (nb, n_mel) >= 0, all fp64 -> namespace(ref, lo, hi, raw_lo, raw_hi)
    of (n_frames, n_mel).  [lo, hi] is the interval a correct fp32 evaluation in ANY summation order stays in, widened by the output
    rounding 2u |ref|; [raw_lo, raw_hi] is the same interval before that widening (what the width condition of
    tests/test_frontend_ref_cpu.py is stated on)."""
    nb = n_fft // 2 + 1
    frames = logmel_frames(audio, n_frames, n_fft, hop)
    spec = frames @ basis.T
    # the STFT GEMM: n_fft products in fp32, any order (the suite's (K + 16) 2^-24 mag form)
    d_spec = (n_fft + 16) * E24 * (frames.abs() @ basis.abs().T)
    re, im, d_re, d_im = spec[:, :nb], spec[:, nb:], d_spec[:, :nb], d_spec[:, nb:]
    pw = re * re + im * im
    # (re +- d)^2 moves by 2 |re| d + d^2; two squares, an add (or one multiply and an fma), rounded: 4 2^-24 pw
    d_pw = 2 * re.abs() * d_re + d_re ** 2 + 2 * im.abs() * d_im + d_im ** 2 + 4 * E24 * pw
    m = pw @ mel
    # the mel GEMM: the filters are non-negative, so the input error passes through them and mag = mel itself
    d_m = d_pw @ mel + (nb + 16) * E24 * m
    floor = 1e-10

    def log10c(v):
        return torch.log10(v.clamp(min=floor))

    # log10 is monotone; from it on LOG_OPS fp32 operations (the floor constant's own rounding, log10, the subtraction of 8, the
    # addition of 4; / 4 is exact), each half an ulp of a value of size max(|log|, 1): the suite's lse_ulp
    def widen(v, sign):
        return v + sign * LOG_OPS * E24 * v.abs().clamp(min=1.0)

    mid, lo, hi = log10c(m), widen(log10c(m - d_m), -1.0), widen(log10c(m + d_m), +1.0)

    # max(x, gmax - 8) and (x + 4) / 4 are monotone in x and in gmax: the ends of the interval come from the ends of both
    def finish(v, gmax):
        return (torch.maximum(v, gmax - 8.0) + 4.0) / 4.0

    ref, raw_lo, raw_hi = finish(mid, mid.max()), finish(lo, lo.max()), finish(hi, hi.max())
    r = 2 * u * torch.maximum(raw_lo.abs(), raw_hi.abs())
    return SimpleNamespace(ref=ref, lo=raw_lo - r, hi=raw_hi + r, raw_lo=raw_lo, raw_hi=raw_hi, log_mel=mid)


def inside(got, lo, hi):
    """"" if lo <= got <= hi everywhere"""
    got = got.detach().double().cpu()
    wrong = ~((got >= lo) & (got <= hi))
    if not bool(wrong.any()):
        return ""
    i = tuple(wrong.nonzero()[0].tolist())
    return f"{int(wrong.sum())} of {wrong.numel()} elements outside their interval, first at {i}: got {float(got[i])!r}, interval [{float(lo[i])!r}, {float(hi[i])!r}]"


# (n_frames, samples handed over, samples that count): exactly the window, shorter than it (the zero frames sit on the 1e-10 floor and the
# max - 8 clamp acts on half the elements), shorter than the reflect padding, longer than the window (the rest is poisoned by the GPU test),
# a count that is no multiple of the hop, and one frame, where the padding is longer than the signal
LOGMEL_CASES = [(12, 1920), (12, 700), (12, 37), (12, 1920 + 333), (17, 17 * 160 - 3), (1, 160), (1, 37)]


LOGMEL_SEED = 7          # the interval's width depends on the smallest power an element happens to have; tests/test_frontend_ref_cpu.py
#                          asserts the width condition for this seed, on the reference alone


def logmel_audio(n, seed=LOGMEL_SEED):
    """Gaussian, std 0.1, as fp32 stores it (a pure tone would make the worst-case interval useless: its width reaches 0.1)"""
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1).float().double()
