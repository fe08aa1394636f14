"""CPU: the front-end references of tests/frontend_ref.py are the operations, and their bounds are neither vacuous nor too tight.

(a) every restatement equals an independent implementation in fp64: F.conv1d / F.layer_norm / F.gelu, F.pad + unfold and the grouped
    F.conv1d, F.avg_pool1d, torch.stft(center=True, pad_mode="reflect", window=hann_window) and transformers' WhisperFeatureExtractor at
    its own 30 s geometry and at a 1 s one;
(b) the log-mel interval is narrow enough to mean something: on the Gaussian inputs of the GPU cases its widest element is at most 2e-3 in
    output units (values span about 0.07 to 0.88), and a reference with a defect planted in it (every frame one sample late, a reflection
    that repeats the edge sample) leaves it;
(c) the same operations evaluated in fp32 torch stay inside the bounds, so the references alone do not trip their own tests;
(d) host checks: ops.avgpool_batch refuses an utterance shorter than the pool kernel.
No number here is measured on the code under test.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import frontend_ref as R
from conftest import pkg

weights = pkg("weights")
ops = pkg("ops")
L = pkg("_lib")

E24 = R.E24
EPS = 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def conv0_inputs(n, C, seed):
    g_ = gen(seed)
    wave = torch.randn(n, generator=g_).float().double()
    w = (torch.randn(C, 10, generator=g_) * 10 ** -0.5).float().double()
    b, g, beta = [(torch.randn(C, generator=g_) * s + o).float().double() for s, o in ((0.5, 0.0), (0.1, 1.0), (0.1, 0.0))]
    return wave, w, b, g, beta


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the references are the operations
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", [(10, 64), (14, 64), (5 * 96 + 10 + 3, 128), (5 * 192 + 10, 512)])
def test_conv0_reference_equals_torch(n, C):
    wave, w, b, g, beta = conv0_inputs(n, C, 1)
    r = R.conv0_ref(wave, w, b, g, beta, R.U[R.F32], EPS)
    y = F.conv1d(wave[None, None], w[:, None], b, stride=5)[0].T
    assert r.ref.shape == (R.conv0_len(n), C) and close(r.pre, y)
    assert close(r.ref, F.gelu(F.layer_norm(y, (C,), g, beta, R.f32(EPS))))
    assert bool((r.tol > 0).all())


def test_conv0_reference_ignores_tail_samples_and_handles_zero_variance():
    wave, w, b, g, beta = conv0_inputs(5 * 24 + 10 + 4, 64, 2)
    a = R.conv0_ref(wave, w, b, g, beta, R.U[R.BF16], EPS)
    wave2 = wave.clone()
    wave2[-4:] = 1e30
    assert torch.equal(R.conv0_ref(wave2, w, b, g, beta, R.U[R.BF16], EPS).ref, a.ref)
    b0 = torch.full_like(b, 0.5)
    z = R.conv0_ref(torch.zeros(30, dtype=torch.float64), w, b0, g, beta, R.U[R.BF16], EPS)
    assert bool((z.var == 0).all()) and torch.equal(z.ref, R.gelu64(beta).expand(5, 64))


@pytest.mark.parametrize("T,H,G,k", [(1, 32, 4, 16), (7, 32, 4, 128), (131, 256, 4, 16), (5, 24, 3, 5)])
def test_stage_reference_equals_pad_and_unfold(T, H, G, k):
    x = torch.randn(T, H, generator=gen(3), dtype=torch.float64)
    Hg = H // G
    xg = R.stage_ref(x, G, k)
    padded = F.pad(x.T, (k // 2, k - k // 2))                               # (H, T + k)
    assert torch.equal(xg, padded.view(G, Hg, T + k).transpose(1, 2))
    win = R.stage_windows(xg, k)                                             # (G, T, k Hg), element (j, c) at j Hg + c
    want = padded.unfold(1, k, 1)[:, :T].reshape(G, Hg, T, k).permute(0, 2, 3, 1).reshape(G, T, k * Hg)
    assert torch.equal(win, want)
    # the grouped GEMM on these windows is Conv1d(H, H, k, padding = k // 2, groups = G) (its last step dropped for an even k)
    w = torch.randn(H, Hg, k, generator=gen(4), dtype=torch.float64)
    y = F.conv1d(x.T[None], w, padding=k // 2, groups=G)[0][:, :T].T        # (T, H)
    wg = w.view(G, Hg, Hg, k).permute(0, 1, 3, 2).reshape(G, Hg, k * Hg)     # row n of group g: (j, c) at j Hg + c
    got = torch.cat([win[g] @ wg[g].T for g in range(G)], 1)
    assert close(got, y)


@pytest.mark.parametrize("T,kernel,stride", [(8, 8, 4), (9, 8, 4), (51, 8, 4), (600, 8, 4), (13, 3, 2)])
def test_avgpool_reference_equals_torch(T, kernel, stride):
    x = torch.randn(T, 24, generator=gen(5), dtype=torch.float64)
    r = R.avgpool_ref(x, kernel, stride, R.U[R.F16])
    assert close(r.ref, F.avg_pool1d(x.T[None], kernel, stride)[0].T)


def test_range_mean_reference_states_the_contract():
    T = 11
    x = torch.randn(T, 8, generator=gen(6), dtype=torch.float64)
    ranges = [(-2, 3), (T - 1, T + 5), (4, 4), (T + 1, T + 3), (2, 9), (5, 3)]
    r = R.range_mean_ref(x, ranges, R.U[R.F32])
    assert close(r.ref[0], x[0:3].sum(0) / 3) and close(r.ref[1], x[T - 1]) and close(r.ref[4], x[2:9].mean(0))
    for i in (2, 3, 5):                                                      # empty after clamping: zeros, no 0 / 0
        assert bool((r.ref[i] == 0).all()) and bool((r.tol[i] == 0).all())
    assert [R.clamp_range(s, e, T) for s, e in ranges] == [(0, 3), (10, 11), (0, 0), (0, 0), (2, 9), (0, 0)]


def _consts():
    basis = weights.windowed_dft_basis(400).double()
    mel = weights.slaney_mel_filters(201, 80).double()
    return basis, mel


@pytest.mark.parametrize("n_frames,n", [(12, 1920), (12, 700), (17, 17 * 160 - 3), (12, 2500)])
def test_logmel_reference_equals_torch_stft(n_frames, n):
    basis, mel = _consts()
    audio = R.logmel_audio(n, 7)
    x = torch.zeros(n_frames * 160, dtype=torch.float64)
    x[:min(n, x.numel())] = audio[:x.numel()]
    st = torch.stft(x, 400, 160, window=torch.hann_window(400, dtype=torch.float64), center=True, pad_mode="reflect", return_complex=True)
    pw = st.abs()[:, :-1].T ** 2                                              # (n_frames, 201): the last frame is dropped
    frames = R.logmel_frames(audio, n_frames)
    spec = frames @ basis.T
    assert close(spec[:, :201] ** 2 + spec[:, 201:] ** 2, pw, 1e-6)           # the basis is stored in fp32
    lm = torch.log10((pw @ mel).clamp(min=1e-10))
    want = (torch.maximum(lm, lm.max() - 8.0) + 4.0) / 4.0
    r = R.logmel_ref(audio, n_frames, basis, mel, R.U[R.F32])
    assert close(r.ref, want, 1e-6)


def test_logmel_one_frame_reads_what_a_longer_window_reads():
    """n_frames = 1: torch refuses to reflect-pad 160 samples by 200, frame 0 still exists.  Positions -159 .. 159 are those of any longer
    window over the same samples; the positions on either side of them reflect once more, at sample 159."""
    audio = R.logmel_audio(160, 8)
    f1 = R.logmel_frames(audio, 1)[0]
    f2 = R.logmel_frames(audio, 2)[0]
    assert torch.equal(f1[41:360], f2[41:360])
    assert torch.equal(f1[:41], audio[118:159]) and torch.equal(f1[360:], audio[119:159].flip(0))


@pytest.mark.parametrize("chunk,n", [(30, 480000), (30, 31234), (1, 16000), (1, 700), (1, 20000)])
def test_logmel_reference_equals_whisper_feature_extractor(chunk, n):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=80, chunk_length=chunk)
    basis, mel = _consts()
    audio = R.logmel_audio(n, 9)
    want = torch.as_tensor(fe(audio.float().numpy(), sampling_rate=16000, return_tensors="np").input_features[0]).double().T
    r = R.logmel_ref(audio, fe.nb_max_frames, basis, mel, R.U[R.F32])
    assert want.shape == r.ref.shape == (chunk * 100, 80)
    # HF computes in fp64 and returns fp32; here basis and filters are the fp32 constants the kernel is handed, each coefficient 2^-24 off:
    # 1 / (n_fft + 16) of the interval's STFT term, which test_logmel_interval_is_narrow holds below 2e-3
    assert close(r.ref, want, 2e-3 / 416 * 4), float((r.ref - want).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the log-mel interval means something
# ------------------------------------------------------------------------------------------------------------------------------
WIDTH_MAX = 2e-3          # the issue's condition on the widest interval, in output units


@pytest.mark.parametrize("n_frames,n", R.LOGMEL_CASES)
def test_logmel_interval_is_narrow_and_a_defect_leaves_it(n_frames, n):
    basis, mel = _consts()
    audio = R.logmel_audio(n, R.LOGMEL_SEED)
    r = R.logmel_ref(audio, n_frames, basis, mel, R.U[R.F32])
    width = float((r.raw_hi - r.raw_lo).max())
    print(f"log-mel {n_frames} frames, {n} samples: widest interval {width:.3g}, values {float(r.ref.min()):.3g} .. {float(r.ref.max()):.3g}")
    assert bool((r.raw_lo <= r.ref).all()) and bool((r.ref <= r.raw_hi).all())
    assert width <= WIDTH_MAX
    # every frame one sample late: no element of a frame that holds signal stays inside
    late = R.logmel_ref(torch.cat([torch.zeros(1, dtype=torch.float64), audio]), n_frames, basis, mel, R.U[R.F32])
    out = ~((late.ref >= r.raw_lo) & (late.ref <= r.raw_hi))
    live = r.log_mel > r.log_mel.max() - 8.0
    assert float(out[live].double().mean()) > 0.9
    # the reflection repeats the edge sample (pad_mode "symmetric"): frame 0 reads a wrong left half
    if n_frames == 1:
        return          # fewer samples than the padding: this defect has no one-frame form
    n_total = n_frames * 160
    x = torch.zeros(n_total, dtype=torch.float64)
    x[:min(n, n_total)] = audio[:n_total]
    f = R.logmel_frames(audio, n_frames)
    f[0, :200] = x[:200].flip(0)
    spec = f @ basis.T
    lm = torch.log10(((spec[:, :201] ** 2 + spec[:, 201:] ** 2) @ mel).clamp(min=1e-10))
    sym = (torch.maximum(lm, lm.max() - 8.0) + 4.0) / 4.0
    assert float((~((sym[0] >= r.raw_lo[0]) & (sym[0] <= r.raw_hi[0]))).double().mean()) > 0.9


# ------------------------------------------------------------------------------------------------------------------------------
# (c) fp32 evaluations stay inside the bounds
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [R.F32, R.BF16, R.F16])
@pytest.mark.parametrize("n,C", [(5 * 96 + 10 + 2, 64), (5 * 24 + 10, 512)])
def test_conv0_fp32_evaluation_stays_inside_the_bound(dt, n, C):
    wave, w, b, g, beta = conv0_inputs(n, C, 11)
    r = R.conv0_ref(wave, w, b, g, beta, R.U[dt], EPS)
    y = F.conv1d(wave.float()[None, None], w.float()[:, None], b.float(), stride=5)[0].T
    got = F.gelu(F.layer_norm(y, (C,), g.float(), beta.float(), EPS)).to(dt).double()
    assert float(((got - r.ref).abs() / r.tol).max()) <= 1.0
    # ... and a row computed from the window one sample late does not
    y2 = F.conv1d(wave.float()[None, None, 1:], w.float()[:, None], b.float(), stride=5)[0].T
    bad_row = F.gelu(F.layer_norm(y2, (C,), g.float(), beta.float(), EPS)).to(dt).double()[-1]
    assert float(((bad_row - r.ref[y2.shape[0] - 1]).abs() / r.tol[y2.shape[0] - 1]).max()) > 1.0


@pytest.mark.parametrize("n_frames,n", R.LOGMEL_CASES)
def test_logmel_fp32_evaluation_stays_inside_the_interval(n_frames, n):
    basis, mel = _consts()
    audio = R.logmel_audio(n, R.LOGMEL_SEED)
    r = R.logmel_ref(audio, n_frames, basis, mel, R.U[R.F32])
    spec = R.logmel_frames(audio, n_frames).float() @ basis.float().T
    lm = torch.log10(((spec[:, :201] ** 2 + spec[:, 201:] ** 2) @ mel.float()).clamp(min=1e-10))
    got = (torch.maximum(lm, lm.max() - 8.0) + 4.0) / 4.0
    assert not R.inside(got, r.lo, r.hi)


# ------------------------------------------------------------------------------------------------------------------------------
# (d) host checks
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seqlens", [[8, 7, 51], [3], [12, 0]])
def test_avgpool_batch_refuses_an_utterance_shorter_than_the_kernel(seqlens):
    """(t - kernel) // stride + 1 is zero or negative there; hubert_plan refuses the same utterance in C"""
    x = torch.zeros(sum(seqlens), 8)
    with pytest.raises(L.SpeechLLMError, match="frames < pool kernel 8"):
        ops.avgpool_batch(x, seqlens, 8, 4)
