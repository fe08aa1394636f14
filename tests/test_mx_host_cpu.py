"""CPU: the host side of the opt-in MX linears (MXFP8 activations x MXFP4 weights on the block-scaled MFMA).  The header
names the format as code 5 without an ABI bump and the new entries are mirrored in the ctypes table; the host packer is held byte for
byte against the MX weight image written here in numpy FROM THE HEADER'S TEXT, and its codes and scale bytes against those of the MXFP4
image of the same weight; the host activation quantiser — the definition the device kernel must reproduce — is held against a numpy
restatement of its rule on EVERY bf16 and every fp16 bit pattern as a block's maximum; every entry refuses what is not built before
any device work; and the workspace sizes of the formats that existed before are the numbers their parent commit reported.  Nothing
here needs a GPU, and no reference calls the C routine it checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import pkg

L = pkg("_lib")
ops = pkg("ops")
cfgm = pkg("config")
weights = pkg("weights")
llama_mod = pkg("audio_llama")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(1 << 20)          # a non-null, 16-byte aligned pointer the argument checks never dereference
ERR_ARG, ERR_UNSUPPORTED = -1, -3
F16, BF16 = torch.float16, torch.bfloat16
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _err():
    return L.lib().sl_last_error().decode()


def test_header_names_format_5_and_keeps_abi_7():
    h = open(os.path.join(REPO, "include", "speechllm.h")).read()
    assert re.search(r"#define SL_WDEC_MX_LINEAR\s+5\b", h)
    assert re.search(r"#define SL_WDEC_MXFP4\s+4\b", h) and re.search(r"#define SL_WDEC_E4M3\s+1\b", h) and re.search(r"#define SL_WDEC_MODEL_DTYPE 0\b", h)
    assert re.search(r"#define SL_ABI_VERSION 7\b", h)
    assert L.lib().sl_version() == 7
    assert L.WDEC_MX_LINEAR == 5 and (L.WDEC_MODEL_DTYPE, L.WDEC_E4M3, L.WDEC_MXFP4) == (0, 1, 4)
    assert L.linear_format_code("mx") == L.linear_format_code("mxfp8_mxfp4") == 5 and L.linear_format_code(None) == 0
    for bad in ("fp8", "mxfp4", "model", torch.float8_e4m3fn):
        with pytest.raises(L.SpeechLLMError):
            L.linear_format_code(bad)


def test_new_exports_are_mirrored():
    for name in ("sl_mx_weight_image_bytes", "sl_pack_weight_mx", "sl_pack_weight_mx_host", "sl_mxfp8_quantize_rows", "sl_mxfp8_quantize_rows_host", "sl_gemm_mx"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    h = open(os.path.join(REPO, "include", "speechllm.h")).read()
    # the struct the ctypes mirror copies: same fields, same order
    body = re.search(r"typedef struct \{([^}]*)\} sl_gemm_mx_args;", h).group(1)
    names = re.findall(r"[\s*,](\w+)\s*[;,]", body)
    assert names == [n for n, _ in L.GemmMxArgs._fields_], names


def test_image_bytes():
    lib = L.lib()
    assert lib.sl_mx_weight_image_bytes(16, 128) == 16 * 64 + 16 * 4
    assert lib.sl_mx_weight_image_bytes(17, 128) == 32 * 64 + 32 * 4
    assert lib.sl_mx_weight_image_bytes(40, 384) == 48 * 192 + 48 * 12
    assert lib.sl_mx_weight_image_bytes(272, 1024) == 272 * 512 + 272 * 32
    for n, k in ((16, 128), (40, 384), (1000, 256)):
        assert lib.sl_mx_weight_image_bytes(n, k) == lib.sl_w4_image_bytes(n, k)
    for n, k in ((16, 64), (0, 128), (16, 0), (16, 192), (-1, 128)):
        assert lib.sl_mx_weight_image_bytes(n, k) == 0 and "sl_mx_weight_image_bytes" in _err()


# ------------------------------------------------------------------------------------------------------------------------------
# the MX weight image, written out from the header's text
# ------------------------------------------------------------------------------------------------------------------------------
def ref_e2m1(w):
    """(N, K) 16-bit weight -> (codes (N, K) uint8, exponents (N, K/32) int64) by the MXFP4 definition, in fp64"""
    N, K = w.shape
    v = w.double().numpy().reshape(N, K // 32, 32)
    a = np.where(np.isnan(v), 0.0, np.abs(v))
    amax = a.max(-1)                                                    # NaN elements skipped
    e = np.full(amax.shape, 13, dtype=np.int64)
    for cand in range(12, -14, -1):                                     # the smallest e of [-13, 13] with amax <= 6 * 2^e
        e = np.where(amax <= 6.0 * 2.0 ** cand, cand, e)
    e = np.where(amax == 0, 0, e)
    with np.errstate(invalid="ignore"):
        x = v / np.exp2(e.astype(np.float64))[:, :, None]               # exact in fp64
    ax = np.where(np.isnan(x), 0.0, np.minimum(np.abs(x), 6.0))         # saturation (inf included); NaN -> 0
    d = np.abs(ax[..., None] - E2M1)                                    # distance to every grid point
    lo = d.argmin(-1)                                                   # the first minimum: the lower of two equidistant codes
    tie = np.take_along_axis(d, np.minimum(lo + 1, 7)[..., None], -1)[..., 0] == np.take_along_axis(d, lo[..., None], -1)[..., 0]
    code = np.where(tie & (lo % 2 == 1) & (lo < 7), lo + 1, lo)         # ties go to the even code
    code = np.where((x < 0) & (code != 0), code + 8, code)              # sign in bit 3; no negative zero
    return code.reshape(N, K).astype(np.uint8), e


def image_from_codes(code, sc):
    """natural-order e2m1 codes (Np, K) and scale bytes (Np, K/32), numpy uint8 -> (element bytes (Np*K/2,), scale bytes (Np*K/32,)) of the
    MX weight image: img[f][j][lane][b] = code[16 f + (lane & 15)][128 j + 32 (lane >> 4) + 2 b] | code[... + 1] << 4 and
    sc[f][j][lane] = the scale byte of row 16 f + (lane & 15), block 4 j + (lane >> 4)"""
    Np, K = code.shape
    f = np.arange(Np // 16)[:, None, None, None]
    j = np.arange(K // 128)[None, :, None, None]
    lane = np.arange(64)[None, None, :, None]
    b = np.arange(16)[None, None, None, :]
    rows, cols = 16 * f + (lane & 15), 128 * j + 32 * (lane >> 4) + 2 * b
    img = code[rows, cols] | (code[rows, cols + 1] << 4)
    sci = sc[(16 * f + (lane & 15))[..., 0], (4 * j + (lane >> 4))[..., 0]]
    return torch.from_numpy(img.reshape(-1).astype(np.uint8)), torch.from_numpy(sci.reshape(-1).astype(np.uint8))


def ref_mx_image(w):
    """-> (the image's element bytes, its scale bytes, natural-order codes (Np, K), scale bytes (Np, K/32)); padding rows are zero codes
    with scale byte 127"""
    N, K = w.shape
    Np = (N + 15) // 16 * 16
    code = np.zeros((Np, K), dtype=np.uint8)
    sc = np.full((Np, K // 32), 127, dtype=np.uint8)
    c, e = ref_e2m1(w)
    code[:N], sc[:N] = c, (e + 127).astype(np.uint8)
    img, sci = image_from_codes(code, sc)
    return img, sci, torch.from_numpy(code), torch.from_numpy(sc)


def _next_up(x, dt):
    t = torch.tensor([x], dtype=dt)
    return float((t.view(torch.int16) + 1).view(dt)[0])


def edge_rows(K, dt):
    """eight rows, each block built for one edge of the definition"""
    r = torch.zeros(8, K)
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    r[0, :32] = torch.linspace(-3, 3, 32)                                # (blocks 1.. of row 0 stay all-zero)
    r[1, 0], r[1, 1], r[1, 2] = float("inf"), 1.0, -2.0 ** 12            # +inf: saturates, e at the top of the clamp
    r[1, 32], r[1, 33] = float("-inf"), 3.0
    r[2, 0], r[2, 1], r[2, 2] = float("nan"), 3.0, -0.5                  # a NaN element is skipped by the maximum, code 0
    r[2, 32:64] = float("nan")                                           # a block that is NaN only
    big = 60000.0 if dt == F16 else 3.0e6                                # above 6 * 2^13: e = 13, saturation
    r[3, 0], r[3, 1], r[3, 2] = big, -big, 6 * 2.0 ** 13
    r[3, 32], r[3, 33] = _next_up(6 * 2.0 ** 12, dt), 2.0 ** 12          # one ulp above 6 * 2^12: the next exponent, the top of the clamp
    tiny = 2.0 ** -15                                                    # below 2^-14: e = -13, values on the 2^-14 grid or zero
    r[4, 0], r[4, 1], r[4, 2], r[4, 3] = tiny, 3 * tiny, -tiny, -0.4 * tiny
    r[4, 32], r[4, 33] = 6 * 2.0 ** -13, 0.25 * 2.0 ** -13               # amax exactly 6 * 2^-13
    for i, e in enumerate((0, -3, 5)):                                   # amax exactly 6 * 2^e with every tie point of both signs
        s = 2.0 ** e
        r[5 + i, 0] = 6 * s
        r[5 + i, 1:8], r[5 + i, 8:15] = ties * s, -ties * s
        r[5 + i, 32], r[5 + i, 33] = _next_up(6 * s, dt), -0.2 * s       # one ulp above: the next exponent
        r[5 + i, 64], r[5 + i, 96], r[5 + i, 97] = 4 * s, -4 * s, 3 * s
    return r.to(dt)


def weight_rows(N, K, dt, seed=0):
    g = torch.Generator().manual_seed(5000 + seed)
    mag = 2.0 ** ((torch.arange(K // 32)[None, :] + torch.arange(N)[:, None]) % 9 - 4).float()
    w = (torch.randn(N, K // 32, 32, generator=g) * mag[:, :, None]).view(N, K).to(dt)
    w[:8] = edge_rows(K, dt)
    return w


SHAPES = [(16, 128), (17, 128), (40, 384), (272, 1024)]


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_host_packer_matches_the_header_byte_for_byte(dt, N, K):
    w = weight_rows(N, K, dt)
    want_b, want_s, nat, sc = ref_mx_image(w)
    img = ops.pack_weight_mx(w)                         # CPU tensor: sl_pack_weight_mx_host
    Np = (N + 15) // 16 * 16
    assert img.numel() == L.lib().sl_mx_weight_image_bytes(N, K) == Np * K // 2 + Np * K // 32
    got_b, got_s = img[:Np * K // 2], img[Np * K // 2:]
    assert torch.equal(got_s, want_s), f"{int((got_s != want_s).sum())} scale bytes differ"
    assert torch.equal(got_b, want_b), f"{int((got_b != want_b).sum())} element bytes differ"
    c2, s2 = ops.mx_image_parts(img, N, K)               # the inverse the Python surface uses
    assert torch.equal(c2, nat) and torch.equal(s2, sc)
    assert bool((c2[N:] == 0).all()) and bool((s2[N:] == 127).all()), "padding rows: zero codes, e = 0"
    assert not bool((c2 == 8).any()), "a negative zero (code 0x8) in the image"
    # the stated answers of the edge rows
    assert bool((c2[0, 32:] == 0).all()) and bool((s2[0, 1:] == 127).all()), "all-zero blocks: e = 0"
    assert int(c2[1, 0]) == 7 and int(s2[1, 0]) == 127 + 13 and int(c2[1, 32]) == 15, "an inf IS the block maximum: e = 13, +-inf saturate at +-6"
    assert int(c2[2, 0]) == 0 and int(c2[2, 1]) == 7 and int(s2[2, 0]) == 127 - 1 and bool((c2[2, 32:64] == 0).all()) and int(s2[2, 1]) == 127
    assert int(s2[3, 0]) == 127 + 13 and [int(c2[3, k]) for k in range(3)] == [7, 15, 7] and int(s2[3, 1]) == 127 + 13
    assert int(s2[4, 0]) == 127 - 13 and [int(c2[4, k]) for k in range(4)] == [0, 2, 0, 0] and int(s2[4, 1]) == 127 - 13 and int(c2[4, 33]) == 0
    for i, e in enumerate((0, -3, 5)):
        assert int(s2[5 + i, 0]) == 127 + e and [int(c2[5 + i, k]) for k in range(8)] == [7, 0, 2, 2, 4, 4, 6, 6]
        assert [int(c2[5 + i, k]) for k in range(8, 15)] == [0, 10, 10, 12, 12, 14, 14]
        assert int(s2[5 + i, 1]) == 127 + e + 1 and int(c2[5 + i, 32]) == 5
    # the values the product multiplies by
    want = (np.concatenate([E2M1, -E2M1])[nat.numpy()].reshape(Np, K // 32, 32) * np.exp2(sc.numpy().astype(np.float64) - 127)[:, :, None]).reshape(Np, K)[:N]
    assert np.array_equal(ops.mx_dequantise(img, N, K).numpy(), want)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_codes_and_scales_are_those_of_the_mxfp4_image(dt, N, K):
    w = weight_rows(N, K, dt, seed=1)
    c4, s4 = ops.w4_image_parts(ops.pack_weight_mxfp4(w), N, K)
    cx, sx = ops.mx_image_parts(ops.pack_weight_mx(w), N, K)
    assert torch.equal(c4, cx) and torch.equal(s4, sx)


def test_host_packer_reads_a_strided_source_with_poison_in_the_pad_columns():
    w = weight_rows(40, 384, BF16, seed=3)
    wide = torch.full((40, 512), 3e4, dtype=BF16)
    wide[:, :384] = w
    assert torch.equal(ops.pack_weight_mx(wide[:, :384]), ops.pack_weight_mx(w))


# ------------------------------------------------------------------------------------------------------------------------------
# MXFP8 activation rows: the rule, restated in numpy
# ------------------------------------------------------------------------------------------------------------------------------
def ref_e4m3_byte(v):
    """fp64 array -> OCP e4m3fn byte of round-to-nearest-even(v), subnormals included, saturating at +-448; NaN -> 0x7F"""
    a = np.abs(v)
    nan = np.isnan(v)
    a = np.where(nan, 0.0, np.minimum(a, 448.0))                          # inf and everything above saturate
    _, ex = np.frexp(a)                                                   # a = m * 2^ex, .5 <= m < 1
    ex = np.maximum(ex - 1, -6)                                           # the binade; below 2^-6 the subnormal grid of 2^-9
    step = np.exp2((ex - 3).astype(np.float64))
    q = np.minimum(np.rint(a / step) * step, 448.0)                       # np.rint: ties to even; a / step is exact
    _, qx = np.frexp(q)
    qx = qx - 1
    normal = q >= 2.0 ** -6
    byte = np.where(normal, ((qx + 7) << 3) + np.rint((q / np.exp2(qx.astype(np.float64)) - 1.0) * 8).astype(np.int64), np.rint(q * 512).astype(np.int64))
    byte = np.where(np.signbit(v), byte | 0x80, byte)
    return np.where(nan, 0x7F, byte).astype(np.uint8)


def ref_mxfp8(x):
    """(M, K) 16-bit rows -> (bytes (M, K) uint8, scale bytes (M, K/32) uint8) by the header's rule, in fp64"""
    M, K = x.shape
    v = x.double().numpy().reshape(M, K // 32, 32)
    fin = np.isfinite(v)
    amax = np.where(fin, np.abs(v), 0.0).max(-1)                          # over the finite elements
    e = np.full(amax.shape, 127, dtype=np.int64)
    for cand in range(126, -128, -1):                                     # the smallest e of [-127, 127] with amax <= 448 * 2^e
        e = np.where(amax <= 448.0 * 2.0 ** cand, cand, e)
    e = np.where(amax == 0, 0, e)
    with np.errstate(invalid="ignore", over="ignore"):
        s = v / np.exp2(e.astype(np.float64))[:, :, None]                 # exact in fp64
    return ref_e4m3_byte(s).reshape(M, K), (e + 127).astype(np.uint8), e, amax


def _patterns(dt):
    """every 16-bit pattern of dt as element 0 of a block, with probe elements no larger than it: the pattern IS the block's maximum"""
    p = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    f = p.float()
    x = torch.zeros(65536, 32)
    x[:, 0] = f
    for k, c in enumerate((0.75, -1.0 / 3, 2.0 ** -5, -1.5 * 2.0 ** -9, 2.0 ** -10, 0.999, -0.53, 17.0 / 448, 1.0 / 448, 0.5 / 448, -1.5 / 448, 2.5 / 448)):
        x[:, 1 + k] = f * c
    x = x.to(dt)
    x[:, 0] = p                                                            # (the round trip through float kept it, NaN payloads aside)
    return x


@pytest.mark.parametrize("dt", [BF16, F16])
def test_host_quantiser_on_every_bit_pattern_as_the_block_maximum(dt):
    x = _patterns(dt)
    q, s = ops.mxfp8_quantize_rows(x)                    # CPU tensor: sl_mxfp8_quantize_rows_host
    want_q, want_s, e, amax = ref_mxfp8(x)
    assert np.array_equal(s.numpy(), want_s), f"{int((s.numpy() != want_s).sum())} scale bytes differ"
    assert np.array_equal(q.numpy(), want_q), f"{int((q.numpy() != want_q).sum())} element bytes differ"
    v = x.double().numpy()
    fin = np.isfinite(v)
    scaled = np.abs(np.where(fin, v, 0.0)) / np.exp2(e.astype(np.float64))
    assert float(scaled.max()) <= 448.0, "a finite element is clipped"
    nz = (amax[:, 0] > 0) & (e[:, 0] > -127)
    assert bool((amax[nz, 0] > 448.0 * np.exp2(e[nz, 0] - 1.0)).all()), "the exponent is not the smallest one"
    # no finite element saturates: 0x7E / 0xFE appear only where the scaled value rounds to 448 anyway, 0x7F only for NaN
    qb = q.numpy()
    assert not bool(((qb & 0x7F) == 0x7F)[~np.isnan(v)].any())
    assert bool(((qb & 0x7F) == 0x7E)[fin].sum() == (np.rint(scaled / 32.0)[fin] * 32.0 >= 448.0).sum())
    # dequantised values: within half an e4m3 step of the input (relative 2^-4 in the normal range, 2^-10 * 2^e absolute below it)
    dq = ops.mxfp8_dequantise(q, s).numpy()
    err = np.abs(dq - v)[fin]
    bound = np.maximum(np.abs(v) * 2.0 ** -4, np.broadcast_to(np.exp2(e.astype(np.float64) - 10)[:, :, None], (65536, 1, 32)).reshape(65536, 32))[fin]
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dt", [BF16, F16])
def test_host_quantiser_on_non_finite_and_edge_blocks(dt):
    K = 256
    x = torch.zeros(6, K)
    x[0, 0], x[0, 1], x[0, 2] = float("inf"), 448.0, -1.0                # inf beside finite values: e from the finite ones, inf -> 448
    x[0, 32], x[0, 33] = float("-inf"), float("nan")                     # no finite nonzero element: e = 0
    x[0, 64:96] = float("nan")
    x[1, 0], x[1, 1] = 448.0, 2.0 ** -9                                  # amax exactly 448: e = 0; the smallest subnormal survives
    x[1, 32], x[1, 33], x[1, 34] = _next_up(448.0, dt), 2.0 ** -10, 3 * 2.0 ** -10      # one ulp above: e = 1; .25 and .75 of the subnormal step
    x[1, 35], x[1, 36] = 2.0 ** -9, 3 * 2.0 ** -9                        # ... and its ties: .5 -> 0 (even), 1.5 -> 2
    x[1, 64], x[1, 65], x[1, 66] = 1.0, -0.0, 2.0 ** -20                 # 448 * 2^-9 < 1 <= 448 * 2^-8: e = -8; the tiny element rounds to zero
    x[2, :32] = torch.linspace(-1, 1, 32) * 1e-3
    x[3, 0], x[3, 1] = 60000.0, -30000.0
    x[4, 0], x[4, 1], x[4, 2] = 6.0e-8, -6.0e-8, 3.0e-8                   # fp16 subnormals / tiny bf16 values
    if dt == BF16:
        x[5, 0], x[5, 1], x[5, 32], x[5, 33] = 3.0e38, -1.0e38, 1.0e-38, 2.0e-39      # both ends of the bf16 range (the low one subnormal)
    x = x.to(dt)
    q, s = ops.mxfp8_quantize_rows(x)
    want_q, want_s, e, _ = ref_mxfp8(x)
    assert np.array_equal(s.numpy(), want_s) and np.array_equal(q.numpy(), want_q)
    assert int(s[0, 0]) == 127 and [int(q[0, k]) for k in range(3)] == [0x7E, 0x7E, 0x80 | 0x38]
    assert int(s[0, 1]) == 127 and int(q[0, 32]) == 0xFE and int(q[0, 33]) == 0x7F
    assert int(s[0, 2]) == 127 and bool((q[0, 64:96] == 0x7F).all())
    assert int(s[1, 0]) == 127 and int(q[1, 0]) == 0x7E and int(q[1, 1]) == 0x01
    assert int(s[1, 1]) == 128 and [int(q[1, k]) for k in (33, 34, 35, 36)] == [0x00, 0x01, 0x00, 0x02]
    assert int(s[1, 2]) == 127 - 8 and int(q[1, 64]) == 0x78 and int(q[1, 65]) == 0x80 and int(q[1, 66]) == 0x00
    assert bool((s[2, 1:] == 127).all()) and bool((q[2, 32:] == 0).all()), "all-zero blocks: e = 0, zero bytes"
    if dt == BF16:
        assert int(s[5, 0]) == 127 + 120 and int(s[5, 1]) == 0, "3.0e38 = 1.77 * 2^127: e = 120; a subnormal maximum: the bottom of the clamp"


def test_host_quantiser_reads_a_strided_source():
    x = (torch.randn(5, 96) * 3).to(BF16)
    wide = torch.full((5, 160), 7e4, dtype=BF16)
    wide[:, :96] = x
    qa, sa = ops.mxfp8_quantize_rows(wide[:, :96])
    qb, sb = ops.mxfp8_quantize_rows(x)
    assert torch.equal(qa, qb) and torch.equal(sa, sb)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals, without a device
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [True, False])
def test_packer_and_quantiser_refuse_float32_ragged_k_and_null_pointers(host):
    lib = L.lib()

    def pack(N, K, dtype, src=FAKE, dst=FAKE, ld=None):
        ld = K if ld is None else ld
        return lib.sl_pack_weight_mx_host(src, ld, dst, N, K, dtype) if host else lib.sl_pack_weight_mx(src, ld, dst, N, K, dtype, None)

    def quant(M, K, dtype, x=FAKE, q=FAKE, s=FAKE, ld=None):
        ld = K if ld is None else ld
        return lib.sl_mxfp8_quantize_rows_host(x, ld, q, s, M, K, dtype) if host else lib.sl_mxfp8_quantize_rows(x, ld, q, s, M, K, dtype, None)

    assert pack(16, 128, L.SL_F32) == ERR_UNSUPPORTED and "float32" in _err()
    assert pack(16, 64, L.SL_BF16) == ERR_ARG and "multiple of 128" in _err()
    assert pack(16, 192, L.SL_F16) == ERR_ARG and "multiple of 128" in _err()
    assert pack(16, 128, 7) == ERR_ARG and "dtype" in _err()
    assert pack(0, 128, L.SL_F16) == ERR_ARG
    assert pack(16, 128, L.SL_BF16, src=None) == ERR_ARG and pack(16, 128, L.SL_BF16, dst=None) == ERR_ARG
    assert pack(16, 128, L.SL_BF16, ld=127) == ERR_ARG and "ld_src" in _err()
    assert quant(4, 128, L.SL_F32) == ERR_UNSUPPORTED and "float32" in _err()
    assert quant(4, 48, L.SL_BF16) == ERR_ARG and "multiple of 32" in _err()
    assert quant(4, 128, 9) == ERR_ARG and "dtype" in _err()
    assert quant(0, 128, L.SL_F16) == ERR_ARG
    assert quant(4, 128, L.SL_F16, x=None) == ERR_ARG and quant(4, 128, L.SL_F16, q=None) == ERR_ARG and quant(4, 128, L.SL_F16, s=None) == ERR_ARG
    assert quant(4, 128, L.SL_F16, ld=100) == ERR_ARG and "ldx" in _err()


def _mx_args(M, N, K, dtype, act=L.ACT_NONE):
    a = L.GemmMxArgs()
    a.Aq, a.lda, a.a_scales, a.W, a.C, a.ldc = FAKE.value, K, FAKE.value, FAKE.value, FAKE.value, N
    a.M, a.N, a.K, a.dtype, a.act = M, N, K, dtype, act
    return a


def test_gemm_mx_refuses_what_is_not_built():
    lib = L.lib()
    assert lib.sl_gemm_mx(C.byref(_mx_args(4, 256, 256, L.SL_F32)), None) == ERR_UNSUPPORTED and "float32" in _err()
    assert lib.sl_gemm_mx(C.byref(_mx_args(4, 256, 192, L.SL_BF16)), None) == ERR_ARG and "multiple of 128" in _err()
    assert lib.sl_gemm_mx(C.byref(_mx_args(4, 256, 64, L.SL_F16)), None) == ERR_ARG and "multiple of 128" in _err()
    assert lib.sl_gemm_mx(C.byref(_mx_args(0, 256, 256, L.SL_BF16)), None) == ERR_ARG
    assert lib.sl_gemm_mx(C.byref(_mx_args(4, 256, 256, L.SL_BF16, act=L.ACT_GELU)), None) == ERR_ARG and "act" in _err()
    assert lib.sl_gemm_mx(C.byref(_mx_args(4, 48, 256, L.SL_BF16, act=L.ACT_SILU_MUL)), None) == ERR_ARG and "multiple of 32" in _err()
    a = _mx_args(4, 256, 256, L.SL_BF16)
    a.lda = 264
    assert lib.sl_gemm_mx(C.byref(a), None) == ERR_ARG and "lda" in _err()
    a = _mx_args(4, 256, 256, L.SL_BF16)
    a.W = None
    assert lib.sl_gemm_mx(C.byref(a), None) == ERR_ARG


def _model(dtype=L.SL_BF16, hidden=256, ffn=512, n_layers=3, reserved=L.WDEC_MX_LINEAR, dec=None):
    """TINY_LLAMA's dimensions; format 5 wants the four *_dec pointers of every layer NULL"""
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab = dtype, hidden, n_layers, 4, 2, 128, ffn, 1000
    m.rms_eps, m.rope_len = 1e-5, 512
    layers = (L.LlamaLayer * n_layers)()
    null_dec = (reserved == L.WDEC_MX_LINEAR) if dec is None else not dec
    for lay in layers:
        for name, _ in L.LlamaLayer._fields_:
            setattr(lay, name, None if (null_dec and name.endswith("_dec")) else FAKE.value)
    m.layers = layers
    m._keep = layers
    for f in ("embed", "lm_head", "final_norm", "rope_cos", "rope_sin", "lm_head_dec"):
        setattr(m, f, FAKE.value)
    m.dec_fused_norm, m.reserved = 1, reserved
    return m


def _kv(slots):
    kv = L.KVCache()
    kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx = FAKE.value, FAKE.value, slots, 64
    return kv


def _step(m, B=2):
    kv = _kv(64)
    return L.lib().sl_llama_decode_step(C.byref(m), C.byref(kv), FAKE, FAKE, B, FAKE, FAKE, 1 << 40, None)


def _generate(m, B=2):
    kv = _kv(64)
    cu = (C.c_int32 * (B + 1))(*range(0, 4 * (B + 1), 4))
    o = L.GenerateOpts()
    o.max_new_tokens = 4
    out = (C.c_int32 * (4 * B))()
    return L.lib().sl_generate(C.byref(m), C.byref(kv), FAKE, cu, B, C.byref(o), out, None, FAKE, 1 << 40, None)


def _prefill(m, B=2):
    kv = _kv(64)
    cu = (C.c_int32 * (B + 1))(*range(0, 4 * (B + 1), 4))
    return L.lib().sl_llama_prefill(C.byref(m), C.byref(kv), FAKE, cu, B, FAKE, FAKE, None, FAKE, 1 << 40, None)


@pytest.mark.parametrize("entry", [_step, _generate, _prefill], ids=["sl_llama_decode_step", "sl_generate", "sl_llama_prefill"])
def test_format_5_is_checked_before_any_launch(entry):
    assert entry(_model(dtype=L.SL_F32)) == ERR_UNSUPPORTED and "float32" in _err() and "format 5" in _err()
    assert entry(_model(ffn=576)) == ERR_UNSUPPORTED and "multiple of 128" in _err() and "576" in _err()
    assert entry(_model(hidden=320)) == ERR_UNSUPPORTED and "multiple of 128" in _err()
    assert entry(_model(dec=True)) == ERR_ARG and "*_dec" in _err() and "layer 0" in _err()
    m = _model()
    m.layers[2].wo_dec = FAKE.value
    assert entry(m) == ERR_ARG and "*_dec" in _err() and "layer 2" in _err()
    m = _model()
    m.layers[1].wgu = None
    assert entry(m) == ERR_ARG and "layer 1" in _err()


@pytest.mark.parametrize("entry", [_step, _generate], ids=["sl_llama_decode_step", "sl_generate"])
def test_codes_2_and_3_are_still_not_formats(entry):
    for bad in (2, 3, 6, 7):
        assert entry(_model(reserved=bad, dec=True)) == ERR_ARG and f"format {bad}" in _err()


def test_format_5_into_the_refusing_entries():
    lib = L.lib()
    m, kv = _model(), _kv(64)
    cu = (C.c_int32 * 3)(0, 4, 8)
    two = (C.c_int32 * 2)(1, 1)
    assert lib.sl_llama_score(C.byref(m), C.byref(kv), FAKE, cu, 2, two, two, FAKE, FAKE, None, None, None, None, None, FAKE, 1 << 40, None) == ERR_UNSUPPORTED
    assert "format 5" in _err() and "sl_llama_score" in _err()
    o = L.GenerateOpts()
    o.max_new_tokens, o.sample, o.temperature, o.top_p = 4, 1, 1.0, 1.0
    out = (C.c_int32 * 16)()
    assert lib.sl_generate_n(C.byref(m), C.byref(kv), FAKE, cu, 2, C.byref(o), out, None, FAKE, 1 << 40, None, None, None, 2) == ERR_UNSUPPORTED
    assert "format 5" in _err() and "sl_generate_n" in _err()


# ------------------------------------------------------------------------------------------------------------------------------
# workspace: the formats that existed report the bytes they reported; format 5 adds the quantised-row buffer
# ------------------------------------------------------------------------------------------------------------------------------
# sl_llama_workspace_bytes of the TINY_LLAMA structs (16-bit, e4m3 = reserved 1, MXFP4 = reserved 4; bf16 and fp16 alike) at
# (n_tok, nseq), recorded from the build of the parent commit a5d165b ("Edge suite: encoder front end and ragged-batch forms")
PARENT_WS = {(1, 1): 25860, (137, 1): 653572, (685, 5): 3258644}


@pytest.mark.parametrize("dtype", [L.SL_BF16, L.SL_F16])
def test_workspace_bytes_of_the_other_formats_are_unchanged_and_format_5_grows(dtype):
    lib = L.lib()
    for (n_tok, nseq), want in PARENT_WS.items():
        for reserved in (L.WDEC_MODEL_DTYPE, L.WDEC_E4M3, L.WDEC_MXFP4):
            m = _model(dtype=dtype, reserved=reserved, dec=True)
            assert lib.sl_llama_workspace_bytes(C.byref(m), n_tok, nseq) == want, (n_tok, nseq, reserved)
        mx = lib.sl_llama_workspace_bytes(C.byref(_model(dtype=dtype)), n_tok, nseq)
        grow = n_tok * 512 + n_tok * 16                                   # Kmax = 512 bytes and 16 scale bytes per row
        assert want + grow <= mx <= want + grow + 2 * 256, (n_tok, nseq, mx)


# ------------------------------------------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_constructor_option_refusals_and_the_default():
    arch = weights.LlamaArch(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=512,
                             vocab_size=100)
    mk = lambda a=arch, **kw: llama_mod.AudioLlamaForCausalLM(a, {}, **kw)
    assert mk(torch_dtype=BF16, linear_dtype="mx").linear_format == L.WDEC_MX_LINEAR
    assert mk(torch_dtype=F16, linear_dtype="mxfp8_mxfp4", kv_cache_dtype="fp8").linear_format == L.WDEC_MX_LINEAR      # independent of the K/V format
    llm = mk(torch_dtype=BF16)
    assert llm.linear_format == L.WDEC_MODEL_DTYPE and llm.weight_format == L.WDEC_MODEL_DTYPE                          # option unset: as before
    with pytest.raises(L.SpeechLLMError, match="float32"):
        mk(torch_dtype=torch.float32, linear_dtype="mx")
    for wd in ("mxfp4", "fp8"):
        with pytest.raises(L.SpeechLLMError, match="exclude each other"):
            mk(torch_dtype=BF16, linear_dtype="mx", weight_dtype=wd)
    llm = mk(torch_dtype=BF16, linear_dtype="mx")
    with pytest.raises(L.SpeechLLMError, match="exclude each other"):
        llm.set_weight_dtype("mxfp4")
    llm = mk(torch_dtype=BF16, weight_dtype="mxfp4")
    with pytest.raises(L.SpeechLLMError, match="exclude each other"):
        llm.set_linear_dtype("mx")
    llm.set_weight_dtype(None)
    llm.set_linear_dtype("mx")
    assert llm.linear_format == L.WDEC_MX_LINEAR
    llm.set_linear_dtype(None)
    assert llm.linear_format == L.WDEC_MODEL_DTYPE
    odd = weights.LlamaArch(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=576,
                            vocab_size=100)
    with pytest.raises(L.SpeechLLMError, match="multiple of 128"):
        mk(odd, torch_dtype=BF16, linear_dtype="mx")
    with pytest.raises(L.SpeechLLMError):
        mk(torch_dtype=BF16, linear_dtype="fp8")


def test_config_key_and_shipped_configs():
    assert cfgm.runtime_linear_dtype(cfgm.from_dict(dict(runtime=dict(linear_dtype="mx")))) == "mx"
    assert cfgm.runtime_linear_dtype(cfgm.from_dict(dict(runtime=dict(linear_dtype="mxfp8_mxfp4")))) == "mx"
    assert cfgm.runtime_linear_dtype(cfgm.from_dict(dict(runtime=dict(linear_dtype="model")))) is None
    assert cfgm.runtime_linear_dtype(cfgm.from_dict(dict())) is None
    with pytest.raises(ValueError):
        cfgm.runtime_linear_dtype(cfgm.from_dict(dict(runtime=dict(linear_dtype="fp8"))))
    for f in ("llama3_hubert", "llama3_whisper", "minichat_hubert", "minichat_whisper"):      # the option is off by default
        assert cfgm.runtime_linear_dtype(cfgm.load_config(os.path.join(REPO, "config", f + ".yaml"))) is None
