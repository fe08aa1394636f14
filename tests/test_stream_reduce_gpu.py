"""The K-split reduce pass with row statistics (gemm_stream.hip: gemm_stream_reduce_rowstat_kernel), checked against the partial
records it sums: they stay in the split workspace after the call, so the expected row is formed from the very same numbers."""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")

K = 4608      # 72 K stages of 64 (16-bit) / 144 of 32 (fp32): 2, 3, 8 and 9 splits all divide it, so none comes out empty
EPS = 1e-5


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def tuning(monkeypatch):
    """Set an SL_* tuning switch and re-read the library's table; restored in the finalizer."""
    def set_(name, value):
        monkeypatch.setenv(name, value)
        L.lib().sl_tuning_reload()

    yield set_
    monkeypatch.undo()
    L.lib().sl_tuning_reload()


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_reduce_pass(M, N, splits, dt, tuning, residual):
    """x bit for bit = ((0 + p0) + p1 + ...) in split order, + residual, rounded once; rstd against float64 at 1e-6 relative;
    norm_out within one unit in the last place of weight * (x * rstd).to(dtype)."""
    tuning("SL_STREAM_CFG", f"{splits},0")       # 128-row blocks (fp32, or <= 384 rows)
    tuning("SL_STREAM_WSPLITS", str(splits))     # 256 x 128 blocks
    code = L.dtype_code(dt)
    assert L.lib().sl_gemm_split_count(M, N, K, code) == splits
    a = rnd(M, K, seed=70).to(dev(), dt)
    wp = ops.pack_weight(rnd(N, K, seed=71, std=K ** -0.5).to(dev(), dt))
    res = None
    if residual == "aligned":
        res = rnd(M, N, seed=72).to(dev(), dt)
    elif residual == "odd pitch":        # rows that start on odd elements: no 8- / 16-byte pieces
        res = rnd(M, N + 1, seed=72).to(dev(), dt)[:, 1:]
    gain = (1.0 + rnd(N, seed=73, std=0.1)).to(dev(), dt)
    np_ = (N + 15) // 16 * 16
    hdr = 8192 + ((32 * M * 4 + 255) & ~255)     # fix-up counters + row-statistics partials in front of the records
    outs = []
    for with_norm in (False, True):
        rstd = torch.zeros(M, device=dev(), dtype=torch.float32)
        h = torch.zeros(M, N, device=dev(), dtype=dt) if with_norm else None
        x = ops.gemm_decode(a, wp, N, residual=res, rstd_out=rstd, eps=EPS, norm_out=h, norm_gain=gain if with_norm else None)
        ws = ops._SPLIT_WS[dev()]
        part = ws[hdr:hdr + splits * M * np_ * 4].view(torch.float32).view(splits, M, np_)[:, :, :N]
        acc = torch.zeros(M, N, device=dev(), dtype=torch.float32)
        for sp in range(splits):
            acc = acc + part[sp]
        want = (acc + res.float() if res is not None else acc).to(dt)
        assert torch.equal(bits(x), bits(want)), f"x differs in {(bits(x) != bits(want)).sum().item()} elements"
        ref = torch.rsqrt(x.double().pow(2).mean(-1) + EPS)
        err = ((rstd.double() - ref).abs() / ref).max().item()
        print(f"M={M} N={N} splits={splits} {dt} norm_out={with_norm}: rstd max rel err {err:.3e}")
        assert err < 1e-6
        if with_norm:
            hw = (gain.float() * (x.float() * rstd[:, None]).to(dt).float()).to(dt)
            ulp = (bits(h).to(torch.int64) - bits(hw).to(torch.int64)).abs().max().item()
            print(f"    norm_out max distance {ulp} ulp")
            assert ulp <= 1
        outs.append((x, rstd))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("splits", [2, 3, 8, 9])
@pytest.mark.parametrize("N", [3072, 1040])
@pytest.mark.parametrize("M", [1024, 1000, 130])
def test_rowstat_reduce_pass_against_its_partial_records(M, N, splits, dt, tuning):
    """The decode chain's form (residual rows of the storage type in aligned pieces).  Row counts with a ragged last block, a width
    whose last 64-lane group is mostly empty (1 040 = 65 fragments), split counts on both sides of the load groups of 2 and 4."""
    check_reduce_pass(M, N, splits, dt, tuning, "aligned")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("residual", ["none", "odd pitch"])
@pytest.mark.parametrize("splits", [2, 9])
@pytest.mark.parametrize("M,N", [(130, 1040), (1000, 3072)])
def test_rowstat_reduce_pass_general_form(M, N, splits, residual, dt, tuning):
    """The same checks on the kernel's general form: no residual, and residual rows that cannot move in aligned pieces."""
    check_reduce_pass(M, N, splits, dt, tuning, residual)
