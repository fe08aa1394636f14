"""Helpers shared by the chapters of the edge suite (tests/test_kernel_edges_gpu.py, tests/test_train_edges_gpu.py,
tests/test_train_gemm_edges_gpu.py, tests/test_frontend_edges_gpu.py): dtypes and their half-ulps, finite poison, the output sentinel, guarded output buffers, poisoned
operand views, the per-element comparison and the `tuning` fixture.  A plain module, not a conftest: the test files import what they use."""
import pytest
import torch

from conftest import pkg

L = pkg("_lib")

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTS = [F16, BF16, F32]
DT16 = [F16, BF16]
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}        # half an ulp, relative
BIG = {F16: 60000.0, BF16: 1e30, F32: 1e30}                    # finite poison
E24 = 2.0 ** -24
FILL = -1504.0                                                 # output sentinel (exact in all three types)


# ------------------------------------------------------------------------------------------------------------------------------
# helpers: data, guarded buffers, bounds
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tuning(monkeypatch):
    """Set an SL_* tuning switch and re-read the library's table; the table is restored in the finalizer, so a failing assert
    between the two reloads cannot leave a switch latched for the rest of the process."""
    def set_(name, value):
        monkeypatch.setenv(name, value)
        L.lib().sl_tuning_reload()

    yield set_
    monkeypatch.undo()
    L.lib().sl_tuning_reload()


def _set(tuning, switches):
    for k, v in switches.items():
        tuning(k, v)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def gauss(shape, seed, std=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * std).double()


def guarded(rows, cols, dtype):
    """(buffer, view): the view is rows x cols inside a sentinel-filled buffer, one row above and below, 8 elements left and at
    least 8 right; leading dimension and offset are multiples of 8 elements (16-byte alignment of the fast paths holds)."""
    ld = (cols + 7) // 8 * 8 + 16
    buf = torch.full((rows + 2, ld), FILL, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1, 8:8 + cols]


def untouched(buf, rows, cols):
    chk = buf.clone()
    chk[1:rows + 1, 8:8 + cols] = FILL
    return bool((chk == FILL).all())


def guarded_flat(n, dtype, pad=64):
    """(buffer, view): n contiguous elements inside a sentinel-filled buffer, `pad` elements (a multiple of 8) in front and behind - for
    the kernels that write packed rows and take no leading dimension"""
    buf = torch.full((n + 2 * pad,), FILL, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n]


def untouched_flat(buf, n, pad=64):
    return bool((buf[:pad] == FILL).all()) and bool((buf[pad + n:] == FILL).all())


def operand_flat(x64, dtype, pad=64, poison=None):
    """x64 of any shape -> (contiguous device view of that shape, its exact stored value in fp64 on the CPU); `pad` elements of
    +-poison in front of and behind it inside the same allocation"""
    big = BIG[dtype] if poison is None else poison
    buf = torch.full((x64.numel() + 2 * pad,), big, dtype=torch.float64)
    buf[::2] *= -1.0
    buf[pad:pad + x64.numel()] = x64.reshape(-1)
    buf = buf.float().to(dtype).to(DEV)
    v = buf[pad:pad + x64.numel()].view(x64.shape)
    return v, v.double().cpu()


def operand(x64, dtype, poison=None):
    """x64 (rows, cols) -> (device view with a leading dimension > cols, its exact stored value in fp64 on the CPU).  Pad columns,
    the row above and two rows below hold +-poison."""
    rows, cols = x64.shape
    ld = (cols + 7) // 8 * 8 + 16
    big = BIG[dtype] if poison is None else poison
    buf = torch.full((rows + 3, ld), big, dtype=torch.float64)
    buf[:, ::2] *= -1.0
    buf[1:rows + 1, 8:8 + cols] = x64
    buf = buf.float().to(dtype).to(DEV)
    v = buf[1:rows + 1, 8:8 + cols]
    return v, v.double().cpu()


def vec(x64, dtype):
    d = x64.float().to(dtype).to(DEV)
    return d, d.double().cpu()


def to_dt(x64, dtype):
    """fp64 -> dtype as torch rounds an fp32 value (round-to-nearest-even, overflow to inf, subnormals kept)"""
    return x64.float().to(dtype)


_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def bad(got, want, tol=None, bits=False):
    """"" if every element agrees: exactly (tol None; bits=True compares the bit patterns, so -0 is not +0), or within tol"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    if bits:
        assert tol is None and got.dtype == want.dtype
        wrong = got.view(_BITS[got.element_size()]) != want.view(_BITS[want.element_size()])
    else:
        wrong = (got != want) if tol is None else ~((got.double() - want.double()).abs() <= tol)
    if not bool(wrong.any()):
        return ""
    i = tuple(wrong.nonzero()[0].tolist())
    worst = "" if tol is None else f", worst err/tol {float(((got.double() - want.double()).abs() / tol).max()):.3g}"
    return f"{int(wrong.sum())} of {wrong.numel()} elements wrong, first at {i}: got {float(got[i])!r} want {float(want[i])!r}{worst}"
