"""GPU, per element: the ctc_pool and stack downsampling kernels on packed ragged batches (sl_segment_mean_batch / _bwd_batch,
sl_stack_rows_batch / _bwd_batch) in fp16 / bf16 / fp32, written in the manner of the edge suite (tests/edge_helpers.py): guarded output
buffers, finite poison around and between the utterances, and bounds derived from the arithmetic the kernels are specified to do.

Bounds (u32 = 2^-24, the fp32 unit roundoff; U[dt] = half an ulp of the storage type, 0 for fp32 where nothing is rounded again):
  forward   y[r] = mean of n rows: fp32 accumulation of n terms (|error| <= (n - 1) u32 sum|x|), one division (u32 relative), one rounding to
            the storage type  ->  |y - mean| <= ((n + 1) u32 + U) * sum|x| / n, second-order terms covered by the factor 1 + 2^-10.
            With small-integer inputs every partial sum is an integer below 2^24, so the accumulation is exact in any order; when n is a power of two
            the division is exact too and y must equal the fp64 mean rounded once to the storage type.
  backward  dx[t] = sum of k terms dy[r] / n_r: one division per term (u32), k - 1 fp32 additions, one rounding to the storage type
            ->  |dx - sum| <= (k u32 + U) * sum|dy[r] / n_r| (same second-order factor); k = 0 gives exactly 0.
  stack     both directions are copies: exact.
"""
import pytest
import torch

from conftest import pkg
from edge_helpers import BIG, BF16, DEV, DTS, E24, F32, FILL, U, bad, ints, to_dt

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")

T_UTT = (5, 49, 1, 130)
# utterance-relative (start, end) pairs, as a dataset row stores them
RANGES = (
    [(2, 3),                       # one frame
     (0, 5),                       # the whole utterance, ending exactly at T_u
     (3, 9)],                      # end past T_u: clamped to (3, 5) — must not read the next utterance's first frame
    [(8, 16), (12, 20),            # two overlapping ranges
     (20, 24), (20, 24),           # a repeated range
     (40, 47), (30, 33),           # an unsorted pair
     (45, 49),                     # ends exactly at T_u
     (44, 60)],                    # end past T_u; frames 0..7, 24..29, 33..39 stay uncovered
    [(0, 1)],                      # the whole of the T = 1 utterance
    [(0, 130), (64, 128)],         # one 130-frame range (and a 64-frame one inside it)
)
CASES = [(dt, H) for dt in DTS for H in ((4, 1024) if dt == F32 else (8, 16, 1024))]
SECOND_ORDER = 1.0 + 2.0 ** -10


def store_u(dt):
    return 0.0 if dt == F32 else U[dt]


def offsets(lens):
    o = [0]
    for n in lens:
        o.append(o[-1] + n)
    return o


def clamp(ranges, T):
    return [[(min(max(s, 0), t_), min(max(e, 0), t_)) for s, e in r] for r, t_ in zip(ranges, T)]


def frames_buffer(x64, dt):
    """(NT, H) frames between one poison row above and one below -> the (contiguous) device view of the frames"""
    buf = torch.full((x64.shape[0] + 2, x64.shape[1]), BIG[dt], dtype=torch.float64)
    buf[1:-1] = x64
    return buf.float().to(dt).to(DEV)[1:-1]


def out_buffer(rows, cols, dt):
    """sentinel-filled (rows + 2, cols) buffer and its middle rows: a guard row above and below a DENSE output (the kernels write rows of cols elements)"""
    buf = torch.full((rows + 2, cols), FILL, dtype=dt, device=DEV)
    return buf, buf[1:rows + 1]


def guards_intact(buf):
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


@pytest.fixture(scope="module")
def table():
    """the packed table and its inverse index, built once by the host routines (checked against brute force in test_downsample_host_cpu.py)"""
    packed, counts = ops.segment_ranges_pack(RANGES, T_UTT)
    row_ptr, cols = ops.segment_csr(packed, sum(T_UTT))
    toff, cl = offsets(T_UTT), clamp(RANGES, T_UTT)
    want = [[toff[u] + s, toff[u] + e] for u in range(len(T_UTT)) for s, e in cl[u]]
    assert packed.tolist() == want and counts == [len(r) for r in RANGES]
    return packed, counts, row_ptr, cols


@pytest.mark.parametrize("dt,H", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_segment_mean_forward_per_element_with_every_other_utterance_poisoned(table, dt, H):
    packed, counts, _, _ = table
    NT, R = sum(T_UTT), packed.shape[0]
    toff, roff = offsets(T_UTT), offsets(counts)
    x64 = ints((NT, H), -4, 4, seed=11 + H)
    ranges_dev = packed.to(DEV)
    lens = (packed[:, 1] - packed[:, 0]).tolist()
    mean64 = torch.stack([x64[s:e].mean(0) for s, e in packed.tolist()])
    mean_abs = torch.stack([x64[s:e].abs().mean(0) for s, e in packed.tolist()])
    assert any(n == 1 for n in lens) and any(n == 130 for n in lens) and sum(1 for n in lens if n & (n - 1) == 0) >= 6

    def check(got, rows, what):
        for r in rows:
            n = lens[r]
            if n & (n - 1) == 0:      # a power of two: exact
                msg = bad(got[r], to_dt(mean64[r], dt))
            else:
                msg = bad(got[r], mean64[r], tol=((n + 1) * E24 + store_u(dt)) * mean_abs[r] * SECOND_ORDER)
            assert not msg, f"{what}: range {r} {packed[r].tolist()} (n = {n}): {msg}"

    buf, y = out_buffer(R, H, dt)
    ops.segment_mean_batch(frames_buffer(x64, dt), ranges_dev, out=y)
    assert guards_intact(buf), "guard rows written"
    check(y, range(R), "clean")
    for u in range(len(T_UTT)):      # every other utterance's frames poisoned: u's means must not move
        xp = x64.clone()
        sign = torch.ones(NT, 1, dtype=torch.float64)
        sign[::2] = -1.0
        keep = torch.zeros(NT, dtype=torch.bool)
        keep[toff[u]:toff[u + 1]] = True
        xp = torch.where(keep[:, None], xp, sign * BIG[dt])
        buf, y = out_buffer(R, H, dt)
        ops.segment_mean_batch(frames_buffer(xp, dt), ranges_dev, out=y)
        assert guards_intact(buf)
        check(y, range(roff[u], roff[u + 1]), f"utterance {u} among poisoned neighbours")


@pytest.mark.parametrize("dt,H", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_segment_mean_backward_per_element_zeros_where_uncovered_and_order_independent(table, dt, H):
    packed, counts, row_ptr, cols = table
    NT, R = sum(T_UTT), packed.shape[0]
    toff, roff = offsets(T_UTT), offsets(counts)
    dy64 = ints((R, H), -8, 8, seed=23 + H)
    lens = (packed[:, 1] - packed[:, 0]).double()
    want = torch.zeros((NT, H), dtype=torch.float64)
    mag = torch.zeros((NT, H), dtype=torch.float64)
    k = torch.zeros(NT, dtype=torch.float64)
    for r, (s, e) in enumerate(packed.tolist()):
        want[s:e] += dy64[r] / lens[r]
        mag[s:e] += dy64[r].abs() / lens[r]
        k[s:e] += 1
    assert int(k.max()) >= 3 and int((k == 0).sum()) >= 20          # a frame under three ranges, and the gaps of utterance 1

    def run(packed_, row_ptr_, cols_, dy_):
        buf, dx = out_buffer(NT, H, dt)
        dyb = torch.full((R + 2, H), BIG[dt], dtype=torch.float64)
        dyb[1:-1] = dy_
        ops.segment_mean_bwd_batch(dyb.float().to(dt).to(DEV)[1:-1], packed_.to(DEV), row_ptr_.to(DEV), cols_.to(DEV), NT, out=dx)
        assert guards_intact(buf), "guard rows written"
        return dx

    dx = run(packed, row_ptr, cols, dy64)
    uncovered = k == 0
    assert bool((dx[uncovered.to(DEV)] == 0).all()), "a frame no range covers must be exactly 0"
    msg = bad(dx, want, tol=(k[:, None] * E24 + store_u(dt)) * mag * SECOND_ORDER)
    assert not msg, msg
    # the same table presented in another order of utterances: every utterance's rows come out bit for bit the same
    order = (3, 1, 0, 2)
    T2 = [T_UTT[u] for u in order]
    packed2, counts2 = ops.segment_ranges_pack([RANGES[u] for u in order], T2)
    row_ptr2, cols2 = ops.segment_csr(packed2, NT)
    dx2 = run(packed2, row_ptr2, cols2, torch.cat([dy64[roff[u]:roff[u + 1]] for u in order]))
    toff2 = offsets(T2)
    for i, u in enumerate(order):
        msg = bad(dx2[toff2[i]:toff2[i + 1]], dx[toff[u]:toff[u + 1]], bits=True)
        assert not msg, f"utterance {u} moved to slot {i}: {msg}"


T_STACK = (1, 3, 4, 5, 8, 130)


@pytest.mark.parametrize("dt,H", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_stack_rows_both_directions_are_exact_copies(dt, H):
    f = 4
    NT = sum(T_STACK)
    toff = offsets(T_STACK)
    P = [t_ // f for t_ in T_STACK]
    assert P == [0, 0, 1, 1, 2, 32]                    # T = 1, 3: no rows; T = 4, 8: every frame kept (Q5)
    poff = offsets(P)
    x64 = ints((NT, H), -100, 100, seed=31 + H)
    buf, y = out_buffer(poff[-1], f * H, dt)
    y2, P2 = ops.stack_rows_batch(frames_buffer(x64, dt), T_STACK, f, out=y)
    assert P2 == P and guards_intact(buf)
    want = torch.cat([x64[toff[u]:toff[u] + P[u] * f].reshape(P[u], f * H) for u in range(len(P))])
    msg = bad(y, to_dt(want, dt))
    assert not msg, msg
    # backward: the stacked rows go back to their frames, the T % f cropped frames get exact zeros
    dy64 = ints((poff[-1], f * H), -100, 100, seed=37 + H)
    dyb = torch.full((poff[-1] + 2, f * H), BIG[dt], dtype=torch.float64)
    dyb[1:-1] = dy64
    buf, dx = out_buffer(NT, H, dt)
    ops.stack_rows_bwd_batch(dyb.float().to(dt).to(DEV)[1:-1], T_STACK, f, out=dx)
    assert guards_intact(buf)
    want = torch.zeros((NT, H), dtype=torch.float64)
    for u in range(len(P)):
        want[toff[u]:toff[u] + P[u] * f] = dy64[poff[u]:poff[u + 1]].reshape(P[u] * f, H)
    msg = bad(dx, to_dt(want, dt), bits=True)
    assert not msg, msg
    cropped = torch.ones(NT, dtype=torch.bool)
    for u in range(len(P)):
        cropped[toff[u]:toff[u] + P[u] * f] = False
    assert int(cropped.sum()) == 1 + 3 + 0 + 1 + 0 + 2 and bool((dx[cropped.to(DEV)] == 0).all())


def test_stack_of_utterances_shorter_than_one_row_gives_no_rows_and_zero_gradient():
    y, P = ops.stack_rows_batch(torch.ones((4, 8), dtype=BF16, device=DEV), (1, 3), 4)
    assert P == [0, 0] and tuple(y.shape) == (0, 32)
    dx = ops.stack_rows_bwd_batch(y, (1, 3), 4)
    assert tuple(dx.shape) == (4, 8) and bool((dx == 0).all())
