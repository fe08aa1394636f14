"""GPU: the backward, loss and optimizer kernels of the KD step (csrc/train_ops.hip) in fp32 / bf16 at the shapes that break kernels, checked
PER ELEMENT - the third chapter of the edge suite (tests/test_kernel_edges_gpu.py holds the first two).

References and bounds are tests/train_ops_ref.py: fp64 on the STORED inputs, a bound per element that counts the kernels' fp32 roundings
(tests/test_train_ref_cpu.py shows on the CPU that the references are the operations, that a planted defect leaves the bounds and that an
fp32 restatement stays inside them).  Kinds of input, named as in the first chapter:
  E  exact: integer operands whose sums are exact in fp32 in any order (atomics included), torch.equal; single roundings restated in
     fp32 torch (dropout, the optimizer's compute-dtype copy); softmax rows and loss rows whose result is 0, 1 or 2^-6 by construction.
  Z  zero probes: dy non-zero in one row (one time step for conv0) - every other row of dx is exactly zero, dbeta is that row.
  G  Gaussian, per element under the derived bound; parameter gradients that come out of atomics under the bound, the scratch-record
     forms (fixed order) also identical over two calls.
  Guard bands and poison, in every case: every output - overwritten or accumulated into - is a 16-byte-aligned slice of a sentinel-filled
  buffer with 64 sentinel elements before and after that must come back untouched; every input slice lies between 64 elements of large
  finite values of alternating sign; masked scores, pad columns and source rows behind the last window hold 1e30.
One case per kernel form at the smallest shape that selects it (the launchers of train_ops.hip decide; the rules are restated beside each
test).  No tolerance here is a measured number, and nothing compares two forms of a kernel with each other only: where two forms promise
the same bits that is asserted IN ADDITION to the reference check.  Exceptions: none.
"""

import pytest
import torch

import train_ops_ref as R
from conftest import pkg
from edge_helpers import BF16, BIG, DEV, E24, F16, F32, FILL, U, bad, tuning  # noqa: F401

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")

DTS = [F32, BF16]
VEC = R.VEC
EPS = 1e-5
GUARD = 64


# ------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------
def call(name, *args):
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr()), name)


def out_buf(shape, dtype, init=None, off=GUARD):
    """(buffer, view): a dense view of `shape` inside a flat sentinel-filled buffer, `off` >= 64 sentinel elements before it and 64 after;
    off = 64 keeps the view 16-byte aligned.  init: the view's starting values (fp64 / any), else the sentinel."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((off + n + GUARD,), FILL, dtype=dtype, device=DEV)
    view = buf[off:off + n].view(*shape)
    if init is not None:
        view.copy_(init.to(DEV).float().to(dtype).view(*shape))
    return buf, view


def intact(buf, view):
    n, off = view.numel(), view.storage_offset()
    return bool((buf[:off] == FILL).all()) and bool((buf[off + n:] == FILL).all())


def pin(x64, dtype, poison=None):
    """x64 -> (dense device view between 64 poisoned elements on either side, its stored value in fp64 on the CPU)"""
    n = x64.numel()
    big = BIG[dtype] if poison is None else poison
    buf = torch.full((n + 2 * GUARD,), big, dtype=torch.float64)
    buf[::2] *= -1.0
    buf[GUARD:GUARD + n] = x64.reshape(-1)
    buf = buf.float().to(dtype).to(DEV)
    v = buf[GUARD:GUARD + n].view(*x64.shape)
    return v, v.double().cpu()


def ok(got, want, tol, what):
    msg = bad(got, want, tol)
    assert not msg, f"{what}: {msg}"


def ptr(t):
    return L.ptr(t)


def code(dt):
    return L.dtype_code(dt)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. LayerNorm backward.  Launcher rules (layernorm_bwd_impl): cols <= 1024 -> 16 floats per lane; with a workspace of at least
#    nb * 2 * cols * 4 bytes the scratch-record form (gelu: float copies, 16 waves; else lean with SL_LNBWD_NW = 16 / 8 / 4 waves) +
#    norm_colreduce_kernel, else atomics on 16-wave blocks of 16 rows; cols > 1024 -> the general TR_MAXF form, 4 waves, 4 rows per block.
# ------------------------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def ln_rows_per_block(entry, nw, rows, cols):
    if cols > 1024:
        return min(64, max(4, ceil_div(ceil_div(rows, 256), 4) * 4))
    if entry == "ws":
        return max(nw, ceil_div(ceil_div(rows, 256 * (16 // nw)), nw) * nw)
    lnb = min(256, max(64, rows // 64))
    return max(16, ceil_div(ceil_div(rows, lnb), 16) * 16)


def ln_run(entry, dt, x, g, b, dy, rows, cols, gelu, g0, b0, ws=None, ws_bytes=None):
    """one launch on fresh guarded outputs -> (dx, dgamma, dbeta), guard bands checked"""
    bx, dx = out_buf((rows, cols), dt)
    bg, dgam = out_buf((cols,), F32, g0)
    bb, dbet = out_buf((cols,), F32, b0)
    if entry == "atomics":
        call("sl_layernorm_bwd", ptr(x), ptr(g), ptr(b), ptr(dy), ptr(dx), ptr(dgam), ptr(dbet), rows, cols, EPS, int(gelu), code(dt))
    else:
        if ws is None:
            ws = torch.empty(int(L.lib().sl_layernorm_bwd_ws_bytes(rows, cols)), dtype=torch.uint8, device=DEV)
        call("sl_layernorm_bwd_ws", ptr(x), ptr(g), ptr(b), ptr(dy), ptr(dx), ptr(dgam), ptr(dbet), rows, cols, EPS, int(gelu), code(dt), ptr(ws),
             ws.numel() if ws_bytes is None else ws_bytes)
    assert intact(bx, dx) and intact(bg, dgam) and intact(bb, dbet), "write outside dx / dgamma / dbeta"
    return dx, dgam, dbet


def ln_case(entry, nw, dt, rows, cols, gelu, seed):
    """G, E and Z on one form and shape"""
    x64, g64, b64, dy64 = R.norm_inputs(rows, cols, dt, seed)
    x, x64 = pin(x64, dt)
    g, g64 = pin(g64, dt)
    b, b64 = pin(b64, dt)
    g0, b0 = R.ints((cols,), -3, 3, seed + 7), R.ints((cols,), 1, 3, seed + 8)
    what = f"{entry} nw={nw} {rows} x {cols} gelu={gelu}"

    def run_and_check(dy64, kind, zero_rows=None, exact_dbeta=False):
        dy, dy_st = pin(dy64, dt)
        ref = R.norm_bwd_ref(x64, g64, b64, dy_st, EPS, gelu=gelu, dt=dt, dgamma0=g0, dbeta0=b0)
        dx, dgam, dbet = ln_run(entry, dt, x, g, b, dy, rows, cols, gelu, g0, b0)
        ok(dx, ref.dx, ref.tol_dx, f"{kind} dx {what}")
        ok(dgam, ref.dgamma, ref.tol_dgamma, f"{kind} dgamma {what}")
        ok(dbet, ref.dbeta, ref.tol_dbeta, f"{kind} dbeta {what}")
        if zero_rows is not None:
            assert bool((dx[zero_rows] == 0).all()), f"{kind} {what}: dx is not exactly zero in a row whose dy is zero"
        if exact_dbeta:
            assert torch.equal(dbet.cpu().double(), ref.dbeta), f"{kind} {what}: dbeta of integer dy is not exact"
        if entry == "ws" and cols <= 1024:          # the records are summed in a fixed order
            _, dgam2, dbet2 = ln_run(entry, dt, x, g, b, dy, rows, cols, gelu, g0, b0)
            assert torch.equal(dgam2, dgam) and torch.equal(dbet2, dbet), f"{kind} {what}: two calls differ"

    run_and_check(dy64, "G")
    run_and_check(R.ints((rows, cols), -4, 4, seed + 9), "E", exact_dbeta=not gelu)
    rpb = ln_rows_per_block(entry, nw, rows, cols)
    for r_star in sorted({0, rows - 1, min(rpb, rows) - 1, (rows - 1) // rpb * rpb}):
        dyz = torch.zeros(rows, cols, dtype=torch.float64)
        dyz[r_star] = R.ints((cols,), 1, 4, seed + r_star) * (1 - 2 * (torch.arange(cols) % 2))
        others = torch.ones(rows, dtype=torch.bool)
        others[r_star] = False
        run_and_check(dyz, f"Z r*={r_star}", zero_rows=others.to(DEV), exact_dbeta=not gelu)


LN_SHAPES = [(33, c) for c in R.LN_COLS] + [(r, "65vec") for r in R.LN_ROWS if r != 33]


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("gelu", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_bwd_atomics(dt, gelu, rows, cols):
    """sl_layernorm_bwd: lean 16-wave (cols <= 1024, no GELU), float-copy 16-wave (GELU), general 4-wave (cols > 1024)"""
    ln_case("atomics", 16, dt, rows, R.cols_of(cols, dt), gelu, 1000 + rows)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("nw,gelu", [(16, False), (16, True), (8, False), (4, False)])
@pytest.mark.parametrize("rows,cols", [(r, c) for r, c in LN_SHAPES if c in ("vec", "63vec", "65vec", 1024)] + [(2065, "vec")])
def test_layernorm_bwd_scratch_records(dt, nw, gelu, rows, cols, tuning):
    """sl_layernorm_bwd_ws + norm_colreduce_kernel.  2 065 rows at cols = vec: 130 blocks of 16 rows (nw = 16) - the stripe loop of the
    column reduce takes a second round of 128 blocks with a ragged tail; the probes include row 2 064."""
    if nw != 16:
        tuning("SL_LNBWD_NW", str(nw))
    ln_case("ws", nw, dt, rows, R.cols_of(cols, dt), gelu, 2000 + rows)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_layernorm_bwd_workspace_one_byte_short_takes_the_atomics_form(dt):
    rows, cols = 33, 65 * VEC[dt]
    x64, g64, b64, dy64 = R.norm_inputs(rows, cols, dt, 31)
    (x, x64), (g, g64), (b, b64), (dy, dy64) = pin(x64, dt), pin(g64, dt), pin(b64, dt), pin(dy64, dt)
    g0, b0 = R.ints((cols,), -3, 3, 1), R.ints((cols,), 1, 3, 2)
    ref = R.norm_bwd_ref(x64, g64, b64, dy64, EPS, dt=dt, dgamma0=g0, dbeta0=b0)
    need = ceil_div(rows, ln_rows_per_block("ws", 16, rows, cols)) * 2 * cols * 4
    assert need <= int(L.lib().sl_layernorm_bwd_ws_bytes(rows, cols))
    for nbytes, touched in ((need - 1, False), (need, True)):
        ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        dx, dgam, dbet = ln_run("ws", dt, x, g, b, dy, rows, cols, False, g0, b0, ws=ws, ws_bytes=nbytes)
        ok(dx, ref.dx, ref.tol_dx, f"dx ws_bytes={nbytes}")
        ok(dgam, ref.dgamma, ref.tol_dgamma, f"dgamma ws_bytes={nbytes}")
        ok(dbet, ref.dbeta, ref.tol_dbeta, f"dbeta ws_bytes={nbytes}")
        assert bool((ws != 0x5A).any()) == touched, f"workspace of {nbytes} bytes (need {need}): touched must be {touched}"
        assert bool((ws[need:] == 0x5A).all())


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_norm_bwd_refuses_rows_wider_than_4096(dt):
    rows, cols = 2, 4096 + VEC[dt]
    x = torch.zeros(rows, cols, dtype=dt, device=DEV)
    gb = torch.ones(cols, dtype=dt, device=DEV)
    bx, dx = out_buf((rows, cols), dt)
    bg, dg = out_buf((cols,), F32)
    with pytest.raises(L.SpeechLLMError):
        call("sl_layernorm_bwd", ptr(x), ptr(gb), ptr(gb), ptr(x), ptr(dx), ptr(dg), ptr(dg), rows, cols, EPS, 0, code(dt))
    with pytest.raises(L.SpeechLLMError):
        call("sl_rmsnorm_bwd", ptr(x), ptr(gb), ptr(x), ptr(dx), rows, cols, EPS, code(dt))
    torch.cuda.synchronize()
    assert bool((bx == FILL).all()) and bool((bg == FILL).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 2. RMSNorm backward (sl_rmsnorm_bwd_add_impl): SL_RMSBWD_LEAN = 2 (default; MAXF = 48 up to 3 072 columns, 64 above), 0 (float copies),
#    1 / 3 (16 / 8 rows per block above 2 048 rows, else 4)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(r, c) for c in R.RMS_COLS for r in R.RMS_ROWS] + [(2049, "vec")])
def test_rmsnorm_bwd(dt, rows, cols, tuning):
    cols = R.cols_of(cols, dt)
    x64, g64, _, dy64 = R.norm_inputs(rows, cols, dt, 3000 + rows, rms=True)
    (x, x64), (g, g64) = pin(x64, dt), pin(g64, dt)
    leans = ["2", "0"] + (["1", "3"] if rows > 2048 else [])
    rpbs = {"2": 4, "0": 4 if rows <= 2048 else 16, "1": 16, "3": 8}
    probes = sorted({r for ln in leans for r in (0, rows - 1, min(rpbs[ln], rows) - 1, (rows - 1) // rpbs[ln] * rpbs[ln])})
    inputs = [("G", dy64, None)]
    for r_star in probes:
        dyz = torch.zeros(rows, cols, dtype=torch.float64)
        dyz[r_star] = R.ints((cols,), 1, 4, r_star) * (1 - 2 * (torch.arange(cols) % 2))
        others = torch.ones(rows, dtype=torch.bool)
        others[r_star] = False
        inputs.append((f"Z r*={r_star}", dyz, others.to(DEV)))
    for kind, d64, zero_rows in inputs:
        dy, d_st = pin(d64, dt)
        ref = R.norm_bwd_ref(x64, g64, torch.zeros(cols).double(), d_st, EPS, rms=True, dt=dt)
        outs = []
        for lean in leans:
            tuning("SL_RMSBWD_LEAN", lean)
            bx, dx = out_buf((rows, cols), dt)
            call("sl_rmsnorm_bwd", ptr(x), ptr(g), ptr(dy), ptr(dx), rows, cols, EPS, code(dt))
            assert intact(bx, dx), "write outside dx"
            ok(dx, ref.dx, ref.tol_dx, f"{kind} SL_RMSBWD_LEAN={lean} {rows} x {cols}")
            if zero_rows is not None:
                assert bool((dx[zero_rows] == 0).all()), f"{kind} lean={lean}: dx is not exactly zero in a row whose dy is zero"
            outs.append(dx)
        for lean, o in zip(leans[1:], outs[1:]):
            assert not bad(o, outs[0], bits=True), f"{kind}: SL_RMSBWD_LEAN={lean} and =2 promise the same bits"


# ------------------------------------------------------------------------------------------------------------------------------
# sl_colsum: the 16-byte kernel when cols, ld and the base pointer are 16-byte aligned, else the scalar kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("form", ["vector", "scalar_cols", "scalar_ld", "scalar_base"])
def test_colsum_integers_exact(dt, form):
    v = VEC[dt]
    # vector: 9 row blocks of 8 (70 rows) x 2 column blocks (33 chunks); scalar: 2 row blocks of 128 x 2 column blocks of 256
    rows, cols, ld, off = {"vector": (70, 33 * v, 34 * v, v), "scalar_cols": (130, 261, 272, v), "scalar_ld": (130, 2 * v, 3 * v + 1, v),
                           "scalar_base": (9, 2 * v, 3 * v, 1)}[form]
    x64 = R.ints((rows, cols), -4, 4, rows + cols)
    buf = torch.full((rows + 2, ld), BIG[dt], dtype=torch.float64)
    buf[:, ::2] *= -1.0
    buf[1:rows + 1, off:off + cols] = x64
    xd = buf.float().to(dt).to(DEV)
    x = xd[1:rows + 1, off:off + cols]
    assert x.stride(0) == ld
    o0 = R.ints((cols,), 1, 5, 3)
    bo, out = out_buf((cols,), F32, o0)
    call("sl_colsum", ptr(x), ld, ptr(out), rows, cols, code(dt))
    assert intact(bo, out), "write outside out"
    msg = bad(out, (o0 + x64.sum(0)).float())
    assert not msg, f"E {form} {rows} x {cols} ld {ld}: {msg}"


# ------------------------------------------------------------------------------------------------------------------------------
# 3. elementwise kernels
# ------------------------------------------------------------------------------------------------------------------------------
def elem_sizes(dt):
    return [VEC[dt], 256 * VEC[dt] + VEC[dt]]


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_gelu_bwd(dt):
    for n in elem_sizes(dt):
        dy64, pre64 = R.gauss((n,), n), R.gauss((n,), n + 1, 2.0)
        pre64[:8] = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 6.0, -6.0, 40.0, -40.0]).double()[:min(8, n)]
        (dy, dy64), (pre, pre64) = pin(dy64, dt), pin(pre64, dt)
        ref = R.gelu_bwd_ref(dy64, pre64, dt)
        bo, dx = out_buf((n,), dt)
        call("sl_gelu_bwd", ptr(dy), ptr(pre), ptr(dx), n, code(dt))
        assert intact(bo, dx) and bool(torch.isfinite(dx.float()).all())
        ok(dx, ref.dx, ref.tol_dx, f"G gelu_bwd n={n}")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_axpby_integers_exact(dt):
    sizes = elem_sizes(dt) + ([8192 * 256 * 4 + 4] if dt == F32 else [])          # fp32: one chunk past the grid cap - a second trip of the grid-stride loop
    for n in sizes:
        x64, y64 = R.ints((n,), -64, 64, n), R.ints((n,), -64, 64, n + 1)
        (x, x64) = pin(x64, dt)
        for a, b in ((1.0, 1.0), (-1.0, 2.0), (2.0, 0.0), (0.0, -1.0)):
            bo, y = out_buf((n,), dt, y64)
            call("sl_axpby", ptr(x), ptr(y), a, b, n, code(dt))
            assert intact(bo, y)
            msg = bad(y, (a * x64 + b * y64).float().to(dt))
            assert not msg, f"E axpby n={n} a={a} b={b}: {msg}"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_dropout_equals_the_host_formula(dt):
    p, seed = 0.25, 0xA5A5_1234_5678_9ABC
    scale = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    for n in elem_sizes(dt):
        (x, x64), (res, res64) = pin(R.gauss((n,), n), dt), pin(R.gauss((n,), n + 1), dt)
        keep = ops.dropout_keep_at(torch.arange(n), p, seed)
        d = torch.where(keep, x64.float() * scale, torch.zeros(()))
        for name, r, want in (("plain", None, d), ("residual", res, res64.float() + d)):
            bo, y = out_buf((n,), dt)
            call("sl_dropout", ptr(x), ptr(r), ptr(y), n, p, seed, code(dt))
            assert intact(bo, y)
            msg = bad(y, want.to(dt), bits=True)
            assert not msg, f"E dropout {name} n={n}: {msg}"
        bo, z = out_buf((n,), dt, x64)          # in place
        call("sl_dropout", ptr(z), 0, ptr(z), n, p, seed, code(dt))
        assert intact(bo, z) and not bad(z, d.to(dt), bits=True), "E dropout in place"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("M,F_", [(1, 16), (5, 16), (1, 48), (5, 48)])
def test_silu_mul_bwd(dt, M, F_):
    g64, up64, d64 = R.gauss((M, F_), M + F_, 3.0), R.gauss((M, F_), M + F_ + 1), R.gauss((M, F_), M + F_ + 2)
    g64[0, :8] = torch.tensor([20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0]).double()
    (gu, gu64), (d, d64) = pin(R.interleave(g64, up64), dt), pin(d64, dt)
    g64, up64 = R.deinterleave(gu64)
    ref = R.silu_mul_bwd_ref(g64, up64, d64, dt)
    bo, dgu = out_buf((M, 2 * F_), dt)
    call("sl_silu_mul_bwd", ptr(gu), ptr(d), ptr(dgu), M, F_, code(dt))
    assert intact(bo, dgu) and bool(torch.isfinite(dgu.float()).all())
    dgate, dup = R.deinterleave(dgu.cpu())
    ok(dgate, ref.dgate, ref.tol_dgate, f"G d gate {M} x {F_}")
    ok(dup, ref.dup, ref.tol_dup, f"G d up {M} x {F_}")
    # saturated gates: sg is exactly 1 (+104: exp(-104) underflows) or 0 (-89, -104: exp overflows) -> d u / d g, or 0
    du, dg_ = (d64 * up64).float().to(dt), (d64 * g64).float().to(dt)
    assert not bad(dgate[0, 6:7], du[0, 6:7]) and not bad(dup[0, 6:7], dg_[0, 6:7]), "gate +104: d gate = d u and d up = d g exactly"
    assert bool((dgate[0, [5, 7]] == 0).all()) and bool((dup[0, [5, 7]] == 0).all()), "gates -89 / -104: exact zeros"


def rope_tables(D, max_pos=64):
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2)))
    return pin(ang.cos(), F32), pin(ang.sin(), F32)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("n_tok,Dv", [(1, 2), (70, 4)])
def test_rope_inplace_against_the_rotation(dt, inverse, n_tok, Dv):
    """forward and inverse each against the fp64 rotation (a kernel with both signs flipped passes inverse(forward(x)) = x); the head behind
    n_rot keeps its bits; 70 tokens x 2 heads x 2 chunks = 280 work items: a second block"""
    D, heads, n_rot = Dv * VEC[dt], 3, 2
    (cos, cos64), (sin, sin64) = rope_tables(D)
    pos = (torch.arange(n_tok) * 11 + 5) % 64          # a single token sits at position 5: position 0 rotates by nothing
    pos[-1] = 0 if n_tok > 1 else 5
    x64 = R.rnd(R.gauss((n_tok, heads * D), n_tok + D), dt)
    ref = R.rope_ref(x64, pos, cos64, sin64, heads, n_rot, D, inverse, dt)
    bo, x = out_buf((n_tok, heads * D), dt, x64)
    pos_d = pos.to(DEV, torch.int32)
    call("sl_rope_inplace", ptr(x), ptr(pos_d), ptr(cos), ptr(sin), n_tok, heads, n_rot, D, int(inverse), code(dt))
    assert intact(bo, x)
    ok(x, ref.y, ref.tol + R.TINY, f"G rope inverse={inverse} {n_tok} x {heads} x {D}")
    assert not bad(x[:, n_rot * D:], x64[:, n_rot * D:].float().to(dt), bits=True), "a head behind n_rot changed"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. explicit softmax: 4 rows per block, a wave per row
# ------------------------------------------------------------------------------------------------------------------------------
POISON_S = 1e30


def softmax_check(name, dt, S64, dims, vis, scale, causal, var):
    """S64 (n_mats, rows, ld) stored scores with poison wherever nothing may be read; vis (n_mats, rows, ld) bool; dims (n_mats) or None.
    Runs the forward and, handed the reference P rounded to the storage type, the backward."""
    n_mats, rows, ld = S64.shape
    S, S64 = pin(S64, F32, POISON_S)
    ref = R.softmax_ref(S64.masked_fill(~vis, 0.0), scale, vis, dt)
    live = vis.any(-1, keepdim=True).expand(-1, -1, ld)          # rows the kernel writes (var: rows below the matrix size)
    bp, P = out_buf((n_mats, rows, ld), dt)
    md = None if dims is None else torch.tensor(dims, dtype=torch.int32, device=DEV)
    if var:
        call("sl_softmax_rows_var", ptr(S), ptr(P), n_mats, rows, ptr(md), ld, scale, int(causal), code(dt))
    else:
        call("sl_softmax_rows", ptr(S), ptr(P), n_mats, rows, var_cols(vis), ld, scale, int(causal), code(dt))
    assert intact(bp, P), "write outside P"
    Pc = P.cpu()
    ok(Pc[vis], ref.P[vis], ref.tol_P[vis], f"G P {name}")
    assert bool((Pc[live & ~vis] == 0).all()), f"{name}: a masked or pad column of P is not an exact zero"
    assert bool((Pc[~live] == FILL).all()), f"{name}: a row past the matrix was written"
    # backward on the reference P as stored
    Pst = ref.P.float().to(dt)
    Pin = torch.full((n_mats, rows, ld), BIG[dt], dtype=torch.float64)
    Pin[live] = Pst.double()[live]
    Pd, _ = pin(Pin, dt)
    dP64 = R.gauss((n_mats, rows, ld), rows + ld).float().double().masked_fill(~vis, POISON_S)
    dP, dP64 = pin(dP64, F32, POISON_S)
    rb = R.softmax_bwd_ref(Pst.double(), dP64.masked_fill(~vis, 0.0), scale, vis, dt)
    bs, dS = out_buf((n_mats, rows, ld), dt)
    if var:
        call("sl_softmax_bwd_var", ptr(Pd), ptr(dP), ptr(dS), n_mats, rows, ptr(md), ld, scale, code(dt))
    else:
        call("sl_softmax_bwd", ptr(Pd), ptr(dP), ptr(dS), n_mats * rows, var_cols(vis), ld, scale, code(dt))
    assert intact(bs, dS), "write outside dS"
    dSc = dS.cpu()
    ok(dSc[vis], rb.dS[vis], rb.tol_dS[vis] + R.TINY, f"G dS {name}")
    assert bool((dSc[live & ~vis] == 0).all()), f"{name}: a masked or pad column of dS is not an exact zero"
    assert bool((dSc[~live] == FILL).all()), f"{name}: a dS row past the matrix was written"
    return Pc


def var_cols(vis):
    return int(vis.any(0).any(0).sum())


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_rows_and_backward(dt, causal, cols):
    scale = 0.25
    ld = (cols + 3 + 7) // 8 * 8
    shapes = [(3, min(cols, 7)), (1, cols)] if causal else [(3, 7), (1, 5)]          # causal: rows < cols (a positive shift) and rows = cols
    for n_mats, rows in shapes:
        vis2 = R.causal_vis(rows, cols, causal)
        vis = torch.zeros(n_mats, rows, ld, dtype=torch.bool)
        vis[:, :, :cols] = vis2
        S64 = R.gauss((n_mats, rows, ld), 7 * cols + rows, 4.0).masked_fill(~vis, POISON_S)
        n_vis = vis2.sum(-1)
        S64[0, 0, int(n_vis[0]) - 1] = float(S64[0, 0, :int(n_vis[0])].max()) + 200.0 / scale          # one score 200 / scale above the rest
        if rows > 1:
            S64[0, 1, :int(n_vis[1])] = 1.5                                                               # all-equal scores
        Pc = softmax_check(f"{n_mats} x {rows} x {cols} ld {ld} causal={causal}", dt, S64, None, vis, scale, causal, False)
        want = torch.zeros(ld)
        want[int(n_vis[0]) - 1] = 1.0
        assert torch.equal(Pc[0, 0].float(), want), "a score 200 / scale above the rest: P must be exactly 1 and 0"
        if rows > 1 and int(n_vis[1]) == 64:
            assert bool((Pc[0, 1, :64].float() == 2.0 ** -6).all()), "64 equal scores: P must be exactly 2^-6"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_softmax_ragged_forms(dt, causal):
    """sl_softmax_rows_var / _bwd_var: matrices of 1, rows_per_mat and 37 rows at a pitch of 40 x 48; rows past a matrix keep the sentinel"""
    rpm, ld, dims, scale = 40, 48, [1, 40, 37], 0.25
    vis = torch.zeros(len(dims), rpm, ld, dtype=torch.bool)
    for i, n in enumerate(dims):
        vis[i, :n, :n] = R.causal_vis(n, n, causal)
    S64 = R.gauss((len(dims), rpm, ld), 77, 4.0).masked_fill(~vis, POISON_S)
    softmax_check(f"var {dims} causal={causal}", dt, S64, dims, vis, scale, causal, True)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. losses: a block of 1 024 threads per row of logits (V = 1 ... 4 100: fewer elements than threads, one each, a second trip)
# ------------------------------------------------------------------------------------------------------------------------------
ROWS = 7


def loss_rows(V, seed):
    """logits with the special rows: row 5 has one logit 1e4 above the rest at its label, row 6 is shifted by +1 000"""
    s, t, lab = R.loss_inputs(ROWS, V, seed)
    s[6] += 1000.0
    t[6] += 1000.0
    s[5, lab[5]] = float(s[5].max()) + 1e4
    return s.float().double(), t.float().double(), lab


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("V", R.LOSS_V)
def test_ce_loss(dt, accumulate, V):
    """labels in [0, V) only: the header's contract (the kernel reads logits[label])"""
    coef = 0.25
    s64, _, lab = loss_rows(V, V)
    s, s64 = pin(s64, F32)
    d0 = R.rnd(R.gauss((ROWS, V), V + 5), dt) if accumulate else None
    cf = torch.tensor([[coef, coef, 0.0, 0.0]] * ROWS).double()
    ref = R.kd_logit_ref(s64, None, lab, cf, torch.zeros(ROWS, dtype=torch.int64), 1, dt, loss0=torch.tensor([[3.0, 0.0]]).double())
    bl, loss = out_buf((1,), F32, torch.tensor([3.0]))
    bd, dl = out_buf((ROWS, V), dt, d0)
    lab_d = lab.to(DEV, torch.int32)          # (named: a temporary's memory would be handed to the next allocation)
    call("sl_ce_loss", ptr(s), ptr(lab_d), ROWS, V, coef, ptr(loss), ptr(dl), accumulate, code(dt))
    assert intact(bl, loss) and intact(bd, dl)
    ok(loss, ref.losses[0, :1], ref.tol_losses[0, :1], f"G ce loss V={V}")
    want = ref.ds + (d0 if accumulate else 0.0)
    ok(dl, want, 2 * U[dt] * want.abs() + ref.e_ds + E24 * want.abs() + R.SUBN[dt] + R.TINY, f"G ce dlogits V={V} accumulate={accumulate}")
    if not accumulate:
        assert float(dl[5, lab[5]]) == 0.0, "a label 1e4 above the rest: its gradient must be exactly 0"
        if V == 1:
            assert float(loss) == 3.0 and bool((dl == 0).all()), "V = 1: loss contribution 0 and gradient exactly 0"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("V", R.LOSS_V)
def test_soft_ce_loss(dt, accumulate, V):
    coef = 0.5
    s64, t64, lab = loss_rows(V, 100 + V)
    (s, s64), (t, t64) = pin(s64, F32), pin(t64, F32)
    d0 = R.rnd(R.gauss((ROWS, V), V + 6), dt) if accumulate else None
    cf = torch.tensor([[0.0, 0.0, coef, coef]] * ROWS).double()
    ref = R.kd_logit_ref(s64, t64, torch.full((ROWS,), -1), cf, torch.zeros(ROWS, dtype=torch.int64), 1, dt, loss0=torch.tensor([[0.0, 3.0]]).double())
    bl, loss = out_buf((1,), F32, torch.tensor([3.0]))
    bd, dl = out_buf((ROWS, V), dt, d0)
    call("sl_soft_ce_loss", ptr(s), ptr(t), ROWS, V, coef, ptr(loss), ptr(dl), accumulate, code(dt))
    assert intact(bl, loss) and intact(bd, dl)
    ok(loss, ref.losses[0, 1:], ref.tol_losses[0, 1:], f"G soft-ce loss V={V}")
    want = ref.ds + (d0 if accumulate else 0.0)
    ok(dl, want, 2 * U[dt] * want.abs() + ref.e_ds + E24 * want.abs() + R.TINY, f"G soft-ce dstudent V={V} accumulate={accumulate}")
    if V == 1 and not accumulate:
        assert float(loss) == 3.0 and bool((dl == 0).all())


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("teacher", [False, True], ids=["ce_only", "teacher"])
@pytest.mark.parametrize("V", R.LOSS_V)
def test_kd_logit_losses(dt, teacher, V):
    """V % 4 == 0: the 16-byte path, else the scalar one.  Rows 0, 1, 5 -> slot 0, rows 2, 3, 4, 6 -> slot 2, slot 1 has none; row 3 has no
    label; row 4 has both soft coefficients 0 and a poisoned teacher row; losses (3, 5) with columns 2 - 4 at the sentinel"""
    s64, t64, lab = loss_rows(V, 200 + V)
    lab[3] = -1
    cf = torch.tensor([[0.5, 0.25, 0.125, 0.5], [1.0, 0.5, 0.25, 0.25]] * 4)[:ROWS].double()
    cf[4, 2:] = 0.0
    slot = torch.tensor([0, 0, 2, 2, 2, 0, 2])
    t64[4] = POISON_S * (1 - 2 * (torch.arange(V) % 2))
    (s, s64), (t, t64) = pin(s64, F32), pin(t64, F32, POISON_S)
    l0 = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]).double()
    ref = R.kd_logit_ref(s64, t64 if teacher else None, lab, cf, slot, 3, dt, loss0=l0)
    bl, losses = out_buf((3, 5), F32)
    losses[:, :2] = l0.float().to(DEV)
    bd, ds = out_buf((ROWS, V), dt)
    lab_d, cf_d, slot_d = lab.to(DEV, torch.int32), cf.float().to(DEV), slot.to(DEV, torch.int32)
    call("sl_kd_logit_losses", ptr(s), ptr(t) if teacher else 0, ptr(lab_d), ptr(cf_d), ptr(slot_d),
         ROWS, V, ptr(losses), 5, ptr(ds), code(dt))
    assert intact(bl, losses) and intact(bd, ds)
    assert bool((losses[:, 2:] == FILL).all()), "losses columns 2 - 4 written"
    assert torch.equal(losses[1, :2].cpu().double(), l0[1]), "the slot without rows changed"
    ok(losses[:, :2], ref.losses, ref.tol_losses, f"G kd losses V={V}")
    ok(ds, ref.ds, ref.tol_ds, f"G kd dstudent V={V}")
    if not teacher:
        assert bool((ds[3] == 0).all()), "a row without label and teacher: gradient exactly 0"
        assert torch.equal(losses[:, 1].cpu().double(), l0[:, 1]), "no teacher: the soft-ce column must not change"
        assert float(ds[5, lab[5]]) == 0.0


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("with_da", [False, True], ids=["loss_only", "da"])
@pytest.mark.parametrize("Hv", [1, 65])
def test_kd_mse_rows(dt, with_da, Hv):
    H, rows = Hv * VEC[dt], 6
    (a, a64), (b, b64) = pin(R.gauss((rows, H), H), dt), pin(R.gauss((rows, H), H + 1), dt)
    cf = torch.tensor([[0.5, 0.25], [0.25, 2.0]] * 3).double()
    slot = torch.tensor([0, 0, 2, 2, 2, 0])
    l0 = torch.tensor([1.0, 2.0, 3.0]).double()
    ref = R.kd_mse_rows_ref(a64, b64, cf, slot, 3, dt, loss0=l0)
    bl, losses = out_buf((3, 5), F32)
    losses[:, 2] = l0.float().to(DEV)
    bd, da = out_buf((rows, H), dt)
    cf_d, slot_d = cf.float().to(DEV), slot.to(DEV, torch.int32)
    call("sl_kd_mse_rows", ptr(a), ptr(b), ptr(cf_d), ptr(slot_d), rows, H, ptr(losses), 5, 2, ptr(da) if with_da else 0, code(dt))
    assert intact(bl, losses) and intact(bd, da)
    assert bool((losses[:, [0, 1, 3, 4]] == FILL).all()) and float(losses[1, 2]) == 2.0
    ok(losses[:, 2], ref.losses, ref.tol_losses, f"G kd_mse losses H={H}")
    if with_da:
        ok(da, ref.da, ref.tol_da, f"G kd_mse da H={H}")
    else:
        assert bool((da == FILL).all())


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 257, 262144 + 1])
def test_mse_loss(dt, accumulate, n):
    """262 145 elements: above the cap of 1 024 blocks x 256 threads"""
    coef = 0.5
    (a, a64), (b, b64) = pin(R.gauss((n,), n % 1000), dt), pin(R.gauss((n,), n % 1000 + 1), dt)
    d0 = R.rnd(R.gauss((n,), 5), dt) if accumulate else None
    ref = R.mse_ref(a64, b64, coef, dt, da0=d0, loss0=3.0)
    bl, loss = out_buf((1,), F32, torch.tensor([3.0]))
    bd, da = out_buf((n,), dt, d0)
    call("sl_mse_loss", ptr(a), ptr(b), n, coef, ptr(loss), ptr(da), accumulate, code(dt))
    assert intact(bl, loss) and intact(bd, da)
    ok(loss, torch.tensor([ref.loss], dtype=torch.float64), torch.tensor([ref.tol_loss], dtype=torch.float64), f"G mse loss n={n}")
    ok(da, ref.da, ref.tol_da, f"G mse da n={n} accumulate={accumulate}")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. front-end backward
# ------------------------------------------------------------------------------------------------------------------------------
def pool_shapes(P, kernel, stride):
    return (P - 1) * stride + kernel + 2          # destination rows: two behind the last window


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("kernel,stride", R.POOL_KS)
@pytest.mark.parametrize("Cv", [1, 3])
def test_avgpool_bwd_and_col2im(dt, kernel, stride, Cv):
    """overlap (8, 4), (10, 5), (3, 2); gaps that must be exact zeros (2, 3); abutting windows (4, 4).  Integer sources: the window sums are
    exact, so a power-of-two kernel is checked with torch.equal and the others to the two roundings of 1 / kernel and the multiply."""
    Cc, P = Cv * VEC[dt], 6
    T = pool_shapes(P, kernel, stride)
    dy, dy64 = pin(R.ints((P, Cc), -8, 8, kernel + Cc), dt)
    ref = R.avgpool_bwd_ref(dy64, T, kernel, stride, dt)
    bo, dx = out_buf((T, Cc), dt)
    call("sl_avgpool_bwd", ptr(dy), ptr(dx), T, Cc, kernel, stride, P, code(dt))
    assert intact(bo, dx)
    name = f"avgpool_bwd k={kernel} s={stride} C={Cc}"
    if kernel & (kernel - 1) == 0:
        msg = bad(dx, ref.dx.float().to(dt))
        assert not msg, f"E {name}: {msg}"
    ok(dx, ref.dx, ref.tol_dx, f"G {name}")
    covered = R.avgpool_bwd_ref(torch.ones(P, Cc).double(), T, kernel, stride).dx > 0
    assert bool((dx.cpu()[~covered] == 0).all()) and bool((~covered[-2:]).all()), f"{name}: rows no window covers must be exact zeros"
    dcol, dcol64 = pin(R.ints((P, kernel * Cc), -8, 8, kernel + Cc + 1), dt)
    bo, dxc = out_buf((T, Cc), dt)
    call("sl_col2im", ptr(dcol), ptr(dxc), T, P, Cc, kernel, stride, code(dt))
    assert intact(bo, dxc)
    msg = bad(dxc, R.col2im_ref(dcol64, T, Cc, kernel, stride).float().to(dt))
    assert not msg, f"E col2im k={kernel} s={stride} C={Cc}: {msg}"


def batch_layout(P_list, kernel, stride):
    """source rows with a poisoned row between utterances, destination rows with two sentinel rows between them"""
    src_off, dst_off, T_list, so, do = [], [], [], 1, 2
    for P in P_list:
        T = pool_shapes(P, kernel, stride)
        src_off.append(so); dst_off.append(do); T_list.append(T)
        so += P + 1
        do += T + 2
    return src_off, dst_off, T_list, so, do


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("kernel,stride", R.POOL_KS)
def test_avgpool_bwd_and_col2im_batch(dt, kernel, stride):
    """utterances of 1, 40 and 3 windows: max_T far above the shortest; non-contiguous destinations whose in-between rows keep the sentinel"""
    Cc, P_list = 3 * VEC[dt], [1, 40, 3]
    src_off, dst_off, T_list, n_src, n_dst = batch_layout(P_list, kernel, stride)
    for which, width in (("avgpool", 1), ("col2im", kernel)):
        src64 = torch.full((n_src, width * Cc), BIG[dt], dtype=torch.float64)
        for u, P in enumerate(P_list):
            src64[src_off[u]:src_off[u] + P] = R.ints((P, width * Cc), -8, 8, 10 * u + kernel)
        src, src64 = pin(src64, dt)
        bo, dst = out_buf((n_dst, Cc), dt)
        desc = L.h2d([[P_list[u], T_list[u], src_off[u], dst_off[u]] for u in range(len(P_list))], torch.int64, DEV)
        if which == "avgpool":
            call("sl_avgpool_bwd_batch", ptr(src), ptr(dst), desc.data_ptr(), len(P_list), max(T_list), Cc, kernel, stride, code(dt))
        else:
            call("sl_col2im_batch", ptr(src), ptr(dst), desc.data_ptr(), len(P_list), max(T_list), Cc, kernel, stride, code(dt))
        assert intact(bo, dst)
        written = torch.zeros(n_dst, dtype=torch.bool)
        for u, P in enumerate(P_list):
            rows = slice(dst_off[u], dst_off[u] + T_list[u])
            written[rows] = True
            s_u = src64[src_off[u]:src_off[u] + P]
            if which == "avgpool":
                ref = R.avgpool_bwd_ref(s_u, T_list[u], kernel, stride, dt)
                ok(dst[rows], ref.dx, ref.tol_dx, f"{which}_batch utterance {u} k={kernel} s={stride}")
                if kernel & (kernel - 1) == 0:
                    assert not bad(dst[rows], ref.dx.float().to(dt))
            else:
                msg = bad(dst[rows], R.col2im_ref(s_u, T_list[u], Cc, kernel, stride).float().to(dt))
                assert not msg, f"E col2im_batch utterance {u}: {msg}"
        assert bool((dst.cpu()[~written] == FILL).all()), f"{which}_batch: a row between two utterances was written"


def test_col2im_batch_above_its_block_cap():
    """bf16, Cc = 1 024, Lin = 2 050: 262 400 work items against 1 024 blocks x 256 threads - the grid-stride loop's second trip"""
    dt, Cc, k, s, Lin = BF16, 1024, 3, 2, 2050
    Lout = (Lin - k) // s + 1
    dcol, dcol64 = pin(R.ints((Lout, k * Cc), -8, 8, 5), dt)
    bo, dx = out_buf((Lin, Cc), dt)
    desc = L.h2d([[Lout, Lin, 0, 0]], torch.int64, DEV)
    call("sl_col2im_batch", ptr(dcol), ptr(dx), desc.data_ptr(), 1, Lin, Cc, k, s, code(dt))
    assert intact(bo, dx)
    want = torch.zeros(Lin, Cc, dtype=torch.float64)
    d3 = dcol64.view(Lout, k, Cc)
    for j in range(k):
        want[j:j + s * Lout:s][:Lout] += d3[:, j]
    msg = bad(dx, want.float().to(dt))
    assert not msg, f"E col2im_batch above the cap: {msg}"


def conv0_buffers(init):
    bufs = [out_buf(tuple(i.shape), F32, i) for i in init]
    return bufs, [v for _, v in bufs]


def conv0_check(got, ref, bufs, what):
    for (b_, v_) in bufs:
        assert intact(b_, v_), f"{what}: write outside a gradient buffer"
    for name, g_ in zip(("dw", "dbias", "dgamma", "dbeta"), got):
        ok(g_, getattr(ref, name), getattr(ref, "tol_" + name), f"{what} {name}")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("C_", [64, 128, 256, 512])
@pytest.mark.parametrize("Lo", R.CONV0_L)
def test_conv0_bwd(dt, C_, Lo):
    """sl_hubert_conv0_bwd: strips of 24 time steps, a wave each; samples 5 t + j of a strip come from two 64-sample registers (index 64 is
    reached by step 11 tap 9 / step 12 tap 4).  G on Gaussian dy, Z with dy at one time step: 0, 11, 12 (the register switch), 23, 24 (the
    strip boundary), L - 1.  All four gradients accumulate onto non-zero integers."""
    r_extra = 0 if Lo % 2 else 4
    wave64, w64, bias64, gamma64, beta64, dy64, init = R.conv0_inputs(C_, Lo, r_extra, 100 * Lo + C_, dt)
    wave, wave64 = pin(wave64, F32)
    params = [pin(p, F32) for p in (w64, bias64, gamma64, beta64)]
    dev = [p[0] for p in params]
    w64, bias64, gamma64, beta64 = [p[1] for p in params]
    probes = [("G", dy64)]
    for t_star in sorted({t for t in (0, 11, 12, 23, 24, Lo - 1) if t < Lo}):
        dz = torch.zeros(Lo, C_, dtype=torch.float64)
        dz[t_star] = dy64[t_star]
        probes.append((f"Z t*={t_star}", dz))
    for kind, d64 in probes:
        dy, d_st = pin(d64, dt)
        ref = R.conv0_bwd_ref(wave64, w64, bias64, gamma64, beta64, d_st, EPS, dt, init)
        bufs, outs = conv0_buffers(init)
        call("sl_hubert_conv0_bwd", ptr(wave), wave.numel(), *[ptr(p) for p in dev], ptr(dy), C_, 10, 5, EPS, *[ptr(o) for o in outs], code(dt))
        conv0_check(outs, ref, bufs, f"{kind} conv0_bwd C={C_} L={Lo}")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("C_", [64, 128, 256, 512])
def test_conv0_bwd_batch(dt, fold, C_, tuning):
    """three utterances of 1, 25 and 97 frames in one launch against the sum of the per-utterance references; SL_CONV0_FOLD = 1 (the block's
    four waves fold through LDS, one flush) and 0 (a flush per wave)"""
    tuning("SL_CONV0_FOLD", fold)
    Ls = [1, 25, 97]
    _, w64, bias64, gamma64, beta64, _, init = R.conv0_inputs(C_, 1, 0, 900 + C_, dt)
    params = [pin(p, F32) for p in (w64, bias64, gamma64, beta64)]
    dev = [p[0] for p in params]
    w64, bias64, gamma64, beta64 = [p[1] for p in params]
    waves, dys, row_off = [], [], [0]
    for u, Lo in enumerate(Ls):
        wv, _, _, _, _, dyu, _ = R.conv0_inputs(C_, Lo, 4 * (u % 2), 950 + u, dt)
        waves.append(wv.float())
        dys.append(dyu)
        row_off.append(row_off[-1] + Lo)
    dy, dy64 = pin(torch.cat(dys), dt)
    zero = [torch.zeros_like(i) for i in init]
    tot = [i.clone() for i in init]
    tol = [E24 * i.abs() for i in init]
    for u, Lo in enumerate(Ls):
        r = R.conv0_bwd_ref(waves[u].double(), w64, bias64, gamma64, beta64, dy64[row_off[u]:row_off[u + 1]], EPS, dt, zero)
        for i, name in enumerate(("dw", "dbias", "dgamma", "dbeta")):
            tot[i] += getattr(r, name)
            tol[i] += getattr(r, "tol_" + name) + E24 * tot[i].abs()
    bufs, outs = conv0_buffers(init)
    ops.hubert_conv0_bwd_batch([w_.to(DEV) for w_ in waves], *dev, dy, row_off, *outs)
    for (b_, v_) in bufs:
        assert intact(b_, v_)
    for i, name in enumerate(("dw", "dbias", "dgamma", "dbeta")):
        ok(outs[i], tot[i], tol[i], f"G conv0_bwd_batch fold={fold} C={C_} {name}")


# ------------------------------------------------------------------------------------------------------------------------------
# 7. optimizer and weight norm
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 1000])
def test_adamw_step_per_element(step):
    """one launch over tensors of 1 ... 4 097 elements (a block covers 4 096) and a view 4 bytes off a 16-byte boundary; compute-dtype copies
    in bf16, fp32 and none; the first four elements of every tensor have g = 0 and v = 0 (the denominator is eps alone)"""
    h = R.ADAMW_HYPER
    sc = R.adamw_scalars(step=step, **h)
    sizes = R.ADAMW_SIZES + [777]
    kinds = [BF16, F32, None, BF16, F32, None, BF16, BF16]
    table = (L.AdamWTensor * len(sizes))()
    first, total, keep, state = [], 0, [], []
    for i, n in enumerate(sizes):
        off = GUARD + 1 if n == 777 else GUARD
        vals = [R.gauss((n,), 10 * i + 1, 0.05), R.gauss((n,), 10 * i + 2, 0.01), R.gauss((n,), 10 * i + 3, 0.01), R.gauss((n,), 10 * i + 4, 1e-4).abs()]
        vals[1][:4], vals[3][:4] = 0.0, 0.0
        bufs = [out_buf((n,), F32, v_, off=off) for v_ in vals]
        st = [v_.double().cpu() for _, v_ in bufs]
        dst = out_buf((n,), kinds[i], off=GUARD + (3 if n == 777 else 0)) if kinds[i] is not None else None
        rec = table[i]
        rec.p, rec.g, rec.m, rec.v, rec.n = [ptr(v_) for _, v_ in bufs] + [n]
        if dst is not None:
            rec.dst, rec.dst_dtype = ptr(dst[1]), code(kinds[i])
        first.append(total)
        total += int(L.lib().sl_adamw_blocks(n))
        keep.append((bufs, dst))
        state.append(st)
    t_dev = L.h2d(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8), torch.uint8, DEV)
    f_dev = L.h2d(torch.tensor(first, dtype=torch.int64), torch.int64, DEV)
    call("sl_adamw_step", t_dev.data_ptr(), f_dev.data_ptr(), len(sizes), total, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], step)
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        bufs, dst = keep[i]
        p0, g0, m0, v0 = state[i]
        ref = R.adamw_ref(p0, g0, m0, v0, sc)
        for b_, v_ in bufs:
            assert intact(b_, v_), f"tensor {i} ({n}): write outside p / g / m / v"
        assert torch.equal(bufs[1][1].cpu().double(), g0), "the gradient changed"
        ok(bufs[0][1], ref.p, ref.tol_p, f"G adamw p, tensor of {n}, step {step}")
        ok(bufs[2][1], ref.m, ref.tol_m, f"G adamw m, tensor of {n}")
        ok(bufs[3][1], ref.v, ref.tol_v, f"G adamw v, tensor of {n}")
        if dst is not None:
            assert intact(*dst), f"tensor {i} ({n}): write outside the compute-dtype copy"
            assert not bad(dst[1], bufs[0][1].to(kinds[i]), bits=True), f"tensor of {n}: the copy is not the RNE cast of the master just written"


@pytest.mark.parametrize("H,Hg,k", R.WN_SHAPES)
def test_weight_norm_bwd_per_element(H, Hg, k):
    """H below and above the 64-block grid (65: an uneven h0..h1 split), k = 7 and the maximum 256"""
    (dWk, dW64), (v, v64), (g, g64) = pin(R.gauss((H, k, Hg), H + k), F32), pin(R.gauss((H, Hg, k), H + k + 1), F32), pin(1 + R.gauss((k,), H + k + 2, 0.1), F32)
    ref = R.weight_norm_bwd_ref(dW64.permute(0, 2, 1), v64, g64)
    outs = []
    for _ in range(2):
        bg, dg = out_buf((k,), F32)
        bv, dv = out_buf((H, Hg, k), F32)
        bw, ws = out_buf((int(L.lib().sl_weight_norm_bwd_workspace_bytes(k)) // 4,), F32)
        call("sl_weight_norm_bwd", ptr(dWk), ptr(v), ptr(g), ptr(dg), ptr(dv), ptr(ws), H, Hg, k)
        assert intact(bg, dg) and intact(bv, dv) and intact(bw, ws)
        ok(dg, ref.dg, ref.tol_dg, f"G weight_norm dg {(H, Hg, k)}")
        ok(dv, ref.dv, ref.tol_dv, f"G weight_norm dv {(H, Hg, k)}")
        outs.append((dg, dv))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "fixed summation order: two calls must agree"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,ld_out", [(1, 1, 1), (65, 63, 72), (64, 130, 64), (257, 64, 257)])
def test_transpose_pad_guarded(dt, rows, cols, ld_out):
    """tests/test_train_kernels_gpu.py::test_transpose_pad with guard bands: y rows have a pitch wider than ld_out whose tail keeps the sentinel"""
    v = VEC[dt]
    ldx, ldy = ceil_div(cols, v) * v + v, ceil_div(ld_out, v) * v + v
    xb, x64 = pin(R.gauss((rows, ldx), rows + cols), dt)
    bo, y = out_buf((cols, ldy), dt)
    call("sl_transpose_pad", ptr(xb), ldx, ptr(y), ldy, rows, cols, ld_out, code(dt))
    assert intact(bo, y)
    assert not bad(y[:, :rows], x64[:, :cols].t().float().to(dt), bits=True), "y[:, :rows] is not x^T"
    assert bool((y[:, rows:ld_out] == 0).all()) and bool((y[:, ld_out:] == FILL).all())
