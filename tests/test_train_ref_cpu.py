"""CPU: the references and per-element bounds of tests/train_ops_ref.py are right, not vacuous and not too tight.

(a) every reference equals torch's fp64 autograd (torch.optim.AdamW in fp64 for the optimizer) of the same operation to 1e-12;
(b) the reference with one defect planted in it - a reduction term dropped, the last row or the last 16-byte chunk left at the output
    sentinel, a mask limit off by one - leaves its own bound at the affected elements, on every Gaussian case of the GPU file (a dropped
    term only where one term of the reduction is still >= 16 x the accumulation term: rows of at most DROP_TERM_MAX_COLS elements;
    wider rows are covered by the exact-zero probes and the sentinel defects);
(c) the `*_sim` restatements - fp32 torch in the kernels' operation order, rounded to the storage type - stay inside every bound, so the
    references alone do not trip their own tests.  No number here is measured.
"""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R

BF16, F32, F16 = R.BF16, R.F32, R.F16
DTS = [F32, BF16]
EPS = 1e-5


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def worst(got, ref, tol, where=None):
    r = (got - ref).abs() / tol
    if where is not None:
        r = r[where]
    return float(r.max())


def outside(got, ref, tol):
    """elements that leave the bound"""
    return ~((got - ref).abs() <= tol)


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the references are the operations
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rms,gelu", [(False, False), (False, True), (True, False)])
def test_norm_reference_equals_autograd(rms, gelu):
    x, g, b, dy = R.norm_inputs(7, 24, F32, 11, rms)
    xr, gr, br = x.clone().requires_grad_(), g.clone().requires_grad_(), b.clone().requires_grad_()
    eps = R.f32(EPS)
    y = gr * (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps)) if rms else F.layer_norm(xr, (24,), gr, br, eps)
    (F.gelu(y) if gelu else y).backward(dy)
    r = R.norm_bwd_ref(x, g, b, dy, EPS, rms=rms, gelu=gelu, dgamma0=torch.ones(24).double())
    assert close(r.dx, xr.grad) and close(r.dgamma - 1.0, gr.grad)
    if not rms:
        assert close(r.dbeta, br.grad)


def test_elementwise_references_equal_autograd():
    dy, pre = R.gauss((5, 16), 1), R.gauss((5, 16), 2, 2.0)
    pr = pre.clone().requires_grad_()
    F.gelu(pr).backward(dy)
    assert close(R.gelu_bwd_ref(dy, pre, F32).dx, pr.grad)
    g, up, d = R.gauss((5, 32), 3, 3.0), R.gauss((5, 32), 4), R.gauss((5, 32), 5)
    gr, ur = g.clone().requires_grad_(), up.clone().requires_grad_()
    (F.silu(gr) * ur).backward(d)
    r = R.silu_mul_bwd_ref(g, up, d, F32)
    assert close(r.dgate, gr.grad) and close(r.dup, ur.grad)
    gu = R.interleave(g, up)
    assert torch.equal(R.deinterleave(gu)[0], g) and torch.equal(R.deinterleave(gu)[1], up) and torch.equal(gu[:, 16:32], up[:, :16])
    # RoPE: hf apply_rotary_pos_emb (x cos + rotate_half(x) sin), and the inverse is its transpose = the backward
    D, heads, n_rot, n = 16, 3, 2, 6
    x = R.gauss((n, heads * D), 6)
    ang = torch.arange(40, dtype=torch.float64)[:, None] * (100.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2)))
    cos, sin = ang.cos(), ang.sin()
    pos = torch.tensor([0, 3, 39, 7, 7, 1])
    xr = x.clone().requires_grad_()
    xv = xr.view(n, heads, D)
    c2, s2 = torch.cat([cos[pos], cos[pos]], -1)[:, None], torch.cat([sin[pos], sin[pos]], -1)[:, None]
    rot = torch.cat([-xv[..., D // 2:], xv[..., :D // 2]], -1)
    y = torch.cat([(xv * c2 + rot * s2)[:, :n_rot], xv[:, n_rot:]], 1).reshape(n, heads * D)
    assert close(R.rope_ref(x, pos, cos, sin, heads, n_rot, D, False, F32).y, y.detach())
    w = R.gauss((n, heads * D), 7)
    y.backward(w)
    assert close(R.rope_ref(w, pos, cos, sin, heads, n_rot, D, True, F32).y, xr.grad)


@pytest.mark.parametrize("causal", [False, True])
def test_softmax_references_equal_autograd(causal):
    rows, cols, scale = 5, 9, 0.25
    S, dP = R.gauss((2, rows, cols), 1, 3.0), R.gauss((2, rows, cols), 2)
    vis = R.causal_vis(rows, cols, causal)
    Sr = S.clone().requires_grad_()
    P = torch.softmax((Sr * scale).masked_fill(~vis, float("-inf")), -1)
    P.backward(dP)
    r = R.softmax_ref(S, scale, vis, F32)
    assert close(r.P, P.detach())
    assert close(R.softmax_bwd_ref(r.P, dP, scale, vis, F32).dS, Sr.grad)


@pytest.mark.parametrize("teacher", [False, True])
def test_loss_references_equal_autograd(teacher):
    rows, V, ns = 6, 13, 3
    s, t, lab = R.loss_inputs(rows, V, 3)
    lab[4] = -1
    coef = R.gauss((rows, 4), 9).abs().float().double()
    coef[5, 2:] = 0.0
    slot = torch.tensor([0, 0, 2, 2, 2, 0])
    sr = s.clone().requires_grad_()
    lsm = F.log_softmax(sr, -1)
    ok = lab >= 0
    ce = torch.where(ok, -lsm[torch.arange(rows), lab.clamp(min=0)], torch.zeros(()).double())
    so = -(F.softmax(t, -1) * lsm).sum(-1) if teacher else torch.zeros(rows).double()
    ((coef[:, 1] * ce).sum() + (coef[:, 3] * so).sum()).backward()
    r = R.kd_logit_ref(s, t if teacher else None, lab, coef, slot, ns, F32)
    assert close(r.ds, sr.grad)
    want = torch.zeros(ns, 2).double()
    want[:, 0].index_add_(0, slot, (coef[:, 0] * ce).detach())
    want[:, 1].index_add_(0, slot, (coef[:, 2] * so).detach())
    assert close(r.losses, want)
    a, b = R.gauss((4, 8), 5), R.gauss((4, 8), 6)
    ar = a.clone().requires_grad_()
    m = F.mse_loss(ar, b) * 0.5
    m.backward()
    rm = R.mse_ref(a, b, 0.5, F32)
    assert close(rm.loss, m.detach()) and close(rm.da, ar.grad)
    mc = torch.tensor([[0.5, 0.25]] * 4).double()
    rk = R.kd_mse_rows_ref(a, b, mc, torch.tensor([1, 1, 0, 1]), 2, F32)
    ar2 = a.clone().requires_grad_()
    (0.125 * (ar2 - b).pow(2).sum()).backward()
    assert close(rk.da, ar2.grad) and close(rk.losses, torch.stack([0.5 * (a - b)[2].pow(2).sum(), 0.5 * (a - b)[[0, 1, 3]].pow(2).sum()]))


@pytest.mark.parametrize("kernel,stride", R.POOL_KS)
def test_front_end_references_equal_autograd(kernel, stride):
    H, T = 4, 23
    P = (T - kernel) // stride + 1
    dy = R.gauss((P, H), 1)
    xr = torch.zeros(1, H, T, dtype=torch.float64, requires_grad=True)
    F.avg_pool1d(xr, kernel, stride)[0].T.backward(dy)
    assert close(R.avgpool_bwd_ref(dy, T, kernel, stride).dx, xr.grad[0].T)
    Cc, C2 = 4, 3
    dcol_w = R.gauss((C2, kernel * Cc), 2)
    dyc = R.gauss((P, C2), 3)
    xr2 = torch.zeros(1, Cc, T, dtype=torch.float64, requires_grad=True)
    F.conv1d(xr2, dcol_w.view(C2, kernel, Cc).permute(0, 2, 1).contiguous(), stride=stride)[0].T.backward(dyc)
    assert close(R.col2im_ref(dyc @ dcol_w, T, Cc, kernel, stride), xr2.grad[0].T)


def test_conv0_reference_equals_autograd():
    C_, L = 64, 25
    wave, w, bias, gamma, beta, dy, init = R.conv0_inputs(C_, L, 4, 5, F32)
    ps = [p.clone().requires_grad_() for p in (w, bias, gamma, beta)]
    y = F.conv1d(wave[None, None], ps[0][:, None], ps[1], stride=5)[0].T
    assert y.shape[0] == L
    F.gelu(F.layer_norm(y, (C_,), ps[2], ps[3], R.f32(EPS))).backward(dy)
    r = R.conv0_bwd_ref(wave, w, bias, gamma, beta, dy, EPS, F32, init)
    for got, i0, p in ((r.dw, init[0], ps[0]), (r.dbias, init[1], ps[1]), (r.dgamma, init[2], ps[2]), (r.dbeta, init[3], ps[3])):
        assert close(got - i0, p.grad, 1e-11)


@pytest.mark.parametrize("step", [1, 1000])
def test_adamw_reference_equals_torch_optim_adamw(step):
    h = R.ADAMW_HYPER
    p0, g, m0, v0 = R.gauss((50,), 1, 0.05), R.gauss((50,), 2, 0.01), R.gauss((50,), 3, 0.01), R.gauss((50,), 4, 1e-4).abs()
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"])
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    p.grad = g.clone()
    opt.step()
    r = R.adamw_ref(p0, g, m0, v0, R.adamw_scalars(step=step, fp32=False, **h))
    assert close(r.p, p.detach()) and close(r.m, opt.state[p]["exp_avg"]) and close(r.v, opt.state[p]["exp_avg_sq"])


@pytest.mark.parametrize("H,Hg,k", R.WN_SHAPES)
def test_weight_norm_reference_equals_autograd(H, Hg, k):
    v, g, dW = R.gauss((H, Hg, k), 1).requires_grad_(), (1 + R.gauss((k,), 2, 0.1)).requires_grad_(), R.gauss((H, Hg, k), 3)
    (g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()).backward(dW)
    r = R.weight_norm_bwd_ref(dW, v.detach(), g.detach())
    assert close(r.dg, g.grad, 1e-11) and close(r.dv, v.grad, 1e-11)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) + (c): simulated kernels inside the bounds, planted defects outside, on the GPU file's Gaussian cases
# ------------------------------------------------------------------------------------------------------------------------------
def _norm_cases():
    for dt in DTS:
        for spec in R.LN_COLS:
            for gelu in (False, True):
                yield dt, False, gelu, 33, R.cols_of(spec, dt)
        for rows in R.LN_ROWS:
            yield dt, False, False, rows, R.cols_of("65vec", dt)
        for spec in R.RMS_COLS:
            yield dt, True, False, 5, R.cols_of(spec, dt)
        yield dt, True, False, 1, R.cols_of("vec", dt)


@pytest.mark.parametrize("dt,rms,gelu,rows,cols", list(_norm_cases()))
def test_norm_backward_bounds(dt, rms, gelu, rows, cols):
    x, g, b, dy = R.norm_inputs(rows, cols, dt, 100 + cols, rms)
    g0, b0 = R.ints((cols,), -3, 3, 7), R.ints((cols,), -3, 3, 8)
    r = R.norm_bwd_ref(x, g, b, dy, EPS, rms=rms, gelu=gelu, dt=dt, dgamma0=g0, dbeta0=b0)
    dx, dgam, dbet = R.norm_bwd_sim(x, g, b, dy, EPS, dt, rms=rms, gelu=gelu, dgamma0=g0, dbeta0=b0)
    w = max(worst(dx, r.dx, r.tol_dx), 0.0 if rms else max(worst(dgam, r.dgamma, r.tol_dgamma), worst(dbet, r.dbeta, r.tol_dbeta)))
    print(f"simulated err / tol {w:.3f}")
    assert w < 1.0
    v = R.VEC[dt]
    # the last chunk of every row / the last row left at the sentinel
    for sl in ((slice(None), slice(cols - v, cols)), (slice(rows - 1, rows), slice(None))):
        bad = dx.clone()
        bad[sl] = R.FILL
        assert bool(outside(bad, r.dx, r.tol_dx)[sl].all())
    if not rms:          # the last row's share of the column sums missing
        last = R.norm_bwd_ref(x[-1:], g, b, dy[-1:], EPS, gelu=gelu)
        if rows <= 33:
            for name in ("dbeta", "dgamma"):          # at every column where that share is not itself next to nothing
                full, share, tol = getattr(r, name), getattr(last, name), getattr(r, "tol_" + name)
                assert bool(outside(full - share, full, tol)[share.abs() > 0.1].all()), name
    if cols <= R.DROP_TERM_MAX_COLS and cols > 1:
        # one term dropped from the row mean of dg xhat (the last element's), and the `- s1` term missing on the last chunk only
        dgv = r.d * g
        s2_bad = ((dgv * r.xh).sum(-1, keepdim=True) - (dgv * r.xh)[:, -1:]) / cols
        s1 = torch.zeros(rows, 1).double() if rms else dgv.mean(-1, keepdim=True)
        bad = r.rstd * (dgv - s1 - r.xh * s2_bad)
        sizeable = (dgv * r.xh)[:, -1].abs() > 0.25          # rows whose dropped term is not itself next to nothing
        assert bool(outside(bad, r.dx, r.tol_dx).any(-1)[sizeable].all()), "a dropped reduction term stays inside the bound"
        if not rms and cols > v:
            bad = r.dx.clone()
            bad[:, -v:] = (r.rstd * (dgv - r.xh * dgv.mul(r.xh).mean(-1, keepdim=True)))[:, -v:]
            assert bool(outside(bad, r.dx, r.tol_dx)[:, -v:].any())


@pytest.mark.parametrize("dt", DTS)
def test_elementwise_bounds(dt):
    n = 257 * R.VEC[dt]
    dy, pre = R.rnd(R.gauss((n,), 1), dt), R.rnd(R.gauss((n,), 2, 2.0), dt)
    pre[:8] = R.rnd(torch.tensor([0.0, -0.0, 1e-4, -1e-4, 6.0, -6.0, 40.0, -40.0]).double(), dt)
    r = R.gelu_bwd_ref(dy, pre, dt)
    assert worst(R.gelu_bwd_sim(dy, pre, dt), r.dx, r.tol_dx) < 1.0
    wrong = dy * 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0)))            # gelu' without its u pdf(u) term
    assert bool(outside(wrong, r.dx, r.tol_dx)[(pre.abs() > 0.3) & (pre.abs() < 3) & (dy.abs() > 0.1)].all())
    for M, F_ in ((1, 16), (5, 48)):
        g, up, d = R.rnd(R.gauss((M, F_), 3, 3.0), dt), R.rnd(R.gauss((M, F_), 4), dt), R.rnd(R.gauss((M, F_), 5), dt)
        g[0, :8] = torch.tensor([20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0]).double()
        r = R.silu_mul_bwd_ref(g, up, d, dt)
        sg, su = R.silu_mul_bwd_sim(g, up, d, dt)
        assert bool(torch.isfinite(sg).all() and torch.isfinite(su).all())
        assert worst(sg, r.dgate, r.tol_dgate) < 1.0 and worst(su, r.dup, r.tol_dup) < 1.0
        swapped = outside(r.dup, r.dgate, r.tol_dgate)                    # the two halves written to each other's place
        assert float(swapped.float().mean()) > 0.75
    D, heads, n_rot, n_tok = 4 * R.VEC[dt], 3, 2, 5
    cos, sin, pos = _rope_tables(D)
    x = R.rnd(R.gauss((n_tok, heads * D), 6), dt)
    for inverse in (False, True):
        r = R.rope_ref(x, pos, cos, sin, heads, n_rot, D, inverse, dt)
        assert worst(R.rope_sim(x, pos, cos, sin, heads, n_rot, D, inverse, dt), r.y, r.tol + R.TINY) < 1.0
        flipped = R.rope_sim(x, pos, cos, sin, heads, n_rot, D, inverse, dt, flip=True)       # the sign of s wrong in both directions
        rot = torch.zeros(n_tok, heads, D, dtype=torch.bool)
        rot[1:, :n_rot] = True                                              # position 0 rotates by nothing
        assert float(outside(flipped, r.y, r.tol + R.TINY)[rot.reshape(n_tok, -1)].float().mean()) > 0.9


def _rope_tables(D, max_pos=64):
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2)))
    return ang.cos().float().double(), ang.sin().float().double(), torch.tensor([0, 5, 63, 17, 17])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
@pytest.mark.parametrize("causal", [False, True])
def test_softmax_bounds(dt, cols, causal):
    scale = 0.25
    for rows in ((min(cols, 7), cols) if causal else (7,)):
        if rows < 1:
            continue
        S, dP = R.gauss((3, rows, cols), cols, 4.0).float().double(), R.gauss((3, rows, cols), cols + 1).float().double()
        vis = R.causal_vis(rows, cols, causal)
        r = R.softmax_ref(S, scale, vis, dt)
        assert worst(R.softmax_sim(S, scale, vis, dt), r.P, r.tol_P + R.TINY) < 1.0
        Pst = R.rnd(r.P, dt)
        b = R.softmax_bwd_ref(Pst, dP, scale, vis, dt)
        assert worst(R.softmax_bwd_sim(Pst, dP, scale, vis, dt), b.dS, b.tol_dS + R.TINY) < 1.0
        if causal and cols > 1:
            # the visible limit one short: every row that sees more than one column loses its last one
            short = R.causal_vis(rows, cols, True, shift=cols - rows - 1)
            bad = R.softmax_sim(S, scale, short, dt)
            many = vis.sum(-1) > 1
            assert bool(outside(bad, r.P, r.tol_P + R.TINY).any(-1)[:, many].all())
        if cols > 1:
            # one term dropped from the backward's dot product
            dot_bad = ((Pst * dP) * vis).sum(-1, keepdim=True) - (Pst * dP * vis)[..., :1]
            bad = scale * Pst * vis * (dP * vis - dot_bad)
            hit = outside(bad, b.dS, b.tol_dS + R.TINY).any(-1)
            assert bool(hit[(Pst * dP * vis)[..., 0].abs() > 0.05].all())          # 0.05 > 2 u x any |dP - dot| of these rows


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("V", R.LOSS_V)
def test_loss_bounds(dt, V):
    rows, ns = 7, 3
    for shift in (0.0, 1000.0):
        s, t, lab = R.loss_inputs(rows, V, V, shift)
        lab[3] = -1
        coef = torch.tensor([[0.5, 0.25, 0.125, 0.5]] * rows).double()
        coef[4, 2:] = 0.0
        slot = torch.tensor([0, 0, 2, 2, 2, 0, 2])
        for teacher in (None, t):
            r = R.kd_logit_ref(s, teacher, lab, coef, slot, ns, dt)
            sim = R.kd_logit_sim(s, teacher, lab, coef, dt)
            assert worst(sim, r.ds, r.tol_ds) < 1.0
            if V > 1:
                # the one-hot term at the wrong column (label off by one), and the last element left at the sentinel
                wrong = R.kd_logit_ref(s, teacher, torch.where(lab >= 0, (lab + 1) % V, lab), coef, slot, ns, dt).ds
                ok = lab >= 0
                assert bool(outside(wrong, r.ds, r.tol_ds)[ok, lab[ok]].all())
            bad = sim.clone()
            bad[:, -1] = R.FILL
            assert bool(outside(bad, r.ds, r.tol_ds)[:, -1].all())
    a, b = R.rnd(R.gauss((257,), 1), dt), R.rnd(R.gauss((257,), 2), dt)
    da0 = R.rnd(R.gauss((257,), 3), dt)
    for acc in (None, da0):
        r = R.mse_ref(a, b, 0.5, dt, da0=acc)
        assert worst(R.mse_sim(a, b, 0.5, dt, da0=acc), r.da, r.tol_da) < 1.0
        assert bool(outside(r.da * (257.0 / 256.0), r.da, r.tol_da)[r.da.abs() > 1e-3].all()) or dt != F32      # 1 / (n - 1): visible in fp32
    H = 65 * R.VEC[dt]
    a2, b2 = R.rnd(R.gauss((6, H), 4), dt), R.rnd(R.gauss((6, H), 5), dt)
    mc = torch.tensor([[0.5, 0.25]] * 6).double()
    r = R.kd_mse_rows_ref(a2, b2, mc, torch.tensor([0, 0, 2, 2, 2, 0]), 3, dt)
    assert worst(R.kd_mse_rows_sim(a2, b2, mc, dt), r.da, r.tol_da) < 1.0
    short = R.kd_mse_rows_ref(a2[:, :-1], b2[:, :-1], mc, torch.tensor([0, 0, 2, 2, 2, 0]), 3, dt).losses       # a row sum one term short
    assert bool(outside(short, r.losses, r.tol_losses)[[0, 2]].all())


@pytest.mark.parametrize("C_", [64, 512])
@pytest.mark.parametrize("L", R.CONV0_L)
def test_conv0_backward_bounds(C_, L):
    wave, w, bias, gamma, beta, dy, init = R.conv0_inputs(C_, L, 4, 10 * L + C_ // 64, BF16)
    r = R.conv0_bwd_ref(wave, w, bias, gamma, beta, dy, EPS, BF16, init)
    sim = R.conv0_bwd_sim(wave, w, bias, gamma, beta, dy, EPS, init)
    worsts = [worst(s_, ref, tol) for s_, ref, tol in zip(sim, (r.dw, r.dbias, r.dgamma, r.dbeta), (r.tol_dw, r.tol_dbias, r.tol_dgamma, r.tol_dbeta))]
    print("simulated err / tol", worsts)
    assert max(worsts) < 1.0
    # the last time step's contribution dropped from the sums (a strip one step short)
    if L > 1:
        short = R.conv0_bwd_ref(wave[:-5], w, bias, gamma, beta, dy[:-1], EPS, BF16, init)
    else:
        short = SimpleNamespace(dw=init[0], dbias=init[1], dgamma=init[2], dbeta=init[3])
    for got, ref, tol in ((short.dw, r.dw, r.tol_dw), (short.dbias, r.dbias, r.tol_dbias), (short.dgamma, r.dgamma, r.tol_dgamma), (short.dbeta, r.dbeta, r.tol_dbeta)):
        assert bool(outside(got, ref, tol)[(got - ref).abs() > 0.05].all())          # wherever that step's share is not next to nothing


@pytest.mark.parametrize("step", [1, 1000])
def test_adamw_bounds(step):
    sc = R.adamw_scalars(step=step, **R.ADAMW_HYPER)
    n = 4097
    p, g, m, v = [x.float().double() for x in (R.gauss((n,), 1, 0.05), R.gauss((n,), 2, 0.01), R.gauss((n,), 3, 0.01), R.gauss((n,), 4, 1e-4).abs())]
    g[:4], v[:4], m[:4] = 0.0, 0.0, torch.tensor([0.0, 1e-3, -1e-3, 1e-8]).double()          # the denominator is eps alone
    r = R.adamw_ref(p, g, m, v, sc)
    sp, sm, sv = R.adamw_sim(p, g, m, v, sc)
    assert max(worst(sp, r.p, r.tol_p), worst(sm, r.m, r.tol_m), worst(sv, r.v, r.tol_v)) < 1.0
    # the bias correction of the second moment left out; beta2 in place of 1 - beta2; the weight decay left out
    for key, val, what in (("bc2_sqrt", 1.0, "p"), ("w2", sc["beta2"], "v"), ("decay", 1.0, "p")):
        wrong = R.adamw_ref(p, g, m, v, dict(sc, **{key: val}))
        hit = outside(getattr(wrong, what), getattr(r, what), getattr(r, "tol_" + what))
        if key == "bc2_sqrt" and step == 1000:
            hit = hit[4:]
        assert float(hit[4:].float().mean()) > 0.9, key


@pytest.mark.parametrize("H,Hg,k", R.WN_SHAPES)
def test_weight_norm_bounds(H, Hg, k):
    dW, v, g = R.gauss((H, Hg, k), 1).float().double(), R.gauss((H, Hg, k), 2).float().double(), (1 + R.gauss((k,), 3, 0.1)).float().double()
    r = R.weight_norm_bwd_ref(dW, v, g)
    sg, sv = R.weight_norm_bwd_sim(dW, v, g)
    assert worst(sg, r.dg, r.tol_dg) < 1.0 and worst(sv, r.dv, r.tol_dv) < 1.0
    if H > 1:          # the last h row missing from the two sums
        short = R.weight_norm_bwd_ref(dW[:-1], v[:-1], g)
        assert float(outside(short.dg, r.dg, r.tol_dg).float().mean()) > 0.9
        assert float(outside(short.dv, r.dv[:-1], r.tol_dv[:-1]).float().mean()) > 0.9


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,stride", R.POOL_KS)
def test_pool_bounds(dt, kernel, stride):
    T, H = 29, R.VEC[dt]
    P = (T - kernel) // stride + 1
    dy = R.ints((P, H), -64, 64, kernel)
    r = R.avgpool_bwd_ref(dy, T, kernel, stride, dt)
    sim = R.rnd((r.dx * kernel).float() * (torch.tensor(1.0) / torch.tensor(float(kernel))), dt)
    if kernel & (kernel - 1) == 0:
        assert torch.equal(sim, R.rnd(r.dx, dt))
    assert bool(((sim - r.dx).abs() <= r.tol_dx).all())
    # p_lo rounded down instead of up: the window before the first one that covers t is added
    bad = torch.zeros(T, H).double()
    for t in range(T):
        first = t - kernel + 1
        lo = 0 if first <= 0 else first // stride
        for p in range(lo, P):
            if p * stride <= t:
                bad[t] += dy[p]
    bad = bad / kernel
    if kernel % stride:
        assert bool(outside(bad, r.dx, r.tol_dx + R.TINY).any())
