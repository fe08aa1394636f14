"""Backward, loss and optimizer kernels of the KD step restated in plain torch, fp64, on the CPU (a helper module of the edge suite's third
chapter, not a conftest; it imports neither a GPU nor the library).

Every `*_ref` takes the STORED (already rounded) inputs in fp64 and returns a namespace of fp64 results; with a storage type `dt` it also
returns, per element, a bound `tol_*` on what a kernel may return.  The bounds are first-order worst-case propagations of the fp32
roundings of csrc/train_ops.hip (built with -ffp-contract=off: every operation rounds once, an fmaf once):

    tol = 2 u |ref|                       the output's rounding to the storage type (u = half an ulp, twice as in the GEMM bound)
        + sum over the operations of the chain of 2^-24 x the magnitude the operation acts on, magnitudes taken term by term with absolute
          values (a reduction of n terms in ANY order, atomics included: n 2^-24 sum |term|), errors of intermediate values carried forward
        + TRANS relative for every device transcendental (__expf, erff, logf, rsqrtf, rcp): the 2e-6 (1 + |.|) term of silu_mul_bound and
          of the GELU bound in tests/test_kernel_edges_gpu.py; the log-sum-exp's last add uses attn_train_ref.py's lse_ulp
        + TINY, the smallest normal fp32 number (a flushed denormal).

No constant here is a measured number.  `*_sim` are the same operations evaluated in fp32 torch in the kernels' order with the storage
rounding: tests/test_train_ref_cpu.py requires them inside the bounds and planted defects outside.  The case tables at the end are shared
by tests/test_train_edges_gpu.py (on the GPU) and the CPU self-check."""
import math
from types import SimpleNamespace

import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}        # half an ulp, relative (as in the edge suite)
VEC = {F16: 8, BF16: 8, F32: 4}                                # elements of a 16-byte access
E24 = 2.0 ** -24
TRANS = 2e-6          # relative allowance of one device transcendental: test_kernel_edges_gpu.py silu_mul_bound / check_gauss (GELU)
TINY = 2.0 ** -126    # smallest normal fp32
GELU_D2 = 0.8         # max |gelu''| = 2 pdf(0) = 0.798: how an error of the pre-activation reaches gelu'
FILL = -1504.0        # the suite's output sentinel
SUBN = {F16: 2.0 ** -25, BF16: 2.0 ** -134, F32: 2.0 ** -150}          # half the storage type's smallest subnormal: fp16 gradients of a wide softmax get there


def lse_ulp(lse):
    """one fp32 operation on a log-sum-exp (tests/attn_train_ref.py, r.lse_ulp)"""
    return E24 * lse.abs().clamp(min=1.0)


def f32(v):
    """a python float as the C ABI's `float` argument holds it"""
    return float(torch.tensor(v, dtype=torch.float32))


def rnd(x, dt):
    """fp32 / fp64 -> the storage type's value, as fp64 (round-to-nearest-even from fp32, torch's)"""
    return x.float().to(dt).double()


def gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _mean(x):
    return x.mean(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm (optionally through GELU) and RMSNorm backward: norm_bwd_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def norm_bwd_ref(x, g, b, dy, eps, rms=False, gelu=False, dt=None, x_err=None, dgamma0=None, dbeta0=None):
    """x, dy (rows, n), g, b (n).  dx = rstd (dg - mean(dg) - xhat mean(dg xhat)), dg = dy gelu'(xhat g + b) g (RMS: no mean terms, xhat = x
    rstd); dgamma = dgamma0 + sum_rows d xhat, dbeta = dbeta0 + sum_rows d.  x_err: an absolute error bound the kernel's own x carries
    (conv0 recomputes it).  Roundings counted: mean n + 1 (sum, divide); centring 1; variance n + 3 (square, sum, divide); rstd the add
    and rsqrtf; xhat 1; z = xhat g + b 2, gelu' TRANS (1 + |z|) (erff and __expf under a product) and the multiply; dg 1; the two row
    means n + 1 and n + 2; the output 3 inside the bracket and the multiply by rstd; column sums rows + 1 in any order and the add into
    the buffer."""
    rows, n = x.shape
    eps = f32(eps)
    mean = torch.zeros(rows, 1, dtype=torch.float64) if rms else _mean(x)
    c = x - mean
    var = _mean(c * c)
    rstd = (var + eps).rsqrt()
    xh = c * rstd
    z = xh * g + b if gelu else None
    d = dy * gelu_grad64(z) if gelu else dy
    dg = d * g
    s1 = torch.zeros(rows, 1, dtype=torch.float64) if rms else _mean(dg)
    s2 = _mean(dg * xh)
    dx = rstd * (dg - s1 - xh * s2)
    g0 = torch.zeros(n, dtype=torch.float64) if dgamma0 is None else dgamma0
    b0 = torch.zeros(n, dtype=torch.float64) if dbeta0 is None else dbeta0
    r = SimpleNamespace(dx=dx, dgamma=g0 + (d * xh).sum(0), dbeta=b0 + d.sum(0), xh=xh, rstd=rstd, d=d)
    if dt is None:
        return r
    u, E = U[dt], E24
    xe = torch.zeros_like(x) if x_err is None else x_err
    e_mean = 0.0 if rms else (n + 1) * E * _mean(x.abs()) + _mean(xe)
    e_c = e_mean + xe + (0.0 if rms else E * c.abs())
    e_var = _mean(2 * c.abs() * e_c) + (n + 3) * E * var
    rr = 0.5 * e_var / (var + eps) + E + TRANS
    e_xh = rstd * e_c + xh.abs() * (rr + E)
    if gelu:
        e_z = g.abs() * e_xh + 2 * E * ((xh * g).abs() + b.abs())
        e_d = dy.abs() * (GELU_D2 * e_z + TRANS * (1 + z.abs())) + E * d.abs()
    else:
        e_d = torch.zeros_like(x)
    e_dg = g.abs() * e_d + E * dg.abs()
    e_s1 = 0.0 if rms else (n + 1) * E * _mean(dg.abs()) + _mean(e_dg)
    e_s2 = (n + 2) * E * _mean((dg * xh).abs()) + _mean(dg.abs() * e_xh + xh.abs() * e_dg)
    r.e_dx = dx.abs() * (rr + E) + rstd * (e_dg + e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + 3 * E * (dg.abs() + s1.abs() + (xh * s2).abs()))
    r.tol_dx = 2 * u * dx.abs() + r.e_dx + TINY
    r.tol_dgamma = (rows + 1) * E * (d * xh).abs().sum(0) + (d.abs() * e_xh + xh.abs() * e_d).sum(0) + E * (g0.abs() + r.dgamma.abs()) + TINY
    r.tol_dbeta = rows * E * d.abs().sum(0) + e_d.sum(0) + E * (b0.abs() + r.dbeta.abs()) + TINY
    return r


def gelu_grad32(u):
    return 0.5 * (1.0 + torch.erf(u * 0.70710678118654752440)) + u * (0.39894228040143267794 * torch.exp(-0.5 * u * u))


def norm_bwd_sim(x, g, b, dy, eps, dt, rms=False, gelu=False, dgamma0=None, dbeta0=None):
    """fp32, the kernel's order (row sums by torch's own tree): (dx as stored, dgamma, dbeta) in fp64"""
    x, g, b, dy = x.float(), g.float(), b.float(), dy.float()
    n = x.shape[1]
    eps = torch.tensor(eps, dtype=F32)
    if rms:
        mean = torch.zeros(x.shape[0], 1)
        rstd = torch.rsqrt((x * x).sum(-1, keepdim=True) / n + eps)
    else:
        mean = x.sum(-1, keepdim=True) / n
        c = x - mean
        rstd = torch.rsqrt((c * c).sum(-1, keepdim=True) / n + eps)
    xh = (x - mean) * rstd
    d = dy * gelu_grad32(xh * g + b) if gelu else dy
    dg = d * g
    s1 = torch.zeros_like(mean) if rms else dg.sum(-1, keepdim=True) / n
    s2 = (dg * xh).sum(-1, keepdim=True) / n
    dx = rstd * (dg - xh * s2) if rms else rstd * (dg - s1 - xh * s2)
    g0 = torch.zeros(n) if dgamma0 is None else dgamma0.float()
    b0 = torch.zeros(n) if dbeta0 is None else dbeta0.float()
    return rnd(dx, dt), (g0 + (d * xh).sum(0)).double(), (b0 + d.sum(0)).double()


# ------------------------------------------------------------------------------------------------------------------------------
# elementwise: GELU backward, SwiGLU backward, RoPE
# ------------------------------------------------------------------------------------------------------------------------------
def gelu_bwd_ref(dy, pre, dt):
    """dx = dy gelu'(pre): TRANS (1 + |pre|) for erff / __expf, one multiply"""
    dx = dy * gelu_grad64(pre)
    return SimpleNamespace(dx=dx, tol_dx=2 * U[dt] * dx.abs() + dy.abs() * TRANS * (1 + pre.abs()) + 2 * E24 * dx.abs() + TINY)


def gelu_bwd_sim(dy, pre, dt):
    return rnd(dy.float() * gelu_grad32(pre.float()), dt)


def silu_mul_bwd_ref(g, up, d, dt):
    """d gate = d up sg (1 + g (1 - sg)), d up = d g sg with sg = 1 / (1 + exp(-g)).  sg: __expf and the reciprocal (2 TRANS, relative) and
    the add; 1 - sg: the error of sg and one rounding; the bracket two roundings; three multiplies each.  A flushed denormal of sg costs
    TINY times what multiplies it."""
    E = E24
    sg = torch.sigmoid(g)
    om = 1.0 - sg
    br = 1.0 + g * om
    dgate, dup = d * up * sg * br, d * g * sg
    e_sg = sg * (2 * TRANS + 2 * E)
    e_br = g.abs() * (e_sg + E * om) + E * ((g * om).abs() + br.abs())
    du = (d * up).abs()
    e_gate = du * (e_sg * br.abs() + sg * e_br) + 3 * E * dgate.abs() + TINY * (1 + du * (1 + g.abs()))
    e_up = (d * g).abs() * e_sg + 2 * E * dup.abs() + TINY * (1 + (d * g).abs())
    u = U[dt]
    return SimpleNamespace(dgate=dgate, dup=dup, tol_dgate=2 * u * dgate.abs() + e_gate, tol_dup=2 * u * dup.abs() + e_up)


def silu_mul_bwd_sim(g, up, d, dt):
    g, up, d = g.float(), up.float(), d.float()
    sg = 1.0 / (1.0 + torch.exp(-g))
    return rnd(d * up * sg * (1.0 + g * (1.0 - sg)), dt), rnd(d * g * sg, dt)


def interleave(g, up):
    """gate / up (M, F) -> gu (M, 2 F) in [16 gate | 16 up] blocks"""
    M, F_ = g.shape
    return torch.stack([g.view(M, F_ // 16, 16), up.view(M, F_ // 16, 16)], dim=2).reshape(M, 2 * F_)


def deinterleave(gu):
    M, F2 = gu.shape
    v = gu.view(M, F2 // 32, 2, 16)
    return v[:, :, 0].reshape(M, F2 // 2), v[:, :, 1].reshape(M, F2 // 2)


def rope_ref(x, pos, cos, sin, heads, n_rot, D, inverse, dt):
    """x (n_tok, heads D); cos, sin (max_pos, D / 2) fp64 of the fp32 tables.  First n_rot heads: (a, b) -> (a c - b s, b c + a s), s
    negated for the inverse; the others keep their bits.  Two products and one add per output."""
    n = x.shape[0]
    xv = x.view(n, heads, D).clone()
    tol = torch.zeros_like(xv)
    h = D // 2
    c, s = cos[pos][:, None, :], (-sin[pos] if inverse else sin[pos])[:, None, :]
    a, b = xv[:, :n_rot, :h].clone(), xv[:, :n_rot, h:].clone()
    xv[:, :n_rot, :h], xv[:, :n_rot, h:] = a * c - b * s, b * c + a * s
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    tol[:, :n_rot] = 2 * U[dt] * xv[:, :n_rot].abs() + 3 * E24 * mag + TINY
    return SimpleNamespace(y=xv.reshape(n, heads * D), tol=tol.reshape(n, heads * D))


def rope_sim(x, pos, cos, sin, heads, n_rot, D, inverse, dt, flip=False):
    n = x.shape[0]
    xv = x.float().view(n, heads, D).clone()
    h = D // 2
    sign = -1.0 if inverse else 1.0
    if flip:
        sign = -sign
    c, s = cos.float()[pos][:, None, :], sign * sin.float()[pos][:, None, :]
    a, b = xv[:, :n_rot, :h].clone(), xv[:, :n_rot, h:].clone()
    xv[:, :n_rot, :h], xv[:, :n_rot, h:] = a * c - b * s, b * c + a * s
    out = x.clone().view(n, heads, D)
    out[:, :n_rot] = rnd(xv[:, :n_rot], dt)
    return out.reshape(n, heads * D)


# ------------------------------------------------------------------------------------------------------------------------------
# explicit softmax and its backward
# ------------------------------------------------------------------------------------------------------------------------------
def causal_vis(rows, cols, causal, shift=None):
    """column j visible to row i: j < cols, and under the causal mask j <= i + cols - rows"""
    if not causal:
        return torch.ones(rows, cols, dtype=torch.bool)
    shift = cols - rows if shift is None else shift
    return torch.arange(cols)[None, :] <= torch.arange(rows)[:, None] + shift


def softmax_ref(S, scale, vis, dt):
    """S (..., rows, cols) stored fp32 scores, vis (rows, cols): P = softmax(scale S) over the visible columns, 0 elsewhere.  The exponent's
    argument: the scale multiply and the subtraction, 2^-24 (|t| + |m|) each; __expf TRANS; the row sum (all terms positive) n roundings on
    top of its terms' errors; the reciprocal and the last multiply."""
    E = E24
    scale = f32(scale)
    t = (S * scale).masked_fill(~vis, float("-inf"))
    m = t.amax(-1, keepdim=True)
    e = torch.exp(t - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    rel_e = (TRANS + 2 * E * (t.abs() + m.abs())).masked_fill(~vis, 0.0)
    rel_l = (rel_e * e).sum(-1, keepdim=True) / l + vis.sum(-1, keepdim=True) * E
    return SimpleNamespace(P=P, tol_P=(2 * U[dt] * P + P * (rel_e + rel_l + 2 * E) + TINY).masked_fill(~vis, 0.0))


def softmax_sim(S, scale, vis, dt):
    t = (S.float() * torch.tensor(scale, dtype=F32)).masked_fill(~vis, float("-inf"))
    e = torch.exp(t - t.amax(-1, keepdim=True))
    return rnd(e * (1.0 / e.sum(-1, keepdim=True)), dt)


def softmax_bwd_ref(P, dP, scale, vis, dt):
    """dS = scale P (dP - sum_visible P dP) on the stored P: the dot n + 1 roundings, the subtraction, two multiplies"""
    scale = f32(scale)
    Pv, dPv = P * vis, dP * vis
    n = vis.sum(-1, keepdim=True)
    dot = (Pv * dPv).sum(-1, keepdim=True)
    dS = scale * Pv * (dPv - dot)
    e = scale * Pv * ((n + 1) * E24 * (Pv * dPv).abs().sum(-1, keepdim=True) + E24 * (dPv.abs() + dot.abs())) + 2 * E24 * dS.abs()
    return SimpleNamespace(dS=dS, tol_dS=(2 * U[dt] * dS.abs() + e + TINY) * vis)


def softmax_bwd_sim(P, dP, scale, vis, dt):
    Pv, dPv = P.float() * vis, dP.float() * vis
    return rnd(torch.tensor(scale, dtype=F32) * Pv * (dPv - (Pv * dPv).sum(-1, keepdim=True)), dt)


# ------------------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------------------
def _lse(s):
    """rows of logits -> lse, softmax, and their errors.  exp: TRANS and the subtraction's rounding of its argument; the sum V roundings on
    its terms' errors; logf TRANS (1 + |log l|) and the final add lse_ulp; the probability: exp, the sum, the reciprocal, the multiply."""
    V = s.shape[-1]
    m = s.amax(-1, keepdim=True)
    a = s - m
    e = torch.exp(a)
    l = e.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    rel_e = TRANS + E24 * a.abs()
    rel_l = (rel_e * e).sum(-1, keepdim=True) / l + V * E24
    return SimpleNamespace(lse=lse, p=e / l, e=e, l=l, rel_e=rel_e, rel_l=rel_l, rp=rel_e + rel_l + 2 * E24,
                           e_lse=rel_l + TRANS * (1 + torch.log(l).abs()) + lse_ulp(lse))


def kd_logit_ref(s, t, labels, coef, slot, n_slots, dt, loss0=None):
    """sl_kd_logit_losses on rows of stored fp32 logits; also sl_ce_loss / sl_soft_ce_loss (one slot, a constant coefficient row).
    s, t (rows, V) (t None: no teacher); labels (rows) int, < 0: no next-token term; coef (rows, 4) = {ce loss, ce grad, soft loss, soft
    grad}; losses (n_slots, 2) = loss0 + per-slot sums; ds = (c1 [lab >= 0] + c3) softmax(s) - c3 softmax(t) - c1 onehot."""
    rows, V = s.shape
    E = E24
    S = _lse(s)
    lab_ok = labels >= 0
    oh = torch.zeros(rows, V, dtype=torch.float64)
    oh[lab_ok, labels[lab_ok]] = 1.0
    s_lab = (s * oh).sum(-1, keepdim=True)
    c0, c1, c2, c3 = [coef[:, i:i + 1] for i in range(4)]
    soft = (t is not None) & ((c2 != 0) | (c3 != 0))
    cce = c1 * lab_ok[:, None]
    ce_term = torch.where(lab_ok[:, None], c0 * (S.lse - s_lab), torch.zeros(()).double())
    e_ce = torch.where(lab_ok[:, None], c0.abs() * (S.e_lse + E * (S.lse.abs() + s_lab.abs())) + E * ce_term.abs(), torch.zeros(()).double())
    if t is not None:
        T = _lse(torch.where(soft, t, torch.zeros(()).double()))          # a row without a soft term never reads its teacher row
        q = (T.p * s).sum(-1, keepdim=True)
        e_q = ((T.rel_e * T.e * s.abs()).sum(-1, keepdim=True) + (V + 1) * E * (T.e * s.abs()).sum(-1, keepdim=True)) / T.l + q.abs() * (T.rel_l + E)
        so_term = torch.where(soft, c2 * (S.lse - q), torch.zeros(()).double())
        e_so = torch.where(soft, c2.abs() * (S.e_lse + e_q + E * (S.lse.abs() + q.abs())) + E * so_term.abs(), torch.zeros(()).double())
        c3e = c3 * soft
        pt, rpt = T.p, T.rp
    else:
        so_term, e_so, c3e, pt, rpt = torch.zeros(rows, 1).double(), torch.zeros(rows, 1).double(), torch.zeros(rows, 1).double(), 0.0, 0.0
    cs = cce + c3e
    ds = cs * S.p - c3e * pt - cce * oh
    e_ds = cs.abs() * S.p * (S.rp + 3 * E) + c3e.abs() * pt * (rpt + 2 * E) + E * cce.abs() * oh + 2 * E * ds.abs()
    losses = torch.zeros(n_slots, 2, dtype=torch.float64) if loss0 is None else loss0.clone()
    mag, err, cnt = losses.abs().clone(), torch.zeros(n_slots, 2, dtype=torch.float64), torch.zeros(n_slots, 2, dtype=torch.float64)
    for col, (term, e_t) in enumerate(((ce_term, e_ce), (so_term, e_so))):
        losses[:, col].index_add_(0, slot, term[:, 0])
        mag[:, col].index_add_(0, slot, term[:, 0].abs())
        err[:, col].index_add_(0, slot, e_t[:, 0])
        cnt[:, col].index_add_(0, slot, (term[:, 0] != 0).double())
    return SimpleNamespace(losses=losses, tol_losses=err + (cnt + 1) * E * mag + TINY, ds=ds, e_ds=e_ds,
                           tol_ds=2 * U[dt] * ds.abs() + e_ds + SUBN[dt] + TINY, p=S.p, lse=S.lse)


def kd_logit_sim(s, t, labels, coef, dt):
    """ds in fp32, the kernel's expression"""
    s32 = s.float()
    rows, V = s.shape
    lab_ok = labels >= 0
    oh = torch.zeros(rows, V)
    oh[lab_ok, labels[lab_ok]] = 1.0
    c = coef.float()
    e = torch.exp(s32 - s32.amax(-1, keepdim=True))
    ps = e * (1.0 / e.sum(-1, keepdim=True))
    cce = c[:, 1:2] * lab_ok[:, None]
    if t is None:
        return rnd(cce * ps - cce * oh, dt)
    soft = (c[:, 2:3] != 0) | (c[:, 3:4] != 0)
    t32 = torch.where(soft, t.float(), torch.zeros(()))
    et = torch.exp(t32 - t32.amax(-1, keepdim=True))
    c3 = c[:, 3:4] * soft
    return rnd((cce + c3) * ps - c3 * (et * (1.0 / et.sum(-1, keepdim=True))) - cce * oh, dt)


def mse_ref(a, b, coef, dt, da0=None, loss0=0.0):
    """sl_mse_loss: loss = loss0 + coef mean((a - b)^2), da = (2 coef / n) (a - b) [+ da0].  Gradient: the subtraction, the two
    operations that form 2 coef / n, the multiply, the add.  Loss: n terms in any order, the square, coef, / n, the atomics."""
    n = a.numel()
    coef = f32(coef)
    d = a - b
    loss = loss0 + coef * (d * d).sum() / n
    da = 2.0 * coef / n * d + (0.0 if da0 is None else da0)
    tol_da = 2 * U[dt] * da.abs() + 4 * E24 * (2.0 * coef / n * d).abs() + E24 * da.abs() + TINY
    tol_loss = (n + 5) * E24 * abs(coef) * float((d * d).sum()) / n + E24 * (abs(loss0) + abs(float(loss))) + TINY
    return SimpleNamespace(loss=float(loss), da=da, tol_da=tol_da, tol_loss=tol_loss)


def mse_sim(a, b, coef, dt, da0=None):
    n = a.numel()
    g = torch.tensor(2.0, dtype=F32) * torch.tensor(coef, dtype=F32) / torch.tensor(float(n), dtype=F32)
    da = g * (a.float() - b.float()) + (0.0 if da0 is None else da0.float())
    return rnd(da, dt)


def kd_mse_rows_ref(a, b, coef, slot, n_slots, dt, loss0=None):
    """sl_kd_mse_rows: losses[slot[r]] += c0 sum_h (a - b)^2, da[r] = c1 (a - b)"""
    rows, H = a.shape
    d = a - b
    acc = (d * d).sum(-1)
    term = coef[:, 0] * acc
    da = coef[:, 1:2] * d
    losses = torch.zeros(n_slots, dtype=torch.float64) if loss0 is None else loss0.clone()
    mag, err, cnt = losses.abs().clone(), torch.zeros(n_slots, dtype=torch.float64), torch.zeros(n_slots, dtype=torch.float64)
    losses.index_add_(0, slot, term)
    mag.index_add_(0, slot, term.abs())
    err.index_add_(0, slot, (H + 3) * E24 * term.abs())
    cnt.index_add_(0, slot, torch.ones(rows, dtype=torch.float64))
    return SimpleNamespace(losses=losses, tol_losses=err + (cnt + 1) * E24 * mag + TINY, da=da, tol_da=2 * U[dt] * da.abs() + 2 * E24 * da.abs() + TINY)


def kd_mse_rows_sim(a, b, coef, dt):
    return rnd(coef[:, 1:2].float() * (a.float() - b.float()), dt)


# ------------------------------------------------------------------------------------------------------------------------------
# front-end backward
# ------------------------------------------------------------------------------------------------------------------------------
def avgpool_bwd_ref(dy, T, kernel, stride, dt=None):
    """dy (P, H) -> dx (T, H): dx[t] = (sum of dy[p] over the windows p < P with p stride <= t < p stride + kernel) / kernel.  With integer
    dy the window sum is exact; 1 / kernel and the multiply round once each (both exact for a power of two)."""
    P, H = dy.shape
    dx = torch.zeros(T, H, dtype=torch.float64)
    for p in range(P):
        dx[p * stride:min(T, p * stride + kernel)] += dy[p]
    dx = dx / kernel
    return SimpleNamespace(dx=dx, tol_dx=None if dt is None else 2 * U[dt] * dx.abs() + 2 * E24 * dx.abs())


def col2im_ref(dcol, Lin, Cc, k, s):
    """dcol (Lout, k Cc) -> dx (Lin, Cc): dx[to s + j] += dcol[to][j Cc : (j + 1) Cc]"""
    Lout = dcol.shape[0]
    dx = torch.zeros(Lin, Cc, dtype=torch.float64)
    for to in range(Lout):
        for j in range(k):
            if to * s + j < Lin:
                dx[to * s + j] += dcol[to, j * Cc:(j + 1) * Cc]
    return dx


def conv0_frames(wave, L, k=10, stride=5):
    return torch.stack([wave[stride * t:stride * t + k] for t in range(L)])


def conv0_bwd_ref(wave, w, bias, gamma, beta, dy, eps, dt, init=None):
    """sl_hubert_conv0_bwd: y = conv(wave; w, bias) (L, C) recomputed (an fmaf chain of k taps on the bias: k roundings), d y through GELU
    and LayerNorm by norm_bwd_ref with that error on its input, then dbias = sum_t dc, dw[c][j] = sum_t dc[t][c] wave[stride t + j] (fmaf
    chains per strip, atomics across strips: L + 1 roundings in any order).  init: the four buffers' starting values (dw, dbias, dgamma,
    dbeta)."""
    C_, k = w.shape
    L = dy.shape[0]
    X = conv0_frames(wave, L, k)
    y = X @ w.T + bias
    e_y = k * E24 * (X.abs() @ w.abs().T + bias.abs())
    z = [torch.zeros(C_, k, dtype=torch.float64)] + [torch.zeros(C_, dtype=torch.float64)] * 3 if init is None else init
    n = norm_bwd_ref(y, gamma, beta, dy, eps, gelu=True, dt=F32, x_err=e_y, dgamma0=z[2], dbeta0=z[3])
    dc = n.dx
    r = SimpleNamespace(dw=z[0] + dc.T @ X, dbias=z[1] + dc.sum(0), dgamma=n.dgamma, dbeta=n.dbeta, tol_dgamma=n.tol_dgamma, tol_dbeta=n.tol_dbeta, dc=dc)
    r.tol_dw = (L + 1) * E24 * (dc.abs().T @ X.abs()) + n.e_dx.T @ X.abs() + E24 * (z[0].abs() + r.dw.abs()) + TINY
    r.tol_dbias = L * E24 * dc.abs().sum(0) + n.e_dx.sum(0) + E24 * (z[1].abs() + r.dbias.abs()) + TINY
    return r


def conv0_bwd_sim(wave, w, bias, gamma, beta, dy, eps, init):
    L = dy.shape[0]
    X = conv0_frames(wave, L, w.shape[1]).float()
    y = X @ w.float().T + bias.float()
    dc, dgam, dbet = norm_bwd_sim(y, gamma, beta, dy, eps, F32, gelu=True, dgamma0=init[2], dbeta0=init[3])
    dc = dc.float()
    return (init[0].float() + dc.T @ X).double(), (init[1].float() + dc.sum(0)).double(), dgam, dbet


# ------------------------------------------------------------------------------------------------------------------------------
# AdamW, weight-norm backward
# ------------------------------------------------------------------------------------------------------------------------------
def adamw_scalars(lr, beta1, beta2, eps, wd, step, fp32=True):
    """the scalars sl_adamw_step forms on the host in double and rounds to fp32 once each"""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    sc = dict(decay=1.0 - lr * wd, w1=1.0 - beta1, beta2=beta2, w2=1.0 - beta2, eps=eps, step_size=lr / bc1, bc2_sqrt=math.sqrt(bc2))
    return {k: (f32(v) if fp32 else v) for k, v in sc.items()}


def adamw_ref(p, g, m, v, sc):
    """one update on fp64 copies of the fp32 state with the scalars `sc`; the bound counts, line by line of adamw_multi_kernel:
    p decay 1; m + w1 (g - m) 3; v beta2 + (w2 g) g 4; sqrt(v) / bc + eps 3 on top of v's error through the square root (v = 0 with g = 0
    is exact: the denominator is eps alone); p - step_size (m / denom) 3 on top of the errors of m and denom."""
    E = E24
    p1 = p * sc["decay"]
    m1 = m + sc["w1"] * (g - m)
    v1 = v * sc["beta2"] + (sc["w2"] * g) * g
    rt = v1.sqrt()
    den = rt / sc["bc2_sqrt"] + sc["eps"]
    upd = sc["step_size"] * (m1 / den)
    p2 = p1 - upd
    e_p1 = E * p1.abs()
    e_m = E * (2 * (sc["w1"] * (g - m)).abs() + m1.abs())
    e_v = E * ((v * sc["beta2"]).abs() + 2 * (sc["w2"] * g * g).abs() + v1.abs())
    e_rt = torch.where(v1 > 0, 0.5 * e_v / rt.clamp(min=TINY), torch.zeros(()).double()) + E * rt
    e_den = e_rt / sc["bc2_sqrt"] + E * (rt / sc["bc2_sqrt"] + den)
    e_upd = sc["step_size"] * (e_m / den + m1.abs() * e_den / (den * den)) + 2 * E * upd.abs()
    return SimpleNamespace(p=p2, m=m1, v=v1, tol_p=e_p1 + e_upd + E * p2.abs() + TINY, tol_m=e_m + TINY, tol_v=e_v + TINY)


def adamw_sim(p, g, m, v, sc):
    t = lambda x: torch.tensor(x, dtype=F32)
    p, g, m, v = p.float(), g.float(), m.float(), v.float()
    p = p * t(sc["decay"])
    m = m + t(sc["w1"]) * (g - m)
    v = v * t(sc["beta2"]) + (t(sc["w2"]) * g) * g
    den = v.sqrt() / t(sc["bc2_sqrt"]) + t(sc["eps"])
    return (p - t(sc["step_size"]) * (m / den)).double(), m.double(), v.double()


def weight_norm_bwd_ref(dW, v, g):
    """dW, v (H, Hg, k), g (k): dg[t] = <dW_t, v_t> / ||v_t||, dv = (g / ||v_t||) (dW - v <dW_t, v_t> / ||v_t||^2).  The two sums: H Hg
    fmaf terms in a fixed order (N roundings); rsqrtf TRANS; dg one multiply; dv: three multiplies on the correction, the subtraction,
    two multiplies outside."""
    E = E24
    N = v.shape[0] * v.shape[1]
    n2, dot = (v * v).sum((0, 1)), (dW * v).sum((0, 1))
    inv = n2.rsqrt()
    e_dot = N * E * (dW * v).abs().sum((0, 1))
    rr = 0.5 * N * E + TRANS
    dg = dot * inv
    corr = v * dot * inv * inv
    dv = g * inv * (dW - corr)
    e_corr = v.abs() * inv * inv * (e_dot + dot.abs() * (2 * rr + 3 * E))
    return SimpleNamespace(dg=dg, dv=dv, tol_dg=inv * e_dot + dg.abs() * (rr + 2 * E) + TINY,
                           tol_dv=dv.abs() * (rr + 3 * E) + (g * inv).abs() * (e_corr + E * (dW.abs() + corr.abs())) + TINY)


def weight_norm_bwd_sim(dW, v, g):
    dW, v, g = dW.float(), v.float(), g.float()
    n2, dot = (v * v).sum((0, 1)), (dW * v).sum((0, 1))
    inv = n2.rsqrt()
    return (dot * inv).double(), (g * inv * (dW - v * dot * inv * inv)).double()


# ------------------------------------------------------------------------------------------------------------------------------
# data and the case tables shared by the GPU tests and the CPU self-check
# ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gauss(shape, seed, std=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * std).double()


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def norm_inputs(rows, cols, dt, seed, rms=False):
    """stored x, gain, bias, dy (fp64 of the storage type's values)"""
    x = rnd(gauss((rows, cols), seed) + (0.0 if rms else 0.5), dt)
    g = rnd(1.0 + gauss((cols,), seed + 1, 0.1), dt)
    b = rnd(gauss((cols,), seed + 2, 0.1), dt)
    return x, g, b, rnd(gauss((rows, cols), seed + 3), dt)


# LayerNorm backward: cols in units of vec (one active lane, lane 63 idle, a second chunk round of one lane, the 16-wave limit, the first
# size of the general form, the maximum) x rows (one wave, a block less one row, a block and one row, two blocks and one row)
LN_COLS = ["vec", "63vec", "65vec", 1024, "1024+vec", 4096]
LN_ROWS = [1, 15, 17, 33]
RMS_COLS = ["vec", 3072, "3072+vec", 4096]
RMS_ROWS = [1, 5]
DROP_TERM_MAX_COLS = 65 * 8          # above this a single dropped reduction term sinks below the derived accumulation term (the suite's 16 x rule)


def cols_of(spec, dt):
    if isinstance(spec, int):
        return spec
    v = VEC[dt]
    return {"vec": v, "63vec": 63 * v, "65vec": 65 * v, "1024+vec": 1024 + v, "3072+vec": 3072 + v}[spec]


SOFTMAX_COLS = [1, 63, 64, 65, 130]
LOSS_V = [1, 3, 4, 1023, 1024, 1028, 4100]
POOL_KS = [(8, 4), (10, 5), (3, 2), (2, 3), (4, 4)]
CONV0_L = [1, 23, 24, 25, 97]
WN_SHAPES = [(1, 1, 1), (3, 5, 7), (65, 12, 16), (64, 4, 256)]
ADAMW_SIZES = [1, 3, 4, 5, 4095, 4096, 4097]
ADAMW_HYPER = dict(lr=5e-5, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)


def loss_inputs(rows, V, seed, shift=0.0):
    """stored fp32 logits (student, teacher) and labels at 0, V - 1, a 4 i + 3 thread-trip boundary and random places"""
    s = (gauss((rows, V), seed, 2.0) + shift).float().double()
    t = (gauss((rows, V), seed + 1, 2.0) + shift).float().double()
    lab = torch.randint(0, V, (rows,), generator=_gen(seed + 2))
    third = 4099 if V >= 4100 else ((V - 4) // 4 * 4 + 3 if V >= 4 else V - 1)          # (lab >> 2) == i: the last quad, or the second trip's first
    fixed = [0, V - 1, third]
    for i, f in enumerate(fixed[:rows]):
        lab[i] = f
    return s, t, lab


def conv0_inputs(C_, L, r, seed, dt):
    n = 5 * (L - 1) + 10 + r
    wave = gauss((n,), seed, 0.5).float().double()
    w = gauss((C_, 10), seed + 1, 0.4).float().double()
    bias, beta = gauss((C_,), seed + 2, 0.1).float().double(), gauss((C_,), seed + 4, 0.1).float().double()
    gamma = (1.0 + gauss((C_,), seed + 3, 0.1)).float().double()
    dy = rnd(gauss((L, C_), seed + 5), dt)
    init = [ints((C_, 10), -3, 3, seed + 6), ints((C_,), -3, 3, seed + 7), ints((C_,), -3, 3, seed + 8), ints((C_,), -3, 3, seed + 9)]
    return wave, w, bias, gamma, beta, dy, init
