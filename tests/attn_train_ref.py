"""Training-mode attention restated in plain torch, fp64, on the CPU (a helper module of the edge suite, not a conftest).

`attn_train_ref` takes the STORED (already rounded) q, k, v, d_out of one sequence, a visibility matrix and an optional dropout keep mask
and returns the forward's training outputs (O, lse), the backward's (delta, dQ, dK, dV) and, for a storage type with half-ulp u, a bound per
element on what a kernel may return.  Every constant of a bound counts roundings of csrc/attention_bwd.hip ("edge suite",
training mode); none is a measured number.  `packed_inputs` builds the two input families (P: probes, G: Gaussian) of the ragged packed
batches that tests/test_kernel_edges_gpu.py runs on the GPU and tests/test_attn_train_bounds_cpu.py runs through an emulation.
"""
from types import SimpleNamespace

import torch

from conftest import pkg

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}        # half an ulp, relative (as in the edge suite)
BIG = {F16: 60000.0, BF16: 1e30, F32: 1e30}                    # finite poison
E24 = 2.0 ** -24

dropout_keep_at = pkg("ops").dropout_keep_at                   # the one host restatement of common.h dropout_keep


def drop_index(t0, nq, nk, nh):
    """the attention kernels' mask index ((query row * n_heads + head) << 16) | key for buffer rows t0 .. t0 + nq - 1: int64 (nh, nq, nk)"""
    t = torch.arange(t0, t0 + nq, dtype=torch.int64)[None, :, None]
    h = torch.arange(nh, dtype=torch.int64)[:, None, None]
    return ((t * nh + h) << 16) | torch.arange(nk, dtype=torch.int64)[None, None, :]


def visibility(nq, nk, causal):
    """key j visible to query i: j < nk, and under a causal mask j <= i + (nk - nq)"""
    if not causal:
        return torch.ones(nq, nk, dtype=torch.bool)
    return torch.arange(nk)[None, :] <= torch.arange(nq)[:, None] + (nk - nq)


def flat(x):
    """(heads, rows, D) -> (rows, heads * D), the packed layout"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def heads(x, n):
    """(rows, n * D) -> (n, rows, D)"""
    return x.view(x.shape[0], n, -1).transpose(0, 1)


def attn_train_ref(q, k, v, d_out, vis, scale, keep=None, p_drop=0.0, dt=None):
    """q, d_out (nh, nq, D), k, v (nkv, nk, D) fp64; vis (nq, nk) bool; keep (nh, nq, nk) bool or None.  Every row must see a key.
    Returns a namespace of fp64 tensors: P, Pd, O, lse, delta, dS per head; dQ (nh, nq, D); dK, dV (nkv, nk, D), summed over the query
    heads of a GQA group.  With dt: tol_O, tol_dQ, tol_dK, tol_dV, the sets zero_* of outputs that must be exactly zero, and the two derived
    parts of the bound on lse: lse_acc (the scores' fp32 accumulation) and lse_ulp (one fp32 operation after the scores)."""
    nh, nq, D = q.shape
    nkv, nk, _ = k.shape
    rep = nh // nkv
    group = lambda x: x.view(nkv, rep, *x.shape[1:]).sum(1)
    kx, vx = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
    s = ((q @ kx.transpose(1, 2)) * scale).masked_fill(~vis[None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    visk = vis[None].expand(nh, nq, nk) if keep is None else vis[None] & keep
    kf = visk.double() / (1.0 - p_drop) if keep is not None else visk.double()
    Pd = P * kf
    O = Pd @ vx
    delta = (d_out * O).sum(-1)
    dPd = d_out @ vx.transpose(1, 2)
    dS = P * (kf * dPd - delta[..., None]) * scale
    r = SimpleNamespace(P=P, Pd=Pd, O=O, lse=lse, delta=delta, dS=dS, dQ=dS @ kx, dK=group(dS.transpose(1, 2) @ q),
                        dV=group(Pd.transpose(1, 2) @ d_out))
    if dt is None:
        return r
    u = U[dt]
    aq, ak, av, ado = q.abs(), kx.abs(), vx.abs(), d_out.abs()
    qk = aq @ ak.transpose(1, 2)
    # forward (attn_bounds of the edge suite, on Pd): Pd packed to the storage type, the output rounding, subnormal probabilities
    r.tol_O = 2 * u * O.abs() + 4 * u * (Pd @ av) + nk * E24
    r.zero_O = (visk.double() @ av) == 0
    r.lse_acc = scale * D * E24 * qk.masked_fill(~vis[None], 0.0).amax(-1)
    r.lse_ulp = E24 * lse.abs().clamp(min=1.0)
    # backward.  rp: relative error of the recomputed probability exp_scaled(s * scale - lse) (attention_bwd.hip, the `pv` lines of both
    # bodies), every rounding of the exponent x counted once, in units of 2^-24: the score's fp32 accumulation over D terms, its scale
    # multiply, the subtraction and the log2(e) multiply with its rounded constant (2) act on scale |q||k|: D + 4; the fp32 rounding of the
    # lse handed over, the subtraction and the log2(e) multiply (2) act on |lse|: 4; the exponential itself is good to one ulp: 2
    rp = E24 * ((D + 4) * scale * qk + 4 * lse.abs()[..., None] + 2.0)
    m_dV = Pd.transpose(1, 2) @ ado
    r.tol_dV = 2 * u * r.dV.abs() + (4 * u + rep * nq * E24) * group(m_dV) + group((Pd * rp).transpose(1, 2) @ ado) + E24
    mag = scale * P * (kf * (ado @ av.transpose(1, 2)) + delta.abs()[..., None])
    A = 2 * u * dS.abs() + 2 * u * scale * P * (ado * O.abs()).sum(-1)[..., None] + ((D + 4) * E24 + rp) * mag
    r.tol_dQ = 2 * u * r.dQ.abs() + A @ ak + nk * E24 * (dS.abs() @ ak) + E24
    r.tol_dK = 2 * u * r.dK.abs() + group(A.transpose(1, 2) @ aq) + rep * nq * E24 * group(dS.abs().transpose(1, 2) @ aq) + E24
    visd = vis[None].expand(nh, nq, nk).double()
    r.zero_dV = group(visk.double().transpose(1, 2) @ ado) == 0
    r.zero_dQ = (visd @ ak) == 0
    r.zero_dK = group(visd.transpose(1, 2) @ aq) == 0
    return r


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def packed_inputs(family, QL, KL, nh, nkv, D, dt, slack, seed, t0=0):
    """Unrounded fp64 inputs of one ragged packed batch: q, d_out (t0 + sum(QL), nh * D) with t0 rows of filler on top, k, v
    (sum(KL) + slack * len(KL), nkv * D) with `slack` poisoned rows (K 8.0, V large) behind every sequence, and the key offsets cu_k.
      G  q, k, v Gaussian (std 0.5), d_out Gaussian (std 1)
      P  as G, but d_out[i, i mod D] = 1 (else 0) and k[j, j mod D] = 1 (else 0), i and j counted inside the sequence: dV[j, d] is fed
         only by the queries i = d (mod D) that see key j, dQ[i, d] only by the keys j = d (mod D) that query i sees
      V  as G, but v[j, j mod D] = 1 (else 0): out[i, d] is the mass Pd puts on the keys j = d (mod D) (the forward's probe)"""
    g = lambda shape, s, std: (torch.randn(*shape, generator=_gen(seed + s)) * std).double()
    nq_tot, rows_k = t0 + sum(QL), sum(KL) + slack * len(KL)
    q, do = g((nq_tot, nh * D), 1, 0.5), g((nq_tot, nh * D), 2, 1.0)
    k = torch.full((rows_k, nkv * D), 8.0, dtype=torch.float64)
    v = torch.full((rows_k, nkv * D), BIG[dt], dtype=torch.float64)
    cu_k, o, qo = [0], 0, t0
    for n_q, n_k in zip(QL, KL):
        k[o:o + n_k], v[o:o + n_k] = g((n_k, nkv * D), 3 + o, 0.5), g((n_k, nkv * D), 1003 + o, 0.5)
        j, i = torch.arange(n_k), torch.arange(n_q)
        if family == "P":
            k[o:o + n_k], do[qo:qo + n_q] = 0.0, 0.0
            for h in range(nkv):
                k[o + j, h * D + j % D] = 1.0
            for h in range(nh):
                do[qo + i, h * D + i % D] = 1.0
        if family == "V":
            v[o:o + n_k] = 0.0
            for h in range(nkv):
                v[o + j, h * D + j % D] = 1.0
        o += n_k + slack
        qo += n_q
        cu_k.append(o)
    return q, k, v, do, cu_k
