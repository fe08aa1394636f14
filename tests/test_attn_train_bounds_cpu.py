"""CPU: the per-element bounds of tests/attn_train_ref.py are neither too tight nor too loose.

An emulation of csrc/attention_bwd.hip's rounding points in fp32 torch (P and dS rounded to bf16 where pack_step packs them, `out` and the
results rounded to bf16, lse handed over in fp32, every product accumulated in fp32) must stay inside the bounds on every input family of
the GPU cases (a), and four wrong emulations - the slips the GPU cases are there to catch - must each leave them, or break an exact zero,
on at least one family (b).  No number here is measured: the worst err / tol that (a) prints is recorded in DESIGN.md.
"""
import functools

import pytest
import torch

import attn_train_ref as R

BF16 = torch.bfloat16
QL, KL, SLACK = [70, 1, 260, 33, 129], [200, 64, 300, 33, 129], 5          # the edge suite's ragged set
P_DROP, SEED = 0.25, 0x1234_5678_9ABC_DEF1
# name: (family, D, nh, nkv, causal, dropout, QL, KL, first buffer row)
FAMILIES = {f"{fam}-D{D}-{'causal' if c else 'full'}{'-drop' if dr else ''}": (fam, D, nh, nkv, c, dr, QL, KL, 0)
            for fam in "PG" for D, nh, nkv in ((64, 4, 4), (128, 6, 2)) for c in (False, True) for dr in (False, True)}
FAMILIES["G-crossing"] = ("G", 64, 64, 64, False, True, [70], [70], 1000)          # (row * 64 + head) passes 65 536 at query 24
FAMILIES["P-crossing"] = ("P", 64, 64, 64, False, True, [70], [70], 1000)
TQ = {64: 64, 128: 32}                                                   # the bf16 dK / dV kernels' query tile


def rb(x):
    return x.to(BF16).float()


def emulate(q, k, v, do, out, lse, vis, scale, keep_q, keep_kv, p, no_drop_scale=False):
    """fp32 restatement of the two block bodies on one sequence: (dq, dk, dv) in fp64 of the bf16 results.  keep_q is the mask the dQ
    body derives, keep_kv the one the dK / dV body derives (the same bits in a correct kernel)."""
    nh, nq, D = q.shape
    nkv = k.shape[0]
    rep = nh // nkv
    group = lambda x: x.view(nkv, rep, *x.shape[1:]).sum(1)
    kx, vx = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
    delta = (do * out).sum(-1)
    P = torch.where(vis[None], torch.exp((q @ kx.transpose(1, 2)) * scale - lse[..., None]), torch.zeros(()))
    dP = do @ vx.transpose(1, 2)
    ds = 1.0 / (1.0 - p)
    res = []
    for keep in (keep_q, keep_kv):
        pd, dpv = P, dP
        if keep is not None:
            pd = torch.where(keep, P * ds, torch.zeros(()))
            dpv = torch.where(keep, dP if no_drop_scale else dP * ds, torch.zeros(()))
        res.append((rb(pd), rb(P * (dpv - delta[..., None]) * scale)))
    dq = rb(res[0][1] @ kx)
    dk = rb(group(res[1][1].transpose(1, 2) @ q))
    dv = rb(group(res[1][0].transpose(1, 2) @ do))
    return dq.double(), dk.double(), dv.double()


@functools.lru_cache(maxsize=None)
def family_data(name):
    """per sequence: the stored inputs, visibility, mask indices and bits, and the fp64 reference with its bounds (computed once)"""
    fam, D, nh, nkv, causal, drop, ql, kl, t0 = FAMILIES[name]
    scale, p = D ** -0.5, (P_DROP if drop else 0.0)
    q_, k_, v_, do_, cu_k = R.packed_inputs(fam, ql, kl, nh, nkv, D, BF16, SLACK, seed=900, t0=t0)
    q_, k_, v_, do_ = [x.float().to(BF16).double() for x in (q_, k_, v_, do_)]          # the stored values
    seqs, qo = [], t0
    for i, (nq, nk) in enumerate(zip(ql, kl)):
        q, do = R.heads(q_[qo:qo + nq], nh), R.heads(do_[qo:qo + nq], nh)
        k, v = R.heads(k_[cu_k[i]:cu_k[i] + nk], nkv), R.heads(v_[cu_k[i]:cu_k[i] + nk], nkv)
        vis = R.visibility(nq, nk, causal)
        idx = R.drop_index(qo, nq, nk + 1, nh)
        keep = R.dropout_keep_at(idx, p, SEED) if drop else None
        ref = R.attn_train_ref(q, k, v, do, vis, scale, None if keep is None else keep[..., :nk], p, dt=BF16)
        seqs.append((qo, nq, nk, q, k, v, do, vis, idx, keep, ref))
        qo += nq
    return seqs


def run_family(name, wrong=None):
    """-> (worst err / tol over dQ, dK, dV of every sequence, number of exact zeros broken)"""
    fam, D, nh, nkv, causal, drop, ql, kl, t0 = FAMILIES[name]
    scale, p = D ** -0.5, (P_DROP if drop else 0.0)
    worst, broken = 0.0, 0
    for qo, nq, nk, q, k, v, do, vis, idx, keep, ref in family_data(name):
        vis_e, keep_q, keep_kv, k_e, v_e = vis, keep, keep, k, v
        if wrong == "causal_lt" and causal:
            vis_e = torch.arange(nk)[None, :] < torch.arange(nq)[:, None] + (nk - nq)
        if wrong == "inner0" and drop:          # the dK / dV body takes the upper counter word of the tile's first query for every query
            first = qo + torch.arange(nq) // TQ[D] * TQ[D]
            hi = ((first[None, :, None] * nh + torch.arange(nh)[:, None, None]) >> 16) << 32
            keep_kv = R.dropout_keep_at((idx & 0xFFFFFFFF) | hi, p, SEED)
        if wrong == "klen_le":                  # key klen passes the mask; its loads are clamped to row klen - 1, its dK / dV row is not stored
            k_e, v_e = torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1)
            vis_e = torch.cat([vis, torch.full((nq, 1), not causal)], 1)
        else:
            keep_q = None if keep_q is None else keep_q[..., :nk]
            keep_kv = None if keep_kv is None else keep_kv[..., :nk]
        f = lambda x: x.float()
        dq, dk, dv = emulate(f(q), f(k_e), f(v_e), f(do), rb(ref.O.float()), ref.lse.float(), vis_e, scale, keep_q, keep_kv, p,
                             no_drop_scale=wrong == "no_drop_scale")
        dk, dv = dk[:, :nk], dv[:, :nk]
        for got, want, tol, zero in ((dq, ref.dQ, ref.tol_dQ, ref.zero_dQ), (dk, ref.dK, ref.tol_dK, ref.zero_dK), (dv, ref.dV, ref.tol_dV, ref.zero_dV)):
            worst = max(worst, float(((got - want).abs() / tol).max()))
            broken += int((got[zero] != 0).sum())
    return worst, broken


@pytest.mark.parametrize("name", list(FAMILIES))
def test_emulated_kernel_stays_inside_the_bounds(name):
    worst, broken = run_family(name)
    print(f"{name}: worst emulated err / tol {worst:.3f}")
    assert broken == 0 and worst < 1.0


@pytest.mark.parametrize("wrong", ["causal_lt", "klen_le", "no_drop_scale", "inner0"])
def test_wrong_emulation_leaves_the_bounds(wrong):
    rejected = []
    for name in FAMILIES:
        worst, broken = run_family(name, wrong)
        if broken or worst >= 1.0:
            rejected.append(f"{name}: err / tol {worst:.3g}, {broken} exact zeros broken")
    print(f"{wrong}: rejected on {len(rejected)} of {len(FAMILIES)} families\n  " + "\n  ".join(rejected))
    assert rejected, f"the bounds accept the wrong emulation '{wrong}' on every family"


def test_dropout_keep_mask_is_dropout_keep_at_on_a_range():
    """one host restatement: ops.dropout_keep_mask(n) is dropout_keep_at(arange(n)), and the bits are those of the restatement the suite
    has always used (written out again here), on 2^20 indices and two seeds; an index above 2^32 uses its upper word"""
    import numpy as np
    ops = R.pkg("ops")
    m32 = np.uint64(0xFFFFFFFF)

    def lowbias32(x):
        x = x & m32
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & m32
        x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & m32
        return x ^ (x >> np.uint64(16))

    n = 1 << 20
    for seed, p in ((0x0123_4567_89AB_CDEF, 0.25), (7, 0.1)):
        i = np.arange(n, dtype=np.uint64)
        h = lowbias32((i & m32) ^ lowbias32((i >> np.uint64(32)) ^ np.uint64(seed & 0xFFFFFFFF)) ^ np.uint64(seed >> 32))
        want = torch.from_numpy((h >> np.uint64(8)) >= np.uint64(int(float(np.float32(p)) * 16777216.0)))
        assert torch.equal(ops.dropout_keep_mask(n, p, seed), want)
        assert torch.equal(ops.dropout_keep_at(torch.arange(n), p, seed), want)
        assert abs(float(want.double().mean()) - (1 - p)) < 5e-3
        lo = torch.arange(n, dtype=torch.int64)
        assert not torch.equal(ops.dropout_keep_at(lo | (1 << 32), p, seed), want)
