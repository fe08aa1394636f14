"""Token log-probabilities: the definition restated in fp64 torch, HF's three warpers restated, fp32 numpy emulations of the
two summation orders the kernels use, and the rounding bound counted from those orders.

Definition: for row b and step t with chosen token y and s the fp32 score row the selection saw (after the logits processors; after the
temperature / top-k / top-p warpers when sampling), token_logprob[b][t] = log_softmax(s)[y] — transformers'
compute_transition_scores(sequences, scores, normalize_logits=True).  NaN counts as -inf."""
import math

import numpy as np
import torch

NEG_INF = float("-inf")
U = 2.0 ** -24              # fp32 unit roundoff: one rounding is a relative error of at most U
EXP_ULP = 1.0               # expf / logf of the device math library: 1 ulp (ROCm OCML accuracy table); 1 ulp <= 2 U relative
LOG_ULP = 1.0
HIGHER_ORDER = 1.01         # the count below is first order in U; the products of two such terms are below 1 % of it at these sizes


# ------------------------------------------------------------------------------------------------ the definition
def transition_logprobs(scores: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """scores (rows, V) any float dtype, tokens (rows) -> (rows) float64 log_softmax(scores)[token]; NaN counts as -inf"""
    s = scores.double()
    s = torch.where(torch.isnan(s), torch.full_like(s, NEG_INF), s)
    return torch.log_softmax(s, dim=-1).gather(1, tokens.long().view(-1, 1))[:, 0]


def warp(scores: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """HF's TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper (min_tokens_to_keep = 1) on (rows, V), in that order, in fp64:
    filtered tokens at -inf.  top-p keeps token i unless the mass of the tokens ranked above it is already >= top_p."""
    s = scores.double() / float(temperature)
    V = s.shape[-1]
    if 0 < top_k < V:
        kth = torch.topk(s, top_k, dim=-1).values[:, -1:]
        s = torch.where(s < kth, torch.full_like(s, NEG_INF), s)
    if top_p < 1.0:
        srt, idx = torch.sort(s, dim=-1, descending=False)
        cum = torch.softmax(srt, dim=-1).cumsum(dim=-1)
        remove = cum <= (1.0 - top_p)
        remove[:, -1:] = False
        s = s.masked_fill(remove.scatter(1, idx, remove), NEG_INF)
    return s


def sequence_logprobs(step_scores, sequences: torch.Tensor, eos=(), pad_zero: bool = True) -> torch.Tensor:
    """step_scores: one (B, V) tensor per step; sequences (B, n_steps) -> (B, n_steps) float64, 0.0 at and after a row's finish"""
    B, T = sequences.shape
    out = torch.zeros(B, T, dtype=torch.float64)
    live = [True] * B
    for t_, s in enumerate(step_scores):
        lp = transition_logprobs(s, sequences[:, t_])
        for b in range(B):
            if live[b] or not pad_zero:
                out[b, t_] = lp[b]
            if live[b] and int(sequences[b, t_]) in eos:
                live[b] = False
    return out


# ------------------------------------------------------------------------------------------------ fp32 emulations of the two orders
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _clean(x):
    x = _f32(x).copy()
    x[np.isnan(x)] = -np.inf
    return x


def _butterfly(v, width, offsets):
    """xor butterfly over groups of `width` consecutive lanes of v (..., lanes): every lane adds its partner's value, in fp32"""
    lanes = np.arange(v.shape[-1])
    for o in offsets:
        v = _f32(v + v[..., lanes ^ o])
    return v


def row_scan_lse_f32(x, threads: int = 1024, subtract_max: bool = True):
    """common.h sl_row_max_lse over one row: -> (m, ls) float32.  Per-thread partial sums in index order (16-byte groups of four when
    V % 4 == 0), xor butterfly 32..1 inside each wave, the waves added in order.  subtract_max=False is the WRONG form exp(x) summed raw."""
    x = _clean(x)
    V = x.shape[0]
    m = np.float32(x.max())
    if m == -np.inf:
        m = np.float32(0.0)
    shift = m if subtract_max else np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(_f32(x - shift), dtype=np.float32)
    if V % 4 == 0:
        n4 = V // 4
        steps = -(-n4 // threads)
        grid = np.zeros((steps, threads, 4), dtype=np.float32)
        idx = np.arange(steps * threads)
        ok = idx < n4
        grid.reshape(-1, 4)[ok] = e.reshape(n4, 4)
        seq = grid.transpose(1, 0, 2).reshape(threads, steps * 4)           # thread t: float4 t, t + threads, ... each in element order
    else:
        steps = -(-V // threads)
        grid = np.zeros(steps * threads, dtype=np.float32)
        grid[:V] = e
        seq = grid.reshape(steps, threads).T
    part = np.zeros(threads, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(seq.shape[1]):
            part = _f32(part + seq[:, k])
        waves = _butterfly(part.reshape(threads // 64, 64), 64, (32, 16, 8, 4, 2, 1))[:, 0]
        total = np.float32(0.0)
        for w in waves:
            total = np.float32(total + w)
        ls = np.log(total, dtype=np.float32) if total > 0 else np.float32(-np.inf)
    return m, np.float32(ls)


def row_logprob_f32(x, token: int, subtract_max: bool = True) -> np.float32:
    """greedy_select_kernel<SC>: (x[token] - m) - ls.  subtract_max=False (wrong): x[token] - log(sum exp(x))"""
    x = _clean(x)
    m, ls = row_scan_lse_f32(x, subtract_max=subtract_max)
    with np.errstate(over="ignore", invalid="ignore"):
        if not subtract_max:
            return np.float32(x[token] - ls)
        return np.float32(np.float32(x[token] - m) - ls)


def group_planes_f32(x):
    """tile_argmax on one row: -> (max_g, sum_g) float32 (ceil(V / 64)).  Lane r of the 16 holds columns r, 16 + r, 32 + r, 48 + r of the
    group and adds them in that order; xor butterfly 1, 2, 4, 8 over the 16 lanes."""
    x = _clean(x)
    V = x.shape[0]
    ng = -(-V // 64)
    pad = np.full(ng * 64, -np.inf, dtype=np.float32)
    pad[:V] = x
    g = pad.reshape(ng, 4, 16)                                              # [group][fragment n][lane r]
    gmax = g.reshape(ng, 64).max(axis=1)
    with np.errstate(invalid="ignore"):
        e = np.exp(_f32(g - gmax[:, None, None]), dtype=np.float32)
    e[np.isnan(e)] = 0.0                                                    # a group of nothing but -inf: sum 0
    lane = np.zeros((ng, 16), dtype=np.float32)
    for n in range(4):
        lane = _f32(lane + e[:, n, :])
    gsum = _butterfly(lane, 16, (1, 2, 4, 8))[:, 0]
    gsum[gmax == -np.inf] = 0.0
    return _f32(gmax), _f32(gsum)


def partial_logprob_f32(gmax, gsum, rescale: bool = True) -> np.float32:
    """greedy_select_partial_kernel<SC> on one row's planes: stripe s adds sum_g * exp(max_g - Mx) over g = s, s + 32, ... in order, the 32
    stripes are added in order; -> -log(total).  rescale=False is the WRONG form that takes every group's own maximum for the row's."""
    gmax, gsum = _f32(gmax), _f32(gsum)
    mx = np.float32(gmax.max())
    stripes = np.zeros(32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(gmax.shape[0]):
            if gmax[g] == -np.inf:
                continue
            w = np.exp(np.float32(gmax[g] - mx), dtype=np.float32) if rescale else np.float32(1.0)
            stripes[g % 32] = np.float32(stripes[g % 32] + np.float32(gsum[g] * w))
        total = np.float32(0.0)
        for s in stripes:
            total = np.float32(total + s)
        return np.float32(-np.log(total, dtype=np.float32)) if total > 0 else np.float32(np.inf)


# ------------------------------------------------------------------------------------------------ the rounding bound
def _row_stats(x, token):
    """fp64: A = sum p_i |x_i - m| (how much a relative rounding of the exponent's argument moves the sum), ls = log sum exp(x - m), and the
    token's log-probability"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    m = x.max()
    d = x - m
    e = np.exp(d)
    S = e.sum()
    fin = np.isfinite(d)
    A = float((e[fin] * np.abs(d[fin])).sum() / S)
    ls = math.log(S)
    return A, ls, float(d[token] - ls), float(abs(d[token]))


def chain_row(V: int, threads: int = 1024) -> int:
    """longest chain of additions of the row scan: a thread's elements, 6 butterfly levels, 16 waves"""
    per_thread = 4 * (-(-(V // 4) // threads)) if V % 4 == 0 else -(-V // threads)
    return per_thread + 6 + threads // 64


def chain_partial(V: int) -> int:
    """... of the select pass over the planes: a stripe's groups, then the 32 stripes"""
    return -(-(-(-V // 64)) // 32) + 32


def bound_group_sum(x_group) -> float:
    """relative bound of one group's sum_g: per term the rounding of v - max_g (U |v - max_g|, weighted: A) and expf (2 U EXP_ULP); 4 in-lane
    additions and 4 butterfly levels"""
    x = np.asarray(x_group, dtype=np.float64)
    x = x[~np.isnan(x)]
    A, _, _, _ = _row_stats(x, 0)
    return HIGHER_ORDER * U * (A + 2 * EXP_ULP + 8)


def bound_row(x, token) -> float:
    """absolute bound of (x[token] - m) - logf(sum expf(x - m)) in the row-scan order"""
    A, ls, lp, dt = _row_stats(x, token)
    V = len(x)
    return HIGHER_ORDER * U * (A + 2 * EXP_ULP + chain_row(V) + 2 * LOG_ULP * abs(ls) + dt + abs(lp))


def bound_partial(x, token=None) -> float:
    """absolute bound of -logf(sum_g sum_g expf(max_g - Mx)): the group sums (A_g + 2 + 8), the rescale (rounding of max_g - Mx: A_s, expf:
    2, the product: 1), the stripe and cross-stripe chains, logf.  |v - max_g| + |max_g - Mx| = |v - Mx|, so A_g + A_s = A of the row."""
    A, ls, _, _ = _row_stats(x, int(np.nanargmax(np.asarray(x, dtype=np.float64))))
    V = len(x)
    return HIGHER_ORDER * U * (A + 2 * EXP_ULP + 8 + 2 * EXP_ULP + 1 + chain_partial(V) + 2 * LOG_ULP * abs(ls))


def bound_sample(warped, token, threads: int = 1024) -> float:
    """absolute bound of logf(p / z) in sample_rows_kernel, `warped` the fp64 warped scores (a = (x - m) / T per survivor).  p = __expf(a):
    the argument carries three roundings of its own (x - m, 1 / T, the product) and the fast exponential two more of the argument (the
    multiplication by log2 e) plus 2 ulp: 5 U |a| + 4 U.  z: a thread's slice in order, then the 1 024 slices in order.  One division, logf."""
    A, ls, lp, dt = _row_stats(warped, token)
    V = len(warped)
    chain = -(-V // threads) + threads
    return HIGHER_ORDER * U * (5 * A + 4 + chain + 5 * dt + 4 + 1 + 2 * LOG_ULP * abs(lp))


def bound_greedy_any(V: int) -> float:
    """bound_row + bound_partial for the GREEDY token of any row of V scores, without the data: d_i = log p_i + ls, so A = sum p_i |d_i| <=
    the entropy <= ln V; 0 <= ls <= ln V; the maximum's log-probability lies in [-ln V, 0] and its |x - m| is 0.  What two runs that saw
    the same scores, one through each form, may differ by."""
    lv = math.log(V)
    A_any = lv
    row = HIGHER_ORDER * U * (A_any + 2 * EXP_ULP + chain_row(V) + 2 * LOG_ULP * lv + lv)
    part = HIGHER_ORDER * U * (A_any + 2 * EXP_ULP + 8 + 2 * EXP_ULP + 1 + chain_partial(V) + 2 * LOG_ULP * lv)
    return row + part


def group_sums_reference(logits: torch.Tensor):
    """logits (M, N) fp32 as the epilogue saw them -> (S, rel_bound, dead), each (ceil(N / 64), M): the fp64 sum over the group's valid columns
    of exp(v - group max), bound_group_sum for every group at once, and the groups whose maximum is -inf (their plane entry is 0)"""
    M, N = logits.shape
    ng = (N + 63) // 64
    x = logits.double()
    x = torch.where(torch.isnan(x), torch.full_like(x, NEG_INF), x)
    x = torch.cat([x, torch.full((M, ng * 64 - N), NEG_INF, dtype=torch.float64, device=x.device)], dim=1).view(M, ng, 64)
    gmax = x.max(dim=2).values
    dead = torch.isinf(gmax) & (gmax < 0)
    d = x - torch.where(dead, torch.zeros_like(gmax), gmax)[:, :, None]
    e = torch.exp(d)
    S = e.sum(dim=2)
    w = torch.where(torch.isfinite(d), e * d.abs(), torch.zeros_like(e)).sum(dim=2)
    A = torch.where(dead, torch.zeros_like(S), w / S.clamp(min=1e-300))
    rel = HIGHER_ORDER * U * (A + 2 * EXP_ULP + 8)
    return S.T.contiguous(), rel.T.contiguous(), dead.T.contiguous()
