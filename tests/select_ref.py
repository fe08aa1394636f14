"""Token selection by sampling: sample_rows_kernel restated in fp64 numpy with what it owes per draw, the inputs the CPU and
GPU tests share, and an fp32 emulation of the kernel that takes planted defects.

Survivor set, as the kernel defines it (NaN counts as -inf everywhere):
  temperature   scores / T (T > 0: the order of the scores is the order of the logits);
  top-k         keep every score >= the k-th largest; ties at the k-th score ALL stay; top_k = 0 or top_k >= V: no top-k;
  top-p         on the top-k survivors: token i is dropped iff the mass of the tokens with a STRICTLY LARGER score is >= top_p, so equal
                scores share their fate.  HF's TopPLogitsWarper sorts and cuts inside a run of equal scores wherever the sort put the cut;
                the two agree wherever no tie sits on the top-p boundary, and only there.
A token of mass zero (-inf, NaN) is never a survivor.

Class E (the exact draw): every survivor has the row's maximum score and every other mass is exactly 0, so every probability is exactly 1
(__expf(0) == 1), z is the integer count n and the pick is survivor number min(floor(fl32(u * n)), n - 1) in index order.
Class G (the interval per draw): the pick i is accepted iff  C_{i-1} - u Z <= 2 eta Z  and  C_i - u Z > -2 eta Z  (accept_rule)."""
import math

import numpy as np
import torch

import token_scores_ref as tsr
from token_scores_ref import EXP_ULP, HIGHER_ORDER, U   # noqa: F401  (EXP_ULP: the 4 of eta is 2 argument roundings + 2 EXP_ULP)

THREADS = 1024
sampled_logprob_bound = tsr.bound_sample


# ------------------------------------------------------------------------------------------------ the survivor set
def clean(x):
    """fp32 row -> fp64, NaN counted as -inf"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    return x


def survivors(x, temperature=1.0, top_k=0, top_p=1.0):
    """one row of fp32 logits -> (keep (V) bool, warped (V) fp64 with -inf at the dropped tokens, margins (n) fp64): margins holds, for
    every top-k survivor of mass above zero, |mass of the strictly larger scores - top_p| (empty without top-p)"""
    x = clean(x)
    V = x.shape[0]
    keep = np.isfinite(x)
    if 0 < top_k < V:
        kth = np.sort(x)[V - top_k]
        keep &= x >= kth
    m = x.max()
    a = (x - (m if np.isfinite(m) else 0.0)) / float(temperature)
    with np.errstate(invalid="ignore"):
        p = np.where(keep, np.exp(a), 0.0)
    margins = np.zeros(0)
    if top_p < 1.0 and keep.any():
        idx = np.flatnonzero(keep)
        order = idx[np.argsort(-x[idx], kind="stable")]
        ps = p[order] / p[order].sum()
        before = np.concatenate([[0.0], np.cumsum(ps)[:-1]])               # mass ranked above, ties split ...
        xs = x[order]
        first = np.concatenate([[True], xs[1:] != xs[:-1]])
        above = before[np.maximum.accumulate(np.where(first, np.arange(len(xs)), 0))]   # ... and shared: the first of the run decides
        margins = np.abs(above - top_p)
        keep = keep.copy()
        keep[order[above >= top_p]] = False
    warped = np.where(keep, a, -np.inf)
    return keep, warped, margins


def hf_split_ties(x, temperature, top_k, top_p):
    """the survivor set with ties SPLIT at the top-p boundary, in index order inside a run of equal scores — what a sort-based top-p does
    (a planted defect)"""
    x = clean(x)
    keep, _, _ = survivors(x, temperature, top_k, 1.0)
    idx = np.flatnonzero(keep)
    order = idx[np.argsort(-x[idx], kind="stable")]
    p = np.exp((x[order] - x.max()) / float(temperature))
    before = np.concatenate([[0.0], np.cumsum(p / p.sum())[:-1]])
    keep[order[before >= top_p]] = False
    return keep


# ------------------------------------------------------------------------------------------------ the uniforms
def uniforms(sample_uniform, seed, gen, rows=None):
    """u of every row of one launch: row b draws at (seed, b, gen[b]) -> (B) fp64 (each exactly a multiple of 2^-24)"""
    rows = range(len(gen)) if rows is None else rows
    return np.array([sample_uniform(seed, int(r), int(g)) for r, g in zip(rows, gen)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ class E
def is_class_e(x, keep):
    """every survivor holds the row's maximum, and every other mass the kernel adds is exactly zero or filtered"""
    x = clean(x)
    return bool(keep.any()) and bool((x[keep] == x.max()).all())


def class_e_ordinal(u, n):
    """survivor number of the draw: min(floor(fl32(u * n)), n - 1), in numpy.float32"""
    target = np.asarray(u, dtype=np.float32) * np.float32(n)
    return np.minimum(np.floor(target).astype(np.int64), n - 1)


def class_e_pick(u, keep):
    idx = np.flatnonzero(keep)
    return idx[class_e_ordinal(u, len(idx))]


def class_e_walk(u, counts):
    """brute force: the kernel's two-level walk on a class E row whose thread t owns counts[t] survivors (THREADS entries), all masses 1.
    The parts are added in thread order, then the slice is walked; every sum is an integer below 2^24, so fp32 holds each exactly and the
    compares below are the kernel's.  -> survivor number per u."""
    counts = np.asarray(counts, dtype=np.int64)
    cum = np.cumsum(counts).astype(np.float32)                              # run + part[t], t = 0 ..
    n = int(counts.sum())
    target = np.asarray(u, dtype=np.float32) * np.float32(n)               # u * z
    t = np.minimum(np.searchsorted(cum[:THREADS - 1], target, side="right"), THREADS - 1)      # first t < 1023 with run + part[t] > target
    run = np.concatenate([[0], np.cumsum(counts)])[t]                      # survivors before slice t
    inside = np.floor(target.astype(np.float64) - run).astype(np.int64)     # first j with run + (j + 1) > target
    short = inside >= counts[t]                                             # the walk ran off the slice: `last`
    return np.where(short, run + counts[t] - 1, run + inside)


# ------------------------------------------------------------------------------------------------ class G
def eta(warped):
    """relative bound of a partial sum of the kernel's masses and of its z.  Per term: the argument (x - m) * (1 / T) carries three
    roundings and the fast exponential two more of the argument plus 2 ulp — 5 U |a| + 4 U, weighted by mass: 5 A + 4 (bound_sample's
    count); the longest addition chain, a thread's slice then the 1 024 parts in order: ceil(V / 1024) + 1024; one rounding for u * z."""
    A = tsr._row_stats(warped, int(np.argmax(warped)))[0]
    V = len(warped)
    return HIGHER_ORDER * U * (5 * A + 4 + (-(-V // THREADS) + THREADS) + 1)


def cdf(warped):
    """-> (idx, C, Z): the survivors in index order, their cumulative masses (C[j] includes survivor j) and the total, fp64"""
    idx = np.flatnonzero(np.isfinite(warped))
    C = np.cumsum(np.exp(warped[idx] - warped[idx].max()))
    return idx, C, float(C[-1])


def accept_rule(warped, u):
    """-> (idx, ok (draws, n) bool, dist (draws, n)): survivor j is an acceptable pick of draw d iff C_{j-1} - u Z <= 2 eta Z and
    C_j - u Z > -2 eta Z; dist is how far outside its own interval [C_{j-1}, C_j) the draw sits, in units of 2 eta Z (0 inside)"""
    idx, C, Z = cdf(warped)
    e2 = 2.0 * eta(warped)
    lo = (np.concatenate([[0.0], C[:-1]])[None, :] - np.asarray(u)[:, None] * Z) / Z
    hi = (C[None, :] - np.asarray(u)[:, None] * Z) / Z
    ok = (lo <= e2) & (hi > -e2)
    dist = np.maximum(np.maximum(lo, 0.0), np.maximum(-hi, 0.0)) / e2
    return idx, ok, dist


def check_draws(warped, u, picks):
    """every pick is a survivor and inside its interval -> (message or "", worst distance / (2 eta) over the draws)"""
    idx, ok, dist = accept_rule(warped, u)
    pos = {int(i): j for j, i in enumerate(idx)}
    worst = 0.0
    for d, tok in enumerate(np.asarray(picks).tolist()):
        if tok not in pos:
            return f"draw {d}: token {tok} is no survivor", worst
        j = pos[tok]
        if not ok[d, j]:
            return f"draw {d} (u = {u[d]!r}): token {tok} sits {dist[d, j]:.3g} x 2 eta outside its interval", worst
        worst = max(worst, float(dist[d, j]))
    return "", worst


# ------------------------------------------------------------------------------------------------ fp32 emulation with planted defects
DEFECTS = ("slice_off_by_one", "sorted_cdf", "ge_in_walk", "u_row_plus_1", "u_step_plus_1", "nan_takes_seat", "ties_split")


def emulate(x, temperature, top_k, top_p, u, defect=None, keep=None):
    """sample_rows_kernel on one fp32 row at every u of `u` -> picks (draws).  The filter is the reference survivor set; the masses, the
    slice sums, z, u * z and the two-level walk are fp32 in the kernel's order (numpy's expf stands in for the fast exponential).
    defect: one of DEFECTS that concerns one row (the two u_* defects are the caller's: it hands in the wrong u)."""
    x32 = np.asarray(x, dtype=np.float32)
    V = x32.shape[0]
    if defect == "nan_takes_seat":
        seat = np.where(np.isnan(x32), np.float32(3.0e38), x32)            # ord_key(+NaN) is above every number
        keep, _, _ = survivors(seat, temperature, top_k, top_p)
        keep &= ~np.isnan(x32)                                              # its mass is no number; the emulation gives it none
    elif defect == "ties_split":
        keep = hf_split_ties(x32, temperature, top_k, top_p)
    elif keep is None:
        keep, _, _ = survivors(x32, temperature, top_k, top_p)
    xc = np.where(np.isnan(x32), np.float32(-np.inf), x32)
    m = xc.max()
    with np.errstate(invalid="ignore"):
        p = np.exp((xc - m) * np.float32(1.0 / np.float32(temperature)), dtype=np.float32)
    p = np.where(keep, p, np.float32(0.0)).astype(np.float32)
    perm = np.arange(V)
    if defect == "sorted_cdf":
        perm = np.argsort(-xc, kind="stable")
        p, keep = p[perm], keep[perm]
    Cn = -(-V // THREADS)
    pad = np.zeros(THREADS * Cn, dtype=np.float32)
    pad[:V] = p
    part = np.cumsum(pad.reshape(THREADS, Cn), axis=1, dtype=np.float32)[:, -1]
    cum = np.cumsum(part, dtype=np.float32)
    z = cum[-1]
    before = np.concatenate([np.zeros(1, dtype=np.float32), cum[:-1]])
    ge = defect == "ge_in_walk"
    picks = []
    for uu in np.asarray(u, dtype=np.float32):
        target = np.float32(uu * z)
        hit = (cum[:THREADS - 1] >= target) if ge else (cum[:THREADS - 1] > target)
        t = int(np.argmax(hit)) if hit.any() else THREADS - 1
        j0 = t * Cn + (1 if defect == "slice_off_by_one" else 0)
        j1 = min(j0 + Cn, V)
        pick = last = -1
        if j0 < j1:
            run = np.cumsum(np.concatenate([before[t:t + 1], p[j0:j1]]), dtype=np.float32)[1:]
            live = keep[j0:j1] & (p[j0:j1] > 0)
            over = ((run >= target) if ge else (run > target)) & keep[j0:j1]
            if over.any():
                pick = j0 + int(np.argmax(over))
            elif live.any():
                last = j0 + int(np.flatnonzero(live)[-1])
        if pick < 0:
            pick = last
        if pick < 0:
            pick = int(np.argmax(keep)) if keep.any() else 0
        picks.append(int(perm[pick]))
    return np.array(picks, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the shared inputs
B = 256
MAX_NEW = 4
SEED = 0xABCDEF0123


def gen_counts(rows=B):
    """gen_count varied per row, every value below MAX_NEW"""
    return [(3 * b + b // 7) % MAX_NEW for b in range(rows)]


def gauss_row(V, r=0):
    """row r of the six Gaussian rows (std 2.5, seed 51) test_sample_select_follows_hf_logits_warpers draws at this V"""
    return (torch.randn(6, V, generator=torch.Generator().manual_seed(51)) * 2.5)[r].numpy().copy()


def with_holes(x, seed=52):
    """-inf at 5 % of the indices, as the logits processors leave a row"""
    x = np.array(x, dtype=np.float32)
    holes = torch.randperm(len(x), generator=torch.Generator().manual_seed(seed))[:max(1, len(x) // 20)].numpy()
    x[holes] = -np.inf
    return x


# name -> (V, temperature, top_k, top_p, row of gauss_row); each also runs with with_holes(row) under name + "_holes".  The row is the
# first of the six whose top-p decisions, with and without the holes, all keep a margin of 1e-3 (a property of the input, asserted in
# tests/test_select_ref_cpu.py): closer than that the fp32 masses may decide a boundary the other way and no reference could say which.
G_CASES = {"v128256_t06_k50_p09": (128256, 0.6, 50, 0.9, 0), "v1000_p075": (1000, 1.0, 0, 0.75, 2), "v1000_t13_k7": (1000, 1.3, 7, 1.0, 0),
           "v1025_t07_k20_p09": (1025, 0.7, 20, 0.9, 0)}


def g_case(name):
    """-> (row fp32 (V), temperature, top_k, top_p)"""
    holes = name.endswith("_holes")
    V, T, k, p, r = G_CASES[name[:-len("_holes")] if holes else name]
    row = gauss_row(V, r)
    return (with_holes(row) if holes else row), T, k, p


G_NAMES = [n + s for n in G_CASES for s in ("", "_holes")]


# small survivor sets: name -> (row, temperature, top_k, top_p, the survivor set).  Masses are powers of two times 1/16 so that the
# top-p decisions are exact: exp(ln 2 * j) in fp64 is within 1e-15 of 2^j, the margins are at least 1/16.
def _ln2(js, V, where):
    x = np.full(V, -30.0, dtype=np.float32)
    for j, i in zip(js, where):
        x[i] = np.float32(math.log(2.0) * j)
    return x


def set_cases():
    out = {}
    # a tie at the k-th score: top_k = 3 keeps four tokens
    out["tie_at_kth"] = (_ln2([3, 2, 1, 1, 0], 1030, [1029, 0, 512, 1024, 7]), 1.0, 3, 1.0, {1029, 0, 512, 1024})
    # masses 8 4 4 2 1 1 over 20: above = 0, .4, .4, .8, .9, .9; top_p = 0.5 keeps the tied pair (a sort-based cut keeps one of the two)
    x = _ln2([3, 2, 2, 1, 0, 0], 2049, [5, 1023, 1024, 2048, 0, 77])
    x[(x == -30.0)] = -np.inf
    out["tie_across_top_p"] = (x, 1.0, 0, 0.5, {5, 1023, 1024})
    # both filters, temperature 2 on doubled scores: top_k = 8 keeps masses 16 8 8 4 4 2 2 2 of 46, above = 0, .35, .35, .70, .70, .87 ..;
    # top_p = 0.8 then drops the three of mass 2
    js = [4, 3, 3, 2, 2, 1, 1, 1, 0, 0]
    where = [3, 64, 65, 1000, 4099, 2, 1001, 2047, 2048, 9]
    x = _ln2([2 * j for j in js], 4100, where)
    out["k8_p08_t2"] = (x, 2.0, 8, 0.8, set(where[:5]))
    # a NaN where a top-k seat would be, and two more: top_k = 4 keeps the four largest NUMBERS
    x = _ln2([5, 4, 3, 2, 1], 1000, [10, 999, 500, 0, 300])
    x[[20, 501, 998]] = np.nan
    out["nan_in_the_seats"] = (x, 1.0, 4, 1.0, {10, 999, 500, 0})
    return out


def covering_seed(sample_uniform, wants, gen, start=1):
    """the first seed >= start at which, for every (warped row) of `wants`, each survivor's interval [C_{j-1}, C_j) / Z, shrunk by
    2 eta on either side, holds the u of some row of the launch: then the set of drawn tokens must EQUAL the survivor set"""
    for seed in range(start, start + 4096):
        u = uniforms(sample_uniform, seed, gen)
        good = True
        for w in wants:
            idx, C, Z = cdf(w)
            e2 = 2.0 * eta(w)
            lo, hi = np.concatenate([[0.0], C[:-1]]) / Z + e2, C / Z - e2
            if not all(bool(((u >= a) & (u < b)).any()) for a, b in zip(lo, hi)):
                good = False
                break
        if good:
            return seed
    raise AssertionError("no covering seed")


# ------------------------------------------------------------------------------------------------ class E inputs
E_SIZES = [1, 3, 64, 1023, 1024, 1025, 2049, 4100, 128256]
E_SCORES = (2.5, 0.0, -1.5)                                 # the common score: both branches of ord_key, and zero
N_PATTERNS = 8


def e_pattern(V, which):
    """the survivor indices of pattern `which` at V (slices of Cn = ceil(V / 1024) elements)"""
    Cn = -(-V // THREADS)
    starts = np.arange(0, V, Cn)
    if which == 0:
        idx = [0]                                                           # a single survivor at index 0
    elif which == 1:
        idx = [V - 1]                                                       # ... at V - 1
    elif which == 2:
        idx = [min(Cn * min(517, len(starts) - 1), V - 1)]                  # ... on a slice boundary (the first element of a slice)
    elif which == 3:
        idx = np.arange(V)                                                  # every token
    elif which == 4:
        idx = starts                                                        # the first element of every slice
    elif which == 5:
        idx = np.minimum(starts + Cn, V) - 1                                # the last element of every slice
    elif which == 6:
        mid = Cn * (len(starts) // 2)
        idx = np.arange(max(0, mid - 2), min(V, mid + 2))                   # a run that crosses a slice boundary
    else:
        idx = np.arange(0, V, 1023)                                         # every 1 023rd token
    return np.unique(np.asarray(idx, dtype=np.int64))


# name -> (temperature, top_k, top_p, the other tokens, one pattern for every row or None).  top_k: "V" = V, "n" = the tie count.
E_FORMS = {"plain": (1.0, 0, 1.0, "-inf", None), "t001": (0.01, 0, 1.0, "-inf", None), "t100": (100.0, 0, 1.0, "-inf", None),
           "k_ge_v": (1.0, "V", 1.0, "-inf", None), "p_tiny": (1.0, 0, 1e-6, "lower", None), "p_tiny_t100": (100.0, 0, 1e-6, "lower", None),
           "k_below_ties": (1.0, 1, 1.0, "lower", None), "k_is_ties_run": (0.01, "n", 1.0, "lower", 6), "k_is_ties_stride": (1.0, "n", 1.0, "lower", 7)}


def e_launch(V, form, rows=B):
    """-> (logits (rows, V) fp32, temperature, top_k, top_p, [survivor indices per row]): row b holds pattern b % 8 (or the form's own) at
    the common score E_SCORES[(b // 8) % 3], the other tokens at -inf or five below"""
    T, k, p, others, fixed = E_FORMS[form]
    logits = np.empty((rows, V), dtype=np.float32)
    idxs = []
    for b in range(rows):
        c = np.float32(E_SCORES[(b // N_PATTERNS) % len(E_SCORES)])
        idx = e_pattern(V, b % N_PATTERNS if fixed is None else fixed)
        logits[b] = -np.inf if others == "-inf" else c - np.float32(5.0)
        logits[b, idx] = c
        idxs.append(idx)
    n = len(idxs[0])
    k = V if k == "V" else (n if k == "n" else k)
    return logits, T, k, p, idxs


def e_seed(sample_uniform, gen):
    """the first seed at which some every-token row of the V = 128 256 launch draws a target fl32(u * n) that is a whole number in
    [1, n): there `>=` for `>` in the walk picks the survivor before"""
    n = 128256
    rows = [b for b in range(B) if b % N_PATTERNS == 3]
    for seed in range(1, 4096):
        t = np.array([sample_uniform(seed, b, gen[b]) for b in rows], dtype=np.float32) * np.float32(n)
        if bool(((t == np.floor(t)) & (t >= 1) & (t < n)).any()):
            return seed
    raise AssertionError("no seed")
