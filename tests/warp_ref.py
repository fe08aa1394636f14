"""The warped sampler: HF's min_p / typical_p / epsilon_cutoff / eta_cutoff behind temperature / top-k / top-p, restated in
fp64 numpy in the style of select_ref.survivors, with the distance of every keep / drop decision from its boundary, the fp32 error the
kernel's own arithmetic can make in that quantity, planted defects, and the inputs the CPU and GPU tests share.

S is the survivor set entering a stage, a = (x - m) / T the warped score relative to the ROW maximum m (NaN read as -inf), p the softmax
over S, Z = sum_S e^a, H = -sum_S p ln p.  The four parameters are the fp32 values the C ABI receives.
  min_p           keep i iff a_i >= max_S a + ln min_p                                   (p_i >= min_p max_S p)
  typical_p       d_i = |-ln p_i - H| = |a_i - c|, c = sum_S p a; drop i iff the mass of the tokens with a strictly smaller d is >= tau
  epsilon_cutoff  keep i iff a_i >= ln(eps Z) or a_i == max_S a
  eta_cutoff      eta = min(eps, sqrt(eps) e^-H); keep i iff a_i >= ln(eta Z) or a_i == max_S a
Equal scores share their fate in every stage.

What the kernel can get wrong in fp32 (the count of select_ref.eta: per-term roundings plus the longest addition chain), relative unless said:
  a          3 U |a|  absolute (x - m, 1 / T, the product)
  e^a        (5 |a| + 4) U  (token_scores_ref.bound_sample's count for the fast exponential)
  Z          sum p (5 |a| + 4) U + CHAIN U,  CHAIN = ceil(V / 1024) + 6 + 16: a thread's strided elements, the wave butterfly, the 16 waves
  sum p a    per term the mass's error, 3 U for a and 1 U for the product; the same chain
  c          err(sum p a) / Z + |c| err(Z) + U |c|  absolute;  d = |a - c|:  err(a) + err(c) + U d  absolute
  H          = ln Z - c:  err(Z) + 2 U |ln Z| (logf, 1 ulp) + err(c) + U |H|  absolute
  radix mass each term truncated to 2^-40 (V 2^-40 in all, Z >= 1 at that stage), one conversion per bin and at most 255 additions in each
             of the 4 passes, tau Z one rounding on top of err(Z):  err(e^a) + (1 + 1020 + 1) U + err(Z) + V 2^-40  relative to Z
Every committed input keeps every decision 4 x that error away from its boundary (tests/test_warp_ref_cpu.py asserts it)."""
import math

import numpy as np

import select_ref as sr
from token_scores_ref import HIGHER_ORDER, LOG_ULP, U

OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
DEFECTS = ("entropy_base_2", "typical_le", "eta_is_epsilon", "min_p_before_temperature", "typical_epsilon_swapped", "no_max_stays")
NEED = 4.0                                                  # every decision clears its boundary by NEED x the derived error


def f32(v):
    return float(np.float32(v))


def chain(V):
    return -(-V // sr.THREADS) + 6 + sr.THREADS // 64


# ------------------------------------------------------------------------------------------------ the derived fp32 errors of one stage
def stage_errors(a, S, V):
    """a (V) fp64 warped scores, S (V) bool -> dict: Z, c, H, lnZ in fp64 and the absolute errors of c and H, the relative error of Z and
    of a radix mass compare, as the module docstring counts them"""
    aS = a[S]
    e = np.exp(aS)
    Z = float(e.sum())
    p = e / Z
    live = e > 0
    c = float((p[live] * aS[live]).sum())
    lnZ = math.log(Z)
    H = lnZ - c
    A = float((p[live] * np.abs(aS[live])).sum())
    A2 = float((p[live] * aS[live] ** 2).sum())
    ch = chain(V)
    eZ = HIGHER_ORDER * U * (5 * A + 4 + ch)
    eS1 = HIGHER_ORDER * U * (5 * A2 + 4 * A + 4 * A + ch * A)              # / Z: masses are p here
    ec = eS1 + abs(c) * eZ + U * abs(c)
    eH = eZ + 2 * LOG_ULP * U * abs(lnZ) + ec + U * abs(H)
    emass = HIGHER_ORDER * U * (5 * A + 4 + 1022) + eZ + V * 2.0 ** -40
    return dict(Z=Z, c=c, H=H, lnZ=lnZ, eZ=eZ, ec=ec, eH=eH, emass=emass)


def _err_a(a):
    return 3 * U * np.abs(a)


def _least(dist, err):
    """-> (the smallest distance / error, the distance there); (inf, inf) when no decision has a boundary"""
    r = np.asarray(dist, dtype=np.float64) / err
    j = int(np.argmin(r))
    return float(r[j]), float(np.asarray(dist)[j])


# ------------------------------------------------------------------------------------------------ the survivor set
def survivors(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, defect=None):
    """one row of fp32 logits -> (keep (V) bool, warped (V) fp64: a at the survivors and -inf elsewhere, clear: {stage: (the smallest
    distance / derived error over the stage's decisions, that distance)}; "top_p" holds select_ref's margin, scaled so that its own
    condition (1e-3 absolute) reads NEED)."""
    min_p, typical_p, epsilon_cutoff, eta_cutoff = f32(min_p), f32(typical_p), f32(epsilon_cutoff), f32(eta_cutoff)
    keep, a, margins = sr.survivors(x, temperature, top_k, top_p)
    keep = keep.copy()
    V = len(a)
    xc = sr.clean(x)
    m = xc.max()
    a = (xc - (m if np.isfinite(m) else 0.0)) / float(temperature)          # relative to the row maximum, dropped tokens included
    clear = {}
    if len(margins):
        clear["top_p"] = (float(margins.min()) / 1e-3 * NEED, float(margins.min()))      # select_ref's own condition: 1e-3 absolute
    if not keep.any():
        return keep, np.where(keep, a, -np.inf), clear

    def do_min_p():
        nonlocal keep
        if min_p <= 0.0:
            return
        t = math.log(min_p) * (float(temperature) if defect == "min_p_before_temperature" else 1.0) + a[keep].max()
        idx = np.flatnonzero(keep)
        err = _err_a(a[idx]) + 3 * U * abs(t)
        with np.errstate(invalid="ignore"):
            dist = np.abs(a[idx] - t)
        dist[a[idx] == a[keep].max()] = np.inf                              # the maximum: a = 0 against ln min_p <= 0, kept whatever rounds
        clear["min_p"] = _least(dist, np.maximum(err, U))
        keep[idx[a[idx] < t]] = False

    def do_typical():
        nonlocal keep
        if typical_p >= 1.0:
            return
        st = stage_errors(a, keep, V)
        idx = np.flatnonzero(keep & (np.exp(a) > 0))
        H = st["H"] / math.log(2.0) if defect == "entropy_base_2" else st["H"]
        d = np.abs((st["lnZ"] - a[idx]) - H)
        order = np.argsort(d, kind="stable")
        ds, ps = d[order], np.exp(a[idx][order]) / st["Z"]
        first = np.concatenate([[True], ds[1:] != ds[:-1]])
        lead = np.maximum.accumulate(np.where(first, np.arange(len(ds)), 0))
        below = np.concatenate([[0.0], np.cumsum(ps)[:-1]])[lead]           # the mass of the strictly smaller d, shared inside a run
        drop = below >= typical_p
        if defect == "typical_le":                                          # the mass of the d "<=" the token's own: the level that crosses tau goes too
            last = np.concatenate([first[1:], [True]])
            tail = np.minimum.accumulate(np.where(last, np.arange(len(ds)), len(ds))[::-1])[::-1]
            drop = np.cumsum(ps)[tail] >= typical_p
            drop[lead == 0] = False                                         # (HF's min_tokens_to_keep: the closest level stays)
        clear["typical_mass"] = _least(np.abs(below - typical_p), np.full(len(below), st["emass"]))
        d_cut = ds[~drop].max()
        other = ds != d_cut
        if other.any():
            err = _err_a(a[idx][order][other]) + 3 * U * abs(a[idx][order][~drop][-1]) + 2 * st["ec"] + U * (ds[other] + d_cut)
            clear["typical_band"] = _least(np.abs(ds[other] - d_cut), err)
        gone = np.zeros(V, dtype=bool)
        gone[idx[order[drop]]] = True
        keep &= ~gone
        keep &= np.exp(a) > 0

    def do_cutoff(name, eps, use_entropy):
        nonlocal keep
        if eps <= 0.0:
            return
        st = stage_errors(a, keep, V)
        le = math.log(eps)
        if use_entropy and defect != "eta_is_epsilon":
            lim = min(le, 0.5 * le - st["H"])
            et = 4 * U * abs(le) + st["eH"]
        else:
            lim, et = le, 2 * U * abs(le)
        t = lim + st["lnZ"]
        et += st["eZ"] + 2 * LOG_ULP * U * abs(st["lnZ"]) + 3 * U * abs(t)
        idx = np.flatnonzero(keep)
        top = a[idx].max()
        with np.errstate(invalid="ignore"):
            dist = np.abs(a[idx] - t)
        if defect != "no_max_stays":
            dist[a[idx] == top] = np.inf                                    # kept by the rule: no boundary (and min(t, top) is continuous in t)
        clear[name] = _least(dist, _err_a(a[idx]) + et)
        lose = a[idx] < t
        if defect != "no_max_stays":
            lose &= a[idx] < top
        keep[idx[lose]] = False

    stages = [do_min_p, do_typical, lambda: do_cutoff("epsilon_cutoff", epsilon_cutoff, False), lambda: do_cutoff("eta_cutoff", eta_cutoff, True)]
    if defect == "typical_epsilon_swapped":
        stages[1], stages[2] = stages[2], stages[1]
    for s in stages:
        if keep.any():
            s()
    return keep, np.where(keep, a, -np.inf), clear


# ------------------------------------------------------------------------------------------------ the shared inputs
SIZES = [1, 2, 65, 1024, 1025, 4099, 128256]


def params(**kw):
    d = dict(temperature=1.0, top_k=0, top_p=1.0, **OFF)
    d.update(kw)
    return d


def warp_of(p):
    """the four values of a parameter dict, as ops.sample_select_w takes them"""
    return {k: p[k] for k in OFF}


# class E (select_ref: every survivor holds the row maximum, so every mass the draw adds is exactly 1 and the pick is known exactly): the
# greedy-degenerate forms of min_p / epsilon_cutoff / eta_cutoff.  name -> (parameters, the other tokens: five below, twenty below, or
# -inf).  Twenty for eta_cutoff: where 128 255 tokens five below hold most of the mass, p e^H of each is about 1 and eta keeps them all.
E_FORMS = {"min_p_1": (params(min_p=1.0), "lower"), "min_p_1_t07": (params(temperature=0.7, min_p=1.0), "lower"),
           "eps_999": (params(epsilon_cutoff=0.999), "lower"), "eta_9": (params(eta_cutoff=0.9), "lower20"),
           "three_holes": (params(min_p=0.5, epsilon_cutoff=0.999, eta_cutoff=0.9), "-inf")}


def e_launch(V, form, rows=sr.B):
    """-> (logits (rows, V) fp32, parameters, [survivor indices per row]): row b holds select_ref's pattern b % 8 at the common score
    E_SCORES[(b // 8) % 3]"""
    p, others = E_FORMS[form]
    logits = np.empty((rows, V), dtype=np.float32)
    idxs = []
    for b in range(rows):
        c = np.float32(sr.E_SCORES[(b // sr.N_PATTERNS) % len(sr.E_SCORES)])
        idx = sr.e_pattern(V, b % sr.N_PATTERNS)
        logits[b] = -np.inf if others == "-inf" else c - np.float32(20.0 if others == "lower20" else 5.0)
        logits[b, idx] = c
        idxs.append(idx)
    return logits, p, idxs


# class G (at most 64 survivors: select_ref.accept_rule then names one token for nearly every draw): Gaussian rows of select_ref.gauss_row.
# name -> (V, parameters, row); each also runs as name + "_holes": -inf at 5 % of the indices and NaN at three more.  The row is the first
# of the six that keeps every decision, with and without the holes, NEED x the derived error from its boundary and at most 64 survivors.
G_CASES = {"v2_min_p": (2, params(min_p=0.3), 0),
           "v65_min_p": (65, params(min_p=0.05), 0),
           "v1024_k40_typ": (1024, params(top_k=40, typical_p=0.6), 0),
           "v1025_t08_eps": (1025, params(temperature=0.8, epsilon_cutoff=0.01), 0),
           "v4099_t07_eta": (4099, params(temperature=0.7, eta_cutoff=0.05), 0),
           "v4099_all": (4099, params(temperature=0.9, top_k=60, top_p=0.95, min_p=0.02, typical_p=0.8, epsilon_cutoff=0.005, eta_cutoff=0.01), 0),
           "v128256_t07_k50_min_p_typ": (128256, params(temperature=0.7, top_k=50, min_p=0.01, typical_p=0.7), 2),
           "v128256_t06_eps": (128256, params(temperature=0.6, epsilon_cutoff=0.004), 0),
           "v128256_t06_eta": (128256, params(temperature=0.6, eta_cutoff=0.05), 2)}
G_NAMES = [n + s_ for n in G_CASES for s_ in ("", "_holes")]


def g_case(name):
    """-> (row fp32 (V), parameters)"""
    holes = name.endswith("_holes")
    V, p, r = G_CASES[name[:-len("_holes")] if holes else name]
    row = sr.gauss_row(V, r)
    if holes:
        row = sr.with_holes(row)
        order = np.argsort(-np.where(np.isfinite(row), row, -np.inf))
        row[order[[1, 5, V // 2][:max(0, V - 1)]]] = np.nan                  # a NaN where a survivor would be, one lower down, one in the tail
    return row, p


# ladder rows: a few score levels with chosen multiplicities over the whole width, the rest of the row at `floor`.  Every decision keeps
# 1e-2 in its own quantity (asserted), where a Gaussian row of this width leaves the derived error nothing to decide; the reductions and
# the indexing run at full width all the same.  name -> (V, [(score, count) ...], floor, parameters)
_L = [(8.0, 3), (6.0, 20)]
LADDERS = {"ladder_min_p": (128256, _L, 0.0, params(min_p=0.05)),
           "ladder_eps": (128256, _L, 0.0, params(epsilon_cutoff=0.001)),
           "ladder_eta": (128256, _L, 0.0, params(eta_cutoff=0.5)),
           "ladder_band": (128256, _L, 0.0, params(typical_p=0.5)),                      # the maximum and the 6.0 level go, 128 233 tokens stay
           "ladder_typ_eps_eta": (128256, [(8.0, 3), (6.0, 20), (3.0, 400)], 0.0, params(temperature=1.25, typical_p=0.9, epsilon_cutoff=3e-5, eta_cutoff=0.3)),
           "band_peak_200": (201, [(5.0, 1)], 0.0, params(typical_p=0.3)),                # the peak goes, the 200 stay
           "band_60": (1025, [(6.0, 1), (2.0, 60)], -np.inf, params(typical_p=0.4)),      # the maximum goes, 60 survivors
           "ladder_4099_all": (4099, [(7.0, 2), (5.5, 9), (2.0, 300)], -1.0, params(temperature=0.8, top_k=2000, top_p=0.98, min_p=0.001, typical_p=0.95,
                                                                                    epsilon_cutoff=2e-4, eta_cutoff=0.05))}


def ladder(name):
    """-> (row fp32 (V), parameters): the level tokens sit at seeded random places, so every level meets many threads' slices"""
    import torch
    V, levels, floor, p = LADDERS[name]
    row = np.full(V, floor, dtype=np.float32)
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(97)).numpy()
    at = 0
    for score, count in levels:
        row[perm[at:at + count]] = score
        at += count
    return row, p


def sparse_check(warped, u, picks):
    """select_ref.check_draws for a survivor set too large for its (draws, survivors) table: the same rule, evaluated at the pick alone"""
    idx, C, Z = sr.cdf(warped)
    e2 = 2.0 * sr.eta(warped)
    pos = np.searchsorted(idx, picks)
    worst = 0.0
    for d, (tok, j) in enumerate(zip(np.asarray(picks).tolist(), pos.tolist())):
        if j >= len(idx) or idx[j] != tok:
            return f"draw {d}: token {tok} is no survivor", worst
        lo = ((C[j - 1] if j else 0.0) - u[d] * Z) / Z
        hi = (C[j] - u[d] * Z) / Z
        dist = max(lo, 0.0, -hi) / e2
        if not (lo <= e2 and hi > -e2):
            return f"draw {d} (u = {u[d]!r}): token {tok} sits {dist:.3g} x 2 eta outside its interval", worst
        worst = max(worst, dist)
    return "", worst


def logprob_ref(warped):
    """log(p / z) of every survivor, fp64"""
    keep = np.isfinite(warped)
    top = warped[keep].max()
    return warped - (top + math.log(np.exp(warped[keep] - top).sum()))


def logprob_bound(warped, token):
    """token_scores_ref.bound_sample with the arguments the kernel really forms: a is relative to the ROW maximum, which a band may have
    dropped, so |a| of every survivor is larger by the distance of the survivors' best from it.  Equal to bound_sample otherwise."""
    keep = np.isfinite(warped)
    a = warped[keep]
    p = np.exp(a - a.max())
    A = float((p * np.abs(a)).sum() / p.sum())
    V = len(warped)
    lp = float(logprob_ref(warped)[token])
    return HIGHER_ORDER * U * (5 * A + 4 + (-(-V // sr.THREADS) + sr.THREADS) + 5 * abs(float(warped[token])) + 4 + 1 + 2 * LOG_ULP * abs(lp))
