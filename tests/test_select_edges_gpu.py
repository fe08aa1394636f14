"""GPU edge suite, token selection: sample_rows_kernel per draw against tests/select_ref.py (class E: the exact index of every draw; class
G: every draw inside its interval, a survivor, and bit for bit the id the parent commit drew, tests/golden/select_edges_ids.npz), survivor
sets, NaN and rows of nothing, the bookkeeping of the sampler's commit launch, and the row scans of greedy, beam top-k and the logits
processors at the smallest sizes and across greedy's second 16-byte pass."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden, pkg

import logits_proc_ref as lpr
import select_ref as sr
import token_scores_ref as tsr
from edge_helpers import DEV, FILL, L, guarded_flat, untouched_flat

pytestmark = pytest.mark.gpu
ops = pkg("ops")
I32, F32 = torch.int32, torch.float32
GEN = sr.gen_counts()
NEG = float("-inf")
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ one guarded launch
def _launch(kind, logits, params, gen, eos=(), pad=0, use_eos=False, unfinished=None, ctx=None, max_new=sr.MAX_NEW):
    """kind: sample / sample_sc / greedy / greedy_sc; every array the entry writes sits between guard bands -> host copies"""
    rows = logits.shape[0]
    init = dict(unfinished=[1] * rows if unfinished is None else unfinished, ctx=list(range(rows)) if ctx is None else ctx, gen=gen, fin=[0] * rows,
                nxt=[-7] * rows, out=[-1] * (rows * max_new))
    bufs = {k: guarded_flat(len(v), I32) for k, v in init.items()}
    for k, v in init.items():
        bufs[k][1].copy_(torch.tensor(v, dtype=I32))
    bufs["lp"] = guarded_flat(rows * max_new, F32)
    s = {k: v[1] for k, v in bufs.items()}
    a = (list(eos), pad, use_eos, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"].view(rows, max_new))
    if kind == "sample":
        ops.sample_select(logits, *params, *a)
    elif kind == "sample_sc":
        ops.sample_select_sc(logits, *params, *a, s["lp"].view(rows, max_new))
    elif kind == "greedy":
        ops.greedy_select(logits, *a)
    else:
        ops.greedy_select_sc(logits, *a, s["lp"].view(rows, max_new))
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert untouched_flat(buf, view.numel()), f"{kind}: guard words around {k} were written"
    out = {k: v.cpu().numpy().copy() for k, v in s.items()}
    out["out"], out["lp"] = out["out"].reshape(rows, max_new), out["lp"].reshape(rows, max_new)
    if not kind.endswith("_sc"):
        assert bool((out["lp"] == FILL).all())
    return out


def _state_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a if k != "lp")


def _drawn_lp(r, gen):
    return r["lp"][np.arange(len(gen)), np.asarray(gen)]


def _e_seed():
    return _cached("e_seed", lambda: sr.e_seed(ops.sample_uniform, GEN))


# ------------------------------------------------------------------------------------------------ the sampler, class E
@pytest.mark.parametrize("V", sr.E_SIZES)
def test_sampler_class_e_every_draw_is_the_exact_index(V):
    """every survivor pattern, score sign and parameter form of select_ref.e_launch: the drawn token is survivor number
    min(floor(fl32(u n)), n - 1) for every one of the 256 draws of every launch, and with _sc its log-probability is -log n within one
    rounding of the division 1 / n and one ulp of logf"""
    seed = _e_seed()
    u = sr.uniforms(ops.sample_uniform, seed, GEN)
    worst = 0.0
    for form in sr.E_FORMS:
        logits, T, k, p, idxs = sr.e_launch(V, form)
        want = np.array([idx[sr.class_e_ordinal(u[b:b + 1], len(idx))[0]] for b, idx in enumerate(idxs)])
        ld = torch.from_numpy(logits).to(DEV)
        runs = [_launch(kind, ld, (T, k, p, seed), GEN) for kind in ("sample", "sample_sc")]
        for r in runs:
            wrong = np.flatnonzero(r["nxt"] != want)
            assert wrong.size == 0, (V, form, f"{wrong.size} of {sr.B} draws wrong, first row {wrong[0]}: got {r['nxt'][wrong[0]]} want {want[wrong[0]]}"
                                                f" (n = {len(idxs[wrong[0]])}, u = {u[wrong[0]]!r})")
            assert np.array_equal(r["out"][np.arange(sr.B), GEN], want) and np.array_equal(r["gen"], np.asarray(GEN) + 1)
        assert _state_equal(*runs)
        lp = _drawn_lp(runs[1], GEN).astype(np.float64)
        for b, idx in enumerate(idxs):
            ref = -math.log(len(idx))
            bound = sr.U + float(np.spacing(np.float32(abs(ref))))
            assert abs(lp[b] - ref) <= bound, (V, form, b, lp[b], ref, bound)
            worst = max(worst, abs(lp[b] - ref) / bound)
    print(f"class E V={V}: {len(sr.E_FORMS)} forms x 2 entries x {sr.B} draws exact; worst log-probability err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the sampler, class G
@pytest.mark.parametrize("name", sr.G_NAMES)
def test_sampler_class_g_every_draw_sits_in_its_interval(name):
    x, T, k, p = sr.g_case(name)
    keep, warped, _ = sr.survivors(x, T, k, p)
    u = sr.uniforms(ops.sample_uniform, sr.SEED, GEN)
    ld = torch.from_numpy(x).to(DEV)[None, :].repeat(sr.B, 1).contiguous()
    runs = [_launch(kind, ld, (T, k, p, sr.SEED), GEN) for kind in ("sample", "sample_sc")]
    assert _state_equal(*runs)
    picks = runs[1]["nxt"]
    msg, worst = sr.check_draws(warped, u, picks)
    print(f"class G {name}: {int(keep.sum())} survivors, worst distance / (2 eta) {worst:.3f}")
    assert msg == "", (name, msg)
    # NaN-free rows keep the bits of the parent commit's draws
    assert np.array_equal(picks, golden("select_edges_ids")[name]), name
    ref_lp = warped - (warped[keep].max() + math.log(np.exp(warped[keep] - warped[keep].max()).sum()))
    lp = _drawn_lp(runs[1], GEN).astype(np.float64)
    bounds = {int(tok): sr.sampled_logprob_bound(warped, int(tok)) for tok in np.unique(picks)}
    ratio = max(abs(lp[b] - ref_lp[picks[b]]) / bounds[int(picks[b])] for b in range(sr.B))
    print(f"class G {name}: worst log-probability err / bound {ratio:.3f}")
    assert ratio <= 1.0 and bool((lp <= 0).all())


# ------------------------------------------------------------------------------------------------ the sampler, survivor sets and NaN
def _set_seed():
    cases = sr.set_cases()
    return _cached("set_seed", lambda: sr.covering_seed(ops.sample_uniform, [sr.survivors(x, T, k, p)[1] for x, T, k, p, _ in cases.values()], GEN))


@pytest.mark.parametrize("name", list(sr.set_cases()))
def test_sampler_draws_exactly_the_survivor_set(name):
    """the seed is chosen on the host so that every survivor's interval, shrunk by 2 eta, holds some row's u: the 256 draws of one launch
    must hit every survivor and nothing else"""
    x, T, k, p, want = sr.set_cases()[name]
    seed = _set_seed()
    warped = sr.survivors(x, T, k, p)[1]
    ld = torch.from_numpy(x).to(DEV)[None, :].repeat(sr.B, 1).contiguous()
    r = _launch("sample_sc", ld, (T, k, p, seed), GEN)
    assert set(r["nxt"].tolist()) == want, (name, sorted(set(r["nxt"].tolist())), sorted(want))
    msg, _ = sr.check_draws(warped, sr.uniforms(ops.sample_uniform, seed, GEN), r["nxt"])
    assert msg == "", (name, msg)
    assert bool(np.isfinite(_drawn_lp(r, GEN)).all())
    if np.isnan(x).any():
        # NaN is -inf: bit for bit the draws and the log-probabilities of the same row with -inf in its place
        assert not set(np.flatnonzero(np.isnan(x)).tolist()) & set(r["nxt"].tolist())
        as_inf = torch.from_numpy(np.where(np.isnan(x), np.float32(NEG), x)).to(DEV)[None, :].repeat(sr.B, 1).contiguous()
        r2 = _launch("sample_sc", as_inf, (T, k, p, seed), GEN)
        assert _state_equal(r, r2) and np.array_equal(r["lp"].view(np.int32), r2["lp"].view(np.int32))


@pytest.mark.parametrize("name", ["v1000_p075_holes", "v1025_t07_k20_p09_holes", "v1000_t13_k7", "v128256_t06_k50_p09"])
def test_sampler_reads_nan_as_minus_infinity_on_the_class_g_rows(name):
    """NaN over the largest logit (a top-k seat, the row maximum), over a survivor in the middle and over dropped tokens: never drawn, the
    draws those of the row with -inf there, every one inside its interval of the reference (which counts NaN as -inf)"""
    x, T, k, p = sr.g_case(name)
    order = np.argsort(-np.where(np.isfinite(x), x, -np.inf))
    x[order[[0, 3, 40, 500]]] = np.nan
    x[order[1]] = -np.nan                                                     # the sign bit set: the other branch of ord_key
    keep, warped, margins = sr.survivors(x, T, k, p)
    assert len(margins) == 0 or margins.min() >= 1e-3
    as_inf = np.where(np.isnan(x), np.float32(NEG), x)
    runs = [_launch("sample_sc", torch.from_numpy(v).to(DEV)[None, :].repeat(sr.B, 1).contiguous(), (T, k, p, sr.SEED), GEN) for v in (x, as_inf)]
    assert _state_equal(*runs) and np.array_equal(runs[0]["lp"].view(np.int32), runs[1]["lp"].view(np.int32))
    assert bool(keep[runs[0]["nxt"]].all()) and bool(np.isfinite(_drawn_lp(runs[0], GEN)).all())
    msg, worst = sr.check_draws(warped, sr.uniforms(ops.sample_uniform, sr.SEED, GEN), runs[0]["nxt"])
    assert msg == "", (name, msg)


@pytest.mark.parametrize("V", [1, 3, 1000, 4100])
@pytest.mark.parametrize("params", [(1.0, 0, 1.0), (0.7, 20, 0.9)])
def test_sampler_on_rows_without_a_finite_logit(V, params):
    """all -inf, all NaN, and a mix: token 0 as greedy gives, a log-probability that is not finite, the neighbours untouched"""
    B = 8
    logits = torch.from_numpy(np.stack([sr.gauss_row(1000)[:V] if V <= 1000 else np.resize(sr.gauss_row(1000), V) for _ in range(B)]).astype(np.float32))
    logits[1] = NEG
    logits[4] = float("nan")
    logits[6] = NEG
    logits[6, ::2] = float("nan")
    gen = [b % sr.MAX_NEW for b in range(B)]
    ld = logits.to(DEV)
    r = _launch("sample_sc", ld, (*params, 77), gen)
    g = _launch("greedy_sc", ld, None, gen)
    for b in (1, 4, 6):
        assert r["nxt"][b] == 0 and r["out"][b, gen[b]] == 0
        assert not np.isfinite(r["lp"][b, gen[b]]) and not np.isfinite(g["lp"][b, gen[b]])
    # greedy: 0 for a row of one kind; in the mixed row its strict scan ("NaN never wins", not even against -inf) stops at the first -inf
    assert g["nxt"][1] == 0 and g["nxt"][4] == 0 and g["nxt"][6] == (1 if V > 1 else 0)
    live = [b for b in range(B) if b not in (1, 4, 6)]
    keep = sr.survivors(logits[0].numpy(), *params)[0]
    assert bool(keep[r["nxt"][live]].all()) and bool(np.isfinite(_drawn_lp(r, gen)[live]).all())
    assert _state_equal(r, _launch("sample", ld, (*params, 77), gen))


# ------------------------------------------------------------------------------------------------ the commit launch
def _commit_restated(tok, unfinished, ctx, gen, eos, pad, use_eos, max_new):
    rows = len(tok)
    s = dict(unfinished=np.array(unfinished, dtype=np.int32), ctx=np.array(ctx, dtype=np.int32), gen=np.array(gen, dtype=np.int32),
             fin=np.zeros(rows, dtype=np.int32), nxt=np.full(rows, -7, dtype=np.int32), out=np.full((rows, max_new), -1, dtype=np.int32))
    wrote_lp = np.zeros((rows, max_new), dtype=bool)
    zero_lp = np.zeros((rows, max_new), dtype=bool)
    for b in range(rows):
        unf, n = int(s["unfinished"][b]), int(s["gen"][b])
        t = int(tok[b]) if (unf or not use_eos) else pad
        if n < max_new:
            s["out"][b, n] = t
            wrote_lp[b, n] = True
            zero_lp[b, n] = bool(use_eos and not unf)
        s["gen"][b] = n + 1
        s["nxt"][b] = t
        if use_eos and unf and t in eos:
            s["unfinished"][b] = 0
            s["fin"][b] = n + 1
        s["ctx"][b] += 1
    return s, wrote_lp, zero_lp


@pytest.mark.parametrize("use_eos", [True, False])
def test_sampler_commit_bookkeeping_equals_the_host_restatement(use_eos):
    """two tied survivors per row (class E: the draw is known exactly): a finished row emits pad, an EOS draw finishes the row and records
    finish_len, gen_count >= max_new writes neither out_ids nor a log-probability but still sets next_ids; use_eos = 0 ignores all of it"""
    V, max_new, pad, eos, seed = 64, sr.MAX_NEW, 5, [3, 10, 63], 4242
    gen = [b % (max_new + 2) for b in range(sr.B)]
    unfinished = [0 if b % 5 == 0 else 1 for b in range(sr.B)]
    ctx = [(7 * b) % 50 for b in range(sr.B)]
    logits = np.full((sr.B, V), NEG, dtype=np.float32)
    pairs = [np.array(sorted({b % V, (3 * b + 10) % V})) for b in range(sr.B)]
    for b, idx in enumerate(pairs):
        logits[b, idx] = 1.25
    u = sr.uniforms(ops.sample_uniform, seed, gen)
    tok = np.array([idx[sr.class_e_ordinal(u[b:b + 1], len(idx))[0]] for b, idx in enumerate(pairs)])
    want, wrote_lp, zero_lp = _commit_restated(tok, unfinished, ctx, gen, eos, pad, use_eos, max_new)
    if use_eos:
        assert int((want["fin"] > 0).sum()) >= 3 and int((want["nxt"] == pad).sum()) >= 40          # the inputs reach the EOS and the pad branch
    ld = torch.from_numpy(logits).to(DEV)
    for kind in ("sample", "sample_sc"):
        r = _launch(kind, ld, (1.0, 0, 1.0, seed), gen, eos=eos, pad=pad, use_eos=use_eos, unfinished=unfinished, ctx=ctx)
        for k in want:
            assert np.array_equal(r[k], want[k]), (kind, k)
        if kind == "sample_sc":
            assert bool((r["lp"][~wrote_lp] == FILL).all())
            assert bool((r["lp"][zero_lp] == 0.0).all())
            live = wrote_lp & ~zero_lp
            n_of = np.array([len(idx) for idx in pairs], dtype=np.float64)[:, None].repeat(max_new, 1)
            assert float(np.abs(r["lp"][live].astype(np.float64) + np.log(n_of[live])).max()) <= sr.U + float(np.spacing(np.float32(math.log(2.0))))


# ------------------------------------------------------------------------------------------------ the row scans at the missing sizes
SCAN_SIZES = [1, 3, 4, 4096, 16384, 16388, 20000]


def _scan_rows(V):
    """six rows on a grid of 1/64 (differences survive the fp32 log-softmax, so the order of the values is the order of the logits; ties
    abound): each carries a run of -inf, a NaN, and an exact tie of the maximum across the two halves of the row.  Row 3 has its only
    maximum at V - 1, row 4 is +100 (a large shift), row 5 holds nothing finite."""
    g = torch.Generator().manual_seed(1000 + V)
    x = (torch.randint(-512, 257, (6, V), generator=g).float() / 64.0).numpy()
    if V >= 4:
        h = V // 2
        x[:, h // 2:h // 2 + max(1, V // 16)] = NEG
        for r in range(6):
            lo, hi = (r * 37) % h, h + (r * 53 + 1) % (V - h)
            if np.isinf(x[r, lo]):
                lo = 0
            x[r, [lo, hi]] = 5.0                                            # above every grid value: the tie of the maximum, first half and second
            x[r, (hi + 1) % V if (hi + 1) % V not in (lo, hi) else 1] = np.nan
        x[3, x[3] == 5.0] = 4.0
        x[3, V - 1] = 5.0
    elif V == 3:
        x[:, 0] = [1.0, NEG, 2.0, np.nan, 1.0, NEG]
        x[:, 1] = [np.nan, 2.0, NEG, NEG, 1.0, np.nan]
        x[:, 2] = [1.0, 2.0, 2.0, 3.0, NEG, NEG]
    else:
        x[:, 0] = [1.0, -2.0, 0.0, NEG, np.nan, 3.5]
    x[4] += 100.0
    if V > 1:
        x[5] = NEG
        x[5, V // 2] = np.nan
    return x.astype(np.float32)


def _clean64(x):
    return np.where(np.isnan(x), -np.inf, x).astype(np.float64)


@pytest.mark.parametrize("V", SCAN_SIZES)
def test_greedy_select_at_the_missing_sizes(V):
    """V = 16 388 and 20 000 reach the second pass of the 16-byte scan (i0 += 4096); token exact (the first maximum, NaN never wins, 0 for
    a row of nothing), log-probability within bound_row of the fp64 definition"""
    x = _scan_rows(V)
    rows = x.shape[0]
    c = _clean64(x)
    tok = c.argmax(axis=1)
    dead = ~np.isfinite(c.max(axis=1))
    gen = [b % sr.MAX_NEW for b in range(rows)]
    ld = torch.from_numpy(x).to(DEV)
    runs = [_launch(kind, ld, None, gen) for kind in ("greedy", "greedy_sc")]
    assert _state_equal(*runs)
    assert np.array_equal(runs[1]["nxt"], np.where(dead, 0, tok)), (V, runs[1]["nxt"], tok)
    ref = tsr.transition_logprobs(torch.from_numpy(x), torch.from_numpy(tok)).numpy()
    worst = 0.0
    for b in range(rows):
        got = float(runs[1]["lp"][b, gen[b]])
        if dead[b]:
            assert not np.isfinite(got)
            continue
        bound = tsr.bound_row(x[b], int(tok[b]))
        assert abs(got - ref[b]) <= bound, (V, b, got, ref[b], bound)
        worst = max(worst, abs(got - ref[b]) / bound)
    print(f"greedy V={V}: worst err / bound_row {worst:.3f}")


def _beam_topk(ld, score, M):
    rows, V = ld.shape
    vb, val = guarded_flat(rows * M, F32)
    tb, tok = guarded_flat(rows * M, I32)
    L.check(L.lib().sl_beam_topk(ld.data_ptr(), rows, V, L.ptr(score), M, val.data_ptr(), tok.data_ptr(), L.stream_ptr()), "sl_beam_topk")
    torch.cuda.synchronize()
    assert untouched_flat(vb, rows * M) and untouched_flat(tb, rows * M)
    return val.view(rows, M).cpu().numpy(), tok.view(rows, M).cpu().numpy()


@pytest.mark.parametrize("V", SCAN_SIZES)
def test_beam_topk_at_the_missing_sizes(V):
    """M in {1, 64} and M = V where V <= 64: the M largest log_softmax + score in the order (larger value, then lower token), NaN as
    -inf, -inf entries by index once the numbers run out; values within 1e-5 (the bound of tests/test_beam_gpu.py)"""
    x = _scan_rows(V)
    rows = x.shape[0]
    score = -np.arange(rows, dtype=np.float32) * 0.75
    c = _clean64(x)
    m = c.max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc =(c - m) - np.log(np.exp(c - m).sum(axis=1, keepdims=True)) + score[:, None].astype(np.float64)
    acc[~np.isfinite(c).any(axis=1)] = -np.inf                              # a row of nothing: every value -inf, the tokens by index
    ld, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(score).to(DEV)
    for M in sorted({M for M in (1, 64, V) if M <= min(V, 64)}):
        val, tok = _beam_topk(ld, sd, M)
        assert not np.isnan(val).any()
        for b in range(rows):
            order = np.lexsort((np.arange(V), -acc[b]))[:M]
            assert np.array_equal(tok[b], order), (V, M, b, tok[b][:8], order[:8])
            want = acc[b, order]
            if not np.isfinite(c[b]).any():
                assert bool(np.isinf(val[b]).all() and (val[b] < 0).all())
                continue
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(val[b]), inf) and float(np.abs(val[b][~inf] - want[~inf]).max()) <= 1e-5, (V, M, b)


def _logits_process(x, hists, p, g, mn, eos, log_softmax, hist_ld=16):
    rows, V = x.shape
    lb, lg = guarded_flat(rows * V, F32)
    lg.copy_(torch.from_numpy(x).reshape(-1))
    sb, scratch = guarded_flat(rows * hist_ld, F32)
    hist = torch.full((rows, hist_ld), 0, dtype=I32)
    for r, h in enumerate(hists):
        hist[r, :len(h)] = torch.tensor(h, dtype=I32)
    hist_d, len_d = hist.to(DEV), torch.tensor([len(h) for h in hists], dtype=I32).to(DEV)
    lp = L.LogitsOpts()
    lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = p, g, mn
    eos_c = (C.c_int32 * 8)(*(list(eos) + [0] * (8 - len(eos))))
    L.check(L.lib().sl_logits_process(lg.data_ptr(), rows, V, hist_d.data_ptr(), hist_ld, len_d.data_ptr(), None, C.byref(lp), eos_c, len(eos),
                                      int(log_softmax), scratch.data_ptr(), L.stream_ptr()), "sl_logits_process")
    torch.cuda.synchronize()
    assert untouched_flat(lb, rows * V) and untouched_flat(sb, rows * hist_ld)
    return lg.view(rows, V).cpu()


@pytest.mark.parametrize("V", SCAN_SIZES)
@pytest.mark.parametrize("log_softmax", [0, 1])
def test_logits_process_at_the_missing_sizes(V, log_softmax):
    """both block sizes (raw and log_softmax = 1) with all three processors on: raw mode bit for bit the restatement (a NaN no processor
    touches stays), log_softmax mode within 1e-5 of the fp64 log-softmax (NaN as -inf) followed by the processors, the same -inf set"""
    x = _scan_rows(V)
    rows = x.shape[0]
    p, g, mn = 1.3, 2, 40
    eos = [0, V - 1] if V > 1 else [0]
    alphabet = [0, V - 1, V // 2, V // 3]
    hists = [[alphabet[(r + j * j) % 4] for j in range(n)] for r, n in enumerate([0, 1, 2, 9, 16, 5])]
    got = _logits_process(x, hists, p, g, mn, eos, log_softmax)
    if not log_softmax:
        want = lpr.process(torch.from_numpy(x), hists, p, g, mn, eos)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(got, nan=7.0).view(I32), torch.nan_to_num(want, nan=7.0).view(I32)), V
        return
    c = torch.from_numpy(_clean64(x))
    want = lpr.process(torch.log_softmax(c, dim=-1), hists, p, g, mn, eos)
    for r in range(rows):
        if not bool(torch.isfinite(c[r]).any()):
            assert bool((torch.isinf(got[r]) & (got[r] < 0)).all()), (V, r)            # a row of nothing: every value -inf, never NaN
            continue
        inf = torch.isinf(want[r])
        assert torch.equal(torch.isinf(got[r]), inf) and not bool(torch.isnan(got[r]).any()), (V, r)
        if bool((~inf).any()):
            err = float((got[r][~inf].double() - want[r][~inf]).abs().max())
            assert err <= 1e-5, (V, r, err)
