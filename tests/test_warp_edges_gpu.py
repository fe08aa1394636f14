"""GPU edge suite, the warped sampler: sl_sample_select_w per draw, 256 rows per launch, against tests/warp_ref.py.  Class E:
the exact index of every draw; class G, ladders and bands: every draw a survivor of the reference, inside its interval, its
log-probability log(p / z) within the 3.5 bound; the commit's bookkeeping and the all-off call bit for bit sl_sample_select_sc's.
What the inputs must satisfy for these to be fair is asserted on the CPU (tests/test_warp_ref_cpu.py)."""
import numpy as np
import pytest
import torch

from conftest import pkg

import select_ref as sr
import warp_ref as wr
from edge_helpers import DEV, FILL, L, guarded_flat, untouched_flat

pytestmark = pytest.mark.gpu
ops = pkg("ops")
I32, F32 = torch.int32, torch.float32
GEN = sr.gen_counts()
SEED = sr.SEED


def _launch(kind, logits, p, seed, gen, warp="dict", eos=(), pad=0, use_eos=False, unfinished=None, max_new=sr.MAX_NEW):
    """kind: w (no log-probabilities) / w_sc / sc (sl_sample_select_sc); every array the entry writes sits between guard bands"""
    rows = logits.shape[0]
    init = dict(unfinished=[1] * rows if unfinished is None else unfinished, ctx=list(range(rows)), gen=gen, fin=[0] * rows, nxt=[-7] * rows,
                out=[-1] * (rows * max_new))
    bufs = {k: guarded_flat(len(v), I32) for k, v in init.items()}
    for k, v in init.items():
        bufs[k][1].copy_(torch.tensor(v, dtype=I32))
    bufs["lp"] = guarded_flat(rows * max_new, F32)
    s = {k: v[1] for k, v in bufs.items()}
    a = (p["temperature"], p["top_k"], p["top_p"], seed, list(eos), pad, use_eos, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"].view(rows, max_new))
    if kind == "sc":
        ops.sample_select_sc(logits, *a, s["lp"].view(rows, max_new))
    else:
        w = wr.warp_of(p) if warp == "dict" else warp
        ops.sample_select_w(logits, *a, s["lp"].view(rows, max_new) if kind == "w_sc" else None, w)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert untouched_flat(buf, view.numel()), f"{kind}: guard words around {k} were written"
    out = {k: v.cpu().numpy().copy() for k, v in s.items()}
    out["out"], out["lp"] = out["out"].reshape(rows, max_new), out["lp"].reshape(rows, max_new)
    if kind == "w":
        assert bool((out["lp"] == FILL).all())
    return out


def _state_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a if k != "lp")


def _drawn_lp(r, gen):
    return r["lp"][np.arange(len(gen)), np.asarray(gen)]


def _rep(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(DEV)[None, :].repeat(sr.B, 1).contiguous()


# ------------------------------------------------------------------------------------------------ class E
@pytest.mark.parametrize("V", wr.SIZES)
def test_warped_class_e_every_draw_is_the_exact_index(V):
    """min_p = 1, epsilon_cutoff = 0.999, eta_cutoff = 0.9 and the three together: the survivors are the ties of the maximum, the pick is
    select_ref.class_e_pick's for each of the 256 draws, the log-probability -log n"""
    u = sr.uniforms(ops.sample_uniform, SEED, GEN)
    for form in wr.E_FORMS:
        logits, p, idxs = wr.e_launch(V, form)
        want = np.array([idx[sr.class_e_ordinal(u[b:b + 1], len(idx))[0]] for b, idx in enumerate(idxs)])      # select_ref.class_e_pick, per row
        ld = torch.from_numpy(logits).to(DEV)
        runs = [_launch(kind, ld, p, SEED, GEN) for kind in ("w", "w_sc")]
        for r in runs:
            wrong = np.flatnonzero(r["nxt"] != want)
            assert wrong.size == 0, (V, form, f"{wrong.size} of {sr.B} draws wrong, first row {wrong[0]}: got {r['nxt'][wrong[0]]} want {want[wrong[0]]}")
            assert np.array_equal(r["out"][np.arange(sr.B), GEN], want) and np.array_equal(r["gen"], np.asarray(GEN) + 1)
        assert _state_equal(*runs)
        lp = _drawn_lp(runs[1], GEN).astype(np.float64)
        for b, idx in enumerate(idxs):
            ref = -np.log(len(idx))
            assert abs(lp[b] - ref) <= sr.U + float(np.spacing(np.float32(abs(ref)))), (V, form, b, lp[b], ref)


# ------------------------------------------------------------------------------------------------ class G, ladders, bands
def _check_case(name, x, p):
    keep, warped, _ = wr.survivors(x, **p)
    u = sr.uniforms(ops.sample_uniform, SEED, GEN)
    ld = _rep(x)
    runs = [_launch(kind, ld, p, SEED, GEN) for kind in ("w", "w_sc")]
    assert _state_equal(*runs)
    picks = runs[1]["nxt"]
    outside = np.flatnonzero(~keep[picks])
    assert outside.size == 0, (name, f"row {outside[0]} drew token {picks[outside[0]]}, no survivor of the reference ({int(keep.sum())} survivors)")
    msg, worst = (sr.check_draws if int(keep.sum()) <= 64 else wr.sparse_check)(warped, u, picks)
    print(f"{name}: {int(keep.sum())} survivors, worst distance / (2 eta) {worst:.3f}")
    assert msg == "", (name, msg)
    ref_lp = wr.logprob_ref(warped)
    lp = _drawn_lp(runs[1], GEN).astype(np.float64)
    bounds = {int(t): wr.logprob_bound(warped, int(t)) for t in np.unique(picks)}
    ratio = max(abs(lp[b] - ref_lp[picks[b]]) / bounds[int(picks[b])] for b in range(sr.B))
    print(f"{name}: worst log-probability err / bound {ratio:.3f}")
    assert ratio <= 1.0 and bool((lp <= 0).all())
    return runs[1]


@pytest.mark.parametrize("name", wr.G_NAMES)
def test_warped_class_g_every_draw_is_a_survivor_inside_its_interval(name):
    x, p = wr.g_case(name)
    r = _check_case(name, x, p)
    if np.isnan(x).any():                                                     # NaN is -inf: bit for bit the row with -inf in its place
        r2 = _launch("w_sc", _rep(np.where(np.isnan(x), np.float32(-np.inf), x)), p, SEED, GEN)
        assert _state_equal(r, r2) and np.array_equal(r["lp"].view(np.int32), r2["lp"].view(np.int32))


@pytest.mark.parametrize("name", list(wr.LADDERS))
def test_warped_ladders_and_bands(name):
    """full-width reductions with margins of 1e-2; in the band cases the row maximum is dropped and never drawn"""
    x, p = wr.ladder(name)
    r = _check_case(name, x, p)
    keep = wr.survivors(x, **p)[0]
    if not keep[int(np.argmax(x))]:
        assert not bool(np.isin(r["nxt"], np.flatnonzero(x == x.max())).any()), name


# ------------------------------------------------------------------------------------------------ off is the unwarped call; bookkeeping
@pytest.mark.parametrize("name", ["v1025_t07_k20_p09", "v128256_t06_k50_p09_holes"])
def test_all_off_and_null_give_the_bits_of_sample_select_sc(name):
    x, T, k, tp = sr.g_case(name)
    p = wr.params(temperature=T, top_k=k, top_p=tp)
    ld = _rep(x)
    base = _launch("sc", ld, p, SEED, GEN)
    off = L.WarpOpts(**wr.OFF)
    for warp in (None, off):
        r = _launch("w_sc", ld, p, SEED, GEN, warp=warp)
        assert _state_equal(base, r) and np.array_equal(base["lp"].view(np.int32), r["lp"].view(np.int32)), (name, warp)


@pytest.mark.parametrize("use_eos", [True, False])
def test_warped_commit_bookkeeping_matches_the_unwarped_call(use_eos):
    """one survivor per row under either call (min_p = 1 here, top_k = 1 there: the argmax), so the two commits see the same tokens: finished
    rows emit pad, an EOS draw finishes its row, gen_count >= max_new writes neither id nor log-probability"""
    V, max_new, pad, eos = 65, sr.MAX_NEW, 5, [3, 10, 63]
    gen = [b % (max_new + 2) for b in range(sr.B)]
    unfinished = [0 if b % 5 == 0 else 1 for b in range(sr.B)]
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(sr.B, V, generator=g) * 2.0
    logits[torch.arange(sr.B), torch.arange(sr.B) % V] = 12.0                  # the argmax walks over every token, the EOS ids among them
    ld = logits.to(DEV)
    a = _launch("w_sc", ld, wr.params(min_p=1.0), 4242, gen, eos=eos, pad=pad, use_eos=use_eos, unfinished=unfinished)
    b = _launch("sc", ld, wr.params(top_k=1), 4242, gen, eos=eos, pad=pad, use_eos=use_eos, unfinished=unfinished)
    assert _state_equal(a, b)
    assert np.array_equal(a["lp"].view(np.int32), b["lp"].view(np.int32))      # log(1 / 1) = 0 where written, FILL elsewhere
    if use_eos:
        assert int((a["fin"] > 0).sum()) >= 3 and int((a["nxt"] == pad).sum()) >= 40


def test_warped_rows_without_a_finite_logit():
    x = np.stack([sr.gauss_row(1000) for _ in range(4)]).astype(np.float32)
    x[1] = -np.inf
    x[2] = np.nan
    gen = [0, 1, 2, 3]
    r = _launch("w_sc", torch.from_numpy(x).to(DEV), wr.params(min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-3), 77, gen)
    for b in (1, 2):
        assert r["nxt"][b] == 0 and not np.isfinite(r["lp"][b, gen[b]])
    keep = wr.survivors(x[0], min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-3)[0]
    assert bool(keep[r["nxt"][[0, 3]]].all())
