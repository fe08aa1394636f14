"""CPU: tests/select_ref.py against HF's warpers and tests/token_scores_ref.py, class E against a brute-force walk over all 2^24 uniforms,
the class G accept rule's non-vacuity and margins on the shared inputs, and the planted defects it and class E must reject."""
import numpy as np
import pytest
import torch

from conftest import pkg

import select_ref as sr
import token_scores_ref as tsr

ops = pkg("ops")
GEN = sr.gen_counts()


def _hf(x, T, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = TemperatureLogitsWarper(float(T))(None, torch.from_numpy(np.asarray(x, dtype=np.float32))[None].clone())
    if 0 < k:
        s = TopKLogitsWarper(top_k=int(k))(None, s)
    if p < 1.0:
        s = TopPLogitsWarper(top_p=float(p))(None, s)
    return torch.isfinite(s)[0].numpy()


# ------------------------------------------------------------------------------------------------ the survivor set
@pytest.mark.parametrize("name", sr.G_NAMES)
def test_survivor_set_is_hfs_and_warps_on_the_class_g_inputs(name):
    x, T, k, p = sr.g_case(name)
    keep, warped, _ = sr.survivors(x, T, k, p)
    assert np.array_equal(keep, _hf(x, T, k, p))
    w = tsr.warp(torch.from_numpy(x)[None], T, k, p)[0].numpy()
    assert np.array_equal(keep, np.isfinite(w))
    # the warped scores themselves: x / T up to the shift by the maximum
    np.testing.assert_allclose(warped[keep] - warped[keep].max(), w[keep] - w[keep].max(), rtol=0, atol=1e-12)


def test_survivor_set_on_the_small_sets_and_where_it_leaves_hf():
    for name, (x, T, k, p, want) in sr.set_cases().items():
        keep, _, margins = sr.survivors(x, T, k, p)
        assert set(np.flatnonzero(keep).tolist()) == want, name
        assert len(margins) == 0 or margins.min() > 0.05, name
        if name == "tie_across_top_p":
            # HF's sort splits the tied pair: it keeps one of the two.  This is the one place the two definitions part.
            hf = _hf(x, T, k, p)
            assert hf.sum() == 2 and hf[5] and (hf[1023] != hf[1024])
            assert set(np.flatnonzero(sr.hf_split_ties(x, T, k, p)).tolist()) == {5, 1023}
        elif name != "nan_in_the_seats":                                    # (torch.topk seats a NaN)
            assert np.array_equal(keep, _hf(x, T, k, p)), name
            assert np.array_equal(keep, np.isfinite(tsr.warp(torch.from_numpy(x)[None], T, k, p)[0].numpy())), name
    x, T, k, p, want = sr.set_cases()["nan_in_the_seats"]
    as_inf = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    assert np.array_equal(sr.survivors(x, T, k, p)[0], _hf(as_inf, T, k, p))


@pytest.mark.parametrize("V", [1, 3, 64, 1025, 4100])
def test_survivor_set_on_the_class_e_launches(V):
    for form in sr.E_FORMS:
        logits, T, k, p, idxs = sr.e_launch(V, form, rows=24)
        for b in range(24):
            keep, _, _ = sr.survivors(logits[b], T, k, p)
            assert np.array_equal(np.flatnonzero(keep), idxs[b]), (V, form, b)
            assert sr.is_class_e(logits[b], keep)


def test_survivor_set_on_class_e_rows_at_128256():
    for form in ("plain", "p_tiny_t100", "k_below_ties", "k_is_ties_stride"):
        logits, T, k, p, idxs = sr.e_launch(128256, form, rows=8)
        for b in range(8):
            assert np.array_equal(np.flatnonzero(sr.survivors(logits[b], T, k, p)[0]), idxs[b]), (form, b)


def test_top_k_zero_and_top_k_at_least_v_are_no_top_k():
    x = sr.gauss_row(1000)
    for k in (0, 1000, 1001):
        assert sr.survivors(x, 1.0, k, 1.0)[0].all()
    x[7] = np.nan
    keep = sr.survivors(x, 1.0, 0, 1.0)[0]
    assert not keep[7] and keep.sum() == 999


# ------------------------------------------------------------------------------------------------ class E
@pytest.mark.parametrize("n", [1, 2, 1023, 131072])
def test_class_e_formula_is_the_two_level_walk_for_every_uniform(n):
    """all 2^24 values of u, every token a survivor: thread t owns min(Cn, n - t Cn) of them"""
    u = np.arange(1 << 24, dtype=np.float64) / float(1 << 24)
    Cn = -(-n // sr.THREADS)
    counts = np.clip(n - np.arange(sr.THREADS) * Cn, 0, Cn)
    assert counts.sum() == n
    walk = sr.class_e_walk(u, counts)
    formula = sr.class_e_ordinal(u, n)
    assert np.array_equal(walk, formula)
    assert formula.min() == 0 and formula.max() == n - 1


def test_class_e_walk_on_sparse_slices():
    """survivors in the first, the last or every 1 023rd place: empty slices in between, and an empty slice 1 023 (V = 1 025)"""
    u = np.arange(0, 1 << 24, 7, dtype=np.float64) / float(1 << 24)
    for V in (1025, 2049, 4100, 128256):
        Cn = -(-V // sr.THREADS)
        for which in range(sr.N_PATTERNS):
            idx = sr.e_pattern(V, which)
            counts = np.bincount(idx // Cn, minlength=sr.THREADS)
            assert np.array_equal(sr.class_e_walk(u, counts), sr.class_e_ordinal(u, len(idx))), (V, which)


# ------------------------------------------------------------------------------------------------ class G: margins and non-vacuity
def test_every_top_p_decision_of_the_class_g_inputs_has_a_margin():
    for name in sr.G_NAMES:
        x, T, k, p = sr.g_case(name)
        margins = sr.survivors(x, T, k, p)[2]
        assert len(margins) == 0 or margins.min() >= 1e-3, (name, margins.min())


@pytest.mark.parametrize("name", sr.G_NAMES)
def test_accept_rule_pins_the_token_for_most_draws(name):
    x, T, k, p = sr.g_case(name)
    keep, warped, _ = sr.survivors(x, T, k, p)
    assert keep.sum() <= 64
    u = sr.uniforms(ops.sample_uniform, sr.SEED, GEN)
    idx, ok, _ = sr.accept_rule(warped, u)
    admitted = ok.sum(axis=1)
    share = float((admitted == 1).mean())
    print(f"{name}: {int(keep.sum())} survivors, 2 eta = {2 * sr.eta(warped):.3e}, exactly one token admitted for {100 * share:.1f} % of {len(u)} draws")
    assert admitted.min() >= 1 and admitted.max() <= 2
    assert share >= 0.95
    # and over a fine grid of u, not only this launch's
    grid = (np.arange(1 << 16, dtype=np.float64) + 0.5) / float(1 << 16)
    adm = sr.accept_rule(warped, grid)[1].sum(axis=1)
    print(f"{name}: over 65 536 evenly spaced u: {100 * float((adm == 1).mean()):.2f} %")
    assert adm.min() >= 1 and adm.max() <= 2 and float((adm == 1).mean()) >= 0.95


def test_eta_is_the_sum_of_its_terms():
    x, T, k, p = sr.g_case("v1025_t07_k20_p09")
    warped = sr.survivors(x, T, k, p)[1]
    A = tsr._row_stats(warped, int(np.argmax(warped)))[0]
    assert sr.eta(warped) == sr.HIGHER_ORDER * sr.U * (5 * A + 4 + 2 + 1024 + 1)
    assert sr.sampled_logprob_bound is tsr.bound_sample


# ------------------------------------------------------------------------------------------------ the emulation and the planted defects
def _g_picks(name, defect, u):
    x, T, k, p = sr.g_case(name)
    return sr.emulate(x, T, k, p, u, defect=defect)


def _g_rejects(name, picks, u):
    x, T, k, p = sr.g_case(name)
    return sr.check_draws(sr.survivors(x, T, k, p)[1], u, picks)[0] != ""


def _e_rejections(V, form, seed, defect=None, du=(0, 0)):
    """draws of the emulated sampler on one class E launch that differ from the exact pick"""
    logits, T, k, p, idxs = sr.e_launch(V, form)
    wrong = 0
    for b in range(sr.B):
        keep = np.zeros(V, dtype=bool)
        keep[idxs[b]] = True
        u_ref = ops.sample_uniform(seed, b, GEN[b])
        u_got = ops.sample_uniform(seed, b + du[0], GEN[b] + du[1])
        got = sr.emulate(logits[b], T, k, p, [u_got], defect=defect, keep=keep)[0]
        wrong += int(got != sr.class_e_pick(np.array([u_ref]), keep)[0])
    return wrong


def test_the_emulated_sampler_passes_both_classes():
    u = sr.uniforms(ops.sample_uniform, sr.SEED, GEN)
    for name in sr.G_NAMES:
        assert not _g_rejects(name, _g_picks(name, None, u), u), name
    for V in (3, 1025, 4100):
        for form in sr.E_FORMS:
            assert _e_rejections(V, form, sr.SEED) == 0, (V, form)


@pytest.mark.parametrize("defect", ["slice_off_by_one", "sorted_cdf"])
def test_class_g_rejects_a_wrong_walk(defect):
    u = sr.uniforms(ops.sample_uniform, sr.SEED, GEN)
    caught = [name for name in sr.G_NAMES if _g_rejects(name, _g_picks(name, defect, u), u)]
    print(defect, "rejected by", caught)
    assert caught


def test_class_e_rejects_a_slice_boundary_off_by_one():
    assert _e_rejections(4100, "plain", sr.SEED, "slice_off_by_one") > 0
    assert _e_rejections(1025, "plain", sr.SEED, "slice_off_by_one") > 0


def test_class_e_rejects_ge_for_gt_in_the_walk():
    seed = sr.e_seed(ops.sample_uniform, GEN)
    assert _e_rejections(128256, "plain", seed) == 0
    assert _e_rejections(128256, "plain", seed, "ge_in_walk") > 0


@pytest.mark.parametrize("du", [(1, 0), (0, 1)])
def test_both_classes_reject_a_uniform_from_the_wrong_row_or_step(du):
    assert _e_rejections(1025, "plain", sr.SEED, None, du) > 0
    u = sr.uniforms(ops.sample_uniform, sr.SEED, GEN)
    u_wrong = sr.uniforms(ops.sample_uniform, sr.SEED, [g + du[1] for g in GEN], rows=[b + du[0] for b in range(sr.B)])
    for name in sr.G_NAMES:
        assert _g_rejects(name, _g_picks(name, None, u_wrong), u), name


def _set_seed():
    cases = sr.set_cases()
    return sr.covering_seed(ops.sample_uniform, [sr.survivors(x, T, k, p)[1] for x, T, k, p, _ in cases.values()], GEN)


def test_survivor_set_checks_reject_a_seated_nan_and_split_ties():
    seed = _set_seed()
    u = sr.uniforms(ops.sample_uniform, seed, GEN)
    cases = sr.set_cases()
    for name, (x, T, k, p, want) in cases.items():
        assert set(sr.emulate(x, T, k, p, u).tolist()) == want, name            # the sound sampler draws exactly the set
    x, T, k, p, want = cases["nan_in_the_seats"]
    assert set(sr.emulate(x, T, k, p, u, defect="nan_takes_seat").tolist()) != want
    x, T, k, p, want = cases["tie_across_top_p"]
    assert set(sr.emulate(x, T, k, p, u, defect="ties_split").tolist()) != want
