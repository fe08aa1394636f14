"""CPU: tests/warp_ref.py (the warped sampler's definition) held to the installed transformers warpers, chained in HF's order
behind temperature / top-k / top-p; the committed inputs shown to clear every boundary by 4 x the kernel's derived fp32 error, to
discriminate the planted defects, and — class G — to pin nearly every draw to one token."""
import numpy as np
import pytest
import torch

import select_ref as sr
import warp_ref as wr

lp = pytest.importorskip("transformers.generation.logits_process")


def hf_keep(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """the survivor set of HF's own warpers in HF's order (generation/utils.py _get_logits_processor), fp64 scores, NaN read as -inf"""
    s = torch.from_numpy(sr.clean(x))[None, :]
    chain = [lp.TemperatureLogitsWarper(float(temperature))] if temperature != 1.0 else []
    if 0 < top_k < s.shape[1]:
        chain.append(lp.TopKLogitsWarper(top_k=int(top_k)))
    if top_p < 1.0:
        chain.append(lp.TopPLogitsWarper(top_p=float(top_p)))
    if min_p > 0.0:
        chain.append(lp.MinPLogitsWarper(min_p=wr.f32(min_p)))
    if typical_p < 1.0:
        chain.append(lp.TypicalLogitsWarper(mass=wr.f32(typical_p)))
    if epsilon_cutoff > 0.0:
        chain.append(lp.EpsilonLogitsWarper(epsilon=wr.f32(epsilon_cutoff)))
    if eta_cutoff > 0.0:
        chain.append(lp.EtaLogitsWarper(epsilon=wr.f32(eta_cutoff)))
    ids = torch.zeros(1, 1, dtype=torch.long)
    for w in chain:
        s = w(ids, s)
    return torch.isfinite(s[0]).numpy()


def _rows():
    """every committed row with its parameters: the class G rows, the ladders, one row of every class E pattern at every size"""
    for name in wr.G_NAMES:
        yield (name, *wr.g_case(name))
    for name in wr.LADDERS:
        yield (name, *wr.ladder(name))
    for V in wr.SIZES:
        for form in wr.E_FORMS:
            logits, p, _ = wr.e_launch(V, form, rows=3 * sr.N_PATTERNS)
            for b in range(logits.shape[0]):
                yield (f"e_{form}_v{V}_{b}", logits[b], p)


# the 13 parameter forms every Gaussian row below runs under
FORMS = [wr.params(min_p=0.1), wr.params(min_p=1.0), wr.params(typical_p=0.2), wr.params(typical_p=0.95), wr.params(epsilon_cutoff=3e-4),
         wr.params(epsilon_cutoff=0.999), wr.params(eta_cutoff=2e-3), wr.params(eta_cutoff=0.6), wr.params(top_k=1, min_p=0.2, typical_p=0.5),
         wr.params(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05), wr.params(temperature=1.3, typical_p=0.9, epsilon_cutoff=1e-3),
         wr.params(temperature=0.8, top_p=0.95, typical_p=0.6, eta_cutoff=0.01),
         wr.params(temperature=0.9, top_k=100, top_p=0.98, min_p=0.01, typical_p=0.8, epsilon_cutoff=1e-3, eta_cutoff=5e-3)]


def test_restatement_equals_the_transformers_warpers_on_every_committed_input():
    n = 0
    for name, x, p in _rows():
        keep = wr.survivors(x, **p)[0]
        assert np.array_equal(keep, hf_keep(x, **p)), (name, int(keep.sum()))
        n += 1
    print(f"{n} committed rows: survivor sets equal to transformers'")


@pytest.mark.parametrize("V", wr.SIZES)
def test_restatement_equals_the_transformers_warpers_on_gaussian_rows(V):
    """Gaussian rows with and without -inf / NaN holes under 13 parameter forms; a row whose top-p decision sits within 1e-9 of its
    boundary is no test of either side (select_ref: HF splits ties there) and is skipped"""
    n = 0
    for r in range(3):
        for holes in (False, True):
            x = sr.gauss_row(V, r)
            if holes:
                x = sr.with_holes(x)
                x[V // 3] = np.nan
            if not np.isfinite(sr.clean(x)).any():                          # a row of nothing (V = 1 with its hole): HF has no answer, the kernel's is token 0
                continue
            for p in FORMS:
                keep, _, clear = wr.survivors(x, **p)
                if "top_p" in clear and clear["top_p"][1] < 1e-9:
                    continue
                assert np.array_equal(keep, hf_keep(x, **p)), (V, r, holes, p)
                n += 1
    assert n >= 35, n


@pytest.mark.parametrize("V", [2, 65, 4099])
def test_greedy_degenerate_forms_leave_the_argmax(V):
    for r in range(3):
        x = sr.gauss_row(V, r)
        for p in (wr.params(min_p=1.0), wr.params(epsilon_cutoff=0.999), wr.params(top_k=1, typical_p=0.5, eta_cutoff=0.3)):
            keep = wr.survivors(x, **p)[0]
            assert np.flatnonzero(keep).tolist() == [int(np.argmax(x))], (V, r, p)


def test_a_band_drops_the_maximum():
    for name in ("band_peak_200", "band_60", "ladder_band"):
        x, p = wr.ladder(name)
        keep = wr.survivors(x, **p)[0]
        assert not keep[int(np.argmax(x))] and keep.any(), name
    x, p = wr.ladder("band_peak_200")
    assert int(wr.survivors(x, **p)[0].sum()) == 200


def test_v1_and_rows_of_nothing():
    every = wr.params(min_p=0.5, typical_p=0.5, epsilon_cutoff=0.5, eta_cutoff=0.5)
    assert wr.survivors(np.array([1.5], dtype=np.float32), **every)[0].tolist() == [True]
    assert not wr.survivors(np.array([np.nan, -np.inf], dtype=np.float32), **every)[0].any()


# ------------------------------------------------------------------------------------------------ input conditions
def test_every_decision_of_every_committed_input_clears_its_boundary():
    """4 x the derived fp32 error of the decided quantity (warp_ref's docstring has the count); the ladders keep 1e-2 in absolute terms"""
    worst = {}
    for name, x, p in _rows():
        clear = wr.survivors(x, **p)[2]
        for stage, (ratio, dist) in clear.items():
            assert ratio >= wr.NEED, (name, stage, ratio, dist)
            if name in wr.LADDERS:
                assert dist >= 1e-2, (name, stage, dist)
            worst[stage] = min(worst.get(stage, np.inf), ratio)
    print({k: round(v, 1) for k, v in worst.items()})
    assert set(worst) >= {"min_p", "typical_mass", "typical_band", "epsilon_cutoff", "eta_cutoff"}


def test_class_g_inputs_have_few_survivors_and_pin_their_draws():
    """at most 64 survivors, and select_ref.accept_rule — the reference alone — admits exactly one token for >= 95 % of the draws of a
    launch whose uniforms are 256 evenly spread values (any launch's are as good as these)"""
    u = (np.arange(sr.B) + 0.5) / sr.B
    names = list(wr.G_NAMES) + [n for n in wr.LADDERS if _n_survivors(n) <= 64]
    for name in names:
        x, p = wr.g_case(name) if name in wr.G_NAMES else wr.ladder(name)
        keep, warped, _ = wr.survivors(x, **p)
        assert 1 <= int(keep.sum()) <= 64, (name, int(keep.sum()))
        _, ok, _ = sr.accept_rule(warped, u)
        share = float((ok.sum(axis=1) == 1).mean())
        assert bool((ok.sum(axis=1) >= 1).all()) and share >= 0.95, (name, share)


def _n_survivors(name):
    x, p = wr.ladder(name)
    return int(wr.survivors(x, **p)[0].sum())


def test_class_e_forms_are_class_e():
    for V in wr.SIZES:
        for form in wr.E_FORMS:
            logits, p, idxs = wr.e_launch(V, form, rows=3 * sr.N_PATTERNS)
            for b in range(logits.shape[0]):
                keep = wr.survivors(logits[b], **p)[0]
                assert np.array_equal(np.flatnonzero(keep), idxs[b]) and sr.is_class_e(logits[b], keep), (V, form, b)


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("defect", wr.DEFECTS)
def test_planted_defects_change_a_survivor_set_on_the_committed_inputs(defect):
    changed = [name for name, x, p in _rows() if not np.array_equal(wr.survivors(x, **p)[0], wr.survivors(x, defect=defect, **p)[0])]
    print(defect, len(changed), changed[:6])
    assert changed, defect
