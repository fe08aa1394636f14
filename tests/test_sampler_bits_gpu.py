"""GPU, the sampler bit for bit: every launch of tools/record_sampler_bits.py (select_ref's class G and class E through sl_sample_select_sc;
warp_ref's class G, ladders and class E through sl_sample_select_w) draws the ids AND the log-probability words recorded in
tests/golden/sampler_bits.npz, which the two sampler kernels wrote before they were folded into one body.  The other
selection suites hold the draws to derived bounds; this one holds a change of the kernels to "no bit moved"."""
import functools

import numpy as np
import pytest

from conftest import golden, pkg

from tools import record_sampler_bits as rec

pytestmark = pytest.mark.gpu
CASES = rec.cases()
_recorded = functools.lru_cache(maxsize=None)(lambda: golden("sampler_bits"))


def test_the_fixture_holds_exactly_the_recorded_launches():
    assert set(_recorded()) == {c + s for c in CASES for s in ("__ids", "__lp")}


@pytest.mark.parametrize("case", list(CASES))
def test_sampler_draws_the_recorded_bits(case):
    want = _recorded()
    ids, words = rec.draw(pkg("ops"), CASES[case])
    wrong = np.flatnonzero(ids != want[case + "__ids"])
    assert wrong.size == 0, (case, f"{wrong.size} of {len(ids)} ids differ, first row {wrong[0]}: got {ids[wrong[0]]} recorded {want[case + '__ids'][wrong[0]]}")
    wrong = np.flatnonzero(words != want[case + "__lp"])
    assert wrong.size == 0, (case, f"{wrong.size} of {len(words)} log-probability words differ, first row {wrong[0]}: got "
                                   f"{words[wrong[0]:wrong[0] + 1].view(np.float32)[0]!r} recorded {want[case + '__lp'][wrong[0]:wrong[0] + 1].view(np.float32)[0]!r}")
