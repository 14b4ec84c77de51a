"""CPU-side tests (no GPU) of the linear full-covariance score's restatement (fullscore_ref.py) and of
the cases test_fullscore_gpu.py runs: the float64 form is the pinned np_emission / np_logp (the
float64 family, written separately in the same module) bit for bit; its distance from the long-double
form at every shape; no sweep utterance of at least N frames has a NaN reference; and every long case
reaches what it is there for, shown by running the score-only scan's accumulator (log_product) on the CPU over the case's own c_t in its right form
and its two broken ones.  These are conditions on the inputs, not on the device: a case that fails
them is replaced, not excused."""
import numpy as np
import pytest

import fullscore_ref as FR
from fullcov_support import extended, offsets, rel_dist
from fullscore_ref import np_emission, np_logp


SWEEP_IDS = [FR.sweep_id(c) for c in FR.SWEEP]


def test_float64_form_is_the_pinned_restatement(G):
    """emission() and logp() in float64 = np_emission and np_logp, bit for bit, the far
    frame's zeros and an utterance of one frame included"""
    hm, X, lens = FR.emission_case(G, 9)
    b = FR.emission(hm, X, np.float64)
    ref = np_emission(hm, X)
    assert b.dtype == np.float64 and np.array_equal(b.view(np.uint64), ref.view(np.uint64))
    assert (b[FR.FAR_FRAME] == 0).all() and (b > 0).any()
    off = offsets(lens)
    for u in range(len(lens)):
        got, want = FR.logp(hm.A, b[off[u]:off[u + 1]], np.float64), np_logp(hm.A, ref[off[u]:off[u + 1]])
        assert np.array_equal(np.float64(got).view(np.uint64), np.float64(want).view(np.uint64)), u
    hm, X, lens = FR.sweep_case(G, FR.SWEEP[1])        # a dense A, T = 0 among the utterances
    b = np_emission(hm, X)
    off = offsets(lens)
    got = FR.score(hm, X, lens, np.float64)
    want = np.array([np_logp(hm.A, b[off[u]:off[u + 1]]) for u in range(len(lens))])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert got[list(lens).index(0)] == 0.0


def spread(hm, X, lens, ref):
    d = rel_dist(FR.score(hm, X, lens, np.float64), ref)
    assert d <= 1e-13
    return d


@extended
@pytest.mark.parametrize("case", FR.SWEEP, ids=SWEEP_IDS)
def test_float64_spread_sweep(G, case):
    """the float64 form against the long-double one (the figure in fullscore_ref's docstring); every
    utterance of at least N frames has a finite reference, so none compares NaN with NaN by accident,
    and the shorter ones on a banded A are finite too: this score has no final-state term"""
    hm, X, lens = FR.sweep_case(G, case)
    ref = FR.reference(G, "sweep", case)
    print(f"{FR.sweep_id(case)}: float64 spread {spread(hm, X, lens, ref):.1e}")
    assert sorted(lens) == sorted(FR.SWEEP_LENS) and len(lens) == 37
    r64 = ref.astype(np.float64)
    assert not np.isnan(r64[lens >= hm.N]).any()
    assert np.isfinite(r64).all() and (r64[lens == 0] == 0.0).all() and (r64[lens > 0] != 0.0).all()


@extended
@pytest.mark.parametrize("name", sorted(FR.LONG))
def test_float64_spread_long(G, name):
    hm, _, X, lens = FR.long_case(G, name)
    ref = FR.reference(G, "long", name)
    assert np.isfinite(ref.astype(np.float64)).all()
    print(f"{name}: float64 spread {spread(hm, X, lens, ref):.1e}")


@extended
@pytest.mark.parametrize("name", sorted(FR.LONG))
def test_long_cases_bite(G, name):
    """log_product on the CPU over the float64 pass's c_t.  With the fold it is the reference's log P
    to 1e-13.  A fold that drops the exponent moves log P by more than 1e-4 relative from 512 values
    on (the 512th value is the first to fold) and by nothing below.  Without a fold the mantissa
    product leaves the normal range (< 2^-1022) on the lengths marked for it, and on no other: there
    the unfolded product is still the reference's log P, so only the marked lengths can tell a
    missing fold."""
    hm, _, X, lens = FR.long_case(G, name)
    marked = FR.LONG[name][5]
    ref = FR.reference(G, "long", name)
    b = FR.emission(hm, X, np.float64)
    off = offsets(lens)
    for u, T in enumerate(lens):
        lp, cs = FR.forward(hm.A, b[off[u]:off[u + 1]], np.float64)
        assert cs.dtype == np.float64 and len(cs) == T
        r = float(ref[u])
        exact, _ = FR.log_product_emulated(cs, "exact")
        drop, _ = FR.log_product_emulated(cs, "drop")
        none, least = FR.log_product_emulated(cs, "none")
        d_exact, d_drop = abs(-exact - r) / abs(r), abs(-drop - r) / abs(r)
        d_none = abs(-none - r) / abs(r) if np.isfinite(none) else np.inf
        print(f"{name} T={T}: with the fold {d_exact:.1e}, exponent dropped {d_drop:.1e}, no fold {d_none:.1e} "
              f"(smallest mantissa product 2^{np.log2(least) if least > 0 else -np.inf:.0f})")
        assert d_exact <= 1e-13 and abs(-exact - float(lp)) <= 1e-13 * abs(r)
        if T >= FR.FOLD_EVERY:
            assert d_drop > 1e-4
        else:
            assert drop == exact
        if T in marked:
            assert least < 2.0 ** -1022 and d_none > 1e-4
        else:
            assert least >= 2.0 ** -1022 and d_none <= 1e-13
    assert set(marked) <= set(int(T) for T in lens)

