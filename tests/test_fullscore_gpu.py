"""The linear full-covariance recogniser (ghmm_emission_full, ghmm_score_full, ghmm_score_full_batch:
k_emission_full<DB, FC_LIN> and the score-only scan forward_run<L, BANDED, false, false, EXACT>) over
the shape range the library is built for, against the long-double restatement tests/fullscore_ref.py —
GPU box only.  The restatement and the cases are pinned on the CPU by test_fullscore_host.py.

(1) the emission at every DB, both sides of each boundary, under fullcov_support.close_b (equal NaN /
    inf / zero pattern, rtol 1e-11);
(2) the score at lane classes 16 / 32 / 64 with banded and dense A, every tail residue of the scan's
    unrolled loop, T = 0, T = 1, T < N, utterances stored out of length order: end to end at the 1e-11
    test_fullcov_gpu holds this call to; the lattice alone, on the device's own b, at 1e-12 (about 300
    times the float64 restatement's worst distance from long double, fullscore_ref's docstring; where
    the float64 restatement on the device's b is itself further than 1e-13 from long double the bar
    of that case is 8 times that distance: no case needs it, the test prints the figures); the batch
    of words from three lane classes bit for bit the single calls;
(3) utterances past 512 frames, where the scan's accumulator (log_product) folds its mantissa
    product's exponent back in, and past about 2 044, where the product would leave the normal range
    without the fold: 1e-11 against long double, the batch bit for bit the single call."""
import numpy as np
import pytest

import fullscore_ref as FR
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import close_b, extended, rel_dist

pytestmark = pytest.mark.gpu

SWEEP_IDS = [FR.sweep_id(c) for c in FR.SWEEP]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------- (1) the emission

@extended
@pytest.mark.parametrize("D", FR.EMISSION_D)
def test_linear_emission_at_every_db(G, ctx, D):
    """5 x 3 x D, one asymmetric inverse covariance (the inv_cov[j][i] order), 233 frames = three tiles
    of 64 and one of 41, frame 40 sixty units from everything: densities that are 0"""
    hm, X, lens = FR.emission_case(G, D)
    ref = FR.emission(hm, X).astype(np.float64)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    try:
        ctx.emission_full(fm, corpus)
        b = ctx.fetch(G.BUF_B, (corpus.frames, hm.N))
    finally:
        fm.close(); corpus.close()
    fin = np.isfinite(ref) & (ref != 0)
    print(f"D={D}: worst relative error {np.max(np.abs(b[fin] - ref[fin]) / np.abs(ref[fin])):.2e} (bar 1e-11)")
    close_b(b, ref)
    assert (ref[FR.FAR_FRAME] == 0).all() and (ref > 0).any()


# ------------------------------------------------------------- (2) the score sweep

@extended
@pytest.mark.parametrize("case", FR.SWEEP, ids=SWEEP_IDS)
def test_score_sweep_end_to_end(G, ctx, case):
    """score_full against the long-double score: equal NaN / inf pattern, 1e-11 relative; T = 0 gives
    +0.0; the utterances shorter than a banded model are held to the reference's value like the rest"""
    hm, X, lens = FR.sweep_case(G, case)
    ref = FR.reference(G, "sweep", case)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    try:
        got = ctx.score_full(fm, corpus)
    finally:
        fm.close(); corpus.close()
    empty = lens == 0
    assert empty.sum() == 1 and (got[empty] == 0.0).all() and not np.signbit(got[empty]).any()
    d = rel_dist(got, ref)
    short = (lens < hm.N) & ~empty
    d_short = rel_dist(got[short], ref[short])
    print(f"{FR.sweep_id(case)}: worst relative error {d:.2e}, over the {short.sum()} utterances of T < N "
          f"{d_short:.2e} (bar 1e-11: ratio {d / 1e-11:.3f})")
    assert d <= 1e-11


@extended
@pytest.mark.parametrize("case", FR.SWEEP, ids=SWEEP_IDS)
def test_score_sweep_lattice_alone(G, ctx, case):
    """the long-double recursion on the device's own b (fetched after the call): 1e-12 relative, or 8
    times the float64 restatement's own distance on that b where that is beyond 1e-13 (see the
    module's docstring: nowhere)"""
    hm, X, lens = FR.sweep_case(G, case)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    try:
        got = ctx.score_full(fm, corpus)
        b = ctx.fetch(G.BUF_B, (corpus.frames, hm.N))
    finally:
        fm.close(); corpus.close()
    exact = FR.lattice_scores(hm.A, b, lens)
    d64 = rel_dist(FR.lattice_scores(hm.A, b, lens, np.float64), exact)
    bar = 1e-12 if d64 <= 1e-13 else 8.0 * d64
    d = rel_dist(got, exact)
    print(f"{FR.sweep_id(case)}: lattice alone {d:.2e}, float64 restatement {d64:.2e}, bar {bar:.1e}: "
          f"ratio {d / bar:.4f}")
    assert d <= bar


def test_score_sweep_batch_equals_single_calls(G, ctx):
    """three words of one corpus, a dense one with zeros on 16 lanes, a dense one on 32 and a banded
    one on 64 (the batch runs them all on 64): score_full_batch = score_full bit for bit"""
    hm, X, lens = FR.sweep_case(G, FR.BATCH_BASE)
    small, wide = FR.batch_models(G)
    hms = [small, hm, wide]
    assert [16 if h.N <= 16 else 32 if h.N <= 32 else 64 for h in hms] == [16, 32, 64]
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    try:
        batch = ctx.score_full_batch(fms, corpus)
        assert batch.shape == (3, len(lens)) and np.isfinite(batch).all()
        for k, fm in enumerate(fms):
            assert np.array_equal(bits(batch[k]), bits(ctx.score_full(fm, corpus))), k
        assert np.array_equal(bits(batch), bits(ctx.score_full_batch(fms, corpus)))   # reproducible
    finally:
        for o in fms + [corpus]:
            o.close()


# ------------------------------------------------------------- (3) long utterances

@extended
@pytest.mark.parametrize("name", sorted(FR.LONG))
def test_long_utterances_through_the_score_only_scan(G, ctx, name):
    """score_full, and score_full_batch with a three-state word in front (the word under test reads b
    with another stride and from a column offset), against long double at 1e-11; the batch bit for bit
    the single calls.  test_fullscore_host.test_long_cases_bite shows on the CPU what a wrong fold does
    to each of these lengths."""
    hm, small, X, lens = FR.long_case(G, name)
    ref = FR.reference(G, "long", name)
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(small), ctx.full_model(hm)]
    try:
        one = ctx.score_full(fms[1], corpus)
        batch = ctx.score_full_batch(fms, corpus)
        first = ctx.score_full(fms[0], corpus)
    finally:
        for o in fms + [corpus]:
            o.close()
    for u, T in enumerate(lens):
        print(f"{name} T={T}: score_full {rel_dist(one[u:u + 1], ref[u:u + 1]):.2e}, "
              f"score_full_batch {rel_dist(batch[1, u:u + 1], ref[u:u + 1]):.2e} (bar 1e-11)")
    d1, db = rel_dist(one, ref), rel_dist(batch[1], ref)
    print(f"{name}: worst error / bar {max(d1, db) / 1e-11:.4f}")
    assert d1 <= 1e-11 and db <= 1e-11
    assert np.array_equal(bits(batch[1]), bits(one)) and np.array_equal(batch[0], first, equal_nan=True)
