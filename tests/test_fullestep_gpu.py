"""The full-covariance E-step (ghmm_estep_full: k_emission_full<DB, FC_POST>, the shared scans,
k_fullstats / k_fullstats_reduce) and M-step over the shape range the library is built for, against
the extended-precision restatement tests/fulltrain_ref.py — GPU box only.  The restatement itself
is pinned on the CPU by test_fulltrain_ref_host.py.

(a) b, post, gamma, the transition sums, den_c and the log-likelihoods against estep(...,
    longdouble) rounded to double, under fullcov_support.close (rtol 1e-11, floor 1e-11 x block
    maximum, equal zeros for b and post), with three changes: gamma and post get 1e-11 absolute
    per entry (a frame's own maximum is 1) instead of the array's maximum; b is held column by
    column (a state's densities are one block, so that the 1e20 of a clamped Gaussian does not
    excuse the other states); the per-utterance log-likelihoods are compared one by one, with an
    equal -inf / NaN pattern.
(b) the statistics kernel alone: num_c, num_mu, num_cov against stats_from() of the DEVICE's own
    gamma and post.  Every entry e must satisfy
        |got_e - ref_e| <= (2 F + 8) * 2^-53 * sum_f |term_{e,f}|
    which is derived, not measured: a term carries at most four roundings before it is added
    (gamma * post, the two differences, w * dif_k; the fma adds the product unrounded), and any
    order of at most F + P additions (P <= F partial blocks) loses at most (F + P) * 2^-53 of the
    sum of absolute values, to first order.  No floor, no block maximum: an entry whose terms are
    all 0 must be exactly 0.
(c) ghmm_mstep_full equals the host M-step of the downloaded statistics bit for bit, GHMM_OPT_DELTA
    included.
(d) four EM iterations beyond the real reference's compiled-in caps against the long-double
    trajectory (log-likelihood rel 1e-9, model 1e-8: the bars of test_gpu_parity's
    test_ten_em_iterations_track_the_oracle and of fullcov_support.check_run).
The cases (fulltrain_ref.CASES, build) and the two checkers (fullcov_support.check_estep for (a),
check_stats_bound for (b)) are shared with the log-domain E-step's tests."""
import numpy as np
import pytest

import fulltrain_ref as R
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import (assert_close, check_estep, check_stats_bound, extended, f64, rand_fmodel, run_device,
                             walk_any)
from fulltrain_ref import build

pytestmark = pytest.mark.gpu


def zero_weight_passes(dev, N, M, D):
    """aligned runs of FSn frames whose gamma * post is exactly 0 for every Gaussian of an element
    batch: the passes k_fullstats skips as a whole (frame blocks start at multiples of FSn)"""
    fsn, batches = R.fs_geometry(N, M, D)
    F = dev["gamma"].shape[0]
    w = np.repeat(dev["gamma"], M, axis=1) * dev["post"]
    n = 0
    for g0, g1 in batches:
        nz = (w[:, g0:g1 + 1] != 0.0).any(1)
        n += sum(1 for f in range(0, F, fsn) if not nz[f:f + fsn].any())
    return fsn, n


# ------------------------------------------------------------- (a) and (b), the sweep

@extended
@pytest.mark.parametrize("name", R.SWEEP)
def test_estep_arrays_against_the_extended_reference(G, ctx, name):
    hm, X, lens, delta, ref = build(G, name)
    dev = run_device(G, ctx, hm, X, lens, log=False, delta=delta)
    check_estep(dev, ref, hm, lens, delta, name)
    if name == "short-12x2x6":
        o = np.concatenate([[0], np.cumsum(lens)])
        for u in (1, 2):    # T = 5 and T = 1 under 12 states
            assert np.all(dev["gamma"][o[u]:o[u + 1]] == 0.0) and dev["ll"][u] == -np.inf


@extended
@pytest.mark.parametrize("name", R.SWEEP)
def test_statistics_within_the_derived_bound(G, ctx, name):
    hm, X, lens, delta, _ = build(G, name)
    dev = run_device(G, ctx, hm, X, lens, log=False, delta=delta)
    worst = check_stats_bound(dev, X, hm, name)
    fsn, skipped = zero_weight_passes(dev, hm.N, hm.M, hm.D)
    print(f"{name}: F = {len(X)}, FSn = {fsn}, whole passes of zero weight = {skipped}, "
          f"worst error / bound = {worst:.4f}")
    # the LDS-driven reduction of the frames per pass is reached where it is meant to be
    assert fsn == {"fsn-64x4x1": 16, "fsn-64x8x1": 8, "fsn-64x3x3": 16}.get(name, 32)


@extended
@pytest.mark.parametrize("name", ["many-8x3x16", "fsn-64x8x1", "large-64x2x48"])
def test_statistics_bound_under_partials(G, ctx, name):
    """GHMM_OPT_PARTIALS = 1 (one frame block: about F / FSn passes of the frame loop), 3 and 0
    (auto).  gamma and post do not depend on the setting, so one reference serves all three; the
    statistics of two settings are only held to the bound, repeated calls at one setting are
    bitwise equal.  With 64 states and D = 48 a batch of elements covers two or three Gaussians,
    whose weights are exactly 0 over whole passes (alpha is exactly 0 for state j before frame j
    of an utterance): the kernel's skip of a whole pass is reached, which the host asserts."""
    hm, X, lens, delta, _ = build(G, name)
    first = None
    for partials in (1, 3, 0):
        dev = run_device(G, ctx, hm, X, lens, log=False, delta=delta, options=((G.OPT_PARTIALS, partials),), twice=True)
        if first is None:
            first = dev
        else:
            assert np.array_equal(dev["gamma"], first["gamma"]) and np.array_equal(dev["post"], first["post"])
        worst = check_stats_bound(dev, X, hm, f"{name} partials={partials}")
        fsn, skipped = zero_weight_passes(dev, hm.N, hm.M, hm.D)
        print(f"{name} partials={partials}: F = {len(X)}, FSn = {fsn}, whole passes of zero weight = "
              f"{skipped}, worst error / bound = {worst:.4f}")
        assert len(X) > 8 * fsn     # several passes per block with one partial
        if name == "large-64x2x48":
            assert skipped > 0


@extended
def test_three_scan_paths(G, ctx):
    """the fused scan (default), GHMM_OPT_KERNELS = 1 (reference order, separate launches) and
    GHMM_OPT_FUSED_SCAN = 2 (paired scans, separate launches) on one case: each against the
    reference, and their statistics against each other at test_paired_scans_equal_the_reference_
    order's bar"""
    name = "paths-8x3x16"
    hm, X, lens, delta, ref = build(G, name)
    out = {}
    for tag, options in (("fused", ()), ("kernels1", ((G.OPT_KERNELS, 1),)), ("separate", ((G.OPT_FUSED_SCAN, 2),))):
        out[tag] = dev = run_device(G, ctx, hm, X, lens, log=False, delta=delta, options=options)
        check_estep(dev, ref, hm, lens, delta, f"{name} {tag}")
        check_stats_bound(dev, X, hm, f"{name} {tag}")
    for tag in ("kernels1", "separate"):
        for key in ("gamma", "ll", "v"):
            assert_close(out[tag][key], out["fused"][key], rtol=1e-9, what=f"{tag} {key}")


def test_empty_corpus(G, ctx):
    """no utterances: estep_full succeeds (k_fullstats_reduce runs over zero partial blocks) and
    every entry of the statistics is exactly 0"""
    rng = np.random.default_rng(41)
    N, M, D = 4, 2, 6
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    fm = ctx.full_model(hm)
    st = ctx.stats_full(N, M, D)
    busy = ctx.corpus(walk_any(rng, hm, [30]), [30])
    empty = ctx.corpus(np.zeros((0, D)), np.zeros(0, dtype=np.int32))
    try:
        ctx.estep_full(fm, busy, st)        # the vector holds something first
        assert np.any(st.download() != 0.0)
        ctx.estep_full(fm, empty, st)
        assert np.all(st.download() == 0.0)
    finally:
        for o in (st, fm, busy, empty):
            o.close()


@extended
def test_only_short_utterances(G, ctx):
    """every utterance shorter than the model: no path into the last state, the Gaussian sums are
    exactly 0 and the log-likelihoods are the reference's -inf"""
    rng = np.random.default_rng(43)
    N, M, D = 12, 2, 6
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    lens = np.array([5, 1, 11, 3], dtype=np.int32)
    X = walk_any(rng, hm, lens)
    ref = R.estep(hm, X, lens, 1, np.longdouble)
    assert np.all(f64(ref["loglik"]) == -np.inf)
    dev = run_device(G, ctx, hm, X, lens, log=False)
    check_estep(dev, ref, hm, lens, 1, "short only")
    for key in ("num_c", "num_mu", "num_cov"):
        assert np.all(dev["stats"][key] == 0.0), key
    check_stats_bound(dev, X, hm, "short only")


# ------------------------------------------------------------- (c) the M-step's plumbing

@pytest.mark.parametrize("N,M,D,lens,dense,delta", [
    (6, 2, 1, (120, 90, 150), False, 1),
    (5, 2, 48, (300, 280, 320), False, 1),
    (33, 2, 4, (120, 90, 150), False, 1),
    (6, 2, 9, (120, 90, 150), True, 0),
    (6, 2, 9, (120, 90, 150), True, 2),
])
def test_mstep_equals_host_mstep(G, ctx, N, M, D, lens, dense, delta):
    """ghmm_mstep_full reads GHMM_OPT_DELTA through the context.  The dense cases take their
    statistics under a band of 3, wider than the M-step's, so that the M-step's own band shows."""
    rng = np.random.default_rng(1000 * N + 10 * D + delta)
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    if dense:
        A = rng.random((N, N)) + 0.05
        hm.A[:] = A / A.sum(1, keepdims=True)
    X = walk_any(rng, hm, lens)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.set_option(G.OPT_DELTA, 3 if dense else delta)
        ctx.estep_full(fm, corpus, st)
        v = st.download()
        ctx.set_option(G.OPT_DELTA, delta)
        ref = hm.mstep(v, delta=delta)
        ctx.mstep_full(fm, st)
        got = fm.get()
        for a, b in zip(got.arrays(), ref.arrays()):
            np.testing.assert_array_equal(a, b)
        if dense:   # the band matters: delta = 1 gives another matrix
            assert not np.array_equal(got.A, hm.mstep(v, delta=1).A)
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
        st.close(); fm.close(); corpus.close()


# ------------------------------------------------------------- (d) several EM iterations

@extended
@pytest.mark.parametrize("N,M,D,U,T", R.EM_CASES)
def test_four_em_iterations_track_the_extended_reference(G, ctx, N, M, D, U, T):
    """from HostFullModel.init_from; the cases' conditioning (float64 against long double, a
    hundredth of these bars) is asserted by test_fulltrain_ref_host.py"""
    X, lens = R.em_corpus(N, M, D, U, T)
    trace, ref_hm = R.em_trajectory(G, X, lens, N, M, 4, np.longdouble)
    assert np.all(np.isfinite(trace))
    fm, corpus = ctx.full_model(G.HostFullModel.init_from(X, lens, N, M)), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        got = []
        for _ in range(4):
            ctx.estep_full(fm, corpus, st)
            got.append(st.loglik()[0])
            ctx.mstep_full(fm, st)
        hm = fm.get()
    finally:
        st.close(); fm.close(); corpus.close()
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(got, trace))
    e_model = R.model_err(hm, lambda k: getattr(ref_hm, k))
    print(f"{(N, M, D, U * T)}: trace error {e_tr:.1e}, model error {e_model:.1e}")
    assert e_tr <= 1e-9
    assert e_model <= 1e-8
