"""The full-covariance E-step (ghmm_estep_full: k_emission_full<DB, FC_POST>, the shared scans,
k_fullstats / k_fullstats_reduce) and M-step over the shape range the library is built for, against
the extended-precision restatement tests/fulltrain_ref.py — GPU box only.  The restatement itself
is pinned on the CPU by test_fulltrain_ref_host.py.

(a) b, post, gamma, the transition sums, den_c and the log-likelihoods against estep(...,
    longdouble) rounded to double, under test_fulltrain_gpu.close (rtol 1e-11, floor 1e-11 x block
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
    test_ten_em_iterations_track_the_oracle and of test_fulltrain_gpu.check_run)."""
import functools

import numpy as np
import pytest

import fulltrain_ref as R
from test_fulltrain_gpu import close, rand_model
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not R.have_extended(), reason="long double is no wider than double here")

U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------- the cases

def walk_any(rng, hm, lens):
    """test_fulltrain_gpu.walk (left-to-right walks, one mixture per frame, noise 0.3), also for
    utterances shorter than the model (one frame per state from the first) and of no frames"""
    out = [np.zeros((0, hm.D))]
    for T in lens:
        if T >= hm.N:
            cuts = np.sort(rng.choice(np.arange(1, T), hm.N - 1, replace=False))
            st = np.searchsorted(cuts, np.arange(T), side="right")
        else:
            st = np.arange(T)
        k = rng.integers(0, hm.M, T)
        out.append(hm.mean[st, k] + rng.normal(0.0, 0.3, (T, hm.D)))
    return np.concatenate(out)


LENS1 = (70, 1, 33, 129)        # 233 frames: three tiles of 64 and one with 41 frames left
LENS2 = (90, 140, 64, 65)
LONG64 = (312, 388, 400, 300, 351, 333, 379, 364)

# id -> (N, M, D, lens, dense A, delta, clamped Gaussian)
CASES = {}
for _D in (8, 9, 17, 24, 25, 33, 40, 41, 47, 48):       # every DB of FC_POST, both sides of each boundary
    CASES[f"db-5x3x{_D}"] = (5, 3, _D, LENS1, False, 1, True)
for _N, _M, _D in ((17, 2, 13), (32, 2, 13), (33, 1, 13), (64, 2, 6)):  # lane classes 32 / 64, second grid row
    CASES[f"lanes-{_N}x{_M}x{_D}"] = (_N, _M, _D, LENS2, False, 1, False)
for _N, _M, _D in ((20, 2, 9), (40, 1, 5)):             # dense A: separate launches, general recursion
    for _delta in (1, 2):
        CASES[f"dense-{_N}x{_M}x{_D}-delta{_delta}"] = (_N, _M, _D, (60, 45, 81), True, _delta, False)
for _delta in (0, 3):                                    # the band of num_a
    CASES[f"band-6x2x7-delta{_delta}"] = (6, 2, 7, (50, 60, 9), True, _delta, False)
CASES["short-12x2x6"] = (12, 2, 6, (40, 5, 1, 0, 30), False, 1, False)   # T < N, T = 1, T = 0
CASES["paths-8x3x16"] = (8, 3, 16, LENS1, False, 1, False)
for _N, _M, _D in ((64, 4, 1), (64, 8, 1), (64, 3, 3)):  # FSn 16 / 8 / 16 in k_fullstats
    CASES[f"fsn-{_N}x{_M}x{_D}"] = (_N, _M, _D, (150, 200, 130), False, 1, False)
CASES["large-64x2x48"] = (64, 2, 48, LONG64, False, 1, False)
CASES["many-8x3x16"] = (8, 3, 16, (337, 120, 400, 256, 199, 311, 288, 143, 390, 222, 175, 264), False, 1, False)
SWEEP = [k for k in CASES if k != "many-8x3x16"]


@functools.lru_cache(maxsize=None)
def build(G, name):
    """(model, frames, lens, delta, the long-double E-step) of a case, computed once"""
    N, M, D, lens, dense, delta, clamp = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    hm = rand_model(G, rng, N, M, D)
    if dense:
        A = rng.random((N, N)) + 0.05
        hm.A[:] = A / A.sum(1, keepdims=True)
    X = walk_any(rng, hm, lens)
    if clamp:
        # test_fulltrain_gpu's non-positive-definite Gaussian: its density overflows to +inf on
        # every frame and is clamped to 1e20
        hm.inv_cov[4, 2] = -np.eye(D)
        hm.mean[4, 2] = hm.mean[4, 0] + 60.0
    ref = R.estep(hm, X, lens, delta, np.longdouble)
    ll = np.asarray(ref["loglik"], dtype=np.float64)
    for u, T in enumerate(lens):
        if T >= N:
            assert np.isfinite(ll[u]), (name, u)    # no case compares NaN with NaN by accident
    if clamp:
        assert np.any(ref["post"][:, 4, 2] > 0)
    return hm, X, np.asarray(lens, dtype=np.int32), delta, ref


def run_device(G, ctx, hm, X, lens, delta=1, options=(), twice=False):
    """estep_full under `options`; everything the tests look at, downloaded"""
    N, M, D = hm.N, hm.M, hm.D
    F, U = len(X), len(lens)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.set_option(G.OPT_DELTA, delta)
        for opt, val in options:
            ctx.set_option(opt, val)
        ctx.estep_full(fm, corpus, st)
        v = st.download()
        out = dict(v=v, stats=G.split_stats_full(v, N, M, D), b=ctx.fetch(G.BUF_B, (F, N)),
                   post=ctx.fetch(G.BUF_POST, (F, N * M)), gamma=ctx.fetch(G.BUF_GAMMA, (F, N)),
                   ll=ctx.fetch(G.BUF_LOGLIK, (U,)))
        if twice:   # repeated calls at one setting stay bitwise equal
            ctx.estep_full(fm, corpus, st)
            assert np.array_equal(v.view(np.uint64), st.download().view(np.uint64))
        return out
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
        for opt, _ in options:
            ctx.set_option(opt, 0)
        st.close(); fm.close(); corpus.close()


def f64(a):
    return np.asarray(a, dtype=np.float64)


def same_kind(got, ref, what):
    """equal NaN pattern and equal infinities; returns the mask of the finite reference entries"""
    got, ref = f64(got), f64(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), f"{what}: infinities differ"
    return np.isfinite(ref)


def check_estep(dev, ref, hm, lens, delta, what):
    """(a)"""
    N, M = hm.N, hm.M
    F = dev["b"].shape[0]
    rb, rpost, rgamma = f64(ref["b"]), f64(ref["post"]).reshape(F, N * M), f64(ref["gamma"])
    if F:
        for i in range(N):
            close(dev["b"][:, i], rb[:, i])
    assert np.array_equal(dev["post"] == 0.0, rpost == 0.0), f"{what}: zeros of post differ"
    for key, got, r in (("post", dev["post"], rpost), ("gamma", dev["gamma"], rgamma)):
        assert np.all(np.isfinite(got)), f"{what}: {key} is not finite"
        worst = (np.abs(got - r) / (1e-11 * np.abs(r) + 1e-11)).max() if F else 0.0
        assert worst <= 1.0, f"{what}: {key} worst error {worst:.3g} x tolerance"
    rst = ref["stats"]
    for key in ("num_a", "den_a", "den_c"):
        close(dev["stats"][key], f64(rst[key]), zeros=False)
    fin = same_kind(dev["ll"], ref["loglik"], f"{what}: loglik")
    rll = f64(ref["loglik"])
    for u in np.nonzero(fin)[0]:
        if lens[u] > 0:
            assert dev["ll"][u] == pytest.approx(rll[u], rel=1e-11), (what, u)
    total = float(dev["stats"]["loglik"])
    if same_kind(total, rst["loglik"], f"{what}: summed loglik"):
        assert total == pytest.approx(float(rst["loglik"]), rel=1e-11), what
    assert float(dev["stats"]["n_utt"]) == float(len(lens))
    i, j = np.indices((N, N))
    assert np.all(dev["stats"]["num_a"][(j < i) | (j > i + delta)] == 0.0), f"{what}: num_a outside the band"


def check_stats_bound(dev, X, hm, what):
    """(b): returns the worst error / bound ratio"""
    F = len(X)
    s, a = R.stats_from(dev["gamma"], dev["post"], X, hm.mean, np.longdouble)
    factor = np.longdouble((2 * F + 8) * U53)
    worst = 0.0
    for key in ("num_c", "num_mu", "num_cov"):
        got = dev["stats"][key].reshape(s[key].shape)
        fin = same_kind(got, s[key], f"{what}: {key}")
        err = np.abs(got[fin].astype(np.longdouble) - s[key][fin])
        tol = factor * a[key][fin]
        assert np.all(got[fin][a[key][fin] == 0] == 0.0), f"{what}: {key} holds a value where every term is 0"
        ratio = float((err / np.where(tol > 0, tol, 1)).max()) if err.size else 0.0
        assert np.all(err <= tol), f"{what}: {key} worst error {ratio:.3g} x bound"
        worst = max(worst, ratio)
    return worst


def fs_geometry(N, M, D):
    """run_fullstats' launch geometry (ghmm_hip.hip): frames staged per pass and the Gaussians
    [g0, g1] of every element batch"""
    G_, E1 = N * M, 1 + D + D * (D + 1) // 2
    batch = 256 * 8                                  # FS_THREADS * FS_EPT
    gwmax = min(batch // E1 + 2, G_)
    fsn = 32                                         # FS_FRAMES
    while fsn > 1 and fsn * (D + 1 + gwmax) * 8 > 48 * 1024:
        fsn //= 2
    E = G_ * E1
    return fsn, [(e0 // E1, (min(e0 + batch, E) - 1) // E1) for e0 in range(0, E, batch)]


def zero_weight_passes(dev, N, M, D):
    """aligned runs of FSn frames whose gamma * post is exactly 0 for every Gaussian of an element
    batch: the passes k_fullstats skips as a whole (frame blocks start at multiples of FSn)"""
    fsn, batches = fs_geometry(N, M, D)
    F = dev["gamma"].shape[0]
    w = np.repeat(dev["gamma"], M, axis=1) * dev["post"]
    n = 0
    for g0, g1 in batches:
        nz = (w[:, g0:g1 + 1] != 0.0).any(1)
        n += sum(1 for f in range(0, F, fsn) if not nz[f:f + fsn].any())
    return fsn, n


# ------------------------------------------------------------- (a) and (b), the sweep

@extended
@pytest.mark.parametrize("name", SWEEP)
def test_estep_arrays_against_the_extended_reference(G, ctx, name):
    hm, X, lens, delta, ref = build(G, name)
    dev = run_device(G, ctx, hm, X, lens, delta)
    check_estep(dev, ref, hm, lens, delta, name)
    if name == "short-12x2x6":
        o = np.concatenate([[0], np.cumsum(lens)])
        for u in (1, 2):    # T = 5 and T = 1 under 12 states
            assert np.all(dev["gamma"][o[u]:o[u + 1]] == 0.0) and dev["ll"][u] == -np.inf


@extended
@pytest.mark.parametrize("name", SWEEP)
def test_statistics_within_the_derived_bound(G, ctx, name):
    hm, X, lens, delta, _ = build(G, name)
    dev = run_device(G, ctx, hm, X, lens, delta)
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
        dev = run_device(G, ctx, hm, X, lens, delta, options=((G.OPT_PARTIALS, partials),), twice=True)
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
        out[tag] = dev = run_device(G, ctx, hm, X, lens, delta, options=options)
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
    hm = rand_model(G, rng, N, M, D)
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
    hm = rand_model(G, rng, N, M, D)
    lens = np.array([5, 1, 11, 3], dtype=np.int32)
    X = walk_any(rng, hm, lens)
    ref = R.estep(hm, X, lens, 1, np.longdouble)
    assert np.all(f64(ref["loglik"]) == -np.inf)
    dev = run_device(G, ctx, hm, X, lens)
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
    hm = rand_model(G, rng, N, M, D)
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
