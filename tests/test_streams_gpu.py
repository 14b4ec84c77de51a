"""The diagonal calls on several feature streams (ghmm_estep_streams, ghmm_score_streams: run_emission
per stream into ctx->b / post_s[p], k_mul_streams, the recursions of the single-stream call on the
product, run_accumulate and k_reduce_all once per stream) at the shapes, options and inputs at which
the single-stream suite pins the kernels under them — GPU box only.

Unless a test says otherwise stream p is synth_case(G, N, M_p, D_p, lens, first=17 * p) with stream
0's A in every stream (streams_util.stream_case), and the reference is oracle_lib.estep_streams /
score_streams: the CPU restatement of the reference's own order of operations, pinned bit for bit to
the real two-stream trainer by tests/test_oracle.py.  Tolerances are _estep_streams_vs_oracle's: RTOL
= 1e-8 on b, log P and every stream's statistics, 1e-7 on the M-step's arrays, 1e-9 on scores.  Every
test first asserts, on the oracle's output alone, the condition that makes its comparison a real one."""
import numpy as np
import pytest

import oracle_lib as O
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import assert_close, code
from streams_util import (_estep_streams_vs_oracle, bits_equal, product_of_single_emissions, stream_case,
                          synth_case, utterances)

pytestmark = pytest.mark.gpu

# name: (N, [(M_p, D_p)], lens, dense A) -- the smallest shapes that reach each code path
SWEEP = {
    # a later stream larger in M and D: every per-stream buffer grows mid-call; vector-ALU statistics
    # then the scheduled matrix-core emission; tile edges 63 / 64 / 65; T = N
    "n6": (6, [(2, 5), (8, 39)], [40, 17, 64, 65, 63, 6], False),
    "n10-p3": (10, [(1, 1), (8, 39), (3, 13)], [120, 77, 64, 10, 33], False),   # P = 3, smallest stream first
    "n16-dense": (16, [(4, 13), (2, 9)], [70, 80], True),                       # N = group width, general recursion
    "n20-dense": (20, [(2, 9), (4, 13)], [60, 45, 81], True),                   # 32-lane groups
    "n32-dense": (32, [(1, 3), (2, 4)], [70, 33], True),                        # last 32-lane size
    "n40": (40, [(1, 5), (2, 6)], [120, 40, 200], False),                       # 64-lane groups
    "n64": (64, [(1, 3), (2, 4)], [70, 64, 100], False),                        # last model of the lane kernels
    "n65": (65, [(1, 4), (2, 3)], [70, 66, 130], False),                        # first model of ghmm_wide.hpp,
    "n65-dense": (65, [(1, 4), (2, 3)], [70, 66, 130], True),                   # both values of its band flag
    "n130": (130, [(2, 3), (1, 4)], [140, 200], False),                         # wide, > 2 states per lane
    "p8": (5, [(2, 6)] * 8, [40, 25, 9], False),                                # P = GHMM_MAX_STREAMS
    # one stream per emission kernel of run_emission, see test_shape_sweep
    "three-kernels": (6, [(2, 5), (2, 3), (100, 2)], [40, 17, 64, 33], False),
    # the transition-band case
    "band": (6, [(2, 5), (3, 9)], [40, 17, 64], False),
}
BITS = ("n6", "n10-p3", "n65", "n65-dense")          # rows that take the bit-level checks as well
TIERS = ("n6", "n20-dense", "n65", "n65-dense")      # rows run under GHMM_OPT_KERNELS 1 and 2 too

_cases = {}


def case(G, name, delta=1):
    """(hms, Xs, lens, O.estep_streams' result): built once, shared, never written to"""
    key = (name, delta)
    if key not in _cases:
        N, shapes, lens, dense = SWEEP[name]
        hms, Xs, lens = stream_case(G, N, shapes, lens, dense=dense)
        _cases[key] = (hms, Xs, lens, O.estep_streams(hms, Xs, lens, delta=delta))
    return _cases[key]


def fits(ref):
    """the sweep's condition: every oracle statistic finite, no entry of the product near the underflow"""
    ref_stats, ref_b, _ = ref
    return all(np.all(np.isfinite(s)) for s in ref_stats) and not np.any((ref_b > 0) & (ref_b < 1e-290))


class Open:
    """device models, corpora and statistics vectors of a several-stream case"""

    def __init__(self, ctx, hms, Xs, lens):
        self.models = [ctx.model(h) for h in hms]
        self.corpora = [ctx.corpus(x, lens) for x in Xs]
        self.stats = [ctx.stats(h.N, h.M, h.D) for h in hms]
        self.all = (self.models, self.corpora, self.stats)

    def vectors(self):
        return [s.download() for s in self.stats]

    def close(self):
        for o in self.models + self.corpora + self.stats:
            o.close()


# ------------------------------------------------------------- shapes, tiers, options

@pytest.mark.parametrize("name,kernels", [(n, 0) for n in SWEEP if n != "band"] +
                         [(n, k) for n in TIERS for k in (1, 2)])
def test_shape_sweep(G, ctx, name, kernels):
    """Product b, log P, every stream's statistics, the M-step and the scores against the oracle, row by
    row of SWEEP; BITS rows with the bit-level properties, TIERS rows under both kernel tiers as well.
    three-kernels (default tier): stream 0 (2 x 5, DP = 8) takes k_emission_sched, stream 1 (2 x 3, DP =
    4, below the scheduled kernel's range) k_emission_mfma, stream 2 (100 x 2: Mp = 112 is seven tiles
    per state, more than a chunk holds, so mfma_ok is false) the vector-ALU k_emission."""
    hms, Xs, lens, ref = case(G, name)
    assert fits(ref)
    ctx.set_option(G.OPT_KERNELS, kernels)
    try:
        _estep_streams_vs_oracle(G, ctx, hms, Xs, lens, f"{name} kernels={kernels}", bits=name in BITS, ref=ref)
    finally:
        ctx.set_option(G.OPT_KERNELS, 0)


@pytest.mark.parametrize("partials", [1, 3])
def test_partials_option(G, ctx, partials):
    """GHMM_OPT_PARTIALS: one frame-block partial sum, and three, under P launches of run_accumulate"""
    hms, Xs, lens, ref = case(G, "n6")
    assert fits(ref)
    ctx.set_option(G.OPT_PARTIALS, partials)
    try:
        _estep_streams_vs_oracle(G, ctx, hms, Xs, lens, f"partials={partials}", ref=ref)
    finally:
        ctx.set_option(G.OPT_PARTIALS, 0)


@pytest.mark.parametrize("delta", [0, 2, 3])
def test_transition_band(G, ctx, delta):
    """GHMM_OPT_DELTA against the oracle's delta"""
    hms, Xs, lens, ref = case(G, "band", delta)
    assert fits(ref)
    _estep_streams_vs_oracle(G, ctx, hms, Xs, lens, f"delta={delta}", delta=delta, ref=ref)


def test_one_stream_is_the_single_stream_call(G, ctx):
    """n_streams = 1 gives the bits of ghmm_estep / ghmm_score"""
    hms, Xs, lens, _ = case(G, "n6")
    hm, X = hms[1], Xs[1]
    F, U = len(X), len(lens)
    d = Open(ctx, [hm], [X], lens)
    model, corpus, st = d.models[0], d.corpora[0], d.stats[0]
    try:
        def arrays():
            return [st.download(), ctx.fetch(G.BUF_B, (F, hm.N)), ctx.fetch(G.BUF_GAMMA, (F, hm.N)),
                    ctx.fetch(G.BUF_POST, (F, hm.N * hm.M)), ctx.fetch(G.BUF_LOGLIK, (U,))]
        ctx.estep(model, corpus, st)
        want = arrays()
        st.upload(np.zeros_like(want[0]))
        ctx.estep_streams([model], [corpus], [st])
        for a, b in zip(arrays(), want):
            assert bits_equal(a, b)
        assert bits_equal(ctx.score_streams([model], [corpus]), ctx.score(model, corpus))
    finally:
        d.close()


# ------------------------------------------------------------- call order

def test_call_order(G, ctx):
    """The workspace is rebuilt by every call.  A single-stream E-step of a larger pair between two
    stream calls leaves their statistics bit-equal; ghmm_estep on stream 0's pair right after a stream
    call is the same call in a fresh context, bit for bit (it does not see the product); and a stream
    call that follows a single-stream call in a fresh context, where post_s is still empty and
    ctx->post is not, gives the same vectors again."""
    hms, Xs, lens, ref = case(G, "n6")
    assert fits(ref)
    big, Xb, lb = synth_case(G, 7, 3, 39, [100, 61, 16])
    F, N, U = len(Xs[0]), hms[0].N, len(lens)

    def single(c, model, corpus, st):
        c.estep(model, corpus, st)
        return [st.download(), c.fetch(G.BUF_B, (F, N)), c.fetch(G.BUF_POST, (F, N * hms[0].M)),
                c.fetch(G.BUF_GAMMA, (F, N)), c.fetch(G.BUF_LOGLIK, (U,))]

    d = Open(ctx, hms, Xs, lens)
    o = Open(ctx, [big], [Xb], lb)
    st0 = ctx.stats(N, hms[0].M, hms[0].D)
    try:
        ctx.estep_streams(*d.all)
        first = d.vectors()
        for v, r in zip(first, ref[0]):
            assert_close(v, r, what="the first stream call")
        ctx.estep(o.models[0], o.corpora[0], o.stats[0])
        ctx.estep_streams(*d.all)
        for a, b in zip(d.vectors(), first):
            assert bits_equal(a, b), "a single-stream call in between changed the stream call's statistics"
        after = single(ctx, d.models[0], d.corpora[0], st0)
    finally:
        st0.close(); o.close(); d.close()
    fresh = G.Context(0)
    try:
        d = Open(fresh, hms, Xs, lens)
        alone = single(fresh, d.models[0], d.corpora[0], d.stats[0])
        for a, b, nm in zip(after, alone, ("statistics", "b", "post", "gamma", "loglik")):
            assert bits_equal(a, b), f"ghmm_estep after a stream call: {nm} differs from a fresh context's"
    finally:
        fresh.close()
    fresh = G.Context(0)
    try:
        o = Open(fresh, [big], [Xb], lb)
        fresh.estep(o.models[0], o.corpora[0], o.stats[0])
        d = Open(fresh, hms, Xs, lens)
        fresh.estep_streams(*d.all)
        for a, b in zip(d.vectors(), first):
            assert bits_equal(a, b), "a stream call after a single-stream call in a fresh context differs"
    finally:
        fresh.close()


# ------------------------------------------------------------- short utterances

@pytest.mark.parametrize("N,shapes,lens,finite", [
    (6, [(2, 5), (3, 9)], [40, 1, 3, 6, 5, 17], [True, False, False, True, False, True]),
    (65, [(1, 4), (2, 3)], [70, 64, 1, 130], [True, False, False, True]),
])
def test_short_utterances(G, ctx, N, shapes, lens, finite):
    """Utterances shorter than the model (T = 1 included) beside ones that fit, on the lane kernels and
    the wide ones: the oracle's log P is -inf for the short ones and every statistic except the summed
    loglik is finite, so log P utterance by utterance and the statistics are compared as numbers.  The
    M-step is left out: its quotients are covered by the sweep."""
    hms, Xs, lens = stream_case(G, N, shapes, lens)
    ref = O.estep_streams(hms, Xs, lens)
    assert np.array_equal(np.isfinite(ref[2]), finite) and np.all(ref[2][~np.array(finite)] == -np.inf)
    for p, r in enumerate(ref[0]):
        s = G.split_stats(r, N, hms[p].M, hms[p].D)
        assert all(np.all(np.isfinite(s[k])) for k in s if k != "loglik") and s["loglik"] == -np.inf
    _estep_streams_vs_oracle(G, ctx, hms, Xs, lens, f"short N={N}", mstep=False, ref=ref)


# ------------------------------------------------------------- the product underflows

UNDER = (5, [(4, 40)], [40, 25, 9])


def alone_is_finite(hms, Xs, lens):
    return all(np.isfinite(O.score(h, xs[p])) for xs in utterances(Xs, lens) for p, h in enumerate(hms))


def test_product_underflow_four_streams(G, ctx):
    """Four 40-coefficient streams of a model far from its data (perturb 0.3): every stream alone scores
    finite, and so is every oracle statistic, but most entries of the product are 0 and a few are
    subnormal numbers (a handful of bits: compared to 1e-300 absolutely, as
    test_fuzz_harsh_models_against_oracle does); no frame is all zero."""
    N, shape, lens = UNDER
    hms, Xs, lens = stream_case(G, N, shape * 4, lens, perturb=0.3)
    ref = O.estep_streams(hms, Xs, lens)
    ref_stats, ref_b, ref_ll = ref
    assert alone_is_finite(hms, Xs, lens)
    assert all(np.all(np.isfinite(s)) for s in ref_stats) and np.all(np.isfinite(ref_ll))
    assert ref_b.size == 370 and np.sum(ref_b == 0) == 272 and np.any((ref_b > 0) & (ref_b < 2.3e-308))
    assert not np.any(np.all(ref_b == 0, axis=1))
    again = _estep_streams_vs_oracle(G, ctx, hms, Xs, lens, "four streams", ref=ref, b_floor=1e-300)
    assert again >= 0      # GHMM_OPT_REFORDER_COUNT can be read after a stream call
    print(f"four-stream underflow: {again} utterances taken again in the reference's order")


def test_product_underflow_eight_streams(G, ctx):
    """Eight such streams of a model that fits (perturb 0.05): every stream alone scores finite, the
    product is 0 on 16 whole frames, and the oracle's log P is NaN, finite, NaN.  log P of both calls must
    be NaN exactly there and within RTOL where it is finite, and the product must be the IEEE product of
    the streams' own densities.  The statistics are compared in their NaN pattern only: almost all of the
    oracle's are NaN (one utterance's c_t = 1/0 reaches every sum).  The 25-frame utterance, whose
    statistics are finite, is then compared in full as a corpus of its own."""
    N, shape, lens = UNDER
    hms, Xs, lens = stream_case(G, N, shape * 8, lens)
    ref_stats, ref_b, ref_ll = O.estep_streams(hms, Xs, lens)
    assert alone_is_finite(hms, Xs, lens)
    assert np.array_equal(np.isnan(ref_ll), [True, False, True]) and abs(ref_ll[1] + 11324.68) < 0.01
    assert np.sum(np.all(ref_b == 0, axis=1)) == 16
    assert all(np.isnan(s).mean() > 0.9 for s in ref_stats)
    F = len(Xs[0])
    d = Open(ctx, hms, Xs, lens)
    try:
        singles = product_of_single_emissions(G, ctx, d.models, d.corpora)
        ctx.estep_streams(*d.all)
        assert bits_equal(ctx.fetch(G.BUF_B, (F, N)), singles)
        assert_close(ctx.fetch(G.BUF_LOGLIK, (3,)), ref_ll, what="eight streams: loglik")
        for p, (v, r) in enumerate(zip(d.vectors(), ref_stats)):
            assert np.array_equal(np.isnan(v), np.isnan(r)), f"eight streams: stream {p} NaN pattern"
        assert_close(ctx.score_streams(d.models, d.corpora), ref_ll, what="eight streams: score")
        assert bits_equal(ctx.fetch(G.BUF_B, (F, N)), singles)
    finally:
        d.close()
    one = [x[40:65] for x in Xs]
    ref = O.estep_streams(hms, one, [25])
    assert all(np.all(np.isfinite(s)) for s in ref[0]) and not np.any((ref[1] > 0) & (ref[1] < 1e-290))
    _estep_streams_vs_oracle(G, ctx, hms, one, np.array([25], dtype=np.int32), "eight streams, T=25", ref=ref)


# ------------------------------------------------------------- class-2 Gaussians in a later stream

def test_class2_gaussians_in_a_later_stream(G, ctx):
    """test_class2_gaussians_both_exact_paths' recipe (one coefficient with variance 1e-4 sitting on a
    frame its state occupies) applied to stream 1, 10 x 8 x 39, behind a small stream 0: the gamma that
    weighs its statistics comes from the product.  GHMM_OPT_VEC_STATS 1, 2 and 0 against the oracle,
    then three EM iterations in auto mode against the oracle's."""
    lens = [300, 211, 128, 77]
    hms, Xs, lens = stream_case(G, 10, [(2, 5), (8, 39)], lens)
    hm, X = hms[1], Xs[1]
    _, d0 = O.estep(hm, X, lens)
    occ = d0["alpha"] * d0["beta"] / d0["scale"][:, None]
    for (i, j, k) in ((4, 3, 7), (0, 0, 38), (9, 7, 0)):
        f = int(np.argmax(occ[:, i] * d0["post"].reshape(-1, 10, 8)[:, i, j]))
        old_var = 1.0 / hm.inv_var[i, j, k]
        hm.mean[i, j, k] = X[f, k]
        hm.inv_var[i, j, k] = 1.0 / 1e-4
        hm.det[i, j] *= 1e-4 / old_var
    ref = O.estep_streams(hms, Xs, lens)
    assert fits(ref)
    corpora = [ctx.corpus(x, lens) for x in Xs]
    stats = [ctx.stats(h.N, h.M, h.D) for h in hms]
    try:
        for mode in (1, 2, 0):
            ctx.set_option(G.OPT_VEC_STATS, mode)
            models = [ctx.model(h) for h in hms]
            ctx.estep_streams(models, corpora, stats)
            for p, (s, r) in enumerate(zip(stats, ref[0])):
                assert_close(s.download(), r, what=f"class-2 in stream 1, GHMM_OPT_VEC_STATS {mode}, stream {p}")
            if mode == 0:
                cur = hms
                for it in range(3):
                    ctx.estep_streams(models, corpora, stats)
                    rs, _, _ = O.estep_streams(cur, Xs, lens)
                    assert all(np.all(np.isfinite(r)) for r in rs)
                    for p, (s, r) in enumerate(zip(stats, rs)):
                        assert_close(s.download(), r, what=f"iteration {it} stream {p}")
                    for m, s in zip(models, stats):
                        ctx.mstep(m, s)
                    cur = [O.mstep(h, r) for h, r in zip(cur, rs)]
            for m in models:
                m.close()
    finally:
        ctx.set_option(G.OPT_VEC_STATS, 0)
        for o in corpora + stats:
            o.close()


# ------------------------------------------------------------- degenerate inputs and refusals

def test_empty_and_zero_length_corpora(G, ctx):
    """No utterance at all, and a corpus holding only a zero-length utterance, on two streams: the call
    succeeds, the statistics are the oracle's (zeros; n_utt counts the empty utterance), the scores have
    the corpus' shape, and the models are untouched."""
    hms, Xs, _ = stream_case(G, 4, [(2, 6), (3, 4)], [30])
    models = [ctx.model(h) for h in hms]
    stats = [ctx.stats(h.N, h.M, h.D) for h in hms]
    before = [a.copy() for m in models for a in m.get().arrays()]
    opened = []
    try:
        for lens in (np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int32)):
            corpora = [ctx.corpus(np.zeros((0, h.D)), lens) for h in hms]
            opened += corpora
            for s in stats:
                s.upload(np.full(s.n, 7.0))
            ctx.estep_streams(models, corpora, stats)
            ref_stats, _, ref_ll = O.estep_streams(hms, [np.zeros((0, h.D)) for h in hms], lens)
            for p, (s, r) in enumerate(zip(stats, ref_stats)):
                assert np.all(np.isfinite(r))
                assert_close(s.download(), r, what=f"U={len(lens)} stream {p}")
            got = ctx.score_streams(models, corpora)
            assert got.shape == (len(lens),)
            if len(lens):     # (with no utterance at all there is no such buffer to ask for)
                assert_close(ctx.fetch(G.BUF_LOGLIK, (len(lens),)), ref_ll, what=f"U={len(lens)} loglik")
        for a, b in zip([a for m in models for a in m.get().arrays()], before):
            assert bits_equal(a, b)
    finally:
        for o in models + stats + opened:
            o.close()


def test_refusals(G, ctx):
    """Every refusal ghmm.h lists, before anything is launched: the statistics vectors keep their bytes."""
    hms, Xs, lens, _ = case(G, "band")
    N = hms[0].N
    d = Open(ctx, hms, Xs, lens)
    models, corpora, stats = d.all
    other_n = ctx.model(synth_case(G, 5, 3, 9, [10])[0])
    fewer = ctx.corpus(Xs[1][:57], lens[:2])
    other_len = ctx.corpus(Xs[1], [lens[0] + 1, lens[1] - 1, lens[2]])
    other_d = ctx.corpus(np.zeros((int(lens.sum()), 4)), lens)
    shape = ctx.stats(N, hms[1].M + 1, hms[1].D)
    full = ctx.stats_full(N, hms[1].M, hms[1].D)
    try:
        ctx.estep_streams(models, corpora, stats)
        before = d.vectors()

        def estep(m=models, c=corpora, s=stats):
            return lambda: ctx.estep_streams(m, c, s)
        assert code(G, estep(m=[models[0], other_n])) == G.ERR_ARG
        assert code(G, estep(c=[corpora[0], fewer])) == G.ERR_ARG
        assert code(G, estep(c=[corpora[0], other_len])) == G.ERR_ARG
        assert code(G, estep(c=[corpora[0], other_d])) == G.ERR_ARG
        assert code(G, estep(s=[stats[0], shape])) == G.ERR_ARG
        assert code(G, estep(s=[stats[0], full])) == G.ERR_ARG
        assert code(G, lambda: ctx.score_streams([models[0], other_n], corpora)) == G.ERR_ARG
        assert code(G, lambda: ctx.score_streams(models, [corpora[0], fewer])) == G.ERR_ARG
        assert code(G, lambda: ctx.score_streams(models, [corpora[0], other_len])) == G.ERR_ARG
        assert code(G, lambda: ctx.score_streams(models, [corpora[0], other_d])) == G.ERR_ARG
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert code(G, estep()) == G.ERR_UNSUPPORTED
            assert code(G, lambda: ctx.score_streams(models, corpora)) == G.ERR_UNSUPPORTED
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        # a stream count outside 1 .. GHMM_MAX_STREAMS and null arrays or entries, through the C ABI itself
        lib, vp = ctx.lib, G.C.c_void_p
        nine = lambda objs: (vp * 9)(*[objs[p % 2].h for p in range(9)])  # noqa: E731
        pm, pc, ps = nine(models), nine(corpora), nine(stats)
        out = np.zeros(len(lens))
        dp = out.ctypes.data_as(G.C.POINTER(G.C.c_double))
        for P in (0, 9, -1):
            assert lib.ghmm_estep_streams(ctx.h, pm, pc, P, ps) == G.ERR_ARG
            assert lib.ghmm_score_streams(ctx.h, pm, pc, P, dp) == G.ERR_ARG
        assert lib.ghmm_estep_streams(ctx.h, None, pc, 2, ps) == G.ERR_ARG
        assert lib.ghmm_estep_streams(ctx.h, pm, None, 2, ps) == G.ERR_ARG
        assert lib.ghmm_estep_streams(ctx.h, pm, pc, 2, None) == G.ERR_ARG
        assert lib.ghmm_score_streams(ctx.h, None, pc, 2, dp) == G.ERR_ARG
        assert lib.ghmm_score_streams(ctx.h, pm, None, 2, dp) == G.ERR_ARG
        assert lib.ghmm_score_streams(ctx.h, pm, pc, 2, None) == G.ERR_ARG
        hole = lambda objs: (vp * 2)(objs[0].h, None)  # noqa: E731
        assert lib.ghmm_estep_streams(ctx.h, hole(models), pc, 2, ps) == G.ERR_ARG
        assert lib.ghmm_estep_streams(ctx.h, pm, hole(corpora), 2, ps) == G.ERR_ARG
        assert lib.ghmm_estep_streams(ctx.h, pm, pc, 2, hole(stats)) == G.ERR_ARG
        assert lib.ghmm_score_streams(ctx.h, hole(models), pc, 2, dp) == G.ERR_ARG
        assert lib.ghmm_score_streams(ctx.h, pm, hole(corpora), 2, dp) == G.ERR_ARG
        for a, b in zip(d.vectors(), before):
            assert bits_equal(a, b), "a refused call changed a statistics vector"
    finally:
        for o in (other_n, fewer, other_len, other_d, shape, full):
            o.close()
        d.close()


def test_posteriors_of_another_emission_are_refused(G, ctx):
    """ctx->post is only ever grown, so it can hold the posteriors of an earlier call of another shape.
    After a stream call (whose posteriors are in one buffer per stream) and after an emission that
    writes none (want_post = 0, ghmm_score), ghmm_accumulate and ghmm_fetch / ghmm_fetch_range of
    GHMM_BUF_POST return GHMM_ERR_ARG before anything is launched or copied; ghmm_forward and
    ghmm_backward on stream 0's pair after a stream call keep working, and a ghmm_emission with
    want_post = 1 makes the row calls valid again."""
    hms, Xs, lens, ref = case(G, "band")
    F, N, M0, U = len(Xs[0]), hms[0].N, hms[0].M, len(lens)
    d = Open(ctx, hms, Xs, lens)
    models, corpora, stats = d.all
    big, Xb, lb = synth_case(G, 7, 3, 39, [100, 61, 16])
    o = Open(ctx, [big], [Xb], lb)
    try:
        ctx.estep(o.models[0], o.corpora[0], o.stats[0])      # ctx->post holds another pair's posteriors
        ctx.fetch(G.BUF_POST, (len(Xb), 7 * 3))

        def refused():
            before = d.vectors()
            assert code(G, lambda: ctx.accumulate(models[0], corpora[0], stats[0])) == G.ERR_ARG
            assert code(G, lambda: ctx.fetch(G.BUF_POST, (F, N * M0))) == G.ERR_ARG
            assert code(G, lambda: ctx.fetch_range(G.BUF_POST, 0, (N * M0,))) == G.ERR_ARG
            for a, b in zip(d.vectors(), before):
                assert bits_equal(a, b), "a refused call changed a statistics vector"
        ctx.estep_streams(models, corpora, stats)
        refused()
        ctx.forward(models[0], corpora[0])                    # the product belongs to stream 0's pair
        assert_close(ctx.fetch(G.BUF_LOGLIK, (U,)), ref[2], what="ghmm_forward on the product")
        ctx.backward(models[0], corpora[0])
        assert ctx.fetch(G.BUF_GAMMA, (F, N)).shape == (F, N)
        refused()
        ctx.score_streams(models, corpora)
        refused()
        ctx.estep(o.models[0], o.corpora[0], o.stats[0])
        ctx.emission(models[0], corpora[0], False)
        ctx.forward(models[0], corpora[0])
        ctx.backward(models[0], corpora[0])
        refused()
        ctx.estep(o.models[0], o.corpora[0], o.stats[0])
        ctx.score(models[0], corpora[0])
        assert code(G, lambda: ctx.fetch(G.BUF_POST, (F, N * M0))) == G.ERR_ARG
        # and the row calls with their own posteriors still give the single-stream E-step
        ctx.emission(models[0], corpora[0], True)
        ctx.forward(models[0], corpora[0])
        ctx.backward(models[0], corpora[0])
        ctx.accumulate(models[0], corpora[0], stats[0])
        want, _ = O.estep(hms[0], Xs[0], lens, dumps=False)
        assert_close(stats[0].download(), want, what="the row calls after a refusal")
        assert ctx.fetch(G.BUF_POST, (F, N * M0)).shape == (F, N * M0)
    finally:
        o.close(); d.close()
