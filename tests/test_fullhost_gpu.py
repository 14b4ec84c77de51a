"""The host side of the full-covariance entry points (csrc/ghmm_fullhost.hpp) and of ghmm_score_batch —
GPU box only.  Two things their shared prologues must not move:

1. Refusals: the code and the text of every argument check the vocabulary calls share, written out
   here as literals (the entry point's name is part of the text), the refusal of GHMM_OPT_ROBUST by
   every full-covariance call, and ghmm_mstep_full_dev's refusal of a diagonal-layout statistics vector.
2. Call order: every call below gives, after any sequence of the others in the same context, the bits
   it gives as the first call on a new context.

The shapes: three words of N = 3, 5 and 17 states (the largest in the 32-lane class), M = 2, D = 9
(eight-column blocks: 16 columns, seven of them padding), 25 states in the vocabulary (one emission
tile); five utterances of 1, 2, 7, 40 and 70 frames, some shorter than a word."""
import numpy as np
import pytest

from fullcov_support import frames, rand_fmodel

pytestmark = pytest.mark.gpu

STATES, M, D = (3, 5, 17), 2, 9
LENS = [1, 2, 7, 40, 70]
ROBUST = "GHMM_OPT_ROBUST is not available with full-covariance models"
STATS = "statistics vector is not a full-covariance one of the model's shape (ghmm_stats_create_full)"


def host_words(G):
    """the vocabulary as HostFullModels, and the corpus"""
    rng = np.random.default_rng(61)
    base = rng.normal(0.0, 1.0, (1, 1, D))
    hms = [rand_fmodel(G, rng, n, M, D, spread=0.6, base=base, asym=False) for n in STATES]
    return hms, frames(rng, hms[2], LENS, scale=1.0)


def diagonal(G, hm):
    """the same N, M, D, means and weights with unit variances"""
    return G.HostModel(hm.A, hm.c, hm.mean, np.ones((hm.N, hm.M, hm.D)), np.ones((hm.N, hm.M)))


def blank(G, N):
    return G.HostFullModel(np.eye(N), np.full((N, M), 1.0 / M), np.zeros((N, M, D)),
                           np.tile(np.eye(D), (N, M, 1, 1)), np.ones((N, M)))


class World:
    """a context with the vocabulary, its diagonal twin and the corpus on it"""

    def __init__(self, G):
        self.hms, self.X = host_words(G)
        self.ctx = G.Context(0)
        self.fms = [self.ctx.full_model(h) for h in self.hms]
        self.dms = [self.ctx.model(diagonal(G, h)) for h in self.hms]
        self.corpus = self.ctx.corpus(self.X, LENS)

    def close(self):
        self.ctx.close()


def refusal(G, fn):
    with pytest.raises(G.GhmmError) as e:
        fn()
    return e.value.code, str(e.value)


def refused(G, fn, code, text):
    assert refusal(G, fn) == (code, f"ghmm error {code}: {text}")


def test_refusal_texts(G):
    w = World(G)
    ctx, corpus, fms, dms = w.ctx, w.corpus, w.fms, w.dms
    try:
        rng = np.random.default_rng(62)
        f3 = ctx.full_model(rand_fmodel(G, rng, 5, 3, D, spread=0.6, asym=False))      # another M
        d3 = ctx.model(diagonal(G, rand_fmodel(G, rng, 5, 3, D, spread=0.6, asym=False)))
        other = ctx.corpus(np.zeros((sum(LENS), 7)), LENS)                             # another D
        batch = (("ghmm_score_full_batch", ctx.score_full_batch, fms, f3),
                 ("ghmm_viterbi_full_batch", ctx.viterbi_full_batch, fms, f3),
                 ("ghmm_logscore_full_batch", ctx.logscore_full_batch, fms, f3),
                 ("ghmm_score_batch", ctx.score_batch, dms, d3))
        for name, call, models, m3 in batch:
            refused(G, lambda: call([], corpus), G.ERR_ARG, f"{name}: null argument")
            refused(G, lambda: call([models[0], m3], corpus), G.ERR_UNSUPPORTED,
                    f"{name}: every model must have the same M and D")
        for name, call, models, _ in batch[:3]:
            refused(G, lambda: call(models, other), G.ERR_ARG, "model has 9 coefficients per frame, corpus has 7")
        refused(G, lambda: ctx.score_batch(dms, other), G.ERR_ARG, "models have 9 coefficients per frame, corpus has 7")
        st = ctx.stats_full(5, M, D)
        target = ctx.full_model(blank(G, 5))
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            for call in (lambda: ctx.score_full_batch(fms, corpus), lambda: ctx.viterbi_full_batch(fms, corpus),
                         lambda: ctx.logscore_full_batch(fms, corpus), lambda: ctx.score_full(fms[1], corpus),
                         lambda: ctx.emission_full(fms[1], corpus), lambda: ctx.viterbi_full(fms[1], corpus),
                         lambda: ctx.logscore_full(fms[1], corpus), lambda: ctx.estep_full(fms[1], corpus, st),
                         lambda: ctx.estep_full_log(fms[1], corpus, st), lambda: target.init_from(corpus)):
                refused(G, call, G.ERR_UNSUPPORTED, ROBUST)
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        refused(G, lambda: ctx.mstep_full_dev(fms[1], ctx.stats(5, M, D)), G.ERR_ARG, STATS)
    finally:
        w.close()


# ------------------------------------------------------------- call order

def estep(log):
    def call(G, w, seen):
        st = w.ctx.stats_full(STATES[1], M, D)
        (w.ctx.estep_full_log if log else w.ctx.estep_full)(w.fms[1], w.corpus, st)
        v = st.download()
        st.close()
        return [v]
    return call


def mstep_dev(G, w, seen):
    """on a fresh copy of the word, from the statistics estep_full gave as a context's first call"""
    fm, st = w.ctx.full_model(w.hms[1]), w.ctx.stats_full(STATES[1], M, D)
    st.upload(seen["estep_full"][0])
    w.ctx.mstep_full_dev(fm, st)
    got = fm.get().arrays()
    fm.close(); st.close()
    return got


def init_dev(G, w, seen):
    fm = w.ctx.full_model(blank(G, STATES[1]))
    got = fm.init_from(w.corpus).arrays()
    fm.close()
    return got


CALLS = (
    ("score_full", lambda G, w, seen: [w.ctx.score_full(fm, w.corpus) for fm in w.fms]),
    ("score_full_batch", lambda G, w, seen: [w.ctx.score_full_batch(w.fms, w.corpus)]),
    ("viterbi_full", lambda G, w, seen: list(w.ctx.viterbi_full(w.fms[2], w.corpus))),
    ("viterbi_full_batch", lambda G, w, seen: [w.ctx.viterbi_full_batch(w.fms, w.corpus)]),
    ("logscore_full", lambda G, w, seen: [w.ctx.logscore_full(fm, w.corpus) for fm in w.fms]),
    ("logscore_full_batch", lambda G, w, seen: [w.ctx.logscore_full_batch(w.fms, w.corpus, final_state=True)]),
    ("score_batch", lambda G, w, seen: [w.ctx.score_batch(w.dms, w.corpus)]),
    ("estep_full", estep(False)),
    ("estep_full_log", estep(True)),
    ("mstep_full_dev", mstep_dev),
    ("init_from", init_dev),
)


def same_bits(a, b):
    """equal shapes and types; floating point: NaNs at the same places, every other entry bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def test_call_order_leaves_results_alone(G):
    first = {}
    for name, call in CALLS:
        w = World(G)
        try:
            first[name] = call(G, w, first)
        finally:
            w.close()
    w = World(G)
    try:
        for order in (CALLS, CALLS[::-1]):
            for name, call in order:
                got = call(G, w, first)
                assert len(got) == len(first[name]), name
                for k, (a, b) in enumerate(zip(got, first[name])):
                    assert same_bits(a, b), f"{name}, result {k}: differs from a new context's first call"
    finally:
        w.close()
