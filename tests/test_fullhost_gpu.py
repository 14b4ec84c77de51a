"""The host side of the full-covariance entry points (csrc/ghmm_fullhost.hpp) and of ghmm_score_batch —
GPU box only.  Two things their shared prologues must not move:

1. Refusals: the code and the text of every argument check the vocabulary calls share, written out
   here as literals (the entry point's name is part of the text), the refusal of GHMM_OPT_ROBUST by
   every full-covariance call, and ghmm_mstep_full_dev's refusal of a diagonal-layout statistics vector.
2. Call order: every call below gives, after any sequence of the others in the same context, the bits
   it gives as the first call on a new context.

The shapes: three words of N = 3, 5 and 17 states (the largest in the 32-lane class), M = 2, D = 9
(eight-column blocks: 16 columns, seven of them padding), 25 states in the vocabulary (one emission
tile); five utterances of 1, 2, 7, 40 and 70 frames, some shorter than a word.  Both kinds have a
second feature stream of another width (M = 1, D = 5) for the several-stream and vocabulary calls."""
import numpy as np
import pytest

from fullcov_support import frames, rand_fmodel

pytestmark = pytest.mark.gpu

STATES, M, D = (3, 5, 17), 2, 9
M2, D2 = 1, 5  # the second feature stream
LENS = [1, 2, 7, 40, 70]
ROBUST = "GHMM_OPT_ROBUST is not available with full-covariance models"
STATS = "statistics vector is not a full-covariance one of the model's shape (ghmm_stats_create_full)"


def host_words(G):
    """the vocabulary as HostFullModels, and the corpus"""
    rng = np.random.default_rng(61)
    base = rng.normal(0.0, 1.0, (1, 1, D))
    hms = [rand_fmodel(G, rng, n, M, D, spread=0.6, base=base, asym=False) for n in STATES]
    return hms, frames(rng, hms[2], LENS, scale=1.0)


def host_stream2(G):
    """the words' second stream and its corpus (draws of their own: host_words' stay as they are)"""
    rng = np.random.default_rng(63)
    base = rng.normal(0.0, 1.0, (1, 1, D2))
    hms = [rand_fmodel(G, rng, n, M2, D2, spread=0.6, base=base, asym=False) for n in STATES]
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
        self.hms2, self.X2 = host_stream2(G)
        self.fms2 = [self.ctx.full_model(h) for h in self.hms2]
        self.dms2 = [self.ctx.model(diagonal(G, h)) for h in self.hms2]
        self.corpora = [self.corpus, self.ctx.corpus(self.X2, LENS)]
        self.fvocab = [list(w) for w in zip(self.fms, self.fms2)]  # vocab[k][p] = stream p of word k
        self.dvocab = [list(w) for w in zip(self.dms, self.dms2)]

    def close(self):
        self.ctx.close()


def refusal(G, fn):
    with pytest.raises(G.GhmmError) as e:
        fn()
    return e.value.code, str(e.value)


def refused(G, fn, code, text):
    assert refusal(G, fn) == (code, f"ghmm error {code}: {text}")


class Raw:
    """the C entry points called as they are (the wrapper cannot pass a null array, a null destination
    or a stream count of its own): (return code, ghmm_last_error's text)"""

    def __init__(self, G, w):
        self.G, self.lib, self.h = G, w.ctx.lib, w.ctx.h
        self.score = np.zeros(len(STATES) * len(LENS))
        self.path = np.zeros(sum(LENS), dtype=np.int32)
        self.word = np.zeros(len(LENS), dtype=np.int32)

    def handles(self, objs):
        if objs is None:
            return None
        return (self.G.C.c_void_p * len(objs))(*[None if o is None else o.h for o in objs])

    def tail(self, kind, dest, stats):
        """the arguments behind the stream count"""
        C = self.G.C
        dp = self.score.ctypes.data_as(C.POINTER(C.c_double)) if dest else None
        ip = [a.ctypes.data_as(C.POINTER(C.c_int32)) if dest else None for a in (self.word, self.path)]
        return {"score": (dp,), "logscore": (0, dp), "viterbi": (ip[1], dp), "recognise": (ip[0], ip[1], dp),
                "estep": (self.handles(stats if dest else None),),
                "estep_full": (self.handles(stats if dest else None), 0)}[kind]

    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.h, *args)
        return rc, self.lib.ghmm_last_error().decode()

    def vocab(self, name, kind, models, K, corpora, P, dest=True):
        return self.call(name, self.handles(models), K, self.handles(corpora), P, *self.tail(kind, dest, None))

    def vocab1(self, name, models, K, corpus, dest=True):
        """the single-stream vocabulary calls: one corpus, no stream count"""
        return self.call(name, self.handles(models), K, corpus.h if corpus else None, *self.tail("logscore", dest, None))

    def streams(self, name, kind, models, corpora, P, dest=True, stats=None):
        return self.call(name, self.handles(models), self.handles(corpora), P, *self.tail(kind, dest, stats))


class robust:
    def __init__(self, G, ctx):
        self.G, self.ctx = G, ctx

    def __enter__(self):
        self.ctx.set_option(self.G.OPT_ROBUST, 1)

    def __exit__(self, *exc):
        self.ctx.set_option(self.G.OPT_ROBUST, 0)


ROBUST_STREAMS = "GHMM_OPT_ROBUST is not available with several feature streams"
BAD_D = "model has 5 coefficients per frame, corpus has 7"
LENGTHS = "stream 1: utterance count or lengths differ from stream 0"


def vocab_refusals(G, w, full):
    """every check the several-stream vocabulary calls of one kind share, and the order of two of them"""
    ctx, raw, c0 = w.ctx, Raw(G, w), w.corpus
    ARG, UNSUPPORTED = 1, 5
    rng = np.random.default_rng(64)
    make = ctx.full_model if full else (lambda h: ctx.model(diagonal(G, h)))
    other_n = make(rand_fmodel(G, rng, 6, M2, D2, spread=0.6, asym=False))        # word 1, stream 1: another N
    other_m = make(rand_fmodel(G, rng, 5, 2, D2, spread=0.6, asym=False))         # ... another M
    other_m0 = make(rand_fmodel(G, rng, 5, 3, D, spread=0.6, asym=False))         # stream 0: another M
    other_d = ctx.corpus(np.zeros((sum(LENS), 7)), LENS)
    other_len = ctx.corpus(np.zeros((sum(LENS), D2)), [1, 2, 7, 41, 69])
    words = w.fvocab if full else w.dvocab
    flat = [m for word in words for m in word]
    first = [word[0] for word in words]
    corpora, K, P = w.corpora, len(words), 2
    bad_n, bad_m = flat[:3] + [other_n] + flat[4:], flat[:3] + [other_m] + flat[4:]
    if full:
        names = (("ghmm_score_full_streams_batch", "score"), ("ghmm_viterbi_full_streams_batch", "score"),
                 ("ghmm_recognise_full_streams", "recognise"), ("ghmm_logscore_full_streams_batch", "logscore"))
        one = "ghmm_logscore_full_batch"
    else:
        names = (("ghmm_score_streams_batch", "score"), ("ghmm_viterbi_streams_batch", "score"),
                 ("ghmm_recognise_streams", "recognise"), ("ghmm_logscore_streams_batch", "logscore"))
        one = "ghmm_logscore_batch"
    for name, kind in names:
        def call(models, k, cs, p, dest=True):
            return raw.vocab(name, kind, models, k, cs, p, dest)
        assert call(None, K, corpora, P) == (ARG, f"{name}: null argument")
        assert call(flat, 0, corpora, P) == (ARG, f"{name}: null argument")
        assert call(flat, K, None, P) == (ARG, f"{name}: null argument")
        assert call(flat, K, [c0, None], P) == (ARG, f"{name}: null argument")
        assert call(flat, K, corpora, 0) == (ARG, f"{name}: 1 to 8 feature streams (asked: 0)")
        assert call(flat, K, corpora, 9) == (ARG, f"{name}: 1 to 8 feature streams (asked: 9)")
        assert call(flat[:3] + [None] + flat[4:], K, corpora, P) == (ARG, f"{name}: null model")
        assert call(flat, K, corpora, P, dest=False) == (ARG, f"{name}: null destination")
        assert call(bad_n, K, corpora, P) == (ARG, f"{name}: word 1: stream 1 has 6 states, stream 0 has 5")
        assert call(bad_m, K, corpora, P) == (UNSUPPORTED, f"{name}: every model must have the same M and D (stream 1)")
        assert call(flat, K, [c0, other_d], P) == (ARG, BAD_D)
        assert call(flat, K, [c0, other_len], P) == (ARG, f"{name}: {LENGTHS}")
        # two faults in one call: the one reported first
        assert call(bad_m, K, corpora, P, dest=False) == (ARG, f"{name}: null destination")
        assert call(bad_n, K, [c0, other_d], P) == (ARG, f"{name}: word 1: stream 1 has 6 states, stream 0 has 5")
        with robust(G, ctx):
            if full:
                assert call(flat, K, corpora, P) == (UNSUPPORTED, ROBUST)
                assert call(flat, K, [c0, other_len], P) == (UNSUPPORTED, ROBUST)
            else:
                assert call(flat, K, corpora, P) == (UNSUPPORTED, f"{name}: {ROBUST_STREAMS}")
                assert call(flat, K, [c0, other_len], P) == (ARG, f"{name}: {LENGTHS}")
    assert raw.vocab1(one, None, K, c0) == (ARG, f"{one}: null argument")
    assert raw.vocab1(one, first, K, None) == (ARG, f"{one}: null argument")
    assert raw.vocab1(one, [first[0], None, first[2]], K, c0) == (ARG, f"{one}: null model")
    assert raw.vocab1(one, first, K, c0, dest=False) == (ARG, f"{one}: null destination")
    assert raw.vocab1(one, [first[1], other_m0], 2, c0) == (UNSUPPORTED, f"{one}: every model must have the same M and D")
    assert raw.vocab1(one, first, K, other_d) == (ARG, "model has 9 coefficients per frame, corpus has 7")
    assert raw.vocab1(one, [first[1], other_m0], 2, c0, dest=False) == (ARG, f"{one}: null destination")
    if full:
        with robust(G, ctx):
            assert raw.vocab1(one, first, K, c0) == (UNSUPPORTED, ROBUST)
    else:  # the Viterbi lattices of a diagonal vocabulary hold one state per lane
        h65 = [rand_fmodel(G, rng, 65, m, d, spread=0.6, asym=False) for m, d in ((M, D), (M2, D2))]
        wide = flat[:4] + [make(h) for h in h65]
        for name, kind in names[1:3]:
            lanes = f"{name}: a word of 65 states: the vocabulary lattices hold one state per lane (64)"
            assert raw.vocab(name, kind, wide, K, corpora, P) == (UNSUPPORTED, lanes)
            with robust(G, ctx):
                assert raw.vocab(name, kind, wide, K, corpora, P) == (UNSUPPORTED, f"{name}: {ROBUST_STREAMS}")


def stream_refusals(G, w, full):
    """the same for the calls on one word's streams"""
    ctx, raw, c0 = w.ctx, Raw(G, w), w.corpus
    ARG, UNSUPPORTED = 1, 5
    rng = np.random.default_rng(65)
    make = ctx.full_model if full else (lambda h: ctx.model(diagonal(G, h)))
    other_n = make(rand_fmodel(G, rng, 6, M2, D2, spread=0.6, asym=False))
    other_d = ctx.corpus(np.zeros((sum(LENS), 7)), LENS)
    other_len = ctx.corpus(np.zeros((sum(LENS), D2)), [1, 2, 7, 41, 69])
    word = (w.fvocab if full else w.dvocab)[1]
    corpora, P = w.corpora, 2
    new_stats = ctx.stats_full if full else ctx.stats
    stats = [new_stats(STATES[1], M, D), new_stats(STATES[1], M2, D2)]
    if full:
        names = (("ghmm_viterbi_full_streams", "viterbi"), ("ghmm_score_full_streams", "score"),
                 ("ghmm_logscore_full_streams", "logscore"), ("ghmm_estep_full_streams", "estep_full"))
        bad = "bad stream arguments (1 to 8 feature streams, no null array)"
        no_stats, robust_text = bad, ROBUST
    else:
        names = (("ghmm_viterbi_streams", "viterbi"), ("ghmm_score_streams", "score"),
                 ("ghmm_logscore_streams", "logscore"), ("ghmm_estep_streams", "estep"))
        bad = "check_streams: bad stream arguments"
        no_stats, robust_text = "ghmm_estep_streams: null statistics", ROBUST_STREAMS
    states = "stream 1 has 6 states, stream 0 has 5"
    for name, kind in names:
        def call(models, cs, p, dest=True):
            return raw.streams(name, kind, models, cs, p, dest, stats)
        estep = kind.startswith("estep")
        assert call(None, corpora, P) == (ARG, bad)
        assert call(word, None, P) == (ARG, bad)
        assert call(word, corpora, 0) == (ARG, bad)
        assert call(word, corpora, 9) == (ARG, bad)
        assert call([word[0], None], corpora, P) == (ARG, "null model or corpus")
        assert call(word, [c0, None], P) == (ARG, "null model or corpus")
        assert call(word, corpora, P, dest=False) == (ARG, no_stats if estep else f"{name}: null destination")
        assert call([word[0], other_n], corpora, P) == (ARG, states)
        assert call(word, [c0, other_d], P) == (ARG, BAD_D)
        assert call(word, [c0, other_len], P) == (ARG, LENGTHS)
        # two faults in one call: the one reported first
        assert call([word[0], other_n], corpora, P, dest=False) == (ARG, bad if estep and full else states)
        assert call([word[0], other_n], [c0, other_len], P) == (ARG, states)
        with robust(G, ctx):
            assert call(word, corpora, P) == (UNSUPPORTED, robust_text)
            assert call(word, [c0, other_len], P) == ((UNSUPPORTED, ROBUST) if full else (ARG, LENGTHS))


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
        for full in (False, True):
            vocab_refusals(G, w, full)
            stream_refusals(G, w, full)
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


def estep_streams(full):
    def call(G, w, seen):
        new_stats = w.ctx.stats_full if full else w.ctx.stats
        sts = [new_stats(STATES[1], M, D), new_stats(STATES[1], M2, D2)]
        if full:
            w.ctx.estep_full_streams(w.fvocab[1], w.corpora, sts)
        else:
            w.ctx.estep_streams(w.dvocab[1], w.corpora, sts)
        got = [st.download() for st in sts]
        for st in sts:
            st.close()
        return got
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
    # two feature streams, the two kinds in turn
    ("score_streams_batch", lambda G, w, seen: [w.ctx.score_streams_batch(w.dvocab, w.corpora)]),
    ("score_full_streams_batch", lambda G, w, seen: [w.ctx.score_full_streams_batch(w.fvocab, w.corpora)]),
    ("viterbi_streams_batch", lambda G, w, seen: [w.ctx.viterbi_streams_batch(w.dvocab, w.corpora)]),
    ("viterbi_full_streams_batch", lambda G, w, seen: [w.ctx.viterbi_full_streams_batch(w.fvocab, w.corpora)]),
    ("logscore_streams_batch",
     lambda G, w, seen: [w.ctx.logscore_streams_batch(w.dvocab, w.corpora, final_state=True)]),
    ("logscore_full_streams_batch",
     lambda G, w, seen: [w.ctx.logscore_full_streams_batch(w.fvocab, w.corpora, final_state=True)]),
    ("recognise_streams", lambda G, w, seen: list(w.ctx.recognise_streams(w.dvocab, w.corpora))),
    ("recognise_full_streams", lambda G, w, seen: list(w.ctx.recognise_full_streams(w.fvocab, w.corpora))),
    ("score_streams", lambda G, w, seen: [w.ctx.score_streams(word, w.corpora) for word in w.dvocab]),
    ("score_full_streams", lambda G, w, seen: [w.ctx.score_full_streams(word, w.corpora) for word in w.fvocab]),
    ("viterbi_streams", lambda G, w, seen: list(w.ctx.viterbi_streams(w.dvocab[2], w.corpora))),
    ("viterbi_full_streams", lambda G, w, seen: list(w.ctx.viterbi_full_streams(w.fvocab[2], w.corpora))),
    ("logscore_streams", lambda G, w, seen: [w.ctx.logscore_streams(word, w.corpora) for word in w.dvocab]),
    ("logscore_full_streams", lambda G, w, seen: [w.ctx.logscore_full_streams(word, w.corpora) for word in w.fvocab]),
    ("estep_streams", estep_streams(False)),
    ("estep_full_streams", estep_streams(True)),
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
