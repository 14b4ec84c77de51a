"""Word posteriors under a word-pair grammar on the GPU: ghmm_grammar_post_streams and
ghmm_grammar_post_full_streams (k_gpost_fwd / k_gpost_bwd) through the C ABI by ghmm.py — GPU box only.  The
cases and grammars are grammar_cases', the restatement of the definition is gpost_cases'; test_gpost_host.py
shows on the CPU that the restatement is the definition.

The long-double restatement runs on the log b fetched from the device (GHMM_BUF_B), so the emission's
rounding is not in the comparison.  gamma, occ and ent are held to fullcov_support.assert_close at RTOL with
every frame its own scale, log P to assert_close at RTOL; non-finite values agree in kind.  Against the live
neighbouring calls (consequences (a) to (c): "to rounding") the bar is 1e-10 relative, test_grammar_gpu's
bound for the same lattice arithmetic."""
import numpy as np
import pytest

import gpost_cases as PC
import grammar_cases as GC
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import assert_close, offsets

pytestmark = pytest.mark.gpu

INF = np.inf
REL = 1e-10


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


class Device:
    """a case's device models (dms[k][p]) and corpora, and the calls of its model kind"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        self.full = case.name in GC.FULLCOV
        mk = ctx.full_model if self.full else ctx.model
        self.dms = [[mk(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self.extra = []

    def post(self, start, pair, fin, dms=None, corpora=None, entries=True):
        fn = self.ctx.grammar_post_full_streams if self.full else self.ctx.grammar_post_streams
        return fn(dms or self.dms, corpora or self.corpora, pair, start, fin, entries=entries)

    def everything(self, start, pair, fin):
        """(occ, ent, loglik, gamma, log b, GHMM_BUF_LOGLIK) of one call"""
        case = self.case
        occ, ent, ll = self.post(start, pair, fin)
        return (occ, ent, ll, self.ctx.fetch(self.G.BUF_GAMMA, (case.F, case.NS)), self.log_b(),
                self.ctx.fetch(self.G.BUF_LOGLIK, (case.U,)))

    def decode(self, start, pair, fin):
        fn = self.ctx.connect_grammar_full_streams if self.full else self.ctx.connect_grammar_streams
        return fn(self.dms, self.corpora, pair, start, fin)

    def logscore(self, k):
        fn = self.ctx.logscore_full_streams if self.full else self.ctx.logscore_streams
        return fn(self.dms[k], self.corpora, True)

    def embed(self, transcripts):
        """estep_embed on the transcripts: (GHMM_BUF_LOGLIK, the tied gamma)"""
        case = self.case
        mk = self.ctx.stats_full if self.full else self.ctx.stats
        stats = [[mk(h.N, h.M, h.D) for h in w] for w in case.words]
        self.extra += [s for row in stats for s in row]
        fn = self.ctx.estep_embed_full_streams if self.full else self.ctx.estep_embed_streams
        fn(self.dms, self.corpora, transcripts, stats)
        self.ctx.sync()
        return self.ctx.fetch(self.G.BUF_LOGLIK, (case.U,)), self.ctx.fetch(self.G.BUF_GAMMA, (case.F, case.NS))

    def log_b(self):
        return self.ctx.fetch(self.G.BUF_B, (self.case.F, self.case.NS))

    def close(self):
        for o in [m for w in self.dms for m in w] + self.corpora + self.extra:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(G, ctx, GC.make(G, name))
        return made[name]
    yield get
    for d in made.values():
        d.close()


def check_rows(case, occ, ent, ll, gamma):
    """what holds of every answer: T = 0 gives log P = +0; a log P that is not finite gives zero rows; (d): at
    every frame of a finite utterance the occ sum to 1, and so do the ent of its first frame"""
    off = offsets(case.lens)
    for u, T in enumerate(case.lens):
        rows = slice(off[u], off[u + 1])
        if T == 0:
            assert ll[u] == 0.0 and not np.signbit(ll[u])
        elif not np.isfinite(ll[u]):
            assert not occ[rows].any() and not ent[rows].any() and not gamma[rows].any(), u
        else:
            assert np.all(np.abs(occ[rows].sum(1) - 1) <= 1e-9) and abs(ent[off[u]].sum() - 1) <= 1e-9, u
            assert all(np.all(a[rows] >= 0) for a in (occ, ent, gamma)), u


def against_the_restatement(d, g, ft=np.longdouble, what=""):
    case = d.case
    occ, ent, ll, gamma, lb, bll = d.everything(*g)
    ref = PC.post(case, lb, *g, ft=ft)
    rll = np.asarray(ref["loglik"], dtype=np.float64)
    fin = np.isfinite(rll)
    print(case.name, what, "log P", ll, "finite", int(fin[case.lens > 0].sum()), "of", int((case.lens > 0).sum()))
    assert same(ll, bll)
    assert_close(ll, rll, what=f"{what} log P")
    for name, got in (("gamma", gamma), ("occ", occ), ("ent", ent)):
        assert_close(got, np.asarray(ref[name], dtype=np.float64), what=f"{what} {name}", rows=True)
    check_rows(case, occ, ent, ll, gamma)
    return occ, ent, ll, gamma, fin


# ------------------------------------------------------------- 1. against the restatement

@pytest.mark.parametrize("name", ["narrow", "ones", "thick", "k72", "k100", "k256"])
def test_against_the_restatement(G, ctx, devices, name):
    """narrow (one wave, P = 3, a random grammar with -inf entries and norepeat, T = 0, 1, 2 and longer in one
    launch), ones (one-state words: the entry and the exit LSE2 on the same state), thick (a dense word past
    state 256: a thread's second pass), k72 (the table staged, R = 2, unrolled rounds and a tail), k100 (the table
    from L2, R = 2, rounds and a tail), k256 (the cap on K, R = 1)"""
    d = devices(name)
    NS, K = d.case.NS, d.case.K
    staged, R, slices = GC.entry_pass(NS, K)
    if name in ("k72", "k100"):
        assert R == 2 and all(r > 0 and t > 0 for r, t in slices)
        # the lattice's own LDS (csrc/ghmm_gpost.hpp): the backward launch is the larger
        assert (NS * 52 + K * 32 + 256 * 16 + K * K * 8 <= 64 << 10) == (name == "k72") == staged
    finite = 0
    for which in PC.GPU_GRAMMARS[name]:
        finite += int(against_the_restatement(d, GC.grammar(d.case, which), what=which)[4][d.case.lens > 0].sum())
    assert finite >= len(PC.GPU_GRAMMARS[name])


def test_the_cap_on_the_states(G, ctx, devices):
    """cap: NS = 2048, 64-state words, eight states per thread, 116 KB of LDS; the float64 restatement"""
    d = devices("cap")
    for which in PC.CAP_GRAMMARS:
        fin = against_the_restatement(d, GC.grammar(d.case, which), ft=np.float64, what=which)[4]
        assert fin[d.case.lens > 0].sum() >= 1


@pytest.mark.parametrize("name", GC.FULLCOV)
def test_full_covariance_words(G, ctx, devices, name):
    """full, and holes: NaN word ends and -inf columns; whatever log P they give, the restatement gives"""
    d = devices(name)
    for which in PC.GPU_GRAMMARS[name]:
        ll = against_the_restatement(d, GC.grammar(d.case, which), what=which)[2]
        if name == "holes":         # NaN word ends in every frame: NaN log P, and (check_rows) zero rows
            assert np.isnan(ll[d.case.lens > 0]).any()
        else:
            assert np.isfinite(ll).all()


@pytest.mark.parametrize("name", ["narrow", "k256", "full"])
def test_flat_and_chain_grammars(G, ctx, devices, name):
    """flat:-5, and a chain laid over ALL utterances: those it does not fit give log P = -inf and zero rows"""
    d = devices(name)
    case = d.case
    against_the_restatement(d, GC.grammar(case, "flat:-5"), what="flat:-5")
    none = 0
    for tr in GC.CHAINS[name]:
        ll = against_the_restatement(d, GC.chain(case.K, tr), what=f"chain {tr}")[2]
        none += int((ll[case.lens > 0] == -INF).sum())
    assert none > 0 or name == "full"       # (full's utterances are all long enough for its chains)


# ------------------------------------------------------------- 2. the consequences, against the live calls

def rel_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (what, got, ref)
    assert np.all(np.abs(got[fin] - ref[fin]) <= REL * np.abs(ref[fin])), (what, got, ref)


@pytest.mark.parametrize("name", ["narrow", "full"])
def test_a_one_word_grammar_is_logscore(G, ctx, devices, name):
    """(a)"""
    d = devices(name)
    for k in range(d.case.K):
        want = d.logscore(k)
        occ, ll = d.post(np.zeros(1), np.full((1, 1), -INF), np.zeros(1), dms=[d.dms[k]], entries=False)
        rel_close(ll, want, (name, k))
        fin = np.repeat(np.isfinite(ll) & (d.case.lens > 0), d.case.lens)
        assert np.all(np.abs(occ[fin, 0] - 1) <= 1e-9) and not occ[~fin].any()


@pytest.mark.parametrize("name", ["narrow", "full"])
def test_a_chain_grammar_is_the_embedded_lattice(G, ctx, devices, name):
    """(b)"""
    d = devices(name)
    case = d.case
    for tr in GC.CHAINS[name]:
        ell, egamma = d.embed([tr] * case.U)
        occ, ent, ll, gamma, lb, _ = d.everything(*GC.chain(case.K, tr))
        rel_close(ll, ell, (name, tr))
        # log Z_u from the tied gamma itself: a frame's tied gammas sum to exp(log P_u - log Z_u)
        rho = np.repeat([egamma[a:b].sum(1)[0] if b > a else 0.0 for a, b in zip(offsets(case.lens)[:-1], offsets(case.lens)[1:])],
                        case.lens)
        assert_close(egamma, gamma * rho[:, None], what=f"{name} {tr} tied gamma", rows=True)


@pytest.mark.parametrize("name", ["narrow", "ones", "k72", "full"])
def test_the_sum_holds_the_best_path(G, ctx, devices, name):
    """(c)"""
    d = devices(name)
    for which in PC.GPU_GRAMMARS[name]:
        g = GC.grammar(d.case, which)
        score = d.decode(*g)[3]
        ll = d.post(*g, entries=False)[1]
        fin = np.isfinite(score)
        assert np.all(ll[fin] >= score[fin] - REL * np.abs(score[fin])), (which, ll, score)
        assert np.array_equal(np.isfinite(ll), fin)


@pytest.mark.parametrize("how", ["in", "out"])
def test_a_word_no_string_can_hold_has_no_posterior(G, ctx, devices, how):
    """(e), exactly"""
    d = devices("narrow")
    case = d.case
    for k in range(case.K):
        g = PC.cut_off(*GC.grammar(case, "flat:-5"), k, how)
        occ, ent, ll, gamma, _, _ = d.everything(*g)
        assert not occ[:, k].any() and not ent[:, k].any() and not gamma[:, case.bo[k]:case.bo[k + 1]].any()
        assert np.isfinite(ll[case.lens > 8]).all()
        check_rows(case, occ, ent, ll, gamma)


# ------------------------------------------------------------- 3. repeats, launches, neighbours, NaN

def timed(G, ctx, call):
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    try:
        out = call()
        kt = {k: n for k, (_, n) in ctx.kernel_times().items() if n and k != "prepare"}
    finally:
        ctx.set_option(G.OPT_TIMING, 0)
    return out, kt


@pytest.mark.parametrize("name", ["narrow", "k72", "k256", "cap", "full"])
def test_launch_counts_and_a_second_call(G, ctx, devices, name):
    """2 P - 1 launches under GHMM_K_EMISSION (full-covariance: P) and TWO under GHMM_K_FORWARD; a second
    identical call repeats every byte, with another call in between"""
    d = devices(name)
    P = d.case.P
    g = GC.grammar(d.case, "random")
    first = d.everything(*g)
    d.decode(*GC.norepeat(d.case.K))
    second, kt = timed(G, ctx, lambda: d.post(*g))
    assert kt == {"emission": P if d.full else 2 * P - 1, "forward": 2}
    assert all(same(a, b) for a, b in zip(first[:3], second))
    assert all(same(a, b) for a, b in zip(first, d.everything(*g)))
    occ_only = d.post(*g, entries=False)
    assert len(occ_only) == 2 and same(occ_only[0], first[0]) and same(occ_only[1], first[2])
    for which in (G.BUF_ALPHA, G.BUF_BETA, G.BUF_SCALE, G.BUF_POST):
        with pytest.raises(G.GhmmError):
            ctx.fetch(which, (d.case.F, d.case.NS))


def test_an_utterance_does_not_depend_on_its_neighbours(G, ctx, devices):
    """narrow's longest utterances alone and inside the batch (GHMM_OPT_KERNELS = 1: the emission's bits do
    not depend on the batch either): the same bytes where log b is, the bar otherwise"""
    d = devices("narrow")
    case = d.case
    off = offsets(case.lens)
    g = GC.grammar(case, "random")
    ctx.set_option(G.OPT_KERNELS, 1)
    try:
        occ, ent, ll, gamma, lb, _ = d.everything(*g)
        for u in (7, 8):
            rows = slice(off[u], off[u + 1])
            alone = [ctx.corpus(X[rows], case.lens[u:u + 1]) for X in case.Xs]
            try:
                o1, e1, l1 = d.post(*g, corpora=alone)
                g1 = ctx.fetch(G.BUF_GAMMA, (case.lens[u], case.NS))
                b1 = ctx.fetch(G.BUF_B, (case.lens[u], case.NS))
            finally:
                for c in alone:
                    c.close()
            assert np.isfinite(l1[0])
            for a, b in ((o1, occ[rows]), (e1, ent[rows]), (g1, gamma[rows]), (l1, ll[u:u + 1])):
                if same(b1, lb[rows]):
                    assert same(a, b), u
                else:
                    assert_close(a, b, what=f"utterance {u} alone", rows=a.ndim == 2)
    finally:
        ctx.set_option(G.OPT_KERNELS, 0)


@pytest.mark.parametrize("name, u", [("full", 1), ("narrow", 7)])
def test_one_nan_frame(G, ctx, devices, name, u):
    """a frame of NaN features in one utterance: a log P that is not finite and zero rows for that utterance,
    the others as before.  Both emissions answer a frame of NaN features with log b = -inf in every column
    (their mixture sums pass over a NaN term), so through the C ABI this gives log P = -inf; were a column of
    the frame NaN, log P would have to be NaN, which the test states as well.  NaN columns in EVERY frame, and
    the NaN log P with zero rows that follow, are holes' (test_full_covariance_words)."""
    d = devices(name)
    case = d.case
    off = offsets(case.lens)
    g = GC.grammar(case, "norepeat")
    occ, ent, ll, gamma, _, _ = d.everything(*g)
    Xs = [np.array(X, dtype=np.float64) for X in case.Xs]
    Xs[0][off[u] + 5] = np.nan
    bad = [ctx.corpus(X, case.lens) for X in Xs]
    try:
        o1, e1, l1 = d.post(*g, corpora=bad)
        g1 = ctx.fetch(G.BUF_GAMMA, (case.F, case.NS))
        b1 = ctx.fetch(G.BUF_B, (case.F, case.NS))
    finally:
        for c in bad:
            c.close()
    rows = slice(off[u], off[u + 1])
    print(name, "log b of the frame", b1[off[u] + 5][:4], "log P", l1[u])
    assert np.all(np.isnan(b1[off[u] + 5]) | (b1[off[u] + 5] == -INF))
    assert np.isnan(l1[u]) if np.isnan(b1[off[u] + 5]).any() else l1[u] == -INF
    assert not o1[rows].any() and not e1[rows].any() and not g1[rows].any()
    keep = np.ones(case.F, dtype=bool)
    keep[rows] = False
    others = np.arange(case.U) != u
    assert np.isfinite(ll[u]) and np.array_equal(np.isfinite(l1[others]), np.isfinite(ll[others]))
    assert_close(l1[others], ll[others], what="log P of the others")
    for a, b, what in ((o1, occ, "occ"), (e1, ent, "ent"), (g1, gamma, "gamma")):
        assert_close(a[keep], b[keep], what=what, rows=True)


# ------------------------------------------------------------- 4. refusals

class Raw:
    """the call through the C ABI on caller-owned destinations pre-filled with a pattern, so that a refusal
    can be seen to have written nothing"""

    def __init__(self, G, ctx, case, full):
        self.G, self.ctx, self.full = G, ctx, full
        n = max(case.F, 1) * 260 + 1
        self.occ, self.ent = np.full(n, -777.0), np.full(n, -777.0)
        self.ll = np.full(case.U + 1, -777.0)

    def untouched(self):
        return all(np.all(a == -777.0) for a in (self.occ, self.ent, self.ll))

    def call(self, vocab, K, corpora, P, start, pair, fin, drop=None):
        G = self.G
        dp = G.C.POINTER(G.C.c_double)
        dest = [a.ctypes.data_as(dp) for a in (self.occ, self.ent, self.ll)]
        if drop is not None:
            dest[drop] = None
        gram = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (start, pair, fin)]
        fn = self.ctx.lib.ghmm_grammar_post_full_streams if self.full else self.ctx.lib.ghmm_grammar_post_streams
        return fn(self.ctx.h, vocab, K, corpora, P, *[None if a is None else a.ctypes.data_as(dp) for a in gram], *dest)


def handles(G, objs):
    return (G.C.c_void_p * len(objs))(*[o.h if o is not None else None for o in objs])


@pytest.mark.parametrize("name", ["mixed", "full"])
def test_refusals_write_nothing(G, ctx, devices, name):
    d = devices(name)
    case = d.case
    K, P = case.K, case.P
    raw = Raw(G, ctx, case, d.full)
    flat = [m for w in d.dms for m in w]
    vocab, corpora = handles(G, flat), handles(G, d.corpora)
    arg, unsupported = G.ERR_ARG, G.ERR_UNSUPPORTED
    start, pair, fin = GC.norepeat(K)
    extra = []

    def with_at(a, i, v):
        a = a.copy()
        a.flat[i] = v
        return a
    try:
        for drop in (0, 2):
            assert raw.call(vocab, K, corpora, P, start, pair, fin, drop=drop) == arg, ("null destination", drop)
        assert raw.call(vocab, K, corpora, P, start, None, fin) == arg, "null pair"
        for bad in (np.nan, INF):
            assert raw.call(vocab, K, corpora, P, with_at(start, K - 1, bad), pair, fin) == arg, ("start", bad)
            assert raw.call(vocab, K, corpora, P, start, with_at(pair, K * K - 1, bad), fin) == arg, ("pair", bad)
            assert raw.call(vocab, K, corpora, P, start, pair, with_at(fin, 0, bad)) == arg, ("fin", bad)
        assert raw.call(None, K, corpora, P, start, pair, fin) == arg
        assert raw.call(vocab, 0, corpora, P, start, pair, fin) == arg
        # K = 257: the first word 257 times (within the cap on the states)
        assert case.Ns[0] * 257 <= 2048
        assert raw.call(handles(G, flat[:P] * 257), 257, corpora, P, None, np.zeros((257, 257)), None) == unsupported
        assert "GHMM_GRAMMAR_MAX_WORDS" in ctx.lib.ghmm_last_error().decode()
        # NS above the cap: 33 times a word of 64 states (2112 > 2048); a word of 65 states
        h = case.words[0]
        rng = np.random.default_rng(3)
        if d.full:
            from fullcov_support import rand_fmodel
            w64 = [ctx.full_model(rand_fmodel(G, rng, 64, x.M, x.D, spread=1.0, asym=False)) for x in h]
        else:
            import vocab_cases as V
            from fullcov_support import banded
            w64 = [ctx.model(V.rand_model(G, rng, 64, x.M, x.D, banded(rng, 64))) for x in h]
            w65 = [ctx.model(V.rand_model(G, rng, 65, x.M, x.D, banded(rng, 65))) for x in h]
            extra += w65
            assert raw.call(handles(G, flat[:P] + w65), 2, corpora, P, None, np.zeros((2, 2)), None) == unsupported
        extra += w64
        assert raw.call(handles(G, w64 * 33), 33, corpora, P, None, np.zeros((33, 33)), None) == unsupported
        assert "2048" in ctx.lib.ghmm_last_error().decode()
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert raw.call(vocab, K, corpora, P, start, pair, fin) == unsupported, "robust"
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert raw.untouched()
        # U = 0 touches nothing, with or without destinations, with or without a table
        empty = [ctx.corpus(np.zeros((0, x.D)), np.zeros(0, dtype=np.int32)) for x in h]
        extra += empty
        assert raw.call(vocab, K, handles(G, empty), P, start, pair, fin) == G.OK
        assert raw.call(vocab, K, handles(G, empty), P, None, None, None, drop=0) == G.OK
        assert raw.untouched()
        # the same arguments, valid, do write: the rows and log P, nothing behind them; ent may be left out
        assert raw.call(vocab, K, corpora, P, start, pair, fin, drop=1) == G.OK
        assert np.all(raw.ent == -777.0)
        assert raw.call(vocab, K, corpora, P, start, pair, fin) == G.OK
        occ, ent, ll = d.post(start, pair, fin)
        for got, ref in ((raw.occ, occ.ravel()), (raw.ent, ent.ravel()), (raw.ll, ll)):
            assert same(got[:len(ref)], ref) and np.all(got[len(ref):] == -777.0)
    finally:
        for o in extra:
            o.close()


def test_utterances_of_no_frames(G, ctx, devices):
    """all utterances empty: U > 0, F = 0: log P = 0, no rows"""
    d = devices("mixed")
    case = d.case
    lens = np.zeros(3, dtype=np.int32)
    empty = [ctx.corpus(np.zeros((0, x.D)), lens) for x in case.words[0]]
    raw = Raw(G, ctx, case, False)
    try:
        rc = raw.call(handles(G, [m for w in d.dms for m in w]), case.K, handles(G, empty), case.P,
                      *GC.random(case.K, 3))
        assert rc == G.OK
        assert np.all(raw.ll[:3] == 0.0) and not np.signbit(raw.ll[:3]).any() and raw.ll[3] == -777.0
        assert np.all(raw.occ == -777.0) and np.all(raw.ent == -777.0)
    finally:
        for c in empty:
            c.close()
