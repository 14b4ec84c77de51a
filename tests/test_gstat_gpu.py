"""Baum-Welch statistics on the grammar lattice on the GPU: ghmm_estep_grammar_streams (the embedded E-step's
emission with posteriors, k_gpost_fwd, k_gpost_bwd in its statistics form, ghmm_estep's statistics launches on
the concatenated vocabulary, k_embed_scatter) through the C ABI by ghmm.py — GPU box only.  The cases and
grammars are grammar_cases', the restatement is gstat_cases'; test_gstat_host.py shows on the CPU that the
restatement is the definition.

The long-double restatement runs on the log b fetched from the device (GHMM_BUF_B) and, with one stream, on the
device's posteriors (GHMM_BUF_POST); with several streams the posteriors are not served and the restated ones of
estep_log_ref.posteriors take their place (narrow: P = 3).  log P, gamma per utterance and every word's and
stream's blocks are held to estep_log_ref.block_dist at RTOL, which is fullcov_support.assert_close's bar, with
equal zero, -inf and NaN patterns.  Against the live neighbouring calls ("to rounding") the bar is the same
RTOL; "bit for bit" is under GHMM_OPT_KERNELS = 1."""
import numpy as np
import pytest

import estep_log_ref as E
import gpost_cases as PC
import grammar_cases as GC
import gstat_cases as GS
import vocab_cases as V
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import RTOL, assert_close, banded, code, extended, offsets
from test_gpost_gpu import handles
from test_logscore_gpu import TIERS, same, tier_of, timed

pytestmark = pytest.mark.gpu

BLOCKS = E.BLOCKS[:-2]          # without loglik and n_utt


class Device:
    """a case's device vocabulary, corpora and per-word statistics vectors"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        self.K, self.P, self.F, self.U, self.NS = case.K, case.P, case.F, case.U, case.NS
        self.dms = [[ctx.model(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self.st = [[ctx.stats(h.N, h.M, h.D) for h in w] for w in case.words]
        self._run = {}
        self._posts = None

    def call(self, g, corpora=None, dms=None, st=None):
        start, pair, fin = g
        self.ctx.estep_grammar_streams(dms or self.dms, corpora or self.corpora, pair, st or self.st, start, fin)

    def vectors(self, st=None):
        return [[s.download() for s in w] for w in (st or self.st)]

    def split(self, v):
        return [[self.G.split_stats(x, h.N, h.M, h.D) for x, h in zip(vw, w)] for vw, w in zip(v, self.case.words)]

    def fetch_all(self, st=None, F=None, U=None):
        G, ctx = self.G, self.ctx
        F, U = self.F if F is None else F, self.U if U is None else U
        r = {"v": self.vectors(st)}
        r["stats"] = self.split(r["v"])
        r["logb"] = ctx.fetch(G.BUF_B, (F, self.NS))
        r["gamma"] = ctx.fetch(G.BUF_GAMMA, (F, self.NS))
        r["ll"] = ctx.fetch(G.BUF_LOGLIK, (U,))
        if self.P == 1:
            r["posts"] = [ctx.fetch(G.BUF_POST, (F, self.NS * self.case.words[0][0].M))]
        return r

    def run(self, which, tier=1, delta=1):
        key = (which, tier, delta)
        if key not in self._run:
            with tier_of(self.G, self.ctx, tier):
                self.ctx.set_option(self.G.OPT_DELTA, delta)
                try:
                    self.call(GC.grammar(self.case, which))
                    self._run[key] = self.fetch_all()
                finally:
                    self.ctx.set_option(self.G.OPT_DELTA, 1)
        return self._run[key]

    def posts_of(self, r):
        """the posteriors the restatement runs on: the device's with one stream, the restated ones beyond"""
        if "posts" in r:
            return r["posts"]
        if self._posts is None:
            case = self.case
            self._posts = [np.concatenate([E.posteriors(w[p], case.Xs[p]) for w in case.words], axis=1)
                           for p in range(case.P)]
        return self._posts

    def restated(self, r, g, delta=1, ft=np.longdouble):
        case = self.case
        return GS.estep(case.words, case.Xs, case.lens, *g, delta=delta, ft=ft, logb=r["logb"], posts=self.posts_of(r))

    def close(self):
        for o in [m for w in self.dms for m in w] + self.corpora + [s for w in self.st for s in w]:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(G, ctx, make_case(G, name))
        return made[name]
    yield get
    for d in made.values():
        d.close()


HOLES_WORD = 1


def make_case(G, name):
    """grammar_cases' case of a name; holes: narrow's first stream with the determinant of word 1's last state
    zeroed, so that log wk = +inf there and the vector tier's log b of that column is NaN in every frame"""
    if name != "holes":
        return GC.make(G, name)
    case = GC.make(G, "narrow").stream0()
    case.name = "narrow"            # (its grammars are narrow's)
    h = case.words[HOLES_WORD][0]
    h.det[h.N - 1, :] = 0.0
    return case


def check_against(d, r, ref, what):
    """log P, gamma per utterance and every word's blocks at RTOL, with equal zero, -inf and NaN patterns"""
    worst = E.block_dist(r["ll"], ref["loglik"])
    assert worst <= RTOL, (what, "log P", worst)
    g64 = np.asarray(ref["gamma"], dtype=np.float64)
    assert np.array_equal(r["gamma"] == 0.0, g64 == 0.0), f"{what}: zeros of gamma differ"
    off = offsets(d.case.lens)
    for u in range(d.U):
        dist = E.block_dist(r["gamma"][off[u]:off[u + 1]], ref["gamma"][off[u]:off[u + 1]])
        assert dist <= RTOL, (what, "gamma of utterance", u, dist)
        worst = max(worst, dist)
    for k in range(d.K):
        for p in range(d.P):
            got, want = r["stats"][k][p], ref["stats"][k][p]
            for b in E.BLOCKS:
                w64 = np.asarray(want[b], dtype=np.float64)
                assert np.array_equal(np.asarray(got[b]) == 0.0, w64 == 0.0), f"{what}: zeros of {b} of word {k} differ"
                dist = E.block_dist(got[b], want[b])
                assert dist <= RTOL, (what, k, p, b, dist)
                worst = max(worst, dist)
    return worst


# ------------------------------------------------------------- 1. against the restatement

@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(GS.GPU_GRAMMARS))
def test_against_the_restatement(G, ctx, devices, name, tier):
    """narrow (P = 3, T = 0, 1, 2 and longer in one launch), ones (one-state words: xi is the self-loop only and
    every state is an end), thick (a dense word in a thread's second pass), k72 and k100 (R = 2 slices, the table
    staged and from L2), k256 (the cap on K, the table from L2)"""
    d = devices(name)
    finite = 0
    for which in GS.GPU_GRAMMARS[name]:
        r = d.run(which, tier)
        ref = d.restated(r, GC.grammar(d.case, which))
        worst = check_against(d, r, ref, f"{name} {which} tier {tier}")
        print(f"{name} {which} tier {tier}: worst distance from the long-double restatement {worst:.2e}")
        finite += int(np.isfinite(r["ll"][d.case.lens > 0]).sum())
        for k in range(d.K):                        # loglik and n_utt: the same bits in every vector
            for p in range(d.P):
                assert same(r["v"][k][p][-2:], r["v"][0][0][-2:])
        assert r["v"][0][0][-1] == d.U
        if name == "ones":
            for k in range(d.K):
                na = r["stats"][k][0]["num_a"]
                assert na.shape == (1, 1) and na[0, 0] > 0
    assert finite >= len(GS.GPU_GRAMMARS[name])


def test_the_cap_on_the_states(G, ctx, devices):
    """cap: NS = 2048, 64-state words, eight states per thread (256 VGPRs and no scratch); the float64 restatement"""
    d = devices("cap")
    for which in GS.CAP_GRAMMARS:
        r = d.run(which, 1)
        ref = d.restated(r, GC.grammar(d.case, which), ft=np.float64)
        check_against(d, r, ref, f"cap {which}")
        assert np.isfinite(r["ll"][d.case.lens > 0]).sum() >= 1


def test_nan_log_p_gives_zero_sums_and_a_nan_loglik(G, ctx, devices):
    """holes: a NaN column in every frame: log P is NaN, every gamma row and EVERY sum is exactly 0 and loglik is
    NaN.  The bad state's own posteriors are NaN as the emission leaves them (its mixture terms are +inf - +inf);
    the call zeroes the posterior rows of an utterance without a finite log P, so no 0 x NaN reaches a sum"""
    d = devices("holes")
    case = d.case
    bad = case.bo[HOLES_WORD + 1] - 1
    M = case.words[0][0].M
    for which in ("flat:-5", "norepeat"):
        with tier_of(G, ctx, 1):
            # the emission alone leaves NaN posteriors in the bad state: what the call has to keep out of the sums
            ctx.estep_embed_streams(d.dms, d.corpora, [(0,) if T else () for T in case.lens], d.st)
            raw = ctx.fetch(G.BUF_POST, (d.F, d.NS, M))
            assert np.isnan(raw[:, bad]).all(), "the case does not make its NaN posteriors"
        d._run.clear()
        r = d.run(which, 1)
        assert np.isnan(r["logb"][:, bad]).all(), "the case does not make its NaN column"
        live = case.lens > 0
        assert np.isnan(r["ll"][live]).all() and np.all(r["ll"][~live] == 0)
        assert not r["gamma"].any() and not r["posts"][0].any()
        for k in range(d.K):
            v = r["v"][k][0]
            assert not np.any(v[:-2]) and not np.isnan(v[:-2]).any(), (which, k)
            assert np.isnan(v[-2]) and v[-1] == d.U


@extended
@pytest.mark.parametrize("delta", GS.DELTAS)
@pytest.mark.parametrize("name", GS.DELTA_CASES)
def test_under_other_deltas(G, ctx, devices, name, delta):
    """GHMM_OPT_DELTA 0, 1, 2, 3, 7 on one state per thread (narrow) and on two with a dense word in the second
    (thick): xi[p][o] for every p and o, num_a non-zero at the widest offset the case has and 0 outside the band"""
    d = devices(name)
    r = d.run("random", 1, delta)
    check_against(d, r, d.restated(r, GC.grammar(d.case, "random"), delta), f"{name} delta {delta}")
    widest = expected = 0
    for k in range(d.K):
        na = r["stats"][k][0]["num_a"]
        i, j = np.indices(na.shape)
        assert not np.any(na[(j < i) | (j > i + delta)]), "num_a outside the band"
        A = np.asarray(d.case.words[k][0].A)
        for o in range(min(delta, na.shape[0] - 1) + 1):
            if np.any(np.diagonal(A, o) > 0):
                expected = max(expected, o)
            if np.any(np.diagonal(na, o) > 0):
                widest = max(widest, o)
    # the widest offset the case has inside the band: its dense words reach every offset up to delta
    assert widest == expected and expected >= min(delta, 2), (widest, expected, delta)


# ------------------------------------------------------------- 2. the consequences, against the live calls

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["narrow", "thick", "k72"])
def test_gamma_and_log_p_are_grammar_posts(G, ctx, devices, name, tier):
    """(a): bit for bit under GHMM_OPT_KERNELS = 1, to rounding otherwise; and the posteriors call gives the
    same bytes before and after this one"""
    d = devices(name)
    for which in GS.GPU_GRAMMARS[name]:
        g = GC.grammar(d.case, which)
        with tier_of(G, ctx, tier):
            before = ctx.grammar_post_streams(d.dms, d.corpora, g[1], g[0], g[2], entries=True)
            pg = ctx.fetch(G.BUF_GAMMA, (d.F, d.NS))
            pl, pb = ctx.fetch(G.BUF_LOGLIK, (d.U,)), ctx.fetch(G.BUF_B, (d.F, d.NS))
            d.call(g)
            sg, sl = ctx.fetch(G.BUF_GAMMA, (d.F, d.NS)), ctx.fetch(G.BUF_LOGLIK, (d.U,))
            sb = ctx.fetch(G.BUF_B, (d.F, d.NS))
            after = ctx.grammar_post_streams(d.dms, d.corpora, g[1], g[0], g[2], entries=True)
        assert all(same(a, b) for a, b in zip(before, after))
        if tier == 1:
            assert same(pb, sb), "the two emission modes differ in log b on the vector tier"
            assert same(pg, sg) and same(pl, sl)
        else:
            assert_close(sl, pl, what=f"{name} {which} log P")
            assert_close(sg, pg, what=f"{name} {which} gamma", rows=True)


@extended
@pytest.mark.parametrize("tier", TIERS)
def test_a_chain_grammar_is_the_embedded_estep(G, ctx, devices, tier):
    """(b) on one-utterance corpora: every block of every word's vector is estep_embed_streams' times the
    reciprocal of a frame's sum of that call's tied gamma; loglik is equal"""
    d = devices("narrow")
    case = d.case
    off = offsets(case.lens)
    est = [[ctx.stats(h.N, h.M, h.D) for h in w] for w in case.words]
    seen = 0
    try:
        with tier_of(G, ctx, tier):
            for tr in GC.CHAINS["narrow"]:
                for u in np.nonzero(case.lens >= 2 * len(tr) + 4)[0][:3]:
                    rows = slice(off[u], off[u + 1])
                    alone = [ctx.corpus(X[rows], case.lens[u:u + 1]) for X in case.Xs]
                    try:
                        ctx.estep_embed_streams(d.dms, alone, [tr], est)
                        ev = d.split(d.vectors(est))
                        eg = ctx.fetch(G.BUF_GAMMA, (case.lens[u], d.NS))
                        el = ctx.fetch(G.BUF_LOGLIK, (1,))
                        d.call(GC.chain(case.K, tr), corpora=alone)
                        gv = d.split(d.vectors())
                        gl = ctx.fetch(G.BUF_LOGLIK, (1,))
                    finally:
                        for c in alone:
                            c.close()
                    assert_close(gl, el, what=f"log P of {tr} on {u}")
                    if not np.isfinite(el[0]) or not eg[0].sum() > 0:
                        continue
                    seen += 1
                    rho = 1.0 / eg[0].sum()
                    for k in range(d.K):
                        for p in range(d.P):
                            for b in BLOCKS:
                                dist = E.block_dist(gv[k][p][b], ev[k][p][b] * rho)
                                assert dist <= RTOL, (tr, u, k, p, b, dist)
                            assert gv[k][p]["loglik"] == gl[0] and gv[k][p]["n_utt"] == 1
    finally:
        for s in [s for w in est for s in w]:
            s.close()
        d._run.clear()
    assert seen >= len(GC.CHAINS["narrow"])


@pytest.mark.parametrize("name", ["narrow", "ones", "thick", "k256"])
def test_rows_frames_and_the_m_step(G, ctx, devices, name):
    """(c): wherever the band holds every a_jj' > 0 the row of num_a sums to den_a; (d): the den_c sum to the
    frames of the utterances with finite log P; (f): ghmm_mstep on every held word gives a finite model"""
    d = devices(name)
    case = d.case
    d._run.clear()              # (a fresh call: the M-steps below read d.st, which must be THIS call's vectors)
    r = d.run("random", 1)
    frames = int(case.lens[np.isfinite(r["ll"])].sum())
    total = sum(float(r["stats"][k][0]["den_c"].sum()) for k in range(d.K))
    assert frames > 0 and abs(total - frames) <= RTOL * frames, (total, frames)
    rows = 0
    for k in range(d.K):
        A = np.asarray(case.words[k][0].A)
        i, j = np.indices(A.shape)
        inside = (j >= i) & (j <= i + 1)
        st = r["stats"][k][0]
        for row in range(A.shape[0]):
            if np.any(A[row][~inside[row]] > 0):
                continue
            rows += 1
            assert abs(st["num_a"][row].sum() - st["den_a"][row]) <= RTOL * st["den_a"][row] + 1e-300, (k, row)
    assert rows > 0
    held = [k for k in range(d.K) if np.all(r["stats"][k][0]["den_c"] > 1e-6)][:8]
    assert held
    for k in held:
        for p in range(d.P):
            m = ctx.model(case.words[k][p])
            try:
                ctx.mstep(m, d.st[k][p])
                new = m.get()
            finally:
                m.close()
            assert all(np.all(np.isfinite(a)) for a in new.arrays()), (k, p)
            assert np.all(np.abs(new.c.sum(1) - 1) <= 1e-9)


@pytest.mark.parametrize("how", ["in", "out"])
def test_a_word_no_string_can_hold_has_zero_sums(G, ctx, devices, how):
    """(e), exactly"""
    d = devices("narrow")
    case = d.case
    for k in range(case.K):
        d.call(PC.cut_off(*GC.grammar(case, "flat:-5"), k, how))
        v = d.vectors()
        assert all(not np.any(v[k][p][:-2]) for p in range(d.P))
        assert same(v[k][0][-2:], v[(k + 1) % d.K][0][-2:]) and v[k][0][-1] == d.U      # the common loglik and n_utt
        assert np.isfinite(ctx.fetch(G.BUF_LOGLIK, (d.U,))[case.lens > 8]).all()
        assert any(np.any(v[q][0][:-2]) for q in range(d.K) if q != k)
        assert not ctx.fetch(G.BUF_GAMMA, (d.F, d.NS))[:, case.bo[k]:case.bo[k + 1]].any()


# ------------------------------------------------------------- 3. repeats, launches, neighbours, the edges

@pytest.mark.parametrize("name", ["narrow", "k72", "k256", "cap"])
def test_launch_counts_and_a_second_call(G, ctx, devices, name):
    """2 P - 1 launches under GHMM_K_EMISSION, two under GHMM_K_FORWARD, per stream ghmm_estep's statistics
    launches (vector tier: one k_mixstats, one k_reduce_all) and the scatter under GHMM_K_REDUCE; a second
    identical call repeats every byte, with another call in between; what the workspace serves afterwards"""
    d = devices(name)
    P = d.P
    g = GC.grammar(d.case, "random")
    with tier_of(G, ctx, 1):
        d.call(g)
        first = d.fetch_all()
        ctx.connect_grammar_streams(d.dms, d.corpora, *[GC.norepeat(d.K)[i] for i in (1, 0, 2)])
        kt = timed(G, ctx, lambda: d.call(g))
        assert kt == {"emission": 2 * P - 1, "forward": 2, "mixstats": P, "reduce": 2 * P}
        second = d.fetch_all()
        for buf in (G.BUF_ALPHA, G.BUF_BETA, G.BUF_SCALE):
            assert code(G, lambda: ctx.fetch(buf, (1,))) == G.ERR_ARG
        if P > 1:
            assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
        assert code(G, lambda: ctx.forward(d.dms[0][0], d.corpora[0])) == G.ERR_ARG   # the row API does not reuse it
    assert all(same(a, b) for va, vb in zip(first["v"], second["v"]) for a, b in zip(va, vb))
    assert all(same(first[x], second[x]) for x in ("logb", "gamma", "ll"))


def test_an_utterance_alone_and_the_sum_of_the_utterances(G, ctx, devices):
    """narrow's utterances one by one (GHMM_OPT_KERNELS = 1: the emission's bits do not depend on the batch):
    gamma and log P are the batch's bytes, and the vectors of the one-utterance calls add up to the batch's, to
    rounding"""
    d = devices("narrow")
    case = d.case
    off = offsets(case.lens)
    g = GC.grammar(case, "random")
    with tier_of(G, ctx, 1):
        d.call(g)
        whole = d.fetch_all()
        total = [[np.zeros_like(v) for v in w] for w in whole["v"]]
        for u in range(d.U):
            rows = slice(off[u], off[u + 1])
            alone = [ctx.corpus(X[rows], case.lens[u:u + 1]) for X in case.Xs]
            try:
                d.call(g, corpora=alone)
                one = d.fetch_all(F=int(case.lens[u]), U=1)
            finally:
                for c in alone:
                    c.close()
            assert same(one["logb"], whole["logb"][rows]) and same(one["gamma"], whole["gamma"][rows])
            assert same(one["ll"], whole["ll"][u:u + 1])
            for k in range(d.K):
                for p in range(d.P):
                    total[k][p] += one["v"][k][p]
    for k in range(d.K):
        for p in range(d.P):
            got, ref = d.split(total)[k][p], whole["stats"][k][p]
            for b in E.BLOCKS:
                assert np.array_equal(np.isnan(got[b]), np.isnan(ref[b]))
                if not np.isnan(ref[b]).any():
                    assert E.block_dist(got[b], ref[b]) <= RTOL, (k, p, b)


def test_no_frames_one_frame_and_no_utterance(G, ctx, devices):
    """T = 0 adds 0 to loglik and counts in n_utt; T = 1 gives den_c only (ones: a one-state word can begin and end
    in one frame; a longer word cannot, its log P is -inf); U = 0 gives all-zero vectors"""
    d = devices("ones")
    case = d.case
    g = GC.flat(d.K, -1.0)
    made = []
    try:
        lens = np.array([0, 1, 0], dtype=np.int32)
        short = [ctx.corpus(X[:1], lens) for X in case.Xs]
        made += short
        d.call(g, corpora=short)
        v = d.split(d.vectors())
        ll = ctx.fetch(G.BUF_LOGLIK, (3,))
        assert ll[0] == 0 and ll[2] == 0 and np.isfinite(ll[1])
        total = 0.0
        for k in range(d.K):
            for p in range(d.P):
                st = v[k][p]
                assert st["loglik"] == ll[1] and st["n_utt"] == 3
                assert not st["num_a"].any() and not st["den_a"].any()
            total += v[k][0]["den_c"].sum()
        assert abs(total - 1) <= 1e-12
        lens0 = np.zeros(2, dtype=np.int32)
        none_frames = [ctx.corpus(np.zeros((0, h.D)), lens0) for h in case.words[0]]
        made += none_frames
        d.call(g, corpora=none_frames)
        for w in d.vectors():
            for x in w:
                assert not np.any(x[:-1]) and x[-1] == 2
        none = [ctx.corpus(np.zeros((0, h.D)), np.zeros(0, dtype=np.int32)) for h in case.words[0]]
        made += none
        d.call(GC.grammar(case, "random"))
        assert np.any(d.st[0][0].download())
        d.call(g, corpora=none)
        assert not any(np.any(x) for w in d.vectors() for x in w)
        assert [float(x) for x in d.st[0][0].loglik()] == [0.0, 0.0]
        # (U = 0 needs no table)
        assert ctx.lib.ghmm_estep_grammar_streams(ctx.h, handles(G, [m for w in d.dms for m in w]), d.K,
                                                  handles(G, none), d.P, None, None, None,
                                                  handles(G, [s for w in d.st for s in w])) == G.OK
    finally:
        for c in made:
            c.close()
        d._run.clear()


# ------------------------------------------------------------- 4. refusals

def raw_call(G, ctx, vocab, K, corpora, P, start, pair, fin, stats):
    dp = G.C.POINTER(G.C.c_double)
    gram = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (start, pair, fin)]
    return ctx.lib.ghmm_estep_grammar_streams(ctx.h, vocab, K, corpora, P,
                                              *[None if a is None else a.ctypes.data_as(dp) for a in gram], stats)


def test_refusals_write_nothing(G, ctx, devices):
    """the union of grammar_post_streams' refusals and estep_embed_streams' checks of the vectors, each before
    anything is launched, grown or written"""
    d = devices("narrow")
    case = d.case
    K, P = d.K, d.P
    flat = [m for w in d.dms for m in w]
    flat_st = [s for w in d.st for s in w]
    vocab, corpora, stats = handles(G, flat), handles(G, d.corpora), handles(G, flat_st)
    arg, unsupported = G.ERR_ARG, G.ERR_UNSUPPORTED
    start, pair, fin = GC.norepeat(K)
    h = case.words[0]
    rng = np.random.default_rng(3)
    w64, w65 = ([ctx.model(V.rand_model(G, rng, N, x.M, x.D, banded(rng, N))) for x in h] for N in (64, 65))
    s64, s65 = ([ctx.stats(N, x.M, x.D) for x in h] for N in (64, 65))
    full = ctx.stats_full(h[0].N, h[0].M, h[0].D)
    other = ctx.stats(h[0].N, h[0].M + 1, h[0].D)
    extra = w64 + w65 + s64 + s65 + [full, other]

    def with_at(a, i, v):
        a = a.copy()
        a.flat[i] = v
        return a
    try:
        with tier_of(G, ctx, 1):
            d.call((start, pair, fin))
            before = d.fetch_all()
            ctx.set_option(G.OPT_TIMING, 1)
            ctx.kernel_times_reset()
            try:
                assert raw_call(G, ctx, vocab, K, corpora, P, start, pair, fin, None) == arg, "null stats"
                for bad in (None, full, other):
                    st = handles(G, [bad] + flat_st[1:])
                    assert raw_call(G, ctx, vocab, K, corpora, P, start, pair, fin, st) == arg, "a null, full or other vector"
                assert raw_call(G, ctx, vocab, K, corpora, P, start, None, fin, stats) == arg, "null pair"
                for bad in (np.nan, np.inf):
                    assert raw_call(G, ctx, vocab, K, corpora, P, with_at(start, K - 1, bad), pair, fin, stats) == arg
                    assert raw_call(G, ctx, vocab, K, corpora, P, start, with_at(pair, K * K - 1, bad), fin, stats) == arg
                    assert raw_call(G, ctx, vocab, K, corpora, P, start, pair, with_at(fin, 0, bad), stats) == arg
                assert raw_call(G, ctx, None, K, corpora, P, start, pair, fin, stats) == arg
                assert raw_call(G, ctx, vocab, 0, corpora, P, start, pair, fin, stats) == arg
                assert case.Ns[0] * 257 <= 2048
                assert raw_call(G, ctx, handles(G, flat[:P] * 257), 257, corpora, P, None, np.zeros((257, 257)), None,
                                handles(G, flat_st[:P] * 257)) == unsupported
                assert "GHMM_GRAMMAR_MAX_WORDS" in ctx.lib.ghmm_last_error().decode()
                assert raw_call(G, ctx, handles(G, flat[:P] + w65), 2, corpora, P, None, np.zeros((2, 2)), None,
                                handles(G, flat_st[:P] + s65)) == unsupported, "65 states"
                assert raw_call(G, ctx, handles(G, w64 * 33), 33, corpora, P, None, np.zeros((33, 33)), None,
                                handles(G, s64 * 33)) == unsupported
                assert "2048" in ctx.lib.ghmm_last_error().decode()
                ctx.set_option(G.OPT_ROBUST, 1)
                try:
                    assert raw_call(G, ctx, vocab, K, corpora, P, start, pair, fin, stats) == unsupported, "robust"
                finally:
                    ctx.set_option(G.OPT_ROBUST, 0)
                assert not any(n for k, (_, n) in ctx.kernel_times().items()), "a refusal launched something"
            finally:
                ctx.set_option(G.OPT_TIMING, 0)
            after = d.fetch_all()
        assert all(same(a, b) for va, vb in zip(before["v"], after["v"]) for a, b in zip(va, vb))
        assert all(same(before[x], after[x]) for x in ("logb", "gamma", "ll"))
        assert not np.any(s64[0].download()) and not np.any(s65[0].download())
    finally:
        for o in extra:
            o.close()
        d._run.clear()
