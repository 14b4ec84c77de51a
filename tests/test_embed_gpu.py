"""The embedded Baum-Welch E-step on the GPU: ghmm_estep_embed_streams (the vocabulary's emission in its "log b
and posteriors" mode, k_embed_fwd / k_embed_bwd over the transcripts' word instances, ghmm_estep's statistics
launches on the concatenated vocabulary, k_embed_scatter) and embed.embedded_em — GPU box only.  The cases and
the restatement are embed_cases.py's; test_embed_host.py shows on the CPU that they hold what is leaned on
here.  Under GHMM_OPT_KERNELS = 1 and under the default (matrix-core) tier unless stated.

  lattice      the long-double restatement on the DEVICE's own log b and posteriors (one stream), per word with
               estep_log_ref.block_dist at RTOL and equal zero, -inf and NaN patterns: log P, the tied gamma,
               num_a, den_a, den_c, num_c, num_mu, num_var, over embed_cases' SMALL and REACH; delta 0, 2, 3 and
               up to 7; the table columns after a call that filled them; every frame's gamma sum against
               exp(log P - log Z); the cap (float64 restatement): log P, the gamma sums, den_c
  emission     BUF_B bit for bit what ghmm_align_streams leaves
  identities   bit for bit under GHMM_OPT_KERNELS = 1: consequence (a) with one and two streams, a second call,
               the same call after a connect_streams on another vocabulary, loglik and n_utt in every vector,
               Stats.loglik() (the mailbox)
  to rounding  consequences (b) and (c); the rows of num_a against den_a
  the point    embedded_em for four iterations against the float64 restatement driven with oracle_lib.mstep
  the contract refusals write nothing, U = 0, the launch counts, BUF_ALPHA afterwards"""
import numpy as np
import pytest

import embed_cases as EC
import estep_log_ref as E
import logscore_cases as LC
import oracle_lib as O
import vocab_cases as V
from _load import load_pkg
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import RTOL, banded, code, extended, offsets
from fullstreams_ref import stream_frames
from test_align_gpu import flat_transcripts, handles
from test_logscore_gpu import TIERS, same, tier_of, timed

pytestmark = pytest.mark.gpu

BLOCKS = E.BLOCKS[:-2]          # without loglik and n_utt


class Device:
    """a case's device vocabulary, corpora and per-word statistics vectors; stream0: the first stream alone"""

    def __init__(self, G, ctx, case, transcripts=None):
        self.G, self.ctx, self.case = G, ctx, case
        self.transcripts = list(case.transcripts if transcripts is None else transcripts)
        self.K, self.P, self.F, self.U, self.NS = case.K, case.P, case.F, case.U, case.NS
        self.dms = [[ctx.model(h) for h in w] for w in case.words]
        self._models = [m for w in self.dms for m in w]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self.st = [[ctx.stats(h.N, h.M, h.D) for h in w] for w in case.words]
        self._run = {}

    def call(self, transcripts=None):
        self.ctx.estep_embed_streams(self.dms, self.corpora, self.transcripts if transcripts is None else transcripts,
                                     self.st)

    def vectors(self):
        return [[s.download() for s in w] for w in self.st]

    def split(self, v):
        return [[self.G.split_stats(x, h.N, h.M, h.D) for x, h in zip(vw, w)] for vw, w in zip(v, self.case.words)]

    def fetch_all(self):
        G, ctx = self.G, self.ctx
        r = {"v": self.vectors()}
        r["stats"] = self.split(r["v"])
        r["logb"] = ctx.fetch(G.BUF_B, (self.F, self.NS))
        r["gamma"] = ctx.fetch(G.BUF_GAMMA, (self.F, self.NS))
        r["ll"] = ctx.fetch(G.BUF_LOGLIK, (self.U,))
        if self.P == 1:
            r["posts"] = [ctx.fetch(G.BUF_POST, (self.F, self.NS * self.case.words[0][0].M))]
        return r

    def run(self, tier, delta=1):
        if (tier, delta) not in self._run:
            with tier_of(self.G, self.ctx, tier):
                self.ctx.set_option(self.G.OPT_DELTA, delta)
                try:
                    self.call()
                    self._run[tier, delta] = self.fetch_all()
                finally:
                    self.ctx.set_option(self.G.OPT_DELTA, 1)
        return self._run[tier, delta]

    def close(self):
        for o in self._models + self.corpora + [s for w in self.st for s in w]:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name, stream0=False):
        if (name, stream0) not in made:
            case = EC.make(G, name)
            if stream0 and case.P > 1:
                one = case.stream0()
                one.transcripts, one.name = case.transcripts, case.name
                case = one
            made[name, stream0] = Device(G, ctx, case)
        return made[name, stream0]
    yield get
    for d in made.values():
        d.close()


def restated(d, r, delta=1, ft=np.longdouble):
    """the restatement on a run's own log b and posteriors, computed once per run and left unchanged"""
    key = ("restated", delta, ft)
    if key not in r:
        r[key] = EC.estep(d.case.words, d.case.Xs, d.case.lens, d.transcripts, delta, ft, logb=r["logb"],
                          posts=r["posts"])
    return r[key]


def check_against(d, r, ref, what):
    """log P, the tied gamma and every word's blocks at RTOL, with equal zero, -inf and NaN patterns"""
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


# ------------------------------------------------------------- 1. the lattice

@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", EC.SMALL + EC.REACH)
def test_lattice_against_the_long_double_restatement(G, ctx, devices, name, tier):
    """SMALL, and REACH: tie_gamma's table loop on 64, 192 and 256 threads (broad, deep, broad256), four and
    eight states per thread (pass4, pass8), 128 and 192 threads (wide128, wide), log Z over a last word of 17
    and of 64 states (mid, deep; the gammas are normalised by it)"""
    d = devices(name, stream0=True)
    r = d.run(tier)
    worst = check_against(d, r, restated(d, r), f"{name} tier {tier}")
    print(f"{name} tier {tier}: worst distance from the long-double restatement {worst:.2e}")
    absent = [k for k in range(d.K) if k not in EC.present(d.case)]
    for k in absent:
        assert not np.any(r["v"][k][0][:-2]) and same(r["v"][k][0][-2:], r["v"][0][0][-2:])
        assert not np.any(r["gamma"][:, d.case.bo[k]:d.case.bo[k + 1]])


@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name,delta", [(n, x) for n in EC.DELTA_CASES for x in EC.DELTAS if x != 1] +
                         [(n, x) for n, xs in EC.WIDE_DELTAS.items() for x in xs])
def test_lattice_under_other_deltas(G, ctx, devices, name, delta, tier):
    """delta 0, 2, 3 on one state per thread; the band up to MAX_DELTA = 7 on one state per thread (narrow), on
    two with a dense word in the second pass (thick) and on four (pass4): xi[p][o] for every p and o"""
    d = devices(name, stream0=True)
    r = d.run(tier, delta)
    check_against(d, r, restated(d, r, delta), f"{name} tier {tier} delta {delta}")
    for k in EC.present(d.case):
        na = r["stats"][k][0]["num_a"]
        i, j = np.indices(na.shape)
        assert not np.any(na[(j < i) | (j > i + delta)]), "num_a outside the band"


@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["broad", "broad256"])
def test_the_table_columns_after_a_call_that_filled_them(G, ctx, devices, name, tier):
    """tie_gamma's table loop and tie_out on a workspace that is not fresh: first the same vocabulary under
    transcripts that speak a word past the registers' end which the case leaves out, then the case.  That
    word's gamma columns are exactly 0 and its vector is all zero but for the common tail; the rest is the
    restatement's.  (On a fresh buffer a skipped loop leaves the zeros that are asked for.)"""
    d = devices(name, stream0=True)
    case = d.case
    nt = EC.launch_shape(case)["threads"]
    held = EC.present(case)
    late = next(k for k in range(case.K) if k not in held and case.bo[k] >= 4 * nt)
    early = next(k for k in range(case.K) if k not in held)
    # (three states a word: nine frames and more take three words, fewer take the late word alone, too short or not)
    other = [() if T == 0 else (late, early, late) if T >= 9 else (late,) for T in case.lens]
    cols = slice(case.bo[late], case.bo[late + 1])
    with tier_of(G, ctx, tier):
        d.call(other)
        stale = ctx.fetch(G.BUF_GAMMA, (d.F, d.NS))
        assert np.all(stale[:, cols].sum(0) > 0), "the first call left nothing in the columns"
        assert np.any(d.st[late][0].download()[:-2])
        d.call()
        r = d.fetch_all()
    assert not np.any(r["gamma"][:, cols])
    assert not np.any(r["v"][late][0][:-2]) and same(r["v"][late][0][-2:], r["v"][held[0]][0][-2:])
    check_against(d, r, restated(d, r), f"{name} tier {tier} after other transcripts")


@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["pass8", "pass4", "deep", "mid"])
def test_every_frames_gamma_sums_to_rho(G, ctx, devices, name, tier):
    """the identity test_lattice_at_the_cap uses, with log Z from the long-double restatement (the device's is
    not fetched): every frame's gamma sum is exp(log P - log Z).  A log Z summed over the wrong lanes (a last
    word of 17 or 64 states) or a state's gamma lost in a later pass shifts it"""
    d = devices(name, stream0=True)
    r = d.run(tier)
    ref = restated(d, r)
    off = offsets(d.case.lens)
    seen = 0
    for u in range(d.U):
        if d.case.lens[u] == 0 or not np.isfinite(float(ref["loglik"][u])):
            continue
        rho = float(np.exp(ref["loglik"][u] - ref["logZ"][u]))
        assert rho > 0
        sums = r["gamma"][off[u]:off[u + 1]].sum(1)
        assert np.all(np.abs(sums - rho) <= RTOL * rho), (name, u, float(np.abs(sums - rho).max() / rho))
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", EC.BIG)
def test_lattice_at_the_cap(G, ctx, devices, name, tier):
    """S = 2046 on 2200 frames, alone and among small utterances: log P, every frame's gamma sum against
    exp(log P - log Z) and den_c against the float64 restatement on the device's log b"""
    d = devices(name)
    r = d.run(tier)
    ref = restated(d, r, ft=np.float64)
    assert E.block_dist(r["ll"], ref["loglik"]) <= RTOL
    off = offsets(d.case.lens)
    for u in range(d.U):
        T = int(d.case.lens[u])
        if T == 0:
            continue
        rho = float(np.exp(ref["loglik"][u] - ref["logZ"][u]))
        assert rho > 0
        sums = r["gamma"][off[u]:off[u + 1]].sum(1)
        assert np.all(np.abs(sums - rho) <= RTOL * rho), (name, u, float(np.abs(sums - rho).max() / rho))
    for k in EC.present(d.case):
        dist = E.block_dist(r["stats"][k][0]["den_c"], ref["stats"][k][0]["den_c"])
        assert dist <= RTOL, (name, k, dist)


# ------------------------------------------------------------- 2. the emission

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["narrow", "mixed", "many", "broad", "pass4", "deep"])
def test_log_b_is_the_alignments(G, ctx, devices, name, tier):
    d = devices(name)
    r = d.run(tier)
    with tier_of(G, ctx, tier):
        ctx.align_streams(d.dms, d.corpora, d.transcripts)
        assert same(r["logb"], ctx.fetch(G.BUF_B, (d.F, d.NS))), "log b is not ghmm_align_streams'"


# ------------------------------------------------------------- 3. identities, bit for bit

@pytest.mark.parametrize("name", ["lane_6x2x9_banded", "lane_9x2x5_dense", "lane_40x1x13_banded", "p2_6_banded"])
def test_one_word_is_estep_log_streams_bit_for_bit(G, ctx, name):
    """consequence (a): one word, one-word transcripts, GHMM_OPT_KERNELS = 1"""
    case = E.make(G, name)
    hms = case.words[0]
    dms = [ctx.model(h) for h in hms]
    corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
    one = [ctx.stats(h.N, h.M, h.D) for h in hms]
    emb = [ctx.stats(h.N, h.M, h.D) for h in hms]
    F, N, U = case.F, hms[0].N, case.U
    try:
        with tier_of(G, ctx, 1):
            ctx.estep_log_streams(dms, corpora, one)
            want = [s.download() for s in one] + [ctx.fetch(b, sh) for b, sh in
                                                  ((G.BUF_GAMMA, (F, N)), (G.BUF_LOGLIK, (U,)), (G.BUF_B, (F, N)))]
            ctx.estep_embed_streams([dms], corpora, [(0,) if T else () for T in case.lens], [emb])
            got = [s.download() for s in emb] + [ctx.fetch(b, sh) for b, sh in
                                                 ((G.BUF_GAMMA, (F, N)), (G.BUF_LOGLIK, (U,)), (G.BUF_B, (F, N)))]
        for what, a, b in zip(["stats"] * len(hms) + ["gamma", "loglik", "log b"], got, want):
            assert same(a, b), f"{name}: {what} is not ghmm_estep_log_streams'"
    finally:
        for o in dms + corpora + one + emb:
            o.close()


def test_repeats_and_nothing_stale(G, ctx, devices):
    """GHMM_OPT_KERNELS = 1: a second identical call, and the same call after a connect_streams on another
    vocabulary, repeat every byte; loglik and n_utt are equal in every vector and Stats.loglik() returns them"""
    d, o = devices("mixed"), devices("narrow")
    with tier_of(G, ctx, 1):
        d.call()
        first = d.fetch_all()
        d.call()
        second = d.fetch_all()
        ctx.connect_streams(o.dms, o.corpora, -5.0)
        o.call()
        d.call()
        third = d.fetch_all()
        mail = [[s.loglik() for s in w] for w in d.st]
    for other in (second, third):
        assert all(same(a, b) for va, vb in zip(first["v"], other["v"]) for a, b in zip(va, vb))
        assert all(same(first[x], other[x]) for x in ("logb", "gamma", "ll"))
    tail = first["v"][0][0][-2:]
    assert tail[1] == d.U and not np.isnan(tail[0])
    for vw, mw in zip(first["v"], mail):
        for v, m in zip(vw, mw):
            assert same(v[-2:], tail)
            assert same(np.asarray(m, dtype=np.float64), tail), "Stats.loglik() is not the vector's"


def test_loglik_through_the_mailbox_after_an_estep_on_the_same_vector(G, ctx, devices):
    """a vector that k_reduce_all has just filled (its mailbox is valid) and the embedded call then overwrites:
    Stats.loglik() must return the embedded call's numbers (ones: every log P is finite)"""
    d = devices("ones")
    with tier_of(G, ctx, 1):
        ctx.estep_log_streams(d.dms[0], d.corpora, d.st[0])
        stale = d.st[0][0].loglik()
        d.call()
        got = np.asarray(d.st[0][0].loglik(), dtype=np.float64)
        v = d.st[0][0].download()
    assert same(got, v[-2:])
    assert np.isfinite(got[0]) and np.isfinite(stale[0]) and got[0] != stale[0]


# ------------------------------------------------------------- 4. consequences to rounding

@pytest.mark.parametrize("tier", TIERS)
def test_one_word_transcripts_give_each_word_its_sub_corpus(G, ctx, devices, tier):
    """consequence (b) on narrow's three streams: word k against estep_log_streams on its utterances"""
    d = devices("narrow")
    case = d.case
    spoken = [0, 1, 2, 0, 1, 2, 0, 1, 2]
    transcripts = [(k,) if T else () for k, T in zip(spoken, case.lens)]
    off = offsets(case.lens)
    with tier_of(G, ctx, tier):
        d.call(transcripts)
        got = d.split(d.vectors())
        for k in range(d.K):
            us = [u for u in range(d.U) if transcripts[u] == (k,)]
            fr = np.concatenate([np.arange(off[u], off[u + 1]) for u in us]).astype(int)
            lens = np.asarray([case.lens[u] for u in us], dtype=np.int32)
            corpora = [ctx.corpus(X[fr], lens) for X in case.Xs]
            st = [ctx.stats(h.N, h.M, h.D) for h in case.words[k]]
            try:
                ctx.estep_log_streams(d.dms[k], corpora, st)
                for p, (s, h) in enumerate(zip(st, case.words[k])):
                    want = G.split_stats(s.download(), h.N, h.M, h.D)
                    for b in BLOCKS:
                        dist = E.block_dist(got[k][p][b], want[b])
                        assert dist <= RTOL, (tier, k, p, b, dist)
            finally:
                for o in corpora + st:
                    o.close()


@pytest.mark.parametrize("tier", TIERS)
def test_a_repeated_word_is_the_sum_of_two_copies(G, ctx, devices, tier):
    """consequence (c): narrow's transcript (0, 0) against a vocabulary with word 0 duplicated and (0, K)"""
    d = devices("narrow")
    case = d.case
    assert (0, 0) in d.transcripts
    two = [(0, d.K) if t == (0, 0) else t for t in d.transcripts]
    copy = [ctx.model(h) for h in case.words[0]]
    st = [ctx.stats(h.N, h.M, h.D) for h in case.words[0]]
    try:
        with tier_of(G, ctx, tier):
            d.call()
            one = d.split(d.vectors())
            ctx.estep_embed_streams(d.dms + [copy], d.corpora, two, d.st + [st])
            both = d.split(d.vectors())
            dup = [G.split_stats(s.download(), h.N, h.M, h.D) for s, h in zip(st, case.words[0])]
        for p in range(d.P):
            for b in BLOCKS:
                dist = E.block_dist(one[0][p][b], both[0][p][b] + dup[p][b])
                assert dist <= RTOL, (tier, p, b, dist)
                assert np.any(dup[p][b]), "the copy received nothing"
                for k in range(1, d.K):
                    assert E.block_dist(one[k][p][b], both[k][p][b]) <= RTOL
    finally:
        for o in copy + st:
            o.close()


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["many", "short"])
def test_rows_of_num_a_sum_to_den_a(G, ctx, devices, name, tier):
    """banded words at delta 1, the last states of non-final instances included"""
    d = devices(name)
    r = d.run(tier)
    seen = 0
    for k in EC.present(d.case):
        A = np.asarray(d.case.words[k][0].A)
        i, j = np.indices(A.shape)
        if np.any((A > 0) & ((j < i) | (j > i + 1))):
            continue
        st = r["stats"][k][0]
        dist = E.block_dist(st["num_a"].sum(1), st["den_a"])
        assert dist <= RTOL, (name, k, dist)
        seen += bool(np.any(st["den_a"]))
    assert seen >= 2
    inner = [k for t in d.transcripts for k in t[:-1]]
    assert inner, "no non-final instance"


# ------------------------------------------------------------- 5. the point

POINT_NS, POINT_SHAPES = (3, 5, 4, 3, 4), ((2, 4), (1, 3))
POINT_UTTS = [((0, 1), (7, 12)), ((2, 0, 3), (9, 8, 7)), ((1, 1), (11, 12)), ((3, 2), (8, 10)), ((0,), (9,)),
              ((2, 3, 0, 1), (9, 7, 8, 12)), ((1, 0), (12, 6))]          # word 4 is in no transcript


def point_case(G):
    """a connected corpus built as align_cases builds its utterances, a far frame in every utterance, and the
    models the training starts from: the truth with every mean moved"""
    rng = np.random.default_rng(2024)
    truth = [[V.rand_model(G, rng, N, M, D, banded(rng, N), spread=2.0, word=f"w{k}") for M, D in POINT_SHAPES]
             for k, N in enumerate(POINT_NS)]
    parts, lens, transcripts = [[] for _ in POINT_SHAPES], [], []
    for seq, seg in POINT_UTTS:
        for k, T in zip(seq, seg):
            x = stream_frames(rng, truth[k], [int(T)])
            for p in range(len(POINT_SHAPES)):
                parts[p].append(x[p])
        lens.append(int(sum(seg)))
        transcripts.append(tuple(seq))
    Xs = [np.concatenate(x) for x in parts]
    off = offsets(lens)
    for X in Xs:
        X[off[:-1] + 2] += LC.FAR
    start = [[G.HostModel(h.A, h.c, h.mean + rng.normal(0.0, 0.15, h.mean.shape), h.inv_var, h.det, word=h.word)
              for h in w] for w in truth]
    return start, Xs, np.asarray(lens, dtype=np.int32), transcripts


@pytest.mark.parametrize("tier", TIERS)
def test_four_embedded_em_iterations_track_the_restatement(G, ctx, tier):
    """embed.embedded_em against the float64 restatement driven with oracle_lib.mstep: the log-likelihood trace
    and the last models at RTOL; the absent word's model is unchanged, bit for bit"""
    embed = load_pkg().embed
    start, Xs, lens, transcripts = point_case(G)
    held = EC.present(None, transcripts)
    assert 4 not in held
    ref, trace = [[h.copy() for h in w] for w in start], []
    for _ in range(4):
        e = EC.estep(ref, Xs, lens, transcripts, ft=np.float64)
        trace.append(float(e["loglik"].sum()))
        for k in held:
            ref[k] = [O.mstep(h, np.asarray(E.vector(st), dtype=np.float64)) for h, st in zip(ref[k], e["stats"][k])]
    assert np.all(np.isfinite(trace)) and trace[-1] > trace[0]
    vocab = [[ctx.model(h) for h in w] for w in start]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    seen = []
    try:
        with tier_of(G, ctx, tier):
            got = embed.embedded_em(ctx, vocab, corpora, transcripts, 4, on_iteration=lambda it, ll: seen.append((it, ll)))
            new = [[m.get() for m in w] for w in vocab]
    finally:
        for o in [m for w in vocab for m in w] + corpora:
            o.close()
    assert [ll for _, ll in seen] == got and [it for it, _ in seen] == [0, 1, 2, 3]
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(got, trace))
    e_model = 0.0
    for k in held:
        for a, b in zip(new[k], ref[k]):
            assert all(np.all(np.isfinite(x)) for x in a.arrays())
            e_model = max([e_model] + [E.block_dist(x, y) for x, y in zip(a.arrays(), b.arrays())])
    print(f"tier {tier}: trace {got}, trace error {e_tr:.1e}, model error {e_model:.1e}")
    assert e_tr <= RTOL and e_model <= RTOL
    for a, b in zip(new[4], start[4]):
        assert all(same(x, np.asarray(y, dtype=np.float64)) for x, y in zip(a.arrays(), b.arrays())), "the absent word changed"


# ------------------------------------------------------------- 6. the contract

def raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, stats, drop=None):
    ip = G.C.POINTER(G.C.c_int32)
    keep = (np.asarray(list(seq) + [0], dtype=np.int32), np.asarray(seq_off, dtype=np.int32))
    args = [a.ctypes.data_as(ip) for a in keep] + [stats]
    if drop is not None:
        args[drop] = None
    return ctx.lib.ghmm_estep_embed_streams(ctx.h, vocab, K, corpora, P, *args)


def test_refusals_write_nothing(G, ctx, devices):
    d = devices("mixed")
    case = d.case
    K, P, U = d.K, d.P, d.U
    flat = [m for w in d.dms for m in w]
    flat_st = [s for w in d.st for s in w]
    vocab, corpora, stats = handles(G, flat), handles(G, d.corpora), handles(G, flat_st)
    arg, unsupported = G.ERR_ARG, G.ERR_UNSUPPORTED
    seq, seq_off = flat_transcripts(d.transcripts)
    with_frames = int(np.nonzero(case.lens > 0)[0][0])
    h = case.words[0]
    rng = np.random.default_rng(3)
    w64, w65 = ([ctx.model(V.rand_model(G, rng, N, x.M, x.D, banded(rng, N))) for x in h] for N in (64, 65))
    s64, s65 = ([ctx.stats(N, x.M, x.D) for x in h] for N in (64, 65))
    full = ctx.stats_full(h[0].N, h[0].M, h[0].D)
    other = ctx.stats(h[0].N, h[0].M + 1, h[0].D)
    extra = w64 + w65 + s64 + s65 + [full, other]
    with tier_of(G, ctx, 1):
        d.call()
        before = d.fetch_all()
        ctx.set_option(G.OPT_TIMING, 1)
        ctx.kernel_times_reset()
        try:
            for drop in range(3):
                assert raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, stats, drop=drop) == arg, ("null", drop)
            for bad in (None, full, other):
                st = handles(G, [bad] + flat_st[1:])
                assert raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, st) == arg, "a null, full or other vector"
            assert raw_call(G, ctx, vocab, K, corpora, P, seq, [1] + seq_off[1:], stats) == arg, "seq_off[0] != 0"
            down = list(seq_off)
            down[U - 1] = down[U] + 1
            assert raw_call(G, ctx, vocab, K, corpora, P, seq + [0, 0], down, stats) == arg, "a decreasing seq_off"
            for bad in (K, -1, 1 << 20):
                assert raw_call(G, ctx, vocab, K, corpora, P, seq[:-1] + [bad], seq_off, stats) == arg, ("word", bad)
            empty = [() if u == with_frames else t for u, t in enumerate(d.transcripts)]
            assert raw_call(G, ctx, vocab, K, corpora, P, *flat_transcripts(empty), stats) == arg, "an empty transcript"
            assert raw_call(G, ctx, None, K, corpora, P, seq, seq_off, stats) == arg
            assert raw_call(G, ctx, vocab, 0, corpora, P, seq, seq_off, stats) == arg
            ones = [(0,)] * U
            assert raw_call(G, ctx, handles(G, flat[:P] + w65), 2, corpora, P, *flat_transcripts(ones),
                            handles(G, flat_st[:P] + s65)) == unsupported, "65 states"
            long = [(1,) * 33 if u == with_frames else (0,) for u in range(U)]
            assert raw_call(G, ctx, handles(G, flat[:P] + w64), 2, corpora, P, *flat_transcripts(long),
                            handles(G, flat_st[:P] + s64)) == unsupported, "S_u above the cap"
            assert "2048" in ctx.lib.ghmm_last_error().decode()
            ctx.set_option(G.OPT_ROBUST, 1)
            try:
                assert raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, stats) == unsupported, "robust"
            finally:
                ctx.set_option(G.OPT_ROBUST, 0)
            assert not any(n for k, (_, n) in ctx.kernel_times().items()), "a refusal launched something"
        finally:
            ctx.set_option(G.OPT_TIMING, 0)
        after = d.fetch_all()
        assert all(same(a, b) for va, vb in zip(before["v"], after["v"]) for a, b in zip(va, vb))
        assert all(same(before[x], after[x]) for x in ("logb", "gamma", "ll"))
        assert not np.any(s64[0].download()) and not np.any(s65[0].download())
        # the longest transcript that fits is taken: 32 times the word of 64 states (too short: log P = -inf)
        fits = [(1,) * 32 if u == with_frames else (0,) for u in range(U)]
        assert raw_call(G, ctx, handles(G, flat[:P] + w64), 2, corpora, P, *flat_transcripts(fits),
                        handles(G, flat_st[:P] + s64)) == G.OK
        assert ctx.fetch(G.BUF_LOGLIK, (U,))[with_frames] == -np.inf
    for o in extra:
        o.close()


def test_no_utterance_gives_all_zero_vectors(G, ctx, devices):
    d = devices("mixed")
    none = [ctx.corpus(np.zeros((0, x.D)), np.zeros(0, dtype=np.int32)) for x in d.case.words[0]]
    try:
        d.call()
        assert np.any(d.st[0][0].download())
        ctx.estep_embed_streams(d.dms, none, [], d.st)
        assert not any(np.any(v) for w in d.vectors() for v in w)
        assert [float(x) for x in d.st[0][0].loglik()] == [0.0, 0.0]
    finally:
        for c in none:
            c.close()
        d._run.clear()


@pytest.mark.parametrize("name", ["narrow", "many", "broad", "pass4", "deep"])
def test_launch_counts_and_the_workspace_afterwards(G, ctx, devices, name):
    """2 P - 1 launches under GHMM_K_EMISSION, two under GHMM_K_FORWARD, per stream ghmm_estep's statistics
    launches (vector tier: one k_mixstats, one k_reduce_all) and the scatter under GHMM_K_REDUCE"""
    d = devices(name)
    P = d.P
    with tier_of(G, ctx, 1):
        kt = timed(G, ctx, d.call)
        assert kt == {"emission": 2 * P - 1, "forward": 2, "mixstats": P, "reduce": 2 * P}
        for buf in (G.BUF_ALPHA, G.BUF_BETA, G.BUF_SCALE):
            assert code(G, lambda: ctx.fetch(buf, (1,))) == G.ERR_ARG
        if P == 1:
            ctx.fetch(G.BUF_POST, (d.F, d.NS * d.case.words[0][0].M))
        else:
            assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
        # the row API does not reuse the workspace
        assert code(G, lambda: ctx.forward(d.dms[0][0], d.corpora[0])) == G.ERR_ARG
        # and an E-step of another kind afterwards serves its own alpha again
        ctx.estep_log_streams(d.dms[0], d.corpora, d.st[0])
        ctx.fetch(G.BUF_ALPHA, (d.F, d.case.Ns[0]))
    d._run.clear()
