"""The embedded Baum-Welch E-step on full-covariance words on the GPU: ghmm_estep_embed_full_streams (the
vocabulary's emission launches with log b and posteriors, k_embed_fwd / k_embed_bwd over the transcripts' word
instances, ghmm_estep_full's statistics launches on the concatenated vocabulary, k_embed_scatter_full) and
embed.embedded_em on full-covariance vocabularies — GPU box only.  The cases and the restatement are
embed_full_cases.py's; test_embed_full_host.py shows on the CPU that they hold what is leaned on here.

  lattice      every case against the long-double restatement on the run's own log b and posteriors, per word
               and stream with estep_log_ref.block_dist at RTOL and equal zero, -inf and NaN patterns: log P, the
               tied gamma, num_a, den_a, den_c, num_c, num_mu, num_cov.  The library serves the posteriors of one
               stream only, so a case of several streams runs twice: its first stream alone on its own log b and
               posteriors, and all its streams on their own log b and the restated posteriors.
  emission     BUF_B bit for bit what ghmm_align_full_streams leaves
  identities   bit for bit: consequence (a) with one and two streams, a second call, mix after deep and deep after
               mix
  to rounding  consequences (b) and (c)
  the point    embedded_em for four iterations against the float64 restatement driven with ghmm_mstep_full_host,
               with mstep_full_dev and with mstep_full
  the contract refusals write nothing, U = 0, the launch counts, what ghmm_fetch serves afterwards, and the
               diagonal call's refusal of full-covariance vectors"""
import numpy as np
import pytest

import align_cases as AC
import embed_cases as EC
import embed_full_cases as FC
import estep_log_ref as E
from _load import load_pkg
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import RTOL, code, extended, offsets, rand_fmodel
from test_align_gpu import flat_transcripts, handles
from test_logscore_gpu import same, timed

pytestmark = pytest.mark.gpu


class Device:
    """a case's device vocabulary, corpora and per-word statistics vectors"""

    def __init__(self, G, ctx, case, transcripts=None):
        self.G, self.ctx, self.case = G, ctx, case
        self.transcripts = list(case.transcripts if transcripts is None else transcripts)
        self.K, self.P, self.F, self.U, self.NS = case.K, case.P, case.F, case.U, case.NS
        self.dms = [[ctx.full_model(h) for h in w] for w in case.words]
        self._models = [m for w in self.dms for m in w]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self.st = [[ctx.stats_full(h.N, h.M, h.D) for h in w] for w in case.words]
        self._run = {}

    def call(self, transcripts=None):
        self.ctx.estep_embed_full_streams(self.dms, self.corpora,
                                          self.transcripts if transcripts is None else transcripts, self.st)

    def vectors(self):
        return [[s.download() for s in w] for w in self.st]

    def split(self, v):
        return [[self.G.split_stats_full(x, h.N, h.M, h.D) for x, h in zip(vw, w)]
                for vw, w in zip(v, self.case.words)]

    def fetch_all(self):
        G, ctx = self.G, self.ctx
        r = {"v": self.vectors()}
        r["stats"] = self.split(r["v"])
        r["logb"] = ctx.fetch(G.BUF_B, (self.F, self.NS))
        r["gamma"] = ctx.fetch(G.BUF_GAMMA, (self.F, self.NS))
        r["ll"] = ctx.fetch(G.BUF_LOGLIK, (self.U,))
        r["posts"] = [ctx.fetch(G.BUF_POST, (self.F, self.NS * self.case.words[0][0].M))] if self.P == 1 else None
        return r

    def run(self, delta=1, transcripts=None):
        key = (delta, None if transcripts is None else tuple(transcripts))
        if key not in self._run:
            self.ctx.set_option(self.G.OPT_DELTA, delta)
            try:
                self.call(transcripts)
                self._run[key] = self.fetch_all()
            finally:
                self.ctx.set_option(self.G.OPT_DELTA, 1)
        return self._run[key]

    def close(self):
        for o in self._models + self.corpora + [s for w in self.st for s in w]:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name, stream0=False):
        if (name, stream0) not in made:
            case = FC.make(G, name)
            if stream0 and case.P > 1:
                one = case.stream0()
                one.transcripts, one.name = case.transcripts, case.name
                case = one
            made[name, stream0] = Device(G, ctx, case)
        return made[name, stream0]
    yield get
    for d in made.values():
        d.close()


def restated(d, r, delta=1, transcripts=None, ft=np.longdouble):
    """the restatement on a run's own log b and (one stream) posteriors, computed once per run and left unchanged"""
    key = ("restated", ft)
    if key not in r:
        r[key] = FC.estep(d.case.words, d.case.Xs, d.case.lens, d.transcripts if transcripts is None else transcripts,
                          delta, ft, logb=r["logb"], posts=r["posts"])
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
            for b in FC.BLOCKS:
                w64 = np.asarray(want[b], dtype=np.float64)
                assert np.array_equal(np.asarray(got[b]) == 0.0, w64 == 0.0), f"{what}: zeros of {b} of word {k} differ"
                dist = E.block_dist(got[b], want[b])
                assert dist <= RTOL, (what, k, p, b, dist)
                worst = max(worst, dist)
    return worst


def check_absent(d, r, transcripts=None):
    """a word no transcript holds: all-zero sums, the common loglik and n_utt, gamma columns of 0"""
    held = FC.present(d.case, transcripts)
    for k in (k for k in range(d.K) if k not in held):
        for p in range(d.P):
            assert not np.any(r["v"][k][p][:-2]) and same(r["v"][k][p][-2:], r["v"][held[0]][0][-2:])
        assert not np.any(r["gamma"][:, d.case.bo[k]:d.case.bo[k + 1]])
    return held


# ------------------------------------------------------------- 1. the lattice

@extended
@pytest.mark.parametrize("name,stream0", [("full", True), ("full", False), ("mix", True), ("mix", False),
                                          ("short", True), ("short", False), ("deep", False), ("deep200", False)])
def test_lattice_against_the_long_double_restatement(G, ctx, devices, name, stream0):
    """deep: without reduce_grid in run_fullstats the blocks of k_reduce_all past 2^32 / 1024 never run, and
    most of num_a, den_a, den_c and the tail stay what the buffer held"""
    d = devices(name, stream0)
    r = d.run()
    worst = check_against(d, r, restated(d, r), f"{name} P = {d.P}")
    print(f"{name} P = {d.P}: worst distance from the long-double restatement {worst:.2e}")
    held = check_absent(d, r)
    assert len(held) < d.K or name == "full"
    tail = r["v"][held[0]][0][-2:]
    assert tail[1] == d.U and all(same(v[-2:], tail) for w in r["v"] for v in w)


@extended
@pytest.mark.parametrize("which", sorted(AC.HOLES))
def test_lattice_on_nan_and_minus_inf_columns(G, ctx, devices, which):
    """holes under align_cases.HOLES' transcripts: equal NaN / -inf / zero patterns and RTOL on the rest"""
    d = devices("holes")
    transcripts, kinds = AC.HOLES[which]
    r = d.run(transcripts=transcripts)
    ref = restated(d, r, transcripts=transcripts)
    worst = check_against(d, r, ref, f"holes {which}")
    print(f"holes {which}: worst distance from the long-double restatement {worst:.2e}")
    # (the sum over paths takes a NaN that the best path passes over: only the finite and the empty kinds carry over)
    for u, kind in enumerate(kinds):
        if kind in ("finite", "0"):
            assert np.isfinite(r["ll"][u]) and (kind == "finite" or r["ll"][u] == 0.0), (which, u, r["ll"][u])
    assert which != "spoken" or (np.isnan(r["ll"][2]) and np.any(np.isnan(r["v"][0][0])))


@extended
@pytest.mark.parametrize("stream0", (True, False))
@pytest.mark.parametrize("delta", FC.DELTAS)
def test_lattice_under_other_deltas(G, ctx, devices, delta, stream0):
    d = devices("mix", stream0)
    r = d.run(delta)
    check_against(d, r, restated(d, r, delta), f"mix P = {d.P} delta {delta}")
    for k in FC.present(d.case):
        na = r["stats"][k][0]["num_a"]
        i, j = np.indices(na.shape)
        assert not np.any(na[(j < i) | (j > i + delta)]), "num_a outside the band"


# ------------------------------------------------------------- 2. the emission

@pytest.mark.parametrize("name", ["full", "mix", "deep", "deep200", "holes"])
def test_log_b_is_the_alignments(G, ctx, devices, name):
    d = devices(name)
    r = d.run()
    ctx.align_full_streams(d.dms, d.corpora, d.transcripts)
    assert same(r["logb"], ctx.fetch(G.BUF_B, (d.F, d.NS))), "log b is not ghmm_align_full_streams'"
    d._run.clear()      # (the workspace is the alignment's now: a later run fetches its own)


# ------------------------------------------------------------- 3. identities, bit for bit

@pytest.mark.parametrize("word,streams", [(0, 1), (1, 1), (0, 2), (1, 2), (3, 2)])
def test_one_word_is_estep_full_streams_bit_for_bit(G, ctx, word, streams):
    """consequence (a): one word of mix (banded, ergodic, of one state), one-word transcripts"""
    case = FC.make(G, "mix")
    hms = case.words[word][:streams]
    dms = [ctx.full_model(h) for h in hms]
    corpora = [ctx.corpus(X, case.lens) for X in case.Xs[:streams]]
    one = [ctx.stats_full(h.N, h.M, h.D) for h in hms]
    emb = [ctx.stats_full(h.N, h.M, h.D) for h in hms]
    F, N, U = case.F, hms[0].N, case.U
    bufs = [(G.BUF_GAMMA, (F, N)), (G.BUF_LOGLIK, (U,)), (G.BUF_B, (F, N))]
    if streams == 1:
        bufs.append((G.BUF_POST, (F, N * hms[0].M)))
    try:
        ctx.estep_full_streams(dms, corpora, one, log=True)
        want = [s.download() for s in one] + [ctx.fetch(b, sh) for b, sh in bufs]
        ctx.estep_embed_full_streams([dms], corpora, [(0,) if T else () for T in case.lens], [emb])
        got = [s.download() for s in emb] + [ctx.fetch(b, sh) for b, sh in bufs]
        for what, a, b in zip(["stats"] * streams + ["gamma", "loglik", "log b", "post"], got, want):
            assert same(a, b), f"word {word}, {streams} streams: {what} is not ghmm_estep_full_streams'"
        assert np.any(got[0][:-2])
    finally:
        for o in dms + corpora + one + emb:
            o.close()


def test_repeats_and_nothing_stale(G, ctx, devices):
    """a second identical call repeats every byte; mix after deep and deep after mix leave nothing stale; loglik
    and n_utt are equal in every vector and Stats.loglik() returns them"""
    d, o = devices("mix"), devices("deep")
    d._run.clear()
    o._run.clear()
    d.call()
    first = d.fetch_all()
    d.call()
    second = d.fetch_all()
    o.call()
    deep_first = o.fetch_all()
    d.call()
    third = d.fetch_all()
    mail = [[s.loglik() for s in w] for w in d.st]
    o.call()
    deep_second = o.fetch_all()
    for a, others in ((first, (second, third)), (deep_first, (deep_second,))):
        for other in others:
            assert all(same(x, y) for va, vb in zip(a["v"], other["v"]) for x, y in zip(va, vb))
            assert all(same(a[x], other[x]) for x in ("logb", "gamma", "ll"))
    tail = first["v"][0][0][-2:]
    assert tail[1] == d.U and not np.isnan(tail[0])
    for vw, mw in zip(first["v"], mail):
        for v, m in zip(vw, mw):
            assert same(v[-2:], tail)
            assert same(np.asarray(m, dtype=np.float64), tail), "Stats.loglik() is not the vector's"


# ------------------------------------------------------------- 4. consequences to rounding

def test_one_word_transcripts_give_each_word_its_sub_corpus(G, ctx, devices):
    """consequence (b) on mix's two streams: word k against estep_full_streams(log) on its utterances"""
    d = devices("mix")
    case = d.case
    spoken = [0, 3, 0, 2, 1, 2, 1, 0]
    transcripts = [(k,) if T else () for k, T in zip(spoken, case.lens)]
    off = offsets(case.lens)
    d.call(transcripts)
    got = d.split(d.vectors())
    d._run.clear()
    for k in sorted(set(spoken)):
        us = [u for u in range(d.U) if transcripts[u] == (k,)]
        fr = np.concatenate([np.arange(off[u], off[u + 1]) for u in us]).astype(int)
        lens = np.asarray([case.lens[u] for u in us], dtype=np.int32)
        corpora = [ctx.corpus(X[fr], lens) for X in case.Xs]
        st = [ctx.stats_full(h.N, h.M, h.D) for h in case.words[k]]
        try:
            ctx.estep_full_streams(d.dms[k], corpora, st, log=True)
            for p, (s, h) in enumerate(zip(st, case.words[k])):
                want = G.split_stats_full(s.download(), h.N, h.M, h.D)
                for b in FC.SUMS:
                    dist = E.block_dist(got[k][p][b], want[b])
                    assert dist <= RTOL, (k, p, b, dist)
        finally:
            for o in corpora + st:
                o.close()


def test_a_repeated_word_is_the_sum_of_two_copies(G, ctx, devices):
    """consequence (c): mix's transcript (0, 0) against a vocabulary with word 0 duplicated and (0, K)"""
    d = devices("mix")
    case = d.case
    assert (0, 0) in d.transcripts
    two = [(0, d.K) if t == (0, 0) else t for t in d.transcripts]
    copy = [ctx.full_model(h) for h in case.words[0]]
    st = [ctx.stats_full(h.N, h.M, h.D) for h in case.words[0]]
    try:
        d.call()
        one = d.split(d.vectors())
        ctx.estep_embed_full_streams(d.dms + [copy], d.corpora, two, d.st + [st])
        both = d.split(d.vectors())
        dup = [G.split_stats_full(s.download(), h.N, h.M, h.D) for s, h in zip(st, case.words[0])]
        d._run.clear()
        for p in range(d.P):
            for b in FC.SUMS:
                dist = E.block_dist(one[0][p][b], both[0][p][b] + dup[p][b])
                assert dist <= RTOL, (p, b, dist)
                assert np.any(dup[p][b]), "the copy received nothing"
                for k in range(1, d.K):
                    assert E.block_dist(one[k][p][b], both[k][p][b]) <= RTOL
    finally:
        for o in copy + st:
            o.close()


# ------------------------------------------------------------- 5. the point

@pytest.fixture(scope="module")
def point(G):
    """the point case and its float64 trajectory, computed once"""
    start, Xs, lens, transcripts = FC.point_case(G)
    return start, Xs, lens, transcripts, FC.em_trajectory(start, Xs, lens, transcripts, ft=np.float64)


@pytest.mark.parametrize("mstep", ("mstep_full_dev", "mstep_full"))
def test_four_embedded_em_iterations_track_the_restatement(G, ctx, point, mstep):
    """embed.embedded_em against the float64 restatement driven with ghmm_mstep_full_host: the log-likelihood
    trace (finite and rising) and the last models at embed_full_cases.em_bound(); the absent word's model is
    unchanged, bit for bit"""
    embed = load_pkg().embed
    start, Xs, lens, transcripts, (trace, ref) = point
    held = FC.present(None, transcripts)
    assert 4 not in held
    vocab = [[ctx.full_model(h) for h in w] for w in start]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    seen = []
    try:
        got = embed.embedded_em(ctx, vocab, corpora, transcripts, FC.POINT_ITERS,
                                on_iteration=lambda it, ll: seen.append((it, ll)), mstep_full=getattr(ctx, mstep))
        new = [[m.get() for m in w] for w in vocab]
    finally:
        for o in [m for w in vocab for m in w] + corpora:
            o.close()
    assert [ll for _, ll in seen] == got and [it for it, _ in seen] == list(range(FC.POINT_ITERS))
    assert np.all(np.isfinite(got)) and np.all(np.diff(got) > 0), got
    for k in held:
        assert all(np.all(np.isfinite(x)) for h in new[k] for x in h.arrays())
    e_tr, e_model = FC.trajectory_dist((got, new), (trace, ref), held)
    print(f"{mstep}: trace {got}, trace error {e_tr:.1e}, model error {e_model:.1e}, bound {FC.em_bound():.1e}")
    assert e_tr <= FC.em_bound() and e_model <= FC.em_bound()
    for a, b in zip(new[4], start[4]):
        assert all(same(x, np.asarray(y, dtype=np.float64)) for x, y in zip(a.arrays(), b.arrays())), "the absent word changed"


def test_embedded_em_picks_the_device_m_step_by_itself(G, ctx, point):
    """without mstep_full: M <= 256 takes mstep_full_dev, whose models are mstep_full's bit for bit, so one
    iteration equals the explicit one's"""
    embed = load_pkg().embed
    start, Xs, lens, transcripts, (trace, _) = point
    vocab = [[ctx.full_model(h) for h in w] for w in start]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    try:
        got = embed.embedded_em(ctx, vocab, corpora, transcripts, 2)
    finally:
        for o in [m for w in vocab for m in w] + corpora:
            o.close()
    assert max(abs(x - y) / abs(y) for x, y in zip(got, trace[:2])) <= FC.em_bound()


# ------------------------------------------------------------- 6. the contract

def raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, stats, drop=None, fn="ghmm_estep_embed_full_streams"):
    ip = G.C.POINTER(G.C.c_int32)
    keep = (np.asarray(list(seq) + [0], dtype=np.int32), np.asarray(seq_off, dtype=np.int32))
    args = [a.ctypes.data_as(ip) for a in keep] + [stats]
    if drop is not None:
        args[drop] = None
    return getattr(ctx.lib, fn)(ctx.h, vocab, K, corpora, P, *args)


def test_refusals_write_nothing(G, ctx, devices):
    d = devices("mix")
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
    w64 = [ctx.full_model(rand_fmodel(G, rng, 64, x.M, x.D, spread=1.0, asym=False)) for x in h]
    s64 = [ctx.stats_full(64, x.M, x.D) for x in h]
    diagonal = ctx.stats(h[0].N, h[0].M, h[0].D)
    other = ctx.stats_full(h[0].N, h[0].M + 1, h[0].D)
    extra = w64 + s64 + [diagonal, other]
    d._run.clear()
    d.call()
    before = d.fetch_all()
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    try:
        for drop in range(3):
            assert raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, stats, drop=drop) == arg, ("null", drop)
        for bad in (None, diagonal, other):
            st = handles(G, [bad] + flat_st[1:])
            assert raw_call(G, ctx, vocab, K, corpora, P, seq, seq_off, st) == arg, "a null, diagonal or other vector"
        assert raw_call(G, ctx, vocab, K, corpora, P, seq, [1] + seq_off[1:], stats) == arg, "seq_off[0] != 0"
        for bad in (K, -1, 1 << 20):
            assert raw_call(G, ctx, vocab, K, corpora, P, seq[:-1] + [bad], seq_off, stats) == arg, ("word", bad)
        empty = [() if u == with_frames else t for u, t in enumerate(d.transcripts)]
        assert raw_call(G, ctx, vocab, K, corpora, P, *flat_transcripts(empty), stats) == arg, "an empty transcript"
        assert "empty transcript" in ctx.lib.ghmm_last_error().decode()
        assert raw_call(G, ctx, None, K, corpora, P, seq, seq_off, stats) == arg
        assert raw_call(G, ctx, vocab, 0, corpora, P, seq, seq_off, stats) == arg
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
    assert not np.any(s64[0].download())
    # the longest transcript that fits is taken: 32 times the word of 64 states (too short: log P = -inf)
    fits = [(1,) * 32 if u == with_frames else (0,) for u in range(U)]
    assert raw_call(G, ctx, handles(G, flat[:P] + w64), 2, corpora, P, *flat_transcripts(fits),
                    handles(G, flat_st[:P] + s64)) == G.OK
    assert ctx.fetch(G.BUF_LOGLIK, (U,))[with_frames] == -np.inf
    d._run.clear()
    for o in extra:
        o.close()


def test_no_utterance_gives_all_zero_vectors_and_no_launch(G, ctx, devices):
    d = devices("mix")
    none = [ctx.corpus(np.zeros((0, x.D)), np.zeros(0, dtype=np.int32)) for x in d.case.words[0]]
    try:
        d.call()
        assert np.any(d.st[0][0].download())
        kt = timed(G, ctx, lambda: ctx.estep_embed_full_streams(d.dms, none, [], d.st))
        assert kt == {}, kt
        assert not any(np.any(v) for w in d.vectors() for v in w)
        assert [float(x) for x in d.st[0][0].loglik()] == [0.0, 0.0]
    finally:
        for c in none:
            c.close()
        d._run.clear()


@pytest.mark.parametrize("name,stream0", [("mix", False), ("mix", True), ("full", False), ("deep", False)])
def test_launch_counts_and_the_workspace_afterwards(G, ctx, devices, name, stream0):
    """per stream ONE launch under GHMM_K_EMISSION (the fold is its epilogue), two under GHMM_K_FORWARD, per
    stream one under GHMM_K_MIXSTATS and two brackets under GHMM_K_REDUCE: ghmm_estep_full's reductions
    (k_fullstats_reduce and k_reduce_all share one, as in every full-covariance E-step) and the scatter"""
    d = devices(name, stream0)
    P = d.P
    kt = timed(G, ctx, d.call)
    assert kt == {"emission": P, "forward": 2, "mixstats": P, "reduce": 2 * P}
    assert ctx.get_option(G.OPT_REFORDER_COUNT) == 0
    for buf in (G.BUF_ALPHA, G.BUF_BETA, G.BUF_SCALE):
        assert code(G, lambda: ctx.fetch(buf, (1,))) == G.ERR_ARG
    for buf, shape in ((G.BUF_B, (d.F, d.NS)), (G.BUF_GAMMA, (d.F, d.NS)), (G.BUF_LOGLIK, (d.U,))):
        ctx.fetch(buf, shape)
    if P == 1:
        ctx.fetch(G.BUF_POST, (d.F, d.NS * d.case.words[0][0].M))
    else:
        assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
    # and an E-step of another kind afterwards serves its own alpha again
    ctx.estep_full_streams(d.dms[0], d.corpora, d.st[0], log=True)
    ctx.fetch(G.BUF_ALPHA, (d.F, d.case.Ns[0]))
    d._run.clear()


def test_the_diagonal_call_still_refuses_full_covariance_vectors(G, ctx):
    case = EC.make(G, "ones")
    dms = [[ctx.model(h) for h in w] for w in case.words]
    corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
    full = [[ctx.stats_full(h.N, h.M, h.D) for h in w] for w in case.words]
    try:
        assert code(G, lambda: ctx.estep_embed_streams(dms, corpora, case.transcripts, full)) == G.ERR_ARG
        assert not any(np.any(s.download()) for w in full for s in w)
    finally:
        for o in [m for w in dms for m in w] + corpora + [s for w in full for s in w]:
            o.close()
