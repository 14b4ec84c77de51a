"""Connected-word decoding under a word-pair grammar on the GPU: ghmm_connect_grammar_streams and
ghmm_connect_grammar_full_streams (k_grammar) and the two recognisers' command lines with GHMM_GRAMMAR —
GPU box only.  The cases, the grammars and the float64 restatement of the definition are grammar_cases.py's;
test_grammar_host.py shows on the CPU that the restatement is the definition and that every (case, grammar)
pair compared here keeps the margin under which a path that differs cannot be blamed on rounding, in all
utterances but at most one.

The restatement runs on the log b fetched from the device (GHMM_BUF_B), so the emission's rounding is not
in the comparison: word, path and begin are compared exactly wherever the restatement's gap is above GAP,
the score to 1e-10 relative (test_connect_gpu.scores_close's bound for the same lattice arithmetic; what
remains is the device's log A against numpy's)."""
import os
import subprocess

import numpy as np
import pytest

import connect_cases as CC
import grammar_cases as GC
from _load import PKG_DIR
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import code, fmt, offsets
from streams_util import synth_case

pytestmark = pytest.mark.gpu

BIN = {False: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-fs"),
       True: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-full-fs")}
INF = np.inf
REL = 1e-10


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def scores_close(got, ref, rel=REL):
    """every score within `rel` of the reference, or the reference's non-finite value itself (a reference
    of 0, an utterance of no frames, is met exactly)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (got[~fin], ref[~fin])
    err = np.abs(got[fin] - ref[fin])
    print("worst relative score error", float((err / np.maximum(np.abs(ref[fin]), 1e-300)).max(initial=0.0)))
    assert np.all(err <= rel * np.abs(ref[fin])), float((err / np.maximum(np.abs(ref[fin]), 1e-300)).max())


class Device:
    """a case's device models (dms[k][p]) and corpora, and the calls of its model kind"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        self.full = case.name in GC.FULLCOV
        mk = ctx.full_model if self.full else ctx.model
        self.dms = [[mk(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]

    def grammar(self, start, pair, fin, dms=None, corpora=None):
        fn = self.ctx.connect_grammar_full_streams if self.full else self.ctx.connect_grammar_streams
        return fn(dms or self.dms, corpora or self.corpora, pair, start, fin)

    def connect(self, p):
        fn = self.ctx.connect_full_streams if self.full else self.ctx.connect_streams
        return fn(self.dms, self.corpora, p)

    def align(self, transcripts):
        fn = self.ctx.align_full_streams if self.full else self.ctx.align_streams
        return fn(self.dms, self.corpora, transcripts)

    def recognise(self):
        fn = self.ctx.recognise_full_streams if self.full else self.ctx.recognise_streams
        return fn(self.dms, self.corpora)

    def log_b(self):
        return self.ctx.fetch(self.G.BUF_B, (self.case.F, self.case.NS))

    def close(self):
        for o in [m for w in self.dms for m in w] + self.corpora:
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


class tier:
    """GHMM_OPT_KERNELS = t inside, the default again afterwards"""

    def __init__(self, G, ctx, t):
        self.G, self.ctx, self.t = G, ctx, t

    def __enter__(self):
        self.ctx.set_option(self.G.OPT_KERNELS, self.t)

    def __exit__(self, *exc):
        self.ctx.set_option(self.G.OPT_KERNELS, 0)


def check_shape_of_a_decoding(case, word, path, begin):
    """what holds of every decoding: the first frame begins a word; a frame that does not begin one
    continues the previous frame's word; a word begins in its first state, behind the last state of the
    word before it; the utterance ends in the last state of its last word"""
    off = offsets(case.lens)
    Ns = np.asarray(case.Ns)
    assert np.all((0 <= word) & (word < case.K)) and np.all((0 <= path) & (path < Ns[word]))
    assert set(np.unique(begin).tolist()) <= {0, 1}
    for u, T in enumerate(case.lens):
        if T == 0:
            continue
        w, s, b = (a[off[u]:off[u + 1]] for a in (word, path, begin))
        assert b[0] == 1, u
        cont = np.nonzero(b[1:] == 0)[0] + 1
        assert np.all(w[cont] == w[cont - 1]), u
        ent = np.nonzero(b[1:] == 1)[0] + 1
        assert np.all(s[ent] == 0) and np.all(s[ent - 1] == Ns[w[ent - 1]] - 1), u
        assert s[-1] == Ns[w[-1]] - 1, u


def against_the_restatement(d, which):
    """one call under the case's grammar `which` against the restatement on the device's log b; returns
    (word, begin, score, the restatement's gap)"""
    case = d.case
    g = GC.grammar(case, which)
    word, path, begin, score = d.grammar(*g)
    lb = d.log_b()
    rw, rp, rb, rs, gap = GC.decode(case, lb, *g)
    live = case.lens > 0
    print(case.name, which, "smallest gaps on the device's log b", np.sort(gap[live])[:2], "scores", score)
    assert np.sum(gap[live] <= GC.GAP) <= GC.MAX_BELOW_GAP, gap
    at = GC.compared(case, gap)
    assert same(word[at], rw[at]) and same(path[at], rp[at]) and same(begin[at], rb[at]), (case.name, which)
    scores_close(score, rs)
    check_shape_of_a_decoding(case, word, path, begin)
    assert np.all(score[~live] == 0.0) and not np.signbit(score[~live]).any()
    GC.allowed(case, word, begin, score, *g)           # (c)
    return word, begin, score, gap


# ------------------------------------------------------------- 1. against the restatement

@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", GC.SHAPES + ("ones",))
def test_against_the_restatement(G, ctx, devices, name, t):
    """narrow (one wave, P = 3, T = 0, 1 and 2), wide (a 64-state word across waves, dense columns), many
    (K = 70: more words than a wave has lanes; the table staged in LDS), thick (two states per thread),
    k256 (the cap on K, the table read from L2, predecessor words up to 255), cap (NS = 2048, more than
    48 KB of LDS beside the grammar), k100 (the table read from L2 in two slices per word, unrolled rounds
    and then a tail), k72 (the same from the staged table, 192 threads), ones (a word that is its own entry and end, no repeats allowed)"""
    d = devices(name)
    case = d.case
    with tier(G, ctx, t):
        for which in GC.GPU_GRAMMARS[name]:
            word, begin, score, gap = against_the_restatement(d, which)
            got = CC.strings(word, begin, case.lens)
            if which == "norepeat":
                fin = np.isfinite(score)
                assert all(w != k for s, f in zip(got, fin) if f for w, k in zip(s[:-1], s[1:])), got
            if name == "k256" and which == "norepeat":
                off = offsets(case.lens)
                first = np.zeros(case.F, dtype=bool)
                first[off[:-1][case.lens > 0]] = True
                entered = np.nonzero((begin == 1) & ~first)[0]
                assert word[entered - 1].max() >= 128         # a predecessor word beyond a signed byte


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", GC.FULLCOV)
def test_full_covariance_words(G, ctx, devices, name, t):
    """full, and holes: log b with NaN and -inf columns.  A NaN word end enters nothing under any grammar
    and is never picked while another end is not NaN; the words with a -inf column are never passed"""
    d = devices(name)
    case = d.case
    with tier(G, ctx, t):
        for which in GC.GPU_GRAMMARS[name]:
            word, begin, score, gap = against_the_restatement(d, which)
            if name == "holes":
                CC.holes_pattern(case, d.log_b())
                fin = np.repeat(np.isfinite(score), case.lens)
                assert not np.isin(word[fin], CC.HOLES_NAN_END).any()
                assert not np.isin(word[fin], CC.HOLES_INF).any()
                assert score[4] == 0.0 and not np.isnan(score[3])


# ------------------------------------------------------------- 2. (a): a flat grammar is the flat penalty

FLAT_CASES = tuple(n for n in CC.ALL + CC.BEYOND if n != "crowd")       # crowd has 300 words: beyond the cap on K


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", FLAT_CASES)
def test_a_flat_grammar_is_connect_streams(G, ctx, devices, name, t):
    """pair == p, start == fin == 0 (given, and as null pointers): the score is ghmm_connect_streams(p)'s
    as a value; at p = 0 and -inf word, path and begin are its bits on every utterance, ties included (ones,
    dup); at p = -5 wherever connect_cases' gap on the device's log b exceeds GAP"""
    d = devices(name)
    case = d.case
    with tier(G, ctx, t):
        for p in (0.0, -5.0, -INF):
            cw, cp, cb, cs = d.connect(p)
            start, pair, fin = GC.flat(case.K, p)
            for g in ((start, pair, fin), (None, pair, None)):
                word, path, begin, score = d.grammar(*g)
                assert np.array_equal(score, cs, equal_nan=True), (name, p, score, cs)
                if p == -5.0:
                    at = GC.compared(case, CC.decode(case, d.log_b(), p)[4]) if g[0] is not None else at
                else:
                    at = np.ones(case.F, dtype=bool)
                assert same(word[at], cw[at]) and same(path[at], cp[at]) and same(begin[at], cb[at]), (name, p)


def test_more_than_256_words_are_refused(G, ctx, devices):
    """crowd (K = 300): GHMM_ERR_UNSUPPORTED, the message names the constant"""
    case = CC.make(G, "crowd")
    dms = [[ctx.model(h) for h in w] for w in case.words]
    corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
    try:
        assert code(G, lambda: ctx.connect_grammar_streams(dms, corpora, np.zeros((300, 300)))) == G.ERR_UNSUPPORTED
        assert "GHMM_GRAMMAR_MAX_WORDS" in ctx.lib.ghmm_last_error().decode()
    finally:
        for o in [m for w in dms for m in w] + corpora:
            o.close()


# ------------------------------------------------------------- 3. (b): a chain grammar is the forced alignment

@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", sorted(GC.CHAINS))
def test_a_chain_grammar_is_align_streams(G, ctx, devices, name, t):
    d = devices(name)
    case = d.case
    finite = 0
    with tier(G, ctx, t):
        for tr in GC.CHAINS[name]:
            aw, ap, ab, asc = d.align([tr] * case.U)
            word, path, begin, score = d.grammar(*GC.chain(case.K, tr))
            assert np.array_equal(score, asc, equal_nan=True), (name, tr, score, asc)
            at = np.repeat(np.isfinite(asc), case.lens)
            finite += int(np.isfinite(asc[case.lens > 0]).sum())
            assert same(word[at], aw[at]) and same(path[at], ap[at]) and same(begin[at], ab[at]), (name, tr)
            got = CC.strings(word, begin, case.lens)
            assert all(s == tuple(tr) for s, f, T in zip(got, np.isfinite(asc), case.lens) if f and T)
    assert finite >= len(GC.CHAINS[name])


# ------------------------------------------------------------- 4. repeats, launches

def timed(G, ctx, call):
    """the call's result and its launches per kind; the preparation of the concatenated vocabularies
    (GHMM_K_PREPARE) is not part of what is pinned"""
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    try:
        out = call()
        kt = {k: n for k, (_, n) in ctx.kernel_times().items() if n and k != "prepare"}
    finally:
        ctx.set_option(G.OPT_TIMING, 0)
    return out, kt


@pytest.mark.parametrize("name", ["narrow", "many", "full", "k256", "cap", "k100", "k72"])
def test_launch_counts_and_a_second_call(G, ctx, devices, name):
    """2 P - 1 launches under GHMM_K_EMISSION (full-covariance: P, the folds are the emission's own
    epilogue) and ONE under GHMM_K_VITERBI: lattice and trace together; a second identical call repeats
    every byte, GHMM_BUF_B included, which is what ghmm_connect_streams leaves"""
    d = devices(name)
    P = d.case.P
    g = GC.grammar(d.case, "random")
    first = d.grammar(*g) + (d.log_b(),)
    second, kt = timed(G, ctx, lambda: d.grammar(*g))
    assert kt == {"emission": P if d.full else 2 * P - 1, "viterbi": 1}
    assert all(same(a, b) for a, b in zip(first, second + (d.log_b(),)))
    d.connect(0.0)
    assert same(d.log_b(), first[4])


def test_other_calls_in_between_change_nothing(G, ctx, devices):
    """cap's call (more than 48 KB of LDS, the largest tables), others between, cap's again; and the
    grammar decoder shares its back-pointer scratch with connect and align"""
    big, small, f = devices("cap"), devices("narrow"), devices("full")
    hm, X, lens = synth_case(G, 7, 2, 4, [50, 20])
    om, oc, st = ctx.model(hm), ctx.corpus(X, lens), ctx.stats(hm.N, hm.M, hm.D)
    gb, gs, gf = (GC.grammar(x.case, "random") for x in (big, small, f))
    try:
        first = big.grammar(*gb) + (big.log_b(),)
        first_s = small.grammar(*gs)
        first_f = f.grammar(*gf)
        ctx.score(om, oc)
        ctx.estep(om, oc, st)
        ctx.sync()
        small.connect(-5.0)
        small.align([(0,)] * small.case.U)
        assert all(same(a, b) for a, b in zip(small.grammar(*gs), first_s))
        small.grammar(*GC.norepeat(small.case.K))
        assert all(same(a, b) for a, b in zip(big.grammar(*gb) + (big.log_b(),), first))
        big.recognise()
        assert all(same(a, b) for a, b in zip(f.grammar(*gf), first_f))
    finally:
        om.close(); oc.close(); st.close()


# ------------------------------------------------------------- 5. refusals

class Raw:
    """the call through the C ABI on caller-owned destinations pre-filled with a pattern, so that a refusal
    can be seen to have written nothing"""

    def __init__(self, G, ctx, case, full):
        self.G, self.ctx, self.full = G, ctx, full
        n = max(case.F, 1) + 1
        self.word, self.path, self.begin = (np.full(n, -7, dtype=np.int32) for _ in range(3))
        self.score = np.full(case.U + 1, -777.0)

    def untouched(self):
        return all(np.all(a == -7) for a in (self.word, self.path, self.begin)) and np.all(self.score == -777.0)

    def call(self, vocab, K, corpora, P, start, pair, fin, drop=None):
        G = self.G
        dp, ip = G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_int32)
        dest = [self.word.ctypes.data_as(ip), self.path.ctypes.data_as(ip), self.begin.ctypes.data_as(ip),
                self.score.ctypes.data_as(dp)]
        if drop is not None:
            dest[drop] = None
        gram = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (start, pair, fin)]
        fn = self.ctx.lib.ghmm_connect_grammar_full_streams if self.full else self.ctx.lib.ghmm_connect_grammar_streams
        return fn(self.ctx.h, vocab, K, corpora, P, *[None if a is None else a.ctypes.data_as(dp) for a in gram],
                  *dest)


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
        for drop in range(4):
            assert raw.call(vocab, K, corpora, P, start, pair, fin, drop=drop) == arg, ("null destination", drop)
        assert raw.call(vocab, K, corpora, P, start, None, fin) == arg, "null pair"
        for bad in (np.nan, INF):
            assert raw.call(vocab, K, corpora, P, with_at(start, K - 1, bad), pair, fin) == arg, ("start", bad)
            assert raw.call(vocab, K, corpora, P, start, with_at(pair, K * K - 1, bad), fin) == arg, ("pair", bad)
            assert raw.call(vocab, K, corpora, P, None, with_at(pair, 0, bad), None) == arg, ("pair", bad)
            assert raw.call(vocab, K, corpora, P, start, pair, with_at(fin, 0, bad)) == arg, ("fin", bad)
        assert raw.call(None, K, corpora, P, start, pair, fin) == arg
        assert raw.call(vocab, 0, corpora, P, start, pair, fin) == arg
        # K = 257: the first word 257 times (at most 17 states each: within the cap on the states)
        z = np.zeros((257, 257))
        assert case.Ns[0] * 257 <= 2048
        assert raw.call(handles(G, flat[:P] * 257), 257, corpora, P, None, z, None) == unsupported, "K = 257"
        assert "GHMM_GRAMMAR_MAX_WORDS" in ctx.lib.ghmm_last_error().decode()
        # NS above the cap: 33 times a word of 64 states (2112 > 2048), every stream's model repeated
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
        # and the same arguments, valid, do write: the frames and the scores, nothing behind them
        assert raw.call(vocab, K, corpora, P, start, pair, fin) == G.OK
        want = d.grammar(start, pair, fin)
        for got, ref in zip((raw.word, raw.path, raw.begin, raw.score), want):
            assert same(got[:len(ref)], ref) and np.all(got[len(ref):] == (-777.0 if got.dtype.kind == "f" else -7))
    finally:
        for o in extra:
            o.close()


def test_utterances_of_no_frames_score_0_and_write_no_entries(G, ctx, devices):
    """all utterances empty: U > 0, F = 0"""
    d = devices("mixed")
    case = d.case
    lens = np.zeros(3, dtype=np.int32)
    empty = [ctx.corpus(np.zeros((0, x.D)), lens) for x in case.words[0]]
    raw = Raw(G, ctx, case, False)
    try:
        rc = raw.call(handles(G, [m for w in d.dms for m in w]), case.K, handles(G, empty), case.P,
                      *GC.random(case.K, 3))
        assert rc == G.OK
        assert np.all(raw.score[:3] == 0.0) and not np.signbit(raw.score[:3]).any() and raw.score[3] == -777.0
        assert all(np.all(a == -7) for a in (raw.word, raw.path, raw.begin))
    finally:
        for c in empty:
            c.close()


# ------------------------------------------------------------- 6. the command line

def write_files(G, tmp, d):
    """the case's words as .hmm files, its utterances of at least one frame as .perfil files per stream,
    and the lists; returns (the utterances written, the feature lists, the words' names)"""
    case = d.case
    off = offsets(case.lens)
    HM = G.HostFullModel if d.full else G.HostModel
    names = [w[0].word for w in case.words]
    assert len(set(names)) == len(names)
    for w, hms in zip(names, case.words):
        HM.write_streams(os.path.join(tmp, w + ".hmm"), hms)
    utts = [u for u in range(case.U) if case.lens[u] > 0]
    lists = []
    for p, X in enumerate(case.Xs):
        for u in utts:
            G.perfil_write(os.path.join(tmp, f"s{p}_u{u}.perfil"), X[off[u]:off[u + 1]])
        lists.append(f"list_{p}.txt")
        open(os.path.join(tmp, lists[-1]), "w").write("\n".join(f"s{p}_u{u}.perfil" for u in utts) + "\n")
    open(os.path.join(tmp, "models.txt"), "w").write("\n".join(w + ".hmm" for w in names) + "\n")
    open(os.path.join(tmp, "words.txt"), "w").write("\n".join(names[case.spoken[u][0]] for u in utts) + "\n")
    return utts, lists, names


def write_grammar(path, start, pair, fin, K=None, drop=0):
    toks = [repr(float(v)) for v in np.concatenate([start, pair.ravel(), fin])]
    toks = toks[:len(toks) - drop]
    open(path, "w").write(f"{len(start) if K is None else K}\n" + " ".join(toks) + "\n")


def run(binary, tmp, args, env):
    e = {k: v for k, v in os.environ.items()
         if k not in ("GHMM_CONNECTED", "GHMM_WORD_PENALTY", "GHMM_GRAMMAR", "GHMM_ALIGN")}
    e.update(env)
    p = subprocess.run([binary] + args, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    return p.returncode, p.stdout.decode(errors="replace")


@pytest.mark.parametrize("name", ["mixed", "full"])
def test_command_line_with_a_grammar_file(G, ctx, devices, tmp_path, name):
    d = devices(name)
    case = d.case
    tmp = str(tmp_path)
    utts, lists, names = write_files(G, tmp, d)
    off = offsets(case.lens)
    args = ["1", "models.txt", "1"] + lists + ["words.txt", "report.txt"]
    HM = G.HostFullModel if d.full else G.HostModel
    mk = ctx.full_model if d.full else ctx.model
    dms = [[mk(h) for h in HM.read_streams(os.path.join(tmp, w + ".hmm"))] for w in names]
    lens = case.lens[utts]
    corpora = [ctx.corpus(np.concatenate([X[off[u]:off[u + 1]] for u in utts]), lens) for X in case.Xs]
    start, pair, fin = GC.random(case.K, GC.RANDOM_SEED[name])
    assert (pair == -INF).any()
    write_grammar(os.path.join(tmp, "g.txt"), start, pair, fin)
    try:
        for env, p in (({}, 0.0), ({"GHMM_WORD_PENALTY": "-1.5"}, -1.5)):
            word, path, begin, score = d.grammar(start, pair + p, fin, dms, corpora)
            want = [f"s0_u{u}.perfil : " + "".join(names[k] + " " for k in s) + ": " + fmt(sc)
                    for u, s, sc in zip(utts, CC.strings(word, begin, lens), score)]
            rc, text = run(BIN[d.full], tmp, args, dict(env, GHMM_CONNECTED="1", GHMM_GRAMMAR="g.txt"))
            assert rc == 0, text[-2000:]
            assert [l for l in text.replace("\r", "").split("\n") if l.startswith("s0_u")] == want
            rep = open(os.path.join(tmp, "report.txt")).read().split("\n")
            assert "Connected word recognition" in rep[0] and f"word penalty {p:g}" in rep[0] and "grammar g.txt" in rep[0]
            assert rep[1:1 + len(want)] == want and rep[1 + len(want):] == [""]
        # malformed: a short file, a token that is no number, another K; the variable without
        # GHMM_CONNECTED=1 and with GHMM_ALIGN=1: a message, exit 1, no report
        write_grammar(os.path.join(tmp, "short.txt"), start, pair, fin, drop=1)
        write_grammar(os.path.join(tmp, "otherk.txt"), *GC.random(case.K + 1, 1))
        open(os.path.join(tmp, "word.txt"), "w").write(open(os.path.join(tmp, "g.txt")).read().replace("-inf", "never", 1))
        con = {"GHMM_CONNECTED": "1"}
        for env, say in ((dict(con, GHMM_GRAMMAR="short.txt"), "is short"),
                         (dict(con, GHMM_GRAMMAR="word.txt"), "is no number"),
                         (dict(con, GHMM_GRAMMAR="otherk.txt"), f"is for {case.K + 1} words"),
                         (dict(con, GHMM_GRAMMAR="missing.txt"), "not found"),
                         ({"GHMM_GRAMMAR": "g.txt"}, "GHMM_GRAMMAR takes GHMM_CONNECTED=1"),
                         ({"GHMM_GRAMMAR": "g.txt", "GHMM_ALIGN": "1"}, "GHMM_GRAMMAR takes GHMM_CONNECTED=1")):
            rc, text = run(BIN[d.full], tmp, args[:-1] + ["report2.txt"], env)
            assert rc == 1 and say in text, (env, text[-500:])
            assert not os.path.exists(os.path.join(tmp, "report2.txt")), env
        # without the variable: the flat-penalty decoder's lines, its first line without a grammar
        word, path, begin, score = (ctx.connect_full_streams if d.full else ctx.connect_streams)(dms, corpora, -5.0)
        want = [f"s0_u{u}.perfil : " + "".join(names[k] + " " for k in s) + ": " + fmt(sc)
                for u, s, sc in zip(utts, CC.strings(word, begin, lens), score)]
        rc, text = run(BIN[d.full], tmp, args, {"GHMM_CONNECTED": "1", "GHMM_WORD_PENALTY": "-5"})
        assert rc == 0, text[-2000:]
        rep = open(os.path.join(tmp, "report.txt")).read().split("\n")
        assert rep[0].endswith("word penalty -5 ") and "grammar" not in rep[0] and rep[1:1 + len(want)] == want
    finally:
        for o in [m for w in dms for m in w] + corpora:
            o.close()
