"""Forced alignment on the GPU: ghmm_align_streams and ghmm_align_full_streams (k_align) and the two
recognisers' command lines with GHMM_ALIGN=1 — GPU box only.  The cases and the float64 restatement of the
definition are align_cases.py's; test_align_host.py shows on the CPU that the restatement is the definition
and that the cases keep the margin under which a path that differs cannot be blamed on rounding.

The restatement runs on the log b fetched from the device (GHMM_BUF_B), so the emission's rounding is not
in the comparison: word, path and begin are compared exactly where the restatement's margin is above GAP,
the score to 1e-10 relative (test_connect_gpu.py's bound for the same lattice arithmetic; what remains is
the device's log A against numpy's); -inf and the 0 of an utterance of no frames are met exactly."""
import os
import subprocess

import numpy as np
import pytest

import align_cases as AC
import connect_cases as CC
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
        self.full = case.name in CC.FULLCOV
        mk = ctx.full_model if self.full else ctx.model
        self.dms = [[mk(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]

    def align(self, transcripts=None, dms=None, corpora=None):
        fn = self.ctx.align_full_streams if self.full else self.ctx.align_streams
        return fn(dms or self.dms, corpora or self.corpora,
                  self.case.transcripts if transcripts is None else transcripts)

    def connect(self, p):
        fn = self.ctx.connect_full_streams if self.full else self.ctx.connect_streams
        return fn(self.dms, self.corpora, p)

    def recognise(self):
        fn = self.ctx.recognise_full_streams if self.full else self.ctx.recognise_streams
        return fn(self.dms, self.corpora)

    def viterbi_batch(self):
        fn = self.ctx.viterbi_full_streams_batch if self.full else self.ctx.viterbi_streams_batch
        return fn(self.dms, self.corpora)

    def viterbi(self, k, corpora):
        fn = self.ctx.viterbi_full_streams if self.full else self.ctx.viterbi_streams
        return fn(self.dms[k], corpora)

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
            made[name] = Device(G, ctx, AC.make(G, name))
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


def check_shape_of_an_alignment(case, transcripts, word, path, begin, score):
    """what holds of every alignment of a finite score: its word instances are the transcript's, in order;
    a frame that does not begin one continues the previous frame's word; an instance begins in its first
    state, behind the last state of the one before; the utterance ends in the last state of the last"""
    off = offsets(case.lens)
    Ns = np.asarray(case.Ns)
    assert np.all((0 <= word) & (word < case.K)) and np.all((0 <= path) & (path < Ns[word]))
    assert set(np.unique(begin).tolist()) <= {0, 1}
    for u, T in enumerate(case.lens):
        if T == 0 or not np.isfinite(score[u]):
            continue
        w, s, b = (a[off[u]:off[u + 1]] for a in (word, path, begin))
        assert b[0] == 1 and tuple(w[b == 1].tolist()) == tuple(transcripts[u]), u
        cont = np.nonzero(b[1:] == 0)[0] + 1
        assert np.all(w[cont] == w[cont - 1]), u
        ent = np.nonzero(b[1:] == 1)[0] + 1
        assert np.all(s[ent] == 0) and np.all(s[ent - 1] == Ns[w[ent - 1]] - 1), u
        assert s[0] == 0 and s[-1] == Ns[w[-1]] - 1, u


def against_the_restatement(d, transcripts=None):
    """one device call against align_cases.align on the device's log b; returns the device's outputs"""
    case = d.case
    transcripts = case.transcripts if transcripts is None else transcripts
    word, path, begin, score = d.align(transcripts)
    lb = d.log_b()
    rw, rp, rb, rs, gap = AC.align(case, lb, transcripts)
    print(case.name, "smallest gap on the device's log b", gap.min(), "scores", score)
    assert np.sum(gap[case.lens > 0] <= AC.GAP) <= AC.MAX_BELOW_GAP, gap
    at = AC.compared(case, gap)
    assert same(word[at], rw[at]) and same(path[at], rp[at]) and same(begin[at], rb[at]), case.name
    scores_close(score, rs)
    assert np.all(score[case.lens == 0] == 0.0) and not np.signbit(score[case.lens == 0]).any()
    check_shape_of_an_alignment(case, transcripts, word, path, begin, score)
    return word, path, begin, score


# ------------------------------------------------------------- 1. against the restatement

@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", AC.SMALL + ("thick",))
def test_against_the_restatement(G, ctx, devices, name, t):
    d = devices(name)
    with tier(G, ctx, t):
        word, path, begin, score = against_the_restatement(d)
    if name == "short":
        assert np.array_equal(score == -INF, [False, True, True, True, True, True, True, False, False])
    if name == "narrow":
        assert np.array_equal(score == -INF, np.isin(d.case.lens, (1, 2)))
    if name == "ones":
        assert np.all(path == 0)


@pytest.mark.parametrize("t", [0, 1])
def test_the_cap(G, ctx, devices, t):
    """S = 2046 on 2200 frames: more than 48 KB of LDS, eight composite states per thread; one instance
    more (S = 2049) is refused"""
    d = devices("cap")
    with tier(G, ctx, t):
        word, path, begin, score = against_the_restatement(d)
        assert np.isfinite(score).all()
        more = [d.case.transcripts[0] + (0,)]
        assert AC.states_of(d.case, more[0]) == 2049
        assert code(G, lambda: d.align(more)) == G.ERR_UNSUPPORTED
        assert "2048" in ctx.lib.ghmm_last_error().decode()


@pytest.mark.parametrize("t", [0, 1])
def test_the_cap_among_small_utterances(G, ctx, devices, t):
    """cap-mixed: S = 2046 in one launch with S = 6, 3 and 60 and an utterance of no frames.  Every block
    runs 256 threads on LDS rows 2046 apart, most of them unused; the last two utterances keep their
    back-pointers behind the long one's 4.5 MB.  Compared as test_the_cap compares; and every small
    utterance's outputs are the bytes of the same utterance aligned in a launch without the long one"""
    d = devices("cap-mixed")
    case = d.case
    long = AC.CAP_MIXED_LONG
    keep = [u for u in range(case.U) if u != long]
    off = offsets(case.lens)
    at = np.concatenate([np.arange(off[u], off[u + 1]) for u in keep])
    corpora = [ctx.corpus(X[at], case.lens[keep]) for X in case.Xs]
    try:
        with tier(G, ctx, t):
            word, path, begin, score = against_the_restatement(d)
            assert np.isfinite(score).all() and score[1] == 0.0
            sw, sp, sb, ss = d.align([case.transcripts[u] for u in keep], corpora=corpora)
        assert same(word[at], sw) and same(path[at], sp) and same(begin[at], sb) and same(score[keep], ss)
    finally:
        for c in corpora:
            c.close()


# ------------------------------------------------------------- 1b. log b that is not finite

@pytest.mark.parametrize("t", [0, 1])
def test_nan_and_minus_inf_columns(G, ctx, devices, t):
    """connect_cases' holes: NaN (det = 0) and -inf (c = 0) columns in log b.  First the precondition on the
    fetched log b.  Then: a transcript that ends in a NaN word end scores NaN; one with such a word in the
    middle -inf (the NaN entry candidate never enters); one through a column of -inf scores -inf; the
    spoken ones are finite, and on them consequences (b) and (c) hold against connect at penalty 0
    wherever connect's score is finite.  All outputs are align_cases.align's on the fetched log b"""
    d = devices("holes")
    case = d.case
    kinds = {"finite": np.isfinite, "nan": np.isnan, "-inf": lambda x: x == -INF, "0": lambda x: x == 0.0}
    with tier(G, ctx, t):
        for name, (trs, want) in AC.HOLES.items():
            word, path, begin, score = against_the_restatement(d, trs)
            nan, inf = CC.holes_pattern(case, d.log_b())        # the precondition
            print("tier", t, name, "NaN columns", nan, "-inf columns", inf)
            assert all(kinds[k](x) for k, x in zip(want, score)), (name, score)
        cword, cpath, cbegin, cscore = d.connect(0.0)
        fin = np.isfinite(cscore) & (case.lens > 0)
        assert fin[:3].all()
        strings = CC.strings(cword, cbegin, case.lens)
        word, path, begin, score = d.align(strings)
        assert np.array_equal(score[fin], cscore[fin]), (score, cscore)                 # (b)
        gap = AC.align(case, d.log_b(), strings)[4]
        at = np.repeat((gap > 0) & fin, case.lens)
        assert same(word[at], cword[at]) and same(path[at], cpath[at]) and same(begin[at], cbegin[at])
        spoken = d.align()[3]
        assert not np.any(spoken[fin] > cscore[fin]), (spoken, cscore)                  # (c)


# ------------------------------------------------------------- 2. the consequences of the definition

def words_to_try(case):
    return range(case.K) if case.K <= 4 else (0, 33, 69)


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", AC.SMALL)
def test_a_one_word_transcript_is_that_word_s_viterbi_score_bit_for_bit(G, ctx, devices, name, t):
    """(a): score == ghmm_viterbi_streams_batch's [k][u] bit for bit; where ghmm_recognise_streams picks
    word k, its path.  (An utterance of no frames takes the transcript as well: whatever it is, 0.)"""
    d = devices(name)
    case = d.case
    with tier(G, ctx, t):
        table = d.viterbi_batch()
        rword, rpath, rscore = d.recognise()
        assert same(rscore, table)
        for k in words_to_try(case):
            word, path, begin, score = d.align([(k,)] * case.U)
            assert same(score, table[k]), (name, t, k)
            picked = np.repeat(rword == k, case.lens)
            assert same(path[picked], rpath[picked]) and np.all(word == k)
            first = np.zeros(case.F, dtype=np.int32)
            first[offsets(case.lens)[:-1][case.lens > 0]] = 1
            assert same(begin, first)


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", AC.SMALL)
def test_connect_s_strings_give_connect_s_score_and_the_spoken_ones_no_more(G, ctx, devices, name, t):
    """(b): the device's own connect_streams strings at penalty 0, fed back as transcripts, give
    score == connect's score for every utterance, and its word, path and begin where the restatement's gap on
    the device's log b is > 0.  (c): the case's transcripts score no higher"""
    d = devices(name)
    case = d.case
    with tier(G, ctx, t):
        cword, cpath, cbegin, cscore = d.connect(0.0)
        strings = CC.strings(cword, cbegin, case.lens)
        word, path, begin, score = d.align(strings)
        lb = d.log_b()
        assert np.array_equal(score, cscore), (score, cscore)
        gap = AC.align(case, lb, strings)[4]
        at = np.repeat(gap > 0, case.lens)
        print(name, t, "utterances with a unique optimum:", int((gap > 0).sum()), "of", case.U)
        assert same(word[at], cword[at]) and same(path[at], cpath[at]) and same(begin[at], cbegin[at])
        spoken = d.align()[3]
        assert np.all(spoken <= cscore), (spoken, cscore)


@pytest.mark.parametrize("name", ["narrow", "full"])
def test_the_segments_scores_sum_to_the_alignment_s(G, ctx, devices, name):
    """every aligned utterance cut with word_segments + cut_segments, every segment scored by viterbi_streams
    with its word: the segment scores of an utterance sum to its alignment's score (only the order of the
    additions differs: 1e-10 relative)"""
    d = devices(name)
    case = d.case
    word, path, begin, score = d.align()
    segments = G.word_segments(word, begin, case.lens)
    cut = G.cut_segments(case.Xs, case.lens, segments, case.K, score=score)
    sums = np.where(np.isfinite(score), 0.0, score)
    seg_scores = []
    for k, (Xs_k, lens_k) in enumerate(cut):
        if len(lens_k) == 0:
            seg_scores.append(iter(()))
            continue
        corpora = [ctx.corpus(X, lens_k) for X in Xs_k]
        try:
            seg_scores.append(iter(d.viterbi(k, corpora)[1].tolist()))
        finally:
            for c in corpora:
                c.close()
    n = 0
    for u, segs in enumerate(segments):
        if not np.isfinite(score[u]):
            continue
        for k, a, b in segs:            # cut_segments keeps the utterances' and the frames' order per word
            sums[u] += next(seg_scores[k])
            n += 1
    assert n >= 5 and all(next(it, None) is None for it in seg_scores)
    scores_close(sums, score)


# ------------------------------------------------------------- 3. launches, repeats, the workspace

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


@pytest.mark.parametrize("name", ["narrow", "many", "full"])
def test_launch_counts_and_a_second_call(G, ctx, devices, name):
    """2 P - 1 launches under GHMM_K_EMISSION (full-covariance: P, the folds are the emission's own
    epilogue) and ONE under GHMM_K_VITERBI: lattice and trace together; a second identical call repeats
    every byte"""
    d = devices(name)
    P = d.case.P
    first = d.align() + (d.log_b(),)
    second, kt = timed(G, ctx, d.align)
    assert kt == {"emission": P if d.full else 2 * P - 1, "viterbi": 1}
    assert all(same(a, b) for a, b in zip(first, second + (d.log_b(),)))


def test_other_calls_in_between_change_nothing(G, ctx, devices):
    d, o, f = devices("mixed"), devices("narrow"), devices("full")
    hm, X, lens = synth_case(G, 7, 2, 4, [50, 20])
    om, oc, st = ctx.model(hm), ctx.corpus(X, lens), ctx.stats(hm.N, hm.M, hm.D)
    try:
        first = d.align() + (d.log_b(),)
        first_f = f.align() + (f.log_b(),)
        ctx.estep_log(om, oc, st)
        ctx.sync()
        o.connect(-5.0)
        o.recognise()
        o.align()
        assert all(same(a, b) for a, b in zip(d.align() + (d.log_b(),), first))
        ctx.estep_log(om, oc, st)
        d.connect(0.0)
        assert all(same(a, b) for a, b in zip(f.align() + (f.log_b(),), first_f))
        # and the connected-word decoder, whose scratch the alignment shares, is not disturbed by it
        con = d.connect(-5.0)
        d.align()
        assert all(same(a, b) for a, b in zip(d.connect(-5.0), con))
    finally:
        om.close(); oc.close(); st.close()


# ------------------------------------------------------------- 4. refusals

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

    def call(self, vocab, K, corpora, P, seq, seq_off, drop=None):
        G = self.G
        dp, ip = G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_int32)
        self.keep = (np.asarray(list(seq) + [0], dtype=np.int32), np.asarray(seq_off, dtype=np.int32))
        args = [a.ctypes.data_as(ip) for a in self.keep + (self.word, self.path, self.begin)]
        args.append(self.score.ctypes.data_as(dp))
        if drop is not None:
            args[drop] = None
        fn = self.ctx.lib.ghmm_align_full_streams if self.full else self.ctx.lib.ghmm_align_streams
        return fn(self.ctx.h, vocab, K, corpora, P, *args)


def handles(G, objs):
    return (G.C.c_void_p * len(objs))(*[o.h if o is not None else None for o in objs])


def flat_transcripts(trs):
    return [k for t in trs for k in t], np.concatenate([[0], np.cumsum([len(t) for t in trs])]).tolist()


@pytest.mark.parametrize("name", ["mixed", "full"])
def test_refusals_write_nothing(G, ctx, devices, name):
    d = devices(name)
    case = d.case
    K, P, U = case.K, case.P, case.U
    raw = Raw(G, ctx, case, d.full)
    flat = [m for w in d.dms for m in w]
    vocab, corpora = handles(G, flat), handles(G, d.corpora)
    arg, unsupported = G.ERR_ARG, G.ERR_UNSUPPORTED
    seq, seq_off = flat_transcripts(case.transcripts)
    with_frames = int(np.nonzero(case.lens > 0)[0][0])
    extra = []
    d.align()
    before = d.log_b()
    try:
        for drop in range(6):
            assert raw.call(vocab, K, corpora, P, seq, seq_off, drop=drop) == arg, ("null argument", drop)
        assert raw.call(vocab, K, corpora, P, seq, [1] + seq_off[1:]) == arg, "seq_off[0] != 0"
        down = list(seq_off)
        down[U - 1] = down[U] + 1
        assert raw.call(vocab, K, corpora, P, seq + [0, 0], down) == arg, "a decreasing seq_off"
        for bad in (K, -1, 1 << 20):
            assert raw.call(vocab, K, corpora, P, seq[:-1] + [bad], seq_off) == arg, ("a word outside", bad)
        empty = [() if u == with_frames else t for u, t in enumerate(case.transcripts)]
        assert raw.call(vocab, K, corpora, P, *flat_transcripts(empty)) == arg, "an empty transcript with frames"
        assert "empty transcript" in ctx.lib.ghmm_last_error().decode()
        assert raw.call(None, K, corpora, P, seq, seq_off) == arg and raw.call(vocab, 0, corpora, P, seq, seq_off) == arg
        # a word of 65 states, and a transcript of more than 2048 states (33 times a word of 64)
        h = case.words[0]
        rng = np.random.default_rng(3)
        if d.full:
            from fullcov_support import rand_fmodel
            w64 = [ctx.full_model(rand_fmodel(G, rng, 64, x.M, x.D, spread=1.0, asym=False)) for x in h]
            w65 = []        # (a full-covariance model of 65 states cannot be made: ghmm_fmodel_create refuses it)
        else:
            import vocab_cases as V
            from fullcov_support import banded
            w64, w65 = ([ctx.model(V.rand_model(G, rng, N, x.M, x.D, banded(rng, N))) for x in h] for N in (64, 65))
        extra += w64 + w65
        ones = [(0,)] * U
        if w65:
            assert raw.call(handles(G, flat[:P] + w65), 2, corpora, P, *flat_transcripts(ones)) == unsupported, "65 states"
            assert "65 states" in ctx.lib.ghmm_last_error().decode()
        long = [(1,) * 33 if u == with_frames else (0,) for u in range(U)]
        assert raw.call(handles(G, flat[:P] + w64), 2, corpora, P, *flat_transcripts(long)) == unsupported, "S_u above the cap"
        assert "2048" in ctx.lib.ghmm_last_error().decode()
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert raw.call(vocab, K, corpora, P, seq, seq_off) == unsupported, "robust"
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert raw.untouched()
        assert same(d.log_b(), before)
        # U = 0 touches nothing, with or without destinations and transcripts
        none = [ctx.corpus(np.zeros((0, x.D)), np.zeros(0, dtype=np.int32)) for x in h]
        extra += none
        assert raw.call(vocab, K, handles(G, none), P, [], [0]) == G.OK
        assert raw.call(vocab, K, handles(G, none), P, [], [0], drop=1) == G.OK
        assert raw.untouched()
        # and the same arguments, valid, do write: the frames and the scores, nothing behind them
        assert raw.call(vocab, K, corpora, P, seq, seq_off) == G.OK
        want = d.align()
        for got, ref in zip((raw.word, raw.path, raw.begin, raw.score), want):
            assert same(got[:len(ref)], ref) and np.all(got[len(ref):] == (-777.0 if got.dtype.kind == "f" else -7))
        # the longest transcript that fits: 32 times the word of 64 states is inside the cap (too short: -inf)
        fits = [(1,) * 32 if u == with_frames else (0,) for u in range(U)]
        assert raw.call(handles(G, flat[:P] + w64), 2, corpora, P, *flat_transcripts(fits)) == G.OK
        assert raw.score[with_frames] == -INF
    finally:
        for o in extra:
            o.close()


def test_utterances_of_no_frames_score_0_and_write_no_entries(G, ctx, devices):
    """all utterances empty (U > 0, F = 0), under an empty transcript, a word, and a transcript far beyond
    the cap: whatever it is"""
    d = devices("mixed")
    case = d.case
    lens = np.zeros(3, dtype=np.int32)
    empty = [ctx.corpus(np.zeros((0, x.D)), lens) for x in case.words[0]]
    raw = Raw(G, ctx, case, False)
    try:
        rc = raw.call(handles(G, [m for w in d.dms for m in w]), case.K, handles(G, empty), case.P,
                      *flat_transcripts([(), (2,), (1,) * 300]))
        assert rc == G.OK
        assert np.all(raw.score[:3] == 0.0) and not np.signbit(raw.score[:3]).any() and raw.score[3] == -777.0
        assert all(np.all(a == -7) for a in (raw.word, raw.path, raw.begin))
    finally:
        for c in empty:
            c.close()


# ------------------------------------------------------------- 5. the command line

def write_files(G, tmp, d):
    """the case's words as .hmm files, its utterances of at least one frame as .perfil files per stream, and
    the lists, the word file holding the transcripts joined by '+'; returns (the utterances written, the
    feature lists, the words' names)"""
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
    open(os.path.join(tmp, "words.txt"), "w").write(
        "\n".join("+".join(names[k] for k in case.transcripts[u]) for u in utts) + "\n")
    return utts, lists, names


def run(binary, tmp, args, env):
    e = {k: v for k, v in os.environ.items() if k not in ("GHMM_CONNECTED", "GHMM_WORD_PENALTY", "GHMM_ALIGN")}
    e.update(env)
    p = subprocess.run([binary] + args, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    return p.returncode, p.stdout.decode(errors="replace")


@pytest.mark.parametrize("name", ["mixed", "full"])
def test_command_line_aligns_transcripts(G, ctx, devices, tmp_path, name):
    d = devices(name)
    case = d.case
    tmp = str(tmp_path)
    utts, lists, names = write_files(G, tmp, d)
    off = offsets(case.lens)
    args = ["1", "models.txt", "1"] + lists + ["words.txt", "report.txt"]
    # what the library call gives on the files' own doubles
    HM = G.HostFullModel if d.full else G.HostModel
    mk = ctx.full_model if d.full else ctx.model
    dms = [[mk(h) for h in HM.read_streams(os.path.join(tmp, w + ".hmm"))] for w in names]
    lens = case.lens[utts]
    corpora = [ctx.corpus(np.concatenate([X[off[u]:off[u + 1]] for u in utts]), lens) for X in case.Xs]
    try:
        word, path, begin, score = d.align([case.transcripts[u] for u in utts], dms, corpora)
        want = [f"s0_u{u}.perfil : " + "  ".join(f"{names[k]} {a} {b}" for k, a, b in segs) + " : " + fmt(sc)
                for u, segs, sc in zip(utts, G.word_segments(word, begin, lens), score)]
        rc, text = run(BIN[d.full], tmp, args, {"GHMM_ALIGN": "1"})
        assert rc == 0, text[-2000:]
        assert [l for l in text.replace("\r", "").split("\n") if l.startswith("s0_u")] == want
        rep = open(os.path.join(tmp, "report.txt")).read().split("\n")
        assert "Forced alignment" in rep[0]
        assert rep[1:1 + len(want)] == want and rep[1 + len(want):] == [""]
        # together with the connected-word decoder, and with several model sets: refused
        rc, text = run(BIN[d.full], tmp, args[:-1] + ["report2.txt"], {"GHMM_ALIGN": "1", "GHMM_CONNECTED": "1"})
        assert rc == 1 and "exclude each other" in text and not os.path.exists(os.path.join(tmp, "report2.txt"))
        rc, text = run(BIN[d.full], tmp, ["2", "models.txt", "models.txt", "1", "1"] + lists + lists +
                       ["words.txt", "report2.txt"], {"GHMM_ALIGN": "1"})
        assert rc == 1 and "exactly one model set" in text and not os.path.exists(os.path.join(tmp, "report2.txt"))
        # an unknown word is refused by name
        lines = open(os.path.join(tmp, "words.txt")).read().split("\n")
        lines[1] = lines[1] + "+nosuchword"
        open(os.path.join(tmp, "words_bad.txt"), "w").write("\n".join(lines))
        rc, text = run(BIN[d.full], tmp, args[:-2] + ["words_bad.txt", "report3.txt"], {"GHMM_ALIGN": "1"})
        assert rc == 1 and "nosuchword" in text and "not in the vocabulary" in text
        # without the variable (or with another value) the isolated-word recogniser runs as it did: the
        # word file's tokens are what was spoken, no name is looked up
        for env in ({}, {"GHMM_ALIGN": "0"}):
            rc, text = run(BIN[d.full], tmp, args, env)
            assert rc == 0, text[-2000:]
            assert open(os.path.join(tmp, "report.txt")).read().startswith("Isolated word recognition")
    finally:
        for o in [m for w in dms for m in w] + corpora:
            o.close()
