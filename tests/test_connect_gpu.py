"""Connected-word decoding on the GPU: ghmm_connect_streams and ghmm_connect_full_streams (k_connect) and the
two recognisers' command lines with GHMM_CONNECTED=1 — GPU box only.  The cases and the float64
restatement of the definition are connect_cases.py's; test_connect_host.py shows on the CPU that the
restatement is the definition and that the cases keep the margin under which a path that differs cannot
be blamed on rounding.

The restatement runs on the log b fetched from the device (GHMM_BUF_B), so the emission's rounding is not
in the comparison: word, path and begin are compared exactly, the score to 1e-10 relative
(test_vocab_streams_gpu.scores_close's bound; what remains is the device's log A against numpy's)."""
import os
import subprocess

import numpy as np
import pytest

import connect_cases as CC
from _load import PKG_DIR
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import code, fmt, offsets, spoken_blocks, bubble
from streams_util import synth_case

pytestmark = pytest.mark.gpu

BIN = {False: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-fs"),
       True: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-full-fs")}
INF = np.inf


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def scores_close(got, ref, rel=1e-10):
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
    """a case's device models (dms[k][p]) and corpora, and the two calls of its model kind"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        self.full = case.name in CC.FULLCOV
        mk = ctx.full_model if self.full else ctx.model
        made = {}       # a host model that stands for several words (ones2048) is one device model: its handle repeats
        self.dms = [[made[id(h)] if id(h) in made else made.setdefault(id(h), mk(h)) for h in w] for w in case.words]
        self.models = list(made.values())
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]

    def connect(self, p, dms=None, corpora=None):
        fn = self.ctx.connect_full_streams if self.full else self.ctx.connect_streams
        return fn(dms or self.dms, corpora or self.corpora, p)

    def recognise(self):
        fn = self.ctx.recognise_full_streams if self.full else self.ctx.recognise_streams
        return fn(self.dms, self.corpora)

    def log_b(self):
        return self.ctx.fetch(self.G.BUF_B, (self.case.F, self.case.NS))

    def close(self):
        for o in self.models + self.corpora:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(G, ctx, CC.make(G, name))
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


# ------------------------------------------------------------- 1. against the restatement

@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", CC.NONTIE + CC.BEYOND)
def test_against_the_restatement(G, ctx, devices, name, t):
    d = devices(name)
    case = d.case
    with tier(G, ctx, t):
        for p in CC.penalties(name):
            word, path, begin, score = d.connect(p)
            lb = d.log_b()
            rw, rp, rb, rs, gap = CC.decode(case, lb, p)
            print(name, t, p, "smallest gap on the device's log b", gap.min())
            assert same(word, rw) and same(path, rp) and same(begin, rb), (name, t, p)
            scores_close(score, rs)
            check_shape_of_a_decoding(case, word, path, begin)
            assert np.all(score[case.lens == 0] == 0.0) and not np.signbit(score[case.lens == 0]).any()
            if p in CC.QUALIFY[name]:
                got = CC.strings(word, begin, case.lens)
                for u in CC.QUALIFY[name][p]:
                    assert got[u] == case.spoken[u], (name, p, u, got[u])
            if p == -1e4:       # one word takes each utterance
                assert begin.sum() == (case.lens > 0).sum()


def check_one_state_closed_form(case, lb, word, path, begin, score):
    """one-state words with A = [[1]] at p = 0: every d_t(k) = e_{t-1} + log b_k(t).  A maximiser of the
    previous frame stays (the tie goes to the word), every other word enters from the lowest maximiser"""
    off = offsets(case.lens)
    for u, T in enumerate(case.lens):
        if T == 0:
            assert score[u] == 0.0
            continue
        b = lb[off[u]:off[u + 1]]
        ds = [b[0]]
        for x in b[1:]:
            ds.append(ds[-1].max() + x)
        assert score[u] == ds[-1].max() and word[off[u + 1] - 1] == int(np.argmax(ds[-1]))
        for f in range(1, T):
            k, prev = word[off[u] + f], ds[f - 1]
            if prev[k] == prev.max():
                assert begin[off[u] + f] == 0 and word[off[u] + f - 1] == k, (u, f)
            else:
                assert begin[off[u] + f] == 1 and word[off[u] + f - 1] == int(np.argmax(prev)), (u, f)
    assert np.all(path == 0)


@pytest.mark.parametrize("t", [0, 1])
def test_one_state_words_follow_from_the_log_b_exactly(G, ctx, devices, t):
    """A = [[1]] and p = 0: check_one_state_closed_form"""
    d = devices("ones")
    case = d.case
    with tier(G, ctx, t):
        for p in CC.penalties("ones"):
            word, path, begin, score = d.connect(p)
            lb = d.log_b()
            rw, rp, rb, rs, _ = CC.decode(case, lb, p)
            assert same(word, rw) and same(path, rp) and same(begin, rb) and same(score, rs), p
            check_shape_of_a_decoding(case, word, path, begin)
            if p == 0.0:
                check_one_state_closed_form(case, lb, word, path, begin, score)


@pytest.mark.parametrize("t", [0, 1])
def test_2048_one_state_words(G, ctx, devices, t):
    """ones2048: K = NS = 2048, every thread folds eight word ends of its own, then the butterfly, then the
    four partials.  log A is exactly 0 on both sides, so everything is compared exactly.  Under
    GHMM_OPT_KERNELS = 1 the copies of a model have equal bits: every pick is a tie of 409 or 410 words and
    goes to the lowest, a word below 5"""
    d = devices("ones2048")
    case = d.case
    assert len(d.models) == 5 and case.K == 2048
    with tier(G, ctx, t):
        for p in CC.penalties("ones2048"):
            word, path, begin, score = d.connect(p)
            lb = d.log_b()
            if t == 1:
                for a in range(5):
                    assert same(lb[:, a::5], np.repeat(lb[:, a:a + 1], lb[:, a::5].shape[1], axis=1)), a
            rw, rp, rb, rs, _ = CC.decode(case, lb, p)
            assert same(word, rw) and same(path, rp) and same(begin, rb) and same(score, rs), p
            check_shape_of_a_decoding(case, word, path, begin)
            if p == 0.0:
                check_one_state_closed_form(case, lb, word, path, begin, score)
            if t == 1:
                assert np.all(word < 5), p


def test_equal_words_take_the_lower_one(G, ctx, devices):
    """dup under GHMM_OPT_KERNELS = 1, where equal Gaussians give equal bits: word 3 is word 0 again, every
    pick and every entry between the two takes word 0"""
    d = devices("dup")
    case = d.case
    with tier(G, ctx, 1):
        for p in CC.penalties("dup"):
            word, path, begin, score = d.connect(p)
            lb = d.log_b()
            assert same(lb[:, case.bo[0]:case.bo[1]], lb[:, case.bo[3]:case.bo[4]])
            rw, rp, rb, rs, _ = CC.decode(case, lb, p)
            assert same(word, rw) and same(path, rp) and same(begin, rb), p
            scores_close(score, rs)
            assert 3 not in word and 0 in word


# ------------------------------------------------------------- 1b. log b that is not finite

@pytest.mark.parametrize("t", [0, 1])
def test_nan_and_minus_inf_columns(G, ctx, devices, t):
    """holes: full-covariance words whose det = 0 (NaN) and c = 0 (-inf) put non-finite columns into log b.
    First the precondition, on the fetched log b: NaN in exactly these columns, -inf in exactly those.
    Then the rules of include/ghmm.h on the device: a NaN word end loses every pick to a value that is
    not NaN (-inf included), a NaN never wins a strict > in the dense step, a NaN pick never enters"""
    d = devices("holes")
    case = d.case
    with tier(G, ctx, t):
        for p in CC.penalties("holes"):
            word, path, begin, score = d.connect(p)
            lb = d.log_b()
            nan, inf = CC.holes_pattern(case, lb)       # the precondition: what the emission launches wrote
            print("tier", t, "p", p, "NaN columns", nan, "-inf columns", inf)
            rw, rp, rb, rs, gap = CC.decode(case, lb, p)
            print("scores", score, "gaps on the device's log b", gap)
            assert np.all(gap[:3] > CC.GAP), gap
            assert same(word, rw) and same(path, rp) and same(begin, rb), (t, p)
            scores_close(score, rs)
            check_shape_of_a_decoding(case, word, path, begin)
            assert np.isfinite(score[:3]).all() and score[3] == -INF and score[4] == 0.0
            fin = np.repeat(np.isfinite(score), case.lens)
            assert not np.isin(word[fin], CC.HOLES_NAN_END).any()
            off = offsets(case.lens)
            assert word[off[3]:off[4]].tolist() == [1, 1]       # -inf beats word 0's NaN: the lowest -inf end


# ------------------------------------------------------------- 2. p = -inf is the isolated-word decoder

@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("name", CC.ALL + CC.BEYOND)
def test_without_entries_it_is_recognise_bit_for_bit(G, ctx, devices, name, t):
    d = devices(name)
    case = d.case
    off = offsets(case.lens)
    with tier(G, ctx, t):
        rword, rpath, rscore = d.recognise()
        word, path, begin, score = d.connect(-INF)
    assert same(word, np.repeat(rword, case.lens).astype(np.int32))
    assert same(path, rpath)
    assert same(score, rscore[rword, np.arange(case.U)])
    first = np.zeros(case.F, dtype=np.int32)
    first[off[:-1][case.lens > 0]] = 1
    assert same(begin, first)


# ------------------------------------------------------------- 3. one stream, repeats, launches

def test_one_stream_is_stream_0_alone(G, ctx, devices):
    d = devices("narrow")
    case = d.case.stream0()
    dms, corpora = [[w[0]] for w in d.dms], d.corpora[:1]
    ctx.viterbi_streams_batch(dms, corpora)
    want_b = ctx.fetch(G.BUF_B, (case.F, case.NS))
    for p in (0.0, -5.0):
        got = d.connect(p, dms, corpora)
        lb = ctx.fetch(G.BUF_B, (case.F, case.NS))
        assert same(lb, want_b)
        rw, rp, rb, rs, _ = CC.decode(case, lb, p)
        assert same(got[0], rw) and same(got[1], rp) and same(got[2], rb)
        scores_close(got[3], rs)


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


@pytest.mark.parametrize("name", ["narrow", "many", "full", "crowd", "cap"])
def test_launch_counts_and_a_second_call(G, ctx, devices, name):
    """2 P - 1 launches under GHMM_K_EMISSION (full-covariance: P, the folds are the emission's own
    epilogue) and ONE under GHMM_K_VITERBI: lattice and trace together, the launch with more than 48 KB of
    LDS (cap) as well; a second identical call repeats every byte"""
    d = devices(name)
    P = d.case.P
    first = d.connect(-5.0) + (d.log_b(),)
    second, kt = timed(G, ctx, lambda: d.connect(-5.0))
    assert kt == {"emission": P if d.full else 2 * P - 1, "viterbi": 1}
    assert all(same(a, b) for a, b in zip(first, second + (d.log_b(),)))


def test_across_the_48_kb_threshold_and_back(G, ctx, devices):
    """cap's call (73 824 bytes of LDS, the largest back-pointer table), then narrow's (one wave, a small
    table in the same buffer), then cap's again: the first and the third are the same bytes"""
    big, small = devices("cap"), devices("narrow")
    first = big.connect(-5.0) + (big.log_b(),)
    between = small.connect(-5.0)
    third = big.connect(-5.0) + (big.log_b(),)
    assert all(same(a, b) for a, b in zip(first, third))
    assert all(same(a, b) for a, b in zip(between, small.connect(-5.0)))


def test_other_calls_in_between_change_nothing(G, ctx, devices):
    d, o, f = devices("mixed"), devices("narrow"), devices("full")
    hm, X, lens = synth_case(G, 7, 2, 4, [50, 20])
    om, oc, st = ctx.model(hm), ctx.corpus(X, lens), ctx.stats(hm.N, hm.M, hm.D)
    try:
        first = d.connect(0.0) + (d.log_b(),)
        first_f = f.connect(0.0) + (f.log_b(),)
        ctx.score(om, oc)
        ctx.estep(om, oc, st)
        ctx.sync()
        o.recognise()
        o.connect(-5.0)
        assert all(same(a, b) for a, b in zip(d.connect(0.0) + (d.log_b(),), first))
        ctx.estep(om, oc, st)
        d.recognise()
        assert all(same(a, b) for a, b in zip(f.connect(0.0) + (f.log_b(),), first_f))
        # as after the batch calls: the row API does not reuse the workspace, and it serves no posteriors
        d.connect(0.0)
        assert code(G, lambda: ctx.forward(d.dms[0][0], d.corpora[0])) == G.ERR_ARG
        assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
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

    def call(self, vocab, K, corpora, P, p, drop=None):
        G = self.G
        dp, ip = G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_int32)
        dest = [self.word.ctypes.data_as(ip), self.path.ctypes.data_as(ip), self.begin.ctypes.data_as(ip),
                self.score.ctypes.data_as(dp)]
        if drop is not None:
            dest[drop] = None
        fn = self.ctx.lib.ghmm_connect_full_streams if self.full else self.ctx.lib.ghmm_connect_streams
        return fn(self.ctx.h, vocab, K, corpora, P, p, *dest)


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
    extra = []
    try:
        for drop in range(4):
            assert raw.call(vocab, K, corpora, P, 0.0, drop=drop) == arg, ("null destination", drop)
        assert raw.call(vocab, K, corpora, P, np.nan) == arg
        assert raw.call(vocab, K, corpora, P, INF) == arg
        assert raw.call(None, K, corpora, P, 0.0) == arg and raw.call(vocab, 0, corpora, P, 0.0) == arg
        # NS above the cap: 33 times a word of 64 states (2112 > 2048), every stream's model repeated
        h = case.words[0]
        rng = np.random.default_rng(3)
        if d.full:
            from fullcov_support import rand_fmodel
            w64 = [ctx.full_model(rand_fmodel(G, rng, 64, x.M, x.D, spread=1.0, asym=False)) for x in h]
            other_m = ctx.full_model(rand_fmodel(G, rng, h[1].N, h[1].M + 1, h[1].D, spread=1.0, asym=False))
        else:
            import vocab_cases as V
            from fullcov_support import banded
            w64 = [ctx.model(V.rand_model(G, rng, 64, x.M, x.D, banded(rng, 64))) for x in h]
            w65 = [ctx.model(V.rand_model(G, rng, 65, x.M, x.D, banded(rng, 65))) for x in h]
            other_m = ctx.model(V.rand_model(G, rng, h[1].N, h[1].M + 1, h[1].D, banded(rng, h[1].N)))
            extra += w65
            assert raw.call(handles(G, flat[:P] + w65), 2, corpora, P, 0.0) == unsupported, "a word of 65 states"
        extra += w64 + [other_m]
        assert raw.call(handles(G, w64 * 33), 33, corpora, P, 0.0) == unsupported, "NS above the cap"
        assert "2048" in ctx.lib.ghmm_last_error().decode()
        assert raw.call(handles(G, w64 * 32), 32, corpora, P, np.nan) == arg        # (NS = 2048 is inside)
        assert raw.call(handles(G, flat[:1] + [other_m] + flat[2:]), K, corpora, P, 0.0) == unsupported, "differing M"
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert raw.call(vocab, K, corpora, P, 0.0) == unsupported, "robust"
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert raw.untouched()
        # U = 0 touches nothing, with or without destinations
        empty = [ctx.corpus(np.zeros((0, x.D)), np.zeros(0, dtype=np.int32)) for x in h]
        extra += empty
        assert raw.call(vocab, K, handles(G, empty), P, 0.0) == G.OK
        assert raw.call(vocab, K, handles(G, empty), P, 0.0, drop=0) == G.OK
        assert raw.untouched()
        # and the same arguments, valid, do write: the frames and the scores, nothing behind them
        assert raw.call(vocab, K, corpora, P, -5.0) == G.OK
        want = d.connect(-5.0)
        for got, ref in zip((raw.word, raw.path, raw.begin, raw.score), want):
            assert same(got[:len(ref)], ref) and np.all(got[len(ref):] == (-777.0 if got.dtype.kind == "f" else -7))
    finally:
        for o in extra:
            o.close()


def test_an_utterance_of_no_frames_scores_0_and_writes_no_entries(G, ctx, devices):
    """all utterances empty: U > 0, F = 0"""
    d = devices("mixed")
    case = d.case
    lens = np.zeros(3, dtype=np.int32)
    empty = [ctx.corpus(np.zeros((0, x.D)), lens) for x in case.words[0]]
    raw = Raw(G, ctx, case, False)
    try:
        rc = raw.call(handles(G, [m for w in d.dms for m in w]), case.K, handles(G, empty), case.P, 0.0)
        assert rc == G.OK
        assert np.all(raw.score[:3] == 0.0) and not np.signbit(raw.score[:3]).any() and raw.score[3] == -777.0
        assert all(np.all(a == -7) for a in (raw.word, raw.path, raw.begin))
    finally:
        for c in empty:
            c.close()
    # ... and one among others: narrow's utterance 0
    n = devices("narrow")
    word, path, begin, score = n.connect(0.0)
    assert n.case.lens[0] == 0 and score[0] == 0.0 and len(word) == n.case.F


# ------------------------------------------------------------- 5. the command line

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


def run(binary, tmp, args, env):
    e = {k: v for k, v in os.environ.items() if k not in ("GHMM_CONNECTED", "GHMM_WORD_PENALTY")}
    e.update(env)
    p = subprocess.run([binary] + args, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    return p.returncode, p.stdout.decode(errors="replace")


@pytest.mark.parametrize("name", ["mixed", "full"])
def test_command_line_decodes_word_strings(G, ctx, devices, tmp_path, name):
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
        for env, p in (({"GHMM_CONNECTED": "1"}, 0.0), ({"GHMM_CONNECTED": "1", "GHMM_WORD_PENALTY": "-5"}, -5.0)):
            word, path, begin, score = d.connect(p, dms, corpora)
            want = [f"s0_u{u}.perfil : " + "".join(names[k] + " " for k in s) + ": " + fmt(sc)
                    for u, s, sc in zip(utts, CC.strings(word, begin, lens), score)]
            rc, text = run(BIN[d.full], tmp, args, env)
            assert rc == 0, text[-2000:]
            assert [l for l in text.replace("\r", "").split("\n") if l.startswith("s0_u")] == want
            rep = open(os.path.join(tmp, "report.txt")).read().split("\n")
            assert "Connected word recognition" in rep[0] and f"word penalty {p:g}" in rep[0]
            assert rep[1:1 + len(want)] == want and rep[1 + len(want):] == [""]
        # several model sets with the variable set: refused
        rc, text = run(BIN[d.full], tmp, ["2", "models.txt", "models.txt", "1", "1"] + lists + lists +
                       ["words.txt", "report2.txt"], {"GHMM_CONNECTED": "1"})
        assert rc == 1 and "exactly one model set" in text and not os.path.exists(os.path.join(tmp, "report2.txt"))
        # without the variable: the isolated-word recogniser as it was, the expectations of the existing
        # command-line tests: every printed score is the %f of the batched score of that word, the
        # rankings are the bubble sort's, the report is the isolated-word one
        ctx_scores = (ctx.score_full_streams_batch if d.full else ctx.score_streams_batch)(dms, corpora)
        texts = []
        for env in ({}, {"GHMM_CONNECTED": "0"}, {"GHMM_WORD_PENALTY": "-5"}):
            rc, text = run(BIN[d.full], tmp, args, env)
            assert rc == 0, text[-2000:]
            texts.append(text)
            assert open(os.path.join(tmp, "report.txt")).read().startswith("Isolated word recognition")
        assert texts[0] == texts[1] == texts[2]
        blocks = spoken_blocks(texts[0])
        assert [b["spoken"] for b in blocks] == [names[case.spoken[u][0]] for u in utts]
        for u, blk in enumerate(blocks):
            order = bubble(ctx_scores[:, u])
            assert [w for w, _ in blk["ranking"]] == [names[k] for k in order], u
            for k, (_, txt) in zip(order, blk["ranking"]):
                assert txt.lstrip("-") == fmt(ctx_scores[k, u]).lstrip("-") if np.isnan(ctx_scores[k, u]) \
                    else txt == fmt(ctx_scores[k, u]), (u, names[k], txt)
    finally:
        for o in [m for w in dms for m in w] + corpora:
            o.close()
