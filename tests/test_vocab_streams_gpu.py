"""Several-stream vocabularies of diagonal models on the GPU: ghmm_viterbi_streams, ghmm_score_streams_batch,
ghmm_viterbi_streams_batch, ghmm_recognise_streams (k_add_streams and the diagonal front end of
k_forward_multi, k_viterbi_multi, k_vocab_best, k_viterbi_pick) and the recogniser's command line on the
batched path — GPU box only.  The vocabularies and their float64 references are vocab_cases.py's;
test_vocab_host.py shows on the CPU that they are not vacuous and keep the margins under which a path
or a winner that differs from the reference cannot be blamed on rounding.

  default kernels        every score within 1e-10 relative of the oracle (fuzz_viterbi_case's bar) or the
                         reference's non-finite value itself, every path and winner equal to the oracle's;
                         ghmm_score_streams_batch within 1e-9 of oracle_lib.score_streams and within 1e-12
                         of the ghmm_score_streams loop
  GHMM_OPT_KERNELS = 1   every state's log b comes from its own Gaussians alone: the vocabulary calls are
                         bit for bit the per-word calls, and the tie case runs (only) here"""
import json
import os
import subprocess

import numpy as np
import pytest

import vocab_cases as V
from _load import PKG_DIR
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import assert_close, bubble, check_viterbi_lattice, code, fmt, offsets, spoken_blocks
from fullstreams_ref import fold
from streams_util import _golden_streams, _stream_data, assert_frames, second_stream, synth_case

pytestmark = pytest.mark.gpu

RECOGNISE = os.path.join(PKG_DIR, "bin", "recognition-continuous-test-fs")


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
    """a case's device models (dms[k][p]) and corpora, its oracle reference, and what the per-word calls
    give under a kernel tier, computed once: per_word(tier) = {"path": [k] -> F, "vit": [K][U],
    "logb": [k] -> [F][N_k], "fwd": [K][U] (the ghmm_score_streams loop)}"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        self.ref = V.Reference(case)
        self.dms = [[ctx.model(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self._per_word = {}

    def per_word(self, tier):
        if tier not in self._per_word:
            G, ctx, case = self.G, self.ctx, self.case
            r = {"path": [], "vit": [], "logb": [], "fwd": []}
            for dm, N in zip(self.dms, case.Ns):
                path, score = ctx.viterbi_streams(dm, self.corpora)
                r["path"].append(path)
                r["vit"].append(score)
                r["logb"].append(ctx.fetch(G.BUF_B, (case.F, N)))
                r["fwd"].append(ctx.score_streams(dm, self.corpora))
            r["vit"], r["fwd"] = np.array(r["vit"]), np.array(r["fwd"])
            for a in [r["vit"], r["fwd"]] + r["path"] + r["logb"]:
                a.setflags(write=False)
            self._per_word[tier] = r
        return self._per_word[tier]

    def close(self):
        for o in [m for w in self.dms for m in w] + self.corpora:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    """Device per vocabulary name (name + "-p1": stream 0 alone), built on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(G, ctx, V.make(G, name))
        return made[name]
    yield get
    for d in made.values():
        d.close()


class vector_kernels:
    """GHMM_OPT_KERNELS = 1 inside, the default again afterwards"""

    def __init__(self, G, ctx):
        self.G, self.ctx = G, ctx

    def __enter__(self):
        self.ctx.set_option(self.G.OPT_KERNELS, 1)

    def __exit__(self, *exc):
        self.ctx.set_option(self.G.OPT_KERNELS, 0)


def check_workspace(G, ctx, d, per_word):
    """GHMM_BUF_B is [F][NS], word k's columns bit for bit what the per-word call left"""
    case = d.case
    b = ctx.fetch(G.BUF_B, (case.F, case.NS))
    for k in range(case.K):
        assert same(b[:, case.bo[k]:case.bo[k + 1]], per_word[k]), k


def check_paths(case, word, path, paths_of):
    off = offsets(case.lens)
    for u in range(case.U):
        assert same(path[off[u]:off[u + 1]], paths_of[word[u]][off[u]:off[u + 1]]), u


# ------------------------------------------------------------- 1. against the oracle, default kernels

@pytest.mark.parametrize("name", ["narrow", "mixed", "wide", "one70"])
def test_viterbi_streams_against_the_oracle(G, ctx, devices, name):
    d = devices(name)
    case, ref, r = d.case, d.ref, d.per_word(0)
    scores_close(r["vit"], ref.vit)
    for k in range(case.K):
        assert same(r["path"][k], ref.paths[k]), k
        if case.F:
            assert_frames(r["logb"][k], ref.logb[k], f"{name} word {k} log b")
    assert np.isfinite(ref.vit).sum() >= 1


@pytest.mark.parametrize("name", ["narrow", "mixed", "wide", "narrow-p1", "mixed-p1"])
def test_tables_against_the_oracle(G, ctx, devices, name):
    d = devices(name)
    case, ref = d.case, d.ref
    table = ctx.viterbi_streams_batch(d.dms, d.corpora)
    scores_close(table, ref.vit)
    b = ctx.fetch(G.BUF_B, (case.F, case.NS))       # the words' columns of log b, against the oracle's
    for k in range(case.K):
        assert_frames(b[:, case.bo[k]:case.bo[k + 1]], ref.logb[k], f"{name} word {k} columns of log b")
    word, path, score = ctx.recognise_streams(d.dms, d.corpora)
    assert same(score, table)
    assert same(word, ref.words) and same(word, V.winners(score))
    check_paths(case, word, path, ref.paths)
    empty = case.lens == 0
    assert np.all(score[:, empty] == 0.0) and not np.signbit(score[:, empty]).any() and np.all(word[empty] == 0)
    hopeless = np.all(score == -np.inf, axis=0)
    assert hopeless.any() and np.all(word[hopeless] == 0)
    assert len(set(word[~hopeless & ~empty].tolist())) >= 2
    # the forward scores: the oracle at streams_util's bar, the word-by-word loop at ghmm_score_batch's
    fwd = ctx.score_streams_batch(d.dms, d.corpora)
    assert_close(fwd, V.forward_table(case), rtol=1e-9, what=name + " score_streams_batch against the oracle")
    assert_close(fwd, d.per_word(0)["fwd"], rtol=1e-12, what=name + " score_streams_batch against the loop")
    assert np.all(fwd[:, empty] == 0.0)


def test_a_product_that_underflows_scores_like_the_loop(G, ctx, devices):
    """frame 5 of utterance 0: each stream's densities are positive, their product is 0 in every state"""
    d = devices("far")
    loop = d.per_word(0)["fwd"]
    fwd = ctx.score_streams_batch(d.dms, d.corpora)
    b = ctx.fetch(G.BUF_B, (d.case.F, d.case.NS))
    assert np.all(b[5, :d.case.Ns[0]] == 0.0) and not np.isfinite(loop[0, 0])
    assert_close(fwd, loop, rtol=1e-12, what="far: score_streams_batch against the loop")
    assert np.isfinite(fwd[:, 1]).all()
    scores_close(ctx.viterbi_streams_batch(d.dms, d.corpora), d.ref.vit)    # the log b stays finite
    assert np.isfinite(d.ref.vit).all()


# ------------------------------------------------------------- 2. bit for bit, GHMM_OPT_KERNELS = 1

@pytest.mark.parametrize("name", ["narrow", "mixed", "mixed-tie", "wide", "mixed-p1"])
def test_vocabulary_calls_are_the_per_word_calls_bit_for_bit(G, ctx, devices, name):
    d = devices(name)
    case = d.case
    with vector_kernels(G, ctx):
        r = d.per_word(1)
        table = ctx.viterbi_streams_batch(d.dms, d.corpora)
        assert same(table, r["vit"])                        # row k = ghmm_viterbi_streams' score of word k
        check_workspace(G, ctx, d, r["logb"])
        word, path, score = ctx.recognise_streams(d.dms, d.corpora)
        assert same(score, table) and same(word, V.winners(score))
        check_paths(case, word, path, r["path"])
        check_workspace(G, ctx, d, r["logb"])
        assert all(same(a, b) for a, b in zip(ctx.recognise_streams(d.dms, d.corpora), (word, path, score)))
        # the lowest predecessor: the oracle's lattice on the device's own log b, bit for bit
        for k, hms in enumerate(case.words):
            check_viterbi_lattice(hms[0].A, r["logb"][k], case.lens, r["path"][k], r["vit"][k])
    if name == "mixed-tie":     # the lowest word
        empty = case.lens == 0
        tie = (score[0] == score[3]) & (score[0] == score.max(0)) & np.isfinite(score[0]) & ~empty
        assert same(score[0], score[3]) and tie.any() and np.all(word[tie] == 0) and 3 not in word
        lb = r["logb"][2]       # identical states: identical bits, every predecessor ties
        assert np.all(lb == lb[:, :1])
        off = offsets(case.lens)
        u = int(np.argmax(case.lens))
        p = r["path"][2][off[u]:off[u + 1]]
        assert np.isfinite(r["vit"][2][u]) and np.all(p[:-1] == 0) and p[-1] == case.Ns[2] - 1
    else:
        assert same(word, d.ref.words)
        scores_close(table, d.ref.vit)


# ------------------------------------------------------------- 3. the fold

@pytest.mark.parametrize("tier", [0, 1])
def test_the_summed_log_b_is_the_ieee_sum_of_the_streams_own(G, ctx, devices, tier):
    d = devices("narrow")
    case = d.case
    ctx.set_option(G.OPT_KERNELS, tier)
    try:
        for dm, N in zip(d.dms, case.Ns):
            parts = []
            for p in range(case.P):
                ctx.viterbi(dm[p], d.corpora[p])
                parts.append(ctx.fetch(G.BUF_B, (case.F, N)))
            ctx.viterbi_streams(dm, d.corpora)
            assert same(ctx.fetch(G.BUF_B, (case.F, N)), fold(parts, log=True))
    finally:
        ctx.set_option(G.OPT_KERNELS, 0)


# ------------------------------------------------------------- 4. n_streams == 1

def test_one_stream_is_the_single_stream_call(G, ctx, devices):
    d = devices("narrow")
    for dm, N in zip(d.dms, d.case.Ns):
        want = ctx.viterbi(dm[1], d.corpora[1]) + (ctx.fetch(G.BUF_B, (d.case.F, N)),)
        got = ctx.viterbi_streams([dm[1]], [d.corpora[1]]) + (ctx.fetch(G.BUF_B, (d.case.F, N)),)
        assert all(same(a, b) for a, b in zip(got, want))
    for name in ("narrow-p1", "mixed-p1"):
        d = devices(name)
        shape = (d.case.F, d.case.NS)
        want = (ctx.score_batch([w[0] for w in d.dms], d.corpora[0]), ctx.fetch(G.BUF_B, shape))
        got = (ctx.score_streams_batch(d.dms, d.corpora), ctx.fetch(G.BUF_B, shape))
        assert same(got[0], want[0]) and same(got[1], want[1]), name


def test_a_word_of_more_states_than_lanes_is_scored_word_by_word(G, ctx, devices):
    """ghmm_score_streams_batch with n_streams > 1 and a word of 70 states: the ghmm_score_streams loop itself,
    as ghmm_score_batch does with one stream (the two Viterbi calls refuse such a vocabulary)"""
    small, big = devices("mixed"), devices("one70")
    vocab, corpora = [small.dms[0], big.dms[0], small.dms[3]], big.corpora
    loop = np.array([ctx.score_streams(w, corpora) for w in vocab])
    batch, kt = timed(G, ctx, lambda: ctx.score_streams_batch(vocab, corpora))
    assert same(batch, loop) and np.isfinite(loop[1, 0])
    assert kt == {"emission": 3 * 3, "forward": 3}
    assert code(G, lambda: ctx.viterbi_streams_batch(vocab, corpora)) == G.ERR_UNSUPPORTED
    assert code(G, lambda: ctx.recognise_streams(vocab, corpora)) == G.ERR_UNSUPPORTED


# ------------------------------------------------------------- 5. launches, reproducibility

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


def test_launch_counts_and_a_second_call(G, ctx, devices):
    """2 P - 1 launches under GHMM_K_EMISSION (P emissions, P - 1 folds) and the one lattice launch; two
    more under GHMM_K_VITERBI for recognise; a second identical call repeats every byte"""
    d = devices("narrow")
    P = d.case.P
    calls = [
        (lambda: ctx.score_streams_batch(d.dms, d.corpora), {"emission": 2 * P - 1, "forward": 1}),
        (lambda: ctx.viterbi_streams_batch(d.dms, d.corpora), {"emission": 2 * P - 1, "viterbi": 1}),
        (lambda: ctx.viterbi_streams(d.dms[1], d.corpora), {"emission": 2 * P - 1, "viterbi": 1}),
        (lambda: ctx.recognise_streams(d.dms, d.corpora), {"emission": 2 * P - 1, "viterbi": 3}),
    ]
    for call, want in calls:
        first = call()
        second, kt = timed(G, ctx, call)
        assert kt == want
        pairs = zip(first, second) if isinstance(first, tuple) else [(first, second)]
        assert all(same(a, b) for a, b in pairs)


def test_other_calls_in_between_change_nothing(G, ctx, devices):
    """the workspace and the cached vocabularies are rebuilt by every call: another model's single-stream
    calls and another vocabulary's ghmm_score_batch between two calls leave them bit-equal"""
    d, o = devices("mixed"), devices("narrow-p1")
    hm, X, lens = synth_case(G, 7, 2, 4, [50, 20])
    om, oc = ctx.model(hm), ctx.corpus(X, lens)
    try:
        def once():
            out = list(ctx.recognise_streams(d.dms, d.corpora))
            out.append(ctx.fetch(G.BUF_B, (d.case.F, d.case.NS)))
            out.append(ctx.score_streams_batch(d.dms, d.corpora))
            out.append(ctx.fetch(G.BUF_B, (d.case.F, d.case.NS)))
            return out
        first = once()
        ctx.viterbi(om, oc)
        ctx.score(om, oc)
        ctx.score_batch([w[0] for w in o.dms], o.corpora[0])
        assert all(same(a, b) for a, b in zip(once(), first))
        # the row API does not reuse the workspace, and it serves no posteriors
        for call in (lambda: ctx.viterbi_streams(d.dms[0], d.corpora),
                     lambda: ctx.score_streams_batch(d.dms, d.corpora),
                     lambda: ctx.viterbi_streams_batch(d.dms, d.corpora),
                     lambda: ctx.recognise_streams(d.dms, d.corpora)):
            call()
            assert code(G, lambda: ctx.forward(d.dms[0][0], d.corpora[0])) == G.ERR_ARG
            assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
    finally:
        om.close(); oc.close()


# ------------------------------------------------------------- 6. refusals

class Raw:
    """the four calls through the C ABI on caller-owned destinations pre-filled with a pattern, so that a
    refusal can be seen to have written nothing"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.lib = G, ctx, ctx.lib
        self.score = np.full((case.K, case.U), -777.0)
        self.word = np.full(case.U, -7, dtype=np.int32)
        self.path = np.full(max(case.F, 1), -7, dtype=np.int32)

    def untouched(self):
        return np.all(self.score == -777.0) and np.all(self.word == -7) and np.all(self.path == -7)

    def _dest(self, dest):
        G = self.G
        dp, ip = G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_int32)
        if not dest:
            return None, None, None
        return self.score.ctypes.data_as(dp), self.word.ctypes.data_as(ip), self.path.ctypes.data_as(ip)

    def calls(self, vocab, K, corpora, P, dest=True, only=("score", "viterbi", "recognise")):
        """[(name, return code)] of the three vocabulary calls; vocab / corpora: ctypes arrays or None"""
        lib, h = self.lib, self.ctx.h
        sc, wd, pa = self._dest(dest)
        fns = {"score": lambda: lib.ghmm_score_streams_batch(h, vocab, K, corpora, P, sc),
               "viterbi": lambda: lib.ghmm_viterbi_streams_batch(h, vocab, K, corpora, P, sc),
               "recognise": lambda: lib.ghmm_recognise_streams(h, vocab, K, corpora, P, wd, pa, sc)}
        return [(name, fns[name]()) for name in only]

    def viterbi(self, models, corpora, P, dest=True):
        sc, _, pa = self._dest(dest)
        return self.lib.ghmm_viterbi_streams(self.ctx.h, models, corpora, P, pa, sc)


def handles(G, objs, n=None):
    objs = list(objs)
    return (G.C.c_void_p * (n or len(objs)))(*[objs[i % len(objs)].h if objs[i % len(objs)] is not None else None
                                               for i in range(n or len(objs))])


def test_refusals_write_nothing(G, ctx, devices):
    d = devices("mixed")
    case = d.case
    K, P = case.K, case.P
    rng = np.random.default_rng(9)
    raw = Raw(G, ctx, case)
    flat = [m for w in d.dms for m in w]
    h1 = case.words[1][1]

    def model(N, M, D):
        return ctx.model(V.rand_model(G, rng, N, M, D, case.words[1][0].A if N == h1.N else np.eye(N)))
    other_n, other_m, other_d = model(h1.N + 1, h1.M, h1.D), model(h1.N, h1.M + 1, h1.D), model(h1.N, h1.M, h1.D + 1)
    big = [model(65, w.M, w.D) for w in case.words[0]]
    lens2 = case.lens.copy()
    lens2[3] += 1
    lens2[4] -= 1
    other_len = ctx.corpus(case.Xs[1], lens2)
    other_u = ctx.corpus(case.Xs[1], np.concatenate([case.lens[:-2], [case.lens[-2:].sum()]]))
    other_cd = ctx.corpus(np.zeros((case.F, h1.D + 2)), case.lens)
    vocab, corpora = handles(G, flat), handles(G, d.corpora)

    def swapped(i, m):
        return handles(G, flat[:i] + [m] + flat[i + 1:])
    try:
        arg, unsupported = G.ERR_ARG, G.ERR_UNSUPPORTED
        cases = [
            ("null vocabulary", None, K, corpora, P, arg),
            ("null corpora", vocab, K, None, P, arg),
            ("null model", swapped(3, None), K, corpora, P, arg),
            ("null corpus", vocab, K, handles(G, [d.corpora[0], None]), P, arg),
            ("K = 0", vocab, 0, corpora, P, arg),
            ("K < 0", vocab, -1, corpora, P, arg),
            ("P = 0", handles(G, flat, 9 * K), K, handles(G, d.corpora, 9), 0, arg),
            ("P = 9", handles(G, flat, 9 * K), K, handles(G, d.corpora, 9), 9, arg),
            ("P < 0", handles(G, flat, 9 * K), K, handles(G, d.corpora, 9), -1, arg),
            ("streams of a word differ in N", swapped(3, other_n), K, corpora, P, arg),
            ("corpora differ in a length", vocab, K, handles(G, [d.corpora[0], other_len]), P, arg),
            ("corpora differ in U", vocab, K, handles(G, [d.corpora[0], other_u]), P, arg),
            ("a corpus of another D", vocab, K, handles(G, [d.corpora[0], other_cd]), P, arg),
            ("words differ in M_1", swapped(3, other_m), K, corpora, P, unsupported),
            ("words differ in D_1", swapped(3, other_d), K, corpora, P, unsupported),
        ]
        for what, v, k, c, p, want in cases:
            for fn, rc in raw.calls(v, k, c, p):
                assert rc == want, (what, fn, rc)
        for fn, rc in raw.calls(vocab, K, corpora, P, dest=False):
            assert rc == arg, ("null destination", fn, rc)
        # a word of more than 64 states: refused by the two Viterbi vocabulary calls alone
        for fn, rc in raw.calls(handles(G, flat[:P] + big), 2, corpora, P, only=("viterbi", "recognise")):
            assert rc == unsupported, ("a word of 65 states", fn, rc)
        word1 = handles(G, d.dms[1])
        assert raw.viterbi(None, corpora, P) == arg and raw.viterbi(word1, None, P) == arg
        assert raw.viterbi(word1, corpora, P, dest=False) == arg
        assert raw.viterbi(handles(G, d.dms[1], 9), handles(G, d.corpora, 9), 9) == arg
        assert raw.viterbi(handles(G, d.dms[1], 9), handles(G, d.corpora, 9), 0) == arg
        assert raw.viterbi(handles(G, [d.dms[1][0], None]), corpora, P) == arg
        assert raw.viterbi(handles(G, [d.dms[1][0], other_n]), corpora, P) == arg
        assert raw.viterbi(word1, handles(G, [d.corpora[0], other_len]), P) == arg
        assert raw.viterbi(word1, handles(G, [d.corpora[0], other_cd]), P) == arg
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            for fn, rc in raw.calls(vocab, K, corpora, P):
                assert rc == unsupported, ("robust", fn, rc)
            assert raw.viterbi(word1, corpora, P) == unsupported
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert raw.untouched()
        raw.calls(swapped(3, other_m), K, corpora, P)
        assert "every model must have the same M and D" in ctx.lib.ghmm_last_error().decode()
        assert "stream 1" in ctx.lib.ghmm_last_error().decode()
        # and the same arguments, valid, do write
        assert all(rc == G.OK for _, rc in raw.calls(vocab, K, corpora, P))
        scores_close(raw.score, d.ref.vit)
        assert same(raw.word, V.winners(raw.score)) and np.all(raw.path[:case.F] >= 0)
    finally:
        for o in [other_n, other_m, other_d, other_len, other_u, other_cd] + big:
            o.close()


def test_empty_corpus_touches_nothing(G, ctx, devices):
    d = devices("mixed")
    empty = [ctx.corpus(np.zeros((0, w.D)), np.zeros(0, dtype=np.int32)) for w in d.case.words[0]]
    raw = Raw(G, ctx, d.case)
    vocab, corpora = handles(G, [m for w in d.dms for m in w]), handles(G, empty)
    try:
        for dest in (True, False):
            assert all(rc == G.OK for _, rc in raw.calls(vocab, d.case.K, corpora, d.case.P, dest=dest))
            assert raw.viterbi(handles(G, d.dms[0]), corpora, d.case.P, dest=dest) == G.OK
        assert raw.untouched()
    finally:
        for c in empty:
            c.close()


# ------------------------------------------------------------- 7. the command line

def test_recogniser_takes_the_batched_path_and_prints_the_loops_text(G, ctx, tmp_path):
    """the 13 recorded two-stream word models agree per stream in M and D, so the command line scores them
    with ghmm_score_streams_batch.  Its text is the model-by-model loop's: every printed score is the %f
    of ghmm_score_streams of that word, and the rankings are equal"""
    tmp = str(tmp_path)
    streams = json.load(open(os.path.join(GOLDEN, "streams_p2.json")))
    words, files = streams["words"], streams["mean_list"]
    Xs, lens = _stream_data(G, streams, range(len(files)))
    lists = []
    for s, prefix in ((1, ""), (2, "d_")):
        for fn in files:
            X = G.perfil_read(os.path.join(GOLDEN, "perfil", fn))
            G.perfil_write(os.path.join(tmp, prefix + fn), X if s == 1 else second_stream(X, streams["D2"]))
        lists.append(f"rec_{s}.txt")
        open(os.path.join(tmp, lists[-1]), "w").write("\n".join(prefix + fn for fn in files) + "\n")
    for w in words:
        G.HostModel.write_streams(os.path.join(tmp, w + ".hmm"), _golden_streams(G, streams["train13_p2"][w], word=w))
    open(os.path.join(tmp, "models.txt"), "w").write("\n".join(w + ".hmm" for w in words) + "\n")
    open(os.path.join(tmp, "words.txt"), "w").write("\n".join(words) + "\n")
    # what the model-by-model loop scores (the files hold the models' doubles as they are)
    vocab = [G.HostModel.read_streams(os.path.join(tmp, w + ".hmm")) for w in words]
    assert len({tuple((h.M, h.D) for h in hms) for hms in vocab}) == 1      # test_main.c's condition for batching
    dms = [[ctx.model(h) for h in hms] for hms in vocab]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    try:
        loop = np.array([ctx.score_streams(dm, corpora) for dm in dms])
        batch, kt = timed(G, ctx, lambda: ctx.score_streams_batch(dms, corpora))
        assert kt == {"emission": 3, "forward": 1}
        assert_close(batch, loop, rtol=1e-12, what="13 words: score_streams_batch against the loop")
    finally:
        for o in [m for dm in dms for m in dm] + corpora:
            o.close()
    p = subprocess.run([RECOGNISE, "1", "models.txt", "1"] + lists + ["words.txt", "report.txt"], cwd=tmp,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-2000:]
    blocks = spoken_blocks(text)
    assert [b["spoken"] for b in blocks] == words and len(blocks) == len(lens)
    for u, blk in enumerate(blocks):
        order = bubble(loop[:, u])
        assert [w for w, _ in blk["ranking"]] == [words[k] for k in order], u
        for k, (_, txt) in zip(order, blk["ranking"]):
            assert txt.lstrip("-") == fmt(loop[k, u]).lstrip("-") if np.isnan(loop[k, u]) \
                else txt == fmt(loop[k, u]), (u, words[k], txt)
    assert np.isfinite(loop).sum() >= len(lens)     # (the recorded table holds the reference's NaN artefacts too)
