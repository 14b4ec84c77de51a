"""Several-stream vocabularies on the GPU: ghmm_viterbi_full_streams, the three ghmm_*_full_streams_batch
calls, ghmm_recognise_full_streams (k_vocab_best, k_viterbi_pick) and the recogniser's command line on
the batched path — GPU box only.  The calls add no arithmetic, so nothing here has a tolerance: every
comparison is bit for bit (NaN in the same places), against calls with parity tests of their own
(ghmm_viterbi_full, ghmm_score_full_streams, ghmm_logscore_full_streams, the *_full_batch calls) or
against oracle_lib.viterbi_lattice on the device's own log b (fullcov_support.check_viterbi_lattice).
The vocabularies are fullvocab_cases.py's; test_fullvocab_host.py shows on the CPU that they hold finite
scores, several winners, utterances no word can end and an exact tie."""
import json
import os
import subprocess

import numpy as np
import pytest

import fullstreams_ref as S
import fullvocab_cases as V
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import (RECOGNISE, bubble, check_blocks, check_viterbi_lattice, code, fmt, offsets, rand_fmodel,
                             spoken_blocks, walk_any)
from streams_util import second_stream

pytestmark = pytest.mark.gpu

P2 = json.load(open(os.path.join(GOLDEN, "fullstreams_p2.json")))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


class Device:
    """a case's device models (fms[k][p]) and corpora, and what the per-word calls give, computed once:
    ref["lin" | "log0" | "log1" | "vit"][k] = the scores of word k alone, ref["path"][k] its Viterbi paths,
    ref["b"][k] / ref["logb"][k] = GHMM_BUF_B after its score_full_streams / viterbi_full_streams"""

    def __init__(self, G, ctx, case):
        self.case = case
        self.fms = [[ctx.full_model(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        r = self.ref = {k: [] for k in ("lin", "log0", "log1", "vit", "path", "b", "logb")}
        for fm, N in zip(self.fms, case.Ns):
            r["lin"].append(ctx.score_full_streams(fm, self.corpora))
            r["b"].append(ctx.fetch(G.BUF_B, (case.F, N)))
            r["log0"].append(ctx.logscore_full_streams(fm, self.corpora))
            r["log1"].append(ctx.logscore_full_streams(fm, self.corpora, final_state=True))
            path, score = ctx.viterbi_full_streams(fm, self.corpora)
            r["path"].append(path)
            r["vit"].append(score)
            r["logb"].append(ctx.fetch(G.BUF_B, (case.F, N)))
        for key in ("lin", "log0", "log1", "vit"):
            r[key] = np.array(r[key])
            r[key].setflags(write=False)

    def close(self):
        for o in [m for w in self.fms for m in w] + self.corpora:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    """Device per vocabulary name (and name + "-p1": stream 0 alone), built on first use"""
    made = {}

    def get(name):
        if name not in made:
            case = V.make(G, name[:-3]).stream0() if name.endswith("-p1") else V.make(G, name)
            made[name] = Device(G, ctx, case)
        return made[name]
    yield get
    for d in made.values():
        d.close()


# ------------------------------------------------------------- ghmm_viterbi_full_streams

@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_viterbi_streams_is_the_lattice_on_the_summed_log_b(G, ctx, devices, name):
    """GHMM_BUF_B = the numpy sum in stream order of the log b ghmm_viterbi_full leaves for every stream
    alone; path and score = the oracle lattice on it with stream 0's A"""
    d = devices(name)
    case = d.case
    finite = 0
    for k, (fm, hms, N) in enumerate(zip(d.fms, case.words, case.Ns)):
        parts = []
        for p in range(case.P):
            ctx.viterbi_full(fm[p], d.corpora[p])
            parts.append(ctx.fetch(G.BUF_B, (case.F, N)))
        assert same(d.ref["logb"][k], S.fold(parts, log=True)), k
        check_viterbi_lattice(hms[0].A, d.ref["logb"][k], case.lens, d.ref["path"][k], d.ref["vit"][k])
        finite += int(np.isfinite(d.ref["vit"][k][case.lens >= N]).sum())
    assert finite >= 2


def test_viterbi_streams_of_one_stream_is_viterbi_full(G, ctx, devices):
    d = devices("narrow")
    for fm, N in zip(d.fms, d.case.Ns):
        want = ctx.viterbi_full(fm[1], d.corpora[1]) + (ctx.fetch(G.BUF_B, (d.case.F, N)),)
        got = ctx.viterbi_full_streams([fm[1]], [d.corpora[1]]) + (ctx.fetch(G.BUF_B, (d.case.F, N)),)
        assert all(same(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------- the three batch calls

def check_workspace(G, ctx, d, per_word):
    """GHMM_BUF_B is [F][NS], word k's columns what the per-word call left"""
    case = d.case
    b = ctx.fetch(G.BUF_B, (case.F, case.NS))
    for k in range(case.K):
        assert same(b[:, case.bo[k]:case.bo[k + 1]], per_word[k]), k


@pytest.mark.parametrize("name", V.ALL)
def test_batch_rows_are_the_per_word_calls(G, ctx, devices, name):
    d = devices(name)
    r = d.ref
    assert same(ctx.score_full_streams_batch(d.fms, d.corpora), r["lin"])
    check_workspace(G, ctx, d, r["b"])
    assert same(ctx.logscore_full_streams_batch(d.fms, d.corpora), r["log0"])
    check_workspace(G, ctx, d, r["logb"])
    assert same(ctx.logscore_full_streams_batch(d.fms, d.corpora, final_state=True), r["log1"])
    assert same(ctx.viterbi_full_streams_batch(d.fms, d.corpora), r["vit"])
    check_workspace(G, ctx, d, r["logb"])
    if name == "far":       # the linear batch repeats the per-word -inf / NaN, the log batch is finite
        assert not np.isfinite(r["lin"][0, 0]) and np.all(r["b"][0][5] == 0.0)
        assert np.isfinite(r["log0"]).all() and np.isfinite(r["log1"]).all()
    else:
        long_enough = np.array([[T >= N for T in d.case.lens] for N in d.case.Ns])
        assert np.isfinite(r["vit"][long_enough]).sum() >= 2 and np.isfinite(r["log1"][long_enough]).sum() >= 2


@pytest.mark.parametrize("name", ["narrow-p1", "mixed-p1"])
def test_batch_of_one_stream_is_the_single_stream_batch(G, ctx, devices, name):
    d = devices(name)
    flat, corpus = [w[0] for w in d.fms], d.corpora[0]
    shape = (d.case.F, d.case.NS)
    for streams, single, kw in ((ctx.score_full_streams_batch, ctx.score_full_batch, {}),
                                (ctx.logscore_full_streams_batch, ctx.logscore_full_batch, {"final_state": False}),
                                (ctx.logscore_full_streams_batch, ctx.logscore_full_batch, {"final_state": True}),
                                (ctx.viterbi_full_streams_batch, ctx.viterbi_full_batch, {})):
        want = (single(flat, corpus, **kw), ctx.fetch(G.BUF_B, shape))
        got = (streams(d.fms, d.corpora, **kw), ctx.fetch(G.BUF_B, shape))
        assert same(got[0], want[0]) and same(got[1], want[1]), single.__name__


# ------------------------------------------------------------- ghmm_recognise_full_streams

@pytest.mark.parametrize("name", ["narrow", "mixed", "mixed-tie", "wide", "far", "narrow-p1", "wide-p1"])
def test_recognise(G, ctx, devices, name):
    d = devices(name)
    case, r = d.case, d.ref
    word, path, score = ctx.recognise_full_streams(d.fms, d.corpora)
    assert same(score, r["vit"]) and same(score, ctx.viterbi_full_streams_batch(d.fms, d.corpora))
    assert same(word, V.winners(score))
    off = offsets(case.lens)
    for u in range(case.U):
        assert same(path[off[u]:off[u + 1]], r["path"][word[u]][off[u]:off[u + 1]]), u
    check_workspace(G, ctx, d, r["logb"])
    empty = case.lens == 0
    assert np.all(score[:, empty] == 0.0) and not np.signbit(score[:, empty]).any() and np.all(word[empty] == 0)
    hopeless = np.all(score == -np.inf, axis=0)
    assert np.all(word[hopeless] == 0)
    if not name.startswith("far"):
        assert hopeless.any() and len(set(word[~hopeless & ~empty].tolist())) >= 2
    if name == "mixed-tie":
        tie = (score[0] == score[3]) & (score[0] == score.max(0)) & np.isfinite(score[0]) & ~empty
        assert tie.any() and np.all(word[tie] == 0) and 3 not in word
    assert all(same(a, b) for a, b in zip(ctx.recognise_full_streams(d.fms, d.corpora), (word, path, score)))


# ------------------------------------------------------------- launches, reproducibility

def test_launch_counts_and_a_second_call(G, ctx, devices):
    """2 P + 1 launches per batch call (the P gathers are not timed: P emissions and the lattice), P + 1
    for viterbi_full_streams, and two more under GHMM_K_VITERBI for recognise; a second identical call
    repeats every byte"""
    d = devices("narrow")
    P = d.case.P
    calls = [
        (lambda: ctx.score_full_streams_batch(d.fms, d.corpora), {"emission": P, "forward": 1}),
        (lambda: ctx.logscore_full_streams_batch(d.fms, d.corpora), {"emission": P, "forward": 1}),
        (lambda: ctx.viterbi_full_streams_batch(d.fms, d.corpora), {"emission": P, "viterbi": 1}),
        (lambda: ctx.viterbi_full_streams(d.fms[1], d.corpora), {"emission": P, "viterbi": 1}),
        (lambda: ctx.recognise_full_streams(d.fms, d.corpora), {"emission": P, "viterbi": 3}),
    ]
    for call, want in calls:
        first = call()
        ctx.set_option(G.OPT_TIMING, 1)
        ctx.kernel_times_reset()
        try:
            second = call()
            kt = {k: n for k, (_, n) in ctx.kernel_times().items() if n}
        finally:
            ctx.set_option(G.OPT_TIMING, 0)
        assert kt == want
        pairs = zip(first, second) if isinstance(first, tuple) else [(first, second)]
        assert all(same(a, b) for a, b in pairs)


def test_a_single_stream_call_in_between_changes_nothing(G, ctx, devices):
    """the workspace and the cached vocabularies are rebuilt by every call: a Viterbi of another model on
    another corpus, and a single-stream batch of other words, between two calls leave them bit-equal"""
    d, o = devices("mixed"), devices("narrow-p1")
    rng = np.random.default_rng(5)
    other = rand_fmodel(G, rng, 7, 2, 4, spread=1.0, asym=False)
    ofm, oc = ctx.full_model(other), ctx.corpus(walk_any(rng, other, [50, 20]), [50, 20])
    try:
        def once():
            out = list(ctx.recognise_full_streams(d.fms, d.corpora))
            out.append(ctx.fetch(G.BUF_B, (d.case.F, d.case.NS)))
            out.append(ctx.score_full_streams_batch(d.fms, d.corpora))
            return out
        first = once()
        ctx.viterbi_full(ofm, oc)
        ctx.viterbi_full_batch([w[0] for w in o.fms], o.corpora[0])
        assert all(same(a, b) for a, b in zip(once(), first))
        # the diagonal row API refuses the workspace after each of the new calls
        dm = ctx.model(G.synth_start_model(*G.synth_truth(3, 1, 9)))
        for call in (lambda: ctx.viterbi_full_streams(d.fms[0], d.corpora),
                     lambda: ctx.score_full_streams_batch(d.fms, d.corpora),
                     lambda: ctx.logscore_full_streams_batch(d.fms, d.corpora),
                     lambda: ctx.viterbi_full_streams_batch(d.fms, d.corpora),
                     lambda: ctx.recognise_full_streams(d.fms, d.corpora)):
            call()
            assert code(G, lambda: ctx.forward(dm, d.corpora[0])) == G.ERR_ARG
        dm.close()
    finally:
        ofm.close(); oc.close()


# ------------------------------------------------------------- refusals

class Raw:
    """the five calls through the C ABI on caller-owned destinations pre-filled with a pattern, so that a
    refusal can be seen to have written nothing"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.lib = G, ctx, ctx.lib
        self.score = np.full((case.K, case.U), -777.0)
        self.word = np.full(case.U, -7, dtype=np.int32)
        self.path = np.full(max(case.F, 1), -7, dtype=np.int32)

    def untouched(self):
        return np.all(self.score == -777.0) and np.all(self.word == -7) and np.all(self.path == -7)

    def calls(self, vocab, K, corpora, P, dest=True):
        """[(name, return code)] of the four vocabulary calls; vocab / corpora: ctypes arrays or None"""
        G, lib, h = self.G, self.lib, self.ctx.h
        dp, ip = G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_int32)
        sc = self.score.ctypes.data_as(dp) if dest else None
        wd = self.word.ctypes.data_as(ip) if dest else None
        pa = self.path.ctypes.data_as(ip) if dest else None
        return [("score", lib.ghmm_score_full_streams_batch(h, vocab, K, corpora, P, sc)),
                ("logscore", lib.ghmm_logscore_full_streams_batch(h, vocab, K, corpora, P, 0, sc)),
                ("viterbi", lib.ghmm_viterbi_full_streams_batch(h, vocab, K, corpora, P, sc)),
                ("recognise", lib.ghmm_recognise_full_streams(h, vocab, K, corpora, P, wd, pa, sc))]

    def viterbi(self, models, corpora, P, dest=True):
        G = self.G
        dp, ip = G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_int32)
        return self.lib.ghmm_viterbi_full_streams(self.ctx.h, models, corpora, P,
                                                  self.path.ctypes.data_as(ip) if dest else None,
                                                  self.score.ctypes.data_as(dp) if dest else None)


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
    flat = [m for w in d.fms for m in w]
    h0, h1 = case.words[1]
    other_n = ctx.full_model(rand_fmodel(G, rng, h1.N + 1, h1.M, h1.D, spread=1.0, asym=False))
    other_m = ctx.full_model(rand_fmodel(G, rng, h1.N, h1.M + 1, h1.D, spread=1.0, asym=False))
    other_d = ctx.full_model(rand_fmodel(G, rng, h1.N, h1.M, h1.D + 1, spread=1.0, asym=False))
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
        word1 = handles(G, d.fms[1])
        assert raw.viterbi(None, corpora, P) == arg and raw.viterbi(word1, None, P) == arg
        assert raw.viterbi(word1, corpora, P, dest=False) == arg
        assert raw.viterbi(handles(G, d.fms[1], 9), handles(G, d.corpora, 9), 9) == arg
        assert raw.viterbi(handles(G, d.fms[1], 9), handles(G, d.corpora, 9), 0) == arg
        assert raw.viterbi(handles(G, [d.fms[1][0], None]), corpora, P) == arg
        assert raw.viterbi(handles(G, [d.fms[1][0], other_n]), corpora, P) == arg
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
        assert same(raw.score, d.ref["vit"]) and same(raw.word, V.winners(raw.score))
    finally:
        for o in (other_n, other_m, other_d, other_len, other_u, other_cd):
            o.close()


def test_empty_corpus_touches_nothing(G, ctx, devices):
    d = devices("mixed")
    empty = [ctx.corpus(np.zeros((0, w.D)), np.zeros(0, dtype=np.int32)) for w in d.case.words[0]]
    raw = Raw(G, ctx, d.case)
    vocab, corpora = handles(G, [m for w in d.fms for m in w]), handles(G, empty)
    try:
        for dest in (True, False):
            assert all(rc == G.OK for _, rc in raw.calls(vocab, d.case.K, corpora, d.case.P, dest=dest))
            assert raw.viterbi(handles(G, d.fms[0]), corpora, d.case.P, dest=dest) == G.OK
        assert raw.untouched()
    finally:
        for c in empty:
            c.close()


# ------------------------------------------------------------- the command line

def test_recogniser_takes_the_batched_path_and_prints_the_recorded_ranking(G, ctx, tmp_path):
    """the 13 recorded two-stream word models agree per stream in M and D, so the command line scores
    them with ghmm_score_full_streams_batch (GHMM_LOG_SCORE=1: the log call).  Its text is the
    model-by-model loop's, byte for byte: every printed score is the %f of ghmm_score_full_streams
    (ghmm_logscore_full_streams) of that word; and it is the recorded ranking under check_blocks"""
    tmp = str(tmp_path)
    models = np.load(os.path.join(GOLDEN, "fullstreams_models.npz"))
    words, ref = P2["words"], P2["recog"]
    Xs, lens = S.bundled_streams(G, GOLDEN, P2["mean_list"], range(13))
    lists = []
    for s, prefix in ((1, ""), (2, "d_")):
        for fn in P2["mean_list"]:
            X = G.perfil_read(os.path.join(GOLDEN, "perfil", fn))
            G.perfil_write(os.path.join(tmp, prefix + fn), X if s == 1 else second_stream(X))
        lists.append(f"rec_{s}.txt")
        open(os.path.join(tmp, lists[-1]), "w").write("\n".join(prefix + fn for fn in P2["mean_list"][:13]) + "\n")
    vocab = []
    for w in words:
        vocab.append([G.HostFullModel(models[f"{w}.A"],
                                      *(models[f"{w}.s{s}.{k}"] for k in ("c", "mean", "inv_cov", "det")), word=w)
                      for s in range(2)])
        G.HostFullModel.write_streams(os.path.join(tmp, w + ".hmm"), vocab[-1])
    assert len({tuple((h.M, h.D) for h in hms) for hms in vocab}) == 1      # test_main.c's condition for batching
    open(os.path.join(tmp, "models.txt"), "w").write("\n".join(w + ".hmm" for w in words) + "\n")
    open(os.path.join(tmp, "words.txt"), "w").write("\n".join(words) + "\n")
    # what the model-by-model loop scores (the files hold the models' doubles as they are)
    fms = [[ctx.full_model(h) for h in G.HostFullModel.read_streams(os.path.join(tmp, w + ".hmm"))] for w in words]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    try:
        loop = {False: np.array([ctx.score_full_streams(fm, corpora) for fm in fms]),
                True: np.array([ctx.logscore_full_streams(fm, corpora) for fm in fms])}
    finally:
        for o in [m for fm in fms for m in fm] + corpora:
            o.close()
    for log in (False, True):
        p = subprocess.run([RECOGNISE, "1", "models.txt", "1"] + lists + ["words.txt", "report.txt"], cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                           env=dict(os.environ, **({"GHMM_LOG_SCORE": "1"} if log else {})))
        text = p.stdout.decode(errors="replace")
        assert p.returncode == 0, text[-2000:]
        blocks = spoken_blocks(text)
        assert [b["spoken"] for b in blocks] == [b["spoken"] for b in ref["blocks"]]
        for u, blk in enumerate(blocks):
            order = bubble(loop[log][:, u])
            assert [w for w, _ in blk["ranking"]] == [words[k] for k in order], (log, u)
            for k, (_, txt) in zip(order, blk["ranking"]):
                assert txt.lstrip("-") == fmt(loop[log][k, u]).lstrip("-") if np.isnan(loop[log][k, u]) \
                    else txt == fmt(loop[log][k, u]), (log, u, words[k], txt)
        if not log:
            check_blocks(loop[log], words, ref["blocks"])
        else:
            assert np.isfinite(loop[log]).all()
