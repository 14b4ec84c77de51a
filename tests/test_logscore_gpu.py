"""The diagonal log-domain forward score on the GPU: ghmm_logscore, ghmm_logscore_batch,
ghmm_logscore_streams, ghmm_logscore_streams_batch (k_logforward_multi behind the diagonal log emission,
k_logforward_wide beyond 64 states) and the diagonal recogniser's GHMM_LOG_SCORE=1 — GPU box only.  The
cases are logscore_cases.py's, the references logscore_ref.py's; test_logscore_host.py shows on the CPU
that they hold what is leaned on here.  Everything runs under GHMM_OPT_KERNELS = 1 and under the default
(matrix-core emission) tier.

  the lattice alone   every device score within fulllogscore_ref.lattice_bound of the long-double lattice
                      run on the device's own log b (fetch(BUF_B)), both final_state values; -inf meets
                      -inf, NaN meets NaN; no case and no utterance is left out
  end to end          against the oracle's log b and the long-double lattice: 1e-10 relative on every
                      finite score (test_vocab_streams_gpu's bar), the worst value printed
  identities          n_streams = 1, the batch rows against the single calls (bit for bit with
                      GHMM_OPT_KERNELS = 1 and for the word-by-word fall-back, 1e-12 otherwise), a second call
  contract            final_state 0 >= 1, launch counts, GHMM_BUF_POST, refusals that write nothing, 513
                      states, U = 0
  the command line    GHMM_LOG_SCORE=1 and, without it, the golden report"""
import json
import os
import subprocess

import numpy as np
import pytest

import logscore_cases as LC
import logscore_ref as R
from _load import PKG_DIR
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import bubble, code, offsets, rel_dist, spoken_blocks
from vocab_cases import rand_model

pytestmark = pytest.mark.gpu

RECOGNISE = os.path.join(PKG_DIR, "bin", "recognition-continuous-test-fs")
TIERS = (1, 0)          # GHMM_OPT_KERNELS


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class tier_of:
    """GHMM_OPT_KERNELS = tier inside, the default again afterwards"""

    def __init__(self, G, ctx, tier):
        self.G, self.ctx, self.tier = G, ctx, tier

    def __enter__(self):
        self.ctx.set_option(self.G.OPT_KERNELS, self.tier)

    def __exit__(self, *exc):
        self.ctx.set_option(self.G.OPT_KERNELS, 0)


class Device:
    """a case's device models (dms[k][p]) and corpora, its reference, and per tier what the public calls
    give, computed once: run(tier) = {"score": {fs: [K][U]}, "logb": [k] -> [F][N_k], "word": {fs: [K][U]}}
    score = the batch call's table (a single-model case: the single call), logb = its columns of GHMM_BUF_B
    (with a word of more than 64 states: what the per-word call left), word = the per-word calls' scores"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        self.ref = R.Reference(case)
        self.dms = [[ctx.model(h) for h in w] for w in case.words]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self.single = case.K == 1 and case.P == 1
        self._run = {}

    def word_call(self, k, fs):
        ctx = self.ctx
        if self.case.P == 1:
            return ctx.logscore(self.dms[k][0], self.corpora[0], final_state=bool(fs))
        return ctx.logscore_streams(self.dms[k], self.corpora, final_state=bool(fs))

    def run(self, tier):
        if tier in self._run:
            return self._run[tier]
        G, ctx, case = self.G, self.ctx, self.case
        r = {"score": {}, "word": {}, "logb": None}
        with tier_of(G, ctx, tier):
            for fs in (0, 1):
                word, logb = [], []
                for k in range(case.K):
                    word.append(self.word_call(k, fs))
                    logb.append(ctx.fetch(G.BUF_B, (case.F, case.Ns[k])))
                r["word"][fs] = np.array(word)
                if self.single:
                    r["score"][fs] = r["word"][fs]
                else:
                    r["score"][fs] = ctx.logscore_streams_batch(self.dms, self.corpora, final_state=bool(fs))
                    if max(case.Ns) <= 64:
                        b = ctx.fetch(G.BUF_B, (case.F, case.NS))
                        logb = [b[:, case.bo[k]:case.bo[k + 1]].copy() for k in range(case.K)]
                if r["logb"] is not None:       # the emission does not depend on final_state
                    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(logb, r["logb"]))
                r["logb"] = logb
        for a in list(r["score"].values()) + list(r["word"].values()) + r["logb"]:
            a.setflags(write=False)
        self._run[tier] = r
        return r

    def close(self):
        for o in [m for w in self.dms for m in w] + self.corpora:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(G, ctx, LC.make(G, name))
        return made[name]
    yield get
    for d in made.values():
        d.close()


# ------------------------------------------------------------- 1. the lattice alone

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", LC.NAMES)
def test_lattice_alone(G, ctx, devices, name, tier):
    d = devices(name)
    case, r = d.case, d.run(tier)
    for fs in (0, 1):
        worst = 0.0
        for k, hms in enumerate(case.words):
            exact, bound = R.lattice_scores(hms[0].A, r["logb"][k], case.lens, fs)
            got = r["score"][fs][k]
            rel_dist(got, exact)        # equal NaN and infinity patterns, an empty utterance's 0 met exactly
            fin = np.isfinite(exact.astype(np.float64)) & (np.asarray(case.lens) > 0)
            err = np.abs(got[fin].astype(np.longdouble) - exact[fin]).astype(np.float64)
            print(f"{name} tier {tier} final_state={fs} word {k}: error / bound",
                  np.round(err / bound[fin], 3).tolist())
            assert (err <= bound[fin]).all(), (fs, k, err, bound[fin])
            worst = max(worst, float((err / bound[fin]).max(initial=0.0)))
        print(f"{name} tier {tier} final_state={fs}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------- 2. end to end

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", LC.NAMES)
def test_end_to_end(G, ctx, devices, name, tier):
    d = devices(name)
    r = d.run(tier)
    for fs in (0, 1):
        for got in (r["score"][fs], r["word"][fs]):
            dist = rel_dist(got, d.ref.score_ld[fs])
            print(f"{name} tier {tier} final_state={fs}: worst relative error {dist:.2e}")
            assert dist <= 1e-10


# ------------------------------------------------------------- 3. identities

@pytest.mark.parametrize("tier", TIERS)
def test_one_stream_is_the_single_stream_call(G, ctx, devices, tier):
    with tier_of(G, ctx, tier):
        for name in ("lane_6x2x9_banded", "wide_65x1x4_banded"):
            d = devices(name)
            m, c, shape = d.dms[0][0], d.corpora[0], (d.case.F, d.case.Ns[0])
            for fs in (False, True):
                want = (ctx.logscore(m, c, final_state=fs), ctx.fetch(G.BUF_B, shape))
                got = (ctx.logscore_streams([m], [c], final_state=fs), ctx.fetch(G.BUF_B, shape))
                assert same(got[0], want[0]) and same(got[1], want[1]), (name, fs)
                ctx.set_option(G.OPT_ROBUST, 1)     # no effect on one stream, as in ghmm_viterbi
                try:
                    assert same(ctx.logscore(m, c, final_state=fs), want[0])
                finally:
                    ctx.set_option(G.OPT_ROBUST, 0)
        for name in ("vocab_p1", "vocab70_p1"):
            d = devices(name)
            flat = [w[0] for w in d.dms]
            for fs in (False, True):
                want = ctx.logscore_batch(flat, d.corpora[0], final_state=fs)
                assert same(ctx.logscore_streams_batch(d.dms, d.corpora, final_state=fs), want), (name, fs)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(LC.VOCAB))
def test_batch_rows_are_the_single_calls(G, ctx, devices, name, tier):
    d = devices(name)
    case, r = d.case, d.run(tier)
    for fs in (0, 1):
        batch, word = r["score"][fs], r["word"][fs]
        assert batch.shape == (case.K, case.U)
        if tier == 1 or max(case.Ns) > 64:
            assert same(batch, word), fs
        else:
            assert rel_dist(batch, word) <= 1e-12, fs
        empty = np.asarray(case.lens) == 0
        assert np.all(batch[:, empty] == 0.0) and not np.signbit(batch[:, empty]).any()
    if max(case.Ns) > 64:       # the 70-state word's row, spelled out
        assert same(r["score"][1][1], r["word"][1][1]) and np.isfinite(r["word"][1][1, 0])


@pytest.mark.parametrize("tier", TIERS)
def test_a_second_call_repeats_every_byte(G, ctx, devices, tier):
    with tier_of(G, ctx, tier):
        for name in ("lane_9x2x5_dense", "wide_130x2x5_banded", "wide_70x1x4_dense", "vocab_p2", "vocab70_p2"):
            d = devices(name)
            r = d.run(tier)
            for fs in (0, 1):
                assert same(np.array([d.word_call(k, fs) for k in range(d.case.K)]), r["word"][fs]), (name, fs)
                if not d.single:
                    again = ctx.logscore_streams_batch(d.dms, d.corpora, final_state=bool(fs))
                    assert same(again, r["score"][fs]), (name, fs)


# ------------------------------------------------------------- 4. the contract

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", LC.NAMES)
def test_the_sum_over_all_states_is_no_smaller(G, ctx, devices, name, tier):
    r = devices(name).run(tier)
    for key in ("score", "word"):
        s0, s1 = r[key][0], r[key][1]
        both = np.isfinite(s0) & np.isfinite(s1)
        assert (s0[both] >= s1[both]).all()
    if name not in LC.EDITED:
        assert np.isfinite(r["score"][0]).all() and np.isfinite(r["score"][1]).any()


def timed(G, ctx, call):
    """the call's launches per kind; the preparation of the concatenated vocabularies is not pinned"""
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    try:
        call()
        return {k: n for k, (_, n) in ctx.kernel_times().items() if n and k != "prepare"}
    finally:
        ctx.set_option(G.OPT_TIMING, 0)


def test_launch_counts_and_the_workspace_afterwards(G, ctx, devices):
    lane, wide, v1, v2 = (devices(n) for n in ("lane_6x2x9_banded", "wide_65x1x4_banded", "vocab_p1", "vocab_p2"))
    calls = [
        (lambda: ctx.logscore(lane.dms[0][0], lane.corpora[0]), 1, lane),
        (lambda: ctx.logscore(wide.dms[0][0], wide.corpora[0], final_state=True), 1, wide),
        (lambda: ctx.logscore_streams(v2.dms[1], v2.corpora), 2, v2),
        (lambda: ctx.logscore_batch([w[0] for w in v1.dms], v1.corpora[0]), 1, v1),
        (lambda: ctx.logscore_streams_batch(v2.dms, v2.corpora, final_state=True), 2, v2),
    ]
    for call, P, d in calls:
        call()
        assert timed(G, ctx, call) == {"emission": 2 * P - 1, "forward": 1}
        # the row API does not reuse the log b, and the workspace serves no posteriors
        assert code(G, lambda: ctx.forward(d.dms[0][0], d.corpora[0])) == G.ERR_ARG
        assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
    # an earlier emission's posteriors are not served either
    ctx.emission(lane.dms[0][0], lane.corpora[0], True)
    ctx.fetch(G.BUF_POST, (lane.case.F, lane.case.Ns[0] * 2))
    ctx.logscore(lane.dms[0][0], lane.corpora[0])
    assert code(G, lambda: ctx.fetch(G.BUF_POST, (lane.case.F, lane.case.Ns[0] * 2))) == G.ERR_ARG


def handles(G, objs):
    return (G.C.c_void_p * len(objs))(*[o.h if o is not None else None for o in objs])


class Raw:
    """the four calls through the C ABI on a caller-owned destination pre-filled with a pattern"""

    def __init__(self, G, ctx, n):
        self.G, self.lib, self.h = G, ctx.lib, ctx.h
        self.out = np.full(n, -777.0)

    def dest(self, on=True):
        return self.out.ctypes.data_as(self.G.C.POINTER(self.G.C.c_double)) if on else None

    def untouched(self):
        return bool(np.all(self.out == -777.0))

    def one(self, m, c, fs=1, dest=True):
        return self.lib.ghmm_logscore(self.h, m.h if m else None, c.h if c else None, fs, self.dest(dest))

    def streams(self, ms, cs, P, fs=1, dest=True):
        return self.lib.ghmm_logscore_streams(self.h, ms, cs, P, fs, self.dest(dest))

    def batch(self, ms, K, c, fs=1, dest=True):
        return self.lib.ghmm_logscore_batch(self.h, ms, K, c.h if c else None, fs, self.dest(dest))

    def streams_batch(self, ms, K, cs, P, fs=1, dest=True):
        return self.lib.ghmm_logscore_streams_batch(self.h, ms, K, cs, P, fs, self.dest(dest))


def test_refusals_write_nothing(G, ctx, devices):
    d = devices("vocab_p2")
    case = d.case
    K, P = case.K, case.P
    rng = np.random.default_rng(19)
    raw = Raw(G, ctx, K * case.U)
    flat = [m for w in d.dms for m in w]
    h1 = case.words[1][1]

    def model(N, M, D):
        return ctx.model(rand_model(G, rng, N, M, D, case.words[1][0].A if N == h1.N else np.eye(N)))
    other_n, other_m, other_d = model(h1.N + 1, h1.M, h1.D), model(h1.N, h1.M + 1, h1.D), model(h1.N, h1.M, h1.D + 1)
    big = [model(513, w.M, w.D) for w in case.words[0]]
    lens2 = np.array(case.lens)
    lens2[0] += 1
    lens2[4] -= 1
    other_len = ctx.corpus(case.Xs[1], lens2)
    other_cd = ctx.corpus(np.zeros((case.F, h1.D + 2)), case.lens)
    vocab, corpora = handles(G, flat), handles(G, d.corpora)
    word1 = handles(G, d.dms[1])
    first = [w[0] for w in d.dms]
    nine_m, nine_c = handles(G, (flat * 9)[:9 * K]), handles(G, (d.corpora * 9)[:9])

    def swapped(i, m):
        return handles(G, flat[:i] + [m] + flat[i + 1:])
    try:
        arg, unsupported = G.ERR_ARG, G.ERR_UNSUPPORTED
        checks = [
            # ghmm_logscore: check_pair, the destination, the state count
            ("one: null model", raw.one(None, d.corpora[0]), arg),
            ("one: null corpus", raw.one(flat[0], None), arg),
            ("one: a corpus of another D", raw.one(flat[0], other_cd), arg),
            ("one: null destination", raw.one(flat[0], d.corpora[0], dest=False), arg),
            ("one: 513 states", raw.one(big[0], d.corpora[0]), unsupported),
            # ghmm_logscore_streams: check_streams
            ("streams: null models", raw.streams(None, corpora, P), arg),
            ("streams: null corpora", raw.streams(word1, None, P), arg),
            ("streams: P = 0", raw.streams(nine_m, nine_c, 0), arg),
            ("streams: P = 9", raw.streams(nine_m, nine_c, 9), arg),
            ("streams: null entry", raw.streams(handles(G, [d.dms[1][0], None]), corpora, P), arg),
            ("streams: streams differ in N", raw.streams(handles(G, [d.dms[1][0], other_n]), corpora, P), arg),
            ("streams: a length differs", raw.streams(word1, handles(G, [d.corpora[0], other_len]), P), arg),
            ("streams: a corpus of another D", raw.streams(word1, handles(G, [d.corpora[0], other_cd]), P), arg),
            ("streams: null destination", raw.streams(word1, corpora, P, dest=False), arg),
            ("streams: 513 states", raw.streams(handles(G, big), corpora, P), unsupported),
            # the vocabulary calls: vocab_check
            ("batch: null vocabulary", raw.batch(None, K, d.corpora[0]), arg),
            ("batch: null corpus", raw.batch(handles(G, first), K, None), arg),
            ("batch: K = 0", raw.batch(handles(G, first), 0, d.corpora[0]), arg),
            ("batch: null model", raw.batch(handles(G, [first[0], None, first[2]]), K, d.corpora[0]), arg),
            ("batch: null destination", raw.batch(handles(G, first), K, d.corpora[0], dest=False), arg),
            ("batch: a corpus of another D", raw.batch(handles(G, first), K, other_cd), arg),
            ("batch: words differ in M", raw.batch(handles(G, [first[0], flat[1]]), 2, d.corpora[0]), unsupported),
            ("batch: 513 states behind a word", raw.batch(handles(G, [first[0], big[0]]), 2, d.corpora[0]),
             unsupported),
            ("streams_batch: null vocabulary", raw.streams_batch(None, K, corpora, P), arg),
            ("streams_batch: null corpora", raw.streams_batch(vocab, K, None, P), arg),
            ("streams_batch: null model", raw.streams_batch(swapped(3, None), K, corpora, P), arg),
            ("streams_batch: null corpus", raw.streams_batch(vocab, K, handles(G, [d.corpora[0], None]), P), arg),
            ("streams_batch: K = 0", raw.streams_batch(vocab, 0, corpora, P), arg),
            ("streams_batch: K < 0", raw.streams_batch(vocab, -1, corpora, P), arg),
            ("streams_batch: P = 0", raw.streams_batch(nine_m, K, nine_c, 0), arg),
            ("streams_batch: P = 9", raw.streams_batch(nine_m, K, nine_c, 9), arg),
            ("streams_batch: streams of a word differ in N", raw.streams_batch(swapped(3, other_n), K, corpora, P), arg),
            ("streams_batch: a length differs",
             raw.streams_batch(vocab, K, handles(G, [d.corpora[0], other_len]), P), arg),
            ("streams_batch: a corpus of another D",
             raw.streams_batch(vocab, K, handles(G, [d.corpora[0], other_cd]), P), arg),
            ("streams_batch: null destination", raw.streams_batch(vocab, K, corpora, P, dest=False), arg),
            ("streams_batch: words differ in M_1", raw.streams_batch(swapped(3, other_m), K, corpora, P), unsupported),
            ("streams_batch: words differ in D_1", raw.streams_batch(swapped(3, other_d), K, corpora, P), unsupported),
            ("streams_batch: 513 states behind a word",
             raw.streams_batch(handles(G, flat[:P] + big), 2, corpora, P), unsupported),
        ]
        for what, rc, want in checks:
            assert rc == want, (what, rc)
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert raw.streams(word1, corpora, P) == unsupported
            assert raw.streams_batch(vocab, K, corpora, P) == unsupported
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert raw.untouched()
        # and the same arguments, valid, do write
        assert raw.streams_batch(vocab, K, corpora, P) == G.OK
        assert same(raw.out.reshape(K, case.U), ctx.logscore_streams_batch(d.dms, d.corpora, final_state=True))
    finally:
        for o in [other_n, other_m, other_d, other_len, other_cd] + big:
            o.close()


def test_empty_corpus_touches_nothing(G, ctx, devices):
    d = devices("vocab_p2")
    empty = [ctx.corpus(np.zeros((0, w.D)), np.zeros(0, dtype=np.int32)) for w in d.case.words[0]]
    raw = Raw(G, ctx, 8)
    vocab, corpora = handles(G, [m for w in d.dms for m in w]), handles(G, empty)
    first = handles(G, [w[0] for w in d.dms])
    try:
        for dest in (True, False):
            for fs in (0, 1):
                assert raw.one(d.dms[0][0], empty[0], fs, dest) == G.OK
                assert raw.streams(handles(G, d.dms[0]), corpora, d.case.P, fs, dest) == G.OK
                assert raw.batch(first, d.case.K, empty[0], fs, dest) == G.OK
                assert raw.streams_batch(vocab, d.case.K, corpora, d.case.P, fs, dest) == G.OK
        assert raw.untouched()
        assert ctx.logscore(d.dms[0][0], empty[0]).shape == (0,)
    finally:
        for c in empty:
            c.close()


# ------------------------------------------------------------- 5. the command line

def test_command_line_log_score(G, tmp_path):
    """bin/recognition-continuous-test-fs on the 13 recorded single-mixture models: with GHMM_LOG_SCORE=1 the
    report's second line says so, every printed score is finite and meets the reference log-domain score
    (rel 1e-9, abs 2e-6: test_gpu_parity's bar for printed scores), the words are ranked as those reference
    scores rank them, and no score lies below a finite print of the linear program (which is met only where
    none of its densities underflowed: -21289.18 against -16796.79 on one pair); without the variable the
    report and the printed rankings are the golden ones"""
    whole = json.load(open(os.path.join(GOLDEN, "whole_program.json")))
    models = np.load(os.path.join(GOLDEN, "train13_m1_models.npz"))
    tmp = str(tmp_path)
    words = whole["words"]

    def lst(name, lines):
        p = os.path.join(tmp, name)
        open(p, "w").write("\n".join(lines) + "\n")
        return p
    hms, paths = [], []
    for w in words:
        hms.append(G.HostModel(*(models[f"{w}.{k}"] for k in ("A", "c", "mean", "inv_var", "det")), word=w))
        paths.append(os.path.join(tmp, w + ".hmm"))
        hms[-1].write(paths[-1], 8)
    Xs = [G.perfil_read(os.path.join(GOLDEN, "perfil", fn)) for fn in whole["mean_list"]]
    ml = lst("models.txt", paths)
    fl = lst("mean_list.txt", [os.path.join(GOLDEN, "perfil", fn) for fn in whole["mean_list"]])
    wl = lst("words.txt", words)
    out = os.path.join(tmp, "hmm-result.txt")

    def report():
        return [l for l in open(out).read().split("\n") if not l.startswith("Date and time")
                and "recognition time" not in l and not l.startswith("Model name")]
    env = {k: v for k, v in os.environ.items() if k != "GHMM_LOG_SCORE"}
    p = subprocess.run([RECOGNISE, "1", ml, "1", fl, wl, out], stdout=subprocess.PIPE, timeout=300, env=env)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert report() == whole["recog13_m1"]["report"]
    plain = spoken_blocks(p.stdout.decode())
    assert plain == whole["recog13_m1"]["blocks"]

    p = subprocess.run([RECOGNISE, "1", ml, "1", fl, wl, out], stdout=subprocess.PIPE, timeout=300,
                       env=dict(env, GHMM_LOG_SCORE="1"))
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    got = report()
    assert got[0] == whole["recog13_m1"]["report"][0]
    assert got[1] == "Algorithm used for recognition: Forward (log domain) "
    blocks = spoken_blocks(p.stdout.decode())
    assert len(blocks) == 13 and all(len(b["ranking"]) == 13 for b in blocks)
    ref = np.array([[R.lattice(h.A, R.log_b([h], [x]), 1) for x in Xs] for h in hms]).astype(np.float64)
    assert np.isfinite(ref).all()
    for u, (blk, rec) in enumerate(zip(blocks, whole["recog13_m1"]["blocks"])):
        assert blk["spoken"] == rec["spoken"]
        printed = {w: float(txt) for w, txt in blk["ranking"]}
        assert all(np.isfinite(v) for v in printed.values())
        assert [w for w, _ in blk["ranking"]] == [words[k] for k in bubble(ref[:, u])], u
        for k, w in enumerate(words):
            assert printed[w] == pytest.approx(ref[k, u], rel=1e-9, abs=2e-6), (u, w)
        for w, txt in rec["ranking"]:       # a linear score only loses paths to underflow
            if "nan" not in txt and "inf" not in txt:
                assert printed[w] >= float(txt) - (1e-9 * abs(float(txt)) + 2e-6), (u, w)
