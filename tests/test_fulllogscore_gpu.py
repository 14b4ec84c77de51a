"""The full-covariance log-domain forward score (ghmm_logscore_full / ghmm_logscore_full_batch) on
the MI355X — GPU box only.

The lattice alone: the GPU's own log b (fetch(BUF_B)) restated in long double
(fulllogscore_ref.lattice), every score inside fulllogscore_ref.lattice_bound, the count of the
step's roundings written out there: T (3 V + La + N + 8) 2^-53.  The float64 restatement on the
same log b is held to that bound first, on the CPU.  End to end against the long-double
restatement: 8 x the float64 restatement's own distance at that shape, not below the 1e-11 that log b
is granted (the GPU sums in another order and its exp and log differ from libm's by an ulp or two).
Against what is already pinned to the reference: score_full_batch and the recorded prints on the
synthetic 13-word set, GHMM_BUF_LOGLIK after estep_full, at rel 1e-9 / abs 2e-6.  NaN and infinity
patterns are equal wherever two scores are compared; no pair is left out."""
import os
import subprocess

import numpy as np
import pytest

import fulllogscore_ref as LR
from _load import PKG_DIR
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import (FULL, banded, check_blocks, close_logb, code, ergodic, frames, load_synth, offsets,
                             rand_fmodel, rel_dist, same_kind_close, shipped, spoken_blocks)

pytestmark = pytest.mark.gpu

MISSES = {"vc_220_f_03_ap_010", "vc_220_f_047_ap_0225"}


def within_bound(got, A, logb, lens, fs):
    """every score of `got` against the long-double lattice on logb: equal NaN / infinity patterns,
    finite ones inside lattice_bound; returns the worst error / bound"""
    off = offsets(lens)
    N = A.shape[0]
    worst = 0.0
    for u, T in enumerate(lens):
        st = {}
        exact = LR.lattice(A, logb[off[u]:off[u + 1]], fs, np.longdouble, st)
        rel_dist([got[u]], [exact])
        if np.isfinite(exact) and T > 0:
            bound = LR.lattice_bound(T, N, st["V"], st["La"])
            err = float(abs(np.longdouble(got[u]) - exact))
            assert err <= bound, (fs, u, T, err, bound)
            worst = max(worst, err / bound)
    return worst


# ------------------------------------------------------------------- the tests

@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_lattice_alone(G, ctx, name):
    """L = 16, 32, 64, banded and dense A, T = 1, T < N, a c = 0 state, a det = 0 Gaussian, 64 x 2 x 48:
    the lattice on the GPU's own log b inside the derived bound, for both final_state settings"""
    hm, X, lens = LR.make_case(G, name)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    for fs in (0, 1):
        got = ctx.logscore_full(fm, corpus, final_state=bool(fs))
        logb = ctx.fetch(G.BUF_B, (corpus.frames, hm.N))
        close_logb(logb, LR.log_emission(hm, X, np.float64), 1e-11)
        cpu = LR.lattice_scores(hm.A, logb, lens, fs, np.float64)
        w_cpu = within_bound(cpu, hm.A, logb, lens, fs)      # the float64 restatement first
        w_gpu = within_bound(got, hm.A, logb, lens, fs)
        print(f"{name} final_state={fs}: error / bound: float64 restatement {w_cpu:.3f}, GPU {w_gpu:.3f}")
        short = np.asarray(lens) < hm.N
        if name.startswith("det0"):
            assert np.isnan(got).any() == (fs == 0 or name == "det0_banded")
            if name == "det0_absorbing" and fs == 1:
                assert np.isfinite(got[[0, 3]]).all()     # the NaN of state 3 stays there
        elif name == "c0_banded":
            assert (got == -np.inf).all() if fs else np.isfinite(got).all()
        elif not name.startswith("c0"):
            if fs == 0:
                assert np.isfinite(got).all()
            elif not LR.CASES[name][3]:
                assert (got[short] == -np.inf).all() and np.isfinite(got[~short]).all()
    fm.close()
    corpus.close()


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_end_to_end(G, ctx, name):
    """against the long-double restatement from X: 8 x the float64 restatement's distance, >= 1e-11"""
    hm, X, lens = LR.make_case(G, name)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    for fs in (0, 1):
        ref = LR.logscore(hm, X, lens, fs)
        d64 = rel_dist(LR.logscore(hm, X, lens, fs, np.float64), ref)
        bar = max(8.0 * d64, 1e-11)
        d = rel_dist(ctx.logscore_full(fm, corpus, final_state=bool(fs)), ref)
        print(f"{name} final_state={fs}: GPU {d:.2e}, float64 restatement {d64:.2e}, bar {bar:.2e}")
        assert d <= bar
    fm.close()
    corpus.close()


def test_synthetic_set_against_the_pinned_scores(G, ctx):
    """the recorded 13 x 12 x 4 x 16 run, all 169 pairs: final_state = 0 meets score_full_batch and the
    reference's prints; final_state = 1 meets GHMM_BUF_LOGLIK after estep_full"""
    sy, hms, Xs = load_synth(G)
    lens = [len(x) for x in Xs]
    corpus = ctx.corpus(np.concatenate(Xs), lens)
    fms = [ctx.full_model(h) for h in hms]
    lin = ctx.score_full_batch(fms, corpus)
    s0 = ctx.logscore_full_batch(fms, corpus)
    assert s0.shape == (13, 13) and np.isfinite(s0).all()
    same_kind_close(s0, lin)
    check_blocks(s0, sy["words"], sy["blocks"])
    s1 = ctx.logscore_full_batch(fms, corpus, final_state=True)
    for k, (h, fm) in enumerate(zip(hms, fms)):
        st = ctx.stats_full(h.N, h.M, h.D)
        ctx.estep_full(fm, corpus, st)
        same_kind_close(s1[k], ctx.fetch(G.BUF_LOGLIK, (13,)))
        st.close()
    for o in fms + [corpus]:
        o.close()


def test_shipped_set_is_finite_where_the_linear_score_is_not(G, ctx):
    """the shipped 13 x 13: score_full_batch is non-finite on 156 pairs, logscore_full_batch finite on
    all 169, 11 spoken words rank first, and the scores meet the long-double restatement"""
    sh, hms, Xs = shipped(G)
    words = [h.word for h in hms]
    lens = [len(x) for x in Xs]
    corpus = ctx.corpus(np.concatenate(Xs), lens)
    fms = [ctx.full_model(h) for h in hms]
    lin = ctx.score_full_batch(fms, corpus)
    assert (~np.isfinite(lin)).sum() == 156
    got = ctx.logscore_full_batch(fms, corpus)
    assert np.isfinite(got).all()
    same_kind_close(got[np.isfinite(lin)], lin[np.isfinite(lin)])
    first = [words[int(np.argmax(got[:, u]))] for u in range(13)]
    spoken = [b["spoken"] for b in sh["blocks"]]
    assert {s for s, f in zip(spoken, first) if s != f} == MISSES
    ref = np.array([[LR.logscore(h, x, [len(x)], 0)[0] for x in Xs] for h in hms])
    r64 = np.array([[LR.logscore(h, x, [len(x)], 0, np.float64)[0] for x in Xs] for h in hms])
    d64 = rel_dist(r64, ref)
    d = rel_dist(got, ref)
    print(f"shipped: GPU {d:.2e}, float64 restatement {d64:.2e}")
    assert d <= max(8.0 * d64, 1e-11)
    for o in fms + [corpus]:
        o.close()


def test_one_far_frame(G, ctx):
    """a synthetic utterance with one frame moved 60 units away: score_full gives -inf or NaN, the
    log-domain score is finite and within the end-to-end bar"""
    sy, hms, Xs = load_synth(G)
    hm = hms[0]
    X = np.concatenate([Xs[0], Xs[0], Xs[0]])
    T = len(Xs[0])
    lens = [T, T, T]
    X[T + T // 2] += 60.0      # inside utterance 1
    X[3 * T - 1] += 60.0       # the last frame of utterance 2
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    lin = ctx.score_full(fm, corpus)
    assert np.isfinite(lin[0]) and not np.isfinite(lin[1]) and not np.isfinite(lin[2])
    for fs in (0, 1):
        got = ctx.logscore_full(fm, corpus, final_state=bool(fs))
        assert np.isfinite(got).all()
        ref = LR.logscore(hm, X, lens, fs)
        d64 = rel_dist(LR.logscore(hm, X, lens, fs, np.float64), ref)
        d = rel_dist(got, ref)
        print(f"far frame final_state={fs}: GPU {d:.2e}, float64 restatement {d64:.2e}")
        assert d <= max(8.0 * d64, 1e-11)
    assert ctx.logscore_full(fm, corpus)[0] == pytest.approx(lin[0], rel=1e-9, abs=2e-6)
    fm.close()
    corpus.close()


@pytest.mark.parametrize("name", ["l16_banded", "l16_dense", "l32_banded", "l64_dense", "wide_64x2x48"])
def test_sum_over_paths_is_no_smaller(G, ctx, name):
    """final_state = 0 >= final_state = 1 >= viterbi_full's score, each within the lattice's bound"""
    hm, X, lens = LR.make_case(G, name)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    s0 = ctx.logscore_full(fm, corpus)
    s1 = ctx.logscore_full(fm, corpus, final_state=True)
    _, vt = ctx.viterbi_full(fm, corpus)
    logb = ctx.fetch(G.BUF_B, (corpus.frames, hm.N))
    off = offsets(lens)
    for u, T in enumerate(lens):
        st = {}
        LR.lattice(hm.A, logb[off[u]:off[u + 1]], 0, np.longdouble, st)
        tol = LR.lattice_bound(T, hm.N, st["V"], st["La"])
        assert not np.isnan([s0[u], s1[u], vt[u]]).any()
        assert s0[u] >= s1[u] - tol and s1[u] >= vt[u] - tol, (u, s0[u], s1[u], vt[u])
        assert (s1[u] == -np.inf) == (vt[u] == -np.inf)
    fm.close()
    corpus.close()


def test_batch_equals_single_calls(G, ctx):
    """mixed N (all three lane widths, banded and dense), T = 0 and T = 1 among the utterances: the
    batch = logscore_full word by word, bit for bit; log b of the batch = the single calls' columns"""
    rng = np.random.default_rng(31)
    base = rng.normal(0.0, 1.0, (1, 1, 9))
    sizes = (6, 3, 17, 6, 40, 1, 9, 64)
    hms = [rand_fmodel(G, rng, n, 2, 9, ergodic(rng, n) if k % 3 == 2 else banded(rng, n), spread=0.6,
                       base=base, asym=True) for k, n in enumerate(sizes)]
    lens = [33, 80, 1, 0, 57, 120, 15, 64, 200, 9, 0]
    X = frames(rng, hms[0], lens)
    X[100] += 300.0
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    for fs in (False, True):
        batch = ctx.logscore_full_batch(fms, corpus, final_state=fs)
        logb = ctx.fetch(G.BUF_B, (corpus.frames, sum(sizes)))
        assert batch.shape == (len(sizes), len(lens))
        assert (batch[:, [3, 10]] == 0.0).all() and not np.signbit(batch[:, [3, 10]]).any()   # T = 0
        assert np.isfinite(batch[:, 4]).all() if not fs else True
        bo = 0
        for k, fm in enumerate(fms):
            one = ctx.logscore_full(fm, corpus, final_state=fs)
            assert np.array_equal(batch[k].view(np.uint64), one.view(np.uint64)), (fs, k)
            n = sizes[k]
            assert np.array_equal(logb[:, bo:bo + n], ctx.fetch(G.BUF_B, (corpus.frames, n)), equal_nan=True), k
            bo += n
        assert np.array_equal(batch, ctx.logscore_full_batch(fms, corpus, final_state=fs))  # reproducible
    for o in fms + [corpus]:
        o.close()


def test_empty_corpus_touches_nothing(G, ctx):
    rng = np.random.default_rng(4)
    hm = rand_fmodel(G, rng, 5, 2, 6, banded(rng, 5), spread=1.0, asym=True)
    fm = ctx.full_model(hm)
    corpus = ctx.corpus(np.zeros((0, 6)), np.zeros(0, dtype=np.int32))
    lib = ctx.lib
    score = np.full(4, 3.5)
    arr = (G._vp * 1)(fm.h)
    for fs in (0, 1):
        assert lib.ghmm_logscore_full(ctx.h, fm.h, corpus.h, fs, G._d(score)) == 0
        assert lib.ghmm_logscore_full(ctx.h, fm.h, corpus.h, fs, None) == 0
        assert lib.ghmm_logscore_full_batch(ctx.h, arr, 1, corpus.h, fs, G._d(score)) == 0
        assert lib.ghmm_logscore_full_batch(ctx.h, arr, 1, corpus.h, fs, None) == 0
    assert (score == 3.5).all()
    assert ctx.logscore_full(fm, corpus).shape == (0,)
    fm.close()
    corpus.close()


def test_refusals_and_counters(G, ctx):
    """the codes of viterbi_full_batch: M or D differing in a batch, D against the corpus, a null
    destination, GHMM_OPT_ROBUST; the lattice launch counts under GHMM_K_FORWARD"""
    rng = np.random.default_rng(41)
    hm = rand_fmodel(G, rng, 5, 2, 6, banded(rng, 5), spread=1.0, asym=True)
    h3 = rand_fmodel(G, rng, 5, 3, 6, banded(rng, 5), spread=1.0, asym=True)
    h7 = rand_fmodel(G, rng, 5, 2, 7, banded(rng, 5), spread=1.0, asym=True)
    lens = [30, 20]
    X = frames(rng, hm, lens)
    fm, f3, f7 = ctx.full_model(hm), ctx.full_model(h3), ctx.full_model(h7)
    corpus = ctx.corpus(X, lens)
    for call, ref in ((ctx.logscore_full_batch, ctx.viterbi_full_batch),):
        for models in ([fm, f3], [fm, f7], [f7]):
            assert code(G, lambda: call(models, corpus)) == code(G, lambda: ref(models, corpus))
    assert code(G, lambda: ctx.logscore_full_batch([fm, f3], corpus)) == G.ERR_UNSUPPORTED  # M differs
    assert code(G, lambda: ctx.logscore_full_batch([fm, f7], corpus)) == G.ERR_UNSUPPORTED  # D differs
    assert code(G, lambda: ctx.logscore_full(f7, corpus)) == G.ERR_ARG                      # corpus D
    assert code(G, lambda: ctx.logscore_full_batch([f7], corpus)) == G.ERR_ARG
    lib = ctx.lib
    arr = (G._vp * 1)(fm.h)
    assert lib.ghmm_logscore_full(ctx.h, fm.h, corpus.h, 0, None) == G.ERR_ARG
    assert lib.ghmm_logscore_full_batch(ctx.h, arr, 1, corpus.h, 0, None) == G.ERR_ARG
    assert lib.ghmm_logscore_full_batch(ctx.h, arr, 1, corpus.h, 0, None) == \
        lib.ghmm_viterbi_full_batch(ctx.h, arr, 1, corpus.h, None)
    ctx.set_option(G.OPT_ROBUST, 1)
    try:
        assert code(G, lambda: ctx.logscore_full(fm, corpus)) == G.ERR_UNSUPPORTED
        assert code(G, lambda: ctx.logscore_full_batch([fm], corpus)) == G.ERR_UNSUPPORTED
    finally:
        ctx.set_option(G.OPT_ROBUST, 0)
    # score_full is what it was after a log-domain call; the diagonal row API refuses the log densities
    s_lin = ctx.score_full(fm, corpus)
    s1 = ctx.logscore_full(fm, corpus)
    assert np.array_equal(ctx.score_full(fm, corpus), s_lin, equal_nan=True)
    hd = G.HostModel(hm.A, np.full((5, 2), 0.5), hm.mean, np.ones((5, 2, 6)), np.ones((5, 2)))
    dm = ctx.model(hd)
    ctx.emission(dm, corpus, False)
    ctx.forward(dm, corpus)
    ctx.logscore_full(fm, corpus)
    assert code(G, lambda: ctx.forward(dm, corpus)) == G.ERR_ARG
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    try:
        s2 = ctx.logscore_full(fm, corpus)
        ctx.logscore_full_batch([fm, fm], corpus, final_state=True)
        kt = ctx.kernel_times()
    finally:
        ctx.set_option(G.OPT_TIMING, 0)
    assert np.array_equal(s1, s2)
    assert kt["emission"][1] == 2 and kt["forward"][1] == 2
    assert sum(n for _, n in kt.values()) == 4
    for o in (fm, f3, f7, dm, corpus):
        o.close()


def test_command_line_log_score(G, tmp_path):
    """bin/recognition-continuous-test-full-fs with GHMM_LOG_SCORE=1 on the shipped set: the header's
    second line, 169 finite printed scores, 11 spoken words ranked first"""
    sh = FULL["shipped"]
    exe = os.path.join(PKG_DIR, "bin", "recognition-continuous-test-full-fs")
    tmp = str(tmp_path)

    def lst(name, lines):
        p = os.path.join(tmp, name)
        open(p, "w").write("\n".join(lines) + "\n")
        return p
    ml = lst("models.txt", [os.path.join(GOLDEN, "full_cov_models", f) for f in sh["models"]])
    fl = lst("mean_list.txt", [os.path.join(GOLDEN, "perfil", f) for f in sh["mean_list"]])
    wl = lst("words.txt", sh["words"])
    out = os.path.join(tmp, "hmm-result.txt")
    p = subprocess.run([exe, "1", ml, "1", fl, wl, out], stdout=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, GHMM_LOG_SCORE="1"))
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    report = open(out).read().split("\n")
    assert report[1] == "Algorithm used for recognition: Forward (log domain) "
    assert report[0] == sh["report"][0]
    assert "Correct words: 11" in report and "Errors: 2" in report
    blocks = spoken_blocks(p.stdout.decode())
    for blk in blocks:
        blk["ranking"] = [(w, float(txt)) for w, txt in blk["ranking"]]
    assert len(blocks) == 13 and all(len(b["ranking"]) == 13 for b in blocks)
    assert all(np.isfinite(v) for b in blocks for _, v in b["ranking"])
    assert {b["spoken"] for b in blocks if b["ranking"][0][0] != b["spoken"]} == MISSES
    # the recorded finite prints of the linear program are met by the log-domain one
    for g, r in zip(blocks, sh["blocks"]):
        got = dict(g["ranking"])
        for w, txt in r["ranking"]:
            if "nan" not in txt and "inf" not in txt:
                assert got[w] == pytest.approx(float(txt), rel=1e-9, abs=2e-6), (r["spoken"], w)
