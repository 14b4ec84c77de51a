"""The full-covariance Viterbi (ghmm_viterbi_full / ghmm_viterbi_full_batch) on the MI355X — GPU
box only.

Its definition is the diagonal Viterbi's (oracle/ghmm_oracle.c) with the full quadratic form, so:
the log densities are checked against the numpy restatement (fullviterbi_ref.py) within
1e-11 * (1 + |ref|); path and score are checked bit for bit against the pinned oracle lattice
(O.viterbi_lattice) run on the GPU's own log b; the batch against the single calls bit for bit;
with diagonal inverse covariances, against the diagonal ghmm_viterbi."""
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import check_viterbi_lattice, close_logb, code, ergodic, frames, offsets, rand_fmodel
from fullviterbi_ref import lattice_margins, log_emission

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------- the tests

@pytest.mark.parametrize("N,M,D", [(6, 1, 9), (12, 4, 16), (20, 8, 39), (3, 2, 1), (64, 1, 13), (5, 3, 48),
                                   (7, 2, 24)])
def test_log_emission_and_lattice(G, ctx, N, M, D):
    """log b (fetch(BUF_B) after viterbi_full) = the restatement within 1e-11 (1 + |ref|), the frame
    far from everything included; path and score = the oracle lattice on that log b, bit for bit"""
    rng = np.random.default_rng(N * 1000 + M * 100 + D)
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=True)
    lens = [70, 1, 33, 129]
    X = frames(rng, hm, lens, scale=1.5)
    X[5] += 60.0
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    path, score = ctx.viterbi_full(fm, corpus)
    logb = ctx.fetch(G.BUF_B, (corpus.frames, N))
    ref = log_emission(hm, X)
    close_logb(logb, ref, 1e-11)
    assert np.isfinite(ref[5]).all()
    check_viterbi_lattice(hm.A, logb, lens, path, score)
    assert np.isfinite(score[[0, 3]]).all()  # (T >= N: the last state is reached)
    fm.close()
    corpus.close()


@pytest.mark.parametrize("kind", ["banded", "ergodic", "ties"])
def test_lattice_bit_identical(G, ctx, kind):
    """banded and ergodic A (zeros included), exact ties, T = 1, T < N and T = 0"""
    rng = np.random.default_rng({"banded": 1, "ergodic": 2, "ties": 3}[kind])
    N, M, D = 20, 3, 8
    if kind == "ties":
        # every state the same mixture and every transition 1/N: all candidates tie
        hm = rand_fmodel(G, rng, N, M, D, A=np.full((N, N), 1.0 / N), spread=0.3, asym=True)
        for a in (hm.c, hm.mean, hm.inv_cov, hm.det):
            a[:] = a[0]
        hm = G.HostFullModel(hm.A, hm.c, hm.mean, hm.inv_cov, hm.det)
    else:
        hm = rand_fmodel(G, rng, N, M, D, A=ergodic(rng, N) if kind == "ergodic" else None, spread=0.3, asym=True)
    lens = [40, 1, 3, 0, 19, 120, 2, 0, 64]
    X = frames(rng, hm, lens, scale=1.0)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    path, score = ctx.viterbi_full(fm, corpus)
    logb = ctx.fetch(G.BUF_B, (corpus.frames, N))
    if kind == "ties":
        assert (logb == logb[:, :1]).all()
        assert np.isfinite(score[[0, 2, 4, 5, 6, 8]]).all() and score[1] == -np.inf  # (T = 1: state 0)
    check_viterbi_lattice(hm.A, logb, lens, path, score)
    assert score[3] == 0.0 and score[7] == 0.0
    # one frame per model size class: L = 16, 32, 64 lanes
    for n in (5, 31, 64):
        h = rand_fmodel(G, rng, n, 2, 4, A=ergodic(rng, n) if kind != "banded" else None, spread=0.3, asym=True)
        ls = [n // 2 + 1, 1, 2 * n]
        Xn = frames(rng, h, ls)
        f, cp = ctx.full_model(h), ctx.corpus(Xn, ls)
        p, s = ctx.viterbi_full(f, cp)
        check_viterbi_lattice(h.A, ctx.fetch(G.BUF_B, (cp.frames, n)), ls, p, s)
        f.close()
        cp.close()
    fm.close()
    corpus.close()


def test_empty_corpus_touches_nothing(G, ctx):
    rng = np.random.default_rng(4)
    hm = rand_fmodel(G, rng, 5, 2, 6, spread=0.3, asym=True)
    fm = ctx.full_model(hm)
    corpus = ctx.corpus(np.zeros((0, 6)), np.zeros(0, dtype=np.int32))
    lib = ctx.lib
    path = np.full(4, 7, dtype=np.int32)
    score = np.full(4, 3.5)
    assert lib.ghmm_viterbi_full(ctx.h, fm.h, corpus.h, path.ctypes.data_as(G._ip), G._d(score)) == 0
    assert lib.ghmm_viterbi_full(ctx.h, fm.h, corpus.h, None, None) == 0
    arr = (G._vp * 1)(fm.h)
    assert lib.ghmm_viterbi_full_batch(ctx.h, arr, 1, corpus.h, G._d(score)) == 0
    assert lib.ghmm_viterbi_full_batch(ctx.h, arr, 1, corpus.h, None) == 0
    assert (path == 7).all() and (score == 3.5).all()
    fm.close()
    corpus.close()


def test_finite_where_the_forward_score_is_not(G, ctx):
    """frames far from every Gaussian: score_full gives -inf / NaN (linear densities of 0), the
    log-domain Viterbi a finite score equal to the restatement's within rel 1e-11"""
    rng = np.random.default_rng(11)
    hm = rand_fmodel(G, rng, 6, 2, 9, spread=0.5, asym=True)
    lens = [50, 31, 8, 80, 12, 40]
    X = frames(rng, hm, lens, scale=0.7)
    off = offsets(lens)
    X[off[1] - 1] += 1e3   # last frame of utterance 0
    X[off[3] + 10] += 1e3  # inside utterance 3
    X[off[3] - 1] += 1e3   # last frame of utterance 2
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    fwd = ctx.score_full(fm, corpus)
    assert fwd[0] == -np.inf and fwd[2] == -np.inf and np.isnan(fwd[3])
    path, score = ctx.viterbi_full(fm, corpus)
    assert np.isfinite(score).all()
    ref_b = log_emission(hm, X)
    ref = np.array([O.viterbi_lattice(hm.A, ref_b[off[u]:off[u + 1]])[1] for u in range(len(lens))])
    assert np.isfinite(ref).all()
    np.testing.assert_allclose(score, ref, rtol=1e-11, atol=0)
    fm.close()
    corpus.close()


def test_diagonal_inverse_covariance_is_the_diagonal_viterbi(G, ctx):
    """inv_cov = diag(inv_var): the paths of ghmm_viterbi on the diagonal model (the data have no
    near-ties along them), the scores within rel 1e-11"""
    rng = np.random.default_rng(21)
    for N, M, D, A in ((7, 3, 12, None), (9, 2, 5, ergodic(rng, 9))):
        hf = rand_fmodel(G, rng, N, M, D, spread=0.8, A=A, asym=True)
        iv = rng.uniform(0.5, 2.0, (N, M, D))
        hf.inv_cov = np.zeros((N, M, D, D))
        hf.inv_cov[..., np.arange(D), np.arange(D)] = iv
        hf.det = 1.0 / iv.prod(-1)
        hd = G.HostModel(hf.A, hf.c, hf.mean, iv, hf.det)
        lens = [60, 45, 90, 1]
        X = frames(rng, hf, lens, scale=0.8)
        off = offsets(lens)
        ref_b = log_emission(hf, X)
        for u in range(len(lens)):
            p, _ = O.viterbi_lattice(hf.A, ref_b[off[u]:off[u + 1]])
            gaps = lattice_margins(hf.A, ref_b[off[u]:off[u + 1]], p)
            assert gaps.size == 0 or gaps.min() > 1e-9, (N, u)
        dm, dc = ctx.model(hd), ctx.corpus(X, lens)
        pd, sd = ctx.viterbi(dm, dc)
        fm, corpus = ctx.full_model(hf), ctx.corpus(X, lens)
        pf, sf = ctx.viterbi_full(fm, corpus)
        assert np.array_equal(pf, pd)
        np.testing.assert_allclose(sf, sd, rtol=1e-11, atol=0)
        for o in (dm, dc, fm, corpus):
            o.close()


def test_batch_shipped_models(G, ctx):
    """the shipped 13 models x 13 utterances: the batch = viterbi_full model by model, bit for bit"""
    mdir = os.path.join(GOLDEN, "full_cov_models")
    hms = [G.HostFullModel.read(os.path.join(mdir, f)) for f in sorted(os.listdir(mdir)) if f.endswith(".hmm")]
    pdir = os.path.join(GOLDEN, "perfil")
    Xs = [G.perfil_read(os.path.join(pdir, f)) for f in sorted(os.listdir(pdir)) if f.endswith(".perfil")]
    assert len(hms) == 13 and len(Xs) == 13
    lens = [len(x) for x in Xs]
    corpus = ctx.corpus(np.concatenate(Xs), lens)
    fms = [ctx.full_model(h) for h in hms]
    batch = ctx.viterbi_full_batch(fms, corpus)
    NS = sum(h.N for h in hms)
    logb = ctx.fetch(G.BUF_B, (corpus.frames, NS))
    assert batch.shape == (13, 13)
    bo = 0
    for k, fm in enumerate(fms):
        path, one = ctx.viterbi_full(fm, corpus)
        assert np.array_equal(batch[k], one, equal_nan=True), k
        N = hms[k].N
        assert np.array_equal(logb[:, bo:bo + N], ctx.fetch(G.BUF_B, (corpus.frames, N)), equal_nan=True), k
        check_viterbi_lattice(hms[k].A, logb[:, bo:bo + N], lens, path, one)
        bo += N
    for o in fms + [corpus]:
        o.close()


def test_batch_vocabulary_larger_than_one_tile(G, ctx):
    """50 words x 15 x 5 x 16 (RC's capacity limits), 240 utterances, a few words of other sizes"""
    rng = np.random.default_rng(51)
    base = rng.normal(0.0, 1.5, (1, 1, 16))
    sizes = [15] * 46 + [1, 33, 64, 7]
    hms = [rand_fmodel(G, rng, n, 5, 16, spread=0.5, base=base, word=f"w{k}",
                       A=ergodic(rng, n) if k % 9 == 4 else None, asym=True) for k, n in enumerate(sizes)]
    lens = rng.integers(20, 90, 240)
    lens[[3, 77]] = [0, 1]
    X = base[0, 0] + rng.normal(0.0, 1.0, (int(lens.sum()), 16))
    X[500] += 200.0
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    batch = ctx.viterbi_full_batch(fms, corpus)
    assert np.isfinite(batch).mean() > 0.5
    assert (batch[:, 3] == 0.0).all()
    for k, fm in enumerate(fms):
        _, one = ctx.viterbi_full(fm, corpus)
        assert np.array_equal(batch[k], one, equal_nan=True), k
    for o in fms + [corpus]:
        o.close()


def test_special_values_refusals_and_workspace(G, ctx):
    """c = 0 gives -inf and det = 0 gives NaN (the formula's values); the refusals of the full calls;
    score_full unchanged after viterbi_full; the diagonal row API refuses the log densities"""
    rng = np.random.default_rng(41)
    hm = rand_fmodel(G, rng, 5, 2, 6, spread=0.3, asym=True)
    hm.c[1] = 0.0          # state 1: every e = -inf
    hm.det[3, 1] = 0.0     # state 3: lk = +inf
    lens = [30, 20]
    X = frames(rng, hm, lens)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    s1 = ctx.score_full(fm, corpus)
    path, score = ctx.viterbi_full(fm, corpus)
    logb = ctx.fetch(G.BUF_B, (corpus.frames, 5))
    assert (logb[:, 1] == -np.inf).all() and np.isnan(logb[:, 3]).all()
    close_logb(logb, log_emission(hm, X), 1e-11)
    check_viterbi_lattice(hm.A, logb, lens, path, score)
    assert np.array_equal(ctx.score_full(fm, corpus), s1, equal_nan=True)

    h3 = rand_fmodel(G, rng, 5, 3, 6, spread=0.3, asym=True)
    h7 = rand_fmodel(G, rng, 5, 2, 7, spread=0.3, asym=True)
    f3, f7 = ctx.full_model(h3), ctx.full_model(h7)
    assert code(G, lambda: ctx.viterbi_full_batch([fm, f3], corpus)) == G.ERR_UNSUPPORTED  # M differs
    assert code(G, lambda: ctx.viterbi_full_batch([fm, f7], corpus)) == G.ERR_UNSUPPORTED  # D differs
    assert code(G, lambda: ctx.viterbi_full(f7, corpus)) == G.ERR_ARG                      # corpus D
    assert code(G, lambda: ctx.viterbi_full_batch([f7], corpus)) == G.ERR_ARG
    lib = ctx.lib
    arr = (G._vp * 1)(fm.h)
    assert lib.ghmm_viterbi_full(ctx.h, fm.h, corpus.h, None, None) == G.ERR_ARG
    assert lib.ghmm_viterbi_full_batch(ctx.h, arr, 1, corpus.h, None) == G.ERR_ARG
    ctx.set_option(G.OPT_ROBUST, 1)
    try:
        assert code(G, lambda: ctx.viterbi_full(fm, corpus)) == G.ERR_UNSUPPORTED
        assert code(G, lambda: ctx.viterbi_full_batch([fm], corpus)) == G.ERR_UNSUPPORTED
    finally:
        ctx.set_option(G.OPT_ROBUST, 0)
    hd = G.HostModel(hm.A, np.full((5, 2), 0.5), hm.mean, np.ones((5, 2, 6)), np.ones((5, 2)))
    dm = ctx.model(hd)
    ctx.emission(dm, corpus, False)
    ctx.forward(dm, corpus)
    ctx.viterbi_full(fm, corpus)
    assert code(G, lambda: ctx.forward(dm, corpus)) == G.ERR_ARG
    ctx.viterbi_full_batch([fm, fm], corpus)
    assert code(G, lambda: ctx.forward(dm, corpus)) == G.ERR_ARG
    assert ctx.fetch(G.BUF_B, (corpus.frames, 10)).shape == (50, 10)
    for o in (fm, f3, f7, dm, corpus):
        o.close()


def test_reproducible_and_timed(G, ctx):
    """repeated calls are bitwise equal; the kernels count under GHMM_K_EMISSION / GHMM_K_VITERBI"""
    rng = np.random.default_rng(61)
    base = rng.normal(0.0, 1.0, (1, 1, 13))
    hms = [rand_fmodel(G, rng, n, 4, 13, base=base, A=ergodic(rng, n) if n == 9 else None, spread=0.3, asym=True)
           for n in (6, 9, 20)]
    lens = rng.integers(1, 200, 50)
    X = base[0, 0] + rng.normal(0.0, 1.0, (int(lens.sum()), 13))
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    p1, s1 = ctx.viterbi_full(fms[1], corpus)
    b1 = ctx.fetch(G.BUF_B, (corpus.frames, 9))
    v1 = ctx.viterbi_full_batch(fms, corpus)
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    try:
        p2, s2 = ctx.viterbi_full(fms[1], corpus)
        b2 = ctx.fetch(G.BUF_B, (corpus.frames, 9))
        v2 = ctx.viterbi_full_batch(fms, corpus)
        kt = ctx.kernel_times()
    finally:
        ctx.set_option(G.OPT_TIMING, 0)
    assert np.array_equal(p1, p2) and np.array_equal(s1, s2) and np.array_equal(b1, b2)
    assert np.array_equal(v1, v2)
    assert kt["emission"][1] == 2 and kt["viterbi"][1] == 2
    assert sum(n for _, n in kt.values()) == 4
    for o in fms + [corpus]:
        o.close()
