"""The full-covariance recogniser (RC = test/source/recognition-full-fs/
recognition_continuous_full_fs.c) on the MI355X — GPU box only.

Checked against recorded runs of the real reference (tests/golden/fullcov_recog.json,
fullcov_synth13.npz, fullcov_hmm_result.txt: make_golden_fullcov.py), against the float64 numpy
restatement of calc_gaus / calc_alpha / calc_probability (fullscore_ref.np_emission, np_logp), and
against the pinned diagonal path.  Tolerances: densities rtol 1e-11 (below 1e-300 a subnormal keeps too few bits for a
relative bound: there the values must agree to 1e-300 absolute, and be 0 exactly where numpy's
are); scores of the reference within rel 1e-9 / abs 2e-6, as the diagonal recogniser's."""
import os
import subprocess

import numpy as np
import pytest

from _load import PKG_DIR
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import (FULL, check_blocks, close_b, code, frames, load_synth, rand_fmodel, same_kind_close,
                             spoken_blocks)
from fullscore_ref import np_emission, np_logp

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------- the tests

def test_shipped_end_to_end(G, tmp_path):
    """bin/recognition-continuous-test-full-fs with the reference's argv on the shipped 4-byte
    models: its report is the shipped hmm-result.txt, its stdout the reference's rankings."""
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
    p = subprocess.run([exe, "1", ml, "1", fl, wl, out], stdout=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    keep = lambda l: (not l.startswith("Date and time") and "recognition time" not in l  # noqa: E731
                      and not l.startswith("Model name"))
    got = [l for l in open(out).read().split("\n") if keep(l)]
    ref = [l for l in open(os.path.join(GOLDEN, "fullcov_hmm_result.txt")).read().split("\n") if keep(l)]
    assert got == ref == sh["report"]
    # stdout: "<word> :  <score>" rows per spoken word
    blocks = spoken_blocks(p.stdout.decode())
    assert len(blocks) == len(sh["blocks"]) == 13
    for g, r in zip(blocks, sh["blocks"]):
        assert g["spoken"] == r["spoken"]
        assert [w for w, _ in g["ranking"]] == [w for w, _ in r["ranking"]], r["spoken"]
        for (_, gv), (w, rv) in zip(g["ranking"], r["ranking"]):
            if "nan" in rv or "inf" in rv:
                assert gv.lstrip("-") == rv.lstrip("-"), (r["spoken"], w)
            else:
                assert float(gv) == pytest.approx(float(rv), rel=1e-9, abs=2e-6), (r["spoken"], w)
    # fewer than 7 arguments: RC's usage text
    p = subprocess.run([exe, "1", ml], stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout.startswith(b"Usage: recognition_continuous_full ")


def test_synthetic_reference_run(G, ctx):
    """score_full_batch on the recorded 13 x 12 x 4 x 16 run: all 169 scores (finite) and rankings."""
    sy, hms, Xs = load_synth(G)
    corpus = ctx.corpus(np.concatenate(Xs), [len(x) for x in Xs])
    fms = [ctx.full_model(h) for h in hms]
    scores = ctx.score_full_batch(fms, corpus)
    assert np.isfinite(scores).all()
    check_blocks(scores, sy["words"], sy["blocks"])
    for o in fms + [corpus]:
        o.close()


@pytest.mark.parametrize("N,M,D", [(6, 1, 9), (12, 4, 16), (20, 8, 39), (3, 2, 1), (64, 1, 13), (5, 3, 48),
                                   (7, 2, 24)])
def test_emission_matches_restatement(G, ctx, N, M, D):
    rng = np.random.default_rng(N * 1000 + M * 100 + D)
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=True)
    lens = [70, 1, 33, 129]
    X = frames(rng, hm, lens, scale=1.5)
    X[5] += 60.0  # a frame far from everything: densities that underflow to 0
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    ctx.emission_full(fm, corpus)
    b = ctx.fetch(G.BUF_B, (corpus.frames, N))
    ref = np_emission(hm, X)
    close_b(b, ref)
    assert (ref[5] == 0).all() and (ref > 0).any()
    got = fm.get()
    for a, r in zip(got.arrays(), hm.arrays()):
        assert np.array_equal(a, r)
    assert fm.dims() == (N, M, D)
    fm.close()
    corpus.close()


def test_score_has_no_final_state_term(G, ctx):
    """log P = -sum_t log c_t (RC:822-836); a frame whose densities are all 0 gives -inf when it is
    the utterance's last frame and NaN when one follows it."""
    rng = np.random.default_rng(11)
    hm = rand_fmodel(G, rng, 6, 2, 9, spread=0.5, asym=False)
    lens = [50, 31, 1, 80, 12, 40]
    X = frames(rng, hm, lens, scale=0.7)
    off = np.concatenate([[0], np.cumsum(lens)])
    X[off[1] - 1] += 1e3   # last frame of utterance 0
    X[off[3] + 10] += 1e3  # inside utterance 3
    X[off[2]] += 1e3       # the one frame of utterance 2
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    got = ctx.score_full(fm, corpus)
    b = np_emission(hm, X)
    ref = np.array([np_logp(hm.A, b[off[u]:off[u + 1]]) for u in range(len(lens))])
    assert got[0] == -np.inf and got[2] == -np.inf and np.isnan(got[3])
    same_kind_close(got, ref, rtol=1e-11, atol=0)
    fm.close()
    corpus.close()


def test_cross_check_with_diagonal_path(G, ctx):
    """inv_cov = diag(inv_var): the same densities as ghmm_emission (vector-ALU tier, the reference's
    order), and log P = the diagonal forward's log P minus log alpha^_{N-1}(T-1).  A det = 0 Gaussian
    gives the same value on both paths."""
    rng = np.random.default_rng(21)
    N, M, D = 7, 3, 12
    hf = rand_fmodel(G, rng, N, M, D, spread=0.8, asym=False)
    iv = rng.uniform(0.5, 2.0, (N, M, D))
    hf.inv_cov = np.zeros((N, M, D, D))
    hf.inv_cov[..., np.arange(D), np.arange(D)] = iv
    hf.det = 1.0 / iv.prod(-1)
    hf.det[2, 1] = 0.0
    hd = G.HostModel(hf.A, hf.c, hf.mean, iv, hf.det)
    lens = [60, 45, 90]
    X = frames(rng, hf, lens, scale=0.8)
    dctx = G.Context(0)
    try:
        dctx.set_option(G.OPT_KERNELS, 1)
        dm, dc = dctx.model(hd), dctx.corpus(X, lens)
        dctx.emission(dm, dc, False)
        bd = dctx.fetch(G.BUF_B, (dc.frames, N))
        dctx.forward(dm, dc)
        alpha = dctx.fetch(G.BUF_ALPHA, (dc.frames, N))
        lld = dctx.fetch(G.BUF_LOGLIK, (len(lens),))
    finally:
        dctx.close()
    fm, corpus = ctx.full_model(hf), ctx.corpus(X, lens)
    ctx.emission_full(fm, corpus)
    bf = ctx.fetch(G.BUF_B, (corpus.frames, N))
    assert np.isinf(bf[:, 2]).any() or np.isnan(bf[:, 2]).any()  # the det = 0 Gaussian shows
    close_b(bf, bd)
    llf = ctx.score_full(fm, corpus)
    last = np.cumsum(lens) - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        same_kind_close(llf, lld - np.log(alpha[last, N - 1]), rtol=1e-11, atol=0)
    fm.close()
    corpus.close()


def test_batch_equals_word_by_word(G, ctx):
    rng = np.random.default_rng(31)
    base = rng.normal(0.0, 1.0, (1, 1, 9))
    hms = [rand_fmodel(G, rng, n, 2, 9, spread=0.6, base=base, asym=False) for n in (6, 3, 17, 6, 40, 1, 9)]
    lens = [33, 80, 1, 57, 120, 15, 64, 200, 9]
    X = frames(rng, hms[0], lens, scale=1.0)
    X[100] += 300.0
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    batch = ctx.score_full_batch(fms, corpus)
    for k, fm in enumerate(fms):
        one = ctx.score_full(fm, corpus)
        assert np.array_equal(batch[k], one, equal_nan=True), k
    for o in fms + [corpus]:
        o.close()


def test_refusals(G, ctx):
    rng = np.random.default_rng(41)
    assert code(G, lambda: ctx.full_model(rand_fmodel(G, rng, 65, 1, 4, spread=0.3, asym=False))) == G.ERR_UNSUPPORTED
    assert code(G, lambda: ctx.full_model(rand_fmodel(G, rng, 3, 1, 49, spread=0.3, asym=False))) == G.ERR_UNSUPPORTED
    # the widest model built still works
    for N, D in ((64, 5), (4, 48)):
        hm = rand_fmodel(G, rng, N, 1, D, spread=0.3, asym=False)
        lens = [70, 40]
        X = frames(rng, hm, lens, scale=0.5)
        fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
        b = np_emission(hm, X)
        off = [0, 70, 110]
        ref = [np_logp(hm.A, b[off[u]:off[u + 1]]) for u in range(2)]
        same_kind_close(ctx.score_full(fm, corpus), ref, rtol=1e-11, atol=0)
        fm.close()
        corpus.close()
    hm = rand_fmodel(G, rng, 5, 2, 6, spread=0.3, asym=False)
    h3 = rand_fmodel(G, rng, 5, 3, 6, spread=0.3, asym=False)
    h7 = rand_fmodel(G, rng, 5, 2, 7, spread=0.3, asym=False)
    X = frames(rng, hm, [30, 20])
    fm, f3, f7 = ctx.full_model(hm), ctx.full_model(h3), ctx.full_model(h7)
    corpus = ctx.corpus(X, [30, 20])
    assert code(G, lambda: ctx.score_full_batch([fm, f3], corpus)) == G.ERR_UNSUPPORTED  # M differs
    assert code(G, lambda: ctx.score_full_batch([fm, f7], corpus)) == G.ERR_UNSUPPORTED  # D differs
    assert code(G, lambda: ctx.score_full(f7, corpus)) == G.ERR_ARG                      # corpus D
    assert code(G, lambda: ctx.emission_full(f7, corpus)) == G.ERR_ARG
    ctx.set_option(G.OPT_ROBUST, 1)
    try:
        assert code(G, lambda: ctx.score_full(fm, corpus)) == G.ERR_UNSUPPORTED
        assert code(G, lambda: ctx.emission_full(fm, corpus)) == G.ERR_UNSUPPORTED
        assert code(G, lambda: ctx.score_full_batch([fm], corpus)) == G.ERR_UNSUPPORTED
    finally:
        ctx.set_option(G.OPT_ROBUST, 0)
    # the workspace after ghmm_emission_full belongs to no diagonal model
    hd = G.HostModel(hm.A, hm.c, hm.mean, np.ones((5, 2, 6)), np.ones((5, 2)))
    dm = ctx.model(hd)
    ctx.emission(dm, corpus, False)
    ctx.forward(dm, corpus)
    ctx.emission_full(fm, corpus)
    assert code(G, lambda: ctx.forward(dm, corpus)) == G.ERR_ARG
    assert code(G, lambda: ctx.fetch(G.BUF_BETA, (corpus.frames, 5))) == G.ERR_ARG
    for o in (fm, f3, f7, dm, corpus):
        o.close()


def test_vocabulary_larger_than_one_tile(G, ctx):
    """50 words x 15 states x 5 mixtures x 16 coefficients (RC's capacity limits), 240 utterances:
    the concatenated vocabulary spans many emission tiles."""
    rng = np.random.default_rng(51)
    base = rng.normal(0.0, 1.5, (1, 1, 16))
    hms = [rand_fmodel(G, rng, 15, 5, 16, spread=0.5, base=base, word=f"w{k}", asym=False) for k in range(50)]
    lens = rng.integers(20, 90, 240)
    X = base[0, 0] + rng.normal(0.0, 1.0, (int(lens.sum()), 16))
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    batch = ctx.score_full_batch(fms, corpus)
    assert np.isfinite(batch).mean() > 0.5
    for k in (0, 17, 49):
        assert np.array_equal(batch[k], ctx.score_full(fms[k], corpus), equal_nan=True), k
    off = np.concatenate([[0], np.cumsum(lens)])
    for u in (0, 101, 239):
        Xu = X[off[u]:off[u + 1]]
        ref = [np_logp(h.A, np_emission(h, Xu)) for h in hms]
        same_kind_close(batch[:, u], ref, rtol=1e-11, atol=0)
    for o in fms + [corpus]:
        o.close()
