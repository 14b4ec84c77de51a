"""The extended Baum-Welch update (ghmm_mstep_ebw; k_mstep_ebw): a numpy restatement of the definition in
include/ghmm.h in a chosen float type (np.longdouble: the reference; np.float64: the device's arithmetic), cases of
a model with HAND-EDITED numerator and denominator vectors in the style of mstep_cases.py, and the restated MMI
loop (embed_cases' numerator, gstat_cases' denominator, this update) that test_gstat_host.py and test_mmi_gpu.py
share.  Plain numpy and the oracle, no GPU, no tests.

A case = name + shape (N, M, D).  Model and corpus: streams_util.synth_case; the numerator vector is
O.estep(hm, X, lens), the denominator vector O.estep(hm, X', lens) on the same model and the corpus with noise
added (both are accumulated on hm, so both num_var are around hm's means); then the edit of the name:
    plain           none
    equal           den = num: every difference is 0, damp = E cd, the means keep their bits
    den-zero        den = 0: mean = num_mu / num_c and the variance is the moment around the NEW mean
    neg-dv          den.num_var of one state = 6 num.num_var + 1e-3: dv strongly negative, the roots decide damp
    no-stats        one Gaussian without statistics in either vector: it keeps mean, variances and det
    row-kept        num.den_a of one row 0: the row of A is kept
    state-skipped   num.den_c of one state 0: its weights are kept (floored and renormalised all the same)"""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
from fullcov_support import need_extended
from streams_util import synth_case

FLOOR = 1.0e-5
# (2, 97, 13): the shape of mstep_cases whose model takes no matrix-core form (model_prepare returns early);
# (2, 130, 5): more Gaussians per state than k_mstep_ebw's block has threads (128): the strided tail of its loops
SHAPES = ((3, 2, 5), (10, 8, 39), (2, 97, 13), (2, 130, 5))
EDITS = ("plain", "equal", "den-zero", "neg-dv", "no-stats", "row-kept", "state-skipped")
NEG_STATE, NO_STATS, KEPT_ROW, SKIPPED = 1, (0, 1), 1, 1
Case = namedtuple("Case", "name shape hm num den E delta")


def split(v, N, M, D, ft=np.float64):
    """the blocks of a flat statistics vector (layout of include/ghmm.h), copies in ft"""
    G, o, out = N * M, 0, {}
    for name, n, shape in (("num_a", N * N, (N, N)), ("den_a", N, (N,)), ("den_c", N, (N,)), ("num_c", G, (N, M)),
                           ("num_mu", G * D, (N, M, D)), ("num_var", G * D, (N, M, D)), ("loglik", 1, ()),
                           ("n_utt", 1, ())):
        out[name] = np.asarray(v[o:o + n]).astype(ft).reshape(shape)
        o += n
    assert o == len(v)
    return out


def roots(s2, dc, dm, dv):
    """the larger real root of s2 x^2 + (dv + s2 dc) x + (dv dc - dm^2), 0 where it is negative: the
    discriminant as (dv - s2 dc)^2 + 4 s2 dm^2 (the same polynomial, never negative) and the root in the form that
    does not subtract two close numbers"""
    with np.errstate(all="ignore"):
        b, q, h = dv + s2 * dc, dv * dc - dm * dm, dv - s2 * dc
        sq = np.sqrt(h * h + 4 * s2 * (dm * dm))
        r = np.where(b <= 0, (sq - b) / (2 * s2), -2 * q / (b + sq))
        return np.where(r > 0, r, 0 * r)


def gaussians(mean, inv_var, det, num, den, E, ft=np.longdouble):
    """the means, variances and determinants of the update: (mean', var' floored, det', kept[N][M], damp[N][M],
    var' before the floor) in ft; num and den are split()'s dicts in ft"""
    mu, s2 = mean.astype(ft), 1 / inv_var.astype(ft)
    with np.errstate(all="ignore"):
        dc = num["num_c"] - den["num_c"]
        dm = (num["num_mu"] - den["num_mu"]) - dc[..., None] * mu
        dv = num["num_var"] - den["num_var"]
        r = roots(s2, dc[..., None], dm, dv)
        rmax = np.zeros(dc.shape, ft)
        for d in range(r.shape[-1]):
            rmax = np.fmax(rmax, r[..., d])
        damp = np.fmax(ft(E) * den["num_c"], 2 * rmax)
        t = dc + damp
        kept = ~((t > 0) & np.isfinite(t))
        tt = np.where(kept, ft(1), t)[..., None]
        step = dm / tt
        raw = (dv + damp[..., None] * s2) / tt - step * step
        var = np.where(raw < FLOOR, ft(FLOOR), raw)
        new_det = np.ones(dc.shape, ft)
        for d in range(var.shape[-1]):
            new_det = new_det * var[..., d]
        k3 = kept[..., None]
        return (np.where(k3, mu, mu + step), np.where(k3, s2, var), np.where(kept, det.astype(ft), new_det), kept,
                damp, raw)


def ebw(hm, num_v, den_v, E, delta=1, ft=np.longdouble):
    """ghmm_mstep_ebw restated on a model (anything with N, M, D, A, c, mean, inv_var, det) and two flat vectors.
    Returns a dict in ft: A, c, mean, inv_var, det, and var, kept, damp for the tests that look inside."""
    if ft is np.longdouble:
        need_extended()
    N, M, D = hm.N, hm.M, hm.D
    num, den = split(num_v, N, M, D, ft), split(den_v, N, M, D, ft)
    with np.errstate(all="ignore"):
        i, j = np.indices((N, N))
        band = (j >= i) & (j <= i + delta)
        upd = num["den_a"] != 0
        A = np.where(upd[:, None], np.where(band, num["num_a"] / np.where(upd, num["den_a"], 1)[:, None], ft(0)),
                     np.asarray(hm.A).astype(ft))
        cu = num["den_c"] != 0
        c = np.where(cu[:, None], num["num_c"] / np.where(cu, num["den_c"], 1)[:, None], np.asarray(hm.c).astype(ft))
        c = np.where(c < FLOOR, ft(FLOOR), c)
        s = np.zeros(N, ft)
        for m in range(M):
            s = s + c[:, m]
        c = c / s[:, None]
        mean, var, det, kept, damp, raw = gaussians(np.asarray(hm.mean), np.asarray(hm.inv_var), np.asarray(hm.det),
                                                    num, den, E, ft)
        inv_var = np.where(kept[..., None], np.asarray(hm.inv_var).astype(ft), 1 / var)
    return {"A": A, "c": c, "mean": mean, "inv_var": inv_var, "det": det, "var": var, "kept": kept, "damp": damp,
            "raw": raw}


# ------------------------------------------------------------- the hand-made cases

def _edit(name, num, den, N, M, D):
    if name == "plain":
        pass
    elif name == "equal":
        for k in den:
            den[k][...] = num[k]
    elif name == "den-zero":
        for k in den:
            den[k][...] = 0.0
    elif name == "neg-dv":
        den["num_var"][NEG_STATE] = 6.0 * num["num_var"][NEG_STATE] + 1e-3
    elif name == "no-stats":
        for s in (num, den):
            for k in ("num_c", "num_mu", "num_var"):
                s[k][NO_STATS] = 0.0
    elif name == "row-kept":
        num["den_a"][KEPT_ROW] = 0.0
    elif name == "state-skipped":
        num["den_c"][SKIPPED] = 0.0
    else:
        raise KeyError(name)


def _views(v, N, M, D):
    G, o, out = N * M, 0, {}
    for name, n, shape in (("num_a", N * N, (N, N)), ("den_a", N, (N,)), ("den_c", N, (N,)), ("num_c", G, (N, M)),
                           ("num_mu", G * D, (N, M, D)), ("num_var", G * D, (N, M, D))):
        out[name] = v[o:o + n].reshape(shape)
        o += n
    return out


@functools.lru_cache(maxsize=None)
def build(G, name, shape, E=2.0):
    """the Case of a name and shape, computed once; callers leave its arrays unchanged"""
    N, M, D = shape
    hm, X, lens = synth_case(G, N, M, D, [37, 20, max(12, N)], dense_A=name == "row-kept")
    rng = np.random.default_rng(77)
    num = O.estep(hm, X, lens, delta=1, dumps=False)[0].copy()
    den = O.estep(hm, X + rng.normal(0.0, 0.7, X.shape), lens, delta=1, dumps=False)[0].copy()
    assert np.all(np.isfinite(num)) and np.all(np.isfinite(den)), (name, shape)
    _edit(name, _views(num, N, M, D), _views(den, N, M, D), N, M, D)
    for a in (num, den):
        a.setflags(write=False)
    return Case(name, shape, hm, num, den, E, 1)


# ------------------------------------------------------------- the restated MMI loop

class Word:
    """a word's stream in a float type: what the restatements read of a HostModel"""

    def __init__(self, N, M, D, A, c, mean, inv_var, det):
        self.N, self.M, self.D = N, M, D
        self.A, self.c, self.mean, self.inv_var, self.det = A, c, mean, inv_var, det

    @classmethod
    def of(cls, hm, ft):
        return cls(hm.N, hm.M, hm.D, *(np.asarray(a).astype(ft) for a in (hm.A, hm.c, hm.mean, hm.inv_var, hm.det)))


def emission(words, Xs, ft):
    """log b [F][NS] (the streams' folded in order) and posts[p] [F][NS][M_p] of a vocabulary in ft, by
    estep_log_ref's formula"""
    import estep_log_ref as E
    import fullestep_log_ref as LE
    import fulllogscore_ref as LR
    P = len(words[0])
    logb, posts = None, []
    for p in range(P):
        es = [E.mixture_terms(w[p], Xs[p], ft) for w in words]
        lbs = [LR.mixture_lse(e) for e in es]
        posts.append(np.concatenate([LE.posteriors(e, lb) for e, lb in zip(es, lbs)], axis=1))
        lb = np.concatenate(lbs, axis=1)
        logb = lb if logb is None else logb + lb
    return logb, posts


def mmi_loop(start, Xs, lens, transcripts, grammar, iters, E=2.0, ft=np.longdouble):
    """mmi_em restated in ft from the HostModels start[k][p]: per iteration the emission, the embedded E-step
    (embed_cases.estep), the grammar E-step (gstat_cases.estep) and the update on every stream of every held word.
    Returns (trace of (sum log P_num, sum log P_den), the last models as Words)"""
    import embed_cases as EC
    import estep_log_ref as EL
    import gstat_cases as GS
    if ft is np.longdouble:
        need_extended()
    words = [[Word.of(h, ft) for h in w] for w in start]
    held = sorted({int(k) for t in transcripts for k in t})
    trace = []
    for _ in range(iters):
        logb, posts = emission(words, Xs, ft)
        n = EC.estep(words, Xs, lens, transcripts, ft=ft, logb=logb, posts=posts)
        d = GS.estep(words, Xs, lens, *grammar, ft=ft, logb=logb, posts=posts)
        trace.append((n["loglik"].sum(), d["loglik"].sum()))
        for k in held:
            for p, w in enumerate(words[k]):
                r = ebw(w, EL.vector(n["stats"][k][p]), EL.vector(d["stats"][k][p]), E, 1, ft)
                words[k][p] = Word(w.N, w.M, w.D, r["A"], r["c"], r["mean"], r["inv_var"], r["det"])
    return trace, words


# the MMI case of test_mmi_gpu.py and test_gstat_host.py: 4 three-state words with close means (word 3 in no
# transcript), 20 utterances of 2 to 3 words on 30 to 60 frames, a bigram grammar from the transcripts
MMI_SEED, MMI_ITERS, MMI_E = 2035, 3, 2.0      # (2031 to 2033 do not rise at every iteration, 2034 barely)
MMI_SHAPE = (1, 4)         # (M, D), one stream


@functools.lru_cache(maxsize=None)
def mmi_case(G, seed=MMI_SEED):
    """(start[k][p], Xs, lens, transcripts, (start, pair, fin)), computed once"""
    import vocab_cases as V
    from fullcov_support import banded
    from fullstreams_ref import stream_frames
    rng = np.random.default_rng(seed)
    M, D = MMI_SHAPE
    base = rng.normal(0.0, 1.0, (3, M, D))
    truth = []
    for k in range(4):
        h = V.rand_model(G, rng, 3, M, D, banded(rng, 3), word=f"w{k}")
        h.mean[:] = base + rng.normal(0.0, 0.6, base.shape)        # close means: confusable words
        truth.append([h])
    parts, lens, transcripts = [], [], []
    for u in range(20):
        L = int(rng.integers(2, 4))
        seq = [int(k) for k in rng.integers(0, 3, L)]
        seg = [int(t) for t in rng.integers(15, 21, L)]
        for k, T in zip(seq, seg):
            parts.append(stream_frames(rng, truth[k], [T])[0])
        lens.append(sum(seg))
        transcripts.append(tuple(seq))
    assert all(30 <= T <= 60 for T in lens)
    Xs = [np.concatenate(parts)]
    start = [[G.HostModel(h.A, h.c, h.mean + rng.normal(0.0, 0.3, h.mean.shape), h.inv_var, h.det, word=h.word)
              for h in w] for w in truth]
    grammar = G.bigram_log(transcripts, 4)
    return start, Xs, np.asarray(lens, dtype=np.int32), transcripts, grammar


__all__ = ["SHAPES", "EDITS", "Case", "split", "roots", "gaussians", "ebw", "build", "Word", "emission", "mmi_loop",
           "mmi_case", "MMI_SEED", "MMI_ITERS", "MMI_E"]
