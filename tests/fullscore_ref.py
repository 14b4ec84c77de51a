"""numpy restatement of the full-covariance recogniser's linear score (include/ghmm.h, ghmm_score_full;
RC = test/source/recognition-full-fs/recognition_continuous_full_fs.c) in a chosen float type, long
double by default, and the shapes test_fullscore_gpu.py runs.  Shared with test_fullscore_host.py,
which pins it to the float64 restatement (np_emission, np_logp) and proves that the long cases reach what they
are there for.  Plain numpy, no GPU.

    b_j(t) = sum_m c_jm exp(-aux_jm / 2) / den_jm        (calc_symbol_probab + calc_gaus, RC:855-954)
        aux = sum_i dif[i] * (sum_j dif[j] * inv_cov[j][i]),  den = pow(2 pi, D/2.0) * pow(|det|, 0.5)
        (det = 0: den = 0, the density is +inf or NaN, as the library documents it)
    alpha_0 = one-hot(0) * b(0);  alpha_t = (alpha^_{t-1} A) * b(t);  c_t = 1 / sum_j alpha_t(j)
    log P = -sum_t log c_t                               (calc_alpha + calc_probability, RC:733-836)
        no final-state term; an utterance of no frames scores 0

With ft = float64 emission() and logp() are np_emission and np_logp below operation for operation (the
same numpy calls on the same dtypes), which test_fullscore_host asserts bit for bit; the two pairs stay
separate code: np_emission / np_logp belong to the float64 family that the recorded runs pin.

The float64 form's relative distance from the long-double one, |x64 - xld| / |xld| over the finite
scores, as test_fullscore_host.test_float64_spread_sweep and _long print it (and hold it below 1e-13):

    sweep   6x2x9 banded 3.0e-16    9x2x5 zeros 3.7e-16     16x1x4 dense 3.6e-16    17x2x6 banded 3.6e-16
            24x2x6 dense 5.2e-16    32x1x5 banded 2.7e-16   33x1x13 banded 3.8e-16  64x1x4 dense 7.3e-16
            64x2x48 banded 2.4e-16
    long    l16_banded 2.3e-15      l16_dense 5.5e-16       l32_banded 6.1e-16      l32_dense 2.4e-16
            l64_banded 1.8e-16      l64_dense 3.0e-16       wide_5x2x48 7.5e-16

log_product_emulated() is the accumulator of the score-only scan (ghmm_kernels.hpp, log_product) on
the CPU: the product of the mantissas of c_t and the sum of their exponents, the product's own
exponent folded into the sum every 512 values.  Its two broken forms are what the long cases must
tell from the right one: a fold that drops the exponent, and no fold at all."""
import functools
import math

import numpy as np

from fullcov_support import banded, ergodic, frames, need_extended, offsets, rand_fmodel
from fulltrain_ref import np_quadform


def emission(hm, X, ft=np.longdouble):
    """b[F][N] of a HostFullModel in ft"""
    if ft is np.longdouble:
        need_extended()
    D = hm.D
    X = np.asarray(X, dtype=np.float64).reshape(-1, D).astype(ft)
    dif = X[:, None, None, :] - hm.mean.astype(ft)[None]                      # F N M D
    t = np.einsum("fnmj,nmji->fnmi", dif, hm.inv_cov.astype(ft))              # sum_j dif[j] inv_cov[j][i]
    aux = np.einsum("fnmi,fnmi->fnm", dif, t)
    den = pow(ft(2.0 * np.pi), ft(D / 2.0)) * np.power(np.abs(hm.det.astype(ft)), ft(0.5))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        g = np.exp(aux * ft(-0.5)) / den[None]
        return (g * hm.c.astype(ft)[None]).sum(-1)


def forward(A, b, ft=np.longdouble):
    """(log P, c_t[T]) of one utterance from its b[T][N] (any float type; widened to ft)"""
    if ft is np.longdouble:
        need_extended()
    A = np.asarray(A, dtype=np.float64).astype(ft)
    b = np.asarray(b).astype(ft)
    N = A.shape[0]
    lp = ft(0.0)
    alpha = np.zeros(N, ft)
    cs = np.empty(b.shape[0], ft)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for t in range(b.shape[0]):
            a = (np.eye(N, dtype=ft)[0] if t == 0 else alpha @ A) * b[t]
            c = ft(1.0) / a.sum()
            alpha = a * c
            lp -= np.log(c)
            cs[t] = c
    return lp, cs


def logp(A, b, ft=np.longdouble):
    return forward(A, b, ft)[0]


def lattice_scores(A, b, lens, ft=np.longdouble):
    """logp() per utterance of a corpus: [U] in ft"""
    off = offsets(lens)
    return np.array([logp(A, b[off[u]:off[u + 1]], ft) for u in range(len(lens))], dtype=ft)


def score(hm, X, lens, ft=np.longdouble):
    """ghmm_score_full restated end to end: [U] in ft"""
    return lattice_scores(hm.A, emission(hm, X, ft), lens, ft)


# ------------------------------------------------ the float64 family: RC restated on whole arrays

def np_emission(hm, X):
    """calc_symbol_probab + calc_gaus, RC:855-954 (det = 0 as the library documents it)"""
    _, aux, den = np_quadform(hm, X)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        g = np.exp(aux * -0.5) / den[None]
        return (g * hm.c[None]).sum(-1)


def np_logp(A, b):
    """calc_alpha (one-hot start) + calc_probability without a final-state term, RC:733-836"""
    N = A.shape[0]
    lp = 0.0
    alpha = np.zeros(N)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for t in range(b.shape[0]):
            a = (np.eye(N)[0] if t == 0 else alpha @ A) * b[t]
            c = 1.0 / a.sum()
            alpha = a * c
            lp -= np.log(c)
    return lp


# ------------------------------------------------ the score-only scan's accumulator on the CPU

FOLD_EVERY = 512


def log_product_emulated(cs, fold="exact"):
    """log_product over the float64 values cs, in float64.  fold = "exact" (the kernel's), "drop" (the
    fold renormalises the mantissa product and forgets its exponent) or "none" (no fold).  Returns
    (sum_t log c_t as log_value() forms it, the smallest mantissa product met on the way)."""
    m, e, n, least = 1.0, 0, 0, 1.0
    for c in cs:
        fm, fe = math.frexp(float(c))
        m *= fm
        e += fe
        n += 1
        least = min(least, abs(m))
        if n == FOLD_EVERY and fold != "none":
            fm, fe = math.frexp(m)
            if fold == "exact":
                e += fe
            m, n = fm, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(e) * 6.93147180369123816490e-01 + (float(e) * 1.90821492927058770002e-10 + float(np.log(m))), least


# ------------------------------------------------ the shapes the GPU tests run

def make_A(rng, N, kind):
    """kind = "banded" (left-to-right), "zeros" (ergodic, 40 % of the entries 0) or "dense" (no entry 0)"""
    return banded(rng, N) if kind == "banded" else ergodic(rng, N, 0.4 if kind == "zeros" else 0.0)


# 1. the linear emission at every DB of k_emission_full, both sides of each boundary
EMISSION_D = (8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 47, 48)
EMISSION_LENS = (70, 1, 33, 129)        # 233 frames: three tiles of 64 and one with 41 frames left
FAR_FRAME = 40


@functools.lru_cache(maxsize=None)
def emission_case(G, D):
    """(HostFullModel 5 x 3 x D with one asymmetric inverse covariance, X, lens); frame 40 lies 60
    units from everything"""
    rng = np.random.default_rng(4000 + D)
    hm = rand_fmodel(G, rng, 5, 3, D, spread=1.0, asym=True)
    X = frames(rng, hm, EMISSION_LENS, scale=1.5)
    X[FAR_FRAME] += 60.0
    return hm, X, np.asarray(EMISSION_LENS, dtype=np.int32)


# 2. the score sweep: (N, M, D, A).  Lane classes 16 / 32 / 64, each with a banded and a dense A
SWEEP = ((6, 2, 9, "banded"), (9, 2, 5, "zeros"), (16, 1, 4, "dense"), (17, 2, 6, "banded"), (24, 2, 6, "dense"),
         (32, 1, 5, "banded"), (33, 1, 13, "banded"), (64, 1, 4, "dense"), (64, 2, 48, "banded"))
# every T from 0 to 34 (every residue of the scan's unrolled loop of 16 with and without a whole
# block in front, T = 0, T = 1, T < N), then 70 and 129: 37 utterances, no whole number of waves
SWEEP_LENS = tuple(range(35)) + (70, 129)
BATCH_BASE = (24, 2, 6, "dense")                       # the corpus of the batch test ...
BATCH_EXTRA = ((9, 2, 6, "zeros"), (33, 2, 6, "banded"))  # ... and the words of the other two lane classes


def sweep_id(case):
    return "%dx%dx%d-%s" % case


@functools.lru_cache(maxsize=None)
def sweep_case(G, case):
    """(HostFullModel, X, lens) of a SWEEP entry, the utterances in shuffled order"""
    N, M, D, kind = case
    rng = np.random.default_rng(5000 + SWEEP.index(case))
    hm = rand_fmodel(G, rng, N, M, D, make_A(rng, N, kind), spread=1.0, asym=True)
    lens = rng.permutation(np.asarray(SWEEP_LENS, dtype=np.int32))
    assert not np.array_equal(np.argsort(-lens, kind="stable"), np.arange(len(lens)))
    return hm, frames(rng, hm, lens), lens


@functools.lru_cache(maxsize=None)
def batch_models(G):
    """the words that share BATCH_BASE's corpus with its own model: one of the 16-lane class (dense
    with zeros), one of the 64-lane class (banded)"""
    rng = np.random.default_rng(5100)
    return tuple(rand_fmodel(G, rng, N, M, D, make_A(rng, N, kind), spread=1.0, asym=True)
                 for N, M, D, kind in BATCH_EXTRA)


# 3. long utterances through the score-only scan: name -> (N, M, D, A, lengths, the lengths at which
# the mantissa product leaves the normal range when nothing folds it)
LONG = {
    "l16_banded": (6, 2, 9, "banded", (511, 512, 513, 514, 1025, 1537, 4100), (4100,)),
    "l16_dense": (9, 2, 5, "zeros", (513, 4100), (4100,)),
    "l32_banded": (20, 2, 8, "banded", (513, 1025), ()),
    "l32_dense": (24, 2, 6, "dense", (513,), ()),
    "l64_banded": (40, 1, 13, "banded", (1025,), ()),
    "l64_dense": (64, 1, 4, "dense", (600,), ()),
    "wide_5x2x48": (5, 2, 48, "banded", (1100,), ()),      # c_t with large exponents
}


@functools.lru_cache(maxsize=None)
def long_case(G, name):
    """(HostFullModel, a 3-state word of the same M and D for the batch, X, lens)"""
    N, M, D, kind, lens, _ = LONG[name]
    rng = np.random.default_rng(6000 + sorted(LONG).index(name))
    hm = rand_fmodel(G, rng, N, M, D, make_A(rng, N, kind), spread=1.0, asym=True)
    small = rand_fmodel(G, rng, 3, M, D, spread=1.0, asym=True)
    return hm, small, frames(rng, hm, lens), np.asarray(lens, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def reference(G, what, key):
    """the long-double scores [U] of a case (what = "sweep" or "long"), computed once"""
    if what == "sweep":
        hm, X, lens = sweep_case(G, key)
    else:
        hm, _, X, lens = long_case(G, key)
    ref = score(hm, X, lens)
    ref.setflags(write=False)
    return ref
