"""numpy restatement of the full-covariance log-domain forward score (include/ghmm.h,
ghmm_logscore_full) in a chosen float type, long double by default.  Shared by
test_fulllogscore_host.py, which pins it to the reference's recorded runs and to the long-double
E-step restatement (fulltrain_ref.py), and by test_fulllogscore_gpu.py, which holds the HIP lattice
against it.  Plain numpy, no GPU.

    log b: fullviterbi_ref.log_emission's formula, Gaussian by Gaussian in ft
        lk = log(c) - log(den),  den = pow(2 pi, D/2.0) * pow(|det|, 0.5)
        e_m = lk_m - aux_m / 2,  aux = sum_i dif[i] * (sum_j dif[j] * inv_cov[j][i])
        log b = m + log(sum_m exp(e_m - m)), m = max of the non-NaN e_m; -inf when m is -inf
    la_0(j) = (j == 0 ? 0 : -inf) + log b_j(0)
    la_t(j) = LSE_{i : a_ij > 0} (la_{t-1}(i) + log a_ij) + log b_j(t)
    LSE(x)  = m + log(sum exp(x_i - m)), m = max x_i; -inf without a term above -inf, NaN with a NaN term
    score   = LSE_j la_{T-1}(j)  (final_state = 0)  or  la_{T-1}(N-1)  (final_state = 1);  T = 0: 0

CASES are the shapes the GPU tests run.  The float64 restatement's worst relative distance from the
long-double one, |x64 - xld| / |xld| over the finite scores of both final_state settings, measured by
test_fulllogscore_host.test_float64_spread (which prints it and holds it below 1e-12):

    l16_banded     1.9e-15      l16_dense      3.5e-16      l32_banded     7.7e-16
    l32_dense      6.7e-16      l64_banded     5.1e-16      l64_dense      1.9e-16
    c0_banded      1.5e-15      c0_dense       3.5e-16      det0_absorbing 2.3e-16
    det0_banded    0 (no finite score)                      wide_64x2x48   6.3e-16
    the shipped 13 x 13 set (test_shipped_set)              1.7e-14
"""
import numpy as np

from fullcov_support import banded, ergodic, frames, need_extended, offsets, rand_fmodel
from fulltrain_ref import gaussians


def mixture_terms(hm, X, ft=np.longdouble):
    """e[F][N][M] of the formula above, Gaussian by Gaussian in ft (fulltrain_ref.gaussians)"""
    if ft is np.longdouble:
        need_extended()
    Xf = np.asarray(X, dtype=np.float64).reshape(-1, hm.D).astype(ft)
    e = np.empty((len(Xf), hm.N, hm.M), ft)
    with np.errstate(all="ignore"):
        for i, k, aux, den in gaussians(hm, Xf, ft):
            lk = np.log(ft(hm.c[i, k])) - np.log(den)
            e[:, i, k] = lk - aux * ft(0.5)
    return e


def mixture_lse(e):
    """log b[F][N] from e[F][N][M]"""
    ft = e.dtype.type
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(e), ft(-np.inf), e).max(-1)
        s = np.exp(e - m[..., None]).sum(-1)
        return np.where(m == -np.inf, ft(-np.inf), m + np.log(s))


def log_emission(hm, X, ft=np.longdouble):
    """log b[F][N] of a HostFullModel in ft"""
    return mixture_lse(mixture_terms(hm, X, ft))


def lse(x, terms=None):
    """LSE over axis 0 of the entries of x that `terms` marks (all of them by default)"""
    ft = x.dtype.type
    with np.errstate(all="ignore"):
        if terms is not None:
            x = np.where(terms, x, ft(-np.inf))
        m = np.where(np.isnan(x), ft(-np.inf), x).max(0)
        mm = np.where(m == -np.inf, ft(0), m)
        return m + np.log(np.exp(x - mm).sum(0))


def log_transitions(A, ft):
    """(the mask a_ij > 0, log a_ij in ft with 0 where a_ij = 0)"""
    terms = np.asarray(A, dtype=np.float64) > 0
    return terms, np.log(np.where(terms, A, 1.0).astype(ft))


def forward_rows(terms, la_A, lb):
    """la_0, la_1, ... la_{T-1} in turn from lb = log b[T][N], T >= 1: the one forward step, which
    fullestep_log_ref.lattice_fb takes too"""
    ft = lb.dtype.type
    la = np.where(np.arange(lb.shape[1]) == 0, ft(0), ft(-np.inf)) + lb[0]
    yield la
    for t in range(1, len(lb)):
        la = lse(la[:, None] + la_A, terms) + lb[t]
        yield la


def lattice(A, logb, final_state, ft=np.longdouble, stats=None):
    """the score of one utterance from its log b[T][N] (any float type; widened to ft).  stats, a
    dict, receives V = the largest finite |la| and La = the largest finite |log a_ij|."""
    if ft is np.longdouble:
        need_extended()
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    if len(logb) == 0:
        return ft(0)
    lb = np.asarray(logb).astype(ft).reshape(-1, N)
    with np.errstate(all="ignore"):
        terms, la_A = log_transitions(A, ft)
        V = 0
        for la in forward_rows(terms, la_A, lb):
            V = max(V, np.abs(la[np.isfinite(la)]).max(initial=0))
        if stats is not None:
            stats["V"] = max(float(V), stats.get("V", 0.0))
            stats["La"] = max(float(np.abs(la_A).max()), stats.get("La", 0.0))
        return la[N - 1] if final_state else lse(la)


def lattice_scores(A, logb, lens, final_state, ft=np.longdouble, stats=None):
    """lattice() per utterance of a corpus: [U] in ft"""
    off = offsets(lens)
    return np.array([lattice(A, logb[off[u]:off[u + 1]], final_state, ft, stats) for u in range(len(lens))],
                    dtype=ft)


def logscore(hm, X, lens, final_state, ft=np.longdouble):
    """ghmm_logscore_full restated end to end: [U] in ft"""
    return lattice_scores(hm.A, log_emission(hm, X, ft), lens, final_state, ft)


# ------------------------------------------------ the lattice's rounding bound
# One step of the device lattice in float64 (u = 2^-53), with V the largest finite |la| and La the
# largest finite |log a_ij|; LSE is a weighted mean of its terms' errors (weights exp(x_i - LSE), sum
# 1), so what a term inherits passes on with weight 1 and the step's own roundings add up:
#   log a_ij rounded to float64 by the host                                  La u
#   term = la_{t-1}(i) + log a_ij, one rounding of a value near la           V u
#   dense: x_i - m (u/e at most after its weight), exp at <= 2 ulp on values <= 1, the sum of N of
#     them, log at <= 2 ulp: together                                        (N + c) u
#   banded: lo - hi, exp, log1p at <= 2 ulp each, on values <= 1: inside the same   c u
#   m + log(sum) (hi + log1p), one rounding of a value near la               V u
#   + log b_j(t), one rounding of la itself                                  V u
# The final LSE over the lanes (final_state = 0) is one more such step without the two outer adds,
# and an utterance of T frames takes T - 1 steps, so T steps cover both:
#   |score - exact lattice on the same log b| <= T (3 V + La + N + c) u,  c = 8
LATTICE_C = 8.0


def lattice_bound(T, N, V, La):
    return T * (3.0 * V + La + N + LATTICE_C) * 2.0 ** -53


# ------------------------------------------------ the shapes the GPU tests run
# name: (N, M, D, dense A, utterance lengths); every list has T = 1 and a T < N
CASES = {
    "l16_banded": (6, 2, 9, False, [70, 1, 33, 129, 3]),
    "l16_dense": (9, 2, 5, True, [70, 1, 33, 90, 3]),
    "l32_banded": (20, 3, 8, False, [40, 1, 3, 19, 120, 2, 64]),
    "l32_dense": (24, 2, 6, True, [40, 1, 3, 19, 100]),
    "l64_banded": (40, 1, 13, False, [90, 1, 39, 150]),
    "l64_dense": (64, 1, 4, True, [10, 80, 1]),
    "c0_banded": (5, 2, 6, False, [30, 1, 3, 20]),       # state 1 has c = 0: log b = -inf
    "c0_dense": (5, 2, 6, True, [30, 1, 3, 20]),
    "det0_banded": (5, 2, 6, False, [30, 1, 3, 20]),     # state 3 has a det = 0 Gaussian: log b = NaN
    "det0_absorbing": (5, 2, 6, True, [30, 1, 3, 20]),   # ... and no way out of state 3: it does not leak
    "wide_64x2x48": (64, 2, 48, False, [70, 1, 150, 20]),
}


def make_case(G, name):
    """(HostFullModel, X, lens) of a CASES entry; frame 5 lies 60 units from everything"""
    N, M, D, dense, lens = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    hm = rand_fmodel(G, rng, N, M, D, ergodic(rng, N) if dense else banded(rng, N), spread=1.0, asym=True)
    if name.startswith("c0"):
        hm.c[1] = 0.0
    if name.startswith("det0"):
        hm.det[3, 1] = 0.0
    if name == "det0_absorbing":
        hm.A[3] = 0.0
        hm.A[3, 3] = 1.0
        hm.A[:, 4] += 0.05          # the last state is reached past state 3
        hm.A[3, 4] = 0.0
        hm.A /= hm.A.sum(1, keepdims=True)
    hm = G.HostFullModel(hm.A, hm.c, hm.mean, hm.inv_cov, hm.det)
    X = frames(rng, hm, lens)
    X[5] += 60.0
    return hm, X, np.asarray(lens, dtype=np.int32)
