"""The reference of the diagonal log-domain Baum-Welch E-step (include/ghmm.h, ghmm_estep_log and
ghmm_estep_log_streams) and its cases, shared by test_estep_log_host.py and test_estep_log_gpu.py.  Plain
numpy and the oracle, no GPU, no tests.  Built from what is already there:

    log b      logscore_ref.log_b: the oracle's float64 log emission per stream, folded in stream order
    post       exp(e_m - log b_i(t)) in the float type asked for, 0 where log b_i(t) = -inf, with
               e_m = log c - D/2 log(2 pi) - log|det| / 2 - aux / 2 (the oracle's formula) and log b its LSE in
               that type (fulllogscore_ref.mixture_lse, fullestep_log_ref.posteriors): equal to
               exp(e_m - mx_i) / sum_m' exp(e_m' - mx_i) of the header
    lattice    fullestep_log_ref.lattice_fb on log b, which does not depend on the kind of model; beyond
               logscore_ref.WIDE_REF states gathered_fb below, which forms only the terms with a_ij > 0
               (the terms left out are those lse masks to -inf and adds as exact zeros);
               test_estep_log_host.test_gathered_lattice_is_the_reference_lattice holds the two together
    sums       calc_mix_param for the diagonal layout, mix_sums below: num_c, num_mu, and num_var around
               the old mean

The cases are logscore_cases.SINGLE as they stand, and the two-stream shapes of logscore_cases.VOCAB,
(M, D) = (2, 5) and (3, 4), as single P = 2 models of 6 and of 70 states, both banded: p2_6_banded on
logscore_cases.VOCAB_LENS, p2_70_banded with a first utterance of 90 frames in place of 40 so that the
last state is reached.  Every case holds T = 1, T < N, T = 0 and (far = True) frame 5 moved 60 units away
in every stream.  DELTA_CASES run under GHMM_OPT_DELTA 0, 2 and 3 as well.

The float64 restatement's distance from the long-double one, measured by
test_estep_log_host.test_float64_spread, which prints the three figures and holds the first below 1e-12 and
the others below RTOL / 8:
    the worst relative distance over the finite log P_u and log Z_u
  | over the statistics vector's blocks the smallest d with |x64 - xld| <= d (|xld| + 1e-5 max|xld|) per block
    (block_dist; the gammas' exponents carry the rounding of T lattice steps on values of size V ~ 3e4)
  | the same over the far frame's posteriors, state by state (0 with one mixture: the posterior is 1)

    lane_6x2x9_banded   1.3e-15 | 1.8e-10 | 0           lane_9x2x5_dense    2.8e-16 | 1.1e-11 | 9.1e-179
    lane_40x1x13_banded 1.2e-15 | 3.4e-10 | 0           lane_64x1x4_dense   2.2e-16 | 1.5e-12 | 0
    lane_c0             2.7e-16 | 0       | 4.3e-104    lane_nan            4.0e-16 | 0       | 1.2e-106
    wide_65x1x4_banded  1.9e-15 | 2.9e-10 | 0           wide_130x2x5_banded 2.9e-15 | 5.2e-11 | 4.3e-13
    wide_70x1x4_dense   2.4e-16 | 2.2e-11 | 0           wide_512x1x4_banded 1.9e-14 | 0       | 0
    wide_c0             1.3e-16 | 0       | 0           wide_nan            1.2e-16 | 0       | 0
    p2_6_banded         3.9e-16 | 1.6e-11 | 6.1e-27     p2_70_banded        2.2e-16 | 4.6e-11 | 1.6e-12
(lane_c0, wide_c0: no path into the last state, every gamma is 0; lane_nan, wide_nan: log Z_u is NaN, every
gamma is 0; wide_512x1x4_banded:
rho_u = exp(log P_u - log Z_u) = exp(-1150) is below float64's range, so every gamma is 0 there too.)
"""
import functools

import numpy as np

import fullestep_log_ref as LE
import fulllogscore_ref as LR
import logscore_cases as LC
import logscore_ref as R
from fullcov_support import banded, need_extended, offsets
from vocab_cases import Case, _frames, rand_model

STREAM_SHAPES = ((2, 5), (3, 4))
# name: (N, utterance lengths)
STREAMS = {"p2_6_banded": (6, LC.VOCAB_LENS), "p2_70_banded": (70, (90, 1, 4, 0, 12))}
NAMES = tuple(LC.SINGLE) + tuple(STREAMS)
EDITED = LC.EDITED
DELTA_CASES = ("lane_6x2x9_banded", "wide_65x1x4_banded")
DELTAS = (0, 2, 3)
COMMON = ("num_a", "den_a", "den_c", "loglik", "n_utt")
BLOCKS = ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_var", "loglik", "n_utt")


def make(G, name, far=True):
    """the Case (one word, P streams) of a name; far = False leaves frame 5 where it was drawn"""
    if name in LC.SINGLE:
        return LC.make(G, name, far)
    N, lens = STREAMS[name]
    rng = np.random.default_rng(900 + list(STREAMS).index(name))
    A = banded(rng, N)
    words = [[rand_model(G, rng, N, M, D, A.copy(), word=name) for M, D in STREAM_SHAPES]]
    Xs = _frames(rng, words, lens, (0,) * len(lens))
    if far:
        for X in Xs:
            X[LC.FAR_FRAME] += LC.FAR
    return Case(words, Xs, lens)


# ------------------------------------------------------------- emission

def mixture_terms(hm, X, ft=np.longdouble):
    """e[F][N][M] of a diagonal HostModel in ft: the oracle's formula (orc_log_emission)"""
    if ft is np.longdouble:
        need_extended()
    Xf = np.asarray(X, dtype=np.float64).reshape(-1, hm.D).astype(ft)
    with np.errstate(all="ignore"):
        dif = Xf[:, None, None, :] - hm.mean.astype(ft)[None]
        aux = (dif * hm.inv_var.astype(ft)[None] * dif).sum(-1)
        lk = (np.log(hm.c.astype(ft)) - ft(0.5) * ft(hm.D) * np.log(ft(2.0 * np.pi))
              - ft(0.5) * np.log(np.abs(hm.det.astype(ft))))
        return lk[None] - ft(0.5) * aux


def posteriors(hm, X, ft=np.longdouble):
    """post[F][N][M] of one stream in ft"""
    e = mixture_terms(hm, X, ft)
    return LE.posteriors(e, LR.mixture_lse(e))


# ------------------------------------------------------------- lattice

def gathered_fb(A, logb, delta=1, ft=np.longdouble):
    """fullestep_log_ref.lattice_fb with only the terms a_ij > 0 formed: the same dict"""
    if ft is np.longdouble:
        need_extended()
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    lb = np.asarray(logb).astype(ft).reshape(-1, N)
    T = len(lb)
    out = {"la": np.zeros((T, N), ft), "lbe": np.zeros((T, N), ft), "gamma": np.zeros((T, N), ft),
           "xi": np.zeros((N, N), ft), "logP": ft(0), "logZ": ft(0), "V": 0.0, "La": 0.0, "T": T}
    if T == 0:
        return out
    with np.errstate(all="ignore"):
        terms, la_A = LR.log_transitions(A, ft)
        idx = np.arange(N)
        Kp, Ks = int(terms.sum(0).max()), int(terms.sum(1).max())
        pred = np.argsort(~terms, axis=0, kind="stable")[:Kp]           # [Kp][N]: column j's predecessors first
        succ = np.argsort(~terms, axis=1, kind="stable")[:, :Ks].T      # [Ks][N]: row i's successors first
        mp, lp = terms[pred, idx[None]], la_A[pred, idx[None]]
        ms, ls = terms[idx[None], succ], la_A[idx[None], succ]
        la, lbe = out["la"], out["lbe"]
        la[0] = np.where(idx == 0, ft(0), ft(-np.inf)) + lb[0]
        for t in range(1, T):
            la[t] = LR.lse(la[t - 1][pred] + lp, mp) + lb[t]
        lbe[T - 1] = np.where(idx == N - 1, ft(0), ft(-np.inf))
        w = np.zeros((T, N), ft)
        for t in range(T - 2, -1, -1):
            w[t] = lb[t + 1] + lbe[t + 1]
            lbe[t] = LR.lse(ls + w[t][succ], ms)
        logP, logZ = la[T - 1, N - 1], LR.lse(la[T - 1])
        out["logP"], out["logZ"] = logP, logZ
        out["V"], out["La"] = LE._finmax(la, lbe), float(np.abs(la_A).max())
        if np.isfinite(logZ):
            out["gamma"] = np.exp(la + lbe - logZ)
            for o in range(0, delta + 1):
                i = idx[:N - o]
                x = np.exp(la[:T - 1, i] + la_A[i, i + o][None] + w[:T - 1, i + o] - logZ).sum(0)
                out["xi"][i, i + o] = np.where(terms[i, i + o], x, ft(0))
    return out


def lattice_fb(A, logb, delta=1, ft=np.longdouble):
    fn = gathered_fb if np.asarray(A).shape[0] > R.WIDE_REF else LE.lattice_fb
    return fn(A, logb, delta, ft)


# ------------------------------------------------------------- statistics

def mix_sums(w, X, mean, ft=np.longdouble):
    """calc_mix_param (TF:1691-1727) on the weights w[F][N][M] = gamma * post, in ft: num_c, num_mu and
    num_var around `mean`"""
    Xf = np.asarray(X, dtype=np.float64).astype(ft)
    w = np.asarray(w).astype(ft)
    with np.errstate(all="ignore"):
        dif = Xf[:, None, None, :] - mean.astype(ft)[None]
        return {"num_c": w.sum(0), "num_mu": (w[..., None] * Xf[:, None, None, :]).sum(0),
                "num_var": (w[..., None] * dif * dif).sum(0)}


def vector(st):
    """the flat statistics vector (layout of include/ghmm.h) of a dict of blocks, in the blocks' type"""
    return np.concatenate([np.atleast_1d(np.asarray(st[k])).ravel() for k in BLOCKS])


def estep(hms, Xs, lens, delta=1, ft=np.longdouble, logb=None, posts=None, normaliser="Z"):
    """ghmm_estep_log_streams restated on the streams hms[p], Xs[p] (one stream: ghmm_estep_log).  logb /
    posts given: the lattice and the sums run on them (widened to ft) instead of on the restated
    emission.  normaliser = "P" divides gamma and xi by P_u instead of Z_u: NOT the definition, there for
    test_estep_log_host to show the difference.  Returns a dict: logb [F][N], posts[p] [F][N][M_p], gamma, la,
    lbe [F][N], loglik[U], logZ[U], utt (the per-utterance lattice dicts) and stats[p] (dicts of BLOCKS)."""
    if ft is np.longdouble:
        need_extended()
    N = hms[0].N
    lens = [int(T) for T in lens]
    F = sum(lens)
    if logb is None:
        logb = R.log_b(hms, Xs).astype(ft)
        posts = [posteriors(hm, X, ft) for hm, X in zip(hms, Xs)]
    else:
        logb = np.asarray(logb).astype(ft).reshape(F, N)
        posts = [np.asarray(p).astype(ft).reshape(F, N, hm.M) for p, hm in zip(posts, hms)]
    common = {"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)}
    gamma, la, lbe = (np.zeros((F, N), ft) for _ in range(3))
    ll, lz, utt = np.zeros(len(lens), ft), np.zeros(len(lens), ft), []
    o = 0
    with np.errstate(all="ignore"):
        for u, T in enumerate(lens):
            r = lattice_fb(hms[0].A, logb[o:o + T], delta, ft)
            if normaliser == "P" and T and np.isfinite(r["logZ"]) and np.isfinite(r["logP"]):
                k = np.exp(r["logZ"] - r["logP"])
                r["gamma"], r["xi"] = r["gamma"] * k, r["xi"] * k
            utt.append(r)
            gamma[o:o + T], la[o:o + T], lbe[o:o + T] = r["gamma"], r["la"], r["lbe"]
            ll[u], lz[u] = r["logP"], r["logZ"]
            common["num_a"] += r["xi"]
            common["den_a"] += r["gamma"][:-1].sum(0)
            common["den_c"] += r["gamma"].sum(0)
            o += T
        common["loglik"] = ll.sum() if len(lens) else ft(0)
        common["n_utt"] = ft(len(lens))
        stats = []
        for hm, X, post in zip(hms, Xs, posts):
            st = dict(common)
            st.update(mix_sums(gamma[:, :, None] * post, X, hm.mean, ft))
            stats.append(st)
    return {"logb": logb, "posts": posts, "gamma": gamma, "la": la, "lbe": lbe, "loglik": ll, "logZ": lz,
            "utt": utt, "stats": stats}


@functools.lru_cache(maxsize=None)
def _reference(G, name, far, delta, ft):
    case = make(G, name, far)
    ref = estep(case.words[0], case.Xs, case.lens, delta, ft)
    for a in [ref[k] for k in ("logb", "gamma", "la", "lbe", "loglik", "logZ")] + ref["posts"]:
        a.setflags(write=False)
    return case, ref


def reference(G, name, far=True, delta=1, ft=np.longdouble):
    """(Case, estep's dict) of a name, computed once and left unchanged"""
    return _reference(G, name, far, delta, ft)


# ------------------------------------------------------------- distances

def block_dist(got, ref):
    """the smallest d with |got - ref| <= d (|ref| + 1e-5 max|ref|) over the finite entries of ref (the shape
    of fullcov_support.assert_close's bar, whose floor 1e-13 is RTOL x 1e-5); non-finite entries must agree in
    kind.  Both are
    taken as float64 holds them: a long double below float64's range is 0"""
    got, ref = (np.asarray(x, dtype=np.float64).astype(np.longdouble).ravel() for x in (got, ref))   # as float64 holds them
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "infinities differ"
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    scale = np.abs(ref[fin]).max()
    if scale == 0:
        assert np.all(got[fin] == 0), "a block of zeros is not met exactly"
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / (np.abs(ref[fin]) + 1e-5 * scale)).max())


def row_dist(got, ref):
    """block_dist with every row (a state's posteriors, a frame's gammas) as a block of its own"""
    got, ref = np.asarray(got), np.asarray(ref)
    return max((block_dist(g, r) for g, r in zip(got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]))),
               default=0.0)
