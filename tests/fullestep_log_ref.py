"""numpy restatement of the full-covariance log-domain E-step (include/ghmm.h, ghmm_estep_full_log)
in a chosen float type, long double by default.  Shared by test_fullestep_log_host.py, which pins it
to the long-double LINEAR E-step restatement (fulltrain_ref.estep), and by test_fullestep_log_gpu.py,
which holds the HIP kernels against it.  Plain numpy, no GPU.  The mixture terms e, their LSE, lse, the
forward step and lattice_bound are fulllogscore_ref's; calc_mix_param's sums are fulltrain_ref.mix_sums.

    e_m = lk_m - aux_m / 2,  log b = LSE_m e_m                       (fulllogscore_ref.log_emission)
    post_t(i,m) = exp(e_m - log b_i(t)), or 0 where log b_i(t) = -inf
    la_0(j)      = (j == 0 ? 0 : -inf) + log b_j(0)
    la_t(j)      = LSE_{i : a_ij > 0} (la_{t-1}(i) + log a_ij) + log b_j(t)
    lbe_{T-1}(i) = (i == N-1 ? 0 : -inf)
    lbe_t(i)     = LSE_{j : a_ij > 0} (log a_ij + (log b_j(t+1) + lbe_{t+1}(j)))
    log P_u = la_{T-1}(N-1);  log Z_u = LSE_j la_{T-1}(j)
    gamma_t(i) = exp(la_t(i) + lbe_t(i) - log Z_u)
    xi_t(i,j)  = exp(la_t(i) + log a_ij + log b_j(t+1) + lbe_{t+1}(j) - log Z_u), t < T-1, a_ij > 0,
                 i <= j <= i + delta
    num_a = sum xi;  den_a = sum_{t<T-1} gamma;  den_c = sum_{t<T} gamma;  calc_mix_param on gamma * post

The normaliser is log Z_u, not log P_u: TFF's gamma = alpha^ beta^ / c_t divides by the probability of
the observations over all end states, so a frame's gammas sum to rho_u = exp(log P_u - log Z_u) <= 1.
Where log Z_u is not finite the utterance's gamma and xi are 0.

The rounding bound of gamma and xi (float64, u = 2^-53), with V the largest finite |la| or |lbe| and
La the largest finite |log a_ij| of the utterance.  fulllogscore_ref.lattice_bound counts a forward
step at (3 V + La + N + 8) u.  A backward step carries two adds in front of its LSE (log b + lbe, then
+ log a_ij) where the forward step has one, so it counts (4 V + La + N + 8) u.  The exponent of
gamma_t(i), la_t(i) + lbe_t(i) - log Z, inherits t forward steps through la_t(i) and T - 1 - t
backward steps through lbe_t(i), T - 1 steps in all of at most (4 V + La + N + 8) u each, and through
log Z the T - 1 forward steps of the last row plus the final LSE: together below 2 T (4 V + La + N + 8) u.
The exponent of xi_t(i,j) inherits the same (la_t(i), lbe_{t+1}(j), log Z) and log a_ij's La u, which
the slack of V per forward step covers.  The exponent's own additions, three roundings of values
no larger than V each in turn (the running sum stays near a lattice value: la + lbe is near log Z),
add 3 V u:
    E = 2 T (4 V + La + N + 8) u + 3 V u
    |gamma - exact| <= exact * expm1(E) + 4 u        (exp at <= 2 ulp on a value <= 1 + E)
and the same per term of xi.  la, lbe and log P themselves are held to lattice_bound.

EM_MODEL_F64: four EM iterations with THIS E-step in float64 and the library's host M-step against the
long-double LINEAR trajectory (fulltrain_ref.em_trajectory), fulltrain_ref.model_err of the last model,
per entry of fulltrain_ref.EM_CASES, measured by test_fullestep_log_host.test_four_em_iterations (which
prints them; the trace distances were 6.9e-14 and 7.4e-14):
"""
import numpy as np

import fulllogscore_ref as LR
import fulltrain_ref as R
from fullcov_support import U53, ergodic, frames, need_extended, rand_fmodel
from fulllogscore_ref import lse

EM_MODEL_F64 = (8.7e-9, 1.5e-10)


def emission(hm, X, ft=np.longdouble):
    """(log b[F][N], post[F][N][M], e[F][N][M]) in ft; log b is fulllogscore_ref.log_emission's: the same
    two calls"""
    e = LR.mixture_terms(hm, X, ft)
    logb = LR.mixture_lse(e)
    return logb, posteriors(e, logb), e


def posteriors(e, logb):
    """exp(e - log b), 0 where log b = -inf"""
    ft = e.dtype.type
    with np.errstate(all="ignore"):
        lb = logb[..., None]
        return np.where(lb == -np.inf, ft(0), np.exp(e - np.where(lb == -np.inf, ft(0), lb)))


def gamma_exponent_bound(T, N, V, La):
    """E of the module docstring"""
    return 2.0 * T * (4.0 * V + La + N + LR.LATTICE_C) * U53 + 3.0 * V * U53


def _finmax(*arrays):
    v = 0.0
    for a in arrays:
        f = a[np.isfinite(a)]
        if f.size:
            v = max(v, float(np.abs(f).max()))
    return v


def lattice_fb(A, logb, delta=1, ft=np.longdouble):
    """one utterance from its log b[T][N] (any float type; widened to ft).  Returns a dict: la, lbe,
    gamma [T][N], xi[N][N] = sum_{t<T-1} xi_t inside the band, logP, logZ, and V, La of the bounds"""
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
        la, lbe = out["la"], out["lbe"]
        for t, row in enumerate(LR.forward_rows(terms, la_A, lb)):
            la[t] = row
        lbe[T - 1] = np.where(np.arange(N) == N - 1, ft(0), ft(-np.inf))
        w = np.zeros((T, N), ft)        # w[t] = log b(t+1) + lbe(t+1)
        for t in range(T - 2, -1, -1):
            w[t] = lb[t + 1] + lbe[t + 1]
            lbe[t] = lse((la_A + w[t][None, :]).T, terms.T)
        logP, logZ = la[T - 1, N - 1], lse(la[T - 1])
        out["logP"], out["logZ"] = logP, logZ
        out["V"], out["La"] = _finmax(la, lbe), float(np.abs(la_A).max())
        if np.isfinite(logZ):
            out["gamma"] = np.exp(la + lbe - logZ)
            for o in range(0, delta + 1):
                for i in range(N - o):
                    j = i + o
                    if terms[i, j]:
                        out["xi"][i, j] = np.exp(la[:T - 1, i] + la_A[i, j] + w[:T - 1, j] - logZ).sum()
    return out


def estep(hm, X, lens, delta=1, ft=np.longdouble, logb=None, post=None):
    """ghmm_estep_full_log restated over the utterances `lens` of X[F][D].  logb / post given: the
    lattice and the sums run on them (widened to ft) instead of on the restated emission.  Returns a
    dict like fulltrain_ref.estep's: logb, post [F][N][M], gamma, la, lbe [F][N], loglik[U], logZ[U],
    utt (the per-utterance lattice_fb dicts) and stats."""
    if ft is np.longdouble:
        need_extended()
    N, M, D = hm.N, hm.M, hm.D
    lens = [int(T) for T in lens]
    F = sum(lens)
    X = np.asarray(X, dtype=np.float64).reshape(F, D)
    Xf = X.astype(ft)
    if logb is None:
        logb, post, _ = emission(hm, X, ft)
    else:
        logb = np.asarray(logb).astype(ft).reshape(F, N)
        post = np.asarray(post).astype(ft).reshape(F, N, M)
    st = {"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)}
    gamma, la, lbe = (np.zeros((F, N), ft) for _ in range(3))
    ll, lz, utt = np.zeros(len(lens), ft), np.zeros(len(lens), ft), []
    o = 0
    with np.errstate(all="ignore"):
        for u, T in enumerate(lens):
            r = lattice_fb(hm.A, logb[o:o + T], delta, ft)
            utt.append(r)
            gamma[o:o + T], la[o:o + T], lbe[o:o + T] = r["gamma"], r["la"], r["lbe"]
            ll[u], lz[u] = r["logP"], r["logZ"]
            st["num_a"] += r["xi"]
            st["den_a"] += r["gamma"][:-1].sum(0)
            st["den_c"] += r["gamma"].sum(0)
            o += T
        st.update(R.mix_sums(gamma[:, :, None] * post, Xf, hm.mean, ft))
        st["loglik"] = ll.sum() if len(lens) else ft(0)
        st["n_utt"] = ft(len(lens))
    return {"logb": logb, "post": post, "gamma": gamma, "la": la, "lbe": lbe, "loglik": ll, "logZ": lz,
            "utt": utt, "stats": st}


# ------------------------------------------------ the shapes the GPU tests run

LATTICE_CASES = [k for k in sorted(LR.CASES) if not k.startswith("det0")]
# a T = 0 utterance and a dense A, run under delta 0, 2 and 3
EMPTY_CASE = (7, 2, 5, [40, 0, 25, 1, 3])
EMPTY_DELTAS = (0, 2, 3)


def make_empty_case(G):
    N, M, D, lens = EMPTY_CASE
    rng = np.random.default_rng(77)
    hm = rand_fmodel(G, rng, N, M, D, ergodic(rng, N), spread=1.0, asym=True)
    X = frames(rng, hm, lens)
    X[5] += 60.0
    return hm, X, np.asarray(lens, dtype=np.int32)
