"""numpy restatement of the full-covariance trainer's E-step (TFF = train/source/hmm-full-fs/
hmm_continuous_full_fs.c) in a chosen float type, extended precision by default.  Shared by
test_fulltrain_ref_host.py, which pins it to the real reference's recorded runs and to the pinned
diagonal oracle, and by test_fullestep_gpu.py, which holds the HIP E-step against it.  Plain
numpy, no GPU, Gaussian by Gaussian (an array over frames x Gaussians x D x D in long double does
not fit in memory at the shapes the GPU tests run).

What is restated:
  calc_symbol_probab / calc_gaus (TFF:1775-1887): dif = x - mu, t_i = sum_j dif[j] inv_cov[j][i],
      aux = sum_i dif[i] t_i, gaus = exp(-aux / 2) / den, den = pow(2 pi, D / 2.0) sqrt(|det|);
      a density of +inf becomes 1e20 unless den == 0; b = sum_m c_m gaus_m; post = c gaus / b, or 0
      where b == 0
  calc_alpha from a one-hot start, calc_beta with beta[T-1][N-1] = c[T-1], both over the full
      matrix A; gamma = alpha beta / c
  calc_transition_probab: num_a[i][j] for i <= j <= i + delta only; den_a, den_c
  calc_probability: log P = -sum_t log c_t + log alpha[T-1][N-1]
  calc_mix_param (TFF:1714-1753): num_c, num_mu, num_cov around the OLD mean, num_cov as the
      upper triangle row-major (numpy.triu_indices order)
An utterance of no frames adds nothing.

The reference program computes in double, where exp overflows above 1.8e308; long double does not
overflow there.  `+inf` is therefore read as "beyond the largest double": with ft = float64 that
is the reference's own test, with ft = longdouble it marks the same densities.

gaussians() is the one Gaussian-by-Gaussian quadratic form in ft: the log-domain restatements
(fulllogscore_ref, fullestep_log_ref) are built on it too.  np_estep and np_quadform are the separate,
vectorised float64 family (with fullscore_ref.np_emission / np_logp and fullviterbi_ref.log_emission),
which the host tests hold the ft family against and which is itself pinned to the recorded runs.

The linear E-step's GPU cases (CASES, SWEEP, build) and the EM cases (EM_CASES, em_corpus,
linear_trajectory) live here; a long-double reference is computed once a session."""
import functools

import numpy as np

from fullcov_support import need_extended, rand_fmodel, walk_any

STAT_KEYS = ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_cov")
_DBL_MAX = np.finfo(np.float64).max


def gaussians(hm, Xf, ft):
    """(i, k, aux[F], den) of every Gaussian in turn, over the frames Xf[F][D] (already of type ft)"""
    two_pi = ft(2.0 * np.pi)  # TFF's 2 * M_PI: the double constant
    for i in range(hm.N):
        for k in range(hm.M):
            dif = Xf - hm.mean[i, k].astype(ft)
            t = dif @ hm.inv_cov[i, k].astype(ft)         # t_i = sum_j dif[j] inv_cov[j][i]
            aux = np.einsum("fi,fi->f", dif, t)
            den = two_pi ** ft(hm.D / 2.0) * np.sqrt(np.abs(ft(hm.det[i, k])))
            yield i, k, aux, den


def _densities(hm, Xf, ft):
    """c * gaus of every frame and Gaussian, [F][N][M]"""
    gm = np.zeros((len(Xf), hm.N, hm.M), ft)
    for i, k, aux, den in gaussians(hm, Xf, ft):
        e = np.exp(aux * ft(-0.5))
        g = e / den
        if den != 0:
            g = np.where((e > _DBL_MAX) | (g > _DBL_MAX), ft(1e20), g)
        gm[:, i, k] = g * ft(hm.c[i, k])
    return gm


def mix_sums(w, Xf, mean, ft):
    """calc_mix_param (TFF:1714-1753) on the weights w[F][N][M] = gamma * post: num_c, num_mu and
    num_cov around `mean`, the upper triangle row-major"""
    N, M, D = mean.shape
    iu = np.triu_indices(D)
    cov = np.zeros((N, M, len(iu[0])), ft)
    for i in range(N):
        for k in range(M):
            dif = Xf - mean[i, k].astype(ft)
            cov[i, k] = np.einsum("f,fk,fk->k", w[:, i, k], dif[:, iu[0]], dif[:, iu[1]])
    return {"num_c": w.sum(0), "num_mu": np.einsum("fnm,fd->nmd", w, Xf), "num_cov": cov}


def estep(hm, X, lens, delta=1, ft=np.longdouble):
    """One E-step of TFF over the utterances `lens` of X[F][D] under the HostFullModel hm.
    Returns a dict: b[F][N], post[F][N][M], gamma, alpha, beta [F][N], loglik[U] (per utterance)
    and stats (num_a, den_a, den_c, num_c, num_mu, num_cov, loglik, n_utt), all of dtype ft."""
    if ft is np.longdouble:
        need_extended()
    N, M, D = hm.N, hm.M, hm.D
    lens = [int(T) for T in lens]
    F = sum(lens)
    X = np.asarray(X, dtype=np.float64).reshape(F, D)
    Xf, A = X.astype(ft), hm.A.astype(ft)
    with np.errstate(all="ignore"):
        gm = _densities(hm, Xf, ft)
        b = gm.sum(-1)
        post = np.where(b[..., None] != 0, gm / np.where(b[..., None] != 0, b[..., None], 1), ft(0))
        st = {"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)}
        gamma, alpha, beta = (np.zeros((F, N), ft) for _ in range(3))
        ll = np.zeros(len(lens), ft)
        e0 = np.zeros(N, ft)
        e0[0] = 1
        o = 0
        for u, T in enumerate(lens):
            if T == 0:
                continue
            bb = b[o:o + T]
            al, c = np.zeros((T, N), ft), np.zeros(T, ft)
            for t in range(T):
                a = (e0 if t == 0 else al[t - 1] @ A) * bb[t]
                c[t] = 1 / a.sum()
                al[t] = a * c[t]
            be = np.zeros((T, N), ft)
            be[T - 1, N - 1] = c[T - 1]
            for t in range(T - 2, -1, -1):
                be[t] = (A @ (be[t + 1] * bb[t + 1])) * c[t]
            ga = al * be / c[:, None]
            alpha[o:o + T], beta[o:o + T], gamma[o:o + T] = al, be, ga
            for i in range(N):
                for j in range(i, min(N, i + delta + 1)):
                    st["num_a"][i, j] += np.sum(al[:-1, i] * A[i, j] * bb[1:, j] * be[1:, j])
            st["den_a"] += ga[:-1].sum(0)
            st["den_c"] += ga.sum(0)
            ll[u] = -np.log(c).sum() + np.log(al[T - 1, N - 1])
            o += T
        st.update(mix_sums(gamma[:, :, None] * post, Xf, hm.mean, ft))
        st["loglik"] = ll.sum() if len(lens) else ft(0)
        st["n_utt"] = ft(len(lens))
    return {"b": b, "post": post, "gamma": gamma, "alpha": alpha, "beta": beta, "loglik": ll, "stats": st}


def pack(st):
    """the statistics dict as the flat float64 vector of ghmm_stats_create_full"""
    return np.concatenate([np.asarray(st[k], dtype=np.float64).ravel() for k in STAT_KEYS] +
                          [[float(st["loglik"]), float(st["n_utt"])]])


def stats_from(gamma, post, X, mean, ft=np.longdouble):
    """calc_mix_param's sums from GIVEN weights: gamma[F][N] and post[F][N*M] are used as they are.
    w = gamma * post and dif = x - mu are formed in float64, as the statistics kernel forms them,
    then widened to ft; the products and the sums are taken in ft.  Returns (sums, abs_sums): two
    dicts of num_c[N][M], num_mu[N][M][D], num_cov[N][M][D(D+1)/2], the second holding for every
    entry the sum of the absolute values of its terms
        num_c: w      num_mu[k]: w * x[k]      num_cov[k][l]: (w * dif[k]) * dif[l]"""
    if ft is np.longdouble:
        need_extended()
    N, M, D = mean.shape
    F = len(X)
    X = np.asarray(X, dtype=np.float64).reshape(F, D)
    gamma = np.asarray(gamma, dtype=np.float64).reshape(F, N)
    post = np.asarray(post, dtype=np.float64).reshape(F, N, M)
    iu = np.triu_indices(D)
    DT = len(iu[0])
    s = {"num_c": np.zeros((N, M), ft), "num_mu": np.zeros((N, M, D), ft), "num_cov": np.zeros((N, M, DT), ft)}
    a = {k: np.zeros_like(v) for k, v in s.items()}
    Xf = X.astype(ft)
    with np.errstate(all="ignore"):
        for i in range(N):
            for k in range(M):
                w64 = gamma[:, i] * post[:, i, k]
                nz = np.nonzero(w64 != 0.0)[0]      # (a weight of exactly 0 adds exactly 0)
                w = w64[nz].astype(ft)
                dif = (X[nz] - mean[i, k]).astype(ft)
                s["num_c"][i, k] = w.sum()
                a["num_c"][i, k] = np.abs(w).sum()
                t = w[:, None] * Xf[nz]
                s["num_mu"][i, k] = t.sum(0)
                a["num_mu"][i, k] = np.abs(t).sum(0)
                t = (w[:, None] * dif)[:, iu[0]] * dif[:, iu[1]]
                s["num_cov"][i, k] = t.sum(0)
                a["num_cov"][i, k] = np.abs(t).sum(0)
    return s, a


def model_err(hm, ref_of):
    """check_run's metric: the largest relative difference of A, c, mean, det, and of inv_cov per
    Gaussian as max|d| / max|ref|"""
    worst = 0.0
    for key in ("A", "c", "mean", "det"):
        g, r = getattr(hm, key), ref_of(key)
        assert np.array_equal(r == 0.0, g == 0.0), key
        nz = r != 0.0
        worst = max(worst, float(np.max(np.abs(g[nz] - r[nz]) / np.abs(r[nz]))))
    ic, ric = hm.inv_cov, ref_of("inv_cov")
    for i in range(hm.N):
        for k in range(hm.M):
            worst = max(worst, float(np.abs(ic[i, k] - ric[i, k]).max() / np.abs(ric[i, k]).max()))
    return worst


# ------------------------------------------------ several EM iterations beyond the reference's caps
# (N, M, D, utterances, frames each).  Larger is not better: 20 x 2 x 39 on 15 000 frames leaves
# the finite numbers at the third iteration in the reference's own arithmetic (375 frames per
# Gaussian are too few at D = 39).
EM_CASES = [(12, 2, 24, 24, 400), (6, 2, 48, 16, 400)]


def em_corpus(N, M, D, U, T):
    """U left-to-right walks of T frames through a random full-covariance model (covariance
    eigenvalues 0.3..1.5, means N(0, 2)), values rounded to float32 as a .perfil file holds them"""
    rng = np.random.default_rng(N * 100 + D)
    mean = rng.normal(0.0, 2.0, (N, M, D))
    ch = np.empty((N, M, D, D))
    for i in range(N):
        for k in range(M):
            Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
            ch[i, k] = np.linalg.cholesky((Q * rng.uniform(0.3, 1.5, D)) @ Q.T)
    Xs = []
    for _ in range(U):
        cuts = np.sort(rng.choice(np.arange(1, T), N - 1, replace=False))
        s = np.searchsorted(cuts, np.arange(T), side="right")
        k = rng.integers(0, M, T)
        z = rng.normal(size=(T, D))
        Xs.append(mean[s, k] + np.einsum("tij,tj->ti", ch[s, k], z))
    X = np.concatenate(Xs).astype(np.float32).astype(np.float64)
    return X, np.full(U, T, dtype=np.int32)


def em_trajectory(G, X, lens, N, M, iterations, ft, estep=estep):
    """`iterations` x (estep in ft: this module's, or fullestep_log_ref's; the library's host M-step)
    from HostFullModel.init_from: the log-likelihood before every M-step and the last model"""
    hm = G.HostFullModel.init_from(X, lens, N, M)
    trace = []
    for _ in range(iterations):
        st = estep(hm, X, lens, 1, ft)["stats"]
        trace.append(float(st["loglik"]))
        hm = hm.mstep(pack(st), delta=1)
    return trace, hm


@functools.lru_cache(maxsize=None)
def linear_trajectory(G, case):
    """(corpus, lens, long-double trace, last model) of four iterations on EM_CASES[case], computed once"""
    N, M, D, U, T = EM_CASES[case]
    X, lens = em_corpus(N, M, D, U, T)
    return (X, lens) + em_trajectory(G, X, lens, N, M, 4, np.longdouble)


# ------------------------------------------------ the float64 family: TFF's E-step, vectorised

def np_quadform(hm, X):
    """(dif[F][N][M][D], aux[F][N][M], den[N][M]) in float64: aux = sum_i dif[i] (sum_j dif[j]
    inv_cov[j][i]), den = pow(2 pi, D/2.0) * pow(|det|, 0.5)"""
    dif = X[:, None, None, :] - hm.mean[None]
    aux = np.einsum("fnmi,fnmi->fnm", dif, np.einsum("fnmj,nmji->fnmi", dif, hm.inv_cov))
    return dif, aux, pow(2.0 * np.pi, hm.D / 2.0) * np.power(np.abs(hm.det), 0.5)


def np_estep(hm, X, lens):
    """calc_symbol_probab / calc_gaus (TFF:1775-1887), calc_alpha / calc_beta /
    calc_transition_probab / calc_den_mix_coef / calc_probability (the diagonal trainer's, final
    state included) and calc_mix_param (TFF:1714-1753), per utterance, summed"""
    N, M, D = hm.N, hm.M, hm.D
    G_, DT = N * M, D * (D + 1) // 2
    iu = np.triu_indices(D)
    with np.errstate(all="ignore"):
        dif, aux, den = np_quadform(hm, X)
        g = np.exp(aux * -0.5) / den[None]
        g = np.where((g == np.inf) & (den[None] != 0.0), 1e20, g)
        gm = g * hm.c[None]
        b = gm.sum(-1)
        post = np.where(b[..., None] != 0.0, gm / b[..., None], 0.0)
    st = {"num_a": np.zeros((N, N)), "den_a": np.zeros(N), "den_c": np.zeros(N), "loglik": 0.0}
    gamma = np.zeros((len(X), N))
    A = hm.A
    o = 0
    for T in lens:
        bb = b[o:o + T]
        al = np.zeros((T, N)); c = np.zeros(T)
        for t in range(T):
            a = (np.eye(N)[0] if t == 0 else al[t - 1] @ A) * bb[t]
            c[t] = 1.0 / a.sum()
            al[t] = a * c[t]
        be = np.zeros((T, N))
        be[T - 1, N - 1] = c[T - 1]
        for t in range(T - 2, -1, -1):
            be[t] = (A @ (be[t + 1] * bb[t + 1])) * c[t]
        ga = al * be / c[:, None]
        gamma[o:o + T] = ga
        for i in range(N):
            for j in (i, i + 1):
                if j < N:
                    st["num_a"][i, j] += np.sum(al[:-1, i] * A[i, j] * bb[1:, j] * be[1:, j])
        st["den_a"] += ga[:-1].sum(0)
        st["den_c"] += ga.sum(0)
        st["loglik"] += -np.log(c).sum() + np.log(al[T - 1, N - 1])
        o += T
    w = gamma[:, :, None] * post
    st["num_c"] = w.sum(0)
    st["num_mu"] = np.einsum("fnm,fd->nmd", w, X)
    st["num_cov"] = np.einsum("fnm,fnmk,fnml->nmkl", w, dif, dif)[..., iu[0], iu[1]].reshape(N, M, DT)
    st["n_utt"] = float(len(lens))
    return b, post.reshape(len(X), G_), gamma, st


# ------------------------------------------------ the linear E-step's shapes on the GPU

LENS1 = (70, 1, 33, 129)        # 233 frames: three tiles of 64 and one with 41 frames left
LENS2 = (90, 140, 64, 65)
LONG64 = (312, 388, 400, 300, 351, 333, 379, 364)

# id -> (N, M, D, lens, dense A, delta, clamped Gaussian)
CASES = {}
for _D in (8, 9, 17, 24, 25, 33, 40, 41, 47, 48):       # every DB of FC_POST, both sides of each boundary
    CASES[f"db-5x3x{_D}"] = (5, 3, _D, LENS1, False, 1, True)
for _N, _M, _D in ((17, 2, 13), (32, 2, 13), (33, 1, 13), (64, 2, 6)):  # lane classes 32 / 64, second grid row
    CASES[f"lanes-{_N}x{_M}x{_D}"] = (_N, _M, _D, LENS2, False, 1, False)
for _N, _M, _D in ((20, 2, 9), (40, 1, 5)):             # dense A: separate launches, general recursion
    for _delta in (1, 2):
        CASES[f"dense-{_N}x{_M}x{_D}-delta{_delta}"] = (_N, _M, _D, (60, 45, 81), True, _delta, False)
for _delta in (0, 3):                                    # the band of num_a
    CASES[f"band-6x2x7-delta{_delta}"] = (6, 2, 7, (50, 60, 9), True, _delta, False)
CASES["short-12x2x6"] = (12, 2, 6, (40, 5, 1, 0, 30), False, 1, False)   # T < N, T = 1, T = 0
CASES["paths-8x3x16"] = (8, 3, 16, LENS1, False, 1, False)
for _N, _M, _D in ((64, 4, 1), (64, 8, 1), (64, 3, 3)):  # FSn 16 / 8 / 16 in k_fullstats
    CASES[f"fsn-{_N}x{_M}x{_D}"] = (_N, _M, _D, (150, 200, 130), False, 1, False)
CASES["large-64x2x48"] = (64, 2, 48, LONG64, False, 1, False)
CASES["many-8x3x16"] = (8, 3, 16, (337, 120, 400, 256, 199, 311, 288, 143, 390, 222, 175, 264), False, 1, False)
SWEEP = [k for k in CASES if k != "many-8x3x16"]


@functools.lru_cache(maxsize=None)
def build(G, name):
    """(model, frames, lens, delta, the long-double E-step) of a case, computed once"""
    N, M, D, lens, dense, delta, clamp = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    if dense:
        A = rng.random((N, N)) + 0.05
        hm.A[:] = A / A.sum(1, keepdims=True)
    X = walk_any(rng, hm, lens)
    if clamp:
        # a non-positive-definite Gaussian: its density overflows to +inf on every frame and is
        # clamped to 1e20
        hm.inv_cov[4, 2] = -np.eye(D)
        hm.mean[4, 2] = hm.mean[4, 0] + 60.0
    ref = estep(hm, X, lens, delta, np.longdouble)
    ll = np.asarray(ref["loglik"], dtype=np.float64)
    for u, T in enumerate(lens):
        if T >= N:
            assert np.isfinite(ll[u]), (name, u)    # no case compares NaN with NaN by accident
    if clamp:
        assert np.any(ref["post"][:, 4, 2] > 0)
    return hm, X, np.asarray(lens, dtype=np.int32), delta, ref


def fs_geometry(N, M, D):
    """run_fullstats' launch geometry (ghmm_fullhost.hpp): frames staged per pass and the Gaussians
    [g0, g1] of every element batch"""
    G_, E1 = N * M, 1 + D + D * (D + 1) // 2
    batch = 256 * 8                                  # FS_THREADS * FS_EPT
    gwmax = min(batch // E1 + 2, G_)
    fsn = 32                                         # FS_FRAMES
    while fsn > 1 and fsn * (D + 1 + gwmax) * 8 > 48 * 1024:
        fsn //= 2
    E = G_ * E1
    return fsn, [(e0 // E1, (min(e0 + batch, E) - 1) // E1) for e0 in range(0, E, batch)]
