"""Host numerics of the full-covariance trainer (TFF = train/source/hmm-full-fs/
hmm_continuous_full_fs.c): ghmm_inv_cov_full, ghmm_mstep_full_host and ghmm_init_model_full
against a plain-Python restatement in the reference's loop order (CPU only).

The restatement uses float64 scalars in TFF's association order and the library is built without
fused multiply-adds, so the two agree bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

FLOOR = 1.0e-5


# ------------------------------------------------------------- restatement of TFF

def ref_inv_cov(cov):
    """inv_cov_matrix (TFF:2164-2202): decomposition, calc_det, isnan -> 0, inv_triang_matrix
    (numpy float64 scalars: IEEE division by zero as in C)"""
    with np.errstate(all="ignore"):
        return _ref_inv_cov(cov)


def _ref_inv_cov(cov):
    D = cov.shape[0]
    z = np.float64(0.0)
    a = [[np.float64(v) for v in row] for row in cov]
    d = [z] * D
    t = [[z] * D for _ in range(D)]
    for i in range(D):
        t[i][i] = 1.0
    d[0] = a[0][0]
    for i in range(1, D):
        t[i][0] = a[i][0] / d[0]
    for j in range(1, D - 1):
        d[j] = a[j][j]
        for k in range(j):
            d[j] -= t[j][k] * t[j][k] * d[k]
        for i in range(j + 1, D):
            t[i][j] = a[i][j]
            for k in range(j):
                t[i][j] -= t[i][k] * d[k] * t[j][k]
            t[i][j] /= d[j]
    j = D - 1
    d[j] = a[j][j]
    for k in range(j):
        d[j] -= t[j][k] * t[j][k] * d[k]
    det = np.float64(1.0)
    for v in d:
        det *= v
    if np.isnan(det):
        det = 0.0
    if det != 0.0:
        im = [[z] * D for _ in range(D)]
        for i in range(D):
            im[i][i] = 1.0
        for k in range(D - 1):
            for i in range(k + 1, D):
                jj = i - k - 1
                im[i][jj] = 0.0
                for l in range(jj, i):
                    im[i][jj] -= t[i][l] * im[l][jj]
        for i in range(D):
            a[i][i] = 0.0
            for jj in range(i, D):
                a[i][i] += im[jj][i] * im[jj][i] / d[jj]
        for i in range(D - 1):
            for jj in range(i + 1, D):
                a[i][jj] = 0.0
                for k in range(jj, D):
                    a[i][jj] += im[k][i] * im[k][jj] / d[k]
                a[jj][i] = a[i][jj]
    return float(det), np.array(a, dtype=np.float64)


def ref_sorting(v):
    idx = list(range(len(v)))
    done = False
    while not done:
        done = True
        for i in range(len(v) - 1):
            if v[idx[i]] < v[idx[i + 1]]:
                idx[i], idx[i + 1] = idx[i + 1], idx[i]
                done = False
    return idx


def ref_mstep(hm, v, delta=1):
    """main's M-step, TFF:306-341, on copies of hm's arrays"""
    N, M, D = hm.N, hm.M, hm.D
    G, DT = N * M, D * (D + 1) // 2
    A, c, mean, cov, det = (x.copy() for x in (hm.A, hm.c, hm.mean, hm.inv_cov, hm.det))
    o = 0
    num_a = v[o:o + N * N].reshape(N, N); o += N * N
    den_a = v[o:o + N]; o += N
    den_c = v[o:o + N]; o += N
    num_c = v[o:o + G].reshape(N, M); o += G
    num_mu = v[o:o + G * D].reshape(N, M, D); o += G * D
    num_cov = v[o:o + G * DT].reshape(N, M, DT)
    for i in range(N):
        if den_a[i] != 0.0:
            for j in range(N):
                A[i, j] = num_a[i, j] / den_a[i] if i <= j <= i + delta else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(N):
            if den_c[i] == 0.0:
                continue
            for j in range(M):
                c[i, j] = num_c[i, j] / den_c[i]
                q = 0
                for k in range(D):
                    mean[i, j, k] = num_mu[i, j, k] / num_c[i, j]
                    for l in range(k, D):
                        cov[i, j, k, l] = num_cov[i, j, q] / num_c[i, j]
                        q += 1
                for k in range(D):
                    if cov[i, j, k, k] < FLOOR:
                        cov[i, j, k, k] = FLOOR
                for k in range(1, D):
                    for l in range(k):
                        cov[i, j, k, l] = cov[i, j, l, k]
    for i in range(N):
        s = 0.0
        for k in range(M):
            if c[i, k] < FLOOR:
                c[i, k] = FLOOR
            s += c[i, k]
        for k in range(M):
            c[i, k] /= s
    for i in range(N):
        for k in range(M):
            if D > 1:
                det[i, k], cov[i, k] = ref_inv_cov(cov[i, k])
            else:
                det[i, k] = cov[i, k, 0, 0]
                cov[i, k, 0, 0] = 1.0 / cov[i, k, 0, 0]
        if D > 1:  # treat_zero_det, TFF:2226-2265
            idx = ref_sorting([det[i, j] for j in range(M)])
            n = 0
            for j in range(M):
                if det[i, j] < 1e-20:
                    l = idx[n]
                    n += 1
                    for k in range(D):
                        mean[i, j, k] = mean[i, l, k] * 1.05
                    for k in range(D):
                        mean[i, l, k] = mean[i, l, k] * 0.95
                    cov[i, j] = cov[i, l].copy()
                    det[i, j] = det[i, l]
                    c[i, l] /= 2.0
                    c[i, j] = c[i, l]
            s = 0.0
            for j in range(M):
                s += c[i, j]
            for j in range(M):
                c[i, j] /= s
    return A, c, mean, cov, det


def assert_same(got, ref):
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)


# ------------------------------------------------------------- fixtures / helpers

def start_model(G, rng, N, M, D):
    A = np.zeros((N, N))
    for i in range(N - 1):
        A[i, i] = A[i, i + 1] = 0.5
    A[-1, -1] = 1.0
    c = rng.dirichlet(np.full(M, 3.0), N)
    mean = rng.normal(0.0, 1.0, (N, M, D))
    ic = np.empty((N, M, D, D))
    for i in range(N):
        for k in range(M):
            Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
            ic[i, k] = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    return G.HostFullModel(A, c, mean, ic, 1.0 / np.linalg.det(ic), word="w")


def stats_from_frames(G, rng, hm, F=200):
    """a statistics vector as calc_mix_param would accumulate it, from random weights"""
    N, M, D = hm.N, hm.M, hm.D
    X = rng.normal(0.0, 1.0, (F, D))
    w = rng.uniform(0.0, 1.0, (F, N, M))
    iu = np.triu_indices(D)
    s = {"num_a": np.zeros((N, N)), "den_a": np.zeros(N), "den_c": np.zeros(N)}
    for i in range(N):
        s["num_a"][i, i] = rng.uniform(1, 5)
        if i + 1 < N:
            s["num_a"][i, i + 1] = rng.uniform(0.1, 1)
        s["den_a"][i] = s["num_a"][i].sum()
        s["den_c"][i] = w[:, i].sum()
    num_c = w.sum(0)
    num_mu = np.einsum("fnm,fd->nmd", w, X)
    dif = X[:, None, None, :] - hm.mean[None]
    num_cov = np.einsum("fnm,fnmk,fnml->nmkl", w, dif, dif)[..., iu[0], iu[1]]
    v = np.concatenate([s["num_a"].ravel(), s["den_a"], s["den_c"], num_c.ravel(), num_mu.ravel(),
                        num_cov.ravel(), [-123.0, 4.0]])
    assert v.size == G.stats_len_full(N, M, D)
    return v


def offs(G, N, M, D):
    G_ = N * M
    o = {"den_c": N * N + N, "num_c": N * N + 2 * N}
    o["num_mu"] = o["num_c"] + G_
    o["num_cov"] = o["num_mu"] + G_ * D
    return o


# ------------------------------------------------------------------- the tests

def test_stats_len_full(G):
    lib = G.host_lib()
    for N, M, D in ((1, 1, 1), (6, 1, 9), (20, 8, 39), (64, 3, 48)):
        assert lib.ghmm_stats_len_full(N, M, D) == G.stats_len_full(N, M, D) == \
            N * N + 2 * N + N * M * (1 + D + D * (D + 1) // 2) + 2


@pytest.mark.parametrize("D", [2, 3, 9, 16, 39])
def test_inv_cov_spd(G, D):
    rng = np.random.default_rng(D)
    B = rng.normal(size=(D, D))
    S = B @ B.T + D * np.eye(D)
    det, inv = G.inv_cov_full(S)
    rdet, rinv = ref_inv_cov(S)
    assert det == rdet
    np.testing.assert_array_equal(inv, rinv)
    assert det == pytest.approx(np.linalg.det(S), rel=1e-10)
    np.testing.assert_allclose(inv, np.linalg.inv(S), rtol=1e-9, atol=1e-12)


def test_inv_cov_rank_deficient_and_nan(G):
    # a zero pivot: det = 0, the matrix is left as it came (TFF:2179)
    S = np.array([[1.0, 1.0, 0.5], [1.0, 1.0, 0.5], [0.5, 0.5, 2.0]])
    det, out = G.inv_cov_full(S)
    assert det == 0.0 and ref_inv_cov(S)[0] == 0.0
    np.testing.assert_array_equal(out, S)
    # NaN determinant -> 0 (TFF:2176), matrix left alone as well
    S = np.array([[2.0, np.nan], [np.nan, 3.0]])
    det, out = G.inv_cov_full(S)
    assert det == 0.0
    np.testing.assert_array_equal(np.isnan(out), np.isnan(S))
    assert out[0, 0] == 2.0 and out[1, 1] == 3.0


@pytest.mark.parametrize("N,M,D", [(4, 3, 5), (3, 2, 1), (5, 1, 9)])
def test_mstep_matches_restatement(G, N, M, D):
    rng = np.random.default_rng(100 * N + 10 * M + D)
    hm = start_model(G, rng, N, M, D)
    v = stats_from_frames(G, rng, hm)
    got = hm.mstep(v)
    assert_same(got.arrays()[:2], ref_mstep(hm, v)[:2])
    ref = ref_mstep(hm, v)
    for g, r in zip((got.A, got.c, got.mean, got.inv_cov, got.det), ref):
        np.testing.assert_array_equal(g, r)
    # a well-conditioned result is a real inverse
    if D > 1:
        cov = np.linalg.inv(got.inv_cov[0, 0])
        assert np.linalg.det(cov) == pytest.approx(got.det[0, 0], rel=1e-9)


@pytest.mark.parametrize("M", [1, 3])
def test_treat_zero_det(G, M):
    """Gaussian 0 of state 1 gets a rank-deficient covariance (det = 0 < 1e-20): with M = 1 it is
    split with itself (mean x 1.05 x 0.95, weight unchanged), with M = 3 it takes the largest-det
    Gaussian's parameters."""
    N, D = 3, 4
    rng = np.random.default_rng(7 + M)
    hm = start_model(G, rng, N, M, D)
    v = stats_from_frames(G, rng, hm)
    o = offs(G, N, M, D)
    g = 1 * M + 0
    DT = D * (D + 1) // 2
    nc = v[o["num_c"] + g]
    # covariance = u u' (rank 1, diagonal above the floor): num_cov = nc * u u'
    u = np.array([1.0, 2.0, -1.0, 0.5])
    iu = np.triu_indices(D)
    v[o["num_cov"] + g * DT:o["num_cov"] + (g + 1) * DT] = nc * np.outer(u, u)[iu]
    got = hm.mstep(v)
    ref = ref_mstep(hm, v)
    for a, b in zip((got.A, got.c, got.mean, got.inv_cov, got.det), ref):
        np.testing.assert_array_equal(a, b)
    mean_new = v[o["num_mu"] + g * D:o["num_mu"] + (g + 1) * D] / nc
    if M == 1:
        np.testing.assert_array_equal(got.mean[1, 0], mean_new * 1.05 * 0.95)
        assert got.c[1, 0] == 1.0
        assert got.det[1, 0] == 0.0
    else:
        assert got.det[1, 0] > 1e-20  # took another Gaussian's det
        l = int(np.argmax([ref_inv_cov_det(hm, v, 1, k) for k in range(M)]))
        np.testing.assert_array_equal(got.inv_cov[1, 0], got.inv_cov[1, l])
        assert got.c[1, 0] == got.c[1, l]


def ref_inv_cov_det(hm, v, i, k):
    return ref_mstep(hm, v)[4][i, k]


def test_den_c_zero_reinverts(G):
    """a state with den_c == 0 keeps its matrix slot (an inverse) and main inverts it again: the
    slot then holds the covariance, det is that of the inverse (TFF:1963, 326)"""
    N, M, D = 3, 2, 3
    rng = np.random.default_rng(11)
    hm = start_model(G, rng, N, M, D)
    v = stats_from_frames(G, rng, hm)
    o = offs(G, N, M, D)
    v[o["den_c"] + 2] = 0.0
    got = hm.mstep(v)
    ref = ref_mstep(hm, v)
    for a, b in zip((got.A, got.c, got.mean, got.inv_cov, got.det), ref):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got.mean[2], hm.mean[2])
    for k in range(M):
        np.testing.assert_allclose(got.inv_cov[2, k], np.linalg.inv(hm.inv_cov[2, k]), rtol=1e-9, atol=1e-12)
        assert got.det[2, k] == pytest.approx(np.linalg.det(hm.inv_cov[2, k]), rel=1e-9)


def test_num_c_zero_gives_nan(G):
    # D = 1: no treat_zero_det, which would otherwise replace the NaN Gaussian (its det -> 0)
    N, M, D = 2, 2, 1
    rng = np.random.default_rng(12)
    hm = start_model(G, rng, N, M, D)
    v = stats_from_frames(G, rng, hm)
    o = offs(G, N, M, D)
    g = 1
    DT = D * (D + 1) // 2
    v[o["num_c"] + g] = 0.0
    v[o["num_mu"] + g * D:o["num_mu"] + (g + 1) * D] = 0.0
    v[o["num_cov"] + g * DT:o["num_cov"] + (g + 1) * DT] = 0.0
    got = hm.mstep(v)
    assert np.isnan(got.mean[0, 1]).all()  # 0 / 0
    ref = ref_mstep(hm, v)
    for a, b in zip((got.A, got.c, got.mean, got.inv_cov, got.det), ref):
        np.testing.assert_array_equal(a, b)


def ref_init_m1(X, lens, N):
    """creating_initial_model with one mixture (TFF:810-952): uniform segmentation, the state's
    mean, the covariance around it, inv_cov_matrix"""
    D = X.shape[1]
    sums = np.zeros((N, D)); cnt = np.zeros(N, dtype=int)
    f0 = 0
    segs = []
    for T in lens:
        q, r = divmod(T, N)
        end = 0
        for k in range(N):
            b = end
            end += q + 1 if k < r else q
            segs.append((k, f0 + b, f0 + end))
        f0 += T
    for k, b, e in segs:
        for t in range(b, e):
            for l in range(D):
                sums[k, l] += X[t, l]
            cnt[k] += 1
    mean = sums / cnt[:, None]
    cov = np.zeros((N, D, D))
    for k, b, e in segs:
        for t in range(b, e):
            dif = [X[t, l] - mean[k, l] for l in range(D)]
            for i in range(D):
                for l in range(i, D):
                    cov[k, i, l] += dif[i] * dif[l]
    det = np.zeros(N)
    for k in range(N):
        for i in range(D):
            for l in range(i, D):
                cov[k, i, l] /= cnt[k]
        for i in range(D):
            if cov[k, i, i] < FLOOR:
                cov[k, i, i] = FLOOR
        for i in range(1, D):
            for l in range(i):
                cov[k, i, l] = cov[k, l, i]
        det[k], cov[k] = ref_inv_cov(cov[k])
    return mean, cov, det


def test_init_model_full_shipped_perfil(G):
    X = G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil"))
    N = 6
    hm = G.Context.init_model_full(X, [len(X)], N, 1)
    mean, cov, det = ref_init_m1(X, [len(X)], N)
    np.testing.assert_array_equal(hm.mean[:, 0], mean)
    np.testing.assert_array_equal(hm.inv_cov[:, 0], cov)
    np.testing.assert_array_equal(hm.det[:, 0], det)
    assert np.all(hm.c == 1.0)
    A = np.zeros((N, N))
    for i in range(N):
        A[i, i] = 0.5 if i < N - 1 else 1.0
        if i < N - 1:
            A[i, i + 1] = 0.5
    np.testing.assert_array_equal(hm.A, A)


def test_init_model_full_mixtures(G):
    """M = 3 on two utterances: weights are the cells' shares (floored, renormalised), every cell
    covariance is symmetric, and the stored matrices are inverses of SPD covariances"""
    X1 = G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_200_f_02_ap_015.perfil"))
    X2 = G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_200_f_02_ap_030.perfil"))
    X = np.concatenate([X1, X2])
    hm = G.HostFullModel.init_from(X, [len(X1), len(X2)], 4, 3)
    np.testing.assert_allclose(hm.c.sum(1), 1.0, rtol=1e-12)
    assert np.all(hm.c >= 1e-5 / 1.1)
    np.testing.assert_array_equal(hm.inv_cov, np.swapaxes(hm.inv_cov, -1, -2))
    fin = hm.det > 0
    assert fin.any()
    for i, k in zip(*np.nonzero(fin)):
        assert np.linalg.det(np.linalg.inv(hm.inv_cov[i, k])) == pytest.approx(hm.det[i, k], rel=1e-6)
