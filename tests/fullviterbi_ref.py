"""numpy restatement of the full-covariance Viterbi's log emission (include/ghmm.h,
ghmm_viterbi_full): the diagonal Viterbi's definition (oracle/ghmm_oracle.c, orc_log_emission)
with the full quadratic form in calc_gaus's direct form (RC:902-954).  Shared by
test_fullviterbi_host.py and test_fullviterbi_gpu.py; the lattice itself is the pinned oracle's
(oracle_lib.viterbi_lattice)."""
import numpy as np


def log_emission(hm, X):
    """log b[F][N] of a HostFullModel:
        lk = log(c) - log(den),  den = pow(2 pi, D/2.0) * pow(|det|, 0.5)
        e_m = lk_m - aux_m / 2,  aux = sum_i dif[i] * (sum_j dif[j] * inv_cov[j][i])
        log b = m + log(sum_m exp(e_m - m)), m = max of the non-NaN e_m; -inf when m is -inf"""
    D = hm.D
    dif = X[:, None, None, :] - hm.mean[None]                       # F N M D
    t = np.einsum("fnmj,nmji->fnmi", dif, hm.inv_cov)
    aux = np.einsum("fnmi,fnmi->fnm", dif, t)
    den = pow(2.0 * np.pi, D / 2.0) * np.power(np.abs(hm.det), 0.5)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        lk = np.log(hm.c) - np.log(den)
        e = lk[None] - 0.5 * aux
        m = np.where(np.isnan(e), -np.inf, e).max(-1)
        s = np.exp(e - m[..., None]).sum(-1)
        return np.where(m == -np.inf, -np.inf, m + np.log(s))


def close_logb(got, ref, rtol):
    """equal NaN and infinity patterns, finite values within rtol * (1 + |ref|)"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "infinities differ"
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]) / (1.0 + np.abs(ref[fin]))
    assert err.size == 0 or err.max() <= rtol, f"max error {err.max():.3e}"


def lattice_margins(A, logb, path):
    """the gap between the best and the second-best predecessor at every step of `path` (the
    back-pointers the path follows), relative to 1 + |best|: a small one is a near-tie that
    rounding may flip"""
    with np.errstate(divide="ignore", invalid="ignore"):
        la = np.where(A > 0, np.log(np.where(A > 0, A, 1.0)), -np.inf)
        T, N = logb.shape
        d = np.where(np.arange(N) == 0, 0.0, -np.inf) + logb[0]
        gaps = []
        for t in range(1, T):
            cand = d[:, None] + la
            j = path[t]
            col = np.sort(cand[:, j])[::-1]
            if N > 1 and np.isfinite(col[1]):
                gaps.append((col[0] - col[1]) / (1.0 + abs(col[0])))
            d = cand.max(0) + logb[t]
    return np.array(gaps)
