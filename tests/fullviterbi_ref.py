"""numpy restatement of the full-covariance Viterbi's log emission (include/ghmm.h,
ghmm_viterbi_full): the diagonal Viterbi's definition (oracle/ghmm_oracle.c, orc_log_emission)
with the full quadratic form in calc_gaus's direct form (RC:902-954).  Shared by
test_fullviterbi_host.py and test_fullviterbi_gpu.py; the lattice itself is the pinned oracle's
(oracle_lib.viterbi_lattice)."""
import numpy as np

from fulltrain_ref import np_quadform


def log_emission(hm, X):
    """log b[F][N] of a HostFullModel:
        lk = log(c) - log(den),  den = pow(2 pi, D/2.0) * pow(|det|, 0.5)
        e_m = lk_m - aux_m / 2,  aux = sum_i dif[i] * (sum_j dif[j] * inv_cov[j][i])
        log b = m + log(sum_m exp(e_m - m)), m = max of the non-NaN e_m; -inf when m is -inf"""
    _, aux, den = np_quadform(hm, X)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        lk = np.log(hm.c) - np.log(den)
        e = lk[None] - 0.5 * aux
        m = np.where(np.isnan(e), -np.inf, e).max(-1)
        s = np.exp(e - m[..., None]).sum(-1)
        return np.where(m == -np.inf, -np.inf, m + np.log(s))


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
