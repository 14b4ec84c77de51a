"""CPU-side tests (no GPU) of the full-covariance Viterbi: the C ABI exports it, the Python face
binds it, and the numpy restatement of its log emission (fullviterbi_ref.py) is the pinned
oracle's formula (O.log_emission) when the inverse covariance is diagonal."""
import ctypes

import numpy as np

import oracle_lib as O
from fullcov_support import close_logb
from fullviterbi_ref import log_emission


def test_abi_exports_the_full_viterbi(G):
    lib = ctypes.CDLL(G.HIP_LIB)
    for name in ("ghmm_viterbi_full", "ghmm_viterbi_full_batch"):
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
    assert callable(G.Context.viterbi_full) and callable(G.Context.viterbi_full_batch)


def diag_models(G, rng, N, M, D):
    A = rng.uniform(0.0, 1.0, (N, N)) * (rng.uniform(size=(N, N)) < 0.6)
    A[:, 0] += 0.05
    A /= A.sum(1, keepdims=True)
    c = rng.dirichlet(np.full(M, 2.0), N)
    mean = rng.normal(0.0, 1.0, (N, M, D))
    iv = rng.uniform(0.3, 3.0, (N, M, D))
    det = 1.0 / iv.prod(-1)
    c[1, 0] = 0.0    # e = -inf
    det[2, -1] = 0.0  # lk = +inf: log b NaN
    ic = np.zeros((N, M, D, D))
    ic[..., np.arange(D), np.arange(D)] = iv
    return G.HostModel(A, c, mean, iv, det), G.HostFullModel(A, c, mean, ic, det)


def test_restatement_is_the_oracle_formula(G):
    rng = np.random.default_rng(5)
    for N, M, D in ((4, 3, 9), (6, 1, 1), (3, 2, 39)):
        hd, hf = diag_models(G, rng, N, M, D)
        X = rng.normal(0.0, 1.5, (120, D))
        X[7] += 60.0  # far from every Gaussian: linear densities underflow, the logs stay finite
        ref = O.log_emission(hd, X)
        got = log_emission(hf, X)
        assert np.isnan(ref[:, 2]).all() and np.isfinite(ref[7, 0])
        close_logb(got, ref, 1e-12)
        # every Gaussian of a state with c = 0: -inf
        hd.c[0] = 0.0
        hf.c[0] = 0.0
        ref = O.log_emission(hd, X)
        assert (ref[:, 0] == -np.inf).all()
        close_logb(log_emission(hf, X), ref, 1e-12)
