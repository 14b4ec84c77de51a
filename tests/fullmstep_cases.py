"""Cases for the full-covariance M-step on the device (ghmm_mstep_full_dev): a HostFullModel (the
model before the step) plus a hand-built full statistics vector, so that no E-step is needed and
every branch of TFF's M-step (ghmm_mstep_full_host, csrc/ghmm_fulltrain.c) can be aimed at.

Shared by test_fullmstep_host.py, which asserts on the host M-step's output that each quirk case
takes the branch it is named for, and by test_fullmstep_gpu.py, which holds the device M-step to
the host's bits.  Plain numpy; the host M-step of a case is computed once (host_result).

Positive-definite cases: covariance B B' + I (B's entries N(0, 1/D)) times num_c, a dense num_a so
that the band of `delta` shows.  Their shapes cover D in {1, 2, 9, 47, 48}, N in {1, 6, 64},
M in {1, 2, 8, MCAP} and delta in {0, 1, 2} without taking the whole product (64 x 256 x 48 would be
300 MB of matrices)."""
import functools

import numpy as np

from fullcov_support import banded, rand_fmodel

MCAP = 256          # ghmm_mstep_full_dev's cap on M (include/ghmm.h)
FLOOR = 1.0e-5      # TFF:38
ZERO_DET = 1e-20    # TFF:2242


def rand_model(G, rng, N, M, D, dense=False):
    """left-to-right (or dense) A, Dirichlet weights, symmetric inverse covariances with eigenvalues 0.5..2"""
    A = banded(rng, N)
    if dense:
        A = rng.random((N, N)) + 0.05
        A /= A.sum(1, keepdims=True)
    return rand_fmodel(G, rng, N, M, D, A, spread=1.0, asym=False, symmetrise=True)


def pd_sums(rng, N, M, D):
    """the sums of an E-step that never ran: dense num_a, covariances B B' + I"""
    B = rng.normal(0.0, 1.0 / np.sqrt(D), (N, M, D, D))
    cov = B @ np.swapaxes(B, -1, -2) + np.eye(D)
    num_c = rng.uniform(5.0, 20.0, (N, M))
    return {"num_a": rng.random((N, N)) + 0.1, "den_a": rng.uniform(2.0, 5.0, N),
            "den_c": num_c.sum(1) * rng.uniform(1.0, 1.1, N), "num_c": num_c,
            "mean": rng.normal(0.0, 1.0, (N, M, D)), "cov": cov}


def pack(s):
    """the flat vector of ghmm_stats_create_full from pd_sums' dict: num_mu = mean * num_c (0 where
    num_c == 0), num_cov = the upper triangle of cov * num_c"""
    N, M, D = s["mean"].shape
    iu = np.triu_indices(D)
    nc = s["num_c"][..., None]
    num_mu = s["mean"] * nc
    num_cov = s["cov"][..., iu[0], iu[1]] * nc
    return np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in
                           (s["num_a"], s["den_a"], s["den_c"], s["num_c"], num_mu, num_cov)] + [[-1234.5, 3.0]])


def new_cov(v, N, M, D):
    """what updating_mix_param forms from the vector v before the floor: (mean, cov) as full
    symmetric matrices, in float64 with IEEE division like the C code"""
    G_ = N * M
    iu = np.triu_indices(D)
    o = N * N + 2 * N
    num_c = v[o:o + G_].reshape(N, M)
    num_mu = v[o + G_:o + G_ + G_ * D].reshape(N, M, D)
    num_cov = v[o + G_ + G_ * D:-2].reshape(N, M, -1)
    with np.errstate(all="ignore"):
        mean = num_mu / num_c[..., None]
        tri = num_cov / num_c[..., None]
    cov = np.zeros((N, M, D, D))
    cov[..., iu[0], iu[1]] = tri
    cov[..., iu[1], iu[0]] = tri
    return mean, cov


# id -> (N, M, D, delta)
PD = {}
for _D in (1, 2, 47, 48):
    PD[f"pd-1x1x{_D}"] = (1, 1, _D, 1)
PD["pd-1x2x9"] = (1, 2, 9, 1)
for _delta in (0, 1, 2):
    PD[f"pd-6x2x9-delta{_delta}"] = (6, 2, 9, _delta)
PD["pd-6x8x47"] = (6, 8, 47, 1)
PD["pd-6x2x48-delta2"] = (6, 2, 48, 2)
PD["pd-6x8x1-delta0"] = (6, 8, 1, 0)
PD["pd-64x2x2-delta2"] = (64, 2, 2, 2)
PD["pd-64x1x9-delta0"] = (64, 1, 9, 0)
PD["pd-64x8x48"] = (64, 8, 48, 1)
PD[f"pd-1x{MCAP}x2"] = (1, MCAP, 2, 1)
PD[f"pd-6x{MCAP}x1-delta2"] = (6, MCAP, 1, 2)
PD[f"pd-1x{MCAP}x9"] = (1, MCAP, 9, 1)


def _tiny(D, scale):
    """a covariance whose determinant is far below 1e-20 and which the floor leaves alone"""
    return np.diag(np.full(D, 2.0e-5) * scale)


def _quirk(G, name):
    rng = np.random.default_rng(sorted(QUIRKS).index(name) + 7000)
    if name == "q1-den_c-zero":            # state 1 is skipped: its slot is inverted a second time
        N, M, D = 3, 2, 5
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["den_c"][1] = 0.0
    elif name == "q1-den_c-zero-d1":       # the same at D = 1: 1 / (1 / var)
        N, M, D = 3, 2, 1
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["den_c"][0] = 0.0
    elif name == "q2-den_a-zero":          # rows 0 and 3 of a dense A are kept
        N, M, D = 4, 2, 3
        hm, s = rand_model(G, rng, N, M, D, dense=True), pd_sums(rng, N, M, D)
        s["den_a"][[0, 3]] = 0.0
    elif name == "q3-num_c-zero":          # Gaussian (1, 1): NaN mean and matrix, det NaN -> 0, replaced
        N, M, D = 2, 3, 4
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["num_c"][1, 1] = 0.0
    elif name == "q3-num_c-zero-m1":       # M = 1: nothing to replace it with, the NaNs stay
        N, M, D = 2, 1, 4
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["num_c"][1, 0] = 0.0
    elif name in ("q4-singular-m1", "q4-singular-m2"):
        # rows 1 and 2 equal: pivots 1, 1, 0 exactly (num_c = 4: exact quotients), det == 0, the
        # matrix stays un-inverted; with M = 1 it is then split with itself and stays, with M = 2 the
        # other Gaussian's inverse replaces it
        N, M, D = 2, int(name[-1]), 3
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["num_c"][0, 0] = 4.0
        s["cov"][0, 0] = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 1.0, 1.0]])
    elif name == "q5-two-small-dets":
        # state 1 of M = 4: Gaussians 0 and 2 below 1e-20; the donors 1 and 3 have EQUAL determinants
        # (the same covariance), so sorting's strict '<' must keep 1 before 3
        N, M, D = 2, 4, 5
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["cov"][1, 0], s["cov"][1, 2] = _tiny(D, 1.0), _tiny(D, 1.5)
        s["cov"][1, 3], s["num_c"][1, 3] = s["cov"][1, 1], s["num_c"][1, 1]
    elif name == "q5-donor-modified":
        # state 0 of M = 4: determinants in the order 1 > 3 > 0 > 2 with 3, 0, 2 below 1e-20:
        # 0 <- 1, then 2 <- 3 (still small), then 3 <- 0, which the first step has rewritten
        N, M, D = 2, 4, 5
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["cov"][0, 3], s["cov"][0, 0], s["cov"][0, 2] = _tiny(D, 3.0), _tiny(D, 2.0), _tiny(D, 1.0)
    elif name == "q6-self-split":          # M = 1 and det < 1e-20: mean x 1.05 x 0.95, weight 1
        N, M, D = 3, 1, 5
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["cov"][2, 0] = _tiny(D, 1.0)
    elif name == "q7-small-weights":       # weights below 1e-5 are floored before the sum
        N, M, D = 2, 4, 3
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["num_c"][0, 1], s["num_c"][0, 3], s["num_c"][1, 0] = 1e-5, 3e-6, 1e-7
        s["den_c"][:] = 40.0
    elif name == "q7-floored-diagonal":    # (the diagonal floor: variances of 1e-7 become 1e-5)
        N, M, D = 2, 2, 4
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        s["cov"][1, 0] = np.diag([1e-7, 0.5, 2e-6, 1.0])
    elif name in ("q8-negative-det", "q8-negative-det-m2"):
        # cov[0][1] = 2 beside unit variances: pivots 1, -3, ...: a negative determinant, which
        # treat_zero_det reads as "below 1e-20": kept (split with itself) at M = 1; at M = 2 both
        # Gaussians of state 0 are negative, so the donor's determinant is negative as well
        N, M, D = 2, int(name[-1]) if name[-1] == "2" else 1, 4
        hm, s = rand_model(G, rng, N, M, D), pd_sums(rng, N, M, D)
        for k in range(M):
            s["cov"][0, k, 0, 1] = s["cov"][0, k, 1, 0] = 2.0 + k
            s["cov"][0, k, 0, 0] = s["cov"][0, k, 1, 1] = 1.0
    else:
        raise KeyError(name)
    return hm, pack(s), 1


QUIRKS = ("q1-den_c-zero", "q1-den_c-zero-d1", "q2-den_a-zero", "q3-num_c-zero", "q3-num_c-zero-m1",
          "q4-singular-m1", "q4-singular-m2", "q5-two-small-dets", "q5-donor-modified", "q6-self-split",
          "q7-small-weights", "q7-floored-diagonal", "q8-negative-det", "q8-negative-det-m2")
NAN_CASES = ("q3-num_c-zero-m1",)   # the cases whose host result holds NaNs
ALL = tuple(PD) + QUIRKS


@functools.lru_cache(maxsize=None)
def build(G, name):
    """(model before the step, statistics vector, delta) of a case"""
    if name in PD:
        N, M, D, delta = PD[name]
        rng = np.random.default_rng(sorted(PD).index(name) + 500)
        return rand_model(G, rng, N, M, D, dense=True), pack(pd_sums(rng, N, M, D)), delta
    return _quirk(G, name)


@functools.lru_cache(maxsize=None)
def host_result(G, name):
    """ghmm_mstep_full_host of the case, computed once; callers leave it unchanged"""
    hm, v, delta = build(G, name)
    with np.errstate(all="ignore"):
        return hm.mstep(v, delta=delta)
