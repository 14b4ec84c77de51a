"""Pins of tests/fulltrain_ref.py, the extended-precision restatement of the full-covariance
trainer's E-step that test_fullestep_gpu.py holds the HIP code against (CPU only).

(a) the real reference's recorded runs (tests/golden/fulltrain_runs.json, fulltrain_models.npz):
    the restated E-step + the library's host M-step, iterated with the trainer's stopping rule,
    under the bars of fullcov_support.check_run (iteration count, mean probability within rel
    1e-9 / abs 2e-6, model within 1e-8).
(b) the pinned diagonal oracle (oracle/ghmm_oracle.c) on diagonal matrices: dense A, transition
    bands 0..3, utterances shorter than the model, of one frame and of none, 33 and 64 states,
    which the recorded runs do not cover (fullcov_support.assert_close: rtol 1e-8, floor 1e-13,
    equal NaN / infinity pattern).
(c) the float64 result equals np_estep, the vectorised float64 restatement, on test_fulltrain_gpu's
    four cases.
(d) the two multi-iteration cases of test_fullestep_gpu.py are well conditioned: their float64 and
    long-double trajectories differ by at most a hundredth of the bars the GPU test asserts."""
import os

import numpy as np
import pytest

import fulltrain_ref as R
import oracle_lib as O
from conftest import GOLDEN
from fullcov_support import RUNS, assert_close, close, extended, rand_fmodel, report_value, walk_any
from fulltrain_ref import np_estep

FTS = [np.float64, np.longdouble]


def ft_param(ft):
    return pytest.param(ft, id=ft.__name__, marks=[extended] if ft is np.longdouble else [])


def train(G, X, lens, N, M, ft):
    """train_main.c's loop (TFF:135-137): old = 1.0; M-step while |old - p| / |old| > 1e-3"""
    hm = G.HostFullModel.init_from(X, lens, N, M)
    old, it = 1.0, 0
    while True:
        it += 1
        st = R.estep(hm, X, lens, 1, ft)["stats"]
        p = float(st["loglik"])
        if abs((old - p) / old) > 1e-3:
            old = p
            hm = hm.mstep(R.pack(st), delta=1)
        else:
            return hm, it, p / len(lens)


# ------------------------------------------------------ (a) the recorded runs

@pytest.mark.parametrize("ft", [ft_param(f) for f in FTS])
@pytest.mark.parametrize("name", sorted(RUNS))
def test_recorded_runs(G, name, ft):
    run = RUNS[name]
    if run["kind"] == "synthetic":
        data = np.load(os.path.join(GOLDEN, "fulltrain_synth.npz"))
        X, lens = data[name + ".X"].astype(np.float64), data[name + ".lens"]
    else:
        Xs = [G.perfil_read(os.path.join(GOLDEN, "perfil", f)) for f in run["perfils"]]
        X, lens = np.concatenate(Xs), np.array([len(x) for x in Xs], dtype=np.int32)
    hm, it, p = train(G, X, lens, run["N"], run["M"], ft)
    ref = run["report"]
    assert it == int(report_value(ref, "number of iterations")), name
    assert p == pytest.approx(float(report_value(ref, "mean probability")), rel=1e-9, abs=2e-6), name
    rec = np.load(os.path.join(GOLDEN, "fulltrain_models.npz"))
    err = R.model_err(hm, lambda k: rec[f"{name}.{k}"])
    print(f"{name} {ft.__name__}: iterations {it}, mean probability {p:.6f}, model error {err:.2e}")
    assert err <= 1e-8, (name, err)


# ------------------------------------------------------ (b) the diagonal oracle

ORACLE_CASES = [
    (10, 3, 7, [60, 45, 33], False, 1),
    (6, 2, 5, [50, 60, 9], True, 3),
    (6, 2, 5, [50, 60, 9], True, 0),
    (20, 2, 9, [60, 45, 81], True, 2),
    (33, 2, 4, [50, 70, 40], True, 1),
    (12, 2, 6, [40, 5, 1, 0, 30], False, 1),     # T < N, T = 1, T = 0
    (64, 1, 3, [100, 130], False, 1),
]


@pytest.mark.parametrize("ft", [ft_param(f) for f in FTS])
@pytest.mark.parametrize("N,M,D,lens,dense,delta", ORACLE_CASES)
def test_diagonal_matrices_equal_the_oracle(G, N, M, D, lens, dense, delta, ft):
    mean_t, std = G.synth_truth(N, M, D)
    X = G.synth_utterances(mean_t, std, lens)
    hm = G.synth_start_model(mean_t, std, 0.05)
    if dense:
        A = np.random.default_rng(7).random((N, N)) + 0.05
        hm.A[:] = A / A.sum(1, keepdims=True)
    lens = np.asarray(lens, dtype=np.int32)
    ref = G.split_stats(O.estep(hm, X, lens, delta=delta, dumps=False)[0], N, M, D)
    ic = np.zeros((N, M, D, D))
    ic[..., np.arange(D), np.arange(D)] = hm.inv_var
    full = G.HostFullModel(hm.A, hm.c, hm.mean, ic, hm.det)
    st = R.estep(full, X, lens, delta, ft)["stats"]
    dg = np.triu_indices(D)
    dg = np.nonzero(dg[0] == dg[1])[0]             # the diagonal's places in the triangle
    mine = dict(st, num_var=st["num_cov"][..., dg])
    for key in ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_var", "loglik"):
        assert_close(np.asarray(mine[key], dtype=np.float64), ref[key], what=f"{key} {ft.__name__}")
    if any(0 < T < N for T in lens) and not dense:
        assert float(st["loglik"]) == -np.inf == float(ref["loglik"])
    # nothing outside the band
    band = np.triu(np.ones((N, N)), 0) - np.triu(np.ones((N, N)), delta + 1)
    assert np.all(np.asarray(st["num_a"], dtype=np.float64)[band == 0] == 0.0)


# ------------------------------------------------------ (c) the existing restatement

@pytest.mark.parametrize("D", [1, 9, 16, 39])
def test_float64_equals_the_existing_restatement(G, D):
    """test_fulltrain_gpu.test_estep_matches_restatement's case, clamped Gaussian included"""
    rng = np.random.default_rng(D)
    N, M = 5, 3
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    lens = [57, 80, 41]
    X = walk_any(rng, hm, lens)
    hm.inv_cov[4, 2] = -np.eye(D)
    hm.mean[4, 2] = hm.mean[4, 0] + 60.0
    rb, rpost, rgamma, rst = np_estep(hm, X, lens)
    r = R.estep(hm, X, lens, 1, np.float64)
    F = len(X)
    assert np.any(r["post"][:, 4, 2] > 0.0)
    close(r["b"], rb, rtol=1e-12)
    close(r["post"].reshape(F, N * M), rpost, rtol=1e-12)
    close(r["gamma"], rgamma, rtol=1e-12, zeros=False)
    for key in R.STAT_KEYS:
        close(r["stats"][key], rst[key], rtol=1e-12, zeros=False)
    assert float(r["stats"]["loglik"]) == pytest.approx(rst["loglik"], rel=1e-12)
    assert float(r["loglik"].sum()) == pytest.approx(rst["loglik"], rel=1e-12)
    assert float(r["stats"]["n_utt"]) == 3.0


def test_stats_from_equals_the_estep_sums(G):
    """stats_from on the E-step's own gamma and post gives the E-step's Gaussian sums, and every
    absolute sum bounds its sum"""
    rng = np.random.default_rng(3)
    N, M, D = 4, 2, 5
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    lens = [30, 0, 25]
    X = walk_any(rng, hm, [30, 25])
    r = R.estep(hm, X, lens, 1, np.float64)
    s, a = R.stats_from(r["gamma"], r["post"], X, hm.mean, np.float64)
    for key in ("num_c", "num_mu", "num_cov"):
        np.testing.assert_allclose(s[key], r["stats"][key], rtol=1e-12, atol=0)
        assert np.all(np.abs(s[key]) <= a[key] * (1 + 1e-12))
    np.testing.assert_array_equal(s["num_c"], a["num_c"])


# ------------------------------------------------------ (d) conditioning of the EM cases

@extended
@pytest.mark.parametrize("N,M,D,U,T", R.EM_CASES)
def test_em_cases_are_well_conditioned(G, N, M, D, U, T):
    """Four iterations in float64 and in long double from the same start: the log-likelihood trace
    within 1e-11 (a hundredth of the GPU test's 1e-9) and the model within 1e-10 (of its 1e-8)."""
    X, lens = R.em_corpus(N, M, D, U, T)
    res = {ft: R.em_trajectory(G, X, lens, N, M, 4, ft) for ft in FTS}
    (tr64, hm64), (trl, hml) = res[np.float64], res[np.longdouble]
    assert np.all(np.isfinite(trl))
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(tr64, trl))
    e_model = R.model_err(hm64, lambda k: getattr(hml, k))
    print(f"{(N, M, D, U * T)}: trace difference {e_tr:.1e}, model difference {e_model:.1e}, "
          f"smallest det {hml.det.min():.1e}")
    assert e_tr <= 1e-11 and e_model <= 1e-10
