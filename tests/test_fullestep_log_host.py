"""CPU-side tests (no GPU) of the full-covariance log-domain E-step: the C ABI exports it and the
Python face binds it, and the numpy restatement of its definition (fullestep_log_ref.py) is pinned
before any GPU test trusts it:

  - in long double it IS the long-double linear E-step (fulltrain_ref.estep) on a fitted model, at the
    initial model of fulltrain_ref.EM_CASES[0] and after one iteration: every statistics block within
    1e-9 of its maximum, loglik within rel 1e-12.  A check of meaning: with log P_u in the place of
    log Z_u the blocks lie 2.6e-4 away.
  - a frame's gammas sum to rho_u = exp(log P_u - log Z_u) at every frame;
  - in float64 it stays inside the derived rounding bounds of fullestep_log_ref's docstring against
    long double, on the same float64 log b, at every shape the GPU tests run;
  - four EM iterations in float64 with the library's host M-step follow the long-double LINEAR
    trajectory (fulltrain_ref.em_trajectory): the model distances are fullestep_log_ref.EM_MODEL_F64."""
import ctypes

import numpy as np
import pytest

import fullestep_log_ref as LE
import fulllogscore_ref as LR
import fulltrain_ref as R
from fullcov_support import check_log_lattice, extended, offsets, rel_dist

LD_EPS = float(np.finfo(np.longdouble).eps)


def test_abi_exports_the_log_estep(G):
    lib = ctypes.CDLL(G.HIP_LIB)
    assert hasattr(lib, "ghmm_estep_full_log")
    assert "ghmm_estep_full_log" in G.SYMBOLS
    assert callable(G.Context.estep_full_log)


def test_restated_log_b_is_log_emission(G):
    """emission()'s log b = fulllogscore_ref.log_emission's, bit for bit, in both float types"""
    for name in ("l16_banded", "c0_dense"):
        hm, X, _ = LR.make_case(G, name)
        for ft in (np.float64, np.longdouble):
            logb, post, e = LE.emission(hm, X, ft)
            assert np.array_equal(logb, LR.log_emission(hm, X, ft))
            assert np.all(post[logb == -np.inf] == 0)
            fin = np.isfinite(logb)
            assert np.allclose(np.asarray(post.sum(-1)[fin], dtype=np.float64), 1.0, rtol=1e-12, atol=0)


def block_dist(got, ref):
    d = {}
    for key in R.STAT_KEYS:
        g, r = np.asarray(got[key], dtype=np.longdouble), np.asarray(ref[key], dtype=np.longdouble)
        assert np.all(np.isfinite(np.asarray(r, dtype=np.float64))), key
        d[key] = float(np.abs(g - r).max() / np.abs(r).max())
    return d


@extended
def test_long_double_restatement_is_the_linear_estep(G):
    """EM_CASES[0], the initial model and the model after one iteration"""
    N, M, D, U, T = R.EM_CASES[0]
    X, lens = R.em_corpus(N, M, D, U, T)
    hm = G.HostFullModel.init_from(X, lens, N, M)
    for it in range(2):
        lin = R.estep(hm, X, lens, 1, np.longdouble)
        log = LE.estep(hm, X, lens, 1, np.longdouble)
        d = block_dist(log["stats"], lin["stats"])
        ll, ref_ll = log["stats"]["loglik"], lin["stats"]["loglik"]
        dl = float(abs(ll - ref_ll) / abs(ref_ll))
        print(f"iteration {it}: blocks {max(d.values()):.1e} ({d}), loglik {dl:.1e}")
        assert max(d.values()) <= 1e-9
        assert dl <= 1e-12
        # the per-utterance log P and the arrays mean the same
        assert rel_dist(log["loglik"], lin["loglik"]) <= 1e-12
        assert float(np.abs(log["gamma"] - lin["gamma"]).max()) <= 1e-9
        assert float(np.abs(log["post"] - lin["post"]).max()) <= 1e-9
        hm = hm.mstep(R.pack(lin["stats"]), delta=1)


def all_cases(G):
    for name in LE.LATTICE_CASES:
        hm, X, lens = LR.make_case(G, name)
        yield name, hm, X, lens, 1
    hm, X, lens = LE.make_empty_case(G)
    for delta in LE.EMPTY_DELTAS:
        yield f"empty_dense_delta{delta}", hm, X, lens, delta


@extended
def test_gammas_sum_to_rho_at_every_frame(G):
    """sum_i gamma_t(i) = exp(log P_u - log Z_u), the same value at every t, in long double: inside
    the gamma bound of the docstring taken with long double's unit roundoff (eps / 2) for 2^-53, N
    entries a frame"""
    scale = (LD_EPS / 2) / LE.U53
    for name, hm, X, lens, delta in all_cases(G):
        r = LE.estep(hm, X, lens, delta, np.longdouble)
        for u, ut in enumerate(r["utt"]):
            if ut["T"] == 0 or not np.isfinite(ut["logZ"]):
                assert np.all(ut["gamma"] == 0)
                continue
            rho = np.exp(ut["logP"] - ut["logZ"])
            assert rho <= 1
            E = LE.gamma_exponent_bound(ut["T"], hm.N, ut["V"], ut["La"]) * scale
            tol = rho * np.expm1(np.longdouble(E)) + hm.N * 4 * LE.U53 * scale
            s = ut["gamma"].sum(1)
            assert np.all(np.abs(s - rho) <= tol), (name, u, float(np.abs(s - rho).max()), float(tol))
            if rho == 0:
                assert np.all(ut["gamma"] == 0)


@extended
def test_float64_restatement_inside_the_bounds(G):
    """float64 against long double on the same float64 log b, every GPU-test case"""
    for name, hm, X, lens, delta in all_cases(G):
        logb = LR.log_emission(hm, X, np.float64)
        off = offsets(lens)
        worst = 0.0
        for u in range(len(lens)):
            lbu = logb[off[u]:off[u + 1]]
            worst = max(worst, check_log_lattice(f"{name}[{u}]", hm.N, LE.lattice_fb(hm.A, lbu, delta, np.float64),
                                             LE.lattice_fb(hm.A, lbu, delta, np.longdouble)))
        print(f"{name}: worst error / bound {worst:.4f}")


@extended
@pytest.mark.parametrize("case", range(len(R.EM_CASES)))
def test_four_em_iterations(G, case):
    """float64 log E-step + host M-step against the long-double linear trajectory: trace at the
    project's rel 1e-9; the model at max(1e-8, 8 x the recorded EM_MODEL_F64), the bar the GPU test
    holds the device to (the recorded figure must stay an honest description of this platform)"""
    N, M, D, U, T = R.EM_CASES[case]
    X, lens = R.em_corpus(N, M, D, U, T)
    trace, ref_hm = R.em_trajectory(G, X, lens, N, M, 4, np.longdouble)
    assert np.all(np.isfinite(trace))
    got, hm = R.em_trajectory(G, X, lens, N, M, 4, np.float64, estep=LE.estep)
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(got, trace))
    e_model = R.model_err(hm, lambda k: getattr(ref_hm, k))
    print(f"EM_CASES[{case}]: trace {e_tr:.1e}, model {e_model:.1e} (EM_MODEL_F64 {LE.EM_MODEL_F64[case]:.1e})")
    assert e_tr <= 1e-9
    assert e_model <= max(1e-8, 8 * LE.EM_MODEL_F64[case])
