"""CPU-side tests (no GPU) of the full-covariance log-domain forward score: the C ABI exports it and
the Python face binds it; the numpy restatement of its definition (fulllogscore_ref.py) meets the
real reference's recorded scores wherever those are finite, equals the long-double E-step
restatement's log P with final_state = 1, and is finite on the whole shipped set, where the
reference prints 156 NaN of 169; the float64 restatement's distance from the long-double one, and
its place inside the lattice's rounding bound, at every shape the GPU tests run."""
import ctypes

import numpy as np
import pytest

import fulllogscore_ref as LR
import fulltrain_ref as R
from fullcov_support import check_blocks, load_synth, offsets, rel_dist, shipped
from fullviterbi_ref import log_emission as log_emission64

MISSES = {"vc_220_f_03_ap_010", "vc_220_f_047_ap_0225"}


def test_abi_exports_the_log_score(G):
    lib = ctypes.CDLL(G.HIP_LIB)
    for name in ("ghmm_logscore_full", "ghmm_logscore_full_batch"):
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
    assert callable(G.Context.logscore_full) and callable(G.Context.logscore_full_batch)


def score_table(hms, Xs, final_state, ft):
    """[word k][utterance u]"""
    return np.array([[LR.logscore(h, x, [len(x)], final_state, ft)[0] for x in Xs] for h in hms], dtype=ft)


def test_restated_log_emission_is_the_viterbi_formula(G):
    """the Gaussian-by-Gaussian log b in float64 = fullviterbi_ref.log_emission, special values included"""
    for name in ("l16_banded", "c0_dense", "det0_banded"):
        hm, X, _ = LR.make_case(G, name)
        got, ref = LR.log_emission(hm, X, np.float64), log_emission64(hm, X)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any() == name.startswith("det0")
        fin = np.isfinite(ref)
        assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
        assert np.allclose(got[fin], ref[fin], rtol=1e-12, atol=0)
        assert np.isfinite(ref[5][~np.isnan(ref[5]) & (ref[5] != -np.inf)]).all()


def test_synthetic_recorded_run(G):
    """all 169 pairs of the recorded 13 x 12 x 4 x 16 run: the float64 restatement (final_state = 0)
    meets the reference's printed scores at check_blocks' bar (rel 1e-9, abs 2e-6)"""
    sy, hms, Xs = load_synth(G)
    scores = score_table(hms, Xs, 0, np.float64)
    assert scores.shape == (13, 13) and np.isfinite(scores).all()
    check_blocks(scores, sy["words"], sy["blocks"])
    worst_abs = worst_rel = 0.0
    for u, blk in enumerate(sy["blocks"]):
        for w, txt in blk["ranking"]:
            d = abs(scores[sy["words"].index(w), u] - float(txt))
            worst_abs, worst_rel = max(worst_abs, d), max(worst_rel, d / abs(float(txt)))
    print(f"synthetic: worst {worst_abs:.2e} absolute, {worst_rel:.2e} relative")


def test_shipped_set(G):
    """the shipped 13 models x 13 utterances: 169 finite scores; the 13 pairs the reference prints as
    numbers are met at the same bar; 11 of 13 spoken words rank first, by margins no rounding moves"""
    sh, hms, Xs = shipped(G)
    words = [h.word for h in hms]
    assert words == sh["words"]
    s64 = score_table(hms, Xs, 0, np.float64)
    assert np.isfinite(s64).all()
    n_fin, worst = 0, 0.0
    for u, blk in enumerate(sh["blocks"]):
        for w, txt in blk["ranking"]:
            if "nan" in txt or "inf" in txt:
                continue
            n_fin += 1
            got = s64[words.index(w), u]
            assert got == pytest.approx(float(txt), rel=1e-9, abs=2e-6), (blk["spoken"], w)
            worst = max(worst, abs(got - float(txt)))
    assert n_fin == 13
    first = [words[int(np.argmax(s64[:, u]))] for u in range(13)]
    spoken = [b["spoken"] for b in sh["blocks"]]
    assert {s for s, f in zip(spoken, first) if s != f} == MISSES
    top = np.sort(s64, axis=0)
    margin = float((top[-1] - top[-2]).min())
    assert margin > 2.5e4
    sld = score_table(hms, Xs, 0, np.longdouble)
    spread = rel_dist(s64, sld)
    print(f"shipped: {n_fin} finite prints met within {worst:.2e}; smallest margin {margin:.0f} nats; "
          f"float64 spread {spread:.2e}")
    assert spread < 1e-12


def test_final_state_is_the_estep_loglik(G):
    """final_state = 1 in long double = fulltrain_ref.estep's log P per utterance (the scaled linear
    recursion with its final-state term) on a model fitted to its data"""
    N, M, D = 4, 2, 6
    X, lens = R.em_corpus(N, M, D, 5, 60)
    hm = G.HostFullModel.init_from(X, lens, N, M)
    hm = hm.mstep(R.pack(R.estep(hm, X, lens, 1, np.longdouble)["stats"]), delta=1)
    ref = R.estep(hm, X, lens, 1, np.longdouble)["loglik"]
    got = LR.logscore(hm, X, lens, 1, np.longdouble)
    assert np.isfinite(np.asarray(ref, dtype=np.float64)).all()
    d = rel_dist(got, ref)
    print(f"final_state = 1 against the E-step restatement: {d:.2e}")
    assert d < 1e-15
    # and final_state = 0 is no smaller
    assert (LR.logscore(hm, X, lens, 0, np.longdouble) >= got).all()


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_float64_spread(G, name):
    """the float64 restatement against the long-double one at a GPU-test shape: the distance end to
    end (the figure in fulllogscore_ref's docstring), and the lattice alone, both restated from the
    same float64 log b, inside fulllogscore_ref.lattice_bound"""
    hm, X, lens = LR.make_case(G, name)
    N = hm.N
    off = offsets(lens)
    b64 = LR.log_emission(hm, X, np.float64)
    worst = 0.0
    for fs in (0, 1):
        s64, sld = LR.logscore(hm, X, lens, fs, np.float64), LR.logscore(hm, X, lens, fs)
        worst = max(worst, rel_dist(s64, sld))
        for u, T in enumerate(lens):
            st = {}
            exact = LR.lattice(hm.A, b64[off[u]:off[u + 1]], fs, np.longdouble, st)
            got = LR.lattice(hm.A, b64[off[u]:off[u + 1]], fs, np.float64)
            rel_dist([got], [exact])
            if np.isfinite(exact):
                assert abs(np.longdouble(got) - exact) <= LR.lattice_bound(T, N, st["V"], st["La"]), (fs, u)
        if name.startswith("det0"):   # (with final_state = 1 the absorbing NaN state never shows)
            assert np.isnan(sld.astype(np.float64)).any() == (fs == 0 or name == "det0_banded")
        if name in ("det0_absorbing", "c0_dense") and fs == 1:
            assert np.isfinite(sld[0])  # the last state is reached round the state without a density
        if name == "c0_banded" and fs == 1:
            assert (sld == -np.inf).all()
        if not name.startswith(("det0", "c0")):
            short = np.asarray(lens) < N
            if fs == 0:
                assert np.isfinite(sld).all()       # T < N included
            else:
                assert np.isfinite(sld[~short]).all()
                if not LR.CASES[name][3]:           # banded: the last state is out of reach in T < N frames
                    assert (sld[short] == -np.inf).all()
    print(f"{name}: float64 spread {worst:.1e}")
    assert worst < 1e-12
