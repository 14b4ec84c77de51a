"""CPU-side tests (no GPU) of the diagonal log-domain forward score: the C ABI exports the four calls and
the Python face binds them; on every case of logscore_cases.py the float64 restatement stays within 1e-12
relative of the long-double one (test_fulllogscore_host.test_float64_spread's bar); the oracle's linear
score of the utterance with the far frame is not finite where the log-domain reference is; final_state = 1
is the oracle's score where that is finite; and the gathered form of the long-double lattice that the
512-state case needs is fulllogscore_ref.lattice."""
import ctypes

import numpy as np
import pytest

import fulllogscore_ref as LR
import logscore_cases as LC
import logscore_ref as R
import oracle_lib as O
from fullcov_support import offsets, rel_dist

CALLS = ("ghmm_logscore", "ghmm_logscore_batch", "ghmm_logscore_streams", "ghmm_logscore_streams_batch")


@pytest.fixture(scope="module")
def refs(G):
    made = {}

    def get(name, far=True):
        if (name, far) not in made:
            case = LC.make(G, name, far)
            made[name, far] = (case, R.Reference(case))
        return made[name, far]
    return get


def test_abi_exports_the_log_score(G):
    lib = ctypes.CDLL(G.HIP_LIB)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
    for name in ("logscore", "logscore_batch", "logscore_streams", "logscore_streams_batch"):
        assert callable(getattr(G.Context, name)), name


@pytest.mark.parametrize("name", LC.NAMES)
def test_the_cases_hold_what_they_claim(G, refs, name):
    case, ref = refs(name)
    lens = np.asarray(case.lens)
    assert (lens == 1).any() and (lens == 0).any() and ((lens > 0) & (lens < max(case.Ns))).any()
    assert lens[0] > LC.FAR_FRAME and lens[0] >= min(case.Ns)
    for lb in ref.logb:
        if name.endswith("_nan"):
            assert np.isnan(lb[:, 3]).all() and not np.isnan(np.delete(lb, 3, axis=1)).any()
        elif name.endswith("_c0"):
            assert (lb[:, 1] == -np.inf).all() and np.isfinite(np.delete(lb, 1, axis=1)).all()
        else:
            assert np.isfinite(lb).all()
    s0, s1 = ref.score[0], ref.score[1]
    assert (s0[:, lens == 0] == 0).all() and (s1[:, lens == 0] == 0).all()
    if name.endswith("_nan"):       # the NaN stays in its absorbing state
        assert np.isnan(s0[:, lens > 0]).all() and np.isfinite(s1[0, 0])
    elif name.endswith("_c0"):      # banded: nothing gets past state 1
        assert (s1[:, lens > 0] == -np.inf).all() and np.isfinite(s0[:, lens > 0]).all()
    else:
        assert np.isfinite(s0).all() and np.isfinite(s1[:, 0]).any()
    both = np.isfinite(s0) & np.isfinite(s1)
    assert (ref.score_ld[0][both] >= ref.score_ld[1][both]).all()


@pytest.mark.parametrize("name", LC.NAMES)
def test_float64_spread(G, refs, name):
    """the float64 lattice against the long-double one on the same float64 log b: the distance (the figure
    in logscore_cases' docstring) below 1e-12, and inside fulllogscore_ref.lattice_bound"""
    case, ref = refs(name)
    worst = 0.0
    for fs in (0, 1):
        worst = max(worst, rel_dist(ref.score64[fs], ref.score_ld[fs]))
        for k, hms in enumerate(case.words):
            ld, bound = R.lattice_scores(hms[0].A, ref.logb[k], case.lens, fs)
            fin = np.isfinite(ld.astype(np.float64))
            with np.errstate(invalid="ignore"):
                err = np.abs(ref.score64[fs][k].astype(np.longdouble) - ld)[fin]
            assert (err <= bound[fin]).all(), (fs, k, err, bound[fin])
    print(f"{name}: float64 spread {worst:.1e}")
    assert worst < 1e-12


@pytest.mark.parametrize("name", [n for n in LC.NAMES if n not in LC.EDITED])
def test_the_linear_score_underflows_where_the_log_score_is_finite(G, refs, name):
    """utterance 0 holds the far frame: the oracle's linear score is -inf or NaN, the reference is finite"""
    case, ref = refs(name)
    T = int(case.lens[0])
    hit = 0
    for k, hms in enumerate(case.words):
        lin = O.score_streams(hms, [X[:T] for X in case.Xs]) if case.P > 1 else O.score(hms[0], case.Xs[0][:T])
        assert not np.isfinite(lin), (k, lin)
        assert np.isfinite(ref.score[0][k, 0])
        hit += bool(np.isfinite(ref.score[1][k, 0]))
    assert hit >= 1


@pytest.mark.parametrize("name", ["lane_6x2x9_banded", "lane_9x2x5_dense", "wide_65x1x4_banded", "vocab_p2"])
def test_final_state_is_the_oracles_score(G, refs, name):
    """without the far frame: final_state = 1 equals the oracle's score (calc_probability with its
    final-state term) to 1e-9 wherever that is finite, and is -inf where that is not"""
    case, ref = refs(name, far=False)
    off = offsets(case.lens)
    n = 0
    for k, hms in enumerate(case.words):
        for u, T in enumerate(case.lens):
            if T == 0:
                continue
            Xu = [X[off[u]:off[u + 1]] for X in case.Xs]
            lin = O.score_streams(hms, Xu) if case.P > 1 else O.score(hms[0], Xu[0])
            got = ref.score[1][k, u]
            if np.isfinite(lin):
                assert got == pytest.approx(lin, rel=1e-9, abs=0), (k, u)
                n += 1
            else:
                assert got == -np.inf, (k, u, lin, got)
    assert n >= 1


@pytest.mark.parametrize("name", LC.NAMES)
def test_gathered_lattice_is_the_reference_lattice(G, refs, name):
    """logscore_ref.gathered_lattice (only the terms a_ij > 0) against fulllogscore_ref.lattice on the case's
    own log b: equal NaN and infinity patterns, 1e-17 relative, equal V and La; the 512-state case on the
    first 6 frames of its utterances"""
    case, ref = refs(name)
    off = offsets(case.lens)
    for k, hms in enumerate(case.words):
        A = hms[0].A
        cut = 6 if A.shape[0] > R.WIDE_REF else 10 ** 9
        for u in range(case.U):
            lb = ref.logb[k][off[u]:off[u + 1]][:cut]
            for fs in (0, 1):
                s1, s2 = {}, {}
                a, b = LR.lattice(A, lb, fs, np.longdouble, s1), R.gathered_lattice(A, lb, fs, np.longdouble, s2)
                assert rel_dist([b], [a]) <= 1e-17, (k, u, fs, a, b)
                assert s1 == pytest.approx(s2, rel=1e-15)
