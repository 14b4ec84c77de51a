"""The yardstick of the device initial model (ghmm_fmodel_init), pinned on the CPU: fullinit_ref.init_full
in float64 equals ghmm_init_model_full bit for bit on every test corpus, and every corpus but the one
documented exception is admitted (fullinit_ref's docstring: every gap >= 1e-9, long double assigns alike)."""
import numpy as np
import pytest

import fullinit_ref as R
from fullcov_support import need_extended


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_host_init(G, name):
    X, lens, N, M = R.corpus(name)
    host = G.HostFullModel.init_from(X, lens, N, M)
    ref = R.reference(name, False)
    for key in ("A", "c", "mean", "inv_cov", "det"):
        assert bits_equal(getattr(host, key), ref[key]), (name, key)


@pytest.mark.parametrize("name", R.ADMITTED)
def test_corpus_is_admitted(name):
    need_extended()
    r64, r80 = R.reference(name, False), R.reference(name, True)
    assert R.min_gap(r64) >= R.MIN_GAP, (name, R.min_gap(r64))
    assert len(r64["assign"]) == len(r80["assign"])
    for a, b in zip(r64["assign"], r80["assign"]):
        assert np.array_equal(a, b), name
    assert np.array_equal(r64["count"], r80["count"]), name


def test_cases_cover_what_they_claim():
    """the properties the case list names, checked on the float64 restatement"""
    X, lens, N, M = R.corpus("short")
    assert lens.max() < N
    r = R.reference("short", False)
    assert np.all(r["count"][N - 1] == 0) and np.all(np.isnan(r["mean"][N - 1])) and np.all(np.isnan(r["c"][N - 1]))
    assert np.all(r["det"][N - 1] == 0)
    r = R.reference("fewdistinct", False)
    empty = r["count"][1] == 0
    assert empty.any(), "no empty cell survived to the covariance pass"
    assert np.all(np.isnan(r["inv_cov"][1][empty])) and np.all(r["det"][1][empty] == 0)
    assert np.all(r["c"][1][empty] < 2e-5) and np.all(r["c"][1][empty] > 0)
    assert R.min_gap(r) < R.MIN_GAP      # the tie its docstring derives: why it is exempt
    for name in ("ragged", "n64"):
        X, lens, N, M = R.corpus(name)
        assert np.all(lens % N != 0) and len(set(lens.tolist())) > 3, name
    # a floor-free case gives the counts back from c exactly (the GPU test relies on it)
    for name in R.ADMITTED:
        r = R.reference(name, False)
        if name != "short":
            assert np.all(r["count"] > 0), name
