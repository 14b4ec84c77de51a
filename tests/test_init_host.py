"""The yardstick of the diagonal device initial model (ghmm_model_init), pinned on the CPU:
init_ref.init_diag in float64 equals ghmm_init_model bit for bit on every test corpus, every corpus but the
one documented exception is admitted (init_ref's docstring: every classification gap >= 1e-9, every consumed
distortion order's gap >= 1e-6, long double decides alike), every case takes the branch it is named for, and
the two no-candidate rules differ where the GPU test says they do."""
import numpy as np
import pytest

import init_ref as R
from fullcov_support import need_extended
from streams_util import bits_equal

KEYS = ("A", "c", "mean", "inv_var", "det")


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_host_init(G, name):
    X, lens, N, M = R.corpus(name)
    host = G.HostModel.init_from(X, lens, N, M)
    ref = R.reference(name, False)
    for key in KEYS:
        assert bits_equal(getattr(host, key), ref[key]), (name, key)


@pytest.mark.parametrize("name", R.ADMITTED)
def test_corpus_is_admitted(name):
    need_extended()
    r64, r80 = R.reference(name, False), R.reference(name, True)
    print(f"init admission {name:11s} classification gap {R.min_gap(r64):.2e} order gap {R.min_order_gap(r64):.2e}")
    assert R.min_gap(r64) >= R.MIN_GAP, (name, R.min_gap(r64))
    assert R.min_order_gap(r64) >= R.ORDER_GAP, (name, R.min_order_gap(r64))
    assert R.same_decisions(r64, r80), name


def splits(r):
    """per largest-distortion split of the float64 run: (cells taken, of how many)"""
    return {(len(o["taken"]), o["level"]) for o in r["orders"] if o["kind"] == "split"}


def test_cases_cover_what_they_claim():
    """the properties the case list names, checked on the float64 restatement"""
    for name, want in R.SPLITS_BY_DISTORTION.items():
        assert splits(R.reference(name, False)) == {want}, name
    # the doubling split alone up to 8 cells, then all 8 (m16) / all 32 (m64) in the order of their distortion,
    # and that order is not the identity somewhere: the branch taken matters
    for name, want in (("m4", (2, 2)), ("m16", (8, 8)), ("m64", (32, 32))):
        r = R.reference(name, False)
        assert splits(r) == {want}, name
        assert any(o["taken"] != sorted(o["taken"]) for o in r["orders"]), name
    # the 1-of-64 split of m65 does not take cell 0 (idx[i] against i)
    X, lens, N, M = R.corpus("m65")
    assert M > 64 and R.reference("m65", False)["orders"][0]["taken"] != [0]
    assert R.corpus("m64")[3] == 64
    # a re-seed in a state that has frames; reseed_last's in the last k-means pass of the last level
    for name in ("reseed", "reseed_last", "g264", "tie"):
        r = R.reference(name, False)
        real = [s for s in r["reseeds"] if r["dur"][s[2]] > 0]
        assert real, name
        assert all(s[4] != s[3] for s in real), name
    r = R.reference("reseed", False)
    assert len({s[0] for s in r["reseeds"]}) == 2            # at two levels, hence once before a split
    r = R.reference("reseed_last", False)
    assert (R.corpus("reseed_last")[3], R.PASSES - 1) in {(s[0], s[1]) for s in r["reseeds"]}
    # short: no utterance reaches the last state, which the host leaves as 0/0
    X, lens, N, M = R.corpus("short")
    assert lens.max() < N
    r = R.reference("short", False)
    assert r["dur"][N - 1] == 0 and np.all(r["count"][N - 1] == 0)
    for key in ("mean", "inv_var", "det", "c"):
        assert np.all(np.isnan(r[key][N - 1])), key
    assert all(np.all(np.isfinite(r[key][:N - 1])) for key in ("mean", "inv_var", "det", "c"))
    # fewer than 16 frames in the corpus; T < N and T % N != 0
    for name in ("f9", "f15"):
        assert len(R.corpus(name)[0]) < 16
    X, lens, N, M = R.corpus("f15")
    assert np.all(lens % N != 0) and len(X) % 64 != 0
    X, lens, N, M = R.corpus("n300")
    assert N > 256 and np.all(lens % N != 0)
    X, lens, N, M = R.corpus("g264")
    assert N * M > 256 and N <= 256
    assert [R.corpus(n)[0].shape[1] for n in ("d64", "d65", "d300", "d39m8")] == [64, 65, 300, 39]
    # tie: exactly equal distances in state 1 in every pass, cell 0 takes every frame, cell 1 ends empty
    r = R.reference("tie", False)
    assert R.min_gap(r) == 0.0
    assert np.all(r["mean"][1] == 0) and r["count"][1].tolist() == [r["dur"][1], 0]
    assert np.all(np.isnan(r["inv_var"][1, 1])) and np.isnan(r["det"][1, 1]) and 0 < r["c"][1, 1] < 2e-5
    # a variance at the floor is met somewhere (a cell of one frame), so the floor pattern test has an object
    assert any(np.any(R.reference(n, False)["inv_var"] == 1.0 / R.FLOOR) for n in ("reseed", "reseed_last"))
    # a floor-free case gives the counts back from c exactly (the GPU test relies on it)
    for name in R.CASES:
        r = R.reference(name, False)
        with np.errstate(invalid="ignore"):
            back = r["c"] * r["dur"][:, None]
        free = r["count"].min(1) > 0
        assert np.array_equal(np.rint(back[free]), r["count"][free]) and \
            np.all(np.abs(back[free] - r["count"][free]) < 1e-9), name
        assert np.all(free | (r["dur"] == 0)) or name == "tie", name


def test_no_candidate_rules_differ(G):
    """one frame of m3's corpus moved to 1e11: no cell is within 1e20 of it.  The host carries the previous
    frame's cell, the device takes cell 0 (include/ghmm.h, ghmm_model_init); on this corpus the two give
    different models, and "carry" is the host's bits"""
    X, lens, N, M, t = R.far_corpus()
    carry, zero = R.far_reference("carry"), R.far_reference("zero")
    assert carry["assign"][-1][t - 1] != 0
    host = G.HostModel.init_from(X, lens, N, M)
    for key in KEYS:
        assert bits_equal(getattr(host, key), carry[key]), key
    assert carry["assign"][-1][t] != 0 and zero["assign"][-1][t] == 0
    assert not np.array_equal(carry["count"], zero["count"])
    assert not bits_equal(carry["mean"], zero["mean"])
    # nothing else is near a tie under either rule
    for r in (carry, zero):
        assert R.min_gap(r) >= R.MIN_GAP and R.min_order_gap(r) >= R.ORDER_GAP
