"""CPU-side tests (no GPU) of the diagonal log-domain Baum-Welch E-step's reference (estep_log_ref.py) and
of its plumbing:

  the definition   without the far frame the long-double log E-step is the oracle's linear one (oracle_lib.estep,
                   estep_streams) at the project's RTOL, block by block; normalising with log P_u instead of
                   log Z_u misses that bar where rho_u < 1
  the point        with the far frame the oracle's linear loglik is not finite, the restatement's statistics are
  the cases        T < N gives log P = -inf and zero gamma, c0 gives log b = -inf, the NaN stays in its absorbing
                   state, banded and dense A at both dispatch widths
  distances        the float64 restatement from the long-double one (the figures of estep_log_ref's docstring),
                   the gathered lattice from fullestep_log_ref.lattice_fb
  symbols          include/ghmm.h, ghmm.SYMBOLS and the built library agree on the two new calls"""
import ctypes
import os
import re

import numpy as np
import pytest

import estep_log_ref as E
import fullestep_log_ref as LE
import logscore_cases as LC
import oracle_lib as O
from _load import ROOT
from fullcov_support import RTOL, assert_close, extended, offsets, rel_dist

CALLS = ("ghmm_estep_log", "ghmm_estep_log_streams")
CLEAN = [n for n in E.NAMES if n not in E.EDITED]


def oracle_stats(G, case, delta=1):
    """the oracle's linear statistics, one dict of blocks per stream"""
    hms = case.words[0]
    if case.P == 1:
        vs = [O.estep(hms[0], case.Xs[0], case.lens, delta, dumps=False)[0]]
    else:
        vs = O.estep_streams(hms, case.Xs, case.lens, delta)[0]
    return [G.split_stats(np.asarray(v), h.N, h.M, h.D) for v, h in zip(vs, hms)]


def test_abi_exports_the_log_estep(G):
    lib = ctypes.CDLL(G.HIP_LIB)
    header = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    for name in ("estep_log", "estep_log_streams"):
        assert callable(getattr(G.Context, name)), name


@extended
@pytest.mark.parametrize("name", CLEAN)
def test_the_definition_is_the_references_where_that_is_finite(G, name):
    case, ref = E.reference(G, name, far=False)
    lin = oracle_stats(G, case)
    worst = 0.0
    for p, (st, ln) in enumerate(zip(ref["stats"], lin)):
        assert np.isfinite(ln["num_a"]).all() and np.isfinite(ln["num_var"]).all(), "the oracle is not finite here"
        for k in E.BLOCKS:
            assert_close(np.asarray(st[k], dtype=np.float64), ln[k], what=f"{name} stream {p} {k}")
            worst = max(worst, E.block_dist(np.asarray(st[k], dtype=np.float64), ln[k]))
    print(f"{name}: log-domain restatement against the oracle's linear E-step, worst block distance {worst:.2e}")


@extended
@pytest.mark.parametrize("name", ["lane_9x2x5_dense", "wide_70x1x4_dense"])
def test_log_p_is_not_the_normaliser(G, name):
    """a dense A leaves probability outside the last state at T-1: rho_u < 1, and gamma / P_u misses the bar
    that gamma / Z_u meets"""
    case, ref = E.reference(G, name, far=False)
    rho = np.exp(ref["loglik"] - ref["logZ"])[np.asarray(case.lens) > 0]
    assert np.isfinite(rho).all() and (rho < 1 - 1e-6).any(), rho
    wrong = E.estep(case.words[0], case.Xs, case.lens, 1, np.longdouble, normaliser="P")
    lin = oracle_stats(G, case)[0]
    for k in ("den_c", "num_c"):
        assert_close(np.asarray(ref["stats"][0][k], dtype=np.float64), lin[k], what=k)
        d = E.block_dist(np.asarray(wrong["stats"][0][k], dtype=np.float64), lin[k])
        print(f"{name}: {k} normalised by log P_u lies {d:.2e} from the oracle")
        with pytest.raises(AssertionError):
            assert_close(np.asarray(wrong["stats"][0][k], dtype=np.float64), lin[k], what=k)


@extended
@pytest.mark.parametrize("name", CLEAN)
def test_the_far_frame_loses_the_linear_estep_and_not_this_one(G, name):
    case, ref = E.reference(G, name)
    lin = oracle_stats(G, case)
    assert not np.isfinite(float(lin[0]["loglik"]))
    T0 = int(case.lens[0])
    assert np.isfinite(float(ref["loglik"][0])) or T0 < case.Ns[0]
    assert np.isfinite(np.asarray(ref["logZ"], dtype=np.float64)).all()
    for st in ref["stats"]:
        for k in E.BLOCKS:
            if k != "loglik":       # (an utterance shorter than a banded model has log P = -inf, as in the linear call)
                assert np.isfinite(np.asarray(st[k], dtype=np.float64)).all(), (name, k)
    assert np.isfinite(np.asarray(ref["loglik"], dtype=np.float64)[np.asarray(case.lens) >= case.Ns[0]]).all()


@extended
@pytest.mark.parametrize("name", E.NAMES)
def test_the_cases_reach_their_branches(G, name):
    case, ref = E.reference(G, name)
    lens, N = np.asarray(case.lens), case.Ns[0]
    off = offsets(lens)
    A = case.words[0][0].A
    i, j = np.indices(A.shape)
    dense = bool(np.any(A[(j != i) & (j != i + 1)] != 0))
    assert (lens == 1).any() and (lens == 0).any() and ((lens > 0) & (lens < N)).any()
    ll = np.asarray(ref["loglik"], dtype=np.float64)
    lb = np.asarray(ref["logb"], dtype=np.float64)
    if name.endswith("_c0"):
        assert (lb[:, 1] == -np.inf).all() and (ll[lens > 0] == -np.inf).all()
    elif name.endswith("_nan"):
        assert np.isnan(lb[:, 3]).all() and not np.isnan(np.delete(lb, 3, axis=1)).any()
        assert np.isfinite(ll[0]) and np.isnan(np.asarray(ref["logZ"], dtype=np.float64)[lens > 0]).all()
        assert np.all(ref["gamma"] == 0)       # log Z is not finite: the rows are 0
    elif not dense:
        short = (lens > 0) & (lens < N)
        assert (ll[short] == -np.inf).all() and np.isfinite(ll[lens >= N]).all()
        for u in np.nonzero(short)[0]:
            assert np.all(ref["gamma"][off[u]:off[u + 1]] == 0)
    assert ll[lens == 0].tolist() == [0.0] * int((lens == 0).sum())


def test_banded_and_dense_at_both_widths(G):
    seen = set()
    for name in E.NAMES:
        A = E.make(G, name).words[0][0].A
        i, j = np.indices(A.shape)
        seen.add((A.shape[0] > 64, bool(np.any(A[(j != i) & (j != i + 1)] != 0))))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert {E.make(G, n).words[0][0].N > 64 for n in E.DELTA_CASES} == {False, True}


@extended
@pytest.mark.parametrize("name", E.NAMES)
def test_float64_spread(G, name):
    """the float64 restatement against the long-double one: log P_u and log Z_u, the statistics vector block by
    block, and the far frame's posteriors state by state (the figures of estep_log_ref's docstring)"""
    case, ld = E.reference(G, name)
    _, f64 = E.reference(G, name, ft=np.float64)
    d_ll = max(rel_dist(f64["loglik"], ld["loglik"]), rel_dist(f64["logZ"], ld["logZ"]))
    d_st = max(E.block_dist(a[k], b[k]) for a, b in zip(f64["stats"], ld["stats"]) for k in E.BLOCKS)
    d_post = max(E.row_dist(a[LC.FAR_FRAME], b[LC.FAR_FRAME]) for a, b in zip(f64["posts"], ld["posts"]))
    print(f"{name}: float64 spread {d_ll:.1e} | {d_st:.1e} | {d_post:.1e}")
    assert d_ll < 1e-12                         # test_logscore_host.test_float64_spread's bar
    assert max(d_st, d_post) < RTOL / 8         # 8 x the distance, the GPU tests' margin, stays below RTOL


@extended
@pytest.mark.parametrize("name", E.NAMES)
def test_gathered_lattice_is_the_reference_lattice(G, name):
    """estep_log_ref.gathered_fb (only the terms a_ij > 0) against fullestep_log_ref.lattice_fb on the case's own
    log b, delta 0 and 3: equal NaN and infinity patterns; la, lbe, log P and log Z 1e-17 relative; gamma and xi,
    whose exponents of size V carry V 2^-63 from either order of the sums, 16 V 2^-63 relative; the 512-state
    case on the first 6 frames of its utterances"""
    case, ref = E.reference(G, name)
    A = case.words[0][0].A
    off = offsets(case.lens)
    cut = 6 if A.shape[0] > 128 else 10 ** 9
    for u in range(case.U):
        lb = ref["logb"][off[u]:off[u + 1]][:cut]
        for delta in (0, 3):
            a, b = LE.lattice_fb(A, lb, delta), E.gathered_fb(A, lb, delta)
            for k in ("la", "lbe"):
                assert rel_dist(b[k], a[k]) <= 1e-17, (u, delta, k)
            for k in ("gamma", "xi"):
                assert rel_dist(b[k], a[k]) <= 16 * max(a["V"], 1.0) * 2.0 ** -63, (u, delta, k)
            assert rel_dist([b["logP"], b["logZ"]], [a["logP"], a["logZ"]]) <= 1e-17
            assert (a["V"], a["La"], a["T"]) == (b["V"], b["La"], b["T"])
