"""lensweep_cases.py holds what test_lensweep_gpu.py leans on — CPU only, with the long-double references
the project already has (logscore_ref.lattice_scores, estep_log_ref.lattice_fb, fulllogscore_ref.lattice) on
the references' own log b.  These are conditions on the cases, not measurements: where one fails the cases
change, not the assertion."""
import numpy as np
import pytest

import estep_log_ref as E
import fulllogscore_ref as LR
import lensweep_cases as S
import logscore_ref as R
from fullcov_support import extended, offsets

ALL = S.NAMES["diag"] + S.NAMES["full"]


def reference_logb(case):
    """the reference's float64 log b of every utterance, by utterance number"""
    X = np.concatenate(case.frames)
    logb = R.log_b([case.hm], [X]) if case.kind == "diag" else LR.log_emission(case.hm, X, np.float64)
    off = offsets(S.LENS)
    return [logb[off[i]:off[i + 1]] for i in range(S.U)]


def test_the_lengths_are_the_sweep():
    assert S.LENS == tuple(range(0, 2 * S.PF + 3)) + tuple(range(5 * S.PF, 6 * S.PF))
    if S.PF == 8:
        assert (S.U, S.F) == (27, 519)
    for T in (0, 1, 2, S.PF, S.PF + 1, 2 * S.PF, 2 * S.PF + 1):
        assert T in S.LENS, T
    assert len(set(S.LENS)) == S.U
    for perm in S.ORDERS.values():
        assert sorted(perm) == list(range(S.U))
    assert len(set(S.ORDERS.values())) == 3
    assert set(S.LANES.values()) == {16, 32, 64} and max(S.STATES) <= 5 * S.PF


@extended
@pytest.mark.parametrize("name", ALL)
def test_every_residue_has_a_finite_score(G, name):
    """every T >= 1 has a finite log Z; every residue (T - 1) mod PF occurs with a finite log P and with T < PF;
    the two references of the score agree on it"""
    case = S.make(G, name)
    logb = reference_logb(case)
    finite, short = set(), set()
    for i, T in enumerate(S.LENS):
        ut = E.lattice_fb(case.hm.A, logb[i], 1)
        if T == 0:
            continue
        assert np.isfinite(ut["logZ"]), (name, T)
        assert ut["logZ"] == LR.lattice(case.hm.A, logb[i], 0) and ut["logP"] == LR.lattice(case.hm.A, logb[i], 1)
        if np.isfinite(ut["logP"]):
            finite.add((T - 1) % S.PF)
            # the walk keeps the gammas of size 1: they are compared above the absolute floor of their bound
            assert ut["logP"] - ut["logZ"] > -30.0, (name, T, float(ut["logP"] - ut["logZ"]))
        if T < S.PF:
            short.add((T - 1) % S.PF)
        if not case.dense:
            assert np.isfinite(ut["logP"]) == (T >= case.N), (name, T)
    assert finite == set(range(S.PF)), (name, finite)
    assert short == set(range(S.PF - 1)), (name, short)     # (T - 1 = PF - 1 is one whole queue: T = PF)
    for fs in (0, 1):
        scores, bound = R.lattice_scores(case.hm.A, np.concatenate(logb), S.LENS, fs)
        assert scores[0] == 0.0 and bound[0] == 0.0 and (bound[1:] > 0).all()


def test_wave_mates_differ_in_length():
    """in the kernels' length-sorted order (by decreasing length, stable) every group of WAVE / L consecutive
    utterances, the ones that share a wave, holds at least two different lengths (L = 64: one utterance a wave)"""
    by_length = sorted(S.LENS, reverse=True)
    for L in (16, 32):
        g = S.WAVE // L
        groups = [by_length[k:k + g] for k in range(0, S.U, g)]
        assert all(len(set(grp)) >= 2 for grp in groups if len(grp) >= 2), L
        assert sum(len(grp) >= 2 for grp in groups) >= S.U // g
        # ... and the trip counts of the main loop differ inside a wave at least once
        assert any(len({(T - 1) // S.PF for T in grp if T}) >= 2 for grp in groups), L


def test_neighbours_differ_between_the_orders():
    """the three memory orders give every non-empty utterance at least two different right-hand neighbours; in
    the mix order the clean utterances that lie directly in front of a poisoned one cover, over the two
    poisons, every residue (T - 1) mod PF"""
    for i, T in enumerate(S.LENS):
        if T == 0:
            continue
        assert len({S.right_neighbour(o, i) for o in S.ORDERS}) >= 2, T
    in_front = set()
    for poison in S.POISONS:
        want = 1 if poison == "odd" else 0
        assert [S.poisoned(i, poison) for i in range(S.U)] == [T > 0 and T % 2 == want for T in S.LENS]
        for i, T in enumerate(S.LENS):
            j = S.right_neighbour("mix", i)
            if T and not S.poisoned(i, poison) and j is not None and S.poisoned(j, poison):
                in_front.add((T - 1) % S.PF)
    assert in_front == set(range(S.PF)), in_front
    assert not any(S.poisoned(i, None) for i in range(S.U))


@pytest.mark.parametrize("name", ALL)
def test_corpora_hold_the_same_utterances(G, name):
    case = S.make(G, name)
    for order in S.ORDERS:
        X, lens = case.corpus(order)
        assert X.shape == (S.F, S.D) and lens.tolist() == [S.LENS[i] for i in S.ORDERS[order]]
        rows = S.by_utterance(X, order)
        assert all(np.array_equal(rows[i], case.frames[i]) for i in range(S.U))
        assert np.array_equal(S.per_utterance(lens, order), S.LENS)
        for poison in S.POISONS:
            Xp, lp = case.corpus(order, poison)
            assert np.array_equal(lp, lens)
            for i, r in enumerate(S.by_utterance(Xp, order)):
                assert np.isnan(r).all() if S.poisoned(i, poison) else np.array_equal(r, case.frames[i])
