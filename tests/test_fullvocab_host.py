"""What test_fullvocab_streams_gpu.py leans on, checked where no GPU is needed: the vocabularies of
fullvocab_cases.py in float64 (fullstreams_ref's log b, oracle_lib.viterbi_lattice, fulllogscore_ref's
lattice through fullstreams_ref.logscore) hold finite scores, several winners, an utterance that no word
can end, and in the tie variant an exact tie; and the winner rule as a pure function on hand-written
tables.  These are conditions on the inputs: with them no assertion of the GPU tests is vacuous."""
import numpy as np
import pytest

import fullvocab_cases as V


@pytest.fixture(scope="module")
def tables(G):
    out = {}
    for name in V.VOCABS + ("mixed-tie",):
        case = V.make(G, name)
        out[name] = (case, V.viterbi_table(case))
    return out


@pytest.mark.parametrize("name", V.VOCABS)
def test_vocabulary_is_not_vacuous(tables, name):
    case, vit = tables[name]
    assert not np.isnan(vit).any()
    long_enough = np.array([[T >= N for T in case.lens] for N in case.Ns])
    assert 2 * np.isfinite(vit[long_enough]).sum() >= long_enough.sum() > 0
    won = V.winners(vit)[(case.lens > 0) & np.isfinite(vit).any(0)]
    assert len(set(won.tolist())) >= 2, won
    hopeless = [u for u, T in enumerate(case.lens) if 0 < T < min(case.Ns) and np.all(vit[:, u] == -np.inf)]
    assert hopeless                                     # too short for every word: all -inf, word 0
    assert np.all(vit[:, case.lens == 0] == 0.0)


@pytest.mark.parametrize("name", V.VOCABS)
def test_shapes_are_the_ones_the_kernels_branch_on(G, name):
    case = V.make(G, name)
    L = {"narrow": 16, "mixed": 32, "wide": 64}[name]
    assert (16 if max(case.Ns) <= 16 else 32 if max(case.Ns) <= 32 else 64) == L
    banded = [bool(np.all(np.triu(w[0].A, 2) == 0) and np.all(np.tril(w[0].A, -1) == 0)) for w in case.words]
    assert True in banded and False in banded           # both steps of viterbi_run in one launch
    for w in case.words:
        assert all(np.array_equal(h.A, w[0].A) and h.N == w[0].N for h in w)
    for p in range(case.P):
        assert len({(w[p].M, w[p].D) for w in case.words}) == 1
        assert len(case.Xs[p]) == case.F and case.Xs[p].shape[1] == case.words[0][p].D
    if name == "wide":
        assert case.NS == 97


def test_tie_variant_has_an_exact_tie_at_the_top(tables):
    case, vit = tables["mixed-tie"]
    assert np.array_equal(vit[0], vit[3])
    top = np.isfinite(vit[0]) & (vit[0] == vit.max(0)) & (case.lens > 0)
    assert top.any()
    assert np.all(V.winners(vit)[top] == 0)


def test_far_underflows_in_the_linear_domain_only(G):
    case = V.make(G, "far")
    lin = V.score_table(case)
    assert not np.isfinite(lin[0, 0])
    for fs in (0, 1):
        assert np.isfinite(V.logscore_table(case, fs)).all()


def test_winner_rule():
    nan, inf = np.nan, np.inf
    table = np.array([
        # NaN first, NaN last, all NaN, all -inf, tie of 0 and 2, tie of 1 and 2, +inf, a later maximum
        [nan, -3.0, nan, -inf, -1.0, -9.0, 0.0, -5.0],
        [-7.0, -2.0, nan, -inf, -4.0, -2.0, inf, -4.0],
        [-8.0, nan, nan, -inf, -1.0, -2.0, inf, -3.0],
    ])
    assert V.winners(table).tolist() == [1, 1, 0, 0, 0, 1, 1, 2]
    assert V.winners(np.array([[nan], [-inf]])).tolist() == [1]      # a NaN never beats a number
    assert V.winners(np.array([[-inf], [nan]])).tolist() == [0]
    assert V.winners(np.zeros((3, 2))).tolist() == [0, 0]            # T = 0: every word scores 0
    assert V.winners(np.zeros((1, 4))).tolist() == [0, 0, 0, 0]
    assert V.winners(np.zeros((2, 0))).tolist() == []
