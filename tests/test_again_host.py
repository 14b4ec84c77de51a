"""What test_again_gpu.py leans on, checked where no GPU is needed: again_cases' prediction of the
utterances that are taken again gives the counts the cases were built for; every utterance that is NOT
predicted keeps the margins under which no other reason can list it (so an exact count on the device is
owed to the rule alone); the cases with hundreds of listed utterances have more of them than
k_backward_fix's grid has groups, so that its loop runs a second round; tails' two tail utterances are
the ones whose beta^ leaves the numbers in the oracle; small is smaller than every target.
The margins are conditions on the inputs, not measurements: if a seed fails them, the seed changes, not
the bound."""
import os

import numpy as np
import pytest

import again_cases as AC
from oracle_lib import ROOT

VARIANTS = ([(n, d, dn) for n in AC.MIX for d, dn in AC.MIX_VARIANTS] +
            [(n, 1, False) for n in AC.MANY + ("tails", "tails_cut", "small")])


@pytest.mark.parametrize("name,delta,dense", VARIANTS)
def test_predicted_counts_and_margins(G, name, delta, dense):
    case = AC.make(G, name, delta, dense)
    mask = AC.listed_mask(case)
    assert int(mask.sum()) == (0 if dense else AC.EXPECTED[name]), case.tag
    # what is listed is what is shorter than its left-to-right model, nothing else
    if not dense:
        assert np.array_equal(mask, (case.lens > 0) & (case.lens < case.N)), case.tag
    # every utterance that is NOT listed is far from every other reason to list it; none is left out
    kept = ~mask
    assert kept.sum() + mask.sum() == case.U
    amin, finite, cmax, bmax = AC.kept_margins(case, kept)
    print(f"{case.tag}: kept {int(kept.sum())}, smallest alpha^[T-1, N-1] {amin:.3g}, largest c_t {cmax:.3g}, "
          f"largest beta^ row sum {bmax:.3g}")
    assert amin >= 1e-100, case.tag
    assert finite, case.tag
    assert cmax <= 1e100, case.tag
    assert bmax <= 1e150, case.tag
    if name not in ("tails", "tails_cut"):
        # the vector tier's criterion names nothing here (GHMM_OPT_KERNELS = 1 counts 0)
        assert not AC.wild_mask(case).any(), case.tag
        assert not np.isnan(case.ref()[0]).any(), case.tag      # (log P of a listed utterance is -inf)


def test_mix_cases_are_what_they_are_for(G):
    for name in AC.MIX:
        case = AC.make(G, name)
        N = case.N
        assert list(case.lens) == [3, 4 * N, N - 3, 6 * N, 5, N - 1, N, 0, 8]
        assert AC.lanes(N) == {"mix16": 16, "mix32": 32, "mix64": 64}[name]
        # listed utterances with several non-empty chunks (8 chunks behind k_combine: T >= 8 fills all)
        mask = AC.listed_mask(case)
        assert np.sum(case.lens[mask] >= 8) >= 1
        assert not mask[6] and case.lens[6] == N      # T = N is kept
        # delta 2 leaves the one-launch path, a dense A lists nothing: the variants share the frames
        assert np.array_equal(AC.make(G, name, 2).X, case.X)
        assert np.array_equal(AC.make(G, name, 1, True).X, case.X)
        A = case.hm.A
        i, j = np.indices(A.shape)
        assert np.all(A[(j != i) & (j != i + 1)] == 0.0)          # band-diagonal
        assert np.all(AC.make(G, name, 1, True).hm.A > 0.0)       # dense


@pytest.mark.parametrize("name", AC.MANY)
def test_many_cases_reach_a_second_round(G, name):
    case = AC.make(G, name)
    n_short, n_fit = AC.MANY_PLAN[name][:2]
    assert case.U == n_short + n_fit
    assert 6000 <= case.F <= 8000
    n = AC.listed(case)
    blocks, gpw = AC.fix_grid(case.N, case.U)
    groups = AC.fix_groups(case.N, case.U)
    assert (blocks, gpw) == {"many64": (256, 1), "many32": (256, 2), "many16": (256, 4)}[name]
    assert (case.U + gpw - 1) // gpw > AC.FIX_BLOCKS       # the cap on the grid is what binds
    assert groups < n <= 2 * groups                          # a second round, and no third
    # in length order (longest first, as the passes visit them) the listed utterances fill the first
    # round and leave a second one, of utterances that have frames (the list's own order is the order
    # of the atomics: whichever utterances the second round gets, each has work in it)
    order = np.argsort(-case.lens, kind="stable")
    in_order = order[AC.listed_mask(case)[order]]
    first, second = in_order[:groups], in_order[groups:]
    assert len(first) == groups and len(second) == n - groups > 0
    assert case.lens[second].min() >= 1 and case.lens[first].min() >= 1
    # the fitting utterances lie among the listed ones, not behind them
    fit = np.nonzero(~AC.listed_mask(case))[0]
    assert fit[0] < case.U // 4 and fit[-1] > 3 * case.U // 4
    if name == "many16":
        assert AC.scan_upb(case.N, case.U, case.F) == (16, 2)   # fix_in_block at 16 utterances per block


def test_grid_restatement_is_the_hosts():
    """the numbers again_cases restates are the ones the host code launches with"""
    src = open(os.path.join(ROOT, "speech-recognition-hmm-continuous_amd", "csrc", "ghmm_hip.hip")).read()
    assert "#define GHMM_FIX_BLOCKS 256u" in src
    assert "blocks < GHMM_FIX_BLOCKS ? blocks : GHMM_FIX_BLOCKS" in src
    assert "L(N <= 16 ? 16 : N <= 32 ? 32 : 64)" in src
    pair = open(os.path.join(ROOT, "speech-recognition-hmm-continuous_amd", "csrc", "ghmm_pair.hpp")).read()
    assert "idx += gridDim.x * (WAVE / L)" in pair
    assert "constexpr int SC_UPB = 4;" in pair and "constexpr int BT_K = 680;" in pair
    assert AC.fix_grid(10, 9) == (3, 4) and AC.fix_grid(40, 300) == (256, 1) and AC.fix_grid(20, 511) == (256, 2)
    assert AC.scan_upb(40, 300, 7000) == (4, 8) and AC.scan_upb(20, 560, 7000) == (8, 4)
    assert AC.scan_upb(10, 4, 4 * 200) == (4, 8) and AC.scan_upb(10, 4, 4 * 100) == (8, 4)


def test_tails_overflow_where_they_should(G):
    case = AC.make(G, "tails")
    assert list(case.lens) == [3, 40, 7, 60, 4, 6]
    wild = AC.wild_mask(case)
    assert list(np.nonzero(wild)[0]) == [4, 5]
    stats, d = case.ref()
    assert np.isnan(stats).any()                    # the reference's NaN pattern is in the statistics
    o = AC.offsets(case.lens)
    for u in np.nonzero(~wild)[0]:
        for k in ("alpha", "beta", "scale"):
            assert np.all(np.isfinite(d[k][o[u]:o[u + 1]])), (u, k)
    assert AC.listed(case) == 4
    cut = AC.make(G, "tails_cut")
    assert list(cut.lens) == [3, 40, 4] and list(np.nonzero(AC.wild_mask(cut))[0]) == [2]
    assert np.array_equal(cut.X[-4:], case.X[o[4]:o[5]])
    assert cut.U < case.U


def test_small_is_smaller_than_every_target(G):
    small = AC.make(G, "small")
    assert list(small.lens) == [3, 40, 7, 60] and AC.listed(small) == 2
    mix16 = AC.make(G, "mix16")
    assert np.array_equal(small.X, mix16.X[:small.F])
    for a, b in zip(small.hm.arrays(), mix16.hm.arrays()):
        assert np.array_equal(a, b)
    for name in AC.MIX + AC.MANY + ("tails",):
        assert small.U < AC.make(G, name).U, name
