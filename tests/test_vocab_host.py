"""What test_vocab_streams_gpu.py leans on, checked where no GPU is needed: the four entry points are
exported and declared, and the vocabularies of vocab_cases.py, in the float64 of the oracle, are not
vacuous and keep the margins under which a path or a winner that differs from the reference cannot be
blamed on rounding.  The margins are conditions on the inputs, not measurements: if a seed fails them, the
seed changes, not the bound."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vocab_cases as V
from oracle_lib import ROOT

CALLS = ("ghmm_viterbi_streams", "ghmm_score_streams_batch", "ghmm_viterbi_streams_batch",
         "ghmm_recognise_streams")


def test_entry_points_are_exported_and_declared(G):
    lib = G.hip_lib()
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
        assert f"int {name}(ghmm_ctx" in hdr, name
    for name in ("viterbi_streams", "score_streams_batch", "viterbi_streams_batch", "recognise_streams"):
        assert callable(getattr(G.Context, name)), name
    assert "exist for the full-covariance models only" not in hdr


@pytest.fixture(scope="module")
def refs(G):
    out = {}
    for name in V.VOCABS + V.TIES + ("one70",):
        case = V.make(G, name)
        out[name] = (case, V.Reference(case))
    return out


@pytest.mark.parametrize("name", V.VOCABS)
def test_vocabulary_is_not_vacuous(refs, name):
    case, ref = refs[name]
    vit = ref.vit
    assert not np.isnan(vit).any()
    long_enough = np.array([[T >= N for T in case.lens] for N in case.Ns])
    assert 2 * np.isfinite(vit[long_enough]).sum() >= long_enough.sum() > 0     # finite scores
    won = ref.words[(case.lens > 0) & np.isfinite(vit).any(0)]
    assert len(set(won.tolist())) >= 2, won
    hopeless = [u for u, T in enumerate(case.lens) if 0 < T < min(case.Ns) and np.all(vit[:, u] == -np.inf)]
    assert hopeless and np.all(ref.words[hopeless] == 0)    # too short for every word: all -inf, word 0
    assert np.any(case.lens == 0) and np.all(vit[:, case.lens == 0] == 0.0)
    fwd = V.forward_table(case)
    assert np.isfinite(fwd[long_enough]).sum() >= 2 and np.all(fwd[:, case.lens == 0] == 0.0)


@pytest.mark.parametrize("name", V.VOCABS + V.TIES)
def test_shapes_are_the_ones_the_kernels_branch_on(refs, name):
    case, _ = refs[name]
    assert (16 if max(case.Ns) <= 16 else 32 if max(case.Ns) <= 32 else 64) == V.LANES[name]
    banded = [bool(np.all(np.triu(w[0].A, 2) == 0) and np.all(np.tril(w[0].A, -1) == 0)) for w in case.words]
    assert True in banded and False in banded           # both steps of viterbi_run in one launch
    for w in case.words:
        assert all(np.array_equal(h.A, w[0].A) and h.N == w[0].N for h in w)
    for p in range(case.P):
        assert len({(w[p].M, w[p].D) for w in case.words}) == 1
        assert len(case.Xs[p]) == case.F and case.Xs[p].shape[1] == case.words[0][p].D
    if name == "narrow":
        assert [(w.M, w.D) for w in case.words[0]] == [(1, 3), (3, 9), (2, 17)]
    if name == "wide":
        assert case.NS == 97


@pytest.mark.parametrize("name", V.VOCABS + ("one70",))
def test_margins(refs, name):
    """every (word, utterance) pair with a finite score keeps more than GAP between the best and the
    runner-up predecessor at every frame of its path, and the two best words of every utterance differ by
    more than GAP relative (an utterance of no frames scores an exact 0 under every word on either side:
    rounding has no part in it)"""
    case, ref = refs[name]
    fin = np.isfinite(ref.vit) & (case.lens > 0)[None, :]
    assert fin.any() and np.all(ref.gap[fin] > V.GAP), ref.gap[fin].min()
    assert np.all(V.top_two_margin(ref.vit)[case.lens > 0] > V.GAP)


def test_one70_takes_the_lattice_of_more_states_than_lanes(refs):
    case, ref = refs["one70"]
    assert case.K == 1 and case.P == 2 and case.Ns == [70] and list(case.lens) == [80, 3]
    assert np.isfinite(ref.vit[0, 0]) and ref.vit[0, 1] == -np.inf


def test_tie_variant_has_an_exact_tie_at_the_top(refs):
    case, ref = refs["mixed-tie"]
    vit = ref.vit
    assert np.array_equal(vit[0], vit[3])
    top = np.isfinite(vit[0]) & (vit[0] == vit.max(0)) & (case.lens > 0)
    assert top.any() and np.all(ref.words[top] == 0) and 3 not in ref.words
    # and the word of equal transitions and identical states: every predecessor ties from frame 2 on
    ties = case.words[2]
    assert np.all(ties[0].A == ties[0].A[0, 0]) and all(np.all(h.mean == h.mean[0]) for h in ties)
    lb = ref.logb[2]
    assert np.all(lb == lb[:, :1])
    u = int(np.argmax(case.lens))
    off = np.concatenate([[0], np.cumsum(case.lens)])
    path, score = O.viterbi_lattice(ties[0].A, lb[off[u]:off[u + 1]])
    assert np.isfinite(score) and np.all(path[:-1] == 0) and path[-1] == ties[0].N - 1


def test_far_underflows_in_the_linear_domain_only(G):
    case = V.make(G, "far")
    fwd = V.forward_table(case)
    assert not np.isfinite(fwd[0, 0]) and np.isfinite(fwd[:, 1]).all()
    b = np.prod([O.emission(h, X) for h, X in zip(case.words[0], case.Xs)], axis=0)
    assert np.all(b[5] == 0.0) and all(np.all(O.emission(h, X)[5] > 0) for h, X in zip(case.words[0], case.Xs))
    assert np.isfinite(V.Reference(case).vit).all()
