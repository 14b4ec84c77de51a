"""What test_grammar_gpu.py leans on, checked where no GPU is needed: the two entry points are exported and
declared; grammar_cases' restatement of the recursion under a word-pair grammar is the definition (it
equals an enumeration of ALL composite paths with their word boundaries on a tiny vocabulary, the score
bit for bit, the path under the tie rules); consequences (a), (b) and (c) of include/ghmm.h hold for it
against connect_cases' and align_cases' restatements; bigram_log counts what a hand counts; and every
(case, grammar) pair that the GPU tests compare keeps, on the oracle's float64 log b, the margin under
which a differing path cannot be blamed on rounding, in all utterances but at most one; and the forms of
the entry pass (table staged or read from L2, slices per word, unrolled rounds, tail) that the cases reach.
The margins are conditions on the inputs, not measurements: if a seed fails them, the seed changes, not
the bound."""
import itertools
import os

import numpy as np
import pytest

import align_cases as AC
import connect_cases as CC
import grammar_cases as GC
from fullcov_support import offsets
from oracle_lib import ROOT

INF = np.inf


def test_entry_points_are_exported_and_declared(G):
    lib = G.hip_lib()
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    for name, face in (("ghmm_connect_grammar_streams", "connect_grammar_streams"),
                       ("ghmm_connect_grammar_full_streams", "connect_grammar_full_streams")):
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
        assert f"int {name}(ghmm_ctx" in hdr, name
        assert callable(getattr(G.Context, face)), face
    assert "#define GHMM_GRAMMAR_MAX_WORDS 256" in hdr        # the cap on K is a named constant
    assert callable(G.bigram_log)


# ------------------------------------------------------------- the restatement is the definition

def enumerate_paths(logAs, logb, start, pair, fin):
    """every composite path of T frames as [(word, state)] with its entries and its score, the sums taken
    in the lattice's order: start + log b, then ((d + log a) or (d + pair)) + log b left to right, then
    + fin.  A path starts in a word's first state and ends in a word's last; a word is entered from a
    word's (or its own) last state only."""
    Ns = [a.shape[0] for a in logAs]
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    T = len(logb)
    nodes = [(k, j) for k, N in enumerate(Ns) for j in range(N)]
    out = []
    for states in itertools.product(nodes, repeat=T):
        if states[0][1] != 0 or states[-1][1] != Ns[states[-1][0]] - 1:
            continue
        entered_opts = []
        for t in range(1, T):
            (pk, pj), (k, j) = states[t - 1], states[t]
            opts = []
            if pk == k and logAs[k][pj, j] != -INF:
                opts.append(False)
            if j == 0 and pj == Ns[pk] - 1:
                opts.append(True)
            entered_opts.append(opts)
        for ent in itertools.product(*entered_opts):
            d = start[states[0][0]] + logb[0, bo[states[0][0]]]
            for t in range(1, T):
                (pk, pj), (k, j) = states[t - 1], states[t]
                d = (d + pair[pk, k] if ent[t - 1] else d + logAs[k][pj, j]) + logb[t, bo[k] + j]
            out.append((d + fin[states[-1][0]], states, (True,) + ent))
    return out


def backward_key(states, ent):
    """the tie rules as an order on paths of equal score, decided from the last frame backwards as the
    trace does: the lowest final word; at every frame staying in the word (the lowest predecessor) ahead
    of entering (from the lowest word)"""
    key = [states[-1][0]]
    for t in range(len(states) - 1, 0, -1):
        key += [1, states[t - 1][0]] if ent[t] else [0, states[t - 1][1]]
    return key


def check_against_enumeration(logAs, logb, start, pair, fin, want_ties):
    word, path, begin, score, gap = GC.decode_log(logAs, logb, start, pair, fin)
    paths = enumerate_paths(logAs, logb, start, pair, fin)
    best = max(x[0] for x in paths)
    assert np.float64(score).tobytes() == np.float64(best).tobytes(), (score, best)
    if best == -INF:
        return False
    top = [x for x in paths if x[0] == best]
    assert (len(top) > 1 and gap == 0) if want_ties else (len(top) == 1 and gap > 0)
    _, states, ent = min(top, key=lambda x: backward_key(x[1], x[2]))
    assert [k for k, _ in states] == word.tolist()
    assert [j for _, j in states] == path.tolist()
    assert [int(e) for e in ent] == begin.tolist()
    # (c): the decoded string uses no forbidden move
    s = [k for (k, _), e in zip(states, ent) if e]
    assert start[s[0]] > -INF and fin[s[-1]] > -INF and all(pair[w, k] > -INF for w, k in zip(s[:-1], s[1:]))
    return True


TINY = [CC.log_a(np.array([[0.6, 0.4], [0.0, 1.0]])), CC.log_a(np.ones((1, 1))),
        CC.log_a(np.array([[0.3, 0.7], [0.0, 1.0]]))]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_restatement_equals_the_enumeration_of_all_paths(T):
    """K = 3, N = (2, 1, 2): random log b, random grammars with -inf entries, no ties"""
    rng = np.random.default_rng(300 * T + 11)
    finite = 0
    for i in range(6):
        logb = rng.normal(-3.0, 2.0, (T, 5))
        start, pair, fin = GC.random(3, 1000 * T + i, forbid=0.3)
        finite += check_against_enumeration(TINY, logb, start, pair, fin, want_ties=False)
    assert finite >= 3, "too few of the drawn grammars leave a path"


@pytest.mark.parametrize("T", [2, 3, 4, 5])
def test_restatement_follows_the_tie_rules(T):
    """integers throughout, so that every sum is exact: all log b equal, log a in {0, -inf}, the grammar in
    {0, -1, -inf}.  Many paths share the best score; the restatement's is the one the tie rules name"""
    logAs = [np.array([[0.0, 0.0], [-INF, 0.0]]), np.zeros((1, 1)), np.array([[0.0, 0.0], [-INF, 0.0]])]
    start = np.array([0.0, 0.0, -1.0])
    pair = np.array([[0.0, 0.0, -INF], [0.0, -INF, 0.0], [0.0, 0.0, 0.0]])
    fin = np.array([0.0, 0.0, 0.0])
    assert check_against_enumeration(logAs, np.full((T, 5), -2.0), start, pair, fin, want_ties=True)


def test_a_nan_end_enters_nothing():
    """x_t(k) starts at -inf with predecessor word 0 and a NaN candidate never wins: a word whose end is
    NaN in every frame is never left and never picked, so no decoded string holds it, whatever pair says"""
    rng = np.random.default_rng(12)
    logb = rng.normal(-3.0, 1.0, (5, 5))
    logb[:, 2] = np.nan                                    # word 1's only state: its end
    for g in (GC.flat(3, 0.0), GC.flat(3, 4.0), GC.random(3, 5, forbid=0.0)):
        word, path, begin, score, gap = GC.decode_log(TINY, logb, *g)
        assert np.isfinite(score) and 1 not in word


# ------------------------------------------------------------- (a), (b), (c) for the restatement

@pytest.fixture(scope="module")
def cases(G):
    made = {}

    def get(name):
        if name not in made:
            case = GC.make(G, name)
            made[name] = (case, GC.oracle_log_b(case))
        return made[name]
    return get


@pytest.mark.parametrize("name", ["narrow", "mixed", "wide", "many", "ones", "full", "thick"])
def test_a_flat_grammar_is_the_flat_penalty(cases, name):
    """(a): the score equals connect_cases.decode_log's as a value at every penalty; at p = 0 and -inf the
    decoding is the same on every utterance, ties included (ones); at other p wherever connect's gap
    exceeds GAP"""
    case, lb = cases(name)
    for p in CC.penalties(name):
        cw, cp, cb, cs, cgap = CC.decode(case, lb, p)
        gw, gp, gb, gs, ggap = GC.decode(case, lb, *GC.flat(case.K, p))
        assert np.array_equal(gs, cs, equal_nan=True), (name, p)
        where = np.ones(case.F, dtype=bool) if p in (0.0, -INF) else GC.compared(case, cgap)
        assert np.array_equal(gw[where], cw[where]) and np.array_equal(gp[where], cp[where]) \
            and np.array_equal(gb[where], cb[where]), (name, p)


@pytest.mark.parametrize("name", sorted(GC.CHAINS))
def test_b_a_chain_grammar_is_the_forced_alignment(cases, name):
    """(b): the score equals align_cases.align_log's as a value; where it is finite, word, path and begin
    are the alignment's"""
    case, lb = cases(name)
    logAs, off = GC.log_as(case), offsets(case.lens)
    finite = 0
    for tr in GC.CHAINS[name]:
        g = GC.chain(case.K, tr)
        for u in range(case.U):
            x = lb[off[u]:off[u + 1]]
            aw, ap, ab, asc, _ = AC.align_log(logAs, case.bo, x, tr)
            gw, gp, gb, gsc, _ = GC.decode_log(logAs, x, *g)
            assert gsc == asc, (name, tr, u, gsc, asc)
            if np.isfinite(asc) and len(x):
                finite += 1
                assert np.array_equal(gw, aw) and np.array_equal(gp, ap) and np.array_equal(gb, ab), (name, tr, u)
    assert finite >= len(GC.CHAINS[name])


@pytest.mark.parametrize("name", sorted(GC.GPU_GRAMMARS))
def test_c_and_the_margins_of_every_pair_the_gpu_tests_compare(cases, name):
    """(c) for the restatement, and at most MAX_BELOW_GAP utterances of the pair with a gap of GAP or less
    on the oracle's log b"""
    case, lb = cases(name)
    if name == "holes":
        CC.holes_pattern(case, lb)
    for which in GC.GPU_GRAMMARS[name]:
        g = GC.grammar(case, which)
        word, path, begin, score, gap = GC.decode(case, lb, *g)
        got = GC.allowed(case, word, begin, score, *g)
        live = case.lens > 0
        print(name, which, "scores", score, "gaps", gap, got)
        assert np.sum(gap[live] <= GC.GAP) <= GC.MAX_BELOW_GAP, (name, which, gap)
        assert np.all(score[~live] == 0.0)
        if which == "norepeat":
            assert all(w != k for s in got for w, k in zip(s[:-1], s[1:]))
        if which != "flat:-5" and name not in ("holes", "cap"):
            assert np.isfinite(score[live]).sum() >= 1, "the grammar leaves no utterance a path"


def test_the_random_grammars_forbid_and_the_k256_case_is_at_the_cap(cases):
    case, lb = cases("k256")
    assert case.K == GC.MAX_K == 256 and case.NS == 640 and set(case.Ns) == {2, 3} and case.lens.max() <= 20
    assert sorted(int(T) for T in case.lens)[:2] == [0, 1]
    assert 255 in {k for s in case.spoken for k in s}
    for name in GC.GPU_GRAMMARS:
        K = cases(name)[0].K
        start, pair, fin = GC.random(K, GC.RANDOM_SEED[name])
        if K > 4:
            assert 0.2 < np.mean(pair == -INF) < 0.4
            assert (start == -INF).any() or (fin == -INF).any()
        assert not np.isnan(pair).any() and pair.max() <= 0 and pair[np.isfinite(pair)].min() >= -6
    # a predecessor word above 127 and the byte's last value are reachable: some utterance enters from them
    g = GC.norepeat(256)
    word, path, begin, score, gap = GC.decode(case, lb, *g)
    off = offsets(case.lens)
    first = np.zeros(case.F, dtype=bool)
    first[off[:-1][case.lens > 0]] = True
    entered = np.nonzero((begin == 1) & ~first)[0]
    assert len(entered) and word[entered - 1].max() >= 128


def test_the_entry_pass_is_held_in_its_forms_and_k100_and_k72_decide_in_both_loops(cases):
    """grammar_entry per case as grammar_cases.entry_pass restates the header's formulas: the table read from
    L2 in sixteen full rounds (k256), in a tail alone with R = 4 (cap), in rounds followed by a tail with
    R = 2 (k100); staged in LDS with rounds and a tail (many, k72).  Under k100's and k72's random grammars
    the traced path takes a predecessor word from the tail (w >= TAIL_FROM) and one from an unrolled round,
    in both slices (even and odd w)"""
    table = {}
    for name in ("k256", "cap", "k100", "many", "k72"):
        case = cases(name)[0]
        table[name] = GC.entry_pass(case.NS, case.K)
        print(name, "K", case.K, "NS", case.NS, "(staged, R, [(unrolled rounds, tail iterations) per slice])", table[name])
    assert table["k256"] == (False, 1, [(16, 0)])
    assert table["cap"] == (False, 4, [(0, 8)] * 4)
    assert table["k100"] == (False, 2, [(3, 2)] * 2)
    assert table["k72"] == (True, 2, [(4, 4)] * 2)
    staged, R, slices = table["many"]
    assert staged and R == 3 and all(rounds > 0 for rounds, _ in slices)
    for name, K, NS in (("k100", 100, 250), ("k72", 72, 180)):
        case, lb = cases(name)
        assert case.K == K and case.NS == NS and set(case.Ns) == {2, 3} and case.lens.max() <= 20
        word, path, begin, score, gap = GC.decode(case, lb, *GC.grammar(case, "random"))
        off = offsets(case.lens)
        first = np.zeros(case.F, dtype=bool)
        first[off[:-1][case.lens > 0]] = True
        entered = np.nonzero((begin == 1) & ~first & GC.compared(case, gap))[0]
        pred = word[entered - 1]
        for r in range(2):
            mine = pred[pred % 2 == r]
            assert (mine >= GC.TAIL_FROM[name]).any() and (mine < GC.TAIL_FROM[name]).any(), (name, r, sorted(pred.tolist()))
    assert 200 <= cases("k100")[0].NS


# ------------------------------------------------------------- bigram_log

def test_bigram_log_on_hand_counted_transcripts(G):
    tr = [(0, 1, 1), (0, 2), (1,), ()]
    # starts: 0 twice, 1 once.  pairs: (0,1), (1,1), (0,2).  ends: 1 twice (after (0,1,1) and (1,)), 2 once.
    start, pair, fin = G.bigram_log(tr, 3, alpha=0.0)
    with np.errstate(divide="ignore"):
        assert np.array_equal(start, np.log(np.array([2, 1, 0]) / 3))
        # row 0: two events, (0,1) and (0,2).  row 1: (1,1) and two ends.  row 2: one end.
        assert np.array_equal(pair, np.log(np.array([[0, 1 / 2, 1 / 2], [0, 1 / 3, 0], [0, 0, 0]])))
        assert np.array_equal(fin, np.log(np.array([0, 2 / 3, 1 / 1])))
    start, pair, fin = G.bigram_log(tr, 3, alpha=1.0)
    assert np.array_equal(start, np.log(np.array([3, 2, 1]) / 6))
    assert np.array_equal(pair, np.log(np.array([[1 / 6, 2 / 6, 2 / 6], [1 / 7, 2 / 7, 1 / 7], [1 / 5, 1 / 5, 1 / 5]])))
    assert np.array_equal(fin, np.log(np.array([1 / 6, 3 / 7, 2 / 5])))
    assert np.isclose(np.exp(start).sum(), 1) and np.allclose(np.exp(pair).sum(1) + np.exp(fin), 1)
    # a word that never occurs, alpha = 0: its row is all -inf, nothing is NaN
    start, pair, fin = G.bigram_log([(0, 0)], 2, alpha=0.0)
    assert np.array_equal(pair, [[np.log(0.5), -INF], [-INF, -INF]]) and np.array_equal(fin, [np.log(0.5), -INF])
    assert np.array_equal(start, [0.0, -INF])
    with pytest.raises(ValueError):
        G.bigram_log([(0, 3)], 3)
    with pytest.raises(ValueError):
        G.bigram_log([(0,)], 3, alpha=-1.0)
