"""What test_connect_gpu.py leans on, checked where no GPU is needed: the two entry points are exported and
declared; connect_cases' restatement of the connected-word recursion is the definition (it equals an
enumeration of ALL composite paths on a tiny vocabulary, the score bit for bit, the path under the tie
rules); the cases, on the oracle's float64 log b, keep the margin under which a differing path cannot be
blamed on rounding; and the composed utterances that decode to what was spoken are the recorded ones.
The margins are conditions on the inputs, not measurements: if a seed fails them, the seed changes, not
the bound."""
import itertools
import os

import numpy as np
import pytest

import connect_cases as CC
from oracle_lib import ROOT

INF = np.inf



def test_entry_points_are_exported_and_declared(G):
    lib = G.hip_lib()
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    for name, face in (("ghmm_connect_streams", "connect_streams"),
                       ("ghmm_connect_full_streams", "connect_full_streams")):
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
        assert f"int {name}(ghmm_ctx" in hdr, name
        assert callable(getattr(G.Context, face)), face
    assert "2048" in hdr        # the cap on the composite states is stated


def test_word_segments():
    G_word = np.array([5, 5, 5, 5, 2, 2, 7, 3, 3, 3], dtype=np.int32)
    begin = np.array([1, 0, 1, 0, 1, 0, 1, 1, 0, 0], dtype=np.int32)
    from _load import ghmm
    seg = ghmm().word_segments(G_word, begin, [6, 0, 1, 3])
    assert seg == [[(5, 0, 1), (5, 2, 3), (2, 4, 5)], [], [(7, 0, 0)], [(3, 0, 2)]]
    with pytest.raises(ValueError):
        ghmm().word_segments(G_word, np.zeros(10, dtype=np.int32), [10])


# ------------------------------------------------------------- the restatement is the definition

def enumerate_paths(logAs, logb, p):
    """every composite path of T frames as [(word, state, entered)] with its score, the sums taken in the
    lattice's order: ((d + log a) or (e + p)) + log b, left to right.  A path starts in a word's first
    state; a word may be entered from another word's (or its own) last state only."""
    Ns = [a.shape[0] for a in logAs]
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    T = len(logb)
    nodes = [(k, j) for k, N in enumerate(Ns) for j in range(N)]
    out = []
    for states in itertools.product(nodes, repeat=T):
        if states[0][1] != 0:
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
            d = 0.0 + logb[0, bo[states[0][0]]]
            for t in range(1, T):
                (pk, pj), (k, j) = states[t - 1], states[t]
                d = (d + p if ent[t - 1] else d + logAs[k][pj, j]) + logb[t, bo[k] + j]
            out.append((d, states, (True,) + ent))
    return out


def backward_key(states, ent, Ns):
    """the tie rules as an order on paths of equal score, decided from the last frame backwards as the
    trace does: the lowest final word; at every frame staying in the word (the lowest predecessor) ahead
    of entering (from the lowest word)"""
    key = [states[-1][0]]
    for t in range(len(states) - 1, 0, -1):
        key += [1, states[t - 1][0]] if ent[t] else [0, states[t - 1][1]]
    return key


def check_against_enumeration(logAs, logb, p, want_unique):
    Ns = [a.shape[0] for a in logAs]
    word, path, begin, score, gap = CC.decode_log(logAs, logb, p)
    paths = enumerate_paths(logAs, logb, p)
    # a path scores only if it ends in the last state of its word
    ends = [x for x in paths if x[1][-1][1] == Ns[x[1][-1][0]] - 1]
    best = max(x[0] for x in ends)
    assert np.float64(score).tobytes() == np.float64(best).tobytes(), (score, best)
    top = [x for x in ends if x[0] == best]
    if want_unique is not None:     # (None: p = 0 ties a one-state word's stay with its own entry by construction)
        assert (len(top) == 1 and gap > 0) if want_unique else (len(top) > 1 and gap == 0)
    _, states, ent = min(top, key=lambda x: backward_key(x[1], x[2], Ns))
    assert [k for k, _ in states] == word.tolist()
    assert [j for _, j in states] == path.tolist()
    assert [int(e) for e in ent] == begin.tolist()


@pytest.mark.parametrize("p", [0.0, -1.5, 2.0, -INF])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_restatement_equals_the_enumeration_of_all_paths(T, p):
    """K = 2, N = (2, 1): random log b and transitions, no ties"""
    rng = np.random.default_rng(100 * T + 7)
    logAs = [CC.log_a(np.array([[0.6, 0.4], [0.0, 1.0]])), CC.log_a(np.ones((1, 1)))]
    for _ in range(6):
        logb = rng.normal(-3.0, 2.0, (T, 3))
        check_against_enumeration(logAs, logb, p, want_unique=True if p != 0.0 else None)


@pytest.mark.parametrize("T", [2, 3, 4, 5])
def test_restatement_follows_the_tie_rules(T):
    """integers throughout, so that every sum is exact: all log b equal, log a in {0, -inf}, p = 0.
    Many paths share the best score; the restatement's is the one the tie rules name"""
    logAs = [np.array([[0.0, 0.0], [-INF, 0.0]]), np.zeros((1, 1))]
    check_against_enumeration(logAs, np.full((T, 3), -2.0), 0.0, want_unique=False)


def test_pick_is_the_order():
    """k_vocab_best's sequential rule and the order `beats` name the same winner, NaN and ties included"""
    rng = np.random.default_rng(5)
    vals = [np.nan, -INF, -1.0, 0.0, 2.5]
    for _ in range(300):
        s = list(rng.choice(vals, size=int(rng.integers(1, 7))))
        best = 0
        for k in range(1, len(s)):
            if CC.beats(s[k], k, s[best], best):
                best = k
        assert best == CC.pick(s)[0], s
        assert all(CC.beats(s[best], best, s[k], k) for k in range(len(s)) if k != best), s


# ------------------------------------------------------------- the cases

@pytest.fixture(scope="module")
def cases(G):
    made = {}

    def get(name):
        if name not in made:
            case = CC.make(G, name)
            made[name] = (case, CC.oracle_log_b(case))
        return made[name]
    return get


@pytest.mark.parametrize("name", CC.ALL)
def test_shapes(cases, name):
    case, lb = cases(name)
    lens = sorted(int(T) for T in case.lens)
    if name == "narrow":
        assert case.Ns == [5, 16, 9] and case.P == 3 and lens == [0, 1, 2, 7, 8, 9, 17, 40, 40]
        assert set(case.spoken) >= {(0,), (1, 2), (2, 0, 1), (0, 0)}
    if name in ("mixed", "dup"):
        assert case.Ns == [3, 16, 17, 6 if name == "mixed" else 3] and case.P == 2
        assert np.any(np.tril(case.words[1][0].A, -1) != 0)         # word 1 is ergodic
    if name == "wide":
        assert case.Ns == [33, 64] and case.NS == 97 and 0 < min(T for T in lens if T) < 33
    if name == "many":
        assert case.K == 70 and set(case.Ns) == {3} and case.NS == 210 and case.P == 1
    if name == "ones":
        assert case.Ns == [1, 1, 1] and all(np.array_equal(w[0].A, [[1.0]]) for w in case.words)
    if name == "dup":
        for a, b in zip(case.words[0], case.words[3]):
            assert all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays()))
    if name == "full":
        assert sorted(len(s) for s in case.spoken) == [1, 2, 2]
    assert lb.shape == (case.F, case.NS) and np.isfinite(lb).all()


@pytest.mark.parametrize("name", CC.NONTIE)
def test_margins(cases, name):
    """every utterance of every non-tie case, under every penalty of the case, keeps more than GAP at every
    decision along its traced path"""
    case, lb = cases(name)
    for p in CC.penalties(name):
        word, path, begin, score, gap = CC.decode(case, lb, p)
        assert np.all(gap[case.lens > 0] > CC.GAP), (name, p, gap)
        assert np.all(score[case.lens == 0] == 0.0)
        if p == -INF:       # nothing enters
            off = np.concatenate([[0], np.cumsum(case.lens)])
            assert begin.sum() == (case.lens > 0).sum() and np.all(begin[off[:-1][case.lens > 0]] == 1)


def test_one_word_takes_each_utterance_under_a_prohibitive_penalty(cases):
    case, lb = cases("narrow")
    word, _, begin, score, _ = CC.decode(case, lb, -1e4)
    assert all(len(s) == 1 for s, T in zip(CC.strings(word, begin, case.lens), case.lens) if T)
    assert all(len(s) == 0 for s, T in zip(CC.strings(word, begin, case.lens), case.lens) if not T)


@pytest.mark.parametrize("name", CC.NONTIE)
def test_spoken_sequences_that_decode(cases, name):
    case, lb = cases(name)
    got = CC.qualifying(case)
    print(name, got)
    assert got == [(p, u) for p in (0.0, -5.0) for u in CC.QUALIFY[name][p]]
    composed = [u for _, u in got if len(case.spoken[u]) > 1]
    if name in ("narrow", "mixed", "full"):
        assert composed, "no composed utterance decodes to what was spoken"
