"""What test_connect_gpu.py leans on, checked where no GPU is needed: the two entry points are exported and
declared; connect_cases' restatement of the connected-word recursion is the definition (it equals an
enumeration of ALL composite paths on a tiny vocabulary, the score bit for bit, the path under the tie
rules); the cases, on the oracle's float64 log b, keep the margin under which a differing path cannot be
blamed on rounding; the composed utterances that decode to what was spoken are the recorded ones; the cases
beyond one composite state per thread reach what they are there for (word 23 on both sides of state 256,
word numbers above 255 through the pick and the trace, no word end in 10 frames at the cap); and holes'
reference log b holds NaN and -inf where its models ask for them, with the decoding the rules name.
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


def test_an_all_nan_pick_is_word_0_and_the_trace_starts_there():
    """the rules of include/ghmm.h where every word end of the last frame is NaN: the final pick is word 0
    (all NaN gives word 0), the score its NaN, and the trace starts in word 0's last state, whatever its
    score; with the ends NaN in every frame no pick ever enters and the utterance stays in word 0; and a
    word end of -inf beats the NaN ones"""
    logAs = [CC.log_a(np.array([[0.6, 0.4], [0.0, 1.0]])), CC.log_a(np.ones((1, 1))),
             CC.log_a(np.array([[0.5, 0.5], [0.0, 1.0]]))]
    rng = np.random.default_rng(11)
    logb = rng.normal(-3.0, 1.0, (4, 5))
    logb[3, [1, 2, 4]] = np.nan                 # the three ends, in the last frame alone
    for p in (0.0, -5.0, -INF):
        word, path, begin, score, gap = CC.decode_log(logAs, logb, p)
        assert np.isnan(score) and word[3] == 0 and path[3] == 1, p
    # ... and in every frame: nothing ever enters, word 0 is walked from its first state
    logb[:, [1, 2, 4]] = np.nan
    word, path, begin, score, gap = CC.decode_log(logAs, logb, 0.0)
    assert np.isnan(score) and word.tolist() == [0] * 4 and begin.tolist() == [1, 0, 0, 0] and path[3] == 1
    # -inf beats NaN: with word 1's end finite or -inf in the last frame, word 1 is picked
    for v in (-2.0, -INF):
        logb[3, 2] = v
        word, path, begin, score, gap = CC.decode_log(logAs, logb, -INF)
        assert word[3] == 1 and score == -INF


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


def dense_words(case):
    """the words with a transition off {j - 1, j}: the ones that take k_connect's dense step"""
    out = []
    for k, w in enumerate(case.words):
        i, j = np.indices(w[0].A.shape)
        if np.any((np.asarray(w[0].A) != 0) & (i != j) & (i != j - 1)):
            out.append(k)
    return out


@pytest.mark.parametrize("name", CC.ALL + CC.BEYOND + ("ones2048",))
def test_shapes(cases, name):
    case, lb = cases(name)
    lens = sorted(int(T) for T in case.lens)
    if name == "thick":
        assert case.K == 28 and case.Ns == [(7, 16, 9, 12)[k % 4] for k in range(28)] and case.NS == 308
        assert dense_words(case) == [1, 23] and case.bo[23] == 252 and case.bo[24] == 264     # straddles 256
        assert lens == [0, 3, 12, 34, 50, 56] and case.spoken[5] == (3,) and case.Ns[3] > 3
        assert sum(23 in s for s in case.spoken) == 3 and sorted(len(s) for s in case.spoken) == [0, 1, 1, 2, 3, 3]
        assert case.P == 1 and (case.words[0][0].M, case.words[0][0].D) == (2, 3)
    if name == "crowd":
        assert case.K == 300 and case.Ns == [(2, 3, 4)[k % 3] for k in range(300)] and case.NS == 900
        assert dense_words(case) == [] and case.P == 1 and (case.words[0][0].M, case.words[0][0].D) == (1, 2)
        assert lens[:2] == [0, 1] and len(lens) == 6
        for seq, seg in CC.UTTS[name][:4]:
            assert 3 <= len(seq) <= 4 and all(5 <= T <= 7 for T in seg)
        assert {299, 257, 256} <= {k for s in case.spoken for k in s}
        assert min(k for s in case.spoken for k in s) < 10
    if name == "cap":
        assert case.K == 32 and set(case.Ns) == {64} and case.NS == 2048 and dense_words(case) == [5]
        assert len({w[0].mean.tobytes() for w in case.words}) == 32       # 32 distinct words
        assert case.lens.tolist() == [155, 40, 64, 10, 0] and case.F < 300
        assert case.spoken[:3] == [(3, 17), (5,), (9,)]
        assert case.P == 1 and (case.words[0][0].M, case.words[0][0].D) == (1, 3)
        assert 2048 * 36 + 96 == 73824 > 48 * 1024                          # k_connect's LDS at the cap
    if name == "ones2048":
        assert case.K == case.NS == 2048 and set(case.Ns) == {1}
        assert all(case.words[k] is case.words[k % 5] for k in range(2048))
        assert len({id(w) for w in case.words}) == 5 and len({w[0].mean.tobytes() for w in case.words[:5]}) == 5
        assert all(np.array_equal(w[0].A, [[1.0]]) for w in case.words[:5])
        assert lens == [0, 3, 5, 8]
        for a in range(5):          # the copies' columns of the oracle's log b are one column
            assert np.all(lb[:, a::5] == lb[:, a:a + 1])
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


@pytest.mark.parametrize("name", CC.NONTIE + CC.BEYOND)
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


@pytest.mark.parametrize("name", CC.NONTIE + CC.BEYOND)
def test_spoken_sequences_that_decode(cases, name):
    case, lb = cases(name)
    got = CC.qualifying(case)
    print(name, got)
    assert got == [(p, u) for p in (0.0, -5.0) for u in CC.QUALIFY[name][p]]
    composed = [u for _, u in got if len(case.spoken[u]) > 1]
    if name in ("narrow", "mixed", "full"):
        assert composed, "no composed utterance decodes to what was spoken"


# ------------------------------------------------------------- more than one composite state per thread

def test_thick_walks_word_23_on_both_sides_of_state_256(cases):
    """some decoded path passes through word 23's composite states below 256 and at or above it: the states
    of a thread's first and second pass"""
    case, lb = cases("thick")
    seen = set()
    for p in CC.penalties("thick"):
        word, path, begin, _, _ = CC.decode(case, lb, p)
        seen |= set((case.bo[word] + path)[word == 23].tolist())
    print(sorted(seen))
    assert min(seen) >= 252 and max(seen) <= 263 and any(s < 256 for s in seen) and any(s >= 256 for s in seen)
    # ... and the pick at p = 0 takes word ends from both passes
    word, _, begin, _, _ = CC.decode(case, lb, 0.0)
    ends = {int(case.bo[k + 1] - 1) for s in CC.strings(word, begin, case.lens) for k in s}
    assert any(s < 256 for s in ends) and any(s >= 256 for s in ends)


def test_crowd_decodes_words_beyond_one_byte(cases):
    """at p = 0 a word >= 256 is decoded on a frame that continues it (the number went through the trace),
    and a word is entered from the pick of a word >= 256 (the number went through word[t - 1])"""
    case, lb = cases("crowd")
    word, path, begin, score, _ = CC.decode(case, lb, 0.0)
    first = np.zeros(case.F, dtype=bool)
    first[np.concatenate([[0], np.cumsum(case.lens)])[:-1][case.lens > 0]] = True
    assert np.any((word >= 256) & (begin == 0))
    entered = np.nonzero((begin == 1) & ~first)[0]
    assert np.any(word[entered - 1] >= 256)
    assert score[case.lens == 1] == -INF      # (no one-state words: one frame reaches no word end)


def test_cap_reaches_no_word_end_in_10_frames_and_has_one_path_in_64(cases):
    case, lb = cases("cap")
    for p in CC.penalties("cap"):
        word, path, begin, score, gap = CC.decode(case, lb, p)
        off = np.concatenate([[0], np.cumsum(case.lens)])
        assert score[3] == -INF and np.all(word[off[3]:off[4]] == 0) and begin[off[3]:off[4]].sum() == 1
        assert np.array_equal(path[off[2]:off[3]], np.arange(64)) and word[off[2]] == word[off[3] - 1]
        assert np.isfinite(score[:3]).all()


# ------------------------------------------------------------- log b that is not finite

def test_holes(cases):
    case, lb = cases("holes")
    assert case.K == 20 and case.Ns == [(8, 16, 24)[k % 3] for k in range(20)] and case.NS == 312 and case.P == 1
    assert (case.words[0][0].M, case.words[0][0].D) == (2, 4)
    assert dense_words(case) == [CC.HOLES_DENSE] and case.words[CC.HOLES_DENSE][0].A[0, -1] == 0.0
    nan, inf = CC.holes_pattern(case, lb)
    assert nan == [7, 112, 151, 311] and inf == [58, 202]
    assert nan[0] // 64 != nan[2] // 64 and nan[3] >= 256           # other waves, a thread's second slot
    assert case.lens.tolist() == [50, 60, 12, 2, 0] and case.spoken[2] == (0,)
    assert not set(k for s in case.spoken[:2] for k in s) & set(CC.HOLES_UNHEALTHY)
    for p in CC.penalties("holes"):
        word, path, begin, score, gap = CC.decode(case, lb, p)
        print(p, score, gap, CC.strings(word, begin, case.lens))
        assert np.isfinite(score[:3]).all() and score[3] == -INF and score[4] == 0.0
        assert np.all(gap[:3] > CC.GAP)
        fin = np.repeat(np.isfinite(score), case.lens)
        assert not np.isin(word[fin], CC.HOLES_NAN_END).any()
        assert not np.isin(word, CC.HOLES_INF).any()                # (never passed: they cannot end)
        off = np.concatenate([[0], np.cumsum(case.lens)])
        # two frames: every healthy end is -inf, and -inf beats word 0's NaN: the lowest word whose end is -inf
        assert word[off[3]:off[4]].tolist() == [1, 1] and begin[off[3]:off[4]].tolist() == [1, 0]
