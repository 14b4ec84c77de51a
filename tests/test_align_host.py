"""What test_align_gpu.py leans on, checked where no GPU is needed: the two entry points are exported and
declared; align_cases' restatement of the forced alignment is the definition (it equals an enumeration of
ALL alignments on tiny inputs, the score bit for bit, the path under the tie rules); on the strings that
connect_cases' decoder finds at penalty 0 it gives that decoder's score, and never more on any other
transcript; the cases, on the oracle's float64 log b, keep the margin under which a differing path cannot
be blamed on rounding; and cut_segments cuts a corpus where word_segments says.
The margins are conditions on the inputs, not measurements: if a seed fails them, the seed changes, not
the bound."""
import os

import numpy as np
import pytest

import align_cases as AC
import connect_cases as CC
from fullcov_support import offsets
from oracle_lib import ROOT

INF = np.inf


def test_entry_points_are_exported_and_declared(G):
    lib = G.hip_lib()
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    for name, face in (("ghmm_align_streams", "align_streams"), ("ghmm_align_full_streams", "align_full_streams")):
        assert hasattr(lib, name), name
        assert name in G.SYMBOLS, name
        assert f"int {name}(ghmm_ctx" in hdr, name
        assert callable(getattr(G.Context, face)), face
    assert callable(G.cut_segments)


# ------------------------------------------------------------- the restatement is the definition

def enumerate_alignments(logAs, cols, logb, transcript):
    """every path of T frames through the transcript's composite states as [(instance, state, entered)]
    with its score, the sums taken in the lattice's order: (d + log a, or d itself on an entry) + log b, left
    to right.  A path starts in state 0 of instance 0; instance i is entered from the last state of
    instance i - 1 only; a path counts if it ends in the last state of the last instance."""
    Ns = [logAs[k].shape[0] for k in transcript]
    T, L = len(logb), len(transcript)
    out = []

    def walk(t, i, j, d, states):
        if t == T:
            if i == L - 1 and j == Ns[i] - 1:
                out.append((d, tuple(states)))
            return
        k = transcript[i]
        for j2 in range(Ns[i]):
            if logAs[k][j, j2] != -INF:
                walk(t + 1, i, j2, (d + logAs[k][j, j2]) + logb[t, cols[k] + j2], states + [(i, j2, False)])
        if j == Ns[i] - 1 and i + 1 < L:
            walk(t + 1, i + 1, 0, d + logb[t, cols[transcript[i + 1]]], states + [(i + 1, 0, True)])

    walk(1, 0, 0, 0.0 + logb[0, cols[transcript[0]]], [(0, 0, True)])
    return out


def backward_key(states):
    """the tie rules as an order on paths of equal score, decided from the last frame backwards as the
    trace does: at every frame staying in the word (the lowest predecessor) ahead of entering"""
    key = []
    for t in range(len(states) - 1, 0, -1):
        key += [1, 0] if states[t][2] else [0, states[t - 1][1]]
    return key


def check_against_enumeration(logAs, cols, logb, transcript, want_unique):
    word, path, begin, score, gap = AC.align_log(logAs, cols, logb, transcript)
    paths = enumerate_alignments(logAs, cols, logb, transcript)
    if not paths:
        assert score == -INF
        return
    best = max(x[0] for x in paths)
    assert np.float64(score).tobytes() == np.float64(best).tobytes(), (score, best)
    top = [x for x in paths if x[0] == best]
    if want_unique is not None:     # (None: a one-state word with a = 1 twice in a row ties stay and entry by construction)
        assert (len(top) == 1 and gap > 0) if want_unique else (len(top) > 1 and gap == 0)
    _, states = min(top, key=lambda x: backward_key(x[1]))
    assert [transcript[i] for i, _, _ in states] == word.tolist()
    assert [j for _, j, _ in states] == path.tolist()
    assert [int(e) for _, _, e in states] == begin.tolist()


TINY_A = [np.array([[0.6, 0.4], [0.0, 1.0]]), np.ones((1, 1)),
          np.array([[0.5, 0.3, 0.2], [0.2, 0.5, 0.3], [0.1, 0.0, 0.9]])]        # the last one ergodic
TINY_COLS = [0, 2, 3]


@pytest.mark.parametrize("transcript", [(0,), (1,), (2,), (0, 1), (1, 1), (2, 0), (0, 2, 1), (1, 2, 2), (0, 0, 0),
                                        (2, 2, 2)])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_restatement_equals_the_enumeration_of_all_alignments(T, transcript):
    """at most 3 instances of at most 3 states, T at most 7: random log b, no ties; where the transcript
    needs more frames than T there is no alignment and the score is -inf"""
    rng = np.random.default_rng(100 * T + 7 + len(transcript))
    logAs = [CC.log_a(A) for A in TINY_A]
    for _ in range(4):
        logb = rng.normal(-3.0, 2.0, (T, 6))
        check_against_enumeration(logAs, TINY_COLS, logb, transcript,
                                  want_unique=None if (1, 1) in zip(transcript, transcript[1:]) and T > 2 else True)


@pytest.mark.parametrize("T", [5, 6, 7])
def test_restatement_follows_the_tie_rules(T):
    """integers throughout, so that every sum is exact: all log b equal, log a in {0, -inf}.  Many alignments
    share the best score; the restatement's is the one the tie rules name: stay ahead of enter, the
    lowest predecessor"""
    logAs = [np.array([[0.0, 0.0], [-INF, 0.0]]), np.zeros((1, 1))]
    check_against_enumeration(logAs, [0, 2], np.full((T, 3), -2.0), (0, 1), want_unique=False)
    check_against_enumeration(logAs, [0, 2], np.full((T, 3), -2.0), (1, 0, 1), want_unique=False)


def test_no_frames_and_too_few():
    logAs = [CC.log_a(A) for A in TINY_A]
    word, path, begin, score, gap = AC.align_log(logAs, TINY_COLS, np.zeros((0, 6)), (0, 2))
    assert len(word) == len(path) == len(begin) == 0 and score == 0.0 and not np.signbit(score)
    assert AC.align_log(logAs, TINY_COLS, np.zeros((0, 6)), ())[3] == 0.0
    # the first word's two states need two frames, the second word one more
    assert AC.align_log(logAs, TINY_COLS, np.full((2, 6), -1.0), (0, 1))[3] == -INF
    assert np.isfinite(AC.align_log(logAs, TINY_COLS, np.full((3, 6), -1.0), (0, 1))[3])


# ------------------------------------------------------------- the cases

@pytest.fixture(scope="module")
def cases(G):
    made = {}

    def get(name):
        if name not in made:
            case = AC.make(G, name)
            made[name] = (case, AC.oracle_log_b(case))
        return made[name]
    return get


@pytest.mark.parametrize("name", AC.ALL)
def test_shapes(cases, name):
    case, lb = cases(name)
    S = [AC.states_of(case, tr) for tr in case.transcripts]
    assert len(case.transcripts) == case.U and lb.shape == (case.F, case.NS) and np.isfinite(lb).all()
    assert all((len(tr) == 0) == (T == 0) for tr, T in zip(case.transcripts, case.lens))
    if name == "narrow":
        assert sorted(set(len(tr) for tr in case.transcripts)) == [0, 1, 2, 3] and len(set(S)) >= 5
        assert (0, 0) in case.transcripts and (2, 0, 1) in case.transcripts
        assert np.any(np.tril(case.words[1][0].A, -1) != 0)         # word 1, mid-transcript, is ergodic
    if name == "wide":
        assert case.transcripts[-1] == (1, 0, 1) and S[-1] == 161 and case.lens[-1] == 250
    if name == "many":
        assert len(case.transcripts[-1]) == 20 and 80 <= case.lens[-1] <= 100
    if name == "ones":
        assert case.Ns == [1, 1, 1] and any(T == 1 and len(tr) == 1 for tr, T in zip(case.transcripts, case.lens))
    if name == "cap":
        assert case.U == 1 and len(case.transcripts[0]) == 682 and S == [2046] and case.lens[0] == 2200
        assert 2046 * 40 > 48 * 1024 and 2046 + 3 > AC.MAX_S
    if name == "cap-mixed":
        assert S == [6, 0, 2046, 3, 60] and case.lens.tolist() == [11, 0, 2200, 7, 90]
        assert case.transcripts[1] == () and AC.CAP_MIXED_LONG == 2
        assert case.transcripts[2] == tuple((11 * i + 5) % 70 for i in range(682))
        assert case.lens[0] * S[0] + case.lens[2] * S[2] > 4.5e6        # where the last two's back-pointers begin
    if name == "thick":
        assert case.transcripts[:6] == [seq if sum(seg) else () for seq, seg in CC.UTTS["thick"]]
        assert case.transcripts[-1] == (1, 23) * 10 and S[-1] == 280 and case.lens[-1] == 110
        # instance 18 (word 1) owns the composite states 252 .. 267: it straddles 256; both words are dense
        assert sum(case.Ns[k] for k in case.transcripts[-1][:18]) == 252 and case.Ns[1] == 16
        for k in (1, 23):
            assert np.any(np.tril(case.words[k][0].A, -1) != 0)
    assert max(S) <= AC.MAX_S


@pytest.mark.parametrize("name", AC.ALL)
def test_margins(cases, name):
    """every case's utterances keep more than GAP at every decision along the traced path, but for at
    most MAX_BELOW_GAP of them; an utterance of no frames scores 0"""
    case, lb = cases(name)
    word, path, begin, score, gap = AC.align(case, lb)
    print(name, "gaps", gap, "scores", score)
    assert np.sum(gap[case.lens > 0] <= AC.GAP) <= AC.MAX_BELOW_GAP, (name, gap)
    assert np.all(score[case.lens == 0] == 0.0)
    off = offsets(case.lens)
    assert np.all(begin[off[:-1][case.lens > 0]] == 1)
    fin = np.isfinite(score)
    assert [int(begin[off[u]:off[u + 1]].sum()) for u in np.nonzero(fin)[0]] == \
        [len(case.transcripts[u]) for u in np.nonzero(fin)[0]]
    if name == "short":
        assert np.array_equal(np.isfinite(score), [True, False, False, False, False, False, False, True, True])
    elif name == "narrow":
        assert np.array_equal(np.isfinite(score), ~np.isin(case.lens, (1, 2)))
    S = np.array([AC.states_of(case, tr) for tr in case.transcripts])
    assert np.all(fin[case.lens >= S]) and fin[-1]      # (fewer frames than states: -inf unless a word skips states)


@pytest.mark.parametrize("name", ["narrow", "mixed", "wide", "many", "ones", "full"])
def test_connect_s_strings_give_connect_s_score_and_no_transcript_gives_more(cases, name):
    """consequences (b) and (c) of include/ghmm.h between the two restatements, on the oracle's log b"""
    case, lb = cases(name)
    cw, cp, cb, cs, cgap = CC.decode(case, lb, 0.0)
    strings = CC.strings(cw, cb, case.lens)
    aw, ap, ab, score, gap = AC.align(case, lb, strings)
    assert np.array_equal(score, cs), (score, cs)
    unique = np.repeat((cgap > 0) & (gap > 0), case.lens)
    assert unique.any()
    for a, c in ((aw, cw), (ap, cp), (ab, cb)):
        assert np.array_equal(a[unique], c[unique])
    rng = np.random.default_rng(9)
    others = [case.transcripts,
              [tuple(int(k) for k in rng.integers(0, case.K, 1 + u % 3)) if T else () for u, T in enumerate(case.lens)],
              [tuple(reversed(s)) for s in strings], [s + s[:1] for s in strings]]
    for trs in others:
        assert np.all(AC.align(case, lb, trs)[3] <= cs), trs


# ------------------------------------------------------------- cut_segments

def test_cut_segments():
    from _load import ghmm
    G = ghmm()
    lens = [6, 0, 1, 3]
    word = np.array([5, 5, 5, 5, 2, 2, 7, 3, 3, 3], dtype=np.int32)
    begin = np.array([1, 0, 1, 0, 1, 0, 1, 1, 0, 0], dtype=np.int32)
    seg = G.word_segments(word, begin, lens)
    X0 = np.arange(10, dtype=np.float64)[:, None] * np.ones((1, 2))
    X1 = 100.0 + np.arange(10, dtype=np.float64)[:, None] * np.ones((1, 3))
    cut = G.cut_segments([X0, X1], lens, seg, 8)
    assert len(cut) == 8
    want = {5: ([0, 1, 2, 3], [2, 2]), 2: ([4, 5], [2]), 7: ([6], [1]), 3: ([7, 8, 9], [3])}
    for k, (Xs_k, lens_k) in enumerate(cut):
        frames, ls = want.get(k, ([], []))
        assert lens_k.dtype == np.int32 and lens_k.tolist() == ls, k
        assert Xs_k[0].shape == (len(frames), 2) and Xs_k[1].shape == (len(frames), 3), k
        assert Xs_k[0][:, 0].tolist() == [float(f) for f in frames], k
        assert Xs_k[1][:, 2].tolist() == [100.0 + f for f in frames], k
    # an utterance without segments gives nothing; a score that is not finite leaves its utterance out
    none = G.cut_segments([X0, X1], lens, [[], [], [], []], 8)
    assert all(len(l) == 0 and all(len(x) == 0 for x in xs) for xs, l in none)
    part = G.cut_segments([X0, X1], lens, seg, 8, score=[-INF, 0.0, -3.0, np.nan])
    assert [k for k, (_, l) in enumerate(part) if len(l)] == [7] and part[7][0][0][:, 0].tolist() == [6.0]
    with pytest.raises(ValueError):
        G.cut_segments([X0], lens, [[(9, 0, 1)], [], [], []], 8)


# ------------------------------------------------------------- log b that is not finite

def test_holes_transcripts_score_as_they_are_named(G):
    """connect_cases' holes on the reference's log b: a transcript that ends in a NaN word end scores NaN;
    one with such a word in the middle -inf (the NaN entry candidate never enters); one through a word with
    a column of -inf scores -inf; the spoken ones are finite above the margin, and consequences (b) and
    (c) hold against the decoder at penalty 0 where its score is finite"""
    case = AC.make(G, "holes")
    lb = AC.oracle_log_b(case)
    kinds = {"finite": np.isfinite, "nan": np.isnan, "-inf": lambda x: x == -INF, "0": lambda x: x == 0.0}
    assert set(AC.HOLES) == {"spoken", "ends-in-nan", "nan-in-the-middle", "through-minus-inf"}
    assert AC.HOLES["spoken"][0] == case.transcripts
    for name, (trs, want) in AC.HOLES.items():
        word, path, begin, score, gap = AC.align(case, lb, trs)
        print(name, score, gap)
        assert all(kinds[k](x) for k, x in zip(want, score)), (name, score)
        assert np.all(gap[case.lens > 0] > AC.GAP), (name, gap)
    trs = AC.HOLES["ends-in-nan"][0]
    assert trs[0][-1] == 9 and trs[1][-1] == 19 and AC.HOLES["nan-in-the-middle"][0][0][1] == 9
    assert AC.HOLES["nan-in-the-middle"][0][1][1] == 0
    assert all(set(t) & set(CC.HOLES_INF) for t in AC.HOLES["through-minus-inf"][0][:2])
    # long enough but for the non-finite columns: more frames than states
    for name in ("nan-in-the-middle", "through-minus-inf"):
        assert all(AC.states_of(case, t) <= T for t, T in list(zip(AC.HOLES[name][0], case.lens))[:2])
    cw, cp, cb, cs, cgap = CC.decode(case, lb, 0.0)
    fin = np.isfinite(cs) & (case.lens > 0)
    assert fin[:3].all()
    strings = CC.strings(cw, cb, case.lens)
    score = AC.align(case, lb, strings)[3]
    assert np.array_equal(score[fin], cs[fin])
    spoken = AC.align(case, lb)[3]
    assert np.all(~(spoken[fin] > cs[fin]))
