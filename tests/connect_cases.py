"""The cases of the connected-word decoder (ghmm_connect_streams, ghmm_connect_full_streams; k_connect) and a
float64 numpy restatement of its definition in include/ghmm.h.  Shared by test_connect_host.py, which
checks on the CPU that the restatement is the definition (against an enumeration of all composite paths)
and that the cases keep the margin under which a differing path cannot be blamed on rounding, and by
test_connect_gpu.py.  Plain numpy and the oracle, no GPU, no tests.

An utterance is the concatenation of fullstreams_ref.stream_frames walks through a stated word sequence,
one walk of a stated length per word.  The smallest shapes at which the kernel can go wrong:
  narrow  vocab_cases' narrow words: K = 3, N = (5, 16, 9), P = 3, word 1 ergodic.  NS = 30: one wave.
          Spoken (0), (1, 2), (2, 0, 1), (0, 0); lengths 0, 1, 2, 7, 8, 9, 17, 40, 40.
  mixed   vocab_cases' mixed words: K = 4, N = (3, 16, 17, 6), P = 2, word 1 ergodic, Nmax = 17.
  wide    vocab_cases' wide words: N = (33, 64), NS = 97: two waves, a word that straddles them, the
          dense step on word 0's columns.  One utterance of 5 frames, shorter than either word: no word
          end is reached, every pick is over -inf alone.
  many    K = 70 words of 3 states, P = 1, (M, D) = (1, 2).  NS = 210: four waves, the pick spans all.
  ones    three one-state words with A = [[1]]: a word is both its own entry and its own end.
  dup     mixed with word 3 a copy of word 0: every pick and every entry between the two takes word 0
          (GHMM_OPT_KERNELS = 1 only, where equal Gaussians give equal bits).
  full    fullvocab_cases' narrow words (its smallest vocabulary: NS = 30), two composed utterances and
          one single word.
Past one composite state per thread (k_connect runs 256 threads), one stream and small (M, D) each:
  thick   K = 28, N = (7, 16, 9, 12)[k % 4], (M, D) = (2, 3).  NS = 308: threads 0..51 own two states, five
          of them a word end in their second pass (none two ends: that is crowd's and cap's).  Words 1
          and 23 are ergodic; word 23 owns the composite states 252..263: its dense step reads the
          previous row on both sides of s = 256.  One utterance of 3 frames, shorter than its word.
  crowd   K = 300, N = (2, 3, 4)[k % 3], banded, (M, D) = (1, 2).  NS = 900: word numbers beyond one byte
          and beyond the thread count.  (No one-state words: with A = [[1]] and p = 0 stay and entry tie.)
  cap     32 words of 64 states, (M, D) = (1, 3).  NS = 2048, the cap: more than 48 KB of LDS, eight states
          and up to eight word ends per thread.  Word 5 has columns off the band (vocab_cases._limited).
          One word on exactly 64 frames (a single path); one utterance of 10 frames reaches no word end:
          every pick is over -inf alone, across four waves, and gives word 0.
  ones2048  K = 2048 one-state words with A = [[1]]: word k is the k % 5-th of five models, the SAME host
          object (a device builds five models and repeats their handles).  Every thread owns eight word
          ends; under GHMM_OPT_KERNELS = 1 the copies' columns are equal bits and every pick an exact
          tie of 409 or 410.  Few frames: the restatement walks 2048 words per frame.
  holes   full-covariance, (M, D) = (2, 4), K = 20, N = (8, 16, 24)[k % 3], NS = 312, with non-finite
          log b: det = 0 in every mixture of the LAST state of words 0, 9 and 19 (their word ends are NaN
          in every frame); c = 0 in state 2 of the banded words 4 and 13 (a column of -inf: they are never
          passed); word 7 ergodic (state 0 does not reach its last state in one step) with det = 0 in
          state 8: its dense step meets NaN candidates.  One utterance speaks word 0; one has 2 frames:
          every healthy end is still -inf, and -inf beats NaN.
A vocabulary for embed_cases alone (no decoder test walks it: 90 words per frame are the restatement's cost):
  broad   K = 90 words of 3 states, banded, (M, D) = (1, 2).  NS = 270: word 85 owns the columns 255..257,
          words 86..89 lie past 256.  Word 87 spoken twice in one utterance, word 89 (column NS - 1), a
          21-word utterance (S = 63: one wave), T = 0 and two frames for three states; word 88 and most of
          the words below 85 are spoken nowhere.
  broad256  K = 350 such words, NS = 1050, and one utterance of 65 words (S = 195: 256 threads).
Penalties: 0 and -5 on every case, -inf on every case, +3 and -1e4 on narrow."""
import numpy as np

import fullvocab_cases as FV
import vocab_cases as V
from fullcov_support import offsets
from fullstreams_ref import stream_frames

ENTRY = -1          # psi of a first state entered from the previous frame's pick
GAP = V.GAP

#        name: (where the words come from, [(spoken words, frames per word)], seed)
UTTS = {
    "narrow": [((0,), (0,)), ((0,), (1,)), ((0,), (2,)), ((0,), (7,)), ((0,), (8,)), ((2,), (9,)),
               ((0, 0), (8, 9)), ((1, 2), (22, 18)), ((2, 0, 1), (12, 8, 20))],
    "mixed": [((0, 3), (6, 10)), ((2, 1), (20, 20)), ((3,), (5,)), ((1, 0, 3), (18, 5, 9)), ((0,), (0,))],
    "wide": [((1, 0), (70, 40)), ((0,), (5,)), ((0, 1), (36, 66)), ((0,), (0,))],
    "many": [((5, 69, 33), (4, 5, 4)), ((64,), (6,)), ((0, 65), (3, 3)), ((17,), (1,))],
    "ones": [((0, 1, 2, 1), (3, 3, 3, 3)), ((2,), (1,)), ((0,), (0,))],
    "full": [((0, 2), (8, 12)), ((2, 0), (14, 9)), ((1,), (20,))],
    "thick": [((5, 23), (14, 20)), ((23, 1, 10), (18, 24, 14)), ((2, 23, 27), (14, 18, 18)), ((12,), (12,)),
              ((0,), (0,)), ((3,), (3,))],
    "crowd": [((299, 3, 257), (6, 5, 7)), ((256, 150, 299, 12), (5, 6, 7, 5)), ((7, 257, 128, 256), (6, 7, 5, 6)),
              ((280, 1, 290), (5, 6, 7)), ((40,), (1,)), ((0,), (0,))],
    "cap": [((3, 17), (80, 75)), ((5,), (40,)), ((9,), (64,)), ((20,), (10,)), ((0,), (0,))],
    "ones2048": [((0, 1, 2, 3), (2, 2, 2, 2)), ((3, 4), (3, 2)), ((4,), (3,)), ((0,), (0,))],
    "broad": [((87, 2, 87, 85), (5, 4, 5, 5)), ((89, 40, 86), (4, 5, 4)),
              (tuple((4 * i + 1) % 84 for i in range(21)), (4,) * 21), ((0,), (0,)), ((89,), (2,))],
    "broad256": [((343, 2, 343, 341), (5, 4, 5, 5)), ((349, 40, 342), (4, 5, 4)),
                 (tuple((5 * i + 1) % 340 for i in range(65)), (4, 3) * 32 + (4,)), ((0,), (0,))],
    "holes": [((2, 5), (30, 20)), ((11, 3, 16), (28, 12, 20)), ((0,), (12,)), ((1,), (2,)), ((0,), (0,))],
}
UTTS["dup"] = UTTS["mixed"]
SEEDS = {"narrow": 611, "mixed": 612, "wide": 613, "many": 614, "ones": 615, "dup": 612, "full": 616,
         "thick": 811, "crowd": 812, "cap": 813, "ones2048": 815, "holes": 816, "broad": 817,
         "broad256": 818}
DIAGONAL = ("narrow", "mixed", "wide", "many", "ones", "dup")
NONTIE = ("narrow", "mixed", "wide", "many", "full")      # compared with the restatement on both tiers
ALL = DIAGONAL + ("full",)
# more than one composite state per thread: compared with the restatement on both tiers, as NONTIE
BEYOND = ("thick", "crowd", "cap")
FULLCOV = ("full", "holes")                                # the cases of full-covariance words
THICK_NS, CROWD_NS, CAP_WORDS, ONES_MODELS = (7, 16, 9, 12), (2, 3, 4), 32, 5
BROAD_WORDS = {"broad": 90, "broad256": 350}
HOLES_NS = (8, 16, 24)
HOLES_NAN_END, HOLES_INF, HOLES_DENSE, HOLES_DENSE_NAN = (0, 9, 19), (4, 13), 7, 8
HOLES_UNHEALTHY = HOLES_NAN_END + HOLES_INF + (HOLES_DENSE,)


def penalties(name):
    return (0.0, -5.0, -np.inf) + ((3.0, -1e4) if name == "narrow" else ())


def _words(G, name, rng):
    if name in ("narrow", "mixed", "wide"):
        return V.make(G, name).words
    if name == "dup":
        words = V.make(G, "mixed").words
        words[3] = [h.copy() for h in words[0]]
        return words
    if name == "full":
        return FV.make(G, "narrow").words
    if name == "many" or name in BROAD_WORDS:
        from fullcov_support import banded
        return [[V.rand_model(G, rng, 3, 1, 2, banded(rng, 3), word=f"w{k}")] for k in range(BROAD_WORDS.get(name, 70))]
    if name in BEYOND + ("ones2048", "holes"):
        return _beyond(G, name, rng)
    return [[V.rand_model(G, rng, 1, 2, 3, np.ones((1, 1)), word=f"w{k}")] for k in range(3)]       # ones


def _beyond(G, name, rng):
    from fullcov_support import banded, ergodic, rand_fmodel
    if name == "thick":
        return [[V.rand_model(G, rng, N, 2, 3, ergodic(rng, N) if k in (1, 23) else banded(rng, N), word=f"w{k}")]
                for k, N in ((k, THICK_NS[k % 4]) for k in range(28))]
    if name == "crowd":
        return [[V.rand_model(G, rng, CROWD_NS[k % 3], 1, 2, banded(rng, CROWD_NS[k % 3]), word=f"w{k}")]
                for k in range(300)]
    if name == "cap":
        return [[V.rand_model(G, rng, 64, 1, 3, V._limited(rng, 64) if k == 5 else banded(rng, 64), word=f"w{k}")]
                for k in range(CAP_WORDS)]
    if name == "ones2048":
        five = [[V.rand_model(G, rng, 1, 2, 3, np.ones((1, 1)), word=f"w{k}")] for k in range(ONES_MODELS)]
        return [five[k % ONES_MODELS] for k in range(2048)]
    words = []                                                                                  # holes
    for k in range(20):
        N = HOLES_NS[k % 3]
        A = None
        if k == HOLES_DENSE:
            A = ergodic(rng, N)
            A[0, N - 1] = 0.0
            A /= A.sum(1, keepdims=True)
        h = rand_fmodel(G, rng, N, 2, 4, A, spread=1.0, asym=False, word=f"w{k}")
        if k in HOLES_NAN_END:
            h.det[N - 1, :] = 0.0
        if k in HOLES_INF:
            h.c[2, :] = 0.0
        if k == HOLES_DENSE:
            h.det[HOLES_DENSE_NAN, :] = 0.0
        words.append([h])
    return words


def make(G, name):
    """vocab_cases.Case (full: fullvocab_cases.Case) with .spoken[u] = the word sequence of utterance u
    (empty for T = 0) and .name"""
    rng = np.random.default_rng(SEEDS[name])
    words = _words(G, name, rng)
    P = len(words[0])
    parts, lens, spoken = [[] for _ in range(P)], [], []
    for seq, seg in UTTS[name]:
        for k, T in zip(seq, seg):
            x = stream_frames(rng, words[k], [int(T)])
            for p in range(P):
                parts[p].append(x[p])
        lens.append(int(sum(seg)))
        spoken.append(tuple(seq) if sum(seg) else ())
    Xs = [np.concatenate(x) for x in parts]
    case = (FV.Case if name in FULLCOV else V.Case)(words, Xs, lens)
    case.spoken, case.name = spoken, name
    return case


# ------------------------------------------------------------- the definition in float64

def log_a(A):
    with np.errstate(divide="ignore"):
        return np.where(A > 0, np.log(np.where(A > 0, A, 1.0)), -np.inf)


def beats(av, ak, bv, bk):
    """the order of include/ghmm.h: a beats b"""
    if av > bv or (np.isnan(bv) and not np.isnan(av)):
        return True
    if bv > av or (np.isnan(av) and not np.isnan(bv)):
        return False
    return ak < bk


def pick(s):
    """(winner, gap) of a score list under k_vocab_best's rule; gap = winner - best of the others where
    both are finite, else inf"""
    best = 0
    for k in range(1, len(s)):
        if s[k] > s[best] or (np.isnan(s[best]) and not np.isnan(s[k])):
            best = k
    rest = [v for k, v in enumerate(s) if k != best and np.isfinite(v)]
    gap = s[best] - max(rest) if rest and np.isfinite(s[best]) else np.inf
    return best, gap


def _margin(win, other):
    return win - other if np.isfinite(win) and np.isfinite(other) else np.inf


def decode_log(logAs, logb, p):
    """One utterance: the recursion and the trace of include/ghmm.h on logb[T][NS] (word k's columns in
    order) and the words' log A, penalty p.  Returns (word[T], path[T], begin[T], score, gap): gap = the
    smallest difference, along the traced path, between the winning candidate and the runner-up at every
    decision (the predecessor within the word, entry against stay, every pick the trace uses, the final
    pick); inf where there is no finite runner-up."""
    Ns = [a.shape[0] for a in logAs]
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    K, T = len(Ns), len(logb)
    if T == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, z.copy(), z.copy(), 0.0, np.inf
    with np.errstate(all="ignore"):
        d = [np.where(np.arange(N) == 0, 0.0, -np.inf) + logb[0, bo[k]:bo[k] + N] for k, N in enumerate(Ns)]
        psi = [[np.zeros(N, dtype=int) for N in Ns]]
        gin = [[np.full(N, np.inf) for N in Ns]]        # the predecessor within the word
        gent = [np.full(K, np.inf)]                     # entry against stay
        w, gpick = np.zeros(T, dtype=int), np.full(T, np.inf)
        for t in range(1, T):
            w[t - 1], gpick[t - 1] = pick([d[k][-1] for k in range(K)])
            x = d[w[t - 1]][-1] + p
            nd, npsi, ngin, ngent = [], [], [], np.full(K, np.inf)
            for k, N in enumerate(Ns):
                cand = d[k][:, None] + logAs[k]                      # [i][j]
                cand = np.where(np.isnan(cand), -np.inf, cand)       # a NaN never wins a strict >
                arg = np.argmax(cand, axis=0)                        # the first maximum; 0 where all are -inf
                top = np.sort(cand, axis=0)[::-1]
                best = top[0].copy()
                g = np.full(N, np.inf)
                if N > 1:
                    g = np.where(np.isfinite(top[0]) & np.isfinite(top[1]), top[0] - top[1], np.inf)
                if x > best[0]:
                    ngent[k] = _margin(x, best[0])
                    best[0], arg[0] = x, ENTRY
                else:
                    ngent[k] = _margin(best[0], x)
                nd.append(best + logb[t, bo[k]:bo[k] + N])
                npsi.append(arg)
                ngin.append(g)
            d = nd
            psi.append(npsi)
            gin.append(ngin)
            gent.append(ngent)
        w[T - 1], gpick[T - 1] = pick([d[k][-1] for k in range(K)])
    k = int(w[T - 1])
    score, gap = d[k][-1], gpick[T - 1]
    s = Ns[k] - 1
    word, path, begin = (np.zeros(T, dtype=np.int32) for _ in range(3))
    for t in range(T - 1, -1, -1):
        word[t], path[t] = k, s
        if t == 0:
            begin[t] = 1
            break
        bp = psi[t][k][s]
        if s == 0:
            gap = min(gap, gent[t][k])
        if bp == ENTRY:
            begin[t] = 1
            gap = min(gap, gpick[t - 1])
            k = int(w[t - 1])
            s = Ns[k] - 1
        else:
            gap = min(gap, gin[t][k][s])
            s = int(bp)
    return word, path, begin, float(score), float(gap)


def decode(case, logb, p):
    """decode_log over a case's utterances on logb[F][NS]: (word[F], path[F], begin[F], score[U], gap[U])"""
    logAs = [log_a(np.asarray(w[0].A, dtype=np.float64)) for w in case.words]
    off = offsets(case.lens)
    outs = [decode_log(logAs, logb[off[u]:off[u + 1]], p) for u in range(case.U)]
    cat = [np.concatenate([o[i] for o in outs]).astype(np.int32) for i in range(3)]
    return cat[0], cat[1], cat[2], np.array([o[3] for o in outs]), np.array([o[4] for o in outs])


def oracle_log_b(case):
    """log b[F][NS] in float64: the oracle's (full-covariance: fullstreams_ref's) summed log emission, word
    by word; a word that is the same host object as an earlier one (ones2048) takes that one's columns"""
    if case.name in FULLCOV:
        import fullstreams_ref as S
        one = lambda hms: np.asarray(S.log_emission(hms, case.Xs, np.float64)[0], dtype=np.float64)
    else:
        one = lambda hms: V.log_b(hms, case.Xs)
    seen = {}
    cols = [seen[id(hms)] if id(hms) in seen else seen.setdefault(id(hms), one(hms)) for hms in case.words]
    return np.concatenate(cols, axis=1) if case.F else np.zeros((0, case.NS))


def holes_pattern(case, lb):
    """(the NaN columns, the -inf columns) that holes' models ask for; asserts that lb[F][NS] holds NaN in
    exactly the former, -inf in exactly the latter and finite values elsewhere, in every frame"""
    nan = [case.bo[k + 1] - 1 for k in HOLES_NAN_END] + [case.bo[HOLES_DENSE] + HOLES_DENSE_NAN]
    inf = [case.bo[k] + 2 for k in HOLES_INF]
    want_nan, want_inf = (np.isin(np.arange(case.NS), c)[None, :].repeat(case.F, 0) for c in (nan, inf))
    assert np.array_equal(np.isnan(lb), want_nan), "log b is not NaN in exactly the columns of det = 0"
    assert np.array_equal(lb == -np.inf, want_inf), "log b is not -inf in exactly the columns of c = 0"
    assert np.isfinite(lb[~want_nan & ~want_inf]).all(), "log b is not finite in the other columns"
    return sorted(int(c) for c in nan), sorted(int(c) for c in inf)


def strings(word, begin, lens):
    """per utterance the decoded word sequence"""
    off = offsets(lens)
    return [tuple(int(word[f]) for f in range(off[u], off[u + 1]) if begin[f]) for u in range(len(lens))]


# The utterances that the restatement decodes to their spoken sequence on the oracle's log b, per case the
# utterances at p = 0 and at p = -5: what qualifying() gives, asserted to be exactly this by
# test_connect_host.py, and asserted of the device by test_connect_gpu.py.  (An utterance too short for
# any word end to be reached is word 0 throughout: narrow's utterance 1 and wide's utterance 1 qualify so.)
QUALIFY = {
    "narrow": {0.0: [1, 3, 4, 5, 6, 7, 8], -5.0: [1, 3, 4, 5, 6, 7, 8]},
    "mixed": {0.0: [0, 1, 3], -5.0: [0, 1, 3]},
    "wide": {0.0: [0, 1, 2], -5.0: [0, 1, 2]},
    "many": {0.0: [2], -5.0: []},
    "full": {0.0: [0, 1, 2], -5.0: [0, 1, 2]},
    "thick": {0.0: [0, 3], -5.0: [3]},
    "crowd": {0.0: [], -5.0: []},         # (300 words of one 2-d Gaussian per state: nothing is recognised)
    "cap": {0.0: [0, 1, 2], -5.0: [0, 1, 2]},
}


def qualifying(case):
    """[(penalty, utterance)] over p = 0, -5 and the utterances of at least one frame"""
    lb = oracle_log_b(case)
    out = []
    for p in (0.0, -5.0):
        word, _, begin, _, _ = decode(case, lb, p)
        got = strings(word, begin, case.lens)
        out += [(p, u) for u in range(case.U) if case.lens[u] and got[u] == case.spoken[u]]
    return out


__all__ = ["ALL", "DIAGONAL", "NONTIE", "BEYOND", "FULLCOV", "GAP", "ENTRY", "UTTS", "penalties", "make", "log_a", "beats", "pick",
           "decode_log", "decode", "oracle_log_b", "holes_pattern", "strings", "QUALIFY", "qualifying"]
