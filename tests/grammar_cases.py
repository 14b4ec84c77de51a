"""The cases of the connected-word decoder under a word-pair grammar (ghmm_connect_grammar_streams,
ghmm_connect_grammar_full_streams; k_grammar) and a float64 numpy restatement of its definition in
include/ghmm.h.  Shared by test_grammar_host.py, which checks on the CPU that the restatement is the
definition (against an enumeration of all composite paths with their word boundaries), that it agrees with
connect_cases' and align_cases' restatements where it must, and that the cases keep the margin under which
a differing path cannot be blamed on rounding, and by test_grammar_gpu.py.  Plain numpy and the oracle, no
GPU, no tests.

The vocabularies and utterances are connect_cases' (narrow, wide, many, thick, cap, ones, full, holes, and
the rest for the flat grammar), with one case more:
  k256    K = 256 words of 2 and 3 states (N = (2, 3)[k % 2]), banded, (M, D) = (1, 2).  NS = 640: the cap
          on K, predecessor words up to 255 in the byte, the table read from L2, a first state in every
          thread.  Utterances of at most 20 frames: the restatement walks 256 words per frame.
  k100    K = 100 such words, NS = 250: 256 threads, so R = 2 slices per word, and the table is still read
          from L2: three unrolled rounds of sixteen candidates and then a tail of two (w = 96 + r, 98 + r) in
          every slice.  Under its random grammar the traced path enters words both from a tail candidate
          (w >= 96) and from an unrolled round (test_grammar_host.py holds the seed to it).
  k72     K = 72 such words, NS = 180: 192 threads, R = 2, and the table IS staged (52 176 bytes): four unrolled
          rounds of eight and then a tail of four (w >= 64) in every slice, held the same way.  (many, the
          other staged case with rounds and a tail, has no traced entry from a tail candidate.)
Grammars (start, pair, fin), by name:
  flat:p      pair == p, start == fin == 0: ghmm_connect_streams(p)
  random      entries in [-6, 0], about 30 % of pair -inf, some -inf in start and fin; seeded per case
  norepeat    the diagonal of pair is -inf, the rest NOREPEAT_P; start == fin == 0
  chain:...   chain(transcript): 0 along the transcript of pairwise distinct words, -inf elsewhere"""
import numpy as np

import connect_cases as CC
import vocab_cases as V
from fullcov_support import banded, offsets
from fullstreams_ref import stream_frames

ENTRY = CC.ENTRY
GAP = CC.GAP
MAX_K = 256
NOREPEAT_P = -2.0
# at most this many utterances of a (case, grammar) pair may have a gap of GAP or less on the oracle's log b
# and be left out of the path comparison (test_grammar_host.py holds every pair below to it)
MAX_BELOW_GAP = 1

K256_NS = (2, 3)
K256_UTTS = [((255, 3, 128), (6, 5, 7)), ((200, 254, 17, 255), (5, 4, 6, 5)), ((1,), (1,)), ((77, 130), (9, 8)),
             ((0,), (0,))]
K256_SEED = 911
K100_UTTS = [((99, 3, 64), (6, 5, 7)), ((70, 98, 17, 99), (5, 4, 6, 5)), ((1,), (1,)), ((37, 96), (9, 8)),
             ((97, 12, 98), (5, 6, 5)), ((0,), (0,))]
K100_SEED = 912
K72_UTTS = [((71, 3, 64), (6, 5, 7)), ((50, 70, 17, 65), (5, 4, 6, 5)), ((1,), (1,)), ((37, 68), (9, 8)),
            ((69, 12, 66), (5, 6, 5)), ((0,), (0,))]
K72_SEED = 913
# name: (K, utterances, seed) of the cases composed here
OWN = {"k256": (MAX_K, K256_UTTS, K256_SEED), "k100": (100, K100_UTTS, K100_SEED), "k72": (72, K72_UTTS, K72_SEED)}
# per case the first word of grammar_entry's tail: its random grammar's traced entries come from both sides of it
TAIL_FROM = {"k100": 96, "k72": 64}
THREADS, WAVE, STAGE_LDS, ITEMS = 256, 64, 64 << 10, 256

# the seed of every case's random grammar (chosen so that MAX_BELOW_GAP holds on the oracle's log b)
RANDOM_SEED = {"narrow": 21, "mixed": 22, "wide": 23, "many": 24, "ones": 25, "thick": 26, "cap": 27, "k256": 28,
               "full": 29, "holes": 30, "crowd": 31, "dup": 32, "k100": 39, "k72": 66}
# the (case, grammar) pairs that test_grammar_gpu.py compares with the restatement
SHAPES = ("narrow", "wide", "many", "thick", "k256", "cap", "k100", "k72")
GPU_GRAMMARS = {name: ("random", "norepeat", "flat:-5") for name in SHAPES}
GPU_GRAMMARS["cap"] = ("random", "norepeat")       # (the restatement walks 32 words of 64 states per frame)
GPU_GRAMMARS["ones"] = ("norepeat", "random")
GPU_GRAMMARS["full"] = ("random", "norepeat")
GPU_GRAMMARS["holes"] = ("random", "norepeat")
FULLCOV = CC.FULLCOV
# transcripts of pairwise distinct words for the chain grammar, per case; every one is laid over ALL the
# case's utterances (one grammar per call), those it was not spoken in and those too short for it included
CHAINS = {
    "narrow": [(0,), (1, 2), (2, 0, 1)],
    "mixed": [(0, 3), (1, 0, 3)],
    "many": [(5, 69, 33), (0, 65)],
    "k256": [(255, 3, 128), (77, 130)],
    "full": [(0, 2), (2, 0)],
}


def make(G, name):
    """connect_cases.make's Case (k256, k100: the cases above, composed the same way)"""
    if name not in OWN:
        return CC.make(G, name)
    K, utts, seed = OWN[name]
    rng = np.random.default_rng(seed)
    words = [[V.rand_model(G, rng, K256_NS[k % 2], 1, 2, banded(rng, K256_NS[k % 2]), word=f"w{k}")]
             for k in range(K)]
    parts, lens, spoken = [], [], []
    for seq, seg in utts:
        for k, T in zip(seq, seg):
            parts.append(stream_frames(rng, words[k], [int(T)])[0])
        lens.append(int(sum(seg)))
        spoken.append(tuple(seq) if sum(seg) else ())
    case = V.Case(words, [np.concatenate(parts)], lens)
    case.spoken, case.name = spoken, name
    return case


def entry_pass(NS, K):
    """what the host and k_grammar work out of a vocabulary (csrc/ghmm_grammar.hpp): whether the pair table is
    staged in LDS (grammar_staged), the slices R per word, and per slice r the unrolled rounds and the tail
    iterations of grammar_entry: (staged, R, [(rounds, tail) for r in range(R)])"""
    staged = NS * 36 + K * 16 + ITEMS * 12 + K * K * 8 <= STAGE_LDS
    threads = min(THREADS, -(-NS // WAVE) * WAVE)
    R = min(4, max(1, threads // K))
    unroll = 8 if staged else 16
    slices = []
    for r in range(R):
        rounds, w = 0, r
        while w + (unroll - 1) * R < K:
            rounds, w = rounds + 1, w + unroll * R
        slices.append((rounds, len(range(w, K, R))))
    return staged, R, slices


# ------------------------------------------------------------- grammars

def flat(K, p):
    return np.zeros(K), np.full((K, K), float(p)), np.zeros(K)


def random(K, seed, forbid=0.3):
    """entries uniform in [-6, 0]; about `forbid` of pair and a sixth of start and fin are -inf, with at
    least one word left to start and one to end, and every word left a successor"""
    rng = np.random.default_rng(seed)
    start, pair, fin = rng.uniform(-6, 0, K), rng.uniform(-6, 0, (K, K)), rng.uniform(-6, 0, K)
    pair[rng.random((K, K)) < forbid] = -np.inf
    if K > 1:
        start[rng.random(K) < 1 / 6] = -np.inf
        fin[rng.random(K) < 1 / 6] = -np.inf
        start[int(rng.integers(K))] = -1.0
        fin[int(rng.integers(K))] = -1.0
    for w in range(K):
        if not np.isfinite(pair[w]).any():
            pair[w, (w + 1) % K] = -3.0
    return start, pair, fin


def norepeat(K, p=NOREPEAT_P):
    pair = np.full((K, K), float(p))
    np.fill_diagonal(pair, -np.inf)
    return np.zeros(K), pair, np.zeros(K)


def chain(K, transcript):
    assert len(set(transcript)) == len(transcript) > 0
    start, pair, fin = np.full(K, -np.inf), np.full((K, K), -np.inf), np.full(K, -np.inf)
    start[transcript[0]] = 0.0
    fin[transcript[-1]] = 0.0
    for w, k in zip(transcript[:-1], transcript[1:]):
        pair[w, k] = 0.0
    return start, pair, fin


def grammar(case, which):
    """(start, pair, fin) of a case by the grammar's name: flat:<p>, random, norepeat"""
    if which.startswith("flat:"):
        return flat(case.K, float(which[5:]))
    if which == "random":
        return random(case.K, RANDOM_SEED[case.name])
    assert which == "norepeat", which
    return norepeat(case.K)


# ------------------------------------------------------------- the definition in float64

def _margin(win, other):
    return win - other if np.isfinite(win) and np.isfinite(other) else np.inf


def decode_log(logAs, logb, start, pair, fin):
    """One utterance: the recursion and the trace of include/ghmm.h on logb[T][NS] (word k's columns in
    order) and the words' log A under the grammar (start and fin may be None: zeros).  Returns (word[T],
    path[T], begin[T], score, gap): gap = the smallest difference, along the traced path, between the
    winning candidate and the runner-up at every decision (the predecessor within the word, entry against
    stay, the predecessor word of every entry the trace takes, the final pick on d + fin); inf where there
    is no finite runner-up."""
    Ns = [a.shape[0] for a in logAs]
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    K, T = len(Ns), len(logb)
    start = np.zeros(K) if start is None else np.asarray(start, dtype=np.float64)
    fin = np.zeros(K) if fin is None else np.asarray(fin, dtype=np.float64)
    pair = np.asarray(pair, dtype=np.float64)
    if T == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, z.copy(), z.copy(), 0.0, np.inf
    ar = np.arange(K)
    with np.errstate(all="ignore"):
        d = [np.where(np.arange(N) == 0, start[k], -np.inf) + logb[0, bo[k]:bo[k] + N] for k, N in enumerate(Ns)]
        psi = [[np.zeros(N, dtype=int) for N in Ns]]
        gin = [[np.full(N, np.inf) for N in Ns]]        # the predecessor within the word
        gent = [np.full(K, np.inf)]                     # entry against stay
        pw, gpw = [np.zeros(K, dtype=int)], [np.full(K, np.inf)]     # the predecessor word and its margin
        for t in range(1, T):
            e = np.array([d[k][-1] for k in range(K)])
            c = e[:, None] + pair                                    # [w][k]
            c = np.where(np.isnan(c), -np.inf, c)                    # a NaN never wins
            xw = np.argmax(c, axis=0)                                # the first maximum: the lowest w; 0 where all are -inf
            xv = c[xw, ar]
            if K > 1:
                two = -np.partition(-c, 1, axis=0)[:2]
                gx = np.where(np.isfinite(two[0]) & np.isfinite(two[1]), two[0] - two[1], np.inf)
            else:
                gx = np.full(K, np.inf)
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
                x = xv[k]
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
            pw.append(xw)
            gpw.append(gx)
        ends = [d[k][-1] + fin[k] for k in range(K)]
        k, gap = CC.pick(ends)
    k = int(k)
    score = ends[k]
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
            gap = min(gap, gpw[t][k])
            k = int(pw[t][k])
            s = Ns[k] - 1
        else:
            gap = min(gap, gin[t][k][s])
            s = int(bp)
    return word, path, begin, float(score), float(gap)


def log_as(case):
    return [CC.log_a(np.asarray(w[0].A, dtype=np.float64)) for w in case.words]


def decode(case, logb, start, pair, fin, per_utt=None):
    """decode_log over a case's utterances on logb[F][NS]: (word[F], path[F], begin[F], score[U], gap[U]);
    per_utt(u) = that utterance's own (start, pair, fin) where every utterance has its own grammar"""
    logAs, off = log_as(case), offsets(case.lens)
    outs = [decode_log(logAs, logb[off[u]:off[u + 1]], *(per_utt(u) if per_utt else (start, pair, fin)))
            for u in range(case.U)]
    cat = [np.concatenate([o[i] for o in outs]).astype(np.int32) for i in range(3)]
    return cat[0], cat[1], cat[2], np.array([o[3] for o in outs]), np.array([o[4] for o in outs])


def compared(case, gap):
    """the frames of the utterances whose gap is above GAP: where word, path and begin are compared"""
    return np.repeat(np.asarray(gap) > GAP, case.lens)


def oracle_log_b(case):
    return CC.oracle_log_b(case)


def allowed(case, word, begin, score, start, pair, fin):
    """consequence (c) of include/ghmm.h: for every utterance with a finite score, the decoded string's
    first word may start, every adjacent pair may follow, the last word may end; returns the strings"""
    start = np.zeros(case.K) if start is None else start
    fin = np.zeros(case.K) if fin is None else fin
    got = CC.strings(word, begin, case.lens)
    for u, s in enumerate(got):
        if case.lens[u] == 0 or not np.isfinite(score[u]):
            continue
        assert start[s[0]] > -np.inf, (u, s)
        assert all(pair[w, k] > -np.inf for w, k in zip(s[:-1], s[1:])), (u, s)
        assert fin[s[-1]] > -np.inf, (u, s)
    return got


__all__ = ["ENTRY", "GAP", "MAX_K", "MAX_BELOW_GAP", "SHAPES", "GPU_GRAMMARS", "CHAINS", "FULLCOV", "RANDOM_SEED",
           "make", "flat", "random", "norepeat", "chain", "grammar", "decode_log", "decode", "log_as", "compared",
           "oracle_log_b", "allowed", "entry_pass"]
