"""The cases of the forced alignment (ghmm_align_streams, ghmm_align_full_streams; k_align) and a float64 numpy
restatement of its definition in include/ghmm.h.  Shared by test_align_host.py, which checks on the CPU
that the restatement is the definition (against an enumeration of all alignments), that it agrees with
connect_cases' decoder where it must, and that the cases keep the margin under which a differing path
cannot be blamed on rounding, and by test_align_gpu.py.  Plain numpy and the oracle, no GPU, no tests.

A case is one of connect_cases' (its vocabulary and its utterances, the transcript of an utterance being
what was spoken), some with further utterances behind them, composed the same way from an rng of their own:
  narrow  as it is: S_u differs within one launch (1, 2 and 3 words; 5 to 30 states), the ergodic word 1
          sits mid-transcript, the repeated word (0, 0), T = 0; the utterances of 1 and 2 frames are
          shorter than their word: -inf.
  mixed   as it is (the command line's case).
  wide    + (1, 0, 1) on 250 frames: S = 161, three waves, instances that straddle wave boundaries, the
          dense step on word 0's columns.
  many    + a 20-word transcript on 90 frames (S = 60): an entry in most frames.
  ones    as it is: one-state words, an instance is its own entry and end; T = 1 with a one-word transcript.
  short   narrow's corpus under other transcripts, most of them longer than their utterance: -inf.
  cap     many's vocabulary, ONE utterance of 682 three-state instances on 2200 frames: S = 2046, the
          launch with more than 48 KB of LDS, eight states per thread.
  full    as it is.
  cap-mixed  many's vocabulary, the cap's utterance among small ones, in this order: a 2-word one (S = 6),
          T = 0 with an empty transcript, cap's 682 instances on 2200 frames (S = 2046), a 1-word one and a
          20-word one.  All five run with 256 threads and LDS rows 2046 apart, the last two keep their
          back-pointers behind the long one's 4.5 MB, order[] puts the long one first.
  thick   connect_cases' thick (NS = 308, the ergodic words 1 and 23) + 20 instances alternating words 1
          and 23 on 110 frames: S = 280, the dense step at s >= 256, in a thread's second pass, with an
          instance that straddles 256.
  holes   connect_cases' holes: full-covariance words with NaN and -inf columns in log b.  Not among ALL
          (the host conditions there ask for a finite log b); HOLES names its transcripts.
The cases of embed_cases alone (in none of the tuples below; embed_cases says what each reaches): wide128 (wide
without its further utterance: S = 97), mid (mixed + two utterances that end on its word of 17 states), broad and broad256 (connect_cases'), pass4 (thick's vocabulary, S = 791),
pass8 (many's, 342 instances: S = 1026) and deep (cap's 64-state words, S = 192)."""
import numpy as np

import connect_cases as CC
from fullcov_support import offsets
from fullstreams_ref import stream_frames

ENTRY = CC.ENTRY
GAP = CC.GAP
MAX_S = 2048
# at most this many utterances of a case may have a gap of GAP or less on the oracle's log b and be left
# out of the path comparison (test_align_host.py holds the cases to it; the seeds below meet it with 0)
MAX_BELOW_GAP = 1

# pass4: thick's ergodic words 1 (16 states) and 23 (12) recurring on 4 frames each, the banded word 4 (7 states,
# 9 frames) after every fifth pair: 59 instances, S = 791, 261 frames
PASS4_SEQ = ((1, 23) * 5 + (4,)) * 5 + (1, 23) * 2

#        name: (connect_cases' case, [(further word sequence, frames per word)], seed of the further frames)
EXTRA = {
    "narrow": ("narrow", [], 0),
    "mixed": ("mixed", [], 0),
    "wide": ("wide", [((1, 0, 1), (95, 55, 100))], 713),
    "many": ("many", [(tuple((7 * i + 3) % 70 for i in range(20)), (5, 4) * 10)], 714),
    "ones": ("ones", [], 0),
    "short": ("narrow", [], 0),
    "cap": ("many", [(tuple((11 * i + 5) % 70 for i in range(682)), (4,) * 154 + (3,) * 528)], 716),
    "full": ("full", [], 0),
    "cap-mixed": ("many", [((12, 40), (5, 6)), ((), ()),
                           (tuple((11 * i + 5) % 70 for i in range(682)), (4,) * 154 + (3,) * 528),
                           ((33,), (7,)), (tuple((7 * i + 3) % 70 for i in range(20)), (5, 4) * 10)], 717),
    "thick": ("thick", [((1, 23) * 10, (6, 5) * 10)], 718),
    "holes": ("holes", [], 0),
    # embed_cases' own (among none of the tuples below: the alignment tests do not walk them)
    "wide128": ("wide", [], 0),
    "mid": ("mixed", [((1, 2), (20, 22)), ((2,), (30,))], 723),
    "broad": ("broad", [], 0),
    "broad256": ("broad256", [], 0),
    "pass4": ("thick", [(PASS4_SEQ, tuple(9 if k == 4 else 4 for k in PASS4_SEQ)), ((6, 23), (20, 6)), ((), ())], 719),
    "pass8": ("many", [(tuple((11 * i + 5) % 70 for i in range(342)), (3,) * 300 + (4,) * 42),
                       ((12, 40), (5, 6))], 722),      # (720: a cancelling num_mu, float64 spread 7e-9)
    "deep": ("cap", [((3, 5, 17), (75, 40, 75)), ((9,), (70,))], 721),
}
ALONE = ("cap", "cap-mixed", "pass4", "pass8", "deep")        # the further utterances are the case's only ones
CAP_MIXED_LONG = 2                  # cap-mixed's utterance of 682 instances
# holes' utterances have 50, 60, 12, 2 and 0 frames; words 0, 9 and 19 end in a NaN column, words 4 and 13
# have a column of -inf.  name: (transcripts, what the scores must be)
HOLES = {
    "spoken": ([(2, 5), (11, 3, 16), (0,), (1,), ()], ("finite", "finite", "nan", "-inf", "0")),
    "ends-in-nan": ([(2, 9), (11, 3, 19), (0,), (1,), ()], ("nan", "nan", "nan", "-inf", "0")),
    "nan-in-the-middle": ([(3, 9, 6), (11, 0, 16), (0,), (1,), ()], ("-inf", "-inf", "nan", "-inf", "0")),
    "through-minus-inf": ([(3, 4, 6), (13, 3), (0,), (1,), ()], ("-inf", "-inf", "nan", "-inf", "0")),
}
# short: narrow's lengths are 0, 1, 2, 7, 8, 9, 17, 40, 40 and its words have 5, 16 (ergodic) and 9 states
SHORT = [(), (0, 2), (0, 2), (0, 2), (2, 0), (0, 2, 0), (2, 0, 2), (0, 2, 0), (2, 1, 0)]
DIAGONAL = ("narrow", "mixed", "wide", "many", "ones", "short", "cap", "cap-mixed", "thick")
ALL = DIAGONAL + ("full",)
SMALL = tuple(n for n in ALL if n not in ALONE + ("thick",))      # what the tests loop over freely


def make(G, name):
    """connect_cases.make's Case with the further utterances appended, .transcripts[u] = utterance u's
    word sequence (empty for T = 0), .name; cap keeps the further utterance alone"""
    base, extra, seed = EXTRA[name]
    case = CC.make(G, base)
    spoken = list(case.spoken)
    if extra:
        rng = np.random.default_rng(seed)
        P = case.P
        parts = [[X] for X in case.Xs]
        lens = [int(T) for T in case.lens]
        if name in ALONE:
            parts, lens, spoken = [[] for _ in range(P)], [], []
        for seq, seg in extra:
            assert len(seq) == len(seg)
            for k, T in zip(seq, seg):
                x = stream_frames(rng, case.words[k], [int(T)])
                for p in range(P):
                    parts[p].append(x[p])
            lens.append(int(sum(seg)))
            spoken.append(tuple(seq))
        case = type(case)(case.words, [np.concatenate(x) for x in parts], lens)
    case.spoken = spoken
    case.transcripts = list(SHORT) if name == "short" else list(spoken)
    case.name = name
    return case


def log_as(case):
    return [CC.log_a(np.asarray(w[0].A, dtype=np.float64)) for w in case.words]


def states_of(case, transcript):
    return int(sum(case.Ns[k] for k in transcript))


# ------------------------------------------------------------- the definition in float64

def _margin(win, other):
    fin = np.isfinite(win) & np.isfinite(other)
    return np.where(fin, win - np.where(fin, other, 0.0), np.inf)


def align_log(logAs, cols, logb, transcript):
    """One utterance: the recursion and the trace of include/ghmm.h on logb[T][NS] (word k's columns from
    cols[k]) and the words' log A, for the transcript's instances.  Returns (word[T], path[T], begin[T],
    score, gap): gap = the smallest difference, along the traced path, between the winning candidate and
    the runner-up at every decision (the predecessor within the word, entry against stay); inf where there
    is no finite runner-up.  The instances are padded to the largest word with states of -inf."""
    T, L = len(logb), len(transcript)
    if T == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, z.copy(), z.copy(), 0.0, np.inf
    assert L > 0
    Ns = np.array([logAs[k].shape[0] for k in transcript])
    Nm = int(Ns.max())
    LA = np.full((L, Nm, Nm), -np.inf)
    col = np.zeros((L, Nm), dtype=int)
    real = np.zeros((L, Nm), dtype=bool)
    for i, k in enumerate(transcript):
        LA[i, :Ns[i], :Ns[i]] = logAs[k]
        col[i, :Ns[i]] = cols[k] + np.arange(Ns[i])
        real[i, :Ns[i]] = True
    last = Ns - 1
    inst = np.arange(L)

    def lb(t):
        return np.where(real, logb[t][col], -np.inf)

    with np.errstate(all="ignore"):
        d = np.full((L, Nm), -np.inf)
        d[0, 0] = 0.0
        d = d + lb(0)
        psi, gin, gent = [np.zeros((L, Nm), dtype=int)], [np.full((L, Nm), np.inf)], [np.full(L, np.inf)]
        for t in range(1, T):
            cand = d[:, :, None] + LA                               # [instance][i'][j]
            cand = np.where(np.isnan(cand), -np.inf, cand)          # a NaN never wins a strict >
            arg = np.argmax(cand, axis=1)                           # the first maximum; 0 where all are -inf
            top = -np.sort(-cand, axis=1)
            best = top[:, 0, :].copy()
            g = _margin(top[:, 0, :], top[:, 1, :]) if Nm > 1 else np.full((L, Nm), np.inf)
            ge = np.full(L, np.inf)
            if L > 1:
                x = d[inst[:-1], last[:-1]]                         # the entry candidate of instances 1 ..
                ent = x > best[1:, 0]
                ge[1:] = np.where(ent, _margin(x, best[1:, 0]), _margin(best[1:, 0], x))
                arg[1:, 0] = np.where(ent, ENTRY, arg[1:, 0])
                best[1:, 0] = np.where(ent, x, best[1:, 0])
            d = best + lb(t)
            psi.append(arg)
            gin.append(g)
            gent.append(ge)
    i, s = L - 1, int(last[L - 1])
    score, gap = d[i, s], np.inf
    word, path, begin = (np.zeros(T, dtype=np.int32) for _ in range(3))
    for t in range(T - 1, -1, -1):
        word[t], path[t] = transcript[i], s
        if t == 0:
            begin[t] = 1
            break
        bp = psi[t][i, s]
        if s == 0 and i > 0:
            gap = min(gap, gent[t][i])
        if bp == ENTRY:
            begin[t] = 1
            i -= 1
            s = int(last[i])
        else:
            gap = min(gap, gin[t][i, s])
            s = int(bp)
    return word, path, begin, float(score), float(gap)


def align(case, logb, transcripts=None):
    """align_log over a case's utterances on logb[F][NS]: (word[F], path[F], begin[F], score[U], gap[U])"""
    transcripts = case.transcripts if transcripts is None else transcripts
    logAs, off = log_as(case), offsets(case.lens)
    outs = [align_log(logAs, case.bo, logb[off[u]:off[u + 1]], transcripts[u]) for u in range(case.U)]
    cat = [np.concatenate([o[i] for o in outs]).astype(np.int32) for i in range(3)]
    return cat[0], cat[1], cat[2], np.array([o[3] for o in outs]), np.array([o[4] for o in outs])


def compared(case, gap):
    """the frames of the utterances whose gap is above GAP: where word, path and begin are compared"""
    return np.repeat(np.asarray(gap) > GAP, case.lens)


def oracle_log_b(case):
    """connect_cases.oracle_log_b: it asks the name only whether the words are full-covariance ones"""
    return CC.oracle_log_b(case)


__all__ = ["ALL", "DIAGONAL", "SMALL", "ALONE", "CAP_MIXED_LONG", "HOLES", "GAP", "MAX_BELOW_GAP", "MAX_S", "ENTRY", "EXTRA", "SHORT", "make", "log_as",
           "states_of", "align_log", "align", "compared", "oracle_log_b"]
