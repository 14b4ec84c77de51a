"""The vocabularies of the several-stream vocabulary calls (ghmm_viterbi_full_streams, the three
ghmm_*_full_streams_batch calls, ghmm_recognise_full_streams), the winner rule of include/ghmm.h as a
pure function, and float64 restatements of the scores built from the reference modules.  Shared by
test_fullvocab_host.py, which checks on the CPU that the cases hold what the GPU tests lean on, and by
test_fullvocab_streams_gpu.py.  Plain numpy, no GPU, no tests.

The smallest shapes at which the new code can go wrong:
  narrow     K = 3, N = (5, 16, 9), P = 3 with (M, D) = (1, 3), (3, 9), (2, 17).  Nmax = 16: L = 16, the
             16-byte-row back-trace with its 8-row unroll, four groups per wave.  Word 1 is ergodic, the
             others banded: the banded / dense vote differs between blockIdx.y rows.
  mixed      K = 4, N = (3, 16, 17, 6), P = 2.  Nmax = 17: L = 32, nonzero column offsets, other active
             lanes per word.  Word 3 is a "ties" model: equal transitions, every state the same mixture.
  mixed-tie  mixed with word 3 replaced by a copy of word 0: exactly equal scores, the lowest word wins.
  wide       K = 2, N = (33, 64), P = 2.  L = 64; NS = 97 > 64: several blockIdx.y rows of the emission
             over the concatenated vocabulary and a last wave of one state.  Word 0 has transitions off
             the band (the dense step at L = 64) that jump at most 3 states ahead, so that 5 frames do
             not reach its last state; word 1 is banded.
  far        fullstreams_ref.make_far_case's two-stream model twice, the means shifted in the second: the
             linear product underflows on a frame, the log score stays finite.
Lengths of narrow and mixed: (0, 1, 2, 7, 8, 9, 17, 40, 5): T = 0, T < N, both sides of the PF = 8
prefetch boundary and of the 8-row back-trace unroll; U = 9 leaves a partly filled last wave at both L.
Lengths of wide: (70, 5, 64, 0), two full 64-frame tiles and one of 11.
Every utterance is a walk through one of the words, so the winners differ between utterances."""
import numpy as np

import fullstreams_ref as S
import oracle_lib as O
from fullcov_support import banded, ergodic, offsets, rand_fmodel

LENS = (0, 1, 2, 7, 8, 9, 17, 40, 5)
WIDE_LENS = (70, 5, 64, 0)
SHAPES = {      # name: (N per word, (M_p, D_p) per stream, lengths, the word each utterance walks, seed)
    "narrow": ((5, 16, 9), ((1, 3), (3, 9), (2, 17)), LENS, (0, 1, 2, 0, 1, 2, 0, 1, 2), 411),
    "mixed": ((3, 16, 17, 6), ((2, 9), (3, 5)), LENS, (0, 1, 2, 3, 0, 1, 2, 3, 0), 412),
    "wide": ((33, 64), ((1, 3), (2, 9)), WIDE_LENS, (1, 1, 0, 0), 413),
}
VOCABS = ("narrow", "mixed", "wide")        # the ones the host conditions are stated for
ALL = VOCABS + ("mixed-tie", "far")


class Case:
    """words[k][p] = HostFullModel of stream p of word k, Xs[p] = stream p's frames, lens"""

    def __init__(self, words, Xs, lens):
        self.words, self.Xs, self.lens = words, Xs, np.asarray(lens, dtype=np.int32)
        self.K, self.P = len(words), len(words[0])
        self.Ns = [w[0].N for w in words]
        self.NS, self.F, self.U = sum(self.Ns), int(self.lens.sum()), len(self.lens)
        self.bo = np.concatenate([[0], np.cumsum(self.Ns)]).astype(int)     # word k's columns of b[F][NS]

    def stream0(self):
        """the single-stream vocabulary made from stream 0 alone"""
        return Case([[w[0]] for w in self.words], self.Xs[:1], self.lens)


def _limited(rng, N, jump=3):
    """ergodic's A without the transitions more than `jump` states ahead (or from the last states back
    to the first): off the band, yet the last state is `(N - 1) / jump` frames away"""
    i, j = np.indices((N, N))
    A = ergodic(rng, N) * ((j <= i + jump) & (j >= i - 2))
    A[N - 1, N - 1] += 0.1
    return A / A.sum(1, keepdims=True)


def _ties(G, rng, N, shapes):
    """every transition 1 / N and every state the same mixture, in every stream: all candidates tie"""
    out = []
    for M, D in shapes:
        hm = rand_fmodel(G, rng, N, M, D, A=np.full((N, N), 1.0 / N), spread=0.3, asym=True, word="w3")
        for a in (hm.c, hm.mean, hm.inv_cov, hm.det):
            a[:] = a[0]
        out.append(G.HostFullModel(hm.A, hm.c, hm.mean, hm.inv_cov, hm.det, word="w3"))
    return out


def _frames(rng, words, lens, spoken):
    """utterance u = fullstreams_ref.stream_frames' walk through word spoken[u]"""
    P = len(words[0])
    parts = [S.stream_frames(rng, words[k], [int(T)]) for k, T in zip(spoken, lens)]
    return [np.concatenate([x[p] for x in parts]) for p in range(P)]


def make(G, name):
    if name == "far":
        hms, Xs, lens = S.make_far_case(G)
        moved = [G.HostFullModel(h.A, h.c, h.mean + 0.5, h.inv_cov, h.det, word="far2") for h in hms]
        return Case([hms, moved], Xs, lens)
    Ns, shapes, lens, spoken, seed = SHAPES["mixed" if name == "mixed-tie" else name]
    rng = np.random.default_rng(seed)
    words = []
    for k, N in enumerate(Ns):
        if name.startswith("mixed") and k == 3:
            words.append(_ties(G, rng, N, shapes))
            continue
        if name == "wide":
            A = _limited(rng, N) if k == 0 else banded(rng, N)
        else:
            A = ergodic(rng, N) if k == 1 else banded(rng, N)
        words.append([rand_fmodel(G, rng, N, M, D, A.copy(), spread=1.0, asym=(p == 1), word=f"w{k}")
                      for p, (M, D) in enumerate(shapes)])
    Xs = _frames(rng, words, lens, spoken)
    if name == "mixed-tie":
        words[3] = [G.HostFullModel(h.A, h.c, h.mean, h.inv_cov, h.det, word="w3") for h in words[0]]
    return Case(words, Xs, lens)


# ------------------------------------------------------------- the winner rule

def winners(table):
    """include/ghmm.h, ghmm_recognise_full_streams: per column of table[K][U], best = 0; k = 1 .. K-1 in
    order takes over if table[k] > table[best], or if table[best] is NaN and table[k] is not"""
    table = np.asarray(table, dtype=np.float64)
    out = np.zeros(table.shape[1], dtype=np.int32)
    for u in range(table.shape[1]):
        best = 0
        for k in range(1, table.shape[0]):
            s, sb = table[k, u], table[best, u]
            if s > sb or (np.isnan(sb) and not np.isnan(s)):
                best = k
        out[u] = best
    return out


# ------------------------------------------------------------- float64 restatements

def viterbi_table(case):
    """score[K][U] of the Viterbi lattice (oracle_lib.viterbi_lattice) on fullstreams_ref's summed log b
    in float64; T = 0 scores 0"""
    off = offsets(case.lens)
    out = np.zeros((case.K, case.U))
    for k, hms in enumerate(case.words):
        logb = np.asarray(S.log_emission(hms, case.Xs, np.float64)[0], dtype=np.float64)
        for u, T in enumerate(case.lens):
            if T:
                out[k, u] = O.viterbi_lattice(hms[0].A, logb[off[u]:off[u + 1]])[1]
    return out


def logscore_table(case, final_state):
    return np.array([np.asarray(S.logscore(hms, case.Xs, case.lens, final_state, np.float64), dtype=np.float64)
                     for hms in case.words])


def score_table(case):
    return np.array([np.asarray(S.score(hms, case.Xs, case.lens, np.float64), dtype=np.float64)
                     for hms in case.words])


__all__ = ["ALL", "VOCABS", "Case", "make", "winners", "viterbi_table", "logscore_table", "score_table"]
