"""The vocabularies of the diagonal several-stream vocabulary calls (ghmm_viterbi_streams,
ghmm_score_streams_batch, ghmm_viterbi_streams_batch, ghmm_recognise_streams) and their float64
references, built from the oracle: every Viterbi score and path is

    oracle_lib.viterbi_lattice(A_k, sum over p in stream order of oracle_lib.log_emission(hm_kp, X_p))

with T = 0 scoring 0, every forward score oracle_lib.score_streams.  Shared by test_vocab_host.py, which
checks on the CPU that the cases hold what the GPU tests lean on, and by test_vocab_streams_gpu.py.  Plain
numpy and the oracle, no GPU, no tests.  The winner rule is fullvocab_cases.winners.

The smallest shapes at which the new code can go wrong:
  narrow     K = 3, N = (5, 16, 9), P = 3 with (M, D) = (1, 3), (3, 9), (2, 17): D = 3 is too narrow for the
             scheduled matrix-core emission, M = 3 is padded to Mp = 4, D = 17 takes the scheduled kernel.
             Nmax = 16: L = 16, the 16-byte-row back-trace with its 8-row unroll.  Word 1 is ergodic, the
             others banded.  Word 0's N * Mp (5, 20, 10) is no multiple of 16 in any stream: the tiles of 16
             Gaussians straddle words.
  mixed      K = 4, N = (3, 16, 17, 6), P = 2 with (M, D) = (2, 9), (3, 5).  Nmax = 17: L = 32, nonzero
             column offsets.  Word 1 is ergodic.
  mixed-tie  mixed with word 3 replaced by a copy of word 0 (exactly equal scores, the lowest word wins) and
             word 2 by a model of equal transitions and identical states (every predecessor ties, the
             lowest wins).  The frames are mixed's.
  wide       K = 2, N = (33, 64), P = 2.  L = 64; NS = 97.  Word 0 has transitions off the band that jump at
             most 3 states ahead, so that 5 frames do not reach its last state; word 1 is banded.
  one70      one word of 70 states, P = 2, for ghmm_viterbi_streams alone: the one-wave-per-utterance
             lattice (k_viterbi_wide).  Lengths (80, 3).
  far        two words of two streams with unit variances; frame 5 of utterance 0 lies sqrt(1000) from its
             state's mean in each stream: each stream's own densities there are about exp(-500) > 0, their
             product is 0 on the whole frame, the log b stays finite.
Lengths of narrow and mixed: (0, 1, 2, 7, 8, 9, 17, 40, 5): T = 0, T < N, both sides of the PF = 8
prefetch boundary and of the 8-row back-trace unroll.  Lengths of wide: (70, 5, 64, 0).
Every utterance is a walk through one of the words, so the winners differ between utterances.
name + "-p1" is stream 0 alone."""
import numpy as np

import oracle_lib as O
from fullcov_support import banded, ergodic, offsets
from fullstreams_ref import fold, stream_frames
from fullvocab_cases import winners

LENS = (0, 1, 2, 7, 8, 9, 17, 40, 5)
WIDE_LENS = (70, 5, 64, 0)
SHAPES = {      # name: (N per word, (M_p, D_p) per stream, lengths, the word each utterance walks, seed)
    "narrow": ((5, 16, 9), ((1, 3), (3, 9), (2, 17)), LENS, (0, 1, 2, 0, 1, 2, 0, 1, 2), 511),
    "mixed": ((3, 16, 17, 6), ((2, 9), (3, 5)), LENS, (0, 1, 2, 3, 0, 1, 2, 3, 0), 512),
    "wide": ((33, 64), ((1, 3), (2, 9)), WIDE_LENS, (1, 1, 0, 0), 513),
    "one70": ((70,), ((2, 9), (3, 5)), (80, 3), (0, 0), 514),
}
VOCABS = ("narrow", "mixed", "wide")        # the vocabularies without a tie: compared under the default kernels
TIES = ("mixed-tie",)                       # compared under GHMM_OPT_KERNELS = 1 only
LANES = {"narrow": 16, "mixed": 32, "mixed-tie": 32, "wide": 64}
GAP = 1e-6                                  # the margin test_vocab_host.py asks of every non-tie case


class Case:
    """words[k][p] = HostModel of stream p of word k, Xs[p] = stream p's frames, lens"""

    def __init__(self, words, Xs, lens):
        self.words, self.Xs, self.lens = words, Xs, np.asarray(lens, dtype=np.int32)
        self.K, self.P = len(words), len(words[0])
        self.Ns = [w[0].N for w in words]
        self.NS, self.F, self.U = sum(self.Ns), int(self.lens.sum()), len(self.lens)
        self.bo = np.concatenate([[0], np.cumsum(self.Ns)]).astype(int)     # word k's columns of b[F][NS]

    def stream0(self):
        """the single-stream vocabulary made from stream 0 alone"""
        return Case([[w[0]] for w in self.words], self.Xs[:1], self.lens)


def rand_model(G, rng, N, M, D, A, spread=1.0, word="w"):
    """Dirichlet weights, means N(0, spread), inverse variances 0.5 .. 2"""
    c = rng.dirichlet(np.full(M, 3.0), N)
    mean = rng.normal(0.0, spread, (N, M, D))
    iv = rng.uniform(0.5, 2.0, (N, M, D))
    return G.HostModel(A, c, mean, iv, np.prod(1.0 / iv, axis=-1), word=word)


def _limited(rng, N, jump=3):
    """ergodic's A without the transitions more than `jump` states ahead or more than two back: off the
    band, yet the last state is `(N - 1) / jump` frames away"""
    i, j = np.indices((N, N))
    A = ergodic(rng, N) * ((j <= i + jump) & (j >= i - 2))
    A[N - 1, N - 1] += 0.1
    return A / A.sum(1, keepdims=True)


def _ties(G, rng, N, shapes):
    """every transition 1 / N and every state the same mixture, in every stream: all candidates tie"""
    out = []
    for M, D in shapes:
        hm = rand_model(G, rng, N, M, D, np.full((N, N), 1.0 / N), spread=0.3, word="ties")
        for a in (hm.c, hm.mean, hm.inv_var, hm.det):
            a[:] = a[0]
        out.append(hm)
    return out


def _frames(rng, words, lens, spoken):
    """utterance u = fullstreams_ref.stream_frames' walk through word spoken[u]"""
    P = len(words[0])
    parts = [stream_frames(rng, words[k], [int(T)]) for k, T in zip(spoken, lens)]
    return [np.concatenate([x[p] for x in parts]) for p in range(P)]


def _far(G):
    rng = np.random.default_rng(577)
    A = banded(rng, 6)
    hms = []
    for M, D in ((2, 4), (1, 6)):
        h = rand_model(G, rng, 6, M, D, A.copy())
        hms.append(G.HostModel(h.A, h.c, h.mean, np.ones((6, M, D)), np.ones((6, M)), word="far"))
    lens = np.array([40, 30], dtype=np.int32)
    Xs = stream_frames(rng, hms, lens)
    for hm, X in zip(hms, Xs):
        v = np.zeros(hm.D)
        v[0] = np.sqrt(1000.0)
        X[5] = hm.mean[0, 0] + v
    moved = [G.HostModel(h.A, h.c, h.mean + 0.5, h.inv_var, h.det, word="far2") for h in hms]
    return Case([hms, moved], Xs, lens)


def make(G, name):
    if name.endswith("-p1"):
        return make(G, name[:-3]).stream0()
    if name == "far":
        return _far(G)
    Ns, shapes, lens, spoken, seed = SHAPES["mixed" if name == "mixed-tie" else name]
    rng = np.random.default_rng(seed)
    words = []
    for k, N in enumerate(Ns):
        if name == "wide":
            A = _limited(rng, N) if k == 0 else banded(rng, N)
        else:
            A = ergodic(rng, N) if k == 1 else banded(rng, N)
        words.append([rand_model(G, rng, N, M, D, A.copy(), word=f"w{k}") for M, D in shapes])
    Xs = _frames(rng, words, lens, spoken)
    if name == "mixed-tie":
        words[2] = _ties(G, rng, Ns[2], shapes)
        words[3] = [h.copy() for h in words[0]]
    return Case(words, Xs, lens)


# ------------------------------------------------------------- float64 references

def log_b(hms, Xs):
    """log b[F][N] of one word: the oracle's log emission of every stream, added in stream order"""
    return fold([O.log_emission(hm, X) for hm, X in zip(hms, Xs)], log=True)


def lattice(A, logb):
    """the Viterbi lattice of include/ghmm.h in numpy, with what the margin condition needs: (path, score,
    gap), gap = the smallest difference along the path between the best and the runner-up candidate
    predecessor (inf where there is no finite runner-up)"""
    T, N = logb.shape
    with np.errstate(divide="ignore"):
        logA = np.where(A > 0, np.log(np.where(A > 0, A, 1.0)), -np.inf)
    d = np.where(np.arange(N) == 0, 0.0, -np.inf) + logb[0]
    psi = np.zeros((T, N), dtype=np.int32)
    gaps = np.full((T, N), np.inf)
    for t in range(1, T):
        cand = d[:, None] + logA                       # [i][j]
        psi[t] = np.argmax(cand, axis=0)               # the first maximum: the lowest predecessor
        top = np.sort(cand, axis=0)[::-1]
        if N > 1:
            with np.errstate(invalid="ignore"):
                g = top[0] - top[1]
            gaps[t] = np.where(np.isfinite(top[1]), g, np.inf)
        d = top[0] + logb[t]
    path = np.zeros(T, dtype=np.int32)
    path[T - 1] = N - 1
    for t in range(T - 1, 0, -1):
        path[t - 1] = psi[t, path[t]]
    gap = min([gaps[t, path[t]] for t in range(1, T)], default=np.inf)
    return path, d[N - 1], gap


class Reference:
    """of a Case: logb[k] = word k's summed log b[F][N_k], vit[K][U] and paths[k] (F entries) from
    oracle_lib.viterbi_lattice, gap[K][U] from lattice() where the score is finite"""

    def __init__(self, case):
        off = offsets(case.lens)
        self.logb = [log_b(hms, case.Xs) for hms in case.words]
        self.vit = np.zeros((case.K, case.U))
        self.gap = np.full((case.K, case.U), np.inf)
        self.paths = [np.full(case.F, -1, dtype=np.int32) for _ in case.words]
        for k, hms in enumerate(case.words):
            for u, T in enumerate(case.lens):
                if T == 0:
                    continue
                lb = self.logb[k][off[u]:off[u + 1]]
                path, score = O.viterbi_lattice(hms[0].A, lb)
                self.vit[k, u] = score
                self.paths[k][off[u]:off[u + 1]] = path
                if np.isfinite(score):
                    p2, s2, self.gap[k, u] = lattice(hms[0].A, lb)
                    assert np.array_equal(p2, path) and s2 == score, (k, u)
        self.words = winners(self.vit)
        for a in [self.vit, self.gap, self.words] + self.logb + self.paths:
            a.setflags(write=False)


def forward_table(case):
    """fwd[K][U] = oracle_lib.score_streams per (word, utterance); T = 0 scores 0"""
    off = offsets(case.lens)
    out = np.zeros((case.K, case.U))
    for k, hms in enumerate(case.words):
        for u, T in enumerate(case.lens):
            if T:
                out[k, u] = O.score_streams(hms, [X[off[u]:off[u + 1]] for X in case.Xs])
    return out


def top_two_margin(vit):
    """per utterance the relative difference of the two best finite scores (inf with fewer than two)"""
    out = np.full(vit.shape[1], np.inf)
    for u in range(vit.shape[1]):
        s = np.sort(vit[np.isfinite(vit[:, u]), u])[::-1]
        if len(s) >= 2:
            out[u] = (s[0] - s[1]) / abs(s[0]) if s[0] != 0 else (np.inf if s[1] != 0 else 0.0)
    return out


__all__ = ["VOCABS", "TIES", "LANES", "GAP", "Case", "make", "winners", "log_b", "lattice", "Reference",
           "forward_table", "top_two_margin"]
