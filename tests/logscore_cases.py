"""The cases of the diagonal log-domain forward score (ghmm_logscore, ghmm_logscore_batch,
ghmm_logscore_streams, ghmm_logscore_streams_batch), shared by test_logscore_host.py and
test_logscore_gpu.py; the references built on them are logscore_ref.py's.  Plain numpy, no GPU, no tests.

Every case is a vocab_cases.Case (words[k][p], Xs[p], lens); the single-model cases hold one word on one
stream.  The smallest shapes at which each path can go wrong.  Every list of lengths has T = 1, a T < N,
T = 0, and frame 5 (inside utterance 0, which is long enough to reach the last state) lies 60 units from
every mean in every stream, so that the linear score of utterance 0 underflows.

  lane lattice (k_logforward_multi on a table of one word; L = 16, 16, 64, 64)
    lane_6x2x9_banded, lane_9x2x5_dense, lane_40x1x13_banded, lane_64x1x4_dense
    lane_c0    5x2x6 banded, c = 0 in state 1: log b = -inf there, the last state is out of reach
    lane_nan   5x2x6 dense, a det = 0 Gaussian in state 3 (log b = NaN), state 3 absorbing and the last
               state reached past it: the NaN stays in state 3 with final_state = 1
  wide (k_logforward_wide, one wave per utterance)
    wide_65x1x4_banded, wide_130x2x5_banded (lanes owning 2 and 3 states), wide_70x1x4_dense,
    wide_512x1x4_banded (utterances of 600, 30, 1 and 0 frames),
    wide_c0    70x1x4 banded with the c = 0 edit, wide_nan  70x1x4 dense with the NaN-absorbing edit
  vocabularies: three words of 3, 6 and 5 states (word 1 ergodic), lengths (40, 1, 4, 0, 12)
    vocab_p1   one stream (M, D) = (2, 5);  vocab_p2  two streams (2, 5), (3, 4)
    vocab70_p1, vocab70_p2   the same with the middle word replaced by an ergodic one of 70 states: the
               word-by-word fall-back

The float64 restatement's worst relative distance from the long-double one, |x64 - xld| / |xld| over the
finite scores of both final_state settings, measured by test_logscore_host.test_float64_spread (which
prints it and holds it below 1e-12):

    lane_6x2x9_banded   1.3e-15   lane_9x2x5_dense    2.8e-16   lane_40x1x13_banded 1.2e-15
    lane_64x1x4_dense   2.2e-16   lane_c0             2.7e-16   lane_nan            4.0e-16
    wide_65x1x4_banded  1.9e-15   wide_130x2x5_banded 2.9e-15   wide_70x1x4_dense   2.4e-16
    wide_512x1x4_banded 1.9e-14   wide_c0             1.3e-16   wide_nan            1.2e-16
    vocab_p1            1.2e-15   vocab_p2            1.7e-15   vocab70_p1          1.2e-15
    vocab70_p2          1.7e-15
"""
import numpy as np

from fullcov_support import banded, ergodic, frames
from vocab_cases import Case, rand_model, _frames

FAR_FRAME, FAR = 5, 60.0

# name: (N, M, D, dense A, utterance lengths, edit)
SINGLE = {
    "lane_6x2x9_banded": (6, 2, 9, False, (70, 1, 3, 0, 33), None),
    "lane_9x2x5_dense": (9, 2, 5, True, (40, 1, 3, 0), None),
    "lane_40x1x13_banded": (40, 1, 13, False, (90, 1, 39, 0), None),
    "lane_64x1x4_dense": (64, 1, 4, True, (80, 10, 1, 0), None),
    "lane_c0": (5, 2, 6, False, (30, 1, 3, 0, 20), "c0"),
    "lane_nan": (5, 2, 6, True, (30, 1, 3, 0, 20), "nan"),
    "wide_65x1x4_banded": (65, 1, 4, False, (80, 1, 30, 0), None),
    "wide_130x2x5_banded": (130, 2, 5, False, (150, 1, 40, 0), None),
    "wide_70x1x4_dense": (70, 1, 4, True, (80, 1, 20, 0), None),
    "wide_512x1x4_banded": (512, 1, 4, False, (600, 30, 1, 0), None),
    "wide_c0": (70, 1, 4, False, (80, 1, 20, 0), "c0"),
    "wide_nan": (70, 1, 4, True, (80, 1, 20, 0), "nan"),
}
# name: (N per word, (M_p, D_p) per stream)
VOCAB_LENS = (40, 1, 4, 0, 12)
VOCAB = {
    "vocab_p1": ((3, 6, 5), ((2, 5),)),
    "vocab_p2": ((3, 6, 5), ((2, 5), (3, 4))),
    "vocab70_p1": ((3, 70, 5), ((2, 5),)),
    "vocab70_p2": ((3, 70, 5), ((2, 5), (3, 4))),
}
NAMES = tuple(SINGLE) + tuple(VOCAB)
EDITED = ("lane_c0", "lane_nan", "wide_c0", "wide_nan")


def _single(G, name, far):
    N, M, D, dense, lens, edit = SINGLE[name]
    rng = np.random.default_rng(700 + list(SINGLE).index(name))
    hm = rand_model(G, rng, N, M, D, ergodic(rng, N) if dense else banded(rng, N))
    if edit == "c0":
        hm.c[1] = 0.0
    if edit == "nan":
        hm.det[3, M - 1] = 0.0
        hm.A[3] = 0.0
        hm.A[3, 3] = 1.0                # no way out of state 3 ...
        hm.A[:, N - 1] += 0.05          # ... and the last state is reached past it
        hm.A[3, N - 1] = 0.0
        hm.A /= hm.A.sum(1, keepdims=True)
    hm = G.HostModel(hm.A, hm.c, hm.mean, hm.inv_var, hm.det, word=name)
    X = frames(rng, hm, lens)
    if far:
        X[FAR_FRAME] += FAR
    return Case([[hm]], [X], lens)


def _vocab(G, name, far):
    Ns, shapes = VOCAB[name]
    rng = np.random.default_rng(760 + len(shapes))      # (the 70-state vocabulary shares the others' words)
    words = []
    for k, N in enumerate((3, 6, 5)):
        A = ergodic(rng, N) if k == 1 else banded(rng, N)
        words.append([rand_model(G, rng, N, M, D, A.copy(), word=f"w{k}") for M, D in shapes])
    Xs = _frames(rng, words, VOCAB_LENS, (0, 1, 2, 0, 1))
    if Ns[1] == 70:
        A = ergodic(rng, 70)
        words[1] = [rand_model(G, rng, 70, M, D, A.copy(), word="w70") for M, D in shapes]
    if far:
        for X in Xs:
            X[FAR_FRAME] += FAR
    return Case(words, Xs, VOCAB_LENS)


def make(G, name, far=True):
    """the Case of a name; far = False leaves frame 5 where it was drawn"""
    return _single(G, name, far) if name in SINGLE else _vocab(G, name, far)
