"""The utterance-length sweep across the prefetch queues of the lane lattices (logforward_run,
logbackward_run and viterbi_run in csrc/ghmm_kernels.hpp, behind k_logforward_multi, k_logfb_fwd, k_logfb_bwd,
k_viterbi and k_viterbi_multi), shared by test_lensweep_host.py and test_lensweep_gpu.py.  Plain numpy, no
GPU, no tests.

These kernels walk an utterance through a software queue of PF frames: whole queues in the main loop, an
unrolled tail of PF - 1 predicated steps for the rest, an operand cursor that is neither clamped nor
predicated and runs up to two queues past the utterance, and (L = 16, 32) four or two utterances of
different lengths in one wave.  What a kernel does therefore depends on (T - 1) mod PF, on T < PF, on the
utterances that lie next to it in memory and on those that share its wave.

    PF, WAVE   read from csrc/ghmm_kernels.hpp, so that the sweep follows the constants
    LENS       every length 0 .. 2 PF + 2 (every residue below one queue, at one queue and at two) and
               5 PF .. 6 PF - 1 (every residue again where a banded model of up to 33 states has reached its
               last state, so that log P is finite); with PF = 8: 0..18 and 40..47, 27 utterances, 519 frames.
               An utterance's number is its index in LENS, whatever the memory order.
    ORDERS     three fixed permutations of the utterances in memory: asc, desc and mix (a seeded shuffle),
               so that an utterance's neighbours differ between them.  The kernels' own `order` array sorts
               by length whatever the memory order: the permutations move neighbours in memory, not wave
               mates.
    CASES      N = 3, 17, 33 (lane widths 16, 32, 64), each banded (left to right: self and next) and dense,
               M = 2, D = 4; diagonal models from vocab_cases.rand_model (logscore_cases.py's generator),
               full-covariance ones from fullcov_support.rand_fmodel (fulllogscore_ref.py's).  Every
               utterance is fullcov_support.walk_any's walk through the states, so that a long utterance's
               gammas are of size 1 and not far below the absolute floor of their bound.  No far frames and
               no edited components: those have their own cases.
    POISONS    odd / even: the frames of every utterance of odd (even) length are NaN."""
import functools
import os
import re

import numpy as np

from _load import PKG_DIR
from fullcov_support import banded, ergodic, offsets, rand_fmodel, walk_any
from vocab_cases import rand_model


def _constant(name):
    text = open(os.path.join(PKG_DIR, "csrc", "ghmm_kernels.hpp")).read()
    found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert len(found) == 1, f"constexpr int {name} = ... is not there exactly once"
    return int(found[0])


PF = _constant("PF")
WAVE = _constant("WAVE")
LENS = tuple(range(0, 2 * PF + 3)) + tuple(range(5 * PF, 6 * PF))
U, F = len(LENS), sum(LENS)

ORDERS = {
    "asc": tuple(range(U)),
    "desc": tuple(range(U - 1, -1, -1)),
    "mix": tuple(int(i) for i in np.random.default_rng(20261).permutation(U)),
}
POISONS = ("odd", "even")

M, D = 2, 4
STATES = (3, 17, 33)
LANES = {3: 16, 17: 32, 33: 64}
KINDS = ("diag", "full")
NAMES = {kind: tuple(f"{kind}_{N}_{shape}" for N in STATES for shape in ("banded", "dense")) for kind in KINDS}


def poisoned(i, poison):
    """utterance i holds NaN frames under `poison` (None: no utterance does)"""
    return poison is not None and LENS[i] > 0 and LENS[i] % 2 == (1 if poison == "odd" else 0)


class Sweep:
    """one case: kind, name, hm (a HostModel or a HostFullModel), N, L, dense, and frames[i] = the frames of
    utterance i, left unchanged"""

    def __init__(self, G, name):
        kind, N, shape = name.split("_")
        self.kind, self.name, self.N, self.dense = kind, name, int(N), shape == "dense"
        self.L = LANES[self.N]
        rng = np.random.default_rng(4000 + 10 * (KINDS.index(kind) * len(NAMES[kind]) + NAMES[kind].index(name)))
        A = ergodic(rng, self.N) if self.dense else banded(rng, self.N)
        if kind == "diag":
            self.hm = rand_model(G, rng, self.N, M, D, A, word=name)
        else:
            self.hm = rand_fmodel(G, rng, self.N, M, D, A, spread=1.0, asym=True, word=name)
        X = walk_any(rng, self.hm, LENS)
        off = offsets(LENS)
        self.frames = [X[off[i]:off[i + 1]].copy() for i in range(U)]
        for x in self.frames:
            x.setflags(write=False)

    def corpus(self, order, poison=None):
        """(X[F][D], lens[U]) with the utterances in memory order ORDERS[order]"""
        perm = ORDERS[order]
        parts = [np.full((LENS[i], D), np.nan) if poisoned(i, poison) else self.frames[i] for i in perm]
        return np.concatenate(parts), np.array([LENS[i] for i in perm], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def make(G, name):
    """the Sweep of a name, built once"""
    return Sweep(G, name)


def by_utterance(rows, order):
    """per-frame rows [F][...] in memory order -> the list of every utterance's rows, by utterance number"""
    perm = ORDERS[order]
    off = offsets([LENS[i] for i in perm])
    out = [None] * U
    for s, i in enumerate(perm):
        out[i] = rows[off[s]:off[s + 1]]
    return out


def per_utterance(values, order):
    """a per-utterance array [U] in memory order -> by utterance number"""
    out = np.empty_like(np.asarray(values))
    out[list(ORDERS[order])] = values
    return out


def right_neighbour(order, i):
    """the non-empty utterance that follows utterance i in memory (None: the padding behind the corpus)"""
    perm = ORDERS[order]
    for j in perm[perm.index(i) + 1:]:
        if LENS[j] > 0:
            return j
    return None
