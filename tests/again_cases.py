"""The cases of the take-again path of the Baum-Welch E-step (fix_in_block inside k_scan_combine,
k_backward_fix behind k_combine, k_backward_fix behind k_backward on the vector tier) and the rule that
predicts, from the oracle's dumps alone, which utterances are taken again (GHMM_OPT_REFORDER_COUNT).
Shared by test_again_host.py, which holds the cases to the conditions under which the rule is the only
reason anything is listed, and by test_again_gpu.py.  Plain numpy and the oracle, no GPU, no tests.

The rule (`listed`): on the paired paths an utterance of T > 0 frames is listed iff the oracle's
alpha^[T-1, N-1] is not > 0 — no path into the last state, here always an utterance shorter than its
left-to-right model, a structural zero that no rounding moves.  The other reasons the kernels have (a
frame's denominator left the numbers; forward and backward mass more than 200 decades apart: a row sum
of beta^ of about 2^680 = 5e204) are kept away from every utterance that is NOT listed by `kept_margins`:
alpha^[T-1, N-1] >= 1e-100, every alpha^, beta^ and c_t finite, c_t <= 1e100, the largest row sum of
beta^ at most 1e150 (50 decades below where the kernel lists).  These are conditions on the inputs, not
measurements: a seed that fails one changes, the margin does not.

  mix16, mix32, mix64   (N, M, D) = (10, 2, 5), (20, 2, 13), (40, 1, 5): one model per group width
            (16, 32 and 64 lanes), lengths [3, 4N, N-3, 6N, 5, N-1, N, 0, 8]: 5 listed, T = N kept (its
            only path takes one frame per state), one utterance of no frames.  The listed utterances of
            8 or more frames have several non-empty chunks that all ask for the utterance: an exact
            count pins the mark that lists it once.  Variants: delta 0, 1, 2 (2: the one-launch path does
            not apply, k_combine<.., DENSE = true> on a band-diagonal A) and dense_A (nothing listed).
  many64, many32, many16   280, 540 and 1100 listed utterances (+ 20, 20, 30 that fit, spread among
            them): more than the 256, 512 and 1024 groups of k_backward_fix's grid, whose loop then runs
            a second round (GHMM_OPT_FUSED_SCAN = 2); by default fix_in_block with 16 utterances per block
            and 2 chunks each.  6 to 8 thousand frames.
  tails     for the vector tier (GHMM_OPT_KERNELS = 1), whose criterion is a non-finite band-only beta^,
            not "no path": (10, 2, 5), Gaussians sharpened x9 as fuzz_estep_case(harsh) does, lengths
            [3, 40, 7, 60] and the last 4 and the last 6 frames of an 80-frame utterance as two more
            utterances: the oracle's beta^ overflows in exactly those two.  A wave of that tier lists all
            its utterances when any of them overflows, so the count is only bounded there (`wild`);
            on the paired paths the rule gives 4.
  tails_cut utterances 0, 1 and 4 of tails (one of the two that overflow): the vector tier's history.
  small     the first four utterances of mix16 ([3, 40, 7, 60], 2 listed): what a context has seen
            before a larger corpus arrives."""
import numpy as np

import oracle_lib as O
from streams_util import synth_case

WAVE = 64
FIX_BLOCKS = 256            # GHMM_FIX_BLOCKS: k_backward_fix's grid is at most this many blocks

SHAPES = {"mix16": (10, 2, 5), "mix32": (20, 2, 13), "mix64": (40, 1, 5),
          "many16": (10, 2, 5), "many32": (20, 2, 13), "many64": (40, 1, 5),
          "tails": (10, 2, 5), "tails_cut": (10, 2, 5), "small": (10, 2, 5)}
MIX = ("mix16", "mix32", "mix64")
MANY = ("many64", "many32", "many16")
#         name: (listed, fitting, lengths of the listed ones cycle through, of the fitting ones)
MANY_PLAN = {"many64": (280, 20, (8, 39), (40, 60)),
             "many32": (540, 20, (4, 19), (20, 60)),
             "many16": (1100, 30, (1, 9), (12, 40))}
# (delta, dense_A) of every mix* variant and what the rule gives there
MIX_VARIANTS = ((0, False), (1, False), (2, False), (1, True))
EXPECTED = {"mix16": 5, "mix32": 5, "mix64": 5, "many64": 280, "many32": 540, "many16": 1100, "tails": 4,
            "tails_cut": 2, "small": 2}


def mix_lens(N):
    return [3, 4 * N, N - 3, 6 * N, 5, N - 1, N, 0, 8]


def many_lens(name):
    """the fitting utterances at even distances among the listed ones"""
    n_short, n_fit, (s0, s1), (f0, f1) = MANY_PLAN[name]
    every = n_short // n_fit
    lens, k = [], 0
    for i in range(n_short):
        lens.append(s0 + i % (s1 - s0 + 1))
        if i % every == every - 1 and k < n_fit:
            lens.append(f0 + (7 * k) % (f1 - f0 + 1))
            k += 1
    assert k == n_fit and len(lens) == n_short + n_fit
    return lens


class Case:
    """hm, X, lens of one case, its name and the band the E-step runs with"""

    def __init__(self, name, hm, X, lens, delta=1, dense=False):
        self.name, self.hm, self.X, self.delta, self.dense = name, hm, np.ascontiguousarray(X), delta, dense
        self.lens = np.asarray(lens, dtype=np.int32)
        self.N, self.M, self.D = hm.N, hm.M, hm.D
        self.U, self.F = len(self.lens), int(self.lens.sum())
        self._ref = None

    def ref(self):
        """(statistics, dumps) of oracle_lib.estep, computed once"""
        if self._ref is None:
            self._ref = O.estep(self.hm, self.X, self.lens, delta=self.delta)
        return self._ref

    @property
    def tag(self):
        return f"{self.name} delta={self.delta} dense={self.dense}"


_made = {}


def make(G, name, delta=1, dense=False):
    """the case `name` (one object per variant: its oracle run is shared by every test)"""
    key = (name, delta, dense)
    if key in _made:
        return _made[key]
    N, M, D = SHAPES[name]
    if name in MIX:
        hm, X, lens = synth_case(G, N, M, D, mix_lens(N), dense_A=dense)
    elif name in MANY:
        hm, X, lens = synth_case(G, N, M, D, many_lens(name))
    elif name == "small":
        hm, X, lens = synth_case(G, N, M, D, mix_lens(N)[:4])
    else:
        hm, X, lens = synth_case(G, N, M, D, [3, 40, 7, 60, 80])
        hm.inv_var *= 9.0
        hm.det /= 9.0 ** D
        o = offsets(lens)
        long_one = X[o[4]:o[5]]
        if name == "tails":
            X = np.concatenate([X[:o[4]], long_one[-4:], long_one[-6:]])
            lens = np.array([3, 40, 7, 60, 4, 6], dtype=np.int32)
        else:
            X = np.concatenate([X[:o[2]], long_one[-4:]])
            lens = np.array([3, 40, 4], dtype=np.int32)
    assert dense is False or name in MIX
    _made[key] = Case(name, hm, X, lens, delta, dense)
    return _made[key]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def listed_mask(case):
    """per utterance: is it taken again on the paired paths?  From the oracle's dumps alone."""
    _, d = case.ref()
    o = offsets(case.lens)
    return np.array([T > 0 and not d["alpha"][o[u] + T - 1, case.N - 1] > 0.0
                     for u, T in enumerate(case.lens)], dtype=bool)


def listed(case):
    return int(listed_mask(case).sum())


def wild_mask(case):
    """per utterance: is the oracle's beta^ non-finite somewhere?  (the vector tier's criterion)"""
    _, d = case.ref()
    o = offsets(case.lens)
    return np.array([not np.all(np.isfinite(d["beta"][o[u]:o[u + 1]])) for u in range(case.U)], dtype=bool)


def kept_margins(case, mask):
    """over the utterances of `mask` (those NOT listed): (the smallest alpha^[T-1, N-1], are all of
    alpha^, beta^ and c_t finite, the largest c_t, the largest row sum of beta^).  An utterance of no
    frames has nothing to hold."""
    _, d = case.ref()
    o = offsets(case.lens)
    amin, finite, cmax, bmax = np.inf, True, 0.0, 0.0
    for u in np.nonzero(mask)[0]:
        T = int(case.lens[u])
        if T == 0:
            continue
        a, b, c = (d[k][o[u]:o[u + 1]] for k in ("alpha", "beta", "scale"))
        amin = min(amin, float(a[T - 1, case.N - 1]))
        finite = finite and bool(np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all())
        cmax = max(cmax, float(c.max()))
        bmax = max(bmax, float(b.sum(axis=1).max()))
    return amin, finite, cmax, bmax


# ---- the host's grid of k_backward_fix (run_backward_fix), restated

def lanes(N):
    return 16 if N <= 16 else 32 if N <= 32 else 64


def fix_grid(N, U):
    """(blocks, groups per block): min(ceil(U / gpw), GHMM_FIX_BLOCKS) blocks of WAVE / L groups; group g
    of the grid takes list entries g, g + groups, g + 2 groups, ..."""
    gpw = WAVE // lanes(N)
    return min((U + gpw - 1) // gpw, FIX_BLOCKS), gpw


def fix_groups(N, U):
    blocks, gpw = fix_grid(N, U)
    return blocks * gpw


def scan_upb(N, U, F):
    """(utterances per block, chunks per utterance) of k_scan_combine's launch (run_scan_combine)"""
    gpw, upb = WAVE // lanes(N), 4
    tmean = F // U
    want = 4 if tmean >= 160 else 8 if tmean >= 80 else 16
    while upb < want and 2 * (2 * upb) // gpw <= 8:
        upb *= 2
    return upb, 32 // upb
