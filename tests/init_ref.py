"""The diagonal trainer's initial model (creating_initial_model, TF:732-1317) restated in numpy, and the
corpora the initial-model tests run on.  No tests; pytest does not collect this file.

init_diag() is csrc/ghmm_init.c ghmm_init_cells_ followed by ghmm_init_model's variance and weight part, in
the host's loop order, with a float type parameter; the segmentation, the sort, the split, the classification
and the corpus generator are fullinit_ref's (the two trainers share ghmm_init_cells_).  What differs from
init_full: both split kinds multiply by (1.005, 0.995), a level takes 3 passes, the variances are diagonal
(floored at 1e-5, det = their product in coefficient order, then inverted; a state without frames gives NaN
throughout, det included).  With ft = float64 the result is ghmm_init_model's bit for bit (test_init_host
pins that); with ft = np.longdouble it is the accuracy reference.

Besides the model it returns
  assign, gaps   per classification pass (the k-means passes in order, then the variance pass) every frame's
                 cell and the relative gap between its nearest and second-nearest cell, as init_full does
  orders         one record per place where the sort of a state's distortions is CONSUMED: the
                 largest-distortion split (kind "split", the first M - n sorted cells are split) and a re-seed
                 when at least one cell of the state is empty (kind "reseed", one sorted cell per empty cell).
                 Each holds level (cells per state at that point), pass (None for a split), state, taken (the
                 cells consumed, in order) and gap: with k cells consumed of n, the smallest relative gap
                 (d[i] - d[i+1]) / d[i] over the sorted pairs i < min(k, n - 1), the pairs that decide which
                 cells are the first k and in which order (1 when there is no such pair; a pair of two
                 empty cells, 0 and 0 in any arithmetic, stays in index order and is passed over; so is a state
                 without frames, whose cells are 0/0 whichever seeds which)
  reseeds        (level, pass, state, empty cell, cell it was seeded from) per re-seed, in order

no_candidate: what a frame farther than 1e20 from every cell of its state is given.  "carry" is the host's
rule (the previous frame's cell in file order, and 1e20 added to that cell's distortion); "zero" is the
device's (k_init_classify starts every frame at cell 0, and the statistics kernel adds the frame's true
distance to cell 0).  The two differ only when some frame lies at least 1e10 from every cell of its state.

A corpus is ADMITTED when in the float64 run every classification gap is >= 1e-9 (fullinit_ref.MIN_GAP),
every consumed order's gap is >= 1e-6 (ORDER_GAP), and the long-double run makes the same assignments and
consumes the same cells in the same order.  The 1e-6 is a condition set five orders above the ~5e-12 that
the matrix-core tier's expanded-form sums are documented to hold (ghmm_mfma.hpp COND_MAX), not a
measurement.  An implementation that adds the same terms in another order then makes the same assignments
and splits, and its model differs from the host's by rounding only.

CASES beyond fullinit_ref's (all of which are admitted for this algorithm too), and what each is there for
(k_init_classify takes FR = 64 frames per block, 256 threads; k_init_cells holds at most 64 cells per state;
the matrix-core statistics kernel takes the frames 16 at a time):
  m6       the split takes 2 of 4 cells by distortion
  m12      the split takes 4 of 8 cells by distortion
  m16      four doublings
  m64      the device bookkeeping's cap: all of k_init_cells' dist[] / idx[]
  m65      the host loop of ghmm_model_init_comm (M > 64), with a 1-of-64 split by distortion
  d64      last D of the matrix-core tier
  d65      first D where the model has no matrix-core form
  d300     FR = 16, and the frame copy loop with 256 / D = 0
  d39m8    the benchmark's own M and D
  g264     N M = 264 > 256: the posterior-row writer with 256 / (N M) = 0
  n300     N = 300 > 256: the gamma-row writer with 256 / N = 0; T % N != 0
  f9       F = 9 < 16: no whole matrix-core step
  f15      F = 15, T = 7 and 8 with N = 3; one partial classify block
  reseed, reseed_last
           a cell of a state that has frames runs empty during the k-means passes and is re-seeded (the shape
           and seed came out of a seeded search over clouds(seed, N, 2, D, lens, noise) with 2..5 frames per
           cell); reseed twice, the second time at the last level; reseed_last in the very last k-means pass
  tie      an exact tie, see below

tie cannot be admitted (its gap is 0) and is exempt from the condition.  The nearest-cell rule's strict `<`
(the lowest cell wins a tie) only shows on an exact tie, and rounding must not be able to break it: state 1's
frames are small integers v, -v in pairs.  Their sums are exact in any order and in either arithmetic, so the
state's mean is exactly 0 in every coefficient, the split gives two cells of 0, and every frame of the state
is equally far from both in every pass: cell 0 takes them all, cell 1 stays empty, is re-seeded after every
pass (from cell 0: 0 again) and ends with count 0, a NaN variance and the floored weight.  That holds for any
implementation that sums the frames themselves (the host; the device's vector-ALU statistics kernel, where
the GPU test runs it), bit for bit; the matrix-core tier sums the frames around an offset, which need not be
exact, so the case is not run there."""
import functools

import numpy as np

import fullinit_ref as F
from fullinit_ref import _classify, _split, clouds, order_desc, segmentation

SPLIT = (1.005, 0.995)     # TF:1138, both split kinds and the re-seeding
PASSES = 3                 # TF:1043
FLOOR = 1.0e-5             # TF:39
FAR = F.FAR
MIN_GAP = F.MIN_GAP
ORDER_GAP = 1e-6


def _order_gap(key, idx, k):
    """the smallest relative gap over the sorted pairs that decide the first k entries of idx"""
    g = 1.0
    for i in range(min(k, len(idx) - 1)):
        a, b = key[idx[i]], key[idx[i + 1]]
        if np.isnan(a) or np.isnan(b):
            return 0.0
        if a == 0 and b == 0:   # two empty cells: an empty sum is 0 in any arithmetic, the stable sort
            continue            # keeps them in index order
        g = min(g, float((a - b) / a) if a > 0 else 0.0)
    return g


def _classify_rule(X, state, cells, n, ft, no_candidate):
    """fullinit_ref._classify under either no-candidate rule: (cell, distance added to the cell's
    distortion, gap)"""
    cell, best, gap = _classify(X, state, cells, n, ft)
    if no_candidate == "zero":
        none = np.nonzero(best >= ft(FAR))[0]
        cell[none] = 0
        for t in none:
            d = ft(0.0)
            for j in range(X.shape[1]):
                a = cells[state[t], 0, j] - X[t, j]
                d = d + a * a
            best[t] = d
    return cell, best, gap


def init_diag(X, lens, N, M, ft=np.float64, no_candidate="carry"):
    """dict(A, c, mean, inv_var, det, count [N, M] of the variance pass, dur [N], state, assign, gaps, orders,
    reseeds)"""
    assert no_candidate in ("carry", "zero")
    X = np.asarray(X, dtype=np.float64).astype(ft)
    nF, D = X.shape
    state = segmentation(lens, N)
    assert state.size == nF
    delta = 1
    A = np.zeros((N, N), dtype=np.float64)
    for i in range(N):
        for j in range(N):
            if j > delta + i or j < i:
                continue
            A[i, j] = 1.0 / (N - i) if delta + 1 > N - i else 1.0 / (delta + 1)
    assign, gaps, orders, reseeds = [], [], [], []
    with np.errstate(all="ignore"):
        cells = np.zeros((N, M, D), dtype=ft)
        count = np.zeros((N, M), dtype=np.int64)
        dist = np.zeros((N, M), dtype=ft)
        np.add.at(cells[:, 0], state, X)
        np.add.at(count[:, 0], state, 1)
        cells[:, 0] = cells[:, 0] / count[:, 0].astype(ft)[:, None]
        n = 1
        while n < M:
            for k in range(N):
                if 2 * n < M:
                    for i in range(n):
                        _split(cells[k], i, n + i, *SPLIT, ft)
                else:
                    idx = order_desc(dist[k], n)
                    orders.append(dict(kind="split", level=n, **{"pass": None}, state=k, taken=idx[:M - n],
                                       gap=_order_gap(dist[k], idx, M - n)))
                    for i in range(M - n):
                        _split(cells[k], idx[i], n + i, *SPLIT, ft)
            n = 2 * n if 2 * n < M else M
            for p in range(PASSES):
                cell, best, gap = _classify_rule(X, state, cells, n, ft, no_candidate)
                assign.append(cell)
                gaps.append(gap)
                count[:, :n] = 0
                dist[:, :n] = 0
                total = np.zeros((N, M, D), dtype=ft)
                np.add.at(dist, (state, cell), best)
                np.add.at(count, (state, cell), 1)
                np.add.at(total, (state, cell), X)
                for k in range(N):
                    cells[k, :n] = total[k, :n] / count[k, :n].astype(ft)[:, None]
                    idx = order_desc(dist[k], n)
                    empty = [j for j in range(n) if count[k, j] == 0]
                    if empty:   # (a state without frames: every cell is 0/0 whichever cell seeds it, gap 1)
                        g = _order_gap(dist[k], idx, len(empty)) if len(empty) < n else 1.0
                        orders.append(dict(kind="reseed", level=n, **{"pass": p}, state=k, taken=idx[:len(empty)],
                                           gap=g))
                    for i, j in enumerate(empty):
                        reseeds.append((n, p, k, j, idx[i]))
                        _split(cells[k], idx[i], j, *SPLIT, ft)
        # the variances and the weights (ghmm_init_model)
        cell, _, gap = _classify_rule(X, state, cells, M, ft, no_candidate)
        assign.append(cell)
        gaps.append(gap)
        dif = X - cells[state, cell]
        var = np.zeros((N, M, D), dtype=ft)
        np.add.at(var, (state, cell), dif * dif)
        count = np.zeros((N, M), dtype=np.int64)
        np.add.at(count, (state, cell), 1)
        dur = np.zeros(N, dtype=np.int64)
        np.add.at(dur, state, 1)
        var = var / count.astype(ft)[:, :, None]
        var[var < ft(FLOOR)] = ft(FLOOR)
        det = np.ones((N, M), dtype=ft)
        for l in range(D):
            det = det * var[:, :, l]
        inv_var = ft(1.0) / var
        c = count.astype(ft) / dur.astype(ft)[:, None]
        for k in range(N):
            c[k][c[k] < ft(FLOOR)] = ft(FLOOR)
            s = ft(0.0)
            for m in range(M):
                s = s + c[k, m]
            c[k] = c[k] / s
    return dict(A=A, c=c, mean=cells, inv_var=inv_var, det=det, count=count, dur=dur, state=state,
                assign=assign, gaps=gaps, orders=orders, reseeds=reseeds)


# ------------------------------------------------------------- the corpora

# name: (N, M, D, lens, seed for clouds)
_SHAPES = {
    "m6": (2, 6, 4, [151, 147, 135], 21),
    "m12": (2, 12, 5, [301, 287, 275], 22),
    "m16": (2, 16, 6, [400, 431, 387], 40),
    "m64": (1, 64, 3, [900, 857], 38),
    "m65": (1, 65, 4, [1500, 1457], 39),
    "d64": (2, 3, 64, [130, 121, 77], 25),
    "d65": (2, 2, 65, [130, 121], 24),
    "d300": (2, 2, 300, [70, 65], 31),
    "d39m8": (3, 8, 39, [200, 231, 187, 155], 26),
    "g264": (33, 8, 3, [1325, 1337, 1255, 1355], 33),
    "n300": (300, 2, 2, [3001, 4555, 2999], 35),
    "f9": (2, 2, 3, [9], 36),
    "f15": (3, 2, 3, [7, 8], 37),
}
# a cell runs empty: few frames per cell around two centres per state (N, M, D, lens, seed, noise)
_RESEED = {
    "reseed": (3, 5, 2, [19, 15], 781, 0.2),        # state 2: in pass 1 of the 4-cell level, in pass 0 of the last
    "reseed_last": (2, 3, 3, [16, 12], 395, 0.6),   # state 1: in the last pass before the variance pass
}
ADMITTED = sorted(F._SHAPES) + sorted(_SHAPES) + sorted(_RESEED)
CASES = ADMITTED + ["tie"]
# the k cells that the case's largest-distortion splits take, of how many
SPLITS_BY_DISTORTION = {"m3": (1, 2), "m5": (1, 4), "m7": (3, 4), "m6": (2, 4), "m12": (4, 8), "m65": (1, 64)}


_TIE_LENS = [24, 20]


def _tie():
    """N = 2, M = 2, D = 2: state 0 a cloud, state 1 small integers v, -v in pairs"""
    X = clouds(78, 2, 2, 2, _TIE_LENS)
    state = segmentation(_TIE_LENS, 2)
    f = np.nonzero(state == 1)[0]
    v = np.random.default_rng(79).integers(1, 8, (f.size // 2, 2)).astype(np.float64)
    X[f[0::2]], X[f[1::2]] = v, -v
    return X


@functools.lru_cache(maxsize=None)
def corpus(name):
    """(X, lens, N, M)"""
    if name in F._SHAPES:
        return F.corpus(name)
    if name in _RESEED:
        N, M, D, lens, seed, noise = _RESEED[name]
        return clouds(seed, N, 2, D, lens, noise), np.array(lens, dtype=np.int32), N, M
    if name == "tie":
        return _tie(), np.array(_TIE_LENS, dtype=np.int32), 2, 2
    N, M, D, lens, seed = _SHAPES[name]
    return clouds(seed, N, M, D, lens), np.array(lens, dtype=np.int32), N, M


@functools.lru_cache(maxsize=None)
def reference(name, extended):
    """init_diag on the case, in long double (extended) or float64; computed once, shared, not to be
    modified"""
    X, lens, N, M = corpus(name)
    return init_diag(X, lens, N, M, np.longdouble if extended else np.float64)


def min_gap(ref):
    return min((float(g.min()) for g in ref["gaps"] if g.size), default=1.0)


def min_order_gap(ref):
    return min((o["gap"] for o in ref["orders"]), default=1.0)


def same_decisions(a, b):
    """two runs assign every frame alike in every pass and consume the same cells in the same order"""
    return len(a["assign"]) == len(b["assign"]) and all(np.array_equal(x, y) for x, y in zip(a["assign"], b["assign"])) \
        and [(o["kind"], o["level"], o["pass"], o["state"], o["taken"]) for o in a["orders"]] == \
            [(o["kind"], o["level"], o["pass"], o["state"], o["taken"]) for o in b["orders"]] \
        and a["reseeds"] == b["reseeds"] and np.array_equal(a["count"], b["count"])


# ------------------------------------------------------------- no candidate within 1e20

@functools.lru_cache(maxsize=None)
def far_corpus():
    """m3's corpus with coefficient 0 of one frame at 1e11: the first frame t for which the host's rule then
    leaves the frame before it, and so t itself, in a cell != 0 in the last pass: (X, lens, N, M, t)"""
    X0, lens, N, M = corpus("m3")
    for t in range(1, len(X0)):
        X = X0.copy()
        X[t, 0] = 1.0e11
        last = init_diag(X, lens, N, M)["assign"][-1]
        if last[t - 1] != 0 and last[t] != 0:
            return X, lens, N, M, t
    raise AssertionError("no frame of m3 qualifies")


@functools.lru_cache(maxsize=None)
def far_reference(rule, extended=False):
    X, lens, N, M, _ = far_corpus()
    return init_diag(X, lens, N, M, np.longdouble if extended else np.float64, no_candidate=rule)
