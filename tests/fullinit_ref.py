"""The full-covariance trainer's initial model (creating_initial_model, TFF:731-1134) restated in numpy,
and the corpora the initial-model tests run on.  No tests; pytest does not collect this file.

init_full() is csrc/ghmm_init.c ghmm_init_cells_ followed by csrc/ghmm_fulltrain.c ghmm_init_model_full's
init_mix_param, in the host's loop order, with a float type parameter.  Every sum the host takes serially
is taken serially here (np.add.at adds in index order; the distance and the inverse's k sums are python
loops), numpy contracts nothing, so with ft = float64 the result is ghmm_init_model_full's bit for bit
(test_fullinit_host pins that); with ft = np.longdouble it is the accuracy reference.  Besides the model
it returns, per classification pass (the k-means passes in order, then init_mix_param's), every frame's
cell and the relative gap (d2 - d1) / d2 between its nearest and second-nearest cell (1 where there is
no second finite distance).

A corpus is ADMITTED when in the float64 run every frame of every pass has a gap >= 1e-9 and the long
double run makes the same assignments: then an implementation that adds the same terms in another order
must make the same assignments too, and its cells differ from the host's by rounding only.

CASES, and what each is there for (the device's k_finit_pass stages 64 frames at a time and gives a
block state k's runs of ceil(U / min(U, ceil(4 CUs / N))) utterances; 256 CUs):
  n1            N = 1: one run per utterance, the whole corpus in one state
  m1            M = 1: no k-means pass, the covariance around the state's mean
  m2, m4        doubling splits only (M = 2 takes the largest-distortion branch on one cell)
  m3, m5, m7    the largest-distortion split after the doubling
  d1            D = 1: det = var, inverse = 1 / var
  d9            D = 9 (odd: the LDS rows are D | 1 = D apart)
  d48           D = 48 with N x M = 2 x 2: the widest rows, and the 38 KB of LDS of the finishing kernel
  n64           N = 64, M = 1, 40 utterances of 65..91 frames: 14 utterance ranges of 3 utterances per state
                (the last holds 1), T % N != 0 throughout
  u1            U = 1, T = 500, N = 3: runs of 167, 167, 166 frames = three stages each, the last partial;
                one block per state adds the frames in the host's order, so the cells are the host's bits
  ragged        23 utterances of unequal length with T % N != 0
  long          4 utterances of 300..420 frames, N = 2: every run spans 3 or 4 stages and ends inside one
  short         every utterance shorter than N = 6: the last state owns no frame (0/0 values), state 4 few
  fewdistinct   a state with two distinct frames and M = 3: see below

fewdistinct cannot be admitted, by construction, and is the one case exempt from the condition.  With
fewer distinct frames than cells some cell holds copies of one frame only when the last level opens
(the cells that hold two values number at most `distinct - n` < M - n, the cells split), and a cell p
that equals its frames is split into 1.005 p and 0.995 p, both |0.005 p| away: a tie up to the rounding
of the two products, gap ~1e-13, whatever the frames are.  It is built with U = 1, where the device adds
every state's frames in one block in the host's order: its k-means sums, hence its cells, distances and
assignments, are the host's BIT FOR BIT, ties included, which the GPU test asserts for this case (and
for u1) instead of relying on the condition."""
import functools

import numpy as np

SPLIT1 = (1.05, 0.95)      # TFF:1176-1177, the doubling split
SPLIT2 = (1.005, 0.995)    # the split of the cells of largest distortion, and the re-seeding
PASSES = 5                 # TFF:1073
FLOOR = 1.0e-5             # TFF:38
FAR = 1.0e20               # TFF:1179-1215
MIN_GAP = 1e-9


def segmentation(lens, N):
    """state of every frame under the uniform segmentation (TFF:1005-1013)"""
    out = []
    for T in lens:
        q, r = divmod(int(T), N)
        out.append(np.repeat(np.arange(N), [q + 1 if k < r else q for k in range(N)]))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def order_desc(key, n):
    """sorting (TFF:1331-1356): adjacent swaps, strict <"""
    idx = list(range(n))
    done = False
    while not done:
        done = True
        for i in range(n - 1):
            if key[idx[i]] < key[idx[i + 1]]:
                idx[i], idx[i + 1] = idx[i + 1], idx[i]
                done = False
    return idx


def _split(ck, frm, to, up, down, ft):
    ck[to] = ck[frm] * ft(up)
    ck[frm] = ck[frm] * ft(down)      # (frm == to: the product above, scaled again, as on the host)


def _classify(X, state, cells, n_cells, ft):
    """ghmm_nearest_ for every frame, the cell index carried over the frames in file order; returns
    (cell, best distance, gap)"""
    F, D = X.shape
    cell = np.full(F, -1, dtype=np.int64)
    best = np.full(F, ft(FAR), dtype=ft)
    gap = np.ones(F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(cells.shape[0]):
            f = np.nonzero(state == k)[0]
            if f.size == 0:
                continue
            dist = np.zeros((f.size, n_cells), dtype=ft)
            for j in range(D):
                a = cells[k, :n_cells, j][None, :] - X[f, j][:, None]
                dist += a * a
            b, c = best[f], cell[f]
            for i in range(n_cells):
                m = dist[:, i] < b
                b[m] = dist[m, i]
                c[m] = i
            best[f], cell[f] = b, c
            if n_cells > 1:
                srt = np.sort(np.where(np.isnan(dist), np.inf, dist), axis=1)
                d1, d2 = srt[:, 0], srt[:, 1]
                ok = np.isfinite(d2) & (d2 > 0)
                g = np.ones(f.size)
                g[ok] = ((d2[ok] - d1[ok]) / d2[ok]).astype(np.float64)
                g[np.isfinite(d2) & (d2 == 0)] = 0.0
                gap[f] = g
    prev = 0
    for t in range(F):          # a frame farther than 1e20 from every cell keeps the previous frame's
        if cell[t] < 0:
            cell[t] = prev
        prev = cell[t]
    return cell, best, gap


def inv_cov(cov, ft):
    """inv_cov_matrix (TFF:2058-2202) on a D x D matrix of type ft, D > 1: (det, matrix slot)"""
    D = cov.shape[0]
    with np.errstate(all="ignore"):
        d = np.zeros(D, dtype=ft)
        t = np.eye(D, dtype=ft)
        d[0] = cov[0, 0]
        t[1:, 0] = cov[1:, 0] / d[0]
        for j in range(1, D):
            s = cov[j, j]
            for k in range(j):
                s = s - t[j, k] * t[j, k] * d[k]
            d[j] = s
            if j < D - 1:
                v = cov[j + 1:, j].copy()
                for k in range(j):
                    v = v - t[j + 1:, k] * d[k] * t[j, k]
                t[j + 1:, j] = v / d[j]
        det = ft(1.0)
        for k in range(D):
            det = det * d[k]
        if np.isnan(det):
            det = ft(0.0)
        if det == 0:
            return det, cov
        im = np.eye(D, dtype=ft)
        for k in range(D - 1):
            i = np.arange(k + 1, D)
            j = i - k - 1
            s = np.zeros(i.size, dtype=ft)
            for l in range(k + 1):
                s = s - t[i, j + l] * im[j + l, j]
            im[i, j] = s
        out = np.zeros((D, D), dtype=ft)
        iu = np.triu_indices(D)
        for k in range(D):
            m = iu[1] <= k
            a, b = iu[0][m], iu[1][m]
            out[a, b] = out[a, b] + im[k, a] * im[k, b] / d[k]
        out[iu[1], iu[0]] = out[iu[0], iu[1]]
        return det, out


def init_full(X, lens, N, M, ft=np.float64):
    """dict(A, c, mean, inv_cov, det, count [N, M] of init_mix_param's pass, assign = [cell per frame]
    per pass, gaps = [gap per frame] per pass, state = the frames' states)"""
    X = np.asarray(X, dtype=np.float64).astype(ft)
    F, D = X.shape
    state = segmentation(lens, N)
    assert state.size == F
    delta = 1
    A = np.zeros((N, N), dtype=np.float64)
    for i in range(N):
        for j in range(N):
            if j > delta + i or j < i:
                continue
            A[i, j] = 1.0 / (N - i) if delta + 1 > N - i else 1.0 / (delta + 1)
    assign, gaps = [], []
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
                        _split(cells[k], i, n + i, *SPLIT1, ft)
                else:
                    idx = order_desc(dist[k], n)
                    for i in range(M - n):
                        _split(cells[k], idx[i], n + i, *SPLIT2, ft)
            n = 2 * n if 2 * n < M else M
            for _ in range(PASSES):
                cell, best, gap = _classify(X, state, cells, n, ft)
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
                    i = 0
                    for j in range(n):
                        if count[k, j] == 0:
                            _split(cells[k], idx[i], j, *SPLIT2, ft)
                            i += 1
        # init_mix_param
        cell, _, gap = _classify(X, state, cells, M, ft)
        assign.append(cell)
        gaps.append(gap)
        dif = X - cells[state, cell]
        cov = np.zeros((N, M, D, D), dtype=ft)
        np.add.at(cov, (state, cell), dif[:, :, None] * dif[:, None, :])
        count = np.zeros((N, M), dtype=np.int64)
        np.add.at(count, (state, cell), 1)
        dur = np.zeros(N, dtype=np.int64)
        np.add.at(dur, state, 1)
        det = np.zeros((N, M), dtype=ft)
        iu = np.triu_indices(D)
        for k in range(N):
            for m in range(M):
                cv = np.zeros((D, D), dtype=ft)
                cv[iu] = cov[k, m][iu] / ft(count[k, m])
                dg = np.arange(D)
                low = cv[dg, dg] < ft(FLOOR)
                cv[dg[low], dg[low]] = ft(FLOOR)
                cv[iu[1], iu[0]] = cv[iu]
                if D > 1:
                    det[k, m], cov[k, m] = inv_cov(cv, ft)
                else:
                    det[k, m] = cv[0, 0]
                    cov[k, m] = ft(1.0) / cv
        c = count.astype(ft) / dur.astype(ft)[:, None]
        for k in range(N):
            c[k][c[k] < ft(FLOOR)] = ft(FLOOR)
            s = ft(0.0)
            for m in range(M):
                s = s + c[k, m]
            c[k] = c[k] / s
    return dict(A=A, c=c, mean=cells, inv_cov=cov, det=det, count=count, assign=assign, gaps=gaps, state=state)


# ------------------------------------------------------------- the corpora

def clouds(seed, N, M, D, lens, noise=0.4):
    """frames around max(M, 2) centres per state (the state is the uniform segmentation's), every
    coefficient offset by 6 so that no mean sits near 0, where the multiplicative splits would not
    separate the cells"""
    rng = np.random.default_rng(seed)
    K = max(M, 2)
    centres = 6.0 + rng.normal(0.0, 2.0, (N, K, D))
    state = segmentation(lens, N)
    pick = rng.integers(0, K, state.size)
    return centres[state, pick] + rng.normal(0.0, noise, (state.size, D))


def _few_distinct():
    """N = 2, M = 3, D = 2, one utterance of 96 frames: state 0 a cloud, state 1 copies of two frames"""
    N, M, D, lens = 2, 3, 2, [96]
    X = clouds(77, N, M, D, lens)
    p, q = np.array([5.25, 7.5]), np.array([8.75, 4.5])
    X[48:] = np.where((np.arange(48) % 3 == 0)[:, None], p, q)
    return X


# name: (N, M, D, lens, seed)
_SHAPES = {
    "n1": (1, 4, 5, [40, 33, 51], 1),
    "m1": (4, 1, 6, [37, 45, 29, 50], 2),
    "m2": (3, 2, 6, [61, 47, 55, 70], 3),
    "m4": (3, 4, 6, [91, 77, 85, 100], 4),
    "m3": (3, 3, 6, [61, 77, 85, 70], 5),
    "m5": (2, 5, 4, [121, 97, 135], 6),
    "m7": (2, 7, 4, [151, 147, 135], 7),
    "d1": (3, 3, 1, [70, 65, 81, 59], 8),
    "d9": (3, 2, 9, [50, 65, 41, 59], 9),
    "d48": (2, 2, 48, [130, 121], 10),
    "n64": (64, 1, 3, [65 + (7 * u + 3) % 27 for u in range(40)], 11),
    "u1": (3, 4, 5, [500], 12),
    "ragged": (5, 3, 4, [31 + (11 * u + 2) % 24 + (1 if (31 + (11 * u + 2) % 24) % 5 == 0 else 0)
                         for u in range(23)], 13),
    "long": (2, 4, 7, [301, 419, 363, 385], 14),
    "short": (6, 2, 3, [3 + (u * 7) % 3 for u in range(60)], 15),
}
CASES = sorted(_SHAPES) + ["fewdistinct"]
ADMITTED = sorted(_SHAPES)
BIT_EQUAL_CELLS = ["u1", "fewdistinct"]     # U = 1: the device adds the frames in the host's order


@functools.lru_cache(maxsize=None)
def corpus(name):
    """(X, lens, N, M)"""
    if name == "fewdistinct":
        return _few_distinct(), np.array([96], dtype=np.int32), 2, 3
    N, M, D, lens, seed = _SHAPES[name]
    return clouds(seed, N, M, D, lens), np.array(lens, dtype=np.int32), N, M


@functools.lru_cache(maxsize=None)
def reference(name, extended):
    """init_full on the case, in long double (extended) or float64; computed once, shared, not to be
    modified"""
    X, lens, N, M = corpus(name)
    return init_full(X, lens, N, M, np.longdouble if extended else np.float64)


def min_gap(ref):
    return min((float(g.min()) for g in ref["gaps"] if g.size), default=1.0)
