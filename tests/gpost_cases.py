"""The word posteriors under a word-pair grammar (ghmm_grammar_post_streams, ghmm_grammar_post_full_streams;
k_gpost_fwd / k_gpost_bwd): a numpy restatement of the definition in include/ghmm.h in a chosen float type,
per utterance on a given log b, and an enumeration of every composite path that the definition sums over.
The vocabularies, utterances and grammars are grammar_cases' and connect_cases', imported unchanged.  Shared
by test_gpost_host.py, which checks on the CPU that the restatement is the definition and that consequences
(a) to (e) of the header hold on it, and by test_gpost_gpu.py, which compares the device with the long-double
restatement run on the device's own log b.  Plain numpy and the oracle, no GPU, no tests.

The float64 restatement's distance from the long-double one on the oracle's log b, per (case, grammar) that
test_gpost_gpu.py compares (estep_log_ref.block_dist over gamma, occ and ent; relative over finite log P),
as test_gpost_host.test_float64_spread prints it; the bar is fullcov_support.RTOL / 8 = 1.25e-9:
    narrow  random 1.2e-12 | norepeat 1.0e-12 | flat:-5 1.0e-12      log P at most 5.8e-16
    ones    random 1.6e-14 | norepeat 1.7e-14                        log P at most 1.6e-16
    thick   random 2.3e-13 | norepeat 2.0e-13 | flat:-5 2.5e-13      log P at most 2.0e-16
    k72     random 2.4e-14 | norepeat 1.8e-14 | flat:-5 2.4e-14      log P at most 2.1e-16
    k100    random 2.2e-14 | norepeat 1.7e-14 | flat:-5 2.5e-14      log P at most 2.3e-16
    k256    random 1.7e-14 | norepeat 2.2e-14 | flat:-5 2.9e-14      log P at most 1.3e-16
    full    random 1.9e-13 | norepeat 1.9e-13                        log P at most 9.0e-17
    holes   random 0       | norepeat 0          (every log P is NaN or the utterance is empty: zero rows)
No case needed another seed or a shorter utterance."""
import numpy as np

import connect_cases as CC
import grammar_cases as GC
from embed_cases import _lse, _lse2
from fullcov_support import need_extended, offsets

# the (case, grammars) that test_gpost_gpu.py compares with the long-double restatement; cap is compared
# with the float64 one alone (32 words of 64 states per frame in long double are the restatement's cost)
GPU_GRAMMARS = {"narrow": ("random", "norepeat", "flat:-5"), "ones": ("random", "norepeat"),
                "thick": ("random", "norepeat", "flat:-5"), "k72": ("random", "norepeat", "flat:-5"),
                "k100": ("random", "norepeat", "flat:-5"), "k256": ("random", "norepeat", "flat:-5"),
                "full": ("random", "norepeat"), "holes": ("random", "norepeat")}
CAP_GRAMMARS = ("random", "norepeat")
SPREAD_CASES = tuple(GPU_GRAMMARS)


def lattice(As, logb, start, pair, fin, ft=np.longdouble):
    """One utterance: the definition on logb[T][NS] (word k's columns in order) and the words' A under the
    grammar (start and fin may be None: zeros), the words padded to the largest with states of -inf.  Returns
    a dict: T, logP, gamma [T][NS], occ [T][K], ent [T][K] (zero rows where logP is not finite), and for the
    tests that look inside la, lbe [T][K][Nm], x [T][K] (row 0 unused) and the real-state mask [K][Nm]."""
    if ft is np.longdouble:
        need_extended()
    K, T = len(As), len(logb)
    Ns = np.array([np.asarray(A).shape[0] for A in As])
    NS, Nm = int(Ns.sum()), int(Ns.max())
    ninf = ft(-np.inf)
    if T == 0:
        return {"T": 0, "logP": ft(0), "gamma": np.zeros((0, NS), ft), "occ": np.zeros((0, K), ft),
                "ent": np.zeros((0, K), ft)}
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    LA = np.full((K, Nm, Nm), ninf, dtype=ft)
    term = np.zeros((K, Nm, Nm), dtype=bool)
    col = np.zeros((K, Nm), dtype=int)
    real = np.zeros((K, Nm), dtype=bool)
    for k, A in enumerate(As):
        A = np.asarray(A, dtype=np.float64)
        pos = A > 0
        term[k, :Ns[k], :Ns[k]] = pos
        LA[k, :Ns[k], :Ns[k]] = np.where(pos, np.log(np.where(pos, A, 1.0).astype(ft)), ninf)
        col[k, :Ns[k]] = bo[k] + np.arange(Ns[k])
        real[k, :Ns[k]] = True
    last, ar = Ns - 1, np.arange(K)
    st = np.zeros(K, ft) if start is None else np.asarray(start, dtype=np.float64).astype(ft)
    fn = np.zeros(K, ft) if fin is None else np.asarray(fin, dtype=np.float64).astype(ft)
    pr = np.asarray(pair, dtype=np.float64).astype(ft).reshape(K, K)
    gterm, fterm = pr > ninf, fn > ninf
    lbf = np.asarray(logb).astype(ft)

    def lb(t):
        return np.where(real, lbf[t][col], ninf)

    la, lbe = (np.full((T, K, Nm), ninf, dtype=ft) for _ in range(2))
    x = np.full((T, K), ninf, dtype=ft)
    with np.errstate(all="ignore"):
        first = np.full((K, Nm), ninf, dtype=ft)
        first[:, 0] = st
        la[0] = first + lb(0)
        for t in range(1, T):
            inn = _lse(np.where(term, la[t - 1][:, :, None] + LA, ninf), 1)
            ends = la[t - 1][ar, last]
            x[t] = _lse(np.where(gterm, ends[:, None] + pr, ninf), 0)
            inn[:, 0] = _lse2(inn[:, 0], x[t])
            la[t] = inn + lb(t)
        logP = _lse(np.where(fterm, la[T - 1][ar, last] + fn, ninf), 0)
        lbe[T - 1][ar, last] = fn
        for t in range(T - 2, -1, -1):
            w = lb(t + 1) + lbe[t + 1]
            wi = _lse(np.where(term, LA + w[:, None, :], ninf), 2)
            y = _lse(np.where(gterm, pr + w[None, :, 0], ninf), 1)
            lbe[t] = wi
            lbe[t][ar, last] = _lse2(wi[ar, last], y)
        gamma, occ, ent = np.zeros((T, K, Nm), ft), np.zeros((T, K), ft), np.zeros((T, K), ft)
        if np.isfinite(logP):
            gamma = np.where(real, np.exp((la + lbe) - logP), ft(0))
            for j in range(Nm):
                occ = occ + gamma[:, :, j]
            ent[0] = gamma[0, :, 0]
            for t in range(1, T):
                ent[t] = np.exp(((x[t] + lb(t)[:, 0]) + lbe[t][:, 0]) - logP)
    return {"T": T, "logP": logP, "gamma": gamma[:, real], "occ": occ, "ent": ent, "la": la, "lbe": lbe, "x": x,
            "real": real}


def post(case, logb, start, pair, fin, ft=np.longdouble, only=None):
    """lattice over a case's utterances (only: a subset, the others left zero) on logb[F][NS]: a dict of
    gamma [F][NS], occ [F][K], ent [F][K], loglik [U] in ft"""
    As = [np.asarray(w[0].A, dtype=np.float64) for w in case.words]
    off = offsets(case.lens)
    gamma, occ, ent = np.zeros((case.F, case.NS), ft), np.zeros((case.F, case.K), ft), np.zeros((case.F, case.K), ft)
    ll = np.zeros(case.U, ft)
    for u in (range(case.U) if only is None else only):
        r = lattice(As, logb[off[u]:off[u + 1]], start, pair, fin, ft)
        gamma[off[u]:off[u + 1]], occ[off[u]:off[u + 1]], ent[off[u]:off[u + 1]] = r["gamma"], r["occ"], r["ent"]
        ll[u] = r["logP"]
    return {"gamma": gamma, "occ": occ, "ent": ent, "loglik": ll}


def enumerate_paths(As, logb, start, pair, fin):
    """One utterance by brute force in float64: every composite path (k_t, j_t) with its word boundaries (a
    path that leaves word k's last state for word k's first state is another path than the one that stays
    inside a one-state word), each with weight exp(start + sum log b + sum log a or pair + fin).  Returns
    (P, gamma [T][NS], occ [T][K], ent [T][K]) as sums over the paths divided by P (P == 0: zeros)."""
    import math
    K, T = len(As), len(logb)
    Ns = [np.asarray(A).shape[0] for A in As]
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    NS = int(bo[-1])
    start = np.zeros(K) if start is None else start
    fin = np.zeros(K) if fin is None else fin
    with np.errstate(divide="ignore"):
        logAs = [CC.log_a(np.asarray(A, dtype=np.float64)) for A in As]
    paths = []          # (log weight, [(k, j, begins)])

    def walk(t, k, j, lw, trail):
        if t == T - 1:
            if j == Ns[k] - 1 and fin[k] > -np.inf:
                paths.append((lw + fin[k], trail))
            return
        for j2 in range(Ns[k]):
            if logAs[k][j, j2] > -np.inf:
                walk(t + 1, k, j2, lw + logAs[k][j, j2] + logb[t + 1, bo[k] + j2], trail + [(k, j2, False)])
        if j == Ns[k] - 1:
            for k2 in range(K):
                if pair[k, k2] > -np.inf:
                    walk(t + 1, k2, 0, lw + pair[k, k2] + logb[t + 1, bo[k2]], trail + [(k2, 0, True)])

    for k in range(K):
        if start[k] > -np.inf:
            walk(0, k, 0, start[k] + logb[0, bo[k]], [(k, 0, True)])
    P = math.fsum(math.exp(lw) for lw, _ in paths)
    gamma, occ, ent = np.zeros((T, NS)), np.zeros((T, K)), np.zeros((T, K))
    if P > 0:
        cells, begins = {}, {}
        for lw, trail in paths:
            wgt = math.exp(lw)
            for t, (k, j, b) in enumerate(trail):
                cells.setdefault((t, bo[k] + j), []).append(wgt)
                if b:
                    begins.setdefault((t, k), []).append(wgt)
        for (t, s), v in cells.items():
            gamma[t, s] = math.fsum(v) / P
        for (t, k), v in begins.items():
            ent[t, k] = math.fsum(v) / P
        for k in range(K):
            occ[:, k] = gamma[:, bo[k]:bo[k + 1]].sum(1)
    return P, gamma, occ, ent


def unreachable(start, pair, fin):
    """the words that no allowed string can hold by consequence (e)'s local test: they cannot be entered
    (start and the whole column of pair -inf) or cannot be left (the whole row of pair and fin -inf)"""
    K = len(pair)
    start = np.zeros(K) if start is None else np.asarray(start)
    fin = np.zeros(K) if fin is None else np.asarray(fin)
    no_in = (start == -np.inf) & np.all(pair == -np.inf, axis=0)
    no_out = (fin == -np.inf) & np.all(pair == -np.inf, axis=1)
    return np.nonzero(no_in | no_out)[0]


def cut_off(start, pair, fin, k, how):
    """the grammar with word k made unreachable: how = "in" (start and its column) or "out" (fin and its row)"""
    K = len(pair)
    start = (np.zeros(K) if start is None else np.array(start, dtype=np.float64)).copy()
    fin = (np.zeros(K) if fin is None else np.array(fin, dtype=np.float64)).copy()
    pair = np.array(pair, dtype=np.float64).copy()
    if how == "in":
        start[k] = -np.inf
        pair[:, k] = -np.inf
    else:
        fin[k] = -np.inf
        pair[k, :] = -np.inf
    return start, pair, fin


__all__ = ["GPU_GRAMMARS", "CAP_GRAMMARS", "SPREAD_CASES", "lattice", "post", "enumerate_paths", "unreachable",
           "cut_off"]
