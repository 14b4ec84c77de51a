"""Baum-Welch statistics on the grammar lattice (ghmm_estep_grammar_streams; k_gpost_fwd and k_gpost_bwd in its
statistics form): a numpy restatement of the definition in include/ghmm.h in a chosen float type, per utterance
on a given log b and posteriors, and an enumeration of every composite path that counts the within-word
transitions.  Built on gpost_cases.lattice (la, lbe and x of the lattice), on estep_log_ref's posteriors and
mix_sums and on embed_cases' LSE; the cases and grammars are gpost_cases.GPU_GRAMMARS' diagonal ones.  Shared by
test_gstat_host.py, which checks on the CPU that the restatement is the definition and that consequences (b) to
(e) of the header hold on it, and by test_gstat_gpu.py, which compares the device with the long-double
restatement run on the device's own log b and posteriors.  Plain numpy and the oracle, no GPU, no tests.

The float64 restatement's distance from the long-double one on the oracle's log b and the restated posteriors, per
(case, grammar) that test_gstat_gpu.py compares, as test_gstat_host.test_float64_spread prints it: the worst
relative distance over the finite log P_u | the worst estep_log_ref.block_dist over gamma and every word's and
stream's statistics blocks; the bar on the second is fullcov_support.RTOL / 8 = 1.25e-9:
    narrow  random 5.8e-16 | 2.4e-11   norepeat 4.8e-16 | 1.7e-11   flat:-5 4.8e-16 | 1.7e-11
    ones    random 1.0e-16 | 1.6e-14   norepeat 1.6e-16 | 1.8e-14
    thick   random 1.9e-16 | 7.4e-12   norepeat 1.7e-16 | 1.3e-11   flat:-5 2.0e-16 | 2.1e-11
    k72     random 1.0e-16 | 3.0e-12   norepeat 2.1e-16 | 7.7e-13   flat:-5 4.3e-17 | 3.4e-13
    k100    random 2.3e-16 | 6.4e-13   norepeat 1.0e-16 | 5.8e-12   flat:-5 1.3e-16 | 8.1e-13
    k256    random 6.1e-17 | 1.4e-12   norepeat 6.4e-17 | 8.2e-13   flat:-5 1.3e-16 | 3.4e-12
No case needed another seed."""
import math

import numpy as np

import connect_cases as CC
import estep_log_ref as E
import gpost_cases as PC
import grammar_cases as GC
import logscore_ref as R
from embed_cases import _lse
from fullcov_support import need_extended, offsets

# the (case, grammars) that test_gstat_gpu.py compares with the long-double restatement: gpost_cases' diagonal
# ones but holes, whose NaN log b the diagonal emission does not produce (test_gstat_gpu makes its own holes);
# cap is compared with the float64 restatement alone
GPU_GRAMMARS = {name: PC.GPU_GRAMMARS[name] for name in ("narrow", "ones", "thick", "k72", "k100", "k256")}
CAP_GRAMMARS = PC.CAP_GRAMMARS
SPREAD_CASES = tuple(GPU_GRAMMARS)
COMMON = ("num_a", "den_a", "den_c")
# the band beyond 1 on one state per thread (narrow) and on two with a dense word in the second (thick)
DELTA_CASES = ("narrow", "thick")
DELTAS = (0, 1, 2, 3, 7)


def utterance(As, logb, start, pair, fin, delta=1, ft=np.longdouble):
    """One utterance: gpost_cases.lattice's dict (la, lbe, x, gamma, logP) and, added from la and lbe by the
    header's lines, per word k the sums over t < T-1 of xi (num_a[k], inside the band j <= j' <= j + delta where
    a_jj' > 0) and of stay (den_a[k]), and over t < T of gamma (den_c[k]); all zero where log P is not finite"""
    K, T = len(As), len(logb)
    Ns = np.array([np.asarray(A).shape[0] for A in As])
    r = dict(PC.lattice(As, logb, start, pair, fin, ft))
    r["num_a"] = [np.zeros((N, N), ft) for N in Ns]
    r["den_a"] = [np.zeros(N, ft) for N in Ns]
    r["den_c"] = [np.zeros(N, ft) for N in Ns]
    if T == 0 or not np.isfinite(r["logP"]):
        return r
    bo = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    ninf = ft(-np.inf)
    lbf = np.asarray(logb).astype(ft)
    la, lbe, logP = r["la"], r["lbe"], r["logP"]
    with np.errstate(all="ignore"):
        for k, A in enumerate(As):
            A = np.asarray(A, dtype=np.float64)
            N = int(Ns[k])
            term = A > 0
            LA = np.where(term, np.log(np.where(term, A, 1.0).astype(ft)), ninf)
            j, jp = np.indices((N, N))
            band = term & (jp >= j) & (jp <= j + delta)
            r["den_c"][k] = r["gamma"][:, bo[k]:bo[k] + N].sum(0)
            if T < 2:
                continue
            w = lbf[1:, bo[k]:bo[k] + N] + lbe[1:, k, :N]                               # w_t, t < T-1
            wi = _lse(np.where(term[None], LA[None] + w[:, None, :], ninf), 2)          # wi_t(k, j)
            a = la[:T - 1, k, :N]
            r["den_a"][k] = np.exp((a + wi) - logP).sum(0)
            x = np.exp(((a[:, :, None] + LA[None]) + w[:, None, :]) - logP)
            r["num_a"][k] = np.where(band[None], x, ft(0)).sum(0)
    return r


def estep(words, Xs, lens, start, pair, fin, delta=1, ft=np.longdouble, logb=None, posts=None, only=None):
    """ghmm_estep_grammar_streams restated on the vocabulary words[k][p], the streams Xs[p] and the grammar.
    logb [F][NS] / posts[p] [F][NS * M_p] given: the lattice and the sums run on them (widened to ft) instead of
    on the restated emission.  only: a subset of the utterances, the others as if they had no frames (they still
    count in n_utt).  Returns a dict: logb, posts[p] [F][NS][M_p], gamma [F][NS], loglik[U] and stats[k][p]
    (dicts of estep_log_ref.BLOCKS)."""
    if ft is np.longdouble:
        need_extended()
    P = len(words[0])
    Ns = [w[0].N for w in words]
    NS = sum(Ns)
    cols = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    lens = [int(T) for T in lens]
    F, U = sum(lens), len(lens)
    if logb is None:
        logb = np.concatenate([R.log_b(w, Xs) for w in words], axis=1).astype(ft)
        posts = [np.concatenate([E.posteriors(w[p], Xs[p], ft) for w in words], axis=1) for p in range(P)]
    else:
        logb = np.asarray(logb).astype(ft).reshape(F, NS)
        posts = [np.asarray(q).astype(ft).reshape(F, NS, words[0][p].M) for p, q in enumerate(posts)]
    As = [np.asarray(w[0].A, dtype=np.float64) for w in words]
    gamma = np.zeros((F, NS), ft)
    ll = np.zeros(U, ft)
    common = [{"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)} for N in Ns]
    off = offsets(lens)
    with np.errstate(all="ignore"):
        for u in (range(U) if only is None else only):
            r = utterance(As, logb[off[u]:off[u + 1]], start, pair, fin, delta, ft)
            ll[u] = r["logP"]
            gamma[off[u]:off[u + 1]] = r["gamma"]
            for k in range(len(words)):
                for b in COMMON:
                    common[k][b] += r[b][k]
        loglik = ll.sum() if U else ft(0)
        stats = []
        for k, w in enumerate(words):
            row = []
            for p, hm in enumerate(w):
                st = dict(common[k])
                sl = slice(cols[k], cols[k] + Ns[k])
                st.update(E.mix_sums(gamma[:, sl, None] * posts[p][:, sl], Xs[p], hm.mean, ft))
                st["loglik"], st["n_utt"] = loglik, ft(U)
                row.append(st)
            stats.append(row)
    return {"logb": logb, "posts": posts, "gamma": gamma, "loglik": ll, "stats": stats}


def enumerate_stats(As, logb, start, pair, fin, delta=1):
    """One utterance by brute force in float64: gpost_cases.enumerate_paths' walk over every composite path with
    its word boundaries, counting besides gamma the within-word transitions of t -> t + 1, t < T-1: num_a[k]
    (those inside the band), den_a[k] (every one that stays in the word, whatever its offset) and den_c[k].
    Returns (P, gamma [T][NS], num_a, den_a, den_c) as sums over the paths divided by P (P == 0: zeros)."""
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
    gamma = np.zeros((T, NS))
    num_a, den_a, den_c = [np.zeros((N, N)) for N in Ns], [np.zeros(N) for N in Ns], [np.zeros(N) for N in Ns]
    if P > 0:
        cells, moves = {}, {}
        for lw, trail in paths:
            wgt = math.exp(lw)
            for t, (k, j, _) in enumerate(trail):
                cells.setdefault((t, k, j), []).append(wgt)
                if t + 1 < T and not trail[t + 1][2]:
                    moves.setdefault((k, j, trail[t + 1][1]), []).append(wgt)
        for (t, k, j), v in cells.items():
            gamma[t, bo[k] + j] = math.fsum(v) / P
        for k in range(K):
            den_c[k] = gamma[:, bo[k]:bo[k + 1]].sum(0)
        for (k, j, j2), v in moves.items():
            den_a[k][j] += math.fsum(v) / P
            if j <= j2 <= j + delta:
                num_a[k][j, j2] = math.fsum(v) / P
    return P, gamma, num_a, den_a, den_c


def worst_dist(got_stats, ref_stats, blocks=E.BLOCKS):
    """the worst estep_log_ref.block_dist over the blocks of stats[k][p] dicts, with where it was met"""
    worst, where = 0.0, None
    for k, (gw, rw) in enumerate(zip(got_stats, ref_stats)):
        for p, (g, r) in enumerate(zip(gw, rw)):
            for b in blocks:
                d = E.block_dist(g[b], r[b])
                if d > worst:
                    worst, where = d, (k, p, b)
    return worst, where


__all__ = ["GPU_GRAMMARS", "CAP_GRAMMARS", "SPREAD_CASES", "COMMON", "DELTA_CASES", "DELTAS", "utterance", "estep",
           "enumerate_stats", "worst_dist", "GC"]
