"""The cases of the embedded Baum-Welch E-step (ghmm_estep_embed_streams; k_embed_fwd / k_embed_bwd) and a numpy
restatement of its definition in include/ghmm.h in a chosen float type (np.longdouble, np.float64), per
utterance on a given log b and posteriors.  Shared by test_embed_host.py, which checks on the CPU that the
restatement is the definition (against an enumeration of every path through the composite model), that it is
estep_log_ref's on one-word transcripts and that the cases hold what is leaned on, and by test_embed_gpu.py.
Plain numpy and the oracle, no GPU, no tests.  Built from estep_log_ref (posteriors, mix_sums, block_dist,
vector) and align_cases (vocabularies, transcripts, states_of).

A case is one of align_cases', some with (far) frame 5 moved logscore_cases.FAR = 60 units away in every stream,
so that the linear densities of that frame underflow:
  narrow     far.  P = 3 with M = 1, 3, 2.  S_u differs within one launch (5 to 30 states), the ergodic word 1
             sits mid-transcript (2, 0, 1) and (1, 2), the repeated word (0, 0), word 0 in seven utterances,
             T = 0 with an empty transcript, one-word transcripts on 1 and 2 frames.
  mixed      P = 2 with (M, D) = (2, 9) and (3, 5); the ergodic word 1 of 16 states behind a word of 17.  (Not
             far: with the far frame its float64 spread, 1.3e-9 in word 0's num_mu of stream 1, is above the bar.)
  many       far.  70 words of 3 states, most of them in no transcript; a 20-word transcript on 90 frames:
             an entry in most frames; T = 1 with a one-word transcript.
  ones       one-state words: an instance is its own entry and exit, LSE2 on both sides of one state.
  short      narrow's corpus under other transcripts, most longer than their utterance: log Z = -inf.
  thick      S = 280 with the ergodic words 1 and 23 alternating: a dense word past state 256, in a thread's
             second pass; most of the 28 words in no transcript.
  cap        one utterance of 682 three-state instances on 2200 frames: S = 2046.
  cap-mixed  the cap's utterance among small ones and T = 0.
REACH, what no case above reaches in k_embed_fwd / k_embed_bwd (launch_shape restates the host's choice of threads
and PASSES; test_embed_host.py holds every case to its role in a coverage table):
  broad      90 banded 3-state words, NS = 270, transcripts of at most 21 words (S <= 63: 64 threads): the columns
             from 4 x 64 = 256 up get their tied gamma through tie_gamma's table loop.  Word 85 straddles 256,
             word 87 (columns 261..263) is spoken twice in one utterance, word 89 owns column NS - 1, word 88 and
             most words below 85 are in no transcript; T = 0; two frames for three states.
  broad256   the same with 350 words (NS = 1050 > 4 x 256) and a 65-word transcript (S = 195: 256 threads).
  pass4      thick's vocabulary; 59 instances, the ergodic words 1 and 23 recurring on 4 frames each and the
             banded word 4 on 9: S = 791 on 261 frames, k_embed_fwd<4> / k_embed_bwd<4> with dense words in a
             thread's third and fourth state; beside it a two-word utterance and T = 0.
  pass8      many's vocabulary; 342 instances on 3 and 4 frames each (a banded 3-state word takes 3 frames at
             least, so T = 1068 and not below 1000): S = 1026, <8> at a size the long-double restatement walks;
             beside it a two-word utterance.
  wide       align_cases' wide: S = 161, 192 threads; its last words have 64 states.
  wide128    wide without its further utterance: S = 97, 128 threads.
  mid        mixed + two utterances that end on its word of 17 states: log Z through group_sum<32>.
  deep       connect_cases.cap's 32 words of 64 states (NS = 2048), (3, 5, 17) on 190 frames and (9,) on 70:
             S = 192; log Z over a last word of 64 states (group_sum<64>, j = 63); word 5 is the off-band
             word; the table loop on 192 threads; and the one concatenated model here whose reduction
             launch (a block per entry of num_a) passes 2^32 threads.
SMALL and REACH are the cases the long-double restatement walks freely; cap and cap-mixed take the float64 one.

The float64 restatement's distance from the long-double one, measured by test_embed_host.test_float64_spread
on the oracle's log b and the restated posteriors, which prints per case the worst relative distance over the
finite log P_u and log Z_u | the worst block_dist over every word's and stream's statistics blocks and the
tied gamma, and holds the second below RTOL / 8 = 1.25e-9:
    narrow  4.8e-16 | 4.0e-11      mixed  2.6e-16 | 3.7e-11      many   6.3e-16 | 1.2e-12
    ones    3.9e-17 | 1.4e-14      short  4.8e-16 | 3.4e-12      thick  2.5e-16 | 8.5e-13
    broad   2.6e-16 | 1.1e-13      broad256 2.5e-16 | 8.0e-13    pass4  1.3e-15 | 7.6e-12
    pass8   6.2e-16 | 1.4e-11     wide   8.8e-16 | 6.1e-11      wide128 4.8e-16 | 1.0e-10
    mid     2.6e-16 | 1.4e-11      deep   7.2e-16 | 1.0e-12
(pass8 under its first seed, 720, had 7.3e-9 in a num_mu entry that cancels to 2.6e-5; the seed was changed.)
"""
import functools

import numpy as np

import align_cases as AC
import estep_log_ref as E
import logscore_cases as LC
import logscore_ref as R
from fullcov_support import need_extended, offsets

SMALL = ("narrow", "mixed", "many", "ones", "short", "thick")
REACH = ("broad", "broad256", "pass4", "pass8", "wide", "wide128", "mid", "deep")
BIG = ("cap", "cap-mixed")
ALL = SMALL + REACH + BIG
FAR_CASES = ("narrow", "many")
DELTA_CASES = ("many", "narrow")        # one narrow (3-state banded words) and one with a dense word
DELTAS = (0, 1, 2, 3)
COMMON = ("num_a", "den_a", "den_c")
# the band beyond 3, per case: MAX_DELTA and one below it on one state per thread (narrow), on two with a dense
# word in the second (thick), MAX_DELTA on four (pass4); test_embed_host holds each to a non-zero num_a at o >= 4
MAX_DELTA = 7
WIDE_DELTAS = {"narrow": (5, 7), "thick": (2, 7), "pass4": (7,)}
WAVE, THREADS = 64, 256


def launch_shape(case, transcripts=None):
    """what the host works out of a call (vocab_embed in csrc/ghmm_lattice_host.hpp): Smax over the utterances
    of at least one frame, the threads, PASSES and whether the vocabulary's columns go past a thread's four
    registers into tie_gamma's table loop"""
    transcripts = case.transcripts if transcripts is None else transcripts
    Smax = max([AC.states_of(case, t) for t, T in zip(transcripts, case.lens) if T] + [1])
    threads = min(THREADS, -(-Smax // WAVE) * WAVE)
    need = -(-Smax // threads)
    passes = next(p for p in (1, 2, 4, 8) if need <= p)
    return {"Smax": Smax, "threads": threads, "passes": passes, "table": case.NS > 4 * threads}


def make(G, name, far=None):
    """align_cases' Case of a name (.transcripts, .words[k][p], .Xs[p], .lens, .bo), the far frame moved"""
    case = AC.make(G, name)
    far = name in FAR_CASES if far is None else far
    case.Xs = [np.array(X, dtype=np.float64) for X in case.Xs]
    if far:
        for X in case.Xs:
            X[LC.FAR_FRAME] += LC.FAR
    case.far = far
    return case


def present(case, transcripts=None):
    """the words some transcript holds, ascending"""
    transcripts = case.transcripts if transcripts is None else transcripts
    return sorted({int(k) for t in transcripts for k in t})


# ------------------------------------------------------------- the definition in a float type

def _lse(x, axis):
    """LSE of include/ghmm.h along an axis: the maximum passes over a NaN, the sum takes it; -inf without a term"""
    ft = x.dtype.type
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(x), ft(-np.inf), x).max(axis, keepdims=True)
        mm = np.where(m == -np.inf, ft(0), m)
        return np.squeeze(m + np.log(np.exp(x - mm).sum(axis, keepdims=True)), axis)


def _lse2(a, b):
    return _lse(np.stack([a, b]), 0)


def lattice(As, cols, logb, transcript, delta=1, ft=np.longdouble):
    """One utterance: the definition on logb[T][NS] (word k's columns from cols[k]) and the words' A, for the
    transcript's instances, padded to the largest word with states of -inf.  Returns a dict: la, lbe, w, wi,
    gamma, stay [T][L][Nm] (w, wi and stay: rows 0 .. T-2 hold values), xi [T][L][Nm][Nm] (the band's terms,
    row T-1 empty), logP, logZ, and the real-state mask [L][Nm]."""
    if ft is np.longdouble:
        need_extended()
    T, L = len(logb), len(transcript)
    ninf = ft(-np.inf)
    if T == 0:
        return {"T": 0, "logP": ft(0), "logZ": ft(0)}
    assert L > 0
    Ns = np.array([np.asarray(As[k]).shape[0] for k in transcript])
    Nm = int(Ns.max())
    LA = np.full((L, Nm, Nm), ninf, dtype=ft)
    term = np.zeros((L, Nm, Nm), dtype=bool)
    col = np.zeros((L, Nm), dtype=int)
    real = np.zeros((L, Nm), dtype=bool)
    for i, k in enumerate(transcript):
        A = np.asarray(As[k], dtype=np.float64)
        pos = A > 0
        term[i, :Ns[i], :Ns[i]] = pos
        LA[i, :Ns[i], :Ns[i]] = np.where(pos, np.log(np.where(pos, A, 1.0).astype(ft)), ninf)
        col[i, :Ns[i]] = cols[k] + np.arange(Ns[i])
        real[i, :Ns[i]] = True
    last = Ns - 1
    inst = np.arange(L)
    lbf = np.asarray(logb).astype(ft)

    def lb(t):
        return np.where(real, lbf[t][col], ninf)

    la, lbe, w, wi = (np.full((T, L, Nm), ninf, dtype=ft) for _ in range(4))
    with np.errstate(all="ignore"):
        first = np.full((L, Nm), ninf, dtype=ft)
        first[0, 0] = 0
        la[0] = first + lb(0)
        for t in range(1, T):
            inn = _lse(np.where(term, la[t - 1][:, :, None] + LA, ninf), 1)
            if L > 1:
                inn[1:, 0] = _lse2(inn[1:, 0], la[t - 1][inst[:-1], last[:-1]])
            la[t] = inn + lb(t)
        lbe[T - 1, L - 1, last[L - 1]] = 0
        for t in range(T - 2, -1, -1):
            w[t] = lb(t + 1) + lbe[t + 1]
            wi[t] = _lse(np.where(term, LA + w[t][:, None, :], ninf), 2)
            lbe[t] = wi[t]
            if L > 1:
                lbe[t][inst[:-1], last[:-1]] = _lse2(wi[t][inst[:-1], last[:-1]], w[t][1:, 0])
        logP = la[T - 1, L - 1, last[L - 1]]
        logZ = _lse(la[T - 1, L - 1, :Ns[L - 1]], 0)
        gamma, stay = np.zeros((T, L, Nm), dtype=ft), np.zeros((T, L, Nm), dtype=ft)
        xi = np.zeros((T, L, Nm, Nm), dtype=ft)
        if np.isfinite(logZ):
            gamma = np.where(real, np.exp((la + lbe) - logZ), ft(0))
            stay[:T - 1] = np.where(real, np.exp((la[:T - 1] + wi[:T - 1]) - logZ), ft(0))
            j, jp = np.indices((Nm, Nm))
            band = term & ((jp >= j) & (jp <= j + delta))[None]
            x = np.exp(((la[:T - 1, :, :, None] + LA[None]) + w[:T - 1, :, None, :]) - logZ)
            xi[:T - 1] = np.where(band[None], x, ft(0))
    return {"T": T, "la": la, "lbe": lbe, "w": w, "wi": wi, "gamma": gamma, "stay": stay, "xi": xi,
            "logP": logP, "logZ": logZ, "real": real, "Ns": Ns}


def tied(r, transcript, Ns_word, cols, NS, ft):
    """an utterance's tied sums from lattice's dict: gamma[T][NS] and per word k of the transcript (num_a,
    den_a, den_c), the instances in ascending order"""
    T = r["T"]
    gamma = np.zeros((T, NS), dtype=ft)
    words = {}
    if T == 0:
        return gamma, words
    for i, k in enumerate(transcript):
        N = Ns_word[k]
        na, da, dc = words.setdefault(k, (np.zeros((N, N), ft), np.zeros(N, ft), np.zeros(N, ft)))
        gamma[:, cols[k]:cols[k] + N] += r["gamma"][:, i, :N]
        na += r["xi"][:, i, :N, :N].sum(0)
        da += r["stay"][:, i, :N].sum(0)
        dc += r["gamma"][:, i, :N].sum(0)
    return gamma, words


def estep(words, Xs, lens, transcripts, delta=1, ft=np.longdouble, logb=None, posts=None):
    """ghmm_estep_embed_streams restated on the vocabulary words[k][p], the streams Xs[p] and the transcripts.
    logb [F][NS] / posts[p] [F][NS * M_p] given: the lattice and the sums run on them (widened to ft) instead
    of on the restated emission.  Returns a dict: logb, posts[p] [F][NS][M_p], gamma [F][NS], loglik[U],
    logZ[U], utt (the per-utterance lattice dicts) and stats[k][p] (dicts of estep_log_ref.BLOCKS)."""
    if ft is np.longdouble:
        need_extended()
    K, P = len(words), len(words[0])
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
    As = [w[0].A for w in words]
    gamma = np.zeros((F, NS), ft)
    ll, lz, utt = np.zeros(U, ft), np.zeros(U, ft), []
    common = [{"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)} for N in Ns]
    off = offsets(lens)
    with np.errstate(all="ignore"):
        for u, T in enumerate(lens):
            r = lattice(As, cols, logb[off[u]:off[u + 1]], transcripts[u], delta, ft)
            utt.append(r)
            ll[u], lz[u] = r["logP"], r["logZ"]
            g, per = tied(r, transcripts[u], Ns, cols, NS, ft)
            gamma[off[u]:off[u + 1]] = g
            for k, (na, da, dc) in per.items():
                common[k]["num_a"] += na
                common[k]["den_a"] += da
                common[k]["den_c"] += dc
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
    return {"logb": logb, "posts": posts, "gamma": gamma, "loglik": ll, "logZ": lz, "utt": utt, "stats": stats}


@functools.lru_cache(maxsize=None)
def _reference(G, name, delta, ft):
    case = make(G, name)
    ref = estep(case.words, case.Xs, case.lens, case.transcripts, delta, ft)
    for a in [ref[k] for k in ("logb", "gamma", "loglik", "logZ")] + ref["posts"]:
        a.setflags(write=False)
    return case, ref


def reference(G, name, delta=1, ft=np.longdouble):
    """(Case, estep's dict) of a name on the restated emission, computed once and left unchanged"""
    return _reference(G, name, delta, ft)


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
