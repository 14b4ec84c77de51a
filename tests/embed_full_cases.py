"""The cases of the embedded Baum-Welch E-step on full-covariance words (ghmm_estep_embed_full_streams) and a
numpy restatement of its definition in include/ghmm.h in a chosen float type (np.longdouble, np.float64).
Shared by test_embed_full_host.py, which checks on the CPU that the restatement is fullestep_log_ref's on
one-word transcripts and that the cases hold what is leaned on, and by test_embed_full_gpu.py.  Plain numpy,
no GPU, no tests.

The restatement is composed from what exists: embed_cases.lattice and embed_cases.tied for the lattice (they
see log b[T][NS] and the words' A, no Gaussian), fullestep_log_ref.emission per word and stream with the log b
summed over the streams in stream order, ((log b^0 + log b^1) + ...), and fulltrain_ref.mix_sums on
gamma[:, cols, None] * post.  estep() accepts logb= / posts= like embed_cases.estep.

  full    align_cases.make(G, "full"): NS = 30, three words on three streams, with its transcripts.
  mix     P = 2 with (M, D) = (2, 5) and (3, 4); words of 5, 16 (ergodic, fullcov_support.ergodic), 9 and 1
          states and a fifth of 4 states that no transcript holds.  Utterances: T = 0 with an empty transcript,
          T = 1 with the one-state word, one-word transcripts on 1 and 2 frames (both too short to reach their
          word's last state: log P = -inf, log Z finite), the repeated word (0, 0), the ergodic word mid-transcript
          (2, 1, 0), (1, 2), and (3, 0, 3): the one-state word as its own entry and exit on either side.  Frame
          logscore_cases.FAR_FRAME of every stream is moved by logscore_cases.FAR, so that the linear densities
          of that frame underflow in float64 and only a log-domain E-step is finite.
  short   mix's corpus under SHORT: transcripts longer than their utterances in utterances SHORT_NO_Z
          (log Z = -inf: they add only log P_u and the count, their gamma rows are 0).
  holes   align_cases.make(G, "holes") with the transcripts of align_cases.HOLES: NaN and -inf columns in
          log b.  Compared with equal NaN / -inf / zero patterns against the restatement run on the device's own
          log b and posteriors; the host's float64 spread is not taken on it (a restated NaN has no distance).
  deep    32 words of 64 banded states, (M, D) = (1, 3), NS = 2048; (3, 5, 17) on 190 frames and (9,) on 70:
          S = 192, the last word has 64 states.  The case whose k_reduce_all launch (a block of 1024
          threads per entry of num_a) passes 2^32 work-items: deep_blocks().  Three banded words of 64 states
          take 192 frames at least, so on 190 frames the first utterance has log P = -inf (log Z is finite: the
          last instance is reached, its last state is not) and zero gammas; word 9 carries the sums.
  deep200 deep's vocabulary with (3, 5, 17) on 200 frames: the same launches with every log P finite, the
          lattice on S = 192 with gammas in three words, log Z over a last word of 64 states.
  deltas  mix under GHMM_OPT_DELTA 0, 2 and 3 (DELTAS).
  point   the training corpus of the four-iteration test, after test_embed_gpu's point_case: four words plus one
          that no transcript holds on two streams, a far frame in every utterance, the means perturbed.

The float64 restatement's distance from the long-double one, measured by
test_embed_full_host.test_float64_spread on the restated emission, which prints per case the worst relative
distance over the finite log P_u and log Z_u | the worst block_dist over every word's and stream's statistics
blocks and the tied gamma, and holds the second below RTOL / 8 = 1.25e-9:
    full   8.6e-17 | 2.9e-11      mix    2.7e-16 | 5.6e-10      short  2.7e-16 | 3.1e-10
    deep   3.5e-16 | 3.0e-13      deep200 3.0e-16 | 2.5e-12     mix under delta 0, 2 and 3: 2.7e-16 | 5.6e-10 each
(mix's worst entry is a num_mu of word 0's stream 1, into which the far frame enters with a coordinate of 60;
every case met the bar under its first seed.)
EM_POINT_F64: four embedded EM iterations on point with this E-step in float64 against the same in long double,
both driven with the library's ghmm_mstep_full_host on the statistics as float64 holds them: the worst relative
distance of the trace and the worst block_dist over the last models' arrays of the words some transcript holds,
measured and printed by test_embed_full_host.test_four_em_iterations: trace 8.3e-15, models 1.1e-11.  The GPU
test's bound is max(RTOL, 8 x EM_POINT_F64) = RTOL.
"""
import functools

import numpy as np

import align_cases as AC
import embed_cases as EC
import estep_log_ref as E
import fullestep_log_ref as FE
import fulltrain_ref as R
import fullvocab_cases as FV
import logscore_cases as LC
from fullcov_support import RTOL, banded, ergodic, need_extended, offsets, rand_fmodel
from fullstreams_ref import stream_frames

BLOCKS = ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_cov", "loglik", "n_utt")
SUMS = BLOCKS[:-2]
NAMES = ("full", "mix", "short", "deep", "deep200")        # what the long-double restatement walks on its own emission
DELTAS = (0, 2, 3)
EM_POINT_F64 = 1.2e-11     # measured: see the module docstring

MIX_SHAPES = ((2, 5), (3, 4))
MIX_NS = (5, 16, 9, 1, 4)                        # word 1 is ergodic, word 4 is in no transcript
MIX_UTTS = [((), ()), ((3,), (1,)), ((0,), (1,)), ((2,), (2,)), ((0, 0), (8, 9)), ((2, 1, 0), (12, 20, 8)),
            ((1, 2), (22, 14)), ((3, 0, 3), (2, 7, 1))]
MIX_SEED = 931
# short: mix's lengths are 0, 1, 1, 2, 17, 40, 36, 10
SHORT = [(), (3, 3), (0,), (2, 1), (0, 2, 0, 2), (2, 1, 0), (1, 2), (3, 0, 2, 3)]
SHORT_NO_Z = (1, 3, 4, 7)                        # the last instance is out of reach: log Z = -inf
DEEP_WORDS, DEEP_N, DEEP_SHAPE, DEEP_SEED = 32, 64, (1, 3), 932
DEEP_UTTS = {"deep": [((3, 5, 17), (75, 40, 75)), ((9,), (70,))],
             "deep200": [((3, 5, 17), (70, 66, 64)), ((9,), (70,))]}
RD_THREADS = 1024

POINT_NS, POINT_SHAPES, POINT_SEED = (3, 5, 4, 3, 4), ((2, 3), (1, 2)), 2025
# test_embed_gpu's utterances with three times the frames, spoken twice: a full covariance of D coefficients
# needs more than D frames per Gaussian to stay regular (with the diagonal test's 7 to 12 frames a word the
# determinants reach 0 in the second iteration)
POINT_UTTS = 2 * [((0, 1), (21, 36)), ((2, 0, 3), (27, 24, 21)), ((1, 1), (33, 36)), ((3, 2), (24, 30)), ((0,), (27,)),
                  ((2, 3, 0, 1), (27, 21, 24, 36)), ((1, 0), (36, 18))]  # word 4 is in no transcript
POINT_ITERS = 4


def _spoken(rng, words, utts):
    """utterance by utterance, word by word, fullstreams_ref.stream_frames' walk through the word"""
    P = len(words[0])
    parts, lens, spoken = [[np.zeros((0, h.D))] for h in words[0]], [], []
    for seq, seg in utts:
        for k, T in zip(seq, seg):
            x = stream_frames(rng, words[k], [int(T)])
            for p in range(P):
                parts[p].append(x[p])
        lens.append(int(sum(seg)))
        spoken.append(tuple(seq))
    return [np.concatenate(x) for x in parts], lens, spoken


def _mix(G):
    rng = np.random.default_rng(MIX_SEED)
    words = []
    for k, N in enumerate(MIX_NS):
        A = ergodic(rng, N) if k == 1 else banded(rng, N)
        words.append([rand_fmodel(G, rng, N, M, D, A.copy(), spread=1.0, asym=False, symmetrise=True, word=f"w{k}")
                      for M, D in MIX_SHAPES])
    Xs, lens, spoken = _spoken(rng, words, MIX_UTTS)
    for X in Xs:
        X[LC.FAR_FRAME] += LC.FAR
    case = FV.Case(words, Xs, lens)
    case.transcripts = spoken
    return case


def _deep(G, name):
    rng = np.random.default_rng(DEEP_SEED)
    M, D = DEEP_SHAPE
    words = [[rand_fmodel(G, rng, DEEP_N, M, D, banded(rng, DEEP_N), spread=1.0, asym=False, symmetrise=True,
                          word=f"w{k}")] for k in range(DEEP_WORDS)]
    Xs, lens, spoken = _spoken(rng, words, DEEP_UTTS[name])
    case = FV.Case(words, Xs, lens)
    case.transcripts = spoken
    return case


def make(G, name):
    """fullvocab_cases' Case of a name (.words[k][p], .Xs[p], .lens, .bo) with .transcripts and .name"""
    if name in ("full", "holes"):
        case = AC.make(G, name)
        if name == "holes":
            case.transcripts = list(AC.HOLES["spoken"][0])
    elif name in ("mix", "short"):
        case = _mix(G)
        if name == "short":
            case.transcripts = list(SHORT)
    else:
        assert name in DEEP_UTTS, name
        case = _deep(G, name)
    case.Xs = [np.array(X, dtype=np.float64) for X in case.Xs]
    case.name = name
    return case


def deep_blocks(NS=DEEP_WORDS * DEEP_N):
    """the blocks of run_fullstats' k_reduce_all launch on a model of NS states: num_a, den_a, den_c, the tail"""
    return NS * NS + 2 * NS + 1


def point_case(G):
    """(the models the training starts from, Xs, lens, transcripts): a connected corpus built as the cases
    above, a far frame in every utterance, the start = the truth with every mean moved"""
    rng = np.random.default_rng(POINT_SEED)
    truth = [[rand_fmodel(G, rng, N, M, D, banded(rng, N), spread=2.0, asym=False, symmetrise=True, word=f"w{k}")
              for M, D in POINT_SHAPES] for k, N in enumerate(POINT_NS)]
    Xs, lens, transcripts = _spoken(rng, truth, POINT_UTTS)
    off = offsets(lens)
    for X in Xs:
        X[off[:-1] + 2] += LC.FAR
    start = [[G.HostFullModel(h.A, h.c, h.mean + rng.normal(0.0, 0.15, h.mean.shape), h.inv_cov, h.det, word=h.word)
              for h in w] for w in truth]
    return start, Xs, np.asarray(lens, dtype=np.int32), transcripts


present = EC.present


# ------------------------------------------------------------- the definition in a float type

def emission(words, Xs, ft=np.longdouble):
    """(log b[F][NS], posts[p][F][NS][M_p]): per word and stream fullestep_log_ref.emission, a word's log b the
    streams' summed in stream order, its posteriors each stream's own"""
    cols, posts = [], [[] for _ in words[0]]
    with np.errstate(all="ignore"):
        for w in words:
            lb = None
            for p, hm in enumerate(w):
                lbp, post, _ = FE.emission(hm, Xs[p], ft)
                lb = lbp if lb is None else lb + lbp
                posts[p].append(post)
            cols.append(lb)
    return np.concatenate(cols, axis=1), [np.concatenate(q, axis=1) for q in posts]


def estep(words, Xs, lens, transcripts, delta=1, ft=np.longdouble, logb=None, posts=None):
    """ghmm_estep_embed_full_streams restated on the vocabulary words[k][p], the streams Xs[p] and the
    transcripts.  logb [F][NS] / posts[p] [F][NS * M_p] given: the lattice and the sums run on them (widened to
    ft) instead of on the restated emission; logb alone: on it and the restated posteriors.  Returns a dict: logb, posts[p] [F][NS][M_p], gamma [F][NS],
    loglik[U], logZ[U] and stats[k][p] (dicts of BLOCKS)."""
    if ft is np.longdouble:
        need_extended()
    P = len(words[0])
    Ns = [w[0].N for w in words]
    NS = sum(Ns)
    cols = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    lens = [int(T) for T in lens]
    F, U = sum(lens), len(lens)
    if logb is None:
        logb, posts = emission(words, Xs, ft)
    else:
        logb = np.asarray(logb).astype(ft).reshape(F, NS)
        if posts is None:       # (several streams: the library serves log b, not the streams' posteriors)
            posts = emission(words, Xs, ft)[1]
        else:
            posts = [np.asarray(q).astype(ft).reshape(F, NS, words[0][p].M) for p, q in enumerate(posts)]
    As = [w[0].A for w in words]
    Xfs = [np.asarray(X, dtype=np.float64).astype(ft) for X in Xs]
    gamma = np.zeros((F, NS), ft)
    ll, lz = np.zeros(U, ft), np.zeros(U, ft)
    common = [{"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)} for N in Ns]
    off = offsets(lens)
    with np.errstate(all="ignore"):
        for u in range(U):
            r = EC.lattice(As, cols, logb[off[u]:off[u + 1]], transcripts[u], delta, ft)
            ll[u], lz[u] = r["logP"], r["logZ"]
            g, per = EC.tied(r, transcripts[u], Ns, cols, NS, ft)
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
                st.update(R.mix_sums(gamma[:, sl, None] * posts[p][:, sl], Xfs[p], hm.mean, ft))
                st["loglik"], st["n_utt"] = loglik, ft(U)
                row.append(st)
            stats.append(row)
    return {"logb": logb, "posts": posts, "gamma": gamma, "loglik": ll, "logZ": lz, "stats": stats}


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


def worst_dist(got, ref, lens):
    """the worst estep_log_ref.block_dist over every block of stats[k][p] and the utterances' tied gamma, with
    where it was met; got and ref are estep's dicts (or hold "stats" and "gamma" like them)"""
    worst, where = 0.0, None
    for k, (gw, rw) in enumerate(zip(got["stats"], ref["stats"])):
        for p, (g, r) in enumerate(zip(gw, rw)):
            for b in BLOCKS:
                d = E.block_dist(g[b], r[b])
                if d > worst:
                    worst, where = d, (k, p, b)
    off = offsets(lens)
    for u in range(len(lens)):
        d = E.block_dist(got["gamma"][off[u]:off[u + 1]], ref["gamma"][off[u]:off[u + 1]])
        if d > worst:
            worst, where = d, ("gamma", u)
    return worst, where


def em_trajectory(start, Xs, lens, transcripts, iters=POINT_ITERS, ft=np.float64):
    """(trace, models): `iters` embedded EM iterations with estep in ft and the library's ghmm_mstep_full_host
    (HostFullModel.mstep) on every stream of every word some transcript holds, the statistics as float64 holds
    them (fulltrain_ref.pack)"""
    held = present(None, transcripts)
    models, trace = [[h.copy() for h in w] for w in start], []
    for _ in range(iters):
        e = estep(models, Xs, lens, transcripts, ft=ft)
        trace.append(float(e["loglik"].sum()))
        for k in held:
            models[k] = [h.mstep(R.pack(st)) for h, st in zip(models[k], e["stats"][k])]
    return trace, models


def trajectory_dist(a, b, held):
    """(the worst relative distance of two traces, the worst block_dist over the held words' models' arrays)"""
    (ta, ma), (tb, mb) = a, b
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(ta, tb))
    e_model = max(E.block_dist(x, y) for k in held for ha, hb in zip(ma[k], mb[k]) for x, y in zip(ha.arrays(), hb.arrays()))
    return e_tr, e_model


def em_bound():
    """the GPU test's bound on trace and models: the margin RTOL / 8 encodes, on the measured float64 distance"""
    return max(RTOL, 8 * EM_POINT_F64)
