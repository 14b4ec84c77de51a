"""numpy restatement of the full-covariance calls on several feature streams (include/ghmm.h,
ghmm_estep_full_streams / ghmm_score_full_streams / ghmm_logscore_full_streams) in a chosen float type,
long double by default, float64 for the pins.  Shared by test_fullstreams_host.py, which pins it to the
real reference's recorded two-stream runs (tests/golden/fullstreams_p2.json) and to the single-stream
restatements, and by test_fullstreams_gpu.py, which holds the HIP code against it.  Plain numpy, no GPU.

Built from the single-stream restatements by import:
  per stream      fulltrain_ref._densities (c * gaus, the 1e20 clamp per stream), its sum b^p and
                  post^p = c gaus / b^p (0 where b^p == 0); in the log domain fullestep_log_ref.emission
  the product     b = ((b^0 * b^1) * b^2)..., log b = ((log b^0 + log b^1) + ...): stream order
                  (TFF:1436-1442, RC:760-789)
  log domain      fulllogscore_ref.lattice_scores and fullestep_log_ref.estep(logb=, post=) on the sum
  statistics      fulltrain_ref.mix_sums per stream on gamma * post^p, that stream's frames and means
The linear recursion on a GIVEN b is the one thing the single-stream module has no entry for (its
estep forms b itself), so `recursions` restates those lines of fulltrain_ref.estep; test_fullstreams_host
holds estep here, on one stream, to fulltrain_ref.estep bit for bit.
The common sums (num_a, den_a, den_c, loglik, n_utt) go into every stream's statistics; the transitions
are stream 0's."""
import numpy as np

import fullestep_log_ref as LE
import fulllogscore_ref as LR
import fulltrain_ref as R
from fullcov_support import need_extended, offsets


def _frames(hms, Xs, ft):
    return [np.asarray(X, dtype=np.float64).reshape(-1, hm.D).astype(ft) for hm, X in zip(hms, Xs)]


def fold(parts, log=False):
    """the product (log: the sum) in stream order, the earlier streams' on the left"""
    out = parts[0]
    with np.errstate(all="ignore"):
        for x in parts[1:]:
            out = out + x if log else out * x
    return out


def emission(hms, Xs, ft=np.longdouble):
    """(b[F][N] the product, [b^p], [post^p[F][N][M_p]]) of TFF's linear densities"""
    bs, posts = [], []
    with np.errstate(all="ignore"):
        for hm, Xf in zip(hms, _frames(hms, Xs, ft)):
            gm = R._densities(hm, Xf, ft)
            b = gm.sum(-1)
            bs.append(b)
            posts.append(np.where(b[..., None] != 0, gm / np.where(b[..., None] != 0, b[..., None], 1), ft(0)))
    return fold(bs), bs, posts


def log_emission(hms, Xs, ft=np.longdouble):
    """(log b[F][N] the sum, [log b^p], [post^p]) of ghmm_estep_full_log's emission"""
    lbs, posts = [], []
    for hm, X in zip(hms, Xs):
        logb, post, _ = LE.emission(hm, X, ft)
        lbs.append(logb)
        posts.append(post)
    return fold(lbs, log=True), lbs, posts


def recursions(A, b, lens, delta, ft):
    """fulltrain_ref.estep's calc_alpha / calc_beta / calc_transition_probab / calc_probability on a given
    b[F][N], operation for operation: (gamma, alpha, beta [F][N], loglik[U], {num_a, den_a, den_c})"""
    N = A.shape[0]
    F = len(b)
    A = A.astype(ft)
    st = {"num_a": np.zeros((N, N), ft), "den_a": np.zeros(N, ft), "den_c": np.zeros(N, ft)}
    gamma, alpha, beta = (np.zeros((F, N), ft) for _ in range(3))
    ll = np.zeros(len(lens), ft)
    e0 = np.zeros(N, ft)
    e0[0] = 1
    o = 0
    with np.errstate(all="ignore"):
        for u, T in enumerate(lens):
            if T == 0:
                continue
            bb = b[o:o + T]
            al, c = np.zeros((T, N), ft), np.zeros(T, ft)
            for t in range(T):
                a = (e0 if t == 0 else al[t - 1] @ A) * bb[t]
                c[t] = 1 / a.sum()
                al[t] = a * c[t]
            be = np.zeros((T, N), ft)
            be[T - 1, N - 1] = c[T - 1]
            for t in range(T - 2, -1, -1):
                be[t] = (A @ (be[t + 1] * bb[t + 1])) * c[t]
            ga = al * be / c[:, None]
            alpha[o:o + T], beta[o:o + T], gamma[o:o + T] = al, be, ga
            for i in range(N):
                for j in range(i, min(N, i + delta + 1)):
                    st["num_a"][i, j] += np.sum(al[:-1, i] * A[i, j] * bb[1:, j] * be[1:, j])
            st["den_a"] += ga[:-1].sum(0)
            st["den_c"] += ga.sum(0)
            ll[u] = -np.log(c).sum() + np.log(al[T - 1, N - 1])
            o += T
    return gamma, alpha, beta, ll, st


def _per_stream_stats(common, gamma, posts, hms, Xfs, ll, n_utt, ft):
    out = []
    with np.errstate(all="ignore"):
        for hm, Xf, post in zip(hms, Xfs, posts):
            st = dict(common)
            st.update(R.mix_sums(gamma[:, :, None] * post, Xf, hm.mean, ft))
            st["loglik"] = ll.sum() if n_utt else ft(0)
            st["n_utt"] = ft(n_utt)
            out.append(st)
    return out


def estep(hms, Xs, lens, delta=1, ft=np.longdouble):
    """ghmm_estep_full_streams, log_domain = 0.  Returns a dict: b (the product), bs, posts (per stream),
    gamma, alpha, beta, loglik[U], stats (a list: stream p's fulltrain_ref statistics dict)"""
    if ft is np.longdouble:
        need_extended()
    lens = [int(T) for T in lens]
    b, bs, posts = emission(hms, Xs, ft)
    gamma, alpha, beta, ll, common = recursions(hms[0].A, b, lens, delta, ft)
    stats = _per_stream_stats(common, gamma, posts, hms, _frames(hms, Xs, ft), ll, len(lens), ft)
    return {"b": b, "bs": bs, "posts": posts, "gamma": gamma, "alpha": alpha, "beta": beta, "loglik": ll,
            "stats": stats}


def estep_log(hms, Xs, lens, delta=1, ft=np.longdouble, logb=None):
    """ghmm_estep_full_streams, log_domain = 1: fullestep_log_ref.estep on the summed log b (logb given:
    on that one, widened to ft) with stream 0's posteriors, then the other streams' Gaussian sums on the
    same gamma.  Returns that call's dict with logbs, posts and stats as lists over the streams."""
    if ft is np.longdouble:
        need_extended()
    lens = [int(T) for T in lens]
    own, lbs, posts = log_emission(hms, Xs, ft)
    if logb is None:
        logb = own
    r = LE.estep(hms[0], Xs[0], lens, delta, ft, logb=logb, post=posts[0])
    common = {k: r["stats"][k] for k in ("num_a", "den_a", "den_c")}
    r["stats"] = _per_stream_stats(common, r["gamma"], posts, hms, _frames(hms, Xs, ft), r["loglik"], len(lens), ft)
    r["logbs"], r["posts"] = lbs, posts
    return r


def score(hms, Xs, lens, ft=np.longdouble):
    """ghmm_score_full_streams: RC's calc_alpha + calc_probability on the product of the recogniser's
    densities (no clamp, c * gaus unrounded in the sum: fullscore_ref's emission), no final-state term"""
    import fullscore_ref as SR
    if ft is np.longdouble:
        need_extended()
    b = fold([SR.emission(hm, X, ft) for hm, X in zip(hms, Xs)])
    return SR.lattice_scores(hms[0].A, b, lens, ft)


def logscore(hms, Xs, lens, final_state, ft=np.longdouble, stats=None):
    """ghmm_logscore_full_streams: fulllogscore_ref.lattice_scores on the sum of the streams' log b"""
    logb = fold([LR.log_emission(hm, X, ft) for hm, X in zip(hms, Xs)], log=True)
    return LR.lattice_scores(hms[0].A, logb, lens, final_state, ft, stats)


def train(G, Xs, lens, N, Ms, ft, estep_fn=estep):
    """train_main.c's loop on P streams (TFF:202-376): ghmm_init_model_full per stream, then the E-step
    here and ghmm_mstep_full_host per stream while |old - p| / |old| > 1e-3 from old = 1.0.  Returns
    (models, iterations, mean probability)"""
    hms = [G.HostFullModel.init_from(X, lens, N, M) for X, M in zip(Xs, Ms)]
    old, it = 1.0, 0
    while True:
        it += 1
        sts = estep_fn(hms, Xs, lens, 1, ft)["stats"]
        p = float(sts[0]["loglik"])
        if abs((old - p) / old) > 1e-3:
            old = p
            hms = [hm.mstep(R.pack(st), delta=1) for hm, st in zip(hms, sts)]
        else:
            return hms, it, p / len(lens)


def bundled_streams(G, golden, mean_list, idx):
    """the two streams of the recorded runs over the bundled utterances `idx`: the 9-d frames and
    streams_util.second_stream of them; ([X1, X2], lens)"""
    import os
    from streams_util import second_stream
    X1 = [G.perfil_read(os.path.join(golden, "perfil", mean_list[i])) for i in idx]
    X2 = [second_stream(x) for x in X1]
    return [np.concatenate(X1), np.concatenate(X2)], np.array([len(x) for x in X1], dtype=np.int32)


# ------------------------------------------------ the shapes the GPU tests run
# The smallest shapes at which the fold can go wrong: 35 states are two blockIdx.y rows of
# k_emission_full (N > 32) with a last wave of 3 states (N % 8 != 0); D = 3, 9, 17 are three DB
# instantiations; M = 1 and 3 (and 2); 70 + 5 + 64 = 139 frames are two full frame tiles and one of 11,
# and the 5-frame utterance is shorter than the model.
STREAM_SHAPES = [(1, 3), (3, 9), (2, 17)]      # (M_p, D_p) of streams 0, 1, 2
N_STATES = 35
LENS = (70, 5, 64)
CASES = {f"p{P}-{kind}": (P, kind) for P in (2, 3) for kind in ("banded", "ergodic")}


def stream_frames(rng, hms, lens):
    """one left-to-right walk per utterance, shared by the streams (an utterance shorter than the model
    takes one frame per state from the first); stream p's frame = a mean of its own mixtures, noise 0.3"""
    N = hms[0].N
    states = []
    for T in lens:
        if T >= N:
            cuts = np.sort(rng.choice(np.arange(1, T), N - 1, replace=False))
            states.append(np.searchsorted(cuts, np.arange(T), side="right"))
        else:
            states.append(np.arange(T))
    st = np.concatenate(states) if states else np.zeros(0, dtype=int)
    return [hm.mean[st, rng.integers(0, hm.M, len(st))] + rng.normal(0.0, 0.3, (len(st), hm.D)) for hm in hms]


def make_case(G, name):
    """([HostFullModel per stream], [X per stream], lens) of a CASES entry; every stream carries the same A"""
    from fullcov_support import banded, ergodic, rand_fmodel
    P, kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 300)
    A = banded(rng, N_STATES) if kind == "banded" else ergodic(rng, N_STATES)
    hms = [rand_fmodel(G, rng, N_STATES, M, D, A.copy(), spread=1.0, asym=(p == 1), word="w")
           for p, (M, D) in enumerate(STREAM_SHAPES[:P])]
    return hms, stream_frames(rng, hms, LENS), np.asarray(LENS, dtype=np.int32)


def make_far_case(G):
    """Two streams of unit covariances, 6 states; frame 5 of each stream lies sqrt(1000) from its state's
    mean, so that each stream's own densities there are about exp(-500) > 0 in double while their
    product underflows to 0 on the whole frame"""
    from fullcov_support import banded, rand_fmodel
    rng = np.random.default_rng(77)
    A = banded(rng, 6)
    hms = []
    for M, D in ((2, 4), (1, 6)):
        h = rand_fmodel(G, rng, 6, M, D, A.copy(), spread=1.0, asym=False)
        ic = np.broadcast_to(np.eye(D), (6, M, D, D)).copy()
        hms.append(G.HostFullModel(h.A, h.c, h.mean, ic, np.ones((6, M)), word="far"))
    lens = np.array([40, 30], dtype=np.int32)
    Xs = stream_frames(rng, hms, lens)
    for hm, X in zip(hms, Xs):
        v = np.zeros(hm.D)
        v[0] = np.sqrt(1000.0)
        X[5] = hm.mean[0, 0] + v
    return hms, Xs, lens


__all__ = ["fold", "emission", "log_emission", "recursions", "estep", "estep_log", "score", "logscore", "train",
           "bundled_streams", "offsets", "CASES", "make_case", "make_far_case", "stream_frames"]
