# One embedded Baum-Welch E-step on full-covariance words (ghmm_estep_embed_full_streams) by
# ghmm_ctx_kernel_time classes, beside the same call on diagonal models of the same shapes
# (ghmm_estep_embed_streams, vector tier and default tier) and beside the work it replaces: the corpus cut at
# its word boundaries into one corpus per word, ghmm_estep_full_streams(log_domain = 1) per word, summed.
#   workload   20 words x 8 states, M = 4, D = 13, one stream; 400 utterances of 3 to 5 words, 40 to 80 frames a
#              word (about 60), the transcript of an utterance being the words it holds
# One warm-up call of each, then REPEATS rounds in which the three alternate under GHMM_OPT_TIMING; per call the
# wall clock with a wait for the stream and the time and launches per kernel class; then medians with min and
# max.  The spread between the repeats is the run-to-run spread a difference has to exceed.  The cut corpora
# are made and uploaded once, outside the timing: a training loop on a fixed segmentation would do the same.
#   python profiles/tools/embed_full_time.py      (from the repository root)
import importlib.util
import os
import sys
import time

import numpy as np

REPEATS = 9
K, N, M, D, U = 20, 8, 4, 13, 400
CLASSES = ("emission", "forward", "mixstats", "reduce")


def load(pkg_dir):
    spec = importlib.util.spec_from_file_location("ghmm_timed", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ghmm_timed"] = mod
    spec.loader.exec_module(mod)
    return mod.ghmm


def banded(rng):
    A = np.zeros((N, N))
    for i in range(N - 1):
        A[i, i] = rng.uniform(0.8, 0.9)
        A[i, i + 1] = 1.0 - A[i, i]
    A[N - 1, N - 1] = 1.0
    return A


def main():
    G = load("speech-recognition-hmm-continuous_amd")
    ctx = G.Context(0)
    rng = np.random.default_rng(12)
    full, diag = [], []
    for _ in range(K):
        A, c, mean = banded(rng), rng.dirichlet(np.full(M, 3.0), N), rng.normal(0, 1.0, (N, M, D))
        ic = np.empty((N, M, D, D))
        for i in range(N):
            for k in range(M):
                Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
                ic[i, k] = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
                ic[i, k] = (ic[i, k] + ic[i, k].T) / 2
        full.append(G.HostFullModel(A, c, mean, ic, 1.0 / np.linalg.det(ic)))
        iv = np.ascontiguousarray(np.diagonal(ic, axis1=-2, axis2=-1))
        diag.append(G.HostModel(A, c, mean, iv, np.prod(1.0 / iv, axis=-1)))
    transcripts, lens, parts, cut = [], [], [], [[] for _ in range(K)]
    for u in range(U):
        words = rng.integers(0, K, rng.integers(3, 6))
        T = 0
        for k in words:
            seg = int(rng.integers(40, 81))
            st = np.minimum(np.arange(seg) * N // seg, N - 1)
            x = full[k].mean[st, rng.integers(0, M, seg)] + rng.normal(0.0, 0.5, (seg, D))
            parts.append(x)
            cut[k].append(x)
            T += seg
        transcripts.append(tuple(int(k) for k in words))
        lens.append(T)
    X, lens = np.concatenate(parts), np.asarray(lens, dtype=np.int32)
    n_inst = sum(len(t) for t in transcripts)
    print(f"{K} words x {N} states x {M} mixtures, D = {D}, one stream; {U} utterances, {n_inst} word instances, "
          f"{len(X)} frames ({len(X) / n_inst:.1f} a word); NS = {K * N}, the largest S_u = {N * max(map(len, transcripts))}")
    corpora = [ctx.corpus(X, lens)]
    fvocab, dvocab = [[ctx.full_model(h)] for h in full], [[ctx.model(h)] for h in diag]
    fstats, dstats = [[ctx.stats_full(N, M, D)] for _ in range(K)], [[ctx.stats(N, M, D)] for _ in range(K)]
    own = [ctx.corpus(np.concatenate(c), np.asarray([len(x) for x in c], dtype=np.int32)) for c in cut]

    def embed_full():
        ctx.estep_embed_full_streams(fvocab, corpora, transcripts, fstats)
        ctx.sync()

    def embed_diag():
        ctx.estep_embed_streams(dvocab, corpora, transcripts, dstats)
        ctx.sync()

    def embed_diag_vector():
        ctx.set_option(G.OPT_KERNELS, 1)
        try:
            embed_diag()
        finally:
            ctx.set_option(G.OPT_KERNELS, 0)

    def words_full():
        for k in range(K):
            ctx.estep_full_streams(fvocab[k], [own[k]], fstats[k], log=True)
        ctx.sync()

    calls = {"embed_full": embed_full, "embed_diag": embed_diag, "embed_diag_vector": embed_diag_vector,
             "words_full": words_full}
    for call in calls.values():
        call()      # warm-up (allocations, code objects)
        call()
    ctx.set_option(G.OPT_TIMING, 1)
    rows = {name: [] for name in calls}
    for rep in range(REPEATS):
        for name, call in calls.items():
            ctx.kernel_times_reset()
            t0 = time.perf_counter()
            call()
            wall = 1e3 * (time.perf_counter() - t0)
            kt = ctx.kernel_times()
            rows[name].append([wall] + [kt[k][0] for k in CLASSES])
            print(f"{name:18s} repeat {rep + 1}: call {wall:8.3f} ms   " +
                  "   ".join(f"{k} {kt[k][0]:7.3f} ms in {kt[k][1]}" for k in CLASSES), flush=True)
    ctx.set_option(G.OPT_TIMING, 0)
    for name, r in rows.items():
        r = np.array(r)
        print(f"{name:18s} median: " + "   ".join(
            f"{what} {np.median(r[:, i]):.3f} ms (min {r[:, i].min():.3f}, max {r[:, i].max():.3f})"
            for i, what in enumerate(("call",) + CLASSES)))
    med = {name: np.median(np.array(r), axis=0) for name, r in rows.items()}
    print(f"embed_full / words_full, median calls: {med['embed_full'][0] / med['words_full'][0]:.3f}; "
          f"kernel classes summed: {med['embed_full'][1:].sum():.3f} ms against {med['words_full'][1:].sum():.3f} ms")
    # the embedded call without the others in between, and without the timing events: what a training loop sees
    embed_full()
    alone = []
    for rep in range(REPEATS):
        t0 = time.perf_counter()
        ctx.estep_embed_full_streams(fvocab, corpora, transcripts, fstats)
        t1 = time.perf_counter()
        ctx.sync()
        alone.append((1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)))
    alone = np.array(alone)
    print(f"embed_full alone, {REPEATS} calls in a row, median: call {np.median(alone[:, 0]):.3f} ms (min "
          f"{alone[:, 0].min():.3f}, max {alone[:, 0].max():.3f})   of which the host enqueues for "
          f"{np.median(alone[:, 1]):.3f} ms (min {alone[:, 1].min():.3f}, max {alone[:, 1].max():.3f})")
    ll = fstats[0][0].loglik()
    print(f"embedded E-step: sum of log P {ll[0]:.6e} over {int(ll[1])} utterances")
    ctx.close()


if __name__ == "__main__":
    main()
