# The embedded Baum-Welch E-step beside what one round of training on a connected corpus costs without it, on
# align_time.py's vocabulary and corpus: 13 words x 6 states x 8 mixtures at D = 39, one feature stream, 1 000
# utterances x 300 frames (each three words of 100 frames), the transcript of an utterance being the three
# words it holds.
#   embed       ghmm_estep_embed_streams and a wait for the stream: the emission with posteriors, k_embed_fwd and
#               k_embed_bwd (lattice of 18 composite states), the statistics launches on the concatenated
#               vocabulary, the scatter
#   cut         the route without it: ghmm_align_streams, word_segments and cut_segments on the host, the 13
#               per-word corpora uploaded, ghmm_estep_log per word, a wait for the stream
# The two alternate in one run under GHMM_OPT_TIMING; per repeat the wall clock of the call and, for embed, the
# time and launches under GHMM_K_FORWARD (the lattice), GHMM_K_EMISSION, GHMM_K_MIXSTATS and GHMM_K_REDUCE;
# then medians with min and max.  The spread between the repeats is the run-to-run spread a difference has to
# exceed.  Then the embedded call seven times in a row, without the other route in between.
#   python profiles/tools/embed_time.py      (from the repository root)
import importlib.util
import os
import sys
import time

import numpy as np

REPEATS = 7
K, N, M, D, U, T = 13, 6, 8, 39, 1000, 300
SEG = 100


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
        A[i, i] = rng.uniform(0.85, 0.95)
        A[i, i + 1] = 1.0 - A[i, i]
    A[N - 1, N - 1] = 1.0
    return A


def main():
    G = load("speech-recognition-hmm-continuous_amd")
    ctx = G.Context(0)
    rng = np.random.default_rng(11)
    hosts = []
    for _ in range(K):
        iv = rng.uniform(0.5, 2.0, (N, M, D))
        hosts.append(G.HostModel(banded(rng), rng.dirichlet(np.full(M, 3.0), N), rng.normal(0, 1.0, (N, M, D)), iv,
                                 np.prod(1.0 / iv, axis=-1)))
    spoken = rng.integers(0, K, (U, T // SEG))
    st = np.minimum(np.arange(SEG) * N // SEG, N - 1)
    mean = np.stack([h.mean for h in hosts])                    # [K][N][M][D]
    X = np.empty((U * T, D))
    for u in range(U):
        for s in range(T // SEG):
            f = u * T + s * SEG
            X[f:f + SEG] = mean[spoken[u, s], st, rng.integers(0, M, SEG)] + rng.normal(0.0, 0.5, (SEG, D))
    lens = np.full(U, T, dtype=np.int32)
    corpora = [ctx.corpus(X, lens)]
    vocab = [[ctx.model(h)] for h in hosts]
    print(f"{K} words x {N} states x {M} mixtures, D = {D}, {U} utterances x {T} frames "
          f"({T // SEG} words of {SEG} frames each)")
    transcripts = [tuple(int(k) for k in s) for s in spoken]
    stats = [[ctx.stats(N, M, D)] for _ in range(K)]
    parts = {}

    def embed():
        ctx.estep_embed_streams(vocab, corpora, transcripts, stats)
        ctx.sync()

    def cut():
        t0 = time.perf_counter()
        word, path, begin, score = ctx.align_streams(vocab, corpora, transcripts)
        t1 = time.perf_counter()
        pieces = G.cut_segments([X], lens, G.word_segments(word, begin, lens), K, score)
        t2 = time.perf_counter()
        own = [ctx.corpus(Xs_k[0], lens_k) for Xs_k, lens_k in pieces]
        t3 = time.perf_counter()
        for k in range(K):
            ctx.estep_log(vocab[k][0], own[k], stats[k][0])
        ctx.sync()
        t4 = time.perf_counter()
        for c in own:
            c.close()
        parts["cut"] = [1e3 * (b - a) for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4))]

    calls = {"embed": embed, "cut": cut}
    for call in calls.values():
        call()      # warm-up (allocations, code objects)
    ctx.set_option(G.OPT_TIMING, 1)
    rows = {name: [] for name in calls}
    for rep in range(REPEATS):
        for name, call in calls.items():
            ctx.kernel_times_reset()
            t0 = time.perf_counter()
            call()
            wall = 1e3 * (time.perf_counter() - t0)
            kt = ctx.kernel_times()
            if name == "embed":
                f, e, m, r = (kt[k] for k in ("forward", "emission", "mixstats", "reduce"))
                rows[name].append((wall, f[0], e[0], m[0], r[0]))
                print(f"embed repeat {rep + 1}: call {wall:8.3f} ms   lattice {f[0]:7.3f} ms in {f[1]} launches   "
                      f"emission {e[0]:7.3f} ms in {e[1]}   mixstats {m[0]:7.3f} ms in {m[1]}   "
                      f"reduce {r[0]:7.3f} ms in {r[1]}", flush=True)
            else:
                a, c, up, es = parts["cut"]
                rows[name].append((wall, a, c, up, es))
                print(f"cut   repeat {rep + 1}: call {wall:8.3f} ms   align {a:7.3f} ms   cut_segments {c:7.3f} ms   "
                      f"13 uploads {up:7.3f} ms   13 estep_log {es:7.3f} ms", flush=True)
    ctx.set_option(G.OPT_TIMING, 0)
    names = {"embed": ("call", "lattice", "emission", "mixstats", "reduce"),
             "cut": ("call", "align", "cut_segments", "uploads", "estep_log")}
    for name, r in rows.items():
        r = np.array(r)
        print(f"{name:5s} median: " + "   ".join(
            f"{what} {np.median(r[:, i]):.3f} ms (min {r[:, i].min():.3f}, max {r[:, i].max():.3f})"
            for i, what in enumerate(names[name])))
    ratio = np.median(np.array(rows["embed"])[:, 0]) / np.median(np.array(rows["cut"])[:, 0])
    print(f"embed / cut, median calls: {ratio:.3f}")
    # the embedded call again without the other route in between (that route allocates and frees thirteen
    # corpora per round, and the call behind it pays for that on the host): what a training loop sees
    embed()
    alone = []
    for rep in range(REPEATS):
        t0 = time.perf_counter()
        ctx.estep_embed_streams(vocab, corpora, transcripts, stats)
        t1 = time.perf_counter()
        ctx.sync()
        alone.append((1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)))
    alone = np.array(alone)
    print(f"embed alone, {REPEATS} calls in a row, median: call {np.median(alone[:, 0]):.3f} ms (min {alone[:, 0].min():.3f}, "
          f"max {alone[:, 0].max():.3f})   of which the host enqueues for {np.median(alone[:, 1]):.3f} ms "
          f"(min {alone[:, 1].min():.3f}, max {alone[:, 1].max():.3f})")
    ll = stats[0][0].loglik()
    print(f"embedded E-step: sum of log P {ll[0]:.6e} over {int(ll[1])} utterances")
    ctx.close()


if __name__ == "__main__":
    main()
