# The forced alignment beside the connected-word decoder, on connect_time.py's vocabulary and corpus: 13
# words x 6 states x 8 mixtures at D = 39, one feature stream, 1 000 utterances x 300 frames (each three
# words of 100 frames), the transcript of an utterance being the three words it holds.
#   connect     ghmm_connect_streams (p = 0): the emission, then k_connect (lattice with the pick, and trace)
#   align       ghmm_align_streams: the same emission, then k_align (lattice of 18 composite states, and trace)
# The two alternate in one run under GHMM_OPT_TIMING; per repeat the wall clock of the call and the time
# and launches under GHMM_K_VITERBI and GHMM_K_EMISSION; then medians with min and max.  The spread between
# the repeats is the run-to-run spread a difference has to exceed.
#   python profiles/tools/align_time.py      (from the repository root)
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
    calls = {"connect": lambda: ctx.connect_streams(vocab, corpora, 0.0),
             "align": lambda: ctx.align_streams(vocab, corpora, transcripts)}
    for call in calls.values():
        call()      # warm-up (allocations, code objects)
    ctx.set_option(G.OPT_TIMING, 1)
    rows = {name: [] for name in calls}
    for rep in range(REPEATS):
        for name, call in calls.items():
            ctx.kernel_times_reset()
            t0 = time.perf_counter()
            out = call()
            wall = 1e3 * (time.perf_counter() - t0)
            kt = ctx.kernel_times()
            v, e = kt["viterbi"], kt["emission"]
            rows[name].append((wall, v[0], e[0]))
            print(f"{name:9s} repeat {rep + 1}: call {wall:8.3f} ms   viterbi {v[0]:8.3f} ms in {v[1]} launch(es)   "
                  f"emission {e[0]:8.3f} ms in {e[1]}", flush=True)
    ctx.set_option(G.OPT_TIMING, 0)
    for name, r in rows.items():
        r = np.array(r)
        print(f"{name:9s} median: call {np.median(r[:, 0]):.3f} ms (min {r[:, 0].min():.3f}, max {r[:, 0].max():.3f})   "
              f"viterbi {np.median(r[:, 1]):.3f} ms (min {r[:, 1].min():.3f}, max {r[:, 1].max():.3f})")
    ratio = np.median(np.array(rows["align"])[:, 1]) / np.median(np.array(rows["connect"])[:, 1])
    print(f"k_align / k_connect, medians: {ratio:.2f}")
    word, path, begin, score = out
    got = G.word_segments(word, begin, lens)
    starts = np.array([[a for _, a, _ in g] for g in got if len(g) == T // SEG])
    print(f"utterances aligned with a finite score: {int(np.isfinite(score).sum())} of {U}; word boundaries "
          f"within 10 frames of where the words were put together: "
          f"{int((np.abs(starts - SEG * np.arange(T // SEG)) <= 10).all(axis=1).sum())} of {len(starts)}")
    ctx.close()


if __name__ == "__main__":
    main()
