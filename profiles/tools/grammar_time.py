# The connected-word decoder under a word-pair grammar beside the flat-penalty decoder, on connect_time.py's
# vocabulary and corpus: 13 words x 6 states x 8 mixtures at D = 39, one feature stream, 1 000 utterances x
# 300 frames (each three words of 100 frames).
#   connect     ghmm_connect_streams (p = 0): the emission, then k_connect (lattice with the pick, and trace)
#   flat        ghmm_connect_grammar_streams with pair == 0: the same emission, then k_grammar
#   bigram      the same call with bigram_log of the spoken strings (alpha = 1)
# The three alternate in one run under GHMM_OPT_TIMING; per repeat the wall clock of the call and the time
# and launches under GHMM_K_VITERBI and GHMM_K_EMISSION.  The spread between the repeats is the run-to-run
# spread a difference has to exceed.  Then the same on two further shapes, where the K x K term weighs
# more: 64 words (the table staged in LDS) and 256 words (the cap; the table read from L2), 3 states x 2
# mixtures at D = 13, 1 000 utterances x 120 frames.
#   python profiles/tools/grammar_time.py      (from the repository root)
import importlib.util
import os
import sys
import time

import numpy as np

REPEATS = 7
SHAPES = [(13, 6, 8, 39, 1000, 300, 100), (64, 3, 2, 13, 1000, 120, 40), (256, 3, 2, 13, 1000, 120, 40)]


def load(pkg_dir):
    spec = importlib.util.spec_from_file_location("ghmm_timed", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ghmm_timed"] = mod
    spec.loader.exec_module(mod)
    return mod.ghmm


def banded(rng, N):
    A = np.zeros((N, N))
    for i in range(N - 1):
        A[i, i] = rng.uniform(0.85, 0.95)
        A[i, i + 1] = 1.0 - A[i, i]
    A[N - 1, N - 1] = 1.0
    return A


def run(G, ctx, K, N, M, D, U, T, SEG):
    rng = np.random.default_rng(11)
    hosts = []
    for _ in range(K):
        iv = rng.uniform(0.5, 2.0, (N, M, D))
        hosts.append(G.HostModel(banded(rng, N), rng.dirichlet(np.full(M, 3.0), N), rng.normal(0, 1.0, (N, M, D)), iv,
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
    print(f"\n{K} words x {N} states x {M} mixtures, D = {D}, {U} utterances x {T} frames "
          f"({T // SEG} words of {SEG} frames each); NS = {K * N}, the pair table {K * K * 8} bytes")
    start, pair, fin = G.bigram_log(spoken, K, alpha=1.0)
    zero = np.zeros((K, K))
    calls = {"connect": lambda: ctx.connect_streams(vocab, corpora, 0.0),
             "flat": lambda: ctx.connect_grammar_streams(vocab, corpora, zero),
             "bigram": lambda: ctx.connect_grammar_streams(vocab, corpora, pair, start, fin)}
    outs = {}
    for call in calls.values():
        call()      # warm-up (allocations, code objects)
    ctx.set_option(G.OPT_TIMING, 1)
    rows = {name: [] for name in calls}
    for rep in range(REPEATS):
        for name, call in calls.items():
            ctx.kernel_times_reset()
            t0 = time.perf_counter()
            outs[name] = call()
            wall = 1e3 * (time.perf_counter() - t0)
            kt = ctx.kernel_times()
            v, e = kt["viterbi"], kt["emission"]
            rows[name].append((wall, v[0], e[0]))
            print(f"{name:8s} repeat {rep + 1}: call {wall:8.3f} ms   viterbi {v[0]:8.3f} ms in {v[1]} launch(es)   "
                  f"emission {e[0]:8.3f} ms in {e[1]}", flush=True)
    ctx.set_option(G.OPT_TIMING, 0)
    for name, r in rows.items():
        r = np.array(r)
        print(f"{name:8s} median: call {np.median(r[:, 0]):.3f} ms (min {r[:, 0].min():.3f}, max {r[:, 0].max():.3f})   "
              f"viterbi {np.median(r[:, 1]):.3f} ms (min {r[:, 1].min():.3f}, max {r[:, 1].max():.3f})")
    med = {name: np.median(np.array(r)[:, 1]) for name, r in rows.items()}
    print(f"k_grammar / k_connect, medians: flat {med['flat'] / med['connect']:.2f}, bigram {med['bigram'] / med['connect']:.2f}")
    same = all(np.array_equal(a, b) for a, b in zip(outs["connect"], outs["flat"]))
    print(f"the flat grammar's four outputs equal ghmm_connect_streams(0)'s: {same}")
    for name in ("connect", "bigram"):
        word, path, begin, score = outs[name]
        got = G.word_segments(word, begin, lens)
        right = sum([k for k, _, _ in g] == list(s) for g, s in zip(got, spoken))
        print(f"{name}: utterances decoded to the words they hold: {right} of {U}")
    for o in [m for w in vocab for m in w] + corpora:
        o.close()


def main():
    G = load("speech-recognition-hmm-continuous_amd")
    ctx = G.Context(0)
    for shape in SHAPES:
        run(G, ctx, *shape)
    ctx.close()


if __name__ == "__main__":
    main()
