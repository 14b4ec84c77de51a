# The diagonal log-domain forward score timed by wall clock on vocab_streams_time.py's vocabulary and corpus:
# 13 words x 6 states, two feature streams (D = 9 and 5, M = 1), 1 000 utterances x 60 frames.
#   loop      ghmm_logscore_streams once per word: 13 x (2 emission launches + 1 fold + 1 lattice launch +
#             1 wait for the stream)
#   batch     ghmm_logscore_streams_batch: 2 gathers and preparations, 2 emission launches, 1 fold, 1 lattice
#             launch, 1 wait
#   beside them, on the same context: ghmm_score_streams_batch (the linear score) and
#   ghmm_viterbi_streams_batch (the best path's score on the same log b)
# and, by GHMM_OPT_TIMING's events, the one-wave-per-utterance lattices at 255 states (ghmm_viterbi's cap;
# band-diagonal A, one stream, D = 9, 256 utterances x 300 frames): k_logforward_wide under GHMM_K_FORWARD
# against k_viterbi_wide under GHMM_K_VITERBI.
#   python profiles/tools/logscore_time.py [package directory [label]]     (from the repository root)
# REPEATS repeats of REPS calls each, every repeat on its own line: the spread between the lines is the
# run-to-run spread a difference has to exceed.
import importlib.util
import os
import sys
import time

import numpy as np

REPS, REPEATS = 10, 3
K, N, U, T = 13, 6, 1000, 60
SHAPES = ((1, 9), (1, 5))       # (M_p, D_p)
WIDE_N, WIDE_U, WIDE_T = 255, 256, 300


def load(pkg_dir):
    spec = importlib.util.spec_from_file_location("ghmm_timed", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ghmm_timed"] = mod
    spec.loader.exec_module(mod)
    return mod.ghmm


def banded(rng, n):
    A = np.zeros((n, n))
    for i in range(n - 1):
        A[i, i] = rng.uniform(0.5, 0.9)
        A[i, i + 1] = 1.0 - A[i, i]
    A[n - 1, n - 1] = 1.0
    return A


def rand_model(G, rng, n, M, D, A):
    iv = rng.uniform(0.5, 2.0, (n, M, D))
    return G.HostModel(A, rng.dirichlet(np.full(M, 3.0), n), rng.normal(0, 1.0, (n, M, D)), iv,
                       np.prod(1.0 / iv, axis=-1))


def timed(name, call):
    call()      # warm-up (allocations, code objects)
    for rep in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            out = call()
        print(f"{name}, repeat {rep + 1}: {1e3 * (time.perf_counter() - t0) / REPS:.3f} ms", flush=True)
    return out


def kernel_ms(G, ctx, name, kind, call):
    call()
    ctx.set_option(G.OPT_TIMING, 1)
    try:
        for rep in range(REPEATS):
            ctx.kernel_times_reset()
            for _ in range(REPS):
                call()
            ms, n = ctx.kernel_times()[kind]
            print(f"{name}, repeat {rep + 1}: {ms / n:.4f} ms per launch ({n} launches)", flush=True)
    finally:
        ctx.set_option(G.OPT_TIMING, 0)


def main():
    pkg = sys.argv[1] if len(sys.argv) > 1 else "speech-recognition-hmm-continuous_amd"
    G = load(pkg)
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    hosts = []
    for _ in range(K):
        A = banded(rng, N)
        hosts.append([rand_model(G, rng, N, M, D, A) for M, D in SHAPES])
    # utterance u walks word u % K: one frame run per state
    st = np.tile(np.repeat(np.arange(N), T // N), U)
    spoken = np.repeat(np.arange(U) % K, T)
    Xs = []
    for p, (_, D) in enumerate(SHAPES):
        mean = np.stack([w[p].mean[:, 0] for w in hosts])       # [K][N][D]
        Xs.append(mean[spoken, st] + rng.normal(0.0, 0.5, (U * T, D)))
    lens = np.full(U, T, dtype=np.int32)
    corpora = [ctx.corpus(X, lens) for X in Xs]
    vocab = [[ctx.model(h) for h in w] for w in hosts]
    label = sys.argv[2] if len(sys.argv) > 2 else pkg
    print(f"{label}: {K} words x {N} states, streams D = {' + '.join(str(D) for _, D in SHAPES)}, "
          f"{U} utterances x {T} frames")

    def loop():
        return np.array([ctx.logscore_streams(w, corpora, final_state=True) for w in vocab])
    one = timed("loop of ghmm_logscore_streams", loop)
    batch = timed("ghmm_logscore_streams_batch", lambda: ctx.logscore_streams_batch(vocab, corpora, final_state=True))
    assert np.allclose(batch, one, rtol=1e-12, atol=0.0, equal_nan=True)
    timed("loop of ghmm_logscore_streams, again", loop)
    lin = timed("ghmm_score_streams_batch", lambda: ctx.score_streams_batch(vocab, corpora))
    vit = timed("ghmm_viterbi_streams_batch", lambda: ctx.viterbi_streams_batch(vocab, corpora))
    fin = np.isfinite(lin)
    print(f"finite linear scores: {int(fin.sum())} of {lin.size}; log-domain against them, worst relative: "
          f"{float(np.max(np.abs(batch[fin] - lin[fin]) / np.abs(lin[fin]))):.2e}; "
          f"pairs with log score < Viterbi score: {int(np.sum(batch < vit))}")

    hw = rand_model(G, rng, WIDE_N, 1, 9, banded(rng, WIDE_N))
    wst = np.tile(np.minimum(np.arange(WIDE_T), WIDE_N - 1), WIDE_U)
    Xw = hw.mean[wst, 0] + rng.normal(0.0, 0.5, (WIDE_U * WIDE_T, 9))
    wm, wc = ctx.model(hw), ctx.corpus(Xw, np.full(WIDE_U, WIDE_T, dtype=np.int32))
    print(f"{WIDE_N} states, band-diagonal A, D = 9, {WIDE_U} utterances x {WIDE_T} frames")
    kernel_ms(G, ctx, "k_logforward_wide", "forward", lambda: ctx.logscore(wm, wc, final_state=True))
    kernel_ms(G, ctx, "k_viterbi_wide", "viterbi", lambda: ctx.viterbi(wm, wc))
    ctx.close()


if __name__ == "__main__":
    main()
