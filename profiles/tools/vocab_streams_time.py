# The diagonal several-stream vocabulary calls timed by wall clock at the recorded recogniser's shape scaled
# up: 13 words x 6 states, two feature streams (D = 9 and 5, M = 1), 1 000 utterances x 60 frames.
#   loop      the recogniser's model-by-model loop: ghmm_score_streams once per word, 13 x (2 emission
#             launches + 1 fold + 1 forward launch + 1 wait for the stream)
#   batch     ghmm_score_streams_batch: 2 gathers and preparations, 2 emission launches, 1 fold, 1 forward
#             launch, 1 wait
#   decode    ghmm_recognise_streams against ghmm_viterbi_streams_batch + a host argmax + one
#             ghmm_viterbi_streams per distinct winner
# The loop uses nothing this call family added, so the same file times a checkout from before it (which
# then prints the loop only):
#   python profiles/tools/vocab_streams_time.py [package directory [label]]     (from the repository root)
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


def load(pkg_dir):
    spec = importlib.util.spec_from_file_location("ghmm_timed", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ghmm_timed"] = mod
    spec.loader.exec_module(mod)
    return mod.ghmm


def rand_model(G, rng, M, D, A):
    iv = rng.uniform(0.5, 2.0, (N, M, D))
    return G.HostModel(A, rng.dirichlet(np.full(M, 3.0), N), rng.normal(0, 1.0, (N, M, D)), iv,
                       np.prod(1.0 / iv, axis=-1))


def banded(rng):
    A = np.zeros((N, N))
    for i in range(N - 1):
        A[i, i] = rng.uniform(0.5, 0.9)
        A[i, i + 1] = 1.0 - A[i, i]
    A[N - 1, N - 1] = 1.0
    return A


def timed(name, call):
    call()      # warm-up (allocations, code objects)
    for rep in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            out = call()
        print(f"{name}, repeat {rep + 1}: {1e3 * (time.perf_counter() - t0) / REPS:.3f} ms", flush=True)
    return out


def close(a, b):
    return np.allclose(a, b, rtol=1e-12, atol=0.0, equal_nan=True)


def main():
    pkg = sys.argv[1] if len(sys.argv) > 1 else "speech-recognition-hmm-continuous_amd"
    G = load(pkg)
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    hosts = []
    for _ in range(K):
        A = banded(rng)
        hosts.append([rand_model(G, rng, M, D, A) for M, D in SHAPES])
    # utterance u walks word u % K: one frame run per state, as long as the states are many
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
        return np.array([ctx.score_streams(w, corpora) for w in vocab])
    lin = timed("loop of ghmm_score_streams", loop)
    if hasattr(ctx, "recognise_streams"):
        blin = timed("ghmm_score_streams_batch", lambda: ctx.score_streams_batch(vocab, corpora))
        assert close(blin, lin)
        timed("loop of ghmm_score_streams, again", loop)

        def by_hand():
            score = ctx.viterbi_streams_batch(vocab, corpora)
            word = np.argmax(score, axis=0).astype(np.int32)
            path = np.empty(U * T, dtype=np.int32)
            for k in np.unique(word):
                pk = ctx.viterbi_streams(vocab[k], corpora)[0].reshape(U, T)
                path.reshape(U, T)[word == k] = pk[word == k]
            return word, path, score
        hand = timed("ghmm_viterbi_streams_batch + argmax + ghmm_viterbi_streams per winner", by_hand)
        dev = timed("ghmm_recognise_streams", lambda: ctx.recognise_streams(vocab, corpora))
        assert np.array_equal(hand[0], dev[0]) and np.array_equal(hand[2], dev[2])
        print(f"distinct winners: {len(np.unique(dev[0]))}, "
              f"utterances won by the word they walk: {int(np.sum(dev[0] == np.arange(U) % K))} of {U}, "
              f"path entries that differ between the two routes: {int(np.sum(hand[1] != dev[1]))} of {U * T}")
    ctx.close()


if __name__ == "__main__":
    main()
