# The Baum-Welch statistics on the grammar lattice beside the word posteriors, on gpost_time.py's three
# vocabularies and corpora (13 words x 6 states, NS = 78; 64 words x 3 states, NS = 192, the table staged in
# LDS; 256 words x 3 states, NS = 768, the cap on K, the table read from L2; 1 000 utterances each), under
# bigram_log of the spoken strings (alpha = 1).
#   post        ghmm_grammar_post_streams (occ and log P): the emission, then k_gpost_fwd and k_gpost_bwd
#               under GHMM_K_FORWARD (the context's timer holds the two launches' sum)
#   stats       ghmm_estep_grammar_streams and a wait for the stream: the emission with posteriors, k_gpost_fwd
#               and k_gpost_bwd in its statistics form under GHMM_K_FORWARD, the statistics launches and the
#               scatter
# The two alternate in one run under GHMM_OPT_TIMING, after a warm-up call each; per repeat the wall clock of
# the call and the time and launches of the lattice and of GHMM_K_EMISSION, then the median of the repeats with
# min and max.  The spread between the repeats is the run-to-run spread a difference has to exceed.
#   python profiles/tools/gstat_time.py [--post-only] [package directory]      (from the repository root)
# With --post-only, or with the package directory of another build (one without the new call), only `post` is
# timed: the old call's lattice time in a run of the same shape on both builds, to set side by side from one
# session.
import sys
import time

import numpy as np

from grammar_time import SHAPES, banded, load

REPEATS = 7


def run(G, ctx, post_only, K, N, M, D, U, T, SEG):
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
    calls = {"post": lambda: ctx.grammar_post_streams(vocab, corpora, pair, start, fin)}
    stats = None
    if not post_only and hasattr(ctx, "estep_grammar_streams"):
        stats = [[ctx.stats(N, M, D)] for _ in range(K)]

        def estep():
            ctx.estep_grammar_streams(vocab, corpora, pair, stats, start, fin)
            ctx.sync()
        calls["stats"] = estep
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
            v, e = kt["forward"], kt["emission"]
            rows[name].append((wall, v[0], e[0]))
            print(f"{name:6s} repeat {rep + 1}: call {wall:8.3f} ms   forward {v[0]:8.3f} ms in {v[1]} launch(es)   "
                  f"emission {e[0]:8.3f} ms in {e[1]}", flush=True)
    ctx.set_option(G.OPT_TIMING, 0)
    for name, r in rows.items():
        r = np.array(r)
        print(f"{name:6s} median: call {np.median(r[:, 0]):.3f} ms (min {r[:, 0].min():.3f}, max {r[:, 0].max():.3f})   "
              f"forward {np.median(r[:, 1]):.3f} ms (min {r[:, 1].min():.3f}, max {r[:, 1].max():.3f})   "
              f"emission {np.median(r[:, 2]):.3f} ms")
    if stats is not None:
        med = {name: np.median(np.array(r)[:, 1]) for name, r in rows.items()}
        print(f"lattice of stats / lattice of post, medians: {med['stats'] / med['post']:.2f}")
        ll = ctx.fetch(G.BUF_LOGLIK, (U,))
        frames = sum(float(s[0].download()[N * N + N:N * N + 2 * N].sum()) for s in stats)
        print(f"finite log P: {int(np.isfinite(ll).sum())} of {U};  sum of den_c {frames:.3f} on {U * T} frames")
    for o in [m for w in vocab for m in w] + corpora + [s for w in (stats or []) for s in w]:
        o.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--post-only"]
    G = load(args[0] if args else "speech-recognition-hmm-continuous_amd")
    ctx = G.Context(0)
    for shape in SHAPES:
        run(G, ctx, "--post-only" in sys.argv[1:], *shape)
    ctx.close()


if __name__ == "__main__":
    main()
