# ghmm_estep_log against ghmm_estep (the same model, corpus and context), the two calls alternating inside
# one run per shape: the whole call (wall clock with the 16-byte log P poll), and with GHMM_OPT_TIMING the
# emission launch (run_emission's mode 3 against mode 0 with posteriors), the lattice (k_logfb_fwd +
# k_logfb_bwd, beyond 64 states k_logfb_wide_fwd + k_logfb_wide_bwd, under "forward", against the linear
# call's launches under "forward" and "backward") and the statistics launches, which are the same kernels.
#   (i)   the benchmark's default: 10 x 8 at D = 39 over 1 000 x 300 frames (bench.py's synthetic corpus)
#   (ii)  20 x 8 at the same D and corpus size
#   (iii) a band-diagonal model of 130 states, 2 mixtures, D = 9, over 256 x 300 frames
#   python profiles/tools/estep_log_time.py            (from the repository root)
# Every shape runs in a child process of its own under a time limit; the first one that fails ends the run.
# REPEATS repeats of REPS rounds each, every repeat on its own line: the spread between the lines is the
# run-to-run spread a difference has to exceed.
import os
import subprocess
import sys
import time

import numpy as np

REPS, REPEATS = 5, 3
KEYS = ("emission", "forward", "backward", "mixstats", "reduce")
SHAPES = ("default", "20x8", "wide130")
LIMIT_S = 300


def timed(G, ctx, fns):
    """the calls of fns in turn, REPS rounds: wall clock per call, then the kernels' times per call"""
    wall = [0.0] * len(fns)
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            wall[i] += 1e3 * (time.perf_counter() - t0) / REPS
    ctx.set_option(G.OPT_TIMING, 1)
    kts = [{} for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            ctx.kernel_times_reset()
            fn()
            for k, v in ctx.kernel_times().items():
                kts[i][k] = kts[i].get(k, 0.0) + v[0] / REPS
    ctx.set_option(G.OPT_TIMING, 0)
    return wall, kts


def run(G, ctx, name, hm, X, lens):
    N, M, D = hm.N, hm.M, hm.D
    corpus, model, st = ctx.corpus(X, lens), ctx.model(hm), ctx.stats(N, M, D)

    def lin():
        ctx.estep(model, corpus, st)
        return st.loglik()[0]

    def log():
        ctx.estep_log(model, corpus, st)
        return st.loglik()[0]

    ll_lin, ll_log = lin(), log()       # warm-up (allocations, code objects)
    print(f"{name}: {N}x{M} D={D}, {len(lens)} utterances, {corpus.frames} frames "
          f"(loglik linear {ll_lin:.6f}, log {ll_log:.6f})", flush=True)
    line = lambda kt: ", ".join(f"{k} {kt.get(k, 0.0):.3f} ms" for k in KEYS)  # noqa: E731
    for rep in range(REPEATS):
        (w_lin, w_log), (k_lin, k_log) = timed(G, ctx, [lin, log])
        print(f"  repeat {rep + 1}\n"
              f"    estep      call {w_lin:.3f} ms: {line(k_lin)}\n"
              f"    estep_log  call {w_log:.3f} ms: {line(k_log)}\n"
              f"    ratios log / linear: call {w_log / w_lin:.3f}, emission {k_log['emission'] / k_lin['emission']:.3f}, "
              f"lattice {k_log['forward'] / (k_lin['forward'] + k_lin.get('backward', 0.0)):.3f}, "
              f"mixstats {k_log['mixstats'] / k_lin['mixstats']:.3f}", flush=True)
    for o in (st, model, corpus):
        o.close()


def banded(rng, n):
    A = np.zeros((n, n))
    for i in range(n - 1):
        A[i, i] = rng.uniform(0.5, 0.9)
        A[i, i + 1] = 1.0 - A[i, i]
    A[n - 1, n - 1] = 1.0
    return A


def child(shape):
    sys.path.insert(0, "tests")
    from _load import load_pkg
    G = load_pkg().ghmm
    ctx = G.Context(0)
    if shape in ("default", "20x8"):
        N = 10 if shape == "default" else 20
        mean, std = G.synth_truth(N, 8, 39)
        lens = np.full(1000, 300, dtype=np.int32)
        X = G.synth_utterances(mean, std, lens, threads=8)
        run(G, ctx, f"({'i' if shape == 'default' else 'ii'}) {shape}", G.synth_start_model(mean, std, 0.05), X, lens)
    else:
        rng = np.random.default_rng(7)
        N, M, D, U, T = 130, 2, 9, 256, 300
        iv = rng.uniform(0.5, 2.0, (N, M, D))
        hm = G.HostModel(banded(rng, N), rng.dirichlet(np.full(M, 3.0), N), rng.normal(0, 1.0, (N, M, D)), iv,
                         np.prod(1.0 / iv, axis=-1))
        # every utterance walks the states left to right, one mixture per frame
        st = np.tile((np.arange(T) * N) // T, U)
        X = hm.mean[st, rng.integers(0, M, U * T)] + rng.normal(0.0, 0.5, (U * T, D))
        run(G, ctx, "(iii) wide130, band-diagonal A", hm, X, np.full(U, T, dtype=np.int32))
    ctx.close()


def main():
    if len(sys.argv) > 1:
        return child(sys.argv[1])
    for shape in SHAPES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), shape], timeout=LIMIT_S)
        if p.returncode != 0:
            sys.exit(f"shape {shape} ended with status {p.returncode}: stopping")


if __name__ == "__main__":
    main()
