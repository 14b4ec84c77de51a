# ghmm_estep_full_streams timed with GHMM_OPT_TIMING at shape (ii) of fulltrain_time.py (15 x 5,
# 2 000 x 150 frames) as two feature streams, D = 16 and D = 8, next to ghmm_estep_full on the D = 16
# stream alone.  The single-stream part uses nothing this call added, so the same file times a
# checkout from before it (which then prints that part only):
#   python profiles/tools/fullstreams_time.py [package directory]     (from the repository root)
# REPEATS repeats of REPS calls each, every repeat on its own line: the spread between the lines is
# the run-to-run spread a difference has to exceed.
import importlib.util
import os
import sys
import time

import numpy as np

REPS, REPEATS = 5, 3
KEYS = ("emission", "forward", "backward", "mixstats", "reduce")


def load(pkg_dir):
    spec = importlib.util.spec_from_file_location("ghmm_timed", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ghmm_timed"] = mod
    spec.loader.exec_module(mod)
    return mod.ghmm


def rand_model(G, rng, N, M, D, A=None):
    if A is None:
        A = np.zeros((N, N))
        for i in range(N - 1):
            A[i, i] = rng.uniform(0.5, 0.9)
            A[i, i + 1] = 1.0 - A[i, i]
        A[N - 1, N - 1] = 1.0
    ic = np.empty((N, M, D, D))
    for i in range(N):
        for k in range(M):
            Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
            ic[i, k] = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    return G.HostFullModel(A, rng.dirichlet(np.full(M, 3.0), N), rng.normal(0, 1.0, (N, M, D)), ic,
                           1.0 / np.linalg.det(ic))


def walks(rng, N, lens):
    out = []
    for T in lens:
        cuts = np.sort(rng.choice(np.arange(1, T), N - 1, replace=False))
        out.append(np.searchsorted(cuts, np.arange(T), side="right"))
    return np.concatenate(out)


def frames(rng, hm, st):
    return hm.mean[st, rng.integers(0, hm.M, len(st))] + rng.normal(0.0, 0.5, (len(st), hm.D))


def timed(G, ctx, name, call, poll):
    call()      # warm-up (allocations, code objects)
    poll()
    for rep in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
            poll()
        wall = 1e3 * (time.perf_counter() - t0) / REPS
        ctx.set_option(G.OPT_TIMING, 1)
        ctx.kernel_times_reset()
        for _ in range(REPS):
            call()
        kt = ctx.kernel_times()
        ctx.set_option(G.OPT_TIMING, 0)
        print(f"{name}, repeat {rep + 1}: E-step {wall:.3f} ms; "
              + ", ".join(f"{k} {kt[k][0] / REPS:.3f} ms ({kt[k][1] // REPS} launches)" for k in KEYS), flush=True)


def main():
    pkg = sys.argv[1] if len(sys.argv) > 1 else "speech-recognition-hmm-continuous_amd"
    G = load(pkg)
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    N, M = 15, 5
    lens = np.full(2000, 150, dtype=np.int32)
    # fulltrain_time.py's (ii) in shape and in the model's draws; one state walk serves both streams
    h16 = rand_model(G, rng, N, M, 16)
    st = walks(rng, N, lens)
    X16 = frames(rng, h16, st)
    c16, f16, s16 = ctx.corpus(X16, lens), ctx.full_model(h16), ctx.stats_full(N, M, 16)
    print(f"{pkg}: {N}x{M}, {len(lens)} utterances, {c16.frames} frames")
    timed(G, ctx, "ghmm_estep_full, D = 16", lambda: ctx.estep_full(f16, c16, s16), s16.loglik)
    if hasattr(ctx, "estep_full_streams"):
        h8 = rand_model(G, rng, N, M, 8, h16.A)
        X8 = frames(rng, h8, st)
        c8, f8, s8 = ctx.corpus(X8, lens), ctx.full_model(h8), ctx.stats_full(N, M, 8)
        timed(G, ctx, "ghmm_estep_full, D = 8", lambda: ctx.estep_full(f8, c8, s8), s8.loglik)
        for log in (False, True):
            timed(G, ctx, f"ghmm_estep_full_streams, D = 16 + 8{', log domain' if log else ''}",
                  lambda: ctx.estep_full_streams([f16, f8], [c16, c8], [s16, s8], log=log), s16.loglik)
        timed(G, ctx, "ghmm_estep_full, D = 16, again", lambda: ctx.estep_full(f16, c16, s16), s16.loglik)
    ctx.close()


if __name__ == "__main__":
    main()
