# ghmm_logscore_full_batch against ghmm_viterbi_full_batch (the same vocabulary, corpus and context) on
# the three shapes of fullviterbi_time.py, the two calls alternating inside one run per shape: the
# whole call (wall clock), and with GHMM_OPT_TIMING the log-emission launch of either call (the same
# kernel) and k_logforward_multi against k_viterbi_multi.
#   python profiles/tools/fulllogscore_time.py            (from the repository root)
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from _load import load_pkg  # noqa: E402

G = load_pkg().ghmm
GOLDEN = os.path.join("tests", "golden")


def rand_model(rng, N, M, D, base):
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
    return G.HostFullModel(A, rng.dirichlet(np.full(M, 3.0), N), base + rng.normal(0, 0.5, (N, M, D)), ic,
                           1.0 / np.linalg.det(ic))


def timed(ctx, fns, reps):
    """the calls of fns in turn, reps rounds: wall clock per call, then the kernels' times per call"""
    for fn in fns:
        fn()  # warm-up (allocations, code objects)
    ctx.sync()
    wall = [0.0] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            wall[i] += 1e3 * (time.perf_counter() - t0) / reps
    ctx.set_option(G.OPT_TIMING, 1)
    kts = [{} for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ctx.kernel_times_reset()
            fn()
            for k, v in ctx.kernel_times().items():
                kts[i][k] = kts[i].get(k, 0.0) + v[0] / reps
    ctx.set_option(G.OPT_TIMING, 0)
    return wall, kts


def run(ctx, name, hms, X, lens, reps):
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    (vt_wall, l0_wall, l1_wall), (vt, l0, l1) = timed(
        ctx, [lambda: ctx.viterbi_full_batch(fms, corpus), lambda: ctx.logscore_full_batch(fms, corpus),
              lambda: ctx.logscore_full_batch(fms, corpus, final_state=True)], reps)
    fin = np.isfinite(ctx.logscore_full_batch(fms, corpus)).mean()
    print(f"{name}: {len(hms)} words x {hms[0].N}x{hms[0].M} D={hms[0].D}, {len(lens)} utterances, "
          f"{corpus.frames} frames (finite log scores: {fin:.3f})\n"
          f"  viterbi_full_batch            call {vt_wall:.3f} ms: log emission {vt['emission']:.3f} ms, "
          f"k_viterbi_multi {vt['viterbi']:.3f} ms\n"
          f"  logscore_full_batch           call {l0_wall:.3f} ms: log emission {l0['emission']:.3f} ms, "
          f"k_logforward_multi {l0['forward']:.3f} ms\n"
          f"  logscore_full_batch (final)   call {l1_wall:.3f} ms: log emission {l1['emission']:.3f} ms, "
          f"k_logforward_multi {l1['forward']:.3f} ms\n"
          f"  call {l0_wall / vt_wall:.3f}, log emission {l0['emission'] / vt['emission']:.3f}, "
          f"k_logforward_multi / k_viterbi_multi {l0['forward'] / vt['viterbi']:.3f}", flush=True)
    for o in fms + [corpus]:
        o.close()


def main():
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    # (i) the shipped 13-word set on the 13 bundled utterances: latency
    mdir = os.path.join(GOLDEN, "full_cov_models")
    hms = [G.HostFullModel.read(os.path.join(mdir, f)) for f in sorted(os.listdir(mdir)) if f.endswith(".hmm")]
    pdir = os.path.join(GOLDEN, "perfil")
    Xs = [G.perfil_read(os.path.join(pdir, f)) for f in sorted(os.listdir(pdir)) if f.endswith(".perfil")]
    run(ctx, "(i) shipped", hms, np.concatenate(Xs), [len(x) for x in Xs], 20)
    # (ii) 50 words x 15 x 5 x 16 over 2 000 x 150 frames: the reference recogniser's capacity limits
    base = rng.normal(0, 1.5, 16)
    hms = [rand_model(rng, 15, 5, 16, base) for _ in range(50)]
    lens = np.full(2000, 150, dtype=np.int32)
    run(ctx, "(ii) capacity", hms, base + rng.normal(0, 1, (int(lens.sum()), 16)), lens, 5)
    # (iii) one 20 x 8 x 39 model over 300 000 frames (BASELINE's emission scale)
    base = rng.normal(0, 1.5, 39)
    hms = [rand_model(rng, 20, 8, 39, base)]
    lens = np.full(1000, 300, dtype=np.int32)
    run(ctx, "(iii) 39-d", hms, base + rng.normal(0, 1, (int(lens.sum()), 39)), lens, 5)
    ctx.close()


if __name__ == "__main__":
    main()
