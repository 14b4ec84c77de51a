# ghmm_score_full_batch (the full-covariance recogniser's vocabulary loop) timed with GHMM_OPT_TIMING
# on three shapes; emission rate counted as 2 (D^2 + D) flop per (frame, Gaussian), against the
# measured v_fma_f64 rate (profiles/r1_mfma_f64_rate.txt: 63.9 TFLOP/s).
#   python profiles/tools/fullcov_time.py            (from the repository root)
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from _load import load_pkg  # noqa: E402

G = load_pkg().ghmm
GOLDEN = os.path.join("tests", "golden")
VALU_F64_TFLOPS = 63.9


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


def run(ctx, name, hms, X, lens, reps):
    corpus = ctx.corpus(X, lens)
    fms = [ctx.full_model(h) for h in hms]
    ctx.score_full_batch(fms, corpus)  # warm-up (allocations, code objects)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.score_full_batch(fms, corpus)
    wall = 1e3 * (time.perf_counter() - t0) / reps
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    for _ in range(reps):
        ctx.score_full_batch(fms, corpus)
    kt = ctx.kernel_times()
    ctx.set_option(G.OPT_TIMING, 0)
    em = kt["emission"][0] / reps
    fw = kt["forward"][0] / reps
    F = corpus.frames
    Gs = sum(h.N * h.M for h in hms)
    D = hms[0].D
    tflops = 2.0 * (D * D + D) * F * Gs / (em * 1e-3) / 1e12
    print(f"{name}: {len(hms)} words x {hms[0].N}x{hms[0].M} D={D}, {len(lens)} utterances, {F} frames: "
          f"call {wall:.3f} ms, emission {em:.3f} ms, forward {fw:.3f} ms; emission {tflops:.1f} TFLOP/s "
          f"= {tflops / VALU_F64_TFLOPS:.2f} of the v_fma_f64 rate", flush=True)
    for o in fms + [corpus]:
        o.close()


def main():
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    # (i) the shipped 13-word set on the 13 bundled utterances: latency
    mdir = os.path.join(GOLDEN, "full_cov_models")
    hms = [G.HostFullModel.read(os.path.join(mdir, f)) for f in sorted(os.listdir(mdir)) if f.endswith(".hmm")]
    pdir = os.path.join(GOLDEN, "perfil")
    Xs = [G.perfil_read(os.path.join(pdir, f)) for f in sorted(os.listdir(pdir))]
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
