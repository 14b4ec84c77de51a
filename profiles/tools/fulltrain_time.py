# ghmm_estep_full (the full-covariance trainer's E-step) timed with GHMM_OPT_TIMING on three shapes;
# k_fullstats counted as 2 (D(D+1)/2 + D + 1) flop per (frame, Gaussian), against the measured
# v_fma_f64 rate (profiles/r1_mfma_f64_rate.txt: 63.9 TFLOP/s).  The kernel skips frames whose
# weights are all exactly 0 for its Gaussians, so the count is nominal: it also says which share of
# the (frame, Gaussian) pairs carried weight.
#   python profiles/tools/fulltrain_time.py            (from the repository root)
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from _load import load_pkg  # noqa: E402

G = load_pkg().ghmm
GOLDEN = os.path.join("tests", "golden")
VALU_F64_TFLOPS = 63.9


def rand_model(rng, N, M, D):
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


def walk(rng, hm, lens):
    out = []
    for T in lens:
        cuts = np.sort(rng.choice(np.arange(1, T), hm.N - 1, replace=False))
        st = np.searchsorted(cuts, np.arange(T), side="right")
        k = rng.integers(0, hm.M, T)
        out.append(hm.mean[st, k] + rng.normal(0.0, 0.5, (T, hm.D)))
    return np.concatenate(out)


def run(ctx, name, hm, X, lens, reps):
    N, M, D = hm.N, hm.M, hm.D
    corpus, fm, st = ctx.corpus(X, lens), ctx.full_model(hm), ctx.stats_full(N, M, D)
    ctx.estep_full(fm, corpus, st)  # warm-up (allocations, code objects)
    st.loglik()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.estep_full(fm, corpus, st)
        st.loglik()
    wall = 1e3 * (time.perf_counter() - t0) / reps
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    for _ in range(reps):
        ctx.estep_full(fm, corpus, st)
    kt = ctx.kernel_times()
    ctx.set_option(G.OPT_TIMING, 0)
    F = corpus.frames
    gamma = ctx.fetch(G.BUF_GAMMA, (F, N))
    live = float(np.mean(gamma != 0.0))
    ms = {k: kt[k][0] / reps for k in ("emission", "forward", "backward", "mixstats", "reduce")}
    E = D * (D + 1) // 2 + D + 1
    tflops = 2.0 * E * F * N * M / (ms["mixstats"] * 1e-3) / 1e12
    print(f"{name}: {N}x{M} D={D}, {len(lens)} utterances, {F} frames: E-step {wall:.3f} ms; "
          + ", ".join(f"{k} {v:.3f} ms" for k, v in ms.items())
          + f"; k_fullstats {tflops:.1f} TFLOP/s nominal = {tflops / VALU_F64_TFLOPS:.2f} of the v_fma_f64 rate"
          f" (gamma != 0 on {100 * live:.1f} % of (frame, state))", flush=True)
    for o in (st, fm, corpus):
        o.close()


def main():
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    # (i) a shipped run: vc_186_f_03_ap_0225, 6 x 1, its TFF initial model, one utterance
    X = G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil"))
    run(ctx, "(i) shipped", G.HostFullModel.init_from(X, [len(X)], 6, 1), X, [len(X)], 50)
    # (ii) 15 x 5 at D = 16 over 2 000 x 150 frames
    hm = rand_model(rng, 15, 5, 16)
    lens = np.full(2000, 150, dtype=np.int32)
    run(ctx, "(ii) 16-d", hm, walk(rng, hm, lens), lens, 5)
    # (iii) 20 x 8 at D = 39 over 1 000 x 300 frames
    hm = rand_model(rng, 20, 8, 39)
    lens = np.full(1000, 300, dtype=np.int32)
    run(ctx, "(iii) 39-d", hm, walk(rng, hm, lens), lens, 5)
    ctx.close()


if __name__ == "__main__":
    main()
