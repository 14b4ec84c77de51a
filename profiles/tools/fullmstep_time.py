# One EM iteration of the full-covariance trainer with the M-step on the host (ghmm_mstep_full:
# statistics and model down, ghmm_mstep_full_host, model up) against the M-step on the device
# (ghmm_mstep_full_dev), on the three shapes of fulltrain_time.py plus 64 x 8 at D = 48.
# An iteration = estep_full + the 16-byte log P poll + the M-step + ctx.sync(), wall time.  The two
# routes alternate; before every timed iteration the model is set back to the start model (outside
# the timer), so both routes always see the same statistics.  One warm-up iteration per route, then
# REPS timed ones each: min / median / max.  Then the GHMM_K_MSTEP event time of the two new launches
# (GHMM_OPT_TIMING) and the wall time of the host route's M-step call alone.
#   python profiles/tools/fullmstep_time.py            (from the repository root)
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from _load import load_pkg  # noqa: E402

G = load_pkg().ghmm
GOLDEN = os.path.join("tests", "golden")
REPS = 20


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


def fmt(ms):
    ms = np.sort(np.asarray(ms))
    return f"min {ms[0]:.3f} / median {np.median(ms):.3f} / max {ms[-1]:.3f} ms"


def run(ctx, name, hm, X, lens):
    N, M, D = hm.N, hm.M, hm.D
    corpus, fm, st = ctx.corpus(X, lens), ctx.full_model(hm), ctx.stats_full(N, M, D)
    routes = {"host": ctx.mstep_full, "device": ctx.mstep_full_dev}
    wall = {k: [] for k in routes}
    mcall = {k: [] for k in routes}
    for rep in range(REPS + 1):         # rep 0: warm-up (allocations, code objects)
        for key, mstep in routes.items():
            fm.set(hm)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.estep_full(fm, corpus, st)
            st.loglik()
            t1 = time.perf_counter()
            mstep(fm, st)
            ctx.sync()
            t2 = time.perf_counter()
            if rep:
                wall[key].append(1e3 * (t2 - t0))
                mcall[key].append(1e3 * (t2 - t1))
    got = {}
    for key, mstep in routes.items():   # the two routes end in the same model
        fm.set(hm)
        ctx.estep_full(fm, corpus, st)
        mstep(fm, st)
        got[key] = fm.get()
    same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got["host"].arrays(), got["device"].arrays()))
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    for _ in range(REPS):
        fm.set(hm)
        ctx.estep_full(fm, corpus, st)
        ctx.mstep_full_dev(fm, st)
    ctx.sync()
    ev_ms, ev_n = ctx.kernel_times()["mstep"]
    ctx.set_option(G.OPT_TIMING, 0)
    sv = 8 * G.stats_len_full(N, M, D) / 1e6
    mv = 8 * (N * N + N * M * (2 + D + D * D)) / 1e6
    print(f"{name}: {N}x{M} D={D}, {len(lens)} utterances, {corpus.frames} frames "
          f"(statistics {sv:.2f} MB, model {mv:.2f} MB); parameters of the two routes equal: {same}")
    for key in routes:
        print(f"    iteration, M-step on the {key:6s}: {fmt(wall[key])};  M-step call + sync alone: {fmt(mcall[key])}")
    print(f"    GHMM_K_MSTEP events (k_fmstep_gauss + k_fmstep_state): {ev_ms / REPS:.3f} ms per M-step "
          f"({ev_n} launches in {REPS} steps)", flush=True)
    for o in (st, fm, corpus):
        o.close()


def main():
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    # (i) a shipped run: vc_186_f_03_ap_0225, 6 x 1, its TFF initial model, one utterance
    X = G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil"))
    run(ctx, "(i) shipped", G.HostFullModel.init_from(X, [len(X)], 6, 1), X, [len(X)])
    # (ii) 15 x 5 at D = 16 over 2 000 x 150 frames
    hm = rand_model(rng, 15, 5, 16)
    lens = np.full(2000, 150, dtype=np.int32)
    run(ctx, "(ii) 16-d", hm, walk(rng, hm, lens), lens)
    # (iii) 20 x 8 at D = 39 over 1 000 x 300 frames
    hm = rand_model(rng, 20, 8, 39)
    lens = np.full(1000, 300, dtype=np.int32)
    run(ctx, "(iii) 39-d", hm, walk(rng, hm, lens), lens)
    # (iv) 64 x 8 at D = 48 over 1 000 x 300 frames
    hm = rand_model(rng, 64, 8, 48)
    run(ctx, "(iv) 48-d", hm, walk(rng, hm, lens), lens)
    ctx.close()


if __name__ == "__main__":
    main()
