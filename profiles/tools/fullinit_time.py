# The full-covariance trainer's initial model on the host (ghmm_init_model_full, then ghmm_fmodel_set:
# what the trainer does without GHMM_DEV_INIT) against the device (ghmm_fmodel_init), on the three shapes
# of fulltrain_time.py.  Wall time, the corpus already uploaded (both routes need it for the E-step), each
# route ending in ctx.sync().  The two routes alternate in one run; one warm-up each, then REPS timed
# ones each: min / median / max.  Then the GHMM_OPT_TIMING event time per kernel class of the device
# route, and one EM iteration (estep_full + the 16-byte log P poll + mstep_full_dev + sync, median of
# REPS) for the init's share of a six-iteration job before and after.
#   python profiles/tools/fullinit_time.py            (from the repository root)
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
sys.path.insert(0, os.path.join("profiles", "tools"))
from _load import load_pkg  # noqa: E402
from fullmstep_time import fmt, rand_model, walk  # noqa: E402

G = load_pkg().ghmm
GOLDEN = os.path.join("tests", "golden")
REPS = 5


def run(ctx, name, N, M, X, lens):
    D = X.shape[1]
    corpus, st = ctx.corpus(X, lens), ctx.stats_full(N, M, D)
    fm = ctx.full_model(G.HostFullModel(np.eye(N), np.full((N, M), 1.0 / M), np.zeros((N, M, D)),
                                        np.tile(np.eye(D), (N, M, 1, 1)), np.ones((N, M))))

    def host():
        fm.set(G.HostFullModel.init_from(X, lens, N, M))

    def device():
        fm.init_from(corpus, fetch=False)

    routes = {"host": host, "device": device}
    wall = {k: [] for k in routes}
    got = {}
    for rep in range(REPS + 1):         # rep 0: warm-up (allocations, code objects)
        for key, route in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            route()
            ctx.sync()
            t1 = time.perf_counter()
            if rep:
                wall[key].append(1e3 * (t1 - t0))
            got[key] = fm.get()
    worst = 0.0
    for a, b in zip(got["host"].arrays(), got["device"].arrays()):
        fin = np.isfinite(a) & (a != 0)
        worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / np.abs(a[fin]), initial=0.0)))
    same_c = np.array_equal(got["host"].c, got["device"].c, equal_nan=True)
    ctx.set_option(G.OPT_TIMING, 1)
    ctx.kernel_times_reset()
    for _ in range(REPS):
        device()
    ctx.sync()
    ev = ctx.kernel_times()
    ctx.set_option(G.OPT_TIMING, 0)
    it = []
    for rep in range(REPS + 1):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.estep_full(fm, corpus, st)
        st.loglik()
        ctx.mstep_full_dev(fm, st)
        ctx.sync()
        if rep:
            it.append(1e3 * (time.perf_counter() - t0))
    it_ms = float(np.median(it))
    print(f"{name}: {N}x{M} D={D}, {len(lens)} utterances, {corpus.frames} frames; weights of the two routes "
          f"bit-equal: {same_c}; largest relative difference of any parameter: {worst:.2e}")
    for key in routes:
        print(f"    initial model on the {key:6s}: {fmt(wall[key])}")
    # the classes of GHMM_OPT_TIMING: "prepare" holds k_finit_pass alone (one launch per k-means pass and the
    # last classification), "reduce" k_finit_cells once per k-means pass plus one k_fullstats_reduce,
    # "mixstats" the one k_fullstats, "mstep" k_finit_gauss + k_finit_state
    print("    events per device init: " + ", ".join(
        f"{k} {ev[k][0] / REPS:.3f} ms ({ev[k][1] // REPS} launches)" for k in ("prepare", "reduce", "mixstats", "mstep")))
    print(f"    one k_finit_pass: {ev['prepare'][0] / max(ev['prepare'][1], 1):.4f} ms (mean over its launches)")
    for key in routes:
        ini = float(np.median(wall[key]))
        print(f"    six-iteration job, init on the {key:6s}: {ini + 6 * it_ms:.3f} ms "
              f"(iteration {it_ms:.3f} ms), the init is {100 * ini / (ini + 6 * it_ms):.1f} % of it", flush=True)
    for o in (st, fm, corpus):
        o.close()


def main():
    ctx = G.Context(0)
    rng = np.random.default_rng(7)
    # (i) a shipped run: vc_186_f_03_ap_0225, 6 x 1, one utterance
    X = G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil"))
    run(ctx, "(i) shipped", 6, 1, X, np.array([len(X)], dtype=np.int32))
    # (ii) 15 x 5 at D = 16 over 2 000 x 150 frames
    hm = rand_model(rng, 15, 5, 16)
    lens = np.full(2000, 150, dtype=np.int32)
    run(ctx, "(ii) 16-d", 15, 5, walk(rng, hm, lens), lens)
    # (iii) 20 x 8 at D = 39 over 1 000 x 300 frames
    hm = rand_model(rng, 20, 8, 39)
    lens = np.full(1000, 300, dtype=np.int32)
    run(ctx, "(iii) 39-d", 20, 8, walk(rng, hm, lens), lens)
    ctx.close()


if __name__ == "__main__":
    main()
