# ghmm_estep_full_log against ghmm_estep_full (the same model, corpus and context) on the three shapes
# of fulltrain_time.py, the two calls alternating inside one run per shape: the whole call (wall clock
# with the 16-byte log P poll), and with GHMM_OPT_TIMING the emission launch (FC_LOGPOST against
# FC_POST), the lattice (k_logfb_fwd + k_logfb_bwd against k_scan_combine, both under "forward") and
# the statistics launches, which are the same kernels.
#   python profiles/tools/fullestep_log_time.py            (from the repository root)
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
sys.path.insert(0, os.path.join("profiles", "tools"))
from _load import load_pkg  # noqa: E402
from fulltrain_time import rand_model, walk  # noqa: E402

G = load_pkg().ghmm
GOLDEN = os.path.join("tests", "golden")
KEYS = ("emission", "forward", "backward", "mixstats", "reduce")


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


def run(ctx, name, hm, X, lens, reps):
    N, M, D = hm.N, hm.M, hm.D
    corpus, fm, st = ctx.corpus(X, lens), ctx.full_model(hm), ctx.stats_full(N, M, D)

    def lin():
        ctx.estep_full(fm, corpus, st)
        return st.loglik()[0]

    def log():
        ctx.estep_full_log(fm, corpus, st)
        return st.loglik()[0]

    (w_lin, w_log), (k_lin, k_log) = timed(ctx, [lin, log], reps)
    ll_lin, ll_log = lin(), log()
    line = lambda kt: ", ".join(f"{k} {kt[k]:.3f} ms" for k in KEYS)  # noqa: E731
    print(f"{name}: {N}x{M} D={D}, {len(lens)} utterances, {corpus.frames} frames "
          f"(loglik linear {ll_lin:.6f}, log {ll_log:.6f})\n"
          f"  estep_full      call {w_lin:.3f} ms: {line(k_lin)}\n"
          f"  estep_full_log  call {w_log:.3f} ms: {line(k_log)}\n"
          f"  ratios log / linear: call {w_log / w_lin:.3f}, emission {k_log['emission'] / k_lin['emission']:.3f}, "
          f"lattice {k_log['forward'] / (k_lin['forward'] + k_lin['backward']):.3f}, "
          f"mixstats {k_log['mixstats'] / k_lin['mixstats']:.3f}", flush=True)
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
