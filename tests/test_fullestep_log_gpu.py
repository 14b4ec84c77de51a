"""The full-covariance log-domain E-step (ghmm_estep_full_log: k_emission_full<DB, FC_LOGPOST>,
k_logfb<L>, then ghmm_estep_full's statistics launches) on the MI355X — GPU box only.  The numpy
restatement it is held against (fullestep_log_ref.py) is pinned on the CPU by
test_fullestep_log_host.py; the bounds are derived in that module's docstring.

  emission   log b = ghmm_viterbi_full's, bitwise, at every DB; post against the long-double
             restatement with log b's 1e-11 (1 + |ref|) carried into the exponent
  lattice    the long-double recursion run on the DEVICE's own log b: la, lbe, log P inside
             fulllogscore_ref.lattice_bound, gamma and the transition sums inside the expm1(E) bounds
  statistics fullcov_support.check_stats_bound on the device's own gamma and post
  the point  a far frame in every utterance: ghmm_estep_full's loglik is not finite, this call's
             statistics are, and the M-step of them does not lower the next log-likelihood
  four EM iterations against the long-double LINEAR trajectory; plumbing; the command line"""
import os
import subprocess

import numpy as np
import pytest

import fullestep_log_ref as LE
import fulllogscore_ref as LR
import fulltrain_ref as R
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import (RUNS, SHIPPED, TRAIN, U53, check_estep, check_log_lattice, check_stats_bound, code,
                             extended, offsets, rand_fmodel, rel_dist, run_device, walk_any)
from fulltrain_ref import LENS1

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------- emission

@extended
@pytest.mark.parametrize("D", [8, 9, 17, 24, 25, 33, 40, 41, 47, 48])
def test_emission_every_db(G, ctx, D):
    """5 x 3 x D, 233 frames (three tiles of 64 and one of 41), frame 40 moved 60 units away"""
    rng = np.random.default_rng(500 + D)
    N, M = 5, 3
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    X = walk_any(rng, hm, LENS1)
    X[40] += 60.0
    dev = run_device(G, ctx, hm, X, LENS1, log=True)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, LENS1)
    try:
        ctx.viterbi_full(fm, corpus)
        vit = ctx.fetch(G.BUF_B, (len(X), N))
    finally:
        fm.close(); corpus.close()
    assert np.isfinite(vit).all()
    assert np.array_equal(dev["logb"].view(np.uint64), vit.view(np.uint64))
    logb, post, e = LE.emission(hm, X, np.longdouble)
    ref = np.asarray(post, dtype=np.float64).reshape(len(X), N * M)
    got = dev["post"]
    assert np.array_equal(got == 0.0, ref == 0.0), "zeros of post differ"
    mag = np.maximum(np.abs(e), np.abs(logb)[..., None]).reshape(len(X), N * M)
    tol = post.reshape(len(X), N * M) * np.expm1(2e-11 * (1 + mag)) + 2.0 ** -52
    err = np.abs(got.astype(np.longdouble) - post.reshape(len(X), N * M))
    print(f"D = {D}: post worst error / bound {float((err / tol).max()):.3g}")
    assert np.all(err <= tol)
    assert np.all(dev["post"][40].reshape(N, M).sum(1) == pytest.approx(1.0, rel=1e-9))   # the far frame too


# ------------------------------------------------------------------- the lattice

LATTICE_IDS = LE.LATTICE_CASES + [f"empty_dense_delta{d}" for d in LE.EMPTY_DELTAS]


def make(G, name):
    if name.startswith("empty_dense_delta"):
        return LE.make_empty_case(G) + (int(name[-1]),)
    return LR.make_case(G, name) + (1,)


def check_sums(dev, ref, N, delta, lens, what):
    """num_a, den_a, den_c against the per-utterance long-double terms: every term inside its
    expm1(E) bound, plus (T_total + U) 2^-53 sum|terms| for the order of the additions"""
    T_total, U = int(np.sum(lens)), len(lens)
    tol = {k: np.zeros_like(ref["stats"][k]) for k in ("num_a", "den_a", "den_c")}
    for ut in ref["utt"]:
        T = ut["T"]
        if T == 0:
            continue
        E = np.longdouble(LE.gamma_exponent_bound(T, N, ut["V"], ut["La"]))
        g = ut["gamma"]
        tol["num_a"] += ut["xi"] * np.expm1(E) + (ut["xi"] != 0) * (T - 1) * 4 * U53
        tol["den_a"] += g[:-1].sum(0) * np.expm1(E) + (T - 1) * 4 * U53
        tol["den_c"] += g.sum(0) * np.expm1(E) + T * 4 * U53
    worst = 0.0
    for k in tol:
        r = ref["stats"][k]
        t = tol[k] + (T_total + U) * U53 * r
        got = dev["stats"][k].reshape(r.shape).astype(np.longdouble)
        assert np.all(np.isfinite(dev["stats"][k])), (what, k)
        err = np.abs(got - r)
        assert np.all(err <= t), (what, k, float((err / np.where(t > 0, t, 1)).max()))
        worst = max(worst, float((err / np.where(t > 0, t, 1)).max()))
    i, j = np.indices((N, N))
    assert np.all(dev["stats"]["num_a"].reshape(N, N)[(j < i) | (j > i + delta)] == 0.0), f"{what}: num_a outside the band"
    return worst


def check_against_own_logb(G, dev, hm, X, lens, delta, what):
    """the long-double recursion on the device's own log b and post; returns the reference"""
    N = hm.N
    ref = LE.estep(hm, X, lens, delta, np.longdouble, logb=dev["logb"], post=dev["post"])
    off = offsets(lens)
    worst = 0.0
    for u, ut in enumerate(ref["utt"]):
        s = slice(off[u], off[u + 1])
        got = {"la": dev["la"][s], "lbe": dev["lbe"][s], "logP": dev["ll"][u], "gamma": dev["gamma"][s]}
        if ut["T"] == 0:
            assert dev["ll"][u] == 0.0
            continue
        worst = max(worst, check_log_lattice(f"{what}[{u}]", N, got, ut, what="GPU", xi=False))
        # a frame's gammas sum to rho_u
        if np.isfinite(ut["logZ"]):
            rho = np.exp(ut["logP"] - ut["logZ"])
            E = np.longdouble(LE.gamma_exponent_bound(ut["T"], N, ut["V"], ut["La"]))
            ssum = dev["gamma"][s].astype(np.longdouble).sum(1)
            assert np.all(np.abs(ssum - rho) <= rho * np.expm1(E) + N * 4 * U53), (what, u)
        else:
            assert np.all(dev["gamma"][s] == 0.0)
    w2 = check_sums(dev, ref, N, delta, lens, what)
    # n_utt exact; the summed loglik keeps the per-utterance pattern
    assert float(dev["stats"]["n_utt"]) == float(len(lens))
    total, rt = float(dev["stats"]["loglik"]), ref["stats"]["loglik"]
    assert np.isnan(total) == bool(np.isnan(rt)) and np.isinf(total) == bool(np.isinf(rt))
    if np.isfinite(rt):
        bound = sum(LR.lattice_bound(ut["T"], N, ut["V"], ut["La"]) for ut in ref["utt"] if ut["T"])
        bound += len(lens) * U53 * float(np.abs(ref["loglik"]).sum())
        assert abs(np.longdouble(total) - rt) <= bound, what
    else:
        assert total == float(rt)
    print(f"{what}: lattice worst error / bound {worst:.4f}, sums {w2:.4f}")
    return ref


@extended
@pytest.mark.parametrize("name", LATTICE_IDS)
def test_lattice_on_the_devices_own_log_b(G, ctx, name):
    hm, X, lens, delta = make(G, name)
    dev = run_device(G, ctx, hm, X, lens, log=True, delta=delta)
    ref = check_against_own_logb(G, dev, hm, X, lens, delta, name)
    ll = np.asarray(ref["loglik"], dtype=np.float64)
    if name == "c0_banded":
        assert (dev["ll"] == -np.inf).all() and np.all(dev["gamma"] == 0.0)
    elif not name.startswith(("c0", "empty")) and not LR.CASES[name][3]:
        short = np.asarray(lens) < hm.N
        assert (ll[short] == -np.inf).all() and np.isfinite(ll[~short]).all()
        off = offsets(lens)
        for u in np.nonzero(short)[0]:
            assert np.all(dev["gamma"][off[u]:off[u + 1]] == 0.0)
    if name.startswith("empty"):
        assert dev["ll"][1] == 0.0 and not np.signbit(dev["ll"][1])


# ------------------------------------------------------------------- statistics

@extended
@pytest.mark.parametrize("name", ["l16_banded", "wide_64x2x48"])
def test_statistics_within_the_derived_bound(G, ctx, name):
    hm, X, lens, delta = make(G, name)
    dev = run_device(G, ctx, hm, X, lens, log=True, delta=delta)
    worst = check_stats_bound(dev, X, hm, name)
    print(f"{name}: statistics worst error / bound {worst:.4f}")


# ------------------------------------------------------------------- the point of the feature

@extended
def test_far_frames_train_where_the_linear_call_cannot(G, ctx):
    rng = np.random.default_rng(61)
    N, M, D = 5, 2, 8
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    lens = np.array([60, 45, 81, 70], dtype=np.int32)
    X = walk_any(rng, hm, lens)
    off = offsets(lens)
    for u in range(len(lens)):
        X[off[u] + 7 + 3 * u] += 60.0        # a far frame in every utterance
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.estep_full(fm, corpus, st)
        assert not np.isfinite(st.loglik()[0])          # the linear call is lost here
        ctx.estep_full_log(fm, corpus, st)
        v = st.download()
        assert np.all(np.isfinite(v))
        ll0 = st.loglik()[0]
        ctx.mstep_full(fm, st)
        new = fm.get()
        for a in new.arrays():
            assert np.all(np.isfinite(a))
        ctx.estep_full_log(fm, corpus, st)
        ll1 = st.loglik()[0]
        print(f"far frames: loglik {ll0:.3f} -> {ll1:.3f}")
        assert np.isfinite(ll1) and ll1 >= ll0
    finally:
        st.close(); fm.close(); corpus.close()
    dev = run_device(G, ctx, hm, X, lens, log=True)
    assert np.array_equal(dev["v"].view(np.uint64), v.view(np.uint64))
    check_against_own_logb(G, dev, hm, X, lens, 1, "far frames")
    check_stats_bound(dev, X, hm, "far frames")
    # end to end from X: the log-likelihood at test_fulllogscore_gpu's bar, the posteriors at the emission test's
    ref = LE.estep(hm, X, lens, 1, np.longdouble)
    r64 = LE.estep(hm, X, lens, 1, np.float64)
    d64 = rel_dist(r64["loglik"], ref["loglik"])
    d = rel_dist(dev["ll"], ref["loglik"])
    print(f"far frames: loglik GPU {d:.2e}, float64 restatement {d64:.2e}")
    assert d <= max(8.0 * d64, 1e-11)


# ------------------------------------------------------------------- four EM iterations

@extended
@pytest.mark.parametrize("case", range(len(R.EM_CASES)))
def test_four_em_iterations_track_the_linear_trajectory(G, ctx, case):
    """trace rel 1e-9 (the project's bar); model max(1e-8, 8 x EM_MODEL_F64[case]): 8 x for the device
    taking the float64 restatement's operations in another order"""
    N, M, D, U, T = R.EM_CASES[case]
    X, lens, trace, ref_hm = R.linear_trajectory(G, case)
    assert np.all(np.isfinite(trace))
    fm, corpus = ctx.full_model(G.HostFullModel.init_from(X, lens, N, M)), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        got = []
        for _ in range(4):
            ctx.estep_full_log(fm, corpus, st)
            got.append(st.loglik()[0])
            ctx.mstep_full(fm, st)
        hm = fm.get()
    finally:
        st.close(); fm.close(); corpus.close()
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(got, trace))
    e_model = R.model_err(hm, lambda k: getattr(ref_hm, k))
    bar = max(1e-8, 8 * LE.EM_MODEL_F64[case])
    print(f"{(N, M, D, U * T)}: trace error {e_tr:.1e}, model error {e_model:.1e} (bar {bar:.1e})")
    assert e_tr <= 1e-9
    assert e_model <= bar


# ------------------------------------------------------------------- plumbing

def test_reproducible_and_partials(G, ctx):
    """two calls give bit-equal vectors; GHMM_OPT_PARTIALS 1 / 3 / 0 leave gamma and post bit-equal"""
    hm, X, lens, delta = make(G, "l32_banded")
    first = None
    for partials in (1, 3, 0):
        dev = run_device(G, ctx, hm, X, lens, log=True, delta=delta, options=((G.OPT_PARTIALS, partials),), twice=True)
        if first is None:
            first = dev
        else:
            for k in ("gamma", "post", "logb", "la", "lbe", "ll"):
                assert np.array_equal(dev[k], first[k], equal_nan=True), (partials, k)


def test_empty_corpus(G, ctx):
    rng = np.random.default_rng(41)
    N, M, D = 4, 2, 6
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    fm = ctx.full_model(hm)
    st = ctx.stats_full(N, M, D)
    busy = ctx.corpus(walk_any(rng, hm, [30]), [30])
    empty = ctx.corpus(np.zeros((0, D)), np.zeros(0, dtype=np.int32))
    try:
        ctx.estep_full_log(fm, busy, st)
        assert np.any(st.download() != 0.0)
        ctx.estep_full_log(fm, empty, st)
        assert np.all(st.download() == 0.0)
    finally:
        for o in (st, fm, busy, empty):
            o.close()


def test_refusals(G, ctx):
    rng = np.random.default_rng(43)
    N, M, D = 4, 2, 6
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    fm = ctx.full_model(hm)
    corpus = ctx.corpus(walk_any(rng, hm, [30]), [30])
    st, diag = ctx.stats_full(N, M, D), ctx.stats(N, M, D)
    try:
        assert code(G, lambda: ctx.estep_full_log(fm, corpus, diag)) == G.ERR_ARG
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert code(G, lambda: ctx.estep_full_log(fm, corpus, st)) == G.ERR_UNSUPPORTED
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        ctx.set_option(G.OPT_TIMING, 1)
        ctx.kernel_times_reset()
        try:
            ctx.estep_full_log(fm, corpus, st)
            kt = ctx.kernel_times()
        finally:
            ctx.set_option(G.OPT_TIMING, 0)
        assert kt["emission"][1] == 1 and kt["forward"][1] == 1 and kt["backward"][1] == 0   # the lattice: GHMM_K_FORWARD
    finally:
        for o in (st, diag, fm, corpus):
            o.close()


@extended
def test_linear_estep_afterwards_is_unchanged(G, ctx):
    """no stale log state leaks: estep_full after estep_full_log on the same context still meets its
    own reference"""
    name = "paths-8x3x16"
    assert name in R.CASES
    hm, X, lens, delta, ref = R.build(G, name)
    run_device(G, ctx, hm, X, lens, log=True, delta=delta)
    N, M, D = hm.N, hm.M, hm.D
    F, U = len(X), len(lens)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.estep_full_log(fm, corpus, st)
        ctx.estep_full(fm, corpus, st)
        v = st.download()
        dev = dict(v=v, stats=G.split_stats_full(v, N, M, D), b=ctx.fetch(G.BUF_B, (F, N)),
                   post=ctx.fetch(G.BUF_POST, (F, N * M)), gamma=ctx.fetch(G.BUF_GAMMA, (F, N)),
                   ll=ctx.fetch(G.BUF_LOGLIK, (U,)))
        beta = ctx.fetch(G.BUF_BETA, (F, N))       # the linear call's on-demand pass still works
    finally:
        st.close(); fm.close(); corpus.close()
    check_estep(dev, ref, hm, lens, delta, name)
    check_stats_bound(dev, X, hm, name)
    np.testing.assert_allclose(beta, np.asarray(ref["beta"], dtype=np.float64), rtol=1e-9,
                               atol=1e-9 * float(np.abs(ref["beta"]).max()))


# ------------------------------------------------------------------- command line

def test_command_line_log_train(G, ctx, tmp_path):
    """hmm-continuous-train-full-fs with GHMM_LOG_TRAIN=1 on one shipped word: the model written =
    init_model_full, then (estep_full_log, mstep_full) under the program's stopping rule, array for
    array; the notice line is printed"""
    name = SHIPPED[0]
    paths = [os.path.join(GOLDEN, "perfil", f) for f in RUNS[name]["perfils"]]
    tmp = str(tmp_path)
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    out = os.path.join(tmp, "out.hmm")
    p = subprocess.run([TRAIN, name, "6", "1", "1", lst, out], cwd=tmp, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, GHMM_LOG_TRAIN="1"))
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-2000:]
    assert "E-step in the log domain (GHMM_LOG_TRAIN)" in text
    iterations = int(next(l for l in open(os.path.join(tmp, "out.txt")).read().split("\n")
                          if l.startswith("number of iterations")).split(":")[1])
    Xs = [G.perfil_read(f) for f in paths]
    X, lens = np.concatenate(Xs), np.array([len(x) for x in Xs], dtype=np.int32)
    fm, corpus = ctx.full_model(G.HostFullModel.init_from(X, lens, 6, 1)), ctx.corpus(X, lens)
    st = ctx.stats_full(6, 1, X.shape[1])
    try:
        old, n = 1.0, 0
        while True:
            n += 1
            ctx.estep_full_log(fm, corpus, st)
            probab = st.loglik()[0]
            if not abs((old - probab) / old) > 1.0e-3:
                break
            old = probab
            ctx.mstep_full(fm, st)
        hm = fm.get()
    finally:
        st.close(); fm.close(); corpus.close()
    assert n == iterations
    got = G.HostFullModel.read(out)
    assert got.word == name
    for a, b in zip(got.arrays(), hm.arrays()):
        np.testing.assert_array_equal(a, b)
