"""ghmm_mstep_full_dev: the full-covariance M-step by HIP kernels on the stream — GPU box only.

1. Parity.  A, c, mean, the matrix slot and det equal ghmm_mstep_full_host's BIT FOR BIT on every case
   of fullmstep_cases.py (uint64 views; on the NaN cases the NaN positions agree and everything else
   is bit-equal).  This is not a measurement: every operation is a correctly rounded IEEE operation,
   uncontracted, in the host's order.  test_fullmstep_host.py shows that the quirk cases reach their
   quirks.
2. The derived constants den, lk and log A, which the device forms itself (sqrt and the device log
   where ghmm_fmodel_set has the host's pow and log), through the three kernels that read them;
   bounds derived at test_derived_constants.
3. Stream order: four EM iterations of estep_full -> loglik -> mstep_full_dev with no other
   synchronisation, against the long-double trajectory, at the bars of
   test_fullestep_gpu.test_four_em_iterations_track_the_extended_reference.
4. The band flag after the step.  5. Refusals and state.  6. The command line under GHMM_DEV_MSTEP=1."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fullmstep_cases as K
import fulltrain_ref as R
from conftest import GOLDEN
from fullcov_support import ctx, recorded  # noqa: F401  (the fixtures)
from fullcov_support import RUNS, SYNTH, TRAIN, U53, check_run, close, code, extended

pytestmark = pytest.mark.gpu

LOG_ULP = 3.0   # the device log / exp: no accuracy table of the device library is installed beside the
#                 compiler, so OpenCL's bound for double log and exp (3 ulp) stands in for it


def dev_mstep(G, ctx, name):
    """the case's model and statistics on the device, after mstep_full_dev: (FullModel, Stats)"""
    hm, v, delta = K.build(G, name)
    fm, st = ctx.full_model(hm), ctx.stats_full(hm.N, hm.M, hm.D)
    try:
        st.upload(v)
        ctx.set_option(G.OPT_DELTA, delta)
        ctx.mstep_full_dev(fm, st)
    except BaseException:
        st.close(); fm.close()
        raise
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
    return fm, st


# ------------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("name", K.ALL)
def test_bitwise_parity_with_the_host_mstep(G, ctx, name):
    ref = K.host_result(G, name)
    fm, st = dev_mstep(G, ctx, name)
    try:
        got = fm.get()
    finally:
        st.close(); fm.close()
    for key in ("A", "c", "mean", "inv_cov", "det"):
        g, r = getattr(got, key), getattr(ref, key)
        if name in K.NAN_CASES:
            assert np.array_equal(np.isnan(g), np.isnan(r)), f"{name}.{key}: NaN positions differ"
            keep = ~np.isnan(r)
            g, r = g[keep], r[keep]
        else:
            assert not np.isnan(r).any(), f"{name}.{key}: list the case in NAN_CASES"
        bad = np.flatnonzero(g.ravel().view(np.uint64) != r.ravel().view(np.uint64))
        assert bad.size == 0, (f"{name}.{key}: {bad.size} of {g.size} entries differ, first at {bad[0]}: "
                               f"{g.ravel()[bad[0]]!r} vs {r.ravel()[bad[0]]!r}")


def test_repeated_steps(G, ctx):
    """a second step from the same vector, with another model's step in between: the skipped state is
    inverted a third time, and no state is carried between calls"""
    name = "q1-den_c-zero"
    hm, v, delta = K.build(G, name)
    ref2 = K.host_result(G, name).mstep(v, delta=delta)     # the skipped state is inverted a third time
    fm, st = dev_mstep(G, ctx, name)
    other, ost = dev_mstep(G, ctx, "pd-6x2x9-delta2")
    try:
        ctx.mstep_full_dev(fm, st)
        got = fm.get()
    finally:
        for o in (st, fm, other, ost):
            o.close()
    for a, b in zip(got.arrays(), ref2.arrays()):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------- 2. derived constants

@functools.lru_cache(maxsize=None)
def constants_corpus(G, name):
    """3 utterances of 20 to 40 frames: left-to-right walks over the NEW means, noise 0.3"""
    out = K.host_result(G, name)
    rng = np.random.default_rng(len(name))
    lens = np.array([20, 33, 40], dtype=np.int32)
    Xs = []
    for T in lens:
        st = np.minimum(np.arange(T) * out.N // T, out.N - 1)
        k = rng.integers(0, out.M, T)
        Xs.append(out.mean[st, k] + rng.normal(0.0, 0.3, (T, out.D)))
    return np.concatenate(Xs), lens


@pytest.mark.parametrize("name", ["pd-6x2x9-delta1", "pd-6x2x48-delta2", "pd-64x2x2-delta2", "q8-negative-det",
                                  "q8-negative-det-m2", "q5-donor-modified"])
def test_derived_constants(G, ctx, name):
    """den, lk and log A after mstep_full_dev (formed on the device) against ghmm_fmodel_set's (host) on
    the SAME fetched parameters: mean, matrix and kernels are identical, only the constants differ.
    u = 2^-53; a correctly rounded operation errs by at most u relative, a function within k ulp by at
    most 2 k u relative.  L = 3: the device log and exp (see LOG_ULP).

    den.  host: pow(|det|, 0.5) within 1 ulp (2u), times aux1 (u): 3u.  device: sqrt (u), times aux1
    (u): 2u.  |den_d - den_h| <= 5u den.  A missing fabs gives NaN for det < 0 (two cases have one).
    b (emission_full).  Each term exp(-aux/2) / den * c: the same exp in both runs, den within 5u, the
    division u per run; the M-term sum of positive terms (one rounding per term, fused or not) M u per
    run:  |b_d - b_h| <= (7 + 2M) u b.
    lk = log(c) - log(den).  host: log within 1 ulp, device within L ulp; log(den) moves by the relative
    error of den (3u, 2u); the subtraction u |lk| per run:
        |lk_d - lk_h| <= u (2 (1 + L) (|log c| + |log den|) + 5 + 2 |lk|) =: dlk
    log b (viterbi_full, GHMM_BUF_B).  F = the kernel's online log-sum-exp of e_m = lk_m - aux_m / 2, the
    same code in both runs, so |F(lk_d) - F(lk_h)| <= max_m dlk_m + 2 E_F with E_F its own rounding:
    e_m one rounding (u |e_m|; for the terms that carry the sum |e_m| <= |log b| + log M, the others'
    errors are damped by exp(e_m - max)), the argument e - max (x exp(-x) <= 1/e: below u/2 per term),
    exp (2 L u per term of a sum in [1, M], so 2 L u relative), M additions (M u), log of a value in
    [1, M] (2 L u log M), the last addition (u |log b|):
        E_F <= u (2 |log b| + log M + 2 L + 1.5 M + 2 L log M)
    log a = log(A).  |d| <= 2 (1 + L) u |log a| =: dla.
    logscore_full.  T frames of la_t(j) = LSE_i(la_{t-1}(i) + log a_ij) + log b_j(t): an input moved by
    d moves an LSE by at most d, so the score moves by at most T (max dlb + max dla) where dlb is the
    bound on log b above; each run's own rounding per frame is two additions (2u S, S = the largest
    |la|, bounded by |score| + the largest |log b|) and an N-term LSE (E_F's form with N for M and S
    for |log b|):
        |score_d - score_h| <= T (max dlb + max dla) + 2 T u (4 S + log N + 2 L + 1.5 N + 2 L log N)
    The worst error / bound ratio of each is printed."""
    X, lens = constants_corpus(G, name)
    fm, st = dev_mstep(G, ctx, name)
    corpus = ctx.corpus(X, lens)
    fm2 = None
    try:
        hm = fm.get()
        N, M, D, F, L = hm.N, hm.M, hm.D, len(X), LOG_ULP
        if name.startswith("q8"):
            assert np.any(hm.det < 0.0)
        fm2 = ctx.full_model(hm)             # ghmm_fmodel_set: the host's constants
        res = []
        for m in (fm, fm2):
            ctx.emission_full(m, corpus)
            b = ctx.fetch(G.BUF_B, (F, N))
            _, vit = ctx.viterbi_full(m, corpus)
            lb = ctx.fetch(G.BUF_B, (F, N))
            res.append((b, lb, vit, ctx.logscore_full(m, corpus, False), ctx.logscore_full(m, corpus, True)))
    finally:
        for o in (fm2, fm, st, corpus):
            if o is not None:
                o.close()
    (b1, lb1, v1, s1, z1), (b2, lb2, v2, s2, z2) = res
    ratios = {}
    # b
    assert np.all(np.isfinite(b2)) and np.all(np.isfinite(b1))
    big = b2 > 1e-290                       # (a relative bound says nothing about subnormals)
    assert big.any() and np.array_equal(b1 == 0.0, b2 == 0.0)
    ratios["b"] = float(np.max(np.abs(b1 - b2)[big] / ((7 + 2 * M) * U53 * b2[big])))
    # log b
    with np.errstate(all="ignore"):
        logc = np.abs(np.log(hm.c))
        den = pow(2.0 * np.pi, D / 2.0) * np.sqrt(np.abs(hm.det))
        logden = np.abs(np.log(den))
        lk = np.abs(np.log(hm.c) - np.log(den))
    dlk = U53 * (2 * (1 + L) * (logc + logden) + 5 + 2 * lk)            # [N][M]
    assert np.all(np.isfinite(lb2)) and np.all(np.isfinite(lb1))
    e_f = U53 * (2 * np.abs(lb2) + np.log(M) + 2 * L + 1.5 * M + 2 * L * np.log(M))
    dlb = dlk.max(1)[None, :] + 2 * e_f                                   # [F][N]
    ratios["log b"] = float(np.max(np.abs(lb1 - lb2) / dlb))
    # log score, both final_state values
    with np.errstate(all="ignore"):
        la = np.where(hm.A > 0.0, np.abs(np.log(np.where(hm.A > 0.0, hm.A, 1.0))), 0.0)
    dla = 2 * (1 + L) * U53 * la.max()
    for key, (g, r) in (("logscore", (s1, s2)), ("logscore final", (z1, z2))):
        assert np.array_equal(np.isfinite(g), np.isfinite(r)) and np.array_equal(g[~np.isfinite(r)], r[~np.isfinite(r)])
        fin = np.isfinite(r)
        if key == "logscore":
            assert fin.all()
        if not fin.any():
            continue
        T = lens[fin].astype(float)
        S = np.abs(r[fin]) + np.abs(lb2).max()
        bound = T * (dlb.max() + dla) + 2 * T * U53 * (4 * S + np.log(N) + 2 * L + 1.5 * N + 2 * L * np.log(N))
        ratios[key] = float(np.max(np.abs(g[fin] - r[fin]) / bound))
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (name, k, v)


# ------------------------------------------------------------------- 3. stream order and trajectory


def em_on_device(G, ctx, case, estep):
    N, M, D, U, T = R.EM_CASES[case]
    X, lens, trace, ref_hm = R.linear_trajectory(G, case)   # computed once for every module
    assert np.all(np.isfinite(trace))
    fm, corpus = ctx.full_model(G.HostFullModel.init_from(X, lens, N, M)), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        got = []
        for _ in range(4):
            estep(fm, corpus, st)
            got.append(st.loglik()[0])     # the stopping rule's 16 bytes: the loop's only wait
            ctx.mstep_full_dev(fm, st)
        hm = fm.get()
    finally:
        st.close(); fm.close(); corpus.close()
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(got, trace))
    e_model = R.model_err(hm, lambda k: getattr(ref_hm, k))
    print(f"{(N, M, D, U * T)} {estep.__name__}: trace error {e_tr:.1e}, model error {e_model:.1e}")
    assert e_tr <= 1e-9
    assert e_model <= 1e-8


@extended
@pytest.mark.parametrize("case", range(len(R.EM_CASES)))
def test_four_em_iterations_on_the_stream(G, ctx, case):
    em_on_device(G, ctx, case, ctx.estep_full)


@extended
def test_four_em_iterations_on_the_stream_log_estep(G, ctx):
    """once, on the second case: there the log-domain E-step in float64 stays 1.5e-10 from the
    long-double trajectory (fullestep_log_ref.EM_MODEL_F64), on the first 8.7e-9, which leaves the
    1e-8 bar no room for the device's order of operations"""
    em_on_device(G, ctx, 1, ctx.estep_full_log)


# ------------------------------------------------------------------- 4. the band flag

@pytest.mark.parametrize("delta", [1, 2])
def test_band_flag_after_the_step(G, ctx, delta):
    """a dense-A model: after the step its A has the band of delta, but the flag only knows "was
    dense" (delta = 1: conservative; delta = 2: must not be band-diagonal).  The next E-step agrees
    with the one of a model SET from the fetched parameters, whose flag ghmm_fmodel_set reads from A."""
    rng = np.random.default_rng(40 + delta)
    N, M, D = 8, 2, 6
    hm = K.rand_model(G, rng, N, M, D, dense=True)
    lens = np.array([60, 45, 81], dtype=np.int32)
    X = np.concatenate([hm.mean[np.minimum(np.arange(T) * N // T, N - 1), rng.integers(0, M, T)]
                        + rng.normal(0.0, 0.3, (T, D)) for T in lens])
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    fm2 = None
    try:
        ctx.set_option(G.OPT_DELTA, delta)
        ctx.estep_full(fm, corpus, st)
        ctx.mstep_full_dev(fm, st)
        ctx.estep_full(fm, corpus, st)
        got = G.split_stats_full(st.download(), N, M, D)
        new = fm.get()
        i, j = np.indices((N, N))
        assert np.all(new.A[(j < i) | (j > i + delta)] == 0.0) and np.all(new.A[(j >= i) & (j <= i + delta)] > 0.0)
        fm2 = ctx.full_model(new)
        ctx.estep_full(fm2, corpus, st)
        ref = G.split_stats_full(st.download(), N, M, D)
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
        for o in (fm2, fm, st, corpus):
            if o is not None:
                o.close()
    assert np.isfinite(float(ref["loglik"]))
    for key in ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_cov"):
        close(got[key], ref[key], zeros=False)
    assert float(got["loglik"]) == pytest.approx(float(ref["loglik"]), rel=1e-11)


# ------------------------------------------------------------------- 5. refusals and state

def test_refusals(G, ctx):
    rng = np.random.default_rng(77)
    hm = K.rand_model(G, rng, 3, 2, 4)
    fm = ctx.full_model(hm)
    diag, other = ctx.stats(3, 2, 4), ctx.stats_full(3, 3, 4)
    wide = K.rand_model(G, rng, 1, K.MCAP + 1, 2)
    wfm, wst = ctx.full_model(wide), ctx.stats_full(1, K.MCAP + 1, 2)
    try:
        assert code(G, lambda: ctx.mstep_full_dev(fm, diag)) == G.ERR_ARG
        assert code(G, lambda: ctx.mstep_full_dev(fm, other)) == G.ERR_ARG
        assert ctx.lib.ghmm_mstep_full_dev(ctx.h, None, other.h) == G.ERR_ARG
        for a, b in zip(fm.get().arrays(), hm.arrays()):
            assert np.array_equal(a, b)
        # M above the cap: refused, nothing launched, the model as it was; the host route takes it
        wst.upload(K.pack(K.pd_sums(rng, 1, K.MCAP + 1, 2)))
        assert code(G, lambda: ctx.mstep_full_dev(wfm, wst)) == G.ERR_UNSUPPORTED
        for a, b in zip(wfm.get().arrays(), wide.arrays()):
            assert np.array_equal(a, b)
        ctx.mstep_full(wfm, wst)
        assert not np.array_equal(wfm.get().mean, wide.mean)
    finally:
        for o in (fm, diag, other, wfm, wst):
            o.close()


@pytest.mark.parametrize("name", ["pd-1x2x9", "pd-6x8x47"])
def test_padded_columns_after_the_step(G, ctx, name):
    """D = 9 and 47 are padded to 16 and 48 columns by k_emission_full; the last Gaussian's padded
    columns read the slack behind mean and inv_cov, which the step must leave as ghmm_fmodel_create
    zeroed it.  The slack cannot be fetched; what shows is that the densities of the stepped model
    are finite and, on frames at the new means, within the bound on b of test_derived_constants of
    those of a fresh model (fresh slack) set from the same parameters."""
    X, lens = constants_corpus(G, name)
    fm, st = dev_mstep(G, ctx, name)
    corpus = ctx.corpus(X, lens)
    fm2 = None
    try:
        hm = fm.get()
        ctx.emission_full(fm, corpus)
        b1 = ctx.fetch(G.BUF_B, (len(X), hm.N))
        fm2 = ctx.full_model(hm)
        ctx.emission_full(fm2, corpus)
        b2 = ctx.fetch(G.BUF_B, (len(X), hm.N))
    finally:
        for o in (fm2, fm, st, corpus):
            if o is not None:
                o.close()
    assert np.all(np.isfinite(b1)) and np.all(b2 > 1e-290)
    assert np.all(np.abs(b1 - b2) <= (7 + 2 * hm.M) * U53 * b2)


# ------------------------------------------------------------------- 6. command line

def test_command_line_dev_mstep(G, recorded, tmp_path):
    """one synthetic recorded run under GHMM_DEV_MSTEP=1: the recorded report and model (check_run),
    and the notice line"""
    name = SYNTH[0]
    run = RUNS[name]
    data = np.load(os.path.join(GOLDEN, "fulltrain_synth.npz"))
    X, lens = data[name + ".X"].astype(np.float64), data[name + ".lens"]
    paths, o = [], 0
    for u, T in enumerate(lens):
        paths.append(str(tmp_path / f"{name}_{u}.perfil"))
        G.perfil_write(paths[-1], X[o:o + T])
        o += T
    tmp = str(tmp_path)
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    out = os.path.join(tmp, "out.hmm")
    p = subprocess.run([TRAIN, name, str(run["N"]), "1", str(run["M"]), lst, out], cwd=tmp, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, GHMM_DEV_MSTEP="1"))
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-2000:]
    assert "M-step on the device (GHMM_DEV_MSTEP)" in text and "M-step on the host" not in text
    check_run(G, recorded, name, run, out, os.path.join(tmp, "out.txt"))
