"""The full-covariance calls on several feature streams (ghmm_estep_full_streams, ghmm_score_full_streams,
ghmm_logscore_full_streams: k_emission_full's FOLD epilogue, the single-stream recursions on the
product, the statistics launches per stream) and the two command lines on two-stream models — GPU box
only.  The reference is tests/fullstreams_ref.py, pinned on the CPU by test_fullstreams_host.py to the
real reference's recorded two-stream runs.  Tolerances are the single-stream suites': fullcov_support's
check_estep, check_log_lattice, close_logb at 1e-11, same_kind_close, and assert_close at RTOL.

GHMM_BUF_POST is not part of the contract for several streams, so where check_estep wants the device's
posteriors the reference's own, rounded to double, stand in: that part of it compares nothing here.  The
posteriors are covered through num_c, num_mu and num_cov of every stream's statistics vector."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fullstreams_ref as S
import fulltrain_ref as R
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import (RECOGNISE, RTOL, TRAIN, assert_close, check_blocks, check_estep, check_log_lattice,
                             close_logb, code, extended, f64, offsets, rand_fmodel, report_value, same_kind_close,
                             spoken_blocks, walk_any)
from streams_util import second_stream

pytestmark = pytest.mark.gpu

P2 = json.load(open(os.path.join(GOLDEN, "fullstreams_p2.json")))
STAT_KEYS = R.STAT_KEYS + ("loglik", "n_utt")


def bits_equal(a, b):
    """bitwise equal where neither is NaN, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


class Streams:
    """device models, corpora and statistics vectors of a several-stream case"""

    def __init__(self, ctx, hms, Xs, lens):
        self.fms = [ctx.full_model(h) for h in hms]
        self.corpora = [ctx.corpus(X, lens) for X in Xs]
        self.sts = [ctx.stats_full(h.N, h.M, h.D) for h in hms]

    def close(self):
        for o in self.sts + self.fms + self.corpora:
            o.close()


def run_streams(G, ctx, hms, Xs, lens, *, log, delta=1, twice=False):
    """estep_full_streams; everything the tests look at, downloaded (BUF_B as "b" or "logb")"""
    N, F, U = hms[0].N, len(Xs[0]), len(lens)
    d = Streams(ctx, hms, Xs, lens)
    try:
        ctx.set_option(G.OPT_DELTA, delta)
        ctx.estep_full_streams(d.fms, d.corpora, d.sts, log=log)
        vs = [s.download() for s in d.sts]
        out = dict(vs=vs, stats=[G.split_stats_full(v, h.N, h.M, h.D) for v, h in zip(vs, hms)])
        out["logb" if log else "b"] = ctx.fetch(G.BUF_B, (F, N))
        out["gamma"] = ctx.fetch(G.BUF_GAMMA, (F, N))
        if log:
            out["la"], out["lbe"] = ctx.fetch(G.BUF_ALPHA, (F, N)), ctx.fetch(G.BUF_BETA, (F, N))
        out["ll"] = ctx.fetch(G.BUF_LOGLIK, (U,))
        if twice:
            ctx.estep_full_streams(d.fms, d.corpora, d.sts, log=log)
            for v, s in zip(vs, d.sts):
                assert bits_equal(v, s.download()), "a second call differs"
        return out
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
        d.close()


def check_stream_stats(dev, ref_stats, what):
    for p, (got, ref) in enumerate(zip(dev["stats"], ref_stats)):
        for key in STAT_KEYS:
            assert_close(got[key], f64(ref[key]), rtol=RTOL, what=f"{what}: stats[{p}].{key}")
    for p in range(1, len(dev["stats"])):       # the common sums are the same numbers in every vector
        for key in ("num_a", "den_a", "den_c", "loglik", "n_utt"):
            assert bits_equal(dev["stats"][p][key], dev["stats"][0][key]), (what, p, key)


# ------------------------------------------------------------- the E-step against the reference

@extended
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_linear_estep(G, ctx, name):
    hms, Xs, lens = S.make_case(G, name)
    ref = S.estep(hms, Xs, lens, 1, np.longdouble)
    assert np.isfinite(f64(ref["loglik"])[[0, 2]]).all()
    dev = run_streams(G, ctx, hms, Xs, lens, log=False, twice=True)
    one = dict(b=dev["b"], gamma=dev["gamma"], ll=dev["ll"], stats=dev["stats"][0],
               post=f64(ref["posts"][0]).reshape(len(Xs[0]), -1))      # (the stand-in of the docstring)
    check_estep(one, dict(b=ref["b"], post=ref["posts"][0], gamma=ref["gamma"], stats=ref["stats"][0],
                          loglik=ref["loglik"]), hms[0], lens, 1, name)
    check_stream_stats(dev, ref["stats"], name)
    if name.endswith("banded"):     # 5 frames under 35 states
        assert dev["ll"][1] == -np.inf and np.all(dev["gamma"][70:75] == 0.0)


@extended
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_log_estep(G, ctx, name):
    hms, Xs, lens = S.make_case(G, name)
    N = hms[0].N
    dev = run_streams(G, ctx, hms, Xs, lens, log=True, twice=True)
    full = S.estep_log(hms, Xs, lens, 1, np.longdouble)
    close_logb(dev["logb"], f64(full["logb"]), 1e-11)
    # the lattice on the device's own sum of logs, utterance by utterance
    ref = S.estep_log(hms, Xs, lens, 1, np.longdouble, logb=dev["logb"])
    off = offsets(lens)
    for u, ut in enumerate(ref["utt"]):
        s = slice(off[u], off[u + 1])
        got = {"la": dev["la"][s], "lbe": dev["lbe"][s], "logP": dev["ll"][u], "gamma": dev["gamma"][s]}
        check_log_lattice(f"{name}[{u}]", N, got, ut, what="GPU", xi=False)
    check_stream_stats(dev, ref["stats"], name)
    same_kind_close(dev["ll"], f64(full["loglik"]))


# ------------------------------------------------------------- the fold is exact

def special_case(G):
    """two streams, 35 states; stream 0 has a state of weight 0 (b = 0, log b = -inf), stream 1 a
    Gaussian of det == 0 (density x / 0, log b NaN)"""
    hms, Xs, lens = S.make_case(G, "p2-banded")
    hms[0].c[1] = 0.0
    hms[1].det[3, 1] = 0.0
    hms[1].det[34, 0] = 0.0
    return hms, Xs, lens


@pytest.mark.parametrize("name", ["p3-ergodic", "special"])
def test_fold_is_exact(G, ctx, name):
    """GHMM_BUF_B after a streams call = the numpy product (sum) in stream order of the b (log b) the
    single-stream calls leave, bit for bit: FC_LIN (score), FC_LOG (logscore), and on the clean case
    FC_POST and FC_LOGPOST (the E-steps)"""
    hms, Xs, lens = special_case(G) if name == "special" else S.make_case(G, name)
    N, F = hms[0].N, len(Xs[0])
    d = Streams(ctx, hms, Xs, lens)
    try:
        def singles(call):
            out = []
            for p in range(len(hms)):
                call(p)
                out.append(ctx.fetch(G.BUF_B, (F, N)))
            return out
        lin = singles(lambda p: ctx.emission_full(d.fms[p], d.corpora[p]))
        log = singles(lambda p: ctx.viterbi_full(d.fms[p], d.corpora[p]))
        if name == "special":
            assert np.all(lin[0][:, 1] == 0.0) and np.all(log[0][:, 1] == -np.inf)
            assert np.isnan(log[1][:, 3]).all() and not np.isfinite(lin[1][:, 34]).any()
        ctx.score_full_streams(d.fms, d.corpora)
        assert bits_equal(ctx.fetch(G.BUF_B, (F, N)), S.fold(lin))
        ctx.logscore_full_streams(d.fms, d.corpora)
        assert bits_equal(ctx.fetch(G.BUF_B, (F, N)), S.fold(log, log=True))
        if name != "special":
            post = singles(lambda p: ctx.estep_full(d.fms[p], d.corpora[p], d.sts[p]))
            ctx.estep_full_streams(d.fms, d.corpora, d.sts)
            assert bits_equal(ctx.fetch(G.BUF_B, (F, N)), S.fold(post))
            ctx.estep_full_streams(d.fms, d.corpora, d.sts, log=True)
            assert bits_equal(ctx.fetch(G.BUF_B, (F, N)), S.fold(log, log=True))
    finally:
        d.close()


# ------------------------------------------------------------- delegation and reproducibility

def test_one_stream_is_the_single_stream_call(G, ctx):
    hms, Xs, lens = S.make_case(G, "p2-ergodic")
    hm, X = hms[1], Xs[1]
    N, F, U = hm.N, len(X), len(lens)
    d = Streams(ctx, [hm], [X], lens)
    fm, corpus, st = d.fms[0], d.corpora[0], d.sts[0]
    try:
        for log, single in ((False, ctx.estep_full), (True, ctx.estep_full_log)):
            def arrays():
                return [st.download(), ctx.fetch(G.BUF_B, (F, N)), ctx.fetch(G.BUF_GAMMA, (F, N)),
                        ctx.fetch(G.BUF_POST, (F, N * hm.M)), ctx.fetch(G.BUF_LOGLIK, (U,))]
            single(fm, corpus, st)
            want = arrays()
            st.upload(np.zeros_like(want[0]))
            ctx.estep_full_streams([fm], [corpus], [st], log=log)
            for a, b in zip(arrays(), want):
                assert bits_equal(a, b), log
        assert bits_equal(ctx.score_full_streams([fm], [corpus]), ctx.score_full(fm, corpus))
        for fs in (False, True):
            assert bits_equal(ctx.logscore_full_streams([fm], [corpus], final_state=fs),
                              ctx.logscore_full(fm, corpus, final_state=fs))
    finally:
        d.close()


@pytest.mark.parametrize("log", [False, True])
def test_a_single_stream_call_in_between_changes_nothing(G, ctx, log):
    """the workspace is rebuilt by every call: an E-step of another model on another corpus between two
    streams calls leaves their results bit-equal"""
    hms, Xs, lens = S.make_case(G, "p3-banded")
    N, F = hms[0].N, len(Xs[0])
    rng = np.random.default_rng(5)
    other = rand_fmodel(G, rng, 7, 2, 4, spread=1.0, asym=False)
    d = Streams(ctx, hms, Xs, lens)
    o = Streams(ctx, [other], [walk_any(rng, other, [50, 20])], [50, 20])
    try:
        def once():
            ctx.estep_full_streams(d.fms, d.corpora, d.sts, log=log)
            return [s.download() for s in d.sts] + [ctx.fetch(G.BUF_B, (F, N)), ctx.fetch(G.BUF_GAMMA, (F, N))]
        first = once()
        ctx.estep_full(o.fms[0], o.corpora[0], o.sts[0])
        for a, b in zip(once(), first):
            assert bits_equal(a, b)
        # the diagonal row API refuses the product, as it refuses ghmm_emission_full's densities
        dm = ctx.model(G.synth_start_model(*G.synth_truth(N, 1, 3)))
        assert code(G, lambda: ctx.forward(dm, d.corpora[0])) != G.OK
        dm.close()
    finally:
        d.close(); o.close()


# ------------------------------------------------------------- the scores

@extended
@pytest.mark.parametrize("name", ["p2-banded", "p3-ergodic"])
def test_scores(G, ctx, name):
    hms, Xs, lens = S.make_case(G, name)
    d = Streams(ctx, hms, Xs, lens)
    try:
        lin = ctx.score_full_streams(d.fms, d.corpora)
        same_kind_close(lin, f64(S.score(hms, Xs, lens)))
        log0 = ctx.logscore_full_streams(d.fms, d.corpora)
        for fs, got in ((0, log0), (1, ctx.logscore_full_streams(d.fms, d.corpora, final_state=True))):
            same_kind_close(got, f64(S.logscore(hms, Xs, lens, fs)))
        fin = np.isfinite(lin) & np.isfinite(log0)
        assert fin.sum() >= 2
        same_kind_close(log0[fin], lin[fin])
    finally:
        d.close()


@extended
def test_product_underflow(G, ctx):
    """frame 5 lies far from every Gaussian of both streams: each stream's densities are positive there,
    their product is 0 on the whole frame; the linear score is the reference's -inf or NaN, the log
    score finite"""
    hms, Xs, lens = S.make_far_case(G)
    d = Streams(ctx, hms, Xs, lens)
    try:
        lin = ctx.score_full_streams(d.fms, d.corpora)
        b = ctx.fetch(G.BUF_B, (len(Xs[0]), hms[0].N))
        assert np.all(b[5] == 0.0)
        ref = f64(S.score(hms, Xs, lens, np.float64))      # (long double does not underflow there)
        assert not np.isfinite(ref[0]) and not np.isfinite(lin[0])
        same_kind_close(lin, ref)
        for fs in (0, 1):
            got = ctx.logscore_full_streams(d.fms, d.corpora, final_state=bool(fs))
            assert np.isfinite(got).all()
            same_kind_close(got, f64(S.logscore(hms, Xs, lens, fs)))
    finally:
        d.close()


# ------------------------------------------------------------- the M-step per stream

@extended
@pytest.mark.parametrize("dev_mstep", [False, True])
def test_two_em_iterations(G, ctx, dev_mstep):
    """the recorded 6-state run's corpus (13 bundled utterances, 9-d and 5-d) from ghmm_init_model_full
    per stream: two iterations against the long-double trajectory at test_fullestep_gpu's bars (trace
    rel 1e-9, model 1e-8); every stream's model ends with the same A"""
    run = P2["train"]["all13_6_p2"]
    Xs, lens = S.bundled_streams(G, GOLDEN, P2["mean_list"], run["utterances"])
    hms = [G.HostFullModel.init_from(X, lens, run["N"], M) for X, M in zip(Xs, run["M"])]
    ref_hms, trace = hms, []
    for _ in range(2):
        sts = S.estep(ref_hms, Xs, lens, 1, np.longdouble)["stats"]
        trace.append(float(sts[0]["loglik"]))
        ref_hms = [h.mstep(R.pack(s), delta=1) for h, s in zip(ref_hms, sts)]
    d = Streams(ctx, hms, Xs, lens)
    try:
        got = []
        for _ in range(2):
            ctx.estep_full_streams(d.fms, d.corpora, d.sts)
            got.append(d.sts[0].loglik()[0])
            for fm, st in zip(d.fms, d.sts):
                (ctx.mstep_full_dev if dev_mstep else ctx.mstep_full)(fm, st)
        out = [fm.get() for fm in d.fms]
    finally:
        d.close()
    assert max(abs(x - y) / abs(y) for x, y in zip(got, trace)) <= 1e-9
    for p, (hm, ref) in enumerate(zip(out, ref_hms)):
        assert np.array_equal(hm.A, out[0].A), p
        assert R.model_err(hm, lambda k: getattr(ref, k)) <= 1e-8, p


# ------------------------------------------------------------- refusals

def test_refusals(G, ctx):
    hms, Xs, lens = S.make_far_case(G)
    rng = np.random.default_rng(9)
    d = Streams(ctx, hms, Xs, lens)
    fms, corpora, sts = d.fms, d.corpora, d.sts
    other_n = ctx.full_model(rand_fmodel(G, rng, 5, 1, hms[1].D, spread=1.0, asym=False))
    other_len = ctx.corpus(Xs[1], [lens[0] + 1, lens[1] - 1])
    other_d = ctx.corpus(np.zeros((int(lens.sum()), 3)), lens)
    diag, shape = ctx.stats(hms[1].N, hms[1].M, hms[1].D), ctx.stats_full(hms[1].N, hms[1].M + 1, hms[1].D)
    try:
        ctx.estep_full_streams(fms, corpora, sts)
        before = [s.download() for s in sts] + [a.copy() for fm in fms for a in fm.get().arrays()]

        def estep(m=fms, c=corpora, s=sts, log=False):
            return lambda: ctx.estep_full_streams(m, c, s, log=log)
        for log in (False, True):
            assert code(G, estep([fms[0], other_n], log=log)) == G.ERR_ARG
            assert code(G, estep(c=[corpora[0], other_len], log=log)) == G.ERR_ARG
            assert code(G, estep(c=[corpora[0], other_d], log=log)) == G.ERR_ARG
            assert code(G, estep(s=[sts[0], diag], log=log)) == G.ERR_ARG
            assert code(G, estep(s=[sts[0], shape], log=log)) == G.ERR_ARG
        for call in (ctx.score_full_streams, ctx.logscore_full_streams):
            assert code(G, lambda: call([fms[0], other_n], corpora)) == G.ERR_ARG
            assert code(G, lambda: call(fms, [corpora[0], other_len])) == G.ERR_ARG
            assert code(G, lambda: call(fms, [corpora[0], other_d])) == G.ERR_ARG
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert code(G, estep()) == code(G, estep(log=True)) == G.ERR_UNSUPPORTED
            assert code(G, lambda: ctx.score_full_streams(fms, corpora)) == G.ERR_UNSUPPORTED
            assert code(G, lambda: ctx.logscore_full_streams(fms, corpora)) == G.ERR_UNSUPPORTED
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        # null arrays and a stream count outside 1 .. GHMM_MAX_STREAMS, through the C ABI itself
        lib, vp = ctx.lib, G.C.c_void_p
        nine = lambda objs: (vp * 9)(*[objs[p % 2].h for p in range(9)])  # noqa: E731
        pm, pc, ps = nine(fms), nine(corpora), nine(sts)
        out = np.zeros(len(lens))
        dp = out.ctypes.data_as(G.C.POINTER(G.C.c_double))
        for P in (0, 9, -1):
            assert lib.ghmm_estep_full_streams(ctx.h, pm, pc, P, ps, 0) == G.ERR_ARG
            assert lib.ghmm_score_full_streams(ctx.h, pm, pc, P, dp) == G.ERR_ARG
            assert lib.ghmm_logscore_full_streams(ctx.h, pm, pc, P, 0, dp) == G.ERR_ARG
        assert lib.ghmm_estep_full_streams(ctx.h, None, pc, 2, ps, 0) == G.ERR_ARG
        assert lib.ghmm_estep_full_streams(ctx.h, pm, None, 2, ps, 1) == G.ERR_ARG
        assert lib.ghmm_estep_full_streams(ctx.h, pm, pc, 2, None, 0) == G.ERR_ARG
        assert lib.ghmm_score_full_streams(ctx.h, None, pc, 2, dp) == G.ERR_ARG
        assert lib.ghmm_logscore_full_streams(ctx.h, pm, None, 2, 0, dp) == G.ERR_ARG
        assert lib.ghmm_score_full_streams(ctx.h, pm, pc, 2, None) == G.ERR_ARG
        after = [s.download() for s in sts] + [a for fm in fms for a in fm.get().arrays()]
        for a, b in zip(after, before):
            assert bits_equal(a, b), "a refused call changed a model or a statistics vector"
    finally:
        for o in (other_n, other_len, other_d, diag, shape):
            o.close()
        d.close()


# ------------------------------------------------------------- the command lines

SKIP = ("starting time", "ending time", "cpu time")


def stream_files(G, tmp):
    """the recorded runs' two streams as files in tmp, under the names the recording used"""
    for fn in P2["mean_list"]:
        X = G.perfil_read(os.path.join(GOLDEN, "perfil", fn))
        G.perfil_write(os.path.join(tmp, fn), X)
        G.perfil_write(os.path.join(tmp, "d_" + fn), second_stream(X))


def write_lists(tmp, tag, idx):
    names = []
    for s, prefix in ((1, ""), (2, "d_")):
        names.append(f"{tag}_{s}.txt")
        open(os.path.join(tmp, names[-1]), "w").write("\n".join(prefix + P2["mean_list"][i] for i in idx) + "\n")
    return names


def train_cli(tmp, name, run, env=None, streams_on=True):
    lists = write_lists(tmp, name, run["utterances"])
    e = dict(os.environ, **(env or {}))
    if streams_on:
        e["GHMM_FULL_STREAMS"] = "1"
    p = subprocess.run([TRAIN, name, str(run["N"]), "2"] + [str(m) for m in run["M"]] + lists + [name + ".hmm"],
                       cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    return p.returncode, p.stdout.decode(errors="replace")


def check_trained(G, models, tmp, name, run, text):
    """fullcov_support.check_run's checks on a two-stream run, and the report line for line"""
    rep = [l for l in open(os.path.join(tmp, name + ".txt")).read().split("\n") if l and not l.startswith(SKIP)]
    ref = run["report"]
    assert rep == ref, (name, rep, ref)     # iterations, the mean probability at 6 decimals, the per-stream lines
    assert report_value(rep, "number of parameters") == "2"
    verify = [float(v) for v in re.findall(r"Verifying Probability: (\S+) >", text)]
    assert len(verify) == len(run["verify"]), name
    np.testing.assert_allclose(verify, run["verify"], atol=1.5e-6, rtol=0)
    out = os.path.join(tmp, name + ".hmm")
    with open(out, "rb") as f:
        assert int.from_bytes(f.read(8), "little") == len(name), f"{name}: length prefix"
    hms = G.HostFullModel.read_streams(out)
    assert len(hms) == 2
    for s, hm in enumerate(hms):
        assert hm.word == name
        key_of = lambda k: f"{name}.A" if k == "A" else f"{name}.s{s}.{k}"  # noqa: E731
        for key in ("A", "c", "mean", "det"):
            np.testing.assert_allclose(getattr(hm, key), models[key_of(key)], rtol=1e-8, atol=0,
                                       err_msg=f"{name}.s{s}.{key}")
        ric = models[key_of("inv_cov")]
        for i in range(hm.N):
            for k in range(hm.M):
                err = np.abs(hm.inv_cov[i, k] - ric[i, k]).max() / np.abs(ric[i, k]).max()
                assert err <= 1e-8, (name, s, i, k, err)
    return hms


@pytest.fixture(scope="module")
def models():
    return np.load(os.path.join(GOLDEN, "fullstreams_models.npz"))


@pytest.fixture(scope="module")
def workdir(G, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fullstreams"))
    stream_files(G, tmp)
    return tmp


@pytest.mark.parametrize("name", sorted(P2["train"]))
def test_trainer_reproduces_the_recorded_runs(G, models, workdir, name):
    rc, text = train_cli(workdir, name, P2["train"][name])
    assert rc == 0, text[-2000:]
    check_trained(G, models, workdir, name, P2["train"][name], text)


@pytest.mark.parametrize("env,notice", [
    ({"GHMM_LOG_TRAIN": "1"}, ["E-step in the log domain (GHMM_LOG_TRAIN)"]),
    ({"GHMM_DEV_MSTEP": "1", "GHMM_DEV_INIT": "1"},
     ["M-step on the device (GHMM_DEV_MSTEP)", "Initial model on the device (GHMM_DEV_INIT)"])])
def test_trainer_variants_reach_the_same_values(G, models, workdir, env, notice):
    name = "all13_4_p2"
    rc, text = train_cli(workdir, name, P2["train"][name], env=env)
    assert rc == 0, text[-2000:]
    for line in notice:
        assert line in text
    check_trained(G, models, workdir, name, P2["train"][name], text)


def test_trainer_without_the_variable_still_refuses(workdir):
    rc, text = train_cli(workdir, "all13_5_p2", P2["train"]["all13_5_p2"], streams_on=False)
    assert rc == 1 and "one feature stream" in text and "GHMM_FULL_STREAMS" in text


def recognise(tmp, model_files, env=None):
    lists = write_lists(tmp, "rec", range(13))
    open(os.path.join(tmp, "models.txt"), "w").write("\n".join(model_files) + "\n")
    open(os.path.join(tmp, "words.txt"), "w").write("\n".join(P2["words"]) + "\n")
    p = subprocess.run([RECOGNISE, "1", "models.txt", "1"] + lists + ["words.txt", "report.txt"], cwd=tmp,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, **(env or {})))
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-2000:]
    return spoken_blocks(text), open(os.path.join(tmp, "report.txt")).read().split("\n")


def printed_scores(blocks, words):
    return np.array([[float(dict(b["ranking"])[w]) for b in blocks] for w in words])


def test_recogniser_reproduces_the_recorded_rankings(G, models, workdir):
    """the 13 recorded word models (written here from the recording with an 8-byte prefix) on the 13
    utterances: RC's ranking blocks line for line, and its report; with GHMM_LOG_SCORE=1 the same
    winners among the models whose recorded score is finite"""
    words, ref = P2["words"], P2["recog"]
    files = []
    for w in words:
        hms = [G.HostFullModel(models[f"{w}.A"], *(models[f"{w}.s{s}.{k}"] for k in ("c", "mean", "inv_cov", "det")),
                               word=w) for s in range(2)]
        files.append(w + ".hmm")
        G.HostFullModel.write_streams(os.path.join(workdir, files[-1]), hms)
    blocks, report = recognise(workdir, files)
    assert [b["spoken"] for b in blocks] == [b["spoken"] for b in ref["blocks"]]
    for got, want in zip(blocks, ref["blocks"]):
        assert [w for w, _ in got["ranking"]] == [w for w, _ in want["ranking"]], want["spoken"]
    check_blocks(printed_scores(blocks, words), words, ref["blocks"])
    keep = lambda ls: [l for l in ls if not l.startswith(("Date and time", "Model name"))  # noqa: E731
                       and "recognition time" not in l]
    assert keep(report) == ref["report"]
    # the log domain
    lblocks, lreport = recognise(workdir, files, env={"GHMM_LOG_SCORE": "1"})
    assert lreport[1] == "Algorithm used for recognition: Forward (log domain) "
    lsc, rsc = printed_scores(lblocks, words), printed_scores(ref["blocks"], words)
    assert np.isfinite(lsc).all()
    fin = np.isfinite(rsc)
    assert fin.any(0).all()
    same_kind_close(lsc[fin], rsc[fin])
    for u in range(13):
        k = np.nonzero(fin[:, u])[0]
        assert k[np.argmax(lsc[k, u])] == k[np.argmax(rsc[k, u])], words[u]


def test_recogniser_loads_what_the_trainer_wrote(G, models, workdir):
    name = "all13_5_p2"
    rc, text = train_cli(workdir, name, P2["train"][name])
    assert rc == 0, text[-2000:]
    blocks, _ = recognise(workdir, [name + ".hmm"])
    assert len(blocks) == 13 and all(len(b["ranking"]) == 1 and b["ranking"][0][0] == name for b in blocks)
    hms = G.HostFullModel.read_streams(os.path.join(workdir, name + ".hmm"))
    Xs, lens = S.bundled_streams(G, GOLDEN, P2["mean_list"], range(13))
    want = f64(S.score(hms, Xs, lens, np.float64))
    same_kind_close(printed_scores(blocks, [name])[0], want)
