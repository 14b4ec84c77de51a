"""ghmm_fmodel_init — the full-covariance trainer's initial model built on the MI355X — against the host
init (ghmm_init_model_full, pinned bit for bit to TFF) and its long-double restatement
(fullinit_ref.init_full).  GPU box only.  The corpora, what each is there for, and the admission
condition they meet on the CPU (test_fullinit_host) are in fullinit_ref's docstring.

1. Discrete parts: A and c are the host's bits, the last classification's one-hot rows (fetched from the
   workspace) give the host's states, cells and counts exactly, every array has the host's NaN / inf / zero
   pattern.  On the U = 1 corpora the means are the host's bits as well (one block per state adds the
   frames in the host's order).
2. Accuracy: mean, the matrix slot and det by rel_dist from the long-double restatement.  No tolerance is
   fixed: with e_host the host init's own distance, the device must stay within 16 e_host + 64 eps
   (eps = 2^-52); both routes add the same terms in different orders, and at these sizes e_host can be one
   ulp by luck.  The measured ratios are recorded in profiles/fullinit_time.txt.
3. Repeatability: a second call and a fresh context give the same bits.
4. Call order: init and two EM iterations with no host synchronisation in between, alone and after an
   unrelated E-step of another shape in the same context, give the same statistics bits; log P is finite
   and within item 2's tolerance of the run started from the host's model.
5. A one-rank communicator gives the bits of comm = None.
6. Refusals.  7. The command line under GHMM_DEV_INIT=1."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fullinit_ref as R
from conftest import GOLDEN
from fullcov_support import ctx, recorded  # noqa: F401  (the fixtures)
from fullcov_support import (FULL, RECOGNISE, RUNS, SHIPPED, TRAIN, check_run, code, need_extended, rel_dist, run_cli,
                             same_kind_mask, spoken_blocks)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
KEYS = ("A", "c", "mean", "inv_cov", "det")


def blank(G, N, M, D):
    return G.HostFullModel(np.eye(N), np.full((N, M), 1.0 / M), np.zeros((N, M, D)),
                           np.tile(np.eye(D), (N, M, 1, 1)), np.ones((N, M)))


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def device_init(G, ctx, X, lens, N, M, comm=None, rows=False):
    """the model ghmm_fmodel_init builds (and, rows: the workspace's one-hot gamma and post)"""
    fm, corpus = ctx.full_model(blank(G, N, M, X.shape[1])), ctx.corpus(X, lens)
    try:
        got = fm.init_from(corpus, comm)
        if not rows:
            return got
        F = len(X)
        return got, ctx.fetch(G.BUF_GAMMA, (F, N)), ctx.fetch(G.BUF_POST, (F, N * M))
    finally:
        fm.close(); corpus.close()


_cache = {}


def result(G, ctx, name):
    """computed once per case, shared, not modified"""
    if name not in _cache:
        X, lens, N, M = R.corpus(name)
        _cache[name] = device_init(G, ctx, X, lens, N, M, rows=True)
    return _cache[name]


@functools.lru_cache(maxsize=None)
def host_init(G, name):
    X, lens, N, M = R.corpus(name)
    return G.HostFullModel.init_from(X, lens, N, M)


@pytest.mark.parametrize("name", R.CASES)
def test_discrete_parts(G, ctx, name):
    X, lens, N, M = R.corpus(name)
    host, ref = host_init(G, name), R.reference(name, False)
    got, gamma, post = result(G, ctx, name)
    assert bits_equal(got.A, host.A), name
    # the last classification: one row per frame, a single 1 in it, at the host's state and cell
    assert np.all((gamma == 0) | (gamma == 1)) and np.all((post == 0) | (post == 1)), name
    assert np.all(gamma.sum(1) == 1) and np.all(post.sum(1) == 1), name
    assert np.array_equal(gamma.argmax(1), ref["state"]), name
    assert np.array_equal(post.argmax(1), ref["state"] * M + ref["assign"][-1]), name
    assert np.array_equal(post.sum(0).reshape(N, M), ref["count"]), name
    assert bits_equal(got.c, host.c), name
    for key in KEYS:
        a, b = getattr(got, key), getattr(host, key)
        fin = same_kind_mask(a, b, f"{name}.{key}")
        assert np.array_equal(a[fin] == 0, b[fin] == 0), f"{name}.{key}: zeros differ"
    if name in R.BIT_EQUAL_CELLS:
        assert bits_equal(got.mean, host.mean), name


def distances(model, ref):
    return {key: rel_dist(getattr(model, key), ref[key])
            for key in ("mean", "inv_cov", "det")}


@pytest.mark.parametrize("name", R.CASES)
def test_accuracy_against_long_double(G, ctx, name):
    """every case, fewdistinct included: it is not admitted by the gap condition, but its long-double run
    makes the float64 run's assignments (asserted here), so the reference is one for it as well"""
    need_extended()
    for a, b in zip(R.reference(name, False)["assign"], R.reference(name, True)["assign"]):
        assert np.array_equal(a, b), name
    ref = R.reference(name, True)
    e_host, e_dev = distances(host_init(G, name), ref), distances(result(G, ctx, name)[0], ref)
    for key in e_host:
        ratio = e_dev[key] / e_host[key] if e_host[key] else float("inf") if e_dev[key] else 0.0
        print(f"fullinit accuracy {name:8s} {key:8s} e_host {e_host[key]:.3e} e_dev {e_dev[key]:.3e} "
              f"ratio {ratio:.3g}")
    for key in e_host:
        assert e_dev[key] <= 16 * e_host[key] + 64 * EPS, (name, key, e_dev[key], e_host[key])


@pytest.mark.parametrize("name", ["m5", "ragged", "short"])
def test_repeatable(G, ctx, name):
    X, lens, N, M = R.corpus(name)
    first = result(G, ctx, name)[0]
    again = device_init(G, ctx, X, lens, N, M)
    fresh_ctx = G.Context(0)
    try:
        fresh = device_init(G, fresh_ctx, X, lens, N, M)
    finally:
        fresh_ctx.close()
    for key in KEYS:
        assert bits_equal(getattr(first, key), getattr(again, key)), (name, key, "second call")
        assert bits_equal(getattr(first, key), getattr(fresh, key)), (name, key, "fresh context")


def test_cap_shape_runs(G, ctx):
    """M = 64 and D = 48, the pass kernel's largest LDS footprint (76 KB, above the default limit): too few
    frames per cell for the admission condition, so only what holds regardless is asserted — the call
    succeeds, repeats its bits, A is the formula's and every state's weights sum to 1"""
    N, M, D, lens = 2, 64, 48, [700, 650]
    X = R.clouds(21, N, 8, D, lens)
    a, b = device_init(G, ctx, X, lens, N, M), device_init(G, ctx, X, lens, N, M)
    for key in KEYS:
        assert bits_equal(getattr(a, key), getattr(b, key)), key
    assert np.array_equal(a.A, [[0.5, 0.5], [0.0, 1.0]])
    assert np.all(np.abs(a.c.sum(1) - 1.0) < 1e-12) and np.all(a.c > 0)


def em_twice(G, ctx, fm, corpus, st):
    for _ in range(2):
        ctx.estep_full(fm, corpus, st)
        ctx.mstep_full_dev(fm, st)
    return st.download()            # the second E-step's statistics (the M-step leaves them as they are)


def test_call_order(G, ctx):
    need_extended()
    name = "m3"
    X, lens, N, M = R.corpus(name)
    D = X.shape[1]
    fm, corpus, st = ctx.full_model(blank(G, N, M, D)), ctx.corpus(X, lens), ctx.stats_full(N, M, D)
    rng = np.random.default_rng(3)
    other_lens = [45, 71]
    other_hm = blank(G, 7, 2, 9)
    other_hm.mean[:] = rng.normal(0.0, 1.0, other_hm.mean.shape)
    other_X = rng.normal(0.0, 1.0, (sum(other_lens), 9))
    other, other_c, other_st = ctx.full_model(other_hm), ctx.corpus(other_X, other_lens), ctx.stats_full(7, 2, 9)
    try:
        fm.init_from(corpus, fetch=False)            # nothing waits between the calls
        v1 = em_twice(G, ctx, fm, corpus, st)
        ctx.estep_full(other, other_c, other_st)     # another shape's E-step leaves its state in the context
        fm.init_from(corpus, fetch=False)
        v2 = em_twice(G, ctx, fm, corpus, st)
        assert np.array_equal(v1.view(np.uint64), v2.view(np.uint64))
        fm.set(host_init(G, name))
        vh = em_twice(G, ctx, fm, corpus, st)
    finally:
        for o in (fm, corpus, st, other, other_c, other_st):
            o.close()
    lp, lp_host = v1[-2], vh[-2]
    e_host = max(distances(host_init(G, name), R.reference(name, True)).values())
    print(f"fullinit call order: log P {lp!r} from the device's model, {lp_host!r} from the host's, "
          f"rel {abs(lp - lp_host) / abs(lp_host):.3e}, bound {16 * e_host + 64 * EPS:.3e}")
    assert np.isfinite(lp) and np.isfinite(lp_host)
    assert abs(lp - lp_host) <= (16 * e_host + 64 * EPS) * abs(lp_host)


def test_one_rank_communicator(G, ctx):
    """over a real RCCL communicator of one rank (all a one-GPU box can hold) every all-reduce is the
    identity: the bits of comm = None"""
    name = "m5"
    X, lens, N, M = R.corpus(name)
    plain = result(G, ctx, name)[0]
    comm = ctx.comm(0, 1)
    try:
        got = device_init(G, ctx, X, lens, N, M, comm=comm)
    finally:
        comm.close()
    for key in KEYS:
        assert bits_equal(getattr(plain, key), getattr(got, key)), key


def test_refusals(G, ctx):
    X, lens, N, M = R.corpus("m2")
    D = X.shape[1]
    corpus = ctx.corpus(X, lens)
    wide, fm = ctx.full_model(blank(G, N, 65, D)), ctx.full_model(blank(G, N, M, D))
    other_d = ctx.corpus(np.ones((20, D + 1)), [20])
    empty = ctx.corpus(np.zeros((0, D)), np.zeros(0, dtype=np.int32))
    try:
        before = wide.get()
        assert code(G, lambda: wide.init_from(corpus)) == G.ERR_UNSUPPORTED
        after = wide.get()
        for a, b in zip(before.arrays(), after.arrays()):
            assert np.array_equal(a, b)
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert code(G, lambda: fm.init_from(corpus)) == G.ERR_UNSUPPORTED
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert code(G, lambda: fm.init_from(empty)) == G.ERR_ARG
        assert code(G, lambda: fm.init_from(other_d)) == G.ERR_ARG
        fm.init_from(corpus)       # and the context still works
    finally:
        for o in (corpus, wide, fm, other_d, empty):
            o.close()


# ------------------------------------------------------------- the command line

DEV = dict(os.environ, GHMM_DEV_INIT="1")
NOTICE = "Initial model on the device (GHMM_DEV_INIT)"


def test_shipped_runs_and_recognition_dev_init(G, recorded, tmp_path):
    """TFF's 13 runs under GHMM_DEV_INIT=1 (M = 1: only the order of the sums differs): the recorded
    iteration counts and mean probabilities (check_run), then the recogniser ranks the 13 written models
    as the shipped hmm-result.txt does"""
    assert len(SHIPPED) == 13
    models = []
    for name in SHIPPED:
        run = RUNS[name]
        d = tmp_path / name
        d.mkdir()
        paths = [os.path.join(GOLDEN, "perfil", f) for f in run["perfils"]]
        _, text, out, txt = run_cli(str(d), name, 6, 1, paths, env=DEV)
        assert NOTICE in text, name
        check_run(G, recorded, name, run, out, txt)
        models.append((name, out))
    sh = FULL["shipped"]
    by_name = {f"mean_{n}.hmm": p for n, p in models}
    by_name.update({os.path.basename(p): p for _, p in models})
    tmp = str(tmp_path)
    ml, fl, wl = (os.path.join(tmp, f) for f in ("models.txt", "mean_list.txt", "words.txt"))
    open(ml, "w").write("\n".join(by_name[m] for m in sh["models"]) + "\n")
    open(fl, "w").write("\n".join(os.path.join(GOLDEN, "perfil", f) for f in sh["mean_list"]) + "\n")
    open(wl, "w").write("\n".join(sh["words"]) + "\n")
    p = subprocess.run([RECOGNISE, "1", ml, "1", fl, wl, os.path.join(tmp, "result.txt")],
                       stdout=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    blocks = spoken_blocks(p.stdout.decode())
    assert len(blocks) == len(sh["blocks"]) == 13
    for g, r in zip(blocks, sh["blocks"]):
        assert g["spoken"] == r["spoken"]
        assert [w for w, _ in g["ranking"]] == [w for w, _ in r["ranking"]], r["spoken"]


def write_perfils(G, tmp, X, lens):
    paths, o = [], 0
    for u, T in enumerate(lens):
        paths.append(os.path.join(tmp, f"u{u}.perfil"))
        G.perfil_write(paths[-1], X[o:o + T])
        o += T
    return paths


def test_command_line_combined_variables(G, tmp_path):
    """M = 4 on the m4 corpus with GHMM_DEV_INIT, GHMM_LOG_TRAIN and GHMM_DEV_MSTEP together: the three
    notices, and the report of the same run on the host's initial model"""
    X, lens, N, M = R.corpus("m4")
    paths = write_perfils(G, str(tmp_path), X, lens)
    reports = []
    for tag, extra in (("host", {}), ("dev", {"GHMM_DEV_INIT": "1"})):
        d = tmp_path / tag
        d.mkdir()
        env = dict(os.environ, GHMM_LOG_TRAIN="1", GHMM_DEV_MSTEP="1", **extra)
        _, text, out, txt = run_cli(str(d), "w", N, M, paths, env=env)
        assert "E-step in the log domain (GHMM_LOG_TRAIN)" in text and "M-step on the device (GHMM_DEV_MSTEP)" in text
        assert (NOTICE in text) == (tag == "dev")
        rep = {l.split(":", 1)[0]: l.split(":", 1)[1].strip() for l in open(txt).read().split("\n") if ":" in l}
        hm = G.HostFullModel.read(out)
        assert np.all(np.isfinite(hm.det)) and np.all(np.isfinite(hm.mean))
        reports.append(rep)
    assert reports[0]["number of iterations"] == reports[1]["number of iterations"]
    assert float(reports[1]["mean probability"]) == pytest.approx(float(reports[0]["mean probability"]),
                                                                  rel=1e-9, abs=2e-6)


def test_command_line_falls_back_above_the_cap(G, tmp_path):
    """M = 65: the fallback line, and the host route's model file byte for byte"""
    X, lens, N, _ = R.corpus("long")
    paths = write_perfils(G, str(tmp_path), X, lens)
    outs = []
    for tag, env in (("host", None), ("dev", DEV)):
        d = tmp_path / tag
        d.mkdir()
        _, text, out, _ = run_cli(str(d), "w", N, 65, paths, env=env)
        assert ("Initial model on the host: " in text) == (tag == "dev")
        assert NOTICE not in text
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1]
