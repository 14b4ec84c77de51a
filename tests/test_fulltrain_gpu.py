"""The full-covariance trainer (TFF = train/source/hmm-full-fs/hmm_continuous_full_fs.c) on the
MI355X — GPU box only.

Checked against recorded runs of the real reference (tests/golden/fulltrain_runs.json,
fulltrain_models.npz, fulltrain_synth.npz: make_golden_fulltrain.py), against the shipped models,
and against the float64 numpy restatement of TFF's E-step (fulltrain_ref.np_estep).  Tolerances:
reports' mean probability within rel 1e-9 / abs 2e-6 and the same iteration count; models within rel 1e-8 of the recorded
64-bit run (inv_cov per Gaussian as max|d| / max|inv_cov|) and within 1e-6 of the shipped 32-bit
files; E-step arrays and statistics rtol 1e-11, with an absolute floor of 1e-11 times the largest entry
of their block (sums of both signs cancel; gamma and the sums may hold a value far below that
where the restatement has an exact 0)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from fullcov_support import ctx, recorded  # noqa: F401  (the fixtures)
from fullcov_support import (FULL, RECOGNISE, RUNS, SHIPPED, SYNTH, TRAIN, check_run, close, code, rand_fmodel, run_cli,
                             spoken_blocks, walk_any)
from fulltrain_ref import np_estep

pytestmark = pytest.mark.gpu


def test_shipped_runs_and_recognition(G, recorded, tmp_path):
    """TFF's 13 runs (<word> 6 1 1 list out.hmm), then the recogniser on the 13 models written:
    the shipped hmm-result.txt's ranking, every score within rel 1e-6 of the shipped models' run"""
    assert len(SHIPPED) == 13
    models = []
    for name in SHIPPED:
        run = RUNS[name]
        d = tmp_path / name
        d.mkdir()
        paths = [os.path.join(GOLDEN, "perfil", f) for f in run["perfils"]]
        _, _, out, txt = run_cli(str(d), name, 6, 1, paths)
        shipped = os.path.join(GOLDEN, "full_cov_models", f"mean_{name}.hmm")
        check_run(G, recorded, name, run, out, txt,
                  shipped_hmm=shipped if os.path.exists(shipped) else None)
        models.append((name, out))
    # the vocabulary in the recogniser's own order (test/test/models/models.txt)
    sh = FULL["shipped"]
    by_name = {f"mean_{n}.hmm": p for n, p in models}
    by_name.update({os.path.basename(p): p for _, p in models})
    tmp = str(tmp_path)
    ml = os.path.join(tmp, "models.txt")
    fl = os.path.join(tmp, "mean_list.txt")
    wl = os.path.join(tmp, "words.txt")
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
        for (_, gv), (w, rv) in zip(g["ranking"], r["ranking"]):
            if "nan" in rv:
                assert "nan" in gv, (r["spoken"], w)
            else:
                assert float(gv) == pytest.approx(float(rv), rel=1e-6), (r["spoken"], w)


@pytest.mark.parametrize("name", SYNTH)
def test_synthetic_runs(G, recorded, tmp_path, name):
    run = RUNS[name]
    data = np.load(os.path.join(GOLDEN, "fulltrain_synth.npz"))
    X, lens = data[name + ".X"].astype(np.float64), data[name + ".lens"]
    paths, o = [], 0
    for u, T in enumerate(lens):
        paths.append(str(tmp_path / f"{name}_{u}.perfil"))
        G.perfil_write(paths[-1], X[o:o + T])
        o += T
    _, _, out, txt = run_cli(str(tmp_path), name, run["N"], run["M"], paths)
    check_run(G, recorded, name, run, out, txt)


@pytest.mark.parametrize("D", [1, 9, 16, 39])
def test_estep_matches_restatement(G, ctx, D):
    rng = np.random.default_rng(D)
    N, M = 5, 3
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    lens = [57, 80, 41]
    X = walk_any(rng, hm, lens)
    # one Gaussian with a non-positive-definite matrix: aux < -1420 on frames far from it, its
    # density overflows to +inf and is clamped to 1e20 (state 4's frames, so b stays finite there)
    hm.inv_cov[4, 2] = -np.eye(D)
    hm.mean[4, 2] = hm.mean[4, 0] + 60.0
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.estep_full(fm, corpus, st)
        v = st.download()
        F = len(X)
        b = ctx.fetch(G.BUF_B, (F, N))
        post = ctx.fetch(G.BUF_POST, (F, N * M))
        gamma = ctx.fetch(G.BUF_GAMMA, (F, N))
        rb, rpost, rgamma, rst = np_estep(hm, X, lens)
        assert np.any(rpost.reshape(F, N, M)[:, 4, 2] > 0.0)  # the clamp is exercised
        close(b, rb)
        close(post, rpost)
        close(gamma, rgamma, zeros=False)
        got = G.split_stats_full(v, N, M, D)
        for key in ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_cov"):
            close(got[key], rst[key], zeros=False)
        assert float(got["loglik"]) == pytest.approx(rst["loglik"], rel=1e-11)
        assert float(got["n_utt"]) == 3.0
        assert st.loglik() == (float(got["loglik"]), 3.0)
    finally:
        st.close(); fm.close(); corpus.close()


def test_estep_clamp_and_zero_b(G, ctx):
    """+inf densities become 1e20; a state whose every density underflows has b = 0 and post = 0"""
    rng = np.random.default_rng(5)
    N, M, D = 3, 2, 4
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    hm.inv_cov[1, 0] = -np.eye(D)          # density exp(+|x - mu|^2 / 2): +inf far away
    hm.mean[2] += 1000.0                   # state 2: every density underflows to exactly 0
    X = walk_any(rng, hm, [30])
    X[:, :] = hm.mean[0, 0] + rng.normal(0.0, 0.3, X.shape)
    X[5] = hm.mean[1, 0] + 50.0
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, [30])
    st = ctx.stats_full(N, M, D)
    try:
        ctx.emission_full(fm, corpus)  # the recogniser's densities: no clamp
        b_rec = ctx.fetch(G.BUF_B, (30, N))
        assert np.isinf(b_rec[5, 1])
        ctx.estep_full(fm, corpus, st)
        b = ctx.fetch(G.BUF_B, (30, N))
        post = ctx.fetch(G.BUF_POST, (30, N * M)).reshape(30, N, M)
        assert np.isfinite(b[5, 1]) and b[5, 1] >= 1e20 * hm.c[1, 0]
        assert np.all(b[:, 2] == 0.0) and np.all(post[:, 2] == 0.0)
        rb, rpost, _, _ = np_estep(hm, X, [30])
        close(b, rb)
        close(post.reshape(30, N * M), rpost)
    finally:
        st.close(); fm.close(); corpus.close()


def test_estep_bitwise_reproducible(G, ctx):
    rng = np.random.default_rng(9)
    hm = rand_fmodel(G, rng, 8, 3, 16, spread=1.0, asym=False)
    lens = list(rng.integers(100, 400, 12))
    X = walk_any(rng, hm, lens)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(8, 3, 16)
    try:
        ctx.estep_full(fm, corpus, st)
        v1 = st.download()
        ctx.estep_full(fm, corpus, st)
        v2 = st.download()
        assert np.array_equal(v1.view(np.uint64), v2.view(np.uint64))
    finally:
        st.close(); fm.close(); corpus.close()


def test_mstep_equals_host_mstep(G, ctx):
    rng = np.random.default_rng(13)
    N, M, D = 6, 2, 9
    hm = rand_fmodel(G, rng, N, M, D, spread=1.0, asym=False)
    lens = [120, 90, 150]
    X = walk_any(rng, hm, lens)
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.estep_full(fm, corpus, st)
        v = st.download()
        ref = hm.mstep(v, delta=1)
        ctx.mstep_full(fm, st)
        got = fm.get()
        for a, b in zip(got.arrays(), ref.arrays()):
            np.testing.assert_array_equal(a, b)
    finally:
        st.close(); fm.close(); corpus.close()


def test_refusals(G, ctx, tmp_path):
    rng = np.random.default_rng(21)
    hm = rand_fmodel(G, rng, 3, 2, 4, spread=1.0, asym=False)
    X = walk_any(rng, hm, [40])
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, [40])
    st = ctx.stats_full(3, 2, 4)
    other = ctx.stats_full(3, 3, 4)
    diag = ctx.stats(3, 2, 4)
    try:
        # D > 48
        assert code(G, lambda: ctx.full_model(G.HostFullModel(np.eye(2), np.ones((2, 1)), np.zeros((2, 1, 49)),
                                                           np.tile(np.eye(49), (2, 1, 1, 1)), np.ones((2, 1))))) \
            == G.ERR_UNSUPPORTED
        # GHMM_OPT_ROBUST
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert code(G, lambda: ctx.estep_full(fm, corpus, st)) == G.ERR_UNSUPPORTED
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        # shape mismatch, and a diagonal statistics vector
        assert code(G, lambda: ctx.estep_full(fm, corpus, other)) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_full(fm, corpus, diag)) == G.ERR_ARG
        assert code(G, lambda: ctx.mstep_full(fm, other)) == G.ERR_ARG
        # a full vector is refused by the diagonal path
        dm = ctx.model(G.synth_start_model(*G.synth_truth(3, 2, 4)))
        assert code(G, lambda: ctx.estep(dm, corpus, st)) == G.ERR_ARG
        dm.close()
    finally:
        for o in (st, other, diag, fm, corpus):
            o.close()
    # the command line: P > 1, several ranks, a diagonal .hmm as [initial_model], usage
    perfil = os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil")
    tmp = str(tmp_path)
    lst = os.path.join(tmp, "l.txt")
    open(lst, "w").write(perfil + "\n")
    p = subprocess.run([TRAIN, "w", "6", "2", "1", "1", lst, lst, os.path.join(tmp, "o.hmm")], cwd=tmp,
                       stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"one feature stream" in p.stdout
    env = dict(os.environ, GHMM_WORLD="2", GHMM_RANK="0", GHMM_COMM_ID=os.path.join(tmp, "id"))
    p = subprocess.run([TRAIN, "w", "6", "1", "1", lst, os.path.join(tmp, "o.hmm")], cwd=tmp,
                       stdout=subprocess.PIPE, timeout=60, env=env)
    assert p.returncode == 1 and b"one GPU" in p.stdout
    diag_hmm = os.path.join(tmp, "diag.hmm")
    X = G.perfil_read(perfil)
    G.HostModel.init_from(X, [len(X)], 6, 1).write(diag_hmm)
    p = subprocess.run([TRAIN, "w", "6", "1", "1", lst, os.path.join(tmp, "o.hmm"), diag_hmm], cwd=tmp,
                       stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"initial model" in p.stdout
    p = subprocess.run([TRAIN, "w", "6"], stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout.startswith(b"Usage: hmm_continuous_full_fs")


def test_initial_model_argument(G, recorded, tmp_path):
    """[initial_model] (the reference reads argv[argc] there): the recorded 64-bit model of a
    shipped run as start, read with ghmm_hmm_read_full, trains on and writes a model"""
    name = SHIPPED[0]
    start = str(tmp_path / "start.hmm")
    hm = G.HostFullModel(*(recorded[f"{name}.{k}"] for k in ("A", "c", "mean", "inv_cov", "det")), word=name)
    hm.write(start)
    paths = [os.path.join(GOLDEN, "perfil", f) for f in RUNS[name]["perfils"]]
    _, _, out, txt = run_cli(str(tmp_path), name, 6, 1, paths, extra=(start,))
    rep = open(txt).read()
    assert "number of iterations" in rep
    got = G.HostFullModel.read(out)
    assert got.N == 6 and got.M == 1 and np.all(np.isfinite(got.det))
