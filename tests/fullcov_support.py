"""What more than one full-covariance test file uses and that is no numerical restatement: fixtures,
the recorded runs' tables, the command-line helpers, the comparators with their tolerances, the random
models and corpora, and the device runner.  No tests; pytest does not collect this file.

The restatements live in the reference modules of their topic (fulltrain_ref, fullscore_ref,
fulllogscore_ref, fullestep_log_ref, fullviterbi_ref, fullmstep_cases), which import this module for
their cases' builders; the three comparators here that need a reference's bound import it when called.
No module under tests/ imports a test_*.py module."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from _load import PKG_DIR
from conftest import GOLDEN

FULL = json.load(open(os.path.join(GOLDEN, "fullcov_recog.json")))
RUNS = json.load(open(os.path.join(GOLDEN, "fulltrain_runs.json")))
SHIPPED = sorted(k for k, v in RUNS.items() if v["kind"] == "shipped")
SYNTH = sorted(k for k, v in RUNS.items() if v["kind"] == "synthetic")
TRAIN = os.path.join(PKG_DIR, "bin", "hmm-continuous-train-full-fs")
RECOGNISE = os.path.join(PKG_DIR, "bin", "recognition-continuous-test-full-fs")

RTOL = 1e-8          # asserted by test_gpu_parity on every intermediate
U53 = 2.0 ** -53


def have_extended():
    """long double carries more than double here (x87: eps = 2^-63)"""
    return np.finfo(np.longdouble).eps < 2.0 ** -60


def need_extended():
    assert have_extended(), ("long double is no wider than double on this platform: "
                             f"eps = {np.finfo(np.longdouble).eps}")


extended = pytest.mark.skipif(not have_extended(), reason="long double is no wider than double here")


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "fulltrain_models.npz"))


def code(G, fn):
    with pytest.raises(G.GhmmError) as e:
        fn()
    return e.value.code


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------- the recorded sets

def shipped(G):
    sh = FULL["shipped"]
    hms = [G.HostFullModel.read(os.path.join(GOLDEN, "full_cov_models", f)) for f in sh["models"]]
    Xs = [G.perfil_read(os.path.join(GOLDEN, "perfil", f)) for f in sh["mean_list"]]
    return sh, hms, Xs


def load_synth(G):
    d = np.load(os.path.join(GOLDEN, "fullcov_synth13.npz"))
    sy = FULL["synthetic"]
    D = 16
    iu = np.triu_indices(D)
    hms, Xs = [], []
    for w in sy["words"]:
        t = d[w + ".inv_cov_triu"].astype(np.float64)
        ic = np.zeros(t.shape[:2] + (D, D))
        ic[..., iu[0], iu[1]] = t
        ic[..., iu[1], iu[0]] = t
        hms.append(G.HostFullModel(d[w + ".A"], d[w + ".c"].astype(np.float64),
                                   d[w + ".mean"].astype(np.float64), ic, d[w + ".det"], word=w))
        Xs.append(d[w + ".X"].astype(np.float64))
    return sy, hms, Xs


def spoken_blocks(text):
    """the recogniser's stdout: per "Spoken word:" line a dict of the word and its ranking, the
    "<word> :  <score> " rows below it as [word, printed score]"""
    blocks = []
    for line in text.replace("\r", "").split("\n"):
        m = re.match(r"Spoken word: (\S+)", line)
        if m:
            blocks.append({"spoken": m.group(1), "ranking": []})
            continue
        m = re.match(r"(\S+) :  (\S+) $", line)
        if m and blocks:
            blocks[-1]["ranking"].append([m.group(1), m.group(2)])
    return blocks


def bubble(p):
    """sorting_probab, RC:968-995 (NaN-blind)"""
    idx = list(range(len(p)))
    done = False
    while not done:
        done = True
        for i in range(len(p) - 1):
            if p[idx[i]] < p[idx[i + 1]]:
                idx[i], idx[i + 1] = idx[i + 1], idx[i]
                done = False
    return idx


def fmt(x):
    if np.isnan(x):
        return "nan"
    return f"{x:f}"


def check_blocks(scores, words, blocks):
    """scores[k, u]; blocks = the reference's printed rankings"""
    for u, blk in enumerate(blocks):
        order = bubble(scores[:, u])
        assert [words[i] for i in order] == [w for w, _ in blk["ranking"]], blk["spoken"]
        for i, (w, txt) in zip(order, blk["ranking"]):
            if "nan" in txt or "inf" in txt:
                assert fmt(scores[i, u]).lstrip("-") == txt.lstrip("-"), (blk["spoken"], w)
            else:
                assert scores[i, u] == pytest.approx(float(txt), rel=1e-9, abs=2e-6), (blk["spoken"], w)


# --------------------------------------------------------------- the trainer's command line

def run_cli(tmp, word, N, M, perfil_paths, extra=(), env=None, check=True):
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(perfil_paths) + "\n")
    out = os.path.join(tmp, "out.hmm")
    p = subprocess.run([TRAIN, word, str(N), "1", str(M), lst, out, *extra], cwd=tmp, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600, env=env)
    text = p.stdout.decode(errors="replace")
    if check:
        assert p.returncode == 0, text[-2000:]
    return p.returncode, text, out, os.path.join(tmp, "out.txt")


def report_value(lines, key):
    return next(l for l in lines if l.startswith(key)).split(":", 1)[1].strip()


def check_run(G, recorded, name, run, out, txt, shipped_hmm=None):
    rep = [l for l in open(txt).read().split("\n") if l]
    ref = run["report"]
    assert rep[0] == ref[0] == ("Continuous HMM created using Forward Backward algorithm. It is considered "
                                "full covariance matrix. It is considered a final state."), (name, rep[0], ref[0])
    assert report_value(rep, "number of iterations") == report_value(ref, "number of iterations"), name
    assert report_value(rep, "number of exemplars") == report_value(ref, "number of exemplars"), name
    assert float(report_value(rep, "mean probability")) == pytest.approx(
        float(report_value(ref, "mean probability")), rel=1e-9, abs=2e-6), name
    with open(out, "rb") as f:
        assert int.from_bytes(f.read(8), "little") == len(name), f"{name}: length prefix"  # 8 bytes
    hm = G.HostFullModel.read(out)
    assert hm.word == name, (hm.word, name)

    def compare(ref_of, tol):
        for key in ("A", "c", "mean", "det"):
            np.testing.assert_allclose(getattr(hm, key), ref_of(key), rtol=tol, atol=0, err_msg=f"{name}.{key}")
        ic, ric = hm.inv_cov, ref_of("inv_cov")
        for i in range(hm.N):
            for k in range(hm.M):
                err = np.abs(ic[i, k] - ric[i, k]).max() / np.abs(ric[i, k]).max()
                assert err <= tol, (name, i, k, err)
    compare(lambda k: recorded[f"{name}.{k}"], 1e-8)
    if shipped_hmm is not None:
        sh = G.HostFullModel.read(shipped_hmm)
        compare(lambda k: getattr(sh, k), 1e-6)
    return hm


# ------------------------------------------------------------- comparators

def close_b(got, ref):
    """linear densities: equal NaN / inf / zero pattern, rtol 1e-11 (1e-300 absolute: a subnormal keeps
    too few bits for a relative bound)"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "infinities differ"
    assert np.array_equal(got[fin] == 0.0, ref[fin] == 0.0), "zeros differ"
    assert np.allclose(got[fin], ref[fin], rtol=1e-11, atol=1e-300), "finite densities differ beyond rtol 1e-11"


def close(got, ref, rtol=1e-11, zeros=True):
    """zeros: the exact zeros must agree (densities, posteriors); gamma and the sums built on it
    may hold a value far below the bound where the other side has 0"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    if zeros:
        assert np.array_equal(got == 0.0, ref == 0.0), "zeros differ"
    scale = np.abs(ref).max() if ref.size else 0.0
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * scale)


def close_logb(got, ref, rtol):
    """equal NaN and infinity patterns, finite values within rtol * (1 + |ref|)"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "infinities differ"
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]) / (1.0 + np.abs(ref[fin]))
    assert err.size == 0 or err.max() <= rtol, f"max error {err.max():.3e}"


def same_kind_close(got, ref, rtol=1e-9, atol=2e-6):
    """equal NaN pattern and equal infinities; the finite entries within rtol / atol"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "inf differs"
    fin = np.isfinite(ref)
    assert np.allclose(got[fin], ref[fin], rtol=rtol, atol=atol), f"finite values beyond rtol {rtol}, atol {atol}"


def same_kind_mask(got, ref, what):
    """equal NaN pattern and equal infinities; returns the mask of the finite reference entries"""
    got, ref = f64(got), f64(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), f"{what}: infinities differ"
    return np.isfinite(ref)


def rel_dist(got, ref):
    """equal NaN and infinity patterns; the worst |got - ref| / |ref| over the finite ones (a finite
    reference of 0, an empty utterance's score, must be met exactly)"""
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), ("NaN pattern differs", got, ref)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), ("infinities differ", got, ref)
    fin = np.isfinite(ref)
    zero = fin & (ref == 0)
    assert np.array_equal(got[zero], ref[zero]), ("a reference of 0 is not met exactly", got, ref)
    fin &= ~zero
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.abs(ref[fin]), initial=0.0))


def assert_close(got, ref, rtol=RTOL, floor=1e-13, what="", rows=False):
    """|got-ref| <= rtol*|ref| + floor*scale; non-finite entries must agree in kind.
    scale = max|ref| over the whole array, or (rows=True: per-frame quantities b, alpha^, beta^,
    gamma, post, whose frames span tens of decades) over the entry's own frame, so that an
    entry is only excused when it is 13 decades below the largest value OF ITS FRAME."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if rows and ref.ndim >= 2:
        r2 = np.abs(ref.reshape(ref.shape[0], -1))
        r2 = np.where(np.isfinite(r2), r2, 0.0)
        rmax = r2.max(axis=1, keepdims=True)
        # (a frame whose reference entries are all 0 — e.g. beta^ of an utterance shorter than the
        # model, underflown in the reference's scaling — has no scale of its own: the array's)
        rmax = np.where(rmax > 0.0, rmax, r2.max() if r2.size else 0.0)
        scale = np.broadcast_to(rmax, r2.shape).ravel()
    else:
        scale = None
    got, ref = got.ravel(), ref.ravel()
    assert got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), f"{what}: inf differs"
    if fin.any():
        sc = np.abs(ref[fin]).max() if scale is None else scale[fin]
        err = np.abs(got[fin] - ref[fin])
        tol = rtol * np.abs(ref[fin]) + floor * sc
        worst = (err / np.maximum(tol, 1e-320)).max()
        assert worst <= 1.0, f"{what}: worst error {worst:.3g} x tolerance"


def check_estep(dev, ref, hm, lens, delta, what):
    """run_device's linear E-step against fulltrain_ref.estep's dict rounded to double: b column by
    column, post and gamma at 1e-11 relative + 1e-11 absolute per entry, the transition sums and den_c
    under close, the log-likelihoods one by one with an equal -inf / NaN pattern"""
    N, M = hm.N, hm.M
    F = dev["b"].shape[0]
    rb, rpost, rgamma = f64(ref["b"]), f64(ref["post"]).reshape(F, N * M), f64(ref["gamma"])
    if F:
        for i in range(N):
            close(dev["b"][:, i], rb[:, i])
    assert np.array_equal(dev["post"] == 0.0, rpost == 0.0), f"{what}: zeros of post differ"
    for key, got, r in (("post", dev["post"], rpost), ("gamma", dev["gamma"], rgamma)):
        assert np.all(np.isfinite(got)), f"{what}: {key} is not finite"
        worst = (np.abs(got - r) / (1e-11 * np.abs(r) + 1e-11)).max() if F else 0.0
        assert worst <= 1.0, f"{what}: {key} worst error {worst:.3g} x tolerance"
    rst = ref["stats"]
    for key in ("num_a", "den_a", "den_c"):
        close(dev["stats"][key], f64(rst[key]), zeros=False)
    fin = same_kind_mask(dev["ll"], ref["loglik"], f"{what}: loglik")
    rll = f64(ref["loglik"])
    for u in np.nonzero(fin)[0]:
        if lens[u] > 0:
            assert dev["ll"][u] == pytest.approx(rll[u], rel=1e-11), (what, u)
    total = float(dev["stats"]["loglik"])
    if same_kind_mask(total, rst["loglik"], f"{what}: summed loglik"):
        assert total == pytest.approx(float(rst["loglik"]), rel=1e-11), what
    assert float(dev["stats"]["n_utt"]) == float(len(lens)), f"{what}: n_utt {float(dev['stats']['n_utt'])}"
    i, j = np.indices((N, N))
    assert np.all(dev["stats"]["num_a"][(j < i) | (j > i + delta)] == 0.0), f"{what}: num_a outside the band"


def check_stats_bound(dev, X, hm, what):
    """the statistics kernel alone: num_c, num_mu, num_cov against fulltrain_ref.stats_from() of the
    DEVICE's own gamma and post, every entry inside (2 F + 8) 2^-53 sum_f |term| (derived in
    test_fullestep_gpu's docstring).  Returns the worst error / bound ratio"""
    from fulltrain_ref import stats_from
    F = len(X)
    s, a = stats_from(dev["gamma"], dev["post"], X, hm.mean, np.longdouble)
    factor = np.longdouble((2 * F + 8) * U53)
    worst = 0.0
    for key in ("num_c", "num_mu", "num_cov"):
        got = dev["stats"][key].reshape(s[key].shape)
        fin = same_kind_mask(got, s[key], f"{what}: {key}")
        err = np.abs(got[fin].astype(np.longdouble) - s[key][fin])
        tol = factor * a[key][fin]
        assert np.all(got[fin][a[key][fin] == 0] == 0.0), f"{what}: {key} holds a value where every term is 0"
        ratio = float((err / np.where(tol > 0, tol, 1)).max()) if err.size else 0.0
        assert np.all(err <= tol), f"{what}: {key} worst error {ratio:.3g} x bound"
        worst = max(worst, ratio)
    return worst


def check_viterbi_lattice(A, logb, lens, path, score):
    """path and score bit for bit the oracle lattice's on the same log b"""
    off = offsets(lens)
    for u, T in enumerate(lens):
        if T == 0:
            assert score[u] == 0.0 and not np.signbit(score[u]), u
            continue
        p, s = O.viterbi_lattice(A, logb[off[u]:off[u + 1]])
        assert np.array_equal(path[off[u]:off[u + 1]], p), u
        assert np.array_equal(np.float64(score[u]), np.float64(s), equal_nan=True), (u, score[u], s)


def check_log_lattice(name, N, got, exact, what="float64", xi=True):
    """one utterance, two fullestep_log_ref.lattice_fb dicts on the same log b: la, lbe, log P inside
    lattice_bound with equal -inf / NaN patterns; gamma and the xi sums inside the expm1(E) bound.
    Returns the worst error / bound."""
    from fullestep_log_ref import gamma_exponent_bound
    from fulllogscore_ref import lattice_bound
    T, V, La = exact["T"], exact["V"], exact["La"]
    if T == 0:
        return 0.0
    worst = 0.0
    lb = lattice_bound(T, N, V, La)
    for key in ("la", "lbe", "logP"):
        g = np.atleast_1d(np.asarray(got[key], dtype=np.longdouble)).ravel()
        r = np.atleast_1d(np.asarray(exact[key], dtype=np.longdouble)).ravel()
        assert np.array_equal(np.isnan(g), np.isnan(r)), (name, key)
        inf = np.isinf(r)
        assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], r[inf]), (name, key)
        fin = np.isfinite(r)
        err = float(np.abs(g[fin] - r[fin]).max(initial=0))
        assert err <= lb, (name, what, key, err, lb)
        worst = max(worst, err / lb)
    E = np.longdouble(gamma_exponent_bound(T, N, V, La))
    g, r = np.asarray(got["gamma"], dtype=np.longdouble), exact["gamma"]
    tol = r * np.expm1(E) + 4 * U53
    assert np.all(np.abs(g - r) <= tol), (name, what, "gamma", float((np.abs(g - r) / tol).max()))
    worst = max(worst, float((np.abs(g - r) / tol).max()))
    if not xi:      # (the device keeps only the sums over the utterances)
        return worst
    g, r = np.asarray(got["xi"], dtype=np.longdouble), exact["xi"]
    tol = r * np.expm1(E) + (T - 1) * 4 * U53 + T * U53 * r       # per term, and the sum's order
    assert np.all(np.abs(g - r) <= tol), (name, what, "xi")
    return worst


# ------------------------------------------------------------- random models and corpora

def banded(rng, N):
    A = np.zeros((N, N))
    for i in range(N - 1):
        A[i, i] = rng.uniform(0.5, 0.9)
        A[i, i + 1] = 1.0 - A[i, i]
    A[N - 1, N - 1] = 1.0
    return A


def ergodic(rng, N, zeros=0.4):
    A = rng.uniform(0.05, 1.0, (N, N)) * (rng.uniform(size=(N, N)) >= zeros)
    A[np.arange(N), (np.arange(N) + 1) % N] += 0.1  # every row reaches somewhere
    return A / A.sum(1, keepdims=True)


def rand_fmodel(G, rng, N, M, D, A=None, *, spread, asym, symmetrise=False, base=None, word="w"):
    """Dirichlet weights, means N(base, spread), inverse covariances with eigenvalues 0.5..2.  The draws,
    in this order: a left-to-right A if none is given, c, the means, one QR and one eigenvalue draw per
    Gaussian, then with `asym` a perturbation that makes Gaussian (0, 0)'s inverse non-symmetric (it
    pins inv_cov[j][i], not [i][j], in the inner sum)."""
    if A is None:
        A = banded(rng, N)
    c = rng.dirichlet(np.full(M, 3.0), N)
    mean = (base if base is not None else 0.0) + rng.normal(0.0, spread, (N, M, D))
    ic = np.empty((N, M, D, D))
    for i in range(N):
        for k in range(M):
            Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
            ic[i, k] = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
            if symmetrise:
                ic[i, k] = (ic[i, k] + ic[i, k].T) / 2
    if asym:
        ic[0, 0] += np.triu(rng.normal(0.0, 0.3, (D, D)), 1)
    return G.HostFullModel(A, c, mean, ic, 1.0 / np.linalg.det(ic), word=word)


def frames(rng, hm, lens, scale=1.0):
    """every frame at the mean of a Gaussian drawn at random, noise `scale`"""
    F = int(np.sum(lens))
    i = rng.integers(0, hm.N, F)
    k = rng.integers(0, hm.M, F)
    return hm.mean[i, k] + rng.normal(0.0, scale, (F, hm.D))


def walk_any(rng, hm, lens):
    """left-to-right walks through the states, one mixture per frame, noise 0.3; an utterance shorter
    than the model takes one frame per state from the first, one of no frames draws nothing"""
    out = [np.zeros((0, hm.D))]
    for T in lens:
        if T >= hm.N:
            cuts = np.sort(rng.choice(np.arange(1, T), hm.N - 1, replace=False))
            st = np.searchsorted(cuts, np.arange(T), side="right")
        else:
            st = np.arange(T)
        k = rng.integers(0, hm.M, T)
        out.append(hm.mean[st, k] + rng.normal(0.0, 0.3, (T, hm.D)))
    return np.concatenate(out)


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ------------------------------------------------------------- the device runner

def run_device(G, ctx, hm, X, lens, *, log, delta=1, options=(), twice=False):
    """estep_full (log: estep_full_log) under `options`; everything the tests look at, downloaded.
    BUF_B arrives as "b" (log: "logb"); the log form also brings la and lbe"""
    N, M, D = hm.N, hm.M, hm.D
    F, U = len(X), len(lens)
    estep = ctx.estep_full_log if log else ctx.estep_full
    fm, corpus = ctx.full_model(hm), ctx.corpus(X, lens)
    st = ctx.stats_full(N, M, D)
    try:
        ctx.set_option(G.OPT_DELTA, delta)
        for opt, val in options:
            ctx.set_option(opt, val)
        estep(fm, corpus, st)
        v = st.download()
        out = dict(v=v, stats=G.split_stats_full(v, N, M, D))
        out["logb" if log else "b"] = ctx.fetch(G.BUF_B, (F, N))
        out["post"], out["gamma"] = ctx.fetch(G.BUF_POST, (F, N * M)), ctx.fetch(G.BUF_GAMMA, (F, N))
        if log:
            out["la"], out["lbe"] = ctx.fetch(G.BUF_ALPHA, (F, N)), ctx.fetch(G.BUF_BETA, (F, N))
        out["ll"] = ctx.fetch(G.BUF_LOGLIK, (U,))
        if log:     # fetching lbe started no linear pass on these buffers
            assert np.array_equal(out["gamma"], ctx.fetch(G.BUF_GAMMA, (F, N))), "gamma changed under the fetches"
            assert np.array_equal(out["la"], ctx.fetch(G.BUF_ALPHA, (F, N)), equal_nan=True), \
                "la changed under the fetches"
        if twice:   # repeated calls at one setting stay bitwise equal
            estep(fm, corpus, st)
            assert np.array_equal(v.view(np.uint64), st.download().view(np.uint64)), "a second call differs"
        return out
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
        for opt, _ in options:
            ctx.set_option(opt, 0)
        st.close(); fm.close(); corpus.close()
