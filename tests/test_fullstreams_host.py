"""The host side of the full-covariance programs on several feature streams (CPU only): the file
format (ghmm_hmm_read_full_streams / ghmm_hmm_write_full_streams) against the file the real reference
wrote, and the pins of tests/fullstreams_ref.py, the restatement that test_fullstreams_gpu.py holds
the HIP code against.

(a) full_streams_models/all13_6_p2.hmm, written by the reference's trainer, read back bit for bit
    what make_golden_fullstreams.py's own struct parser recorded (fullstreams_models.npz); the
    write -> read round trip with 4- and 8-byte prefixes; a file one byte short and a diagonal file
    give ERR_FORMAT; HostFullModel.read on the two-stream file still gives ERR_UNSUPPORTED.
(b) the float64 restatement from ghmm_init_model_full per stream, with ghmm_mstep_full_host per
    stream, reproduces every recorded training run of the real reference: iteration count, the mean
    probability at the printed 6 decimals, and the written model at test_fulltrain_ref_host's bar
    (fulltrain_ref.model_err <= 1e-8 per stream, A included).
(c) on one stream the restatement is fulltrain_ref.estep / fullestep_log_ref.estep /
    fullscore_ref.score / fulllogscore_ref.logscore bit for bit, and the summed-log calls agree with
    the product's where both are finite."""
import json
import os

import numpy as np
import pytest

import fullestep_log_ref as LE
import fulllogscore_ref as LR
import fullscore_ref as SR
import fullstreams_ref as S
import fulltrain_ref as R
from conftest import GOLDEN
from fullcov_support import code, rand_fmodel, report_value, walk_any

P2 = json.load(open(os.path.join(GOLDEN, "fullstreams_p2.json")))
FIXTURE = os.path.join(GOLDEN, "full_streams_models", "all13_6_p2.hmm")
KEYS = ("c", "mean", "det", "inv_cov")


@pytest.fixture(scope="module")
def models():
    return np.load(os.path.join(GOLDEN, "fullstreams_models.npz"))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------- (a) the file format

def test_reads_the_reference_file_bit_for_bit(G, models):
    hms = G.HostFullModel.read_streams(FIXTURE)
    assert len(hms) == 2 and [h.M for h in hms] == [2, 1] and [h.D for h in hms] == [9, 5]
    for p, hm in enumerate(hms):
        assert hm.word == "all13_6_p2" and hm.N == 6
        assert same_bits(hm.A, models["all13_6_p2.A"])
        for key in KEYS:
            assert same_bits(getattr(hm, key), models[f"all13_6_p2.s{p}.{key}"]), (p, key)


@pytest.mark.parametrize("len_bytes", [4, 8])
def test_round_trip(G, tmp_path, len_bytes):
    hms = G.HostFullModel.read_streams(FIXTURE)
    out = str(tmp_path / "rt.hmm")
    G.HostFullModel.write_streams(out, hms, len_bytes)
    if len_bytes == 8:
        assert open(out, "rb").read() == open(FIXTURE, "rb").read()
    else:
        assert os.path.getsize(out) == os.path.getsize(FIXTURE) - 4
    back = G.HostFullModel.read_streams(out)
    assert len(back) == 2
    for a, b in zip(hms, back):
        assert a.word == b.word
        for x, y in zip(a.arrays(), b.arrays()):
            assert same_bits(x, y)
    # three streams, and the cap of the caller
    three = hms + [hms[1]]
    G.HostFullModel.write_streams(out, three, len_bytes)
    assert [h.D for h in G.HostFullModel.read_streams(out)] == [9, 5, 5]
    assert code(G, lambda: G.HostFullModel.read_streams(out, max_streams=2)) == G.ERR_UNSUPPORTED


def test_one_stream_file_is_the_single_stream_writers(G, tmp_path):
    hm = G.HostFullModel.read_streams(FIXTURE)[0]
    a, b = str(tmp_path / "a.hmm"), str(tmp_path / "b.hmm")
    hm.write(a)
    G.HostFullModel.write_streams(b, [hm])
    assert open(a, "rb").read() == open(b, "rb").read()
    assert len(G.HostFullModel.read_streams(a)) == 1


def test_refusals(G, tmp_path):
    raw = open(FIXTURE, "rb").read()
    short = str(tmp_path / "short.hmm")
    open(short, "wb").write(raw[:-1])
    assert code(G, lambda: G.HostFullModel.read_streams(short)) == G.ERR_FORMAT
    longer = str(tmp_path / "long.hmm")
    open(longer, "wb").write(raw + b"\0")
    assert code(G, lambda: G.HostFullModel.read_streams(longer)) == G.ERR_FORMAT
    # a diagonal file of two streams
    hms = G.HostFullModel.read_streams(FIXTURE)
    diag = str(tmp_path / "diag.hmm")
    G.HostModel.write_streams(diag, [G.HostModel(h.A, h.c, h.mean, np.ones_like(h.mean), h.det, word="w")
                                     for h in hms])
    assert code(G, lambda: G.HostFullModel.read_streams(diag)) == G.ERR_FORMAT
    assert code(G, lambda: G.HostFullModel.read_streams(str(tmp_path / "missing.hmm"))) == G.ERR_IO
    # the single-stream reader keeps refusing several streams
    assert code(G, lambda: G.HostFullModel.read(FIXTURE)) == G.ERR_UNSUPPORTED
    # streams that differ in N are not written
    other = G.HostFullModel(np.eye(5), hms[1].c[:5], hms[1].mean[:5], hms[1].inv_cov[:5], hms[1].det[:5])
    assert code(G, lambda: G.HostFullModel.write_streams(str(tmp_path / "x.hmm"), [hms[0], other])) == G.ERR_ARG


# ------------------------------------------------------------- (b) the recorded runs

def recorded(name):
    return P2["train"].get(name) or P2["word_models"][name]


@pytest.mark.parametrize("name", sorted(P2["train"]) + sorted(P2["word_models"]))
def test_recorded_runs(G, models, name):
    run = recorded(name)
    Xs, lens = S.bundled_streams(G, GOLDEN, P2["mean_list"], run["utterances"])
    hms, it, p = S.train(G, Xs, lens, run["N"], run["M"], np.float64)
    ref = run["report"]
    assert it == int(report_value(ref, "number of iterations")) == len(run["verify"]), name
    assert f"{p:f}" == report_value(ref, "mean probability"), name
    assert report_value(ref, "number of parameters") == "2"
    worst = 0.0
    for s, hm in enumerate(hms):
        assert np.array_equal(hm.A, hms[0].A), "every stream's M-step writes the same A"
        worst = max(worst, R.model_err(hm, lambda k: models[f"{name}.A" if k == "A" else f"{name}.s{s}.{k}"]))
    print(f"{name}: iterations {it}, mean probability {p:.6f}, model error {worst:.2e}")
    assert worst <= 1e-8, (name, worst)


# ------------------------------------------------------------- (c) one stream, and log against linear

def small_case(G):
    rng = np.random.default_rng(11)
    lens = np.array([40, 5, 0, 33], dtype=np.int32)
    h0 = rand_fmodel(G, rng, 6, 2, 5, spread=1.0, asym=True)
    h1 = rand_fmodel(G, rng, 6, 3, 3, h0.A, spread=1.0, asym=False)
    return [h0, h1], [walk_any(rng, h0, lens), walk_any(rng, h1, lens)], lens


def test_one_stream_is_the_single_stream_restatement(G):
    hms, Xs, lens = small_case(G)
    ft = np.float64
    a, b = S.estep(hms[:1], Xs[:1], lens, 1, ft), R.estep(hms[0], Xs[0], lens, 1, ft)
    assert np.array_equal(R.pack(a["stats"][0]), R.pack(b["stats"]), equal_nan=True)
    for k in ("b", "gamma", "alpha", "beta", "loglik"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    a, b = S.estep_log(hms[:1], Xs[:1], lens, 1, ft), LE.estep(hms[0], Xs[0], lens, 1, ft)
    assert np.array_equal(R.pack(a["stats"][0]), R.pack(b["stats"]), equal_nan=True)
    assert np.array_equal(S.score(hms[:1], Xs[:1], lens, ft), SR.score(hms[0], Xs[0], lens, ft), equal_nan=True)
    for fs in (0, 1):
        assert np.array_equal(S.logscore(hms[:1], Xs[:1], lens, fs, ft), LR.logscore(hms[0], Xs[0], lens, fs, ft),
                              equal_nan=True)


def test_two_streams_log_and_linear_agree(G):
    hms, Xs, lens = small_case(G)
    ft = np.float64
    lin, log = S.estep(hms, Xs, lens, 1, ft), S.estep_log(hms, Xs, lens, 1, ft)
    np.testing.assert_allclose(np.exp(log["logb"]), lin["b"], rtol=1e-12)
    assert np.array_equal(lin["b"], lin["bs"][0] * lin["bs"][1])
    fin = np.isfinite(lin["loglik"])
    assert list(fin) == [True, False, True, True] and np.array_equal(np.isfinite(log["loglik"]), fin)   # T = 5 < N
    np.testing.assert_allclose(log["loglik"][fin], lin["loglik"][fin], rtol=1e-12)
    for p in range(2):
        sl, sg = lin["stats"][p], log["stats"][p]
        for k in ("num_a", "den_a", "den_c", "num_c", "num_mu", "num_cov"):
            np.testing.assert_allclose(sg[k], sl[k], rtol=1e-9, atol=1e-9 * np.abs(sl[k]).max(), err_msg=f"{p} {k}")
    sc, lsc = S.score(hms, Xs, lens, ft), S.logscore(hms, Xs, lens, 0, ft)
    np.testing.assert_allclose(lsc, sc, rtol=1e-12)
    assert np.array_equal(S.logscore(hms, Xs, lens, 1, ft)[fin], log["loglik"][fin])


def test_far_case_underflows_only_in_the_product(G):
    """the GPU suite's underflow case is what it says: on frame 5 each stream's densities are positive
    doubles, their product is 0 for every state, and the log-domain score stays finite"""
    hms, Xs, lens = S.make_far_case(G)
    b, bs, _ = S.emission(hms, Xs, np.float64)
    assert bs[0][5].max() > 0 and bs[1][5].max() > 0 and np.all(b[5] == 0.0)
    assert np.all(b[np.arange(len(b)) != 5].max(1) > 0)
    sc = S.score(hms, Xs, lens, np.float64)
    assert not np.isfinite(sc[0]) and np.isfinite(sc[1])
    assert np.isfinite(S.logscore(hms, Xs, lens, 0, np.float64)).all()
