"""The diagonal log-domain Baum-Welch E-step on the GPU: ghmm_estep_log and ghmm_estep_log_streams (the
emission's "log b and posteriors" mode on both tiers, k_logfb_fwd / k_logfb_bwd up to 64 states,
k_logfb_wide_fwd / k_logfb_wide_bwd beyond, then ghmm_estep's statistics launches) and the trainer's
GHMM_LOG_TRAIN=1 — GPU box only.  The cases and the reference are estep_log_ref.py's; test_estep_log_host.py
shows on the CPU that they hold what is leaned on here.  Everything runs under GHMM_OPT_KERNELS = 1 and under
the default (matrix-core) tier.

  emission     log b bit for bit ghmm_viterbi's (ghmm_logscore's beyond Viterbi's 255 states); post against the
               long-double restatement at RTOL on every frame but the far one, equal zeros; on the far frame each
               state's posteriors sum to 1 within 1e-9 and lie within max(RTOL, 8 x the float64 restatement's
               distance) of the restatement
  lattice      the long-double recursion on the DEVICE's own log b and post: la, lbe, log P inside
               fulllogscore_ref.lattice_bound, gamma and the transition sums inside the expm1(E) bounds of
               test_fullestep_log_gpu.check_sums, every frame's gammas summing to rho_u; delta 0, 2, 3
  identities   bit for bit: BUF_LOGLIK = logscore(final_state=True), one stream = the single call, a second
               call, GHMM_OPT_PARTIALS, the common sums of two streams, BUF_B = viterbi_streams' sum
  statistics   num_c, num_mu, num_var against the long-double calc_mix_param of the device's own gamma and post at
               RTOL; without the far frame the whole vector against estep on the same context at RTOL
  the point    a far frame in every utterance: estep's loglik is not finite, estep_log's vector and the model
               mstep makes of it are, and the next log-likelihood is no lower; two streams; 70 states
  four EM iterations against the oracle's linear trajectory; the contract; the command line"""
import json
import os
import subprocess

import numpy as np
import pytest

import estep_log_ref as E
import logscore_cases as LC
import oracle_lib as O
from _load import PKG_DIR
from conftest import GOLDEN
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import RTOL, U53, assert_close, check_log_lattice, code, extended, offsets
from streams_util import synth_case
from test_fullestep_log_gpu import check_sums
from test_logscore_gpu import TIERS, same, tier_of, timed
from vocab_cases import rand_model

pytestmark = pytest.mark.gpu

TRAIN = os.path.join(PKG_DIR, "bin", "hmm-continuous-train-fs")
FAR = LC.FAR_FRAME


class Device:
    """a case's device models, corpora and statistics vectors, and per (tier, delta) what estep_log (two streams:
    estep_log_streams) leaves, downloaded once: v[p], stats[p], logb, posts[p], la, lbe, gamma, ll, and beside
    them vit = BUF_B after viterbi (None beyond 255 states), ls_b = BUF_B after logscore, ls = logscore's
    scores with final_state 0 and 1.  posts[p] of a several-stream call, which the workspace does not serve, is
    BUF_POST after estep_log on stream p alone: the same emission launch."""

    def __init__(self, G, ctx, name, far=True):
        self.G, self.ctx, self.name = G, ctx, name
        self.case = case = E.make(G, name, far)
        self.hms = case.words[0]
        self.N, self.P, self.F, self.U = case.Ns[0], case.P, case.F, case.U
        self.dms = [ctx.model(h) for h in self.hms]
        self.corpora = [ctx.corpus(X, case.lens) for X in case.Xs]
        self.st = [ctx.stats(h.N, h.M, h.D) for h in self.hms]
        self._run = {}

    def call(self):
        if self.P == 1:
            self.ctx.estep_log(self.dms[0], self.corpora[0], self.st[0])
        else:
            self.ctx.estep_log_streams(self.dms, self.corpora, self.st)

    def fetch_all(self):
        G, ctx, F, N = self.G, self.ctx, self.F, self.N
        r = {"v": [s.download() for s in self.st]}
        r["stats"] = [G.split_stats(v, h.N, h.M, h.D) for v, h in zip(r["v"], self.hms)]
        r["logb"], r["gamma"] = ctx.fetch(G.BUF_B, (F, N)), ctx.fetch(G.BUF_GAMMA, (F, N))
        r["la"], r["lbe"] = ctx.fetch(G.BUF_ALPHA, (F, N)), ctx.fetch(G.BUF_BETA, (F, N))
        r["ll"] = ctx.fetch(G.BUF_LOGLIK, (self.U,))
        # fetching lbe started no linear pass on these buffers
        assert np.array_equal(r["gamma"], ctx.fetch(G.BUF_GAMMA, (F, N))), "gamma changed under the fetches"
        assert np.array_equal(r["la"], ctx.fetch(G.BUF_ALPHA, (F, N)), equal_nan=True), "la changed under the fetches"
        if self.P == 1:
            r["posts"] = [ctx.fetch(G.BUF_POST, (F, N * self.hms[0].M))]
        return r

    def run(self, tier, delta=1):
        if (tier, delta) in self._run:
            return self._run[tier, delta]
        G, ctx = self.G, self.ctx
        with tier_of(G, ctx, tier):
            ctx.set_option(G.OPT_DELTA, delta)
            try:
                self.call()
                r = self.fetch_all()
                if self.P > 1:
                    assert code(G, lambda: ctx.fetch(G.BUF_POST, (1,))) == G.ERR_ARG
                    r["posts"] = []
                    one = [ctx.stats(h.N, h.M, h.D) for h in self.hms]
                    for m, c, s, h in zip(self.dms, self.corpora, one, self.hms):
                        ctx.estep_log(m, c, s)
                        r["posts"].append(ctx.fetch(G.BUF_POST, (self.F, self.N * h.M)))
                        s.close()
            finally:
                ctx.set_option(G.OPT_DELTA, 1)
            r["vit"] = None
            if self.N <= 255:
                if self.P == 1:
                    ctx.viterbi(self.dms[0], self.corpora[0])
                else:
                    ctx.viterbi_streams(self.dms, self.corpora)
                r["vit"] = ctx.fetch(G.BUF_B, (self.F, self.N))
            r["ls"] = {}
            for fs in (0, 1):
                r["ls"][fs] = (ctx.logscore(self.dms[0], self.corpora[0], final_state=bool(fs)) if self.P == 1 else
                               ctx.logscore_streams(self.dms, self.corpora, final_state=bool(fs)))
            r["ls_b"] = ctx.fetch(G.BUF_B, (self.F, self.N))
        self._run[tier, delta] = r
        return r

    def close(self):
        for o in self.dms + self.corpora + self.st:
            o.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name, far=True):
        if (name, far) not in made:
            made[name, far] = Device(G, ctx, name, far)
        return made[name, far]
    yield get
    for d in made.values():
        d.close()


# ------------------------------------------------------------- 1. emission

@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", E.NAMES)
def test_emission(G, ctx, devices, name, tier):
    d = devices(name)
    r = d.run(tier)
    if r["vit"] is not None:
        assert same(r["logb"], r["vit"]), "log b is not ghmm_viterbi's"
    assert same(r["logb"], r["ls_b"]), "log b is not ghmm_logscore's"
    _, ld = E.reference(G, name)
    _, f64 = E.reference(G, name, ft=np.float64)
    near = np.arange(d.F) != FAR
    for p, (got, hm) in enumerate(zip(r["posts"], d.hms)):
        ref = np.asarray(ld["posts"][p], dtype=np.float64).reshape(d.F, -1)
        assert_close(got[near], ref[near], rows=True, what=f"{name} tier {tier} stream {p}: post")
        assert np.array_equal(got[near] == 0.0, ref[near] == 0.0), "zeros of post differ"
        far_got, far_ref = got[FAR].reshape(d.N, hm.M), ref[FAR].reshape(d.N, hm.M)
        sums = far_got.sum(1)
        alive = np.isfinite(ld["posts"][p][FAR]).all(1) & (np.asarray(ld["posts"][p][FAR]).sum(1) != 0)
        assert np.all(np.abs(sums[alive] - 1.0) <= 1e-9), "a state's posteriors of the far frame do not sum to 1"
        d64 = E.row_dist(f64["posts"][p][FAR], ld["posts"][p][FAR])
        bar = max(RTOL, 8.0 * d64)
        dist = E.row_dist(far_got, far_ref)
        print(f"{name} tier {tier} stream {p}: far frame's post at {dist:.2e} (bar {bar:.1e}, float64 {d64:.1e})")
        assert dist <= bar


@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nt", (0, 2), ids=["nt-auto", "nt-off"])
@pytest.mark.parametrize("N,M,D", [(10, 8, 39), (7, 3, 39), (3, 5, 15), (3, 16, 39), (2, 32, 39), (2, 64, 15)])
def test_emission_at_the_matrix_core_kernels_shapes(G, ctx, N, M, D, nt, tier):
    """the shapes at which k_emission_sched takes another path: the benchmark's 10 x 8 at D = 39 (whole tiles, the
    16-byte stores), mixtures padded 3 -> 4 (the guarded stores), an odd Gaussian count (no aligned pairs), one
    state per tile, a state on two and on four tiles, at 16 and 40 operand columns; 106 frames (six whole
    frame tiles and one of 10), frame 5 far away; with the non-temporal stores and (GHMM_OPT_NT_POST = 2) without"""
    from fullcov_support import banded, frames
    rng = np.random.default_rng(1000 + 100 * N + M)
    hm = rand_model(G, rng, N, M, D, banded(rng, N))
    lens = np.array([37, 64, 5], dtype=np.int32)
    X = frames(rng, hm, lens)
    X[FAR] += LC.FAR
    F = len(X)
    model, corpus, st = ctx.model(hm), ctx.corpus(X, lens), ctx.stats(N, M, D)
    try:
        with tier_of(G, ctx, tier):
            ctx.set_option(G.OPT_NT_POST, nt)
            try:
                ctx.estep_log(model, corpus, st)
            finally:
                ctx.set_option(G.OPT_NT_POST, 0)
            logb, got = ctx.fetch(G.BUF_B, (F, N)), ctx.fetch(G.BUF_POST, (F, N * M))
            ctx.viterbi(model, corpus)
            assert same(logb, ctx.fetch(G.BUF_B, (F, N))), "log b is not ghmm_viterbi's"
    finally:
        for o in (model, corpus, st):
            o.close()
    ld = E.posteriors(hm, X)
    ref = np.asarray(ld, dtype=np.float64).reshape(F, -1)
    near = np.arange(F) != FAR
    assert_close(got[near], ref[near], rows=True, what="post")
    assert np.array_equal(got[near] == 0.0, ref[near] == 0.0), "zeros of post differ"
    assert np.all(np.abs(got[FAR].reshape(N, M).sum(1) - 1.0) <= 1e-9)
    d64 = E.row_dist(E.posteriors(hm, X[FAR:FAR + 1], np.float64)[0], ld[FAR])
    dist = E.row_dist(got[FAR].reshape(N, M), ref[FAR].reshape(N, M))
    print(f"{N}x{M}x{D} tier {tier} nt {nt}: far frame's post at {dist:.2e} (float64 {d64:.1e})")
    assert dist <= max(RTOL, 8.0 * d64)


# ------------------------------------------------------------- 2. the lattice on the device's own log b and post

def check_on_own_emission(d, r, delta, what):
    """the long-double lattice and sums on the device's own log b and posteriors; returns that reference"""
    N, lens = d.N, d.case.lens
    ref = E.estep(d.hms, d.case.Xs, lens, delta, np.longdouble, logb=r["logb"], posts=r["posts"])
    off = offsets(lens)
    worst = 0.0
    for u, ut in enumerate(ref["utt"]):
        s = slice(off[u], off[u + 1])
        got = {"la": r["la"][s], "lbe": r["lbe"][s], "logP": r["ll"][u], "gamma": r["gamma"][s]}
        if ut["T"] == 0:
            assert r["ll"][u] == 0.0 and not np.signbit(r["ll"][u])
            continue
        worst = max(worst, check_log_lattice(f"{what}[{u}]", N, got, ut, what="GPU", xi=False))
        if np.isfinite(ut["logZ"]):         # a frame's gammas sum to rho_u
            rho = np.exp(ut["logP"] - ut["logZ"])
            Eb = np.longdouble(E.LE.gamma_exponent_bound(ut["T"], N, ut["V"], ut["La"]))
            ssum = r["gamma"][s].astype(np.longdouble).sum(1)
            assert np.all(np.abs(ssum - rho) <= rho * np.expm1(Eb) + N * 4 * U53), (what, u)
        else:
            assert np.all(r["gamma"][s] == 0.0), (what, u)
    for p in range(d.P):
        w2 = check_sums({"stats": r["stats"][p]}, {"utt": ref["utt"], "stats": ref["stats"][p]}, N, delta, lens,
                        f"{what} stream {p}")
        assert float(r["stats"][p]["n_utt"]) == float(len(lens))
        total, rt = float(r["stats"][p]["loglik"]), ref["stats"][p]["loglik"]
        assert np.isnan(total) == bool(np.isnan(rt)) and np.isinf(total) == bool(np.isinf(rt)), (what, total, rt)
        if np.isfinite(rt):
            bound = sum(E.LR.lattice_bound(ut["T"], N, ut["V"], ut["La"]) for ut in ref["utt"] if ut["T"])
            bound += len(lens) * U53 * float(np.abs(ref["loglik"]).sum())
            assert abs(np.longdouble(total) - rt) <= bound, what
        else:
            assert total == float(rt)
    print(f"{what}: lattice worst error / bound {worst:.4f}, sums {w2:.4f}")
    return ref


LATTICE_RUNS = [(n, 1) for n in E.NAMES] + [(n, dl) for n in E.DELTA_CASES for dl in E.DELTAS]


@extended
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name,delta", LATTICE_RUNS)
def test_lattice_on_the_devices_own_emission(G, ctx, devices, name, delta, tier):
    d = devices(name)
    r = d.run(tier, delta)
    ref = check_on_own_emission(d, r, delta, f"{name} tier {tier} delta {delta}")
    # statistics: calc_mix_param of the device's own gamma and post, in long double, at RTOL
    for p, hm in enumerate(d.hms):
        for k in ("num_c", "num_mu", "num_var"):
            assert_close(r["stats"][p][k], np.asarray(ref["stats"][p][k], dtype=np.float64),
                         what=f"{name} tier {tier} stream {p} {k}")
    lens, ll = np.asarray(d.case.lens), r["ll"]
    if name.endswith("_c0"):
        assert (ll[lens > 0] == -np.inf).all() and np.all(r["gamma"] == 0.0) and (r["logb"][:, 1] == -np.inf).all()
    elif name.endswith("_nan"):
        assert np.isnan(r["logb"][:, 3]).all() and np.isfinite(ll[0]) and np.all(r["gamma"] == 0.0)
    elif "banded" in name:
        short = (lens > 0) & (lens < d.N)
        assert (ll[short] == -np.inf).all() and np.isfinite(ll[lens >= d.N]).all()


# ------------------------------------------------------------- 3. identities, bit for bit

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", E.NAMES)
def test_loglik_is_the_log_score(G, ctx, devices, name, tier):
    d = devices(name)
    r = d.run(tier)
    assert same(r["ll"], r["ls"][1]), "BUF_LOGLIK is not logscore(final_state=True)"
    assert np.isfinite(r["ls"][0][np.asarray(d.case.lens) > 0]).all() or name in E.EDITED


@pytest.mark.parametrize("tier", TIERS)
def test_one_stream_a_second_call_and_partials(G, ctx, devices, tier):
    with tier_of(G, ctx, tier):
        for name in ("lane_6x2x9_banded", "lane_9x2x5_dense", "wide_65x1x4_banded", "wide_70x1x4_dense", "p2_6_banded",
                     "p2_70_banded"):
            d = devices(name)
            want = d.run(tier)
            for partials in (1, 3, 0):
                ctx.set_option(G.OPT_PARTIALS, partials)
                try:
                    d.call()
                    first = [s.download() for s in d.st]
                    d.call()                # a second call repeats every byte
                    assert all(same(a, s.download()) for a, s in zip(first, d.st)), (name, partials)
                    r = d.fetch_all()
                finally:
                    ctx.set_option(G.OPT_PARTIALS, 0)
                for k in ("logb", "la", "lbe", "gamma", "ll"):
                    assert same(r[k], want[k]), (name, partials, k)
                if d.P == 1:
                    assert same(r["posts"][0], want["posts"][0]), (name, partials)
                if partials == 0:
                    assert all(same(a, b) for a, b in zip(r["v"], want["v"])), name
            if d.P == 1:                    # n_streams == 1 is the single call
                ctx.estep_log_streams(d.dms, d.corpora, d.st)
                r = d.fetch_all()
                assert same(r["v"][0], want["v"][0]) and same(r["logb"], want["logb"]), name
                assert same(r["posts"][0], want["posts"][0]) and same(r["gamma"], want["gamma"]), name
                ctx.set_option(G.OPT_ROBUST, 1)     # no effect on one stream, as in ghmm_logscore
                try:
                    d.call()
                    assert same(d.st[0].download(), want["v"][0]), name
                finally:
                    ctx.set_option(G.OPT_ROBUST, 0)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(E.STREAMS))
def test_two_streams_share_the_common_sums(G, ctx, devices, name, tier):
    d = devices(name)
    r = d.run(tier)
    for k in E.COMMON:
        assert same(r["stats"][0][k], r["stats"][1][k]), k
    assert same(r["logb"], r["vit"]), "BUF_B is not the sum viterbi_streams leaves"


# ------------------------------------------------------------- 4. without the far frame: the linear call

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", [n for n in E.NAMES if n not in E.EDITED])
def test_the_whole_vector_is_esteps_where_that_is_finite(G, ctx, devices, name, tier):
    d = devices(name, far=False)
    r = d.run(tier)
    lin = [ctx.stats(h.N, h.M, h.D) for h in d.hms]
    try:
        with tier_of(G, ctx, tier):
            if d.P == 1:
                ctx.estep(d.dms[0], d.corpora[0], lin[0])
            else:
                ctx.estep_streams(d.dms, d.corpora, lin)
        for p, (s, h) in enumerate(zip(lin, d.hms)):
            want = G.split_stats(s.download(), h.N, h.M, h.D)
            assert np.isfinite(want["num_var"]).all()
            for k in E.BLOCKS:
                assert_close(r["stats"][p][k], want[k], what=f"{name} tier {tier} stream {p} {k}")
    finally:
        for s in lin:
            s.close()


# ------------------------------------------------------------- 5. the point of the feature

def far_in_every_utterance(G, N, shapes, lens, seed):
    """a banded word on the streams `shapes`, frames walking through it, one far frame in every utterance"""
    from fullstreams_ref import stream_frames
    from fullcov_support import banded
    rng = np.random.default_rng(seed)
    A = banded(rng, N)
    hms = [rand_model(G, rng, N, M, D, A.copy()) for M, D in shapes]
    Xs = stream_frames(rng, hms, lens)
    off = offsets(lens)
    for u in range(len(lens)):
        for X in Xs:
            X[off[u] + 7 + 3 * u] += 60.0
    return hms, Xs, np.asarray(lens, dtype=np.int32)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("N,shapes,lens", [
    (5, ((2, 8),), (60, 45, 81, 70)),
    (6, ((2, 5), (3, 4)), (60, 45, 81, 70)),
    (70, ((2, 5),), (150, 120, 200)),
], ids=["one-stream", "two-streams", "70-states"])
def test_far_frames_train_where_the_linear_call_cannot(G, ctx, N, shapes, lens, tier):
    hms, Xs, lens = far_in_every_utterance(G, N, shapes, lens, 61 + N)
    dms = [ctx.model(h) for h in hms]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    st = [ctx.stats(h.N, h.M, h.D) for h in hms]
    try:
        with tier_of(G, ctx, tier):
            ctx.estep_streams(dms, corpora, st)
            assert not np.isfinite(st[0].loglik()[0])           # the linear call is lost here
            ctx.estep_log_streams(dms, corpora, st)
            for s in st:
                assert np.all(np.isfinite(s.download()))
            ll0 = st[0].loglik()[0]
            for m, s in zip(dms, st):
                ctx.mstep(m, s)
            for m in dms:
                for a in m.get().arrays():
                    assert np.all(np.isfinite(a))
            ctx.estep_log_streams(dms, corpora, st)
            ll1 = st[0].loglik()[0]
        print(f"far frames, {N} states, {len(shapes)} stream(s), tier {tier}: loglik {ll0:.3f} -> {ll1:.3f}")
        assert np.isfinite(ll1) and ll1 >= ll0
    finally:
        for o in dms + corpora + st:
            o.close()


# ------------------------------------------------------------- 6. four EM iterations

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("N,M,D,lens", [(6, 2, 9, (70, 90, 80, 64, 75)), (70, 1, 4, (150, 170, 160))],
                         ids=["6x2x9", "70x1x4"])
def test_four_em_iterations_track_the_oracles_linear_trajectory(G, ctx, N, M, D, lens, tier):
    """(estep_log, mstep) from HostModel.init_from on a clean synthetic corpus against (oracle_lib.estep, mstep):
    the log-likelihood trace and the last model at RTOL"""
    hm0, X, lens = synth_case(G, N, M, D, list(lens))
    hm = G.HostModel.init_from(X, lens, N, M)
    ref, trace = hm.copy(), []
    for _ in range(4):
        v, _ = O.estep(ref, X, lens, dumps=False)
        trace.append(v[-2])
        ref = O.mstep(ref, v)
    assert np.all(np.isfinite(trace))
    model, corpus, st = ctx.model(hm), ctx.corpus(X, lens), ctx.stats(N, M, D)
    try:
        with tier_of(G, ctx, tier):
            got = []
            for _ in range(4):
                ctx.estep_log(model, corpus, st)
                got.append(st.loglik()[0])
                ctx.mstep(model, st)
            new = model.get()
    finally:
        for o in (model, corpus, st):
            o.close()
    e_tr = max(abs(x - y) / abs(y) for x, y in zip(got, trace))
    e_model = max(E.block_dist(a, b) for a, b in zip(new.arrays(), ref.arrays()))
    print(f"{N}x{M}x{D} tier {tier}: trace error {e_tr:.1e}, model error {e_model:.1e}")
    assert e_tr <= RTOL
    for k, a, b in zip(("A", "c", "mean", "inv_var", "det"), new.arrays(), ref.arrays()):
        assert_close(a, b, what=k)


# ------------------------------------------------------------- 7. the contract

def test_refusals_write_nothing(G, ctx, devices):
    d1, d2 = devices("lane_6x2x9_banded"), devices("p2_6_banded")
    rng = np.random.default_rng(23)
    h = d1.hms[0]
    big_h = [rand_model(G, rng, 513, M, D, np.eye(513)) for M, D in ((h.M, h.D),) + E.STREAM_SHAPES]
    big = [ctx.model(x) for x in big_h]
    big_st = [ctx.stats(513, x.M, x.D) for x in big_h]
    full = ctx.stats_full(h.N, h.M, h.D)
    other = ctx.stats(h.N, h.M + 1, h.D)
    other_n = ctx.model(rand_model(G, rng, 7, *E.STREAM_SHAPES[1], np.eye(7)))
    try:
        d1.call()
        d2.call()
        keep = [s.download() for s in d1.st + d2.st]
        pattern = np.full(big_st[0].download().shape, -777.0)
        big_st[0].upload(pattern)
        assert code(G, lambda: ctx.estep_log(big[0], d1.corpora[0], big_st[0])) == G.ERR_UNSUPPORTED
        assert same(big_st[0].download(), pattern), "513 states: the vector was written"
        assert code(G, lambda: ctx.estep_log_streams(big[1:], d2.corpora, big_st[1:])) == G.ERR_UNSUPPORTED
        assert code(G, lambda: ctx.estep_log(d1.dms[0], d1.corpora[0], full)) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_log(d1.dms[0], d1.corpora[0], other)) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_log(d1.dms[0], d2.corpora[0], d1.st[0])) == G.ERR_ARG      # another D
        # the streams call: check_streams, then every stream's vector
        assert code(G, lambda: ctx.estep_log_streams([d2.dms[0], other_n], d2.corpora, d2.st)) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_log_streams(d2.dms, [d2.corpora[0], d1.corpora[0]], d2.st)) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_log_streams(d2.dms, d2.corpora, [d2.st[0], other])) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_log_streams(d2.dms, d2.corpora, [d2.st[0], full])) == G.ERR_ARG
        assert code(G, lambda: ctx.estep_log_streams(d2.dms * 5, d2.corpora * 5, d2.st * 5)) == G.ERR_ARG      # P = 10
        ctx.set_option(G.OPT_ROBUST, 1)
        try:
            assert code(G, lambda: ctx.estep_log_streams(d2.dms, d2.corpora, d2.st)) == G.ERR_UNSUPPORTED
        finally:
            ctx.set_option(G.OPT_ROBUST, 0)
        assert all(same(a, s.download()) for a, s in zip(keep, d1.st + d2.st)), "a refusal wrote a vector"
    finally:
        for o in big + big_st + [full, other, other_n]:
            o.close()


def test_empty_corpus_after_a_busy_call(G, ctx, devices):
    for name in ("lane_6x2x9_banded", "wide_65x1x4_banded", "p2_6_banded"):
        d = devices(name)
        empty = [ctx.corpus(np.zeros((0, h.D)), np.zeros(0, dtype=np.int32)) for h in d.hms]
        try:
            d.call()
            assert all(np.any(s.download() != 0.0) for s in d.st)
            if d.P == 1:
                ctx.estep_log(d.dms[0], empty[0], d.st[0])
            else:
                ctx.estep_log_streams(d.dms, empty, d.st)
            assert all(np.all(s.download() == 0.0) for s in d.st), name
        finally:
            for c in empty:
                c.close()


def test_launch_counts(G, ctx, devices):
    for name in ("lane_6x2x9_banded", "wide_65x1x4_banded", "p2_6_banded", "p2_70_banded"):
        d = devices(name)
        d.call()
        kt = timed(G, ctx, d.call)
        assert kt.get("emission") == 2 * d.P - 1 and kt.get("forward") == 2 and "backward" not in kt, (name, kt)
        # the row API does not reuse the log b
        assert code(G, lambda: ctx.forward(d.dms[0], d.corpora[0])) == G.ERR_ARG


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("N,M,D,lens,dense", [(10, 8, 39, [90, 120, 65, 5, 1], False), (70, 2, 5, [90, 120], True)])
def test_linear_estep_afterwards_is_unchanged(G, ctx, N, M, D, lens, dense, tier):
    """no stale log state: estep after estep_log on the same context still meets test_gpu_parity's bar against the
    oracle, and fetch(BUF_BETA) there still starts its on-demand pass"""
    from streams_util import assert_frames
    hm, X, lens = synth_case(G, N, M, D, lens, dense_A=dense)
    ref_stats, ref = O.estep(hm, X, lens)
    model, corpus, st = ctx.model(hm), ctx.corpus(X, lens), ctx.stats(N, M, D)
    F = len(X)
    try:
        with tier_of(G, ctx, tier):
            ctx.estep_log(model, corpus, st)
            ctx.fetch(G.BUF_BETA, (F, N))
            ctx.estep(model, corpus, st)
            assert_frames(ctx.fetch(G.BUF_B, (F, N)), ref["b"], "b")
            assert_frames(ctx.fetch(G.BUF_POST, (F, N * M)), ref["post"].reshape(F, -1), "post")
            assert_frames(ctx.fetch(G.BUF_ALPHA, (F, N)), ref["alpha"], "alpha")
            assert_frames(ctx.fetch(G.BUF_BETA, (F, N)), ref["beta"], "beta")
            assert_close(ctx.fetch(G.BUF_LOGLIK, (len(lens),)), ref["loglik"], what="loglik")
            got, refs = G.split_stats(st.download(), N, M, D), G.split_stats(ref_stats, N, M, D)
        for k in refs:
            assert_close(got[k], refs[k], what="stats." + k)
    finally:
        for o in (model, corpus, st):
            o.close()


# ------------------------------------------------------------- 8. the command line

def test_command_line_log_train(G, ctx, tmp_path):
    """hmm-continuous-train-fs with GHMM_LOG_TRAIN=1 on one bundled word: the notice line; the iteration count and
    the model written = the device's initial model, then (estep_log, mstep) under the program's stopping rule, array for
    array.  Without the variable: the golden report of whole_program.json."""
    whole = json.load(open(os.path.join(GOLDEN, "whole_program.json")))
    word = "vc_186_f_03_ap_0225"
    perfil = os.path.join(GOLDEN, "perfil", f"mean_{word}.perfil")
    tmp = str(tmp_path)
    lst = os.path.join(tmp, "parameters.txt")
    open(lst, "w").write(perfil + "\n")
    out = os.path.join(tmp, "result.hmm")

    def train(env):
        p = subprocess.run([TRAIN, word, "6", "1", "1", lst, out], cwd=tmp, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300, env=env)
        text = p.stdout.decode(errors="replace")
        assert p.returncode == 0, text[-2000:]
        return text, open(os.path.join(tmp, "result.txt")).read().split("\n")
    plain = {k: v for k, v in os.environ.items() if k != "GHMM_LOG_TRAIN"}
    text, report = train(plain)
    exp = whole["train13_m1"][word]
    assert "E-step in the log domain" not in text
    assert report[9] == f"mean probability: {exp['mean_probability']:f} "
    assert report[10] == f"number of iterations: {exp['iterations']} "

    text, report = train(dict(plain, GHMM_LOG_TRAIN="1"))
    assert "E-step in the log domain (GHMM_LOG_TRAIN)" in text
    iterations = int(next(l for l in report if l.startswith("number of iterations")).split(":")[1])
    X = G.perfil_read(perfil)
    lens = np.array([len(X)], dtype=np.int32)
    model, corpus = ctx.model(G.HostModel.init_from(X, lens, 6, 1)), ctx.corpus(X, lens)
    st = ctx.stats(6, 1, X.shape[1])
    try:
        model.init_from(corpus, fetch=False)       # the program's initial model: built on the device
        old, n = 1.0, 0
        while True:
            n += 1
            ctx.estep_log(model, corpus, st)
            probab = st.loglik()[0]
            if not abs((old - probab) / old) > 1.0e-3:
                break
            old = probab
            ctx.mstep(model, st)
        hm = model.get()
    finally:
        for o in (model, corpus, st):
            o.close()
    assert n == iterations
    got = G.HostModel.read(out)
    assert got.word == word
    for a, b in zip(got.arrays(), hm.arrays()):
        np.testing.assert_array_equal(a, b)
