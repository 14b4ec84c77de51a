"""ghmm_model_init — the diagonal trainer's initial model built on the MI355X — against the host init
(ghmm_init_model, pinned bit for bit to TF) and its long-double restatement (init_ref.init_diag).  GPU box
only.  The corpora, what each is there for, and the admission condition they meet on the CPU
(test_init_host) are in init_ref's docstring.  Every case runs on both tiers: "vector" is GHMM_OPT_KERNELS = 1
(the k-means passes' sums from k_mixstats), "default" takes them from the matrix-core expanded-form sums
where the model has that form (D <= 64) — except `tie`, whose exactness argument holds for the vector tier.

1. Discrete parts: A and c are the host's bits, the counts recovered from c are the restatement's, the
   one-hot gamma rows (fetched from the workspace) give the restatement's state for every frame, mean,
   inv_var and det have the host's NaN / zero pattern and the same entries at the 1e-5 floor.
2. Accuracy: mean, inv_var and det by rel_dist from the long-double restatement.  With e_host the host
   init's own distance the device must stay within 16 e_host + 64 eps (eps = 2^-52): both routes add the
   same terms in different orders.  The default tier's means add run_accumulate's kappa and nothing else
   (mean_widening).  The measured ratios are recorded in profiles/init_accuracy.txt.
3. Repeatability: a second call and a fresh context give the same bits.
4. Call order: init and two EM iterations with no host synchronisation in between, alone and after an
   unrelated E-step of another shape in the same context, give the same statistics bits; log P is finite and
   within item 2's bound of the run started from the host's model.  The init leaves no mixture posteriors:
   GHMM_BUF_POST is refused until the next emission.
5. Grid options: GHMM_OPT_CUS = 8 and GHMM_OPT_PARTIALS = 3 change the order of the sums only.
6. Refusals leave the model alone and the context usable.
7. A frame farther than 1e20 from every cell goes to cell 0 (include/ghmm.h), not to the previous frame's
   cell as on the host: the discrete parts against the restatement under that rule, vector tier."""
import contextlib

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: one HIP runtime in the process)

import init_ref as R
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import banded, code, need_extended, rel_dist, same_kind_mask
from streams_util import bits_equal

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
KEYS = ("A", "c", "mean", "inv_var", "det")
TIERS = {"vector": 1, "default": 0}
RUNS = [(name, tier) for name in R.CASES for tier in TIERS if not (name == "tie" and tier == "default")]
IDS = [f"{name}-{tier}" for name, tier in RUNS]


def blank(G, N, M, D):
    return G.HostModel(np.eye(N), np.full((N, M), 1.0 / M), np.zeros((N, M, D)), np.ones((N, M, D)), np.ones((N, M)))


@contextlib.contextmanager
def options(G, ctx, tier, extra=()):
    ctx.set_option(G.OPT_KERNELS, TIERS[tier])
    for opt, val in extra:
        ctx.set_option(opt, val)
    try:
        yield
    finally:
        ctx.set_option(G.OPT_KERNELS, 0)
        for opt, _ in extra:
            ctx.set_option(opt, 0)


def device_init(G, ctx, X, lens, N, M, tier, extra=()):
    """(the model ghmm_model_init builds, the workspace's one-hot gamma rows)"""
    model, corpus = ctx.model(blank(G, N, M, X.shape[1])), ctx.corpus(X, lens)
    try:
        with options(G, ctx, tier, extra):
            got = model.init_from(corpus)
            return got, ctx.fetch(G.BUF_GAMMA, (len(X), N))
    finally:
        model.close(); corpus.close()


_cache, _host = {}, {}


def result(G, ctx, name, tier):
    """computed once per case and tier, shared, not modified"""
    if (name, tier) not in _cache:
        _cache[name, tier] = device_init(G, ctx, *R.corpus(name), tier)
    return _cache[name, tier]


def host_init(G, name):
    if name not in _host:
        _host[name] = G.HostModel.init_from(*R.corpus(name))
    return _host[name]


def check_discrete(got, gamma, host, ref, what):
    N, M = ref["count"].shape
    assert bits_equal(got.A, host.A), what
    assert np.all((gamma == 0) | (gamma == 1)) and np.all(gamma.sum(1) == 1), what
    assert np.array_equal(gamma.argmax(1), ref["state"]), what
    assert np.array_equal(gamma.sum(0), ref["dur"]), what
    assert bits_equal(got.c, host.c), what
    with np.errstate(invalid="ignore"):
        back = got.c * ref["dur"][:, None]
    free = ref["count"].min(1) > 0          # no weight at the floor: c dur gives the counts back
    assert np.array_equal(np.rint(back[free]), ref["count"][free]), what
    for key in ("mean", "inv_var", "det"):
        a, b = getattr(got, key), getattr(host, key)
        fin = same_kind_mask(a, b, f"{what}.{key}")
        assert np.array_equal(a[fin] == 0, b[fin] == 0), f"{what}.{key}: zeros differ"
    assert np.array_equal(got.inv_var == 1.0 / R.FLOOR, host.inv_var == 1.0 / R.FLOOR), f"{what}: floored variances"


@pytest.mark.parametrize("name,tier", RUNS, ids=IDS)
def test_discrete_parts(G, ctx, name, tier):
    got, gamma = result(G, ctx, name, tier)
    check_discrete(got, gamma, host_init(G, name), R.reference(name, False), f"{name}/{tier}")


def distances(model, ref):
    return {key: rel_dist(getattr(model, key), ref[key]) for key in ("mean", "inv_var", "det")}


def bound(e_host, widen=0.0):
    """the full-covariance suite's form, 16 e_host + 64 eps, plus `widen` (mean_widening, the default tier's
    means only); never above the 1e-9 that test_device_initial_model_against_reference asserts"""
    return min(16 * e_host + 64 * EPS + widen, 1e-9)


def mean_widening(name, cus=256):
    """The one widening, for the means of the default tier where the model has the matrix-core form
    (D <= 64): the project's own relative rounding bound for those sums, `kappa` in run_accumulate,
    2 u (F / (4 CUs) + 2 CUs + 64) with u = 2^-53 — the length of a wave's share of the frames plus the
    partials, times u, doubled — and nothing on top of it.  Why the means need it: there the k-means passes
    give mean = (S1 + o S0) / S0 with S1 = sum (x - o) over the cell's frames, S0 their count and o the
    expanded form's offset, the mean of the model's means.  S1 cancels against o S0, so a coefficient whose
    cell mean is small next to the data's centre (the clouds sit around 6 +- 2, a few centres come near 0)
    is not as close to the restatement as the host's plain sum, which is all that e_host sees.  kappa is
    1.28e-13 at 256 CUs and 2.3e-14 at 8 for d39m8, where the largest measured errors are 7.5e-14 and
    2.6e-14: the margin is a factor of 2."""
    X, lens, N, M = R.corpus(name)
    F, D = X.shape
    if D > 64:
        return 0.0
    return 2.0 * 2.0 ** -53 * (F / (cus * 4.0) + 2.0 * cus + 64.0)


def check_accuracy(G, name, tier, got, label="init accuracy", cus=256):
    ref = R.reference(name, True)
    e_host, e_dev = distances(host_init(G, name), ref), distances(got, ref)
    widen = {key: mean_widening(name, cus) if (key, tier) == ("mean", "default") else 0.0 for key in e_host}
    for key in e_host:
        ratio = e_dev[key] / e_host[key] if e_host[key] else float("inf") if e_dev[key] else 0.0
        print(f"{label} {name:11s} {tier:7s} {key:7s} e_host {e_host[key]:.3e} e_dev {e_dev[key]:.3e} ratio {ratio:.3g} "
              f"bound {bound(e_host[key], widen[key]):.3e} (of which widening {widen[key]:.3e})")
    for key in e_host:
        assert e_dev[key] <= bound(e_host[key], widen[key]), (name, tier, key, e_dev[key], e_host[key])


@pytest.mark.parametrize("name,tier", RUNS, ids=IDS)
def test_accuracy_against_long_double(G, ctx, name, tier):
    """every case, tie included: it is not admitted by the gap condition, but its long-double run makes the
    float64 run's decisions (asserted here), so the reference is one for it as well"""
    need_extended()
    assert R.same_decisions(R.reference(name, False), R.reference(name, True)), name
    check_accuracy(G, name, tier, result(G, ctx, name, tier)[0])


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["m5", "ragged", "m65"])
def test_repeatable(G, ctx, name, tier):
    """the partial sums are added in block order: nothing depends on which block finishes first"""
    corpus = R.corpus(name)
    first = result(G, ctx, name, tier)[0]
    again = device_init(G, ctx, *corpus, tier)[0]
    fresh_ctx = G.Context(0)
    try:
        fresh = device_init(G, fresh_ctx, *corpus, tier)[0]
    finally:
        fresh_ctx.close()
    for key in KEYS:
        assert bits_equal(getattr(first, key), getattr(again, key)), (name, tier, key, "second call")
        assert bits_equal(getattr(first, key), getattr(fresh, key)), (name, tier, key, "fresh context")


def em_twice(ctx, model, corpus, st):
    for _ in range(2):
        ctx.estep(model, corpus, st)
        ctx.mstep(model, st)
    return st.download()            # the second E-step's statistics (the M-step leaves them as they are)


@pytest.mark.parametrize("tier", TIERS)
def test_call_order(G, ctx, tier):
    need_extended()
    name = "m3"
    X, lens, N, M = R.corpus(name)
    D, F = X.shape[1], len(X)
    model, corpus, st = ctx.model(blank(G, N, M, D)), ctx.corpus(X, lens), ctx.stats(N, M, D)
    rng = np.random.default_rng(3)
    other_lens = [45, 71]
    other_hm = blank(G, 7, 2, 9)
    other_hm.A[:] = banded(rng, 7)
    other_hm.mean[:] = rng.normal(0.0, 1.0, other_hm.mean.shape)
    other_X = rng.normal(0.0, 1.0, (sum(other_lens), 9))
    other, other_c, other_st = ctx.model(other_hm), ctx.corpus(other_X, other_lens), ctx.stats(7, 2, 9)
    try:
        with options(G, ctx, tier):
            ctx.emission(model, corpus, True)
            ctx.fetch(G.BUF_POST, (F, N * M))                # an emission's posteriors are served
            model.init_from(corpus, fetch=False)             # nothing waits between the calls
            assert code(G, lambda: ctx.fetch(G.BUF_POST, (F, N * M))) == G.ERR_ARG      # the init's one-hot rows are not
            model.init_from(corpus, fetch=False)
            v1 = em_twice(ctx, model, corpus, st)
            ctx.estep(other, other_c, other_st)              # another shape's E-step leaves its state in the context
            model.init_from(corpus, fetch=False)
            assert code(G, lambda: ctx.fetch(G.BUF_POST, (F, N * M))) == G.ERR_ARG
            ctx.emission(model, corpus, True)
            post = ctx.fetch(G.BUF_POST, (F, N * M))         # served again
            assert np.all(np.isfinite(post)) and not np.all((post == 0) | (post == 1))
            v2 = em_twice(ctx, model, corpus, st)
            assert np.array_equal(v1.view(np.uint64), v2.view(np.uint64))
            model.set(host_init(G, name))
            vh = em_twice(ctx, model, corpus, st)
    finally:
        for o in (model, corpus, st, other, other_c, other_st):
            o.close()
    lp, lp_host = v1[-2], vh[-2]
    e_host = max(distances(host_init(G, name), R.reference(name, True)).values())
    print(f"init call order {tier}: log P {lp!r} from the device's model, {lp_host!r} from the host's, "
          f"rel {abs(lp - lp_host) / abs(lp_host):.3e}, bound {bound(e_host):.3e}")
    assert np.isfinite(lp) and np.isfinite(lp_host)
    assert abs(lp - lp_host) <= bound(e_host) * abs(lp_host)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("opt,val", [("OPT_CUS", 8), ("OPT_PARTIALS", 3)])
def test_grid_options(G, ctx, opt, val, tier):
    need_extended()
    name = "d39m8"
    got, gamma = device_init(G, ctx, *R.corpus(name), tier, extra=[(getattr(G, opt), val)])
    check_discrete(got, gamma, host_init(G, name), R.reference(name, False), f"{name}/{tier}/{opt}")
    check_accuracy(G, name, tier, got, label=f"init accuracy {opt}={val}", cus=val if opt == "OPT_CUS" else 256)


def test_refusals(G, ctx):
    X, lens, N, M = R.corpus("m2")
    D = X.shape[1]
    start = blank(G, N, M, D)
    start.mean[:] = np.arange(N * M * D).reshape(N, M, D)
    model = ctx.model(start)
    other_d = ctx.corpus(np.ones((20, D + 1)), [20])
    empty = ctx.corpus(np.zeros((0, D)), np.zeros(0, dtype=np.int32))
    corpus = ctx.corpus(X, lens)
    try:
        before = model.get()
        assert code(G, lambda: model.init_from(empty)) == G.ERR_ARG
        assert code(G, lambda: model.init_from(other_d)) == G.ERR_ARG
        for a, b, c in zip(before.arrays(), model.get().arrays(), start.arrays()):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        got = model.init_from(corpus)       # and the context still works
        gamma = ctx.fetch(G.BUF_GAMMA, (len(X), N))
    finally:
        for o in (model, other_d, empty, corpus):
            o.close()
    check_discrete(got, gamma, host_init(G, "m2"), R.reference("m2", False), "m2 after the refusals")
    first = result(G, ctx, "m2", "default")[0]
    for key in KEYS:
        assert bits_equal(getattr(got, key), getattr(first, key)), key


def test_no_candidate_takes_cell_zero(G, ctx):
    """R.far_corpus: one frame at 1e11, no cell within 1e20.  The device puts it into cell 0 in every pass;
    test_init_host shows that the host's rule gives another model on this corpus"""
    X, lens, N, M, t = R.far_corpus()
    ref = R.far_reference("zero")
    got, gamma = device_init(G, ctx, X, lens, N, M, "vector")
    expected = G.HostModel(ref["A"], ref["c"], ref["mean"], ref["inv_var"], ref["det"])
    check_discrete(got, gamma, expected, ref, "far")
    assert not bits_equal(got.c, R.far_reference("carry")["c"])
