"""The cases of mstep_cases.py reach what they are named for — host only.

test_mstep_gpu.py holds ghmm_mstep to the expected model's bits on these cases; that says nothing if
a "quirk" case never reaches its quirk.  Here each one is checked on the ORACLE's result
(O.mstep, oracle/ghmm_oracle.c: the reference's operations in its order, built without contraction),
with expected values formed by the same IEEE operations in the same order, so compared exactly."""
import numpy as np
import pytest

import mstep_cases as K
import oracle_lib as O


def parts(G, cid):
    c = K.build(G, cid)
    return c, G.split_stats(c.v, *c.shape), K.expected(G, cid)


def ids(name):
    return [k for k in K.ALL if K.CASES[k][0] == name]


def prod_in_order(row):
    d = 1.0
    for x in row:
        d *= float(x)
    return d


def floor_and_renormalise(c):
    """changing_zero_coef, TF:1338-1359"""
    c = [K.FLOOR if float(x) < K.FLOOR else float(x) for x in c]
    s = 0.0
    for x in c:
        s += x
    return np.array([x / s for x in c]), s


def test_case_table():
    """every path of the table by plain, state-skipped and var-floor-all; every quirk at both quirk
    shapes (det-overflow at the small one); the shapes' arithmetic (asserted at import as well)"""
    for shape, path in K.PATHS.items():
        assert K.path_of(*shape) == path
        for name in K.PATH_EDITS:
            assert K.case_id(name, shape) in K.CASES
    assert {K.path_of(*s) for s in K.PATHS} == {"mfma", "lds", "global"}
    for shape in K.QUIRK_SHAPES:
        for name in K.EDITS:
            if name not in ("det-subnormal", "det-overflow"):
                assert K.case_id(name, shape) in K.CASES
    assert K.case_id("det-overflow", (5, 3, 5)) in K.CASES and K.case_id("det-subnormal", (3, 2, 64)) in K.CASES
    for cid in K.ALL:
        N = K.CASES[cid][1][0]
        assert min(K.lens_of(N)) >= N and sum(K.lens_of(N)) <= 100
    # (5, 3, 5): Mp 4, two tiles, tile 0 shared by four states, padding behind the last state;
    # (10, 8, 39): 8 = Mp, one wave per padded Gaussian, N Mp a multiple of 16: no padding columns
    ok, Mp, NT, DP, TC, np_ = K.geometry(5, 3, 5)
    assert (Mp, NT) == (4, 2) and 16 // Mp == 4 and NT * 16 > 5 * Mp
    ok, Mp, NT, DP, TC, np_ = K.geometry(10, 8, 39)
    assert Mp == 8 and NT * 16 == 10 * Mp


@pytest.mark.parametrize("cid", K.ALL)
def test_finite_flag_and_band(G, cid):
    """the `finite` flag agrees with the result; updated rows are +0.0 outside the band and positive
    inside; everything but A is the oracle's own output"""
    c, s, out = parts(G, cid)
    assert K.is_finite_model(out) == c.finite, cid
    N = c.shape[0]
    inside = K.band(N, c.delta)
    upd = s["den_a"] != 0.0
    assert np.all(out.A[upd][~inside[upd]] == 0.0) and not np.any(np.signbit(out.A[upd]))
    assert np.all(out.A[upd][inside[upd]] > 0.0)
    with np.errstate(all="ignore"):
        raw = O.mstep(c.hm, c.v)
    for a, b in zip(out.arrays()[1:], raw.arrays()[1:]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(out.A[inside], raw.A[inside])


@pytest.mark.parametrize("cid", ids("plain") + ids("delta2"))
def test_plain(G, cid):
    """the quotients, the floor, the product in index order.  (With a few dozen frames the larger
    shapes have Gaussians that hold one frame: some variances and weights sit at the floor unedited.)"""
    c, s, out = parts(G, cid)
    assert np.array_equal(out.mean, s["num_mu"] / s["num_c"][..., None])
    var = s["num_var"] / s["num_c"][..., None]
    var = np.where(var < K.FLOOR, K.FLOOR, var)
    assert np.array_equal(out.inv_var, 1.0 / var)
    for i in range(c.shape[0]):
        assert np.array_equal(out.c[i], floor_and_renormalise(s["num_c"][i] / s["den_c"][i])[0])
    for g in ((0, 0), (c.shape[0] - 1, c.shape[1] - 1)):
        assert out.det[g] == prod_in_order(var[g])
    if c.shape == (5, 3, 5):
        assert np.all(var > K.FLOOR) and np.all(out.c > K.FLOOR)     # the small shape has no floor of its own
    if c.name == "delta2":
        i = np.arange(c.shape[0] - 2)
        assert np.all(out.A[i, i + 2] > 0.0) and np.all(c.hm.A > 0.0)


@pytest.mark.parametrize("cid", ids("row-kept"))
def test_row_kept(G, cid):
    """the row is the old one, its entries outside the band (a dense start) included"""
    c, s, out = parts(G, cid)
    r = K.KEPT_ROW
    assert np.array_equal(out.A[r], c.hm.A[r])
    assert np.all(out.A[r][~K.band(c.shape[0], c.delta)[r]] > 0.0)
    assert not np.array_equal(out.A[0], c.hm.A[0]) and np.all(out.A[0][1 + c.delta:] == 0.0)


@pytest.mark.parametrize("cid", ids("state-skipped"))
def test_state_skipped(G, cid):
    """the slot of inverse variances is inverted again, det is their product; mean as it was; c is
    floored and renormalised again"""
    c, s, out = parts(G, cid)
    i = K.SKIPPED
    assert np.array_equal(out.inv_var[i], 1.0 / c.hm.inv_var[i])
    assert np.array_equal(out.mean[i], c.hm.mean[i])
    for k in range(c.shape[1]):
        assert out.det[i, k] == prod_in_order(c.hm.inv_var[i, k])
    assert not np.allclose(out.det[i], c.hm.det[i], rtol=1e-3)      # not last iteration's det
    assert np.array_equal(out.c[i], floor_and_renormalise(c.hm.c[i])[0])
    assert not np.array_equal(out.mean[0], c.hm.mean[0])            # the other states are updated


@pytest.mark.parametrize("cid", ids("nothing-updated"))
def test_nothing_updated(G, cid):
    c, s, out = parts(G, cid)
    assert np.array_equal(out.A, c.hm.A) and np.array_equal(out.mean, c.hm.mean)
    assert np.array_equal(out.inv_var, 1.0 / c.hm.inv_var)
    assert not s["num_c"].any()                                     # no count: the old data centre stays
    for i in range(c.shape[0]):
        assert np.array_equal(out.c[i], floor_and_renormalise(c.hm.c[i])[0])


@pytest.mark.parametrize("cid", ids("weight-floor") + ids("weight-floor-finite"))
def test_weight_floor(G, cid):
    """the floored weight is 1e-5 / sum, the sum taken in index order over the floored weights; the
    Gaussian without a count has 0/0 mean and variances that no floor touches, and a NaN det"""
    c, s, out = parts(G, cid)
    i, M = K.WF_STATE, c.shape[1]
    raw = s["num_c"][i] / s["den_c"][i]
    assert 0.0 < raw[K.WF_TINY] < K.FLOOR
    want, total = floor_and_renormalise(raw)
    assert np.array_equal(out.c[i], want) and out.c[i, K.WF_TINY] == K.FLOOR / total
    assert np.all(np.isfinite(out.mean[i, K.WF_TINY])) and np.all(np.isfinite(out.inv_var[i, K.WF_TINY]))
    nan = {k: np.isnan(getattr(out, k)) for k in ("A", "c", "mean", "inv_var", "det")}
    if c.name == "weight-floor":
        z = K.WF_ZERO
        assert raw[z] == 0.0 and out.c[i, z] == K.FLOOR / total
        exp_mean = np.zeros(out.mean.shape, bool)
        exp_mean[i, z] = True
        exp_det = np.zeros(out.det.shape, bool)
        exp_det[i, z] = True
        assert np.array_equal(nan["mean"], exp_mean) and np.array_equal(nan["inv_var"], exp_mean)
        assert np.array_equal(nan["det"], exp_det) and not nan["A"].any() and not nan["c"].any()
    else:
        assert not any(v.any() for v in nan.values())


@pytest.mark.parametrize("cid", ids("var-floor-all") + ids("det-subnormal"))
def test_var_floor_all(G, cid):
    """every variance of the Gaussian at the floor: inverse variances 1 / 1e-5, det = 1e-5^D in index
    order — 1e-25 at D = 5, subnormal at D = 63 and 64; a collapsed component (class 1: cond > 1e4
    around the data centre, no coefficient above the floor)"""
    c, s, out = parts(G, cid)
    N, M, D = c.shape
    g = K.SUBNORMAL if c.name == "det-subnormal" else K.floored_gaussian(N, M)
    assert np.all(s["num_var"][g] / s["num_c"][g] < K.FLOOR)
    assert np.all(out.inv_var[g] == 1.0 / K.FLOOR)
    assert out.det[g] == prod_in_order([K.FLOOR] * D) and out.det[g] > 0.0
    if D == 5:
        assert out.det[g] == pytest.approx(1e-25, rel=1e-12)
    if D >= 63:
        assert out.det[g] < np.finfo(np.float64).tiny                # subnormal, not 0
    if D == 64:
        assert out.det[g] == pytest.approx(1e-320, rel=1e-3)
    centre = s["num_mu"].sum((0, 1)) / s["num_c"].sum()
    assert np.sum((out.mean[g] - centre) ** 2 * out.inv_var[g]) > K.COND_MAX
    assert not np.any(out.inv_var[g] < 0.99 / K.FLOOR)
    if c.name == "var-floor-all":                                    # the edit collapses it, not the data
        assert np.sum(K.expected(G, K.case_id("plain", c.shape)).inv_var[g] < 0.99 / K.FLOOR) >= D - 1


@pytest.mark.parametrize("cid", ids("var-negative"))
def test_var_negative(G, cid):
    c, s, out = parts(G, cid)
    plain = K.expected(G, K.case_id("plain", c.shape))
    assert s["num_var"][K.NEG] < 0.0 and out.inv_var[K.NEG] == 1.0 / K.FLOOR != plain.inv_var[K.NEG]
    assert np.sum(out.inv_var != plain.inv_var) == 1 and np.sum(out.det != plain.det) == 1


@pytest.mark.parametrize("cid", ids("narrow-one-coefficient"))
def test_narrow_one_coefficient(G, cid):
    """class 2: cond > 1e4 around the data centre of the EDITED vector, with variances above the floor"""
    c, s, out = parts(G, cid)
    i, k, d = K.NARROW
    centre = s["num_mu"].sum((0, 1)) / s["num_c"].sum()
    assert abs(out.mean[i, k, d] - centre[d]) >= 2.0
    assert out.inv_var[i, k, d] == pytest.approx(1e4, rel=1e-12) and np.any(out.inv_var[i, k] < 0.99 / K.FLOOR)
    assert np.sum((out.mean[i, k] - centre) ** 2 * out.inv_var[i, k]) > K.COND_MAX


@pytest.mark.parametrize("cid", ids("det-overflow"))
def test_det_overflow(G, cid):
    c, s, out = parts(G, cid)
    assert out.det[K.OVER] == np.inf and np.all(np.isfinite(out.inv_var[K.OVER])) and np.all(out.inv_var[K.OVER] > 0.0)
    assert np.sum(~np.isfinite(out.det)) == 1 and np.all(np.isfinite(out.mean))


@pytest.mark.parametrize("cid", ids("band-dirty-delta2"))
def test_band_dirty(G, cid):
    """the dirt is outside the band only: the expected model is delta2's"""
    c, s, out = parts(G, cid)
    N = c.shape[0]
    assert np.all(s["num_a"][~K.band(N, 2)] == 0.37)
    with np.errstate(all="ignore"):
        assert np.all(O.mstep(c.hm, c.v).A[~K.band(N, 2)] > 0.0)     # the oracle does not mask
    clean = K.expected(G, K.case_id("delta2", c.shape))
    for a, b in zip(out.arrays(), clean.arrays()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("cid", ids("nan-in-one-state"))
def test_nan_in_one_state(G, cid):
    c, s, out = parts(G, cid)
    exp = np.zeros(out.mean.shape, bool)
    exp[K.NAN_G] = True
    assert np.array_equal(np.isnan(out.mean), exp)
    assert not any(np.isnan(getattr(out, k)).any() for k in ("A", "c", "inv_var", "det"))


def test_det_underflow_and_overflow_at_d70(G):
    """one state, two mixtures, D = 70: variances at the floor give det == 0 exactly, variances of 3e4
    give inf (the product in index order); neither shape is taken by the device tests' follow-up calls"""
    rng = np.random.default_rng(5)
    N, M, D = 1, 2, 70
    hm = G.HostModel(np.ones((1, 1)), np.full((1, 2), 0.5), rng.normal(size=(N, M, D)), np.ones((N, M, D)),
                     np.ones((N, M)))
    v = np.zeros(G.stats_len(N, M, D))
    s = G.split_stats(v, N, M, D)
    s["num_a"][:], s["den_a"][:], s["den_c"][:], s["num_c"][:] = 3.0, 4.0, 10.0, 5.0
    s["num_mu"][:] = 5.0 * hm.mean
    s["num_var"][0, 0], s["num_var"][0, 1] = 5.0 * 1e-9, 5.0 * 3e4
    out = O.mstep(hm, v)
    assert out.det[0, 0] == 0.0 and out.det[0, 1] == np.inf and not K.is_finite_model(out)
    assert np.all(out.inv_var[0, 0] == 1.0 / K.FLOOR)


def test_det_subnormal_follow_up_is_decided_by_the_oracle(G):
    cid = K.case_id("det-subnormal", (3, 2, 64))
    c = K.build(G, cid)
    with np.errstate(all="ignore"):
        fin = bool(np.all(np.isfinite(O.estep(K.expected(G, cid), c.X, c.lens, dumps=False)[0])))
    assert K.follow_up(G, cid) == fin
    assert all(K.follow_up(G, k) == K.EDITS[K.CASES[k][0]][0] for k in K.ALL if k != cid)


@pytest.mark.parametrize("cid", [K.case_id("plain", s) for s in ((10, 8, 39), (2, 96, 13), (2, 97, 13), (2, 184, 39))])
def test_weight_sum_order_shows_in_the_bits(G, cid):
    """one shape per code path where the weights summed from the other end give other bits: a device
    sum out of index order cannot pass the bit comparison there"""
    c, s, out = parts(G, cid)
    differs = False
    for i in range(c.shape[0]):
        raw = s["num_c"][i] / s["den_c"][i]
        assert np.array_equal(out.c[i], floor_and_renormalise(raw)[0])
        differs |= not np.array_equal(out.c[i], floor_and_renormalise(raw[::-1])[0][::-1])
    assert differs
