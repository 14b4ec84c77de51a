"""The extended Baum-Welch update on the CPU: the positivity argument of include/ghmm.h on ebw_cases' restatement,
what the update reduces to with an empty denominator and with equal vectors, the hand-made cases' reach, the
float64 evaluation's distance from the long-double one, and the entry points' declarations.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import ebw_cases as B
import estep_log_ref as E
import oracle_lib as O
from _load import ROOT, load_pkg
from fullcov_support import RTOL, extended

LD = np.longdouble


def one(dc, dm, dv, s2, cd, Ec=2.0, ft=LD):
    """the update of single coefficients: arrays of dc, dm (around the old mean 0), dv, s2 and cd"""
    dc, dm, dv, s2, cd = (np.asarray(x, dtype=np.float64).astype(ft).reshape(-1, 1) for x in (dc, dm, dv, s2, cd))
    num = {"num_c": dc[:, :] + cd, "num_mu": (dm + 0)[..., None], "num_var": dv[..., None]}
    den = {"num_c": cd, "num_mu": np.zeros_like(dm)[..., None], "num_var": np.zeros_like(dv)[..., None]}
    mean = np.zeros(dm.shape + (1,))
    return B.gaussians(mean, 1 / np.asarray(s2, dtype=np.float64)[..., None], np.ones(dc.shape), num, den, Ec, ft)


# ------------------------------------------------------------- 1. positivity

@extended
def test_the_variance_is_positive_beyond_the_larger_root():
    """random and adversarial (dc, dm, dv): (dc + damp)^2 s2' = q(damp), q(-dc) = -dm^2 <= 0, and with damp =
    max(E cd, twice the larger root) every Gaussian that is not kept has dc + damp > 0 and s2' > 0 before the
    floor"""
    rng = np.random.default_rng(5)
    n = 4000
    dc = rng.normal(0, 3, n)
    dm = rng.normal(0, 5, n) * rng.choice([1e-6, 1.0, 1e3], n)
    dv = rng.normal(0, 5, n) * rng.choice([1e-6, 1.0, 1e3], n)
    s2 = rng.uniform(1e-4, 50, n)
    cd = np.abs(rng.normal(0, 3, n)) * rng.choice([0.0, 1.0], n)
    adv = np.array([  # dc, dm, dv, s2, cd
        [-5.0, 0.0, -100.0, 1.0, 5.0], [-5.0, 30.0, -100.0, 1.0, 5.0], [0.0, 1.0, 0.0, 1.0, 0.0],
        [1.0, 0.0, -1e6, 1e-3, 0.0], [-1e-9, 1e-3, -1e3, 10.0, 1e-9], [3.0, 1e4, 1.0, 2.0, 0.0],
        [-2.0, 0.0, 0.0, 1.0, 2.0], [0.0, 0.0, -1.0, 1.0, 0.0], [1e-12, 1e-12, -1e-12, 1.0, 0.0],
        [-1.0, 1e-8, 1.0, 1e-4, 1.0]])
    dc, dm, dv, s2, cd = (np.concatenate([x, adv[:, i]]) for i, x in enumerate((dc, dm, dv, s2, cd)))
    for Ec in (0.0, 2.0):
        mean, var, det, kept, damp, raw = one(dc, dm, dv, s2, cd, Ec)
        kept, damp, raw = kept[:, 0], damp[:, 0], raw[:, 0, 0]
        L = lambda x: np.asarray(x, dtype=np.float64).astype(LD)      # noqa: E731
        a, b, q0 = L(s2), L(dv) + L(s2) * L(dc), L(dv) * L(dc) - L(dm) * L(dm)
        q = lambda x: (a * x + b) * x + q0                            # noqa: E731
        assert np.all(q(-L(dc)) <= 1e-12 * (np.abs(a * L(dc) ** 2) + np.abs(b * L(dc)) + np.abs(q0) + 1e-300))
        live = ~kept
        assert live.sum() > n // 2
        t = L(dc) + damp
        assert np.all(t[live] > 0)
        assert np.all(raw[live] > 0), (Ec, float(raw[live].min()))
        scale = np.abs(a * damp * damp) + np.abs(b * damp) + np.abs(q0)
        assert np.all(np.abs(t * t * raw - q(damp))[live] <= 1e-14 * scale[live])
        # no statistics at all: kept
        assert kept[(dc == 0) & (damp == 0)].all()


# ------------------------------------------------------------- 2. what it reduces to

@extended
@pytest.mark.parametrize("shape", B.SHAPES[:2])
def test_an_empty_denominator_is_maximum_likelihood_around_the_new_mean(G, shape):
    """den = 0: the mean is num_mu / num_c and the variance the moment around the NEW mean, which is
    ghmm_mstep's variance (the moment around the OLD mean) less (mu' - mu)^2; A and c are ghmm_mstep's"""
    case = B.build(G, "den-zero", shape)
    r = B.ebw(case.hm, case.num, case.den, case.E)
    ml = O.mstep(case.hm, case.num)
    num = B.split(case.num, *shape, LD)
    # (Cauchy-Schwarz: dv dc >= dm^2, so no root is positive but by the rounding of a Gaussian that holds one frame)
    assert not r["kept"].any() and np.all(r["damp"] <= 1e-12 * num["num_c"])
    assert E.block_dist(r["mean"], num["num_mu"] / num["num_c"][..., None]) <= 1e-12
    step = r["mean"] - case.hm.mean
    assert np.abs(step).max() > 1e-3
    want = 1 / ml.inv_var.astype(LD) - step * step
    free = (r["raw"] > 2 * B.FLOOR) & (1 / ml.inv_var > 2 * B.FLOOR)
    assert free.sum() >= 20      # (the Gaussians that hold a few frames sit on the floor in both)
    assert np.all(np.abs(r["var"] - want)[free] <= 1e-12 * (1 / ml.inv_var)[free])
    assert E.block_dist(r["A"], ml.A) <= 1e-15 and E.block_dist(r["c"], ml.c) <= 1e-15


@extended
@pytest.mark.parametrize("shape", B.SHAPES[:2])
def test_equal_vectors_leave_the_gaussians_where_they_are(G, shape):
    """num = den: the means keep their bits and the variances their values; the weights and transitions are
    still the numerator's"""
    case = B.build(G, "equal", shape)
    for ft in (LD, np.float64):
        r = B.ebw(case.hm, case.num, case.den, case.E, ft=ft)
        assert not r["kept"].any() and np.all(r["damp"] > 0)
        assert np.array_equal(r["mean"], case.hm.mean.astype(ft))
        assert E.block_dist(r["inv_var"], case.hm.inv_var) <= 4e-16
    assert E.block_dist(r["A"], O.mstep(case.hm, case.num).A) <= 1e-15


@extended
@pytest.mark.parametrize("shape", B.SHAPES)
def test_the_cases_reach_what_they_are_named_for(G, shape):
    N, M, D = shape
    r = B.ebw(*B.build(G, "neg-dv", shape)[2:6])
    num, den = (B.split(v, N, M, D) for v in B.build(G, "neg-dv", shape)[3:5])
    assert np.all((num["num_var"] - den["num_var"])[B.NEG_STATE] < 0)
    assert np.mean(r["damp"][B.NEG_STATE] > 2.0 * den["num_c"][B.NEG_STATE]) > 0.5, "the roots do not decide damp"
    assert np.all(r["var"] >= B.FLOOR) and np.all(np.isfinite(r["var"]))
    c = B.build(G, "no-stats", shape)
    r = B.ebw(c.hm, c.num, c.den, c.E)
    assert r["kept"][B.NO_STATS] and r["kept"].sum() == 1
    assert np.array_equal(r["mean"][B.NO_STATS], c.hm.mean[B.NO_STATS].astype(LD))
    assert np.array_equal(r["inv_var"][B.NO_STATS], c.hm.inv_var[B.NO_STATS].astype(LD))
    assert r["det"][B.NO_STATS] == c.hm.det[B.NO_STATS]
    c = B.build(G, "row-kept", shape)
    r = B.ebw(c.hm, c.num, c.den, c.E)
    assert np.array_equal(r["A"][B.KEPT_ROW], c.hm.A[B.KEPT_ROW].astype(LD)) and np.any(np.tril(c.hm.A, -1)[B.KEPT_ROW] > 0)
    c = B.build(G, "state-skipped", shape)
    r = B.ebw(c.hm, c.num, c.den, c.E)
    assert E.block_dist(r["c"][B.SKIPPED], c.hm.c[B.SKIPPED]) <= 1e-15 and not r["kept"].any()
    r = B.ebw(*B.build(G, "plain", shape)[2:6])
    assert not r["kept"].any() and np.all(np.isfinite(r["det"])) and np.all(r["det"] > 0)


# ------------------------------------------------------------- 3. float64 against long double

@extended
@pytest.mark.parametrize("shape", B.SHAPES)
@pytest.mark.parametrize("name", B.EDITS)
def test_float64_spread(G, name, shape):
    """the update evaluated in float64 (the device's arithmetic) against long double, held below RTOL / 8"""
    c = B.build(G, name, shape)
    ld, f64 = B.ebw(c.hm, c.num, c.den, c.E), B.ebw(c.hm, c.num, c.den, c.E, ft=np.float64)
    assert np.array_equal(ld["kept"], f64["kept"])
    d = max(E.block_dist(f64[k], ld[k]) for k in ("A", "c", "mean", "inv_var", "det"))
    print(f"{name} {shape}: float64 from long double {d:.1e}")
    assert d <= RTOL / 8


# ------------------------------------------------------------- 4. the entry points

def test_the_entry_points_are_declared_bound_and_built(G):
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    lib = ctypes.CDLL(G.HIP_LIB)
    assert re.search(r"\bint ghmm_mstep_ebw\s*\(", hdr)
    assert "ghmm_mstep_ebw" in G.SYMBOLS and hasattr(lib, "ghmm_mstep_ebw")
    assert hasattr(G.Context, "mstep_ebw") and callable(load_pkg().embed.mmi_em)
    doc = load_pkg().embed.mmi_em.__doc__
    assert "log Z_u" in doc and "log P_u" in doc and "no I-smoothing" in doc
