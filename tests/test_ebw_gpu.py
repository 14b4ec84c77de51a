"""The extended Baum-Welch update on the GPU: ghmm_mstep_ebw (k_mstep_ebw, then the model's preparation) through
the C ABI by ghmm.py — GPU box only.  The cases and the long-double restatement are ebw_cases'; test_ebw_host.py
shows on the CPU that the cases reach what they are named for and that the update evaluated in float64 stays
within RTOL / 8 of the long-double one.  The kernel has one path for every shape: (3, 2, 5) and (10, 8, 39) take
the matrix-core preparation, (2, 97, 13) takes none (model_prepare returns early), and (2, 130, 5) has more
Gaussians per state than the block has threads (128), so a thread takes a second trip of the kernel's loops."""
import numpy as np
import pytest

import ebw_cases as B
import estep_log_ref as E
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import RTOL, code, extended
from test_logscore_gpu import TIERS, same, tier_of

pytestmark = pytest.mark.gpu


def run(G, ctx, case, E_=None, num=None, den=None):
    """the update on a fresh device model: (the new HostModel, the model handle's owner closes it)"""
    N, M, D = case.shape
    m, sn, sd = ctx.model(case.hm), ctx.stats(N, M, D), ctx.stats(N, M, D)
    try:
        sn.upload(case.num if num is None else num)
        sd.upload(case.den if den is None else den)
        ctx.mstep_ebw(m, sn, sd, case.E if E_ is None else E_)
        return m.get()
    finally:
        for o in (m, sn, sd):
            o.close()


@extended
@pytest.mark.parametrize("shape", B.SHAPES)
@pytest.mark.parametrize("name", B.EDITS)
def test_against_the_long_double_restatement(G, ctx, name, shape):
    case = B.build(G, name, shape)
    new = run(G, ctx, case)
    ref = B.ebw(case.hm, case.num, case.den, case.E)
    worst = 0.0
    for k, got in zip(("A", "c", "mean", "inv_var", "det"), new.arrays()):
        d = E.block_dist(got, ref[k])
        assert d <= RTOL, (name, shape, k, d)
        worst = max(worst, d)
    print(f"{name} {shape}: worst distance from the long-double restatement {worst:.2e}")
    # a variance is at least the floor and finite, whatever dv was
    assert np.all(np.isfinite(new.inv_var)) and np.all(1.0 / new.inv_var >= B.FLOOR * (1 - 1e-15))
    if name == "equal":
        assert same(new.mean, case.hm.mean), "equal vectors moved a mean"
    if name == "no-stats":
        g = B.NO_STATS
        assert same(new.mean[g], case.hm.mean[g]) and same(new.inv_var[g], case.hm.inv_var[g])
        assert new.det[g] == case.hm.det[g]


@pytest.mark.parametrize("shape", B.SHAPES)
@pytest.mark.parametrize("name", ["plain", "row-kept", "state-skipped", "no-stats"])
def test_weights_and_transitions_are_the_m_steps_bits(G, ctx, name, shape):
    """A and c (and through them log A: an emission-free Viterbi would read it; here the next check reads it) are
    ghmm_mstep(num)'s on a copy, bit for bit"""
    case = B.build(G, name, shape)
    N, M, D = shape
    new = run(G, ctx, case)
    m, s = ctx.model(case.hm), ctx.stats(N, M, D)
    try:
        s.upload(case.num)
        ctx.mstep(m, s)
        ml = m.get()
    finally:
        m.close()
        s.close()
    assert same(new.A, ml.A) and same(new.c, ml.c)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("shape", B.SHAPES)
def test_the_next_emission_sees_the_new_model(G, ctx, shape, tier):
    """an emission, the log-domain one and a Viterbi pass after the update match those after ghmm_model_set of the
    downloaded model, on both kernel tiers: the derived constants (wk, logwk, log A) and the matrix-core form
    were prepared"""
    from streams_util import synth_case
    case = B.build(G, "plain", shape)
    N, M, D = shape
    _, X, lens = synth_case(G, N, M, D, [37, 20, max(12, N)])
    m, sn, sd, corpus = ctx.model(case.hm), ctx.stats(N, M, D), ctx.stats(N, M, D), ctx.corpus(X, lens)
    other = None
    F = int(np.sum(lens))
    try:
        with tier_of(G, ctx, tier):
            ctx.emission(m, corpus)          # (the old model's preparation has been used once)
            sn.upload(case.num)
            sd.upload(case.den)
            ctx.mstep_ebw(m, sn, sd, case.E)
            ctx.emission(m, corpus)
            b1 = ctx.fetch(G.BUF_B, (F, N))
            path1, score1 = ctx.viterbi(m, corpus)
            ll1 = ctx.logscore(m, corpus)
            other = ctx.model(m.get())
            ctx.emission(other, corpus)
            b2 = ctx.fetch(G.BUF_B, (F, N))
            path2, score2 = ctx.viterbi(other, corpus)
            ll2 = ctx.logscore(other, corpus)
    finally:
        for o in (m, sn, sd, corpus, other):
            if o is not None:
                o.close()
    assert np.all(np.isfinite(b1)) and np.any(b1 > 0)
    assert same(b1, b2) and same(score1, score2) and np.array_equal(path1, path2) and same(ll1, ll2)


def test_refusals(G, ctx):
    case = B.build(G, "plain", B.SHAPES[0])
    N, M, D = case.shape
    m, sn, sd = ctx.model(case.hm), ctx.stats(N, M, D), ctx.stats(N, M, D)
    other, full = ctx.stats(N, M + 1, D), ctx.stats_full(N, M, D)
    try:
        sn.upload(case.num)
        sd.upload(case.den)
        before = m.get()
        lib, arg = ctx.lib, G.ERR_ARG
        assert lib.ghmm_mstep_ebw(ctx.h, None, sn.h, sd.h, 2.0) == arg
        assert lib.ghmm_mstep_ebw(ctx.h, m.h, None, sd.h, 2.0) == arg
        assert lib.ghmm_mstep_ebw(ctx.h, m.h, sn.h, None, 2.0) == arg
        for bad in (other, full):
            assert code(G, lambda: ctx.mstep_ebw(m, bad, sd)) == arg
            assert code(G, lambda: ctx.mstep_ebw(m, sn, bad)) == arg
        for bad in (-1e-9, np.nan, np.inf, -np.inf):
            assert code(G, lambda: ctx.mstep_ebw(m, sn, sd, bad)) == arg, bad
        after = m.get()
        assert all(same(a, b) for a, b in zip(before.arrays(), after.arrays()))
        ctx.mstep_ebw(m, sn, sd, 0.0)        # E = 0 is allowed
        assert all(np.all(np.isfinite(a)) for a in m.get().arrays())
    finally:
        for o in (m, sn, sd, other, full):
            o.close()
