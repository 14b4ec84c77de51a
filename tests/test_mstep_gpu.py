"""ghmm_mstep, the diagonal M-step on the device, on the hand-made statistics of mstep_cases.py — GPU
box only.  test_mstep_host.py shows that the cases reach their quirks.

a. Parameters.  A, c, mean, inv_var and det equal the expected model (O.mstep, A masked to the band)
   BIT FOR BIT (NaN in the same places): correctly rounded divisions, a product and a sum in index
   order, on every code path (k_mstep_mfma, k_mstep through LDS, k_mstep through global memory).
b. What the step derives and ghmm_model_get does not show — wk, logwk, log A — under
   GHMM_OPT_KERNELS = 1: every call that reads them gives the bits it gives on a twin model SET from
   the very parameters the step produced (k_prepare forms them by the same expressions).
c. The matrix-core preparation that k_mstep_mfma rebuilds (Wm, the offsets, the statistics classes,
   the flags), on the default tier: the stepped model and its twin each against the ORACLE on the
   fetched parameters at the suite's RTOL; then a second step and a third E-step.
d. Two steps in a row from uploaded vectors.  e. Refusals."""
import numpy as np
import pytest
import torch  # (before the library is loaded: one HIP runtime in the process; test a. wraps a tensor)

import mstep_cases as K
import oracle_lib as O
from fullcov_support import RTOL, assert_close, code
from streams_util import assert_frames, bits_equal

pytestmark = pytest.mark.gpu

KEYS = ("A", "c", "mean", "inv_var", "det")


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context(0)
    yield c
    c.close()


def assert_model_bits(got, ref, what):
    for key in KEYS:
        g, r = getattr(got, key), getattr(ref, key)
        if bits_equal(g, r):
            continue
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}.{key}: NaN positions differ"
        keep = ~np.isnan(r)
        bad = np.flatnonzero(g[keep].view(np.uint64) != r[keep].view(np.uint64))
        raise AssertionError(f"{what}.{key}: {bad.size} of {g.size} entries differ, first at {bad[0]}: "
                             f"{g[keep][bad[0]]!r} vs {r[keep][bad[0]]!r}")


def stepped(G, ctx, case, wrap=None):
    """the case's model after ghmm_mstep on its uploaded vector: (Model, Stats); wrap: a torch tensor on
    the device for the vector to live in (caller-owned memory)"""
    N, M, D = case.shape
    model = ctx.model(case.hm)
    stats = None
    try:
        stats = ctx.stats(N, M, D) if wrap is None else ctx.stats(N, M, D, dev_ptr=wrap.data_ptr())
        stats.upload(case.v)
        ctx.set_option(G.OPT_DELTA, case.delta)
        ctx.mstep(model, stats)
    except BaseException:
        model.close()
        if stats is not None:
            stats.close()
        raise
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
    return model, stats


# ------------------------------------------------------------------- a. parameters, bit for bit

@pytest.mark.parametrize("cid", K.ALL)
def test_parameters_bit_for_bit(G, ctx, cid):
    """twice on fresh objects, then with the vector in caller-owned device memory"""
    case, ref = K.build(G, cid), K.expected(G, cid)
    for run in ("first", "second", "wrapped"):
        buf = torch.zeros(G.stats_len(*case.shape), dtype=torch.float64, device="cuda") if run == "wrapped" else None
        if buf is not None:
            torch.cuda.synchronize()        # (the fill runs on torch's stream, the upload on the context's)
        model, stats = stepped(G, ctx, case, wrap=buf)
        try:
            got = model.get()
            if buf is not None:
                ctx.sync()
                assert bits_equal(buf.cpu().numpy(), case.v), "the step wrote into the caller's vector"
        finally:
            stats.close(); model.close()
        assert_model_bits(got, ref, f"{cid} ({run})")


@pytest.mark.parametrize("shape", sorted(set(K.PATHS) | set(K.QUIRK_SHAPES)))
def test_which_shapes_take_the_matrix_core_form(G, ctx, shape):
    """the matrix-core half of mstep_cases.PATHS from an observable: right after ghmm_model_set on a
    fresh model GHMM_K_PREPARE counts model_prepare's two timed scopes when the model takes the
    matrix-core form and one when it does not"""
    case = K.build(G, K.case_id("plain", shape))
    ctx.set_option(G.OPT_TIMING, 1)
    model = None
    try:
        ctx.kernel_times_reset()
        model = ctx.model(case.hm)
        launches = ctx.kernel_times()["prepare"][1]
    finally:
        ctx.set_option(G.OPT_TIMING, 0)
        if model is not None:
            model.close()
    assert launches == (2 if K.path_of(*shape) == "mfma" else 1), (shape, launches)


# ------------------------------------------------------------------- b. derived state, tier 1

def read_everything(G, ctx, model, corpus, stats, N, M):
    """every call that reads the model's derived state: b, post, scores, Viterbi, the E-step's vector"""
    F = corpus.frames
    ctx.emission(model, corpus, True)
    out = {"b": ctx.fetch(G.BUF_B, (F, N)), "post": ctx.fetch(G.BUF_POST, (F, N * M))}
    out["score"] = ctx.score(model, corpus)
    out["path"], out["vscore"] = ctx.viterbi(model, corpus)
    ctx.estep(model, corpus, stats)
    out["stats"] = stats.download()
    return out


@pytest.mark.parametrize("cid", K.FINITE)
def test_derived_constants_equal_a_fresh_models(G, ctx, cid):
    if not K.follow_up(G, cid):
        return      # det-subnormal when the oracle's own E-step on the stepped model is not finite
    case = K.build(G, cid)
    N, M, D = case.shape
    model, stats = stepped(G, ctx, case)
    twin = corpus = None
    try:
        twin = ctx.model(model.get())
        corpus = ctx.corpus(case.X, case.lens)
        ctx.set_option(G.OPT_KERNELS, 1)
        ctx.set_option(G.OPT_DELTA, case.delta)
        a = read_everything(G, ctx, model, corpus, stats, N, M)
        b = read_everything(G, ctx, twin, corpus, stats, N, M)
    finally:
        ctx.set_option(G.OPT_KERNELS, 0)
        ctx.set_option(G.OPT_DELTA, 1)
        for o in (twin, corpus, stats, model):
            if o is not None:
                o.close()
    assert np.array_equal(a["path"], b["path"]), f"{cid}: Viterbi paths differ"
    for key in ("b", "post", "score", "vscore", "stats"):
        assert bits_equal(a[key], b[key]), f"{cid}: {key} of the stepped model differs from its twin's"


# ------------------------------------------------------------------- c. derived state, default tier

VEC_STATS_CASES = ("var-floor-all", "narrow-one-coefficient", "nothing-updated")


def subnormal_states(b_ref, M):
    """[F][N]: where the ORACLE's own posteriors carry less than assert_frames asks.  post = term / b_i(t),
    and a term or a b_i(t) in the subnormal range is a multiple of 2^-1074: the M terms and their sum
    are each off by up to that much, the quotient by (M + 1) 2^-1074 / b_i(t) — above assert_frames'
    absolute floor of 1e-13 (the frame's largest posterior is ~1) when 0 < b_i(t) < (M + 1) 2^-1074 1e13
    ~ 4e-310.  With D = 39 and a few dozen frames a state far from the frame is there: at
    plain-13x8x39, frame 13, state 2 the oracle has b = 1.9e-315 and post = 0.0951829266; the device
    gives 0.0951829242 (2.5 x the tolerance) on BOTH tiers, for the stepped model and its twin alike.
    Those (frame, state) rows are held to [0, 1] only; b == 0 rows (post = 0, TF:1773-1778) stay in."""
    return (b_ref > 0.0) & (b_ref < (M + 1) * 2.0 ** -1074 * 1e13)


def against_oracle(G, ctx, model, corpus, stats, hm, case, what, ref):
    """b, post, the E-step's vector, scores and Viterbi paths of `model` against the oracle on hm.
    ref: the oracle's results on hm (oracle_results).  The score bound: log P is the sum of T logs of
    scale factors (plus one of alpha_T), each held to RTOL relative like every per-frame quantity, so
    it moves by at most (T + 1) RTOL absolutely."""
    N, M, D = case.shape
    F = corpus.frames
    ctx.emission(model, corpus, True)
    assert_frames(ctx.fetch(G.BUF_B, (F, N)), ref["b"], what + " b")
    post = ctx.fetch(G.BUF_POST, (F, N, M))
    vague = subnormal_states(ref["b"], M)
    assert np.all(np.isfinite(post[vague])) and np.all(post[vague] >= 0.0) and np.all(post[vague] <= 1.0 + RTOL)
    assert_frames(np.where(vague[..., None], ref["post"], post).reshape(F, -1), ref["post"].reshape(F, -1), what + " post")
    ctx.estep(model, corpus, stats)
    got, rs = G.split_stats(stats.download(), N, M, D), G.split_stats(ref["stats"], N, M, D)
    for k in rs:
        assert_close(got[k], rs[k], what=f"{what} stats.{k}")
    score = ctx.score(model, corpus)
    path, _ = ctx.viterbi(model, corpus)
    o = 0
    for u, T in enumerate(case.lens):
        assert np.isfinite(ref["score"][u]) and abs(score[u] - ref["score"][u]) <= (T + 1) * RTOL, \
            f"{what} score of utterance {u}: {score[u]!r} vs {ref['score'][u]!r}"
        assert np.array_equal(path[o:o + T], ref["paths"][u]), f"{what} Viterbi path of utterance {u}"
        o += T


def oracle_results(hm, case):
    with np.errstate(all="ignore"):
        b, post = O.emission(hm, case.X, want_post=True)
        out = {"b": b, "post": post, "stats": O.estep(hm, case.X, case.lens, delta=case.delta, dumps=False)[0],
               "score": [], "paths": []}
        o = 0
        for T in case.lens:
            out["score"].append(O.score(hm, case.X[o:o + T]))
            out["paths"].append(O.viterbi(hm, case.X[o:o + T])[0])
            o += T
    return out


def stats_against_oracle(G, got, ref, shape, what):
    got, rs = G.split_stats(got, *shape), G.split_stats(ref, *shape)
    for k in rs:
        assert_close(got[k], rs[k], what=f"{what} stats.{k}")


@pytest.mark.parametrize("cid", [k for k in K.FINITE if k in K.MFMA])
def test_rebuilt_preparation_against_the_oracle(G, ctx, cid):
    case = K.build(G, cid)
    N, M, D = case.shape
    model, stats = stepped(G, ctx, case)
    twin = corpus = None
    try:
        hm1 = model.get()
        ref1 = oracle_results(hm1, case)
        assert np.all(np.isfinite(ref1["stats"])), cid
        twin = ctx.model(hm1)
        corpus = ctx.corpus(case.X, case.lens)
        ctx.set_option(G.OPT_DELTA, case.delta)
        for m, tag in ((model, "stepped"), (twin, "twin")):
            against_oracle(G, ctx, m, corpus, stats, hm1, case, f"{cid} {tag}", ref1)
        if case.name in VEC_STATS_CASES:
            for mode in (0, 1, 2):
                ctx.set_option(G.OPT_VEC_STATS, mode)
                for m, tag in ((model, "stepped"), (twin, "twin")):
                    ctx.estep(m, corpus, stats)
                    stats_against_oracle(G, stats.download(), ref1["stats"], case.shape,
                                         f"{cid} {tag}, GHMM_OPT_VEC_STATS {mode}:")
            ctx.set_option(G.OPT_VEC_STATS, 0)
        # a second step from the device's own vector (its tile offsets are now the E-step's choice),
        # and a third E-step
        with np.errstate(all="ignore"):
            hm2 = K.mask_band(O.mstep(hm1, ref1["stats"]), ref1["stats"], case.delta)
        for m, tag in ((model, "stepped"), (twin, "twin")):
            ctx.estep(m, corpus, stats)
            ctx.mstep(m, stats)
            new = m.get()
            for key in KEYS:
                assert_close(getattr(new, key), getattr(hm2, key), rtol=1e-7, what=f"{cid} {tag} second step.{key}")
            ctx.estep(m, corpus, stats)
            # (the third E-step's model is the device's second, hm2 the oracle's: 1e-7 apart at most, so
            # the statistics are compared on the device's own parameters)
            with np.errstate(all="ignore"):
                ref3 = O.estep(new, case.X, case.lens, delta=case.delta, dumps=False)[0]
            stats_against_oracle(G, stats.download(), ref3, case.shape, f"{cid} {tag} third E-step:")
    finally:
        ctx.set_option(G.OPT_VEC_STATS, 0)
        ctx.set_option(G.OPT_DELTA, 1)
        for o in (twin, corpus, stats, model):
            if o is not None:
                o.close()


# ------------------------------------------------------------------- d. two steps in a row

@pytest.mark.parametrize("shape", K.QUIRK_SHAPES + ((2, 112, 64),))
def test_two_steps_in_a_row_from_uploaded_vectors(G, ctx, shape):
    """no E-step between: the skipped state's slot is inverted twice more, nothing is carried over"""
    cid = K.case_id("state-skipped", shape)
    case = K.build(G, cid)
    ref2 = K.mask_band(O.mstep(K.expected(G, cid), case.v), case.v, case.delta)
    model, stats = stepped(G, ctx, case)
    try:
        stats.upload(case.v)
        ctx.mstep(model, stats)
        got = model.get()
    finally:
        stats.close(); model.close()
    assert_model_bits(got, ref2, cid + " (second step)")
    assert bits_equal(got.inv_var[K.SKIPPED], 1.0 / (1.0 / case.hm.inv_var[K.SKIPPED]))


# ------------------------------------------------------------------- e. refusals

def test_refusals_leave_the_model_alone(G, ctx):
    case = K.build(G, K.case_id("plain", (5, 3, 5)))
    N, M, D = case.shape
    model = ctx.model(case.hm)
    other, full, good = ctx.stats(N, M + 1, D), ctx.stats_full(N, M, D), ctx.stats(N, M, D)
    try:
        before = model.get()
        good.upload(case.v)
        assert code(G, lambda: ctx.mstep(model, other)) == G.ERR_ARG
        assert code(G, lambda: ctx.mstep(model, full)) == G.ERR_ARG
        assert ctx.lib.ghmm_mstep(ctx.h, None, good.h) == G.ERR_ARG
        assert_model_bits(model.get(), before, "after the refusals")
        assert_model_bits(before, case.hm, "ghmm_model_get")
        ctx.mstep(model, good)      # and the model still takes a step
        assert_model_bits(model.get(), K.expected(G, K.case_id("plain", (5, 3, 5))), "the step after the refusals")
    finally:
        for o in (other, full, good, model):
            o.close()
