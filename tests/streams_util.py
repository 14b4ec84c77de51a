"""What the several-streams (param_number P > 1) tests share — a plain module, no conftest.

second_stream: the reference ships one stream of 9-d frames per utterance; the second one is derived
from it deterministically — the two-frame difference of the first five coefficients, x[t+1] - x[t-1]
(clamped at the ends).  Used by tests/golden/make_golden_streams.py (which feeds it to the REAL
reference) and by the tests (which feed the same frames to the oracle and the GPU).

synth_case, assert_frames and the diagonal stream helpers: used by tests/test_gpu_parity.py (which
keeps them under their old names; profiles/fuzz_*.py reach them through it) and by
tests/test_streams_gpu.py."""
import os

import numpy as np

import oracle_lib as O
from fullcov_support import RTOL, assert_close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMMON = ("num_a", "den_a", "den_c", "loglik", "n_utt")   # the sums every stream's vector holds


def second_stream(X, D2=5):
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    nxt = X[np.minimum(np.arange(T) + 1, T - 1), :D2]
    prv = X[np.maximum(np.arange(T) - 1, 0), :D2]
    return np.ascontiguousarray(nxt - prv)


def assert_frames(got, ref, what, rtol=RTOL):
    """Per-frame arrays: every entry against the largest of its own frame (assert_close, rows)."""
    ref = np.asarray(ref)
    got = np.asarray(got).reshape(ref.shape)
    assert_close(got, ref, rtol=rtol, what=what, rows=True)


def bits_equal(a, b):
    """bitwise equal where neither is NaN, NaN in the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def synth_case(G, N, M, D, lens, perturb=0.05, first=0, dense_A=False, seed=3):
    mean, std = G.synth_truth(N, M, D)
    X = G.synth_utterances(mean, std, lens, first_utt=first)
    hm = G.synth_start_model(mean, std, perturb)
    if dense_A:
        rng = np.random.default_rng(seed)
        A = rng.random((N, N)) + 0.05
        hm.A[:] = A / A.sum(1, keepdims=True)
    return hm, X, np.asarray(lens, dtype=np.int32)


def stream_case(G, N, shapes, lens, dense=False, perturb=0.05):
    """A P-stream case: stream p = synth_case(G, N, M_p, D_p, lens, first=17 * p) for shapes[p] =
    (M_p, D_p), with stream 0's A in every stream.  Returns (hms, Xs, lens)."""
    hms, Xs = [], []
    for p, (M, D) in enumerate(shapes):
        hm, X, la = synth_case(G, N, M, D, lens, perturb=perturb, first=17 * p, dense_A=dense)
        if p:
            hm.A[:] = hms[0].A
        hms.append(hm)
        Xs.append(X)
    return hms, Xs, la


def _stream_data(G, streams, idx):
    Xs = [G.perfil_read(os.path.join(GOLDEN, "perfil", streams["mean_list"][k])) for k in idx]
    lens = np.array([len(x) for x in Xs], dtype=np.int32)
    return [np.concatenate(Xs), np.concatenate([second_stream(x, streams["D2"]) for x in Xs])], lens


def _golden_streams(G, rec, word=""):
    m = rec["model"]
    return [G.HostModel(m["A"], s["c"], s["mean"], s["inv_var"], s["det"], word=word) for s in m["streams"]]


def utterances(Xs, lens):
    """per utterance, every stream's frames of it"""
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return [[x[o:o + t] for x in Xs] for o, t in zip(offs, lens)]


def product_of_single_emissions(G, ctx, models, corpora):
    """((b^0 * b^1) * b^2) ... by IEEE multiplication on the host, of GHMM_BUF_B as ghmm_emission of
    each stream alone leaves it in this context"""
    F, N = corpora[0].frames, models[0].N
    prod = None
    for m, c in zip(models, corpora):
        ctx.emission(m, c, True)
        b = ctx.fetch(G.BUF_B, (F, N))
        prod = b if prod is None else prod * b
    return prod


def _estep_streams_vs_oracle(G, ctx, hms, Xs, lens, tag, delta=1, bits=False, mstep=True, ref=None,
                             b_floor=0.0):
    """ghmm_estep_streams, ghmm_mstep per stream and ghmm_score_streams against the oracle: product b,
    log P and every stream's statistics at RTOL, the M-step's arrays at 1e-7, the scores at 1e-9.
      delta   the transition band, for O.estep_streams and GHMM_OPT_DELTA (restored to 1)
      bits    the bit-level properties as well: the product is the IEEE product in stream order of
              every stream's own emission; the common sums are the same bits in every vector; a
              second call repeats every vector; ghmm_score_streams equals the E-step's log P to
              1e-12; after the M-step every stream holds the same A
      mstep   False leaves the M-step comparison out (the scores are then the given models')
      ref     O.estep_streams(hms, Xs, lens, delta) where the caller has it already
      b_floor entries of the product below it are compared to it absolutely (subnormal values)
    Returns the E-step's GHMM_OPT_REFORDER_COUNT."""
    models = [ctx.model(h) for h in hms]
    corpora = [ctx.corpus(x, lens) for x in Xs]
    stats = [ctx.stats(h.N, h.M, h.D) for h in hms]
    F, N, U = int(np.sum(lens)), hms[0].N, len(lens)
    ctx.set_option(G.OPT_DELTA, delta)
    try:
        singles = product_of_single_emissions(G, ctx, models, corpora) if bits else None
        ctx.estep_streams(models, corpora, stats)
        reordered = ctx.get_option(G.OPT_REFORDER_COUNT)
        ref_stats, ref_b, ref_ll = ref if ref is not None else O.estep_streams(hms, Xs, lens, delta=delta)
        b = ctx.fetch(G.BUF_B, (F, N))
        if bits:
            assert bits_equal(b, singles), tag + " product b is not the IEEE product of the streams' own b"
        if b_floor:
            b = np.where((np.abs(ref_b) < b_floor) & (np.abs(b - ref_b) <= b_floor), ref_b, b)
        assert_frames(b, ref_b, tag + " product b")
        ll = ctx.fetch(G.BUF_LOGLIK, (U,))
        assert_close(ll, ref_ll, what=tag + " loglik")
        vs = [s.download() for s in stats]
        for p, (v, r) in enumerate(zip(vs, ref_stats)):
            got, rs = G.split_stats(v, N, hms[p].M, hms[p].D), G.split_stats(r, N, hms[p].M, hms[p].D)
            for k in rs:
                assert_close(got[k], rs[k], what=f"{tag} stream {p} stats.{k}")
            if bits:
                first = G.split_stats(vs[0], N, hms[0].M, hms[0].D)
                for k in COMMON:
                    assert bits_equal(got[k], first[k]), f"{tag} stream {p} {k} differs from stream 0's"
        if bits:
            assert_close(ctx.score_streams(models, corpora), ll, rtol=1e-12, floor=0.0,
                         what=tag + " score against the E-step's log P")
            ctx.estep_streams(models, corpora, stats)
            for p, (v, s) in enumerate(zip(vs, stats)):
                assert bits_equal(v, s.download()), f"{tag} stream {p}: a second call differs"
        if mstep:
            # M-step per stream (TF:332-346): every stream's call writes the same A
            for p in range(len(hms)):
                ctx.mstep(models[p], stats[p])
                new, ref_new = models[p].get(), O.mstep(hms[p], ref_stats[p])
                for nm, a, b in zip(("A", "c", "mean", "inv_var", "det"), new.arrays(), ref_new.arrays()):
                    assert_close(a, b, rtol=1e-7, what=f"{tag} stream {p} mstep.{nm}")
                if bits:
                    assert bits_equal(new.A, models[0].get().A), f"{tag} stream {p}: A differs from stream 0's"
        now = [m.get() for m in models]
        assert_close(ctx.score_streams(models, corpora), [O.score_streams(now, xs) for xs in utterances(Xs, lens)],
                     rtol=1e-9, what=tag + (" score after the M-step" if mstep else " score"))
    finally:
        ctx.set_option(G.OPT_DELTA, 1)
        for o in models + corpora + stats:
            o.close()
    return reordered
