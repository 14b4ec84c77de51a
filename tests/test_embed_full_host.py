"""embed_full_cases on the CPU: the restatement of ghmm_estep_embed_full_streams against the single-word
full-covariance log-domain E-step (fullestep_log_ref.estep), its identities, what the cases claim, the entry
point's declaration and binding, and the float64 spreads that embed_full_cases' docstring records.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import align_cases as AC
import embed_full_cases as FC
import estep_log_ref as E
import fullestep_log_ref as FE
import fulltrain_ref as R
import logscore_cases as LC
from _load import ROOT, load_pkg
from fullcov_support import RTOL, extended, offsets


def near(a, b, rel):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
    assert np.all(np.abs(a[fin] - b[fin]) <= rel * np.abs(b[fin]))


# ------------------------------------------------------------- the restatement on one word

@extended
def test_one_word_with_one_word_transcripts_is_the_single_word_estep(G):
    """consequence (a) on the restatement: one word of one stream against fullestep_log_ref.estep.  Both run in
    long double on the same expressions; only the order of the sums over t differs (numpy's pairwise sum on
    another layout): T x 2^-64 and far below the 1e-14 asked"""
    case = FC.make(G, "mix")
    off = offsets(case.lens)
    for k in (0, 1, 3):
        hm, X = case.words[k][0], case.Xs[0]
        us = [u for u in range(case.U) if case.lens[u] and u != 2]
        fr = np.concatenate([np.arange(off[u], off[u + 1]) for u in us]).astype(int)
        lens = [int(case.lens[u]) for u in us]
        emb = FC.estep([[hm]], [X[fr]], lens, [(0,)] * len(us))
        one = FE.estep(hm, X[fr], lens)
        for b in FC.BLOCKS:
            d = E.block_dist(emb["stats"][0][0][b], one["stats"][b])
            assert d <= 1e-14, (k, b, d)
        near(emb["loglik"], one["loglik"], 1e-17)
        near(emb["logZ"], one["logZ"], 1e-17)
        assert E.block_dist(emb["gamma"], one["gamma"]) <= 1e-14
        assert np.array_equal(emb["logb"], one["logb"]), "log b of one stream is fullestep_log_ref.emission's"


@extended
def test_one_word_transcripts_give_each_word_its_sub_corpus(G):
    """consequence (b) on the restatement, two streams: word k's sums against the restatement on the vocabulary
    of that word alone and the sub-corpus of its utterances"""
    case = FC.make(G, "mix")
    spoken = [0, 3, 0, 2, 1, 2, 1, 0]
    transcripts = [(k,) if T else () for k, T in zip(spoken, case.lens)]
    emb = FC.estep(case.words, case.Xs, case.lens, transcripts)
    off = offsets(case.lens)
    for k in sorted(set(spoken)):
        us = [u for u in range(case.U) if transcripts[u] == (k,)]
        fr = np.concatenate([np.arange(off[u], off[u + 1]) for u in us]).astype(int)
        one = FC.estep([case.words[k]], [X[fr] for X in case.Xs], [case.lens[u] for u in us], [(0,)] * len(us))
        for p in range(case.P):
            for b in FC.SUMS:
                d = E.block_dist(emb["stats"][k][p][b], one["stats"][0][p][b])
                assert d <= 1e-12, (k, p, b, d)
        near(emb["loglik"][us], one["loglik"], 1e-15)


@extended
@pytest.mark.parametrize("name", ("mix", "short", "full"))
def test_rows_of_num_a_sum_to_den_a_and_frames_to_rho(G, name):
    case, ref = FC.reference(G, name)
    off = offsets(case.lens)
    seen = 0
    for k in FC.present(case):
        A = np.asarray(case.words[k][0].A)
        i, j = np.indices(A.shape)
        if np.any((A > 0) & ((j < i) | (j > i + 1))):
            continue                                        # the band does not hold every a_jj' > 0
        st = ref["stats"][k][0]
        assert E.block_dist(st["num_a"].sum(1), st["den_a"]) <= 1e-12, (name, k)
        seen += bool(np.any(st["den_a"]))
    assert seen >= 2
    for u in range(case.U):
        rows = ref["gamma"][off[u]:off[u + 1]]
        if case.lens[u] == 0 or not np.isfinite(ref["logZ"][u]):
            assert not rows.any()
            continue
        rho = np.exp(ref["loglik"][u] - ref["logZ"][u])
        assert np.all(np.abs(rows.sum(1) - rho) <= 1e-12 * rho + 1e-300), (name, u)


# ------------------------------------------------------------- the cases hold what is leaned on

def test_the_cases_hold_what_their_descriptions_claim(G):
    mix, short, deep, full = (FC.make(G, n) for n in ("mix", "short", "deep", "full"))
    # full
    assert full.NS == 30 and full.K == 3 and full.transcripts == AC.make(G, "full").transcripts
    # mix: the shapes, the words, the utterances
    assert mix.P == 2 and [(h.M, h.D) for h in mix.words[0]] == [(2, 5), (3, 4)]
    assert mix.Ns == [5, 16, 9, 1, 4]
    A = mix.words[1][0].A
    i, j = np.indices(A.shape)
    assert np.any((A > 0) & ((j < i) | (j > i + 1))), "word 1 is not ergodic"
    assert all(np.array_equal(w[0].A, w[1].A) for w in mix.words)
    ts, lens = mix.transcripts, [int(T) for T in mix.lens]
    assert (lens[0], ts[0]) == (0, ()) and (lens[1], ts[1]) == (1, (3,))
    assert any(len(t) == 1 and T == 1 for t, T in zip(ts, lens)) and any(len(t) == 1 and T == 2 for t, T in zip(ts, lens))
    assert (0, 0) in ts and any(1 in t[1:-1] for t in ts) and any(len(t) > 2 and t[0] == 3 and t[-1] == 3 for t in ts)
    assert FC.present(mix) == [0, 1, 2, 3], "word 4 is absent, the others are spoken"
    # the far frame: inside an utterance, its linear densities are 0 in float64 in every stream and word, its
    # log b finite
    off = offsets(lens)
    u = int(np.searchsorted(off, LC.FAR_FRAME, side="right") - 1)
    assert lens[u] > 1 and off[u] <= LC.FAR_FRAME < off[u + 1]
    with np.errstate(all="ignore"):
        for w in mix.words:
            for p, h in enumerate(w):
                gm = R._densities(h, mix.Xs[p][LC.FAR_FRAME:LC.FAR_FRAME + 1], np.float64)
                assert not gm.any(), "the far frame does not underflow"
                near_by = R._densities(h, mix.Xs[p][LC.FAR_FRAME + 1:LC.FAR_FRAME + 2], np.float64)
                assert np.all(np.isfinite(near_by))
        lb, _ = FC.emission(mix.words, mix.Xs, np.float64)
    assert np.all(np.isfinite(lb)), "log b is not finite"
    # short: the same corpus, log Z = -inf where stated and only there
    assert all(np.array_equal(a, b) for a, b in zip(short.Xs, mix.Xs)) and np.array_equal(short.lens, mix.lens)
    ref = FC.estep(short.words, short.Xs, short.lens, short.transcripts, ft=np.float64)
    no_z = [u for u in range(short.U) if short.lens[u] and ref["logZ"][u] == -np.inf]
    assert tuple(no_z) == FC.SHORT_NO_Z
    for u in no_z:
        assert AC.states_of(short, short.transcripts[u]) > short.lens[u] or len(short.transcripts[u]) > 1
        assert not ref["gamma"][off[u]:off[u + 1]].any()
    assert any(np.isfinite(ref["loglik"][u]) and short.lens[u] for u in range(short.U))
    # deep
    assert deep.K == 32 and set(deep.Ns) == {64} and deep.NS == 2048 and deep.P == 1
    assert [(h.M, h.D) for h in deep.words[0]] == [(1, 3)]
    for w in deep.words:
        i, j = np.indices(w[0].A.shape)
        assert not np.any((w[0].A > 0) & ((j < i) | (j > i + 1))), "a word of deep is not banded"
    assert deep.transcripts == [(3, 5, 17), (9,)] and [int(T) for T in deep.lens] == [190, 70]
    assert max(AC.states_of(deep, t) for t in deep.transcripts) == 192
    assert FC.deep_blocks(deep.NS) * FC.RD_THREADS > 2 ** 32
    # deep on 190 frames cannot reach the last of 192 banded states; deep200 can, and is the same vocabulary
    deep200 = FC.make(G, "deep200")
    assert deep200.transcripts == deep.transcripts and [int(T) for T in deep200.lens] == [200, 70]
    assert all(np.array_equal(a[0].mean, b[0].mean) for a, b in zip(deep.words, deep200.words))
    lp = {n: FC.estep(c.words, c.Xs, c.lens, c.transcripts, ft=np.float64) for n, c in (("deep", deep), ("deep200", deep200))}
    assert lp["deep"]["loglik"][0] == -np.inf and np.isfinite(lp["deep"]["logZ"][0]) and np.isfinite(lp["deep"]["loglik"][1])
    assert not lp["deep"]["gamma"][:190].any() and lp["deep"]["gamma"][190:].any()
    assert np.all(np.isfinite(lp["deep200"]["loglik"]))
    assert all(lp["deep200"]["stats"][k][0]["den_c"].all() for k in (3, 5, 9, 17))
    assert all(FC.deep_blocks(c.NS) * FC.RD_THREADS < 2 ** 32 for c in (mix, full))
    # holes: the transcripts of align_cases
    holes = FC.make(G, "holes")
    assert all(len(t) == holes.U for t, _ in AC.HOLES.values())
    # point
    start, Xs, plens, ptr = FC.point_case(G)
    assert len(start) == 5 and FC.present(None, ptr) == [0, 1, 2, 3] and len(Xs) == 2


def test_the_entry_point_is_declared_bound_and_built(G):
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    assert re.search(r"\bint ghmm_estep_embed_full_streams\s*\(", hdr)
    assert "such an entry point can follow" not in hdr
    assert "ghmm_estep_embed_full_streams" in G.SYMBOLS
    if os.path.exists(G.HIP_LIB):
        assert hasattr(ctypes.CDLL(G.HIP_LIB), "ghmm_estep_embed_full_streams")
    assert hasattr(G.Context, "estep_embed_full_streams")
    assert callable(load_pkg().embed.embedded_em)


# ------------------------------------------------------------- float64 against long double

def spread(G, name, delta=1):
    case, ld = FC.reference(G, name, delta)
    _, f64 = FC.reference(G, name, delta, np.float64)
    fin = np.isfinite(np.asarray(ld["loglik"], dtype=np.float64))
    assert np.array_equal(fin, np.isfinite(f64["loglik"]))
    dl = max((abs(float((a - b) / b)) for x in ("loglik", "logZ") for a, b in zip(f64[x], ld[x])
              if np.isfinite(float(b)) and b != 0), default=0.0)
    ds, where = FC.worst_dist(f64, ld, case.lens)
    return dl, ds, where


@extended
@pytest.mark.parametrize("name", FC.NAMES)
def test_float64_spread(G, name):
    """the figures of embed_full_cases' docstring"""
    dl, ds, where = spread(G, name)
    print(f"{name}: float64 from long double: log P, log Z {dl:.1e} | blocks {ds:.1e} (worst {where})")
    assert dl <= 1e-12
    assert ds <= RTOL / 8


@extended
@pytest.mark.parametrize("delta", FC.DELTAS)
def test_float64_spread_under_other_deltas(G, delta):
    dl, ds, where = spread(G, "mix", delta)
    print(f"mix delta {delta}: float64 from long double: log P, log Z {dl:.1e} | blocks {ds:.1e} (worst {where})")
    assert dl <= 1e-12
    assert ds <= RTOL / 8
    _, ref = FC.reference(G, "mix", delta)
    for k in FC.present(FC.make(G, "mix")):
        na = ref["stats"][k][0]["num_a"]
        i, j = np.indices(na.shape)
        assert not np.any(na[(j < i) | (j > i + delta)]), "num_a outside the band"
    if delta >= 2:
        na = ref["stats"][1][0]["num_a"]
        assert np.any(na[np.indices(na.shape)[1] >= np.indices(na.shape)[0] + 2]), "the ergodic word's band is empty"


@extended
def test_four_em_iterations(G):
    """EM_POINT_F64 of embed_full_cases: the float64 trajectory of the point case against the long-double one;
    the trace is finite and rising"""
    start, Xs, lens, transcripts = FC.point_case(G)
    held = FC.present(None, transcripts)
    f64 = FC.em_trajectory(start, Xs, lens, transcripts, ft=np.float64)
    ld = FC.em_trajectory(start, Xs, lens, transcripts, ft=np.longdouble)
    e_tr, e_model = FC.trajectory_dist(f64, ld, held)
    print(f"point: trace {f64[0]}, float64 from long double: trace {e_tr:.1e}, models {e_model:.1e}")
    assert np.all(np.isfinite(f64[0])) and np.all(np.diff(f64[0]) > 0)
    assert max(e_tr, e_model) <= FC.EM_POINT_F64, "EM_POINT_F64 is below what is measured here"
