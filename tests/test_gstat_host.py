"""Baum-Welch statistics on the grammar lattice on the CPU: gstat_cases' restatement IS the definition of
include/ghmm.h (against an enumeration of every composite path that counts the within-word transitions),
consequences (b) to (e) of the header hold on it against embed_cases' restatement and on its own sums, the float64
restatement's spread from the long-double one, and the entry point's declaration.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import embed_cases as EC
import estep_log_ref as E
import gpost_cases as PC
import grammar_cases as GC
import gstat_cases as GS
from _load import ROOT
from fullcov_support import RTOL, extended, offsets
from test_gpost_host import SMALL_GRAMMARS, narrow, small  # noqa: F401  (the fixtures)


# ------------------------------------------------------------- 1. the restatement is the definition

@extended
@pytest.mark.parametrize("delta", [0, 1])
@pytest.mark.parametrize("which", sorted(SMALL_GRAMMARS))
def test_the_restatement_sums_every_path(small, which, delta):
    """3 words of 1, 2 and 2 states (one ergodic: a transition below the diagonal stays in the word and is in
    den_a but never in num_a), utterances of 1, 2 and 6 frames, the five grammars, the band 0 and 1"""
    As, utts = small
    start, pair, fin = SMALL_GRAMMARS[which]
    finite = moved = 0
    for lb in utts:
        P, gamma, num_a, den_a, den_c = GS.enumerate_stats(As, lb, start, pair, fin, delta)
        for ft in (np.longdouble, np.float64):
            r = GS.utterance(As, lb, start, pair, fin, delta, ft)
            if P == 0:
                assert r["logP"] == -np.inf and not r["gamma"].any()
                assert not any(np.any(r[b][k]) for b in GS.COMMON for k in range(3))
                continue
            finite += ft is np.float64
            assert abs(float(r["logP"]) - np.log(P)) <= 1e-12 * max(1.0, abs(np.log(P)))
            assert np.all(np.abs(np.asarray(r["gamma"], dtype=np.float64) - gamma) <= 1e-12)
            for k in range(3):
                for got, ref in ((r["num_a"][k], num_a[k]), (r["den_a"][k], den_a[k]), (r["den_c"][k], den_c[k])):
                    assert np.all(np.abs(np.asarray(got, dtype=np.float64) - ref) <= 1e-12), (which, k)
                if len(lb) == 1:
                    assert not r["num_a"][k].any() and not r["den_a"][k].any()      # T = 1: den_c only
            moved += bool(num_a[2][0, 1] > 0) if delta else bool(num_a[2][0, 1] == 0 and num_a[2][0, 0] > 0)
            # the ergodic word's way back (1 -> 0) stays in the word: in den_a, outside every band
            assert r["num_a"][2][1, 0] == 0
    assert (finite > 0) == (which != "nothing")
    assert (moved > 0) == (which != "nothing")


def test_no_frames_and_no_path(small):
    As, utts = small
    g = SMALL_GRAMMARS["random"]
    z = GS.utterance(As, utts[-1][:0], *g, ft=np.float64)
    assert z["logP"] == 0 and not any(np.any(z[b][k]) for b in GS.COMMON for k in range(3))
    n = GS.utterance(As, utts[-1], *SMALL_GRAMMARS["nothing"], ft=np.float64)
    assert n["logP"] == -np.inf and not any(np.any(n[b][k]) for b in GS.COMMON for k in range(3))


# ------------------------------------------------------------- 2. the consequences

@pytest.fixture(scope="module")
def narrow_emission(G):
    """narrow (P = 3) with its restated log b and posteriors in long double, computed once"""
    case = GC.make(G, "narrow")
    ref = GS.estep(case.words, case.Xs, case.lens, *GC.grammar(case, "flat:-5"))
    for a in [ref["logb"]] + ref["posts"]:
        a.setflags(write=False)
    return case, ref


@extended
def test_a_chain_grammar_is_the_embedded_estep(narrow_emission):
    """(b): one-utterance corpora under the chain grammar of a transcript of pairwise distinct words: every block
    of every word's vector is the embedded E-step's times exp(log Z - log P), the reciprocal of a frame's sum of
    that call's tied gamma; loglik is equal"""
    case, em = narrow_emission
    off = offsets(case.lens)
    seen = 0
    for tr in GC.CHAINS["narrow"]:
        g = GC.chain(case.K, tr)
        for u, T in enumerate(case.lens):
            if T == 0:
                continue
            rows = slice(off[u], off[u + 1])
            Xs = [X[rows] for X in case.Xs]
            posts = [q[rows] for q in em["posts"]]
            a = GS.estep(case.words, Xs, [T], *g, logb=em["logb"][rows], posts=posts)
            e = EC.estep(case.words, Xs, [T], [tr], logb=em["logb"][rows], posts=posts)
            lp, lz = e["loglik"][0], e["logZ"][0]
            assert (a["loglik"][0] == lp) if not np.isfinite(lp) else abs(a["loglik"][0] - lp) <= 1e-15 * abs(lp)
            if not np.isfinite(lz) or not np.isfinite(lp):      # (no path into the last state: both are all zero)
                assert not any(np.any(s[k][p][b]) for s in (a["stats"], e["stats"]) for k in range(case.K)
                               for p in range(case.P) for b in E.BLOCKS[:-2])
                continue
            seen += 1
            rho = np.exp(lz - lp)
            assert abs(1 / rho - e["gamma"][0].sum()) <= 1e-15 * abs(1 / rho)
            for k in range(case.K):
                for p in range(case.P):
                    for b in E.BLOCKS[:-2]:
                        assert E.block_dist(a["stats"][k][p][b], e["stats"][k][p][b] * rho) <= 1e-12, (tr, u, k, p, b)
                    assert a["stats"][k][p]["loglik"] == a["loglik"][0] and a["stats"][k][p]["n_utt"] == 1
    assert seen >= len(GC.CHAINS["narrow"])


@extended
@pytest.mark.parametrize("name", ["narrow", "ones", "thick"])
def test_the_rows_of_num_a_and_the_frames(G, name):
    """(c): wherever the band holds every a_jj' > 0 the row of num_a sums to den_a; (d): the den_c of all words
    sum to the frames of the utterances with finite log P"""
    case = GC.make(G, name)
    lb = GC.oracle_log_b(case)
    one = case.stream0() if case.P > 1 else case
    ones = [[w[0]] for w in one.words]
    banded_rows = 0
    for which in GS.GPU_GRAMMARS[name]:
        for delta in (1, 7):
            r = GS.estep(ones, one.Xs[:1], case.lens, *GC.grammar(case, which), delta=delta, logb=lb,
                         posts=[np.ones((case.F, case.NS, ones[0][0].M)) / ones[0][0].M])
            frames = sum(int(T) for T, ll in zip(case.lens, r["loglik"]) if np.isfinite(ll))
            assert frames > 0
            total = sum(st[0]["den_c"].sum() for st in r["stats"])
            assert abs(total - frames) <= 1e-12 * frames, (which, float(total), frames)
            for k, w in enumerate(ones):
                A = np.asarray(w[0].A, dtype=np.float64)
                i, j = np.indices(A.shape)
                inside = (j >= i) & (j <= i + delta)
                st = r["stats"][k][0]
                for row in range(A.shape[0]):
                    if np.any(A[row][~inside[row]] > 0):
                        continue
                    banded_rows += 1
                    d, s = st["den_a"][row], st["num_a"][row].sum()
                    assert abs(s - d) <= 1e-13 * max(abs(d), 1e-300), (which, k, row)
                assert not np.any(st["num_a"][~inside])
    assert banded_rows > 0


@extended
@pytest.mark.parametrize("how", ["in", "out"])
def test_a_word_no_string_can_hold_has_no_sums(narrow_emission, how):
    """(e), exactly"""
    case, em = narrow_emission
    for k in range(case.K):
        g = PC.cut_off(*GC.grammar(case, "flat:-5"), k, how)
        assert list(PC.unreachable(*g)) == [k]
        for ft in (np.longdouble, np.float64):
            r = GS.estep(case.words, case.Xs, case.lens, *g, ft=ft, logb=em["logb"], posts=em["posts"])
            for p in range(case.P):
                assert not any(np.any(r["stats"][k][p][b]) for b in E.BLOCKS[:-2])
            assert np.isfinite(r["loglik"][case.lens > 8]).all()
            assert any(np.any(r["stats"][q][0]["den_c"]) for q in range(case.K) if q != k)


# ------------------------------------------------------------- 3. float64 against long double

@extended
@pytest.mark.parametrize("name", GS.SPREAD_CASES)
def test_float64_spread(G, name):
    """the figures of gstat_cases' docstring, held below RTOL / 8 (test_embed_host.test_float64_spread's protocol)"""
    case = GC.make(G, name)
    base = GS.estep(case.words, case.Xs, case.lens, *GC.grammar(case, GS.GPU_GRAMMARS[name][0]), only=())
    for which in GS.GPU_GRAMMARS[name]:
        g = GC.grammar(case, which)
        ld = GS.estep(case.words, case.Xs, case.lens, *g, logb=base["logb"], posts=base["posts"])
        f64 = GS.estep(case.words, case.Xs, case.lens, *g, ft=np.float64, logb=base["logb"], posts=base["posts"])
        lld = np.asarray(ld["loglik"], dtype=np.float64)
        fin = np.isfinite(lld)
        assert np.array_equal(lld[~fin], f64["loglik"][~fin], equal_nan=True)
        dl = max((abs(float((a - b) / b)) for a, b in zip(f64["loglik"][fin], ld["loglik"][fin]) if b != 0), default=0.0)
        db = max(E.block_dist(f64["gamma"], ld["gamma"]), GS.worst_dist(f64["stats"], ld["stats"])[0])
        print(f"{name} {which}: float64 from long double: log P {dl:.1e} | blocks {db:.1e}")
        assert dl <= 1e-12
        assert db <= RTOL / 8


# ------------------------------------------------------------- 4. the entry point

def test_the_entry_point_is_declared_bound_and_built(G):
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    lib = ctypes.CDLL(G.HIP_LIB)
    assert re.search(r"\bint ghmm_estep_grammar_streams\s*\(", hdr)
    assert "ghmm_estep_grammar_streams" in G.SYMBOLS and hasattr(lib, "ghmm_estep_grammar_streams")
    assert hasattr(G.Context, "estep_grammar_streams")
    # the header says which normaliser this is
    doc = hdr[hdr.index("Baum-Welch statistics on the grammar lattice"):hdr.index("int ghmm_estep_grammar_streams")]
    assert "NOT ghmm_estep_embed_streams' log Z_u" in doc


# ------------------------------------------------------------- 5. the MMI loop on the restatement

@extended
def test_the_restated_mmi_objective_rises(G):
    """ebw_cases.mmi_case under its seed: over the restated loop (embed_cases' numerator, this file's denominator,
    ebw_cases' update, E = 2) the objective sum log P_num - sum log P_den rises strictly at every iteration, in
    long double and in float64; test_mmi_gpu.py asks the same of the device.  One iteration more than the
    device's loop is restated, so that the last update is seen to have raised the objective as well."""
    import ebw_cases as B
    start, Xs, lens, transcripts, grammar = B.mmi_case(G)
    assert 3 not in {k for t in transcripts for k in t} and len(lens) == 20
    for ft in (np.longdouble, np.float64):
        trace, _ = B.mmi_loop(start, Xs, lens, transcripts, grammar, B.MMI_ITERS + 1, B.MMI_E, ft)
        obj = [float(a - b) for a, b in trace]
        print(ft.__name__, "objective", obj)
        assert all(np.isfinite(obj)) and all(y > x for x, y in zip(obj[:-1], obj[1:])), obj
