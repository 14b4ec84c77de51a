"""The word posteriors under a word-pair grammar on the CPU: gpost_cases' restatement IS the definition of
include/ghmm.h (against an enumeration of every composite path with its word boundaries), consequences (a)
to (e) of the header hold on it against logscore_ref's, embed_cases' and grammar_cases' restatements,
word_confidence on hand-made arrays, the float64 restatement's spread from the long-double one, and the
entry points' declarations.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import connect_cases as CC
import embed_cases as EC
import estep_log_ref as E
import gpost_cases as PC
import grammar_cases as GC
import logscore_ref as R
from _load import PKG_DIR, ROOT
from fullcov_support import RTOL, extended, offsets

BIN = {False: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-fs"),
       True: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-full-fs")}


@pytest.fixture(scope="module")
def narrow(G):
    case = GC.make(G, "narrow")
    return case, GC.oracle_log_b(case)


@pytest.fixture(scope="module")
def small(narrow):
    """a 3-word vocabulary of 1, 2 and 2 states (one word ergodic) on five columns of narrow's oracle log b,
    narrow's first utterances of at least one frame cut to at most 6 frames"""
    case, lb = narrow
    As = [np.ones((1, 1)), np.array([[0.6, 0.4], [0.0, 1.0]]), np.array([[0.5, 0.5], [0.3, 0.7]])]
    off = offsets(case.lens)
    utts = [lb[off[u]:off[u] + min(int(T), 6), 3:8] for u, T in enumerate(case.lens) if T][:6]
    assert sorted({len(x) for x in utts}) == [1, 2, 6]
    return As, utts


SMALL_GRAMMARS = {"flat": GC.flat(3, -1.5), "random": GC.random(3, 5), "norepeat": GC.norepeat(3),
                  "chain": GC.chain(3, (1, 0, 2)), "nothing": (np.zeros(3), np.full((3, 3), -np.inf), np.full(3, -np.inf))}


# ------------------------------------------------------------- 1. the restatement is the definition

@extended
@pytest.mark.parametrize("which", sorted(SMALL_GRAMMARS))
def test_the_restatement_sums_every_path(small, which):
    As, utts = small
    start, pair, fin = SMALL_GRAMMARS[which]
    finite = 0
    for lb in utts:
        P, gamma, occ, ent = PC.enumerate_paths(As, lb, start, pair, fin)
        for ft in (np.longdouble, np.float64):
            r = PC.lattice(As, lb, start, pair, fin, ft)
            if P == 0:
                assert r["logP"] == -np.inf
                assert not r["gamma"].any() and not r["occ"].any() and not r["ent"].any()
                continue
            finite += ft is np.float64
            assert abs(float(r["logP"]) - np.log(P)) <= 1e-12 * max(1.0, abs(np.log(P)))
            for got, ref in ((r["gamma"], gamma), (r["occ"], occ), (r["ent"], ent)):
                assert np.all(np.abs(np.asarray(got, dtype=np.float64) - ref) <= 1e-12), which
    assert (finite > 0) == (which != "nothing")


def test_none_is_all_zero(small):
    As, utts = small
    _, pair, _ = SMALL_GRAMMARS["random"]
    a = PC.lattice(As, utts[-1], None, pair, None, np.float64)
    b = PC.lattice(As, utts[-1], np.zeros(3), pair, np.zeros(3), np.float64)
    assert all(np.array_equal(a[k], b[k]) for k in ("logP", "gamma", "occ", "ent"))
    z = PC.lattice(As, utts[-1][:0], None, pair, None, np.float64)
    assert z["logP"] == 0 and z["gamma"].shape == (0, 5) and z["occ"].shape == (0, 3)


# ------------------------------------------------------------- 2. the consequences

@extended
def test_a_one_word_grammar_is_logscore(narrow):
    """(a): K = 1, pair = -inf, start = fin = 0"""
    case, lb = narrow
    off = offsets(case.lens)
    for k in range(case.K):
        A = np.asarray(case.words[k][0].A, dtype=np.float64)
        cols = slice(case.bo[k], case.bo[k + 1])
        for u in range(case.U):
            x = lb[off[u]:off[u + 1], cols]
            got = PC.lattice([A], x, np.zeros(1), np.full((1, 1), -np.inf), np.zeros(1))["logP"]
            ref = R.lattice(A, x, 1)
            assert (got == ref) if not np.isfinite(ref) else abs(got - ref) <= 1e-15 * abs(ref), (k, u)


@extended
@pytest.mark.parametrize("name", ["narrow", "many"])
def test_a_chain_grammar_is_the_embedded_lattice(G, name):
    """(b): log P is the embedded lattice's, and its gamma is this gamma times exp(log P - log Z)"""
    case = GC.make(G, name)
    lb = GC.oracle_log_b(case)
    As = [np.asarray(w[0].A, dtype=np.float64) for w in case.words]
    off = offsets(case.lens)
    finite = 0
    for tr in GC.CHAINS[name]:
        g = GC.chain(case.K, tr)
        for u, T in enumerate(case.lens):
            if T == 0:
                continue
            x = lb[off[u]:off[u + 1]]
            r = PC.lattice(As, x, *g)
            e = EC.lattice(As, case.bo, x, tr)
            if not np.isfinite(e["logP"]):
                assert r["logP"] == e["logP"] and not r["gamma"].any()
                continue
            finite += 1
            assert abs(r["logP"] - e["logP"]) <= 1e-15 * abs(e["logP"])
            tied, _ = EC.tied(e, tr, case.Ns, case.bo, case.NS, np.longdouble)
            want = r["gamma"] * np.exp(r["logP"] - e["logZ"])
            assert E.block_dist(want, tied) <= 1e-12, (name, tr, u)
    assert finite >= len(GC.CHAINS[name])


@extended
@pytest.mark.parametrize("name", ["narrow", "ones", "many"])
def test_the_sum_holds_the_best_path_and_the_rows_sum_to_one(G, name):
    """(c) and (d)"""
    case = GC.make(G, name)
    lb = GC.oracle_log_b(case)
    live = 0
    for which in ("random", "norepeat", "flat:-5"):
        g = GC.grammar(case, which)
        ref = PC.post(case, lb, *g)
        score = GC.decode(case, lb, *g)[3]
        off = offsets(case.lens)
        for u, T in enumerate(case.lens):
            ll = ref["loglik"][u]
            assert ll >= score[u] - 1e-12 * abs(score[u]) if np.isfinite(score[u]) else True
            assert np.isfinite(ll) == np.isfinite(score[u])
            if T == 0 or not np.isfinite(ll):
                continue
            live += 1
            occ, ent = ref["occ"][off[u]:off[u + 1]], ref["ent"][off[u]:off[u + 1]]
            assert np.all(np.abs(occ.sum(1) - 1) <= 1e-13) and abs(ent[0].sum() - 1) <= 1e-13
            assert np.all(ent <= occ * (1 + 1e-12) + 1e-300) and ent.sum() >= 1 - 1e-13
    assert live >= 6


@extended
@pytest.mark.parametrize("how", ["in", "out"])
def test_a_word_no_string_can_hold_has_no_posterior(narrow, how):
    """(e), exactly"""
    case, lb = narrow
    for k in range(case.K):
        g = PC.cut_off(*GC.grammar(case, "flat:-5"), k, how)
        assert list(PC.unreachable(*g)) == [k]
        for ft in (np.longdouble, np.float64):
            ref = PC.post(case, lb, *g, ft=ft)
            assert np.all(ref["occ"][:, k] == 0) and np.all(ref["ent"][:, k] == 0)
            assert np.all(ref["gamma"][:, case.bo[k]:case.bo[k + 1]] == 0)
            assert np.isfinite(ref["loglik"][case.lens > 8]).all()


# ------------------------------------------------------------- 3. word_confidence

def test_word_confidence(G):
    occ = np.array([[1.0, 0.0], [0.5, 0.5], [0.25, 0.75], [0.0, 1.0], [0.125, 0.875]])
    word = np.array([0, 0, 1, 1, 1], dtype=np.int32)
    begin = np.array([1, 0, 1, 1, 1], dtype=np.int32)
    lens = [3, 0, 2]
    seg = G.word_segments(word, begin, lens)
    assert seg == [[(0, 0, 1), (1, 2, 2)], [], [(1, 0, 0), (1, 1, 1)]]
    assert G.word_confidence(seg, occ, lens) == [[(0, 0, 1, 0.75), (1, 2, 2, 0.75)], [], [(1, 0, 0, 1.0), (1, 1, 1, 0.875)]]
    with pytest.raises(ValueError):
        G.word_confidence(seg[:2], occ, lens)
    with pytest.raises(ValueError):
        G.word_confidence([[(0, 0, 3)], [], []], occ, lens)


# ------------------------------------------------------------- 4. float64 against long double

@extended
@pytest.mark.parametrize("name", PC.SPREAD_CASES)
def test_float64_spread(G, name):
    """the figures of gpost_cases' docstring, held below RTOL / 8 (test_embed_host.test_float64_spread's protocol)"""
    case = GC.make(G, name)
    lb = GC.oracle_log_b(case)
    for which in PC.GPU_GRAMMARS[name]:
        g = GC.grammar(case, which)
        ld, f64 = PC.post(case, lb, *g), PC.post(case, lb, *g, ft=np.float64)
        lld = np.asarray(ld["loglik"], dtype=np.float64)
        fin = np.isfinite(lld)
        assert np.array_equal(lld[~fin], f64["loglik"][~fin], equal_nan=True)
        dl = max((abs(float((a - b) / b)) for a, b in zip(f64["loglik"][fin], ld["loglik"][fin]) if b != 0), default=0.0)
        db = max(E.block_dist(f64[x], ld[x]) for x in ("gamma", "occ", "ent"))
        print(f"{name} {which}: float64 from long double: log P {dl:.1e} | blocks {db:.1e}")
        assert dl <= 1e-12
        assert db <= RTOL / 8


# ------------------------------------------------------------- 5. the entry points and the command line

def test_the_entry_points_are_declared_bound_and_built(G):
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    lib = ctypes.CDLL(G.HIP_LIB)
    for name in ("ghmm_grammar_post_streams", "ghmm_grammar_post_full_streams"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr)
        assert name in G.SYMBOLS and hasattr(lib, name)
    assert hasattr(G.Context, "grammar_post_streams") and hasattr(G.Context, "grammar_post_full_streams")
    assert callable(G.word_confidence)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("env", [{"GHMM_CONFIDENCE": "1"}, {"GHMM_CONFIDENCE": "1", "GHMM_ALIGN": "1"},
                                 {"GHMM_CONFIDENCE": "1", "GHMM_ALIGN": "1", "GHMM_CONNECTED": "1"}])
def test_confidence_takes_the_connected_decoder(tmp_path, full, env):
    """GHMM_CONFIDENCE without GHMM_CONNECTED=1, or with GHMM_ALIGN=1: a message and exit 1 before any file is
    read (the files named here do not exist) and before a context is created"""
    import subprocess
    e = {k: v for k, v in os.environ.items()
         if k not in ("GHMM_CONNECTED", "GHMM_WORD_PENALTY", "GHMM_GRAMMAR", "GHMM_ALIGN", "GHMM_CONFIDENCE")}
    e.update(env)
    p = subprocess.run([BIN[full], "1", "models.txt", "1", "list.txt", "words.txt", "report.txt"], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert p.returncode == 1 and "GHMM_CONFIDENCE takes GHMM_CONNECTED=1" in p.stdout.decode(errors="replace")
    assert not os.path.exists(os.path.join(str(tmp_path), "report.txt"))
