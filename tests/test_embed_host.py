"""The embedded Baum-Welch E-step without a GPU: embed_cases' restatement is the definition of include/ghmm.h
(against an enumeration of every path through the composite model), it is estep_log_ref's E-step on one-word
transcripts, the identities the header states hold on it, its float64 form stays close to the long-double
one, the entry point is declared, bound and built, the cases hold what test_embed_gpu.py leans on, and a
coverage table of what the host works out of every case (threads, PASSES, the table loop, the last word's size,
the passes that own a dense word) shows which branches of the two kernels the cases reach."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import align_cases as AC
import embed_cases as EC
import estep_log_ref as E
import logscore_cases as LC
from _load import ROOT, load_pkg
from fullcov_support import RTOL, extended, have_extended, offsets

FT = np.longdouble if have_extended() else np.float64


# ------------------------------------------------------------- the definition, path by path

TINY_A = [np.array([[0.6, 0.4], [0.0, 1.0]]), np.array([[0.5, 0.5], [0.3, 0.7]])]      # banded, ergodic
TINY_COLS = [0, 2]
TINY = [((0, 1), 6), ((0, 0), 5), ((1,), 4), ((1, 0, 1), 6), ((0, 1), 2), ((0, 1), 1)]


def enumerate_paths(As, cols, logb, transcript, delta, ft):
    """every path s_0 .. s_{T-1} through the transcript's composite states from state 0, weighted by the
    product of its b and a (the exit into the next instance weighs 1): P, Z, and gamma, xi and stay as sums
    over the paths that END in the last state of the last instance, over Z"""
    T = len(logb)
    inst = [(i, j) for i, k in enumerate(transcript) for j in range(As[k].shape[0])]
    S, L = len(inst), len(transcript)
    b = np.exp(np.asarray(logb).astype(ft))
    col = [cols[transcript[i]] + j for i, j in inst]
    Nm = max(As[k].shape[0] for k in transcript)

    def step(s, s2):
        (i, j), (i2, j2) = inst[s], inst[s2]
        if i2 == i:
            return ft(As[transcript[i]][j, j2])
        if i2 == i + 1 and j2 == 0 and j == As[transcript[i]].shape[0] - 1:
            return ft(1)
        return ft(0)

    P = Z = ft(0)
    gamma, stay = np.zeros((T, L, Nm), ft), np.zeros((T, L, Nm), ft)
    xi = np.zeros((T, L, Nm, Nm), ft)
    for tail in itertools.product(range(S), repeat=T - 1):
        path = (0,) + tail
        wgt = b[0, col[0]]
        for t in range(1, T):
            wgt = wgt * step(path[t - 1], path[t]) * b[t, col[path[t]]]
        if wgt == 0:
            continue
        if inst[path[-1]][0] == L - 1:
            Z += wgt
        if path[-1] != S - 1:
            continue
        P += wgt
        for t, s in enumerate(path):
            i, j = inst[s]
            gamma[t, i, j] += wgt
            if t < T - 1 and inst[path[t + 1]][0] == i:
                j2 = inst[path[t + 1]][1]
                stay[t, i, j] += wgt
                if j <= j2 <= j + delta:
                    xi[t, i, j, j2] += wgt
    with np.errstate(all="ignore"):
        return {"logP": np.log(P), "logZ": np.log(Z), "gamma": gamma / Z, "stay": stay / Z, "xi": xi / Z}


def near(got, ref, tol=1e-12):
    got, ref = np.asarray(got, dtype=FT), np.asarray(ref, dtype=FT)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])
    assert np.all(np.abs(got[fin] - ref[fin]) <= tol * np.abs(ref[fin])), float(np.abs(got[fin] - ref[fin]).max())


@pytest.mark.parametrize("delta", (0, 1))
@pytest.mark.parametrize("transcript,T", TINY)
def test_the_restatement_is_the_definition_path_by_path(transcript, T, delta):
    rng = np.random.default_rng(40 + T + len(transcript))
    logb = rng.normal(-3.0, 2.0, (T, 4))
    r = EC.lattice(TINY_A, TINY_COLS, logb, transcript, delta, FT)
    e = enumerate_paths(TINY_A, TINY_COLS, logb, transcript, delta, FT)
    near(r["logP"], e["logP"])
    near(r["logZ"], e["logZ"])
    if not np.isfinite(e["logZ"]):          # too short for its transcript: nothing but log P
        assert r["logP"] == -np.inf and not r["gamma"].any() and not r["xi"].any() and not r["stay"].any()
        return
    for what in ("gamma", "xi", "stay"):
        near(r[what], e[what])
    # the tied sums are the sums of these over the instances of a word
    Ns = [2, 2]
    g, per = EC.tied(r, transcript, Ns, TINY_COLS, 4, FT)
    for k in set(transcript):
        ii = [i for i, kk in enumerate(transcript) if kk == k]
        near(per[k][0], sum(e["xi"][:, i].sum(0) for i in ii))
        near(per[k][1], sum(e["stay"][:, i].sum(0) for i in ii))
        near(per[k][2], sum(e["gamma"][:, i].sum(0) for i in ii))
        near(g[:, TINY_COLS[k]:TINY_COLS[k] + 2], sum(e["gamma"][:, i] for i in ii))


def test_the_exit_has_no_xi_and_stay_is_what_remains():
    """in the last state of an instance before the last, gamma - stay is the mass that leaves the word"""
    rng = np.random.default_rng(7)
    logb = rng.normal(-3.0, 2.0, (6, 4))
    r = EC.lattice(TINY_A, TINY_COLS, logb, (0, 1), 1, FT)
    left = (r["gamma"] - r["stay"])[:5]
    assert np.all(np.abs(left[:, 0, 0]) < 1e-15) and np.all(np.abs(left[:, 1, :]) < 1e-15)
    assert left[:, 0, 1].sum() > 0.5        # every path leaves word 0 once, up to rho
    near(r["xi"][:, 0].sum(-1), r["stay"][:, 0], 1e-12)      # word 0 is banded: the band holds every a_jj' > 0


# ------------------------------------------------------------- identities on the cases

@extended
def test_one_word_transcripts_give_the_single_word_estep(G):
    """consequence (b) on the restatement: word k's sums are estep_log_ref.estep's on its utterances"""
    case = EC.make(G, "narrow")
    spoken = [0, 1, 2, 0, 1, 2, 0, 1, 2]
    transcripts = [(k,) if T else () for k, T in zip(spoken, case.lens)]
    emb = EC.estep(case.words, case.Xs, case.lens, transcripts)
    off = offsets(case.lens)
    for k in range(case.K):
        us = [u for u in range(case.U) if transcripts[u] == (k,)]
        fr = np.concatenate([np.arange(off[u], off[u + 1]) for u in us]).astype(int)
        one = E.estep(case.words[k], [X[fr] for X in case.Xs], [case.lens[u] for u in us])
        for p in range(case.P):
            for b in E.BLOCKS[:-2]:
                d = E.block_dist(emb["stats"][k][p][b], one["stats"][p][b])
                assert d <= 1e-12, (k, p, b, d)
        near(emb["loglik"][us], one["loglik"], 1e-15)
        near(emb["logZ"][us], one["logZ"], 1e-15)


@extended
@pytest.mark.parametrize("name", ("many", "short", "narrow"))
def test_rows_of_num_a_sum_to_den_a_and_frames_to_rho(G, name):
    case, ref = EC.reference(G, name)
    off = offsets(case.lens)
    for k in EC.present(case):
        A = np.asarray(case.words[k][0].A)
        i, j = np.indices(A.shape)
        if np.any((A > 0) & ((j < i) | (j > i + 1))):
            continue                                        # the band does not hold every a_jj' > 0
        st = ref["stats"][k][0]
        assert E.block_dist(st["num_a"].sum(1), st["den_a"]) <= 1e-12, (name, k)
    for u, r in enumerate(ref["utt"]):
        if r["T"] == 0 or not np.isfinite(r["logZ"]):
            assert not ref["gamma"][off[u]:off[u + 1]].any()
            continue
        rho = np.exp(r["logP"] - r["logZ"])
        sums = ref["gamma"][off[u]:off[u + 1]].sum(1)
        assert np.all(np.abs(sums - rho) <= 1e-12 * rho + 1e-300), (name, u)


@extended
@pytest.mark.parametrize("name", EC.SMALL + EC.REACH)
def test_float64_spread(G, name):
    """the figures of embed_cases' docstring"""
    case, ld = EC.reference(G, name)
    _, f64 = EC.reference(G, name, ft=np.float64)
    fin = np.isfinite(np.asarray(ld["loglik"], dtype=np.float64))
    assert np.array_equal(fin, np.isfinite(f64["loglik"]))
    dl = max((abs(float((a - b) / b)) for x in ("loglik", "logZ") for a, b in zip(f64[x], ld[x])
              if np.isfinite(float(b)) and b != 0), default=0.0)
    ds, where = EC.worst_dist(f64["stats"], ld["stats"])
    dg = E.block_dist(f64["gamma"], ld["gamma"])
    print(f"{name}: float64 from long double: log P, log Z {dl:.1e} | blocks {max(ds, dg):.1e} (worst {where})")
    assert dl <= 1e-12
    assert max(ds, dg) <= RTOL / 8


# ------------------------------------------------------------- the entry point

def test_the_entry_point_is_declared_bound_and_built(G):
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    assert re.search(r"\bint ghmm_estep_embed_streams\s*\(", hdr)
    assert "ghmm_estep_embed_streams" in G.SYMBOLS
    assert hasattr(ctypes.CDLL(G.HIP_LIB), "ghmm_estep_embed_streams")
    assert hasattr(G.Context, "estep_embed_streams")
    assert callable(load_pkg().embed.embedded_em)


# ------------------------------------------------------------- the cases hold what is leaned on

def test_the_cases_hold_what_their_descriptions_claim(G):
    cases = {n: EC.make(G, n) for n in EC.ALL}
    S = {n: [AC.states_of(c, t) if T else 0 for t, T in zip(c.transcripts, c.lens)] for n, c in cases.items()}

    def dense(c, k):
        A = np.asarray(c.words[k][0].A)
        i, j = np.indices(A.shape)
        return bool(np.any((A > 0) & (j != i) & (j != i + 1)))

    n = cases["narrow"]
    assert len({s for s in S["narrow"] if s}) >= 4 and min(s for s in S["narrow"] if s) == 5 and max(S["narrow"]) == 30
    assert any(len(t) > 1 and any(dense(n, k) for k in t) for t in n.transcripts)
    assert any(len(t) == 3 and dense(n, t[1]) for t in cases["short"].transcripts), "no dense word mid-transcript"
    assert (0, 0) in n.transcripts
    assert sum(0 in t for t in n.transcripts) >= 3
    assert any(T == 0 and t == () for t, T in zip(n.transcripts, n.lens))
    assert n.P == 3 and sorted(w.M for w in n.words[0]) == [1, 2, 3] and n.far
    m = cases["mixed"]
    assert m.P == 2 and [(w.M, w.D) for w in m.words[0]] == [(2, 9), (3, 5)]
    assert any(dense(m, k) for k in EC.present(m))
    o = cases["ones"]
    assert all(N == 1 for N in o.Ns) and any(len(t) == 4 for t in o.transcripts)
    assert any(T == 1 and len(t) == 1 for t, T in zip(o.transcripts, o.lens))
    y = cases["many"]
    assert any(len(t) == 20 and 85 <= T <= 95 for t, T in zip(y.transcripts, y.lens))
    assert len(EC.present(y)) < y.K and y.far
    assert any(T == 1 and len(t) == 1 for t, T in zip(y.transcripts, y.lens))
    h = cases["thick"]
    t = h.transcripts[-1]
    assert S["thick"][-1] > 256 and len(EC.present(h)) < h.K
    starts = np.concatenate([[0], np.cumsum([h.Ns[k] for k in t])])
    assert any(dense(h, k) and starts[i + 1] > 256 for i, k in enumerate(t)), "no dense word past state 256"
    assert any(starts[i] < 256 < starts[i + 1] for i in range(len(t))), "no instance straddles 256"
    assert S["cap"] == [2046] and list(cases["cap"].lens) == [2200]
    cm = cases["cap-mixed"]
    assert S["cap-mixed"][AC.CAP_MIXED_LONG] == 2046 and 0 in list(cm.lens) and min(s for s in S["cap-mixed"] if s) <= 6
    assert max(max(s) for s in S.values()) <= AC.MAX_S
    # the far frame lies inside an utterance and its linear densities underflow
    for name in EC.FAR_CASES:
        c = cases[name]
        off = offsets(c.lens)
        assert any(off[u] <= LC.FAR_FRAME < off[u + 1] for u in range(c.U))
        _, ref = EC.reference(G, name, ft=np.float64)
        assert np.all(np.exp(ref["logb"][LC.FAR_FRAME]) == 0.0) and np.all(np.isfinite(ref["logb"][LC.FAR_FRAME]))
    # utterances shorter than their transcript: log Z = -inf and nothing but log P
    _, ref = EC.reference(G, "short", ft=np.float64)
    dead = [u for u, r in enumerate(ref["utt"]) if r["T"] and r["logZ"] == -np.inf]
    assert len(dead) >= 3 and all(ref["loglik"][u] == -np.inf for u in dead)
    assert any(np.isfinite(r["logZ"]) and r["T"] for r in ref["utt"])


# ------------------------------------------------------------- what the cases reach in the two kernels

TOO_SHORT = {"broad": (4,), "wide": (1,), "wide128": (1,), "mid": (2,)}       # fewer frames than states on purpose: log P = -inf


def _dense(c, k):
    A = np.asarray(c.words[k][0].A)
    i, j = np.indices(A.shape)
    return bool(np.any((A > 0) & (j != i) & (j != i + 1)))


def reach(c):
    """a case's row of the coverage table: EC.launch_shape's figures, the size classes of the last words (the
    arm of k_embed_fwd's log Z sum), the passes (0-based: state s is thread s % threads' pass s // threads) in
    which a thread owns a state of a dense word, and whether an utterance repeats a word whose columns all lie
    past a thread's four registers (tie_gamma's table loop walks a chain of two)"""
    row = EC.launch_shape(c)
    nt = row["threads"]
    live = [t for t, T in zip(c.transcripts, c.lens) if T]
    row["last"] = {16 if c.Ns[t[-1]] <= 16 else 32 if c.Ns[t[-1]] <= 32 else 64 for t in live}
    row["dense_pass"] = set()
    for t in live:
        starts = np.concatenate([[0], np.cumsum([c.Ns[k] for k in t])])
        for i, k in enumerate(t):
            if _dense(c, k):
                row["dense_pass"] |= {int(s) // nt for s in range(starts[i], starts[i + 1])}
    row["repeat_in_table"] = any(t.count(k) > 1 and c.bo[k] >= 4 * nt for t in live for k in set(t))
    return row


def test_the_cases_cover_the_launch_shapes_and_the_branches_behind_them(G):
    """the coverage table: what vocab_embed works out of every case (threads = min(256, Smax rounded up to 64),
    PASSES = ceil(Smax / threads) rounded up to 1, 2, 4, 8) and the branches that follow from it"""
    cases = {n: EC.make(G, n) for n in EC.ALL}
    table = {n: reach(c) for n, c in cases.items()}
    for n, r in table.items():
        print(f"{n:10s} Smax {r['Smax']:5d} threads {r['threads']:3d} PASSES {r['passes']} table {int(r['table'])} "
              f"last {sorted(r['last'])} dense in passes {sorted(r['dense_pass'])} repeat in table {int(r['repeat_in_table'])}")
    assert {r["threads"] for r in table.values()} == {64, 128, 192, 256}
    assert {r["passes"] for r in table.values()} == {1, 2, 4, 8}
    assert {r["threads"] for r in table.values() if r["table"]} >= {64, 256}
    assert set().union(*(r["last"] for r in table.values())) == {16, 32, 64}
    assert any(p >= 2 for r in table.values() for p in r["dense_pass"])
    assert any(r["table"] and r["repeat_in_table"] for r in table.values())
    # ... and every new case in its own role
    for n in ("broad", "broad256"):
        c, r = cases[n], table[n]
        nt = r["threads"]
        assert r["table"] and r["repeat_in_table"] and nt == (64 if n == "broad" else 256), (n, r)
        assert c.NS >= 4 * nt + 8 and set(c.Ns) == {3}
        held = EC.present(c)
        assert c.K - 1 in held, "column NS - 1 is in no transcript"
        out = [k for k in range(c.K) if k not in held]
        assert any(c.bo[k] >= 4 * nt for k in out) and any(c.bo[k + 1] <= 4 * nt for k in out)
        assert any(c.bo[k] < 4 * nt < c.bo[k + 1] for k in held), "no spoken word straddles the registers' end"
        assert any(T == 0 for T in c.lens)
    assert max(len(t) for t in cases["broad"].transcripts) <= 21
    assert table["pass4"]["passes"] == 4 and {2, 3} <= table["pass4"]["dense_pass"]
    assert 0 in list(cases["pass4"].lens) and any(len(t) == 2 for t in cases["pass4"].transcripts)
    assert table["pass8"]["passes"] == 8 and 1024 < table["pass8"]["Smax"] <= 1100
    assert max(cases["pass8"].lens) < 1100 and len(cases["pass8"].lens) == 2
    assert table["thick"]["passes"] == 2 and 1 in table["thick"]["dense_pass"]
    assert table["wide"]["threads"] == 192 and table["wide128"]["threads"] == 128
    d = cases["deep"]
    assert table["deep"]["Smax"] == 192 and table["deep"]["last"] == {64} and set(d.Ns) == {64}
    assert any(_dense(d, k) for k in EC.present(d)), "the off-band word is in no transcript"
    # ... and its concatenated model's reduction (a block of 1024 threads per Gaussian, per entry of num_a, per
    # state twice, one for the tail) is the one launch here whose blocks do not fit a 32-bit count of threads
    blocks = {n: c.NS * c.words[0][0].M + c.NS ** 2 + 2 * c.NS + 1 for n, c in cases.items()}
    assert [n for n, b in blocks.items() if b * 1024 >= 2 ** 32] == ["deep"]
    assert max(max(AC.states_of(c, t) for t in c.transcripts) for c in cases.values()) <= AC.MAX_S


@pytest.mark.parametrize("name", EC.REACH)
def test_the_new_utterances_have_finite_scores_on_the_oracles_log_b(G, name):
    """log Z is finite in every utterance of at least one frame, log P in all but those listed as too short"""
    case = EC.make(G, name)
    lb = AC.oracle_log_b(case)
    As = [w[0].A for w in case.words]
    off = offsets(case.lens)
    for u, (t, T) in enumerate(zip(case.transcripts, case.lens)):
        if T == 0:
            continue
        r = EC.lattice(As, case.bo, lb[off[u]:off[u + 1]], t, 0, np.float64)
        assert np.isfinite(r["logZ"]), (name, u)
        assert np.isfinite(r["logP"]) == (u not in TOO_SHORT.get(name, ())), (name, u, float(r["logP"]))


@pytest.mark.parametrize("name,delta", [(n, d) for n, ds in EC.WIDE_DELTAS.items() for d in ds])
def test_the_wide_bands_are_not_empty(G, name, delta):
    """some word of the case has a non-zero num_a at the band's last offset (and so, at delta >= 4, at an offset
    of 4 or more): without it a run at that delta proves nothing about xi[p][o] there"""
    assert 2 <= delta <= EC.MAX_DELTA and EC.MAX_DELTA in EC.WIDE_DELTAS[name]
    case, ref = EC.reference(G, name, delta, np.float64)
    far = 0
    for k in EC.present(case):
        na = np.asarray(ref["stats"][k][0]["num_a"])
        i, j = np.indices(na.shape)
        assert not np.any(na[(j < i) | (j > i + delta)])
        far += int(np.count_nonzero(na[j == i + delta]))
    assert far > 0, (name, delta)
