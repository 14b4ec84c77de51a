"""The lane lattices (logforward_run, logbackward_run, viterbi_run: k_logforward_multi, k_logfb_fwd,
k_logfb_bwd, k_viterbi) on the utterance-length sweep of lensweep_cases.py — GPU box only: every tail residue
of the PF-frame prefetch queue at every lane width (16, 32, 64), banded and dense, for both model kinds, and
an utterance's independence of what lies next to it in memory.  test_lensweep_host.py shows on the CPU that
the cases hold what is leaned on here.  The diagonal cases run under GHMM_OPT_KERNELS = 1 and under the
default tier, as test_logscore_gpu.py's do.  No tolerance is new:

  a. scores       logscore / logscore_full, final_state 0 and 1, in the mix order: test_logscore_gpu's
                  test_lattice_alone.  The long-double lattice on the device's own log b (fetch(BUF_B)), every
                  utterance inside the bound logscore_ref.lattice_scores returns (fulllogscore_ref.lattice_bound
                  with the utterance's own V and La); the -inf pattern exact, an empty utterance 0.0 exactly.
                  All PF residues (T - 1) mod PF are met with a finite log P.
  b. E-step       estep_log / estep_full_log in the mix order: la, lbe, log P and gamma of every utterance
                  against estep_log_ref.lattice_fb on the device's own log b under fullcov_support's
                  check_log_lattice (test_lattice_on_the_devices_own_emission, ..._own_log_b); num_a, den_a,
                  den_c under those tests' check_sums, loglik under their sum of lattice bounds, n_utt exact,
                  and the five common blocks under estep_log_ref.block_dist at RTOL.
  c. Viterbi      viterbi / viterbi_full in the mix order: path and score bit for bit the oracle lattice's on
                  the device's own log b (test_lattice_bit_identical's check_viterbi_lattice); from the frames,
                  diagonal: the oracle's path exactly and its score at 1e-10 relative
                  (test_fuzz_viterbi_against_oracle), full covariance: log b within 1e-11 (1 + |ref|) of
                  fullviterbi_ref's (test_log_emission_and_lattice).
  d. neighbours   the same calls in the asc, desc and mix orders: every utterance's own log b rows are bit-equal
                  across the three, and then so are its scores, its la, lbe and gamma rows and its Viterbi path
                  and score, compared as uint64.  The summed statistics are not compared: their reduction
                  order follows the memory order.
  e. poison       the frames of the odd-length (even-length) utterances NaN, mix order: every clean utterance's
                  log b, scores, lattice rows and Viterbi result are bit-equal to the clean run's; a poisoned
                  frame's log b holds no finite value, and every poisoned utterance meets the references run on
                  the device's own log b (a, b and c again, NaN meeting NaN): not a finite number among its
                  scores, gamma rows of exact zeros.  The value of log b on a NaN frame belongs to the emission
                  and is not pinned here: the vector tier and the full-covariance kernel give the references'
                  -inf (no e_m is above -inf: every e_m > m is false), the matrix-core tier gives NaN, so the
                  poisoned utterances score -inf there and NaN here; either value leaves no finite number in a
                  lattice it enters, and 0 x -inf is as much a NaN as 0 x NaN.  A prefetched value that reached the arithmetic from beyond an utterance shows as a NaN, or as
                  changed bits, in a clean utterance."""
import numpy as np
import pytest

import estep_log_ref as E
import fulllogscore_ref as LR
import lensweep_cases as S
import logscore_ref as R
import oracle_lib as O
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import RTOL, U53, check_log_lattice, check_viterbi_lattice, close_logb, extended, rel_dist
from fullviterbi_ref import log_emission as full_log_emission
from test_fullestep_log_gpu import check_sums
from test_logscore_gpu import TIERS, same, tier_of

pytestmark = pytest.mark.gpu

RUNS = [(name, tier) for name in S.NAMES["diag"] for tier in TIERS] + [(name, None) for name in S.NAMES["full"]]
ROWS = ("la", "lbe", "gamma")
CALLS = ("score", "estep", "viterbi")


class Device:
    """a case's device model and statistics vector and, per (tier, memory order, poison), what the three
    calls leave, downloaded once and sorted by utterance number:
        logb[call][i] = utterance i's rows of BUF_B after `call` (score, estep, viterbi)
        score[fs][U], ll[U], vscore[U], la / lbe / gamma / path [i] = utterance i's rows, stats = the blocks
    and, in memory order, mem = {logb: BUF_B after viterbi, path, vscore, X, lens}"""

    def __init__(self, G, ctx, case):
        self.G, self.ctx, self.case = G, ctx, case
        hm = case.hm
        self.full = case.kind == "full"
        self.model = ctx.full_model(hm) if self.full else ctx.model(hm)
        self.st = (ctx.stats_full if self.full else ctx.stats)(hm.N, hm.M, hm.D)
        self._run = {}

    def _calls(self, corpus):
        G, ctx, m, N = self.G, self.ctx, self.model, self.case.N
        shape = (S.F, N)
        logscore, estep, viterbi, split = (
            (ctx.logscore_full, ctx.estep_full_log, ctx.viterbi_full, G.split_stats_full) if self.full else
            (ctx.logscore, ctx.estep_log, ctx.viterbi, G.split_stats))
        r = {"score": {}, "logb": {}}
        for fs in (0, 1):
            r["score"][fs] = logscore(m, corpus, final_state=bool(fs))
            b = ctx.fetch(G.BUF_B, shape)
            assert fs == 0 or same(b, r["logb"]["score"]), "the emission depends on final_state"
            r["logb"]["score"] = b
        estep(m, corpus, self.st)
        r["stats"] = split(self.st.download(), N, S.M, S.D)
        r["logb"]["estep"] = ctx.fetch(G.BUF_B, shape)
        r["la"], r["lbe"] = ctx.fetch(G.BUF_ALPHA, shape), ctx.fetch(G.BUF_BETA, shape)
        r["gamma"], r["ll"] = ctx.fetch(G.BUF_GAMMA, shape), ctx.fetch(G.BUF_LOGLIK, (S.U,))
        r["path"], r["vscore"] = viterbi(m, corpus)
        r["logb"]["viterbi"] = ctx.fetch(G.BUF_B, shape)
        return r

    def run(self, tier, order, poison=None):
        key = (tier, order, poison)
        if key in self._run:
            return self._run[key]
        X, lens = self.case.corpus(order, poison)
        corpus = self.ctx.corpus(X, lens)
        try:
            if tier is None:
                r = self._calls(corpus)
            else:
                with tier_of(self.G, self.ctx, tier):
                    r = self._calls(corpus)
        finally:
            corpus.close()
        out = {"mem": {"logb": r["logb"]["viterbi"], "path": r["path"], "vscore": r["vscore"], "X": X, "lens": lens},
               "stats": r["stats"],
               "logb": {c: S.by_utterance(r["logb"][c], order) for c in CALLS},
               "score": {fs: S.per_utterance(r["score"][fs], order) for fs in (0, 1)},
               "ll": S.per_utterance(r["ll"], order), "vscore": S.per_utterance(r["vscore"], order)}
        for k in ROWS + ("path",):
            out[k] = S.by_utterance(r[k], order)
        self._run[key] = out
        return out

    def close(self):
        self.model.close()
        self.st.close()


@pytest.fixture(scope="module")
def devices(G, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(G, ctx, S.make(G, name))
        return made[name]
    yield get
    for d in made.values():
        d.close()


def label(name, tier, *more):
    return " ".join([name] + ([] if tier is None else [f"tier {tier}"]) + [str(x) for x in more])


# ------------------------------------------------------------- the checks of a, b and c, on any run

def check_scores(case, r, what, verbose=False):
    """a.  Returns (worst error / bound, the residues met with a finite log P)"""
    worst, residues = 0.0, set()
    logb = np.concatenate(r["logb"]["score"])
    for fs in (0, 1):
        exact, bound = R.lattice_scores(case.hm.A, logb, S.LENS, fs)
        got = r["score"][fs]
        rel_dist(got, exact)        # equal NaN and infinity patterns, an empty utterance's 0 met exactly
        assert got[0] == 0.0 and not np.signbit(got[0]), what
        fin = np.isfinite(exact.astype(np.float64)) & (np.asarray(S.LENS) > 0)
        err = np.abs(got[fin].astype(np.longdouble) - exact[fin]).astype(np.float64)
        ratio = err / bound[fin]
        if verbose:
            print(f"{what} final_state={fs}: error / bound by length",
                  {int(T): round(float(x), 3) for T, x in zip(np.asarray(S.LENS)[fin], ratio)})
        assert (err <= bound[fin]).all(), (what, fs, np.asarray(S.LENS)[fin][err > bound[fin]].tolist())
        worst = max(worst, float(ratio.max(initial=0.0)))
        if fs == 1:
            residues = {(int(T) - 1) % S.PF for T in np.asarray(S.LENS)[fin]}
    return worst, residues


def check_lattice(case, r, what, sums):
    """b.  Returns (worst error / bound of the lattice rows, of the sums, worst block_dist of the common blocks)"""
    N, A = case.N, case.hm.A
    utt = [E.lattice_fb(A, r["logb"]["estep"][i], 1) for i in range(S.U)]
    worst = 0.0
    for i, ut in enumerate(utt):
        if ut["T"] == 0:
            assert r["ll"][i] == 0.0 and not np.signbit(r["ll"][i]), what
            continue
        got = {"la": r["la"][i], "lbe": r["lbe"][i], "logP": r["ll"][i], "gamma": r["gamma"][i]}
        worst = max(worst, check_log_lattice(f"{what}[T = {ut['T']}]", N, got, ut, what="GPU", xi=False))
        if np.isfinite(ut["logZ"]):         # a frame's gammas sum to rho_u
            rho = np.exp(ut["logP"] - ut["logZ"])
            Eb = np.longdouble(E.LE.gamma_exponent_bound(ut["T"], N, ut["V"], ut["La"]))
            ssum = r["gamma"][i].astype(np.longdouble).sum(1)
            assert np.all(np.abs(ssum - rho) <= rho * np.expm1(Eb) + N * 4 * U53), (what, ut["T"])
        else:
            assert np.all(r["gamma"][i] == 0.0), (what, ut["T"])
    if not sums:
        return worst, 0.0, 0.0
    ft = np.longdouble
    ref = {"num_a": sum((ut["xi"] for ut in utt), np.zeros((N, N), ft)),
           "den_a": sum((ut["gamma"][:-1].sum(0) for ut in utt), np.zeros(N, ft)),
           "den_c": sum((ut["gamma"].sum(0) for ut in utt), np.zeros(N, ft)),
           "loglik": sum((ut["logP"] for ut in utt), ft(0)), "n_utt": ft(S.U)}
    st = r["stats"]
    w2 = check_sums({"stats": st}, {"utt": utt, "stats": ref}, N, 1, S.LENS, what)
    assert float(st["n_utt"]) == float(S.U), what
    total, rt = float(st["loglik"]), ref["loglik"]
    assert np.isnan(total) == bool(np.isnan(rt)) and np.isinf(total) == bool(np.isinf(rt)), (what, total, rt)
    if np.isfinite(rt):
        bound = sum(LR.lattice_bound(ut["T"], N, ut["V"], ut["La"]) for ut in utt if ut["T"])
        bound += S.U * U53 * float(sum(abs(ut["logP"]) for ut in utt))
        assert abs(np.longdouble(total) - rt) <= bound, what
    else:
        assert total == float(rt), what
    dist = max(E.block_dist(st[k], ref[k]) for k in E.COMMON)
    assert dist <= RTOL, (what, dist)
    return worst, w2, dist


def check_viterbi(case, r, what, from_frames=True):
    """c"""
    mem = r["mem"]
    check_viterbi_lattice(case.hm.A, mem["logb"], mem["lens"], mem["path"], mem["vscore"])
    if not from_frames:
        return
    if case.kind == "full":
        close_logb(mem["logb"], full_log_emission(case.hm, mem["X"]), 1e-11)
        return
    for i, T in enumerate(S.LENS):
        if T == 0:
            continue
        p, sc = O.viterbi(case.hm, case.frames[i])
        assert np.array_equal(r["path"][i], p), f"{what} T = {T}: path differs"
        got = r["vscore"][i]
        assert (got == sc) if not np.isfinite(sc) else abs(got - sc) <= 1e-10 * abs(sc), (what, T, got, sc)


# ------------------------------------------------------------- a, b, c: against the references

@extended
@pytest.mark.parametrize("name,tier", RUNS)
def test_scores_against_the_reference(G, ctx, devices, name, tier):
    d = devices(name)
    what = label(name, tier)
    worst, residues = check_scores(d.case, d.run(tier, "mix"), what, verbose=True)
    print(f"{what}: scores worst error / bound {worst:.3f}; residues (T - 1) mod {S.PF} met with a finite log P: "
          f"{sorted(residues)}")
    assert residues == set(range(S.PF)), what


@extended
@pytest.mark.parametrize("name,tier", RUNS)
def test_estep_lattice_against_the_reference(G, ctx, devices, name, tier):
    d = devices(name)
    what = label(name, tier)
    r = d.run(tier, "mix")
    worst, w2, dist = check_lattice(d.case, r, what, sums=True)
    print(f"{what}: lattice worst error / bound {worst:.4f}, sums {w2:.4f}, common blocks at {dist:.2e}")
    assert same(r["ll"], r["score"][1]), "BUF_LOGLIK is not the score with final_state = 1"
    lens = np.asarray(S.LENS)
    if not d.case.dense:
        short = (lens > 0) & (lens < d.case.N)
        assert (r["ll"][short] == -np.inf).all() and np.isfinite(r["ll"][lens >= d.case.N]).all()
        for i in np.nonzero(short)[0]:
            assert np.all(r["gamma"][i] == 0.0)


@pytest.mark.parametrize("name,tier", RUNS)
def test_viterbi_against_the_oracle(G, ctx, devices, name, tier):
    d = devices(name)
    check_viterbi(d.case, d.run(tier, "mix"), label(name, tier))


# ------------------------------------------------------------- d. neighbour independence, bit for bit

def bits_differ(a, b, clean=None):
    """the utterance lengths at which two runs differ in a bit, per quantity, over the utterances `clean` marks"""
    out = {}
    keep = [i for i in range(S.U) if clean is None or clean[i]]

    def note(key, x, y):
        bad = [S.LENS[i] for i in keep if not same(np.atleast_1d(x[i]), np.atleast_1d(y[i]))]
        if bad:
            out[key] = bad
    for fs in (0, 1):
        note(f"score final_state={fs}", a["score"][fs], b["score"][fs])
    note("log P", a["ll"], b["ll"])
    for k in ROWS:
        note(k, a[k], b[k])
    note("Viterbi score", a["vscore"], b["vscore"])
    bad = [S.LENS[i] for i in keep if not np.array_equal(a["path"][i], b["path"][i])]
    if bad:
        out["Viterbi path"] = bad
    return out


def logb_differ(a, b, clean=None):
    return {c: [S.LENS[i] for i in range(S.U) if (clean is None or clean[i]) and not same(a["logb"][c][i], b["logb"][c][i])]
            for c in CALLS}


@pytest.mark.parametrize("name,tier", RUNS)
def test_an_utterance_does_not_depend_on_its_neighbours(G, ctx, devices, name, tier):
    d = devices(name)
    mix = d.run(tier, "mix")
    for order in ("asc", "desc"):
        other = d.run(tier, order)
        diff = logb_differ(other, mix)
        assert not any(diff.values()), (label(name, tier, order), "log b rows differ between the orders", diff)
        diff = bits_differ(other, mix)
        assert not diff, (label(name, tier, order), "lengths at which the orders differ", diff)


# ------------------------------------------------------------- e. poisoned neighbours

@extended
@pytest.mark.parametrize("poison", S.POISONS)
@pytest.mark.parametrize("name,tier", RUNS)
def test_poisoned_neighbours(G, ctx, devices, name, tier, poison):
    d = devices(name)
    what = label(name, tier, poison)
    mix, r = d.run(tier, "mix"), d.run(tier, "mix", poison)
    clean = [not S.poisoned(i, poison) for i in range(S.U)]
    diff = logb_differ(r, mix, clean)
    assert not any(diff.values()), (what, "clean utterances' log b rows differ from the clean run's", diff)
    diff = bits_differ(r, mix, clean)
    assert not diff, (what, "clean utterances differ from the clean run at lengths", diff)
    # the poisoned ones: the references on the device's own log b
    for c in CALLS:
        for i in range(S.U):
            if not clean[i]:
                assert not np.isfinite(r["logb"][c][i]).any(), (what, c, S.LENS[i])
    check_scores(d.case, r, what)
    check_lattice(d.case, r, what, sums=False)
    check_viterbi(d.case, r, what, from_frames=False)
    for i in range(S.U):
        if clean[i]:
            continue
        assert not np.isfinite([r["score"][0][i], r["score"][1][i], r["ll"][i], r["vscore"][i]]).any(), (what, S.LENS[i])
        assert np.all(r["gamma"][i] == 0.0) and not np.isfinite(r["la"][i]).any(), (what, S.LENS[i])
    got = {k: sorted({("nan" if np.isnan(x) else str(x)) for i, x in enumerate(v) if not clean[i]})
           for k, v in (("score0", r["score"][0]), ("score1", r["score"][1]), ("viterbi", r["vscore"]))}
    print(f"{what}: the poisoned utterances give {got}")
