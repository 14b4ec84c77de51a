"""The take-again path of the Baum-Welch E-step on the GPU — GPU box only: the utterances that the scaled
backward pass cannot carry and that fix_in_block (inside k_scan_combine), k_backward_fix behind k_combine
and k_backward_fix behind k_backward (GHMM_OPT_KERNELS = 1) take again, whole, in the reference's order
of operations, and the context state that ties the passes together (fix_mark, fix_list, the two-slot
counter fix_cnt, indexed by the parity of the pass's stamp).  The cases and the rule that predicts what
is listed are again_cases.py's; test_again_host.py holds them, on the CPU, to the margins under which
the rule is the only reason anything is listed.

  1. GHMM_OPT_REFORDER_COUNT equals the prediction exactly (the mark lists an utterance once, whichever
     of its chunks asks first), with hundreds of listed utterances too (k_backward_fix's strided second
     round; fix_in_block at 16 utterances per block), and everything the pass leaves agrees with the
     oracle at the project's RTOL with equal NaN and inf patterns.
  2. What an E-step leaves does not depend on what the context ran before it: after a history on a smaller
     corpus (which leaves the counters at either parity, and a workspace that has to grow) the count, the
     statistics, gamma, log P and beta^ are the bits of a context without a history — ghmm.h's promise:
     the same launches in the same order on the same inputs.
  3. The option reads 0 after a gamma / xi pass that keeps no list, and the last counting pass's value
     across calls that run no such pass.

Every test creates and closes its own context: its history is the point."""
import numpy as np
import pytest

import again_cases as AC
from fullcov_support import RTOL, assert_close
from streams_util import assert_frames, stream_case
import oracle_lib as O

pytestmark = pytest.mark.gpu

PATHS = ("default", "separate", "vector")


def path_options(G, path):
    return {"default": (), "separate": ((G.OPT_FUSED_SCAN, 2),), "vector": ((G.OPT_KERNELS, 1),)}[path]


def context(G, path="default", delta=1):
    ctx = G.Context(0)
    for opt, val in path_options(G, path):
        ctx.set_option(opt, val)
    ctx.set_option(G.OPT_DELTA, delta)
    return ctx


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def distance(got, ref, rows=False, floor=1e-13):
    """the worst |got - ref| / (|ref| + (floor / RTOL) scale) over the finite reference entries, with
    assert_close's scale: what it compares with RTOL (printed, asserted by assert_close itself)"""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    r = np.where(np.isfinite(ref), np.abs(ref), 0.0)
    if rows and ref.ndim >= 2:
        scale = r.reshape(len(r), -1).max(axis=1).reshape((-1,) + (1,) * (ref.ndim - 1))
        scale = np.where(scale > 0.0, scale, r.max(initial=0.0))
    else:
        scale = r.max(initial=0.0)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref) / np.maximum(np.abs(ref) + floor / RTOL * scale, 1e-320)
    return float(np.max(d[fin], initial=0.0))


# ---------------------------------------------------------------- 1. exact counts and the oracle

def estep_outputs(G, ctx, model, corpus, stats, case):
    """one ghmm_estep and what it leaves, the count first, beta^ (formed on demand) last"""
    F, N, U = case.F, case.N, case.U
    ctx.estep(model, corpus, stats)
    out = dict(count=ctx.get_option(G.OPT_REFORDER_COUNT), v=stats.download())
    out["gamma"] = ctx.fetch(G.BUF_GAMMA, (F, N))
    out["loglik"] = ctx.fetch(G.BUF_LOGLIK, (U,))
    out["alpha"] = ctx.fetch(G.BUF_ALPHA, (F, N))
    out["beta"] = ctx.fetch(G.BUF_BETA, (F, N))
    out["count_after_beta"] = ctx.get_option(G.OPT_REFORDER_COUNT)
    return out


def check_against_oracle(G, case, out, tag):
    ref_stats, ref = case.ref()
    N, M, D = case.N, case.M, case.D
    got, refs = G.split_stats(out["v"], N, M, D), G.split_stats(ref_stats, N, M, D)
    with np.errstate(invalid="ignore", over="ignore"):
        ref_gamma = ref["alpha"] * ref["beta"] / ref["scale"][:, None]     # TF:1655-1660
    worst = {k: distance(got[k], refs[k]) for k in refs}
    worst.update(loglik_u=distance(out["loglik"], ref["loglik"]), alpha=distance(out["alpha"], ref["alpha"], True),
                 beta=distance(out["beta"], ref["beta"], True), gamma=distance(out["gamma"], ref_gamma, True))
    print(f"{tag}: count {out['count']}, worst relative distance from the oracle "
          f"{max(worst.values()):.3g} ({max(worst, key=worst.get)})")
    for k in refs:
        assert_close(got[k], refs[k], what=f"{tag} stats.{k}")
    assert_close(out["loglik"], ref["loglik"], what=tag + " loglik")
    assert_frames(out["alpha"], ref["alpha"], tag + " alpha")
    assert_frames(out["beta"], ref["beta"], tag + " beta")
    assert_frames(out["gamma"], ref_gamma, tag + " gamma")


def count_check(case, path, out, tag):
    if path == "vector":
        # a wave lists all of its utterances when any of them overflows: bounds only
        n_wild = int(AC.wild_mask(case).sum())
        assert n_wild <= out["count"] <= n_wild * (AC.WAVE // AC.lanes(case.N)), (tag, out["count"], n_wild)
    else:
        assert out["count"] == AC.listed(case), (tag, out["count"], AC.listed(case))
    assert out["count_after_beta"] == out["count"], (tag, out["count_after_beta"])


COUNT_CASES = ([(n, d, dn, p) for n in AC.MIX for d, dn in AC.MIX_VARIANTS for p in PATHS] +
               [(n, 1, False, p) for n in AC.MANY for p in PATHS[:2]] +
               [("tails", 1, False, p) for p in PATHS])


@pytest.mark.parametrize("name,delta,dense,path", COUNT_CASES)
def test_count_is_the_prediction_and_the_pass_is_the_oracles(G, name, delta, dense, path):
    case = AC.make(G, name, delta, dense)
    tag = f"{case.tag} {path}"
    ctx = context(G, path, delta)
    try:
        model, corpus = ctx.model(case.hm), ctx.corpus(case.X, case.lens)
        out = estep_outputs(G, ctx, model, corpus, ctx.stats(case.N, case.M, case.D), case)
    finally:
        ctx.close()
    print(f"{tag}: count {out['count']}, predicted {AC.listed(case)}, wild {int(AC.wild_mask(case).sum())}")
    count_check(case, path, out, tag)
    check_against_oracle(G, case, out, tag)


# ---------------------------------------------------------------- 2. history independence

class Target:
    """One E-step whose outputs must not depend on the context's history.  path, delta: the context's
    options for its whole life; case: the diagonal case whose corpus the histories score and whose
    count is the prediction; small: what the histories run E-steps on."""
    path, delta, small = "default", 1, "small"

    def __init__(self, G):
        self.G = G
        self.case = AC.make(G, "mix16", self.delta)

    def open(self, ctx):
        """device objects of the target, made before any history runs (no launch depends on them)"""
        c = self.case
        self.model, self.corpus = ctx.model(c.hm), ctx.corpus(c.X, c.lens)
        self.stats = ctx.stats(c.N, c.M, c.D)

    def run(self, ctx):
        out = estep_outputs(self.G, ctx, self.model, self.corpus, self.stats, self.case)
        out["v"] = [out["v"]]
        return out

    def expected(self, count):
        return count == AC.listed(self.case)


class Default(Target):
    pass


class Separate(Target):
    path = "separate"


class Delta2(Target):
    delta = 2


class Vector(Target):
    path, small = "vector", "tails_cut"

    def __init__(self, G):
        self.G = G
        self.case = AC.make(G, "tails")

    def expected(self, count):
        n_wild = int(AC.wild_mask(self.case).sum())
        return n_wild <= count <= n_wild * (AC.WAVE // AC.lanes(self.case.N))


class Streams(Target):
    """ghmm_estep_streams on two streams of mix16's lengths (b is the product: the same structural zeros)"""

    def open(self, ctx):
        Target.open(self, ctx)
        hms, Xs, lens = stream_case(self.G, 10, [(2, 5), (1, 3)], list(self.case.lens))
        self.models = [ctx.model(h) for h in hms]
        self.corpora = [ctx.corpus(x, lens) for x in Xs]
        self.svec = [ctx.stats(h.N, h.M, h.D) for h in hms]

    def run(self, ctx):
        G, c = self.G, self.case
        ctx.estep_streams(self.models, self.corpora, self.svec)
        out = dict(count=ctx.get_option(G.OPT_REFORDER_COUNT), v=[s.download() for s in self.svec])
        out["gamma"] = ctx.fetch(G.BUF_GAMMA, (c.F, c.N))
        out["loglik"] = ctx.fetch(G.BUF_LOGLIK, (c.U,))
        out["beta"] = ctx.fetch(G.BUF_BETA, (c.F, c.N))
        return out


class Rows(Target):
    """the row API: ghmm_emission, ghmm_forward, ghmm_backward, ghmm_accumulate"""

    def run(self, ctx):
        G, c = self.G, self.case
        ctx.emission(self.model, self.corpus, True)
        ctx.forward(self.model, self.corpus)
        ctx.backward(self.model, self.corpus)
        count = ctx.get_option(G.OPT_REFORDER_COUNT)
        ctx.accumulate(self.model, self.corpus, self.stats)
        out = dict(count=count, v=[self.stats.download()])
        out["gamma"] = ctx.fetch(G.BUF_GAMMA, (c.F, c.N))
        out["loglik"] = ctx.fetch(G.BUF_LOGLIK, (c.U,))
        out["beta"] = ctx.fetch(G.BUF_BETA, (c.F, c.N))
        return out


class Full(Target):
    """ghmm_estep_full on mix16's model as a full-covariance one (diagonal inverse covariances)"""

    def open(self, ctx):
        Target.open(self, ctx)
        G, hm = self.G, self.case.hm
        ic = np.zeros((hm.N, hm.M, hm.D, hm.D))
        ic[:, :, np.arange(hm.D), np.arange(hm.D)] = hm.inv_var
        self.fmodel = ctx.full_model(G.HostFullModel(hm.A, hm.c, hm.mean, ic, hm.det))
        self.fstats = ctx.stats_full(hm.N, hm.M, hm.D)

    def run(self, ctx):
        G, c = self.G, self.case
        ctx.estep_full(self.fmodel, self.corpus, self.fstats)
        out = dict(count=ctx.get_option(G.OPT_REFORDER_COUNT), v=[self.fstats.download()])
        out["gamma"] = ctx.fetch(G.BUF_GAMMA, (c.F, c.N))
        out["loglik"] = ctx.fetch(G.BUF_LOGLIK, (c.U,))
        out["beta"] = ctx.fetch(G.BUF_BETA, (c.F, c.N))
        return out


TARGETS = {"mix16_default": Default, "mix16_separate": Separate, "mix16_delta2": Delta2, "tails_vector": Vector,
           "streams": Streams, "rows": Rows, "full": Full}
HISTORIES = ("none", "estep1", "estep2", "estep3", "score_grow", "log_grow")


def run_with_history(G, tname, history):
    """the target's outputs after `history` on a fresh context, and the counts the history's own
    E-steps on the small corpus read"""
    target = TARGETS[tname](G)
    small = AC.make(G, target.small)
    assert small.U < target.case.U
    ctx = context(G, target.path, target.delta)
    try:
        target.open(ctx)
        # (the small corpus runs under the target's model: the same shape, and for tails the same one)
        s_model, s_corpus = ctx.model(small.hm), ctx.corpus(small.X, small.lens)
        s_stats = ctx.stats(small.N, small.M, small.D)
        small_counts = []

        def small_estep():
            ctx.estep(s_model, s_corpus, s_stats)
            small_counts.append(ctx.get_option(G.OPT_REFORDER_COUNT))

        if history.startswith("estep"):
            for _ in range(int(history[5:])):
                small_estep()
        elif history == "score_grow":
            small_estep()
            ctx.score(target.model, target.corpus)       # more utterances than any call before it
            small_estep()
        elif history == "log_grow":
            small_estep()
            ctx.estep_log(target.model, target.corpus, target.stats)
        out = target.run(ctx)
    finally:
        ctx.close()
    return target, out, small_counts


_plain = {}


def without_history(G, tname):
    if tname not in _plain:
        _plain[tname] = run_with_history(G, tname, "none")[1]
    return _plain[tname]


@pytest.mark.parametrize("history", HISTORIES)
@pytest.mark.parametrize("tname", list(TARGETS))
def test_history_independence(G, tname, history):
    ref = without_history(G, tname)
    target, out, small_counts = run_with_history(G, tname, history)
    small = AC.make(G, target.small)
    print(f"{tname} after {history}: count {out['count']} (no history {ref['count']}, predicted "
          f"{AC.listed(target.case)}), the history's own counts {small_counts}")
    if target.path == "vector":
        n_wild = int(AC.wild_mask(small).sum())
        assert all(n_wild <= n <= n_wild * 4 and n == small_counts[0] for n in small_counts), small_counts
    else:
        assert all(n == AC.listed(small) for n in small_counts), small_counts
    assert target.expected(out["count"]), out["count"]
    assert out["count"] == ref["count"]
    assert len(out["v"]) == len(ref["v"])
    for p, (a, b) in enumerate(zip(out["v"], ref["v"])):
        assert np.array_equal(a, b, equal_nan=True) and same_bits(a, b), f"statistics vector {p} differs"
    for key in ("gamma", "loglik", "beta"):
        assert np.array_equal(out[key], ref[key], equal_nan=True) and same_bits(out[key], ref[key]), key + " differs"


# ---------------------------------------------------------------- 3. the option after list-less passes

def test_option_after_passes_that_keep_no_list(G):
    from streams_util import synth_case
    mix, many = AC.make(G, "mix16"), AC.make(G, "many16")
    wide_hm, wide_X, wide_lens = synth_case(G, 70, 1, 3, [90, 40, 75])      # 40 < 70 states: no path
    n = AC.listed(mix)
    assert n == 5
    ctx = context(G)
    try:
        model, corpus = ctx.model(mix.hm), ctx.corpus(mix.X, mix.lens)
        stats = ctx.stats(mix.N, mix.M, mix.D)
        wide, wide_c, wide_s = ctx.model(wide_hm), ctx.corpus(wide_X, wide_lens), ctx.stats(70, 1, 3)
        larger = ctx.corpus(many.X, many.lens)
        empty = ctx.corpus(np.zeros((0, mix.D)), np.zeros(0, dtype=np.int32))
        read = lambda: ctx.get_option(G.OPT_REFORDER_COUNT)      # noqa: E731

        assert read() == 0                                  # no pass yet
        ctx.estep(model, corpus, stats)
        assert read() == n
        ctx.estep(wide, wide_c, wide_s)                     # k_backward_wide keeps no list
        assert read() == 0
        ref, _ = O.estep(wide_hm, wide_X, wide_lens, dumps=False)
        assert_close(wide_s.download(), ref, what="70 states")
        ctx.estep(model, corpus, stats)
        assert read() == n
        ctx.estep_log(model, corpus, stats)                 # the log-domain lattice takes nothing again
        assert read() == 0
        ctx.estep(model, corpus, stats)
        assert read() == n
        v = stats.download()
        ctx.score(model, larger)                            # no gamma / xi pass; the workspace grows
        assert read() == n
        ctx.estep(model, corpus, stats)                     # and the next pass starts from 0 again
        assert read() == n
        assert same_bits(v, stats.download())
        ctx.estep_embed_streams([[model]], [corpus], [(0,)] * mix.U, [[stats]])
        assert read() == 0
        ctx.estep(model, corpus, stats)
        assert read() == n
        ctx.estep(model, empty, stats)                      # no utterance: nothing to take again
        assert read() == 0
    finally:
        ctx.close()
