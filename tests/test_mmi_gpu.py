"""MMI training on the GPU: embed.mmi_em (ghmm_estep_embed_streams as the numerator, ghmm_estep_grammar_streams
as the denominator, ghmm_mstep_ebw) against the restated loop of ebw_cases.mmi_loop — GPU box only.

The case is ebw_cases.mmi_case: 4 three-state words with close means (word 3 in no transcript), 20 utterances of
2 to 3 words on 30 to 60 frames, the bigram_log grammar of the transcripts, 3 iterations, E = 2 (E = 2 gives a
strictly rising objective under the case's seed; test_gstat_host.py asserts that on the restatement, in long
double and in float64).  The objective of an iteration is sum log P_num - sum log P_den under the models the
iteration started from.

The bar on each iteration's objective against the float64 restatement is measured, not fixed: 8 times the float64
restatement's spread from the long-double one over the same loop, the spread being the largest |objective_64 -
objective_ld| over the loop's iterations (the loop compounds rounding, so the largest is the figure that speaks
for the loop).  The test recomputes it; under the case's seed the three differences are 1.8e-13, 2.0e-14 and
1.0e-12, so the bar is 8.3e-12 on objectives near 87 that are differences of sums near -3.6e3 (measured on
the device against the float64 restatement: 0, 0 and 1.4e-12).  The device runs
under GHMM_OPT_KERNELS = 1, the tier whose arithmetic the float64 restatement follows."""
import numpy as np
import pytest

import ebw_cases as B
from _load import load_pkg
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import extended
from test_logscore_gpu import same, tier_of

pytestmark = pytest.mark.gpu


@extended
def test_three_mmi_iterations_raise_the_objective_and_track_the_restatement(G, ctx):
    embed = load_pkg().embed
    start, Xs, lens, transcripts, grammar = B.mmi_case(G)
    held = sorted({k for t in transcripts for k in t})
    assert held == [0, 1, 2]
    t64, _ = B.mmi_loop(start, Xs, lens, transcripts, grammar, B.MMI_ITERS, B.MMI_E, np.float64)
    tld, _ = B.mmi_loop(start, Xs, lens, transcripts, grammar, B.MMI_ITERS, B.MMI_E, np.longdouble)
    o64 = [float(a - b) for a, b in t64]
    old = [a - b for a, b in tld]
    spread = max(abs(float(np.longdouble(x) - y)) for x, y in zip(o64, old))
    bar = 8 * spread
    vocab = [[ctx.model(h) for h in w] for w in start]
    corpora = [ctx.corpus(X, lens) for X in Xs]
    seen, reduced = [], []
    try:
        with tier_of(G, ctx, 1):
            got = embed.mmi_em(ctx, vocab, corpora, transcripts, grammar[1], B.MMI_ITERS, start=grammar[0],
                               fin=grammar[2], E=B.MMI_E, on_iteration=lambda it, n, d: seen.append((it, n, d)),
                               reduce=lambda s: reduced.append((s.N, s.M, s.D)))
            new = [[m.get() for m in w] for w in vocab]
    finally:
        for o in [m for w in vocab for m in w] + corpora:
            o.close()
    # the hook for an all-reduce sees the numerator and the denominator vector of every held word, every iteration
    assert len(reduced) == B.MMI_ITERS * 2 * len(held) and set(reduced) == {(3,) + B.MMI_SHAPE}
    assert [(n, d) for _, n, d in seen] == got and [it for it, _, _ in seen] == list(range(B.MMI_ITERS))
    obj = [n - d for n, d in got]
    print(f"objective on the device {obj}, restated in float64 {o64}; sums {got[0]}")
    print(f"spread of the float64 restatement from the long-double one {spread:.2e}, bar {bar:.2e}; "
          f"device from float64 {[abs(x - y) for x, y in zip(obj, o64)]}")
    assert all(np.isfinite(obj)) and all(y > x for x, y in zip(obj[:-1], obj[1:])), obj
    assert all(abs(x - y) <= bar for x, y in zip(obj, o64)), (obj, o64, bar)
    for k in held:
        assert all(np.all(np.isfinite(a)) for a in new[k][0].arrays())
        assert not same(new[k][0].mean, start[k][0].mean)
    for a, b in zip(new[3][0].arrays(), start[3][0].arrays()):
        assert same(a, np.asarray(b, dtype=np.float64)), "the word in no transcript changed"


def test_full_covariance_models_are_refused(G, ctx):
    from fullcov_support import rand_fmodel
    embed = load_pkg().embed
    rng = np.random.default_rng(1)
    fm = ctx.full_model(rand_fmodel(G, rng, 3, 1, 2, spread=1.0, asym=False))
    try:
        with pytest.raises(TypeError):
            embed.mmi_em(ctx, [[fm]], [], [], np.zeros((1, 1)), 1)
    finally:
        fm.close()
