"""Embedded Baum-Welch training on word transcripts (diagonal and full-covariance models): EM directly on
the composite model of every utterance's transcript, over Context.estep_embed_streams or
Context.estep_embed_full_streams (ghmm_estep_embed_streams and ghmm_estep_embed_full_streams in
include/ghmm.h) and the per-word M-step as it is.

Where the isolated-word trainers need a connected corpus aligned and cut at hard Viterbi boundaries
(align_streams, cut_segments) before every round, here every frame is shared softly between neighbouring
words and the statistics are tied over all instances of a word; nothing goes through the host between the
E-step and the M-steps (a full-covariance word of more than FM_MAXM Gaussians per state takes the host
M-step, which has no cap).
"""
from .ghmm import FullModel

FM_MAXM = 256       # what ghmm_mstep_full_dev takes per state (csrc/ghmm_fullcov.hpp)


def embedded_em(ctx, vocab, corpora, transcripts, iters, on_iteration=None, mstep_full=None):
    """`iters` iterations of embedded Baum-Welch on the device models vocab[k][p] (stream p of word k,
    updated in place; all diagonal or all full-covariance), the corpora[p] and transcripts[u] = the sequence
    of utterance u's words' indices into vocab.  One iteration is one embedded E-step, then the M-step on
    every stream of every word that some transcript holds, and only those: a word without an instance gets
    zero sums, and the M-step on den_c == 0 would re-invert its variances (include/ghmm.h), so such a word
    keeps its model.  Full-covariance models take mstep_full_dev where M <= FM_MAXM and mstep_full beyond;
    mstep_full, if given, is used for them instead (ctx.mstep_full or ctx.mstep_full_dev).
    on_iteration(it, loglik), if given, is called after each iteration's M-steps.  Returns the
    log-likelihood trace: the sum over the utterances of log P_u under the models each iteration STARTED
    from."""
    full = isinstance(vocab[0][0], FullModel)
    if any(isinstance(m, FullModel) != full for word in vocab for m in word):
        raise TypeError("a vocabulary is all diagonal or all full-covariance")
    if full:
        estep, new_stats = ctx.estep_embed_full_streams, ctx.stats_full

        def mstep(m, s):
            (mstep_full or (ctx.mstep_full_dev if m.M <= FM_MAXM else ctx.mstep_full))(m, s)
    else:
        estep, new_stats, mstep = ctx.estep_embed_streams, ctx.stats, ctx.mstep
    held = sorted({int(k) for t in transcripts for k in t})
    stats = [[new_stats(m.N, m.M, m.D) for m in word] for word in vocab]
    trace = []
    try:
        for it in range(int(iters)):
            estep(vocab, corpora, transcripts, stats)
            loglik = stats[0][0].loglik()[0]
            for k in held:
                for m, s in zip(vocab[k], stats[k]):
                    mstep(m, s)
            trace.append(float(loglik))
            if on_iteration is not None:
                on_iteration(it, float(loglik))
    finally:
        for word in stats:
            for s in word:
                s.close()
    return trace
