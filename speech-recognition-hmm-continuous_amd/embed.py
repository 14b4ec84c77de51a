"""Embedded Baum-Welch training on word transcripts (diagonal and full-covariance models): EM directly on
the composite model of every utterance's transcript, over Context.estep_embed_streams or
Context.estep_embed_full_streams (ghmm_estep_embed_streams and ghmm_estep_embed_full_streams in
include/ghmm.h) and the per-word M-step as it is; and MMI training (mmi_em) over the same numerator E-step, the
grammar lattice's E-step as the denominator and the extended Baum-Welch update.

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


def mmi_em(ctx, vocab, corpora, transcripts, pair, iters, start=None, fin=None, E=2.0, on_iteration=None,
           reduce=None):
    """`iters` iterations of MMI training by extended Baum-Welch on the diagonal device models vocab[k][p]
    (updated in place), the corpora[p], transcripts[u] = the sequence of utterance u's words' indices into
    vocab, and the word-pair grammar (pair, start, fin: connect_grammar_streams', bigram_log estimates it from
    transcripts).  One iteration is estep_embed_streams into the numerator vectors, estep_grammar_streams into
    the denominator vectors, then mstep_ebw(E) on every stream of every word that some transcript holds; the
    others keep their models, as in embedded_em.  on_iteration(it, num, den), if given, is called after each
    iteration's updates.  Returns the trace of (sum_u log P_num, sum_u log P_den) under the models each
    iteration STARTED from: their difference is the MMI objective.

    The numerator's occupancies are normalised by log Z_u (the LSE over the last instance's states,
    estep_embed_streams') and the denominator's by log P_u (the grammar lattice's total): a numerator frame's
    gammas sum to exp(log P_u - log Z_u) <= 1, a denominator frame's to 1.  This matters where a transcript's
    last word can end in a state other than its last with noticeable probability (dense words, very short
    utterances): the numerator then weighs that utterance by less than one, while the traced log P_num is the
    path sum into the last state in both.  With left-to-right words on utterances longer than their
    transcripts the two normalisers agree to rounding.
    There is no acoustic scale, no grammar scale and no I-smoothing: E is the only constant.
    reduce(stats), if given, is called on every numerator and every denominator vector of the held words between
    the E-steps and the updates, and before the trace's sums are read.  With one process per GPU, each on its
    share of the utterances, pass `lambda s: ctx.stats_allreduce(s, comm)`: without it every rank would update
    on its local statistics alone.
    Diagonal vocabularies only: TypeError on a FullModel."""
    if any(isinstance(m, FullModel) for word in vocab for m in word):
        raise TypeError("mmi_em takes diagonal models (the grammar E-step has no full-covariance twin yet)")
    held = sorted({int(k) for t in transcripts for k in t})
    num = [[ctx.stats(m.N, m.M, m.D) for m in word] for word in vocab]
    den = [[ctx.stats(m.N, m.M, m.D) for m in word] for word in vocab]
    trace = []
    try:
        for it in range(int(iters)):
            ctx.estep_embed_streams(vocab, corpora, transcripts, num)
            ctx.estep_grammar_streams(vocab, corpora, pair, den, start, fin)
            if reduce is not None:
                for k in held:
                    for s in num[k] + den[k]:
                        reduce(s)
            k0 = held[0] if held else 0         # (every vector carries the common sums; a reduced one, the reduced)
            ln, ld = float(num[k0][0].loglik()[0]), float(den[k0][0].loglik()[0])
            for k in held:
                for m, n, d in zip(vocab[k], num[k], den[k]):
                    ctx.mstep_ebw(m, n, d, E)
            trace.append((ln, ld))
            if on_iteration is not None:
                on_iteration(it, ln, ld)
    finally:
        for word in num + den:
            for s in word:
                s.close()
    return trace
