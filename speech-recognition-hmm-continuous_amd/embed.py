"""Embedded Baum-Welch training on word transcripts (diagonal models): EM directly on the composite model
of every utterance's transcript, over Context.estep_embed_streams (ghmm_estep_embed_streams in
include/ghmm.h) and the per-word M-step as it is.

Where the isolated-word trainers need a connected corpus aligned and cut at hard Viterbi boundaries
(align_streams, cut_segments) before every round, here every frame is shared softly between neighbouring
words and the statistics are tied over all instances of a word; nothing goes through the host between the
E-step and the M-steps.
"""


def embedded_em(ctx, vocab, corpora, transcripts, iters, on_iteration=None):
    """`iters` iterations of embedded Baum-Welch on the device models vocab[k][p] (stream p of word k,
    updated in place), the corpora[p] and transcripts[u] = the sequence of utterance u's words' indices into
    vocab.  One iteration is one embedded E-step, then mstep on every stream of every word that some
    transcript holds, and only those: a word without an instance gets zero sums, and ghmm_mstep on den_c == 0
    would re-invert its variances (include/ghmm.h), so such a word keeps its model.  on_iteration(it,
    loglik), if given, is called after each iteration's M-steps.  Returns the log-likelihood trace: the sum
    over the utterances of log P_u under the models each iteration STARTED from."""
    held = sorted({int(k) for t in transcripts for k in t})
    stats = [[ctx.stats(m.N, m.M, m.D) for m in word] for word in vocab]
    trace = []
    try:
        for it in range(int(iters)):
            ctx.estep_embed_streams(vocab, corpora, transcripts, stats)
            loglik = stats[0][0].loglik()[0]
            for k in held:
                for m, s in zip(vocab[k], stats[k]):
                    ctx.mstep(m, s)
            trace.append(float(loglik))
            if on_iteration is not None:
                on_iteration(it, float(loglik))
    finally:
        for word in stats:
            for s in word:
                s.close()
    return trace
