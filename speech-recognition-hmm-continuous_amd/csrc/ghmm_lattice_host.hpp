// ghmm_lattice_host.hpp — what the several-stream and vocabulary calls of both model kinds share on
// the host.  Part of ghmm_hip.hip's translation unit, included once ahead of ghmm_viterbi: the diagonal
// entry points behind it and the full-covariance ones (ghmm_fullhost.hpp) call into it.  Once an emission
// launch has written b or log b into the workspace nothing here knows which kind of Gaussian produced it:
// the helpers see the context, a corpus, a table of the words' recursions and the workspace.  The
// checks and the host-built tables are templates over the model type (ghmm_model and ghmm_fmodel both
// have N, M, D, A and logA) and take the kind's own pair check (check_pair, check_full).

// A vocabulary pass: NS = the vocabulary's states, Nmax = the largest word's, dtab = the table of the
// words' recursions on the device (dtab[k] = {word k's A or log A, its N, the offset of its states in
// b[F][NS]}).  A single word is a vocabulary of one (one_word_table).
struct vocab_pass {
    int NS = 0, Nmax = 0;
    const fwd_model *dtab = nullptr;
};

// ------------------------------------------------ checks

// One word on P feature streams, models[p] / corpora[p] = stream p (behind the caller's check of the
// arrays and of P): per stream the kind's pair check, the states and the utterance lengths against
// stream 0's, then whatever else the caller checks per stream (`then`: the full-covariance E-step's
// statistics vector).  Called by check_streams and check_full_streams.
template <class Model, class Pair, class Then>
static int stream_checks(Model *const *models, ghmm_corpus *const *corpora, int P, Pair pair, Then then)
{
    for (int p = 0; p < P; p++) {
        int rc = pair(models[p], corpora[p]);
        if (rc) return rc;
        if (models[p]->N != models[0]->N) {
            ghmm_set_error("stream %d has %d states, stream 0 has %d", p, models[p]->N, models[0]->N);
            return GHMM_ERR_ARG;
        }
        if (corpora[p]->U != corpora[0]->U || corpora[p]->len != corpora[0]->len) {
            ghmm_set_error("stream %d: utterance count or lengths differ from stream 0", p);
            return GHMM_ERR_ARG;
        }
        if ((rc = then(p))) return rc;
    }
    return GHMM_OK;
}

// A vocabulary of n_models words on P feature streams (models[k * P + p] = stream p of word k,
// corpora[p] = stream p of the utterances; the single-stream calls pass P = 1).  `what` = the entry
// point's name in the texts.  Nothing is launched, grown or written here; fills v->NS and v->Nmax.
// Called by vocab_check (diagonal, which adds its own refusals behind it) and fvocab_begin.
template <class Model, class Pair>
static int vocab_checks(Model *const *models, int n_models, ghmm_corpus *const *corpora, int P, bool have_dest,
                        const char *what, Pair pair, vocab_pass *v)
{
    int rc;
    ARG_CHECK_AS(what, models && n_models > 0 && corpora, "null argument");
    if (P < 1 || P > GHMM_MAX_STREAMS) {
        ghmm_set_error("%s: 1 to %d feature streams (asked: %d)", what, GHMM_MAX_STREAMS, P);
        return GHMM_ERR_ARG;
    }
    for (int p = 0; p < P; p++) ARG_CHECK_AS(what, corpora[p], "null argument");
    const ghmm_corpus *c = corpora[0];
    ARG_CHECK_AS(what, have_dest || c->U == 0, "null destination");
    for (int k = 0; k < n_models * P; k++) ARG_CHECK_AS(what, models[k], "null model");
    v->NS = v->Nmax = 0;
    for (int k = 0; k < n_models; k++) {
        const int N = models[(size_t)k * P]->N;
        for (int p = 1; p < P; p++)
            if (models[(size_t)k * P + p]->N != N) {
                ghmm_set_error("%s: word %d: stream %d has %d states, stream 0 has %d", what, k, p,
                               models[(size_t)k * P + p]->N, N);
                return GHMM_ERR_ARG;
            }
        v->NS += N;
        v->Nmax = N > v->Nmax ? N : v->Nmax;
    }
    for (int p = 0; p < P; p++)
        for (int k = 1; k < n_models; k++)
            if (models[(size_t)k * P + p]->M != models[p]->M || models[(size_t)k * P + p]->D != models[p]->D) {
                if (P > 1) ghmm_set_error("%s: every model must have the same M and D (stream %d)", what, p);
                else ghmm_set_error("%s: every model must have the same M and D", what);
                return GHMM_ERR_UNSUPPORTED;
            }
    for (int p = 0; p < P; p++) {
        if ((rc = pair(models[p], corpora[p]))) return rc;
        if (corpora[p]->U != c->U || corpora[p]->len != c->len) {
            ghmm_set_error("%s: stream %d: utterance count or lengths differ from stream 0", what, p);
            return GHMM_ERR_ARG;
        }
    }
    return GHMM_OK;
}

// ------------------------------------------------ tables and the cached concatenated models

// The concatenated vocabulary of one stream lives in the context from one call to the next (a recogniser
// scores batch after batch against one vocabulary: creating and freeing twenty device buffers per call
// was 0.75 ms of a 0.9 ms call): *slot stays while its shape is (N, M, D), otherwise it is destroyed and
// `create` makes a new one.  Called by vocab_gather and fvocab_begin.
template <class Model, class Create>
static int cat_slot(ghmm_ctx *ctx, Model **slot, int N, int M, int D, void (*destroy)(ghmm_ctx *, Model *),
                    Create create)
{
    if (*slot && ((*slot)->N != N || (*slot)->M != M || (*slot)->D != D)) {
        destroy(ctx, *slot);
        *slot = nullptr;
    }
    return *slot ? GHMM_OK : create(slot);
}

// A pass's tables, built on the host and uploaded into the context's one table buffer, ahead of the
// launches that read them on the same stream: the words' recursions (dtab[k].A = word k's A, or its log A
// with log_domain, stream 0's; N; the offset of the word's states in b), then from the next 16-byte
// boundary every stream's gather sources, *dsrc (src(m, g0) = the kind's source for word model m, whose
// Gaussians go to g0 .. g0 + m->N * m->M of that stream's concatenated model; stream p's n_models
// entries start at (*dsrc)[p * n_models]).  Called by vocab_gather and fvocab_begin.
template <class Src, class Model, class MakeSrc>
static int vocab_tables(ghmm_ctx *ctx, Model *const *models, int n_models, int P, bool log_domain, MakeSrc src,
                        vocab_pass *v, const Src **dsrc)
{
    int rc;
    std::vector<fwd_model> tab((size_t)n_models);
    std::vector<Src> srcs((size_t)n_models * P);
    for (int p = 0; p < P; p++) {
        int go = 0, so = 0;
        for (int k = 0; k < n_models; k++) {
            const Model *m = models[(size_t)k * P + p];
            if (p == 0) tab[k] = {log_domain ? m->logA : m->A, m->N, so};
            srcs[(size_t)p * n_models + k] = src(m, go);
            go += m->N * m->M;
            so += m->N;
        }
    }
    const size_t tab_bytes = tab.size() * sizeof(fwd_model), src_bytes = srcs.size() * sizeof(Src);
    if ((rc = ctx->bt_tab.grow(tab_bytes + src_bytes + 16))) return rc;
    v->dtab = (const fwd_model *)ctx->bt_tab.p;
    *dsrc = (const Src *)(ctx->bt_tab + ((tab_bytes + 15) / 16) * 16);
    // (the tables leave pageable host vectors: the copies complete before the call returns them)
    HIP_TRY(hipMemcpyAsync(ctx->bt_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync((void *)*dsrc, srcs.data(), src_bytes, hipMemcpyHostToDevice, ctx->stream));
    return GHMM_OK;
}

// A single word as a vocabulary of one, for the log-domain score's lattice launch: its table (log A)
// into the table buffer, bt_ll for its scores.  Called by logscore_word, ghmm_logscore_full and
// ghmm_logscore_full_streams.
static int one_word_table(ghmm_ctx *ctx, const double *logA, int N, const ghmm_corpus *c, vocab_pass *v)
{
    int rc;
    const fwd_model one = {logA, N, 0};
    if ((rc = ctx->bt_ll.grow((size_t)c->U)) || (rc = ctx->bt_tab.grow(sizeof one))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->bt_tab, &one, sizeof one, hipMemcpyHostToDevice, ctx->stream));
    v->NS = v->Nmax = N;
    v->dtab = (const fwd_model *)ctx->bt_tab.p;
    return GHMM_OK;
}

// ------------------------------------------------ the vocabulary lattices
// Each runs over the n_models entries of v.dtab on the b or log b[F][NS] in the workspace, one state per
// lane (Nmax <= 64), and writes bt_ll[n_models][U].  Called by the batch calls of both kinds.

// k_forward_multi on b: log P, with the final-state term if final_state; scale / sinv: n_models * F + 1
// doubles each for c_t and 1 / c_t, or the sink where nobody reads them
static int vocab_forward(ghmm_ctx *ctx, const vocab_pass &v, int n_models, const ghmm_corpus *c, double *scale,
                         double *sinv, int final_state)
{
    const lane_grid lg(v.Nmax, c->U);
    kscope ks(ctx, GHMM_K_FORWARD);
    GHMM_BY_LANES(lg.L, hipLaunchKernelGGL(k_forward_multi<LL>, dim3(lg.blocks, (unsigned)n_models), dim3(WAVE), 0,
                                           ctx->stream, c->U, v.NS, c->F, v.dtab, ctx->b, c->off, scale, sinv,
                                           ctx->bt_ll, ctx->sink, c->order, final_state));
    return launch_ok("k_forward_multi");
}

// k_viterbi_multi on log b (dtab: log A): the best path's score
static int vocab_viterbi(ghmm_ctx *ctx, const vocab_pass &v, int n_models, const ghmm_corpus *c)
{
    const lane_grid lg(v.Nmax, c->U);
    kscope ks(ctx, GHMM_K_VITERBI);
    GHMM_BY_LANES(lg.L, hipLaunchKernelGGL(k_viterbi_multi<LL>, dim3(lg.blocks, (unsigned)n_models), dim3(WAVE), 0,
                                           ctx->stream, c->U, v.NS, v.dtab, ctx->b, c->off, ctx->bt_ll, ctx->sink,
                                           c->order));
    return launch_ok("k_viterbi_multi");
}

// k_logforward_multi on log b (dtab: log A): la_{T-1}(N_k - 1), or LSE_j la_{T-1}(j) with final_state == 0
static int vocab_logforward(ghmm_ctx *ctx, const vocab_pass &v, int n_models, const ghmm_corpus *c, int final_state)
{
    const lane_grid lg(v.Nmax, c->U);
    kscope ks(ctx, GHMM_K_FORWARD);
    GHMM_BY_LANES(lg.L, hipLaunchKernelGGL(k_logforward_multi<LL>, dim3(lg.blocks, (unsigned)n_models), dim3(WAVE),
                                           0, ctx->stream, c->U, v.NS, v.dtab, ctx->b, c->off, ctx->bt_ll, ctx->sink,
                                           c->order, final_state));
    return launch_ok("k_logforward_multi");
}

// the pass's scores, bt_ll[n_models][U], to the host; waits for the stream
static int vocab_scores_out(ghmm_ctx *ctx, int n_models, const ghmm_corpus *c, double *host)
{
    HIP_TRY(hipMemcpyAsync(host, ctx->bt_ll, (size_t)n_models * c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

// ------------------------------------------------ Viterbi paths

// what a Viterbi lattice writes: psi in rows of `row` bytes per frame (the lanes per utterance, or the
// states of a model beyond 64), and the state per frame
static int viterbi_ws(ghmm_ctx *ctx, const ghmm_corpus *c, int row)
{
    int rc;
    if ((rc = ctx->psi.grow((size_t)c->F * row + 16))) return rc;
    return ctx->path.grow((size_t)c->F);
}

// a Viterbi lattice's paths (ctx->path) and scores (ctx->loglik) to the host; waits for the stream
static int viterbi_out(ghmm_ctx *ctx, const ghmm_corpus *c, int32_t *path_host, double *score_host)
{
    int rc;
    HIP_TRY(hipMemcpyAsync(score_host, ctx->loglik, (size_t)c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (c->F && (rc = d2h_pageable(ctx, path_host, ctx->path, (size_t)c->F, true))) return rc;
    HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

// k_viterbi of one word of N <= 64 states on its log A and the log b[F][N] in the workspace (psi and
// path sized by the caller, U > 0), then viterbi_out.  Called by run_viterbi (diagonal), ghmm_viterbi_full
// and ghmm_viterbi_full_streams.
static int run_viterbi_lanes(ghmm_ctx *ctx, int N, const double *logA, const ghmm_corpus *c, int32_t *path_host,
                             double *score_host)
{
    int rc;
    const lane_grid lg(N, c->U);
    {
        kscope ks(ctx, GHMM_K_VITERBI);
        GHMM_BY_LANES(lg.L, hipLaunchKernelGGL(k_viterbi<LL>, dim3(lg.blocks), dim3(WAVE), 0, ctx->stream, N, c->U,
                                               logA, ctx->b, c->off, ctx->psi, ctx->path, ctx->loglik, ctx->sink,
                                               c->order));
    }
    if ((rc = launch_ok("k_viterbi"))) return rc;
    return viterbi_out(ctx, c, path_host, score_host);
}

// The word decoder behind its emission launches: the score table (vocab_viterbi), then on the device and
// without a host round trip every utterance's winning word (k_vocab_best) and that word's lattice again
// with back-pointers on the log b already in the workspace (k_viterbi_pick, over (blocks, words) like
// k_viterbi_multi).  One stream wait.  Called by ghmm_recognise_streams and ghmm_recognise_full_streams.
static int vocab_decode(ghmm_ctx *ctx, const vocab_pass &v, int n_models, const ghmm_corpus *c, int32_t *word_host,
                        int32_t *path_host, double *score_host)
{
    int rc;
    const lane_grid lg(v.Nmax, c->U);
    if ((rc = ctx->best_word.grow((size_t)c->U)) || (rc = viterbi_ws(ctx, c, lg.L))) return rc;
    if ((rc = vocab_viterbi(ctx, v, n_models, c))) return rc;
    {
        kscope ks(ctx, GHMM_K_VITERBI);
        hipLaunchKernelGGL(k_vocab_best, dim3((unsigned)((c->U + 255) / 256)), dim3(256), 0, ctx->stream, n_models,
                           c->U, (const double *)ctx->bt_ll, ctx->best_word);
    }
    if ((rc = launch_ok("k_vocab_best"))) return rc;
    {
        kscope ks(ctx, GHMM_K_VITERBI);
        GHMM_BY_LANES(lg.L, hipLaunchKernelGGL(k_viterbi_pick<LL>, dim3(lg.blocks, (unsigned)n_models), dim3(WAVE), 0,
                                               ctx->stream, c->U, v.NS, v.dtab, ctx->b, c->off,
                                               (const int *)ctx->best_word, ctx->psi, ctx->path, ctx->sink,
                                               c->order));
    }
    if ((rc = launch_ok("k_viterbi_pick"))) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "word_host takes the device's ints as they are");
    HIP_TRY(hipMemcpyAsync(score_host, ctx->bt_ll, (size_t)n_models * c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(word_host, ctx->best_word, (size_t)c->U * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (c->F && (rc = d2h_pageable(ctx, path_host, ctx->path, (size_t)c->F, true))) return rc;
    HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

// ------------------------------------------------ connected words

// The connected-word decoder's own refusals, behind the vocabulary checks that filled v and before
// anything is launched, grown or written: the penalty, and what k_connect holds (a word's states in six
// bits of its state table, the composite states in LDS).  Called by ghmm_connect_streams and
// ghmm_connect_full_streams.
static int connect_check(const vocab_pass &v, double penalty, const char *what)
{
    if (penalty != penalty || penalty == INFINITY) {
        ghmm_set_error("%s: the word penalty is NaN or +inf", what);
        return GHMM_ERR_ARG;
    }
    if (v.Nmax > 64 || v.NS > CONNECT_MAX_NS) {
        ghmm_set_error("%s: %d states in all, the largest word %d: the connected-word lattice takes %d and 64",
                       what, v.NS, v.Nmax, CONNECT_MAX_NS);
        return GHMM_ERR_UNSUPPORTED;
    }
    return GHMM_OK;
}

// The connected-word decoder behind its emission launches (U > 0, connect_check passed): k_connect, one
// workgroup per utterance, lattice and trace in ONE launch on the log b[F][NS] in the workspace; then the
// scores (bt_ll[U]), the word per frame and, in one byte per frame, the state (bits 0..5) with the begin
// mark (bit 7), which the host takes apart.  One stream wait.
static int vocab_connect(ghmm_ctx *ctx, const vocab_pass &v, int n_models, const ghmm_corpus *c, double penalty,
                         int32_t *word_host, int32_t *path_host, int32_t *begin_host, double *score_host)
{
    int rc;
    if ((rc = ctx->cn_psi.grow((size_t)c->F * v.NS + 16)) || (rc = ctx->cn_word.grow((size_t)c->F)) ||
        (rc = ctx->path.grow((size_t)c->F)) || (rc = ctx->bt_ll.grow((size_t)c->U)))
        return rc;
    const size_t lds = connect_lds(v.NS);
    if (lds > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_connect))) return rc;
    const int threads = std::min(CONNECT_THREADS, ((v.NS + WAVE - 1) / WAVE) * WAVE);
    {
        kscope ks(ctx, GHMM_K_VITERBI);
        hipLaunchKernelGGL(k_connect, dim3((unsigned)c->U), dim3((unsigned)threads), lds, ctx->stream, c->U, n_models,
                           v.NS, v.dtab, (const double *)ctx->b, c->off, penalty, ctx->cn_psi, ctx->cn_word,
                           ctx->path, ctx->bt_ll, c->order);
    }
    if ((rc = launch_ok("k_connect"))) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "word_host takes the device's ints as they are");
    HIP_TRY(hipMemcpyAsync(score_host, ctx->bt_ll, (size_t)c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (c->F) {
        HIP_TRY(hipMemcpyAsync(word_host, ctx->cn_word, (size_t)c->F * 4, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = d2h_pageable(ctx, path_host, ctx->path, (size_t)c->F, true))) return rc;
        for (long long f = 0; f < c->F; f++) {
            begin_host[f] = path_host[f] >> 7;
            path_host[f] &= 63;
        }
    } else
        HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

// ------------------------------------------------ connected words under a word-pair grammar

// The grammar decoder's own refusals, behind the vocabulary checks that filled v and before anything is
// launched, grown or written: what k_grammar holds (connect_check's states; a predecessor word in a
// byte, the dense K x K table), a missing table when there are utterances, and entries that are NaN or
// +inf (-inf forbids; start and fin may be null: all 0).  Called by ghmm_connect_grammar_streams and
// ghmm_connect_grammar_full_streams.
static int grammar_check(const vocab_pass &v, int K, int U, const double *start, const double *pair,
                         const double *fin, const char *what)
{
    int rc = connect_check(v, 0.0, what);
    if (rc) return rc;
    static_assert(GRAMMAR_MAX_K == GHMM_GRAMMAR_MAX_WORDS, "the header's cap is the kernel's");
    if (K > GRAMMAR_MAX_K) {
        ghmm_set_error("%s: a vocabulary of %d words: the dense word-pair table takes GHMM_GRAMMAR_MAX_WORDS = %d",
                       what, K, GRAMMAR_MAX_K);
        return GHMM_ERR_UNSUPPORTED;
    }
    if (!pair) {
        ARG_CHECK_AS(what, U == 0, "null pair table");
        return GHMM_OK;
    }
    const struct {
        const double *p;
        size_t n;
        const char *name;
    } arrays[3] = {{start, (size_t)K, "start"}, {pair, (size_t)K * K, "pair"}, {fin, (size_t)K, "fin"}};
    for (const auto &a : arrays)
        for (size_t i = 0; a.p && i < a.n; i++)
            if (a.p[i] != a.p[i] || a.p[i] == INFINITY) {
                ghmm_set_error("%s: %s[%zu] is NaN or +inf", what, a.name, i);
                return GHMM_ERR_ARG;
            }
    return GHMM_OK;
}

// The grammar decoder behind its emission launches (U > 0, grammar_check passed): the grammar (start[K] |
// pair[K][K] | fin[K]; a null start or fin as zeros) into the context's gr_tab ahead of the launch on the
// same stream, then k_grammar, one workgroup per utterance, lattice and trace in ONE launch on the log
// b[F][NS] in the workspace; then the scores, the word per frame and the state byte with the begin mark
// as vocab_connect returns them.  The back-pointers and the word per frame go through the connected-word
// decoder's scratch (cn_psi, cn_word): both calls write what they read.  One stream wait.
static int vocab_connect_grammar(ghmm_ctx *ctx, const vocab_pass &v, int K, const ghmm_corpus *c, const double *start,
                                 const double *pair, const double *fin, int32_t *word_host, int32_t *path_host,
                                 int32_t *begin_host, double *score_host)
{
    int rc;
    const size_t KK = (size_t)K * K;
    if ((rc = ctx->cn_psi.grow((size_t)c->F * v.NS + 16)) || (rc = ctx->cn_word.grow((size_t)c->F)) ||
        (rc = ctx->path.grow((size_t)c->F)) || (rc = ctx->bt_ll.grow((size_t)c->U)) ||
        (rc = ctx->gr_entw.grow((size_t)c->F * K + 16)) || (rc = ctx->gr_tab.grow(KK + 2 * (size_t)K)))
        return rc;
    // (pageable sources: the copies complete before the calls return them)
    double *dstart = ctx->gr_tab, *dpair = dstart + K, *dfin = dpair + KK;
    if (start) HIP_TRY(hipMemcpyAsync(dstart, start, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(hipMemsetAsync(dstart, 0, (size_t)K * 8, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dpair, pair, KK * 8, hipMemcpyHostToDevice, ctx->stream));
    if (fin) HIP_TRY(hipMemcpyAsync(dfin, fin, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(hipMemsetAsync(dfin, 0, (size_t)K * 8, ctx->stream));
    const size_t lds = grammar_lds(v.NS, K);
    if (lds > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_grammar))) return rc;
    const int threads = std::min(CONNECT_THREADS, ((v.NS + WAVE - 1) / WAVE) * WAVE);
    {
        kscope ks(ctx, GHMM_K_VITERBI);
        hipLaunchKernelGGL(k_grammar, dim3((unsigned)c->U), dim3((unsigned)threads), lds, ctx->stream, c->U, K, v.NS,
                           v.dtab, (const double *)ctx->b, c->off, (const double *)ctx->gr_tab.p,
                           (int)grammar_staged(v.NS, K), ctx->cn_psi, ctx->gr_entw, ctx->cn_word, ctx->path, ctx->bt_ll,
                           c->order);
    }
    if ((rc = launch_ok("k_grammar"))) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "word_host takes the device's ints as they are");
    HIP_TRY(hipMemcpyAsync(score_host, ctx->bt_ll, (size_t)c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (c->F) {
        HIP_TRY(hipMemcpyAsync(word_host, ctx->cn_word, (size_t)c->F * 4, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = d2h_pageable(ctx, path_host, ctx->path, (size_t)c->F, true))) return rc;
        for (long long f = 0; f < c->F; f++) {
            begin_host[f] = path_host[f] >> 7;
            path_host[f] &= 63;
        }
    } else
        HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

// The grammar lattice's two launches on the log b[F][NS] in the workspace (U > 0, grammar_check passed,
// em_la, gp_x, gr_tab and what the backward form writes grown by the caller): the grammar as
// vocab_connect_grammar uploads it and behind it a TRANSPOSED copy of the table (start[K] | pair[K][K] |
// fin[K] | pairT[K][K], pairT[k' * K + k] = pair[k][k']: the backward launch reduces along the table's rows,
// ghmm_gpost.hpp says why it reads a copy) into the context's gr_tab ahead of the launches on the same
// stream; then k_gpost_fwd (la rows [F][NS] into em_la, x rows [F][K] into gp_x, log P_u into loglik) and
// k_gpost_bwd, one workgroup per utterance each, both under GHMM_K_FORWARD: the posteriors form (gamma[F][NS],
// occ and ent [F][K] into gp_occ and gp_ent) or with `stats` the statistics form (gamma and one partial per
// utterance for a model of NS states in part_xi, part_dena and part_denc; occ and ent are not formed; the
// posterior rows in `posts` of an utterance without a finite log P are zeroed).
// Nothing waits.  Called by vocab_grammar_post and vocab_grammar_stats.
static int gpost_launches(ghmm_ctx *ctx, const vocab_pass &v, int K, const ghmm_corpus *c, const double *start,
                          const double *pair, const double *fin, bool stats, const gpost_posts &posts)
{
    int rc;
    const size_t KK = (size_t)K * K;
    // (pageable sources: the copies complete before the calls return them)
    double *dstart = ctx->gr_tab, *dpair = dstart + K, *dfin = dpair + KK, *dpairT = dfin + K;
    std::vector<double> pairT(KK);
    for (int w = 0; w < K; w++)
        for (int k = 0; k < K; k++) pairT[(size_t)k * K + w] = pair[(size_t)w * K + k];
    if (start) HIP_TRY(hipMemcpyAsync(dstart, start, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(hipMemsetAsync(dstart, 0, (size_t)K * 8, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dpair, pair, KK * 8, hipMemcpyHostToDevice, ctx->stream));
    if (fin) HIP_TRY(hipMemcpyAsync(dfin, fin, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(hipMemsetAsync(dfin, 0, (size_t)K * 8, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dpairT, pairT.data(), KK * 8, hipMemcpyHostToDevice, ctx->stream));
    const size_t base_f = gpost_fwd_lds_base(v.NS, K), base_b = gpost_bwd_lds_base(v.NS, K);
    const size_t lds_f = gpost_lds(base_f, K), lds_b = gpost_lds(base_b, K);
    const int threads = std::min(GPOST_THREADS, ((v.NS + WAVE - 1) / WAVE) * WAVE);
    const int passes = (v.NS + threads - 1) / threads;
#define GHMM_GPOST_FWD(PS)                                                                                         \
    do {                                                                                                           \
        if (lds_f > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_gpost_fwd<PS>))) return rc;                 \
        kscope ks(ctx, GHMM_K_FORWARD);                                                                            \
        hipLaunchKernelGGL(k_gpost_fwd<PS>, dim3((unsigned)c->U), dim3((unsigned)threads), lds_f, ctx->stream, c->U, \
                           K, v.NS, v.dtab, (const double *)ctx->b, c->off, (const double *)ctx->gr_tab.p,         \
                           (int)gpost_staged(base_f, K), ctx->em_la, ctx->gp_x, ctx->loglik, c->order);            \
    } while (0)
    if (passes <= 1) GHMM_GPOST_FWD(1);
    else if (passes <= 2) GHMM_GPOST_FWD(2);
    else if (passes <= 4) GHMM_GPOST_FWD(4);
    else GHMM_GPOST_FWD(8);
#undef GHMM_GPOST_FWD
    if ((rc = launch_ok("k_gpost_fwd"))) return rc;
#define GHMM_GPOST_BWD(PS, ST, OCC, ENT, DELTA, PXI, PDA, PDC)                                                     \
    do {                                                                                                           \
        if (lds_b > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_gpost_bwd<PS, ST>))) return rc;             \
        kscope ks(ctx, GHMM_K_FORWARD);                                                                            \
        hipLaunchKernelGGL((k_gpost_bwd<PS, ST>), dim3((unsigned)c->U), dim3((unsigned)threads), lds_b, ctx->stream, \
                           c->U, K, v.NS, v.dtab, (const double *)ctx->b, c->off, (const double *)ctx->gr_tab.p,   \
                           (int)gpost_staged(base_b, K), (const double *)ctx->em_la, (const double *)ctx->gp_x,    \
                           (const double *)ctx->loglik, ctx->gamma, OCC, ENT, c->order, DELTA, PXI, PDA, PDC,      \
                           posts);                                                                                 \
    } while (0)
#define GHMM_GPOST_BWD_POST(PS)                                                                                    \
    GHMM_GPOST_BWD(PS, false, ctx->gp_occ, ctx->gp_ent, 0, (double *)nullptr, (double *)nullptr, (double *)nullptr)
#define GHMM_GPOST_BWD_STATS(PS)                                                                                   \
    GHMM_GPOST_BWD(PS, true, (double *)nullptr, (double *)nullptr, (int)ctx->delta, ctx->part_xi, ctx->part_dena,  \
                   ctx->part_denc)
    if (!stats) {
        if (passes <= 1) GHMM_GPOST_BWD_POST(1);
        else if (passes <= 2) GHMM_GPOST_BWD_POST(2);
        else if (passes <= 4) GHMM_GPOST_BWD_POST(4);
        else GHMM_GPOST_BWD_POST(8);
    } else {
        if (passes <= 1) GHMM_GPOST_BWD_STATS(1);
        else if (passes <= 2) GHMM_GPOST_BWD_STATS(2);
        else if (passes <= 4) GHMM_GPOST_BWD_STATS(4);
        else GHMM_GPOST_BWD_STATS(8);
    }
#undef GHMM_GPOST_BWD_STATS
#undef GHMM_GPOST_BWD_POST
#undef GHMM_GPOST_BWD
    return launch_ok("k_gpost_bwd");
}

// The word posteriors under a grammar behind their emission launches (U > 0, grammar_check passed): the
// lattice's two launches (gpost_launches, the posteriors form), then log P, occ and (if asked for) ent to
// the host.  The workspace's bookkeeping is embed_lattice's: it belongs to the concatenated vocabulary,
// holds log b, gamma and log P, and alpha, beta and c_t are nobody's.  Waits for the stream.  Called by
// ghmm_grammar_post_streams and ghmm_grammar_post_full_streams; it knows no kind of Gaussian.
static int vocab_grammar_post(ghmm_ctx *ctx, const vocab_pass &v, int K, const ghmm_corpus *c, const double *start,
                              const double *pair, const double *fin, double *occ_host, double *ent_host,
                              double *loglik_host)
{
    int rc;
    const size_t KK = (size_t)K * K, F = (size_t)c->F, NS = (size_t)v.NS, FK = F * K;
    if ((rc = ctx->em_la.grow(F * NS + 1)) || (rc = ctx->gamma.grow(F * NS)) || (rc = ctx->gp_x.grow(FK + 1)) ||
        (rc = ctx->gp_occ.grow(FK + 1)) || (rc = ctx->gp_ent.grow(FK + 1)) ||
        (rc = ctx->gr_tab.grow(2 * KK + 2 * (size_t)K)))
        return rc;
    ws_disown(ctx);
    ctx->em_c = c;
    ctx->b_is_log = true;
    ctx->N = v.NS;
    ctx->embed_ws = true;
    ctx->fix_counted = false;
    if ((rc = gpost_launches(ctx, v, K, c, start, pair, fin, false, gpost_posts{}))) return rc;
    HIP_TRY(hipMemcpyAsync(loglik_host, ctx->loglik, (size_t)c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (ent_host && (rc = d2h_pageable(ctx, ent_host, ctx->gp_ent, FK * 8))) return rc;
    return d2h_pageable(ctx, occ_host, ctx->gp_occ, FK * 8);
}

// ------------------------------------------------ forced alignment

// What align_check works out of a call's transcripts for vocab_align: the utterances' back-pointer
// offsets (rows of S_u bytes: poff[u] = the sum of T * S over the utterances before u), their total, and
// the largest S_u among the utterances of at least one frame (the launch's LDS and waves).
struct align_plan {
    std::vector<long long> poff;
    long long psi_bytes = 0;
    int Smax = 0;
};

// The forced alignment's own refusals, behind the vocabulary checks that filled v and before anything is
// launched, grown or written (U > 0, both transcript arrays present): the transcripts' shape and words,
// and what k_align holds (a word's states in six bits of its state table, an utterance's composite
// states in LDS).  An utterance of no frames may have any transcript of known words, an empty one
// included: no lattice is built for it.  Called by ghmm_align_streams and ghmm_align_full_streams.
template <class Model>
static int align_check(Model *const *models, int n_models, int P, const ghmm_corpus *c, const vocab_pass &v,
                       const int32_t *seq, const int32_t *seq_off, const char *what, align_plan *pl)
{
    if (seq_off[0] != 0) {
        ghmm_set_error("%s: seq_off[0] is %d, not 0", what, (int)seq_off[0]);
        return GHMM_ERR_ARG;
    }
    for (int u = 0; u < c->U; u++)
        if (seq_off[u + 1] < seq_off[u]) {
            ghmm_set_error("%s: seq_off decreases at utterance %d", what, u);
            return GHMM_ERR_ARG;
        }
    for (int32_t n = 0; n < seq_off[c->U]; n++)
        if (seq[n] < 0 || seq[n] >= n_models) {
            ghmm_set_error("%s: transcript entry %d is word %d of a vocabulary of %d", what, (int)n, (int)seq[n],
                           n_models);
            return GHMM_ERR_ARG;
        }
    for (int u = 0; u < c->U; u++)
        if (c->len[u] > 0 && seq_off[u + 1] == seq_off[u]) {
            ghmm_set_error("%s: utterance %d has %d frames and an empty transcript", what, u, (int)c->len[u]);
            return GHMM_ERR_ARG;
        }
    if (v.Nmax > 64) {
        ghmm_set_error("%s: a word of %d states: the alignment lattice takes 64", what, v.Nmax);
        return GHMM_ERR_UNSUPPORTED;
    }
    pl->poff.assign((size_t)c->U, 0);
    pl->psi_bytes = 0;
    pl->Smax = 0;
    for (int u = 0; u < c->U; u++) {
        pl->poff[u] = pl->psi_bytes;
        if (c->len[u] <= 0) continue;
        long long S = 0;
        for (int32_t n = seq_off[u]; n < seq_off[u + 1]; n++) S += models[(size_t)seq[n] * P]->N;
        if (S > ALIGN_MAX_S) {
            ghmm_set_error("%s: utterance %d: its transcript has %lld states, the alignment lattice takes %d", what,
                           u, S, ALIGN_MAX_S);
            return GHMM_ERR_UNSUPPORTED;
        }
        pl->Smax = std::max(pl->Smax, (int)S);
        pl->psi_bytes += (long long)c->len[u] * S;
    }
    return GHMM_OK;
}

// The forced alignment behind its emission launches (U > 0, align_check passed): the call's tables
// (poff[U] | seq_off[U + 1] | seq) into the context's al_tab ahead of the launch on the same stream, then
// k_align, one workgroup per utterance, lattice and trace in ONE launch on the log b[F][NS] in the
// workspace; then the scores (bt_ll[U]), the word per frame and, in one byte per frame, the state (bits
// 0..5) with the begin mark (bit 7), which the host takes apart.  The back-pointers and the word per frame
// go through the connected-word decoder's scratch (cn_psi, cn_word): both calls write what they read.
// One stream wait.
static int vocab_align(ghmm_ctx *ctx, const vocab_pass &v, const ghmm_corpus *c, const align_plan &pl,
                       const int32_t *seq, const int32_t *seq_off, int32_t *word_host, int32_t *path_host,
                       int32_t *begin_host, double *score_host)
{
    int rc;
    static_assert(sizeof(int) == sizeof(int32_t), "the transcripts and word_host are the device's ints");
    const size_t U = (size_t)c->U, n_seq = (size_t)seq_off[c->U];
    const size_t off_at = U * 8, seq_at = off_at + (U + 1) * 4, tab_bytes = seq_at + n_seq * 4;
    if ((rc = ctx->cn_psi.grow((size_t)pl.psi_bytes + 16)) || (rc = ctx->cn_word.grow((size_t)c->F)) ||
        (rc = ctx->path.grow((size_t)c->F)) || (rc = ctx->bt_ll.grow(U)) || (rc = ctx->al_tab.grow(tab_bytes)))
        return rc;
    // (pageable sources: the copies complete before the calls return them)
    HIP_TRY(hipMemcpyAsync(ctx->al_tab, pl.poff.data(), U * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->al_tab + off_at, seq_off, (U + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_seq) HIP_TRY(hipMemcpyAsync(ctx->al_tab + seq_at, seq, n_seq * 4, hipMemcpyHostToDevice, ctx->stream));
    const int Smax = std::max(pl.Smax, 1);
    const size_t lds = align_lds(Smax);
    if (lds > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_align))) return rc;
    const int threads = std::min(CONNECT_THREADS, ((Smax + WAVE - 1) / WAVE) * WAVE);
    {
        kscope ks(ctx, GHMM_K_VITERBI);
        hipLaunchKernelGGL(k_align, dim3((unsigned)c->U), dim3((unsigned)threads), lds, ctx->stream, c->U, v.NS, v.dtab,
                           (const double *)ctx->b, c->off, (const long long *)ctx->al_tab.p,
                           (const int *)(ctx->al_tab + off_at), (const int *)(ctx->al_tab + seq_at), ctx->cn_psi,
                           ctx->cn_word, ctx->path, ctx->bt_ll, c->order, Smax);
    }
    if ((rc = launch_ok("k_align"))) return rc;
    HIP_TRY(hipMemcpyAsync(score_host, ctx->bt_ll, U * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (c->F) {
        HIP_TRY(hipMemcpyAsync(word_host, ctx->cn_word, (size_t)c->F * 4, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = d2h_pageable(ctx, path_host, ctx->path, (size_t)c->F, true))) return rc;
        for (long long f = 0; f < c->F; f++) {
            begin_host[f] = path_host[f] >> 7;
            path_host[f] &= 63;
        }
    } else
        HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

// ------------------------------------------------ embedded Baum-Welch

// The embedded E-step's lattice behind its emission launches (U > 0, align_check passed; pl.poff counts
// la entries here: rows of S_u doubles): the call's tables (poff[U] | seq_off[U + 1] | seq, then from the
// next 16-byte boundary the caller's n_dst scatter entries, returned in *ddst) into the context's al_tab
// ahead of the launches on the same stream, then k_embed_fwd (la rows into em_la, log P_u into loglik,
// log Z_u into logk) and k_embed_bwd (the tied gamma[F][NS] and one partial per utterance for a model of
// NS states, as run_log_lattice leaves them for the statistics launches).  Both launches count under
// GHMM_K_FORWARD.  Nothing waits.  Called by embed_lattice (below) for ghmm_estep_embed_streams and
// ghmm_estep_embed_full_streams; it knows no kind of Gaussian.
static int vocab_embed(ghmm_ctx *ctx, const vocab_pass &v, const ghmm_corpus *c, const align_plan &pl,
                       const int32_t *seq, const int32_t *seq_off, const embed_dst *dst, size_t n_dst,
                       const embed_dst **ddst)
{
    int rc;
    static_assert(sizeof(int) == sizeof(int32_t), "the transcripts are the device's ints");
    const size_t U = (size_t)c->U, n_seq = (size_t)seq_off[c->U], NS = (size_t)v.NS;
    const size_t off_at = U * 8, seq_at = off_at + (U + 1) * 4, dst_at = ((seq_at + n_seq * 4 + 15) / 16) * 16;
    const size_t tab_bytes = dst_at + n_dst * sizeof(embed_dst);
    if ((rc = ctx->em_la.grow((size_t)pl.psi_bytes + 1)) || (rc = ctx->em_head.grow(U * NS)) ||
        (rc = ctx->gamma.grow((size_t)c->F * NS)) || (rc = ctx->logk.grow(U)) ||
        (rc = ctx->part_xi.grow(U * NS * (MAX_DELTA + 1))) || (rc = ctx->part_dena.grow(U * NS)) ||
        (rc = ctx->part_denc.grow(U * NS)) || (rc = ctx->al_tab.grow(tab_bytes)))
        return rc;
    // (pageable sources: the copies complete before the calls return them)
    HIP_TRY(hipMemcpyAsync(ctx->al_tab, pl.poff.data(), U * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->al_tab + off_at, seq_off, (U + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_seq) HIP_TRY(hipMemcpyAsync(ctx->al_tab + seq_at, seq, n_seq * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->al_tab + dst_at, dst, n_dst * sizeof(embed_dst), hipMemcpyHostToDevice, ctx->stream));
    *ddst = (const embed_dst *)(ctx->al_tab + dst_at);
    const int Smax = std::max(pl.Smax, 1);
    const size_t lds_f = embed_fwd_lds(Smax), lds_b = embed_bwd_lds(Smax);
    const int threads = std::min(EMBED_THREADS, ((Smax + WAVE - 1) / WAVE) * WAVE);
    const int passes = (Smax + threads - 1) / threads;
    const long long *dpoff = (const long long *)ctx->al_tab.p;
    const int *dseq_off = (const int *)(ctx->al_tab + off_at), *dseq = (const int *)(ctx->al_tab + seq_at);
#define GHMM_EMBED_FWD(PS)                                                                                         \
    do {                                                                                                           \
        if (lds_f > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_embed_fwd<PS>))) return rc;                 \
        kscope ks(ctx, GHMM_K_FORWARD);                                                                            \
        hipLaunchKernelGGL(k_embed_fwd<PS>, dim3((unsigned)c->U), dim3((unsigned)threads), lds_f, ctx->stream, c->U, \
                           v.NS, v.dtab, (const double *)ctx->b, c->off, dpoff, dseq_off, dseq, ctx->em_la,        \
                           ctx->loglik, ctx->logk, c->order, Smax);                                                \
    } while (0)
    if (passes <= 1) GHMM_EMBED_FWD(1);
    else if (passes <= 2) GHMM_EMBED_FWD(2);
    else if (passes <= 4) GHMM_EMBED_FWD(4);
    else GHMM_EMBED_FWD(8);
#undef GHMM_EMBED_FWD
    if ((rc = launch_ok("k_embed_fwd"))) return rc;
#define GHMM_EMBED_BWD(PS)                                                                                         \
    do {                                                                                                           \
        if (lds_b > (48u << 10) && (rc = lds_attr(ctx, (const void *)k_embed_bwd<PS>))) return rc;                 \
        kscope ks(ctx, GHMM_K_FORWARD);                                                                            \
        hipLaunchKernelGGL(k_embed_bwd<PS>, dim3((unsigned)c->U), dim3((unsigned)threads), lds_b, ctx->stream, c->U, \
                           v.NS, (int)ctx->delta, v.dtab, (const double *)ctx->b, c->off, dpoff, dseq_off, dseq,   \
                           (const double *)ctx->em_la, (const double *)ctx->logk, ctx->gamma, ctx->part_xi,        \
                           ctx->part_dena, ctx->part_denc, ctx->em_head, c->order, Smax);                          \
    } while (0)
    if (passes <= 1) GHMM_EMBED_BWD(1);
    else if (passes <= 2) GHMM_EMBED_BWD(2);
    else if (passes <= 4) GHMM_EMBED_BWD(4);
    else GHMM_EMBED_BWD(8);
#undef GHMM_EMBED_BWD
    if ((rc = launch_ok("k_embed_bwd"))) return rc;
    ctx->slots = c->U; // one partial per utterance
    ctx->loglik_pieces = false;
    return GHMM_OK;
}

// An embedded E-step on a corpus of no utterances: every sum is empty, loglik and n_utt are 0.  Called by
// the embedded E-steps of both kinds, behind their checks.
static int embed_empty(ghmm_ctx *ctx, ghmm_stats *const *stats, int n)
{
    for (int k = 0; k < n; k++) {
        stats[k]->mbox_valid = false;
        HIP_TRY(hipMemsetAsync(stats[k]->v, 0, stats[k]->n * 8, ctx->stream));
    }
    return GHMM_OK;
}

// An embedded E-step between its emission launches and its statistics launches, the same for both kinds
// of Gaussian (M0 = stream 0's mixtures): the workspace's bookkeeping, the scatter's table (stream p's
// n_models entries from (*ddst)[p * n_models]: word k's vector, states and first column) and the lattice.
template <class Model>
static int embed_lattice(ghmm_ctx *ctx, Model *const *models, int n_models, int P, int M0, const ghmm_corpus *c,
                         const vocab_pass &v, const align_plan &pl, const int32_t *seq, const int32_t *seq_off,
                         ghmm_stats *const *stats, const embed_dst **ddst)
{
    // the workspace belongs to the concatenated vocabulary: the row API does not reuse it, and what an
    // earlier pass left in alpha, beta and c_t goes with nothing here
    ws_disown(ctx);
    ctx->em_c = c;
    ctx->b_is_log = true;
    ctx->post_valid = P == 1;
    ctx->N = v.NS;
    ctx->G = v.NS * M0;
    ctx->embed_ws = true;
    ctx->fix_counted = false; // (the word lattice runs in the log domain: no utterance is taken again)
    std::vector<embed_dst> dst((size_t)n_models * P);
    for (int p = 0; p < P; p++) {
        int bo = 0;
        for (int k = 0; k < n_models; k++) {
            const Model *m = models[(size_t)k * P + p];
            dst[(size_t)p * n_models + k] = {stats[(size_t)k * P + p]->v, m->N, bo};
            bo += m->N;
        }
    }
    return vocab_embed(ctx, v, c, pl, seq, seq_off, dst.data(), dst.size(), ddst);
}

// ------------------------------------------------ Baum-Welch statistics on the grammar lattice

// The grammar E-step between its emission launches and its statistics launches (U > 0, grammar_check and the
// stats checks passed; M0 = stream 0's mixtures): the workspace's bookkeeping, which is embed_lattice's; the
// scatter's table (stream p's n_models entries from (*ddst)[p * n_models]: word k's vector, states and first
// column) into the context's al_tab ahead of the launches on the same stream; then the lattice's two launches
// in the statistics form (gpost_launches), which leave gamma[F][NS], log P_u and one partial per utterance for
// a model of NS states, as vocab_embed leaves them for the statistics launches.  Nothing waits.  Called by
// ghmm_estep_grammar_streams; it knows no kind of Gaussian.
template <class Model>
static int vocab_grammar_stats(ghmm_ctx *ctx, Model *const *models, int n_models, int P, int M0, const ghmm_corpus *c,
                               const vocab_pass &v, const double *start, const double *pair, const double *fin,
                               ghmm_stats *const *stats, const embed_dst **ddst)
{
    int rc;
    const int K = n_models;
    const size_t KK = (size_t)K * K, F = (size_t)c->F, NS = (size_t)v.NS, U = (size_t)c->U;
    std::vector<embed_dst> dst((size_t)n_models * P);
    for (int p = 0; p < P; p++) {
        int bo = 0;
        for (int k = 0; k < n_models; k++) {
            const Model *m = models[(size_t)k * P + p];
            dst[(size_t)p * n_models + k] = {stats[(size_t)k * P + p]->v, m->N, bo};
            bo += m->N;
        }
    }
    if ((rc = ctx->em_la.grow(F * NS + 1)) || (rc = ctx->gamma.grow(F * NS)) || (rc = ctx->gp_x.grow(F * K + 1)) ||
        (rc = ctx->gr_tab.grow(2 * KK + 2 * (size_t)K)) || (rc = ctx->part_xi.grow(U * NS * (MAX_DELTA + 1))) ||
        (rc = ctx->part_dena.grow(U * NS)) || (rc = ctx->part_denc.grow(U * NS)) ||
        (rc = ctx->al_tab.grow(dst.size() * sizeof(embed_dst))))
        return rc;
    ws_disown(ctx);
    ctx->em_c = c;
    ctx->b_is_log = true;
    ctx->post_valid = P == 1;
    ctx->N = v.NS;
    ctx->G = v.NS * M0;
    ctx->embed_ws = true;
    ctx->fix_counted = false; // (the lattice runs in the log domain: no utterance is taken again)
    // (a pageable source: the copy completes before the call returns it)
    HIP_TRY(hipMemcpyAsync(ctx->al_tab, dst.data(), dst.size() * sizeof(embed_dst), hipMemcpyHostToDevice,
                           ctx->stream));
    *ddst = (const embed_dst *)ctx->al_tab.p;
    // the posteriors the statistics launches will read: an utterance without a finite log P has its rows zeroed
    static_assert(GPOST_MAX_STREAMS == GHMM_MAX_STREAMS, "the kernel's view holds every stream");
    gpost_posts posts{};
    posts.P = P;
    for (int p = 0; p < P; p++) {
        posts.post[p] = P == 1 ? ctx->post.p : ctx->post_s[p].p;
        posts.M[p] = models[p]->M;
    }
    if ((rc = gpost_launches(ctx, v, K, c, start, pair, fin, true, posts))) return rc;
    ctx->slots = c->U; // one partial per utterance
    ctx->loglik_pieces = false;
    return GHMM_OK;
}
