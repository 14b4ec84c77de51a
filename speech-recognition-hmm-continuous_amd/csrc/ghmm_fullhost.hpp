// ghmm_fullhost.hpp — the host side of the full-covariance entry points (recogniser RC, trainer TFF):
// models, checks, launches of the kernels in ghmm_fullcov.hpp.  Part of ghmm_hip.hip's translation
// unit, included once at its end: it uses that file's context and workspace, the checks, tables and
// lattice launches both model kinds share (ghmm_lattice_host.hpp) and the RCCL table resolved there.

// ------------------------------------------------ the full-covariance recogniser (RC)

struct GHMM_LOCAL ghmm_fmodel {
    int N = 0, M = 0, D = 0;
    // what the shared recursions of ghmm_estep_full read (run_forward / run_backward /
    // run_scan_combine): N, and A (the model's transitions: they live here) with its band flag.
    // Nothing else of it is set; it is never passed to ghmm_model_destroy.
    ghmm_model rec;
    dev_buf<double> &A = rec.A;
    dev_buf<double> c, mean, inv_cov, det;
    dev_buf<double> den; // pow(2 pi, D/2) * sqrt(|det|) per Gaussian (RC:921-931)
    // ghmm_viterbi_full: log(c) - log(den) per Gaussian, and A > 0 ? log(A) : -inf, both formed on
    // the host (the oracle's expressions, evaluated by the same libm)
    dev_buf<double> lk, logA;
};

// any N (the concatenated vocabulary of ghmm_score_full_batch has hundreds of states)
static int fmodel_alloc(ghmm_ctx *ctx, int N, int M, int D, ghmm_fmodel **out)
{
    ghmm_fmodel *fm = new (std::nothrow) ghmm_fmodel();
    if (!fm) return GHMM_ERR_ALLOC;
    fm->N = N; fm->M = M; fm->D = D;
    fm->rec.N = N; fm->rec.M = M; fm->rec.D = D;
    const size_t G = (size_t)N * M;
    // mean and inv_cov with FC_SLACK doubles behind them: the kernel's padded columns read there
    const size_t nmean = G * D + FC_SLACK, ncov = G * D * D + FC_SLACK;
    int rc;
    if ((rc = fm->A.alloc((size_t)N * N)) || (rc = fm->c.alloc(G)) ||
        (rc = fm->mean.alloc(nmean)) || (rc = fm->inv_cov.alloc(ncov)) ||
        (rc = fm->det.alloc(G)) || (rc = fm->den.alloc(G)) || (rc = fm->lk.alloc(G)) ||
        (rc = fm->logA.alloc((size_t)N * N))) {
        ghmm_fmodel_destroy(ctx, fm);
        return rc;
    }
    if (hipMemsetAsync(fm->mean, 0, nmean * 8, ctx->stream) != hipSuccess ||
        hipMemsetAsync(fm->inv_cov, 0, ncov * 8, ctx->stream) != hipSuccess) {
        ghmm_fmodel_destroy(ctx, fm);
        ghmm_set_error("hipMemsetAsync failed");
        return GHMM_ERR_HIP;
    }
    *out = fm;
    return GHMM_OK;
}

extern "C" int ghmm_fmodel_create(ghmm_ctx *ctx, int N, int M, int D, ghmm_fmodel **out)
{
    int rc = use(ctx);
    if (rc) return rc;
    ARG_CHECK(out, "null output");
    *out = nullptr;
    ARG_CHECK(N > 0 && M > 0 && D > 0, "N, M and D must be positive");
    if (N > 64 || D > FC_DMAX) {
        ghmm_set_error("full-covariance models take up to 64 states and %d coefficients (asked: %d states, "
                       "%d coefficients)", FC_DMAX, N, D);
        return GHMM_ERR_UNSUPPORTED;
    }
    return fmodel_alloc(ctx, N, M, D, out);
}

extern "C" void ghmm_fmodel_destroy(ghmm_ctx *ctx, ghmm_fmodel *fm)
{
    if (!fm) return;
    if (ctx && ctx->last_m == &fm->rec) ctx->last_m = nullptr;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete fm; // (a partly built one too: its buffers free themselves)
}

extern "C" int ghmm_fmodel_set(ghmm_ctx *ctx, ghmm_fmodel *fm, const double *A, const double *c,
                               const double *mean, const double *inv_cov, const double *det)
{
    int rc = use(ctx);
    if (ctx && fm && ctx->last_m == &fm->rec) ctx->last_m = nullptr; // alpha^ / W belong to the old parameters
    if (rc) return rc;
    ARG_CHECK(fm && A && c && mean && inv_cov && det, "null argument");
    const size_t G = (size_t)fm->N * fm->M, NN = (size_t)fm->N * fm->N;
    fm->rec.banded = true; // (as ghmm_model_set decides it: the paired scans' band-diagonal forms)
    for (int i = 0; i < fm->N; i++)
        for (int j = 0; j < fm->N; j++)
            if (A[(size_t)i * fm->N + j] != 0.0 && j != i && j != i + 1) fm->rec.banded = false;
    // calc_gaus's normaliser as the reference forms it: aux1 = pow(2 pi, D/2.0), aux2 = pow(|det|, 0.5)
    std::vector<double> den(G), lk(G), logA(NN);
    const double aux1 = pow(2.0 * M_PI, fm->D / 2.0);
    for (size_t g = 0; g < G; g++) {
        den[g] = aux1 * pow(fabs(det[g]), 0.5);
        lk[g] = log(c[g]) - log(den[g]);
    }
    for (size_t k = 0; k < NN; k++) logA[k] = A[k] > 0.0 ? log(A[k]) : -INFINITY;
    HIP_TRY(hipMemcpyAsync(fm->A, A, NN * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->c, c, G * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->mean, mean, G * fm->D * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->inv_cov, inv_cov, G * fm->D * fm->D * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->det, det, G * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->den, den.data(), G * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->lk, lk.data(), G * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fm->logA, logA.data(), NN * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(stream_sync(ctx)); // (pageable sources)
    return GHMM_OK;
}

extern "C" int ghmm_fmodel_get(ghmm_ctx *ctx, ghmm_fmodel *fm, double *A, double *c, double *mean,
                               double *inv_cov, double *det)
{
    int rc = use(ctx);
    if (rc) return rc;
    ARG_CHECK(fm, "null model");
    const size_t G = (size_t)fm->N * fm->M, NN = (size_t)fm->N * fm->N;
    if (A) HIP_TRY(hipMemcpyAsync(A, fm->A, NN * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (c) HIP_TRY(hipMemcpyAsync(c, fm->c, G * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, fm->mean, G * fm->D * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (inv_cov)
        HIP_TRY(hipMemcpyAsync(inv_cov, fm->inv_cov, G * fm->D * fm->D * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (det) HIP_TRY(hipMemcpyAsync(det, fm->det, G * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

extern "C" int ghmm_fmodel_dims(const ghmm_fmodel *fm, int *N, int *M, int *D)
{
    ARG_CHECK(fm, "null model");
    if (N) *N = fm->N;
    if (M) *M = fm->M;
    if (D) *D = fm->D;
    return GHMM_OK;
}

static int check_full(ghmm_ctx *ctx, const ghmm_fmodel *fm, const ghmm_corpus *c)
{
    if (!fm || !c) {
        ghmm_set_error("null model or corpus");
        return GHMM_ERR_ARG;
    }
    if (fm->D != c->D) {
        ghmm_set_error("model has %d coefficients per frame, corpus has %d", fm->D, c->D);
        return GHMM_ERR_ARG;
    }
    if (ctx->robust) {
        ghmm_set_error("GHMM_OPT_ROBUST is not available with full-covariance models");
        return GHMM_ERR_UNSUPPORTED;
    }
    return GHMM_OK;
}

// one k_emission_full launch; post only where MODE writes posteriors, lk only where it works in logs.
// FOLD: a later feature stream's launch, which combines with the b of the streams before it
template <int DB, int MODE, bool FOLD>
static void launch_emission_full(ghmm_ctx *ctx, const ghmm_fmodel *fm, const ghmm_corpus *c, double *post)
{
    constexpr bool POST = MODE == FC_POST || MODE == FC_LOGPOST, LOG = MODE == FC_LOG || MODE == FC_LOGPOST;
    const int nch = (fm->N + FC_SC - 1) / FC_SC;
    const dim3 grid((unsigned)((c->F + WAVE - 1) / WAVE), (unsigned)((nch + FC_WAVES - 1) / FC_WAVES));
    const size_t lds = (size_t)fc_lds_doubles(fm->D) * sizeof(double);
    hipLaunchKernelGGL((k_emission_full<DB, MODE, FOLD>), grid, dim3(FC_WAVES * WAVE), lds, ctx->stream, fm->N, fm->M,
                       fm->D, c->F, c->X, fm->mean, fm->inv_cov, fm->den, fm->c, ctx->b,
                       POST ? post : (double *)nullptr, LOG ? fm->lk : (const double *)nullptr);
}

template <int DB, bool FOLD>
static void emission_full_by_mode(ghmm_ctx *ctx, const ghmm_fmodel *fm, const ghmm_corpus *c, int mode, double *post)
{
    switch (mode) {
    case FC_POST: launch_emission_full<DB, FC_POST, FOLD>(ctx, fm, c, post); break;
    case FC_LOGPOST: launch_emission_full<DB, FC_LOGPOST, FOLD>(ctx, fm, c, post); break;
    case FC_LOG: launch_emission_full<DB, FC_LOG, FOLD>(ctx, fm, c, post); break;
    default: launch_emission_full<DB, FC_LIN, FOLD>(ctx, fm, c, post); break;
    }
}

template <bool FOLD>
static void emission_full_by_db(ghmm_ctx *ctx, const ghmm_fmodel *fm, const ghmm_corpus *c, int mode, double *post)
{
    switch ((fm->D + 7) / 8 * 8) {
    case 8: emission_full_by_mode<8, FOLD>(ctx, fm, c, mode, post); break;
    case 16: emission_full_by_mode<16, FOLD>(ctx, fm, c, mode, post); break;
    case 24: emission_full_by_mode<24, FOLD>(ctx, fm, c, mode, post); break;
    case 32: emission_full_by_mode<32, FOLD>(ctx, fm, c, mode, post); break;
    case 40: emission_full_by_mode<40, FOLD>(ctx, fm, c, mode, post); break;
    default: emission_full_by_mode<48, FOLD>(ctx, fm, c, mode, post); break;
    }
}

// mode: FC_LIN (b), FC_POST (b and the mixture posteriors), FC_LOG (log b), FC_LOGPOST (log b and
// the mixture posteriors).  stream_post: a model of several feature streams (emission_full_streams);
// stream p's posteriors go there, and p > 0 (`fold`) multiplies into, or adds onto, the b in the workspace
static int run_emission_full(ghmm_ctx *ctx, const ghmm_fmodel *fm, const ghmm_corpus *c, int mode = FC_LIN,
                             bool fold = false, double *stream_post = nullptr)
{
    if (!fold) {
        ws_disown(ctx);
        ctx->em_c = c;
        ctx->b_is_log = mode == FC_LOG || mode == FC_LOGPOST;
        ctx->post_valid = !stream_post && (mode == FC_POST || mode == FC_LOGPOST);
    }
    if (c->F == 0) return GHMM_OK;
    kscope ks(ctx, GHMM_K_EMISSION);
    double *post = stream_post ? stream_post : ctx->post;
    if (fold) emission_full_by_db<true>(ctx, fm, c, mode, post);
    else emission_full_by_db<false>(ctx, fm, c, mode, post);
    return launch_ok("k_emission_full");
}

extern "C" int ghmm_emission_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c)
{
    int rc = use(ctx);
    if (rc || (rc = check_full(ctx, fm, c))) return rc;
    if ((rc = ws_full(ctx, fm->N, fm->M, c))) return rc;
    return run_emission_full(ctx, fm, c);
}

// calc_alpha + calc_probability without the final-state term (RC:733-836) on the b in the workspace:
// k_scan_pair's only = 3; the scores to the host
static int run_score_full(ghmm_ctx *ctx, const ghmm_fmodel *fm, const ghmm_corpus *c, double *loglik_host)
{
    int rc;
    const lane_grid lg(fm->N, c->U);
    {
        kscope ks(ctx, GHMM_K_FORWARD);
        GHMM_BY_LANES(lg.L, hipLaunchKernelGGL(k_scan_pair<LL>, dim3(lg.blocks, 1u), dim3(WAVE), 0, ctx->stream, fm->N,
                                               c->U, 3, fm->A, ctx->b, c->off, ctx->alpha, ctx->scale, ctx->sinv,
                                               (const double *)nullptr, ctx->loglik, ctx->wrow, ctx->sb, ctx->sink,
                                               c->order));
    }
    if ((rc = launch_ok("k_scan_pair"))) return rc;
    HIP_TRY(hipMemcpyAsync(loglik_host, ctx->loglik, (size_t)c->U * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_sync(ctx));
    return GHMM_OK;
}

extern "C" int ghmm_score_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, double *loglik_host)
{
    int rc = use(ctx);
    if (rc || (rc = check_full(ctx, fm, c))) return rc;
    ARG_CHECK(loglik_host || c->U == 0, "null destination");
    if ((rc = ws_full(ctx, fm->N, fm->M, c)) || (rc = run_emission_full(ctx, fm, c))) return rc;
    if (c->U == 0) return GHMM_OK;
    return run_score_full(ctx, fm, c, loglik_host);
}

// A vocabulary call up to its one launch, on P feature streams (models[k * P + p] = stream p of word k,
// corpora[p] = stream p of the utterances; the single-stream calls pass P = 1).  The shared checks
// (vocab_checks; `what` = the entry point's name in their texts), then, unless the corpus is empty (the
// caller returns), the pass's tables (vocab_tables: dtab[k].A = word k's A under FC_LIN, its log A under
// FC_LOG), per stream the concatenated vocabulary (NS states, transitions unused; ctx->fbt_cat[p],
// cat_slot) with every word's Gaussians of that stream gathered into it by one launch, and the
// vocabulary's b or log b in the workspace: one emission launch per stream over its concatenated
// vocabulary, stream 0 plain, every later stream folded into the same b[F][NS].  The FOLD epilogue is per
// state, so column bo_k + i holds what emission_full_streams leaves in column i for word k alone.  Under
// FC_LOGPOST (the embedded E-step) the same launches also write the mixture posteriors, the table holds
// log A as under FC_LOG.  The launch that follows writes bt_ll.
static int fvocab_begin(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *const *corpora, int P,
                        bool have_dest, int mode, const char *what, vocab_pass *v)
{
    int rc = use(ctx);
    if (rc) return rc;
    rc = vocab_checks(models, n_models, corpora, P, have_dest, what,
                      [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); }, v);
    if (rc || corpora[0]->U == 0) return rc;
    const ghmm_corpus *c = corpora[0];
    if ((rc = ctx->bt_ll.grow((size_t)n_models * c->U))) return rc;
    const fgather_src *dsrc;
    const bool want_post = mode == FC_POST || mode == FC_LOGPOST;
    rc = vocab_tables<fgather_src>(ctx, models, n_models, P, mode == FC_LOG || mode == FC_LOGPOST,
                                   [](const ghmm_fmodel *m, int g0) {
        return fgather_src{m->c, m->mean, m->inv_cov, m->den, m->lk, g0, m->N * m->M};
    }, v, &dsrc);
    if (rc) return rc;
    for (int p = 0; p < P; p++) {
        const int NS = v->NS, M = models[p]->M, D = models[p]->D;
        rc = cat_slot(ctx, &ctx->fbt_cat[p], NS, M, D, ghmm_fmodel_destroy,
                      [=](ghmm_fmodel **slot) { return fmodel_alloc(ctx, NS, M, D, slot); });
        if (rc) return rc;
        ghmm_fmodel *cat = ctx->fbt_cat[p];
        hipLaunchKernelGGL(k_gather_fmodels, dim3((unsigned)n_models), dim3(256), 0, ctx->stream, D,
                           dsrc + (size_t)p * n_models, cat->c, cat->mean, cat->inv_cov, cat->den, cat->lk);
        if ((rc = launch_ok("k_gather_fmodels"))) return rc;
    }
    if ((rc = ws_full(ctx, v->NS, models[0]->M, c))) return rc;
    // the posteriors of a mode that writes them: one stream's into the workspace's own buffer, which
    // ghmm_fetch serves, several streams' into post_s[p] (as ghmm_estep_full_streams keeps them)
    for (int p = 0; want_post && p < P; p++) {
        dev_buf<double> &post = P == 1 ? ctx->post : ctx->post_s[p];
        if ((rc = post.grow((size_t)c->F * v->NS * models[p]->M))) return rc;
    }
    for (int p = 0; p < P; p++)
        if ((rc = run_emission_full(ctx, ctx->fbt_cat[p], corpora[p], mode, p > 0,
                                    want_post && P > 1 ? ctx->post_s[p].p : nullptr)))
            return rc;
    return GHMM_OK;
}

// the linear score of a vocabulary: no final-state term, nobody reads c_t (the sink takes them)
static int fvocab_score(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *const *corpora, int P,
                        double *loglik_host, const char *what)
{
    vocab_pass v;
    int rc = fvocab_begin(ctx, models, n_models, corpora, P, loglik_host != nullptr, FC_LIN, what, &v);
    if (rc || corpora[0]->U == 0) return rc;
    if ((rc = vocab_forward(ctx, v, n_models, corpora[0], ctx->sink, ctx->sink, 0))) return rc;
    return vocab_scores_out(ctx, n_models, corpora[0], loglik_host);
}

extern "C" int ghmm_score_full_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *c,
                                     double *loglik_host)
{
    return fvocab_score(ctx, models, n_models, &c, 1, loglik_host, __func__);
}

// ------------------------------------------------ the full-covariance Viterbi

extern "C" int ghmm_viterbi_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, int32_t *path_host,
                                 double *score_host)
{
    int rc = use(ctx);
    if (rc || (rc = check_full(ctx, fm, c))) return rc;
    ARG_CHECK((path_host && score_host) || c->U == 0, "null destination");
    if (c->U == 0) return GHMM_OK;
    if ((rc = ws_full(ctx, fm->N, fm->M, c)) || (rc = viterbi_ws(ctx, c, lane_grid(fm->N, c->U).L))) return rc;
    if ((rc = run_emission_full(ctx, fm, c, FC_LOG))) return rc;
    return run_viterbi_lanes(ctx, fm->N, fm->logA, c, path_host, score_host);
}

static int fvocab_viterbi(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *const *corpora, int P,
                          double *score_host, const char *what)
{
    vocab_pass v;
    int rc = fvocab_begin(ctx, models, n_models, corpora, P, score_host != nullptr, FC_LOG, what, &v);
    if (rc || corpora[0]->U == 0) return rc;
    if ((rc = vocab_viterbi(ctx, v, n_models, corpora[0]))) return rc;
    return vocab_scores_out(ctx, n_models, corpora[0], score_host);
}

extern "C" int ghmm_viterbi_full_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *c,
                                       double *score_host)
{
    return fvocab_viterbi(ctx, models, n_models, &c, 1, score_host, __func__);
}

// ------------------------------------------------ the full-covariance log-domain forward score

static int emission_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora, int P,
                                 int mode); // (with the several-stream calls, below)

// one word (models[0]'s log A) as a vocabulary of one: its table first, then the streams' log b
static int flogscore_word(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora, int P,
                          int final_state, double *loglik_host)
{
    int rc;
    vocab_pass one;
    ghmm_fmodel *fm = models[0];
    ghmm_corpus *c = corpora[0];
    if ((rc = one_word_table(ctx, fm->logA, fm->N, c, &one))) return rc;
    if (P == 1) {
        if ((rc = ws_full(ctx, fm->N, fm->M, c)) || (rc = run_emission_full(ctx, fm, c, FC_LOG))) return rc;
    } else if ((rc = emission_full_streams(ctx, models, corpora, P, FC_LOG)))
        return rc;
    if ((rc = vocab_logforward(ctx, one, 1, c, final_state))) return rc;
    return vocab_scores_out(ctx, 1, c, loglik_host);
}

extern "C" int ghmm_logscore_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, int final_state,
                                  double *loglik_host)
{
    int rc = use(ctx);
    if (rc || (rc = check_full(ctx, fm, c))) return rc;
    ARG_CHECK(loglik_host || c->U == 0, "null destination");
    if (c->U == 0) return GHMM_OK;
    return flogscore_word(ctx, &fm, &c, 1, final_state, loglik_host);
}

static int fvocab_logscore(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *const *corpora, int P,
                           int final_state, double *loglik_host, const char *what)
{
    vocab_pass v;
    int rc = fvocab_begin(ctx, models, n_models, corpora, P, loglik_host != nullptr, FC_LOG, what, &v);
    if (rc || corpora[0]->U == 0) return rc;
    if ((rc = vocab_logforward(ctx, v, n_models, corpora[0], final_state))) return rc;
    return vocab_scores_out(ctx, n_models, corpora[0], loglik_host);
}

extern "C" int ghmm_logscore_full_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *c,
                                        int final_state, double *loglik_host)
{
    return fvocab_logscore(ctx, models, n_models, &c, 1, final_state, loglik_host, __func__);
}

// ------------------------------------------------ the full-covariance trainer (TFF)

static int check_stats_full(const ghmm_fmodel *fm, const ghmm_stats *s)
{
    if (!s || !s->full || s->N != fm->N || s->M != fm->M || s->D != fm->D) {
        ghmm_set_error("statistics vector is not a full-covariance one of the model's shape "
                       "(ghmm_stats_create_full)");
        return GHMM_ERR_ARG;
    }
    return GHMM_OK;
}

// calc_mix_param over every frame (k_fullstats, from ctx->gamma and the posteriors in post) into *P_out
// frame-block partials in ctx->part_mu
static int run_fullstats_part(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, const double *post, long long *P_out)
{
    const int N = fm->N, M = fm->M, D = fm->D, G = N * M, D1 = D + 1;
    const long long E = (long long)G * fs_elems(D);
    const int NB = (int)((E + FS_THREADS * FS_EPT - 1) / (FS_THREADS * FS_EPT));
    int rc;
    // frame-block partials: about four blocks per CU in all, as k_mixstats
    long long P = ctx->partials > 0 ? ctx->partials : (4LL * ctx->cus + NB - 1) / NB;
    if (P < 1) P = 1;
    int GWmax = (FS_THREADS * FS_EPT) / fs_elems(D) + 2;
    if (GWmax > G) GWmax = G;
    int FSn = FS_FRAMES;
    while (FSn > 1 && (size_t)FSn * (D1 + GWmax) * sizeof(double) > 48 * 1024) FSn /= 2;
    const size_t lds = (size_t)FSn * (D1 + GWmax) * sizeof(double);
    long long fpb = (c->F + P - 1) / P;
    fpb = ((fpb + FSn - 1) / FSn) * FSn;
    if (fpb < FSn) fpb = FSn;
    P = c->F > 0 ? (c->F + fpb - 1) / fpb : 0;
    if (P > 0) {
        if ((rc = ctx->part_mu.grow((size_t)P * (size_t)E))) return rc;
        kscope ks(ctx, GHMM_K_MIXSTATS);
        hipLaunchKernelGGL(k_fullstats, dim3((unsigned)P, (unsigned)NB), dim3(FS_THREADS), lds, ctx->stream, N, M, D,
                           c->F, fpb, FSn, c->X, ctx->gamma, post, fm->mean, ctx->part_mu);
        if ((rc = launch_ok("k_fullstats"))) return rc;
    }
    *P_out = P;
    return GHMM_OK;
}

// the ordered reduction of those partials into num_c / num_mu / num_cov at stats_c
static int run_fullstats_reduce(ghmm_ctx *ctx, const ghmm_fmodel *fm, long long P, double *stats_c)
{
    const int G = fm->N * fm->M;
    const long long E = (long long)G * fs_elems(fm->D);
    hipLaunchKernelGGL(k_fullstats_reduce, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, ctx->stream, G, fm->D,
                       (int)P, (const double *)ctx->part_mu, stats_c);
    return launch_ok("k_fullstats_reduce");
}

// the statistics of an E-step: both of the above, and the utterance sums (num_a, den_a, den_c, log P,
// count) by k_reduce_all without its Gaussian blocks
static int run_fullstats(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_stats *s, const double *post)
{
    const int N = fm->N, M = fm->M, D = fm->D;
    int rc;
    long long P = 0;
    if ((rc = run_fullstats_part(ctx, fm, c, post, &P))) return rc;
    {
        kscope ks(ctx, GHMM_K_REDUCE);
        if ((rc = run_fullstats_reduce(ctx, fm, P, s->v + (size_t)N * N + 2 * (size_t)N))) return rc;
        reduce_args ra{};
        ra.N = N; ra.M = M; ra.D = D; ra.U = c->U; ra.delta = (int)ctx->delta;
        ra.S = ctx->slots;
        ra.lpart = ctx->loglik_pieces ? ctx->lpart : nullptr;
        ra.logk = ctx->logk;
        ra.part_xi = ctx->part_xi; ra.part_dena = ctx->part_dena; ra.part_denc = ctx->part_denc;
        ra.loglik = ctx->loglik; ra.stats = s->v;
        ra.no_mix = 1;
        ra.tail = s->v + (s->n - 2);
        ra.mbox = (s->mbox_slot >= 0 && ctx->mbox_page_dev) ? ctx->mbox_page_dev + 4 * s->mbox_slot : nullptr;
        ra.mbox_seq = ++ctx->mbox_seq;
        s->mbox_expect = ra.mbox_seq;
        s->mbox_mark = ctx->launch_mark;
        s->mbox_valid = ra.mbox != nullptr;
        // (reduce_grid: at the embedded E-step's concatenated N = 2048 the blocks times RD_THREADS pass
        // 2^32 work-items along x; a single word's grid, N <= 64, is the one-row grid it always was)
        hipLaunchKernelGGL(k_reduce_all, reduce_grid((long long)N * N + 2 * N + 1), dim3(RD_THREADS), 0, ctx->stream,
                           ra);
    }
    return launch_ok("k_reduce_all");
}

// calc_alpha / calc_beta / calc_transition_probab / calc_den_mix_coef / calc_probability are the
// diagonal trainer's, final-state term included (TFF:274-299): the same launches, on this model's A
// and the densities in the workspace
static int run_recursions_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c)
{
    int rc;
    ghmm_model *rm = &fm->rec;
    bool fused = false;
    if ((rc = run_scan_combine(ctx, rm, c, &fused))) return rc;
    if (!fused) {
        if ((rc = run_forward(ctx, rm, c, true))) return rc;
        if ((rc = run_backward(ctx, rm, c, false))) return rc;
    }
    return GHMM_OK;
}

extern "C" int ghmm_estep_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_stats *s)
{
    int rc = use(ctx);
    if (rc || (rc = check_full(ctx, fm, c)) || (rc = check_stats_full(fm, s))) return rc;
    ghmm_model *rm = &fm->rec;
    if ((rc = ws_full(ctx, fm->N, fm->M, c)) || (rc = ws_fb(ctx, rm, c))) return rc;
    if ((rc = ctx->post.grow((size_t)c->F * fm->N * fm->M))) return rc;
    if ((rc = ctx->lognorm.grow((size_t)c->F))) return rc;
    if ((rc = run_emission_full(ctx, fm, c, FC_POST))) return rc;
    if ((rc = run_recursions_full(ctx, fm, c))) return rc;
    return run_fullstats(ctx, fm, c, s, ctx->post);
}

// The same E-step with every quantity formed in the log domain (definition in include/ghmm.h): log b
// and the posteriors from FC_LOGPOST, the lattice and its utterance sums from k_logfb_fwd / k_logfb_bwd
// (both counted under GHMM_K_FORWARD), then the linear call's statistics launches as they are.
extern "C" int ghmm_estep_full_log(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_stats *s)
{
    int rc = use(ctx);
    if (rc || (rc = check_full(ctx, fm, c)) || (rc = check_stats_full(fm, s))) return rc;
    if ((rc = ws_full(ctx, fm->N, fm->M, c)) || (rc = ws_fb(ctx, &fm->rec, c))) return rc;
    if ((rc = ctx->post.grow((size_t)c->F * fm->N * fm->M))) return rc;
    if ((rc = run_emission_full(ctx, fm, c, FC_LOGPOST))) return rc;
    if ((rc = run_log_lattice(ctx, fm->N, fm->logA, c, true))) return rc;
    return run_fullstats(ctx, fm, c, s, ctx->post);
}

extern "C" int ghmm_mstep_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_stats *s)
{
    int rc = use(ctx);
    if (rc) return rc;
    ARG_CHECK(fm, "null model");
    if ((rc = check_stats_full(fm, s))) return rc;
    std::vector<double> v(s->n);
    if ((rc = ghmm_stats_download(ctx, s, v.data()))) return rc;
    ghmm_host_fmodel h;
    memset(&h, 0, sizeof h);
    if ((rc = ghmm_host_fmodel_alloc(&h, fm->N, fm->M, fm->D))) return rc;
    if (!(rc = ghmm_fmodel_get(ctx, fm, h.A, h.c, h.mean, h.inv_cov, h.det)) &&
        !(rc = ghmm_mstep_full_host(v.data(), (int)ctx->delta, &h)))
        rc = ghmm_fmodel_set(ctx, fm, h.A, h.c, h.mean, h.inv_cov, h.det);
    ghmm_host_fmodel_free(&h);
    return rc;
}

// The M-step's two launches on full-layout statistics in HBM: k_fmstep_gauss and k_fmstep_state, or
// (INIT) the initial model's k_finit_gauss and k_finit_state
template <bool INIT>
static int run_fmstep(ghmm_ctx *ctx, ghmm_fmodel *fm, const double *stats, int delta)
{
    constexpr auto k_gauss = INIT ? k_finit_gauss : k_fmstep_gauss;
    constexpr auto k_state = INIT ? k_finit_state : k_fmstep_state;
    const int N = fm->N, M = fm->M, D = fm->D;
    int rc;
    {
        kscope ks(ctx, GHMM_K_MSTEP);
        hipLaunchKernelGGL(k_gauss, dim3((unsigned)(N * M)), dim3(FM_THREADS), fm_gauss_lds_bytes(D), ctx->stream, N,
                           M, D, stats, fm->mean, fm->inv_cov, fm->det);
    }
    if ((rc = launch_ok(INIT ? "k_finit_gauss" : "k_fmstep_gauss"))) return rc;
    {
        kscope ks(ctx, GHMM_K_MSTEP);
        hipLaunchKernelGGL(k_state, dim3((unsigned)N), dim3(FM_THREADS), 0, ctx->stream, N, M, D, stats,
                           pow(2.0 * M_PI, D / 2.0), delta, fm->A, fm->c, fm->mean, fm->inv_cov, fm->det, fm->den,
                           fm->lk, fm->logA);
    }
    return launch_ok(INIT ? "k_finit_state" : "k_fmstep_state");
}

// The same M-step by k_fmstep_gauss and k_fmstep_state (ghmm_fullcov.hpp), where the statistics lie:
// nothing is downloaded and the stream is not synchronised.
extern "C" int ghmm_mstep_full_dev(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_stats *s)
{
    int rc = use(ctx);
    if (rc) return rc;
    ARG_CHECK(fm, "null model");
    if ((rc = check_stats_full(fm, s))) return rc;
    if (fm->M > FM_MAXM) {
        ghmm_set_error("the device M-step takes up to %d Gaussians per state (asked: %d); ghmm_mstep_full "
                       "has no such cap", FM_MAXM, fm->M);
        return GHMM_ERR_UNSUPPORTED;
    }
    if (ctx->last_m == &fm->rec) ctx->last_m = nullptr; // alpha^ / W belong to the old parameters
    // transitions are re-estimated inside the band i <= j <= i + delta only: a band-diagonal A stays
    // band-diagonal exactly when that band is i, i + 1.  The new A is not seen here, so a model set
    // with a wider A stays on the general recursions even if its new A happens to be band-diagonal.
    fm->rec.banded = fm->rec.banded && ctx->delta <= 1;
    return run_fmstep<false>(ctx, fm, s->v, (int)ctx->delta);
}

// ------------------------------------------------ the full-covariance trainer's initial model
// creating_initial_model (TFF:731-1134) from a corpus in HBM: the kernels of ghmm_fullcov.hpp
// (k_finit_*), enqueued back to back on the context's stream; nothing is downloaded and the stream is
// not synchronised.  ctx->finit holds, in this order, the passes' block partials [P][N][M][D + 2], one
// slice [N][M][D + 2] of their sums (a communicator's all-reduce runs on it), and the last pass's
// statistics in the full layout.
extern "C" int ghmm_fmodel_init(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_comm *cm)
{
    int rc = use(ctx);
    if (rc) return rc;
    ARG_CHECK(fm, "null model");
    ARG_CHECK(c, "null corpus");
    if ((rc = check_full(ctx, fm, c))) return rc;
    ARG_CHECK(c->U > 0 && c->F > 0, "empty corpus");
    if (fm->M > FI_MAXM) {
        ghmm_set_error("the device initial model takes up to %d Gaussians per state (asked: %d); "
                       "ghmm_init_model_full has no such cap", FI_MAXM, fm->M);
        return GHMM_ERR_UNSUPPORTED;
    }
    const rccl_api *api = nullptr;
    if (cm) {
        ARG_CHECK(cm->comm, "null communicator");
        ARG_CHECK(cm->device == ctx->device, "communicator and context are on different devices");
        if (!(api = rccl_or_error())) return GHMM_ERR_UNSUPPORTED;
    }
    const int N = fm->N, M = fm->M, D = fm->D, G = N * M, E2 = D + 2;
    const size_t slice = (size_t)G * E2, nfull = ghmm_stats_len_full(N, M, D);
    // about four blocks per CU in all, as run_fullstats sizes its grid: utterance ranges per state
    int P = (4 * ctx->cus + N - 1) / N;
    if (P > c->U) P = c->U;
    const int upb = (c->U + P - 1) / P;
    P = (c->U + upb - 1) / upb;
    if ((rc = ctx->finit.grow((size_t)(P + 1) * slice + nfull))) return rc;
    if ((rc = ctx->gamma.grow((size_t)c->F * N))) return rc;
    if ((rc = ctx->post.grow((size_t)c->F * G))) return rc;
    double *part = ctx->finit, *sums = part + (size_t)P * slice, *full = sums + slice;
    double *full_c = full + (size_t)N * N + 2 * (size_t)N;
    const size_t pass_lds = fi_pass_lds_bytes(M, D);
    if (pass_lds > 48 * 1024 && (rc = lds_attr(ctx, (const void *)k_finit_pass))) return rc;
    // the workspace is rewritten (gamma and post hold the last classification's one-hot rows), and the
    // model's parameters change: nothing an earlier pass left behind goes with either any more
    ws_disown(ctx);
    ctx->F = c->F;
    ctx->U = c->U;
    ctx->N = N;
    ctx->G = G;
    ctx->post_valid = true; // the last classification's one-hot rows, which ghmm_fetch serves
    fm->rec.banded = true; // init_transition_probab's A: j = i or i + 1

    // one classification of every frame against n_cells cells per state, the cells' sums into part;
    // gamma / post: where the one-hot rows go (the last pass's)
    auto finit_pass = [&](int n_cells, int classify, double *gamma, double *post) -> int {
        {
            kscope ks(ctx, GHMM_K_PREPARE);
            hipLaunchKernelGGL(k_finit_pass, dim3((unsigned)N, (unsigned)P), dim3(FI_THREADS), pass_lds, ctx->stream,
                               N, M, D, n_cells, classify, c->U, upb, c->X, c->off, fm->mean, part, gamma, post);
        }
        return launch_ok("k_finit_pass");
    };
    auto pass = [&](int n_cells, int do_split, bool first) -> int {
        int r;
        if ((r = finit_pass(n_cells, first ? 0 : 1, nullptr, nullptr))) return r;
        const double *src = part;
        int np = P;
        if (cm) { // the sums of all shards: every rank then does the same bookkeeping on the same numbers
            {
                kscope ks(ctx, GHMM_K_REDUCE);
                hipLaunchKernelGGL(k_finit_reduce, dim3((unsigned)((slice + 255) / 256)), dim3(256), 0, ctx->stream,
                                   (long long)slice, P, (const double *)part, sums);
            }
            if ((r = launch_ok("k_finit_reduce"))) return r;
            RCCL_TRY(api, api->AllReduce(sums, sums, slice, ncclDouble, ncclSum, cm->comm, ctx->stream));
            src = sums;
            np = 1;
        }
        {
            kscope ks(ctx, GHMM_K_REDUCE);
            hipLaunchKernelGGL(k_finit_cells, dim3((unsigned)N), dim3(64), (size_t)n_cells * E2 * sizeof(double),
                               ctx->stream, N, M, D, n_cells, do_split, first ? 1 : 0, np, src, 1.05, 0.95, 1.005,
                               0.995, fm->mean);
        }
        return launch_ok("k_finit_cells");
    };
    // init_mix_mean (TFF:970-1134): the state's mean, then five passes per level
    if ((rc = pass(1, 1 < M ? 1 : 0, true))) return rc;
    int nc = 1;
    while (nc < M) {
        nc = (2 * nc < M) ? 2 * nc : M;
        for (int it = 0; it < 5; it++)
            if ((rc = pass(nc, (it == 4 && nc < M) ? 1 : 0, false))) return rc;
    }
    // init_mix_param (TFF:810-952): one more classification, its one-hot rows into gamma and post;
    // k_fullstats takes dif around the model's mean, which is the cell
    long long PF = 0;
    if ((rc = finit_pass(M, 1, ctx->gamma, ctx->post)) || (rc = run_fullstats_part(ctx, fm, c, ctx->post, &PF))) return rc;
    {
        kscope ks(ctx, GHMM_K_REDUCE);
        if ((rc = run_fullstats_reduce(ctx, fm, PF, full_c))) return rc;
    }
    if (cm)
        RCCL_TRY(api, api->AllReduce(full_c, full_c, (size_t)G * fs_elems(D), ncclDouble, ncclSum, cm->comm,
                                     ctx->stream));
    return run_fmstep<true>(ctx, fm, full, 1);
}

// ------------------------------------------------ several feature streams (TFF, RC: param_number P > 1)
// Every recursion runs on the product over the streams of the emission densities, taken in stream
// order (TFF:1436-1442, TFF:1460-1465, RC:760-789); the mixtures are each stream's own (TFF:256-297,
// TFF:316-342).  The product is formed by the emission launches themselves: stream 0 writes b, every
// later stream's launch (k_emission_full's FOLD) multiplies into it, or adds onto log b.  There is no
// second b and no pass of its own for the product.

// the array and range check, then the shared stream_checks with, per stream, the statistics vector's
// (`stats` may be null where want_stats is not set: the score calls); nothing is launched before every
// check has passed
static int check_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora, int P,
                              ghmm_stats *const *stats, bool want_stats)
{
    if (!models || !corpora || (want_stats && !stats) || P < 1 || P > GHMM_MAX_STREAMS) {
        ghmm_set_error("bad stream arguments (1 to %d feature streams, no null array)", GHMM_MAX_STREAMS);
        return GHMM_ERR_ARG;
    }
    return stream_checks(
        models, corpora, P, [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); },
        [=](int p) { return want_stats ? check_stats_full(models[p], stats[p]) : GHMM_OK; });
}

// the workspace of stream 0's shape, then every stream's emission in stream order: ctx->b ends up
// holding the product (log modes: the sum of logs), ctx->post_s[p] stream p's posteriors
static int emission_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora, int P,
                                 int mode)
{
    int rc;
    const bool want_post = mode == FC_POST || mode == FC_LOGPOST;
    if ((rc = ws_full(ctx, models[0]->N, models[0]->M, corpora[0]))) return rc;
    for (int p = 0; want_post && p < P; p++)
        if ((rc = ctx->post_s[p].grow((size_t)corpora[p]->F * models[p]->N * models[p]->M))) return rc;
    for (int p = 0; p < P; p++)
        if ((rc = run_emission_full(ctx, models[p], corpora[p], mode, p > 0, want_post ? ctx->post_s[p] : nullptr)))
            return rc;
    return GHMM_OK;
}

extern "C" int ghmm_estep_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                                       int P, ghmm_stats *const *stats, int log_domain)
{
    int rc = use(ctx);
    if (rc || (rc = check_full_streams(ctx, models, corpora, P, stats, true))) return rc;
    if (P == 1)
        return log_domain ? ghmm_estep_full_log(ctx, models[0], corpora[0], stats[0])
                          : ghmm_estep_full(ctx, models[0], corpora[0], stats[0]);
    ghmm_fmodel *fm = models[0];
    ghmm_corpus *c = corpora[0];
    if ((rc = ws_fb(ctx, &fm->rec, c))) return rc;
    if (!log_domain && (rc = ctx->lognorm.grow((size_t)c->F))) return rc;
    if ((rc = emission_full_streams(ctx, models, corpora, P, log_domain ? FC_LOGPOST : FC_POST))) return rc;
    // the single-stream calls' recursion launches, on models[0]'s transitions and the product
    if ((rc = log_domain ? run_log_lattice(ctx, fm->N, fm->logA, c, true) : run_recursions_full(ctx, fm, c))) return rc;
    // calc_mix_param per stream (TFF:289-297) with the common gamma; the transition sums, den_c, log P
    // and the exemplar count go into every stream's vector
    for (int p = 0; p < P && !rc; p++) rc = run_fullstats(ctx, models[p], corpora[p], stats[p], ctx->post_s[p]);
    return rc;
}

extern "C" int ghmm_score_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                                       int P, double *loglik_host)
{
    int rc = use(ctx);
    if (rc || (rc = check_full_streams(ctx, models, corpora, P, nullptr, false))) return rc;
    if (P == 1) return ghmm_score_full(ctx, models[0], corpora[0], loglik_host);
    ghmm_corpus *c = corpora[0];
    ARG_CHECK(loglik_host || c->U == 0, "null destination");
    if ((rc = emission_full_streams(ctx, models, corpora, P, FC_LIN))) return rc;
    if (c->U == 0) return GHMM_OK;
    return run_score_full(ctx, models[0], c, loglik_host);
}

extern "C" int ghmm_logscore_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models,
                                          ghmm_corpus *const *corpora, int P, int final_state,
                                          double *loglik_host)
{
    int rc = use(ctx);
    if (rc || (rc = check_full_streams(ctx, models, corpora, P, nullptr, false))) return rc;
    if (P == 1) return ghmm_logscore_full(ctx, models[0], corpora[0], final_state, loglik_host);
    ARG_CHECK(loglik_host || corpora[0]->U == 0, "null destination");
    if (corpora[0]->U == 0) return GHMM_OK;
    return flogscore_word(ctx, models, corpora, P, final_state, loglik_host);
}

// ------------------------------------------------ several-stream vocabularies
// Viterbi on several streams, the three batched vocabulary calls on several streams, and the word
// decoder (definitions in include/ghmm.h).  No new arithmetic: the streams' emission launches with
// FOLD, then the lattice launches of ghmm_lattice_host.hpp on the folded b or log b.

extern "C" int ghmm_viterbi_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                                         int P, int32_t *path_host, double *score_host)
{
    int rc = use(ctx);
    if (rc || (rc = check_full_streams(ctx, models, corpora, P, nullptr, false))) return rc;
    if (P == 1) return ghmm_viterbi_full(ctx, models[0], corpora[0], path_host, score_host);
    ghmm_fmodel *fm = models[0];
    ghmm_corpus *c = corpora[0];
    ARG_CHECK((path_host && score_host) || c->U == 0, "null destination");
    if (c->U == 0) return GHMM_OK;
    if ((rc = viterbi_ws(ctx, c, lane_grid(fm->N, c->U).L))) return rc;
    if ((rc = emission_full_streams(ctx, models, corpora, P, FC_LOG))) return rc;
    return run_viterbi_lanes(ctx, fm->N, fm->logA, c, path_host, score_host);
}

extern "C" int ghmm_score_full_streams_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                             ghmm_corpus *const *corpora, int P, double *loglik_host)
{
    return fvocab_score(ctx, models, n_models, corpora, P, loglik_host, __func__);
}

extern "C" int ghmm_logscore_full_streams_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                                ghmm_corpus *const *corpora, int P, int final_state,
                                                double *loglik_host)
{
    return fvocab_logscore(ctx, models, n_models, corpora, P, final_state, loglik_host, __func__);
}

extern "C" int ghmm_viterbi_full_streams_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                               ghmm_corpus *const *corpora, int P, double *score_host)
{
    return fvocab_viterbi(ctx, models, n_models, corpora, P, score_host, __func__);
}

extern "C" int ghmm_recognise_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                           ghmm_corpus *const *corpora, int P, int32_t *word_host,
                                           int32_t *path_host, double *score_host)
{
    vocab_pass v;
    int rc = fvocab_begin(ctx, models, n_models, corpora, P, word_host && path_host && score_host, FC_LOG, __func__,
                          &v);
    if (rc || corpora[0]->U == 0) return rc;
    return vocab_decode(ctx, v, n_models, corpora[0], word_host, path_host, score_host);
}

extern "C" int ghmm_connect_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                         ghmm_corpus *const *corpora, int P, double word_penalty,
                                         int32_t *word_host, int32_t *path_host, int32_t *begin_host,
                                         double *score_host)
{
    vocab_pass v;
    const bool have_dest = word_host && path_host && begin_host && score_host;
    // the vocabulary checks once ahead of fvocab_begin's own: the decoder's refusals need NS and come
    // before anything is launched
    int rc = use(ctx);
    if (rc) return rc;
    rc = vocab_checks(models, n_models, corpora, P, have_dest, __func__,
                      [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); }, &v);
    if (rc || (rc = connect_check(v, word_penalty, __func__))) return rc;
    rc = fvocab_begin(ctx, models, n_models, corpora, P, have_dest, FC_LOG, __func__, &v);
    if (rc || corpora[0]->U == 0) return rc;
    return vocab_connect(ctx, v, n_models, corpora[0], word_penalty, word_host, path_host, begin_host, score_host);
}

extern "C" int ghmm_connect_grammar_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                                 ghmm_corpus *const *corpora, int P, const double *start,
                                                 const double *pair, const double *fin, int32_t *word_host,
                                                 int32_t *path_host, int32_t *begin_host, double *score_host)
{
    vocab_pass v;
    const bool have_dest = word_host && path_host && begin_host && score_host;
    // as in ghmm_connect_full_streams: the vocabulary checks once ahead of fvocab_begin's own, the
    // decoder's refusals need NS and come before anything is launched
    int rc = use(ctx);
    if (rc) return rc;
    rc = vocab_checks(models, n_models, corpora, P, have_dest, __func__,
                      [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); }, &v);
    if (rc || (rc = grammar_check(v, n_models, corpora[0]->U, start, pair, fin, __func__))) return rc;
    rc = fvocab_begin(ctx, models, n_models, corpora, P, have_dest, FC_LOG, __func__, &v);
    if (rc || corpora[0]->U == 0) return rc;
    return vocab_connect_grammar(ctx, v, n_models, corpora[0], start, pair, fin, word_host, path_host, begin_host,
                                 score_host);
}

extern "C" int ghmm_grammar_post_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                              ghmm_corpus *const *corpora, int P, const double *start,
                                              const double *pair, const double *fin, double *occ_host,
                                              double *ent_host, double *loglik_host)
{
    vocab_pass v;
    const bool have_dest = occ_host && loglik_host;
    // as in ghmm_connect_grammar_full_streams: the vocabulary checks once ahead of fvocab_begin's own, the
    // lattice's refusals need NS and come before anything is launched
    int rc = use(ctx);
    if (rc) return rc;
    rc = vocab_checks(models, n_models, corpora, P, have_dest, __func__,
                      [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); }, &v);
    if (rc || (rc = grammar_check(v, n_models, corpora[0]->U, start, pair, fin, __func__))) return rc;
    rc = fvocab_begin(ctx, models, n_models, corpora, P, have_dest, FC_LOG, __func__, &v);
    if (rc || corpora[0]->U == 0) return rc;
    return vocab_grammar_post(ctx, v, n_models, corpora[0], start, pair, fin, occ_host, ent_host, loglik_host);
}

extern "C" int ghmm_align_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                       ghmm_corpus *const *corpora, int P, const int32_t *seq,
                                       const int32_t *seq_off, int32_t *word_host, int32_t *path_host,
                                       int32_t *begin_host, double *score_host)
{
    vocab_pass v;
    align_plan pl;
    const bool have_dest = word_host && path_host && begin_host && score_host && seq && seq_off;
    // as in ghmm_connect_full_streams: the vocabulary checks once ahead of fvocab_begin's own, the
    // alignment's refusals need the words' states and come before anything is launched
    int rc = use(ctx);
    if (rc) return rc;
    rc = vocab_checks(models, n_models, corpora, P, have_dest, __func__,
                      [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); }, &v);
    if (rc || corpora[0]->U == 0) return rc;
    if ((rc = align_check(models, n_models, P, corpora[0], v, seq, seq_off, __func__, &pl)) ||
        (rc = fvocab_begin(ctx, models, n_models, corpora, P, have_dest, FC_LOG, __func__, &v)))
        return rc;
    return vocab_align(ctx, v, corpora[0], pl, seq, seq_off, word_host, path_host, begin_host, score_host);
}

// ------------------------------------------------ embedded Baum-Welch on word transcripts
// ghmm_estep_embed_full_streams (definition in include/ghmm.h): ghmm_estep_embed_streams for
// full-covariance words.  fvocab_begin's gathers and its emission launches under FC_LOGPOST (log b and
// every stream's posteriors, the folds in the launches' epilogue), the lattice over the transcripts' word
// instances (embed_lattice: it sees log b[F][NS] and the words' table), run_fullstats once per stream on
// the CONCATENATED model into a vector of the context's, and one scatter per stream of every word's blocks
// into its own vector (k_embed_scatter_full).

// k_fullstats puts its batches of FS_THREADS * FS_EPT elements on gridDim.y: whether the concatenated
// model of NS states has more batches than the device takes there.  Nothing is launched here.
static int fullstats_extent_check(ghmm_ctx *ctx, int NS, int M, int D, int p, const char *what)
{
    int max_y = 0;
    HIP_TRY(hipDeviceGetAttribute(&max_y, hipDeviceAttributeMaxGridDimY, ctx->device));
    const long long E = (long long)NS * M * fs_elems(D);
    const long long NB = (E + FS_THREADS * FS_EPT - 1) / (FS_THREADS * FS_EPT);
    if (NB > max_y) {
        ghmm_set_error("%s: stream %d: %d states of %d Gaussians of %d coefficients are %lld batches of statistics, "
                       "the launch takes %d", what, p, NS, M, D, NB, max_y);
        return GHMM_ERR_UNSUPPORTED;
    }
    return GHMM_OK;
}

extern "C" int ghmm_estep_embed_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                             ghmm_corpus *const *corpora, int P, const int32_t *seq,
                                             const int32_t *seq_off, ghmm_stats *const *stats)
{
    vocab_pass v;
    align_plan pl;
    // as in ghmm_align_full_streams: the vocabulary checks once ahead of fvocab_begin's own, the other
    // refusals need the words' states and come before anything is launched
    int rc = use(ctx);
    if (rc) return rc;
    rc = vocab_checks(models, n_models, corpora, P, seq && seq_off, __func__,
                      [ctx](const ghmm_fmodel *fm, const ghmm_corpus *c) { return check_full(ctx, fm, c); }, &v);
    if (rc) return rc;
    ARG_CHECK(stats, "null statistics");
    for (int k = 0; k < n_models * P; k++)
        if ((rc = check_stats_full(models[k], stats[k]))) return rc;
    ghmm_corpus *c = corpora[0];
    if (c->U == 0) return embed_empty(ctx, stats, n_models * P);
    if ((rc = align_check(models, n_models, P, c, v, seq, seq_off, __func__, &pl))) return rc;
    for (int p = 0; p < P; p++)
        if ((rc = fullstats_extent_check(ctx, v.NS, models[p]->M, models[p]->D, p, __func__))) return rc;
    if ((rc = fvocab_begin(ctx, models, n_models, corpora, P, true, FC_LOGPOST, __func__, &v))) return rc;
    const embed_dst *ddst;
    if ((rc = embed_lattice(ctx, models, n_models, P, models[0]->M, c, v, pl, seq, seq_off, stats, &ddst))) return rc;
    for (int p = 0; p < P; p++) {
        ghmm_fmodel *cat = ctx->fbt_cat[p];
        ghmm_stats cs; // the concatenated model's vector: the context's, without a mailbox
        cs.N = cat->N; cs.M = cat->M; cs.D = cat->D;
        cs.full = true;
        cs.n = ghmm_stats_len_full(cat->N, cat->M, cat->D);
        if ((rc = ctx->em_vec[p].grow(cs.n))) return rc;
        cs.v = ctx->em_vec[p];
        if ((rc = run_fullstats(ctx, cat, corpora[p], &cs, P == 1 ? ctx->post : ctx->post_s[p]))) return rc;
        {
            // the chunks of the largest word at this stream's shape (every range is shared between them)
            const size_t most = ghmm_stats_len_full(v.Nmax, cat->M, cat->D);
            const int ch = (int)std::min<size_t>(1024, (most + EMBED_SCATTER_PER_BLOCK - 1) / EMBED_SCATTER_PER_BLOCK);
            kscope ks(ctx, GHMM_K_REDUCE);
            hipLaunchKernelGGL(k_embed_scatter_full, dim3((unsigned)n_models, (unsigned)ch), dim3(256), 0, ctx->stream,
                               cat->N, cat->M, cat->D, (const double *)cs.v, ddst + (size_t)p * n_models);
        }
        if ((rc = launch_ok("k_embed_scatter_full"))) return rc;
        // (the words' vectors are not k_reduce_all's: its mailbox does not describe them)
        for (int k = 0; k < n_models; k++) stats[(size_t)k * P + p]->mbox_valid = false;
    }
    return GHMM_OK;
}
