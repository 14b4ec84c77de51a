/*
 * recognition-continuous-test-fs — the reference recogniser's command line on the
 * MI355X core.
 *
 * Same argv, list/.perfil/.hmm formats and report file as the reference's main()
 * (RF:87-428):
 *     models_number model1..N coef_model1..N input_file1..N word_file output_file
 * The reference re-reads every utterance file once per word model and runs
 * emission + forward per (utterance, model) (RF:326-374).  Here all utterances are
 * read once, kept in HBM, and every word model scores the whole batch with one
 * ghmm_score call; the ranking, the correct / error / second-candidate bookkeeping
 * and the report text follow RF:374-412 and RF:1014-1194 line by line, including
 * the NaN-blind bubble sort (RF:968-995).
 *
 * A model set may have several feature streams (param_number P > 1): its P feature lists follow
 * each other on the command line (RF:253-262) and the score runs on the product of the streams'
 * emission densities (RF:349-366): the whole vocabulary in one pass with ghmm_score_streams_batch (on
 * one stream that is ghmm_score_batch) as long as the words agree in every stream's M, model by model
 * with ghmm_score_streams otherwise.
 *
 * Built with -DGHMM_FULL_COV this is recognition-continuous-test-full-fs, the full-covariance
 * recogniser RC = test/source/recognition-full-fs/recognition_continuous_full_fs.c: the same
 * argv, lists and bookkeeping (RC:283-412), its usage text and header (RC:1019-1033), models read
 * with ghmm_hmm_read_full_streams (RC:591-707) and scored with ghmm_score_full_streams_batch, whose
 * log P has no final-state term (calc_probability, RC:822-836): the whole vocabulary in one pass, on
 * one feature stream (where it is ghmm_score_full_batch) or several, as long as the words agree in
 * every stream's M; a set whose words do not is scored model by model with ghmm_score_full_streams.
 * With GHMM_LOG_SCORE=1 in the environment either program scores in the log domain instead and says so
 * in the report's second line: the full-covariance one with ghmm_logscore_full_streams_batch /
 * ghmm_logscore_full_streams and final_state = 0, the diagonal one with ghmm_logscore_streams_batch /
 * ghmm_logscore_streams and final_state = 1 (its final-state term kept); the same quantities, finite
 * where the linear densities underflow.  Without the variable nothing changes.
 * With GHMM_CONNECTED=1 (and optionally GHMM_WORD_PENALTY=<double>, default 0) either program decodes
 * every utterance as a STRING of the vocabulary's words instead (ghmm_connect_streams /
 * ghmm_connect_full_streams): exactly one model set; the output file's first line says so, then one line
 * per utterance, also on stdout: the feature file's name (stream 1's), the words' names in order, the
 * score.  The word file is read for the utterance count as always; what it says was spoken is not used.
 * Without the variable nothing changes.
 * With GHMM_GRAMMAR=<file> beside GHMM_CONNECTED=1 the string is decoded under a word-pair grammar
 * (ghmm_connect_grammar_streams / ghmm_connect_grammar_full_streams).  The file is text: K, then the K
 * start scores, then K rows of K pair scores (row w, column k: word k after word w, the words in the model
 * list's order), then the K end scores; every token goes through strtod, which accepts -inf (forbidden).
 * GHMM_WORD_PENALTY is added to every pair score.  The output file's first line names the grammar file.
 * A file that is short or holds a token that is no number, GHMM_GRAMMAR without GHMM_CONNECTED=1 or with
 * GHMM_ALIGN=1: a message and exit 1 before any model or feature file is read; a K that is not the
 * model list's: the same as soon as the list has been counted, before any feature file is read.
 * Without the variable nothing changes.
 * With GHMM_ALIGN=1 either program aligns every utterance with its known transcript instead
 * (ghmm_align_streams / ghmm_align_full_streams): exactly one model set; every token of the word file is
 * that utterance's transcript, the words' names joined by '+' (three+five+five), an unknown name is an
 * error that names it; the output file's first line says forced alignment, then one line per utterance,
 * also on stdout: feature_file : word first last  word first last ... : score (frames counted inside the
 * utterance).  Together with GHMM_CONNECTED=1 it is refused.  Without the variable nothing changes.
 * With GHMM_CONFIDENCE=1 beside GHMM_CONNECTED=1 (with or without GHMM_GRAMMAR) every decoded word carries its
 * confidence, the mean over its frames of the posterior that the frame lies in that word
 * (ghmm_grammar_post_streams / ghmm_grammar_post_full_streams under the decoder's grammar; without a grammar
 * file the flat grammar pair == GHMM_WORD_PENALTY, start == fin == 0): name(0.93), and the line ends with the
 * Viterbi score and then log P, the utterance's total over every string the grammar allows.  The output
 * file's first line says that confidences are on.  GHMM_CONFIDENCE without GHMM_CONNECTED=1 or with
 * GHMM_ALIGN=1: a message and exit 1 before any file is read.  Without the variable nothing changes.
 */
#include "ghmm.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/times.h>
#include <time.h>

#define MAX_SETS 16

static void die(const char *what, int rc)
{
    const char *d = ghmm_last_error();
    printf("%s: %s \n", what, (d && *d) ? d : ghmm_strerror(rc));
    exit(1);
}

static void usage(void)
{
#ifdef GHMM_FULL_COV
    puts("Usage: recognition_continuous_full models_number  model1 ... modelN coef_model1 ... coef_modelN input_file1 ... input_fileM  word_file output_file");
#else
    puts("Usage: recognition_continuous_fs models_number  model1 ... modelN coef_model1 ... coef_modelN input_file1 ... input_fileM  word_file output_file");
#endif
    puts("models_number: number of model");
    puts("model1: name of file with the name of model 1");
    puts("modelN: name of file with the name of model N");
    puts("coef_model1: weighting coefficient of model 1");
    puts("coef_modelN: weighting coefficient of model N");
    puts("input_file1: name of file with name of files with parameters 1 ");
    puts("input_fileM: name of file with name of files with parameters M ");
    puts("word_file: name of file with the spoken words ");
    puts("output_file: name of output file ");
    exit(1);
}

static FILE *open_read(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        printf("file %s not found \n", path);
        exit(1);
    }
    return f;
}

static double cpu_units(void)
{
    struct tms t;
    times(&t);
    return t.tms_utime / 60.0; /* RF:278 */
}

/* sorting_probab, RF:968-995 */
static void rank_scores(const double *probab, int *index, int n)
{
    int done = 0;
    for (int i = 0; i < n; i++) index[i] = i;
    while (!done) {
        done = 1;
        for (int i = 0; i < n - 1; i++)
            if (probab[index[i]] < probab[index[i + 1]]) {
                int aux = index[i];
                index[i] = index[i + 1];
                index[i + 1] = aux;
                done = 0;
            }
    }
}

static FILE *f_out;

/* GHMM_CONNECTED=1: the one model set's vocabulary (hm[k * GHMM_MAX_STREAMS + p]) on its P streams, every
 * utterance decoded as a word string; one line per utterance to stdout and the output file.
 * GHMM_ALIGN=1 (seq_off != NULL): every utterance aligned with its transcript seq[seq_off[u] .. seq_off[u+1])
 * instead, the line holding every word instance's first and last frame.
 * GHMM_GRAMMAR (gram != NULL): start[K] | pair[K][K] | fin[K], the penalty already added to pair.
 * GHMM_CONFIDENCE (confidence != 0, decoding only): the word posteriors under the same grammar (none: the
 * flat one, pair == penalty), every word printed with its mean occ, the line closed by the score and log P */
#ifdef GHMM_FULL_COV
typedef ghmm_host_fmodel host_model_t;
typedef ghmm_fmodel dev_model_t;
#else
typedef ghmm_host_model host_model_t;
typedef ghmm_model dev_model_t;
#endif
static void run_connected(const host_model_t *hm, int word_number, int P, double *const *X, const int32_t *len,
                          int n_utt, const int *D, double penalty, char *const *utt_name, const int32_t *seq,
                          const int32_t *seq_off, const double *gram, int confidence)
{
    int rc;
    size_t F = 0;
    for (int u = 0; u < n_utt; u++) F += (size_t)len[u];
    ghmm_ctx *ctx;
    if ((rc = ghmm_ctx_create(0, NULL, &ctx))) die("GPU context", rc);
    ghmm_corpus *corpus[GHMM_MAX_STREAMS];
    for (int p = 0; p < P; p++)
        if ((rc = ghmm_corpus_create(ctx, X[p], len, n_utt, D[p], &corpus[p]))) die("corpus", rc);
    dev_model_t **flat = (dev_model_t **)calloc((size_t)word_number * P, sizeof(dev_model_t *));
    int32_t *wd = (int32_t *)malloc((F ? F : 1) * 3 * sizeof(int32_t)), *st = wd + (F ? F : 1), *bg = st + (F ? F : 1);
    double *sc = (double *)malloc((size_t)n_utt * sizeof(double));
    if (!flat || !wd || !sc) die("memory", GHMM_ERR_ALLOC);
    for (int k = 0; k < word_number; k++)
        for (int p = 0; p < P; p++) {
            const host_model_t *m = &hm[(size_t)k * GHMM_MAX_STREAMS + p];
            if (m->D != D[p]) {
                printf("model %s has %d coefficients, data has %d \n", m->word, m->D, D[p]);
                exit(1);
            }
            dev_model_t **slot = &flat[(size_t)k * P + p];
#ifdef GHMM_FULL_COV
            if ((rc = ghmm_fmodel_create(ctx, m->N, m->M, m->D, slot))) die("model", rc);
            if ((rc = ghmm_fmodel_set(ctx, *slot, m->A, m->c, m->mean, m->inv_cov, m->det))) die("model", rc);
#else
            if ((rc = ghmm_model_create(ctx, m->N, m->M, m->D, slot))) die("model", rc);
            if ((rc = ghmm_model_set(ctx, *slot, m->A, m->c, m->mean, m->inv_var, m->det))) die("model", rc);
#endif
        }
#ifdef GHMM_FULL_COV
    rc = seq_off ? ghmm_align_full_streams(ctx, flat, word_number, corpus, P, seq, seq_off, wd, st, bg, sc)
         : gram  ? ghmm_connect_grammar_full_streams(ctx, flat, word_number, corpus, P, gram, gram + word_number,
                                                     gram + word_number + (size_t)word_number * word_number, wd, st,
                                                     bg, sc)
                 : ghmm_connect_full_streams(ctx, flat, word_number, corpus, P, penalty, wd, st, bg, sc);
#else
    rc = seq_off ? ghmm_align_streams(ctx, flat, word_number, corpus, P, seq, seq_off, wd, st, bg, sc)
         : gram  ? ghmm_connect_grammar_streams(ctx, flat, word_number, corpus, P, gram, gram + word_number,
                                                gram + word_number + (size_t)word_number * word_number, wd, st, bg, sc)
                 : ghmm_connect_streams(ctx, flat, word_number, corpus, P, penalty, wd, st, bg, sc);
#endif
    if (rc) die(seq_off ? "alignment" : "decoding", rc);
    double *occ = NULL, *ll = NULL;
    if (confidence) {
        const size_t Kw = (size_t)word_number;
        double *flat_pair = NULL;
        occ = (double *)malloc((F ? F : 1) * Kw * sizeof(double));
        ll = (double *)malloc((size_t)n_utt * sizeof(double));
        if (!gram && (flat_pair = (double *)malloc(Kw * Kw * sizeof(double))))
            for (size_t i = 0; i < Kw * Kw; i++) flat_pair[i] = penalty;
        if (!occ || !ll || (!gram && !flat_pair)) die("memory", GHMM_ERR_ALLOC);
#ifdef GHMM_FULL_COV
        rc = ghmm_grammar_post_full_streams(ctx, flat, word_number, corpus, P, gram, gram ? gram + Kw : flat_pair,
                                            gram ? gram + Kw + Kw * Kw : NULL, occ, NULL, ll);
#else
        rc = ghmm_grammar_post_streams(ctx, flat, word_number, corpus, P, gram, gram ? gram + Kw : flat_pair,
                                       gram ? gram + Kw + Kw * Kw : NULL, occ, NULL, ll);
#endif
        if (rc) die("word posteriors", rc);
        free(flat_pair);
    }
    size_t f = 0;
    for (int u = 0; u < n_utt; u++) {
        FILE *to[2] = {stdout, f_out};
        for (int o = 0; o < 2; o++) {
            fprintf(to[o], "%s :", utt_name[u]);
            for (int t = 0, n = 0; t < len[u]; t++) {
                if (!bg[f + t]) continue;
                const char *name = hm[(size_t)wd[f + t] * GHMM_MAX_STREAMS].word;
                if (!seq_off && !confidence) {
                    fprintf(to[o], " %s", name);
                    continue;
                }
                int last = t;
                while (last + 1 < len[u] && !bg[f + last + 1]) last++;
                if (confidence) {
                    double sum = 0.0;
                    for (int q = t; q <= last; q++) sum += occ[(f + q) * (size_t)word_number + wd[f + t]];
                    fprintf(to[o], " %s(%.2f)", name, sum / (last - t + 1));
                    continue;
                }
                fprintf(to[o], "%s %s %d %d", n++ ? " " : "", name, t, last);
            }
            if (confidence) fprintf(to[o], " : %f %f\n", sc[u], ll[u]);
            else fprintf(to[o], " : %f\n", sc[u]);
        }
        f += (size_t)len[u];
    }
    for (int k = 0; k < word_number * P; k++)
#ifdef GHMM_FULL_COV
        ghmm_fmodel_destroy(ctx, flat[k]);
#else
        ghmm_model_destroy(ctx, flat[k]);
#endif
    for (int p = 0; p < P; p++) ghmm_corpus_destroy(ctx, corpus[p]);
    ghmm_ctx_destroy(ctx);
    free(flat); free(wd); free(sc); free(occ); free(ll);
}

/* GHMM_GRAMMAR: the file's K into *K_out and its start[K] | pair[K][K] | fin[K] as one array; a file that
 * cannot be opened, is short or holds a token that is no number ends the program */
static double *read_grammar(const char *path, int *K_out)
{
    FILE *f = open_read(path);
    char tok[256], *end;
    long K = 0;
    if (fscanf(f, "%255s", tok) == 1) K = strtol(tok, &end, 10);
    if (K < 1 || K > 1 << 20 || *end) {
        printf("grammar file %s: its first token must be the number of words \n", path);
        exit(1);
    }
    const size_t n = (size_t)K * (size_t)K + 2 * (size_t)K;
    double *g = (double *)malloc(n * sizeof(double));
    if (!g) die("memory", GHMM_ERR_ALLOC);
    for (size_t i = 0; i < n; i++) {
        if (fscanf(f, "%255s", tok) != 1) {
            printf("grammar file %s is short: %zu of the %zu scores of %ld words \n", path, i, n, K);
            exit(1);
        }
        g[i] = strtod(tok, &end);
        if (end == tok || *end) {
            printf("grammar file %s: score %zu (%s) is no number \n", path, i, tok);
            exit(1);
        }
    }
    fclose(f);
    *K_out = (int)K;
    return g;
}

/* writing_result_word, RF:1111-1150 */
static void report_word(int correct, int error, int second, int word_number, const char *spoken,
                        const int *wrong_word, char **word, double cpu_time, int word_frames)
{
    int sum = correct + error;
    double per = (double)correct / (double)sum;
    cpu_time /= sum;
    word_frames /= sum;
    fprintf(f_out, "\nResults: \n");
    fprintf(f_out, "Spoken word: %s\n", spoken);
    fprintf(f_out, "Correct words: %d\n", correct);
    fprintf(f_out, "Errors: %d\n", error);
    fprintf(f_out, "Percentagen correct : %.2f%%\n", per * 100.0);
    fprintf(f_out, "Second candidate: %d\n", second);
    if (error != 0) {
        fprintf(f_out, "Wrong words: \n");
        for (int i = 0; i < word_number; i++)
            if (wrong_word[i] != 0)
                fprintf(f_out, "%s: %d time%s\n", word[i], wrong_word[i], wrong_word[i] == 1 ? "" : "s");
    }
    fprintf(f_out, "Average recognition time: %.2f sec. \n", cpu_time);
    fprintf(f_out, "Average word length: %d frames \n", word_frames);
}

int main(int argc, char **argv)
{
    char date_time[64];
    time_t now;
    time(&now);
    strftime(date_time, sizeof date_time, "%d-%h-%Y %X", localtime(&now));
    if (argc < 7) usage();
    int K = atoi(argv[1]);
    if (K < 1 || K > MAX_SETS || argc < 3 * K + 4) usage();
    double coef_model[MAX_SETS];
    for (int i = 0; i < K; i++) coef_model[i] = atof(argv[K + 2 + i]);
    const char *output_file = argv[argc - 1], *word_file = argv[argc - 2];
    int rc;
    const char *env_log = getenv("GHMM_LOG_SCORE");
    const int log_score = env_log && strcmp(env_log, "1") == 0;
    const char *env_con = getenv("GHMM_CONNECTED"), *env_pen = getenv("GHMM_WORD_PENALTY");
    const int connected = env_con && strcmp(env_con, "1") == 0;
    const double word_penalty = (connected && env_pen) ? atof(env_pen) : 0.0;
    if (connected && K != 1) {
        printf("GHMM_CONNECTED=1 takes exactly one model set (given: %d) \n", K);
        exit(1);
    }
    const char *env_al = getenv("GHMM_ALIGN");
    const int align = env_al && strcmp(env_al, "1") == 0;
    const char *env_conf = getenv("GHMM_CONFIDENCE");
    const int confidence = env_conf && strcmp(env_conf, "1") == 0;
    if (confidence && (!connected || align)) {
        printf("GHMM_CONFIDENCE takes GHMM_CONNECTED=1%s \n", align ? ", not GHMM_ALIGN=1" : "");
        exit(1);
    }
    if (align && connected) {
        printf("GHMM_ALIGN=1 and GHMM_CONNECTED=1 exclude each other \n");
        exit(1);
    }
    if (align && K != 1) {
        printf("GHMM_ALIGN=1 takes exactly one model set (given: %d) \n", K);
        exit(1);
    }
    const char *env_gram = getenv("GHMM_GRAMMAR");
    double *gram = NULL;
    int gram_K = 0;
    if (env_gram && !connected) {
        printf("GHMM_GRAMMAR takes GHMM_CONNECTED=1%s \n", align ? ", not GHMM_ALIGN=1" : "");
        exit(1);
    }
    if (env_gram) gram = read_grammar(env_gram, &gram_K);
    char **utt_words = NULL; /* alignment: every utterance's token of the word file, its transcript */
    char **utt_name = NULL; /* connected decoding: every utterance's feature file (stream 1's) */

    /* models: one list per set, the same vocabulary in every set */
#ifdef GHMM_FULL_COV
    ghmm_host_fmodel *fhm[MAX_SETS]; /* fhm[j][k * GHMM_MAX_STREAMS + p]: set j, word k, stream p */
#else
    ghmm_host_model *hm[MAX_SETS]; /* hm[j][k * GHMM_MAX_STREAMS + p]: set j, word k, stream p */
#endif
    int Pj[MAX_SETS];              /* feature streams of set j (param_number of its models) */
    int word_number = 0;
    printf("\r\nLoading Models\r\n");
    for (int j = 0; j < K; j++) {
        FILE *fl = open_read(argv[2 + j]);
        char name[4096];
        int n = 0, cap = 0;
#ifdef GHMM_FULL_COV
        fhm[j] = NULL;
        while (fscanf(fl, "%4095s", name) == 1) {
            printf("Model: %s\r\n", name);
            if (n == cap) {
                cap = cap ? 2 * cap : 32;
                fhm[j] = (ghmm_host_fmodel *)realloc(fhm[j], (size_t)cap * GHMM_MAX_STREAMS * sizeof(ghmm_host_fmodel));
                if (!fhm[j]) die("memory", GHMM_ERR_ALLOC);
            }
            /* the file says how many feature streams the model has (RC:591-707) */
            int pn = 0;
            if ((rc = ghmm_hmm_read_full_streams(name, &fhm[j][(size_t)n * GHMM_MAX_STREAMS], GHMM_MAX_STREAMS, &pn)))
                die("reading model", rc);
            if (n == 0) Pj[j] = pn;
            if (pn != Pj[j]) {
                printf("model %s has %d parameters, the first model of %s has %d \n", name, pn, argv[2 + j], Pj[j]);
                exit(1);
            }
            n++;
        }
#else
        hm[j] = NULL;
        while (fscanf(fl, "%4095s", name) == 1) {
            printf("Model: %s\r\n", name);
            if (n == cap) {
                cap = cap ? 2 * cap : 32;
                hm[j] = (ghmm_host_model *)realloc(hm[j], (size_t)cap * GHMM_MAX_STREAMS * sizeof(ghmm_host_model));
                if (!hm[j]) die("memory", GHMM_ERR_ALLOC);
            }
            int pn = 0;
            if ((rc = ghmm_hmm_read_streams(name, &hm[j][(size_t)n * GHMM_MAX_STREAMS], GHMM_MAX_STREAMS, &pn)))
                die("reading model", rc);
            if (n == 0) Pj[j] = pn;
            if (pn != Pj[j]) {
                printf("model %s has %d parameters, the first model of %s has %d \n", name, pn, argv[2 + j], Pj[j]);
                exit(1);
            }
            n++;
        }
#endif
        fclose(fl);
        if (j > 0 && n != word_number) {
            printf("model list %s holds %d models, expected %d \n", argv[2 + j], n, word_number);
            exit(1);
        }
        word_number = n;
    }
    if (word_number == 0) {
        printf("no models in %s \n", argv[2]);
        exit(1);
    }
    if (gram && gram_K != word_number) {
        printf("grammar file %s is for %d words, the model list %s holds %d \n", env_gram, gram_K, argv[2], word_number);
        exit(1);
    }
    if (gram) /* the flat penalty on top of every pair score */
        for (size_t i = 0; i < (size_t)gram_K * gram_K; i++) gram[gram_K + i] += word_penalty;
    char **word = (char **)malloc((size_t)word_number * sizeof(char *));
#ifdef GHMM_FULL_COV
    for (int k = 0; k < word_number; k++) word[k] = fhm[K - 1][(size_t)k * GHMM_MAX_STREAMS].word; /* RC:229 */
#else
    for (int k = 0; k < word_number; k++) word[k] = hm[K - 1][(size_t)k * GHMM_MAX_STREAMS].word; /* RF:229 */
#endif
    int n_lists = 0;
    for (int j = 0; j < K; j++) n_lists += Pj[j];
    if (argc != 2 * K + n_lists + 4) usage();

    /* spoken words and their feature files, read once */
    FILE *fw = open_read(word_file);
    /* one feature list per (set, stream), in command-line order (RF:253-262) */
    FILE *ff[MAX_SETS][GHMM_MAX_STREAMS];
    const char *ffname[MAX_SETS][GHMM_MAX_STREAMS];
    for (int j = 0, q = 0; j < K; j++)
        for (int p = 0; p < Pj[j]; p++, q++) {
            ffname[j][p] = argv[2 + 2 * K + q];
            ff[j][p] = open_read(ffname[j][p]);
        }
    char (*spoken)[256] = NULL;
    int n_utt = 0, cap_u = 0;
    double *X[MAX_SETS][GHMM_MAX_STREAMS] = {{0}};
    size_t frames[MAX_SETS][GHMM_MAX_STREAMS] = {{0}}, capx[MAX_SETS][GHMM_MAX_STREAMS] = {{0}};
    int32_t *len[MAX_SETS] = {0};
    int D[MAX_SETS][GHMM_MAX_STREAMS] = {{0}};
    char w[4096], path[4096];
    while (fscanf(fw, "%4095s", w) == 1) {
        if (n_utt == cap_u) {
            cap_u = cap_u ? 2 * cap_u : 64;
            spoken = realloc(spoken, (size_t)cap_u * sizeof *spoken);
            for (int j = 0; j < K; j++) len[j] = (int32_t *)realloc(len[j], (size_t)cap_u * sizeof(int32_t));
            if (connected || align) utt_name = (char **)realloc(utt_name, (size_t)cap_u * sizeof(char *));
            if (align) utt_words = (char **)realloc(utt_words, (size_t)cap_u * sizeof(char *));
        }
        snprintf(spoken[n_utt], sizeof spoken[n_utt], "%s", w);
        if (align && !(utt_words[n_utt] = strdup(w))) die("memory", GHMM_ERR_ALLOC);
        for (int j = 0; j < K; j++)
            for (int p = 0; p < Pj[j]; p++) {
                if (fscanf(ff[j][p], "%4095s", path) != 1) {
                    printf("reading error on file %s \n", ffname[j][p]);
                    exit(1);
                }
                int d, T;
                double *x;
                if ((rc = ghmm_perfil_read(path, &d, &T, &x))) die("reading", rc);
                if (n_utt == 0) D[j][p] = d;
                if (d != D[j][p]) {
                    printf("file %s has %d coefficients per frame, expected %d \n", path, d, D[j][p]);
                    exit(1);
                }
                if (p == 0) len[j][n_utt] = T;
                if ((connected || align) && p == 0 && !(utt_name[n_utt] = strdup(path))) die("memory", GHMM_ERR_ALLOC);
                if (T != len[j][n_utt]) {
                    printf("file %s has %d frames, parameter 1 of the same utterance has %d \n", path, T, len[j][n_utt]);
                    exit(1);
                }
                if (frames[j][p] + (size_t)T > capx[j][p]) {
                    capx[j][p] = (frames[j][p] + (size_t)T) * 2;
                    X[j][p] = (double *)realloc(X[j][p], capx[j][p] * (size_t)d * sizeof(double));
                    if (!X[j][p]) die("memory", GHMM_ERR_ALLOC);
                }
                memcpy(X[j][p] + frames[j][p] * (size_t)d, x, (size_t)T * (size_t)d * sizeof(double));
                ghmm_free(x);
                frames[j][p] += (size_t)T;
            }
        n_utt++;
    }
    fclose(fw);
    for (int j = 0; j < K; j++)
        for (int p = 0; p < Pj[j]; p++) fclose(ff[j][p]);

    f_out = fopen(output_file, "w");
    if (!f_out) {
        printf("can't open file %s \n", output_file);
        exit(1);
    }
    if (align) {
        /* the transcripts: every token's names, joined by '+', as indices into the vocabulary */
        int32_t *seq = NULL, *seq_off = (int32_t *)malloc(((size_t)n_utt + 1) * sizeof(int32_t));
        size_t n_seq = 0, cap_seq = 0;
        if (!seq_off) die("memory", GHMM_ERR_ALLOC);
        seq_off[0] = 0;
        for (int u = 0; u < n_utt; u++) {
            for (char *tok = strtok(utt_words[u], "+"); tok; tok = strtok(NULL, "+")) {
                int k = 0;
                while (k < word_number && strcmp(tok, word[k]) != 0) k++;
                if (k == word_number) {
                    printf("utterance %s: word %s of its transcript is not in the vocabulary \n", utt_name[u], tok);
                    exit(1);
                }
                if (n_seq == cap_seq) {
                    cap_seq = cap_seq ? 2 * cap_seq : 256;
                    if (!(seq = (int32_t *)realloc(seq, cap_seq * sizeof(int32_t)))) die("memory", GHMM_ERR_ALLOC);
                }
                seq[n_seq++] = k;
            }
            seq_off[u + 1] = (int32_t)n_seq;
        }
        if (!seq && !(seq = (int32_t *)calloc(1, sizeof(int32_t)))) die("memory", GHMM_ERR_ALLOC);
#ifdef GHMM_FULL_COV
        fprintf(f_out, "Forced alignment using Continuous HMM (full covariance matrix): Viterbi over every utterance's transcript \n");
        if (n_utt > 0) run_connected(fhm[0], word_number, Pj[0], X[0], len[0], n_utt, D[0], 0.0, utt_name, seq, seq_off, NULL, 0);
#else
        fprintf(f_out, "Forced alignment using Continuous HMM (diagonal covariance matrix): Viterbi over every utterance's transcript \n");
        if (n_utt > 0) run_connected(hm[0], word_number, Pj[0], X[0], len[0], n_utt, D[0], 0.0, utt_name, seq, seq_off, NULL, 0);
#endif
        if (ferror(f_out) || fclose(f_out) != 0) {
            printf("writing error on file %s \n", output_file);
            exit(1);
        }
        free(seq); free(seq_off);
        return 0;
    }
    if (connected) {
#ifdef GHMM_FULL_COV
        fprintf(f_out, "Connected word recognition using Continuous HMM (full covariance matrix): Viterbi over the vocabulary, word penalty %g", word_penalty);
        if (gram) fprintf(f_out, ", grammar %s", env_gram);
        if (confidence) fprintf(f_out, ", word confidences (mean frame posterior), then the score and log P");
        fprintf(f_out, " \n");
        if (n_utt > 0) run_connected(fhm[0], word_number, Pj[0], X[0], len[0], n_utt, D[0], word_penalty, utt_name, NULL, NULL, gram, confidence);
#else
        fprintf(f_out, "Connected word recognition using Continuous HMM (diagonal covariance matrix): Viterbi over the vocabulary, word penalty %g", word_penalty);
        if (gram) fprintf(f_out, ", grammar %s", env_gram);
        if (confidence) fprintf(f_out, ", word confidences (mean frame posterior), then the score and log P");
        fprintf(f_out, " \n");
        if (n_utt > 0) run_connected(hm[0], word_number, Pj[0], X[0], len[0], n_utt, D[0], word_penalty, utt_name, NULL, NULL, gram, confidence);
#endif
        if (ferror(f_out) || fclose(f_out) != 0) {
            printf("writing error on file %s \n", output_file);
            exit(1);
        }
        return 0;
    }
#ifdef GHMM_FULL_COV
    /* writing_header, RC:1019-1033 (coef_model is a double there) */
    fprintf(f_out, "Isolated word recognition using Continuous HMM. It is considered full covariance matrix.\n");
    fprintf(f_out, log_score ? "Algorithm used for recognition: Forward (log domain) \n"
                             : "Algorithm used for recognition: Forward \n");
    fprintf(f_out, "Number of models: %d  \n", K);
    for (int i = 0; i < K; i++) {
        fprintf(f_out, "Model name %d: %s\n", i + 1, argv[2 + i]);
        fprintf(f_out, "Weighting coefficient of model %d:%.2f\n", i + 1, coef_model[i]);
    }
#else
    /* writing_header, RF:1014-1031.  The reference declares coef_model as int* there
       and prints it with %.2d: the integer words of the double array are shown. */
    fprintf(f_out, "Isolated word recognition using Continuous HMM (diagonal covariance matrix). It is considered a final state. \n");
    fprintf(f_out, log_score ? "Algorithm used for recognition: Forward (log domain) \n"
                             : "Algorithm used for recognition: Forward \n");
    fprintf(f_out, "Number of models: %d  \n", K);
    for (int i = 0; i < K; i++) {
        int as_int;
        memcpy(&as_int, (const char *)coef_model + sizeof(int) * (size_t)i, sizeof as_int);
        fprintf(f_out, "Model name %d: %s\n", i + 1, argv[2 + i]);
        fprintf(f_out, "Weighting coefficient of model %d:%.2d\n", i + 1, as_int);
    }
#endif
    fprintf(f_out, "Date and time: %s \n\n", date_time);

    /* score[k][u] = sum_j w_j log P(utterance u | model k of set j), RF:366 */
    double *score = (double *)calloc((size_t)word_number * (size_t)(n_utt ? n_utt : 1), sizeof(double));
    double *part = (double *)malloc((size_t)(n_utt ? n_utt : 1) * sizeof(double));
    double old_aux = cpu_units();
    printf("\r\nStarting Tests\r\n");
    if (n_utt > 0) {
        ghmm_ctx *ctx;
        if ((rc = ghmm_ctx_create(0, NULL, &ctx))) die("GPU context", rc);
#ifdef GHMM_FULL_COV
        for (int j = 0; j < K; j++) {
            /* the whole vocabulary in one batched call on the product of the streams' densities (RC:760-789)
               when the words share every stream's M (ghmm_score_full_streams_batch; with one stream that is
               ghmm_score_full_batch), model by model otherwise (ghmm_score_full_streams; with one stream
               ghmm_score_full); GHMM_LOG_SCORE=1: their log-domain counterparts without the final-state term */
            const int P = Pj[j];
            ghmm_corpus *corpus[GHMM_MAX_STREAMS];
            for (int p = 0; p < P; p++)
                if ((rc = ghmm_corpus_create(ctx, X[j][p], len[j], n_utt, D[j][p], &corpus[p]))) die("corpus", rc);
            ghmm_fmodel **fm = (ghmm_fmodel **)calloc((size_t)word_number * GHMM_MAX_STREAMS, sizeof(ghmm_fmodel *));
            double *all = (double *)malloc((size_t)word_number * (size_t)n_utt * sizeof(double));
            if (!fm || !all) die("memory", GHMM_ERR_ALLOC);
            int same = 1;
            for (int k = 0; k < word_number; k++)
                for (int p = 0; p < P; p++) {
                    ghmm_host_fmodel *m = &fhm[j][(size_t)k * GHMM_MAX_STREAMS + p];
                    if (m->D != D[j][p]) {
                        printf("model %s has %d coefficients, data has %d \n", m->word, m->D, D[j][p]);
                        exit(1);
                    }
                    if (m->M != fhm[j][p].M) same = 0;
                    ghmm_fmodel **slot = &fm[(size_t)k * GHMM_MAX_STREAMS + p];
                    if ((rc = ghmm_fmodel_create(ctx, m->N, m->M, m->D, slot))) die("model", rc);
                    if ((rc = ghmm_fmodel_set(ctx, *slot, m->A, m->c, m->mean, m->inv_cov, m->det))) die("model", rc);
                }
            if (same) {
                /* flat[k * P + p]: the layout of the batched calls (P == 1: ghmm_score_full_batch's) */
                ghmm_fmodel **flat = (ghmm_fmodel **)malloc((size_t)word_number * P * sizeof(ghmm_fmodel *));
                if (!flat) die("memory", GHMM_ERR_ALLOC);
                for (int k = 0; k < word_number; k++)
                    for (int p = 0; p < P; p++) flat[(size_t)k * P + p] = fm[(size_t)k * GHMM_MAX_STREAMS + p];
                if ((rc = log_score ? ghmm_logscore_full_streams_batch(ctx, flat, word_number, corpus, P, 0, all)
                                    : ghmm_score_full_streams_batch(ctx, flat, word_number, corpus, P, all)))
                    die("scoring", rc);
                free(flat);
            } else {
                /* (one stream: ghmm_logscore_full / ghmm_score_full themselves) */
                for (int k = 0; k < word_number; k++) {
                    ghmm_fmodel **mk = &fm[(size_t)k * GHMM_MAX_STREAMS];
                    double *dst = all + (size_t)k * n_utt;
                    if ((rc = log_score ? ghmm_logscore_full_streams(ctx, mk, corpus, P, 0, dst)
                                        : ghmm_score_full_streams(ctx, mk, corpus, P, dst)))
                        die("scoring", rc);
                }
            }
            for (int k = 0; k < word_number; k++) {
                for (int u = 0; u < n_utt; u++)
                    score[(size_t)k * n_utt + u] += coef_model[j] * all[(size_t)k * n_utt + u];
                for (int p = 0; p < P; p++) ghmm_fmodel_destroy(ctx, fm[(size_t)k * GHMM_MAX_STREAMS + p]);
            }
            free(fm);
            free(all);
            for (int p = 0; p < P; p++) ghmm_corpus_destroy(ctx, corpus[p]);
        }
#else
        for (int j = 0; j < K; j++) {
            const int P = Pj[j];
            ghmm_corpus *corpus[GHMM_MAX_STREAMS];
            for (int p = 0; p < P; p++)
                if ((rc = ghmm_corpus_create(ctx, X[j][p], len[j], n_utt, D[j][p], &corpus[p]))) die("corpus", rc);
            /* the whole vocabulary in one batched call on the product of the streams' densities when the
               words share every stream's M and D (ghmm_score_streams_batch; with one stream that is
               ghmm_score_batch), model by model otherwise (ghmm_score_streams); GHMM_LOG_SCORE=1: their
               log-domain counterparts with final_state = 1, the final-state term kept */
            ghmm_model **dm = (ghmm_model **)calloc((size_t)word_number * GHMM_MAX_STREAMS, sizeof(ghmm_model *));
            double *all = (double *)malloc((size_t)word_number * (size_t)n_utt * sizeof(double));
            if (!dm || !all) die("memory", GHMM_ERR_ALLOC);
            int same = 1;
            for (int k = 0; k < word_number; k++)
                for (int p = 0; p < P; p++) {
                    ghmm_host_model *m = &hm[j][(size_t)k * GHMM_MAX_STREAMS + p];
                    if (m->D != D[j][p]) {
                        printf("model %s has %d coefficients, data has %d \n", m->word, m->D, D[j][p]);
                        exit(1);
                    }
                    if (m->M != hm[j][p].M) same = 0;
                    ghmm_model **slot = &dm[(size_t)k * GHMM_MAX_STREAMS + p];
                    if ((rc = ghmm_model_create(ctx, m->N, m->M, m->D, slot))) die("model", rc);
                    if ((rc = ghmm_model_set(ctx, *slot, m->A, m->c, m->mean, m->inv_var, m->det))) die("model", rc);
                }
            if (same) {
                /* flat[k * P + p]: the layout of the batched call (P == 1: ghmm_score_batch's) */
                ghmm_model **flat = (ghmm_model **)malloc((size_t)word_number * P * sizeof(ghmm_model *));
                if (!flat) die("memory", GHMM_ERR_ALLOC);
                for (int k = 0; k < word_number; k++)
                    for (int p = 0; p < P; p++) flat[(size_t)k * P + p] = dm[(size_t)k * GHMM_MAX_STREAMS + p];
                if ((rc = log_score ? ghmm_logscore_streams_batch(ctx, flat, word_number, corpus, P, 1, all)
                                    : ghmm_score_streams_batch(ctx, flat, word_number, corpus, P, all)))
                    die("scoring", rc);
                free(flat);
            } else {
                for (int k = 0; k < word_number; k++) {
                    ghmm_model **mk = &dm[(size_t)k * GHMM_MAX_STREAMS];
                    double *dst = all + (size_t)k * n_utt;
                    if ((rc = log_score ? ghmm_logscore_streams(ctx, mk, corpus, P, 1, dst)
                                        : ghmm_score_streams(ctx, mk, corpus, P, dst)))
                        die("scoring", rc);
                }
            }
            for (int k = 0; k < word_number; k++) {
                for (int u = 0; u < n_utt; u++)
                    score[(size_t)k * n_utt + u] += coef_model[j] * all[(size_t)k * n_utt + u];
                for (int p = 0; p < P; p++) ghmm_model_destroy(ctx, dm[(size_t)k * GHMM_MAX_STREAMS + p]);
            }
            free(dm);
            free(all);
            for (int p = 0; p < P; p++) ghmm_corpus_destroy(ctx, corpus[p]);
        }
#endif
        ghmm_ctx_destroy(ctx);
    }

    /* bookkeeping and report, RF:283-412 */
    int correct = 0, error = 0, second = 0, sum_correct = 0, sum_error = 0, sum_second = 0;
    int word_frames = 0, total_frames = 0;
    double cpu_time, sum_cpu_time = 0.0, aux;
    int *index = (int *)malloc((size_t)word_number * sizeof(int));
    int *wrong_word = (int *)calloc((size_t)word_number, sizeof(int));
    double *probab = (double *)malloc((size_t)word_number * sizeof(double));
    char last_word[256] = " ";
    for (int u = 0; u < n_utt; u++) {
        printf("\r\nSpoken word: %s", spoken[u]);
        if (strcmp(last_word, spoken[u]) != 0) {
            if (strcmp(last_word, " ") != 0) {
                aux = cpu_units();
                cpu_time = aux - old_aux;
                old_aux = aux;
                sum_cpu_time += cpu_time;
                report_word(correct, error, second, word_number, last_word, wrong_word, word, cpu_time,
                            word_frames);
                sum_correct += correct;
                sum_error += error;
                sum_second += second;
                total_frames += word_frames;
                word_frames = 0;
                correct = error = second = 0;
                for (int i = 0; i < word_number; i++) wrong_word[i] = 0;
            }
            fprintf(f_out, "\nSpoken word: %s\n", spoken[u]);
        }
        for (int k = 0; k < word_number; k++) probab[k] = score[(size_t)k * n_utt + u];
        word_frames += len[K - 1][u];
        rank_scores(probab, index, word_number);
        printf("\r\nWriting result\r\n");
        for (int i = 0; i < word_number; i++) printf("%s :  %f \n", word[index[i]], probab[index[i]]);
        printf("\n");
        if (strcmp(spoken[u], word[index[0]]) == 0) {
            correct++;
        } else {
            error++;
            wrong_word[index[0]]++;
            if (word_number > 1 && strcmp(spoken[u], word[index[1]]) == 0) second++;
        }
        snprintf(last_word, sizeof last_word, "%s", spoken[u]);
    }
    printf("\r\nEnding Tests\r\n");
    aux = cpu_units();
    cpu_time = aux - old_aux;
    sum_cpu_time += cpu_time;
    if (n_utt > 0) {
#ifdef GHMM_FULL_COV
        report_word(correct, error, second, word_number, last_word, wrong_word, word, cpu_time, word_frames);
#else
        /* the reference passes models_number where word_number belongs (RF:400) */
        report_word(correct, error, second, K, last_word, wrong_word, word, cpu_time, word_frames);
#endif
        sum_correct += correct;
        sum_error += error;
        sum_second += second;
        total_frames += word_frames;
        /* writing_total_result, RF:1164-1194 */
        int sum = sum_correct + sum_error;
        double per = (double)sum_correct / (double)sum;
        fprintf(f_out, "\nConsidering all the words: \n");
        fprintf(f_out, "Results: \n");
        fprintf(f_out, "Correct words: %d\n", sum_correct);
        fprintf(f_out, "Errors: %d\n", sum_error);
        fprintf(f_out, "Percentagen correct : %.2f%%\n", per * 100.0);
        fprintf(f_out, "Second candidate: %d\n", sum_second);
        fprintf(f_out, "Average recognition time: %.2f sec. \n", sum_cpu_time / sum);
        fprintf(f_out, "Average word length: %d frames \n", total_frames / sum);
    }
    if (ferror(f_out) || fclose(f_out) != 0) {
        printf("writing error on file %s \n", output_file);
        exit(1);
    }
    for (int j = 0; j < K; j++) {
#ifdef GHMM_FULL_COV
        for (int k = 0; k < word_number; k++)
            for (int p = 0; p < Pj[j]; p++) ghmm_host_fmodel_free(&fhm[j][(size_t)k * GHMM_MAX_STREAMS + p]);
        free(fhm[j]);
#else
        for (int k = 0; k < word_number; k++)
            for (int p = 0; p < Pj[j]; p++) ghmm_host_model_free(&hm[j][(size_t)k * GHMM_MAX_STREAMS + p]);
        free(hm[j]);
#endif
        for (int p = 0; p < Pj[j]; p++) free(X[j][p]);
        free(len[j]);
    }
    free(word); free(spoken); free(score); free(part); free(index); free(wrong_word); free(probab);
    return 0;
}
