/*
 * ghmm_fulltrain.c — host numerics of the full-covariance trainer.
 *
 * TFF = train/source/hmm-full-fs/hmm_continuous_full_fs.c, the reference's full-covariance
 * trainer.  What is O(N M D^3) and runs once per iteration or once per job lives here, in the
 * reference's order of operations (the E-step is the HIP part, ghmm_estep_full):
 *   - ghmm_init_model_full: creating_initial_model (TFF:731-1134);
 *   - ghmm_mstep_full_host: updating_transition_probab, updating_mix_param, inv_cov_matrix and
 *     treat_zero_det as main() chains them (TFF:306-345);
 *   - ghmm_inv_cov_full: inv_cov_matrix (TFF:2058-2202) on its own.
 * A Gaussian's matrix slot (ghmm_host_fmodel.inv_cov) is the reference's `cov_matrix`: it holds
 * the inverse covariance after a successful inversion, and whatever inv_cov_matrix left there
 * otherwise (see the quirks below).
 *
 * Written without fused multiply-adds (the reference's build contracts nothing): the products
 * are spelled in the reference's association order.
 */
#include "ghmm.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define FF_DELTA 1        /* TFF:37 */
#define FF_FLOOR 1.0e-5   /* TFF:38 */
#define FF_SPLIT_UP 1.05  /* TFF:1176-1177: the doubling split */
#define FF_SPLIT_DOWN 0.95
#define FF_PASSES 5       /* TFF:1073 */
#define FF_ZERO_DET 1e-20 /* TFF:2242 */

/* ghmm_init.c */
double ghmm_nearest_(const double *x, const double *cells, int n_cells, int D, int *cell);
int ghmm_init_cells_(const double *X, const int32_t *len, int n_utt, int N, int M, int D,
                     double first_up, double first_down, int passes, double *cells);

size_t ghmm_stats_len_full(int N, int M, int D)
{
    const size_t G = (size_t)N * M, DT = (size_t)D * (D + 1) / 2;
    return (size_t)N * N + 2 * (size_t)N + G * (1 + (size_t)D + DT) + 2;
}

/* decomposition (TFF:2058-2096): cov = T D T' with T unit lower triangular; reads the diagonal
   and the lower triangle of cov.  t is D x D, d has D entries. */
static void decomposition(int D, const double *cov, double *d, double *t)
{
    for (int i = 0; i < D; i++) d[i] = 0.0;
    for (int i = 0; i < D - 1; i++) {
        t[i * D + i] = 1.0;
        for (int j = i + 1; j < D; j++) t[i * D + j] = 0.0;
    }
    t[(D - 1) * D + D - 1] = 1.0;
    d[0] = cov[0];
    for (int i = 1; i < D; i++) t[i * D] = cov[i * D] / d[0];
    for (int j = 1; j < D - 1; j++) {
        d[j] = cov[j * D + j];
        for (int k = 0; k < j; k++) d[j] -= t[j * D + k] * t[j * D + k] * d[k];
        for (int i = j + 1; i < D; i++) {
            t[i * D + j] = cov[i * D + j];
            for (int k = 0; k < j; k++) t[i * D + j] -= t[i * D + k] * d[k] * t[j * D + k];
            t[i * D + j] /= d[j];
        }
    }
    const int j = D - 1;
    d[j] = cov[j * D + j];
    for (int k = 0; k < j; k++) d[j] -= t[j * D + k] * t[j * D + k] * d[k];
}

/* inv_triang_matrix (TFF:2118-2142): inverse of the unit lower triangular m, by subdiagonals */
static void inv_triang(int D, const double *m, double *im)
{
    for (int i = 0; i < D - 1; i++) {
        im[i * D + i] = 1.0;
        for (int j = i + 1; j < D; j++) im[i * D + j] = 0.0;
    }
    im[(D - 1) * D + D - 1] = 1.0;
    for (int k = 0; k < D - 1; k++)
        for (int i = k + 1; i < D; i++) {
            const int j = i - k - 1;
            im[i * D + j] = 0.0;
            for (int l = j; l < i; l++) im[i * D + j] -= m[i * D + l] * im[l * D + j];
        }
}

double ghmm_inv_cov_full(int D, double *cov)
{
    if (D < 1 || D > 64 || !cov) return NAN;
    double d[64], t[64 * 64], im[64 * 64];
    decomposition(D, cov, d, t);
    double det = 1.0; /* calc_det (TFF:2020-2032) */
    for (int i = 0; i < D; i++) det *= d[i];
    if (isnan(det)) det = 0.0; /* TFF:2176 */
    /* quirk (TFF:2179): det == 0 leaves the matrix as it came, un-inverted */
    if (det != 0.0) {
        inv_triang(D, t, im);
        for (int i = 0; i < D; i++) {
            cov[i * D + i] = 0.0;
            for (int j = i; j < D; j++) cov[i * D + i] += im[j * D + i] * im[j * D + i] / d[j];
        }
        for (int i = 0; i < D - 1; i++)
            for (int j = i + 1; j < D; j++) {
                cov[i * D + j] = 0.0;
                for (int k = j; k < D; k++) cov[i * D + j] += im[k * D + i] * im[k * D + j] / d[k];
                cov[j * D + i] = cov[i * D + j];
            }
    }
    return det;
}

/* sorting (TFF:1331-1356): indices by decreasing key, adjacent swaps with strict '<' */
static void order_desc(const double *key, int *idx, int n)
{
    int done = 0;
    for (int i = 0; i < n; i++) idx[i] = i;
    while (!done) {
        done = 1;
        for (int i = 0; i < n - 1; i++) {
            const int j = idx[i], k = idx[i + 1];
            if (key[j] < key[k]) {
                idx[i] = k;
                idx[i + 1] = j;
                done = 0;
            }
        }
    }
}

/* changing_zero_coef (TFF:1377-1393) */
static void floor_weights(int M, double *c)
{
    double sum = 0.0;
    for (int k = 0; k < M; k++) {
        if (c[k] < FF_FLOOR) c[k] = FF_FLOOR;
        sum += c[k];
    }
    for (int k = 0; k < M; k++) c[k] /= sum;
}

/* treat_zero_det (TFF:2226-2265) for state i: a Gaussian with det < 1e-20 takes the mean (x1.05),
   matrix, det and half the weight of the Gaussian of largest det in sorting's order, whose mean
   is scaled by 0.95; then the weights are renormalised.  Quirk: with M = 1 the Gaussian is split
   with itself (its mean scaled by 1.05 * 0.95 = 0.9975, its weight c / 2 / (c / 2) = 1). */
static void treat_zero_det(ghmm_host_fmodel *hfm, int i, int *idx, double *key)
{
    const int M = hfm->M, D = hfm->D;
    const size_t DD = (size_t)D * D;
    double *c = hfm->c + (size_t)i * M;
    for (int j = 0; j < M; j++) key[j] = hfm->det[(size_t)i * M + j];
    order_desc(key, idx, M);
    int n = 0;
    for (int j = 0; j < M; j++) {
        const size_t gj = (size_t)i * M + j;
        if (hfm->det[gj] < FF_ZERO_DET) {
            const size_t gl = (size_t)i * M + idx[n++];
            for (int k = 0; k < D; k++) hfm->mean[gj * D + k] = hfm->mean[gl * D + k] * 1.05;
            for (int k = 0; k < D; k++) hfm->mean[gl * D + k] = hfm->mean[gl * D + k] * 0.95;
            memmove(hfm->inv_cov + gj * DD, hfm->inv_cov + gl * DD, DD * sizeof(double));
            hfm->det[gj] = hfm->det[gl];
            c[idx[n - 1]] /= 2.0;
            c[j] = c[idx[n - 1]];
        }
    }
    double sum = 0.0;
    for (int j = 0; j < M; j++) sum += c[j];
    for (int j = 0; j < M; j++) c[j] /= sum;
}

/* the matrix slot of every Gaussian of state-range [0, N) after its covariance has been formed:
   det and inverse (TFF:320-341) */
static void invert_all(ghmm_host_fmodel *hfm, int with_treat)
{
    const int N = hfm->N, M = hfm->M, D = hfm->D;
    const size_t DD = (size_t)D * D;
    int idx[64];
    double key[64];
    int *pidx = M <= 64 ? idx : (int *)malloc((size_t)M * sizeof(int));
    double *pkey = M <= 64 ? key : (double *)malloc((size_t)M * sizeof(double));
    for (int i = 0; i < N; i++) {
        for (int k = 0; k < M; k++) {
            const size_t g = (size_t)i * M + k;
            double *cv = hfm->inv_cov + g * DD;
            if (D > 1) {
                hfm->det[g] = ghmm_inv_cov_full(D, cv);
            } else {
                hfm->det[g] = cv[0];
                cv[0] = 1.0 / cv[0];
            }
        }
        if (D > 1 && with_treat && pidx && pkey) treat_zero_det(hfm, i, pidx, pkey);
    }
    if (pidx != idx) free(pidx);
    if (pkey != key) free(pkey);
}

int ghmm_mstep_full_host(const double *stats, int delta, ghmm_host_fmodel *hfm)
{
    if (!stats || !hfm || !hfm->A || hfm->N <= 0 || hfm->M <= 0 || hfm->D <= 0 || hfm->D > 64 || delta < 0)
        return GHMM_ERR_ARG;
    const int N = hfm->N, M = hfm->M, D = hfm->D, G = N * M;
    const size_t DT = (size_t)D * (D + 1) / 2, DD = (size_t)D * D;
    const double *num_a = stats, *den_a = num_a + (size_t)N * N, *den_c = den_a + N;
    const double *num_c = den_c + N, *num_mu = num_c + G, *num_cov = num_mu + (size_t)G * D;

    /* updating_transition_probab (TFF:1907-1929): num_a is only accumulated inside the band
       i <= j <= i + delta (TFF:1601 of the shared calc_transition_probab); outside it the
       quotient is 0 / den_a = 0 */
    for (int i = 0; i < N; i++)
        if (den_a[i] != 0.0)
            for (int j = 0; j < N; j++)
                hfm->A[(size_t)i * N + j] = (j >= i && j <= i + delta) ? num_a[(size_t)i * N + j] / den_a[i] : 0.0;

    /* updating_mix_param (TFF:1951-2000): upper triangle / num_c, diagonal floor, mirror.
       Quirk: a state with den_c == 0 keeps last iteration's matrix slot, which holds the INVERSE
       covariance; invert_all below inverts it again, as main() does.
       Quirk: num_c == 0 gives 0/0 = NaN means and matrix entries, as in the reference. */
    for (int i = 0; i < N; i++) {
        if (den_c[i] == 0.0) continue;
        for (int j = 0; j < M; j++) {
            const size_t g = (size_t)i * M + j;
            double *cv = hfm->inv_cov + g * DD;
            const double *nc = num_cov + g * DT;
            hfm->c[g] = num_c[g] / den_c[i];
            size_t q = 0;
            for (int k = 0; k < D; k++) {
                hfm->mean[g * D + k] = num_mu[g * D + k] / num_c[g];
                for (int l = k; l < D; l++) cv[k * D + l] = nc[q++] / num_c[g];
            }
            for (int k = 0; k < D; k++)
                if (cv[k * D + k] < FF_FLOOR) cv[k * D + k] = FF_FLOOR;
            for (int k = 1; k < D; k++)
                for (int l = 0; l < k; l++) cv[k * D + l] = cv[l * D + k];
        }
    }
    for (int i = 0; i < N; i++) floor_weights(M, hfm->c + (size_t)i * M);

    /* inv_cov_matrix per Gaussian, then treat_zero_det per state (D > 1), or det = var and
       inverse = 1 / var (D = 1, no treat_zero_det) — TFF:320-341 */
    invert_all(hfm, 1);
    return GHMM_OK;
}

int ghmm_init_model_full(const double *X, const int32_t *len, int n_utt, int N, int M, int D,
                         ghmm_host_fmodel *hfm)
{
    if (!X || !len || n_utt <= 0 || N <= 0 || M <= 0 || D <= 0 || D > 64 || !hfm) return GHMM_ERR_ARG;
    int rc = ghmm_host_fmodel_alloc(hfm, N, M, D);
    if (rc) return rc;

    /* init_transition_probab (TFF:772-791) */
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            double a;
            if (j > FF_DELTA + i || j < i) a = 0.0;
            else if (FF_DELTA + 1 > N - i) a = 1.0 / (double)(N - i);
            else a = 1.0 / (double)(FF_DELTA + 1);
            hfm->A[(size_t)i * N + j] = a;
        }

    /* init_mix_mean (TFF:970-1134): the doubling split x1.05 / x0.95, five passes */
    const size_t DD = (size_t)D * D, G = (size_t)N * M;
    double *cells = (double *)calloc(G * D, sizeof(double)); /* [N][M][D] */
    int *count = (int *)calloc(G, sizeof(int));
    int *dur = (int *)calloc((size_t)N, sizeof(int));
    double *dif = (double *)malloc((size_t)D * sizeof(double));
    if (!cells || !count || !dur || !dif ||
        ghmm_init_cells_(X, len, n_utt, N, M, D, FF_SPLIT_UP, FF_SPLIT_DOWN, FF_PASSES, cells) != GHMM_OK) {
        free(cells); free(count); free(dur); free(dif);
        ghmm_host_fmodel_free(hfm);
        return GHMM_ERR_ALLOC;
    }

    /* init_mix_param (TFF:810-952): the covariance of each cell around its cell mean, upper
       triangle, frames in file order (uniform segmentation, cell index carried between frames) */
    {
        size_t f0 = 0;
        int cell = 0;
        for (int u = 0; u < n_utt; u++) {
            const int T = len[u], q = T / N, r = T % N;
            int end = 0;
            for (int k = 0; k < N; k++) {
                const int begin = end;
                end += k < r ? q + 1 : q;
                for (int j = begin; j < end; j++) {
                    const double *x = X + (f0 + (size_t)j) * D;
                    ghmm_nearest_(x, cells + (size_t)k * M * D, M, D, &cell);
                    const size_t g = (size_t)k * M + cell;
                    for (int l = 0; l < D; l++) dif[l] = x[l] - cells[g * D + l];
                    double *cv = hfm->inv_cov + g * DD;
                    for (int i = 0; i < D; i++)
                        for (int l = i; l < D; l++) cv[i * D + l] += dif[i] * dif[l];
                    count[g]++;
                }
                dur[k] += end - begin;
            }
            f0 += (size_t)T;
        }
    }
    for (size_t g = 0; g < G; g++) {
        double *cv = hfm->inv_cov + g * DD;
        for (int k = 0; k < D; k++)
            for (int l = k; l < D; l++) cv[k * D + l] /= (double)count[g];
        for (int k = 0; k < D; k++)
            if (cv[k * D + k] < FF_FLOOR) cv[k * D + k] = FF_FLOOR;
        for (int k = 1; k < D; k++)
            for (int l = 0; l < k; l++) cv[k * D + l] = cv[l * D + k];
        for (int k = 0; k < D; k++) hfm->mean[g * D + k] = cells[g * D + k];
        hfm->c[g] = (double)count[g];
    }
    /* the inverse and det (inv_cov_matrix; D = 1: det = var, inverse = 1 / var); the initial
       model has no treat_zero_det (TFF:918-930) */
    invert_all(hfm, 0);
    for (int i = 0; i < N; i++) {
        double *c = hfm->c + (size_t)i * M;
        for (int j = 0; j < M; j++) c[j] /= (double)dur[i];
        floor_weights(M, c);
    }
    free(cells); free(count); free(dur); free(dif);
    return GHMM_OK;
}
