/*
 * ghmm.h — C ABI of the MI355X-native continuous-density GMM-HMM core.
 *
 * This is the drop-in boundary for the diagonal-covariance hot path of
 * edielsonpf/speech-recognition-hmm-continuous.  The reference has no library
 * or FFI layer: its numerical core is a set of file-local C functions called
 * from main().  Every entry point below names the reference
 * function(s) it replaces.  Path aliases:
 *
 *   TF = train/source/hmm-fs/hmm_continuous_fs.c            (trainer, diagonal)
 *   RF = test/source/recognition-fs/recognition_continuous_fs.c (recogniser, diagonal)
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns GHMM_OK (0) or an error
 *     code and never calls exit(); ghmm_last_error() holds the detail text.
 *   - all arithmetic on the path is IEEE double ("f64"), like the reference.
 *   - a model is held as flat struct-of-arrays (the reference's `struct state`
 *     TF:53-64 is array-of-structs with fixed capacity):
 *         A[N*N] row-major, c[N*M], mean[N*M*D], inv_var[N*M*D], det[N*M]
 *     with the reference's meaning: inv_var = 1/sigma^2 (TF:2012), det = prod
 *     sigma^2 of the NON-inverted variances (TF:1976), exactly what a .hmm file holds.
 *   - frames are row-major X[F][D] (F = all frames of all utterances, back to
 *     back), i.e. the payload order of the reference's .perfil files (TF:527-544).
 *   - per-frame outputs are frame-major: b[F][N], post[F][N*M], alpha[F][N] ...
 *     (the reference keeps them state-major with a 500-frame cap, TF:107-114).
 *   - one ghmm_ctx per GPU per host thread; no global mutable state.
 *   - the library needs a gfx950 device: ghmm_ctx_create fails with
 *     GHMM_ERR_NODEVICE otherwise.  There is no CPU fallback.
 */
#ifndef GHMM_H
#define GHMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHMM_VERSION 200

enum {
    GHMM_OK = 0,
    GHMM_ERR_ARG = 1,         /* bad argument / shape mismatch */
    GHMM_ERR_ALLOC = 2,       /* host or device allocation failed */
    GHMM_ERR_HIP = 3,         /* a HIP runtime call failed */
    GHMM_ERR_NODEVICE = 4,    /* no usable gfx950 device */
    GHMM_ERR_UNSUPPORTED = 5, /* valid request outside what is built (e.g. more than 512 states in the recursions) */
    GHMM_ERR_IO = 6,          /* file could not be opened / read / written */
    GHMM_ERR_FORMAT = 7       /* file content is not a .perfil / .hmm */
};

const char *ghmm_strerror(int code);
const char *ghmm_last_error(void); /* thread-local detail of the last failure */
int ghmm_version(void);

/* ------------------------------------------------------------------ context */

typedef struct ghmm_ctx ghmm_ctx;

/* `hip_stream` may be NULL (the library creates its own stream) or a
 * hipStream_t owned by the caller (e.g. torch's current stream); every kernel
 * and copy of this context is issued on it. */
int ghmm_ctx_create(int device, void *hip_stream, ghmm_ctx **out);
void ghmm_ctx_destroy(ghmm_ctx *ctx);
int ghmm_ctx_sync(ghmm_ctx *ctx);

enum {
    /* band of transitions that receive statistics: i <= j <= i+delta.
     * The reference hard-codes DELTA 1 (TF:38, TF:1601). Default 1. */
    GHMM_OPT_DELTA = 1,
    /* 0 (default): emission densities in the reference's linear domain
     *    (exp() underflows exactly where the reference's does, TF:1821-1836);
     * 1: per-frame max-normalised densities (the log of the normaliser is added back
     *    into the log-likelihood): finite where the reference's densities underflow as a
     *    whole frame.  It is still a linear-domain recursion: a frame whose REACHABLE states
     *    lie more than ~308 decades below its best state ends the utterance as in the
     *    reference (profiles/fuzz_robust.py). */
    GHMM_OPT_ROBUST = 2,
    /* 0 auto, 1 vector-ALU kernels and the reference's order of the recursions (calc_alpha,
     * then calc_beta scaled by its c_t, one pass each), 2 MFMA (f64 16x16x4) kernels and the
     * forward / backward recursions side by side (what auto picks); 3 is a measurement variant
     * of 2 (statistics kernel with its operands straight from HBM instead of staged through LDS) */
    GHMM_OPT_KERNELS = 3,
    /* 1: bracket every kernel with HIP events on the context's stream */
    GHMM_OPT_TIMING = 4,
    /* number of frame-block partial sums kept by the statistics kernel (0 auto) */
    GHMM_OPT_PARTIALS = 5,
    /* compute units the one-block-per-CU kernels size their grids for (0 = all of the
     * device's, the default): for a caller whose stream is restricted to part of the device
     * (hipExtStreamCreateWithCUMask) */
    GHMM_OPT_CUS = 6,
    /* read-only (ghmm_ctx_get_option; synchronises the stream): utterances the context's last
     * gamma / xi pass took again in the reference's own order of operations — on the default
     * tier no path into the last state, or forward and backward mass more than 200 decades apart
     * at some frame (ghmm_pair.hpp, RANGE); under GHMM_OPT_KERNELS = 1 a band-only beta^ that left
     * the numbers, where a wave takes all of its utterances again when one of them asks.  0 on
     * data the model fits.  The last pass is that of ghmm_estep, ghmm_backward, ghmm_estep_streams,
     * ghmm_estep_full and its stream form, or the one ghmm_fetch(GHMM_BUF_BETA) starts after an
     * E-step (it counts the same utterances).  A pass that takes nothing again by construction
     * reads 0: a model of more than 64 states, ghmm_estep_log and the other log-domain E-steps,
     * ghmm_estep_embed_streams and ghmm_estep_embed_full_streams, a linear E-step on a corpus of no
     * utterances.  Calls that run no
     * gamma / xi pass (scores, Viterbi, ghmm_forward, ghmm_model_init, the embedded E-step on a
     * corpus of no utterances) leave the value as it is, whatever corpus they see. */
    GHMM_OPT_REFORDER_COUNT = 7,
    /* matrix-core tier, Gaussians too ill-conditioned for the expanded sums although their
     * variances are not at the floor ("class 2"): 0 (default) their direct-form sums come from
     * the vector-ALU statistics kernel, launched while the host has recently seen such a
     * Gaussian, and from an exact recomputation inside the reduction otherwise; 1 always
     * launch that kernel; 2 never (always the recomputation).  All three are exact; a
     * measurement / test switch. */
    GHMM_OPT_VEC_STATS = 8,
    /* mixture posteriors (gaus_probab_dens, TF:110) written with non-temporal stores: 0 (default)
     * when they are at most 1 GiB, 1 always, 2 never.  Same bytes either way; a measurement
     * switch (profiles/tools/nt_ab.py). */
    GHMM_OPT_NT_POST = 9,
    /* ghmm_estep's recursions: both scans and the gamma / xi pass in ONE launch (a block scans its
     * utterances with two waves, then all of its waves take the chunks) whenever A is band-diagonal
     * — 0 (default) and 1; 2 = the separate launches.  Same operations either way; a measurement
     * switch (profiles/tools/fused_ab.py). */
    GHMM_OPT_FUSED_SCAN = 10
};
int ghmm_ctx_set_option(ghmm_ctx *ctx, int option, int64_t value);
int ghmm_ctx_get_option(ghmm_ctx *ctx, int option, int64_t *value);

/* kernel ids for ghmm_ctx_kernel_time() */
enum {
    GHMM_K_EMISSION = 0,
    GHMM_K_FORWARD = 1,  /* forward recursion; inside ghmm_estep on a band-diagonal A the one launch that
                          * holds both recursions and the gamma / xi pass (then GHMM_K_BACKWARD counts nothing) */
    GHMM_K_BACKWARD = 2, /* backward recursion's share: gamma / xi pass and the fix-up launch */
    GHMM_K_MIXSTATS = 3,
    GHMM_K_REDUCE = 4,
    GHMM_K_MSTEP = 5,
    GHMM_K_VITERBI = 6,
    GHMM_K_PREPARE = 7,
    GHMM_K_COUNT = 8
};
/* Sum of HIP-event durations and launch count since the last reset (needs
 * GHMM_OPT_TIMING = 1).  Synchronises the context's stream. */
int ghmm_ctx_kernel_time(ghmm_ctx *ctx, int kernel, double *total_ms, int64_t *launches);
int ghmm_ctx_kernel_time_reset(ghmm_ctx *ctx);
const char *ghmm_kernel_name(int kernel);

/* -------------------------------------------------------------------- model */

typedef struct ghmm_model ghmm_model;

/* Device-resident model, one feature stream (the reference's param_number P;
 * every BASELINE configuration uses P = 1). Replaces `struct state
 * state_mix[P][N]` + `transition_probab[N][N]` (TF:104, TF:146). */
int ghmm_model_create(ghmm_ctx *ctx, int N, int M, int D, ghmm_model **out);
void ghmm_model_destroy(ghmm_ctx *ctx, ghmm_model *m);
/* host -> device; also rebuilds the derived per-Gaussian constants
 * (pow(2*pi, D/2) * sqrt(|det|), TF:1821-1827). */
int ghmm_model_set(ghmm_ctx *ctx, ghmm_model *m, const double *A, const double *c,
                   const double *mean, const double *inv_var, const double *det);
/* device -> host (synchronises); any pointer may be NULL */
int ghmm_model_get(ghmm_ctx *ctx, ghmm_model *m, double *A, double *c, double *mean,
                   double *inv_var, double *det);
int ghmm_model_dims(const ghmm_model *m, int *N, int *M, int *D);

/* ------------------------------------------------------------------- corpus */

typedef struct ghmm_corpus ghmm_corpus;

/* A batch of utterances resident in HBM.  `len[u]` = frames of utterance u.
 * _create copies host frames to the device; _wrap adopts a device pointer the
 * caller keeps alive (no copy). Replaces the per-frame fread loop TF:282-288. */
int ghmm_corpus_create(ghmm_ctx *ctx, const double *X_host, const int32_t *len, int n_utt, int D,
                       ghmm_corpus **out);
int ghmm_corpus_wrap(ghmm_ctx *ctx, const double *X_dev, const int32_t *len, int n_utt, int D,
                     ghmm_corpus **out);
void ghmm_corpus_destroy(ghmm_ctx *ctx, ghmm_corpus *c);
int64_t ghmm_corpus_frames(const ghmm_corpus *c);
int ghmm_corpus_utterances(const ghmm_corpus *c);

/* creating_initial_model (TF:732-1317) on the device, from a corpus resident in HBM:
 * ghmm_init_model's definition (ghmm_init.c), written into `m` (its N, M, D).  Synchronises.
 *   Segmentation: uniform, every utterance cut into N runs of T / N frames, the first T % N runs one
 *     frame longer (TF:1005-1013); state i owns run i.  A state that owns no frame gets the host's
 *     0/0 values (NaN mean, inverse variance, det and weights); the other states are not affected.
 *   A: a_ij = 1 / min(2, N - i) for j = i, i + 1, else 0 (TF:774-806).
 *   Cells: the state's mean first; while 2n < M every cell is split x1.005 / x0.995, otherwise the
 *     M - n cells of largest distortion are, in `sorting`'s order (adjacent swaps, strict <,
 *     TF:1289-1315).  Each level runs three nearest-mean passes: squared Euclidean distance summed in
 *     coefficient order, strict < from 1e20, so the lowest cell wins a tie and a cell whose mean is NaN
 *     is never chosen.  After every pass mean = sum / count, and empty cells are re-seeded
 *     x1.005 / x0.995 from the cells of largest distortion, in the host's order.
 *   Variances: one more classification against the final cells; per coefficient the squared
 *     deviations from the CELL MEAN over the count, floored at 1e-5; det = their product in
 *     coefficient order, then inverted; weights = count / (frames of the state), floored at 1e-5 and
 *     renormalised in index order.
 *   One difference: a frame farther than 1e20 from every cell takes cell 0, where the host carries the
 *     previous frame's cell.  Reached only when some frame lies at least 1e10 from every cell of its
 *     state.
 * The sums are added in a fixed order of the device's own, so the values differ from the host's in the
 * last bits; the discrete parts (A, every assignment and count, hence c) are the host's wherever neither a
 * frame nor a distortion that decides a split or a re-seed sits within rounding of a tie.  Two calls on the
 * same inputs give the same bits.  No cap on M (where each part runs).
 * An empty corpus or a corpus of another D: GHMM_ERR_ARG before anything is written.  A failure later on
 * (an allocation, a launch) leaves the model's parameters undefined: set or initialise it again.
 * The context's workspace is overwritten: GHMM_BUF_GAMMA holds the one-hot state rows, GHMM_BUF_POST is
 * refused until the next emission. */
int ghmm_model_init(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c);

/* ---------------------------------------------------- sufficient statistics */

/* Flat Baum-Welch accumulator vector — the ONLY thing that crosses GPUs
 * (one all-reduce(SUM) per EM iteration).  Layout, in doubles:
 *   num_a[N*N]   TF:1614  (only the band i <= j <= i+delta is ever non-zero)
 *   den_a[N]     TF:1618
 *   den_c[N]     TF:1660
 *   num_c[N*M]   TF:1716
 *   num_mu[N*M*D]  TF:1718
 *   num_var[N*M*D] TF:1720-1722 (around the OLD mean)
 *   loglik       TF:318  (sum of per-utterance log P)
 *   n_utt        TF:320
 */
typedef struct ghmm_stats ghmm_stats;
size_t ghmm_stats_len(int N, int M, int D);
int ghmm_stats_create(ghmm_ctx *ctx, int N, int M, int D, ghmm_stats **out);
/* adopt caller-owned device memory of ghmm_stats_len() doubles (e.g. a torch
 * tensor that torch.distributed all-reduces in place) */
int ghmm_stats_wrap(ghmm_ctx *ctx, int N, int M, int D, double *dev_ptr, ghmm_stats **out);
void ghmm_stats_destroy(ghmm_ctx *ctx, ghmm_stats *s);
double *ghmm_stats_device_ptr(ghmm_stats *s);
int ghmm_stats_download(ghmm_ctx *ctx, ghmm_stats *s, double *host);
/* the two numbers the EM driver's stopping rule reads every iteration (TF:318-325):
 * out[0] = sum of log P over the utterances (`probab`), out[1] = utterance count
 * (`exemplar_number`) — a 16-byte download instead of the whole vector; straight behind an
 * E-step into a vector the library owns, a poll of pinned host memory the reduction kernel wrote
 * (returns as soon as the two numbers exist: the stream is NOT drained) */
int ghmm_stats_loglik(ghmm_ctx *ctx, ghmm_stats *s, double out[2]);
int ghmm_stats_upload(ghmm_ctx *ctx, ghmm_stats *s, const double *host);

/* ---------------------------------------------- the path, one row at a time */

/* calc_symbol_probab + calc_gaus, TF:1749-1841 (want_post = 1: also the
 * within-state mixture posteriors `gauss[i][j]`, TF:1773-1778) and RF:860-947
 * (want_post = 0).  Results stay in the context workspace. */
int ghmm_emission(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, int want_post);
/* calc_alpha TF:1380-1443 / RF:739-799 + calc_probability TF:1536-1553.
 * Models of up to 512 states (the reference's cap is 20, TF:41): one state per lane up to 64,
 * one wave per utterance with the states strided over its lanes beyond (GHMM_ERR_UNSUPPORTED
 * above 512; ghmm_viterbi: 255, its back-pointers are bytes). */
int ghmm_forward(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c);
/* calc_beta TF:1463-1516, fused with the per-utterance part of
 * calc_transition_probab TF:1577-1620 and calc_den_mix_coef TF:1642-1664 */
int ghmm_backward(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c);
/* calc_mix_param TF:1691-1727 over every frame, then the ordered reduction of
 * all partial sums into `stats`.  GHMM_ERR_ARG, before anything is launched, unless the emission that
 * owns the workspace wrote its mixture posteriors there (ghmm_emission with want_post = 1). */
int ghmm_accumulate(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, ghmm_stats *stats);

/* workspace buffers readable with ghmm_fetch (all double, frame-major) */
enum {
    GHMM_BUF_B = 0,      /* b[F][N]        symbol_probab        TF:107 */
    GHMM_BUF_POST = 1,   /* post[F][N*M]   gaus_probab_dens     TF:110; GHMM_ERR_ARG when the emission that
                          * owns the workspace wrote none (want_post = 0, a score or Viterbi call) or kept
                          * them per stream (ghmm_estep_streams, n_streams > 1) */
    GHMM_BUF_ALPHA = 2,  /* alpha^[F][N]                        TF:112 */
    GHMM_BUF_BETA = 3,   /* beta^[F][N]                         TF:114; after ghmm_estep it is formed on
                          * this call (the E-step itself only needs gamma and xi) */
    GHMM_BUF_SCALE = 4,  /* c_t[F]         scaling_factor       TF:116 */
    GHMM_BUF_GAMMA = 5,  /* gamma[F][N] = alpha^*beta^/c_t      TF:1657 */
    GHMM_BUF_LOGLIK = 6, /* log P per utterance [U]             TF:1536 */
    GHMM_BUF_LOGNORM = 7 /* log of the per-frame normaliser [F] (GHMM_OPT_ROBUST) */
};
int ghmm_fetch(ghmm_ctx *ctx, int which, double *host, size_t n_doubles);
/* the same for doubles [first, first + n_doubles) of the buffer (e.g. a block of frames of a
 * b[F][N] too large for host memory: BASELINE's 2 000-state x 1 M-frame emission is 16 GB) */
int ghmm_fetch_range(ghmm_ctx *ctx, int which, size_t first, double *host, size_t n_doubles);

/* -------------------------------------------------- the path, batched/fused */

/* One E-step over the whole corpus: emission -> forward and backward recursions ->
 * gamma / xi -> statistics -> ordered reduction (TF:244-321).  `stats` is overwritten (the
 * zeroing of TF:244-270 is implied).  Asynchronous on the context's stream. */
int ghmm_estep(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, ghmm_stats *stats);
/* M-step from (possibly all-reduced) statistics, on the device, in place:
 * updating_transition_probab TF:1862-1889, updating_mix_param TF:1911-1955 with
 * changing_zero_coef TF:1338-1359, calc_det TF:1976 + inv_matrix TF:2012 as
 * called at TF:343-346.  num_a is read inside the band i <= j <= i + GHMM_OPT_DELTA only —
 * the only entries calc_transition_probab ever accumulates (TF:1601); a_ij outside it
 * becomes 0 / den_a = 0 as in the reference.  Asynchronous.
 * A, c, mean, inv_var and det are the reference's BIT FOR BIT (a NaN's sign and payload aside; A outside
 * the band as above): correctly rounded divisions, a sum and a product in index order, on every shape
 * (tests/test_mstep_gpu.py).  Its quirks, all the reference's:
 *   updating_transition_probab (TF:1862-1889): a row with den_a == 0 is kept as it was, its entries
 *     outside the band included (only an updated row is masked).
 *   updating_mix_param (TF:1911-1955): a state with den_c == 0 is skipped: mean as it was, and its
 *     variance slot, which holds last iteration's INVERSE variances, goes through calc_det / inv_matrix
 *     again: det = their product, inv_var = 1 / inv_var.  num_c == 0 in an updated state: 0/0 mean and
 *     variances.  Variances below 1e-5 become 1e-5, negative ones (rounding) included; a NaN variance is
 *     NOT floored (NaN < 1e-5 is false) and gives a NaN det.
 *   changing_zero_coef (TF:1338-1359) on every state, skipped ones too: weights below 1e-5 become 1e-5,
 *     then all are divided by their sum taken in index order.
 *   calc_det (TF:1976): det = the product of the D variances in index order: it may underflow to a
 *     subnormal or to 0 (every variance at the floor: 1e-320 at D = 64, 0 from D = 65) or overflow to inf.
 * The derived constants are den = pow(2 pi, D/2) * sqrt(|det|), wk = c / den, logwk = log(c) - log(den),
 * log a = a > 0 ? log(a) : -inf, by the expressions ghmm_model_set uses (the same bits).  A subnormal det
 * is an ordinary value (sqrt(1e-320) = 1e-160).  det == 0: wk = +inf and logwk = +inf; det == inf: wk = 0
 * and logwk = -inf; NaN det: NaN both: the next emission carries them as the reference's calc_gaus would. */
int ghmm_mstep(ghmm_ctx *ctx, ghmm_model *m, ghmm_stats *stats);
/* The extended Baum-Welch (EBW) update of discriminative (MMI) training, on the device, in place, asynchronous
 * (diagonal models; the reference has no such call).  `num` holds the numerator statistics (the transcripts':
 * ghmm_estep_embed_streams, ghmm_estep_log, ...) and `den` the denominator statistics (every word string the
 * grammar allows: ghmm_estep_grammar_streams), both possibly all-reduced, both of m's shape.  m must be the
 * model BOTH vectors were accumulated on: num_var is taken around the old mean (see ghmm_stats).
 * Per Gaussian g = (i, m) and coefficient d, with mu = mean, s2 = 1 / inv_var, cn = num.num_c[g],
 * cd = den.num_c[g]:
 *   dc     = cn - cd
 *   dm_d   = (num.num_mu - den.num_mu)[g,d] - dc * mu_d          the first moment around the old mean
 *   dv_d   = (num.num_var - den.num_var)[g,d]                    the second moment around the old mean
 *   r_d    = the larger real root of q_d(x) = s2_d x^2 + (dv_d + s2_d dc) x + (dv_d dc - dm_d^2), 0 if negative
 *   damp   = max(E * cd, 2 * max_d r_d)
 *   mu'_d  = mu_d + dm_d / (dc + damp)
 *   s2'_d  = (dv_d + damp s2_d) / (dc + damp) - (mu'_d - mu_d)^2, then floored at 1e-5 as ghmm_mstep floors
 * (dc + damp)^2 s2'_d = q_d(damp), and q_d(-dc) = -dm_d^2 <= 0, so -dc does not lie beyond the larger root:
 * for damp beyond it both dc + damp and q_d(damp) are positive, and s2'_d > 0 before the floor.  (The
 * discriminant of q_d is (dv_d - s2_d dc)^2 + 4 s2_d dm_d^2 >= 0: the roots are always real, and it is formed so.)
 * A Gaussian whose dc + damp is not a positive finite number (no statistics at all) keeps its mean, its
 * variances and its det.  The sums inside a Gaussian run in index order; the divisions are correctly rounded;
 * the results are pinned by tolerance against a long-double restatement (tests/ebw_cases.py), not to the bit.
 * Weights and transitions come from the NUMERATOR alone, by ghmm_mstep's expressions, band mask, floors and
 * quirks, bit for bit what ghmm_mstep(m, num) gives: a = num.num_a / num.den_a inside i <= j <= i +
 * GHMM_OPT_DELTA and 0 outside, a row with den_a == 0 kept; c = num.num_c / num.den_c through
 * changing_zero_coef, a state with num.den_c == 0 keeping its weights (floored and renormalised all the same).
 * Unlike ghmm_mstep a state with num.den_c == 0 does NOT have its variance slot inverted again: its Gaussians
 * follow the rule above like any other.  det = the product of the new variances in index order; den, wk, logwk
 * and log a by ghmm_mstep's expressions.  The model's band flag becomes `was banded && delta <= 1`.
 * Afterwards the model is prepared as after ghmm_model_set (a new epoch, the matrix-core form), so the next
 * emission on either kernel tier sees it.  There is no acoustic or grammar scale and no I-smoothing: E is the
 * only constant.  ONE launch under GHMM_K_MSTEP (k_mstep_ebw, block = state), then the preparation's.
 * GHMM_ERR_ARG, before anything is launched or written: a null argument, a vector of another shape, a
 * full-covariance vector, E negative, NaN or infinite. */
int ghmm_mstep_ebw(ghmm_ctx *ctx, ghmm_model *m, ghmm_stats *num, ghmm_stats *den, double E);
/* Forward-algorithm score per utterance (RF:354-366): emission without
 * posteriors + the forward recursion + log P.  Synchronises, writes loglik[U] on the host.
 * (Only log P is kept: alpha^ and c_t stay in registers; ghmm_forward leaves them in the workspace.) */
int ghmm_score(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, double *loglik_host);
/* The recogniser's whole vocabulary loop (RF:326-374) in two launches: ONE emission launch
 * over the concatenated Gaussians of all `n_models` word models and ONE forward launch
 * over every (model, utterance) pair.  All models must share M and D (states may
 * differ).  loglik_host[k*U + u] = log P(utterance u | model k).  Synchronises. */
int ghmm_score_batch(ghmm_ctx *ctx, ghmm_model *const *models, int n_models, ghmm_corpus *c,
                     double *loglik_host);
/* Several feature streams (param_number P > 1): every recursion runs on the product over streams
 * of the emission densities, b_i(t) = prod_p b^p_i(t) in stream order (calc_alpha TF:1406-1409 /
 * 1429-1432, calc_beta TF:1501-1504, calc_transition_probab TF:1607-1610); calc_symbol_probab
 * (TF:278-288) and calc_mix_param (TF:306-315) run once per stream with that stream's own
 * mixtures and posteriors.  models[p] / corpora[p] / stats[p] = stream p: same states, same
 * utterances and lengths, own M_p and D_p; the transitions are models[0]'s.  stats[p] has the
 * single-stream layout (the common sums are written into every one), so that ghmm_mstep(models[p],
 * stats[p]) for every p is the M-step (TF:332-346: all of them write the same A).
 *   1 <= n_streams <= GHMM_MAX_STREAMS;  n_streams == 1 is the single-stream call itself (ghmm_estep,
 *   ghmm_score): the same bits.
 * The product: every stream's emission is the launch ghmm_emission makes for that stream alone, stream 0
 * into b, every later stream into a buffer of its own that one IEEE multiply per entry folds into b,
 * the earlier streams' product on the left: b = ((b^0 * b^1) * b^2)..., which is the reference's
 * `product = 1.0; product *= ...` since 1.0 * b^0 == b^0.  Zeros, subnormal values, NaN and inf
 * propagate as the multiplication gives them; a frame whose product is 0 in every state ends its
 * utterance as in the reference (c_t = 1/0, log P NaN, NaN statistics).
 * Asynchrony, reproducibility (a second identical call repeats every vector bit for bit), GHMM_OPT_DELTA,
 * GHMM_OPT_PARTIALS, GHMM_OPT_KERNELS and GHMM_OPT_VEC_STATS are the single-stream calls'; utterances are
 * taken again in the reference's order as there (GHMM_OPT_REFORDER_COUNT).
 * The common sums (num_a, den_a, den_c, loglik, n_utt) are reduced once per stream from the same partial
 * sums in the same order: they are the same bits in every stream's vector, and every stream's ghmm_mstep
 * writes the same A bit for bit.
 * Afterwards GHMM_BUF_B holds the product and GHMM_BUF_ALPHA / _BETA / _SCALE / _GAMMA / _LOGLIK are as
 * after the single-stream call on it.  The workspace belongs to stream 0's (model, corpus) pair:
 * ghmm_forward and ghmm_backward on that pair run on the product.  The mixture posteriors lie in one
 * buffer per stream that ghmm_fetch does not serve: ghmm_fetch / ghmm_fetch_range(GHMM_BUF_POST) and
 * ghmm_accumulate return GHMM_ERR_ARG until a ghmm_emission(want_post = 1) or ghmm_estep has written
 * posteriors of its own (the same holds after ghmm_emission(want_post = 0), ghmm_score, ghmm_score_batch
 * and ghmm_viterbi: the workspace never serves the posteriors of an earlier emission).
 * Refusals, each before anything is launched or written: GHMM_OPT_ROBUST set with n_streams > 1 gives
 * GHMM_ERR_UNSUPPORTED; a null array or entry, n_streams outside the range, streams that differ in N, in
 * the utterance count or in a length, a corpus of another D than its model, or a statistics vector that
 * is full-covariance or not of its stream's shape gives GHMM_ERR_ARG.
 * Viterbi and the batched vocabulary calls on several streams are in the section "several-stream
 * vocabularies of diagonal models" below (ghmm_viterbi_streams, ghmm_score_streams_batch,
 * ghmm_viterbi_streams_batch, ghmm_recognise_streams). */
int ghmm_estep_streams(ghmm_ctx *ctx, ghmm_model *const *models, ghmm_corpus *const *corpora,
                       int n_streams, ghmm_stats *const *stats);
/* forward score per utterance of a P-stream model (RF:349-366) */
int ghmm_score_streams(ghmm_ctx *ctx, ghmm_model *const *models, ghmm_corpus *const *corpora,
                       int n_streams, double *loglik_host);

/* Max-plus lattice with the reference's one-hot start (RF:249-251) and
 * final-state termination (TF:1487, TF:1549); ties take the lowest predecessor.
 * ABSENT from the reference: defined by oracle/.
 * path_host[F] = state per frame, score_host[U] = best log score.  (The device keeps
 * one byte per frame; it is widened to int32 on the way into path_host.) */
int ghmm_viterbi(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, int32_t *path_host,
                 double *score_host);

/* The forward score of a diagonal model in the log domain (absent from the reference): the sum over
 * paths where ghmm_viterbi takes the best one, on the same log b and log A.
 *     log b_j(t)  what ghmm_viterbi's emission launch writes (either tier)
 *     log a_ij    the model's log A: a_ij > 0 ? log(a_ij) : -inf
 * The lattice is ghmm_logscore_full's, word for word:
 *     la_0(j) = (j == 0 ? 0 : -inf) + log b_j(0)                      (the one-hot start)
 *     la_t(j) = LSE_{i : a_ij > 0} (la_{t-1}(i) + log a_ij) + log b_j(t)
 *     LSE(x)  = m + log(sum_i exp(x_i - m)),  m = max_i x_i
 * LSE is -inf when it has no term or every term is -inf, and NaN when a term is NaN.  A transition
 * with a_ij == 0 is not a term: a NaN in a predecessor that cannot be reached from does not leak.
 *     final_state != 0:  log P = la_{T-1}(N-1)       the diagonal recogniser's and trainer's convention
 *                        (calc_probability with its final-state term, RF:349-366): equal to ghmm_score
 *                        up to rounding where that is finite and none of its densities underflowed
 *     final_state == 0:  log P = LSE_j la_{T-1}(j)
 * Where the linear densities of ghmm_score underflow (one frame far from every Gaussian ends the
 * utterance with -inf or NaN there) this score stays finite.  T = 0 scores 0; U = 0 touches nothing; a
 * null destination with U > 0 gives GHMM_ERR_ARG.  1 to 512 states (GHMM_ERR_UNSUPPORTED above): up to
 * 64 the lattice kernel of ghmm_logscore_full on a table of one word, beyond that one wave per utterance
 * with the states in LDS (k_logforward_wide: a band-diagonal log A takes a two-term step, any other the
 * dense one of N exp per state and frame).  The checks are ghmm_viterbi's; GHMM_OPT_ROBUST has no effect,
 * as there.  Afterwards GHMM_BUF_B holds log b[F][N]; the row API does not reuse it and GHMM_BUF_POST
 * gives GHMM_ERR_ARG.  One launch under GHMM_K_EMISSION, one under GHMM_K_FORWARD.  Synchronises; a
 * second identical call repeats every byte. */
int ghmm_logscore(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, int final_state, double *loglik_host);

/* ghmm_estep with every quantity formed in the log domain (absent from the reference): where
 * ghmm_estep's linear densities underflow to 0 on a whole frame (c_t = 1/0, NaN statistics, and a NaN
 * model out of ghmm_mstep) this call keeps finite statistics.  ghmm_estep's contract otherwise: the same
 * ghmm_stats_create vector, overwritten by the launches ghmm_estep makes, one partial per utterance;
 * asynchronous on the context's stream; bitwise reproducible (a second identical call repeats every
 * byte); GHMM_OPT_DELTA and GHMM_OPT_PARTIALS honoured; GHMM_OPT_ROBUST has no effect, as in
 * ghmm_logscore; a full-covariance statistics vector or one of another shape gives GHMM_ERR_ARG;
 * ghmm_mstep, ghmm_stats_allreduce and ghmm_stats_loglik take the result as it is.  1 to 512 states;
 * above that GHMM_ERR_UNSUPPORTED before anything is launched or written.
 * Emission: e_m = log(wk_m) - aux_m / 2 and log b_i(t) are what ghmm_viterbi's emission launch writes,
 * bit for bit, on either tier (GHMM_OPT_KERNELS 1 and default).
 *     post_t(i,m) = exp(e_m - mx_i) / sum_m' exp(e_m' - mx_i),  mx_i = max_m e_m
 * the very terms log b's own sum is made of; 0 where log b_i(t) = -inf.
 * Lattice: log a_ij is the model's log A (a_ij > 0 ? log(a_ij) : -inf); a transition with a_ij == 0 is
 * not a term; LSE as at ghmm_logscore.
 *     la_0(j)      = (j == 0 ? 0 : -inf) + log b_j(0)
 *     la_t(j)      = LSE_{i : a_ij > 0} (la_{t-1}(i) + log a_ij) + log b_j(t)     (ghmm_logscore's)
 *     lbe_{T-1}(i) = (i == N-1 ? 0 : -inf)
 *     lbe_t(i)     = LSE_{j : a_ij > 0} (log a_ij + (log b_j(t+1) + lbe_{t+1}(j)))
 *     log P_u      = la_{T-1}(N-1)            -> GHMM_BUF_LOGLIK and the vector's loglik: the bits of
 *                                             ghmm_logscore with final_state = 1
 *     log Z_u      = LSE_j la_{T-1}(j)        the normaliser of gamma and xi (ghmm_logscore's final_state = 0)
 *     gamma_t(i)   = exp(la_t(i) + lbe_t(i) - log Z_u)
 *     xi_t(i,j)    = exp(la_t(i) + log a_ij + log b_j(t+1) + lbe_{t+1}(j) - log Z_u),
 *                    t < T-1, a_ij > 0, i <= j <= i + delta
 *     num_a[i][j] = sum_u sum_{t<T-1} xi_t(i,j);  den_a[i] = sum_u sum_{t<T-1} gamma_t(i);
 *     den_c[i] = sum_u sum_{t<T} gamma_t(i);  num_c / num_mu / num_var: calc_mix_param on
 *     w = gamma * post, the launches of ghmm_estep.
 * The normaliser is log Z_u, not log P_u: the reference's scaled recursions give gamma = alpha^ beta^ / c_t,
 * which divides by the probability of the observations over ALL end states while beta starts in the
 * last state only, so a frame's gammas sum to exp(log P_u - log Z_u) <= 1, the same value at every t.
 * An utterance with T < N or no path into the last state has every lbe = -inf: its gammas are exactly
 * 0 and log P_u = -inf, as in the linear call.  Where log Z_u is not finite the utterance's gamma rows
 * are 0 and it adds nothing to any sum except loglik (its log P_u as it is) and n_utt.  T = 0 adds 0 to
 * loglik and counts in n_utt.  U = 0 gives an all-zero vector.  A NaN log b (det == 0) gives the
 * formula's values.
 * Up to 64 states the lattice is ghmm_estep_full_log's two launches (one state per lane); beyond that
 * one wave per utterance with the states in LDS (k_logfb_wide_fwd / k_logfb_wide_bwd: a band-diagonal
 * log A takes two-term steps, any other the dense ones of N exp per state and frame).
 * Afterwards ghmm_fetch returns GHMM_BUF_B: log b, _POST, _GAMMA, _LOGLIK, _ALPHA: la, _BETA: lbe; the
 * row API does not reuse these buffers and no linear beta pass is started on them.  One launch under
 * GHMM_K_EMISSION, the two lattice launches under GHMM_K_FORWARD, none under GHMM_K_BACKWARD. */
int ghmm_estep_log(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, ghmm_stats *stats);

/* ------------- several-stream vocabularies of diagonal models: Viterbi, batched scoring and word decoding */

/* ghmm_viterbi's lattice on the sum of the streams' log b, log b = ((log b^0 + log b^1) + ...): every
 * term is the log b that ghmm_viterbi's emission launch makes for that stream alone, stream 0 into b,
 * every later stream into a buffer of its own that one IEEE addition per entry folds into b, the earlier
 * streams' sum on the left; NaN and +-inf propagate as the addition gives them.  The transitions are
 * models[0]'s log A; up to 255 states as in ghmm_viterbi (beyond 64 the one-wave-per-utterance kernel).
 * path_host[F], score_host[U]; T = 0 scores 0.  n_streams == 1 is ghmm_viterbi itself, the same bits.
 * Afterwards GHMM_BUF_B holds the summed log b[F][N]; the row API does not reuse it and GHMM_BUF_POST
 * gives GHMM_ERR_ARG.  The folds count under GHMM_K_EMISSION: 2 n_streams - 1 launches there, one under
 * GHMM_K_VITERBI.  The checks and refusals are ghmm_score_streams's, each before anything is launched or
 * written, and a null destination with U > 0 gives GHMM_ERR_ARG; U = 0 touches nothing.  Synchronises. */
int ghmm_viterbi_streams(ghmm_ctx *ctx, ghmm_model *const *models, ghmm_corpus *const *corpora,
                         int n_streams, int32_t *path_host, double *score_host);
/* A vocabulary of n_models words on n_streams streams in one pass, for the three calls below:
 *   models[k * n_streams + p] = stream p of word k;  corpora[p] = stream p of the utterances;
 *   the streams of one word have the same N, the transitions are stream 0's;
 *   for every stream p all words share M_p and D_p;
 *   the corpora have the same utterance count and lengths, corpora[p] has D_p coefficients.
 * Per stream one gather of the words' Gaussians into that stream's concatenated vocabulary (kept in the
 * context between calls, rebuilt when its shape changes; stream 0's is the one ghmm_score_batch uses) and
 * one emission launch over it, stream 0 into b[F][NS] (NS = the sum of the words' N), every later stream
 * into a buffer of its own that one launch folds into b, by multiplication or, on log b, by addition,
 * as in ghmm_score_streams and ghmm_viterbi_streams; then ONE lattice launch over every (word, utterance)
 * pair on word k's columns and stream 0's A or log A.  Under GHMM_OPT_TIMING: 2 n_streams - 1 launches
 * under GHMM_K_EMISSION (n_streams emissions, n_streams - 1 folds), one under GHMM_K_FORWARD or
 * GHMM_K_VITERBI; one wait for the stream.
 * out[k*U + u] is what the matching per-word call gives word k alone (ghmm_score_streams with its
 * final-state term, RF:349-366; ghmm_viterbi_streams' score): bit for bit with GHMM_OPT_KERNELS = 1,
 * where every state's density comes from its own Gaussians alone; under the matrix-core emission the
 * Gaussians are evaluated around the concatenated vocabulary's offsets, in tiles of 16 that may straddle
 * two words, so a score agrees with the per-word call's to rounding (1e-12 relative) and identical
 * Gaussians at different tile positions need not give identical bits: an exact tie between two words
 * is a property of the GHMM_OPT_KERNELS = 1 tier only.
 * Afterwards GHMM_BUF_B holds the product (or the sum of logs) over [F][NS]; as after ghmm_score_batch the
 * row API does not reuse it, and GHMM_BUF_POST gives GHMM_ERR_ARG.  U = 0 touches nothing.  A second
 * identical call repeats every byte.
 * Refusals, each before anything is launched or written.  GHMM_ERR_ARG: a null array or entry,
 * n_models < 1, n_streams outside 1..GHMM_MAX_STREAMS, a null destination with U > 0, streams of one
 * word that differ in N, corpora that differ in the utterance count or in a length, a corpus whose D is
 * not its stream's.  GHMM_ERR_UNSUPPORTED: words that differ in M_p or D_p for some stream p;
 * GHMM_OPT_ROBUST set with n_streams > 1; a word of more than 64 states in the two Viterbi calls. */
/* loglik_host[k*U + u] = ghmm_score_streams of word k: calc_probability with its final-state term
 * (RF:349-366) on the product of the streams' densities.  n_streams == 1 is ghmm_score_batch itself: the
 * same bits, the same cached vocabulary, the same two fall-backs (GHMM_OPT_ROBUST, a word of more than
 * 64 states).  n_streams > 1 and a word of more than 64 states: the word-by-word ghmm_score_streams loop. */
int ghmm_score_streams_batch(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                             ghmm_corpus *const *corpora, int n_streams, double *loglik_host);
/* score_host[k*U + u] = ghmm_viterbi_streams' score of word k (no paths); T = 0 scores 0.  Every word has
 * at most 64 states. */
int ghmm_viterbi_streams_batch(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                               ghmm_corpus *const *corpora, int n_streams, double *score_host);
/* Which word was it, and how does it align (n_streams >= 1): ghmm_viterbi_streams_batch's score table,
 * every utterance's winning word picked on the device, and the winner's lattice run again with
 * back-pointers on the log b already in the workspace, all enqueued without a host round trip and
 * ended by one wait for the stream.
 *   score_host[n_models*U]  the batch call's table, bit for bit
 *   word_host[U]            the winner: best = 0; for k = 1 .. n_models-1 in order, k takes over if
 *                           score[k] > score[best], or if score[best] is NaN and score[k] is not.  Ties
 *                           go to the lowest word, a NaN never beats a number, and all NaN or all -inf
 *                           gives word 0
 *   path_host[F]            over utterance u's frames, the path of ghmm_viterbi's lattice for word
 *                           word_host[u] on that word's columns of GHMM_BUF_B (ties take the lowest
 *                           predecessor); with GHMM_OPT_KERNELS = 1 bit for bit ghmm_viterbi_streams' path
 *                           of that word
 * T = 0 scores 0 under every word, gives word 0 and no path entries.  U = 0 touches nothing.  The
 * vocabulary layout, GHMM_BUF_B afterwards and the refusals are the batch calls' (all three destinations
 * are needed when U > 0).  The two extra launches count under GHMM_K_VITERBI (three there in all).  A
 * second identical call repeats every byte. */
int ghmm_recognise_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                           ghmm_corpus *const *corpora, int n_streams, int32_t *word_host,
                           int32_t *path_host, double *score_host);
/* Connected words: which STRING of words was it, and how does it align (n_streams >= 1).  The reference
 * has no such decoder.  One max-plus lattice over the states of all words at once, on the vocabulary's
 * log b[F][NS] (word k = 0 .. K-1 has N_k states in columns bo_k .. bo_k + N_k - 1; log A_k is stream
 * 0's, -inf where a = 0); p = word_penalty:
 *   d_0(k,j)  = (j == 0 ? 0 : -inf) + log b_{k,j}(0)        every word may start the utterance; no penalty
 *   e_{t-1}   = d_{t-1}(w, N_w - 1),  w = w_{t-1} = pick_k d_{t-1}(k, N_k - 1)
 *   in_t(k,j) = max_i (d_{t-1}(k,i) + log a^k_ij), the candidates in ascending i, a later one wins only
 *               on a strict >, best starts at -inf with predecessor 0: ghmm_viterbi's step, the same bits
 *   x_t       = e_{t-1} + p
 *   d_t(k,0)  = (x_t > in_t(k,0) ? x_t : in_t(k,0)) + log b_{k,0}(t)    the entry wins only on a strict >:
 *                                                      a tie stays in the word; a NaN x_t never enters
 *   d_t(k,j)  = in_t(k,j) + log b_{k,j}(t)             j > 0
 *   score_u   = d_{T-1}(w, N_w - 1),  w = pick_k d_{T-1}(k, N_k - 1)
 * pick is ghmm_recognise_streams' rule (best = 0; k = 1 .. K-1 in order takes over if s[k] > s[best], or if
 * s[best] is NaN and s[k] is not), which is the order: a beats b if a's value is greater; or b's is NaN
 * and a's is not; or neither value beats the other and a's word is lower.
 * The trace starts in the last state of the final pick, whatever its score, and follows the
 * back-pointers; where the back-pointer of (t, k, 0) is the entry, frame t begins a word and the trace
 * continues at (t-1, w_{t-1}, N_w - 1).
 *   word_host[F]   the word per frame
 *   path_host[F]   the state within that word
 *   begin_host[F]  1 on the first frame of every word instance (frame 0 of an utterance included), else
 *                  0: what tells "five five" from one long "five"
 *   score_host[U]  the score per utterance; T = 0 scores 0 and writes no frame entries
 * Consequences: with p = -inf nothing ever enters, and word, path and score are the bits of
 * ghmm_recognise_streams (its word_host[u] on every frame of u, its score of that word), begin is 1 at
 * every utterance's first frame only.  A word of one state is both its own entry and its own end.  A
 * finite positive penalty is allowed.
 * The vocabulary layout, the gathers, the emission launches and folds, GHMM_BUF_B afterwards and U = 0
 * (touches nothing) are the batch calls'.  Then ONE launch under GHMM_K_VITERBI holds the lattice and the
 * trace (one workgroup per utterance, csrc/ghmm_connect.hpp): 2 n_streams - 1 launches under
 * GHMM_K_EMISSION, one under GHMM_K_VITERBI, one wait for the stream.  A second identical call repeats
 * every byte.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_recognise_streams refuses
 * (a word of more than 64 states and GHMM_OPT_ROBUST with n_streams > 1 included; all four destinations
 * are needed when U > 0); a NaN or +inf penalty gives GHMM_ERR_ARG; more than 2048 states in the
 * vocabulary (NS; what the kernel keeps in LDS) gives GHMM_ERR_UNSUPPORTED. */
int ghmm_connect_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                         ghmm_corpus *const *corpora, int n_streams, double word_penalty,
                         int32_t *word_host, int32_t *path_host, int32_t *begin_host, double *score_host);
/* Connected words under a word-pair grammar: ghmm_connect_streams' vocabulary, corpora, lattice and
 * outputs, with a score for every ordered pair of words instead of one flat penalty (n_streams >= 1; the
 * reference has no such decoder).  K = n_models:
 *   pair[K*K]  row-major: pair[w*K + k] is the log score of word k following word w
 *   start[K]   start[k] scores word k opening the utterance; null means all 0
 *   fin[K]     fin[k] scores word k closing the utterance; null means all 0
 * -inf forbids; finite values of either sign are allowed.  On the vocabulary's log b[F][NS], in
 * ghmm_connect_streams' notation:
 *   d_0(k,j)  = (j == 0 ? start[k] : -inf) + log b_{k,j}(0)
 *   in_t(k,j) = ghmm_connect_streams' in_t(k,j): ghmm_viterbi's step inside word k, the same bits
 *   c_t(w,k)  = d_{t-1}(w, N_w - 1) + pair[w][k]
 *   x_t(k)    = the best c_t(w,k) over w, best starting at -inf with predecessor word 0: a candidate wins
 *               on a strictly greater value, among equal values the lower w wins, a NaN candidate never
 *               wins (an order: any reduction tree gives the same answer)
 *   d_t(k,0)  = (x_t(k) > in_t(k,0) ? x_t(k) : in_t(k,0)) + log b_{k,0}(t)    the entry wins only on a strict >
 *   d_t(k,j)  = in_t(k,j) + log b_{k,j}(t)             j > 0
 *   score_u   = d_{T-1}(w, N_w - 1) + fin[w],  w = pick_k (d_{T-1}(k, N_k - 1) + fin[k])
 * pick is ghmm_recognise_streams' rule.  The trace starts in the last state of the final pick, whatever
 * its score; where the back-pointer of (t, k, 0) is the entry, frame t begins a word and the trace
 * continues at (t-1, w, N_w - 1) with w the predecessor word kept for (t, k).  word_host[F], path_host[F],
 * begin_host[F] and score_host[U] have ghmm_connect_streams' shape; T = 0 scores 0 and writes no frame
 * entries.  Where the score is not finite the frame entries are what the trace gives on back-pointers of
 * -inf candidates and carry no meaning.
 * Consequences:
 *   (a) with pair == p everywhere and start == fin == 0 the score equals ghmm_connect_streams(p)'s as a
 *       value (rounding is monotone: max_w fl(e_w + p) = fl(max_w e_w + p)); at p = 0 and p = -inf word,
 *       path and begin are that call's bit for bit, ties included; at other p wherever the optimum is
 *       unique beyond rounding;
 *   (b) for a transcript of pairwise distinct words k_0 .. k_{L-1}, with start 0 at k_0, pair 0 at
 *       (k_i, k_{i+1}), fin 0 at k_{L-1} and -inf everywhere else, the score equals ghmm_align_streams'
 *       as a value; where it is finite, word, path and begin are that call's;
 *   (c) for any grammar and any utterance with a finite score, the decoded string's first word has
 *       start > -inf, every adjacent pair has pair > -inf, and the last word has fin > -inf.
 * The vocabulary layout, the gathers, the emission launches and folds, GHMM_BUF_B afterwards and U = 0
 * (touches nothing) are ghmm_connect_streams'.  The grammar travels to the device ahead of the launch on
 * the context's stream; then ONE launch under GHMM_K_VITERBI holds the lattice and the trace (one
 * workgroup per utterance, csrc/ghmm_grammar.hpp): 2 n_streams - 1 launches under GHMM_K_EMISSION, one
 * under GHMM_K_VITERBI, one wait for the stream.  A second identical call repeats every byte.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_connect_streams refuses
 * (more than 2048 states in the vocabulary, a word of more than 64 states, GHMM_OPT_ROBUST with
 * n_streams > 1, a missing destination when U > 0); GHMM_ERR_ARG for a null pair when U > 0 and for a NaN
 * or +inf anywhere in start, pair or fin; GHMM_ERR_UNSUPPORTED for K > GHMM_GRAMMAR_MAX_WORDS (the dense
 * K x K table and a predecessor word in one byte; a sparse successor list is not offered). */
#define GHMM_GRAMMAR_MAX_WORDS 256
int ghmm_connect_grammar_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                                 ghmm_corpus *const *corpora, int n_streams, const double *start,
                                 const double *pair, const double *fin, int32_t *word_host,
                                 int32_t *path_host, int32_t *begin_host, double *score_host);
/* Forced alignment: WHERE does each word of a known transcript lie (n_streams >= 1).  The reference has no
 * such call.  seq_off[U + 1], seq[seq_off[U]]: utterance u's transcript is the words
 * seq[seq_off[u] .. seq_off[u+1]): L_u instances, instance i = word k_i with N_i states.  The vocabulary
 * layout, the gathers, the emission launches and folds, and GHMM_BUF_B afterwards are
 * ghmm_connect_streams': the WHOLE vocabulary's log b[F][NS] is computed, not only the transcript's words
 * (gathering only the words a batch uses is not done).  The composite states of u are s = 0 .. S_u - 1,
 * S_u = sum_i N_i, instance i owning a contiguous run of them; state (i, j) reads column bo_{k_i} + j of
 * log b; log A is word k_i's, stream 0's, -inf where a = 0:
 *   d_0(i,j)  = (i == 0 && j == 0 ? 0 : -inf) + log b_{k_i,j}(0)
 *   in_t(i,j) = max_{i'} (d_{t-1}(i,i') + log a_{i'j}), the candidates in ascending i', a later one wins only
 *               on a strict >, best starts at -inf with predecessor 0: ghmm_viterbi's step, the same bits
 *   x_t(i)    = d_{t-1}(i-1, N_{i-1} - 1)          i > 0; no penalty term: the value itself
 *   d_t(i,0)  = (i > 0 && x_t(i) > in_t(i,0) ? x_t(i) : in_t(i,0)) + log b(t)    the entry wins only on a
 *                                                  strict >: a tie stays in the word; a NaN never enters
 *   d_t(i,j)  = in_t(i,j) + log b(t)               j > 0
 *   score_u   = d_{T-1}(L_u - 1, N_{L_u-1} - 1)
 * The trace starts in the last state of the last instance, whatever its score, and follows the
 * back-pointers as ghmm_connect_streams' does; an entry back-pointer at (t, i, 0) continues at
 * (t-1, i-1, N_{i-1} - 1).  The outputs have ghmm_connect_streams' shape:
 *   word_host[F]   the word of the instance per frame
 *   path_host[F]   the state within the word
 *   begin_host[F]  1 on the first frame of every instance (frame 0 of an utterance included), else 0
 *   score_host[U]  the score per utterance
 * T = 0 scores 0 and writes no frame entries, whatever its transcript (an empty one is allowed there, and
 * the cap below is not applied to it).  A score of -inf says that the utterance is too short for its
 * transcript (fewer frames than the shortest path through its instances) or that no path exists; the
 * frame entries are then what the trace gives on back-pointers of -inf candidates and carry no meaning.
 * Consequences:
 *   (a) a one-word transcript (k) gives score == ghmm_viterbi_streams_batch's [k][u] bit for bit under
 *       either GHMM_OPT_KERNELS; where ghmm_recognise_streams picks word k, its path;
 *   (b) with the strings that ghmm_connect_streams decodes at penalty 0 as transcripts, score == that
 *       call's score (== as values); where the optimum is unique, word, path and begin are its;
 *   (c) for any transcript, score <= ghmm_connect_streams' penalty-0 score.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_recognise_streams refuses
 * (all four destinations and both transcript arrays are needed when U > 0); GHMM_ERR_ARG for
 * seq_off[0] != 0, a decreasing seq_off, a word outside 0 .. n_models-1, an empty transcript on an
 * utterance with T > 0; GHMM_ERR_UNSUPPORTED for an utterance of T > 0 whose S_u exceeds 2048 (what the
 * kernel keeps in LDS) or a word of more than 64 states.  U = 0 touches nothing.
 * 2 n_streams - 1 launches under GHMM_K_EMISSION, ONE under GHMM_K_VITERBI (lattice and trace, one
 * workgroup per utterance, csrc/ghmm_align.hpp), one wait for the stream.  A second identical call repeats
 * every byte. */
int ghmm_align_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                       ghmm_corpus *const *corpora, int n_streams, const int32_t *seq, const int32_t *seq_off,
                       int32_t *word_host, int32_t *path_host, int32_t *begin_host, double *score_host);
/* Embedded Baum-Welch: the E-step on the composite model of every utterance's transcript (n_streams >= 1;
 * diagonal models).  The reference has no such call.  models[k * n_streams + p], corpora[p], seq and
 * seq_off are ghmm_align_streams' vocabulary and transcript layout; stats[k * n_streams + p] is a
 * ghmm_stats_create vector of word k's stream-p shape (N_k, M_p, D_p), OVERWRITTEN, so that
 * ghmm_mstep(models[k * n_streams + p], stats[k * n_streams + p]) works unchanged.  The composite
 * states, their columns in log b and log A are ghmm_align_streams'; LSE as at ghmm_logscore; a
 * transition with a_ij == 0 is not a term; LSE2(x, y) = hi + log1p(exp(lo - hi)), lo == -inf giving hi:
 *   la_0(i,j)   = (i == 0 && j == 0 ? 0 : -inf) + log b(0)
 *   in_t(i,j)   = LSE_{i' : a_i'j > 0} (la_{t-1}(i,i') + log a_i'j)        ghmm_estep_log's step, its bits
 *   la_t(i,0)   = (i > 0 ? LSE2(in_t(i,0), la_{t-1}(i-1, N_{i-1}-1)) : in_t(i,0)) + log b(t)
 *   la_t(i,j)   = in_t(i,j) + log b(t)                                     j > 0; the entry carries weight 0
 *   lbe_{T-1}(i,j) = (i == L-1 && j == N_i-1 ? 0 : -inf)
 *   w_t(i,j)    = log b_{i,j}(t+1) + lbe_{t+1}(i,j)
 *   wi_t(i,j)   = LSE_{j' : a_jj' > 0} (log a_jj' + w_t(i,j'))             within the word: ghmm_estep_log's step
 *   lbe_t(i,j)  = (j == N_i-1 && i < L-1) ? LSE2(wi_t(i,j), w_t(i+1,0)) : wi_t(i,j)
 *   log P_u     = la_{T-1}(L-1, N_{L-1}-1)
 *   log Z_u     = LSE_j la_{T-1}(L-1, j)                                   over the LAST instance's states
 *   gamma_t(i,j)  = exp((la_t(i,j) + lbe_t(i,j)) - log Z_u)
 *   xi_t(i;j,j')  = exp(((la_t(i,j) + log a_jj') + w_t(i,j')) - log Z_u)   t < T-1, a_jj' > 0, j <= j' <= j + delta
 *   stay_t(i,j)   = exp((la_t(i,j) + wi_t(i,j)) - log Z_u)                 the share of gamma that stays in the word
 * LSE2 is formed ONLY in the first state of an instance behind the first and in the last state of an
 * instance before the last.  The sums of word k are tied over every instance i with k_i == k, in ascending
 * instance order, then over the utterances in ghmm_estep_log's order (one partial per utterance):
 *   gamma_t(k,j)    = sum_i gamma_t(i,j)          GHMM_BUF_GAMMA [F][NS]; 0 in the columns of absent words
 *   num_a[k][j][j'] = sum_u sum_{t<T-1} sum_i xi_t(i;j,j')
 *   den_a[k][j]     = sum_u sum_{t<T-1} sum_i stay_t(i,j)
 *   den_c[k][j]     = sum_u sum_{t<T}   gamma_t(k,j)
 *   num_c / num_mu / num_var of stream p: calc_mix_param on w = gamma_t(k,j) * post^p_t(k,j,m),
 *                     ghmm_estep_log's posteriors
 *   loglik = sum_u log P_u and n_utt = U: the same bits in EVERY stats[k * n_streams + p]
 * den_a is built on stay, not gamma: the exit into the next instance has no parameter and receives no xi,
 * so with stay the rows of the next A still sum to 1 (sum_j' num_a[k][j][j'] == den_a[k][j] to rounding
 * wherever the band holds every a_jj' > 0); with gamma a word's last self-loop would shrink every
 * iteration by the mass that left the word.  log Z_u over the last instance is ghmm_estep_log's
 * normaliser carried over: a frame's gammas sum to exp(log P_u - log Z_u), the same value at every t.
 * Where log Z_u is not finite (an utterance too short for its transcript, no path, a NaN column) the
 * utterance adds nothing but its log P_u to loglik and 1 to n_utt, and its gamma rows are 0.  T = 0 adds 0
 * to loglik and counts in n_utt; its transcript may be empty.  U = 0 gives all-zero vectors.  A word that
 * no transcript holds gets zero sums and the common loglik and n_utt: ghmm_mstep on it would re-invert its
 * variances (see ghmm_mstep), so a trainer skips it.
 * Consequences:
 *   (a) with n_models == 1 and one-word transcripts, under GHMM_OPT_KERNELS = 1, stats[p], GHMM_BUF_GAMMA,
 *       GHMM_BUF_LOGLIK and GHMM_BUF_B are ghmm_estep_log_streams' on the same context, bit for bit;
 *   (b) with one-word transcripts and any vocabulary, word k's sums are ghmm_estep_log_streams' on the
 *       sub-corpus of its utterances, to rounding;
 *   (c) a transcript (k, k) gives word k the sum of what two separate copies of the word would get.
 * Asynchronous on the context's stream; a second identical call repeats every byte; GHMM_OPT_DELTA is
 * honoured; GHMM_OPT_ROBUST has no effect with one stream and is refused with several, as in the
 * vocabulary calls.  Afterwards GHMM_BUF_B holds log b[F][NS], GHMM_BUF_GAMMA the tied gamma[F][NS],
 * GHMM_BUF_LOGLIK log P_u; GHMM_BUF_POST is served for n_streams == 1 and refused beyond, as after
 * ghmm_estep_log_streams; GHMM_BUF_ALPHA, _BETA and _SCALE give GHMM_ERR_ARG (the composite la rows are
 * ragged and nobody else's to read); the row API does not reuse any of these buffers.  A vector's mailbox
 * is not written: ghmm_stats_loglik copies and waits.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_align_streams refuses (a
 * word of more than 64 states, S_u > 2048 on an utterance with T > 0, an empty transcript with T > 0, a
 * word outside the vocabulary, ...; both transcript arrays are needed when U > 0); GHMM_ERR_ARG for a
 * null stats array or entry, a vector that is not word k's stream-p shape, or a full-covariance one.
 * Full-covariance words go through ghmm_estep_embed_full_streams (below): the same lattice, which sees
 * only log b[F][NS] and the words' table (csrc/ghmm_embed.hpp).
 * 2 n_streams - 1 launches under GHMM_K_EMISSION; TWO under GHMM_K_FORWARD (the lattice forwards and
 * backwards, one workgroup per utterance); per stream ghmm_estep's statistics launches on the
 * concatenated vocabulary under GHMM_K_MIXSTATS and GHMM_K_REDUCE, and one more under GHMM_K_REDUCE that
 * hands every word its own blocks. */
int ghmm_estep_embed_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                             ghmm_corpus *const *corpora, int n_streams, const int32_t *seq,
                             const int32_t *seq_off, ghmm_stats *const *stats);
/* Word posteriors under a word-pair grammar: how far to trust each word that ghmm_connect_grammar_streams
 * decodes, and the utterance's total likelihood under the grammar (n_streams >= 1; diagonal models; the
 * reference has no such call).  One log-domain forward-backward over the lattice of
 * ghmm_connect_grammar_streams: its max becomes a log-sum-exp, and a backward pass follows.  The vocabulary,
 * the corpora, K = n_models, start[K], pair[K*K] and fin[K] are that call's (a null start or fin means all 0;
 * -inf forbids).  On the vocabulary's log b[F][NS], in that call's notation; LSE as at ghmm_logscore; a term
 * whose log a or grammar score is -inf is not a term; an LSE over no terms is -inf; LSE2 is
 * ghmm_estep_embed_streams':
 *   la_0(k,j)   = (j == 0 ? start[k] : -inf) + log b_{k,j}(0)
 *   in_t(k,j)   = LSE_{i : a_ij > 0} (la_{t-1}(k,i) + log a^k_ij)            ghmm_estep_log's step inside word k
 *   x_t(k)      = LSE_{w : pair[w][k] > -inf} (la_{t-1}(w, N_w-1) + pair[w][k])
 *   la_t(k,0)   = LSE2(in_t(k,0), x_t(k)) + log b_{k,0}(t);   la_t(k,j) = in_t(k,j) + log b_{k,j}(t), j > 0
 *   log P_u     = LSE_{k : fin[k] > -inf} (la_{T-1}(k, N_k-1) + fin[k])
 *   lbe_{T-1}(k,j) = (j == N_k-1 ? fin[k] : -inf)
 *   w_t(k,j)    = log b_{k,j}(t+1) + lbe_{t+1}(k,j)
 *   wi_t(k,j)   = LSE_{j' : a_jj' > 0} (log a^k_jj' + w_t(k,j'))
 *   y_t(k)      = LSE_{k' : pair[k][k'] > -inf} (pair[k][k'] + w_t(k',0))
 *   lbe_t(k,j)  = (j == N_k-1) ? LSE2(wi_t(k,j), y_t(k)) : wi_t(k,j)
 *   gamma_t(k,j) = exp((la_t(k,j) + lbe_t(k,j)) - log P_u)                    GHMM_BUF_GAMMA [F][NS]
 *   occ_t(k)    = sum_j gamma_t(k,j), j ascending                             occ_host[F*K]
 *   ent_0(k)    = gamma_0(k,0)
 *   ent_t(k)    = exp(((x_t(k) + log b_{k,0}(t)) + lbe_t(k,0)) - log P_u)     ent_host[F*K], may be null
 * A NaN term makes its LSE NaN.  Inside a word the steps are ghmm_estep_embed_streams' (the banded two-term
 * form or the dense one, chosen per word).  The order of the terms inside x_t, y_t and log P_u is NOT pinned
 * to the bit: any reduction tree is allowed (the library keeps a running maximum and a sum scaled by it), and
 * the results are pinned by tolerance against a long-double restatement (tests/gpost_cases.py).
 *   occ_host[F*K]  occ_t(k): the posterior that frame t lies in word k.  The mean of occ over the frames of a
 *                  decoded word instance is that word's confidence
 *   ent_host[F*K]  ent_t(k): the posterior that an instance of word k BEGINS at frame t; its sum over (t, k)
 *                  is the expected number of words.  May be null: not copied then
 *   loglik_host[U] log P_u, the total over every word string that the grammar allows; two grammars on the
 *                  same audio compare by it
 * Where log P_u is not finite (no allowed string fits in T frames, a NaN column, a grammar that forbids
 * everything) the utterance's gamma, occ and ent rows are 0 and loglik_host[u] is that value.  T = 0 gives
 * log P = 0 and writes no rows.  U = 0 touches nothing.  A second identical call repeats every byte.
 * Consequences:
 *   (a) with K = 1, pair = -inf and start = fin = 0, log P_u is ghmm_logscore_streams(final_state = 1)'s, to
 *       rounding;
 *   (b) under the chain grammar of a transcript of pairwise distinct words (consequence (b) of
 *       ghmm_connect_grammar_streams), log P_u is ghmm_estep_embed_streams' GHMM_BUF_LOGLIK for that
 *       transcript, to rounding, and that call's tied gamma equals this gamma times exp(log P_u - log Z_u);
 *   (c) log P_u >= ghmm_connect_grammar_streams' score of the same call, to rounding: the sum holds the best
 *       path;
 *   (d) at every frame of an utterance with finite log P_u, sum_k occ_t(k) = 1, and sum_k ent_0(k) = 1, to
 *       rounding;
 *   (e) a word that no allowed string can hold (start[k] and its whole column of pair -inf: it cannot be
 *       entered; or its whole row of pair and fin[k] -inf: it cannot be left) has occ == 0 exactly.
 * Afterwards GHMM_BUF_B holds log b[F][NS], GHMM_BUF_GAMMA gamma[F][NS], GHMM_BUF_LOGLIK log P_u;
 * GHMM_BUF_ALPHA, _BETA and _SCALE give GHMM_ERR_ARG as after ghmm_estep_embed_streams, and GHMM_BUF_POST
 * as well (the emission is the decoder's: it writes no posteriors); the row API does not reuse any of these
 * buffers.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_connect_grammar_streams
 * refuses (K > GHMM_GRAMMAR_MAX_WORDS, more than 2048 states in the vocabulary, a word of more than 64
 * states, GHMM_OPT_ROBUST with n_streams > 1, a null pair when U > 0, a NaN or +inf anywhere in start, pair
 * or fin); GHMM_ERR_ARG for a null occ_host or loglik_host when U > 0.
 * The vocabulary layout, the gathers, the emission launches and folds are ghmm_connect_grammar_streams':
 * 2 n_streams - 1 launches under GHMM_K_EMISSION; the grammar and a transposed copy of pair travel to the
 * device on the context's stream; then TWO launches under GHMM_K_FORWARD (the lattice forwards and
 * backwards, one workgroup per utterance, csrc/ghmm_gpost.hpp); one wait for the stream per output copied.
 * Full-covariance words go through ghmm_grammar_post_full_streams (below): the same lattice, which sees
 * only log b[F][NS] and the words' table. */
int ghmm_grammar_post_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                              ghmm_corpus *const *corpora, int n_streams, const double *start,
                              const double *pair, const double *fin, double *occ_host,
                              double *ent_host, double *loglik_host);
/* Baum-Welch statistics on the grammar lattice: the E-step over EVERY word string that the grammar allows
 * (n_streams >= 1; diagonal models; the reference has no such call).  These are the denominator occupancies of
 * discriminative training (ghmm_mstep_ebw takes them), and on their own EM on untranscribed or loosely
 * transcribed audio under a grammar.  The vocabulary, the corpora and start, pair, fin are
 * ghmm_grammar_post_streams'; stats[k * n_streams + p] is ghmm_estep_embed_streams' layout (a ghmm_stats_create
 * vector of word k's stream-p shape) and is OVERWRITTEN.  la, lbe, w, wi, x, y, log P_u and gamma are exactly
 * ghmm_grammar_post_streams' definition, its allowance on the order of the terms inside x_t, y_t and log P_u
 * included.  Added, for t < T-1, a_jj' > 0 and j <= j' <= j + GHMM_OPT_DELTA:
 *   xi_t(k;j,j')    = exp(((la_t(k,j) + log a^k_jj') + w_t(k,j')) - log P_u)
 *   stay_t(k,j)     = exp((la_t(k,j) + wi_t(k,j)) - log P_u)
 *   num_a[k][j][j'] = sum_u sum_{t<T-1} xi_t(k;j,j')
 *   den_a[k][j]     = sum_u sum_{t<T-1} stay_t(k,j)
 *   den_c[k][j]     = sum_u sum_{t<T}   gamma_t(k,j)
 *   num_c / num_mu / num_var of stream p: calc_mix_param on w = gamma_t(k,j) * post^p_t(k,j,m),
 *                     ghmm_estep_log's posteriors
 *   loglik = sum_u log P_u and n_utt = U: the same bits in EVERY stats[k * n_streams + p]
 * over the utterances in ghmm_estep_log's order (one partial per utterance).  There is one copy of each word
 * in this lattice: nothing is tied.  The normaliser is log P_u, THIS lattice's total over every allowed word
 * string; it is NOT ghmm_estep_embed_streams' log Z_u (the LSE over the last instance's states), so the two
 * calls' vectors differ by exp(log Z_u - log P_u) per utterance even where their lattices coincide ((b) below).
 * den_a is built on stay for the reason given at ghmm_estep_embed_streams: the exit into another word has no
 * parameter and receives no xi.
 * Where log P_u is not finite the utterance adds nothing but its log P_u to loglik and 1 to n_utt, and its
 * gamma rows are 0; so that "nothing" holds of the mixture sums as well (a column whose log b is NaN has NaN
 * posteriors, and 0 x NaN is NaN), its rows of the mixture posteriors are set to 0 too, in every stream:
 * GHMM_BUF_POST shows them so.  T = 0 adds 0 to loglik and counts in n_utt.  T = 1 gives den_c only.  U = 0 gives all-zero
 * vectors.
 * Consequences:
 *   (a) on the same context GHMM_BUF_LOGLIK and GHMM_BUF_GAMMA are ghmm_grammar_post_streams', bit for bit
 *       under GHMM_OPT_KERNELS = 1 (the emission with posteriors gives the bits of log b that the emission
 *       without them gives on that tier, and the lattice arithmetic is the same code), to rounding otherwise;
 *   (b) under the chain grammar of a transcript of pairwise distinct words and a one-utterance corpus, every
 *       block of every word's vector equals ghmm_estep_embed_streams' for that transcript times
 *       exp(log Z_u - log P_u), to rounding; that factor is the reciprocal of a frame's sum of that call's tied
 *       gamma.  loglik is equal to rounding;
 *   (c) wherever the band holds every a_jj' > 0, sum_j' num_a[k][j][j'] = den_a[k][j] to rounding;
 *   (d) sum_k sum_j den_c[k][j] is the number of frames of the utterances with finite log P_u, to rounding;
 *   (e) ghmm_grammar_post_streams' (e): a word that no allowed string can hold gets exactly zero sums;
 *   (f) ghmm_mstep(models[k * n_streams + p], stats[k * n_streams + p]) works unchanged.  A word with zero
 *       sums would have its variances re-inverted (see ghmm_mstep), so a trainer skips it.
 * Asynchronous on the context's stream; a second identical call repeats every byte; GHMM_OPT_DELTA is honoured.
 * Afterwards GHMM_BUF_B holds log b[F][NS], GHMM_BUF_GAMMA gamma[F][NS], GHMM_BUF_LOGLIK log P_u; GHMM_BUF_POST
 * is served for n_streams == 1 and refused beyond; GHMM_BUF_ALPHA, _BETA and _SCALE give GHMM_ERR_ARG; the row
 * API does not reuse any of these buffers.  A vector's mailbox is not written: ghmm_stats_loglik copies and
 * waits.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_grammar_post_streams refuses of
 * the vocabulary, the corpora and the grammar; GHMM_ERR_ARG for a null stats array or entry, a vector that is
 * not word k's stream-p shape, or a full-covariance one.
 * Launches: ghmm_estep_embed_streams' emission sequence (2 n_streams - 1 under GHMM_K_EMISSION, with the
 * posteriors); TWO under GHMM_K_FORWARD (k_gpost_fwd unchanged and k_gpost_bwd in its statistics form, which
 * keeps the sums of a thread's states in registers over the frames and forms no occ or ent; csrc/ghmm_gpost.hpp);
 * then per stream ghmm_estep_embed_streams' statistics launches and scatter.  Full-covariance words: not yet. */
int ghmm_estep_grammar_streams(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                               ghmm_corpus *const *corpora, int n_streams, const double *start,
                               const double *pair, const double *fin, ghmm_stats *const *stats);
/* ghmm_logscore (above) on the sum of the streams' log b, log b = ((log b^0 + log b^1) + ...) folded
 * exactly as in ghmm_viterbi_streams, with models[0]'s log A and both final_state conventions; 1 to 512
 * states.  n_streams == 1 is ghmm_logscore itself, the same bits.  The checks and refusals are
 * ghmm_score_streams's (GHMM_OPT_ROBUST with n_streams > 1: GHMM_ERR_UNSUPPORTED), each before anything
 * is launched or written; a null destination with U > 0 gives GHMM_ERR_ARG; U = 0 touches nothing.
 * Afterwards GHMM_BUF_B holds the summed log b[F][N]; the row API does not reuse it and GHMM_BUF_POST
 * gives GHMM_ERR_ARG.  2 n_streams - 1 launches under GHMM_K_EMISSION, one under GHMM_K_FORWARD.
 * Synchronises; a second identical call repeats every byte. */
int ghmm_logscore_streams(ghmm_ctx *ctx, ghmm_model *const *models, ghmm_corpus *const *corpora,
                          int n_streams, int final_state, double *loglik_host);
/* ghmm_estep_log (above) on several feature streams, as ghmm_estep_streams is ghmm_estep on them:
 * log b = ((log b^0 + log b^1) + ...) folded exactly as in ghmm_viterbi_streams, stream p's posteriors
 * kept apart, ONE lattice on models[0]'s log A, then ghmm_estep's statistics launches once per stream on
 * the common gamma and stream p's posteriors, frames and means; the transition sums, den_c, log P and
 * the exemplar count are the same bits in every stats[p].  n_streams == 1 is ghmm_estep_log itself, the
 * same bits.  The checks and refusals are ghmm_estep_streams's (check by check, then every stream's
 * vector) and more than 512 states gives GHMM_ERR_UNSUPPORTED, each before anything is launched or
 * written.  Afterwards GHMM_BUF_B holds the summed log b[F][N], _GAMMA, _LOGLIK, _ALPHA (la) and _BETA
 * (lbe) are served, and GHMM_BUF_POST gives GHMM_ERR_ARG as after ghmm_estep_streams.  2 n_streams - 1
 * launches under GHMM_K_EMISSION, two under GHMM_K_FORWARD.  Asynchronous. */
int ghmm_estep_log_streams(ghmm_ctx *ctx, ghmm_model *const *models, ghmm_corpus *const *corpora,
                           int n_streams, ghmm_stats *const *stats);
/* loglik_host[k*U + u] = ghmm_logscore_streams of word k alone, the vocabulary in one pass as laid out
 * above: the gathers, one log-emission launch per stream over its concatenated vocabulary, the folds,
 * and ONE lattice launch over every (word, utterance) pair on stream 0's log A (2 n_streams - 1 launches
 * under GHMM_K_EMISSION, one under GHMM_K_FORWARD).  Bit for bit the per-word call with
 * GHMM_OPT_KERNELS = 1; under the matrix-core emission to rounding (1e-12 relative), as stated above.
 * A vocabulary with a word of more than 64 states is scored word by word by ghmm_logscore_streams (the
 * same bits on either tier), as ghmm_score_streams_batch does; a word of more than 512 states gives
 * GHMM_ERR_UNSUPPORTED before anything is written.  The other refusals, GHMM_BUF_B afterwards and U = 0
 * are ghmm_score_streams_batch's.  ghmm_logscore_batch is n_streams == 1 with the corpus itself: the
 * same bits. */
int ghmm_logscore_batch(ghmm_ctx *ctx, ghmm_model *const *models, int n_models, ghmm_corpus *c,
                        int final_state, double *loglik_host);
int ghmm_logscore_streams_batch(ghmm_ctx *ctx, ghmm_model *const *models, int n_models,
                                ghmm_corpus *const *corpora, int n_streams, int final_state,
                                double *loglik_host);

/* ------------------------------------------ the full-covariance recogniser */

/* RC = test/source/recognition-full-fs/recognition_continuous_full_fs.c, the reference's
 * full-covariance recogniser.  A separate opaque model: nothing of the diagonal E-step,
 * M-step or Viterbi takes it (its own Viterbi is below).  One feature stream, 1 <= N <= 64 states, M >= 1 mixtures,
 * 1 <= D <= 48 coefficients (GHMM_ERR_UNSUPPORTED outside; the reference's caps are 15, 5
 * and 16).  Per Gaussian: mean[D], det (of the NON-inverted covariance) and the inverse
 * covariance inv_cov[D][D] row-major as the .hmm file stores it (RC:591-707):
 *     A[N*N], c[N*M], mean[N*M*D], inv_cov[N*M*D*D], det[N*M]
 * calc_gaus (RC:902-954) is evaluated in the reference's direct form and order:
 *     dif = x - mu;  aux = sum_i dif[i] * (sum_j dif[j] * inv_cov[j][i]);
 *     gaus = exp(-aux/2) / (pow(2 pi, D/2) * sqrt(|det|))
 * det == 0: the reference leaves gaus uninitialised; here it is what the diagonal emission
 * gives such a Gaussian: exp(-aux/2) / 0 (inf, or NaN where exp(-aux/2) is 0).
 * GHMM_OPT_ROBUST is not available: every call below returns GHMM_ERR_UNSUPPORTED with it. */
typedef struct ghmm_fmodel ghmm_fmodel;
int ghmm_fmodel_create(ghmm_ctx *ctx, int N, int M, int D, ghmm_fmodel **out);
void ghmm_fmodel_destroy(ghmm_ctx *ctx, ghmm_fmodel *fm);
/* host -> device; also rebuilds the per-Gaussian constants den = pow(2 pi, D/2) * sqrt(|det|) and
 * log(c) - log(den), and log A (A > 0 ? log(A) : -inf) for the Viterbi calls, all on the host */
int ghmm_fmodel_set(ghmm_ctx *ctx, ghmm_fmodel *fm, const double *A, const double *c,
                    const double *mean, const double *inv_cov, const double *det);
/* device -> host (synchronises); any pointer may be NULL */
int ghmm_fmodel_get(ghmm_ctx *ctx, ghmm_fmodel *fm, double *A, double *c, double *mean,
                    double *inv_cov, double *det);
int ghmm_fmodel_dims(const ghmm_fmodel *fm, int *N, int *M, int *D);
/* calc_symbol_probab + calc_gaus (RC:855-954): b[F][N] into the workspace, readable with
 * ghmm_fetch(GHMM_BUF_B).  The row API of the diagonal models refuses these densities. */
int ghmm_emission_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c);
/* emission + calc_alpha (RC:733-800) + calc_probability (RC:822-836) per utterance:
 * log P = -sum_t log c_t, WITHOUT the final-state term log alpha^_{N-1}(T-1) that the diagonal
 * recogniser adds (ghmm_score).  Synchronises, writes loglik[U] on the host. */
int ghmm_score_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, double *loglik_host);
/* The vocabulary loop of RC (RC:326-374) in two launches, like ghmm_score_batch: one emission
 * launch over the concatenated Gaussians of all words, one forward launch over every (word,
 * utterance) pair.  All models share M and D.  loglik_host[k*U + u] = log P(utterance u | model k),
 * bit for bit what ghmm_score_full gives word by word.  Synchronises. */
int ghmm_score_full_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *c,
                          double *loglik_host);
/* Viterbi decoding of full-covariance models (absent from the reference, as the diagonal Viterbi
 * is): the diagonal definition (ghmm_viterbi, oracle/ghmm_oracle.c) with the quadratic form above.
 *     lk = log(c) - log(den);  e_m = lk_m - aux_m / 2     (den and aux as in calc_gaus above)
 *     log b_i(t) = m + log(sum_m exp(e_m - m)),  m = max_m e_m;  -inf when every e_m is -inf
 * (so c == 0 gives e = -inf; det == 0 gives lk = +inf and a log b of NaN, the formula's values).
 * In the log domain a frame far from every Gaussian keeps a finite log b where the linear densities
 * of ghmm_score_full underflow to 0 (its score is then -inf or NaN).  The lattice is ghmm_viterbi's:
 * one-hot start, delta_t(j) = max_i (delta_{t-1}(i) + log a_ij) + log b_j(t), ties take the lowest
 * i, score = delta_{T-1}(N-1), path by back-pointers from state N-1; T = 0 scores 0.  The score
 * therefore ends in the last state: it is not RC's forward score, which has no final-state term.
 * path_host[F] = state per frame, score_host[U] = best log score; U = 0 touches neither.
 * Afterwards ghmm_fetch(GHMM_BUF_B) returns log b[F][N].  Synchronises. */
int ghmm_viterbi_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, int32_t *path_host,
                      double *score_host);
/* The Viterbi score of every (word, utterance) pair in three launches, like ghmm_score_full_batch:
 * the gather of the words' Gaussians, one log-emission launch over the concatenated vocabulary and
 * one lattice launch (score only, no path).  All models share M and D.  score_host[k*U + u] is bit
 * for bit what ghmm_viterbi_full gives word k; GHMM_BUF_B then holds log b[F][sum of N].
 * Synchronises. */
int ghmm_viterbi_full_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *c,
                            double *score_host);
/* The forward score of full-covariance models in the log domain (absent from the reference): the
 * sum over paths where ghmm_viterbi_full takes the best one, on the same log b, lk and log A
 * (log a_ij = a_ij > 0 ? log(a_ij) : -inf, formed by ghmm_fmodel_set).
 *     la_0(j) = (j == 0 ? 0 : -inf) + log b_j(0)                      (the one-hot start)
 *     la_t(j) = LSE_{i : a_ij > 0} (la_{t-1}(i) + log a_ij) + log b_j(t)
 *     LSE(x)  = m + log(sum_i exp(x_i - m)),  m = max_i x_i
 * LSE is -inf when it has no term or every term is -inf, and NaN when a term is NaN.  A transition
 * with a_ij == 0 is not a term: a NaN in a predecessor that cannot be reached from does not leak.
 *     final_state == 0:  log P = LSE_j la_{T-1}(j)   calc_probability (RC:822-836), no final-state
 *                        term; equal to ghmm_score_full up to rounding wherever that is finite
 *     final_state != 0:  log P = la_{T-1}(N-1)       the trainer's convention (TFF:299): the log P
 *                        that ghmm_estep_full leaves in GHMM_BUF_LOGLIK, and the sum-over-paths
 *                        counterpart of ghmm_viterbi_full's score
 * Where the linear densities of ghmm_score_full underflow to 0 on a whole frame (its score is then
 * -inf or NaN) this score stays finite.  T = 0 scores 0; U = 0 touches nothing.  Caps and refusals
 * are ghmm_score_full's (GHMM_OPT_ROBUST set: GHMM_ERR_UNSUPPORTED).  The lattice launch counts
 * under GHMM_K_FORWARD.  Afterwards ghmm_fetch(GHMM_BUF_B) returns log b[F][N].  Synchronises. */
int ghmm_logscore_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, int final_state,
                       double *loglik_host);
/* The same score of every (word, utterance) pair in three launches, like ghmm_viterbi_full_batch:
 * the gather, one log-emission launch over the concatenated vocabulary, one lattice launch.  All
 * models share M and D.  loglik_host[k*U + u] is bit for bit what ghmm_logscore_full gives word k
 * (that call is the same lattice kernel on a table of one word); GHMM_BUF_B then holds
 * log b[F][sum of N].  Synchronises. */
int ghmm_logscore_full_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models, ghmm_corpus *c,
                             int final_state, double *loglik_host);

/* -------------------------------------------- the full-covariance trainer */

/* TFF = train/source/hmm-full-fs/hmm_continuous_full_fs.c, the reference's full-covariance trainer
 * (the one that wrote the models RC reads).  One feature stream, on a ghmm_fmodel, whose caps hold:
 * 1 <= N <= 64, M >= 1, 1 <= D <= 48.  GHMM_OPT_ROBUST is refused with GHMM_ERR_UNSUPPORTED.
 * Statistics vector of the full-covariance layout, in doubles (G = N*M, DT = D(D+1)/2):
 *   num_a[N*N]  den_a[N]  den_c[N]        TFF:1601-1660 (the diagonal trainer's sums)
 *   num_c[G]  num_mu[G*D]                  TFF:1740-1744
 *   num_cov[G*DT]                          TFF:1748-1750, upper triangle k <= l, row-major, around
 *                                          the OLD mean
 *   loglik  n_utt                          TFF:299-300
 * Being flat like the diagonal one, ghmm_stats_download / _upload / _loglik / _allreduce take it as
 * they are; the diagonal calls (ghmm_estep, ghmm_mstep, ...) refuse it. */
size_t ghmm_stats_len_full(int N, int M, int D);
int ghmm_stats_create_full(ghmm_ctx *ctx, int N, int M, int D, ghmm_stats **out);
/* One E-step over the whole corpus (TFF:254-301): calc_symbol_probab + calc_gaus with the mixture
 * posteriors (TFF:1775-1887: densities of +inf become 1e20, post = c*gaus / b or 0 where b == 0),
 * the diagonal trainer's recursions on fm's A with the final-state term in log P, then
 * calc_mix_param (TFF:1714-1753) and an ordered reduction into `stats` (overwritten; bitwise
 * reproducible).  Afterwards ghmm_fetch(GHMM_BUF_B / _POST / _GAMMA ...) returns the trainer's
 * arrays.  Asynchronous on the context's stream. */
int ghmm_estep_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_stats *stats);
/* The same E-step with every quantity formed in the log domain (absent from the reference): where
 * ghmm_estep_full's linear densities underflow to 0 on a whole frame (c_t = 1/0, NaN statistics) this
 * call keeps finite statistics.  ghmm_estep_full's contract otherwise: the same
 * ghmm_stats_create_full vector, overwritten; asynchronous on the context's stream; bitwise
 * reproducible; GHMM_OPT_DELTA and GHMM_OPT_PARTIALS honoured; GHMM_OPT_ROBUST gives
 * GHMM_ERR_UNSUPPORTED, a diagonal statistics vector GHMM_ERR_ARG; ghmm_mstep_full takes the result.
 * Emission: lk, e_m = lk_m - aux_m / 2 and log b_i(t) are ghmm_viterbi_full's, from the same online
 * log-sum-exp, bit for bit.
 *     post_t(i,m) = exp(e_m - log b_i(t)), or 0 where log b_i(t) = -inf
 * TFF's clamp of a +inf density to 1e20 has no counterpart: a Gaussian that is not positive definite
 * keeps its finite e.
 * Lattice: log a_ij is ghmm_fmodel_set's; a transition with a_ij == 0 is not a term; LSE as above.
 *     la_0(j)      = (j == 0 ? 0 : -inf) + log b_j(0)
 *     la_t(j)      = LSE_{i : a_ij > 0} (la_{t-1}(i) + log a_ij) + log b_j(t)     (ghmm_logscore_full's)
 *     lbe_{T-1}(i) = (i == N-1 ? 0 : -inf)
 *     lbe_t(i)     = LSE_{j : a_ij > 0} (log a_ij + (log b_j(t+1) + lbe_{t+1}(j)))
 *     log P_u      = la_{T-1}(N-1)            -> GHMM_BUF_LOGLIK and the vector's loglik (TFF:299)
 *     log Z_u      = LSE_j la_{T-1}(j)        the normaliser of gamma and xi
 *     gamma_t(i)   = exp(la_t(i) + lbe_t(i) - log Z_u)
 *     xi_t(i,j)    = exp(la_t(i) + log a_ij + log b_j(t+1) + lbe_{t+1}(j) - log Z_u),
 *                    t < T-1, a_ij > 0, i <= j <= i + delta
 *     num_a[i][j] = sum_u sum_{t<T-1} xi_t(i,j);  den_a[i] = sum_u sum_{t<T-1} gamma_t(i);
 *     den_c[i] = sum_u sum_{t<T} gamma_t(i);  num_c / num_mu / num_cov: calc_mix_param on
 *     w = gamma * post, the launches of ghmm_estep_full.
 * The normaliser is log Z_u, not log P_u: TFF's scaled recursions give gamma = alpha^ beta^ / c_t,
 * which divides by the probability of the observations over ALL end states while beta starts in the
 * last state only, so a frame's gammas sum to exp(log P_u - log Z_u) <= 1, the same value at every t.
 * An utterance with T < N or no path into the last state has every lbe = -inf: its gammas are exactly
 * 0 and log P_u = -inf, as in the linear call.  Where log Z_u is not finite the utterance's gamma rows
 * are 0 and it adds nothing to any sum except loglik (its log P_u as it is) and n_utt.  T = 0 adds 0 to
 * loglik and counts in n_utt.  A NaN log b (det == 0) gives the formula's values.
 * Afterwards ghmm_fetch returns GHMM_BUF_B: log b, _POST, _GAMMA, _LOGLIK, _ALPHA: la, _BETA: lbe.
 * The lattice launch counts under GHMM_K_FORWARD. */
int ghmm_estep_full_log(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_stats *stats);
/* The M-step (TFF:306-341): downloads the statistics and the model, applies ghmm_mstep_full_host
 * with GHMM_OPT_DELTA, and sets the model again.  Synchronises. */
int ghmm_mstep_full(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_stats *stats);
/* The same M-step (TFF:306-341) by HIP kernels on the context's stream, where `stats` lies (owned,
 * wrapped or just all-reduced): nothing is downloaded, no model arithmetic runs on the host, the
 * stream is not synchronised.  `fm` is rewritten in place; GHMM_OPT_DELTA is honoured; a diagonal
 * statistics vector or one of another shape gives GHMM_ERR_ARG, a null model GHMM_ERR_ARG.
 * M <= 256 (what the per-state kernel keeps in LDS): above it the call returns GHMM_ERR_UNSUPPORTED,
 * launches nothing and leaves the model as it is (ghmm_mstep_full has no such cap).
 * A, c, mean, the matrix slot and det are ghmm_mstep_full_host's BIT FOR BIT (a NaN's sign and payload
 * aside): the same correctly rounded operations, uncontracted, in the same order.  Its quirks:
 *   updating_transition_probab (TFF:1907-1929): a row with den_a == 0 is kept; inside i <= j <= i + delta
 *     a = num_a / den_a, outside it 0.
 *   updating_mix_param (TFF:1951-2000): a state with den_c == 0 is skipped, and its matrix slot, which
 *     holds last iteration's INVERSE, is inverted again; otherwise c = num_c / den_c, mean = num_mu /
 *     num_c, upper triangle = num_cov / num_c (num_c == 0: 0/0 entries), diagonal floored at 1e-5, mirrored.
 *   changing_zero_coef (TFF:1377-1393) per state: weights floored at 1e-5, summed in index order, divided.
 *   inv_cov_matrix (TFF:2058-2202) per Gaussian, D > 1: decomposition with its serial k sums; det = the
 *     product of the pivots in index order, a NaN det becomes 0; det == 0 leaves the matrix un-inverted;
 *     inv_triang_matrix by subdiagonals; the product sums (im*im)/d terms in increasing k and mirrors the
 *     upper triangle.  D = 1: det = var, inverse = 1 / var, no treat_zero_det.
 *   treat_zero_det (TFF:2226-2265) per state, D > 1: `sorting`'s stable decreasing order (strict <); a
 *     Gaussian with det < 1e-20 takes the next donor's mean x1.05 (the donor's x0.95), matrix, det and half
 *     its weight, serially over j, so a donor may already have been modified; the weights are renormalised;
 *     M = 1 splits the Gaussian with itself.
 * The derived constants are formed on the device as ghmm_mstep forms the diagonal ones: pow(2 pi, D/2)
 * comes from the host as a kernel argument, den = that * sqrt(|det|), lk = log(c) - log(den), log a =
 * a > 0 ? log(a) : -inf.  These three are NOT bit-equal to ghmm_fmodel_set's, which uses the host's
 * pow(x, 0.5) and log: they agree to the last few ulp.
 * The model's band flag (which recursions the next E-step takes) becomes `was banded && delta <= 1`, as
 * in ghmm_mstep: the host does not see the new A, so the flag is conservative (a model set with a wider
 * A keeps the general recursions).  Both launches count under GHMM_K_MSTEP. */
int ghmm_mstep_full_dev(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_stats *stats);

/* ---------------------- the full-covariance trainer and recogniser on several feature streams */

/* TFF and RC both take param_number = P feature streams: every recursion runs on the product over the
 * streams of the emission densities, taken in stream order from 1.0 (TFF:1436-1442, TFF:1460-1465,
 * RC:760-789), while calc_symbol_probab, calc_mix_param and the mixture update run once per stream
 * with that stream's own mixtures (TFF:256-297, TFF:316-342).  The three calls below mirror
 * ghmm_estep_streams / ghmm_score_streams:
 *   1 <= n_streams <= GHMM_MAX_STREAMS;  models[p] / corpora[p] = stream p;
 *   every stream has the same N, the same utterance count and the same lengths;
 *   every stream has its own M_p and D_p, within ghmm_fmodel's caps;
 *   the transitions (A, log A, the band flag) are models[0]'s;
 *   n_streams == 1 is the single-stream call itself (ghmm_estep_full, or with log_domain
 *   ghmm_estep_full_log; ghmm_score_full; ghmm_logscore_full): the same bits.
 * The product is formed by the emission launches: stream 0 writes b, the launch of every later stream
 * multiplies its density into it with one IEEE multiply, the earlier streams' product on the left, so
 * b = ((b^0 * b^1) * b^2)..., which is the reference's `product = 1.0; product *= ...` since
 * 1.0 * b^0 == b^0.  In the log domain log b = ((log b^0 + log b^1) + log b^2)...; NaN and +-inf
 * propagate as the multiplication or addition gives them.  Each stream's mixture posteriors are formed
 * from that stream's own density, and TFF's 1e20 clamp applies per stream (TFF:1775-1887).
 * Asynchrony, reproducibility, GHMM_OPT_DELTA and GHMM_OPT_PARTIALS are the single-stream calls'.
 * Afterwards GHMM_BUF_B holds the product (or the sum of logs) and GHMM_BUF_GAMMA / _ALPHA / _BETA /
 * _LOGLIK are as after the single-stream call; GHMM_BUF_POST is not part of the contract when
 * n_streams > 1.  The workspace is owned as after ghmm_emission_full: the diagonal row API refuses it.
 * Refusals, each before anything is launched: GHMM_OPT_ROBUST set gives GHMM_ERR_UNSUPPORTED; a null
 * array or entry, n_streams outside the range, streams that differ in N, in the utterance count or in
 * a length, a corpus of another D than its model, or a statistics vector that is diagonal or not of its
 * stream's shape gives GHMM_ERR_ARG.
 * Viterbi over several streams and the batched vocabulary calls (*_full_batch) for several streams are
 * in the section "several-stream vocabularies" below. */
/* One E-step over the whole corpus.  stats[p] is a ghmm_stats_create_full(N, M_p, D_p) vector.
 * log_domain == 0: every stream's emission as in ghmm_estep_full, ghmm_estep_full's recursion launches
 * on the product, then calc_mix_param and the reductions once per stream with that stream's
 * posteriors, frames and means (TFF:289-297).  log_domain != 0: ghmm_estep_full_log's definition with
 * log b = sum_p log b^p in stream order and per-stream post.  The common sums (num_a, den_a, den_c,
 * loglik, n_utt) go into every vector, so ghmm_mstep_full(models[p], stats[p]) or ghmm_mstep_full_dev
 * for every p is the M-step of TFF:313-342; all of them write the same A. */
int ghmm_estep_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                            int n_streams, ghmm_stats *const *stats, int log_domain);
/* ghmm_score_full on the product: no final-state term (RC:822-836).  Synchronises. */
int ghmm_score_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                            int n_streams, double *loglik_host);
/* ghmm_logscore_full on the sum of the streams' log b, with both final_state conventions: finite
 * where the linear product underflows to 0.  Synchronises. */
int ghmm_logscore_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                               int n_streams, int final_state, double *loglik_host);

/* ------------- several-stream vocabularies: Viterbi, batched scoring and word decoding (full-covariance) */

/* ghmm_viterbi_full on the sum of the streams' log b, log b = ((log b^0 + log b^1) + ...) as
 * ghmm_logscore_full_streams forms it, with models[0]'s log A: path_host[F], score_host[U].
 * n_streams == 1 is ghmm_viterbi_full itself, the same bits.  Afterwards GHMM_BUF_B holds the summed
 * log b[F][N].  The checks and refusals are those of the three calls above, and a null destination with
 * U > 0 gives GHMM_ERR_ARG; U = 0 touches nothing.  Synchronises. */
int ghmm_viterbi_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, ghmm_corpus *const *corpora,
                              int n_streams, int32_t *path_host, double *score_host);
/* A vocabulary of n_models words on n_streams streams in one pass, for the four calls below:
 *   models[k * n_streams + p] = stream p of word k;  corpora[p] = stream p of the utterances;
 *   the streams of one word have the same N; for every stream p all words share M_p and D_p;
 *   the corpora have the same utterance count and lengths, corpora[p] has D_p coefficients.
 * Per stream one gather of the words' Gaussians into that stream's concatenated vocabulary (kept in the
 * context between calls, rebuilt when its shape changes) and one emission launch over it, stream 0
 * plain, every later stream folded into the same b[F][NS] (NS = the sum of the words' N) as in the
 * calls above; then the one lattice launch of the single-stream *_full_batch call on word k's columns
 * and stream 0's A or log A: 2 n_streams + 1 launches and one wait for the stream.
 * out[k*U + u] is bit for bit what the matching call above gives word k alone (ghmm_score_full_streams,
 * ghmm_logscore_full_streams, ghmm_viterbi_full_streams' score).  n_streams == 1 is the *_full_batch
 * call, the same bits and the same cached vocabulary.  Afterwards GHMM_BUF_B holds the product (or the
 * sum of logs) over [F][NS]; the diagonal row API refuses the workspace.  U = 0 touches nothing.
 * Refusals, each before anything is launched or written.  GHMM_ERR_ARG: a null array or entry,
 * n_models < 1, n_streams outside 1..GHMM_MAX_STREAMS, a null destination with U > 0, streams of one
 * word that differ in N, corpora that differ in the utterance count or in a length, a corpus whose D is
 * not its stream's.  GHMM_ERR_UNSUPPORTED: GHMM_OPT_ROBUST set; words that differ in M_p or D_p for
 * some stream p. */
int ghmm_score_full_streams_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                  ghmm_corpus *const *corpora, int n_streams, double *loglik_host);
int ghmm_logscore_full_streams_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                     ghmm_corpus *const *corpora, int n_streams, int final_state,
                                     double *loglik_host);
int ghmm_viterbi_full_streams_batch(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                    ghmm_corpus *const *corpora, int n_streams, double *score_host);
/* Which word was it, and how does it align (n_streams >= 1): ghmm_viterbi_full_streams_batch's score
 * table, every utterance's winning word picked on the device, and the winner's lattice run again with
 * back-pointers on the log b already in the workspace, all enqueued without a host round trip and
 * ended by one wait for the stream.
 *   score_host[n_models*U]  the batch call's table, bit for bit
 *   word_host[U]            the winner: best = 0; for k = 1 .. n_models-1 in order, k takes over if
 *                           score[k] > score[best], or if score[best] is NaN and score[k] is not.  Ties
 *                           go to the lowest word, a NaN never beats a number, and all NaN or all -inf
 *                           gives word 0
 *   path_host[F]            over utterance u's frames, bit for bit ghmm_viterbi_full_streams' path of
 *                           word word_host[u]
 * T = 0 scores 0 under every word, gives word 0 and no path entries.  U = 0 touches nothing.  The
 * vocabulary layout, GHMM_BUF_B afterwards and the refusals are the batch calls' (all three destinations
 * are needed when U > 0).  The two extra launches count under GHMM_K_VITERBI.  A second identical call
 * repeats every byte. */
int ghmm_recognise_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                ghmm_corpus *const *corpora, int n_streams, int32_t *word_host,
                                int32_t *path_host, double *score_host);
/* ghmm_connect_streams (above) for full-covariance words: the same definition, outputs and lattice launch
 * on ghmm_recognise_full_streams' log b[F][NS] (n_streams launches under GHMM_K_EMISSION, the folds being
 * the emission's own epilogue, one under GHMM_K_VITERBI, one wait for the stream); with
 * word_penalty = -inf word, path and score are that call's bits.  Refusals, each before anything is launched, grown or written: whatever
 * ghmm_recognise_full_streams refuses (GHMM_OPT_ROBUST set included; all four destinations are needed
 * when U > 0); a NaN or +inf penalty gives GHMM_ERR_ARG; more than 2048 states in the vocabulary gives
 * GHMM_ERR_UNSUPPORTED. */
int ghmm_connect_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                              ghmm_corpus *const *corpora, int n_streams, double word_penalty,
                              int32_t *word_host, int32_t *path_host, int32_t *begin_host,
                              double *score_host);
/* ghmm_connect_grammar_streams (above) for full-covariance words: the same definition, outputs, grammar
 * arrays, refusals and lattice launch on ghmm_recognise_full_streams' log b[F][NS] (n_streams launches
 * under GHMM_K_EMISSION, one under GHMM_K_VITERBI, one wait for the stream); consequences (a) to (c) hold
 * against ghmm_connect_full_streams and ghmm_align_full_streams.  GHMM_OPT_ROBUST set is refused as there. */
int ghmm_connect_grammar_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                      ghmm_corpus *const *corpora, int n_streams, const double *start,
                                      const double *pair, const double *fin, int32_t *word_host,
                                      int32_t *path_host, int32_t *begin_host, double *score_host);
/* ghmm_align_streams (above) for full-covariance words: the same definition, outputs, refusals and lattice
 * launch on ghmm_recognise_full_streams' log b[F][NS] (n_streams launches under GHMM_K_EMISSION, one under
 * GHMM_K_VITERBI, one wait for the stream); consequences (a) to (c) hold against
 * ghmm_viterbi_full_streams_batch, ghmm_recognise_full_streams and ghmm_connect_full_streams. */
int ghmm_align_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                            ghmm_corpus *const *corpora, int n_streams, const int32_t *seq,
                            const int32_t *seq_off, int32_t *word_host, int32_t *path_host,
                            int32_t *begin_host, double *score_host);
/* ghmm_estep_embed_streams (above) for full-covariance words: the same definition word for word (the la /
 * lbe / w / wi recursions, LSE2 only at the entries and exits, the tying over instances in ascending
 * order, den_a built on stay, the log Z_u normaliser, the T = 0 and U = 0 rules), with these differences.
 * models[k * n_streams + p] are ghmm_fmodels; stats[k * n_streams + p] is a ghmm_stats_create_full vector
 * of word k's stream-p shape, OVERWRITTEN, so that ghmm_mstep_full and ghmm_mstep_full_dev on it work
 * unchanged.  log b and the posteriors are ghmm_estep_full_streams(log_domain = 1)'s: one emission launch
 * per stream over the concatenated vocabulary, every later stream folded in by the launch's own epilogue;
 * column bo_k + i of log b holds, bit for bit, what ghmm_align_full_streams leaves there.
 *   num_c / num_mu / num_cov of stream p: calc_mix_param on w = gamma_t(k,j) * post^p_t(k,j,m), gamma tied,
 *                     by ghmm_estep_full's statistics launches on the concatenated model (frames whose
 *                     weights are all exactly 0, as in the columns of words an utterance does not hold,
 *                     add exactly nothing and are skipped)
 * Consequences:
 *   (a) with n_models == 1 and one-word transcripts, stats[p], GHMM_BUF_GAMMA, GHMM_BUF_LOGLIK, GHMM_BUF_B
 *       and (n_streams == 1) GHMM_BUF_POST are ghmm_estep_full_streams(log_domain = 1)'s on the same
 *       context and options, bit for bit;
 *   (b) with one-word transcripts and any vocabulary, word k's sums are those of the sub-corpus of its
 *       utterances, to rounding;
 *   (c) a transcript (k, k) gives word k the sum of what two separate copies of the word would get.
 * Asynchronous on the context's stream; a second identical call repeats every byte; GHMM_OPT_DELTA is
 * honoured; GHMM_OPT_REFORDER_COUNT reads 0.  Afterwards GHMM_BUF_B holds log b[F][NS], GHMM_BUF_GAMMA the
 * tied gamma[F][NS], GHMM_BUF_LOGLIK log P_u; GHMM_BUF_POST is served for n_streams == 1 and refused
 * beyond; GHMM_BUF_ALPHA, _BETA and _SCALE give GHMM_ERR_ARG.  A vector's mailbox is not written:
 * ghmm_stats_loglik copies and waits.
 * Refusals, each before anything is launched, grown or written: whatever ghmm_align_full_streams refuses
 * (GHMM_OPT_ROBUST set, a word outside the vocabulary, S_u > 2048 on an utterance with T > 0, an empty
 * transcript with T > 0, ...; both transcript arrays are needed when U > 0); GHMM_ERR_ARG for a null stats
 * array or entry, a vector that is not word k's stream-p full-covariance shape, or a diagonal one;
 * GHMM_ERR_UNSUPPORTED for a concatenated vocabulary whose NS * M_p * (1 + D_p + D_p (D_p + 1) / 2) sums
 * are more batches of 2048 than the statistics launch's grid takes.  U = 0 zeroes every vector and
 * launches nothing.
 * Per stream one gather and ONE launch under GHMM_K_EMISSION (the fold is the emission's epilogue); TWO
 * launches under GHMM_K_FORWARD; per stream one under GHMM_K_MIXSTATS and TWO brackets under GHMM_K_REDUCE:
 * ghmm_estep_full's reductions (k_fullstats_reduce and k_reduce_all, timed and counted as one, as in
 * every full-covariance E-step) and the scatter that hands every word its own blocks
 * (k_embed_scatter_full, csrc/ghmm_embed.hpp). */
int ghmm_estep_embed_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                  ghmm_corpus *const *corpora, int n_streams, const int32_t *seq,
                                  const int32_t *seq_off, ghmm_stats *const *stats);
/* ghmm_grammar_post_streams (above) for full-covariance words: the same definition, outputs, grammar arrays,
 * edge cases, consequences and refusals, on ghmm_recognise_full_streams' log b[F][NS] (n_streams launches
 * under GHMM_K_EMISSION, the folds being the emission's own epilogue, two under GHMM_K_FORWARD, one wait for
 * the stream).  GHMM_OPT_ROBUST set is refused as in ghmm_connect_grammar_full_streams. */
int ghmm_grammar_post_full_streams(ghmm_ctx *ctx, ghmm_fmodel *const *models, int n_models,
                                   ghmm_corpus *const *corpora, int n_streams, const double *start,
                                   const double *pair, const double *fin, double *occ_host,
                                   double *ent_host, double *loglik_host);

/* -------------------------------------- several GPUs: the one collective */

/* Utterances shard data-parallel over ranks (one rank = one process or host thread with
 * its own ghmm_ctx on its own GPU); the accumulators are plain sums over utterances
 * (TF:1614, 1618, 1660, 1716-1722, 318-320), so the ONLY exchange per EM iteration is one
 * sum of the flat statistics vector over ranks: ncclAllReduce(ncclDouble, ncclSum) of RCCL,
 * in place, on the context's stream.  Every rank then applies the same
 * ghmm_mstep redundantly (identical inputs, identical models, no broadcast).  RCCL
 * (librccl.so.1) is loaded on the first ghmm_comm_* call; a process that never makes one
 * does not touch it. */
typedef struct ghmm_comm ghmm_comm;
#define GHMM_COMM_ID_BYTES 128
/* rank 0: a fresh rendezvous id (ncclGetUniqueId) to hand to every rank out of band */
int ghmm_comm_unique_id(void *id_bytes);
/* collective over all `world` ranks (ncclCommInitRank) */
int ghmm_comm_create(ghmm_ctx *ctx, const void *id_bytes, int rank, int world, ghmm_comm **out);
/* the same with the id passed through a file: rank 0 creates the id and writes `path`
 * (atomically, via rename), the other ranks wait up to timeout_s for it to appear; rank 0
 * removes the file once every rank has joined (ghmm_rendezvous_file below).  A `path` per job is
 * good practice, no longer a requirement. */
int ghmm_comm_create_file(ghmm_ctx *ctx, const char *path, int rank, int world, double timeout_s,
                          ghmm_comm **out);
/* the id exchange of ghmm_comm_create_file on its own — host code, no GPU, no RCCL (also in
 * libghmm_host.so): rank 0 passes its id IN and returns once every other rank has taken it;
 * the other ranks receive it in id_bytes.  Ranks announce themselves in `path`.join.<rank>
 * with a fresh nonce that the published `path` echoes, so a file left by an earlier job is
 * never taken for this job's id; a rank 0 that starts late is waited for; every wait ends
 * after timeout_s with GHMM_ERR_IO.  world = 1: returns at once, nothing is written. */
int ghmm_rendezvous_file(const char *path, int rank, int world, double timeout_s, void *id_bytes);
void ghmm_comm_destroy(ghmm_comm *comm);
int ghmm_comm_rank(const ghmm_comm *comm);
int ghmm_comm_size(const ghmm_comm *comm);
/* stats <- sum over ranks of stats, in place, asynchronous on the context's stream */
int ghmm_stats_allreduce(ghmm_ctx *ctx, ghmm_stats *stats, ghmm_comm *comm);
/* ghmm_model_init over a corpus sharded across ranks: the k-means sums of every pass are
 * all-reduced, every rank does the same cell bookkeeping and ends with the same model.
 * comm == NULL: this rank's corpus alone (= ghmm_model_init). */
int ghmm_model_init_comm(ghmm_ctx *ctx, ghmm_model *m, ghmm_corpus *c, ghmm_comm *comm);
/* The full-covariance trainer's initial model (creating_initial_model, TFF:731-1134) from a corpus in
 * HBM: ghmm_init_model_full's definition (below), computed by HIP kernels and written into `fm` in
 * place — A, c, mean, the matrix slot, det, and den / lk / log A formed on the device as
 * ghmm_mstep_full_dev forms them.  The model's band flag is set (A is one-step left-to-right).
 * comm == NULL: this rank's corpus alone.  Otherwise the corpus is one rank's shard: every pass's sums
 * are all-reduced on the stream (ghmm_stats_allreduce's collective) and every rank ends with the same
 * model, as in ghmm_model_init_comm.
 * Stream: every pass is enqueued on the context's stream with no host round trip between them, and the
 * call RETURNS WITHOUT WAITING for them, like ghmm_mstep_full_dev; ghmm_fmodel_get, ghmm_ctx_sync or
 * any later call on the same context is ordered after it.
 *   Segmentation: uniform, every utterance cut into N runs of T / N frames, the first T % N runs one
 *     frame longer (TFF:1005-1013); state i owns run i.  A state that owns no frame gets the host's
 *     0/0 values (NaN mean, matrix and weight, det 0).
 *   A: init_transition_probab (TFF:772-791), a_ij = 1 / min(2, N - i) for j = i, i + 1, else 0.
 *   Cells (init_mix_mean, TFF:970-1134): the state's mean first; while 2n < M every cell is split
 *     x1.05 / x0.95, otherwise the M - n cells of largest distortion are split x1.005 / x0.995, in
 *     `sorting`'s order (adjacent swaps, strict <).  Each level runs five nearest-mean passes: squared
 *     Euclidean distance summed in coefficient order, strict < from 1e20 so the lowest cell wins a tie
 *     and a cell whose mean is NaN is never chosen.  After every pass mean = sum / count, and empty
 *     cells are re-seeded x1.005 / x0.995 from the cells of largest distortion, in the host's order.
 *   Covariance (init_mix_param, TFF:810-952): one more classification against the final cells; each
 *     cell's upper triangle around the CELL MEAN (not the mean of the frames now assigned), divided by
 *     the count, the diagonal floored at 1e-5, mirrored; inv_cov_matrix per Gaussian as in
 *     ghmm_mstep_full_dev (D = 1: det = var, inverse = 1 / var) WITHOUT treat_zero_det; weights =
 *     count / (frames of the state), floored at 1e-5 and renormalised in index order; mean = the cell.
 *   One difference: a frame farther than 1e20 from every cell takes cell 0 (the host carries the
 *     previous frame's cell).  Reached only when some frame lies at least 1e10 from every cell of its
 *     state.
 * Given equal sums the quotients, the inverse, det and the weights are the host's bit for bit (the
 * shared, uncontracted bodies of the device M-step).  The sums themselves are added block by block in a
 * fixed order, so they differ from the host's frame-order sums in the last bits; the discrete parts (A,
 * every assignment and count, hence c where no floor applies) equal the host's wherever no frame sits
 * within rounding of a tie between two cells.  No floating-point atomics: two calls on the same inputs
 * give the same bits.
 * Caps: ghmm_fmodel's (N <= 64, D <= 48), and M <= 64 — above it the call returns
 * GHMM_ERR_UNSUPPORTED, launches nothing and leaves the model as it is (ghmm_init_model_full has no
 * such cap).  GHMM_OPT_ROBUST set: GHMM_ERR_UNSUPPORTED.  An empty corpus, a corpus of another D, a
 * null model or corpus: GHMM_ERR_ARG.
 * The context's workspace (GHMM_BUF_*) is overwritten: afterwards GHMM_BUF_GAMMA and GHMM_BUF_POST hold
 * the last classification's one-hot rows, and nothing an earlier E-step left is reused.  Counted under
 * GHMM_K_PREPARE (the passes and the last classification), GHMM_K_REDUCE (the cell bookkeeping and
 * the reductions), GHMM_K_MIXSTATS (the covariance sums) and GHMM_K_MSTEP (the finishing launches). */
int ghmm_fmodel_init(ghmm_ctx *ctx, ghmm_fmodel *fm, ghmm_corpus *c, ghmm_comm *comm);

/* ------------------------------------------------- host side: file formats */

#define GHMM_MAX_WORD 256

/* .perfil: int32 D, then T*D doubles, T implied by EOF (TF:527-581).
 * *X is malloc'ed; the caller frees it with ghmm_free(). */
int ghmm_perfil_read(const char *path, int *D, int *T, double **X);
int ghmm_perfil_write(const char *path, int D, int T, const double *X);
/* coefficient count and frame count from the header and the file size, nothing else read */
int ghmm_perfil_stat(const char *path, int *D, int *T);
void ghmm_free(void *p);

/* Length-balanced shard of `rank` among `world` (sort by length, deal in
 * turn): index[0 .. *n_out) = this rank's utterances in ascending index order (index has
 * room for (n_utt + world - 1) / world entries).  Frames per rank differ by at most the
 * longest utterance. */
int ghmm_shard_balanced(const int32_t *len, int n_utt, int rank, int world, int32_t *index,
                        int *n_out);

/* .hmm model file (writer TF:2043-2146, readers TF:604-711, RF:595-715), one
 * stream.  The reader accepts both a 4-byte and an 8-byte length prefix (the
 * shipped models come from a 32-bit build); the writer emits `len_bytes`
 * (8 = what a 64-bit build of the reference writes, or 4). Arrays are malloc'ed
 * by the reader. */
typedef struct ghmm_host_model {
    char word[GHMM_MAX_WORD];
    int N, M, D;
    double *A, *c, *mean, *inv_var, *det;
} ghmm_host_model;
int ghmm_host_model_alloc(ghmm_host_model *hm, int N, int M, int D);
void ghmm_host_model_free(ghmm_host_model *hm);
int ghmm_hmm_read(const char *path, ghmm_host_model *hm);
int ghmm_hmm_write(const char *path, const ghmm_host_model *hm, int len_bytes);
/* The same for models of several feature streams (the reference's param_number P, TF:2084-2099:
 * int M[P], int D[P], then per stream the states' mixtures): hm[p] = stream p with its own M and
 * D; word, N and A are common (the reader fills them into every hm[p]).  The reader takes up
 * to max_streams (<= GHMM_MAX_STREAMS) and reports the file's count. */
#define GHMM_MAX_STREAMS 8
int ghmm_hmm_read_streams(const char *path, ghmm_host_model *hm, int max_streams, int *n_streams);
int ghmm_hmm_write_streams(const char *path, const ghmm_host_model *hm, int n_streams, int len_bytes);
/* The full-covariance .hmm file (reader RC:591-707; what the reference's full-covariance trainer
 * writes, e.g. its shipped test/test/models): the same header, then per state c[M] and per
 * mixture mean[D], det, inv_cov[D][D].  One stream: the reader returns GHMM_ERR_UNSUPPORTED for
 * a file of several streams and GHMM_ERR_FORMAT for anything else that does not fit (a diagonal
 * .hmm included); 4- or 8-byte length prefix, told apart by the exact file size. */
typedef struct ghmm_host_fmodel {
    char word[GHMM_MAX_WORD];
    int N, M, D;
    double *A, *c, *mean, *det, *inv_cov;
} ghmm_host_fmodel;
int ghmm_host_fmodel_alloc(ghmm_host_fmodel *hfm, int N, int M, int D);
void ghmm_host_fmodel_free(ghmm_host_fmodel *hfm);
int ghmm_hmm_read_full(const char *path, ghmm_host_fmodel *hfm);
int ghmm_hmm_write_full(const char *path, const ghmm_host_fmodel *hfm, int len_bytes);
/* The same for full-covariance models of several feature streams (writer TFF:2278-2400, reader
 * RC:591-707): length-prefixed word, int N, int P, int M[P], int D[P], A[N][N], then per stream, per
 * state c[M_p] and per mixture mean[D_p], det, inv_cov[D_p][D_p].  hfm[p] = stream p with its own M
 * and D; word, N and A are common (the reader fills them into every hfm[p]).  The reader takes up to
 * max_streams (<= GHMM_MAX_STREAMS) and reports the file's count (more: GHMM_ERR_UNSUPPORTED); a
 * diagonal file, or anything else that does not fit, gives GHMM_ERR_FORMAT; 4- or 8-byte length
 * prefix, told apart by the exact file size.  ghmm_hmm_read_full keeps refusing P > 1. */
int ghmm_hmm_read_full_streams(const char *path, ghmm_host_fmodel *hfm, int max_streams, int *n_streams);
int ghmm_hmm_write_full_streams(const char *path, const ghmm_host_fmodel *hfm, int n_streams, int len_bytes);

/* creating_initial_model TF:732-1317 (uniform segmentation, LBG splitting with
 * factors 1.005/0.995, three k-means passes, per-cell variance floored at 1e-5)
 * on utterances already in host memory.  Host code. */
int ghmm_init_model(const double *X, const int32_t *len, int n_utt, int N, int M, int D,
                    ghmm_host_model *hm);

/* The full-covariance trainer's host side (TFF, see ghmm_estep_full), in the reference's order of
 * operations.  The matrix slot inv_cov of a Gaussian is TFF's cov_matrix: normally the inverse covariance. */
/* creating_initial_model (TFF:731-1134): uniform segmentation, LBG splitting x1.05 / x0.95 (the
 * split of the cells of largest distortion and the re-seeding of empty cells: x1.005 / x0.995),
 * five nearest-mean passes, the full covariance of each cell around its mean (diagonal floored at
 * 1e-5, mirrored), inverse and det by inv_cov_matrix (D = 1: det = var, inverse = 1 / var),
 * weights floored and renormalised; one-step left-to-right A. */
int ghmm_init_model_full(const double *X, const int32_t *len, int n_utt, int N, int M, int D,
                         ghmm_host_fmodel *hfm);
/* The M-step of main (TFF:306-341) on a full statistics vector: updating_transition_probab
 * (TFF:1907-1929, inside the band i <= j <= i + delta), updating_mix_param (TFF:1951-2000) with
 * changing_zero_coef, inv_cov_matrix per Gaussian (TFF:2164-2202) and, for D > 1, treat_zero_det
 * per state (TFF:2226-2265).  The reference's quirks are kept: a state with den_c == 0 keeps its
 * matrix slot (an inverse) and has it inverted again; num_c == 0 gives 0/0 means; det == 0 (NaN
 * det included) leaves the matrix un-inverted; with M = 1 treat_zero_det splits a Gaussian with
 * itself (mean x0.9975, weight unchanged). */
int ghmm_mstep_full_host(const double *stats, int delta, ghmm_host_fmodel *hfm);
/* inv_cov_matrix (TFF:2164-2202) alone: LDL' decomposition, det = prod of the pivots (NaN -> 0),
 * cov[D*D] replaced by its inverse unless det == 0.  Returns det; 1 <= D <= 64. */
double ghmm_inv_cov_full(int D, double *cov);

/* -------------------------------------------- host side: synthetic corpora */

#define GHMM_SYNTH_SEED 20260104ull

/* ground truth: mean[N*M*D] ~ N(0, 2^2), stddev[N*M*D] ~ U[0.5, 1.5] */
int ghmm_synth_truth(uint64_t seed, int N, int M, int D, double *mean, double *stddev);
/* utterances first_utt .. first_utt+n_utt-1 of the corpus (seed): left-to-right
 * walk over the N states, one mixture per frame.  X holds sum(len)*D doubles. */
int ghmm_synth_utterances(uint64_t seed, int N, int M, int D, const double *mean,
                          const double *stddev, int64_t first_utt, int n_utt,
                          const int32_t *len, double *X);
/* starting model = truth perturbed by +-perturb (relative on stddev, in units
 * of stddev on the mean), uniform mixture weights, one-step left-to-right A */
int ghmm_synth_start_model(uint64_t seed, int N, int M, int D, const double *mean,
                           const double *stddev, double perturb, double *A, double *c,
                           double *mu0, double *inv_var0, double *det0);

#ifdef __cplusplus
}
#endif
#endif /* GHMM_H */
