// ghmm_fullcov.hpp — emission densities of the full-covariance recogniser (gfx950, vector ALU).
//
// calc_symbol_probab + calc_gaus of RC = test/source/recognition-full-fs/
// recognition_continuous_full_fs.c (RC:855-954), in the reference's direct form and order:
//   dif = x - mu;  t_i = sum_j dif[j] inv_cov[j][i] (j ascending);  aux = sum_i dif[i] t_i;
//   gaus = exp(-aux/2) / den;  b_i = sum_m c_m gaus_m (m ascending)
// with den = pow(2 pi, D/2) sqrt(|det|) prepared on the host (ghmm_fmodel_set).  The expanded
// form x'Cx - 2 mu'Cx + mu'C mu would put the work on the matrix cores, but its cancellation is
// what the diagonal tier needs a re-evaluation path for, and f64 MFMA gains at most ~1.2x over
// v_fma_f64 here (profiles/r1_mfma_f64_rate.txt: 77 vs 64 TFLOP/s, and the two pipes never
// overlap): this is the vector-ALU kernel alone.
//
// Shape: a block of FC_WAVES waves shares one tile of 64 frames (one frame per lane), read from
// HBM once, coalesced, into LDS.  Each wave takes up to FC_SC consecutive states of the
// (concatenated) model.  Per Gaussian, a lane holds the D partial sums t[] in registers; mean,
// inv_cov and den are wave-uniform (the Gaussian index is a loop counter), so they come through
// the scalar cache and every v_fma_f64 has one scalar operand: row j of inv_cov updates all D
// sums t[i] with the lane's dif[j] = x[j] - mu[j] (x from the LDS tile; recomputed for the last
// sum instead of held: a register array of dif[] and fully unrolled rows ran the scalar file out
// and spilled it into vector lanes).  DB = D rounded up to a multiple of 8 (template): the
// columns past D are computed and never read (they read the next row's values, or the slack
// behind the array).
// The densities of a wave's states go to an LDS tile first and leave as rows of contiguous
// states (b[F][NS], row-major): ordinary vector stores, 8 states = 64 bytes per frame row.
//
// FC_LOG is the full-covariance Viterbi's variant (ghmm_viterbi_full): log b instead of b, with
// the diagonal Viterbi's definition (oracle/ghmm_oracle.c, orc_log_emission) on the quadratic form
// above.  Per Gaussian e = lk - aux/2, lk = log(c) - log(den) prepared on the host like den;
// per state log b = m + log(sum_m exp(e_m - m)), m = max_m e_m, -inf when every e is -inf.
// The sum is taken online (one exp per Gaussian, as the linear form has): a larger e rescales the
// running sum by exp(m_old - e) and adds 1, any other adds exp(e - m), an e of -inf adds exactly 0.
// That is the oracle's sum up to rounding and gives its special values: an e of NaN makes the sum
// NaN (log b NaN unless every other e is -inf, then -inf), an e of +inf (det == 0, c > 0) makes
// m = +inf, where the oracle's exp(inf - inf) gives NaN.
//
// FC_LOGPOST is the log-domain E-step's variant (ghmm_estep_full_log): FC_LOG's online sum, operation
// for operation, so that log b has FC_LOG's bits, plus the mixture posteriors in FC_POST's pattern:
// e_m goes to post as it is formed and is replaced in place by exp(e_m - log b) once the state's
// log b is known, 0 where log b is -inf (each lane rereads only what it wrote itself).  There is no
// clamp of a +inf density: a Gaussian that is not positive definite keeps its finite e.
#pragma once
#include <hip/hip_runtime.h>

namespace ghmm {

constexpr int FC_WAVES = 4;   // waves per block (one frame tile)
constexpr int FC_SC = 8;      // states per wave
constexpr int FC_DMAX = 48;   // widest feature vector built
constexpr int FC_SLACK = 64;  // doubles allocated behind mean[] and inv_cov[] (the padded columns' reads)
// what k_emission_full writes into b
constexpr int FC_LIN = 0;  // the recogniser's densities (RC)
constexpr int FC_POST = 1; // the trainer's densities and the mixture posteriors (TFF)
constexpr int FC_LOG = 2;  // log densities for the Viterbi lattice
constexpr int FC_LOGPOST = 3; // log densities and the mixture posteriors for the log-domain E-step

// doubles of LDS a block needs: the frame tile and every wave's density tile
__host__ __device__ inline int fc_lds_doubles(int D) { return WAVE * (D | 1) + FC_WAVES * WAVE * (FC_SC | 1); }

//
// MODE = FC_POST is the trainer's variant (TFF = train/source/hmm-full-fs/hmm_continuous_full_fs.c,
// calc_symbol_probab + calc_gaus, TFF:1775-1887), which also writes the mixture posteriors
// post[F][NS*M].  It differs from the recogniser's in two places, both reproduced:
//   - a density of +inf becomes 1e20 (`isinf(gaus) == 1`: +inf only; a Gaussian with det == 0,
//     whose density the reference leaves uninitialised, keeps the recogniser's exp(-aux/2) / 0);
//   - the weighted density c * gaus is rounded before it is added into b (multiply, add, then
//     divide): post = (c * gaus) / b, or 0 where b == 0.
// The weighted densities go to post as they are formed and are divided in place once b is known
// (each lane rereads only what it wrote itself).
//
// FOLD is the variant for the second and later feature streams of a model of several streams
// (ghmm_estep_full_streams and the score calls, TFF:1436-1442, RC:760-789): everything up to the store
// epilogue is the stream's own, the 1e20 clamp and the posteriors (formed from the stream's own bi)
// included; the epilogue then combines with what b holds from the streams before instead of
// overwriting it: b = b_old * bt, one multiply with the earlier streams' product on the left (linear
// modes), or log b = logb_old + bt (log modes).  Stream 0 is launched without FOLD, so b ends as
// ((b0 * b1) * b2)..., the reference's `product = 1.0; product *= ...` (1.0 * b0 == b0).
template <int DB, int MODE = FC_LIN, bool FOLD = false>
__global__ void __launch_bounds__(FC_WAVES * WAVE)
k_emission_full(int NS, int M, int D, long long F, const double *__restrict__ X,
                const double *__restrict__ mean, const double *__restrict__ inv_cov,
                const double *__restrict__ den, const double *__restrict__ c, double *__restrict__ b,
                double *__restrict__ post, const double *__restrict__ lk)
{
    constexpr bool POST = MODE == FC_POST, LPOST = MODE == FC_LOGPOST, LOG = MODE == FC_LOG || LPOST;
    extern __shared__ double lds[];
    const int DS = D | 1; // odd row stride: conflict-free per-lane reads
    const int SS = FC_SC | 1;
    // (readfirstlane: the compiler takes threadIdx.x / WAVE for divergent, and the Gaussian's
    // loads would become vector loads of one address instead of scalar loads)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
    double *xt = lds;
    double *bt = lds + WAVE * DS + w * WAVE * SS;
    const long long f0 = (long long)blockIdx.x * WAVE;
    const int nf = (int)((F - f0) < WAVE ? (F - f0) : WAVE);
    for (int k = threadIdx.x; k < nf * D; k += FC_WAVES * WAVE) {
        const int r = k / D;
        xt[r * DS + (k - r * D)] = X[f0 * D + k];
    }
    __syncthreads();
    const int s0 = (blockIdx.y * FC_WAVES + w) * FC_SC;
    const int ns = s0 < NS ? (NS - s0 < FC_SC ? NS - s0 : FC_SC) : 0;
    // lanes past the corpus' last frame evaluate the tile's last frame again (never stored)
    const double *x = xt + (lane < nf ? lane : nf - 1) * DS;
    for (int s = 0; s < ns; s++) {
        double bi = 0.0;
        double mx = -INFINITY; // (LOG: the running maximum; bi is the sum relative to it)
        for (int m = 0; m < M; m++) {
            const size_t g = (size_t)(s0 + s) * M + m;
            const double *mu = mean + g * D;
            const double *C = inv_cov + g * D * D;
            double t[DB];
#pragma unroll
            for (int i = 0; i < DB; i++) t[i] = 0.0;
            for (int j = 0; j < D; j++) {
                const double dj = x[j] - mu[j];
                const double *row = C + j * D;
#pragma unroll
                for (int i = 0; i < DB; i++) t[i] = fma(dj, row[i], t[i]);
            }
            double aux = 0.0;
#pragma unroll
            for (int i = 0; i < DB; i++)
                if (i < D) aux = fma(x[i] - mu[i], t[i], aux); // (uniform branch)
            if constexpr (LOG) {
                const double e = lk[g] - 0.5 * aux;
                const bool up = e > mx; // (false for a NaN e)
                const double r = exp(up ? mx - e : (e == -INFINITY ? -INFINITY : e - mx));
                bi = up ? fma(bi, r, 1.0) : bi + r;
                mx = up ? e : mx;
                if constexpr (LPOST)
                    if (lane < nf) post[(f0 + lane) * ((long long)NS * M) + (long long)g] = e;
            } else if constexpr (POST) {
                double gaus = exp(aux * -0.5) / den[g];
                if (gaus == INFINITY && den[g] != 0.0) gaus = 1e20;
                const double gm = gaus * c[g];
                bi += gm;
                if (lane < nf) post[(f0 + lane) * ((long long)NS * M) + (long long)g] = gm;
            } else {
                const double gaus = exp(aux * -0.5) / den[g];
                bi += gaus * c[g];
            }
        }
        if constexpr (LOG) bi = mx == -INFINITY ? -INFINITY : mx == INFINITY ? NAN : mx + log(bi);
        if constexpr (POST) {
            if (lane < nf) {
                double *pr = post + (f0 + lane) * ((long long)NS * M) + (long long)(s0 + s) * M;
                for (int m = 0; m < M; m++) pr[m] = bi != 0.0 ? pr[m] / bi : 0.0;
            }
        }
        if constexpr (LPOST) {
            if (lane < nf) {
                double *pr = post + (f0 + lane) * ((long long)NS * M) + (long long)(s0 + s) * M;
                for (int m = 0; m < M; m++) pr[m] = bi != -INFINITY ? exp(pr[m] - bi) : 0.0;
            }
        }
        bt[lane * SS + s] = bi;
    }
    __syncthreads();
    for (int k = lane; k < nf * ns; k += WAVE) {
        const int r = k / ns, col = k - r * ns;
        if constexpr (FOLD) {
            double *dst = b + (f0 + r) * NS + s0 + col;
            *dst = LOG ? *dst + bt[r * SS + col] : *dst * bt[r * SS + col];
        } else {
            b[(f0 + r) * NS + s0 + col] = bt[r * SS + col];
        }
    }
}

// ---------------------------------------------------------------- trainer statistics
// calc_mix_param (TFF:1714-1753) over a block of frames: per Gaussian g the E = 1 + D + D(D+1)/2
// sums, with the weight w = gamma_t(state(g)) * post_t(g) and dif = x - (OLD) mean:
//   num_c += w;  num_mu[k] += w * x[k];  num_cov[k][l] += (w * dif[k]) * dif[l]  (k <= l)
// Element space G * E (element 0 of a Gaussian: num_c, 1..D: num_mu, then the upper triangle
// row-major: num_cov).  Same shape as k_mixstats: blockIdx.x = frame range, blockIdx.y = batch of
// FS_THREADS * FS_EPT elements; frames are staged through LDS together with their weights, with a
// column x[D] = 1 so that every element is one form, acc += (w * (x[k] - mu_k)) * (x[l] - mu_l):
// mu = 0 and l = D for num_mu, k = l = D for num_c (exact: the factors are 1).  Frames whose
// weights are all exactly 0 add exactly nothing and are skipped.  Each block writes its partial
// sums; k_fullstats_reduce adds them in block order: no atomics, bitwise reproducible.
constexpr int FS_THREADS = 256;
constexpr int FS_EPT = 8;
constexpr int FS_FRAMES = 32; // frames staged per pass (<= 64: one bit each in the skip mask)

__host__ __device__ inline int fs_elems(int D) { return 1 + D + D * (D + 1) / 2; }

__global__ void __launch_bounds__(FS_THREADS)
k_fullstats(int N, int M, int D, long long F, long long frames_per_block, int FSn,
            const double *__restrict__ X, const double *__restrict__ gamma, const double *__restrict__ post,
            const double *__restrict__ mean, double *__restrict__ part)
{
    extern __shared__ double lds[];
    const int G = N * M, D1 = D + 1, E1 = fs_elems(D);
    const long long E = (long long)G * E1;
    const int tid = threadIdx.x;
    const long long e0 = (long long)blockIdx.y * (FS_THREADS * FS_EPT);
    if (e0 >= E) return;
    const long long e1 = (e0 + FS_THREADS * FS_EPT < E) ? e0 + FS_THREADS * FS_EPT : E;
    const int g0 = (int)(e0 / E1), g1 = (int)((e1 - 1) / E1);
    const int GW = g1 - g0 + 1;
    double *xs = lds;           // [FSn][D1]
    double *ws = lds + FSn * D1; // [FSn][GW]
    const int kmax = (int)((e1 - e0 + FS_THREADS - 1) / FS_THREADS);

    int gx[FS_EPT], kx[FS_EPT], lx[FS_EPT];
    double mk[FS_EPT], ml[FS_EPT], acc[FS_EPT];
#pragma unroll
    for (int k = 0; k < FS_EPT; k++) {
        const long long e = e0 + tid + (long long)k * FS_THREADS;
        const bool ok = e < e1;
        const int g = ok ? (int)(e / E1) : g0;
        int r = ok ? (int)(e - (long long)g * E1) : 0, a = D, bb = D;
        if (r >= 1 && r <= D) {
            a = r - 1;
        } else if (r > D) {
            int q = r - 1 - D, row = 0;
            while (q >= D - row) {
                q -= D - row;
                row++;
            }
            a = row;
            bb = row + q;
        }
        gx[k] = g - g0;
        kx[k] = a;
        lx[k] = bb;
        mk[k] = (r > D) ? mean[(size_t)g * D + a] : 0.0;
        ml[k] = (r > D) ? mean[(size_t)g * D + bb] : 0.0;
        acc[k] = 0.0;
    }
    const long long fb0 = (long long)blockIdx.x * frames_per_block;
    const long long fb1 = (fb0 + frames_per_block < F) ? fb0 + frames_per_block : F;
    __shared__ unsigned long long nzmask;
    for (long long fs = fb0; fs < fb1; fs += FSn) {
        const int nf = (int)((fb1 - fs) < FSn ? (fb1 - fs) : FSn);
        __syncthreads();
        if (tid == 0) nzmask = 0ull;
        for (int k = tid; k < nf * GW; k += FS_THREADS) {
            const int r = k / GW, g = g0 + (k - r * GW);
            ws[k] = gamma[(fs + r) * N + g / M] * post[(fs + r) * G + g];
        }
        __syncthreads();
        if (tid < nf) {
            bool nz = false;
            for (int gl = 0; gl < GW; gl++) nz |= ws[tid * GW + gl] != 0.0;
            if (nz) atomicOr(&nzmask, 1ull << tid);
        }
        __syncthreads();
        const unsigned long long nzm = nzmask;
        if (nzm == 0ull) continue;
        for (int k = tid; k < nf * D1; k += FS_THREADS) {
            const int r = k / D1, d = k - r * D1;
            if ((nzm >> r) & 1ull) xs[k] = d < D ? X[(fs + r) * D + d] : 1.0;
        }
        __syncthreads();
        for (int r = 0; r < nf; r++) {
            if (!((nzm >> r) & 1ull)) continue;
            const double *xr = xs + r * D1;
#pragma unroll
            for (int k = 0; k < FS_EPT; k++)
                if (k < kmax) { // block-uniform
                    const double w = ws[r * GW + gx[k]];
                    const double wd = w * (xr[kx[k]] - mk[k]);
                    acc[k] = fma(wd, xr[lx[k]] - ml[k], acc[k]);
                }
        }
    }
#pragma unroll
    for (int k = 0; k < FS_EPT; k++) {
        const long long e = e0 + tid + (long long)k * FS_THREADS;
        if (e < e1) part[(size_t)blockIdx.x * E + e] = acc[k];
    }
}

// the frame-block partials [P][G*E] in block order into num_c / num_mu / num_cov of the full
// statistics layout (include/ghmm.h), one element per thread
__global__ void __launch_bounds__(256)
k_fullstats_reduce(int G, int D, int P, const double *__restrict__ part, double *__restrict__ stats_c)
{
    const int E1 = fs_elems(D);
    const long long E = (long long)G * E1, e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    double v = 0.0;
    for (int p = 0; p < P; p++) v += part[(size_t)p * E + e];
    const int g = (int)(e / E1), r = (int)(e - (long long)g * E1);
    const int DT = D * (D + 1) / 2;
    double *num_c = stats_c, *num_mu = num_c + G, *num_cov = num_mu + (size_t)G * D;
    if (r == 0) num_c[g] = v;
    else if (r <= D) num_mu[(size_t)g * D + r - 1] = v;
    else num_cov[(size_t)g * DT + r - 1 - D] = v;
}

// ghmm_score_full_batch / ghmm_viterbi_full_batch: word k's Gaussians (ng of them from g0) copied into the concatenated model
struct fgather_src {
    const double *c, *mean, *inv_cov, *den, *lk;
    int g0, ng;
};
__global__ void __launch_bounds__(256)
k_gather_fmodels(int D, const fgather_src *__restrict__ src, double *__restrict__ c, double *__restrict__ mean,
                 double *__restrict__ inv_cov, double *__restrict__ den, double *__restrict__ lk)
{
    const fgather_src s = src[blockIdx.x];
    for (int k = threadIdx.x; k < s.ng; k += 256) {
        c[s.g0 + k] = s.c[k];
        den[s.g0 + k] = s.den[k];
        lk[s.g0 + k] = s.lk[k];
    }
    const size_t n = (size_t)s.ng * D, o = (size_t)s.g0 * D;
    for (size_t k = threadIdx.x; k < n; k += 256) mean[o + k] = s.mean[k];
    const size_t n2 = n * D, o2 = o * D;
    for (size_t k = threadIdx.x; k < n2; k += 256) inv_cov[o2 + k] = s.inv_cov[k];
}

// ------------------------------------------------ the trainer's M-step on the device (ghmm_mstep_full_dev)
//
// ghmm_mstep_full_host (csrc/ghmm_fulltrain.c: TFF:306-341) in two launches on the context's stream:
//   k_fmstep_gauss  a block per Gaussian: updating_mix_param's quotients, the diagonal floor and the
//                   mirror, then inv_cov_matrix (decomposition, calc_det, inv_triang_matrix, the
//                   product) — or det = var, 1 / var at D = 1;
//   k_fmstep_state  a block per state, afterwards: the weights and changing_zero_coef, treat_zero_det
//                   (D > 1), the state's row of A, and den / lk / log A.
// Every value the host route computes is computed here by the same IEEE operations in the same order,
// so A, c, mean, the matrix slot and det come out bit-equal to the host's (NaN payloads aside).  That
// needs three things.  (1) No contraction: the library is built with -ffp-contract=on, so both bodies
// open with `#pragma clang fp contract(off)`; `/` on doubles is the correctly rounded division.
// (2) Every sum over k or l runs in ONE lane, in the host's order; the lanes only spread independent
// rows or entries.  (3) What the host does serially over Gaussians (sorting, the treat_zero_det walk,
// the weight sums) runs in lane 0 on LDS copies; the walk is reduced there to a list of (receiver,
// donor) pairs, and the D and D x D copies of each pair are then made by all lanes in the list's
// order.  A lane owns the same coefficient (entry) in every pair, so a donor that an earlier pair has
// modified is read as modified without a barrier.
// LDS of k_fmstep_gauss: the covariance [D][D | 1] — its strict lower triangle becomes T in place
// (decomposition reads an entry of cov only when it writes that entry of T), the diagonal and the
// upper triangle stay, and give the matrix back where det == 0 — the inverse of T [D][D | 1], and the
// pivots: (2 D (D | 1) + D) doubles, 38 016 bytes at D = 48.
constexpr int FM_THREADS = 256;
constexpr int FM_MAXM = 256;       // Gaussians per state k_fmstep_state holds in LDS (ghmm.h states it)
constexpr double FM_FLOOR = 1.0e-5;    // TFF:38
constexpr double FM_ZERO_DET = 1e-20;  // TFF:2242

__host__ __device__ inline size_t fm_gauss_lds_bytes(int D) { return ((size_t)2 * D * (D | 1) + D) * sizeof(double); }

// entry q of a row-major upper triangle (k <= l) of a D x D matrix
__device__ inline void fm_tri(int q, int D, int &k, int &l)
{
    int r = 0, o = 0;
    while (q - o >= D - r) {
        o += D - r;
        r++;
    }
    k = r;
    l = r + (q - o);
}

// INIT is ghmm_fmodel_init's variant (init_mix_param, TFF:883-930): every Gaussian is formed from the
// sums (there is no den_c to be zero) and its mean, which is the k-means cell, is kept
template <bool INIT>
__device__ __forceinline__ void fm_gauss_body(int N, int M, int D, const double *__restrict__ stats,
                                              double *__restrict__ mean, double *__restrict__ inv_cov,
                                              double *__restrict__ det, double *fm_lds)
{
#pragma clang fp contract(off)
    const int g = blockIdx.x, i = g / M, tid = threadIdx.x, G = N * M, DS = D | 1, DT = D * (D + 1) / 2;
    const double *den_c = stats + (size_t)N * N + N, *num_c = den_c + N, *num_mu = num_c + G;
    const double *num_cov = num_mu + (size_t)G * D;
    double *C = fm_lds, *IM = C + D * DS, *dd = IM + D * DS;
    double *cv = inv_cov + (size_t)g * D * D;
    // updating_mix_param (TFF:1951-2000); a state with den_c == 0 keeps its slot: last iteration's
    // inverse, inverted again below
    const bool upd = INIT || den_c[i] != 0.0;
    if (upd) {
        const double ncg = num_c[g];
        const double *nc = num_cov + (size_t)g * DT;
        if constexpr (!INIT)
            for (int k = tid; k < D; k += FM_THREADS) mean[(size_t)g * D + k] = num_mu[(size_t)g * D + k] / ncg;
        for (int q = tid; q < DT; q += FM_THREADS) {
            int k, l;
            fm_tri(q, D, k, l);
            double v = nc[q] / ncg;
            if (k == l && v < FM_FLOOR) v = FM_FLOOR; // (a NaN stays)
            C[k * DS + l] = v;
            C[l * DS + k] = v;
        }
    } else {
        for (int e = tid; e < D * D; e += FM_THREADS) C[(e / D) * DS + e % D] = cv[e];
    }
    __syncthreads();
    if (D == 1) { // TFF:330-334: det = var, inverse = 1 / var
        if (tid == 0) {
            det[g] = C[0];
            cv[0] = 1.0 / C[0];
        }
        return;
    }
    // decomposition (TFF:2058-2096): a lane per row below the pivot, the pivot's own sum in another
    // wave's lane; T[r][j] overwrites cov[r][j]
    if (tid == 0) dd[0] = C[0];
    for (int r = 1 + tid; r < D; r += FM_THREADS) C[r * DS] = C[r * DS] / C[0];
    __syncthreads();
    for (int j = 1; j < D; j++) {
        if (tid == FM_THREADS - 1) {
            double s = C[j * DS + j];
            for (int k = 0; k < j; k++) s -= C[j * DS + k] * C[j * DS + k] * dd[k];
            dd[j] = s;
        }
        for (int r = j + 1 + tid; r < D; r += FM_THREADS) {
            double s = C[r * DS + j];
            for (int k = 0; k < j; k++) s -= C[r * DS + k] * dd[k] * C[j * DS + k];
            C[r * DS + j] = s;
        }
        __syncthreads();
        for (int r = j + 1 + tid; r < D; r += FM_THREADS) C[r * DS + j] = C[r * DS + j] / dd[j];
        __syncthreads();
    }
    // calc_det (TFF:2020-2032), every lane for itself; a NaN becomes 0 (TFF:2176)
    double dt = 1.0;
    for (int k = 0; k < D; k++) dt *= dd[k];
    if (dt != dt) dt = 0.0;
    if (tid == 0) det[g] = dt;
    if (dt == 0.0) {
        // quirk (TFF:2179): the matrix stays as it came, un-inverted
        if (upd)
            for (int q = tid; q < DT; q += FM_THREADS) {
                int k, l;
                fm_tri(q, D, k, l);
                const double v = C[k * DS + l];
                cv[k * D + l] = v;
                cv[l * D + k] = v;
            }
        return;
    }
    // inv_triang_matrix (TFF:2118-2142) by subdiagonals, a lane per row
    for (int k = tid; k < D; k += FM_THREADS) IM[k * DS + k] = 1.0;
    __syncthreads();
    for (int k = 0; k < D - 1; k++) {
        for (int r = k + 1 + tid; r < D; r += FM_THREADS) {
            const int j = r - k - 1;
            double s = 0.0;
            for (int l = j; l < r; l++) s -= C[r * DS + l] * IM[l * DS + j];
            IM[r * DS + j] = s;
        }
        __syncthreads();
    }
    // the product (TFF:2183-2199): an entry of the upper triangle per lane, its k sum in order
    for (int q = tid; q < DT; q += FM_THREADS) {
        int a, b;
        fm_tri(q, D, a, b);
        double s = 0.0;
        for (int k = b; k < D; k++) s += IM[k * DS + a] * IM[k * DS + b] / dd[k];
        cv[a * D + b] = s;
        cv[b * D + a] = s;
    }
}

__global__ void __launch_bounds__(FM_THREADS)
k_fmstep_gauss(int N, int M, int D, const double *__restrict__ stats, double *__restrict__ mean,
               double *__restrict__ inv_cov, double *__restrict__ det)
{
    extern __shared__ double fm_lds[];
    fm_gauss_body<false>(N, M, D, stats, mean, inv_cov, det, fm_lds);
}

// INIT is ghmm_fmodel_init's variant: the row of A is init_transition_probab's formula (TFF:772-791),
// the weights are count / (frames of the state) (TFF:932-948; the state's frames are the sum of its
// cells' counts, exact), and there is no treat_zero_det (TFF:918-930)
template <bool INIT>
__device__ __forceinline__ void fm_state_body(int N, int M, int D, const double *__restrict__ stats, double norm2pi,
                                              int delta, double *__restrict__ A, double *__restrict__ c,
                                              double *mean, double *inv_cov, double *__restrict__ det,
                                              double *__restrict__ den, double *__restrict__ lk,
                                              double *__restrict__ logA)
{
#pragma clang fp contract(off)
    __shared__ double cw[FM_MAXM], dl[FM_MAXM];
    __shared__ int idx[FM_MAXM], pj[FM_MAXM], pl[FM_MAXM];
    __shared__ int npairs;
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *num_a = stats, *den_a = num_a + (size_t)N * N, *den_c = den_a + N, *num_c = den_c + N;
    // updating_transition_probab (TFF:1907-1929): a row with den_a == 0 is kept; 0 outside the band
    const double da = INIT ? 0.0 : den_a[i];
    for (int j = tid; j < N; j += FM_THREADS) {
        const size_t q = (size_t)i * N + j;
        double a;
        if constexpr (INIT) {
            if (j > delta + i || j < i) a = 0.0;
            else if (delta + 1 > N - i) a = 1.0 / (double)(N - i);
            else a = 1.0 / (double)(delta + 1);
            A[q] = a;
        } else {
            a = A[q];
            if (da != 0.0) {
                a = (j >= i && j - i <= delta) ? num_a[q] / da : 0.0;
                A[q] = a;
            }
        }
        logA[q] = a > 0.0 ? log(a) : -INFINITY;
    }
    double dc = den_c[i];
    if constexpr (INIT) {
        dc = 0.0; // (whole numbers: any order gives the same sum)
        for (int m = 0; m < M; m++) dc += num_c[(size_t)i * M + m];
    }
    for (int m = tid; m < M; m += FM_THREADS) {
        const size_t g = (size_t)i * M + m;
        cw[m] = (INIT || dc != 0.0) ? num_c[g] / dc : c[g];
        dl[m] = det[g];
    }
    __syncthreads();
    if (tid == 0) {
        // changing_zero_coef (TFF:1377-1393)
        double sum = 0.0;
        for (int k = 0; k < M; k++) {
            if (cw[k] < FM_FLOOR) cw[k] = FM_FLOOR;
            sum += cw[k];
        }
        for (int k = 0; k < M; k++) cw[k] = cw[k] / sum;
        int np = 0;
        if (!INIT && D > 1) {
            // treat_zero_det (TFF:2226-2265).  sorting (TFF:1331-1356): adjacent swaps, strict '<',
            // on the determinants as inv_cov_matrix left them
            for (int k = 0; k < M; k++) idx[k] = k;
            bool done = false;
            while (!done) {
                done = true;
                for (int k = 0; k < M - 1; k++) {
                    const int a = idx[k], b = idx[k + 1];
                    if (dl[a] < dl[b]) {
                        idx[k] = b;
                        idx[k + 1] = a;
                        done = false;
                    }
                }
            }
            // the walk: determinants and weights move here, means and matrices by the pairs below
            int n = 0;
            for (int j = 0; j < M; j++)
                if (dl[j] < FM_ZERO_DET) {
                    const int l = idx[n++];
                    pj[np] = j;
                    pl[np] = l;
                    np++;
                    dl[j] = dl[l];
                    cw[l] = cw[l] / 2.0;
                    cw[j] = cw[l];
                }
            sum = 0.0;
            for (int j = 0; j < M; j++) sum += cw[j];
            for (int j = 0; j < M; j++) cw[j] = cw[j] / sum;
        }
        npairs = np;
    }
    __syncthreads();
    const size_t DD = (size_t)D * D;
    for (int p = 0; p < npairs; p++) {
        const size_t gj = (size_t)i * M + pj[p], gl = (size_t)i * M + pl[p];
        for (int k = tid; k < D; k += FM_THREADS) {
            const double v = mean[gl * D + k], up = v * 1.05;
            mean[gj * D + k] = up;
            mean[gl * D + k] = (gj == gl ? up : v) * 0.95; // (M = 1, or its own donor: split with itself)
        }
        if (gj != gl)
            for (size_t e = tid; e < DD; e += FM_THREADS) inv_cov[gj * DD + e] = inv_cov[gl * DD + e];
    }
    // the derived constants, as the diagonal k_mstep forms them (ghmm_fmodel_set's on the host)
    for (int m = tid; m < M; m += FM_THREADS) {
        const size_t g = (size_t)i * M + m;
        const double cg = cw[m], d = dl[m];
        c[g] = cg;
        det[g] = d;
        const double dn = norm2pi * sqrt(fabs(d));
        den[g] = dn;
        lk[g] = log(cg) - log(dn);
    }
}

__global__ void __launch_bounds__(FM_THREADS)
k_fmstep_state(int N, int M, int D, const double *__restrict__ stats, double norm2pi, int delta,
               double *__restrict__ A, double *__restrict__ c, double *mean, double *inv_cov,
               double *__restrict__ det, double *__restrict__ den, double *__restrict__ lk,
               double *__restrict__ logA)
{
    fm_state_body<false>(N, M, D, stats, norm2pi, delta, A, c, mean, inv_cov, det, den, lk, logA);
}

// ------------------------------------------------ the trainer's initial model on the device (ghmm_fmodel_init)
//
// creating_initial_model (TFF:731-1134; csrc/ghmm_fulltrain.c ghmm_init_model_full and csrc/ghmm_init.c
// ghmm_init_cells_) without a trip to the host.  Per k-means pass:
//   k_finit_pass   classifies the frames and accumulates, per cell, D coefficient sums, the count and the
//                  distortion — the E2 = D + 2 numbers a pass needs, nothing of the covariance;
//   k_finit_cells  a block per state: adds the blocks' partials in block order, then the host loop's cell
//                  bookkeeping (quotients, re-seeding of empty cells, the split that opens the next level).
// The last pass (init_mix_param) is k_finit_pass once more, now writing the frames' one-hot gamma and post
// rows (the same classification rule in every pass), k_fullstats on them — its dif is taken around the
// model's mean, which is the cell — then k_finit_gauss / k_finit_state: the INIT variants of the M-step's
// bodies above.
//
// k_finit_pass: block (k, p) = state k, utterances [p * upb, (p + 1) * upb).  Under the uniform
// segmentation state k owns one contiguous run of every utterance (the first T % N runs one frame longer),
// so the block walks those runs only, FI_FRAMES frames at a time through LDS (rows D | 1 doubles apart:
// a lane per frame reads conflict-free).  Classification: wave w of the four takes cells w, w + 4, ... in
// ascending order with the host's strict '<' from 1e20 (a NaN distance is never smaller); lane r of wave 0
// then takes the smallest of the four candidates, the lowest cell among equals — the cell the host's one
// ascending scan keeps.  No candidate: cell 0 (the host carries the previous frame's cell; reached only by
// a frame >= 1e10 from every cell of its state).  The distance is the host's sum, uncontracted, in coefficient order.
// Accumulation: entry (cell c, l) of the block's [n_cells][E2] table in LDS belongs to ONE thread, the one
// with tid % E2 == l and tid / E2 == c % (FI_THREADS / E2), which walks the staged frames in order: no
// atomics, and a block's sums are the frames' in corpus order.  l < D: x[l]; l == D: 1; l == D + 1: the distance.
constexpr int FI_THREADS = 256;
constexpr int FI_FRAMES = 64;  // frames per stage: one lane of each wave per frame
constexpr int FI_MAXM = 64;    // cells per state (ghmm.h states it)
constexpr double FI_FAR = 1.0e20; // TFF:1179-1215

__host__ __device__ inline size_t fi_pass_lds_bytes(int M, int D)
{
    return ((size_t)M * (D | 1) + (size_t)M * (D + 2) + (size_t)FI_FRAMES * (D | 1)) * sizeof(double);
}

__global__ void __launch_bounds__(FI_THREADS)
k_finit_pass(int N, int M, int D, int n_cells, int classify, int U, int upb, const double *__restrict__ X,
             const long long *__restrict__ off, const double *__restrict__ cells, double *__restrict__ part,
             double *__restrict__ gamma, double *__restrict__ post)
{
#pragma clang fp contract(off)
    extern __shared__ double fi_lds[];
    __shared__ double cand_d[FI_THREADS / WAVE][FI_FRAMES];
    __shared__ int cand_c[FI_THREADS / WAVE][FI_FRAMES];
    __shared__ double dmin[FI_FRAMES];
    __shared__ int cid[FI_FRAMES], cgr[FI_FRAMES];
    constexpr int NW = FI_THREADS / WAVE;
    const int k = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, DS = D | 1, E2 = D + 2;
    const int w = tid / WAVE, lane = tid % WAVE;
    double *cl = fi_lds;               // [n_cells][DS]
    double *acc = cl + (size_t)M * DS; // [n_cells][E2]
    double *xs = acc + (size_t)M * E2; // [FI_FRAMES][DS]
    for (int e = tid; e < n_cells * D; e += FI_THREADS) {
        const int c = e / D;
        cl[c * DS + (e - c * D)] = cells[(size_t)k * M * D + e];
    }
    for (int e = tid; e < n_cells * E2; e += FI_THREADS) acc[e] = 0.0;
    const int ngrp = FI_THREADS / E2, l = tid % E2, grp = tid / E2; // (E2 <= 50: at least five groups)
    const int u0 = p * upb, u1 = (u0 + upb < U) ? u0 + upb : U;
    for (int u = u0; u < u1; u++) {
        const long long o = off[u];
        const int T = (int)(off[u + 1] - o), q = T / N, r = T % N;
        const int rb = k * q + (k < r ? k : r), re = rb + q + (k < r ? 1 : 0);
        for (int s = rb; s < re; s += FI_FRAMES) {
            const int nf = (re - s < FI_FRAMES) ? re - s : FI_FRAMES;
            const double *src = X + (o + s) * D;
            __syncthreads(); // (the last stage's readers, or the fills above)
            for (int e = tid; e < nf * D; e += FI_THREADS) {
                const int fr = e / D;
                xs[fr * DS + (e - fr * D)] = src[e];
            }
            __syncthreads();
            if (classify) {
                if (lane < nf) {
                    const double *x = xs + lane * DS;
                    double best = FI_FAR;
                    int cell = -1;
                    for (int c = w; c < n_cells; c += NW) {
                        const double *mu = cl + c * DS;
                        double dist = 0.0;
                        for (int d = 0; d < D; d++) {
                            const double a = mu[d] - x[d];
                            dist += a * a;
                        }
                        if (dist < best) {
                            best = dist;
                            cell = c;
                        }
                    }
                    cand_d[w][lane] = best;
                    cand_c[w][lane] = cell;
                }
                __syncthreads();
                if (tid < nf) {
                    double best = FI_FAR;
                    int cell = -1;
                    for (int v = 0; v < NW; v++) {
                        const double d = cand_d[v][tid];
                        const int c = cand_c[v][tid];
                        if (c >= 0 && (cell < 0 || d < best || (d == best && c < cell))) {
                            best = d;
                            cell = c;
                        }
                    }
                    if (cell < 0) cell = 0;
                    dmin[tid] = best;
                    cid[tid] = cell;
                    cgr[tid] = cell % ngrp;
                }
            } else if (tid < nf) { // the state's mean: one cell, nothing to compare (TFF:1005-1030)
                dmin[tid] = 0.0;
                cid[tid] = 0;
                cgr[tid] = 0;
            }
            __syncthreads();
            if (gamma) { // the last pass: the frames' one-hot rows, each written whole by the block that owns the frame
                const int G = N * M;
                for (int e = tid; e < nf * N; e += FI_THREADS) {
                    const int fr = e / N;
                    gamma[(o + s) * N + e] = (e - fr * N) == k ? 1.0 : 0.0;
                }
                for (int e = tid; e < nf * G; e += FI_THREADS) {
                    const int fr = e / G;
                    post[(o + s) * G + e] = (e - fr * G) == k * M + cid[fr] ? 1.0 : 0.0;
                }
            }
            if (grp < ngrp)
                for (int fr = 0; fr < nf; fr++)
                    if (cgr[fr] == grp) {
                        const double v = l < D ? xs[fr * DS + l] : (l == D ? 1.0 : dmin[fr]);
                        acc[cid[fr] * E2 + l] += v;
                    }
        }
    }
    __syncthreads();
    double *out = part + ((size_t)p * N + k) * M * E2;
    for (int e = tid; e < n_cells * E2; e += FI_THREADS) out[e] = acc[e];
}

// the blocks' partials [P][N][M][E2] in block order into one slice [N][M][E2] (a corpus sharded over
// ranks: this slice is what is all-reduced; k_finit_cells then reads it as P = 1)
__global__ void __launch_bounds__(256)
k_finit_reduce(long long n, int P, const double *__restrict__ part, double *__restrict__ sums)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double v = 0.0;
    for (int p = 0; p < P; p++) v += part[(size_t)p * n + e];
    sums[e] = v;
}

// The cell bookkeeping between two passes (csrc/ghmm_init.c ghmm_init_cells_, TFF:1043-1270): the host
// loop's operations in the host loop's order, as k_init_cells has them for the diagonal layout — block =
// state, thread = coefficient (every thread walks the same order of cells and only ever touches its own
// coefficients).  (up1, down1) is the doubling split, (up2, down2) the split of the cells of largest
// distortion and the re-seeding of empty cells.  M <= FI_MAXM.
__global__ void __launch_bounds__(64)
k_finit_cells(int N, int M, int D, int n_cells, int do_split, int first, int P, const double *__restrict__ part,
              double up1, double down1, double up2, double down2, double *__restrict__ cells)
{
#pragma clang fp contract(off)
    extern __shared__ double fi_st[]; // [n_cells][E2]
    __shared__ double dist[FI_MAXM];
    __shared__ int idx[FI_MAXM];
    const int k = blockIdx.x, tid = threadIdx.x, E2 = D + 2;
    const size_t slice = (size_t)N * M * E2;
    for (int e = tid; e < n_cells * E2; e += 64) {
        double v = 0.0;
        for (int p = 0; p < P; p++) v += part[(size_t)p * slice + (size_t)k * M * E2 + e];
        fi_st[e] = v;
    }
    __syncthreads();
    for (int j = tid; j < n_cells; j += 64) dist[j] = fi_st[j * E2 + D + 1];
    __syncthreads();
    double *ck = cells + (size_t)k * M * D;
    // indices by decreasing key, adjacent-swap passes with strict '<' (TFF:1289-1315)
    auto order_desc = [&](int n) {
        if (tid == 0) {
            for (int i = 0; i < n; i++) idx[i] = i;
            bool done = false;
            while (!done) {
                done = true;
                for (int i = 0; i < n - 1; i++)
                    if (dist[idx[i]] < dist[idx[i + 1]]) {
                        const int t = idx[i];
                        idx[i] = idx[i + 1];
                        idx[i + 1] = t;
                        done = false;
                    }
            }
        }
        __syncthreads();
    };
    auto split_cell = [&](int from, int to, double up, double down) {
        for (int l = tid; l < D; l += 64) {
            const double v = ck[(size_t)from * D + l], hi = v * up;
            ck[(size_t)to * D + l] = hi;
            ck[(size_t)from * D + l] = (from == to ? hi : v) * down; // (a cell re-seeded from itself)
        }
    };
    for (int j = 0; j < n_cells; j++)
        for (int l = tid; l < D; l += 64) ck[(size_t)j * D + l] = fi_st[j * E2 + l] / fi_st[j * E2 + D];
    if (!first) { // empty cells are re-seeded from the cells of largest distortion
        order_desc(n_cells);
        int i = 0;
        for (int j = 0; j < n_cells; j++)
            if (fi_st[j * E2 + D] == 0.0) split_cell(idx[i++], j, up2, down2);
    }
    if (do_split) {
        if (2 * n_cells < M) {
            for (int i = 0; i < n_cells; i++) split_cell(i, n_cells + i, up1, down1);
        } else {
            order_desc(n_cells);
            for (int i = 0; i < M - n_cells; i++) split_cell(idx[i], n_cells + i, up2, down2);
        }
    }
}

__global__ void __launch_bounds__(FM_THREADS)
k_finit_gauss(int N, int M, int D, const double *__restrict__ stats, double *__restrict__ mean,
              double *__restrict__ inv_cov, double *__restrict__ det)
{
    extern __shared__ double fm_lds[];
    fm_gauss_body<true>(N, M, D, stats, mean, inv_cov, det, fm_lds);
}

__global__ void __launch_bounds__(FM_THREADS)
k_finit_state(int N, int M, int D, const double *__restrict__ stats, double norm2pi, int delta,
              double *__restrict__ A, double *__restrict__ c, double *mean, double *inv_cov,
              double *__restrict__ det, double *__restrict__ den, double *__restrict__ lk,
              double *__restrict__ logA)
{
    fm_state_body<true>(N, M, D, stats, norm2pi, delta, A, c, mean, inv_cov, det, den, lk, logA);
}

} // namespace ghmm
