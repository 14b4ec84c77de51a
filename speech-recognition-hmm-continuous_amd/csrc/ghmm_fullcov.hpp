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
template <int DB, int MODE = FC_LIN>
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
        b[(f0 + r) * NS + s0 + col] = bt[r * SS + col];
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

} // namespace ghmm
