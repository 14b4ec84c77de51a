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
#pragma once
#include <hip/hip_runtime.h>

namespace ghmm {

constexpr int FC_WAVES = 4;   // waves per block (one frame tile)
constexpr int FC_SC = 8;      // states per wave
constexpr int FC_DMAX = 48;   // widest feature vector built
constexpr int FC_SLACK = 64;  // doubles allocated behind mean[] and inv_cov[] (the padded columns' reads)

// doubles of LDS a block needs: the frame tile and every wave's density tile
__host__ __device__ inline int fc_lds_doubles(int D) { return WAVE * (D | 1) + FC_WAVES * WAVE * (FC_SC | 1); }

template <int DB>
__global__ void __launch_bounds__(FC_WAVES * WAVE)
k_emission_full(int NS, int M, int D, long long F, const double *__restrict__ X,
                const double *__restrict__ mean, const double *__restrict__ inv_cov,
                const double *__restrict__ den, const double *__restrict__ c, double *__restrict__ b)
{
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
            const double gaus = exp(aux * -0.5) / den[g];
            bi += gaus * c[g];
        }
        bt[lane * SS + s] = bi;
    }
    __syncthreads();
    for (int k = lane; k < nf * ns; k += WAVE) {
        const int r = k / ns, col = k - r * ns;
        b[(f0 + r) * NS + s0 + col] = bt[r * SS + col];
    }
}

// ghmm_score_full_batch: word k's Gaussians (ng of them from g0) copied into the concatenated model
struct fgather_src {
    const double *c, *mean, *inv_cov, *den;
    int g0, ng;
};
__global__ void __launch_bounds__(256)
k_gather_fmodels(int D, const fgather_src *__restrict__ src, double *__restrict__ c, double *__restrict__ mean,
                 double *__restrict__ inv_cov, double *__restrict__ den)
{
    const fgather_src s = src[blockIdx.x];
    for (int k = threadIdx.x; k < s.ng; k += 256) {
        c[s.g0 + k] = s.c[k];
        den[s.g0 + k] = s.den[k];
    }
    const size_t n = (size_t)s.ng * D, o = (size_t)s.g0 * D;
    for (size_t k = threadIdx.x; k < n; k += 256) mean[o + k] = s.mean[k];
    const size_t n2 = n * D, o2 = o * D;
    for (size_t k = threadIdx.x; k < n2; k += 256) inv_cov[o2 + k] = s.inv_cov[k];
}

} // namespace ghmm
