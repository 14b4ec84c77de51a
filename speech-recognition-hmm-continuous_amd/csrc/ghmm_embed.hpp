// ghmm_embed.hpp — embedded Baum-Welch on word transcripts (ghmm_estep_embed_streams; definition in
// include/ghmm.h): a log-domain forward-backward over the states of the transcript's word instances, on
// the log b[F][NS] that the vocabulary's emission launches left in the workspace, with gamma and xi tied
// over the instances of a word.  The composite states, their columns and the entry from instance i - 1
// into instance i are k_align's; inside an instance the steps are k_logfb_fwd's and k_logfb_bwd's (the
// banded two-term form hi + log1p(exp(lo - hi)), the dense m + log(sum exp) with its NaN rule, chosen per
// WORD as k_logfb chooses it per model), so that a one-word transcript gives ghmm_estep_log's bits.
//
// Two launches (k_logfb was split in two for its registers; here the backward pass alone holds up to
// 8 x 11 running sums per thread).  One workgroup per utterance (longest first, order[]), of 1 to 4 waves
// sized by the launch's largest S_u; a block loops over its own S_u composite states, s = tid, tid +
// blockDim.x, ...  Both build k_align's state table from the transcript (embed_table).
//
// k_embed_fwd: LDS per composite state as in k_align (40 bytes).  Stores every la row, S_u doubles per
// frame from the utterance's own offset (poff[u], in doubles: the sum of T * S over the utterances
// before it), then log P_u = la_{T-1}(S - 1) and, by wave 0 with k_logfb_fwd's cross-lane sum, log Z_u
// over the last instance's states.  One barrier per frame; a thread loads the NEXT frame's log b of its
// states ahead of the step, so that the load is in flight across the barrier (k_embed_fwd<PASSES>: states
// per thread, as below).
//
// k_embed_bwd<PASSES>: LDS per composite state: two rows of w_t(s) = log b_s(t + 1) + lbe_{t+1}(s), two
// rows of the frame's composite gammas, log a_jj, log a_{j,j+1}, the facts, the column, and the link to
// the same state of the NEXT instance of the same word (60 bytes, 120 KB at the cap).  A thread forms
// lbe_t, gamma_t, stay_t and the band's xi_t of its states from w_t, leaves w_{t-1} and gamma_t in the
// other rows, and after the frame's ONE barrier the block writes the tied gamma row: column c takes the
// sum over the chain of instances that starts at the first instance of c's word (chead[c], a per-block
// table in global memory: the vocabulary's columns are not bounded by the lattice's cap), 0 where the
// transcript lacks the word.  A thread's la and log b of the NEXT step are loaded a frame ahead, as in the
// forward launch.  The running sums (xi[0..delta], stay, gamma) stay in registers over t
// (PASSES states per thread, compile-time indices) and are tied the same way at the end into one
// partial per utterance, in the layout k_reduce_all reads for a model of NS states.
#pragma once
#include "ghmm_align.hpp"

namespace ghmm {

constexpr int EMBED_THREADS = CONNECT_THREADS;

// LDS of k_embed_fwd for S composite states: d[2][S] | la_self[S] | la_prev[S] | meta[S] | col[S]
constexpr size_t embed_fwd_lds(int S) { return (size_t)S * 40; }
// ... of k_embed_bwd: w[2][S] | g[2][S] | la_self[S] | la_next[S] | meta[S] | col[S] | nxt[S]
constexpr size_t embed_bwd_lds(int S) { return (size_t)S * 60; }

// facts of composite state s, packed: instance within the transcript (12 bits), state within the word
// (6 bits), the word's log A has entries off the band (k_logfb's test), first state of an instance behind
// the first (takes the entry), last state of an instance before the last (takes the exit), instance is
// the first of its word in the transcript (owns the word's tied sums)
constexpr int EM_J_SHIFT = 12, EM_DENSE = 1 << 18, EM_FIRST = 1 << 19, EM_LAST = 1 << 20, EM_HEAD = 1 << 21;

// where the scatter puts word k of one stream: its vector, its states, its first column
struct embed_dst {
    double *v;
    int N, bo;
};

// the two-term LSE of the banded step: hi + log1p(exp(lo - hi)); lo == -inf gives hi
__device__ __forceinline__ double embed_lse2(double c0, double c1)
{
    const bool up = c0 < c1;
    const double hi = up ? c1 : c0, lo = up ? c0 : c1;
    const double x = lo == -INFINITY ? -INFINITY : lo - hi; // (not -inf - -inf; a NaN lo stays)
    return hi + log1p(exp_emis(x));
}

// k_align's state table from the transcript sq[L]: the instances' state counts and their inclusive scan
// in `room` (2 * L ints, which the caller writes only behind the closing barrier), then per instance its
// states' facts and columns and, with nxt, the links.  Returns S_u.  Ends on a barrier.
__device__ __forceinline__ int embed_table(const fwd_model *__restrict__ tab, const int *__restrict__ sq, int L,
                                           int *room, int *meta, int *col, int *nxt)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    int *sa = room, *sb = sa + L;
    for (int i = tid; i < L; i += nt) sa[i] = tab[sq[i]].N;
    __syncthreads();
    for (int o = 1; o < L; o <<= 1) {
        for (int i = tid; i < L; i += nt) sb[i] = sa[i] + (i >= o ? sa[i - o] : 0);
        __syncthreads();
        int *sw = sa;
        sa = sb;
        sb = sw;
    }
    const int S = sa[L - 1];
    for (int i = tid; i < L; i += nt) {
        const int k = sq[i];
        const fwd_model mk = tab[k];
        const int N = mk.N, s0 = sa[i] - N;
        bool dense = false;
        for (int r = 0; r < N; r++)
            for (int c = 0; c < N; c++) dense |= mk.A[r * N + c] != -INFINITY && c != r && c != r + 1;
        int ns0 = -1;
        bool head = true;
        if (nxt) {
            for (int i2 = i + 1; i2 < L; i2++)
                if (sq[i2] == k) {
                    ns0 = sa[i2] - N;
                    break;
                }
            for (int i0 = i - 1; i0 >= 0 && head; i0--) head = sq[i0] != k;
        }
        for (int j = 0; j < N; j++) {
            meta[s0 + j] = i | (j << EM_J_SHIFT) | (dense ? EM_DENSE : 0) | (j == 0 && i > 0 ? EM_FIRST : 0) |
                           (j == N - 1 && i < L - 1 ? EM_LAST : 0) | (head ? EM_HEAD : 0);
            col[s0 + j] = mk.bo + j;
            if (nxt) nxt[s0 + j] = ns0 >= 0 ? ns0 + j : -1;
        }
    }
    __syncthreads(); // (the scan is read no more: its room may be written)
    return S;
}

// poff, seq_off and seq: the call's tables in the context, as for k_align (poff in doubles here).  PASSES:
// composite states per thread (the launch's largest S_u over the threads, rounded up to 1, 2, 4 or 8), so
// that a thread keeps its states' columns and the NEXT frame's log b in registers: the loads are in flight
// across the frame's barrier.
template <int PASSES>
__global__ void __launch_bounds__(EMBED_THREADS)
k_embed_fwd(int U, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
            const long long *__restrict__ off, const long long *__restrict__ poff, const int *__restrict__ seq_off,
            const int *__restrict__ seq, double *__restrict__ la, double *__restrict__ loglik,
            double *__restrict__ logz, const int *__restrict__ order, int Smax)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int u = order[blockIdx.x];
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    if (T <= 0) {
        if (tid == 0) {
            loglik[u] = 0.0;
            logz[u] = 0.0;
        }
        return;
    }
    const int *sq = seq + seq_off[u];
    const int L = seq_off[u + 1] - seq_off[u]; // >= 1 (the host refuses an empty transcript with T > 0)
    double *d = lds, *la_self = lds + 2 * (size_t)Smax, *la_prev = lds + 3 * (size_t)Smax;
    int *meta = (int *)(lds + 4 * (size_t)Smax), *col = meta + Smax;
    const int S = embed_table(tab, sq, L, (int *)d, meta, col, nullptr);
    const double *lb = logb + f0 * NS;
    double *lu = la + poff[u];
    int cs[PASSES];
    double qn[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        const int s = tid + p * nt;
        cs[p] = 0;
        qn[p] = 0.0;
        if (s < S) {
            const int mt = meta[s];
            const int j = (mt >> EM_J_SHIFT) & 63;
            const fwd_model mk = tab[sq[mt & ((1 << EM_J_SHIFT) - 1)]];
            la_self[s] = mk.A[j * mk.N + j];
            la_prev[s] = j > 0 ? mk.A[(j - 1) * mk.N + j] : -INFINITY;
            cs[p] = col[s];
            const double v = (s == 0 ? 0.0 : -INFINITY) + lb[cs[p]];
            d[s] = v;
            lu[s] = v;
            qn[p] = lb[(size_t)(T > 1 ? 1 : 0) * NS + cs[p]];
        }
    }
    __syncthreads();

    for (int t = 1; t < T; t++) {
        const double *prev = d + (size_t)((t + 1) & 1) * Smax;
        double *cur = d + (size_t)(t & 1) * Smax;
        const size_t tn = (size_t)(t + 1 < T ? t + 1 : t); // the frame prefetched (clamped into the utterance)
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            if (s >= S) continue;
            const double q = qn[p];
            qn[p] = lb[tn * NS + cs[p]];
            const int mt = meta[s];
            const int j = (mt >> EM_J_SHIFT) & 63;
            double r;
            if (!(mt & EM_DENSE)) {
                const double lp = la_prev[s], ls = la_self[s];
                const double c1 = lp != -INFINITY ? prev[s - 1] + lp : -INFINITY; // (j > 0 where lp is a term)
                const double c0 = ls != -INFINITY ? prev[s] + ls : -INFINITY;
                r = embed_lse2(c0, c1);
            } else {
                const fwd_model mk = tab[sq[mt & ((1 << EM_J_SHIFT) - 1)]];
                const double *pw = prev + (s - j);
                double m = -INFINITY;
                for (int i = 0; i < mk.N; i++) {
                    const double a = mk.A[i * mk.N + j];
                    const double v = a != -INFINITY ? pw[i] + a : -INFINITY;
                    m = fmax(m, v); // (a NaN term is passed over here and taken by the sum)
                }
                const double mm = m == -INFINITY ? 0.0 : m;
                double sum = 0.0;
                for (int i = 0; i < mk.N; i++) {
                    const double a = mk.A[i * mk.N + j];
                    const double v = a != -INFINITY ? pw[i] + a : -INFINITY;
                    sum += exp_emis(v - mm);
                }
                r = m + log(sum);
            }
            if (mt & EM_FIRST) r = embed_lse2(r, prev[s - 1]); // the entry, with weight 0
            const double v = r + q;
            cur[s] = v;
            lu[(size_t)t * S + s] = v;
        }
        __syncthreads();
    }
    // log P_u and, by wave 0 alone, log Z_u over the last instance's states: k_logfb_fwd's cross-lane LSE
    // with the group_sum of the lanes that word takes on its own
    if (tid >= WAVE) return;
    const double *row = d + (size_t)((T - 1) & 1) * Smax;
    const int Nl = tab[sq[L - 1]].N;
    const double dd = tid < Nl ? row[S - Nl + tid] : -INFINITY;
    double m = dd; // (fmax passes over a NaN, the sum takes it)
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, WAVE));
    m = fmax(m, -INFINITY);
    const double mm = m == -INFINITY ? 0.0 : m;
    const double e = exp_emis(dd - mm);
    const double sum = Nl <= 16 ? group_sum<16>(e) : Nl <= 32 ? group_sum<32>(e) : group_sum<64>(e);
    if (tid == 0) {
        loglik[u] = row[S - 1];
        logz[u] = m + log(sum);
    }
}

// chead: NS ints per block; part_*: one partial per utterance (slot = u of U), NS states
template <int PASSES>
__global__ void __launch_bounds__(EMBED_THREADS)
k_embed_bwd(int U, int NS, int delta, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
            const long long *__restrict__ off, const long long *__restrict__ poff, const int *__restrict__ seq_off,
            const int *__restrict__ seq, const double *__restrict__ la, const double *__restrict__ logz,
            double *__restrict__ gamma, double *__restrict__ part_xi, double *__restrict__ part_dena,
            double *__restrict__ part_denc, int *chead_all, const int *__restrict__ order, int Smax)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int u = order[blockIdx.x];
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    if (T <= 0) {
        for (int c = tid; c < NS; c += nt) {
            for (int o = 0; o <= delta; o++) part_xi[pxi_at(u, c, o, U)] = 0.0;
            part_dena[pden_at(u, c, U)] = 0.0;
            part_denc[pden_at(u, c, U)] = 0.0;
        }
        return;
    }
    const int *sq = seq + seq_off[u];
    const int L = seq_off[u + 1] - seq_off[u];
    double *w = lds, *g = lds + 2 * (size_t)Smax, *la_self = lds + 4 * (size_t)Smax, *la_next = lds + 5 * (size_t)Smax;
    int *meta = (int *)(lds + 6 * (size_t)Smax), *col = meta + Smax, *nxt = col + Smax;
    int *chead = chead_all + (size_t)blockIdx.x * NS;
    for (int c = tid; c < NS; c += nt) chead[c] = -1;
    const int S = embed_table(tab, sq, L, (int *)w, meta, col, nxt); // (its barriers order the -1s ahead of the heads)
    const double *lb = logb + f0 * NS;
    const double *lu = la + poff[u];
    const double logZ = logz[u];
    const bool zok = fabs(logZ) < INFINITY; // (false for a NaN)

    double xi[PASSES][MAX_DELTA + 1], gs[PASSES], gl[PASSES], st[PASSES];
    // a state's column, and the NEXT step's la and log b, loaded a frame ahead (in flight across the barrier)
    int cs[PASSES];
    double an[PASSES], bn[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        gs[p] = gl[p] = st[p] = 0.0;
        cs[p] = 0;
        an[p] = bn[p] = 0.0;
#pragma unroll
        for (int o = 0; o <= MAX_DELTA; o++) xi[p][o] = 0.0;
    }
    // frame T-1: lbe = 0 in the last state of the last instance; gamma_{T-1}; w_{T-2}
    {
        double *wn = w + (size_t)((T - 2) & 1) * Smax, *gt = g + (size_t)((T - 1) & 1) * Smax;
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            if (s < S) {
                const int mt = meta[s];
                const int j = (mt >> EM_J_SHIFT) & 63;
                const fwd_model mk = tab[sq[mt & ((1 << EM_J_SHIFT) - 1)]];
                la_self[s] = mk.A[j * mk.N + j];
                la_next[s] = j + 1 < mk.N ? mk.A[j * mk.N + j + 1] : -INFINITY;
                if (mt & EM_HEAD) chead[col[s]] = s;
                cs[p] = col[s];
                const double be = s == S - 1 ? 0.0 : -INFINITY;
                const double al = lu[(size_t)(T - 1) * S + s];
                const double gv = zok ? exp_emis((al + be) - logZ) : 0.0;
                gl[p] = gv; // gamma_{T-1}: in den_c (t < T) but not in den_a (t < T-1)
                gt[s] = gv;
                if (T > 1) {
                    wn[s] = be + lb[(size_t)(T - 1) * NS + cs[p]];
                    an[p] = lu[(size_t)(T - 2) * S + s];
                    bn[p] = lb[(size_t)(T - 2) * NS + cs[p]];
                }
            }
        }
    }
    __syncthreads();
    // the tied gamma row of frame t from the composite row gt: every column of the vocabulary (the heads of a
    // thread's first four columns stay in registers; a vocabulary wider than that reads the table)
    constexpr int HC = 4;
    int hd[HC];
#pragma unroll
    for (int q = 0; q < HC; q++) hd[q] = tid + q * nt < NS ? chead[tid + q * nt] : -1;
    auto tie_gamma = [&](int t, const double *gt) {
        double *go = gamma + (size_t)(f0 + t) * NS;
#pragma unroll
        for (int q = 0; q < HC; q++)
            if (tid + q * nt < NS) {
                double v = 0.0;
                for (int s = hd[q]; s >= 0; s = nxt[s]) v += gt[s];
                go[tid + q * nt] = v;
            }
        for (int c = tid + HC * nt; c < NS; c += nt) {
            double v = 0.0;
            for (int s = chead[c]; s >= 0; s = nxt[s]) v += gt[s];
            go[c] = v;
        }
    };
    tie_gamma(T - 1, g + (size_t)((T - 1) & 1) * Smax);

    for (int t = T - 2; t >= 0; t--) {
        const double *wt = w + (size_t)(t & 1) * Smax;
        double *wn = w + (size_t)((t + 1) & 1) * Smax, *gt = g + (size_t)(t & 1) * Smax;
        const size_t tp = (size_t)(t > 0 ? t - 1 : 0); // the frame prefetched (clamped into the utterance)
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            if (s < S) {
                const int mt = meta[s];
                const int j = (mt >> EM_J_SHIFT) & 63;
                const double al = an[p], lbt = bn[p]; // la_t(s), log b_s(t)
                an[p] = lu[tp * S + s];
                bn[p] = lb[tp * NS + cs[p]];
                const double ls = la_self[s], ln = la_next[s], ws = wt[s];
                double wi;
                if (!(mt & EM_DENSE)) {
                    const double c0 = ls != -INFINITY ? ls + ws : -INFINITY;
                    const double c1 = ln != -INFINITY ? ln + wt[s + 1] : -INFINITY; // (j + 1 < N where ln is a term)
                    wi = embed_lse2(c0, c1);
                } else {
                    const fwd_model mk = tab[sq[mt & ((1 << EM_J_SHIFT) - 1)]];
                    const double *pw = wt + (s - j), *ar = mk.A + j * mk.N;
                    double m = -INFINITY;
                    for (int i = 0; i < mk.N; i++) {
                        const double a = ar[i];
                        const double v = a != -INFINITY ? a + pw[i] : -INFINITY;
                        m = fmax(m, v); // (a NaN term is passed over here and taken by the sum)
                    }
                    const double mm = m == -INFINITY ? 0.0 : m;
                    double sum = 0.0;
                    for (int i = 0; i < mk.N; i++) {
                        const double a = ar[i];
                        const double v = a != -INFINITY ? a + pw[i] : -INFINITY;
                        sum += exp_emis(v - mm);
                    }
                    wi = m + log(sum);
                }
                // the band's xi: a transition with a_{j,j+o} == 0 (or outside the word / the band) is not a term
                if (zok) {
                    if (ls != -INFINITY) xi[p][0] += exp_emis(((al + ls) + ws) - logZ);
                    if (delta >= 1 && ln != -INFINITY) xi[p][1] += exp_emis(((al + ln) + wt[s + 1]) - logZ);
                    if (delta >= 2) {
                        const fwd_model mk = tab[sq[mt & ((1 << EM_J_SHIFT) - 1)]];
#pragma unroll
                        for (int o = 2; o <= MAX_DELTA; o++)
                            if (o <= delta && j + o < mk.N) {
                                const double a = mk.A[j * mk.N + j + o];
                                if (a != -INFINITY) xi[p][o] += exp_emis(((al + a) + wt[s + o]) - logZ);
                            }
                    }
                }
                const double be = (mt & EM_LAST) ? embed_lse2(wi, wt[s + 1]) : wi; // the exit into the next instance
                const double gv = zok ? exp_emis((al + be) - logZ) : 0.0;
                gs[p] += gv;
                st[p] += zok ? exp_emis((al + wi) - logZ) : 0.0;
                gt[s] = gv;
                if (t > 0) wn[s] = be + lbt;
            }
        }
        __syncthreads();
        tie_gamma(t, gt);
    }
    __syncthreads(); // (the last tied row has been read: g is free for the sums)

    // the running sums, tied like gamma: one round per kind through g's first row
    auto tie_out = [&](double *dst, int o) { // o < 0: a den, else xi[o]
        for (int c = tid; c < NS; c += nt) {
            double v = 0.0;
            for (int s = chead[c]; s >= 0; s = nxt[s]) v += g[s];
            dst[o < 0 ? pden_at(u, c, U) : pxi_at(u, c, o, U)] = v;
        }
        __syncthreads();
    };
#pragma unroll
    for (int o = 0; o <= MAX_DELTA; o++)
        if (o <= delta) {
#pragma unroll
            for (int p = 0; p < PASSES; p++)
                if (tid + p * nt < S) g[tid + p * nt] = xi[p][o];
            __syncthreads();
            tie_out(part_xi, o);
        }
#pragma unroll
    for (int p = 0; p < PASSES; p++)
        if (tid + p * nt < S) g[tid + p * nt] = st[p];
    __syncthreads();
    tie_out(part_dena, -1);
#pragma unroll
    for (int p = 0; p < PASSES; p++)
        if (tid + p * nt < S) g[tid + p * nt] = gs[p] + gl[p];
    __syncthreads();
    tie_out(part_denc, -1);
}

// One block per word: word k's diagonal blocks of the concatenated model's vector `cat` (NS states, M
// mixtures, D coefficients) into its own vector, with the common loglik and n_utt.
__global__ void __launch_bounds__(256)
k_embed_scatter(int NS, int M, int D, const double *__restrict__ cat, const embed_dst *__restrict__ dst)
{
    const embed_dst e = dst[blockIdx.x];
    const int N = e.N, bo = e.bo, tid = threadIdx.x, nt = blockDim.x;
    const size_t GS = (size_t)NS * M, G = (size_t)N * M;
    const double *s_na = cat, *s_da = s_na + (size_t)NS * NS, *s_dc = s_da + NS, *s_nc = s_dc + NS;
    const double *s_mu = s_nc + GS, *s_var = s_mu + GS * D, *s_tail = s_var + GS * D;
    double *d_na = e.v, *d_da = d_na + (size_t)N * N, *d_dc = d_da + N, *d_nc = d_dc + N;
    double *d_mu = d_nc + G, *d_var = d_mu + G * D, *d_tail = d_var + G * D;
    for (int q = tid; q < N * N; q += nt) d_na[q] = s_na[(size_t)(bo + q / N) * NS + bo + q % N];
    for (int q = tid; q < N; q += nt) {
        d_da[q] = s_da[bo + q];
        d_dc[q] = s_dc[bo + q];
    }
    for (size_t q = tid; q < G; q += nt) d_nc[q] = s_nc[(size_t)bo * M + q];
    for (size_t q = tid; q < G * D; q += nt) {
        d_mu[q] = s_mu[(size_t)bo * M * D + q];
        d_var[q] = s_var[(size_t)bo * M * D + q];
    }
    if (tid < 2) d_tail[tid] = s_tail[tid];
}

// The same for the full-covariance layout (num_cov: the upper triangle, D (D + 1) / 2 per Gaussian), over a
// grid of (word, chunk): word k's Gaussians are contiguous in the concatenated num_c, num_mu and num_cov, so
// each of the three is one range, and the chunks of a word share every range between them (a 64-state word's
// num_cov is tens of thousands of doubles: not one block's loop).  Plain loads and stores, every element
// written by exactly one thread.
constexpr int EMBED_SCATTER_PER_BLOCK = 1024; // doubles a chunk moves at the largest word (the host's grid)
__global__ void __launch_bounds__(256)
k_embed_scatter_full(int NS, int M, int D, const double *__restrict__ cat, const embed_dst *__restrict__ dst)
{
    const embed_dst e = dst[blockIdx.x];
    const int N = e.N, bo = e.bo;
    const size_t q0 = (size_t)blockIdx.y * blockDim.x + threadIdx.x, step = (size_t)gridDim.y * blockDim.x;
    const size_t DT = (size_t)D * (D + 1) / 2, GS = (size_t)NS * M, G = (size_t)N * M, g0 = (size_t)bo * M;
    const double *s_na = cat, *s_da = s_na + (size_t)NS * NS, *s_dc = s_da + NS, *s_nc = s_dc + NS;
    const double *s_mu = s_nc + GS, *s_cov = s_mu + GS * D, *s_tail = s_cov + GS * DT;
    double *d_na = e.v, *d_da = d_na + (size_t)N * N, *d_dc = d_da + N, *d_nc = d_dc + N;
    double *d_mu = d_nc + G, *d_cov = d_mu + G * D, *d_tail = d_cov + G * DT;
    for (size_t q = q0; q < (size_t)N * N; q += step) d_na[q] = s_na[(bo + q / N) * NS + bo + q % N];
    for (size_t q = q0; q < (size_t)N; q += step) {
        d_da[q] = s_da[bo + q];
        d_dc[q] = s_dc[bo + q];
    }
    for (size_t q = q0; q < G; q += step) d_nc[q] = s_nc[g0 + q];
    for (size_t q = q0; q < G * D; q += step) d_mu[q] = s_mu[g0 * D + q];
    for (size_t q = q0; q < G * DT; q += step) d_cov[q] = s_cov[g0 * DT + q];
    if (q0 < 2) d_tail[q0] = s_tail[q0];
}

} // namespace ghmm
