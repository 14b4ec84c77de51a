// ghmm_grammar.hpp — connected-word Viterbi decoding under a word-pair grammar
// (ghmm_connect_grammar_streams and ghmm_connect_grammar_full_streams; definition in include/ghmm.h):
// k_connect's lattice (ghmm_connect.hpp) with K entry values per frame instead of one.  Word k's first
// state may be entered at frame t from the end of ANY word w of frame t-1 at the price pair[w][k]; the
// best such w is kept per (frame, word) for the trace.  start[] scores the word that opens the utterance,
// fin[] is added to the word ends before the final pick.
//
// The scheme is k_connect's: one workgroup per utterance (longest first, order[]), of 1 to 4 waves; the
// composite states s = tid, tid + blockDim.x, ... of a thread are the same in every frame; d[2][NS] and
// every state's log a_jj and log a_{j-1,j} live in LDS; byte back-pointers in rows of NS; the trace by one
// lane in the same launch.
//
// What differs:
//   The word ends sit in a compact LDS row e[2][K], double-buffered by frame parity: the owner of word
//   k's last state stores d_t there as it stores d_t, ahead of the frame's barrier.  No butterfly and no
//   wave partials: nobody needs the best end of a frame, only the K ends.
//   x_t(k) = max_w (e_{t-1}(w) + pair[w][k]) is a pass of its own ahead of the step, spread over ALL
//   lanes: item i = r * K + k (i = tid, tid + blockDim.x, ...) takes word k and the candidates w = r, r + R,
//   r + 2R, ... in ascending order under a strict >, R = blockDim.x / K clamped to 1..4 slices per word, and
//   leaves its (value, word) in LDS; behind a barrier the owner of word k's first state combines the R
//   partials under the order of include/ghmm.h (greater wins; equal: the lower w; a NaN candidate never
//   wins; all -inf gives word 0; every partial starts at (-inf, 0), which is the definition's start).  TWO
//   barriers per frame, one more than k_connect: with the loop inside the step instead, the lanes that own
//   no first state idle through it, a wave runs it once per pass over its states, and lanes on first states
//   two or three doubles apart waste most of every load.  Lanes on consecutive k read consecutive
//   doubles of row w of the table as the caller passed it (pair[w * K + k]): no transpose.  The table is
//   staged in LDS while the launch stays within GRAMMAR_STAGE_LDS (K <= about 80 beside a small
//   vocabulary); beyond it the lanes read it from L2 (K * K * 8 bytes, 512 KB at the cap, shared by every
//   workgroup), 16 loads in flight each.
//   entw[F][K], a byte per (frame, word): the winning w, written only where the entry won, read by the
//   trace only there.
//   (The loop inside the step, by the first state's owner, with ONE barrier per frame, was built first and
//   measured: 1.1, 1.4 and 2.8 times this form's time at K = 13, 64 and 256; DESIGN.md has the table.)
//   The final pick is ghmm_recognise_streams' rule on d_{T-1}(k, N_k - 1) + fin[k], by the tracing lane.
//
// Back-pointers, path[] and the band shortcut are k_connect's (CONNECT_ENTRY, CONNECT_BEGIN).  word[] is
// written by the trace alone.
#pragma once
#include "ghmm_connect.hpp"

namespace ghmm {

constexpr int GRAMMAR_MAX_K = 256;               // words: the dense K x K table, a predecessor word in a byte
constexpr size_t GRAMMAR_STAGE_LDS = 64u << 10;  // the pair table is staged while the launch's LDS stays within this

constexpr int GRAMMAR_ITEMS = 256;               // K * R <= max(K, blockDim.x): the entry pass's partials
// LDS of k_grammar without the staged table:
// d[2][NS] | la_self[NS] | la_prev[NS] | e[2][K] | px[GRAMMAR_ITEMS] | (table) | meta[NS] | pxw[GRAMMAR_ITEMS]
constexpr size_t grammar_lds_base(int NS, int K) { return (size_t)NS * 36 + (size_t)K * 16 + GRAMMAR_ITEMS * 12; }
constexpr bool grammar_staged(int NS, int K)
{
    return grammar_lds_base(NS, K) + (size_t)K * K * 8 <= GRAMMAR_STAGE_LDS;
}
constexpr size_t grammar_lds(int NS, int K)
{
    return grammar_lds_base(NS, K) + (grammar_staged(NS, K) ? (size_t)K * K * 8 : 0);
}

// slice r of R of x(k): the best candidate and its word over the ends ep[w], w = r, r + R, ..., and column k
// of the table (col = table + k, rows K apart).  The loads of UNROLL candidates are independent and go
// out together; the compares stay in ascending w.
template <int UNROLL>
__device__ __forceinline__ void grammar_entry(const double *ep, const double *col, int K, int r, int R, double &xb,
                                              int &xw)
{
    xb = -INFINITY;
    xw = 0;
    int w = r;
    for (; w + (UNROLL - 1) * R < K; w += UNROLL * R) {
        double c[UNROLL];
#pragma unroll
        for (int i = 0; i < UNROLL; i++) c[i] = ep[w + i * R] + col[(size_t)(w + i * R) * K];
#pragma unroll
        for (int i = 0; i < UNROLL; i++)
            if (c[i] > xb) {
                xb = c[i];
                xw = w + i * R;
            }
    }
    for (; w < K; w += R) {
        const double c = ep[w] + col[(size_t)w * K];
        if (c > xb) {
            xb = c;
            xw = w;
        }
    }
}

// gram = start[K] | pair[K][K] | fin[K]
__global__ void __launch_bounds__(CONNECT_THREADS)
k_grammar(int U, int K, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
          const long long *__restrict__ off, const double *__restrict__ gram, int staged,
          unsigned char *__restrict__ psi, unsigned char *__restrict__ entw, int *__restrict__ word,
          unsigned char *__restrict__ path, double *__restrict__ score, const int *__restrict__ order)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int u = order[blockIdx.x];
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    if (T <= 0) {
        if (tid == 0) score[u] = 0.0;
        return;
    }
    const size_t KK = staged ? (size_t)K * K : 0;
    double *d = lds, *la_self = lds + 2 * (size_t)NS, *la_prev = lds + 3 * (size_t)NS, *e = lds + 4 * (size_t)NS;
    double *px = e + 2 * (size_t)K, *ptab = px + GRAMMAR_ITEMS;
    int *meta = (int *)(ptab + KK), *pxw = meta + NS;
    const int R = min(4, max(1, nt / K)), items = K * R; // items <= max(K, nt) <= GRAMMAR_ITEMS
    const double *start = gram, *pair = gram + K, *fin = gram + K + (size_t)K * K;
    const double *lb = logb + f0 * NS;
    unsigned char *ps = psi + (size_t)f0 * NS;
    unsigned char *ew = entw + (size_t)f0 * K;
    int *wu = word + f0;

    // every state's word, and the table ...
    for (int k = tid; k < K; k += nt) {
        const fwd_model mk = tab[k];
        for (int j = 0; j < mk.N; j++) meta[mk.bo + j] = k;
    }
    for (size_t i = tid; i < KK; i += nt) ptab[i] = pair[i];
    __syncthreads();
    // ... then, a state per thread, its facts, its two band entries of log A, and frame 0
    for (int s = tid; s < NS; s += nt) {
        const int k = meta[s];
        const fwd_model mk = tab[k];
        const int N = mk.N, j = s - mk.bo;
        bool dense = false;
        for (int i = 0; i < N; i++) dense |= mk.A[i * N + j] != -INFINITY && i != j && i != j - 1;
        la_self[s] = mk.A[j * N + j];
        la_prev[s] = j > 0 ? mk.A[(j - 1) * N + j] : -INFINITY;
        const double v = ((j == 0) ? start[k] : -INFINITY) + lb[s];
        d[s] = v;
        if (j == N - 1) e[k] = v;
        ps[s] = 0;
        meta[s] = k | (j << CN_J_SHIFT) | (j == N - 1 ? CN_END : 0) | (dense ? CN_DENSE : 0);
    }
    __syncthreads();

    for (int t = 1; t < T; t++) {
        const double *prev = d + (size_t)((t + 1) & 1) * NS, *ep = e + (size_t)((t + 1) & 1) * K;
        double *cur = d + (size_t)(t & 1) * NS, *ec = e + (size_t)(t & 1) * K;
        // the entry pass: e_{t-1} is complete behind the previous frame's barrier
        for (int i = tid; i < items; i += nt) {
            const int k = i % K, r = i / K;
            double xb;
            int xw;
            if (staged) grammar_entry<8>(ep, ptab + k, K, r, R, xb, xw);
            else grammar_entry<16>(ep, pair + k, K, r, R, xb, xw); // L2 latency: more loads in flight
            px[i] = xb;
            pxw[i] = xw;
        }
        __syncthreads();
        for (int s = tid; s < NS; s += nt) {
            const double q = lb[(size_t)t * NS + s];
            const int mt = meta[s];
            const int j = (mt >> CN_J_SHIFT) & 63, k = mt & ((1 << CN_J_SHIFT) - 1);
            double best = -INFINITY;
            int arg = 0;
            if (!(mt & CN_DENSE)) {
                const double c1 = (j > 0 ? prev[s - 1] : 0.0) + la_prev[s]; // predecessor j - 1 (the lower index first)
                const double c0 = prev[s] + la_self[s];
                if (c1 > best) {
                    best = c1;
                    arg = j - 1;
                }
                if (c0 > best) {
                    best = c0;
                    arg = j;
                }
            } else {
                const fwd_model mk = tab[k];
                const double *pw = prev + (s - j);
                for (int i = 0; i < mk.N; i++) {
                    const double v = pw[i] + mk.A[i * mk.N + j];
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
            }
            if (j == 0) {
                double xb = px[k];
                int xw = pxw[k];
                for (int r = 1; r < R; r++) {
                    const double v = px[r * K + k];
                    const int w = pxw[r * K + k];
                    if (v > xb || (v == xb && w < xw)) {
                        xb = v;
                        xw = w;
                    }
                }
                if (xb > best) { // entry wins only on a strict >; a NaN never enters
                    best = xb;
                    arg = CONNECT_ENTRY;
                    ew[(size_t)t * K + k] = (unsigned char)xw;
                }
            }
            const double v = best + q;
            cur[s] = v;
            if (mt & CN_END) ec[k] = v;
            ps[(size_t)t * NS + s] = (unsigned char)arg;
        }
        __syncthreads();
    }
    __threadfence_block();
    if (tid != 0) return;
    const double *el = e + (size_t)((T - 1) & 1) * K;
    double bv = el[0] + fin[0];
    int k = 0;
    for (int w = 1; w < K; w++) {
        const double v = el[w] + fin[w];
        if (v > bv || (bv != bv && v == v)) {
            bv = v;
            k = w;
        }
    }
    score[u] = bv;
    int s = tab[k].N - 1;
    unsigned char *pu = path + f0;
    for (int t = T - 1; t >= 0; t--) {
        const int bp = ps[(size_t)t * NS + tab[k].bo + s];
        const bool enter = t == 0 || bp == CONNECT_ENTRY;
        wu[t] = k;
        pu[t] = (unsigned char)(s | (enter ? CONNECT_BEGIN : 0));
        if (t > 0 && enter) {
            k = ew[(size_t)t * K + k];
            s = tab[k].N - 1;
        } else {
            s = bp;
        }
    }
}

} // namespace ghmm
