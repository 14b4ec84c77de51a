// ghmm_connect.hpp — connected-word Viterbi decoding over a vocabulary (ghmm_connect_streams and
// ghmm_connect_full_streams; definition in include/ghmm.h): ONE max-plus lattice over the states of
// all words at once, on the log b[F][NS] that the vocabulary's emission launches left in the
// workspace.  Inside a word the step is viterbi_run's; the best word end of frame t-1 plus the word
// penalty may enter every word's first state at frame t.
//
// One workgroup per utterance (longest first, order[]), of 1 to 4 waves: the composite states
// s = tid, tid + blockDim.x, ... of a thread are the same in every frame.  LDS holds the running
// scores d[2][NS], every state's log a_jj and log a_{j-1,j}, one packed word of state facts, and the
// waves' partial picks.
//
// One barrier per frame.  A thread that owns a word's last state folds its d_t into a running
// (value, word) pick under the order below; the wave reduces it by a butterfly and lane 0 leaves the
// wave's partial in LDS, double-buffered by frame parity, ahead of the frame's barrier.  Behind the
// barrier every thread combines the partials (at most four) itself: e_{t-1} and w_{t-1} are known to
// everybody without a second barrier, and the row d_{t-1} is complete.
//
// The pick of a list is k_vocab_best's rule as an order, so that any reduction tree gives the same
// answer: a beats b if a's value is greater; or b's is NaN and a's is not; or neither value beats the
// other and a's word is lower.  (NaN, INT_MAX) loses to everything: what a thread without a word end
// contributes.
//
// Back-pointers: one byte per (frame, composite state), rows of NS bytes: the predecessor within the
// word (< 64), or CONNECT_ENTRY where the state was entered from the previous frame's pick.  w_t goes
// to word[f0 + t], one int per frame; the trace (one lane, as in k_viterbi_wide) walks back from the
// last frame and overwrites word[] in place: frame t's entry is rewritten after w_t was last read (by
// frame t + 1) and before w_{t-1} is.  path[f0 + t] = the state within the word, | CONNECT_BEGIN on the
// first frame of a word instance.
//
// The band shortcut: a column of log A whose entries off {j - 1, j} are all -inf takes the two
// candidates alone.  A candidate with log a = -inf is -inf or NaN and never wins a strict >, so the
// bits are the dense loop's.
#pragma once
#include "ghmm_kernels.hpp"

#include <climits>

namespace ghmm {

constexpr int CONNECT_MAX_NS = 2048; // composite states: 36 bytes of LDS each, 72 KB at the cap
constexpr int CONNECT_THREADS = 256;
constexpr int CONNECT_ENTRY = 255;   // the back-pointer of a word's first state entered from the pick
constexpr int CONNECT_BEGIN = 128;   // path[]: the frame begins a word instance (the state is below 64)

// LDS of k_connect for NS composite states: d[2][NS] | la_self[NS] | la_prev[NS] | pv[2][4] | meta[NS] | pk[2][4]
constexpr size_t connect_lds(int NS) { return (size_t)NS * 36 + 8 * 8 + 8 * 4; }

// facts of composite state s, packed: word (12 bits; K <= NS <= 2048), state within the word (6 bits),
// last state of its word, column of log A has entries off the band
constexpr int CN_J_SHIFT = 12, CN_END = 1 << 18, CN_DENSE = 1 << 19;

__device__ __forceinline__ bool connect_beats(double av, int ak, double bv, int bk)
{
    if (av > bv || (bv != bv && av == av)) return true;
    if (bv > av || (av != av && bv == bv)) return false;
    return ak < bk;
}

__global__ void __launch_bounds__(CONNECT_THREADS)
k_connect(int U, int K, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
          const long long *__restrict__ off, double penalty, unsigned char *__restrict__ psi,
          int *__restrict__ word, unsigned char *__restrict__ path, double *__restrict__ score,
          const int *__restrict__ order)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x, nw = nt / WAVE;
    const int u = order[blockIdx.x];
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    if (T <= 0) {
        if (tid == 0) score[u] = 0.0;
        return;
    }
    double *d = lds, *la_self = lds + 2 * (size_t)NS, *la_prev = lds + 3 * (size_t)NS, *pv = lds + 4 * (size_t)NS;
    int *meta = (int *)(pv + 8), *pk = meta + NS;
    const double *lb = logb + f0 * NS;
    unsigned char *ps = psi + (size_t)f0 * NS;
    int *wu = word + f0;

    // every state's word ...
    for (int k = tid; k < K; k += nt) {
        const fwd_model mk = tab[k];
        for (int j = 0; j < mk.N; j++) meta[mk.bo + j] = k;
    }
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
        d[s] = ((j == 0) ? 0.0 : -INFINITY) + lb[s];
        ps[s] = 0;
        meta[s] = k | (j << CN_J_SHIFT) | (j == N - 1 ? CN_END : 0) | (dense ? CN_DENSE : 0);
    }
    __syncthreads();

    // the wave's partial pick of row `row` (complete for this thread's own states) into slot `par`
    auto publish = [&](const double *row, int par) {
        double bv = NAN;
        int bk = INT_MAX;
        for (int s = tid; s < NS; s += nt) {
            const int mt = meta[s];
            if (mt & CN_END) {
                const double v = row[s];
                const int k = mt & ((1 << CN_J_SHIFT) - 1);
                if (connect_beats(v, k, bv, bk)) {
                    bv = v;
                    bk = k;
                }
            }
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, WAVE);
            const int ok = __shfl_xor(bk, o, WAVE);
            if (connect_beats(ov, ok, bv, bk)) {
                bv = ov;
                bk = ok;
            }
        }
        if ((tid & (WAVE - 1)) == 0) {
            pv[par * 4 + tid / WAVE] = bv;
            pk[par * 4 + tid / WAVE] = bk;
        }
    };
    // the block's pick from the waves' partials in slot `par`
    auto combine = [&](int par, double &ev, int &ek) {
        ev = pv[par * 4];
        ek = pk[par * 4];
        for (int w = 1; w < nw; w++) {
            const double ov = pv[par * 4 + w];
            const int ok = pk[par * 4 + w];
            if (connect_beats(ov, ok, ev, ek)) {
                ev = ov;
                ek = ok;
            }
        }
    };

    publish(d, 0);
    __syncthreads();
    for (int t = 1; t < T; t++) {
        const double *prev = d + (size_t)((t + 1) & 1) * NS;
        double *cur = d + (size_t)(t & 1) * NS;
        double ev;
        int ek;
        combine((t + 1) & 1, ev, ek);
        if (tid == 0) wu[t - 1] = ek;
        const double x = ev + penalty;
        for (int s = tid; s < NS; s += nt) {
            const double q = lb[(size_t)t * NS + s];
            const int mt = meta[s];
            const int j = (mt >> CN_J_SHIFT) & 63;
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
                const fwd_model mk = tab[mt & ((1 << CN_J_SHIFT) - 1)];
                const double *pw = prev + (s - j);
                for (int i = 0; i < mk.N; i++) {
                    const double v = pw[i] + mk.A[i * mk.N + j];
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
            }
            if (j == 0 && x > best) { // entry wins only on a strict >; a NaN x never enters
                best = x;
                arg = CONNECT_ENTRY;
            }
            cur[s] = best + q;
            ps[(size_t)t * NS + s] = (unsigned char)arg;
        }
        publish(cur, t & 1);
        __syncthreads();
    }
    __threadfence_block();
    if (tid != 0) return;
    double ev;
    int k;
    combine((T - 1) & 1, ev, k);
    score[u] = ev;
    int s = tab[k].N - 1;
    unsigned char *pu = path + f0;
    for (int t = T - 1; t >= 0; t--) {
        const int bp = ps[(size_t)t * NS + tab[k].bo + s];
        const bool enter = t == 0 || bp == CONNECT_ENTRY;
        wu[t] = k;
        pu[t] = (unsigned char)(s | (enter ? CONNECT_BEGIN : 0));
        if (t > 0 && enter) {
            k = wu[t - 1];
            s = tab[k].N - 1;
        } else {
            s = bp;
        }
    }
}

} // namespace ghmm
