// ghmm_align.hpp — forced alignment of a word transcript (ghmm_align_streams and ghmm_align_full_streams;
// definition in include/ghmm.h): a left-to-right max-plus lattice over the states of the transcript's
// word instances, on the log b[F][NS] that the vocabulary's emission launches left in the workspace.
// Inside an instance the step is k_connect's (viterbi_run's); the last state of instance i - 1 at frame
// t - 1 may enter the first state of instance i at frame t.  Every instance has ONE fixed predecessor, so
// where k_connect reduces a pick over all word ends per frame, nothing is reduced here: the entry
// candidate of an instance's first state is prev[s - 1].
//
// One workgroup per utterance (longest first, order[]), of 1 to 4 waves sized by the launch's largest
// S_u; a block loops over its own S_u composite states, s = tid, tid + blockDim.x, ...  LDS per composite
// state: the running scores d[2], log a_jj, log a_{j-1,j}, one packed word of facts, and the state's
// column in log b: 40 bytes, 80 KB at the cap.  One barrier per frame.
//
// The block builds its state table from the transcript once: the instances' state counts, an inclusive
// scan of them in LDS (in the room of d, which nobody has written yet), then per instance its states'
// facts and columns, then per state the two band entries of log A and frame 0.
//
// Back-pointers: one byte per (frame, composite state) in rows of S_u bytes from the utterance's own
// offset (poff[u], built on the host: sum of T * S over the utterances before it): the predecessor within
// the word (< 64), or CONNECT_ENTRY where the state was entered from the instance before.  The trace (one
// lane, as in k_connect) starts in the last state of the last instance and writes word[f0 + t] = the
// instance's word and path[f0 + t] = the state within the word, | CONNECT_BEGIN on an instance's first frame.
//
// The band shortcut and the dense fall-back are k_connect's, with its candidate order: the same bits.
#pragma once
#include "ghmm_connect.hpp"

namespace ghmm {

constexpr int ALIGN_MAX_S = CONNECT_MAX_NS; // composite states of one utterance's transcript

// LDS of k_align for S composite states: d[2][S] | la_self[S] | la_prev[S] | meta[S] | col[S]
constexpr size_t align_lds(int S) { return (size_t)S * 40; }

// facts of composite state s, packed: instance within the transcript (12 bits; L <= S <= 2048), state
// within the word (6 bits), column of log A has entries off the band, first state of an instance behind
// the first (takes the entry candidate)
constexpr int AL_J_SHIFT = 12, AL_DENSE = 1 << 18, AL_FIRST = 1 << 19;

// poff, seq_off and seq: the call's tables in the context (vocab_align uploads them ahead of the launch)
__global__ void __launch_bounds__(CONNECT_THREADS)
k_align(int U, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
        const long long *__restrict__ off, const long long *__restrict__ poff, const int *__restrict__ seq_off,
        const int *__restrict__ seq, unsigned char *__restrict__ psi, int *__restrict__ word,
        unsigned char *__restrict__ path, double *__restrict__ score, const int *__restrict__ order, int Smax)
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
    const int *sq = seq + seq_off[u];
    const int L = seq_off[u + 1] - seq_off[u]; // >= 1 (the host refuses an empty transcript with T > 0)
    double *d = lds, *la_self = lds + 2 * (size_t)Smax, *la_prev = lds + 3 * (size_t)Smax;
    int *meta = (int *)(lds + 4 * (size_t)Smax), *col = meta + Smax;

    // the instances' state counts and their inclusive scan, in d's room (2 * L ints of 4 * Smax)
    int *sa = (int *)d, *sb = sa + L;
    for (int i = tid; i < L; i += nt) sa[i] = tab[sq[i]].N;
    __syncthreads();
    for (int o = 1; o < L; o <<= 1) {
        for (int i = tid; i < L; i += nt) sb[i] = sa[i] + (i >= o ? sa[i - o] : 0);
        __syncthreads();
        int *sw = sa;
        sa = sb;
        sb = sw;
    }
    const int S = sa[L - 1]; // <= Smax (the host's sum)
    // every instance's states: facts and columns
    for (int i = tid; i < L; i += nt) {
        const fwd_model mk = tab[sq[i]];
        const int s0 = sa[i] - mk.N;
        for (int j = 0; j < mk.N; j++) {
            meta[s0 + j] = i | (j << AL_J_SHIFT) | (j == 0 && i > 0 ? AL_FIRST : 0);
            col[s0 + j] = mk.bo + j;
        }
    }
    __syncthreads(); // (the scan is read no more: d may be written)
    const double *lb = logb + f0 * NS;
    unsigned char *ps = psi + poff[u];
    // a state per thread: its two band entries of log A, whether its column is dense, and frame 0
    for (int s = tid; s < S; s += nt) {
        const int mt = meta[s];
        const int j = (mt >> AL_J_SHIFT) & 63;
        const fwd_model mk = tab[sq[mt & ((1 << AL_J_SHIFT) - 1)]];
        const int N = mk.N;
        bool dense = false;
        for (int i = 0; i < N; i++) dense |= mk.A[i * N + j] != -INFINITY && i != j && i != j - 1;
        la_self[s] = mk.A[j * N + j];
        la_prev[s] = j > 0 ? mk.A[(j - 1) * N + j] : -INFINITY;
        d[s] = (s == 0 ? 0.0 : -INFINITY) + lb[col[s]];
        ps[s] = 0;
        if (dense) meta[s] = mt | AL_DENSE;
    }
    __syncthreads();

    for (int t = 1; t < T; t++) {
        const double *prev = d + (size_t)((t + 1) & 1) * Smax;
        double *cur = d + (size_t)(t & 1) * Smax;
        for (int s = tid; s < S; s += nt) {
            const double q = lb[(size_t)t * NS + col[s]];
            const int mt = meta[s];
            const int j = (mt >> AL_J_SHIFT) & 63;
            double best = -INFINITY;
            int arg = 0;
            if (!(mt & AL_DENSE)) {
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
                const fwd_model mk = tab[sq[mt & ((1 << AL_J_SHIFT) - 1)]];
                const double *pw = prev + (s - j);
                for (int i = 0; i < mk.N; i++) {
                    const double v = pw[i] + mk.A[i * mk.N + j];
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
            }
            if (mt & AL_FIRST) { // entry wins only on a strict >; a NaN never enters
                const double x = prev[s - 1];
                if (x > best) {
                    best = x;
                    arg = CONNECT_ENTRY;
                }
            }
            cur[s] = best + q;
            ps[(size_t)t * S + s] = (unsigned char)arg;
        }
        __syncthreads();
    }
    __threadfence_block();
    if (tid != 0) return;
    int s = S - 1;
    score[u] = d[(size_t)((T - 1) & 1) * Smax + s];
    int *wu = word + f0;
    unsigned char *pu = path + f0;
    for (int t = T - 1; t >= 0; t--) {
        const int mt = meta[s];
        const int j = (mt >> AL_J_SHIFT) & 63;
        const int bp = ps[(size_t)t * S + s];
        const bool enter = t == 0 || bp == CONNECT_ENTRY;
        wu[t] = sq[mt & ((1 << AL_J_SHIFT) - 1)];
        pu[t] = (unsigned char)(j | (enter ? CONNECT_BEGIN : 0));
        if (t > 0 && enter) s -= 1; // (an entry is marked on AL_FIRST states alone: s >= 1)
        else if (t > 0) s += bp - j;
    }
}

} // namespace ghmm
