// ghmm_gpost.hpp — word posteriors under a word-pair grammar (ghmm_grammar_post_streams and
// ghmm_grammar_post_full_streams; definition in include/ghmm.h): the log-domain forward-backward over the
// lattice that k_grammar (ghmm_grammar.hpp) walks with max.  Word k's first state is entered at frame t from
// the end of ANY word w of frame t-1 with weight pair[w][k]; the max over w becomes a log-sum-exp, and a
// backward pass gives every composite state its posterior gamma, every (frame, word) the posterior occ that
// the frame lies in the word and the posterior ent that an instance of the word begins there, and the
// utterance its total log P over every word string the grammar allows.
//
// Two launches, one workgroup per utterance (longest first, order[]), of 1 to 4 waves.
//   Layout: k_grammar's.  The composite states s = tid, tid + blockDim.x, ... of a thread are the same in
//   every frame (PASSES of them, a template parameter: 1, 2, 4 or 8); two rows of the lattice and every
//   state's two band entries of log A live in LDS; the word ends (forward) and the first states' w_t
//   (backward) sit in compact double-buffered rows of K.
//   Time: k_embed's (ghmm_embed.hpp).  A thread loads the NEXT frame's log b (backward: la, and x for a first
//   state) of its states ahead of the step, so that the loads are in flight across the frame's barriers.
//   Inside a word the steps are k_embed's: the banded two-term hi + log1p(exp(lo - hi)) or the dense
//   m + log(sum exp) with its NaN rule, chosen per WORD.
//
// k_gpost_fwd: x_t(k) = LSE_w (la_{t-1}(w, N_w - 1) + pair[w][k]) is k_grammar's entry pass: item i = r * K + k
// (i = tid, tid + blockDim.x, ...) takes word k and the candidates w = r, r + R, ..., R = blockDim.x / K
// clamped to 1..4 slices per word, and leaves a running (max, sum scaled by the max) pair in LDS, so the
// table is read ONCE per frame; behind a barrier the owner of word k's first state combines the R pairs into
// x_t(k), stores it (xrow[F][K]: the backward launch forms ent from it) and takes it into la_t(k, 0) by LSE2.
// Lanes on consecutive k read consecutive doubles of row w of the table as passed (pair[w * K + k]).  Every
// la row is stored, [F][NS], not ragged.  log P_u by one lane from the last frame's word ends and fin.
//
// k_gpost_bwd: y_t(k) = LSE_k' (pair[k][k'] + w_t(k', 0)) reduces along ROW k of the table.  With the forward
// pass's items (lanes on consecutive k, candidates k' in sequence) a wave would read pair[k * K + k'] at a
// stride of K doubles: K separate cache lines per load from L2, and from a staged table in LDS the lanes
// of a half-wave K * 2 banks apart, that is all on ONE bank whenever K is a multiple of 32 (a 32-way
// conflict; the banks of a 64-bit read are (address / 4) mod 64).  The other cure, lanes on consecutive k' for
// one k, reads the row coalesced but then needs a cross-lane (max, sum) reduction per word, K of them per
// frame, and leaves y_t(k) in one lane that is not the owner of the word's last state.  So the host uploads
// a TRANSPOSED copy beside the table (pairT[k' * K + k] = pair[k][k']; K * K doubles more in gr_tab, at most
// 512 KB, one copy per call), and the exit pass IS the entry pass on it: consecutive lanes, consecutive
// doubles, no conflict, the same code.  Only this form was built; there is no timing of the other order.
// The step forms lbe_t, gamma_t and w_{t-1} of a thread's states; gamma leaves from the register that formed
// it, and after the frame's barrier lane k adds word k's gammas in ascending j into occ and copies the
// first state's entry share into ent.  Where log P_u is not finite the block writes zero rows and returns.
//
// k_gpost_bwd<PASSES, true> is the statistics form of the backward launch (ghmm_estep_grammar_streams): the same
// step, and besides gamma every thread keeps the running sums of its states over the frames in registers, as
// k_embed_bwd does (xi[0..delta], stay, gamma; 8 x 11 at PASSES = 8), and writes them at the end straight into
// one partial per utterance in the layout k_reduce_all reads for a model of NS states.  There is one copy of
// each word in this lattice: nothing is tied, no list is walked, no LDS is added.  occ and ent are not formed
// (null is passed; rows_out and the g / ge rows are skipped).  The exits (T <= 0, a log P that is not finite)
// write zero partials, and the second zeroes the utterance's posterior rows as well (gpost_posts).  The <PASSES, false> instantiations are the code they were before the parameter.
//
// The table (forward: pair, backward: pairT) is staged in LDS while the launch's LDS stays within
// GRAMMAR_STAGE_LDS, otherwise read from L2, as in k_grammar.
#pragma once
#include "ghmm_embed.hpp"
#include "ghmm_grammar.hpp"

namespace ghmm {

constexpr int GPOST_THREADS = CONNECT_THREADS;
constexpr int GPOST_ITEMS = GRAMMAR_ITEMS; // K * R <= max(K, blockDim.x): the entry pass's partials

// LDS of k_gpost_fwd without the staged table:
// d[2][NS] | la_self[NS] | la_prev[NS] | e[2][K] | pm[GPOST_ITEMS] | ps[GPOST_ITEMS] | (table) | meta[NS]
constexpr size_t gpost_fwd_lds_base(int NS, int K) { return (size_t)NS * 36 + (size_t)K * 16 + GPOST_ITEMS * 16; }
// ... of k_gpost_bwd:
// w[2][NS] | g[2][NS] | la_self[NS] | la_next[NS] | wf[2][K] | ge[2][K] | pm[GPOST_ITEMS] | ps[GPOST_ITEMS] |
// (table) | meta[NS]                                       (116 KB at NS = 2048, K = 256: nothing is staged there)
constexpr size_t gpost_bwd_lds_base(int NS, int K) { return (size_t)NS * 52 + (size_t)K * 32 + GPOST_ITEMS * 16; }
constexpr bool gpost_staged(size_t base, int K) { return base + (size_t)K * K * 8 <= GRAMMAR_STAGE_LDS; }
constexpr size_t gpost_lds(size_t base, int K) { return base + (gpost_staged(base, K) ? (size_t)K * K * 8 : 0); }
static_assert(gpost_lds(gpost_bwd_lds_base(CONNECT_MAX_NS, GRAMMAR_MAX_K), GRAMMAR_MAX_K) <= 150u << 10 &&
                  gpost_lds(gpost_fwd_lds_base(CONNECT_MAX_NS, GRAMMAR_MAX_K), GRAMMAR_MAX_K) <= 150u << 10,
              "the lattice at its caps fits the raised LDS limit");

// one more term c of a running log-sum-exp kept as (m, s): the sum is m + log(s), s scaled by exp(-m).  -inf
// is not a term; a NaN goes into s and stays.  Starts at (-inf, 0).
__device__ __forceinline__ void gpost_add(double c, double &m, double &s)
{
    if (c == -INFINITY) return;
    const double dd = c - m;          // (+inf at the first term)
    const bool up = dd > 0.0;
    const double e = exp_emis(up ? -dd : dd);
    s = up ? fma(s, e, 1.0) : s + e;
    m = up ? c : m;
}

// slice r of R of an LSE over w = r, r + R, ... of v[w] + tab[w][k] (col = tab + k, rows K apart); an entry
// of -inf in the table is not a term.  The loads of UNROLL candidates are independent and go out together.
template <int UNROLL>
__device__ __forceinline__ void gpost_entry(const double *v, const double *col, int K, int r, int R, double &m,
                                            double &s)
{
    m = -INFINITY;
    s = 0.0;
    int w = r;
    for (; w + (UNROLL - 1) * R < K; w += UNROLL * R) {
        double c[UNROLL];
#pragma unroll
        for (int i = 0; i < UNROLL; i++) {
            const double g = col[(size_t)(w + i * R) * K];
            c[i] = g != -INFINITY ? v[w + i * R] + g : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < UNROLL; i++) gpost_add(c[i], m, s);
    }
    for (; w < K; w += R) {
        const double g = col[(size_t)w * K];
        gpost_add(g != -INFINITY ? v[w] + g : -INFINITY, m, s);
    }
}

// the R slices of word k into one value: max of the maxima, the sums rescaled to it
__device__ __forceinline__ double gpost_combine(const double *pm, const double *ps, int K, int k, int R)
{
    double m = pm[k];
    for (int r = 1; r < R; r++) m = fmax(m, pm[r * K + k]);
    const double mm = m == -INFINITY ? 0.0 : m;
    double s = 0.0;
    for (int r = 0; r < R; r++) s += ps[r * K + k] * exp_emis(pm[r * K + k] - mm);
    return m + log(s);
}

// every state's word and whether that word's log A has entries off the band (k_embed's test, per word), a
// word per thread.  The caller's barrier follows.
__device__ __forceinline__ void gpost_words(const fwd_model *__restrict__ tab, int K, int *meta)
{
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const fwd_model mk = tab[k];
        const int N = mk.N;
        bool dense = false;
        for (int r = 0; r < N; r++)
            for (int c = 0; c < N; c++) dense |= mk.A[r * N + c] != -INFINITY && c != r && c != r + 1;
        for (int j = 0; j < N; j++) meta[mk.bo + j] = k | (dense ? CN_DENSE : 0);
    }
}

// the step inside a word on the previous row: LSE_i (row[s0 + i] + log a_ij), banded or dense; forward reads
// column j of log A (stride N), backward row j (stride 1)
__device__ __forceinline__ double gpost_dense(const double *pw, const double *a, int N, int stride)
{
    double m = -INFINITY;
    for (int i = 0; i < N; i++) {
        const double la = a[i * stride];
        const double v = la != -INFINITY ? pw[i] + la : -INFINITY;
        m = fmax(m, v); // (a NaN term is passed over here and taken by the sum)
    }
    const double mm = m == -INFINITY ? 0.0 : m;
    double sum = 0.0;
    for (int i = 0; i < N; i++) {
        const double la = a[i * stride];
        const double v = la != -INFINITY ? pw[i] + la : -INFINITY;
        sum += exp_emis(v - mm);
    }
    return m + log(sum);
}

// gram = start[K] | pair[K][K] | fin[K] | pairT[K][K].  la[F][NS], xrow[F][K] (row 0 of an utterance is not
// written: nothing enters at frame 0), loglik[U].
template <int PASSES>
__global__ void __launch_bounds__(GPOST_THREADS)
k_gpost_fwd(int U, int K, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
            const long long *__restrict__ off, const double *__restrict__ gram, int staged, double *__restrict__ la,
            double *__restrict__ xrow, double *__restrict__ loglik, const int *__restrict__ order)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int u = order[blockIdx.x];
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    if (T <= 0) {
        if (tid == 0) loglik[u] = 0.0;
        return;
    }
    const size_t KK = staged ? (size_t)K * K : 0;
    double *d = lds, *la_self = lds + 2 * (size_t)NS, *la_prev = lds + 3 * (size_t)NS, *e = lds + 4 * (size_t)NS;
    double *pm = e + 2 * (size_t)K, *ps = pm + GPOST_ITEMS, *ptab = ps + GPOST_ITEMS;
    int *meta = (int *)(ptab + KK);
    const int R = min(4, max(1, nt / K)), items = K * R; // items <= max(K, nt) <= GPOST_ITEMS
    const double *start = gram, *pair = gram + K, *fin = gram + K + (size_t)K * K;
    const double *lb = logb + f0 * NS;
    double *lu = la + f0 * NS, *xu = xrow + f0 * K;

    gpost_words(tab, K, meta);
    for (size_t i = tid; i < KK; i += nt) ptab[i] = pair[i];
    __syncthreads();
    // a state per thread and pass: its facts, its two band entries of log A, frame 0, and frame 1's log b
    double qn[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        const int s = tid + p * nt;
        qn[p] = 0.0;
        if (s < NS) {
            const int k = meta[s] & ((1 << CN_J_SHIFT) - 1);
            const fwd_model mk = tab[k];
            const int N = mk.N, j = s - mk.bo;
            la_self[s] = mk.A[j * N + j];
            la_prev[s] = j > 0 ? mk.A[(j - 1) * N + j] : -INFINITY;
            const double v = (j == 0 ? start[k] : -INFINITY) + lb[s];
            d[s] = v;
            lu[s] = v;
            if (j == N - 1) e[k] = v;
            meta[s] = (meta[s] & CN_DENSE) | k | (j << CN_J_SHIFT) | (j == N - 1 ? CN_END : 0);
            qn[p] = lb[(size_t)(T > 1 ? 1 : 0) * NS + s];
        }
    }
    __syncthreads();

    for (int t = 1; t < T; t++) {
        const double *prev = d + (size_t)((t + 1) & 1) * NS, *ep = e + (size_t)((t + 1) & 1) * K;
        double *cur = d + (size_t)(t & 1) * NS, *ec = e + (size_t)(t & 1) * K;
        const size_t tn = (size_t)(t + 1 < T ? t + 1 : t); // the frame prefetched (clamped into the utterance)
        // the entry pass: e_{t-1} is complete behind the previous frame's barrier
        for (int i = tid; i < items; i += nt) {
            const int k = i % K, r = i / K;
            double m, s;
            if (staged) gpost_entry<8>(ep, ptab + k, K, r, R, m, s);
            else gpost_entry<16>(ep, pair + k, K, r, R, m, s); // L2 latency: more loads in flight
            pm[i] = m;
            ps[i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            if (s >= NS) continue;
            const double q = qn[p];
            qn[p] = lb[tn * NS + s];
            const int mt = meta[s];
            const int j = (mt >> CN_J_SHIFT) & 63, k = mt & ((1 << CN_J_SHIFT) - 1);
            double r;
            if (!(mt & CN_DENSE)) {
                const double lp = la_prev[s], ls = la_self[s];
                const double c1 = lp != -INFINITY ? prev[s - 1] + lp : -INFINITY; // (j > 0 where lp is a term)
                const double c0 = ls != -INFINITY ? prev[s] + ls : -INFINITY;
                r = embed_lse2(c0, c1);
            } else {
                const fwd_model mk = tab[k];
                r = gpost_dense(prev + (s - j), mk.A + j, mk.N, mk.N);
            }
            if (j == 0) {
                const double x = gpost_combine(pm, ps, K, k, R);
                xu[(size_t)t * K + k] = x;
                r = embed_lse2(r, x);
            }
            const double v = r + q;
            cur[s] = v;
            lu[(size_t)t * NS + s] = v;
            if (mt & CN_END) ec[k] = v;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double *el = e + (size_t)((T - 1) & 1) * K;
    double m = -INFINITY, s = 0.0;
    for (int k = 0; k < K; k++) {
        const double g = fin[k];
        gpost_add(g != -INFINITY ? el[k] + g : -INFINITY, m, s);
    }
    loglik[u] = m + log(s);
}

// The statistics form's view of the mixture posteriors that the statistics launches will weigh with gamma:
// stream p's rows post[p][F][NS * M[p]].  An utterance whose log P is not finite must add nothing to any sum,
// and 0 x NaN is not nothing (a column whose log b is NaN has NaN posteriors), so the block zeroes the
// utterance's posterior rows beside its gamma rows: every weight is then exactly 0 and the statistics launches
// pass over its frames.
constexpr int GPOST_MAX_STREAMS = 8;
struct gpost_posts {
    double *post[GPOST_MAX_STREAMS];
    int M[GPOST_MAX_STREAMS];
    int P;
};

// gamma[F][NS], occ[F][K], ent[F][K].  STATS (ghmm_estep_grammar_streams): occ and ent are null and not formed;
// part_*: one partial per utterance (slot = u of U) for a model of NS states, as k_embed_bwd leaves them for
// k_reduce_all.  Without STATS delta and part_* are not read.
template <int PASSES, bool STATS = false>
__global__ void __launch_bounds__(GPOST_THREADS)
k_gpost_bwd(int U, int K, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
            const long long *__restrict__ off, const double *__restrict__ gram, int staged,
            const double *__restrict__ la, const double *__restrict__ xrow, const double *__restrict__ loglik,
            double *__restrict__ gamma, double *__restrict__ occ, double *__restrict__ ent,
            const int *__restrict__ order, int delta, double *__restrict__ part_xi, double *__restrict__ part_dena,
            double *__restrict__ part_denc, gpost_posts posts)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int u = order[blockIdx.x];
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    // an utterance that adds nothing to the sums (no frames, or a log P that is not finite): zero partials
    auto no_sums = [&]() {
        for (int c = tid; c < NS; c += nt) {
            for (int o = 0; o <= delta; o++) part_xi[pxi_at(u, c, o, U)] = 0.0;
            part_dena[pden_at(u, c, U)] = 0.0;
            part_denc[pden_at(u, c, U)] = 0.0;
        }
    };
    if (T <= 0) {
        if constexpr (STATS) no_sums();
        return;
    }
    double *gu = gamma + f0 * NS, *ou = nullptr, *nu = nullptr;
    if constexpr (!STATS) {
        ou = occ + f0 * K;
        nu = ent + f0 * K;
    }
    const double logP = loglik[u];
    if (!(fabs(logP) < INFINITY)) { // (a NaN included) no allowed string, or a NaN column: zero rows
        for (size_t i = tid; i < (size_t)T * NS; i += nt) gu[i] = 0.0;
        if constexpr (STATS) {
            no_sums();
            for (int p = 0; p < posts.P; p++) {
                const size_t row = (size_t)NS * posts.M[p];
                double *pu = posts.post[p] + (size_t)f0 * row;
                for (size_t i = tid; i < (size_t)T * row; i += nt) pu[i] = 0.0;
            }
        } else
            for (size_t i = tid; i < (size_t)T * K; i += nt) {
                ou[i] = 0.0;
                nu[i] = 0.0;
            }
        return;
    }
    const size_t KK = staged ? (size_t)K * K : 0;
    double *w = lds, *g = lds + 2 * (size_t)NS, *la_self = lds + 4 * (size_t)NS, *la_next = lds + 5 * (size_t)NS;
    double *wf = lds + 6 * (size_t)NS, *ge = wf + 2 * (size_t)K, *pm = ge + 2 * (size_t)K, *ps = pm + GPOST_ITEMS;
    double *ptab = ps + GPOST_ITEMS;
    int *meta = (int *)(ptab + KK);
    const int R = min(4, max(1, nt / K)), items = K * R;
    const double *fin = gram + K + (size_t)K * K, *pairT = fin + K;
    const double *lb = logb + f0 * NS, *lu = la + f0 * NS, *xu = xrow + f0 * K;

    gpost_words(tab, K, meta);
    for (size_t i = tid; i < KK; i += nt) ptab[i] = pairT[i];
    __syncthreads();
    // the NEXT step's la, log b and (first states) x, loaded a frame ahead
    double an[PASSES], bn[PASSES], xn[PASSES];
    // STATS: a state's running sums over the frames, in registers as in k_embed_bwd (one copy of each word in
    // this lattice: nothing is tied); without STATS one element each, never touched
    constexpr int SP = STATS ? PASSES : 1, SO = STATS ? MAX_DELTA + 1 : 1;
    double xi[SP][SO], st[SP], gs[SP], gl[SP];
    if constexpr (STATS) {
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            st[p] = gs[p] = gl[p] = 0.0;
#pragma unroll
            for (int o = 0; o <= MAX_DELTA; o++) xi[p][o] = 0.0;
        }
    }
    // frame T-1: lbe = fin in the words' last states; gamma_{T-1}; w_{T-2}
    {
        double *wn = w + (size_t)((T - 2) & 1) * NS, *wfn = wf + (size_t)((T - 2) & 1) * K;
        double *gt = g + (size_t)((T - 1) & 1) * NS, *get = ge + (size_t)((T - 1) & 1) * K;
        const size_t tp = (size_t)(T > 1 ? T - 2 : 0);
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            an[p] = bn[p] = xn[p] = 0.0;
            if (s < NS) {
                const int k = meta[s] & ((1 << CN_J_SHIFT) - 1);
                const fwd_model mk = tab[k];
                const int N = mk.N, j = s - mk.bo;
                la_self[s] = mk.A[j * N + j];
                la_next[s] = j + 1 < N ? mk.A[j * N + j + 1] : -INFINITY;
                meta[s] = (meta[s] & CN_DENSE) | k | (j << CN_J_SHIFT) | (j == N - 1 ? CN_END : 0);
                const double be = j == N - 1 ? fin[k] : -INFINITY;
                const double al = lu[(size_t)(T - 1) * NS + s], lbt = lb[(size_t)(T - 1) * NS + s];
                const double gv = exp_emis((al + be) - logP);
                gu[(size_t)(T - 1) * NS + s] = gv;
                if constexpr (STATS) gl[p] = gv; // gamma_{T-1}: in den_c (t < T) but not in den_a (t < T-1)
                else {
                    gt[s] = gv;
                    if (j == 0) get[k] = T > 1 ? exp_emis(((xu[(size_t)(T - 1) * K + k] + lbt) + be) - logP) : gv;
                }
                if (T > 1) {
                    wn[s] = be + lbt;
                    if (j == 0) {
                        wfn[k] = be + lbt;
                        xn[p] = xu[(tp > 0 ? tp : 1) * K + k]; // (row 0 holds nothing; frame 0 does not use it)
                    }
                    an[p] = lu[tp * NS + s];
                    bn[p] = lb[tp * NS + s];
                }
            }
        }
    }
    __syncthreads();
    // occ and ent of frame t from the frame's rows: lane k adds word k's gammas in ascending j
    auto rows_out = [&](int t) {
        const double *gt = g + (size_t)(t & 1) * NS, *get = ge + (size_t)(t & 1) * K;
        for (int k = tid; k < K; k += nt) {
            const fwd_model mk = tab[k];
            double v = 0.0;
            for (int j = 0; j < mk.N; j++) v += gt[mk.bo + j];
            ou[(size_t)t * K + k] = v;
            nu[(size_t)t * K + k] = get[k];
        }
    };
    if constexpr (!STATS) rows_out(T - 1);

    for (int t = T - 2; t >= 0; t--) {
        const double *wt = w + (size_t)(t & 1) * NS, *wft = wf + (size_t)(t & 1) * K;
        double *wn = w + (size_t)((t + 1) & 1) * NS, *wfn = wf + (size_t)((t + 1) & 1) * K;
        double *gt = g + (size_t)(t & 1) * NS, *get = ge + (size_t)(t & 1) * K;
        const size_t tp = (size_t)(t > 0 ? t - 1 : 0); // the frame prefetched (clamped into the utterance)
        // the exit pass: the first states' w_t are complete behind the previous step's barrier
        for (int i = tid; i < items; i += nt) {
            const int k = i % K, r = i / K;
            double m, s;
            if (staged) gpost_entry<8>(wft, ptab + k, K, r, R, m, s);
            else gpost_entry<16>(wft, pairT + k, K, r, R, m, s);
            pm[i] = m;
            ps[i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            if (s >= NS) continue;
            const int mt = meta[s];
            const int j = (mt >> CN_J_SHIFT) & 63, k = mt & ((1 << CN_J_SHIFT) - 1);
            const double al = an[p], lbt = bn[p], x = xn[p]; // la_t(s), log b_s(t), x_t(k)
            an[p] = lu[tp * NS + s];
            bn[p] = lb[tp * NS + s];
            if (j == 0) xn[p] = xu[(tp > 0 ? tp : 1) * K + k];
            double wi;
            if (!(mt & CN_DENSE)) {
                const double ls = la_self[s], ln = la_next[s];
                const double c0 = ls != -INFINITY ? ls + wt[s] : -INFINITY;
                const double c1 = ln != -INFINITY ? ln + wt[s + 1] : -INFINITY; // (j + 1 < N where ln is a term)
                wi = embed_lse2(c0, c1);
            } else {
                const fwd_model mk = tab[k];
                wi = gpost_dense(wt + (s - j), mk.A + j * mk.N, mk.N, 1);
            }
            const double be = (mt & CN_END) ? embed_lse2(wi, gpost_combine(pm, ps, K, k, R)) : wi;
            const double gv = exp_emis((al + be) - logP);
            gu[(size_t)t * NS + s] = gv;
            if constexpr (STATS) {
                // the band's xi: a transition with a_{j,j+o} == 0 (or outside the word / the band) is not a term
                const double ls = la_self[s], ln = la_next[s];
                if (ls != -INFINITY) xi[p][0] += exp_emis(((al + ls) + wt[s]) - logP);
                if (delta >= 1 && ln != -INFINITY) xi[p][1] += exp_emis(((al + ln) + wt[s + 1]) - logP);
                if (delta >= 2) {
                    const fwd_model mk = tab[k];
#pragma unroll
                    for (int o = 2; o <= MAX_DELTA; o++)
                        if (o <= delta && j + o < mk.N) {
                            const double a = mk.A[j * mk.N + j + o];
                            if (a != -INFINITY) xi[p][o] += exp_emis(((al + a) + wt[s + o]) - logP);
                        }
                }
                gs[p] += gv;
                st[p] += exp_emis((al + wi) - logP);
            } else {
                gt[s] = gv;
                if (j == 0) get[k] = t > 0 ? exp_emis(((x + lbt) + be) - logP) : gv;
            }
            if (t > 0) {
                wn[s] = be + lbt;
                if (j == 0) wfn[k] = be + lbt;
            }
        }
        __syncthreads();
        if constexpr (!STATS) rows_out(t);
    }
    if constexpr (STATS) {
        // every composite state is its own: the sums leave from the registers that formed them
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int s = tid + p * nt;
            if (s >= NS) continue;
#pragma unroll
            for (int o = 0; o <= MAX_DELTA; o++)
                if (o <= delta) part_xi[pxi_at(u, s, o, U)] = xi[p][o];
            part_dena[pden_at(u, s, U)] = st[p];
            part_denc[pden_at(u, s, U)] = gs[p] + gl[p];
        }
    }
}

} // namespace ghmm
