// Where k_connect's time goes: the kernel's frame loop copied with parts switched off (timing only: the
// variants without the pick or the barrier do not compute the decoder's answer).  13 words x 6 states,
// banded, 1000 utterances x 300 frames of random log b.  Result in profiles/connect_time.txt.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=on -Iinclude \
//       -Ispeech-recognition-hmm-continuous_amd/csrc profiles/tools/connect_lab.hip -o profiles/tools/connect_lab
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cmath>
#include "ghmm_connect.hpp"
using namespace ghmm;

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(e_)); exit(2); } } while (0)

template <bool PICK, bool BAR, bool TRACE>
__global__ void __launch_bounds__(CONNECT_THREADS)
k_lab(int U, int K, int NS, const fwd_model *__restrict__ tab, const double *__restrict__ logb,
      const long long *__restrict__ off, double penalty, unsigned char *__restrict__ psi,
      int *__restrict__ word, unsigned char *__restrict__ path, double *__restrict__ score)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nt = blockDim.x, nw = nt / WAVE;
    const int u = blockIdx.x;
    const long long f0 = off[u];
    const int T = (int)(off[u + 1] - f0);
    double *d = lds, *la_self = lds + 2 * (size_t)NS, *la_prev = lds + 3 * (size_t)NS, *pv = lds + 4 * (size_t)NS;
    int *meta = (int *)(pv + 8), *pk = meta + NS;
    const double *lb = logb + f0 * NS;
    unsigned char *ps = psi + (size_t)f0 * NS;
    int *wu = word + f0;
    for (int k = tid; k < K; k += nt) {
        const fwd_model mk = tab[k];
        for (int j = 0; j < mk.N; j++) meta[mk.bo + j] = k;
    }
    if (tid < 16) { pv[tid & 7] = -INFINITY; pk[tid & 7] = 0; }
    __syncthreads();
    for (int s = tid; s < NS; s += nt) {
        const int k = meta[s];
        const fwd_model mk = tab[k];
        const int N = mk.N, j = s - mk.bo;
        la_self[s] = mk.A[j * N + j];
        la_prev[s] = j > 0 ? mk.A[(j - 1) * N + j] : -INFINITY;
        d[s] = ((j == 0) ? 0.0 : -INFINITY) + lb[s];
        ps[s] = 0;
        meta[s] = k | (j << CN_J_SHIFT) | (j == N - 1 ? CN_END : 0);
    }
    __syncthreads();
    auto publish = [&](const double *row, int par) {
        double bv = NAN;
        int bk = INT_MAX;
        for (int s = tid; s < NS; s += nt) {
            const int mt = meta[s];
            if (mt & CN_END) {
                const double v = row[s];
                const int k = mt & ((1 << CN_J_SHIFT) - 1);
                if (connect_beats(v, k, bv, bk)) { bv = v; bk = k; }
            }
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, WAVE);
            const int ok = __shfl_xor(bk, o, WAVE);
            if (connect_beats(ov, ok, bv, bk)) { bv = ov; bk = ok; }
        }
        if ((tid & (WAVE - 1)) == 0) { pv[par * 4 + tid / WAVE] = bv; pk[par * 4 + tid / WAVE] = bk; }
    };
    auto combine = [&](int par, double &ev, int &ek) {
        ev = pv[par * 4];
        ek = pk[par * 4];
        for (int w = 1; w < nw; w++) {
            const double ov = pv[par * 4 + w];
            const int ok = pk[par * 4 + w];
            if (connect_beats(ov, ok, ev, ek)) { ev = ov; ek = ok; }
        }
    };
    if (PICK) publish(d, 0);
    __syncthreads();
    for (int t = 1; t < T; t++) {
        const double *prev = d + (size_t)((t + 1) & 1) * NS;
        double *cur = d + (size_t)(t & 1) * NS;
        double ev = -INFINITY;
        int ek = 0;
        if (PICK) combine((t + 1) & 1, ev, ek);
        if (tid == 0) wu[t - 1] = ek;
        const double x = ev + penalty;
        for (int s = tid; s < NS; s += nt) {
            const double q = lb[(size_t)t * NS + s];
            const int mt = meta[s];
            const int j = (mt >> CN_J_SHIFT) & 63;
            double best = -INFINITY;
            int arg = 0;
            const double c1 = (j > 0 ? prev[s - 1] : 0.0) + la_prev[s];
            const double c0 = prev[s] + la_self[s];
            if (c1 > best) { best = c1; arg = j - 1; }
            if (c0 > best) { best = c0; arg = j; }
            if (j == 0 && x > best) { best = x; arg = CONNECT_ENTRY; }
            cur[s] = best + q;
            ps[(size_t)t * NS + s] = (unsigned char)arg;
        }
        if (PICK) publish(cur, t & 1);
        if (BAR) __syncthreads();
    }
    __syncthreads();
    if (tid != 0) return;
    double ev;
    int k;
    combine((T - 1) & 1, ev, k);
    k = k < 0 || k >= K ? 0 : k;
    score[u] = ev;
    if (!TRACE) return;
    int s = tab[k].N - 1;
    unsigned char *pu = path + f0;
    for (int t = T - 1; t >= 0; t--) {
        int bp = ps[(size_t)t * NS + tab[k].bo + s];
        const bool enter = t == 0 || bp == CONNECT_ENTRY;
        wu[t] = k;
        pu[t] = (unsigned char)(s | (enter ? CONNECT_BEGIN : 0));
        if (t > 0 && enter) {
            k = wu[t - 1];
            k = k < 0 || k >= K ? 0 : k;
            s = tab[k].N - 1;
        } else {
            s = bp < tab[k].N ? bp : 0;
        }
    }
}

template <bool PICK, bool BAR, bool TRACE>
static void run(const char *name, int threads, int U, int K, int NS, const fwd_model *tab, const double *lb,
                const long long *off, unsigned char *psi, int *word, unsigned char *path, double *score)
{
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<float> ms;
    for (int r = 0; r < 8; r++) {
        CK(hipEventRecord(a, 0));
        hipLaunchKernelGGL((k_lab<PICK, BAR, TRACE>), dim3(U), dim3(threads), connect_lds(NS), 0, U, K, NS, tab, lb, off,
                           0.0, psi, word, path, score);
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        CK(hipGetLastError());
        float t;
        CK(hipEventElapsedTime(&t, a, b));
        if (r) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("%-34s %d threads: median %.3f ms (min %.3f, max %.3f)\n", name, threads, ms[ms.size() / 2], ms.front(),
           ms.back());
}

int main()
{
    const int K = 13, N = 6, NS = K * N, U = 1000, T = 300;
    const size_t F = (size_t)U * T;
    std::vector<double> A((size_t)N * N, -INFINITY), lb(F * NS);
    for (int i = 0; i < N; i++) {
        A[i * N + i] = log(i + 1 < N ? 0.9 : 1.0);
        if (i + 1 < N) A[i * N + i + 1] = log(0.1);
    }
    srand(5);
    for (auto &x : lb) x = -60.0 + 20.0 * rand() / RAND_MAX;
    std::vector<long long> off(U + 1);
    for (int u = 0; u <= U; u++) off[u] = (long long)u * T;
    double *dA, *dlb, *dscore;
    fwd_model *dtab;
    long long *doff;
    unsigned char *dpsi, *dpath;
    int *dword;
    CK(hipMalloc(&dA, A.size() * 8));
    CK(hipMalloc(&dlb, lb.size() * 8));
    CK(hipMalloc(&dscore, U * 8));
    CK(hipMalloc(&dtab, K * sizeof(fwd_model)));
    CK(hipMalloc(&doff, (U + 1) * 8));
    CK(hipMalloc(&dpsi, F * NS + 16));
    CK(hipMalloc(&dpath, F));
    CK(hipMalloc(&dword, F * 4));
    std::vector<fwd_model> tab(K);
    for (int k = 0; k < K; k++) tab[k] = {dA, N, k * N};
    CK(hipMemcpy(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dlb, lb.data(), lb.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dtab, tab.data(), K * sizeof(fwd_model), hipMemcpyHostToDevice));
    CK(hipMemcpy(doff, off.data(), (U + 1) * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dword, 0, F * 4));
    const int th = 128; // what the library launches for NS = 78
    run<true, true, true>("whole kernel", th, U, K, NS, dtab, dlb, doff, dpsi, dword, dpath, dscore);
    run<true, true, false>("without the trace", th, U, K, NS, dtab, dlb, doff, dpsi, dword, dpath, dscore);
    run<false, true, false>("without trace and pick", th, U, K, NS, dtab, dlb, doff, dpsi, dword, dpath, dscore);
    run<false, false, false>("without trace, pick and barrier", th, U, K, NS, dtab, dlb, doff, dpsi, dword, dpath, dscore);
    run<true, false, false>("without trace and barrier", th, U, K, NS, dtab, dlb, doff, dpsi, dword, dpath, dscore);
    run<true, true, true>("whole kernel", th, U, K, NS, dtab, dlb, doff, dpsi, dword, dpath, dscore);
    return 0;
}
