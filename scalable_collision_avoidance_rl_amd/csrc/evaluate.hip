// Policy evaluation over a stored rollout window [T][E][N] (benchmark_agent.py:59-106, :148-156): the per-episode table of
// the FIRST episode of every env -- length, collisions, per-agent and per-env returns, the critic's mean advantage
// G_t - V(z_t) -- and the collision histogram.  The env's episode layer (dronesim.hip) keeps sums over the finished episodes of an env;
// a table, a histogram and a per-agent critic check need the episodes themselves.
//
// episode_eval_kernel is returns_kernel's scan (scans.hip; shared pieces in scan_common.hpp) with three float64 accumulators
// per column riding along: one thread per (env, agent) column walks the window backwards, eight steps requested ahead of the
// eight being folded, four adjacent columns as 16-byte accesses when N % 4 == 0, the done bytes of a stage fetched by the wave
// with one load.  Every accumulator restarts where `done` is set, so at t = 0 it holds the first episode and the last flag
// seen gives its length.  reward, true_reward and V are read once, G is written once.  The per-env pieces (collisions, the mean
// over agents in ascending agent order) are a second small launch: no float atomics anywhere, bit-identical run to run.
#include "scan_common.hpp"
#include "dronesim.h"

namespace {

struct EvalArgs {
    const float *reward, *true_reward, *V;
    const uint8_t *done;
    float *G;
    int32_t *ep_len;
    double *agent_return, *agent_true_return, *mean_adv;
    float gamma;
    int T, E, N;
};

template <int V, bool HASV> struct EvStage {
    typename ColVec<V>::type r[kStageT], tr[kStageT], v[HASV ? kStageT : 1];
    DoneStage ds;
    bool dn[kStageT];
};

template <bool COOP, int V, bool HASV>
__device__ __forceinline__ void eval_fetch(EvStage<V, HASV> &st, const EvalArgs &a, size_t EN, size_t col, size_t e, size_t e_first, int t0)
{
    typedef typename ColVec<V>::type vec;
    if (COOP) st.ds.fetch(a.done, e_first, a.E, a.T, [&](int u) { return t0 - u; });
#pragma unroll
    for (int u = 0; u < kStageT; ++u) {
        const int t = t0 - u;
        const size_t at = (size_t)(t >= 0 ? t : 0) * EN + col;
        st.r[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(a.reward + at)) : vec(0.0f);
        st.tr[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(a.true_reward + at)) : vec(0.0f);
        if (HASV) st.v[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(a.V + at)) : vec(0.0f);
        if (!COOP) st.dn[u] = t >= 0 && a.done[(size_t)t * a.E + e] != 0;
    }
}

template <bool COOP, int V, bool HASV>
__device__ __forceinline__ void eval_scan(const EvalArgs &a, size_t EN, size_t col, size_t e, size_t e_first, int de, bool act)
{
    typedef typename ColVec<V>::type vec;
    const int T = a.T;
    const float gamma = a.gamma;
    vec g = vec(0.0f);
    double sr[V], st[V], sa[V];
#pragma unroll
    for (int q = 0; q < V; ++q) sr[q] = st[q] = sa[q] = 0.0;
    int L = 0;
    EvStage<V, HASV> cur, nxt;
    eval_fetch<COOP, V, HASV>(cur, a, EN, col, e, e_first, T - 1);
    for (int t0 = T - 1; t0 >= 0; t0 -= kStageT) {
        if (t0 - kStageT >= 0) eval_fetch<COOP, V, HASV>(nxt, a, EN, col, e, e_first, t0 - kStageT);
#pragma unroll
        for (int u = 0; u < kStageT; ++u) {
            const int t = t0 - u;
            if (t >= 0) {                                                         // (wave-uniform: the flag pick is a wave operation)
                const bool dn = COOP ? cur.ds.get(de, u) : cur.dn[u];
                const bool last = dn || t == T - 1;
                float *gp = reinterpret_cast<float *>(&g);
                const float *rp = reinterpret_cast<const float *>(&cur.r[u]);
                const float *tp = reinterpret_cast<const float *>(&cur.tr[u]);
                const float *vp = reinterpret_cast<const float *>(&cur.v[HASV ? u : 0]);
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    gp[q] = last ? rp[q] : fmaf(gp[q], gamma, rp[q]);             // dronesim_returns' recurrence, bit for bit
                    sr[q] = (dn ? 0.0 : sr[q]) + (double)rp[q];                   // benchmark_agent.py:85
                    st[q] = (dn ? 0.0 : st[q]) + (double)tp[q];                   // :86
                    if (HASV) sa[q] = (dn ? 0.0 : sa[q]) + ((double)gp[q] - (double)vp[q]);   // :105
                }
                if (dn) L = t + 1;
                if (act && a.G) __builtin_nontemporal_store(g, reinterpret_cast<vec *>(a.G + (size_t)t * EN + col));
            }
        }
        cur = nxt;
    }
    if (!act) return;
#pragma unroll
    for (int q = 0; q < V; ++q) {
        if (a.agent_return) a.agent_return[col + q] = L > 0 ? sr[q] : 0.0;
        if (a.agent_true_return) a.agent_true_return[col + q] = L > 0 ? st[q] : 0.0;
        if (HASV && a.mean_adv) a.mean_adv[col + q] = L > 0 ? sa[q] / (double)L : 0.0;
    }
    if (col == e * (size_t)a.N) a.ep_len[e] = L;                                   // the env's first column reports its length
}

template <int V, bool HASV>
__global__ void __launch_bounds__(256) episode_eval_kernel(const EvalArgs a)
{
    const ScanCols<V> c(a.E, a.N);
    const bool coop = c.within_stage();
    if (coop) eval_scan<true, V, HASV>(a, c.EN, c.col, c.e, c.e_first, c.de, c.act);
    else eval_scan<false, V, HASV>(a, c.EN, c.col, c.e, c.e_first, c.de, c.act);
}

// Per env: the collisions of the first episode and the means over agents, agents in ascending order.  One thread per (task,
// env) -- task 0 the collisions, 1 the return, 2 the true return -- so that the three sequential sums of an env run side by
// side; consecutive threads read consecutive n_coll entries at every step.
__global__ void __launch_bounds__(256) episode_env_kernel(const int32_t *__restrict__ n_coll, const int32_t *__restrict__ ep_len,
                                                          const double *__restrict__ agent_return, const double *__restrict__ agent_true_return,
                                                          int32_t *__restrict__ ep_collisions, double *__restrict__ ep_return,
                                                          double *__restrict__ ep_true_return, int E, int N)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * (size_t)E) return;
    const int task = (int)(idx / (size_t)E);
    const size_t e = idx - (size_t)task * E;
    if (task == 0) {
        if (!ep_collisions) return;
        const int L = ep_len[e];
        int c = 0;
        for (int t = 0; t < L; ++t) c += n_coll[(size_t)t * E + e];               // benchmark_agent.py:87
        ep_collisions[e] = c;
        return;
    }
    const double *src = task == 1 ? agent_return : agent_true_return;
    double *dst = task == 1 ? ep_return : ep_true_return;
    if (!dst) return;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < N; ++i) s += src[e * N + i];
    dst[e] = s / (double)N;                                                        // :85-86, :98-99
}

// ONE workgroup: it can write the counts itself (accumulate == 0) without a second launch or a memset node, and without a
// single atomic on global memory -- the bins are counted in LDS (integer atomics: order-independent) and flushed with plain
// stores.  Tables beyond kHistLds bins are counted in global memory by the same workgroup (zero, barrier, 64-bit atomics).
constexpr int kHistLds = 4096;
constexpr int kHistThreads = 1024;

__global__ void __launch_bounds__(kHistThreads) histogram_kernel(const int32_t *__restrict__ values, const uint8_t *__restrict__ valid,
                                                                 int E, int n_bins, long long *counts, int accumulate)
{
    __shared__ unsigned h[kHistLds];
    const int nb = n_bins + 1;
    const bool lds = nb <= kHistLds;                                               // (uniform)
    if (lds) {
        for (int b = threadIdx.x; b < nb; b += kHistThreads) h[b] = 0u;
    } else if (!accumulate) {
        for (int b = threadIdx.x; b < nb; b += kHistThreads) counts[b] = 0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < E; e += kHistThreads) {
        const int v = values[e];
        if (v >= 0 && (valid == nullptr || valid[e] != 0)) {
            const int b = v < n_bins ? v : n_bins;                                 // the last bin takes the overflow
            if (lds) atomicAdd(&h[b], 1u);
            else atomicAdd(reinterpret_cast<unsigned long long *>(counts + b), 1ull);
        }
    }
    if (!lds) return;
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kHistThreads) counts[b] = (accumulate ? counts[b] : 0ll) + (long long)h[b];
}

}   // namespace

extern "C" {

int dronesim_episode_eval(const float *reward, const float *true_reward, const int32_t *n_coll, const uint8_t *done,
                          const float *V, float gamma, int32_t *ep_len, int32_t *ep_collisions,
                          double *agent_return, double *agent_true_return, double *ep_return, double *ep_true_return,
                          float *G, double *mean_adv, int T, int E, int N, void *stream)
{
    if (!reward || !true_reward || !done || !ep_len || T < 0 || E < 0 || N < 1)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_eval: bad argument");
    if (ep_collisions && !n_coll) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_eval: ep_collisions needs n_coll");
    if (mean_adv && !V) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_eval: mean_adv needs V");
    if ((ep_return && !agent_return) || (ep_true_return && !agent_true_return))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_eval: ep_return / ep_true_return need agent_return / agent_true_return");
    if (E == 0) return DRONESIM_OK;
    const size_t cols = (size_t)E * N;
    EvalArgs a;
    a.reward = reward; a.true_reward = true_reward; a.V = mean_adv ? V : nullptr; a.done = done; a.G = G; a.ep_len = ep_len;
    a.agent_return = agent_return; a.agent_true_return = agent_true_return; a.mean_adv = mean_adv;
    a.gamma = gamma; a.T = T; a.E = E; a.N = N;
    // the returns scan's window for the column quadruples (scan_common.hpp has the measurements), over every [T][E N] array
    const bool v4 = column_quads(N, cols, 1048576, reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(true_reward) |
                                                   reinterpret_cast<uintptr_t>(a.V) | reinterpret_cast<uintptr_t>(G));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((v4 ? cols / 4 : cols) + 255) / 256));
    if (v4) {
        if (a.V) hipLaunchKernelGGL((episode_eval_kernel<4, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((episode_eval_kernel<4, false>), grid, dim3(256), 0, s, a);
    } else {
        if (a.V) hipLaunchKernelGGL((episode_eval_kernel<1, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((episode_eval_kernel<1, false>), grid, dim3(256), 0, s, a);
    }
    const int rc = dronesim_launched();
    if (rc != DRONESIM_OK || !(ep_collisions || ep_return || ep_true_return)) return rc;
    hipLaunchKernelGGL(episode_env_kernel, dim3((unsigned)((3 * (size_t)E + 255) / 256)), dim3(256), 0, s, n_coll, ep_len, agent_return,
                       agent_true_return, ep_collisions, ep_return, ep_true_return, E, N);
    return dronesim_launched();
}

int dronesim_histogram_i32(const int32_t *values, const uint8_t *valid, int E, int n_bins, int64_t *counts, int accumulate,
                           void *stream)
{
    if (!values || !counts || E < 0 || n_bins < 1 || n_bins > (1 << 24))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_histogram_i32: bad argument");
    hipLaunchKernelGGL(histogram_kernel, dim3(1), dim3(kHistThreads), 0, static_cast<hipStream_t>(stream), values, valid, E, n_bins,
                       reinterpret_cast<long long *>(counts), accumulate);
    return dronesim_launched();
}

}   // extern "C"
