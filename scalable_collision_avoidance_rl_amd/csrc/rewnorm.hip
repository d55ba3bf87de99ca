// Reward normalisation: the running discounted return of every (env, agent) column, its per-group running moments and the
// reward scale made from them, kept and applied on the device (include/dronesim.h: dronesim_rewnorm_workspace,
// dronesim_rewnorm_update, dronesim_rewnorm_apply).  Return-based reward scaling: no mean is subtracted.
#include "scan_common.hpp"
#include "dronesim.h"

#include <math.h>
#include <stdio.h>

namespace {

// update, launch 1 (rewnorm_scan_kernel): a FORWARD scan over the stored window reward [T][E N], one thread per column on
// scan_common.hpp's types (ScanCols<1>, DoneStage with the step order t0 + u), float64 throughout:
//     R <- fma(gamma, R, r[t]);   R counted if finite;   R <- 0 behind done[t]
// with R carried in from ret [E][N] and written back.  The counted values are accumulated without a division per step as the
// shifted sums n, sum (R - K), sum (R - K)^2 with K the column's first counted value (a value of the column: a carry of 1e6
// +- 1 keeps its variance), converted ONCE to (n, mean = K + s1 / n, m2 = s2 - s1^2 / n) and written to ws [3][E N].
// The carry is NOT repaired: a NaN or +-inf reward makes R non-finite, and it stays so (gamma inf = inf, gamma NaN = NaN,
// 0 inf = NaN) until the column's next `done`; those steps are simply not counted.
// The loop is staged like the backward scans and software-pipelined like them: the rows and flags of stage s + 1 are
// requested before stage s is folded.  Here that matters more than there -- the fold of a step is a dependent chain of
// float64 operations (fma, subtract, add, fma), so a wave that waits for its stage first and folds afterwards leaves the
// memory system idle for the length of eight such chains per stage.  Measured, whole update, alternating builds in one
// session (T = 200): request - wait - fold took 93.3 us at 4096 envs x 64 agents against 89.2 / 86.9 pipelined, and 79.7 us at
// 512 x 256 (one group per agent) against 72.0 / 73.6.
// update, launch 2 (rewnorm_env_fold_kernel): one workgroup per agent; lane r folds a contiguous ascending run of envs with
// Chan's rule, one fixed LDS tree folds the runs: the agent's triple, ws2 [3][N].
// update, launch 3 (rewnorm_group_kernel): one workgroup; lane g folds the agents of group g in ascending order with Chan's
// rule, merges the window's triple into state [3][G] and makes the group's scale; then scale [N] is rewritten from it.
// Every order is a function of (T, E, N, group) only; no atomics, no memset, nothing allocated.
// scale_g = 1 / sqrt(m2_g / count_g + eps), and 1 where count_g = 0 OR where m2_g / count_g + eps == 0: unlike the
// observation table (inv = 0 there: a constant input column carries nothing), a zero scale would erase the reward signal.
constexpr int kRnThreads = 256;
constexpr size_t kRnStreamBytes = (size_t)32 << 20;     // apply: non-temporal accesses from this window size on
constexpr int kRnRows = 8;                              // apply: time steps per thread

__device__ __forceinline__ void rn_merge(double &na, double &ma, double &qa, double nb, double mb, double qb)
{
    if (nb == 0.0) return;
    if (na == 0.0) { na = nb; ma = mb; qa = qb; return; }
    const double n = na + nb, d = mb - ma, f = nb / n;
    ma = fma(d, f, ma);
    qa = qa + qb + d * d * na * f;
    na = n;
}

struct RnStage {
    float r[kStageT];
    DoneStage ds;
    bool end[kStageT];
};

template <bool COOP>
__device__ __forceinline__ void rn_fetch(RnStage &st, const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                         size_t EN, size_t col, size_t e, size_t e_first, int E, int T, int t0)
{
    if (COOP) st.ds.fetch(done, e_first, E, T, [&](int u) { return t0 + u; });
#pragma unroll
    for (int u = 0; u < kStageT; ++u) {
        const int t = t0 + u;
        st.r[u] = t < T ? __builtin_nontemporal_load(reward + (size_t)t * EN + col) : 0.0f;
        if (!COOP) st.end[u] = t < T && done[(size_t)t * E + e] != 0;
    }
}

template <bool COOP>
__device__ __forceinline__ void rn_scan(const float *__restrict__ reward, const uint8_t *__restrict__ done, double gamma,
                                        double *__restrict__ ret, double *__restrict__ ws, int T, int E, size_t EN, size_t col,
                                        size_t e, size_t e_first, int de, bool act)
{
    RnStage cur, nxt;
    rn_fetch<COOP>(cur, reward, done, EN, col, e, e_first, E, T, 0);
    double R = ret[col], n = 0.0, K = 0.0, s1 = 0.0, s2 = 0.0;
    for (int t0 = 0; t0 < T; t0 += kStageT) {
        if (t0 + kStageT < T) rn_fetch<COOP>(nxt, reward, done, EN, col, e, e_first, E, T, t0 + kStageT);
#pragma unroll
        for (int u = 0; u < kStageT; ++u) {
            if (t0 + u < T) {                                           // (wave-uniform: the flag pick is a wave operation)
                const bool end = COOP ? cur.ds.get(de, u) : cur.end[u];
                R = fma(gamma, R, (double)cur.r[u]);
                const bool fin = __builtin_isfinite(R);
                K = (fin && n == 0.0) ? R : K;
                const double d = fin ? R - K : 0.0;
                n += fin ? 1.0 : 0.0;
                s1 += d;
                s2 = fma(d, d, s2);
                R = end ? 0.0 : R;
            }
        }
        cur = nxt;
    }
    if (!act) return;
    ret[col] = R;
    const bool any = n > 0.0;
    ws[col] = n;
    ws[EN + col] = any ? K + s1 / n : 0.0;
    ws[2 * EN + col] = any ? fmax(s2 - s1 * s1 / n, 0.0) : 0.0;
}

__global__ void __launch_bounds__(kRnThreads) rewnorm_scan_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                                   double gamma, double *__restrict__ ret, double *__restrict__ ws,
                                                                   int T, int E, int N)
{
    const ScanCols<1> c(E, N);
    if (c.within_stage()) rn_scan<true>(reward, done, gamma, ret, ws, T, E, c.EN, c.col, c.e, c.e_first, c.de, c.act);
    else rn_scan<false>(reward, done, gamma, ret, ws, T, E, c.EN, c.col, c.e, c.e_first, c.de, c.act);
}

// ws [3][E N] -> ws2 [3][N]: workgroup i is agent i, lane r the envs [r per, (r + 1) per)
__global__ void __launch_bounds__(kRnThreads) rewnorm_env_fold_kernel(const double *__restrict__ ws, double *__restrict__ ws2, int E, int N)
{
    __shared__ double pn[kRnThreads], pm[kRnThreads], pq[kRnThreads];
    const int r = threadIdx.x, i = blockIdx.x;
    const size_t EN = (size_t)E * N;
    const int per = (E + kRnThreads - 1) / kRnThreads;
    const long long lo = (long long)r * per, hi = lo + per < E ? lo + per : E;
    double n = 0.0, m = 0.0, q = 0.0;
    for (long long e = lo; e < hi; ++e) {
        const size_t c = (size_t)e * N + i;
        rn_merge(n, m, q, ws[c], ws[EN + c], ws[2 * EN + c]);
    }
    pn[r] = n; pm[r] = m; pq[r] = q;
    for (int w = kRnThreads >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (r < w) rn_merge(pn[r], pm[r], pq[r], pn[r + w], pm[r + w], pq[r + w]);
    }
    if (r != 0) return;
    ws2[i] = pn[0];
    ws2[N + i] = pm[0];
    ws2[2 * (size_t)N + i] = pq[0];
}

// ws2 [3][N] -> state [3][G], scale [N]; gs [G]: the groups' scales on their way to the agents (workspace)
__global__ void __launch_bounds__(kRnThreads) rewnorm_group_kernel(const double *__restrict__ ws2, const int *__restrict__ group,
                                                                    int n_groups, int N, double *__restrict__ state,
                                                                    double *__restrict__ gs, double *__restrict__ scale, double eps)
{
    // the agents' triples pass through LDS in chunks of kRnThreads: the one lane that folds a group of 256 agents took 43 us
    // reading them from memory and takes 26 with them in LDS (what is left is its chain of 256 merges, a division each; a
    // branch-free division-free fold was slower, every lane then does the arithmetic of every agent: DESIGN.md)
    __shared__ double an[kRnThreads], am[kRnThreads], aq[kRnThreads];
    __shared__ int ag[kRnThreads];
    const int tid = threadIdx.x;
    for (int gb = 0; gb < n_groups; gb += kRnThreads) {
        const int g = gb + tid;
        double n = 0.0, m = 0.0, q = 0.0;
        for (int c0 = 0; c0 < N; c0 += kRnThreads) {
            __syncthreads();
            if (c0 + tid < N) {
                const int i = c0 + tid;
                an[tid] = ws2[i]; am[tid] = ws2[N + i]; aq[tid] = ws2[2 * (size_t)N + i];
                ag[tid] = group ? group[i] : 0;
            }
            __syncthreads();
            const int cnt = N - c0 < kRnThreads ? N - c0 : kRnThreads;
            if (g < n_groups)
                for (int j = 0; j < cnt; ++j)
                    if (ag[j] == g) rn_merge(n, m, q, an[j], am[j], aq[j]);
        }
        if (g >= n_groups) continue;
        double sn = state[g], sm = state[n_groups + g], sq = state[2 * (size_t)n_groups + g];
        if (n > 0.0) {                                                   // (a group without a counted value keeps its state's bits)
            rn_merge(sn, sm, sq, n, m, q);
            state[g] = sn;
            state[n_groups + g] = sm;
            state[2 * (size_t)n_groups + g] = sq;
        }
        const double var = sn > 0.0 ? sq / sn + eps : 0.0;
        gs[g] = var > 0.0 ? 1.0 / sqrt(var) : 1.0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += kRnThreads) {
        const int g = group ? group[i] : 0;
        scale[i] = (g >= 0 && g < n_groups) ? gs[g] : 1.0;               // (ids are the caller's to validate; never read outside gs)
    }
}

// out[t][c] = (float)((double)reward[t][c] scale[c % N]), clamped: thread x owns V adjacent columns and kRnRows steps
template <int V, bool NT>
__global__ void __launch_bounds__(kRnThreads) rewnorm_apply_kernel(const float *reward, float *out, const double *__restrict__ scale,
                                                                    int T, size_t EN, int N, float lim)
{
    typedef typename ColVec<V>::type vec;
    const size_t col = ((size_t)blockIdx.x * kRnThreads + threadIdx.x) * V;
    if (col >= EN) return;
    double s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = scale[(col + k) % N];
    const int t_lo = blockIdx.y * kRnRows, t_hi = t_lo + kRnRows < T ? t_lo + kRnRows : T;
    vec v[kRnRows];
#pragma unroll
    for (int j = 0; j < kRnRows; ++j) {
        if (t_lo + j < t_hi) {
            const vec *p = reinterpret_cast<const vec *>(reward + (size_t)(t_lo + j) * EN + col);
            v[j] = NT ? __builtin_nontemporal_load(p) : *p;
        }
    }
#pragma unroll
    for (int j = 0; j < kRnRows; ++j) {
        if (t_lo + j < t_hi) {
            float *f = reinterpret_cast<float *>(&v[j]);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float u = (float)((double)f[k] * s[k]);
                f[k] = u > lim ? lim : (u < -lim ? -lim : u);            // (comparisons: NaN stays NaN; lim = +inf never clamps)
            }
            vec *p = reinterpret_cast<vec *>(out + (size_t)(t_lo + j) * EN + col);
            if (NT) __builtin_nontemporal_store(v[j], p);
            else *p = v[j];
        }
    }
}

int rn_shape(const char *who, int T, int E, int N)
{
    static thread_local char msg[160];
    if (T >= 1 && E >= 1 && N >= 1) return DRONESIM_OK;
    snprintf(msg, sizeof msg, "%s: T, E and N must be >= 1, got %d, %d, %d", who, T, E, N);
    return dronesim_fail(DRONESIM_EINVAL, msg);
}

// ws: [3][E N] column triples | [3][N] agent triples | [N] group scales, doubles
size_t rn_ws_bytes(int E, int N) { return (3 * (size_t)E * N + 4 * (size_t)N) * sizeof(double); }

}  // namespace

extern "C" int dronesim_rewnorm_workspace(int T, int E, int N, size_t *bytes)
{
    if (const int rc = rn_shape("dronesim_rewnorm_workspace", T, E, N)) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_workspace: NULL bytes");
    *bytes = rn_ws_bytes(E, N);
    return DRONESIM_OK;
}

extern "C" int dronesim_rewnorm_update(const float *reward, const uint8_t *done, int T, int E, int N, double gamma, const int *group,
                                       int n_groups, double *ret, double *state, double *scale, double eps, void *ws, size_t ws_bytes,
                                       void *stream)
{
    if (const int rc = rn_shape("dronesim_rewnorm_update", T, E, N)) return rc;
    if (!reward || !done || !ret || !state || !scale || !ws)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: NULL reward / done / ret / state / scale / workspace");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: gamma must be in [0, 1]");
    if (!(eps >= 0.0) || isinf(eps)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: eps must be finite and >= 0");
    if (n_groups < 1 || n_groups > N) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: n_groups must be in [1, N]");
    if (!group && n_groups != 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: a NULL group map needs n_groups = 1");
    if (ws_bytes < rn_ws_bytes(E, N))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: the workspace is smaller than dronesim_rewnorm_workspace's size");
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_update: the workspace is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t EN = (size_t)E * N;
    double *w = (double *)ws, *w2 = w + 3 * EN, *gs = w2 + 3 * (size_t)N;
    hipLaunchKernelGGL(rewnorm_scan_kernel, dim3((unsigned)((EN + kRnThreads - 1) / kRnThreads)), dim3(kRnThreads), 0, st, reward, done,
                       gamma, ret, w, T, E, N);
    hipLaunchKernelGGL(rewnorm_env_fold_kernel, dim3((unsigned)N), dim3(kRnThreads), 0, st, w, w2, E, N);
    hipLaunchKernelGGL(rewnorm_group_kernel, dim3(1), dim3(kRnThreads), 0, st, w2, group, n_groups, N, state, gs, scale, eps);
    return dronesim_launched();
}

extern "C" int dronesim_rewnorm_apply(const float *reward, float *out, int T, int E, int N, const double *scale, float clip, void *stream)
{
    if (const int rc = rn_shape("dronesim_rewnorm_apply", T, E, N)) return rc;
    if (!reward || !out || !scale) return dronesim_fail(DRONESIM_EINVAL, "dronesim_rewnorm_apply: NULL reward / out / scale");
    const float lim = clip > 0.f ? clip : INFINITY;                      // (clip <= 0, NaN or +inf: no clamp)
    const size_t EN = (size_t)E * N;
    const bool nt = (size_t)T * EN * sizeof(float) >= kRnStreamBytes;
    const bool v4 = (EN % 4) == 0 && ((reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    const size_t lanes = v4 ? EN / 4 : EN;
    const dim3 grid((unsigned)((lanes + kRnThreads - 1) / kRnThreads), (unsigned)((T + kRnRows - 1) / kRnRows)), block(kRnThreads);
    hipStream_t st = (hipStream_t)stream;
    if (v4 && nt) hipLaunchKernelGGL((rewnorm_apply_kernel<4, true>), grid, block, 0, st, reward, out, scale, T, EN, N, lim);
    else if (v4) hipLaunchKernelGGL((rewnorm_apply_kernel<4, false>), grid, block, 0, st, reward, out, scale, T, EN, N, lim);
    else if (nt) hipLaunchKernelGGL((rewnorm_apply_kernel<1, true>), grid, block, 0, st, reward, out, scale, T, EN, N, lim);
    else hipLaunchKernelGGL((rewnorm_apply_kernel<1, false>), grid, block, 0, st, reward, out, scale, T, EN, N, lim);
    return dronesim_launched();
}
