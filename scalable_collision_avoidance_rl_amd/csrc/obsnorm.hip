// Observation normalisation: running per-column mean and variance of float32 row matrices, kept and applied on the device
// (include/dronesim.h: dronesim_obsnorm_workspace, dronesim_obsnorm_update, dronesim_obsnorm_apply): float64 sums over the finite
// values, Chan's merge, fixed order.
#include "colstats_common.hpp"
#include "../../include/dronesim.h"

#include <math.h>

namespace {

// x [R][C], C = N d_in columns, over the decomposition of colstats_common.hpp (lane groups, column tiles, slabs, the lane map, the tree).
// update, launch 1 (obsnorm_sums_kernel): a lane shifts every column of its own by K, the first FINITE value it meets there (0 while
// it has met none: the shift is a value of the column, so -500 +- 0.5 keeps its variance, and it is never NaN or inf), and
// accumulates in double, over the finite values only, their count and the sums of d = x - K and of d^2.  After the loop the lane
// holds (n, mean = K + sum d / n, M2 = sum d^2 - (sum d)^2 / n); ONE fixed LDS tree folds the q lanes of a column with Chan's rule
// into the slab's triple, ws [S][3][C] doubles.
// update, launch 2 (obsnorm_merge_kernel): a workgroup takes 32 columns; lane (run, column) folds a contiguous run of slabs in
// ascending order, a fixed tree folds the 32 runs, and lane (0, column) merges the window's triple into the state and rewrites
// the table.  An all-equal column has K = c and d = 0 in every lane, every mean c and every delta 0: mean = c and M2 = 0 exactly.
// apply (obsnorm_apply_kernel): the same lane-to-element map; the lane's table entries are read once, outside the row loop.
constexpr int kOnCols = 32;
// the window-sized apply streams (non-temporal accesses, as the return scans); a step's observation stays cached for the policy
constexpr size_t kOnStreamBytes = (size_t)32 << 20;

// Chan's rule: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb); counts are doubles holding exact integers; an empty side changes nothing
__device__ __forceinline__ void on_merge(double &na, double &ma, double &qa, double nb, double mb, double qb)
{
    if (nb == 0.0) return;
    if (na == 0.0) { na = nb; ma = mb; qa = qb; return; }
    const double n = na + nb, d = mb - ma, f = nb / n;
    ma = fma(d, f, ma);
    qa = qa + qb + d * d * na * f;
    na = n;
}

template <int V, bool VEC>
__global__ __launch_bounds__(kColThreads) void obsnorm_sums_kernel(const float *__restrict__ x, double *__restrict__ ws, int R, int C,
                                                                   int tw, int q, int qp, long long rps)
{
    __shared__ double bn[kColThreads][V], bm[kColThreads][V], bq[kColThreads][V];
    const int t = threadIdx.x;
    ColLane<V> lane(tw, q, C);
    const bool lane_on = lane.on();
    lane.slab(rps, R);
    double cnt[V], k0[V], sd[V], sd2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) cnt[k] = k0[k] = sd[k] = sd2[k] = 0.0;
    if (lane_on && lane.has_rows()) {
        const float *p = x + (size_t)lane.row() * C + lane.col();
        const size_t step = lane.step();
        const long long n = lane.n();
#pragma unroll 4
        for (long long j = 0; j < n; ++j) {
            float v[V];
            col_load<V, VEC, false>(p + j * step, v);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const bool fin = __builtin_isfinite(v[k]);
                k0[k] = (fin && cnt[k] == 0.0) ? (double)v[k] : k0[k];
                const double d = fin ? (double)v[k] - k0[k] : 0.0;
                cnt[k] += fin ? 1.0 : 0.0;
                sd[k] += d;
                sd2[k] = fma(d, d, sd2[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const bool any = cnt[k] > 0.0;
        bn[t][k] = cnt[k];
        bm[t][k] = any ? k0[k] + sd[k] / cnt[k] : 0.0;
        bq[t][k] = any ? fmax(sd2[k] - sd[k] * sd[k] / cnt[k], 0.0) : 0.0;
    }
    col_tree(lane_on, lane.rl, tw, q, qp, [&](int a, int b) {
#pragma unroll
        for (int k = 0; k < V; ++k) on_merge(bn[a][k], bm[a][k], bq[a][k], bn[b][k], bm[b][k], bq[b][k]);
    }, [&](int self) {
        double *o = ws + (size_t)blockIdx.x * 3 * C + lane.col();
#pragma unroll
        for (int k = 0; k < V; ++k) {
            o[k] = bn[self][k];
            o[C + k] = bm[self][k];
            o[2 * (size_t)C + k] = bq[self][k];
        }
    });
}

__global__ __launch_bounds__(kColThreads) void obsnorm_merge_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                                    double *__restrict__ table, int C, int S, double eps)
{
    __shared__ double pn[kColThreads], pm[kColThreads], pq[kColThreads];
    const int t = threadIdx.x, run = t / kOnCols, c = blockIdx.x * kOnCols + t % kOnCols;
    const ColRun r = col_run(kColRuns, run, S);
    double n = 0.0, m = 0.0, m2 = 0.0;
    if (c < C) {
        for (int s = r.s_lo; s < r.s_hi; ++s) {
            const double *w = ws + (size_t)s * 3 * C + c;
            on_merge(n, m, m2, w[0], w[C], w[2 * (size_t)C]);
        }
    }
    pn[t] = n; pm[t] = m; pq[t] = m2;
    for (int w = kColRuns >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (run < w) on_merge(pn[t], pm[t], pq[t], pn[t + w * kOnCols], pm[t + w * kOnCols], pq[t + w * kOnCols]);
    }
    if (run != 0 || c >= C) return;
    double sn = state[c], sm = state[C + c], sq = state[2 * (size_t)C + c];
    if (pn[t] > 0.0) {                                                   // (a column without a finite value keeps its state's bits)
        on_merge(sn, sm, sq, pn[t], pm[t], pq[t]);
        state[c] = sn;
        state[C + c] = sm;
        state[2 * (size_t)C + c] = sq;
    }
    const double var = sn > 0.0 ? sq / sn + eps : 0.0;
    table[c] = sn > 0.0 ? sm : 0.0;
    table[C + c] = sn > 0.0 ? (var > 0.0 ? 1.0 / sqrt(var) : 0.0) : 1.0;
}

template <int V, bool VEC, bool NT>
__global__ __launch_bounds__(kColThreads) void obsnorm_apply_kernel(const float *x, float *y, const double *__restrict__ table, int R,
                                                                    int C, int tw, int q, long long rps, float lim)
{
    ColLane<V> lane(tw, q, C);
    lane.slab(rps, R);
    if (!(lane.on() && lane.has_rows())) return;
    double mean[V], inv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { mean[k] = table[(size_t)lane.g * V + k]; inv[k] = table[(size_t)C + (size_t)lane.g * V + k]; }
    const size_t at = lane.at(), step = lane.step();
    const long long n = lane.n();
#pragma unroll 4
    for (long long j = 0; j < n; ++j) {
        float v[V];
        col_load<V, VEC, NT>(x + at + j * step, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float u = (float)(((double)v[k] - mean[k]) * inv[k]);
            v[k] = u > lim ? lim : (u < -lim ? -lim : u);                // (comparisons: NaN stays NaN; lim = +inf never clamps)
        }
        col_store<V, VEC, NT>(y + at + j * step, v);
    }
}

}  // namespace

extern "C" int dronesim_obsnorm_workspace(int R, int C, size_t *bytes)
{
    ColPlan p;
    if (const int rc = col_validate("dronesim_obsnorm_workspace", 'C', R, C, bytes ? nullptr : "NULL bytes", nullptr, &p)) return rc;
    *bytes = col_ws_bytes(p, 3, C);
    return DRONESIM_OK;
}

extern "C" int dronesim_obsnorm_update(const float *x, int R, int C, double *state, double *table, double eps, void *ws, size_t ws_bytes,
                                       void *stream)
{
    ColPlan p;
    if (const int rc = col_validate("dronesim_obsnorm_update", 'C', R, C, x && state && table && ws ? nullptr : "NULL x / state / table / workspace",
                                    eps >= 0.0 ? nullptr : "eps must be >= 0", &p, {"dronesim_obsnorm_workspace", 3, ws, ws_bytes}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int qp = col_qp(p.q);
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles), block(kColThreads);
    double *w = (double *)ws;
    col_dispatch(p, reinterpret_cast<uintptr_t>(x), [&](auto V, auto VEC) {
        hipLaunchKernelGGL((obsnorm_sums_kernel<V(), VEC()>), grid, block, 0, st, x, w, R, C, p.tw, p.q, qp, p.rps);
    });
    hipLaunchKernelGGL(obsnorm_merge_kernel, dim3((unsigned)((C + kOnCols - 1) / kOnCols)), block, 0, st, w, state, table, C, p.S, eps);
    return dronesim_launched();
}

extern "C" int dronesim_obsnorm_apply(const float *x, float *y, int R, int C, const double *table, float clip, void *stream)
{
    ColPlan p;
    if (const int rc = col_validate("dronesim_obsnorm_apply", 'C', R, C, x && y && table ? nullptr : "NULL x / y / table", nullptr, &p)) return rc;
    const float lim = clip > 0.f ? clip : INFINITY;                      // (clip <= 0, NaN or +inf: no clamp)
    const bool nt = (size_t)R * (size_t)C * sizeof(float) >= kOnStreamBytes;
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles), block(kColThreads);
    hipStream_t st = (hipStream_t)stream;
    col_dispatch(p, reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y), [&](auto V, auto VEC) {
        if (nt) hipLaunchKernelGGL((obsnorm_apply_kernel<V(), VEC(), true>), grid, block, 0, st, x, y, table, R, C, p.tw, p.q, p.rps, lim);
        else hipLaunchKernelGGL((obsnorm_apply_kernel<V(), VEC(), false>), grid, block, 0, st, x, y, table, R, C, p.tw, p.q, p.rps, lim);
    });
    return dronesim_launched();
}
