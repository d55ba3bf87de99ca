// Observation normalisation: running per-column mean and variance of float32 row matrices, kept and applied on the device
// (include/dronesim.h: dronesim_obsnorm_workspace, dronesim_obsnorm_update, dronesim_obsnorm_apply): float64 sums over the finite
// values, Chan's merge, fixed order.
#include "common.hpp"
#include "../../include/dronesim.h"

#include <math.h>

namespace {

// x [R][C], C = N d_in columns.  The decomposition is standardize.hip's (`std_plan`), a function of (R, C) only:
//   lane group   V = 4 adjacent columns where C % 4 == 0 (one 16-byte access where the pointers allow it), else 1
//   column tile  `tw` lane groups: 16 (64 floats) where C % 64 == 0, else the whole row, capped at 1024 lanes
//   iteration    a workgroup of 1024 lanes covers q = 1024 / tw rows of its tile at once: lane t holds row t / tw, group t % tw, and
//                meets the same columns in every iteration
//   slab         `rps` rows (a multiple of q); S slabs x tiles workgroups aim at kOnBlocks, one per CU
// update, launch 1 (obsnorm_sums_kernel): a lane shifts every column of its own by K, the first FINITE value it meets there (0 while
// it has met none: the shift is a value of the column, so -500 +- 0.5 keeps its variance, and it is never NaN or inf), and
// accumulates in double, over the finite values only, their count and the sums of d = x - K and of d^2.  After the loop the lane
// holds (n, mean = K + sum d / n, M2 = sum d^2 - (sum d)^2 / n); ONE fixed LDS tree folds the q lanes of a column with Chan's rule
// into the slab's triple, ws [S][3][C] doubles.
// update, launch 2 (obsnorm_merge_kernel): a workgroup takes 32 columns; lane (run, column) folds a contiguous run of slabs in
// ascending order, a fixed tree folds the 32 runs, and lane (0, column) merges the window's triple into the state and rewrites
// the table.  An all-equal column has K = c and d = 0 in every lane, every mean c and every delta 0: mean = c and M2 = 0 exactly.
// apply (obsnorm_apply_kernel): the same lane-to-element map; the lane's table entries are read once, outside the row loop.
constexpr int kOnThreads = 1024, kOnBlocks = 256, kOnRuns = 32, kOnCols = 32;
// the window-sized apply streams (non-temporal accesses, as the return scans); a step's observation stays cached for the policy
constexpr size_t kOnStreamBytes = (size_t)32 << 20;

struct OnPlan {
    int V, tw, tiles, q, S;
    long long rps;
};

OnPlan on_plan(int R, int C)
{
    OnPlan p;
    p.V = C % 4 == 0 ? 4 : 1;
    const int nv = C / p.V, cap = kOnThreads / p.V;
    p.tw = (p.V == 4 && C % 64 == 0) ? 16 : (nv <= cap ? nv : cap);
    p.tiles = (nv + p.tw - 1) / p.tw;
    p.q = kOnThreads / p.tw;
    const long long iters = ((long long)R + p.q - 1) / p.q;
    long long want = kOnBlocks / p.tiles;
    want = want < 1 ? 1 : (want > iters ? iters : want);
    p.rps = ((iters + want - 1) / want) * p.q;
    p.S = (int)(((long long)R + p.rps - 1) / p.rps);
    return p;
}

typedef float on_f4 __attribute__((ext_vector_type(4)));

template <int V, bool VEC, bool NT>
__device__ __forceinline__ void on_load(const float *p, float (&v)[V])
{
    if (VEC) {
        const on_f4 f = NT ? __builtin_nontemporal_load(reinterpret_cast<const on_f4 *>(p)) : *reinterpret_cast<const on_f4 *>(p);
        v[0] = f.x; v[V > 1 ? 1 : 0] = f.y; v[V > 2 ? 2 : 0] = f.z; v[V > 3 ? 3 : 0] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = NT ? __builtin_nontemporal_load(p + k) : p[k];
    }
}

template <int V, bool VEC, bool NT>
__device__ __forceinline__ void on_store(float *o, const float (&v)[V])
{
    if (VEC) {
        on_f4 f;
        f.x = v[0]; f.y = v[V > 1 ? 1 : 0]; f.z = v[V > 2 ? 2 : 0]; f.w = v[V > 3 ? 3 : 0];
        if (NT) __builtin_nontemporal_store(f, reinterpret_cast<on_f4 *>(o));
        else *reinterpret_cast<on_f4 *>(o) = f;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (NT) __builtin_nontemporal_store(v[k], o + k);
            else o[k] = v[k];
        }
    }
}

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
__global__ __launch_bounds__(kOnThreads) void obsnorm_sums_kernel(const float *__restrict__ x, double *__restrict__ ws, int R, int C,
                                                                  int tw, int q, int qp, long long rps)
{
    __shared__ double bn[kOnThreads][V], bm[kOnThreads][V], bq[kOnThreads][V];
    const int t = threadIdx.x, rl = t / tw, g = blockIdx.y * tw + t % tw;
    const bool lane_on = rl < q && g * V < C;
    const long long r_begin = (long long)blockIdx.x * rps;
    const long long r_end = r_begin + rps < R ? r_begin + rps : R;
    double cnt[V], k0[V], sd[V], sd2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) cnt[k] = k0[k] = sd[k] = sd2[k] = 0.0;
    if (lane_on && r_begin + rl < r_end) {
        const float *p = x + (size_t)(r_begin + rl) * C + (size_t)g * V;
        const size_t step = (size_t)q * C;
        const long long n = (r_end - r_begin - rl + q - 1) / q;
#pragma unroll 4
        for (long long j = 0; j < n; ++j) {
            float v[V];
            on_load<V, VEC, false>(p + j * step, v);
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
    // fixed tree over the q lanes (rows) of a column: b[t] <- b[t] + b[t + w tw], w = qp / 2 .. 1 (qp = q rounded up to 2^n)
    for (int w = qp >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (lane_on && rl < w && rl + w < q) {
#pragma unroll
            for (int k = 0; k < V; ++k) on_merge(bn[t][k], bm[t][k], bq[t][k], bn[t + w * tw][k], bm[t + w * tw][k], bq[t + w * tw][k]);
        }
    }
    if (lane_on && rl == 0) {                                            // (its own entries: the last level's writer)
        double *o = ws + (size_t)blockIdx.x * 3 * C + (size_t)g * V;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            o[k] = bn[t][k];
            o[C + k] = bm[t][k];
            o[2 * (size_t)C + k] = bq[t][k];
        }
    }
}

__global__ __launch_bounds__(kOnThreads) void obsnorm_merge_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                                   double *__restrict__ table, int C, int S, double eps)
{
    __shared__ double pn[kOnThreads], pm[kOnThreads], pq[kOnThreads];
    const int t = threadIdx.x, run = t / kOnCols, c = blockIdx.x * kOnCols + t % kOnCols;
    const int ch = (S + kOnRuns - 1) / kOnRuns;
    const int s_lo = run * ch, s_hi = (s_lo + ch) < S ? (s_lo + ch) : S;
    double n = 0.0, m = 0.0, m2 = 0.0;
    if (c < C) {
        for (int s = s_lo; s < s_hi; ++s) {
            const double *w = ws + (size_t)s * 3 * C + c;
            on_merge(n, m, m2, w[0], w[C], w[2 * (size_t)C]);
        }
    }
    pn[t] = n; pm[t] = m; pq[t] = m2;
    for (int w = kOnRuns >> 1; w > 0; w >>= 1) {
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
__global__ __launch_bounds__(kOnThreads) void obsnorm_apply_kernel(const float *x, float *y, const double *__restrict__ table, int R,
                                                                   int C, int tw, int q, long long rps, float lim)
{
    const int t = threadIdx.x, rl = t / tw, g = blockIdx.y * tw + t % tw;
    const long long r_begin = (long long)blockIdx.x * rps;
    const long long r_end = r_begin + rps < R ? r_begin + rps : R;
    if (!(rl < q && g * V < C && r_begin + rl < r_end)) return;
    double mean[V], inv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { mean[k] = table[(size_t)g * V + k]; inv[k] = table[(size_t)C + (size_t)g * V + k]; }
    const size_t at = (size_t)(r_begin + rl) * C + (size_t)g * V, step = (size_t)q * C;
    const long long n = (r_end - r_begin - rl + q - 1) / q;
#pragma unroll 4
    for (long long j = 0; j < n; ++j) {
        float v[V];
        on_load<V, VEC, NT>(x + at + j * step, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float u = (float)(((double)v[k] - mean[k]) * inv[k]);
            v[k] = u > lim ? lim : (u < -lim ? -lim : u);                // (comparisons: NaN stays NaN; lim = +inf never clamps)
        }
        on_store<V, VEC, NT>(y + at + j * step, v);
    }
}

template <int V, bool VEC>
void on_launch_apply(bool nt, dim3 grid, hipStream_t st, const float *x, float *y, const double *table, int R, int C, const OnPlan &p,
                     float lim)
{
    if (nt) hipLaunchKernelGGL((obsnorm_apply_kernel<V, VEC, true>), grid, dim3(kOnThreads), 0, st, x, y, table, R, C, p.tw, p.q, p.rps, lim);
    else hipLaunchKernelGGL((obsnorm_apply_kernel<V, VEC, false>), grid, dim3(kOnThreads), 0, st, x, y, table, R, C, p.tw, p.q, p.rps, lim);
}

}  // namespace

extern "C" int dronesim_obsnorm_workspace(int R, int C, size_t *bytes)
{
    if (R < 1 || C < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_workspace: R < 1 or C < 1");
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_workspace: NULL bytes");
    *bytes = sizeof(double) * 3 * (size_t)on_plan(R, C).S * (size_t)C;
    return DRONESIM_OK;
}

extern "C" int dronesim_obsnorm_update(const float *x, int R, int C, double *state, double *table, double eps, void *ws, size_t ws_bytes,
                                       void *stream)
{
    if (R < 1 || C < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_update: R < 1 or C < 1");
    if (!x || !state || !table || !ws) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_update: NULL x / state / table / workspace");
    if (!(eps >= 0.0)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_update: eps must be >= 0");
    const OnPlan p = on_plan(R, C);
    if (ws_bytes < sizeof(double) * 3 * (size_t)p.S * (size_t)C)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_update: workspace smaller than dronesim_obsnorm_workspace()");
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_update: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int qp = 1;
    while (qp < p.q) qp <<= 1;
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles), block(kOnThreads);
    double *w = (double *)ws;
    // 16-byte reads where every lane group starts 16-byte aligned; the lanes' columns and rows do not depend on it
    if (p.V == 4 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0)
        hipLaunchKernelGGL((obsnorm_sums_kernel<4, true>), grid, block, 0, st, x, w, R, C, p.tw, p.q, qp, p.rps);
    else if (p.V == 4)
        hipLaunchKernelGGL((obsnorm_sums_kernel<4, false>), grid, block, 0, st, x, w, R, C, p.tw, p.q, qp, p.rps);
    else
        hipLaunchKernelGGL((obsnorm_sums_kernel<1, false>), grid, block, 0, st, x, w, R, C, p.tw, p.q, qp, p.rps);
    hipLaunchKernelGGL(obsnorm_merge_kernel, dim3((unsigned)((C + kOnCols - 1) / kOnCols)), block, 0, st, w, state, table, C, p.S, eps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}

extern "C" int dronesim_obsnorm_apply(const float *x, float *y, int R, int C, const double *table, float clip, void *stream)
{
    if (R < 1 || C < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_apply: R < 1 or C < 1");
    if (!x || !y || !table) return dronesim_fail(DRONESIM_EINVAL, "dronesim_obsnorm_apply: NULL x / y / table");
    const OnPlan p = on_plan(R, C);
    const float lim = clip > 0.f ? clip : INFINITY;                      // (clip <= 0, NaN or +inf: no clamp)
    const bool nt = (size_t)R * (size_t)C * sizeof(float) >= kOnStreamBytes;
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles);
    hipStream_t st = (hipStream_t)stream;
    if (p.V == 4 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0)
        on_launch_apply<4, true>(nt, grid, st, x, y, table, R, C, p, lim);
    else if (p.V == 4)
        on_launch_apply<4, false>(nt, grid, st, x, y, table, R, C, p, lim);
    else
        on_launch_apply<1, false>(nt, grid, st, x, y, table, R, C, p, lim);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}
