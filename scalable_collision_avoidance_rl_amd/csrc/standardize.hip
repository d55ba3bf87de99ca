// Per-agent standardisation of a window of values, the PPO learner's advantages (include/dronesim.h: dronesim_standardize_workspace,
// dronesim_standardize): float64 sums, two launches, fixed order.
#include "common.hpp"
#include "../../include/dronesim.h"

#include <math.h>

namespace {

// Per-agent standardisation of x [R][N] (include/dronesim.h: dronesim_standardize), two launches over one decomposition that
// depends on (R, N) only:
//   lane group   V = 4 adjacent columns where N % 4 == 0 (one 16-byte access where the pointers allow it), else 1
//   column tile  `tw` lane groups: 16 (64 floats, 256 contiguous bytes per row) where N % 64 == 0 -- at N = 64 the whole row --,
//                else the whole row, capped so that a tile has at most 1024 columns
//   iteration    a workgroup of 1024 lanes covers q = 1024 / tw rows of its tile at once: lane t holds row t / tw, group t % tw,
//                i.e. flat position t of the q x tw block (with one tile per row: of the flat array) -- N = 5 or 70 walk the
//                array contiguously with 1020 / 980 lanes, and a lane meets the same columns in every iteration
//   slab         `rps` rows (a multiple of q); S slabs x tiles workgroups aim at kStdBlocks, one per CU
// Pass 1: every lane of a column shifts by the same K, the column's value in the slab's first row (a value of the column: no
// cancellation at -500 +- 0.5), and accumulates in double the sums of d = x - K and of d^2; the q lanes of a column are folded
// through LDS by ONE fixed tree (both sums per level) into the slab's sum rows K + sum d and its second moment about the slab's
// own mean, sum d^2 - (sum d)^2 / rows: ws [S][2][N].  Nothing but the tree and one division per column follows the loop.
// Pass 2: every workgroup requests its first kStdPre iterations of rows, then folds the S partials of its tile's columns in ONE
// sweep -- up to kStdRuns contiguous runs of slabs, one lane each, ascending, then the runs ascending: the plain sums (mean), and the
// moments about slab 0's mean m0, sum_s (m2_s + e_s^2 / n_s) with e_s = sum_s - n_s m0, which - (sum_s e_s)^2 / R is the moment
// about the mean -- into mean and 1 / (std + eps), and maps its rows.  An all-equal column has K = c, d = 0, sum = rows c and
// e_s = 0 exactly.  The tile rule keeps that fold at S x 64 x 16 bytes per workgroup for the wide shapes (C5 shard: 64 KiB).
constexpr int kStdThreads = 1024, kStdBlocks = 256, kStdRuns = 32, kStdPre = 4;

struct StdPlan {
    int V, tw, tiles, q, S;
    long long rps;
};

StdPlan std_plan(int R, int N)
{
    StdPlan p;
    p.V = N % 4 == 0 ? 4 : 1;
    const int nv = N / p.V, cap = kStdThreads / p.V;
    p.tw = (p.V == 4 && N % 64 == 0) ? 16 : (nv <= cap ? nv : cap);
    p.tiles = (nv + p.tw - 1) / p.tw;
    p.q = kStdThreads / p.tw;
    const long long iters = ((long long)R + p.q - 1) / p.q;
    long long want = kStdBlocks / p.tiles;
    want = want < 1 ? 1 : (want > iters ? iters : want);
    p.rps = ((iters + want - 1) / want) * p.q;
    p.S = (int)(((long long)R + p.rps - 1) / p.rps);
    return p;
}

typedef float std_f4 __attribute__((ext_vector_type(4)));

// NT: the last use of the element (pass 2 reads a row once more and writes it once), as the return scans do
template <int V, bool VEC, bool NT>
__device__ __forceinline__ void std_load(const float *p, float (&v)[V])
{
    if (VEC) {
        const std_f4 f = NT ? __builtin_nontemporal_load(reinterpret_cast<const std_f4 *>(p)) : *reinterpret_cast<const std_f4 *>(p);
        v[0] = f.x; v[V > 1 ? 1 : 0] = f.y; v[V > 2 ? 2 : 0] = f.z; v[V > 3 ? 3 : 0] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = NT ? __builtin_nontemporal_load(p + k) : p[k];
    }
}

template <int V, bool VEC>
__device__ __forceinline__ void std_store(float *o, const float (&v)[V])
{
    if (VEC) {
        std_f4 f;
        f.x = v[0]; f.y = v[V > 1 ? 1 : 0]; f.z = v[V > 2 ? 2 : 0]; f.w = v[V > 3 ? 3 : 0];
        __builtin_nontemporal_store(f, reinterpret_cast<std_f4 *>(o));
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) __builtin_nontemporal_store(v[k], o + k);
    }
}

template <int V, bool VEC>
__global__ __launch_bounds__(kStdThreads) void standardize_sums_kernel(const float *__restrict__ x, double *__restrict__ ws, int R,
                                                                       int N, int tw, int q, int qp, long long rps)
{
    __shared__ double b1[kStdThreads][V], b2[kStdThreads][V];
    const int t = threadIdx.x, rl = t / tw, g = blockIdx.y * tw + t % tw;
    const bool lane_on = rl < q && g * V < N;
    const long long r_begin = (long long)blockIdx.x * rps;
    const long long r_end = r_begin + rps < R ? r_begin + rps : R;
    double sd[V], sd2[V], k0[V];
#pragma unroll
    for (int k = 0; k < V; ++k) sd[k] = sd2[k] = k0[k] = 0.0;
    if (lane_on) {
        float v[V];
        std_load<V, VEC, false>(x + (size_t)r_begin * N + (size_t)g * V, v);   // K: the slab's first row (cached: one read per
                                                                                 // column tile; its owners meet it again at j = 0)
#pragma unroll
        for (int k = 0; k < V; ++k) k0[k] = (double)v[k];
        if (r_begin + rl < r_end) {
            const float *p = x + (size_t)(r_begin + rl) * N + (size_t)g * V;
            const size_t step = (size_t)q * N;
            const long long n = (r_end - r_begin - rl + q - 1) / q;
#pragma unroll 4
            for (long long j = 0; j < n; ++j) {
                std_load<V, VEC, false>(p + j * step, v);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const double d = (double)v[k] - k0[k];
                    sd[k] += d;
                    sd2[k] = fma(d, d, sd2[k]);
                }
            }
        }
    }
    // fixed tree over the q lanes (rows) of a column: b[t] += b[t + w tw], w = qp / 2 .. 1 (qp = q rounded up to 2^n)
#pragma unroll
    for (int k = 0; k < V; ++k) { b1[t][k] = sd[k]; b2[t][k] = sd2[k]; }
    for (int w = qp >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (lane_on && rl < w && rl + w < q) {
#pragma unroll
            for (int k = 0; k < V; ++k) { b1[t][k] += b1[t + w * tw][k]; b2[t][k] += b2[t + w * tw][k]; }
        }
    }
    if (lane_on && rl == 0) {                                            // (its own sums: the last level's writer)
        const double rows = (double)(r_end - r_begin);
        double *o = ws + (size_t)blockIdx.x * 2 * N + (size_t)g * V;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double s = b1[t][k];
            o[k] = fma(rows, k0[k], s);
            o[N + k] = fmax(b2[t][k] - s * s / rows, 0.0);
        }
    }
}

template <int V, bool VEC>
__global__ __launch_bounds__(kStdThreads) void standardize_apply_kernel(const float *x, float *y, const double *__restrict__ ws,
                                                                        float *__restrict__ stats, int R, int N, int tw, int q,
                                                                        long long rps, int S, float eps)
{
    __shared__ double part[3][kStdThreads], mean_s[kStdThreads], inv_s[kStdThreads];
    const int t = threadIdx.x;
    // the map's first rows, requested before the fold: lane t at row t / tw, group t % tw, as in pass 1
    const int rl = t / tw, gl = t % tw, g = blockIdx.y * tw + gl;
    const long long r_begin = (long long)blockIdx.x * rps;
    const long long r_end = r_begin + rps < R ? r_begin + rps : R;
    const bool map_on = rl < q && g * V < N && r_begin + rl < r_end;
    const long long n = map_on ? (r_end - r_begin - rl + q - 1) / q : 0;
    const size_t at = (size_t)(r_begin + rl) * N + (size_t)g * V, step = (size_t)q * N;
    float pv[kStdPre][V];
#pragma unroll
    for (int u = 0; u < kStdPre; ++u) {
#pragma unroll
        for (int k = 0; k < V; ++k) pv[u][k] = 0.f;
        if (u < n) std_load<V, VEC, true>(x + at + u * step, pv[u]);
    }
    const int c0 = blockIdx.y * tw * V;                                  // the tile's first column
    const int nc = (N - c0) < tw * V ? (N - c0) : tw * V;                // its columns (<= 1024)
    // the fold: lane (run, column) takes the slabs [run ch, (run + 1) ch) in ascending order, lane (0, column) then the runs
    const int runs = kStdThreads / nc < kStdRuns ? kStdThreads / nc : kStdRuns, run = t / nc, col = t % nc;
    const int ch = (S + runs - 1) / runs;
    const int s_lo = run * ch, s_hi = (s_lo + ch) < S ? (s_lo + ch) : S;
    const double n_full = (double)(rps < R ? rps : R), n_last = (double)(R - (long long)(S - 1) * rps);
    double a = 0.0, b = 0.0, e1 = 0.0;
    if (run < runs && s_lo < s_hi) {
        const double m0 = ws[c0 + col] / n_full, inv_full = 1.0 / n_full, inv_last = 1.0 / n_last;
#pragma unroll 8
        for (int s = s_lo; s < s_hi; ++s) {
            const double sum = ws[(size_t)s * 2 * N + c0 + col], m2 = ws[(size_t)s * 2 * N + N + c0 + col];
            const double ns = s == S - 1 ? n_last : n_full, e = fma(-ns, m0, sum);
            a += sum;
            e1 += e;
            b += fma(e * e, s == S - 1 ? inv_last : inv_full, m2);
        }
    }
    part[0][t] = a;
    part[1][t] = b;
    part[2][t] = e1;
    __syncthreads();
    if (t < nc) {
        double tot = 0.0, m2 = 0.0, es = 0.0;
        for (int u = 0; u < runs; ++u) {
            tot += part[0][u * nc + t];
            m2 += part[1][u * nc + t];
            es += part[2][u * nc + t];
        }
        const double mean = tot / (double)R;
        const double sd = sqrt(fmax(m2 - es * es / (double)R, 0.0) / (double)R), den = sd + (double)eps;
        mean_s[t] = mean;
        inv_s[t] = den > 0.0 ? 1.0 / den : 0.0;                          // (an all-equal column at eps = 0: y = 0, not 0 / 0)
        if (stats && blockIdx.x == 0) {
            stats[c0 + t] = (float)mean;
            stats[N + c0 + t] = (float)sd;
        }
    }
    __syncthreads();
    // the map: y = (x - mean) * (1 / (std + eps)) in double (within 2^-52 of the quotient before the rounding to float)
    if (!map_on) return;
    double mean[V], inv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { mean[k] = mean_s[gl * V + k]; inv[k] = inv_s[gl * V + k]; }
#pragma unroll
    for (int u = 0; u < kStdPre; ++u) {
        if (u < n) {
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = (float)(((double)pv[u][k] - mean[k]) * inv[k]);
            std_store<V, VEC>(y + at + u * step, v);
        }
    }
#pragma unroll 4
    for (long long j = kStdPre; j < n; ++j) {
        float v[V];
        std_load<V, VEC, true>(x + at + j * step, v);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (float)(((double)v[k] - mean[k]) * inv[k]);
        std_store<V, VEC>(y + at + j * step, v);
    }
}

}  // namespace

extern "C" int dronesim_standardize_workspace(int R, int N, size_t *bytes)
{
    if (R < 1 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize_workspace: R < 1 or N < 1");
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize_workspace: NULL bytes");
    *bytes = sizeof(double) * 2 * (size_t)std_plan(R, N).S * (size_t)N;
    return DRONESIM_OK;
}

extern "C" int dronesim_standardize(const float *x, float *y, float *stats, int R, int N, float eps, void *ws, size_t ws_bytes,
                                    void *stream)
{
    if (R < 1 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: R < 1 or N < 1");
    if (!x || !y || !ws) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: NULL x / y / workspace");
    if (!(eps >= 0.f)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: eps must be >= 0");
    const StdPlan p = std_plan(R, N);
    if (ws_bytes < sizeof(double) * 2 * (size_t)p.S * (size_t)N)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: workspace smaller than dronesim_standardize_workspace()");
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int qp = 1;
    while (qp < p.q) qp <<= 1;
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles), block(kStdThreads);
    double *w = (double *)ws;
    // 16-byte accesses where every lane group starts 16-byte aligned; the lanes' columns and rows do not depend on it
    const bool vec = p.V == 4 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
    if (vec) {
        hipLaunchKernelGGL((standardize_sums_kernel<4, true>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<4, true>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    } else if (p.V == 4) {
        hipLaunchKernelGGL((standardize_sums_kernel<4, false>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<4, false>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    } else {
        hipLaunchKernelGGL((standardize_sums_kernel<1, false>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<1, false>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}
