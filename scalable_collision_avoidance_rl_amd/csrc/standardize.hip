// Per-agent standardisation of a window of values, the PPO learner's advantages (include/dronesim.h: dronesim_standardize_workspace,
// dronesim_standardize): float64 sums, two launches, fixed order.
#include "colstats_common.hpp"
#include "../../include/dronesim.h"

#include <math.h>

namespace {

// x [R][N], two launches over the decomposition of colstats_common.hpp (lane groups, column tiles, slabs, the lane map, the tree).
// Pass 1: every lane of a column shifts by the same K, the column's value in the slab's first row (a value of the column: no
// cancellation at -500 +- 0.5), and accumulates in double the sums of d = x - K and of d^2; the q lanes of a column are folded
// through LDS by ONE fixed tree (both sums per level) into the slab's sum rows K + sum d and its second moment about the slab's
// own mean, sum d^2 - (sum d)^2 / rows: ws [S][2][N].  Nothing but the tree and one division per column follows the loop.
// Pass 2: every workgroup requests its first kStdPre iterations of rows, then folds the S partials of its tile's columns in ONE
// sweep -- up to kColRuns contiguous runs of slabs, one lane each, ascending, then the runs ascending: the plain sums (mean), and the
// moments about slab 0's mean m0, sum_s (m2_s + e_s^2 / n_s) with e_s = sum_s - n_s m0, which - (sum_s e_s)^2 / R is the moment
// about the mean -- into mean and 1 / (std + eps), and maps its rows.  An all-equal column has K = c, d = 0, sum = rows c and
// e_s = 0 exactly.  The tile rule keeps that fold at S x 64 x 16 bytes per workgroup for the wide shapes (C5 shard: 64 KiB).
constexpr int kStdPre = 4;

template <int V, bool VEC>
__global__ __launch_bounds__(kColThreads) void standardize_sums_kernel(const float *__restrict__ x, double *__restrict__ ws, int R,
                                                                       int N, int tw, int q, int qp, long long rps)
{
    __shared__ double b1[kColThreads][V], b2[kColThreads][V];
    const int t = threadIdx.x;
    ColLane<V> lane(tw, q, N);
    const bool lane_on = lane.on();
    lane.slab(rps, R);
    double sd[V], sd2[V], k0[V];
#pragma unroll
    for (int k = 0; k < V; ++k) sd[k] = sd2[k] = k0[k] = 0.0;
    if (lane_on) {
        float v[V];
        // K: the slab's first row (cached: one read per column tile; its owners meet it again at j = 0)
        col_load<V, VEC, false>(x + (size_t)lane.r_begin * N + lane.col(), v);
#pragma unroll
        for (int k = 0; k < V; ++k) k0[k] = (double)v[k];
        if (lane.has_rows()) {
            const float *p = x + (size_t)lane.row() * N + lane.col();
            const size_t step = lane.step();
            const long long n = lane.n();
#pragma unroll 4
            for (long long j = 0; j < n; ++j) {
                col_load<V, VEC, false>(p + j * step, v);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const double d = (double)v[k] - k0[k];
                    sd[k] += d;
                    sd2[k] = fma(d, d, sd2[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) { b1[t][k] = sd[k]; b2[t][k] = sd2[k]; }
    // colstats_common.hpp's tree, on a loop of its own: through col_tree the V = 1 kernel issued the read-out's fma behind its
    // division, and with the read-out left here the loop's exit test changed -- the pairs of a level are the header's
    for (int w = qp >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (col_tree_pairs(lane_on, lane.rl, w, q)) {
#pragma unroll
            for (int k = 0; k < V; ++k) { b1[t][k] += b1[t + w * tw][k]; b2[t][k] += b2[t + w * tw][k]; }
        }
    }
    if (lane_on && lane.rl == 0) {                                       // (its own sums: the last level's writer)
        const double rows = (double)(lane.r_end - lane.r_begin);
        double *o = ws + (size_t)blockIdx.x * 2 * N + lane.col();
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double s = b1[t][k];
            o[k] = fma(rows, k0[k], s);
            o[N + k] = fmax(b2[t][k] - s * s / rows, 0.0);
        }
    }
}

template <int V, bool VEC>
__global__ __launch_bounds__(kColThreads) void standardize_apply_kernel(const float *x, float *y, const double *__restrict__ ws,
                                                                        float *__restrict__ stats, int R, int N, int tw, int q,
                                                                        long long rps, int S, float eps)
{
    __shared__ double part[3][kColThreads], mean_s[kColThreads], inv_s[kColThreads];
    const int t = threadIdx.x;
    // the map's first rows, requested before the fold
    ColLane<V> lane(tw, q, N);
    lane.slab(rps, R);
    const bool map_on = lane.on() && lane.has_rows();
    const long long n = map_on ? lane.n() : 0;
    const size_t at = lane.at(), step = lane.step();
    float pv[kStdPre][V];
#pragma unroll
    for (int u = 0; u < kStdPre; ++u) {
#pragma unroll
        for (int k = 0; k < V; ++k) pv[u][k] = 0.f;
        if (u < n) col_load<V, VEC, true>(x + at + u * step, pv[u]);
    }
    const int c0 = blockIdx.y * tw * V;                                  // the tile's first column
    const int nc = (N - c0) < tw * V ? (N - c0) : tw * V;                // its columns (<= 1024)
    // the fold: lane (run, column) takes its run of slabs in ascending order, lane (0, column) then the runs
    const int runs = kColThreads / nc < kColRuns ? kColThreads / nc : kColRuns, run = t / nc, col = t % nc;
    const ColRun r = col_run(runs, run, S);
    const double n_full = (double)(rps < R ? rps : R), n_last = (double)(R - (long long)(S - 1) * rps);
    double a = 0.0, b = 0.0, e1 = 0.0;
    if (run < runs && r.s_lo < r.s_hi) {
        const double m0 = ws[c0 + col] / n_full, inv_full = 1.0 / n_full, inv_last = 1.0 / n_last;
#pragma unroll 8
        for (int s = r.s_lo; s < r.s_hi; ++s) {
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
    for (int k = 0; k < V; ++k) { mean[k] = mean_s[lane.gl * V + k]; inv[k] = inv_s[lane.gl * V + k]; }
#pragma unroll
    for (int u = 0; u < kStdPre; ++u) {
        if (u < n) {
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = (float)(((double)pv[u][k] - mean[k]) * inv[k]);
            col_store<V, VEC, true>(y + at + u * step, v);
        }
    }
#pragma unroll 4
    for (long long j = kStdPre; j < n; ++j) {
        float v[V];
        col_load<V, VEC, true>(x + at + j * step, v);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (float)(((double)v[k] - mean[k]) * inv[k]);
        col_store<V, VEC, true>(y + at + j * step, v);
    }
}

}  // namespace

extern "C" int dronesim_standardize_workspace(int R, int N, size_t *bytes)
{
    ColPlan p;
    if (const int rc = col_validate("dronesim_standardize_workspace", 'N', R, N, bytes ? nullptr : "NULL bytes", nullptr, &p)) return rc;
    *bytes = col_ws_bytes(p, 2, N);
    return DRONESIM_OK;
}

extern "C" int dronesim_standardize(const float *x, float *y, float *stats, int R, int N, float eps, void *ws, size_t ws_bytes,
                                    void *stream)
{
    ColPlan p;
    if (const int rc = col_validate("dronesim_standardize", 'N', R, N, x && y && ws ? nullptr : "NULL x / y / workspace",
                                    eps >= 0.f ? nullptr : "eps must be >= 0", &p, {"dronesim_standardize_workspace", 2, ws, ws_bytes}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int qp = col_qp(p.q);
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles), block(kColThreads);
    double *w = (double *)ws;
    col_dispatch(p, reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y), [&](auto V, auto VEC) {
        hipLaunchKernelGGL((standardize_sums_kernel<V(), VEC()>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<V(), VEC()>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    });
    return dronesim_launched();
}
