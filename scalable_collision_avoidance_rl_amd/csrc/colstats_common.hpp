// colstats_common.hpp -- what the per-column statistics of a float32 row matrix x [R][C] share (standardize.hip: mean / std of a
// window, two launches; obsnorm.hip: running mean / variance over the finite values, and their map): ONE decomposition, a function
// of (R, C) only, which fixes the reduction order and with it the bits of both features:
//   lane group   V = 4 adjacent columns where C % 4 == 0 (one 16-byte access where the pointers allow it), else 1
//   column tile  `tw` lane groups: 16 (64 floats, 256 contiguous bytes per row) where C % 64 == 0 -- at C = 64 the whole row --,
//                else the whole row, capped so that a tile has at most 1024 columns
//   iteration    a workgroup of 1024 lanes covers q = 1024 / tw rows of its tile at once: lane t holds row t / tw, group t % tw,
//                i.e. flat position t of the q x tw block (with one tile per row: of the flat array) -- C = 5 or 70 walk the
//                array contiguously with 1020 / 980 lanes, and a lane meets the same columns in every iteration
//   slab         `rps` rows (a multiple of q); S slabs x tiles workgroups aim at kColBlocks, one per CU
// A sums kernel accumulates per lane over its rows, then ONE fixed LDS tree folds the q lanes of a column into the slab's partial,
// which the column's first lane writes to ws [S][planes][C] doubles; a second launch folds the S partials in contiguous runs of
// slabs, ascending.  What is accumulated, the shift, the rule that combines two partials and the fold stay with each file; the
// plan, the lane-to-element map, the 16- / 4-byte accesses, the tree's shape, the run split, the host's (V, VEC) choice and the
// shared refusals are here.
#pragma once
#include "common.hpp"

#include <stdio.h>
#include <type_traits>

constexpr int kColThreads = 1024, kColBlocks = 256, kColRuns = 32;

struct ColPlan {
    int V, tw, tiles, q, S;
    long long rps;
};

inline ColPlan col_plan(int R, int C)
{
    ColPlan p;
    p.V = C % 4 == 0 ? 4 : 1;
    const int nv = C / p.V, cap = kColThreads / p.V;
    p.tw = (p.V == 4 && C % 64 == 0) ? 16 : (nv <= cap ? nv : cap);
    p.tiles = (nv + p.tw - 1) / p.tw;
    p.q = kColThreads / p.tw;
    const long long iters = ((long long)R + p.q - 1) / p.q;
    long long want = kColBlocks / p.tiles;
    want = want < 1 ? 1 : (want > iters ? iters : want);
    p.rps = ((iters + want - 1) / want) * p.q;
    p.S = (int)(((long long)R + p.rps - 1) / p.rps);
    return p;
}

// q rounded up to a power of two: the width of the tree's first level
inline int col_qp(int q)
{
    int qp = 1;
    while (qp < q) qp <<= 1;
    return qp;
}

inline size_t col_ws_bytes(const ColPlan &p, int planes, int C) { return sizeof(double) * planes * (size_t)p.S * (size_t)C; }

typedef float col_f4 __attribute__((ext_vector_type(4)));

// One lane group: VEC one 16-byte access, else V 4-byte ones.  NT: the last use of the element (a map reads a row once more and
// writes it once), as the return scans do
template <int V, bool VEC, bool NT>
__device__ __forceinline__ void col_load(const float *p, float (&v)[V])
{
    if (VEC) {
        const col_f4 f = NT ? __builtin_nontemporal_load(reinterpret_cast<const col_f4 *>(p)) : *reinterpret_cast<const col_f4 *>(p);
        v[0] = f.x; v[V > 1 ? 1 : 0] = f.y; v[V > 2 ? 2 : 0] = f.z; v[V > 3 ? 3 : 0] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = NT ? __builtin_nontemporal_load(p + k) : p[k];
    }
}

template <int V, bool VEC, bool NT>
__device__ __forceinline__ void col_store(float *o, const float (&v)[V])
{
    if (VEC) {
        col_f4 f;
        f.x = v[0]; f.y = v[V > 1 ? 1 : 0]; f.z = v[V > 2 ? 2 : 0]; f.w = v[V > 3 ? 3 : 0];
        if (NT) __builtin_nontemporal_store(f, reinterpret_cast<col_f4 *>(o));
        else *reinterpret_cast<col_f4 *>(o) = f;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (NT) __builtin_nontemporal_store(v[k], o + k);
            else o[k] = v[k];
        }
    }
}

// The lane-to-element map of a workgroup (blockIdx.x: slab, blockIdx.y: column tile): lane t holds row `rl` of every iteration and
// lane group `gl` of the tile (`g` of the row, first column col()); on(): the lane has columns.  slab(): the workgroup's rows
// [r_begin, r_end); a lane that is on() and has_rows() meets n() of them, the first one row() at element at(), the next step()
// elements on.  Small functions that the kernels call where they need the value, not members filled by one constructor: hipcc
// optimises a function before it inlines it and leaves its instructions where the call stands, and the kernels want the 64-bit
// division of n() behind their branch and the sums kernels on() in front of the slab -- written this way the kernels compile to
// the instructions of the four hand-written copies of this map.  n() is (r_end - row() + q - 1) / q in the association the
// optimiser gave those copies.
template <int V> struct ColLane {
    int rl, gl, g, q, C;
    long long r_begin, r_end;
    __device__ __forceinline__ ColLane(int tw, int q_, int C_) : q(q_), C(C_)
    {
        const int t = threadIdx.x;
        rl = t / tw; g = blockIdx.y * tw + t % tw; gl = t % tw;
    }
    __device__ __forceinline__ void slab(long long rps, int R)
    {
        r_begin = (long long)blockIdx.x * rps;
        r_end = r_begin + rps < R ? r_begin + rps : R;
    }
    __device__ __forceinline__ bool on() const { return rl < q && g * V < C; }
    __device__ __forceinline__ long long row() const { return r_begin + rl; }
    __device__ __forceinline__ bool has_rows() const { return row() < r_end; }
    __device__ __forceinline__ long long n() const { return ((long long)q - 1 + r_end - row()) / q; }
    __device__ __forceinline__ size_t at() const { return (size_t)row() * C + (size_t)g * V; }
    __device__ __forceinline__ size_t col() const { return (size_t)g * V; }
    __device__ __forceinline__ size_t step() const { return (size_t)q * C; }
};

// The fixed tree over the q lanes (rows) of a column: combine(t, t + w tw) for w = qp / 2 .. 1 (qp = col_qp(q)), then root(t) in
// lane (0, column), which reads the column's partial from its own LDS entries: it wrote them in the last level, so no barrier
// stands between the tree and root.  col_tree_pairs: the lanes that combine at level w (standardize.hip keeps the loop itself).
__device__ __forceinline__ bool col_tree_pairs(bool on, int rl, int w, int q) { return on && rl < w && rl + w < q; }

template <typename F, typename G>
__device__ __forceinline__ void col_tree(bool on, int rl, int tw, int q, int qp, F combine, G root)
{
    const int t = threadIdx.x;
    for (int w = qp >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (col_tree_pairs(on, rl, w, q)) combine(t, t + w * tw);
    }
    if (on && rl == 0) root(t);
}

// The S slabs in `runs` contiguous runs: run `run` folds the slabs [s_lo, s_hi) in ascending order (empty behind the last slab).
// (`runs` is the first parameter: hipcc orders the sum S - 1 + runs by it, and this order gives the folds their earlier code.)
struct ColRun {
    int s_lo, s_hi;
};
__device__ __forceinline__ ColRun col_run(int runs, int run, int S)
{
    const int ch = (S + runs - 1) / runs;
    ColRun r;
    r.s_lo = run * ch;
    r.s_hi = (r.s_lo + ch) < S ? (r.s_lo + ch) : S;
    return r;
}

// Host: f(V, VEC) as std::integral_constants -- 16-byte accesses where every lane group starts 16-byte aligned (`addresses`: the OR
// of the row matrices' bases); the lanes' columns and rows do not depend on it
template <typename F> void col_dispatch(const ColPlan &p, uintptr_t addresses, F f)
{
    if (p.V == 4 && (addresses & 15u) == 0) f(std::integral_constant<int, 4>(), std::true_type());
    else if (p.V == 4) f(std::integral_constant<int, 4>(), std::false_type());
    else f(std::integral_constant<int, 1>(), std::false_type());
}

// Host: the refusals the entry points share, "<fn>: <what>", in the ABI's order: the shape (`cols`: the letter the entry point's
// declaration gives the column count), a NULL pointer (`null`: its text, nullptr if none is NULL), the entry point's own condition
// (`own`: its text, nullptr if it holds), and, where a workspace comes with the call, its size against the plan's
// [S][planes][C] doubles (`query`: the function that returns it) and its 8-byte alignment.  Fills the plan.
struct ColWorkspace {
    const char *query;
    int planes;
    const void *ws;
    size_t bytes;
};
inline int col_validate(const char *fn, char cols, int R, int C, const char *null, const char *own, ColPlan *p,
                        ColWorkspace w = ColWorkspace())
{
    char msg[160];
    if (R < 1 || C < 1) snprintf(msg, sizeof(msg), "%s: R < 1 or %c < 1", fn, cols);
    else if (null) snprintf(msg, sizeof(msg), "%s: %s", fn, null);
    else if (own) snprintf(msg, sizeof(msg), "%s: %s", fn, own);
    else {
        *p = col_plan(R, C);
        if (!w.query) return DRONESIM_OK;
        if (w.bytes < col_ws_bytes(*p, w.planes, C)) snprintf(msg, sizeof(msg), "%s: workspace smaller than %s()", fn, w.query);
        else if (reinterpret_cast<uintptr_t>(w.ws) & 7u) snprintf(msg, sizeof(msg), "%s: workspace not 8-byte aligned", fn);
        else return DRONESIM_OK;
    }
    return dronesim_fail(DRONESIM_EINVAL, msg);
}
