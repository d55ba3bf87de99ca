// obstacle_common.hpp -- the pieces that DEFINE the numbers of the obstacle kernels, shared by obstacles.hip (one list [M][3] for
// all envs) and env_obstacles.hip (a list per env, [E][M][3]): the gap (obstacle_gap: the ONE place that evaluates it), the minimum
// that keeps a NaN, the sorted insertion into the per-agent list, the cost term and its hit constant, the load of a record's row 0
// and the per-env reduction of the episode tables.  A per-env result is therefore bit-identical to the shared kernel run on that
// env's records with that env's list: both files differ only in how a disc reaches the lane.
#pragma once
#include "common.hpp"

namespace {

typedef float ob_f4 __attribute__((ext_vector_type(4)));
typedef float ob_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float ob_nan_min(float a, float b) { return (a < b || a != a) ? a : b; }   // numpy.minimum: a NaN stays

struct ObstacleGap { float px, py, gap; };

__device__ __forceinline__ ObstacleGap obstacle_gap(float x, float y, float ri, float ox, float oy, float orad)
{
    ObstacleGap g;
    g.px = ox - x; g.py = oy - y;
    const float d = __builtin_sqrtf(fmaf(g.py, g.py, g.px * g.px));
    g.gap = (d - ri) - orad;
    return g;
}

// Row 0 of a record, W floats wide (record_load_width's rule; wave-uniform)
__device__ __forceinline__ void load_row0(const float *rec, int W, float &zx, float &zy)
{
    if (W == 4) {                                              // k1 even, c = 2, 16-byte aligned: row 0 with row 1
        const ob_f4 v = *reinterpret_cast<const ob_f4 *>(rec);
        zx = v.x; zy = v.y;
    } else if (W == 2) {
        const ob_f2 v = *reinterpret_cast<const ob_f2 *>(rec);
        zx = v.x; zy = v.y;
    } else {
        zx = rec[0]; zy = rec[1];
    }
}

// MS list slots kept sorted by (gap, id) in registers: the discs come in ascending id, so a new one goes in front of the first
// slot with a LARGER gap (or an empty one) and everything behind moves down one -- arrays indexed by unrolled counters only.
template <int MS>
__device__ __forceinline__ void sense_insert(float (&bg)[MS], float (&bx)[MS], float (&by)[MS], float (&br)[MS], int (&bi)[MS], bool in,
                                             const ObstacleGap &g, float orad, int o)
{
    float cg = g.gap, cx = g.px, cy = g.py, cr = orad;
    int ci = o;
    bool moving = false;                                       // the carried entry has displaced a slot: every later slot moves down
#pragma unroll
    for (int s = 0; s < MS; ++s) {
        moving = moving || (in && (cg < bg[s] || bi[s] < 0));
        const float tg = bg[s], tx = bx[s], ty = by[s], tr = br[s];
        const int ti = bi[s];
        bg[s] = moving ? cg : tg; bx[s] = moving ? cx : tx; by[s] = moving ? cy : ty; br[s] = moving ? cr : tr; bi[s] = moving ? ci : ti;
        cg = moving ? tg : cg; cx = moving ? tx : cx; cy = moving ? ty : cy; cr = moving ? tr : cr; ci = moving ? ti : ci;
    }
}

// One disc's term of the obstacle cost (include/dronesim.h): the reference's pair term b log(d_i / d_ij) with the disc in the
// neighbour's place.  A NaN gap, a NaN range and a range <= 0 with a positive gap fail both comparisons: 0.
constexpr float kObstacleHitCost = 9.99e3f;

__device__ __forceinline__ float obstacle_cost_term(float gap, float range, bool near)
{
    return gap <= 0.0f ? kObstacleHitCost : (near ? logf(range / gap) : 0.0f);
}

// The episode tables per env, agents in ascending order: task 0 the smallest gap, task 1 the hit steps summed
__global__ void __launch_bounds__(256) obstacle_env_kernel(const int32_t *__restrict__ ep_len, const float *__restrict__ min_gap,
                                                           const int32_t *__restrict__ hit_steps, float *__restrict__ ep_min_gap,
                                                           int32_t *__restrict__ ep_hit_steps, int E, int N)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * (size_t)E) return;
    const int task = (int)(idx / (size_t)E);
    const size_t e = idx - (size_t)task * E;
    const bool valid = ep_len[e] > 0;
    if (task == 0) {
        if (!ep_min_gap) return;
        float m = __builtin_nanf("");
        if (valid) {
            m = min_gap[e * N];
            for (int i = 1; i < N; ++i) m = ob_nan_min(min_gap[e * N + i], m);
        }
        ep_min_gap[e] = m;
        return;
    }
    if (!ep_hit_steps) return;
    int n = 0;
    if (valid)
        for (int i = 0; i < N; ++i) n += hit_steps[e * N + i];
    ep_hit_steps[e] = n;
}

}   // namespace
