// Static obstacle discs (include/dronesim.h states the rule): dronesim_obstacle_sense lists, per record (e, i), the m nearest of
// the M discs within the agent's range from the agent's OWN observation -- the list the obstacle shield (shield.hip) turns into
// half-planes --, dronesim_episode_obstacle_safety reduces a stored window to per-episode clearance and hit tables,
// dronesim_obstacle_observe appends that list to every record (the networks' obstacle columns) and dronesim_obstacle_reward takes
// the obstacle cost of the observation after every stored step off its reward.
//
// Both need the agent's position, which its record holds: row 0 is x_i - xF_i, so x = z[0] + xF[i][0], y = z[1] + xF[i][1].  The
// gap to disc o = (ox, oy, or):  p = o.xy - (x, y),  d = sqrtf(fmaf(p.y, p.y, p.x p.x)),  gap = (d - radius[i]) - or  (obstacle_gap
// in obstacle_common.hpp: the ONE place that evaluates it; sqrtf is the correctly rounded one, so the sense planes and the tables agree bit for bit).
//
// One thread per record, consecutive threads on consecutive records.  The disc loop is wave-uniform: the workgroup stages the list
// once in LDS (12 bytes a disc, 12 KB at M = 1024) and every lane then reads the same LDS address, which broadcasts -- no lane
// gathers from global memory.  A thread past the end stays (the staging has a barrier, the scan's flag fetch is a wave operation).
#include "record_entry.hpp"
#include "scan_common.hpp"
#include "obstacle_common.hpp"

namespace {

constexpr int kMaxObstacles = DRONESIM_MAX_OBSTACLES;

// the workgroup's copy of the list: s[3 o + 0..2] = (x, y, r) of disc o
__device__ __forceinline__ void stage_obstacles(float *s, const float *__restrict__ obstacles, int M)
{
    for (int q = threadIdx.x; q < 3 * M; q += blockDim.x) s[q] = obstacles[q];
    __syncthreads();
}

// the smallest gap over ALL discs (+inf at M = 0)
__device__ __forceinline__ float obstacle_gap_min(const float *s, int M, float x, float y, float ri)
{
    float gm = __builtin_inff();
    for (int o = 0; o < M; ++o)                                // (wave-uniform; the three reads broadcast)
        gm = ob_nan_min(obstacle_gap(x, y, ri, s[3 * o], s[3 * o + 1], s[3 * o + 2]).gap, gm);
    return gm;
}

// ---- dronesim_obstacle_sense ------------------------------------------------------------------------------------------------------
struct SenseArgs {
    const float *z, *xF, *radius, *sense, *obstacles;
    float *orow;
    int32_t *oid;
    float *gap_min;
    uint8_t *hit;
    int N, stride, M, W;                                       // stride: floats per record (k1 c); W: record_load_width's rule
    unsigned long long records;
};

template <int MS>
__global__ void __launch_bounds__(256) obstacle_sense_kernel(const SenseArgs a)
{
    __shared__ float s_obs[3 * kMaxObstacles];
    stage_obstacles(s_obs, a.obstacles, a.M);
    const unsigned long long r0 = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    const bool act = r0 < a.records;
    const unsigned long long r = act ? r0 : a.records - 1;
    const int i = (int)(r % (unsigned)a.N);
    const float *rec = a.z + r * (unsigned long long)a.stride;
    float zx, zy;
    load_row0(rec, a.W, zx, zy);
    const float x = zx + a.xF[2 * i], y = zy + a.xF[2 * i + 1];
    const float ri = a.radius[i], range = a.sense[i];

    const float inf = __builtin_inff();
    float bg[MS], bx[MS], by[MS], br[MS];
    int bi[MS];
#pragma unroll
    for (int s = 0; s < MS; ++s) { bg[s] = inf; bx[s] = by[s] = br[s] = 0.0f; bi[s] = -1; }
    float gm = inf;
    const int M = a.M;
    for (int o = 0; o < M; ++o) {
        const float orad = s_obs[3 * o + 2];
        const ObstacleGap g = obstacle_gap(x, y, ri, s_obs[3 * o], s_obs[3 * o + 1], orad);
        gm = ob_nan_min(g.gap, gm);
        const bool in = g.gap <= range;                        // (a NaN gap is not in range)
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;  // most discs are out of every lane's range: the wave skips the insertion
        sense_insert<MS>(bg, bx, by, br, bi, in, g, orad, o);
    }
    if (!act) return;
    float *orow = a.orow + r * (unsigned long long)(3 * MS);
    int32_t *oid = a.oid + r * (unsigned long long)MS;
#pragma unroll
    for (int s = 0; s < MS; ++s) {
        orow[3 * s] = bx[s]; orow[3 * s + 1] = by[s]; orow[3 * s + 2] = br[s];
        oid[s] = bi[s];
    }
    if (a.gap_min) a.gap_min[r] = gm;
    if (a.hit) a.hit[r] = gm <= 0.0f ? 1 : 0;
}

// ---- dronesim_obstacle_observe, dronesim_obstacle_reward ---------------------------------------------------------------------------
// (obstacle_cost_term, the one disc's term of the cost, is in obstacle_common.hpp)
struct ObserveArgs {
    const float *z, *xF, *radius, *sense, *obstacles;
    float *x_out, *cost;
    float weight;
    int N, stride, M, W, OW;                                   // W: row 0's load width; OW: 4 where x_out is 16-byte aligned, else 1
    unsigned long long records;
};

// The sense kernel's scan with the record's augmented image as its output: [0, d) the record's own bits, then the MS list slots
// (p.x, p.y, o.r).  The records of a workgroup are contiguous in z and in x_out, so the block leaves as ONE contiguous run of
// 256 (d + 3 MS) floats: every thread parks its list in LDS (12 MS bytes), and after the barrier the workgroup walks the run in
// lane order -- element g is float q = g mod (d + 3 MS) of record g / (d + 3 MS), from z (global, contiguous as well) where q < d and
// from the parked lists otherwise -- with 16-byte stores where x_out allows it (a block starts at a multiple of 1024 (d + 3 MS)
// bytes), dword stores otherwise: every store instruction of a wave covers whole lines.  No record passes through registers, so
// d is a run-time value and nothing is indexed dynamically.  COST: the sum of obstacle_cost_term over ALL discs in ascending
// id, times weight (its own rounding), one dword per thread.
template <int MS, bool COST>
__global__ void __launch_bounds__(256) obstacle_observe_kernel(const ObserveArgs a)
{
    __shared__ float s_obs[3 * kMaxObstacles];
    __shared__ float s_list[256 * 3 * MS];
    stage_obstacles(s_obs, a.obstacles, a.M);
    const unsigned long long rb = (unsigned long long)blockIdx.x * 256u;
    const unsigned long long r0 = rb + threadIdx.x;
    const bool act = r0 < a.records;
    const unsigned long long r = act ? r0 : a.records - 1;
    const int i = (int)(r % (unsigned)a.N);
    float zx, zy;
    load_row0(a.z + r * (unsigned long long)a.stride, a.W, zx, zy);
    const float x = zx + a.xF[2 * i], y = zy + a.xF[2 * i + 1];
    const float ri = a.radius[i], range = a.sense[i];

    const float inf = __builtin_inff();
    float bg[MS], bx[MS], by[MS], br[MS];
    int bi[MS];
#pragma unroll
    for (int s = 0; s < MS; ++s) { bg[s] = inf; bx[s] = by[s] = br[s] = 0.0f; bi[s] = -1; }
    float sum = 0.0f;
    const int M = a.M;
    for (int o = 0; o < M; ++o) {
        const float orad = s_obs[3 * o + 2];
        const ObstacleGap g = obstacle_gap(x, y, ri, s_obs[3 * o], s_obs[3 * o + 1], orad);
        const bool in = g.gap <= range;                        // (a NaN gap is not in range)
        const bool any_in = __builtin_amdgcn_ballot_w64(in) != 0ull;
        if (COST) {                                            // a hit adds its constant in range or not; the log runs with the insertion
            if (any_in) sum += obstacle_cost_term(g.gap, range, in);
            else sum += g.gap <= 0.0f ? kObstacleHitCost : 0.0f;
        }
        if (!any_in) continue;
        sense_insert<MS>(bg, bx, by, br, bi, in, g, orad, o);
    }
    float *mine = s_list + 3 * MS * threadIdx.x;
#pragma unroll
    for (int s = 0; s < MS; ++s) { mine[3 * s] = bx[s]; mine[3 * s + 1] = by[s]; mine[3 * s + 2] = br[s]; }
    if (COST && act) a.cost[r] = a.weight * sum;
    __syncthreads();

    const unsigned d = (unsigned)a.stride, w = d + 3u * MS;
    const unsigned long long left = a.records - rb;
    const unsigned total = (left < 256u ? (unsigned)left : 256u) * w;             // floats of this block's run (<= 256 * 57)
    const float *zb = a.z + rb * d;
    float *ob = a.x_out + rb * w;
    if (a.OW == 4) {
        for (unsigned g0 = 4u * threadIdx.x; g0 < total; g0 += 1024u) {
            unsigned rec = g0 / w, q = g0 - rec * w;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = 0.0f;
                if (g0 + j < total) v[j] = q < d ? zb[rec * d + q] : s_list[rec * (3u * MS) + (q - d)];
                if (++q == w) { q = 0; ++rec; }
            }
            if (g0 + 4u <= total) {
                ob_f4 o4; o4.x = v[0]; o4.y = v[1]; o4.z = v[2]; o4.w = v[3];
                *reinterpret_cast<ob_f4 *>(ob + g0) = o4;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (g0 + j < total) ob[g0 + j] = v[j];
            }
        }
    } else {
        for (unsigned g0 = threadIdx.x; g0 < total; g0 += 256u) {
            const unsigned rec = g0 / w, q = g0 - rec * w;
            ob[g0] = q < d ? zb[rec * d + q] : s_list[rec * (3u * MS) + (q - d)];
        }
    }
}

struct RewardArgs {
    const float *z_post, *z_final;
    const uint8_t *done;
    const float *reward, *xF, *radius, *sense, *obstacles;
    float *reward_out, *cost;                                  // reward_out may be reward itself (one thread reads and writes an element)
    float weight;
    int N, stride, M, W;
    unsigned long long records;                                // T E N
};

// Elementwise over (t, e, i): the cost of the observation after step t -- z_final's record where the step ended an episode and
// z_final is given, the post-step ring slot's otherwise (RolloutStorage.next_z's substitution) -- off the reward.
__global__ void __launch_bounds__(256) obstacle_reward_kernel(const RewardArgs a)
{
    __shared__ float s_obs[3 * kMaxObstacles];
    stage_obstacles(s_obs, a.obstacles, a.M);
    const unsigned long long r0 = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    const bool act = r0 < a.records;
    const unsigned long long r = act ? r0 : a.records - 1;
    const unsigned long long te = r / (unsigned)a.N;
    const int i = (int)(r - te * (unsigned)a.N);
    const float *src = (a.z_final && a.done[te] != 0) ? a.z_final : a.z_post;
    float zx, zy;
    load_row0(src + r * (unsigned long long)a.stride, a.W, zx, zy);
    const float x = zx + a.xF[2 * i], y = zy + a.xF[2 * i + 1];
    const float ri = a.radius[i], range = a.sense[i];
    float sum = 0.0f;
    const int M = a.M;
    for (int o = 0; o < M; ++o) {
        const float gap = obstacle_gap(x, y, ri, s_obs[3 * o], s_obs[3 * o + 1], s_obs[3 * o + 2]).gap;
        const bool in = gap <= range;
        if (__builtin_amdgcn_ballot_w64(in) != 0ull) sum += obstacle_cost_term(gap, range, in);
        else sum += gap <= 0.0f ? kObstacleHitCost : 0.0f;
    }
    if (!act) return;
    {
#pragma clang fp contract(off)                                 // two roundings, as the rule states: the stored cost is the one subtracted
        const float cost = a.weight * sum;
        a.reward_out[r] = a.reward[r] - cost;
        if (a.cost) a.cost[r] = cost;
    }
}

// ---- dronesim_episode_obstacle_safety ---------------------------------------------------------------------------------------------
// SafetyScan's scan (evaluate.hip) with the disc loop in its step: the same backward driver, the same restart at `done`, the same
// rare-path load of z_final.  A thread needs floats 0, 1 of record [t][e][i] only -- 8 bytes, so the staged load is 8 bytes wide
// where c = 2 and the bases allow it (W = 2; a record starts at a multiple of 8 k1 bytes) and two dwords otherwise (W = 1): a
// 16-byte load would fetch the same lines and hold twice the stage registers.  The launch sits between two bounds -- the z stream
// (every line of the window once, as dronesim_episode_safety) and T M gap evaluations per thread --, so the rows of the next stage
// are in flight while the disc loops of this one run (the driver's pipelining), and the loop body is the nine instructions of
// obstacle_gap plus one minimum on LDS broadcasts.
template <int W> struct ObstacleScan {
    static constexpr bool kBeginFirst = false;
    typedef bool Flag;
    struct Rows { float zx[kStageT], zy[kStageT]; };
    struct State { float gm, xf, yf, ri; int hits, L; };       // xf, yf, ri: the column's own goal and radius
    const float *z, *z_final;
    const uint8_t *flags;
    const float *xF, *radius;
    const float *s_obs;                                        // the workgroup's staged list
    int N, stride, M;
    __device__ __forceinline__ State begin(const ScanCols<1> &cols, int) const
    {
        const size_t i = cols.col - cols.e * (size_t)N;
        return State{__builtin_inff(), xF[2 * i], xF[2 * i + 1], radius[i], 0, 0};
    }
    template <bool NT>
    __device__ __forceinline__ void record(const float *__restrict__ p, float &zx, float &zy) const
    {
        if (W == 2) {
            const ob_f2 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const ob_f2 *>(p)) : *reinterpret_cast<const ob_f2 *>(p);
            zx = v.x; zy = v.y;
        } else {
            zx = p[0]; zy = p[1];
        }
    }
    __device__ __forceinline__ void load(Rows &st, int u, int t, const ScanCols<1> &cols) const
    {
        if (t >= 0) {
            const size_t at = (size_t)t * cols.EN + cols.col;
            record<true>(z + at * (size_t)stride, st.zx[u], st.zy[u]);
        } else {
            st.zx[u] = st.zy[u] = 0.0f;
        }
    }
    __device__ __forceinline__ bool own(int t, const ScanCols<1> &cols) const
    {
        return t >= 0 && flags[(size_t)t * cols.E + cols.e] != 0;
    }
    template <bool COOP>
    __device__ __forceinline__ void step(State &s, const ScanStage<ObstacleScan> &st, int u, int t, const ScanCols<1> &cols) const
    {
        const bool dn = COOP ? st.ds.get(cols.de, u) : st.flag[u];
        float zx = st.rows.zx[u], zy = st.rows.zy[u];
        if (dn && z_final)                                     // rare: the finished episode's terminal observation
            record<false>(z_final + ((size_t)t * cols.EN + cols.col) * (size_t)stride, zx, zy);
        const float gap = obstacle_gap_min(s_obs, M, zx + s.xf, zy + s.yf, s.ri);
        const int h = gap <= 0.0f ? 1 : 0;
        if (dn) {
            s.gm = gap; s.hits = h; s.L = t + 1;
        } else {
            s.gm = ob_nan_min(gap, s.gm); s.hits += h;
        }
    }
};

template <int W>
__global__ void __launch_bounds__(256) episode_obstacle_kernel(ObstacleScan<W> p, const float *__restrict__ obstacles, int32_t *ep_len,
                                                               float *min_gap, int32_t *hit_steps, int T, int E)
{
    __shared__ float s_obs[3 * kMaxObstacles];
    stage_obstacles(s_obs, obstacles, p.M);
    p.s_obs = s_obs;
    const ScanCols<1> c(E, p.N);
    const bool coop = c.within_stage();
    typename ObstacleScan<W>::State s;
    if (coop) s = scan_backward<true, 1>(p, c, T);
    else s = scan_backward<false, 1>(p, c, T);
    if (!c.act) return;
    const bool valid = s.L > 0;                                // no episode: NaN (0 is a meaningful gap), 0
    if (min_gap) min_gap[c.col] = valid ? s.gm : __builtin_nanf("");
    if (hit_steps) hit_steps[c.col] = valid ? s.hits : 0;
    if (c.col == c.e * (size_t)p.N) ep_len[c.e] = s.L;         // the env's first column reports its length
}

}   // namespace

extern "C" {

int dronesim_obstacle_sense(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                            int E, int N, int k1, int c, int M, int m, float *orow, int32_t *oid, float *gap_min, uint8_t *hit,
                            void *stream)
{
    const char *where = "dronesim_obstacle_sense";
    if (!z || !xF || !radius || !sense || !orow || !oid) return fail_at(where, "NULL z / xF / radius / sense / orow / oid");
    if (E < 0) return fail_at(where, "E < 0");
    int rc = check_records(where, N, k1, 1, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK) rc = check_discs(where, M, obstacles);
    if (rc == DRONESIM_OK) rc = check_slots(where, m);
    if (rc != DRONESIM_OK || E == 0) return rc;
    SenseArgs a;
    a.z = z; a.xF = xF; a.radius = radius; a.sense = sense; a.obstacles = obstacles; a.orow = orow; a.oid = oid; a.gap_min = gap_min; a.hit = hit;
    a.N = N; a.stride = k1 * c; a.M = M; a.W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z));
    a.records = (unsigned long long)E * (unsigned long long)N;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
    if (m == 1) hipLaunchKernelGGL(obstacle_sense_kernel<1>, grid, dim3(256), 0, s, a);
    else if (m == 2) hipLaunchKernelGGL(obstacle_sense_kernel<2>, grid, dim3(256), 0, s, a);
    else if (m == 3) hipLaunchKernelGGL(obstacle_sense_kernel<3>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(obstacle_sense_kernel<4>, grid, dim3(256), 0, s, a);
    return dronesim_launched();
}

int dronesim_obstacle_observe(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                              int R, int N, int k1, int c, int M, int m, float *x_out, float *cost_out, float weight, void *stream)
{
    const char *where = "dronesim_obstacle_observe";
    if (!z || !xF || !radius || !sense || !x_out) return fail_at(where, "NULL z / xF / radius / sense / x_out");
    if (R < 0) return fail_at(where, "R < 0");
    int rc = check_records(where, N, k1, 1, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK) rc = check_discs(where, M, obstacles);
    if (rc == DRONESIM_OK) rc = check_slots(where, m);
    if (rc == DRONESIM_OK) rc = check_weight(where, weight);
    if (rc != DRONESIM_OK || R == 0) return rc;
    ObserveArgs a;
    a.z = z; a.xF = xF; a.radius = radius; a.sense = sense; a.obstacles = obstacles; a.x_out = x_out; a.cost = cost_out; a.weight = weight;
    a.N = N; a.stride = k1 * c; a.M = M; a.W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z));
    a.OW = (reinterpret_cast<uintptr_t>(x_out) & 15u) == 0 ? 4 : 1;
    a.records = (unsigned long long)R * (unsigned long long)N;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
#define DRONESIM_OBSERVE(MS)                                                                                 \
    do {                                                                                                     \
        if (cost_out) hipLaunchKernelGGL((obstacle_observe_kernel<MS, true>), grid, dim3(256), 0, s, a);     \
        else hipLaunchKernelGGL((obstacle_observe_kernel<MS, false>), grid, dim3(256), 0, s, a);             \
    } while (0)
    if (m == 1) DRONESIM_OBSERVE(1);
    else if (m == 2) DRONESIM_OBSERVE(2);
    else if (m == 3) DRONESIM_OBSERVE(3);
    else DRONESIM_OBSERVE(4);
#undef DRONESIM_OBSERVE
    return dronesim_launched();
}

int dronesim_obstacle_reward(const float *z_post, const float *z_final, const uint8_t *done, const float *reward, const float *xF,
                             const float *radius, const float *sense, const float *obstacles, int T, int E, int N, int k1, int c, int M,
                             float weight, float *reward_out, float *cost_out, void *stream)
{
    const char *where = "dronesim_obstacle_reward";
    if (!z_post || !done || !reward || !xF || !radius || !sense || !reward_out)
        return fail_at(where, "NULL z_post / done / reward / xF / radius / sense / reward_out");
    if (T < 0 || E < 0) return fail_at(where, "T or E < 0");
    int rc = check_records(where, N, k1, 1, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK) rc = check_discs(where, M, obstacles);
    if (rc == DRONESIM_OK) rc = check_weight(where, weight);
    if (rc != DRONESIM_OK || T == 0 || E == 0) return rc;
    RewardArgs a;
    a.z_post = z_post; a.z_final = z_final; a.done = done; a.reward = reward; a.xF = xF; a.radius = radius; a.sense = sense;
    a.obstacles = obstacles; a.reward_out = reward_out; a.cost = cost_out; a.weight = weight;
    a.N = N; a.stride = k1 * c; a.M = M;
    a.W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z_post) | reinterpret_cast<uintptr_t>(z_final));
    a.records = (unsigned long long)T * (unsigned long long)E * (unsigned long long)N;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(obstacle_reward_kernel, dim3((unsigned)((a.records + 255) / 256)), dim3(256), 0, s, a);
    return dronesim_launched();
}

int dronesim_episode_obstacle_safety(const float *z, const float *z_final, const uint8_t *done, const float *xF, const float *radius,
                                     const float *obstacles, int T, int E, int N, int k1, int c, int M, int32_t *ep_len,
                                     float *min_obstacle_gap, int32_t *obstacle_hit_steps, float *ep_min_obstacle_gap,
                                     int32_t *ep_obstacle_hit_steps, void *stream)
{
    const char *where = "dronesim_episode_obstacle_safety";
    if (T < 0 || E < 0) return fail_at(where, "T or E < 0");
    int rc = check_records(where, N, k1, 1, INT_MAX, c);
    if (rc == DRONESIM_OK) rc = check_discs(where, M, obstacles);
    if (rc != DRONESIM_OK) return rc;
    if ((ep_min_obstacle_gap && !min_obstacle_gap) || (ep_obstacle_hit_steps && !obstacle_hit_steps))
        return fail_at(where, "a per-env table needs the per-agent one it reduces");
    if (E == 0) return DRONESIM_OK;                            // (an empty window has no addresses: checked before the pointers)
    if (!xF || !radius || !ep_len || (T > 0 && (!z || !done))) return fail_at(where, "NULL z / done / xF / radius / ep_len");
    const size_t cols = (size_t)E * N;
    // a thread reads floats 0, 1 of a record: the scan has no 16-byte variant, a rule's 4 is served by the 8-byte one
    const int W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(z_final));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((cols + 255) / 256));
    if (W >= 2) {
        const ObstacleScan<2> p{z, z_final, done, xF, radius, nullptr, N, k1 * c, M};
        hipLaunchKernelGGL(episode_obstacle_kernel<2>, grid, dim3(256), 0, s, p, obstacles, ep_len, min_obstacle_gap, obstacle_hit_steps, T, E);
    } else {
        const ObstacleScan<1> p{z, z_final, done, xF, radius, nullptr, N, k1 * c, M};
        hipLaunchKernelGGL(episode_obstacle_kernel<1>, grid, dim3(256), 0, s, p, obstacles, ep_len, min_obstacle_gap, obstacle_hit_steps, T, E);
    }
    rc = dronesim_launched();
    if (rc != DRONESIM_OK || !(ep_min_obstacle_gap || ep_obstacle_hit_steps)) return rc;
    hipLaunchKernelGGL(obstacle_env_kernel, dim3((unsigned)((2 * (size_t)E + 255) / 256)), dim3(256), 0, s, ep_len, min_obstacle_gap,
                       obstacle_hit_steps, ep_min_obstacle_gap, ep_obstacle_hit_steps, E, N);
    return dronesim_launched();
}

}   // extern "C"
