// Per-env obstacle sets (include/dronesim_env_obstacles.h states the rule): the four list-walking kernels of obstacles.hip with a
// disc list PER ENV, obstacles [E][M][3] and count [E], in place of the one list all envs share.  Everything that defines a number
// -- the gap, the minimum, the sorted insertion, the cost term, the row-0 load -- is obstacle_common.hpp's, shared with
// obstacles.hip: a per-env result is bit-identical to the shared kernel run on that env's records with that env's list.
//
// What changes is how a disc reaches the lane.  One thread per record (or column), consecutive threads on consecutive records, so
// a 256-record workgroup touches rows row_lo .. row_lo + 254 / N + 1 at most (a row = N records of one env), row q belongs to env
// q % E -- the envs of a workgroup wrap from E - 1 to 0 wherever the leading dims are rows -- and the lanes of one wave read
// DIFFERENT lists.  Two paths, chosen on the host by env_plan (dronesim_env_obstacle_plan is its public face):
//   STAGED   the workgroup copies the lists of the rows it touches into dynamic LDS: slot j holds env (row_lo + j) % E (contiguous
//            in global memory except at the wrap), a lane reads slot row - row_lo.  Lanes of one env read one address (broadcast);
//            the slot stride is 3 M | 1 floats, ODD, so that disc o of the up to 64 envs of a wave falls into different banks
//            (3 M floats at M = 64 would put every env's disc o into the same bank: a 13-env wave at N = 5 would serialise);
//   direct   every lane loads its env's disc from global memory: one address per env the wave spans, the lists are L2-resident
//            (E M 12 bytes: 3 MB at 4096 x 64); no LDS for the list.
// The disc loop runs to the largest count of the WAVE; a lane whose own count is used up keeps its state (its loads are skipped on
// the direct path, its LDS reads stay inside its slot on the staged one).  count[e] is clamped into 0..M first.  A thread past
// the end stays (the staging has a barrier, the scan's flag fetch is a wave operation).
#include "record_entry.hpp"
#include "scan_common.hpp"
#include "obstacle_common.hpp"

namespace {

// Bytes of lists a workgroup may stage, by the nominal 12 M bytes a slot: (254 / N + 2) 12 M <= kStageBudget takes the staged path.
// A tuning value, started at 48 KB and moved to 32 KB by measurement (profiles/env_obstacles_path_ab.jsonl):
// at N = 5, M = 64 (52 slots, 39.0 KB) the staged observe-with-cost took 191.5 us against 136.2 us direct and the staged sense
// 129.6 against 108.6 (2^20 records).  Bytes alone do not order the shapes -- the envs a wave spans do: at N = 1, 2 (64, 32 envs
// a wave) the direct path issues that many addresses per load and loses 1.7x to staging at 24.0 .. 24.2 KB, so the budget stays
// above those; the table scan reuses the staged lists T times and prefers staging at every shape.  The odd stride adds up to
// 4 bytes a slot: with it and the 12 KB the observe kernel parks its output lists in a workgroup holds under 46 KB, and the
// dynamic part stays under the 48 KB a kernel gets without opting in to more (hipFuncSetAttribute, per kernel and device).
constexpr size_t kStageBudget = 32 * 1024;

struct EnvPlan {
    int staged, rows;                                          // rows: the most rows (envs) a workgroup touches
    unsigned stride;                                           // floats per LDS slot
    size_t list_bytes;                                         // dynamic LDS of the launch
};

inline EnvPlan env_plan(int N, int M)
{
    EnvPlan p;
    p.rows = 254 / N + 2;
    p.stride = (3u * (unsigned)M) | 1u;
    p.staged = M > 0 && (size_t)p.rows * 12u * (size_t)M <= kStageBudget ? 1 : 0;
    p.list_bytes = p.staged ? (size_t)p.rows * p.stride * sizeof(float) : 0;
    return p;
}

struct EnvLists {
    const float *obstacles;                                    // [E][M][3]
    const int32_t *count;                                      // [E] or NULL
    int E, M;
    unsigned stride;                                           // floats per LDS slot (STAGED)
};

extern __shared__ float s_env[];                               // STAGED: slot j at s_env + j stride

// One lane's list: its env's rows in global memory (direct) or its slot in LDS (STAGED), and its clamped count
template <bool STAGED> struct LaneList {
    const float *g;
    unsigned base;
    int cnt;
    // disc o (o < M); `valid` = o < cnt: the direct path loads nothing otherwise, and the caller drops what it computes
    __device__ __forceinline__ void disc(int o, bool valid, float &ox, float &oy, float &orad) const
    {
        if (STAGED) {
            ox = s_env[base + 3u * o]; oy = s_env[base + 3u * o + 1u]; orad = s_env[base + 3u * o + 2u];
        } else {
            ox = oy = orad = 0.0f;
            if (valid) { ox = g[3 * o]; oy = g[3 * o + 1]; orad = g[3 * o + 2]; }
        }
    }
};

// The lists of the workgroup whose first item (record or column) is rb, of `items` items of N per row: stages them (STAGED; one
// barrier) and returns the lane's own view for its row.  Every thread of the workgroup calls it.
template <bool STAGED>
__device__ __forceinline__ LaneList<STAGED> env_lists(const EnvLists &L, unsigned long long rb, unsigned long long items, int N,
                                                      unsigned long long row)
{
    const unsigned long long row_lo = rb / (unsigned)N;
    if (STAGED) {
        const unsigned long long last = rb + 255u < items ? rb + 255u : items - 1;
        const unsigned nrows = (unsigned)(last / (unsigned)N - row_lo) + 1u;      // <= 254 / N + 2
        const unsigned w = 3u * (unsigned)L.M, total = nrows * w;
        const unsigned e0 = (unsigned)(row_lo % (unsigned)L.E);
        for (unsigned q = threadIdx.x; q < total; q += 256u) {
            const unsigned j = q / w, f = q - j * w;
            const unsigned ej = (e0 + j) % (unsigned)L.E;
            s_env[j * L.stride + f] = L.obstacles[(size_t)ej * w + f];
        }
        __syncthreads();
    }
    const unsigned e = (unsigned)(row % (unsigned)L.E);
    LaneList<STAGED> l;
    const int cnt = L.count ? L.count[e] : L.M;
    l.cnt = cnt < 0 ? 0 : (cnt > L.M ? L.M : cnt);
    l.g = L.obstacles + (size_t)e * (size_t)(3 * L.M);
    l.base = (unsigned)(row - row_lo) * L.stride;
    return l;
}

// the largest count of the wave (wave-uniform: the trip count of the disc loop)
__device__ __forceinline__ int wave_max_count(int cnt)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const int other = __shfl_xor(cnt, off, 64);
        cnt = other > cnt ? other : cnt;
    }
    return __builtin_amdgcn_readfirstlane(cnt);
}

// ---- dronesim_env_obstacle_sense --------------------------------------------------------------------------------------------------
struct EnvSenseArgs {
    const float *z, *xF, *radius, *sense;
    float *orow;
    int32_t *oid;
    float *gap_min;
    uint8_t *hit;
    int N, stride, W;                                          // stride: floats per record (k1 c); W: record_load_width's rule
    unsigned long long records;
    EnvLists L;
};

template <int MS, bool STAGED>
__global__ void __launch_bounds__(256) env_obstacle_sense_kernel(const EnvSenseArgs a)
{
    const unsigned long long rb = (unsigned long long)blockIdx.x * 256u;
    const unsigned long long r0 = rb + threadIdx.x;
    const bool act = r0 < a.records;
    const unsigned long long r = act ? r0 : a.records - 1;
    const unsigned long long row = r / (unsigned)a.N;
    const int i = (int)(r - row * (unsigned)a.N);
    const LaneList<STAGED> l = env_lists<STAGED>(a.L, rb, a.records, a.N, row);
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
    const int Mw = wave_max_count(l.cnt);
    for (int o = 0; o < Mw; ++o) {
        const bool valid = o < l.cnt;
        float ox, oy, orad;
        l.disc(o, valid, ox, oy, orad);
        const ObstacleGap g = obstacle_gap(x, y, ri, ox, oy, orad);
        gm = valid ? ob_nan_min(g.gap, gm) : gm;
        const bool in = valid && g.gap <= range;               // (a NaN gap is not in range)
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
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

// ---- dronesim_env_obstacle_observe, dronesim_env_obstacle_reward ------------------------------------------------------------------
struct EnvObserveArgs {
    const float *z, *xF, *radius, *sense;
    float *x_out, *cost;
    float weight;
    int N, stride, W, OW;                                      // W: row 0's load width; OW: 4 where x_out is 16-byte aligned, else 1
    unsigned long long records;
    EnvLists L;
};

// obstacle_observe_kernel (obstacles.hip) with the lane's own list: the same scan, the same parked lists, the same contiguous run
// of 256 (d + 3 MS) floats out of the workgroup in lane order.
template <int MS, bool COST, bool STAGED>
__global__ void __launch_bounds__(256) env_obstacle_observe_kernel(const EnvObserveArgs a)
{
    __shared__ float s_list[256 * 3 * MS];
    const unsigned long long rb = (unsigned long long)blockIdx.x * 256u;
    const unsigned long long r0 = rb + threadIdx.x;
    const bool act = r0 < a.records;
    const unsigned long long r = act ? r0 : a.records - 1;
    const unsigned long long row = r / (unsigned)a.N;
    const int i = (int)(r - row * (unsigned)a.N);
    const LaneList<STAGED> l = env_lists<STAGED>(a.L, rb, a.records, a.N, row);
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
    const int Mw = wave_max_count(l.cnt);
    for (int o = 0; o < Mw; ++o) {
        const bool valid = o < l.cnt;
        float ox, oy, orad;
        l.disc(o, valid, ox, oy, orad);
        const ObstacleGap g = obstacle_gap(x, y, ri, ox, oy, orad);
        const bool in = valid && g.gap <= range;               // (a NaN gap is not in range)
        const bool any_in = __builtin_amdgcn_ballot_w64(in) != 0ull;
        if (COST) {                                            // a hit adds its constant in range or not; the log runs with the insertion
            float term;
            if (any_in) term = obstacle_cost_term(g.gap, range, in);
            else term = g.gap <= 0.0f ? kObstacleHitCost : 0.0f;
            sum = valid ? sum + term : sum;
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

struct EnvRewardArgs {
    const float *z_post, *z_final;
    const uint8_t *done;
    const float *reward, *xF, *radius, *sense;
    float *reward_out, *cost;                                  // reward_out may be reward itself (one thread reads and writes an element)
    float weight;
    int N, stride, W;
    unsigned long long records;                                // T E N
    EnvLists L;
};

// Elementwise over (t, e, i), as obstacle_reward_kernel: row te = t E + e belongs to env te % E = e
template <bool STAGED>
__global__ void __launch_bounds__(256) env_obstacle_reward_kernel(const EnvRewardArgs a)
{
    const unsigned long long rb = (unsigned long long)blockIdx.x * 256u;
    const unsigned long long r0 = rb + threadIdx.x;
    const bool act = r0 < a.records;
    const unsigned long long r = act ? r0 : a.records - 1;
    const unsigned long long te = r / (unsigned)a.N;
    const int i = (int)(r - te * (unsigned)a.N);
    const LaneList<STAGED> l = env_lists<STAGED>(a.L, rb, a.records, a.N, te);
    const float *src = (a.z_final && a.done[te] != 0) ? a.z_final : a.z_post;
    float zx, zy;
    load_row0(src + r * (unsigned long long)a.stride, a.W, zx, zy);
    const float x = zx + a.xF[2 * i], y = zy + a.xF[2 * i + 1];
    const float ri = a.radius[i], range = a.sense[i];
    float sum = 0.0f;
    const int Mw = wave_max_count(l.cnt);
    for (int o = 0; o < Mw; ++o) {
        const bool valid = o < l.cnt;
        float ox, oy, orad;
        l.disc(o, valid, ox, oy, orad);
        const float gap = obstacle_gap(x, y, ri, ox, oy, orad).gap;
        const bool in = valid && gap <= range;
        float term;
        if (__builtin_amdgcn_ballot_w64(in) != 0ull) term = obstacle_cost_term(gap, range, in);
        else term = gap <= 0.0f ? kObstacleHitCost : 0.0f;
        sum = valid ? sum + term : sum;
    }
    if (!act) return;
    {
#pragma clang fp contract(off)                                 // two roundings, as the rule states: the stored cost is the one subtracted
        const float cost = a.weight * sum;
        a.reward_out[r] = a.reward[r] - cost;
        if (a.cost) a.cost[r] = cost;
    }
}

// ---- dronesim_episode_env_obstacle_safety -----------------------------------------------------------------------------------------
// ObstacleScan (obstacles.hip) with the column's own list in its step: the same backward driver, the same restart at `done`, the
// same rare-path load of z_final, the same 8-byte or two-dword load of floats 0, 1 of a record.  A column belongs to one env for
// the whole window, so its list view and the wave's trip count are fixed before the scan.
template <int W, bool STAGED> struct EnvObstacleScan {
    static constexpr bool kBeginFirst = false;
    typedef bool Flag;
    struct Rows { float zx[kStageT], zy[kStageT]; };
    struct State { float gm, xf, yf, ri; int hits, L; };       // xf, yf, ri: the column's own goal and radius
    const float *z, *z_final;
    const uint8_t *flags;
    const float *xF, *radius;
    int N, stride;
    LaneList<STAGED> list;                                     // the column's list (set by the kernel)
    int Mw;                                                    // the wave's largest count
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
    // the smallest gap over ALL discs of the column's env (+inf without discs)
    __device__ __forceinline__ float gap_min(float x, float y, float ri) const
    {
        float gm = __builtin_inff();
        for (int o = 0; o < Mw; ++o) {
            const bool valid = o < list.cnt;
            float ox, oy, orad;
            list.disc(o, valid, ox, oy, orad);
            const float gap = obstacle_gap(x, y, ri, ox, oy, orad).gap;
            gm = valid ? ob_nan_min(gap, gm) : gm;
        }
        return gm;
    }
    template <bool COOP>
    __device__ __forceinline__ void step(State &s, const ScanStage<EnvObstacleScan> &st, int u, int t, const ScanCols<1> &cols) const
    {
        const bool dn = COOP ? st.ds.get(cols.de, u) : st.flag[u];
        float zx = st.rows.zx[u], zy = st.rows.zy[u];
        if (dn && z_final)                                     // rare: the finished episode's terminal observation
            record<false>(z_final + ((size_t)t * cols.EN + cols.col) * (size_t)stride, zx, zy);
        const float gap = gap_min(zx + s.xf, zy + s.yf, s.ri);
        const int h = gap <= 0.0f ? 1 : 0;
        if (dn) {
            s.gm = gap; s.hits = h; s.L = t + 1;
        } else {
            s.gm = ob_nan_min(gap, s.gm); s.hits += h;
        }
    }
};

template <int W, bool STAGED>
__global__ void __launch_bounds__(256) episode_env_obstacle_kernel(EnvObstacleScan<W, STAGED> p, const EnvLists L, int32_t *ep_len,
                                                                   float *min_gap, int32_t *hit_steps, int T, int E)
{
    const ScanCols<1> c(E, p.N);
    p.list = env_lists<STAGED>(L, (unsigned long long)blockIdx.x * 256u, (unsigned long long)c.EN, p.N, (unsigned long long)c.e);
    p.Mw = wave_max_count(p.list.cnt);
    const bool coop = c.within_stage();
    typename EnvObstacleScan<W, STAGED>::State s;
    if (coop) s = scan_backward<true, 1>(p, c, T);
    else s = scan_backward<false, 1>(p, c, T);
    if (!c.act) return;
    const bool valid = s.L > 0;                                // no episode: NaN (0 is a meaningful gap), 0
    if (min_gap) min_gap[c.col] = valid ? s.gm : __builtin_nanf("");
    if (hit_steps) hit_steps[c.col] = valid ? s.hits : 0;
    if (c.col == c.e * (size_t)p.N) ep_len[c.e] = s.L;         // the env's first column reports its length
}

inline EnvLists env_lists_of(const float *obstacles, const int32_t *count, int E, int M, const EnvPlan &plan)
{
    EnvLists L;
    L.obstacles = obstacles; L.count = count; L.E = E; L.M = M; L.stride = plan.stride;
    return L;
}

}   // namespace

extern "C" {

int dronesim_env_obstacle_plan(int N, int M, int m, int *staged, int *rows_per_block, size_t *lds_bytes)
{
    const char *where = "dronesim_env_obstacle_plan";
    if (N < 1 || N > DRONESIM_MAX_AGENTS) return fail_at(where, "N outside 1..1024");
    if (M < 0 || M > DRONESIM_MAX_ENV_OBSTACLES) return fail_at(where, "M outside 0..64");
    const int rc = check_slots(where, m);
    if (rc != DRONESIM_OK) return rc;
    const EnvPlan p = env_plan(N, M);
    if (staged) *staged = p.staged;
    if (rows_per_block) *rows_per_block = p.rows;
    if (lds_bytes) *lds_bytes = p.list_bytes + 256u * 3u * sizeof(float) * (size_t)m;   // + the observe kernel's parked lists
    return DRONESIM_OK;
}

int dronesim_env_obstacle_sense(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                                const int32_t *count, int E, int N, int k1, int c, int M, int m, float *orow, int32_t *oid,
                                float *gap_min, uint8_t *hit, void *stream)
{
    const char *where = "dronesim_env_obstacle_sense";
    if (!z || !xF || !radius || !sense || !orow || !oid) return fail_at(where, "NULL z / xF / radius / sense / orow / oid");
    if (E < 0) return fail_at(where, "E < 0");
    int rc = check_records(where, N, k1, 1, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK) rc = check_env_discs(where, M, obstacles);
    if (rc == DRONESIM_OK) rc = check_slots(where, m);
    if (rc != DRONESIM_OK || E == 0) return rc;
    const EnvPlan plan = env_plan(N, M);
    EnvSenseArgs a;
    a.z = z; a.xF = xF; a.radius = radius; a.sense = sense; a.orow = orow; a.oid = oid; a.gap_min = gap_min; a.hit = hit;
    a.N = N; a.stride = k1 * c; a.W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z));
    a.records = (unsigned long long)E * (unsigned long long)N;
    a.L = env_lists_of(obstacles, count, E, M, plan);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
#define DRONESIM_ENV_SENSE(MS)                                                                                            \
    do {                                                                                                                  \
        if (plan.staged) hipLaunchKernelGGL((env_obstacle_sense_kernel<MS, true>), grid, dim3(256), plan.list_bytes, s, a); \
        else hipLaunchKernelGGL((env_obstacle_sense_kernel<MS, false>), grid, dim3(256), 0, s, a);                         \
    } while (0)
    if (m == 1) DRONESIM_ENV_SENSE(1);
    else if (m == 2) DRONESIM_ENV_SENSE(2);
    else if (m == 3) DRONESIM_ENV_SENSE(3);
    else DRONESIM_ENV_SENSE(4);
#undef DRONESIM_ENV_SENSE
    return dronesim_launched();
}

int dronesim_env_obstacle_observe(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                                  const int32_t *count, int R, int E, int N, int k1, int c, int M, int m, float *x_out,
                                  float *cost_out, float weight, void *stream)
{
    const char *where = "dronesim_env_obstacle_observe";
    if (!z || !xF || !radius || !sense || !x_out) return fail_at(where, "NULL z / xF / radius / sense / x_out");
    if (R < 0 || E < 0) return fail_at(where, "R or E < 0");
    if (R > 0 && (E == 0 || R % E != 0)) return fail_at(where, "R must be a multiple of E (row q belongs to env q % E)");
    int rc = check_records(where, N, k1, 1, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK) rc = check_env_discs(where, M, obstacles);
    if (rc == DRONESIM_OK) rc = check_slots(where, m);
    if (rc == DRONESIM_OK) rc = check_weight(where, weight);
    if (rc != DRONESIM_OK || R == 0) return rc;
    const EnvPlan plan = env_plan(N, M);
    EnvObserveArgs a;
    a.z = z; a.xF = xF; a.radius = radius; a.sense = sense; a.x_out = x_out; a.cost = cost_out; a.weight = weight;
    a.N = N; a.stride = k1 * c; a.W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z));
    a.OW = (reinterpret_cast<uintptr_t>(x_out) & 15u) == 0 ? 4 : 1;
    a.records = (unsigned long long)R * (unsigned long long)N;
    a.L = env_lists_of(obstacles, count, E, M, plan);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
#define DRONESIM_ENV_OBSERVE2(MS, COST)                                                                                            \
    do {                                                                                                                           \
        if (plan.staged) hipLaunchKernelGGL((env_obstacle_observe_kernel<MS, COST, true>), grid, dim3(256), plan.list_bytes, s, a); \
        else hipLaunchKernelGGL((env_obstacle_observe_kernel<MS, COST, false>), grid, dim3(256), 0, s, a);                          \
    } while (0)
#define DRONESIM_ENV_OBSERVE(MS)                         \
    do {                                                 \
        if (cost_out) DRONESIM_ENV_OBSERVE2(MS, true);   \
        else DRONESIM_ENV_OBSERVE2(MS, false);           \
    } while (0)
    if (m == 1) DRONESIM_ENV_OBSERVE(1);
    else if (m == 2) DRONESIM_ENV_OBSERVE(2);
    else if (m == 3) DRONESIM_ENV_OBSERVE(3);
    else DRONESIM_ENV_OBSERVE(4);
#undef DRONESIM_ENV_OBSERVE
#undef DRONESIM_ENV_OBSERVE2
    return dronesim_launched();
}

int dronesim_env_obstacle_reward(const float *z_post, const float *z_final, const uint8_t *done, const float *reward, const float *xF,
                                 const float *radius, const float *sense, const float *obstacles, const int32_t *count, int T, int E,
                                 int N, int k1, int c, int M, float weight, float *reward_out, float *cost_out, void *stream)
{
    const char *where = "dronesim_env_obstacle_reward";
    if (!z_post || !done || !reward || !xF || !radius || !sense || !reward_out)
        return fail_at(where, "NULL z_post / done / reward / xF / radius / sense / reward_out");
    if (T < 0 || E < 0) return fail_at(where, "T or E < 0");
    int rc = check_records(where, N, k1, 1, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK) rc = check_env_discs(where, M, obstacles);
    if (rc == DRONESIM_OK) rc = check_weight(where, weight);
    if (rc != DRONESIM_OK || T == 0 || E == 0) return rc;
    const EnvPlan plan = env_plan(N, M);
    EnvRewardArgs a;
    a.z_post = z_post; a.z_final = z_final; a.done = done; a.reward = reward; a.xF = xF; a.radius = radius; a.sense = sense;
    a.reward_out = reward_out; a.cost = cost_out; a.weight = weight;
    a.N = N; a.stride = k1 * c;
    a.W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z_post) | reinterpret_cast<uintptr_t>(z_final));
    a.records = (unsigned long long)T * (unsigned long long)E * (unsigned long long)N;
    a.L = env_lists_of(obstacles, count, E, M, plan);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
    if (plan.staged) hipLaunchKernelGGL(env_obstacle_reward_kernel<true>, grid, dim3(256), plan.list_bytes, s, a);
    else hipLaunchKernelGGL(env_obstacle_reward_kernel<false>, grid, dim3(256), 0, s, a);
    return dronesim_launched();
}

int dronesim_episode_env_obstacle_safety(const float *z, const float *z_final, const uint8_t *done, const float *xF,
                                         const float *radius, const float *obstacles, const int32_t *count, int T, int E, int N,
                                         int k1, int c, int M, int32_t *ep_len, float *min_obstacle_gap, int32_t *obstacle_hit_steps,
                                         float *ep_min_obstacle_gap, int32_t *ep_obstacle_hit_steps, void *stream)
{
    const char *where = "dronesim_episode_env_obstacle_safety";
    if (T < 0 || E < 0) return fail_at(where, "T or E < 0");
    int rc = check_records(where, N, k1, 1, INT_MAX, c);
    if (rc == DRONESIM_OK) rc = check_env_discs(where, M, obstacles);
    if (rc != DRONESIM_OK) return rc;
    if ((ep_min_obstacle_gap && !min_obstacle_gap) || (ep_obstacle_hit_steps && !obstacle_hit_steps))
        return fail_at(where, "a per-env table needs the per-agent one it reduces");
    if (E == 0) return DRONESIM_OK;                            // (an empty window has no addresses: checked before the pointers)
    if (!xF || !radius || !ep_len || (T > 0 && (!z || !done))) return fail_at(where, "NULL z / done / xF / radius / ep_len");
    const size_t cols = (size_t)E * N;
    // a thread reads floats 0, 1 of a record: the scan has no 16-byte variant, a rule's 4 is served by the 8-byte one
    const int W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(z_final));
    const EnvPlan plan = env_plan(N, M);
    const EnvLists L = env_lists_of(obstacles, count, E, M, plan);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((cols + 255) / 256));
#define DRONESIM_ENV_SCAN(WW, ST)                                                                                             \
    do {                                                                                                                      \
        EnvObstacleScan<WW, ST> p{};                                                                                          \
        p.z = z; p.z_final = z_final; p.flags = done; p.xF = xF; p.radius = radius; p.N = N; p.stride = k1 * c;               \
        hipLaunchKernelGGL((episode_env_obstacle_kernel<WW, ST>), grid, dim3(256), ST ? plan.list_bytes : 0, s, p, L, ep_len, \
                           min_obstacle_gap, obstacle_hit_steps, T, E);                                                       \
    } while (0)
    if (W >= 2) {
        if (plan.staged) DRONESIM_ENV_SCAN(2, true);
        else DRONESIM_ENV_SCAN(2, false);
    } else {
        if (plan.staged) DRONESIM_ENV_SCAN(1, true);
        else DRONESIM_ENV_SCAN(1, false);
    }
#undef DRONESIM_ENV_SCAN
    rc = dronesim_launched();
    if (rc != DRONESIM_OK || !(ep_min_obstacle_gap || ep_obstacle_hit_steps)) return rc;
    hipLaunchKernelGGL(obstacle_env_kernel, dim3((unsigned)((2 * (size_t)E + 255) / 256)), dim3(256), 0, s, ep_len, min_obstacle_gap,
                       obstacle_hit_steps, ep_min_obstacle_gap, ep_obstacle_hit_steps, E, N);
    return dronesim_launched();
}

}   // extern "C"
