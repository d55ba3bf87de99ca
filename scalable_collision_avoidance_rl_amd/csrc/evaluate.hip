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
// dronesim_episode_safety (below) reduces the same first episode from the stored observations: clearance, goal distance, arrival.
#include "record_entry.hpp"
#include "scan_common.hpp"

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

// Per-episode safety tables from the stored OBSERVATIONS (dronesim_episode_safety): how close every agent of an env's first
// episode came to another one, how far from its goal it ended and when it first stood inside its goal disk.  The same backward
// scan with the same restart at `done` (scan_common.hpp's pipelined driver, V = 1), over strided records instead of dense
// [T][E N] planes: thread (e, i) needs floats 0, 1 (row 0: x_i - xF_i) and c, c + 1 (row 1: x_j - x_i of the closest neighbour)
// of record [t][e][i] of k1 c floats, and the id in slot 1 of its neighbour list.  Consecutive threads read consecutive
// records, so every 64-byte segment of z and nbr is fetched once; what varies is the width of the loads that alignment allows:
//   W = 4   c = 2, k1 even, bases 16-byte aligned: the record stride 8 k1 is a multiple of 16 -- both rows as ONE 16-byte load
//   W = 2   c = 2, bases 8-byte aligned: rows start at multiples of 8 -- one 8-byte load per row
//   W = 1   anything else: dword loads.  With c = 5 a record is 20 k1 bytes and row 1 starts at byte 20: nothing wider is aligned.
// A step that ends an episode takes its observation from z_final / nbr_final when they are given (under auto_reset z[t] is then
// the NEXT episode's first observation); such steps are rare (about one per env and 100 steps), their record is loaded where
// it is needed, as EndsScan loads Vend.
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }   // numpy.minimum: a NaN stays
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

struct SafetyRec { float zx, zy, nx, ny; };

template <int W, bool NT>
__device__ __forceinline__ SafetyRec safety_record(const float *__restrict__ p, int c)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    SafetyRec r;
    if (W == 4) {
        const f4 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p)) : *reinterpret_cast<const f4 *>(p);
        r.zx = v.x; r.zy = v.y; r.nx = v.z; r.ny = v.w;
    } else if (W == 2) {                                       // (plain loads: the second one finds the first one's lines)
        const f2 a = *reinterpret_cast<const f2 *>(p), b = *reinterpret_cast<const f2 *>(p + 2);
        r.zx = a.x; r.zy = a.y; r.nx = b.x; r.ny = b.y;
    } else {
        r.zx = p[0]; r.zy = p[1]; r.nx = p[c]; r.ny = p[c + 1];
    }
    return r;
}

template <int W> struct SafetyScan {
    static constexpr bool kBeginFirst = false;
    typedef bool Flag;
    struct Rows { SafetyRec rec[kStageT]; int j[kStageT]; };
    struct State { float clr, goal, ri, di; int arrive, L; };  // ri, di: the column's own radius and Delta
    const float *z, *z_final;
    const int32_t *nbr, *nbr_final;
    const uint8_t *flags;
    const float *radius, *delta;
    float done_radius;
    int N, k1, c;
    __device__ __forceinline__ State begin(const ScanCols<1> &cols, int) const
    {
        const size_t i = cols.col - cols.e * (size_t)N;
        const float di = delta[i];
        return State{di, di, radius[i], di, -1, 0};
    }
    __device__ __forceinline__ void load(Rows &st, int u, int t, const ScanCols<1> &cols) const
    {
        if (t >= 0) {
            const size_t at = (size_t)t * cols.EN + cols.col;
            st.rec[u] = safety_record<W, true>(z + at * (size_t)(k1 * c), c);
            st.j[u] = __builtin_nontemporal_load(nbr + at * (size_t)k1 + 1);
        } else {
            st.rec[u] = SafetyRec{0.0f, 0.0f, 0.0f, 0.0f};
            st.j[u] = -1;
        }
    }
    __device__ __forceinline__ bool own(int t, const ScanCols<1> &cols) const
    {
        return t >= 0 && flags[(size_t)t * cols.E + cols.e] != 0;
    }
    template <bool COOP>
    __device__ __forceinline__ void step(State &s, const ScanStage<SafetyScan> &st, int u, int t, const ScanCols<1> &cols) const
    {
        const bool dn = COOP ? st.ds.get(cols.de, u) : st.flag[u];
        SafetyRec r = st.rows.rec[u];
        int j = st.rows.j[u];
        if (dn && z_final) {                                   // rare: the finished episode's terminal observation
            const size_t at = (size_t)t * cols.EN + cols.col;
            r = safety_record<W, false>(z_final + at * (size_t)(k1 * c), c);
            j = nbr_final[at * (size_t)k1 + 1];
        }
        const float goal = __builtin_amdgcn_sqrtf(fmaf(r.zy, r.zy, r.zx * r.zx));       // ends_classify_kernel's test (scans.hip)
        const bool inside = goal <= done_radius;
        float clr = s.di;
        if ((unsigned)j < (unsigned)N)                          // a ghost row or an id outside [0, N) never indexes radius
            clr = nan_min(__builtin_amdgcn_sqrtf(fmaf(r.ny, r.ny, r.nx * r.nx)) - s.ri - radius[j], s.di);
        if (dn) {
            s.clr = clr; s.goal = goal; s.arrive = inside ? t + 1 : -1; s.L = t + 1;
        } else {
            s.clr = nan_min(clr, s.clr);
            s.arrive = inside ? t + 1 : s.arrive;
        }
    }
};

struct SafetyOut {
    int32_t *ep_len, *arrive_step;
    float *min_clearance, *goal_dist_final;
};

template <int W>
__global__ void __launch_bounds__(256) episode_safety_kernel(const SafetyScan<W> p, const SafetyOut o, int T, int E)
{
    const ScanCols<1> c(E, p.N);
    const bool coop = c.within_stage();
    typename SafetyScan<W>::State s;
    if (coop) s = scan_backward<true, 1>(p, c, T);
    else s = scan_backward<false, 1>(p, c, T);
    if (!c.act) return;
    const bool valid = s.L > 0;                                // no episode: NaN (0 is a meaningful clearance), -1
    const float nan = __builtin_nanf("");
    if (o.min_clearance) o.min_clearance[c.col] = valid ? s.clr : nan;
    if (o.goal_dist_final) o.goal_dist_final[c.col] = valid ? s.goal : nan;
    if (o.arrive_step) o.arrive_step[c.col] = valid ? s.arrive : -1;
    if (c.col == c.e * (size_t)p.N) o.ep_len[c.e] = s.L;       // the env's first column reports its length
}

// Per env, agents in ascending order: task 0 the smallest clearance, task 1 the largest final goal distance and whether every
// agent ended inside its goal disk (the test on the stored float32 distance: the scan's own bits).
__global__ void __launch_bounds__(256) safety_env_kernel(const int32_t *__restrict__ ep_len, const float *__restrict__ min_clearance,
                                                         const float *__restrict__ goal_dist_final, float done_radius,
                                                         float *__restrict__ ep_min_clearance, float *__restrict__ ep_goal_dist_max,
                                                         uint8_t *__restrict__ ep_arrived, int E, int N)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * (size_t)E) return;
    const int task = (int)(idx / (size_t)E);
    const size_t e = idx - (size_t)task * E;
    const bool valid = ep_len[e] > 0;
    const float nan = __builtin_nanf("");
    if (task == 0) {
        if (!ep_min_clearance) return;
        float m = nan;
        if (valid) {
            m = min_clearance[e * N];
            for (int i = 1; i < N; ++i) m = nan_min(min_clearance[e * N + i], m);
        }
        ep_min_clearance[e] = m;
        return;
    }
    if (!ep_goal_dist_max && !ep_arrived) return;
    float m = nan;
    bool outside = !valid;
    if (valid) {
        m = goal_dist_final[e * N];
        outside = !(m <= done_radius);
        for (int i = 1; i < N; ++i) {
            const float g = goal_dist_final[e * N + i];
            m = nan_max(g, m);
            outside |= !(g <= done_radius);
        }
    }
    if (ep_goal_dist_max) ep_goal_dist_max[e] = m;
    if (ep_arrived) ep_arrived[e] = outside ? 0 : 1;
}

}   // namespace

extern "C" {

int dronesim_episode_eval(const float *reward, const float *true_reward, const int32_t *n_coll, const uint8_t *done,
                          const float *V, float gamma, int32_t *ep_len, int32_t *ep_collisions,
                          double *agent_return, double *agent_true_return, double *ep_return, double *ep_true_return,
                          float *G, double *mean_adv, int T, int E, int N, void *stream)
{
    const char *where = "dronesim_episode_eval";
    if (!reward || !true_reward || !done || !ep_len) return fail_at(where, "NULL reward / true_reward / done / ep_len");
    if (T < 0 || E < 0 || N < 1) return fail_at(where, "T or E < 0, or N < 1");
    if (ep_collisions && !n_coll) return fail_at(where, "ep_collisions needs n_coll");
    if (mean_adv && !V) return fail_at(where, "mean_adv needs V");
    if ((ep_return && !agent_return) || (ep_true_return && !agent_true_return))
        return fail_at(where, "ep_return / ep_true_return need agent_return / agent_true_return");
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

int dronesim_episode_safety(const float *z, const int32_t *nbr, const float *z_final, const int32_t *nbr_final, const uint8_t *done,
                            const float *radius, const float *delta, float done_radius, int T, int E, int N, int k1, int c,
                            int32_t *ep_len, float *min_clearance, float *goal_dist_final, int32_t *arrive_step,
                            float *ep_min_clearance, float *ep_goal_dist_max, uint8_t *ep_arrived, void *stream)
{
    const char *where = "dronesim_episode_safety";
    if (!z || !nbr || !done || !radius || !delta || !ep_len) return fail_at(where, "NULL z / nbr / done / radius / delta / ep_len");
    if (T < 0 || E < 0) return fail_at(where, "T or E < 0");
    int rc = check_records(where, N, k1, 2, INT_MAX, c);
    if (rc != DRONESIM_OK) return rc;
    if (done_radius != done_radius) return fail_at(where, "done_radius is NaN");
    if ((z_final == nullptr) != (nbr_final == nullptr)) return fail_at(where, "z_final and nbr_final go together");
    if ((ep_min_clearance && !min_clearance) || ((ep_goal_dist_max || ep_arrived) && !goal_dist_final))
        return fail_at(where, "ep_min_clearance needs min_clearance, ep_goal_dist_max / ep_arrived need goal_dist_final");
    if (E == 0) return DRONESIM_OK;
    const size_t cols = (size_t)E * N;
    const SafetyOut o{ep_len, arrive_step, min_clearance, goal_dist_final};
    const int W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(z_final));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((cols + 255) / 256));
    if (W == 4) {
        const SafetyScan<4> p{z, z_final, nbr, nbr_final, done, radius, delta, done_radius, N, k1, c};
        hipLaunchKernelGGL(episode_safety_kernel<4>, grid, dim3(256), 0, s, p, o, T, E);
    } else if (W == 2) {
        const SafetyScan<2> p{z, z_final, nbr, nbr_final, done, radius, delta, done_radius, N, k1, c};
        hipLaunchKernelGGL(episode_safety_kernel<2>, grid, dim3(256), 0, s, p, o, T, E);
    } else {
        const SafetyScan<1> p{z, z_final, nbr, nbr_final, done, radius, delta, done_radius, N, k1, c};
        hipLaunchKernelGGL(episode_safety_kernel<1>, grid, dim3(256), 0, s, p, o, T, E);
    }
    rc = dronesim_launched();
    if (rc != DRONESIM_OK || !(ep_min_clearance || ep_goal_dist_max || ep_arrived)) return rc;
    hipLaunchKernelGGL(safety_env_kernel, dim3((unsigned)((2 * (size_t)E + 255) / 256)), dim3(256), 0, s, ep_len, min_clearance,
                       goal_dist_final, done_radius, ep_min_clearance, ep_goal_dist_max, ep_arrived, E, N);
    return dronesim_launched();
}

int dronesim_histogram_i32(const int32_t *values, const uint8_t *valid, int E, int n_bins, int64_t *counts, int accumulate,
                           void *stream)
{
    if (!values || !counts || E < 0 || n_bins < 1 || n_bins > (1 << 24))
        return fail_at("dronesim_histogram_i32", "NULL values / counts, E < 0 or n_bins outside 1..2^24");
    hipLaunchKernelGGL(histogram_kernel, dim3(1), dim3(kHistThreads), 0, static_cast<hipStream_t>(stream), values, valid, E, n_bins,
                       reinterpret_cast<long long *>(counts), accumulate);
    return dronesim_launched();
}

}   // extern "C"
