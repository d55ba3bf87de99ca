// scans.hip -- the learner-side scans over a stored rollout [T][E][N] (SAC_agents.py:304-307, 333-351) behind
// include/dronesim.h: Monte-Carlo returns, bootstrapped lambda-returns with and without the kinds of the episode ends (two
// policies of scan_common.hpp's pipelined driver), the classification of those ends, and the two advantages.
#include "scan_common.hpp"
#include "dronesim.h"

namespace {

// Monte-Carlo returns: G[t] = fma(G[t+1], gamma, r[t]), in order; an episode restarts behind `done` and the window's last
// step counts as one.  Its own copy of the driver's loop: as a policy its quadruple kernel took 98 VGPRs, not 96 (4 waves, not 5).
template <int V> struct RetStage {
    typename ColVec<V>::type r[kStageT];
    DoneStage ds;
    bool last[kStageT];
};

template <bool COOP, int V>
__device__ __forceinline__ void returns_fetch(RetStage<V> &st, const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                              size_t EN, size_t col, size_t e, size_t e_first, int E, int T, int t0)
{
    typedef typename ColVec<V>::type vec;
    if (COOP) st.ds.fetch(done, e_first, E, T, [&](int u) { return t0 - u; });
#pragma unroll
    for (int u = 0; u < kStageT; ++u) {
        const int t = t0 - u;
        st.r[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(reward + (size_t)t * EN + col)) : vec(0.0f);
        if (!COOP) st.last[u] = t == T - 1 || (done != nullptr && t >= 0 && done[(size_t)t * E + e] != 0);
    }
}

template <bool COOP, int V>
__device__ __forceinline__ void returns_scan(const float *__restrict__ reward, const uint8_t *__restrict__ done, float gamma,
                                             float *__restrict__ G, int T, int E, size_t EN, size_t col, size_t e,
                                             size_t e_first, int de, bool act)
{
    typedef typename ColVec<V>::type vec;
    vec g = vec(0.0f);
    RetStage<V> cur, nxt;
    returns_fetch<COOP, V>(cur, reward, done, EN, col, e, e_first, E, T, T - 1);
    for (int t0 = T - 1; t0 >= 0; t0 -= kStageT) {
        if (t0 - kStageT >= 0) returns_fetch<COOP, V>(nxt, reward, done, EN, col, e, e_first, E, T, t0 - kStageT);
#pragma unroll
        for (int u = 0; u < kStageT; ++u) {
            const int t = t0 - u;
            if (t >= 0) {
                const bool last = COOP ? (t == T - 1 || cur.ds.get(de, u)) : cur.last[u];
                if (V == 1) {
                    g = last ? cur.r[u] : vec(fmaf(*reinterpret_cast<float *>(&g), gamma, *reinterpret_cast<const float *>(&cur.r[u])));   // :306  Gt[t] = Gt[t+1]*discount + r[t]
                } else {
                    float *gp = reinterpret_cast<float *>(&g);
                    const float *rp = reinterpret_cast<const float *>(&cur.r[u]);
#pragma unroll
                    for (int q = 0; q < V; ++q) gp[q] = last ? rp[q] : fmaf(gp[q], gamma, rp[q]);                                         // :306
                }
                if (act) __builtin_nontemporal_store(g, reinterpret_cast<vec *>(G + (size_t)t * EN + col));
            }
        }
        cur = nxt;
    }
}

template <int V>
__global__ void __launch_bounds__(256) returns_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                      float gamma, float *__restrict__ G, int T, int E, int N)
{
    const ScanCols<V> c(E, N);
    const bool coop = done != nullptr && c.within_stage();
    if (coop) returns_scan<true, V>(reward, done, gamma, G, T, E, c.EN, c.col, c.e, c.e_first, c.de, c.act);
    else returns_scan<false, V>(reward, done, gamma, G, T, E, c.EN, c.col, c.e, c.e_first, c.de, c.act);
}

// Bootstrapped lambda-returns (TD(lambda) / GAE): the returns scan with one more input stream -- the values Vv [T+1][E][N],
// Vv[t] the value of the observation step t acted on, Vv[T] that of the observation after the window -- and up to two outputs:
//     G[t] = done[t] ? r[t] : r[t] + gamma ((1 - lam) Vv[t+1] + lam G[t+1]),   G[T] = Vv[T];      A[t] = G[t] - Vv[t]
// Vv[t+1] of step t is Vv[t] of step t + 1: every row is loaded once and carried in `vn`.  At lam = 1 the mix
// fmaf(1, Gn, 0 * Vn) is Gn itself, so the step is returns_scan's fmaf(Gn, gamma, r) and a column whose window ends with
// `done` gets dronesim_returns' bits.  (The window's last step is NOT an end here: it bootstraps.)
template <int V> struct LambdaScan {
    typedef typename ColVec<V>::type vec;
    static constexpr bool kBeginFirst = true;
    typedef bool Flag;
    struct Rows { vec r[kStageT], v[kStageT]; };
    struct State { vec g, vn; float oml; };
    const float *reward, *Vv;
    const uint8_t *flags;
    float gamma, lam;
    float *G, *A;
    __device__ __forceinline__ State begin(const ScanCols<V> &c, int T) const
    {
        const float oml = 1.0f - lam;
        const vec vn = __builtin_nontemporal_load(reinterpret_cast<const vec *>(Vv + (size_t)T * c.EN + c.col));   // the bootstrap: Gn = Vv[T]
        return State{vn, vn, oml};
    }
    __device__ __forceinline__ void load(Rows &st, int u, int t, const ScanCols<V> &c) const
    {
        st.r[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(reward + (size_t)t * c.EN + c.col)) : vec(0.0f);
        st.v[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(Vv + (size_t)t * c.EN + c.col)) : vec(0.0f);
    }
    __device__ __forceinline__ bool own(int t, const ScanCols<V> &c) const
    {
        return flags != nullptr && t >= 0 && flags[(size_t)t * c.E + c.e] != 0;
    }
    template <bool COOP>
    __device__ __forceinline__ void step(State &s, const ScanStage<LambdaScan> &st, int u, int t, const ScanCols<V> &c) const
    {
        const Rows &cur = st.rows;
        const bool last = COOP ? st.ds.get(c.de, u) : st.flag[u];
        vec g = s.g, vn = s.vn;
        const float oml = s.oml;
        float *gp = reinterpret_cast<float *>(&g);
        const float *rp = reinterpret_cast<const float *>(&cur.r[u]), *vp = reinterpret_cast<const float *>(&vn);
#pragma unroll
        for (int q = 0; q < V; ++q) gp[q] = last ? rp[q] : fmaf(fmaf(lam, gp[q], oml * vp[q]), gamma, rp[q]);
        vn = cur.v[u];
        if (c.act) {
            if (G) __builtin_nontemporal_store(g, reinterpret_cast<vec *>(G + (size_t)t * c.EN + c.col));
            if (A) __builtin_nontemporal_store(g - vn, reinterpret_cast<vec *>(A + (size_t)t * c.EN + c.col));
        }
        s.g = g; s.vn = vn;
    }
};

template <int V>
__global__ void __launch_bounds__(256) lambda_returns_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                             const float *__restrict__ Vv, float gamma, float lam,
                                                             float *__restrict__ G, float *__restrict__ A, int T, int E, int N)
{
    const ScanCols<V> c(E, N);
    const LambdaScan<V> p{reward, Vv, done, gamma, lam, G, A};
    const bool coop = done != nullptr && c.within_stage();
    if (coop) scan_backward<true, V>(p, c, T);
    else scan_backward<false, V>(p, c, T);
}

// LambdaScan with the KIND of every episode end in the place of `done` ("Time-limit ends"):
//     ends[t][e] = 0   G[t] = r[t] + gamma ((1 - lam) Vv[t+1] + lam G[t+1])                       LambdaScan's step
//     ends[t][e] = 1   G[t] = r[t]                                              terminal:         LambdaScan's done step
//     ends[t][e] = 2   G[t] = r[t] + gamma Vend[k][e][i],  k += 1               truncated (time limit): the bootstrap is the
//                                                                               value of the episode's terminal observation
// k counts the column's truncated ends from the back of the window; an end with k >= M is folded as terminal.  The flag is the
// byte instead of a bool; the Vend row is loaded at the step that needs it and at no other (about one step in 200 per env:
// the wave waits for it there).
template <int V> struct EndsScan {
    typedef typename ColVec<V>::type vec;
    static constexpr bool kBeginFirst = false;
    typedef unsigned Flag;
    struct Rows { vec r[kStageT], v[kStageT]; };
    struct State { vec g, vn; int k; };                       // k: truncated ends of this column's env met so far
    const float *reward, *Vv, *Vend;
    const uint8_t *flags;
    int M;
    float gamma, lam, oml;                                     // oml = 1 - lam, from the kernel (in begin() hipcc forms it in both flag branches)
    float *G, *A;
    __device__ __forceinline__ State begin(const ScanCols<V> &c, int T) const
    {
        const vec vn = __builtin_nontemporal_load(reinterpret_cast<const vec *>(Vv + (size_t)T * c.EN + c.col));   // the bootstrap: Gn = Vv[T]
        return State{vn, vn, 0};
    }
    __device__ __forceinline__ void load(Rows &st, int u, int t, const ScanCols<V> &c) const
    {
        st.r[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(reward + (size_t)t * c.EN + c.col)) : vec(0.0f);
        st.v[u] = t >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const vec *>(Vv + (size_t)t * c.EN + c.col)) : vec(0.0f);
    }
    __device__ __forceinline__ unsigned own(int t, const ScanCols<V> &c) const { return t >= 0 ? (unsigned)flags[(size_t)t * c.E + c.e] : 0u; }
    template <bool COOP>
    __device__ __forceinline__ void step(State &s, const ScanStage<EndsScan> &st, int u, int t, const ScanCols<V> &c) const
    {
        const Rows &cur = st.rows;
        const unsigned kind = COOP ? st.ds.byte(c.de, u) : st.flag[u];
        vec g = s.g, vn = s.vn;
        int k = s.k;
        float *gp = reinterpret_cast<float *>(&g);
        const float *rp = reinterpret_cast<const float *>(&cur.r[u]), *vp = reinterpret_cast<const float *>(&vn);
        if (kind == 2u && k < M) {                             // rare: the value of the terminal observation, slot k of this env
            const vec ve = *reinterpret_cast<const vec *>(Vend + (size_t)k * c.EN + c.col);
            const float *ep = reinterpret_cast<const float *>(&ve);
#pragma unroll
            for (int q = 0; q < V; ++q) gp[q] = fmaf(ep[q], gamma, rp[q]);
            ++k;
        } else {
            const bool last = kind != 0u;
#pragma unroll
            for (int q = 0; q < V; ++q) gp[q] = last ? rp[q] : fmaf(fmaf(lam, gp[q], oml * vp[q]), gamma, rp[q]);
        }
        vn = cur.v[u];
        if (c.act) {
            if (G) __builtin_nontemporal_store(g, reinterpret_cast<vec *>(G + (size_t)t * c.EN + c.col));
            if (A) __builtin_nontemporal_store(g - vn, reinterpret_cast<vec *>(A + (size_t)t * c.EN + c.col));
        }
        s.g = g; s.vn = vn; s.k = k;
    }
};

template <int V>
__global__ void __launch_bounds__(256) lambda_returns_ends_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ ends,
                                                                  const float *__restrict__ Vv, const float *__restrict__ Vend,
                                                                  int M, float gamma, float lam, float *__restrict__ G,
                                                                  float *__restrict__ A, int T, int E, int N)
{
    const ScanCols<V> c(E, N);
    const EndsScan<V> p{reward, Vv, Vend, ends, M, gamma, lam, 1.0f - lam, G, A};
    const bool coop = c.within_stage();
    if (coop) scan_backward<true, V>(p, c, T);
    else scan_backward<false, V>(p, c, T);
}

// The kind of every episode end of a stored window, recovered from the window itself (dronesim_episode_ends; DESIGN.md,
// "Time-limit ends").  done = "every agent within done_radius of its goal" OR "time limit", and under auto_reset the terminal
// observation of every finished episode is in z_final[t]: agent i's offset from its goal is the first two floats of its row.
// So a set `done` with some agent outside the disk can only be the time limit.
//
// Stage 1: ends[t][e] = 0 / 1 (terminal) / 2 (truncated), before any demotion.  A wave takes 64 consecutive entries of `done`
// in its own [T][E] order (coalesced byte loads) and ballots them; set entries are rare (about E per 200 steps), and for each
// the WHOLE wave reads that env's N offsets (lane = agent, strided by 64 above 64 agents) and ballots the step kernel's own
// arrival test, !(sqrt(fma(zy, zy, zx zx)) <= done_radius): a non-finite offset counts as outside.
__global__ void __launch_bounds__(256) ends_classify_kernel(const uint8_t *__restrict__ done, const float *__restrict__ z_final,
                                                            size_t total, int N, int d, float done_radius, uint8_t *__restrict__ ends)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t base = wave * 64; base < total; base += nwaves * 64) {      // (wave-uniform trip count: the ballots are wave operations)
        const size_t idx = base + lane;
        const bool set = idx < total && done[idx] != 0;
        unsigned long long m = __builtin_amdgcn_ballot_w64(set);
        unsigned kind = set ? 1u : 0u;
        while (m) {
            const unsigned b = (unsigned)__builtin_ctzll(m);
            m &= m - 1ull;
            const float *rows = z_final + (base + b) * (size_t)N * d;       // (base + b < total: its lane saw a set flag)
            bool outside = false;
            for (int i = (int)lane; i < N; i += 64) {
                const float zx = rows[(size_t)i * d], zy = rows[(size_t)i * d + 1];
                outside |= !(__builtin_amdgcn_sqrtf(fmaf(zy, zy, zx * zx)) <= done_radius);
            }
            if (__builtin_amdgcn_ballot_w64(outside) != 0ull && lane == b) kind = 2u;
        }
        if (idx < total) ends[idx] = (uint8_t)kind;
    }
}

// Stage 2: one thread per env walks ends[:, e] backwards (coalesced across envs, eight steps requested together), ranks the
// truncated ends from the back of the window -- slot_t[k][e] = t of the k-th, -1 where there is none --, demotes those with
// k >= M to terminal in place, and writes n_trunc[e], the count before the demotion.
__global__ void __launch_bounds__(256) ends_rank_kernel(uint8_t *__restrict__ ends, int T, int E, int M, int32_t *__restrict__ slot_t,
                                                        int32_t *__restrict__ n_trunc)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= E) return;
    int k = 0;
    for (int t0 = T - 1; t0 >= 0; t0 -= kStageT) {
        unsigned kind[kStageT];
#pragma unroll
        for (int u = 0; u < kStageT; ++u) kind[u] = t0 - u >= 0 ? (unsigned)ends[(size_t)(t0 - u) * E + e] : 0u;
#pragma unroll
        for (int u = 0; u < kStageT; ++u) {
            if (kind[u] == 2u) {
                if (k < M) slot_t[(size_t)k * E + e] = t0 - u;
                else ends[(size_t)(t0 - u) * E + e] = (uint8_t)1;
                ++k;
            }
        }
    }
    n_trunc[e] = k;
    for (int m = k; m < M; ++m) slot_t[(size_t)m * E + e] = -1;
}

// Stage 3: z_trunc[m][e] = z_final[slot_t[m][e]][e], all zeros where slot_t is -1: every element is written here (no memset,
// no uninitialised row reaches the critic).  An (m, e) block is N d floats; VW floats per lane, lanes contiguous.
template <int VW>
__global__ void __launch_bounds__(256) ends_gather_kernel(const float *__restrict__ z_final, const int32_t *__restrict__ slot_t,
                                                          int E, size_t per_block, size_t items, float *__restrict__ z_trunc)
{
    typedef typename ColVec<VW>::type vec;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const size_t blk = it / per_block, within = it - blk * per_block;   // blk = m E + e
        const int t = slot_t[blk];
        const size_t e = blk % (size_t)E;
        vec v = vec(0.0f);
        if (t >= 0) v = __builtin_nontemporal_load(reinterpret_cast<const vec *>(z_final) + ((size_t)t * E + e) * per_block + within);
        reinterpret_cast<vec *>(z_trunc)[it] = v;
    }
}

// K1C = K + 1 at compile time (3 for the reference's k_closest = 2: the neighbour triple is one 12-byte load), 0 = any
// K1 at run time.  A stage of eight steps requests V and the neighbour ids of all eight first, then the G values they
// name (slot 0 is the agent itself: a coalesced row read; the others fall into the same 4 N-byte row), then folds.
template <int K1C>
__global__ void __launch_bounds__(256) advantage_kernel(const float *__restrict__ G, const float *__restrict__ V,
                                                        const int *__restrict__ nbr, const uint8_t *__restrict__ done,
                                                        float gamma, float *__restrict__ w, int T, int E, int N, int K1)
{
    const ScanCols<1> c(E, N);
    const size_t EN = c.EN, col = c.col, e = c.e, e_first = c.e_first;
    const int de = c.de;
    const bool act = c.act, coop = done != nullptr && c.within_stage();
    double disc = 1.0;                                         // gamma^t kept in double: 200 products stay exact to f32
    const float inv_n = 1.0f / (float)N;
    for (int t0 = 0; t0 < T; t0 += kStageT) {
        DoneStage ds;
        if (coop) ds.fetch(done, e_first, E, T, [&](int u) { return t0 + u; });
        if (K1C > 0) {
            float v[kStageT], adv[kStageT];
            int j[kStageT][K1C > 0 ? K1C : 1];
            float g[kStageT][K1C > 0 ? K1C : 1];
#pragma unroll
            for (int u = 0; u < kStageT; ++u) {
                const int t = min(t0 + u, T - 1);
                const size_t o = (size_t)t * EN + col;
                v[u] = __builtin_nontemporal_load(V + o);
#pragma unroll
                for (int q = 0; q < K1C; ++q) j[u][q] = __builtin_nontemporal_load(nbr + o * K1C + q);
            }
#pragma unroll
            for (int u = 0; u < kStageT; ++u) {
                const int t = min(t0 + u, T - 1);
                const float *Grow = G + (size_t)t * EN + e * N;
#pragma unroll
                for (int q = 0; q < K1C; ++q) g[u][q] = Grow[max(j[u][q], 0)];
            }
            // (all 8 K1 gathers are requested above before the first is used, and the "no neighbour" case is an AND mask:
            // written as `j >= 0 ? gq - v : 0` hipcc puts a branch around every gather and waits for each in turn --
            // 24 round trips in series per stage, found in the ISA in round 4)
#pragma unroll
            for (int u = 0; u < kStageT; ++u) {
                float a = 0.0f;
#pragma unroll
                for (int q = 0; q < K1C; ++q)
                    a += __uint_as_float(__float_as_uint(g[u][q] - v[u]) & (j[u][q] >= 0 ? 0xffffffffu : 0u));   // :345-346  (i itself is slot 0)
                adv[u] = a;
            }
#pragma unroll
            for (int u = 0; u < kStageT; ++u) {
                const int t = t0 + u;
                if (t < T) {
                    if (act) __builtin_nontemporal_store(inv_n * (float)disc * adv[u], w + (size_t)t * EN + col);   // :351
                    const bool d = coop ? ds.get(de, u) : (done != nullptr && done[(size_t)t * E + e] != 0);
                    disc = d ? 1.0 : disc * (double)gamma;
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < kStageT; ++u) {
                const int t = t0 + u;
                if (t < T) {
                    const size_t o = (size_t)t * EN + col;
                    const float v = V[o];
                    const int *nb = nbr + o * K1;
                    const float *Grow = G + (size_t)t * EN + e * N;
                    float adv = 0.0f;
                    for (int q = 0; q < K1; ++q) {
                        const int jq = nb[q];
                        if (jq >= 0) adv += Grow[jq] - v;      // :345-346  (i itself is slot 0)
                    }
                    if (act) w[o] = inv_n * (float)disc * adv; // :351
                    const bool d = coop ? ds.get(de, u) : (done != nullptr && done[(size_t)t * E + e] != 0);
                    disc = d ? 1.0 : disc * (double)gamma;
                }
            }
        }
    }
}

// advantage_kernel's sibling for the PPO learner (SAC_agents.py:498-501, :512-513): the neighbour sum of the returns less the
// agent's own baseline, with no gamma^t and no 1 / N, so nothing runs along t and a thread owns one (t, e, i):
//   adv = sum_{j in Ni[t]} G[t, e, j] - c V[t, e, i],   c = 1 (the reference's form) or |Ni[t]| (per_neighbour).
// Coalesced reads of V and the neighbour rows and a coalesced store; the gathers of G fall into the env's own 4 N-byte row.
template <int K1C>
__global__ void __launch_bounds__(256) neighbour_advantage_kernel(const float *__restrict__ G, const float *__restrict__ V,
                                                                  const int *__restrict__ nbr, int per_neighbour,
                                                                  float *__restrict__ adv, size_t rows, int N, int K1)
{
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= rows * N) return;
    const float *Grow = G + (o / N) * N;
    const int k1 = K1C > 0 ? K1C : K1;
    float q = 0.0f;
    int cnt = 0;
    if (K1C > 0) {
        int j[K1C > 0 ? K1C : 1];
        float g[K1C > 0 ? K1C : 1];
#pragma unroll
        for (int s = 0; s < K1C; ++s) j[s] = __builtin_nontemporal_load(nbr + o * K1C + s);
#pragma unroll
        for (int s = 0; s < K1C; ++s) g[s] = Grow[max(j[s], 0)];
#pragma unroll
        for (int s = 0; s < K1C; ++s) {
            q += j[s] >= 0 ? g[s] : 0.0f;
            cnt += j[s] >= 0;
        }
    } else {
        for (int s = 0; s < k1; ++s) {
            const int js = nbr[o * k1 + s];
            if (js >= 0) { q += Grow[js]; ++cnt; }
        }
    }
    const float c = per_neighbour ? (float)cnt : 1.0f;
    adv[o] = q - c * V[o];
}

}   // namespace

extern "C" {

int dronesim_returns(const float *reward, const uint8_t *done, float gamma, float *G,
                     int T, int E, int N, void *stream)
{
    if (!reward || !G || T < 0 || E < 0 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_returns: bad argument");
    if (T == 0 || E == 0) return DRONESIM_OK;
    const size_t cols = (size_t)E * N;
    const bool v4 = column_quads(N, cols, 1048576, reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(G));
    if (v4)
        hipLaunchKernelGGL(returns_kernel<4>, dim3((unsigned)((cols / 4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           reward, done, gamma, G, T, E, N);
    else
        hipLaunchKernelGGL(returns_kernel<1>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           reward, done, gamma, G, T, E, N);
    return dronesim_launched();
}

int dronesim_lambda_returns(const float *reward, const uint8_t *done, const float *V, float gamma, float lam, float *G, float *A,
                            int T, int E, int N, void *stream)
{
    if (!reward || !V) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns: reward or V is NULL");
    if (!G && !A) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns: G and A are both NULL");
    if (T < 0 || E < 0 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns: bad T, E or N");
    if (!(lam >= 0.0f && lam <= 1.0f)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns: lam must be in [0, 1]");
    if (gamma != gamma) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns: gamma is NaN");
    if (T == 0 || E == 0) return DRONESIM_OK;
    const size_t cols = (size_t)E * N;
    const bool v4 = column_quads(N, cols, 524288, reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(V) |
                                                  reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(A));
    if (v4)
        hipLaunchKernelGGL(lambda_returns_kernel<4>, dim3((unsigned)((cols / 4 + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), reward, done, V, gamma, lam, G, A, T, E, N);
    else
        hipLaunchKernelGGL(lambda_returns_kernel<1>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), reward, done, V, gamma, lam, G, A, T, E, N);
    return dronesim_launched();
}

int dronesim_episode_ends(const uint8_t *done, const float *z_final, int T, int E, int N, int d, float done_radius,
                          uint8_t *ends, int32_t *slot_t, int32_t *n_trunc, float *z_trunc, int M, void *stream)
{
    if (!done || !z_final) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_ends: done or z_final is NULL");
    if (!ends || !slot_t || !n_trunc || !z_trunc) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_ends: an output is NULL");
    if (T < 0 || E < 0 || N < 1 || d < 2) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_ends: bad T, E, N or d");
    if (M < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_ends: M must be at least 1");
    if (done_radius != done_radius) return dronesim_fail(DRONESIM_EINVAL, "dronesim_episode_ends: done_radius is NaN");
    if (E == 0) return DRONESIM_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t total = (size_t)T * E, ND = (size_t)N * d;
    const size_t kMaxBlocks = (size_t)1 << 20;                  // (both kernels loop over what a capped grid leaves)
    const size_t cb = (total + 255) / 256;
    if (total > 0)
        hipLaunchKernelGGL(ends_classify_kernel, dim3((unsigned)(cb < kMaxBlocks ? cb : kMaxBlocks)), dim3(256), 0, s,
                           done, z_final, total, N, d, done_radius, ends);
    hipLaunchKernelGGL(ends_rank_kernel, dim3((unsigned)(((size_t)E + 255) / 256)), dim3(256), 0, s, ends, T, E, M, slot_t, n_trunc);
    // the vector width from N d, the floats of one (t, e) block (a row's d is a multiple of two floats only at c = 2), and the
    // two base addresses: every block of both arrays then starts 16-byte aligned
    const bool v4 = (ND % 4) == 0 && ((reinterpret_cast<uintptr_t>(z_final) | reinterpret_cast<uintptr_t>(z_trunc)) & 15u) == 0;
    const size_t per = v4 ? ND / 4 : ND, items = (size_t)M * E * per;
    const size_t gb = (items + 255) / 256;
    const dim3 grid((unsigned)(gb < kMaxBlocks ? gb : kMaxBlocks));
    if (v4) hipLaunchKernelGGL(ends_gather_kernel<4>, grid, dim3(256), 0, s, z_final, slot_t, E, per, items, z_trunc);
    else hipLaunchKernelGGL(ends_gather_kernel<1>, grid, dim3(256), 0, s, z_final, slot_t, E, per, items, z_trunc);
    return dronesim_launched();
}

int dronesim_lambda_returns_ends(const float *reward, const uint8_t *ends, const float *V, const float *Vend, int M, float gamma,
                                 float lam, float *G, float *A, int T, int E, int N, void *stream)
{
    if (!reward || !V) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: reward or V is NULL");
    if (!ends || !Vend) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: ends or Vend is NULL");
    if (!G && !A) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: G and A are both NULL");
    if (T < 0 || E < 0 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: bad T, E or N");
    if (M < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: M must be at least 1");
    if (!(lam >= 0.0f && lam <= 1.0f)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: lam must be in [0, 1]");
    if (gamma != gamma) return dronesim_fail(DRONESIM_EINVAL, "dronesim_lambda_returns_ends: gamma is NaN");
    if (T == 0 || E == 0) return DRONESIM_OK;
    const size_t cols = (size_t)E * N;
    const bool v4 = column_quads(N, cols, 524288, reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(V) |
                                                  reinterpret_cast<uintptr_t>(Vend) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(A));
    if (v4)
        hipLaunchKernelGGL(lambda_returns_ends_kernel<4>, dim3((unsigned)((cols / 4 + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), reward, ends, V, Vend, M, gamma, lam, G, A, T, E, N);
    else
        hipLaunchKernelGGL(lambda_returns_ends_kernel<1>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), reward, ends, V, Vend, M, gamma, lam, G, A, T, E, N);
    return dronesim_launched();
}

int dronesim_advantage(const float *G, const float *V, const int32_t *nbr_idx, const uint8_t *done,
                       float gamma, float *w, int T, int E, int N, int K1, void *stream)
{
    if (!G || !V || !nbr_idx || !w || T < 0 || E < 0 || N < 1 || K1 < 1)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_advantage: bad argument");
    if (T == 0 || E == 0) return DRONESIM_OK;
    const size_t cols = (size_t)E * N;
    if (K1 == 3)
        hipLaunchKernelGGL(advantage_kernel<3>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           G, V, nbr_idx, done, gamma, w, T, E, N, K1);
    else
        hipLaunchKernelGGL(advantage_kernel<0>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           G, V, nbr_idx, done, gamma, w, T, E, N, K1);
    return dronesim_launched();
}

int dronesim_neighbour_advantage(const float *G, const float *V, const int32_t *nbr_idx, int per_neighbour, float *adv,
                                 int T, int E, int N, int K1, void *stream)
{
    if (!G || !V || !nbr_idx || !adv || T < 0 || E < 0 || N < 1 || K1 < 1 || per_neighbour < 0 || per_neighbour > 1)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_neighbour_advantage: bad argument");
    if (T == 0 || E == 0) return DRONESIM_OK;
    const size_t rows = (size_t)T * E, items = rows * N;
    const dim3 grid((unsigned)((items + 255) / 256));
    if (K1 == 3)
        hipLaunchKernelGGL(neighbour_advantage_kernel<3>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           G, V, nbr_idx, per_neighbour, adv, rows, N, K1);
    else
        hipLaunchKernelGGL(neighbour_advantage_kernel<0>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           G, V, nbr_idx, per_neighbour, adv, rows, N, K1);
    return dronesim_launched();
}

// developer hook (tests/test_lambda_host.py; not declared in include/dronesim.h): the quadruple rule as the entry points apply it
int dronesim_debug_column_quads(int N, uint64_t cols, uint64_t upper, uint64_t addresses)
{
    return column_quads(N, (size_t)cols, (size_t)upper, (uintptr_t)addresses) ? 1 : 0;
}

}   // extern "C"
