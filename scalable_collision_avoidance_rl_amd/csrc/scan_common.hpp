// scan_common.hpp -- what the scans over a stored window [T][E N] share (scans.hip: returns, lambda-returns with and without
// end kinds, advantages; evaluate.hip: the per-episode tables): the column type, the wave's flag fetch, a thread's column
// identity, a pipelined backward driver that a per-scan policy plugs its streams and its fold into (the two lambda scans; the
// returns and evaluation scans keep loops of their own on these types), and the host rule for the 16-byte column quadruples.  One thread per (env, agent) column walks the T axis; consecutive threads touch consecutive
// addresses at every t (coalesced streams), every stream is touched once (non-temporal loads / stores).
#pragma once
#include "common.hpp"

// Time steps per stage: requested together before the sequential recurrence consumes them.
constexpr int kStageT = 8;

// V = 4: a thread owns FOUR adjacent columns (agents of one env: N % 4 == 0) and moves them as 16-byte loads / stores --
// a quarter of the memory instructions for the same bytes in flight (round 5; the un-pipelined round-4 scan lost with
// four columns per thread because a wave then had nothing to overlap its stage wait with).  V = 1: any shape.
template <int V> struct ColVec;
template <> struct ColVec<1> { typedef float type; };
template <> struct ColVec<4> { typedef float type __attribute__((ext_vector_type(4))); };

// flags[t][e] (done, or the kind of end) for the eight time steps t_of(0..7) of a stage, fetched by the WAVE with one load
// instruction instead of eight per thread: lane 8 k + u reads the flag of (step u, k-th env the wave touches), every thread
// then picks its env's flags with a lane permute.  (One 1-byte load per thread and step -- all lanes of a wave on the same
// address -- made the returns scan 2x slower than a copy of the same size: 147 us against 74 without the flags at T = 200 x
// C3.)  Valid when the wave's columns span at most 8 envs (ScanCols::within_stage, wave-uniform); otherwise threads read
// their own flags.
struct DoneStage {
    static_assert(kStageT == 8, "lane 8 k + u: eight steps x eight envs fill the 64 lanes");
    unsigned v;
    template <typename TOf>
    __device__ __forceinline__ void fetch(const uint8_t *done, size_t e_first, int E, int T, TOf t_of)
    {
        const int lane = threadIdx.x & 63, k = lane >> 3, u = lane & 7;
        const int t = t_of(u);
        v = (t >= 0 && t < T && e_first + k < (size_t)E) ? done[(size_t)t * E + e_first + k] : 0u;
    }
    __device__ __forceinline__ bool get(int de, int u) const { return __shfl((int)v, 8 * de + u, 64) != 0; }
    __device__ __forceinline__ unsigned byte(int de, int u) const { return (unsigned)__shfl((int)v, 8 * de + u, 64); }   // (the kind of end)
};

// The columns of one thread that owns V adjacent ones of the E N.  A thread past the end stays and walks the last columns
// with `act` clear -- no early exit: the flag fetch is a wave operation.
template <int V> struct ScanCols {
    size_t EN, col, e, e_first;     // e: the columns' env (V == 4: N % 4 == 0, the four belong to one env); e_first: lane 0's
    int E, de;
    bool act;
    __device__ __forceinline__ ScanCols(int E_, int N) : E(E_)
    {
        EN = (size_t)E * N;
        const size_t col0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
        act = col0 < EN;
        col = act ? col0 : EN - V;
        e = col / N;
        e_first = (size_t)__shfl((long long)e, 0, 64);
        de = (int)(e - e_first);
    }
    // this wave's columns span at most 8 envs: DoneStage serves them
    __device__ __forceinline__ bool within_stage() const { return __builtin_amdgcn_ballot_w64(de >= 8) == 0ull; }
};

// The backward scan, software-pipelined: the rows (and flags) of stage s + 1 are requested BEFORE stage s is folded and
// stored, so that a thread always has kStageT .. 2 kStageT loads per stream in flight and the sequential recurrence runs in
// the shadow of the next stage's HBM round trip.  (Round 4 requested a stage, waited for all of it, folded, stored, and only
// then requested the next: 4 waves per SIMD x 8 loads did not cover the round trip -- 84 us = 0.62 of the roofline against
// 74 us for a copy of the same bytes.)
// A policy P holds a scan's arguments and supplies the rows a stage holds (P::Rows), the running state of a column
// (P::State), the type of a flag (P::Flag) and its source (P::flags, [T][E]), and
//   begin(c, T)              the state before the last step; kBeginFirst: its loads go out in front of the prologue fetch (the
//                            ends scan wants them behind: in front hipcc hoisted them above the COOP branch and waited there)
//   load(rows, u, t, c)      row t into slot u (t may be negative: nothing to load)
//   own(t, c)                the flag of step t read by the thread itself (not COOP: kept in the stage's flag[u])
//   step<COOP>(s, stage, u, t, c)   the fold of step t and its stores; COOP: its flag is stage.ds' pick for (c.de, u)
// all __forceinline__: the driver adds no call, no pointer and no run-time switch to a scan.  It returns the state behind t = 0.
template <typename P> struct ScanStage {
    typename P::Rows rows;
    DoneStage ds;
    typename P::Flag flag[kStageT];
};

template <bool COOP, int V, typename P>
__device__ __forceinline__ void scan_fetch(ScanStage<P> &st, const P &policy, const ScanCols<V> &cols, int T, int t0)
{
    const P p = policy;
    const ScanCols<V> c = cols;
    if (COOP) st.ds.fetch(p.flags, c.e_first, c.E, T, [&](int u) { return t0 - u; });
#pragma unroll
    for (int u = 0; u < kStageT; ++u) {
        const int t = t0 - u;
        p.load(st.rows, u, t, c);
        if (!COOP) st.flag[u] = p.own(t, c);
    }
}

template <bool COOP, int V, typename P>
__device__ __forceinline__ typename P::State scan_backward(const P &policy, const ScanCols<V> &cols, int T)
{
    const P p = policy;                                       // (locals, here and in scan_fetch: hipcc optimises a function BEFORE it
    const ScanCols<V> c = cols;                               // inlines it, and through the references it kept the columns in memory)
    ScanStage<P> cur, nxt;
    typename P::State s;
    if (P::kBeginFirst) s = p.begin(c, T);
    scan_fetch<COOP, V>(cur, p, c, T, T - 1);
    if (!P::kBeginFirst) s = p.begin(c, T);
    for (int t0 = T - 1; t0 >= 0; t0 -= kStageT) {
        if (t0 - kStageT >= 0) scan_fetch<COOP, V>(nxt, p, c, T, t0 - kStageT);
#pragma unroll
        for (int u = 0; u < kStageT; ++u) {
            const int t = t0 - u;
            if (t >= 0) p.template step<COOP>(s, cur, u, t, c);   // (wave-uniform: the flag pick is a wave operation)
        }
        cur = nxt;
    }
    return s;
}

// Host: 16-byte column quadruples (V = 4) when every row of the [.][E N] arrays starts 16-byte aligned (`addresses`: the OR
// of their bases; a NULL one counts as aligned), an env's agents come in fours and the quadruples fill the chip without
// queueing.  Lower bound: below one quadruple wave per SIMD (1024 x 64 x 4 = 262144 columns) half the SIMDs idle -- T = 200 x
// 512 x 256: 38.6 us with one column per thread, 45.6 with four --, at C3's 262144 columns four per thread win (78.1 -> 69.8
// us: 0.75 of the roofline).  Upper bound, the caller's: with one staged stream (returns, evaluation) one column per thread
// is 3 % ahead again from 1048576 columns up (profiles/r5_retbench.log); with two staged streams (the lambda scans) the
// quadruple kernel holds 169 VGPRs = two waves per SIMD, so all quadruple waves are resident at once only below 2 x 1024 x
// 64 x 4 = 524288 columns, and from there on it is one column per thread (66 VGPRs, seven waves per SIMD).
inline bool column_quads(int N, size_t cols, size_t upper, uintptr_t addresses)
{
    return (N % 4) == 0 && (addresses & 15u) == 0 && cols >= 262144 && cols < upper;
}
