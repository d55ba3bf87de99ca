// policy_split.hip -- the split-precision policy forward of rounds 2-5: mlp3_split_kernel with the bf16x3 and f16x2 schemes
// (dronesim_mlp_forward_bf16x3, _f16x2; f16x2's default is mlp3_rt16_kernel in policy_rowtile.hip; overview: policy_common.hpp).
// bf16x3 variant: float32-ACCURATE results on the bf16 matrix instructions.  Every float32 operand is split by
// truncation into three bf16 parts, x = hi + mid + lo EXACTLY (8 + 8 + 8 significant bits), and a product is the sum
// of the six partial products of weight at least 2^-16:  hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid  (the dropped
// ones are below 2^-24 of the product), accumulated in float32, smallest first.  Six v_mfma_f32_32x32x16_bf16 per
// k-step of 16 cost 6/16 of the matrix time of the eight v_mfma_f32_32x32x2_f32 they replace; the result meets the
// reference's own torch modules to the 1e-5 bar like the exact-f32 kernel (tools/split_bf16_emulation.py: a two-part
// split with three products does NOT -- 4-5x over the bar on the Gaussian and critic heads).
// Weights are split and packed per fragment on the host (policies.py) into one consumption-ordered stream per
// (agent, wave) (include/dronesim.h).
// The three layers are fused in REGISTERS, transposed like the bf16 kernel (D[feature][env row]): one workgroup =
// 64 env rows (two 32-row tiles) of one agent, 4 waves; wave w owns the output chunks w, w+4, ... of layer 2 and keeps
// their accumulators for the whole launch while it streams over the first hidden layer chunk by chunk -- each chunk of
// h1 is computed where it is consumed (layer 1 has K = d_in <= 16: one k-step), relu + split happen on the accumulator
// registers (the bias went in as their initial value), whose layout IS a valid B operand once the k order of W2 / W3
// is permuted to match on the host ("accumulator" order, include/dronesim.h).  No activation ever touches LDS; the
// only barriers are around the final sum of the four waves' layer-3 partials.  Non-finite activations are outside the
// split's domain (inf - inf).
// The kernel is software-pipelined by hand inside each wave (mlp3_bf16x3_kernel: `stage`): between the twelve matrix
// instructions of a stage sit the LDS reads of the NEXT stage's fragments, the DMA requests of the stage four ahead and
// one row tile's share of the relu + split that the stages after the next layer-1 step will consume -- a wave never
// waits on L2, LDS or its own vector work with the matrix pipe idle.  Measured on the MI355X (tools/trace_x3.py,
// tools/micro/mfma_dma.hip): the matrix pipe is ~70 % busy at the ACTUAL shader clock, and that clock is what gives:
// 2.07 GHz with the weight stream switched off, 1.6 GHz with it on (power management), against 2.4 GHz nominal --
// ring depth 3 / 4 / 5, spreading the roles over the SIMDs and L1-resident weights all leave the time unchanged.
// TILES row tiles of 32 env rows per wave: every weight fragment loaded feeds all of them.  2 = 64-row workgroups, two per
// CU (256 registers per wave) -- the instantiated one; 4 = 128-row workgroups, one per CU, would halve the weight bytes
// per matrix instruction with the 256 accumulator registers of a wave in the AGPR half of its 512 (see launch below).
#include <type_traits>
#include "policy_common.hpp"

namespace {
template <int N, int I = 0, class F> __device__ __forceinline__ void for_each_slot(F &f)
{
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); for_each_slot<N, I + 1>(f); }
}

struct MArgsX {
    int E, N, d_in, h1, h2, nc1, nc2;
    const float *x, *b1, *b2, *b3;
    const float *wscale;           // f16x2: [N][3] power-of-two factors the packed weights were multiplied by, or NULL
    const char *ws;                // the per-(agent, wave) fragment streams
    int stages;                    // stages per stream (padded)
    FinishArgs fin;
    long long *trace;              // developer trace builds only (NULL otherwise)
};


__device__ __forceinline__ unsigned upper_halves(unsigned odd, unsigned even)      // -> {even.hi16 (low), odd.hi16 (high)}
{
    return __builtin_amdgcn_perm(odd, even, 0x07060302u);
}

// ---- the split schemes (SchemeF16x2: policy_common.hpp).  A scheme names its parts (part 0 = the leading one), the partial products it keeps, in
//      issue order -- smallest first as far as the register hand-over of the weight fragments allows: a fragment part is
//      re-loaded with the NEXT stage's bytes right behind its last product -- and how two float32 values become one
//      dword of every part.
struct SchemeBf16x3 {                                  // v = hi + mid + lo exactly (truncation), products >= 2^-16
    static constexpr int kParts = 3, kProducts = 6;
    static constexpr bool kScaled = false;             // (an exact split: the weights' magnitude does not matter)
    __device__ static constexpr int w_part(int q) { constexpr int t[6] = {2, 1, 0, 1, 0, 0}; return t[q]; }   // lo.hi mid.mid hi.lo
    __device__ static constexpr int b_part(int q) { constexpr int t[6] = {0, 1, 2, 0, 1, 0}; return t[q]; }   // mid.hi hi.mid hi.hi
    __device__ static constexpr int last_use(int p) { constexpr int t[3] = {5, 3, 0}; return t[p]; }
    __device__ static constexpr int request_slot(int p) { constexpr int t[3] = {3, 6, 9}; return t[p]; }
    __device__ static __forceinline__ f32x16 mfma(const u32x4 &w, const u32x4 &b, const f32x16 &acc)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
    // the upper 16 bits of a float32 ARE a bf16: 5 vector instructions per value with the relu, 3 per pair to pack
    template <bool RELU> __device__ static __forceinline__ void split_pair(float v0, float v1, unsigned (&d)[3])
    {
        if (RELU) { v0 = fmaxf(v0, 0.0f); v1 = fmaxf(v1, 0.0f); }
        const unsigned h0 = __float_as_uint(v0), h1 = __float_as_uint(v1);
        const float r0 = v0 - __uint_as_float(h0 & 0xffff0000u), r1 = v1 - __uint_as_float(h1 & 0xffff0000u);
        const unsigned m0 = __float_as_uint(r0), m1 = __float_as_uint(r1);
        const float l0 = r0 - __uint_as_float(m0 & 0xffff0000u), l1 = r1 - __uint_as_float(m1 & 0xffff0000u);
        d[0] = upper_halves(h1, h0); d[1] = upper_halves(m1, m0); d[2] = upper_halves(__float_as_uint(l1), __float_as_uint(l0));
    }
};

struct NoJob { template <int SLOT> __device__ __forceinline__ void slot() {} };
#define SplitJobInStage SplitJob

template <int P> __device__ __forceinline__ Parts<P> parts_from_lds(const char *p)      // parts 1 KiB apart
{
    Parts<P> r;
    if constexpr (P == 3)
        asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:1024\n\tds_read_b128 %2, %3 offset:2048\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r.p[0]), "=&v"(r.p[1]), "=&v"(r.p[2]) : "v"(lds_addr(p)) : "memory");
    else
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r.p[0]), "=&v"(r.p[1]) : "v"(lds_addr(p)) : "memory");
    return r;
}

#define X3_PIN() __builtin_amdgcn_sched_barrier(0)
#define X3_RING_READ(dst, p) dst = *reinterpret_cast<const u32x4 *>(p)

template <class S, int TILES>
__global__ void __launch_bounds__(256, TILES <= 2 ? 2 : 1) mlp3_split_kernel(const float *x, int E, int N, int d_in, const MArgsX rest)
{
    constexpr int P = S::kParts, kStageBytes = P * 1024;
    constexpr int kTilesX = TILES, kRowsX = 32 * TILES, kRingX = split_ring_depth(TILES);
    MArgsX a = rest;
    a.x = x; a.E = E; a.N = N; a.d_in = d_in;
    constexpr int kMaxChunks = 4;                        // layer-2 chunks per wave: h2 <= 512
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int agent, row_block;
    xcd_work_item((a.E + kRowsX - 1) / kRowsX, agent, row_block);
    const int e0 = row_block * kRowsX;
    const int NC1 = a.nc1;
    const int nb = (a.nc1 + a.nc2) * 32;
    // S::kScaled: the power-of-two factors of this agent's packed layers and their (exact) inverses
    float ws1 = 1.0f, ws2 = 1.0f, wi1 = 1.0f, wi2 = 1.0f, wi3 = 1.0f;
    if (S::kScaled && a.wscale != nullptr) {
        const float *wsp = a.wscale + 3 * (size_t)agent;
        const float ws3 = wsp[2];
        ws1 = wsp[0]; ws2 = wsp[1];
        // 1 / factor by v_rcp_f32: EXACT for the powers of two include/dronesim.h asks for (a device-side pointer cannot be checked by
        // the host entry point; exponent arithmetic on the bit pattern, as in round 5, was only right for normal powers of two)
        wi1 = __builtin_amdgcn_rcpf(ws1);
        wi2 = __builtin_amdgcn_rcpf(ws2);
        wi3 = __builtin_amdgcn_rcpf(ws3);
    }
    if (kTrace && a.trace && lane == 0) {                          // shader clock and the 100 MHz clock at entry
        a.trace[((size_t)blockIdx.x * 4 + wave) * 8 + 0] = __builtin_amdgcn_s_memtime();
        a.trace[((size_t)blockIdx.x * 4 + wave) * 8 + 1] = __builtin_amdgcn_s_memrealtime();
    }
    float *sbias = reinterpret_cast<float *>(smem);                // b1 | b2 (zero padded to chunks) | b3 (32)
    char *sxb = reinterpret_cast<char *>(sbias + bias_table_floats(nb));   // x operand [tile][part][lane] x 16 B
    float *spart = reinterpret_cast<float *>(sxb + split_x_bytes(kTilesX, P));   // [4 waves][kRowsX rows][33], shares LDS with the rings

    // ---- the x operand: row 32 t + (lane & 31), inputs 8 (lane >> 5) .. + 7, split once, kept in LDS (every wave uses it)
    if (wave < kTilesX) {
        const int t = wave;
        const int e = e0 + 32 * t + (lane & 31), k0 = 8 * (lane >> 5);
        const float *xr = a.x + ((size_t)min(e, a.E - 1) * a.N + agent) * a.d_in;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // clamped address, value masked with an AND: written as `cond ? xv : 0` hipcc turns the select into a branch
            // around the load and waits for each of the eight loads in turn (eight round trips in series at the head of
            // every workgroup; found in the ISA in round 4)
            const float xv = xr[min(k0 + j, a.d_in - 1)];
            v[j] = __uint_as_float(__float_as_uint(xv) & ((e < a.E && k0 + j < a.d_in) ? 0xffffffffu : 0u));
        }
        Parts<P> xp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned d[P];
            S::template split_pair<false>(v[2 * q], v[2 * q + 1], d);              // (no relu on the inputs)
#pragma unroll
            for (int p = 0; p < P; ++p) xp.p[p][q] = d[p];
        }
        u32x4 *dp = reinterpret_cast<u32x4 *>(sxb + t * kStageBytes) + lane;
#pragma unroll
        for (int p = 0; p < P; ++p) dp[64 * p] = xp.p[p];
    }
    uint32_t tval[kRowsX / 64], epval[kRowsX / 64];                // step / episode counters of the rows this thread finishes
#pragma unroll
    for (int r = 0; r < kRowsX / 64; ++r) {                        // (the sampling stream's position; 4 lanes per row)
        const int e = e0 + 64 * r + (tid >> 2);
        tval[r] = epval[r] = 0;
        if (e < a.E && a.fin.sample_kind != 0) {
            if (a.fin.t_dev) tval[r] = (uint32_t)a.fin.t_dev[e];
            if (a.fin.episode_dev) epval[r] = (uint32_t)a.fin.episode_dev[e];
        }
    }
    {                                                              // biases -> LDS, zero padded: nb + 32 <= 1056 floats.  All
        constexpr int kIt = 5;                                     // loads first, none behind a branch (same reason as above)
        float bv[kIt];
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int idx = tid + 256 * it, j2 = idx - a.nc1 * 32, j3 = idx - nb;
            const bool in1 = idx < a.nc1 * 32, in2 = idx < nb;
            const float *p = in1 ? a.b1 + (size_t)agent * a.h1 + min(idx, a.h1 - 1)
                           : in2 ? a.b2 + (size_t)agent * a.h2 + min(j2, a.h2 - 1)
                                 : a.b3 + (size_t)agent * a.fin.nout + min(max(j3, 0), a.fin.nout - 1);
            const bool ok = in1 ? idx < a.h1 : in2 ? j2 < a.h2 : j3 < a.fin.nout;
            bv[it] = __uint_as_float(__float_as_uint(*p) & (ok ? 0xffffffffu : 0u));
            if (S::kScaled) bv[it] *= in1 ? ws1 : in2 ? ws2 : 1.0f;    // b1, b2 start accumulators of SCALED products; b3 is added at the end
        }
#pragma unroll
        for (int it = 0; it < kIt; ++it)
            if (tid + 256 * it < nb + 32) sbias[tid + 256 * it] = bv[it];
    }
    __syncthreads();

    const int nmine = (a.nc2 - wave + 3) / 4;                      // output chunks of this wave (wave-uniform): wave + 4 i
    f32x16 acc2[kMaxChunks][kTilesX];
#pragma unroll
    for (int i = 0; i < kMaxChunks; ++i) {                         // start from the layer-2 biases (zero padded)
        const f32x16 b = bias_tile(sbias + (a.nc1 + min(wave + 4 * i, a.nc2 - 1)) * 32, lane);
#pragma unroll
        for (int t = 0; t < kTilesX; ++t) acc2[i][t] = b;
    }
    f32x16 y[kTilesX];
#pragma unroll
    for (int t = 0; t < kTilesX; ++t) y[t] = f32x16{};

    // ---- The weight fragments of this wave form ONE linear stream of stages (the P parts of one 32-feature chunk x
    //      16 k slots, 1 KiB each), laid out by the host in the order the matrix instructions want them
    //      (include/dronesim.h):
    //          W1(0), W2(0,0,*) | W1(1), W2(0,1,*), W2(1,0,*) | W1(2), W2(1,1,*), W2(2,0,*) | ... | W3(*)
    //      (W2(c1, ss, i): k-step 2 c1 + ss of this wave's i-th output chunk).  They travel global -> LDS by DMA
    //      (global_load_lds, 1 KiB per instruction) into a ring PRIVATE to the wave, requested kRingX stages before
    //      their matrix instructions and picked up part by part during the PREVIOUS stage's matrix instructions, into
    //      the registers that stage has just finished with: no copies, no exposed LDS or L2 latency.  The ring needs no
    //      barrier (one wave writes and reads it); a read is ordered behind its DMA by the counted s_waitcnt vmcnt.
    //      The stream is padded by kRingX stages, so the producer never needs to know where it ends.
    char *ring = reinterpret_cast<char *>(spart) + (size_t)wave * split_ring_bytes(kTilesX, P);
    const char *gp = a.ws + (((size_t)agent * 4 + wave) * a.stages * P * 64 + lane) * 16;
    int pslot = 0;
    auto request_part = [&](int p) {                               // 1 KiB of the stage kRingX ahead
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gp + p * 1024),
                                         (__attribute__((address_space(3))) void *)(ring + pslot * kStageBytes + p * 1024), 16, 0, 0);
    };
    auto request_done = [&]() {
        gp += kStageBytes;
        pslot = pslot + 1 == kRingX ? 0 : pslot + 1;
    };
    u32x4 wf[P];                                                   // the current stage's fragments, part 0 first
    int nslot = 1;                                                 // ring slot of the NEXT stage
    // one stage: acc[t] += W * B[t], the scheme's products on both tiles; slot s = the gap behind matrix instruction s:
    // `job` is offered every slot, the ring reads and the DMA requests sit where the scheme puts them
    auto stage = [&](f32x16 (&acc)[kTilesX], const Parts<P> (&b)[kTilesX], auto &job) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(P * (kRingX - 2)) : "memory");    // the NEXT stage has landed
        const char *np = ring + nslot * kStageBytes + lane * 16;
        X3_PIN();
        auto slot_work = [&](auto SLOT) {
            constexpr int s = decltype(SLOT)::value, q = s / TILES, t = s % TILES;
            acc[t] = S::mfma(wf[S::w_part(q)], b[t].p[S::b_part(q)], acc[t]);
            X3_PIN();
            if constexpr (t == TILES - 1) {
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (S::last_use(p) == q) X3_RING_READ(wf[p], np + p * 1024);
            }
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (S::request_slot(p) * TILES / 2 == s) { request_part(p); if (p == P - 1) request_done(); }
            job.template slot<s>();
            X3_PIN();
        };
        for_each_slot<S::kProducts * TILES>(slot_work);
        nslot = nslot + 1 == kRingX ? 0 : nslot + 1;
        X3_PIN();
    };

    if (nmine > 0) {
#pragma unroll 1
        for (int j = 0; j < kRingX; ++j) {
#pragma unroll
            for (int p = 0; p < P; ++p) request_part(p);
            request_done();
        }
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(P * (kRingX - 1)) : "memory");
#pragma unroll
        for (int p = 0; p < P; ++p) wf[p] = *reinterpret_cast<const u32x4 *>(ring + p * 1024 + lane * 16);

        NoJob nojob;
        f32x16 a1[kTilesX];
        Parts<P> hB0[kTilesX], hB1[kTilesX];                       // layer-2 operands of k-steps 2 c1 and 2 c1 + 1
        {                                                          // layer 1, chunk 0
            Parts<P> xB[kTilesX];
#pragma unroll
            for (int t = 0; t < kTilesX; ++t) { a1[t] = bias_tile(sbias, lane); xB[t] = parts_from_lds<P>(sxb + t * kStageBytes + lane * 16); }
            stage(a1, xB, nojob);
#pragma unroll
            for (int t = 0; t < kTilesX; ++t) { SplitJob<S, 0, TILES> j(a1[t], hB0[t], wi1); j.all(); }
        }
        for (int c1 = 0; c1 < NC1; ++c1) {
            // k-step 2 c1 of every chunk of mine; meanwhile the other half of a1 becomes hB1 (tile i in stage i)
#pragma unroll
            for (int i = 0; i < kMaxChunks; ++i) {
                if (i < nmine) {                                   // wave-uniform
                    if (i < kTilesX) { SplitJobInStage<S, 1, TILES> j(a1[i], hB1[i], wi1); stage(acc2[i], hB0, j); }
                    else stage(acc2[i], hB0, nojob);
                }
            }
#pragma unroll
            for (int t = 0; t < kTilesX; ++t)                     // tiles no stage of mine has dealt with (fewer chunks than tiles)
                if (t >= nmine) { SplitJob<S, 1, TILES> j(a1[t], hB1[t], wi1); j.all(); }
            if (c1 + 1 < NC1) {                                    // layer 1 of the next chunk
                Parts<P> xB[kTilesX];
                a1[0] = bias_tile(sbias + (c1 + 1) * 32, lane);
#pragma unroll
                for (int t = 0; t < kTilesX; ++t) { a1[t] = a1[0]; xB[t] = parts_from_lds<P>(sxb + t * kStageBytes + lane * 16); }
                stage(a1, xB, nojob);
            }
            // k-step 2 c1 + 1; meanwhile the first half of the next chunk becomes hB0 (stale and unused after the last chunk)
#pragma unroll
            for (int i = 0; i < kMaxChunks; ++i) {
                if (i < nmine) {
                    if (i < kTilesX) { SplitJobInStage<S, 0, TILES> j(a1[i], hB0[i], wi1); stage(acc2[i], hB1, j); }
                    else stage(acc2[i], hB1, nojob);
                }
            }
#pragma unroll
            for (int t = 0; t < kTilesX; ++t)
                if (t >= nmine) { SplitJob<S, 0, TILES> j(a1[t], hB0[t], wi1); j.all(); }
        }

        // ---- layer 3 from the finished layer-2 accumulators, same stream
#pragma unroll
        for (int i = 0; i < kMaxChunks; ++i) {
            if (i < nmine) {
                Parts<P> pB[kTilesX];
#pragma unroll
                for (int t = 0; t < kTilesX; ++t) { SplitJob<S, 0, TILES> j(acc2[i][t], pB[t], wi2); j.all(); }
                stage(y, pB, nojob);
#pragma unroll
                for (int t = 0; t < kTilesX; ++t) { SplitJob<S, 1, TILES> j(acc2[i][t], pB[t], wi2); j.all(); }
                stage(y, pB, nojob);
            }
        }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the partial sums reuse the rings: no DMA may land late
    if (kTrace && a.trace && lane == 0) {                          // ... and when this wave's stream is done
        a.trace[((size_t)blockIdx.x * 4 + wave) * 8 + 2] = __builtin_amdgcn_s_memtime();
        a.trace[((size_t)blockIdx.x * 4 + wave) * 8 + 3] = __builtin_amdgcn_s_memrealtime();
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTilesX; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            spart[((size_t)wave * kRowsX + t * 32 + (lane & 31)) * 33 + cd_row(r, lane)] = y[t][r];
    __syncthreads();

#pragma unroll
    for (int r = 0; r < kRowsX / 64; ++r) {                        // activation + sampling: four lanes per env row
        const int row = 64 * r + (tid >> 2), part = tid & 3;
        const int e = e0 + row;
        if (e >= a.E) return;
        float yv[kQ];
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int j = part + 4 * i;
            float v = 0.0f;
            if (j < a.fin.nout) {
                if (S::kScaled) {                                  // the waves' partials carry layer 3's weight factor
                    float pv = 0.0f;
#pragma unroll
                    for (int w = 0; w < 4; ++w) pv += spart[((size_t)w * kRowsX + row) * 33 + j];
                    v = fmaf(pv, wi3, sbias[nb + j]);
                } else {
                    v = sbias[nb + j];
#pragma unroll
                    for (int w = 0; w < 4; ++w) v += spart[((size_t)w * kRowsX + row) * 33 + j];
                }
            }
            yv[i] = v;
        }
        finish_quad(a.fin, yv, e, agent, part, tval[r], epval[r]);
    }
}
#undef X3_PIN
#undef X3_RING_READ

static_assert(SchemeBf16x3::kParts == split_parts(0) && SchemeF16x2::kParts == split_parts(1) && !SchemeBf16x3::kScaled && SchemeF16x2::kScaled,
              "the plan sizes a scheme's stages, and the entry point hands wscale on, by the scheme's number");

// `scheme`: 0 bf16x3, 1 f16x2 (the plan's `layout`, and the variant it picks)
int mlp_forward_split(int scheme, const DroneMlpBf16 *m, const PolicyCall &c)
{
    // TILES = 4 (128-row workgroups, one per CU, accumulators in the AGPR half of a 512-register wave) builds and is
    // correct, but hipcc 7.2 places the accumulators badly (1100 v_accvgpr copies, scratch spills whose waits drain the
    // DMA ring): 561 vs 301 us at C3 Gaussian f16x2.  Not instantiated; it needs hand-placed AGPR accumulators.
    static const PolicyLaunch<MArgsX> variants[2] = {launch_policy<mlp3_split_kernel<SchemeBf16x3, 2>>, launch_policy<mlp3_split_kernel<SchemeF16x2, 2>>};
    return policy_forward(scheme ? "dronesim_mlp_forward_f16x2" : "dronesim_mlp_forward_bf16x3", "mlp3_split_kernel", kFamSplit, variants, m, c, scheme,
                          m ? m->reserved : 0, m && m->w1p && m->b1 && m->b2 && m->b3, nullptr, [m, scheme](MArgsX &a, const PolicyPlan &p) {
        a.nc1 = chunks32(m->h1); a.nc2 = chunks32(m->h2);
        a.stages = p.stream;
        a.b1 = m->b1; a.b2 = m->b2; a.b3 = m->b3;
        a.wscale = scheme ? m->wscale : nullptr;                   // SchemeF16x2::kScaled
        a.ws = reinterpret_cast<const char *>(m->w1p);
    });
}

}   // namespace

extern "C" int dronesim_mlp_bf16x3_stages(int h1, int h2) { return split_stages(chunks32(h1), chunks32(h2)); }

extern "C" int dronesim_mlp_forward_bf16x3(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                                           uint64_t seed, uint64_t counter, int64_t env_base,
                                           const int32_t *t, const int32_t *episode, int E, void *stream)
{
    return mlp_forward_split(0, m, {x, out, act, act_idx, seed, counter, env_base, t, episode, E, stream});
}

extern "C" int dronesim_mlp_forward_f16x2(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                                          uint64_t seed, uint64_t counter, int64_t env_base,
                                          const int32_t *t, const int32_t *episode, int E, void *stream)
{
    return mlp_forward_split(1, m, {x, out, act, act_idx, seed, counter, env_base, t, episode, E, stream});
}
