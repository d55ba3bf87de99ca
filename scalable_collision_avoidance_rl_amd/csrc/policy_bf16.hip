// policy_bf16.hip -- the plain-bf16 policy forward (opt-in, dronesim_mlp_forward_bf16): weights and activations in bfloat16,
// float32 accumulation, on
// v_mfma_f32_32x32x16_bf16 (16x the float32 matrix rate).  Formulated transposed -- D[feature][env row] =
// W^T (A operand, pre-packed per fragment on the host, one 16-byte load per lane) x activations (B operand,
// [row][k]) -- so that a lane's accumulator registers are features of ONE env row.
// One workgroup = 64 env rows (2 row tiles sharing every weight fragment) of one agent, 4 waves; wave w owns
// feature chunks w, w+4, ... of every layer.  <= 168 VGPRs and ~48 KiB of LDS at h = 300: three workgroups per CU.
//   layer 1: B = x tile (LDS), relu -> h1 tile in LDS as bf16 [64][h1 pad + 8]
//   layer 2: B = h1 tile (LDS, one ds_read_b128 per lane and fragment, fetched one k-step ahead), A = weight
//            fragments streaming from L2 through a register ring that runs kRing k-steps ahead and across chunk
//            borders (pinned with sched_barrier: the scheduler otherwise sinks every load next to its use).
//            The kernel is occupancy-bound, not bandwidth-bound: at 3 workgroups per CU the MFMA pipe, the LDS
//            and the L2 each sit near 30 %; keeping part of the h1 tile in registers (measured: up to 128 VGPRs)
//            cut LDS traffic but cost the third workgroup and lost 20 %.
//   layer 3: the accumulator layout of a finished layer-2 chunk (lane = env row, registers = features
//            (r&3) + 8 (r>>2) + 4 (lane>>5)) IS a valid B operand if the k order of W3's fragments is permuted
//            to match (done once on the host, see dronesim.h) -- bias + relu + convert in registers, no LDS.
//   the four waves' layer-3 partials are summed through LDS, then activation + sampling, one thread per row.
// LDS row strides are odd multiples of 16 bytes (conflict-free b128 reads).
#include "policy_common.hpp"

namespace {
struct MArgsB {
    int E, N, d_in, h1, h2, nc1, nc2, ks1;
    const float *x, *b1, *b2, *b3;
    const bf16x8 *w1p, *w2p, *w3p;       // [agent][chunk][k-step][64 lanes] fragments
    FinishArgs fin;
    long long *trace;                    // developer trace builds only (NULL otherwise)
};

// relu(acc + bias) of one 32-feature chunk -> bf16 rows [row][feature].  `bias` points at the chunk's 32 biases
// in LDS (zero beyond the layer width; the padded weights are zero there too, so those features come out 0).
__device__ __forceinline__ void store_chunk(const f32x16 (&acc)[kTiles], const float *bias, __bf16 *dst, int ld, int lane)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int fl = 8 * q + 4 * (lane >> 5);            // local feature of register 4q (C/D layout rows)
        const float4 bv = *reinterpret_cast<const float4 *>(bias + fl);
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            bf16x4 p;
            p[0] = (__bf16)fmaxf(acc[t][4 * q + 0] + bv.x, 0.0f);
            p[1] = (__bf16)fmaxf(acc[t][4 * q + 1] + bv.y, 0.0f);
            p[2] = (__bf16)fmaxf(acc[t][4 * q + 2] + bv.z, 0.0f);
            p[3] = (__bf16)fmaxf(acc[t][4 * q + 3] + bv.w, 0.0f);
            *reinterpret_cast<bf16x4 *>(dst + (t * 32 + (lane & 31)) * ld + fl) = p;
        }
    }
}

template <int NC1>                       // 32-feature chunks of the first hidden layer (h1 <= 32 NC1)
__global__ void __launch_bounds__(256, NC1 <= 8 ? 4 : 3) mlp3_bf16_kernel(const float *x, int E, int N, int d_in, const MArgsB rest)
{
    MArgsB a = rest;                     // leading scalars are preloaded into SGPRs at wave launch (csrc/Makefile)
    a.x = x; a.E = E; a.N = N; a.d_in = d_in;
    // occupancy first: h1 <= 256 leaves LDS for four workgroups per CU, which needs <= 128 VGPRs (ring of 4);
    // wider layers fit three (two beyond h1 = 352), where 168 VGPRs allow weight fragments 8 k-steps ahead
    constexpr int kRing = NC1 <= 8 ? 4 : 8;
    constexpr int KS2 = 2 * NC1;                         // k-steps (of 16) of layer 2
    constexpr int L1C = (NC1 + 3) / 4;                   // layer-1 chunks per wave (upper bound)
    constexpr int kMaxChunks = 4;                        // layer-2 chunks per wave: h2 <= 512
    constexpr int ld1 = bf16_h1_stride(NC1);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int agent, row_block;
    xcd_work_item((a.E + kRowsB - 1) / kRowsB, agent, row_block);
    const int e0 = row_block * kRowsB;
    const int nb = (NC1 + a.nc2) * 32;
    __bf16 *sx = reinterpret_cast<__bf16 *>(smem);                 // [64][24]
    float *sbias = reinterpret_cast<float *>(sx + bf16_x_elems());  // b1 | b2 (zero padded to chunks) | b3 (32)
    __bf16 *sh1 = reinterpret_cast<__bf16 *>(sbias + nb + 32);     // [64][ld1]; later f32 partials [4][64][33]
    static_assert(bias_table_floats(0) == 32, "the bias table's b3 tail (a literal here: through bias_table_floats the address arithmetic is re-associated)");
    float *spart = reinterpret_cast<float *>(sh1);
    PT(0);

    // ---- everything that does not depend on LDS is requested up front: x, biases, the sampling counters of
    //      this thread's row, this wave's layer-1 fragments and the head of its layer-2 weight stream
    float xv[4];                                                   // x tile: thread = (row, 4 of 16 k slots)
    {
        const int r = tid >> 2, c0 = (tid & 3) * 4, e = e0 + r;
        const float *xr = a.x + ((size_t)e * a.N + agent) * a.d_in;
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = (e < a.E && c0 + j < a.d_in) ? xr[c0 + j] : 0.0f;   // zero padded to k = 16
    }
    uint32_t tval = 0, epval = 0;
    if (e0 + (tid >> 2) < a.E && a.fin.sample_kind != 0) {          // of the row this thread finishes (4 lanes per row)
        if (a.fin.t_dev) tval = (uint32_t)a.fin.t_dev[e0 + (tid >> 2)];
        if (a.fin.episode_dev) epval = (uint32_t)a.fin.episode_dev[e0 + (tid >> 2)];
    }
    float bv[5];                                                   // (16 + 16) * 32 + 32 <= 5 * 256 bias words
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const int idx = tid + 256 * u;
        float v = 0.0f;
        if (idx < NC1 * 32) { if (idx < a.h1) v = a.b1[(size_t)agent * a.h1 + idx]; }
        else if (idx < nb) { if (idx - NC1 * 32 < a.h2) v = a.b2[(size_t)agent * a.h2 + idx - NC1 * 32]; }
        else if (idx - nb < a.fin.nout) v = a.b3[(size_t)agent * a.fin.nout + idx - nb];
        bv[u] = v;
    }
    bf16x8 w1f[L1C];
#pragma unroll
    for (int i = 0; i < L1C; ++i)
        if (wave + 4 * i < NC1) w1f[i] = a.w1p[((size_t)agent * NC1 + wave + 4 * i) * 64 + lane];
    const bf16x8 *w2a = a.w2p + (size_t)agent * a.nc2 * KS2 * 64 + lane;
    const bf16x8 *w3a = a.w3p + (size_t)agent * a.nc2 * 2 * 64 + lane;
    bf16x8 ring[kRing];
#pragma unroll
    for (int g = 0; g < kRing; ++g) {                              // stream position g = chunk slot * KS2 + k-step
        const int c = wave + 4 * (g / KS2);
        if (g / KS2 < kMaxChunks && c < a.nc2) ring[g] = w2a[((size_t)c * KS2 + g % KS2) * 64];
    }
    __builtin_amdgcn_sched_barrier(0);                             // all requests are out before anything waits
    {
        bf16x4 p;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = (__bf16)xv[j];
        *reinterpret_cast<bf16x4 *>(sx + (tid >> 2) * kLdx + (tid & 3) * 4) = p;
    }
#pragma unroll
    for (int u = 0; u < 5; ++u)
        if (tid + 256 * u < nb + 32) sbias[tid + 256 * u] = bv[u];
    __syncthreads();
    PT(1);

    // ---- layer 1 -> sh1 (bf16): wave w owns feature chunks w, w+4, ...
    {
        const __bf16 *xrow = sx + (lane & 31) * kLdx + 8 * (lane >> 5);
        bf16x8 bx[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) bx[t] = *reinterpret_cast<const bf16x8 *>(xrow + t * 32 * kLdx);
#pragma unroll
        for (int i = 0; i < L1C; ++i) {
            const int c = wave + 4 * i;
            if (c < NC1) {
                f32x16 acc[kTiles] = {};
#pragma unroll
                for (int t = 0; t < kTiles; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[i], bx[t], acc[t], 0, 0, 0);
                store_chunk(acc, sbias + c * 32, sh1 + c * 32, ld1, lane);
            }
        }
    }
    PT(2);
    __syncthreads();
    PT(3);

    // ---- layers 2 + 3 fused over this wave's feature chunks
    const __bf16 *brow = sh1 + (lane & 31) * ld1 + 8 * (lane >> 5);
    f32x16 y[kTiles] = {};
    PT(4);
#pragma unroll
    for (int i = 0; i < kMaxChunks; ++i) {
        const int c = wave + 4 * i;
        if (c < a.nc2) {                                           // wave-uniform
            bf16x8 w3f[2];
            w3f[0] = w3a[(size_t)(2 * c) * 64];
            w3f[1] = w3a[(size_t)(2 * c + 1) * 64];
            f32x16 acc[kTiles] = {};
            bf16x8 bl[2][kTiles];                                   // h1 fragments, fetched one k-step ahead
#pragma unroll
            for (int t = 0; t < kTiles; ++t) bl[0][t] = *reinterpret_cast<const bf16x8 *>(brow + t * 32 * ld1);
#pragma unroll
            for (int s = 0; s < KS2; ++s) {
                const int g = i * KS2 + s;
                if (s + 1 < KS2) {
#pragma unroll
                    for (int t = 0; t < kTiles; ++t)
                        bl[(s + 1) & 1][t] = *reinterpret_cast<const bf16x8 *>(brow + t * 32 * ld1 + (s + 1) * 16);
                }
#pragma unroll
                for (int t = 0; t < kTiles; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[g % kRing], bl[s & 1][t], acc[t], 0, 0, 0);
                const int g2 = g + kRing, i2 = g2 / KS2;           // refill the slot just consumed
                if (i2 < kMaxChunks) {
                    const int c2 = wave + 4 * i2;
                    if (c2 < a.nc2) ring[g % kRing] = w2a[((size_t)c2 * KS2 + g2 % KS2) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);                 // keep the ring kRing steps ahead: the scheduler
            }                                                      // otherwise sinks each load next to its use
            // bias + relu in registers; registers 8 s .. 8 s + 7 of a lane are the k slots of layer-3 k-step s
            const float *bc = sbias + (NC1 + c) * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float4 b0 = *reinterpret_cast<const float4 *>(bc + 16 * s);
                const float4 b1 = *reinterpret_cast<const float4 *>(bc + 16 * s + 8);
#pragma unroll
                for (int t = 0; t < kTiles; ++t) {
                    bf16x8 p;
                    p[0] = (__bf16)fmaxf(acc[t][8 * s + 0] + b0.x, 0.0f);
                    p[1] = (__bf16)fmaxf(acc[t][8 * s + 1] + b0.y, 0.0f);
                    p[2] = (__bf16)fmaxf(acc[t][8 * s + 2] + b0.z, 0.0f);
                    p[3] = (__bf16)fmaxf(acc[t][8 * s + 3] + b0.w, 0.0f);
                    p[4] = (__bf16)fmaxf(acc[t][8 * s + 4] + b1.x, 0.0f);
                    p[5] = (__bf16)fmaxf(acc[t][8 * s + 5] + b1.y, 0.0f);
                    p[6] = (__bf16)fmaxf(acc[t][8 * s + 6] + b1.z, 0.0f);
                    p[7] = (__bf16)fmaxf(acc[t][8 * s + 7] + b1.w, 0.0f);
                    y[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3f[s], p, y[t], 0, 0, 0);
                }
            }
        }
    }
    PT(5);
    __syncthreads();                                               // everyone is done reading sh1
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            spart[((size_t)wave * kRowsB + t * 32 + (lane & 31)) * 33 + cd_row(r, lane)] = y[t][r];
    __syncthreads();
    PT(6);

    {
        const int row = tid >> 2, part = tid & 3;
        const int e = e0 + row;
        if (e >= a.E) return;
        float yv[kQ];
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int j = part + 4 * i;
            float v = 0.0f;
            if (j < a.fin.nout) {
                v = sbias[nb + j];
#pragma unroll
                for (int w = 0; w < 4; ++w) v += spart[((size_t)w * kRowsB + row) * 33 + j];
            }
            yv[i] = v;
        }
        finish_quad(a.fin, yv, e, agent, part, tval, epval);
        PT(7);
    }
}

}   // namespace

extern "C" int dronesim_mlp_forward_bf16(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                                         uint64_t seed, uint64_t counter, int64_t env_base,
                                         const int32_t *t, const int32_t *episode, int E, void *stream)
{
#define K(n) launch_policy<mlp3_bf16_kernel<n>>,
    static const PolicyLaunch<MArgsB> variants[512 / 32] = {K(1) K(2) K(3) K(4) K(5) K(6) K(7) K(8)           // [NC1 - 1]: the h1 tile's register residency
                                                            K(9) K(10) K(11) K(12) K(13) K(14) K(15) K(16)};  // is compile-time (check_mlp: h1 <= 512)
#undef K
    return policy_forward("dronesim_mlp_forward_bf16", "mlp3_bf16_kernel", kFamBf16, variants, m, {x, out, act, act_idx, seed, counter, env_base, t, episode, E, stream},
                          0, 0, m && m->w1p && m->w2p && m->w3p && m->b1 && m->b2 && m->b3, nullptr, [m](MArgsB &a, const PolicyPlan &) {
        a.nc1 = chunks32(m->h1); a.nc2 = chunks32(m->h2); a.ks1 = 1;
        a.b1 = m->b1; a.b2 = m->b2; a.b3 = m->b3;
        a.w1p = reinterpret_cast<const bf16x8 *>(m->w1p); a.w2p = reinterpret_cast<const bf16x8 *>(m->w2p);
        a.w3p = reinterpret_cast<const bf16x8 *>(m->w3p);
    });
}
