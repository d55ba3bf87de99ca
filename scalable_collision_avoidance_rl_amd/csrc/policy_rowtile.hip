// policy_rowtile.hip -- the ROW-TILE policy forward of round 6, the default of the host class: mlp3_rt_kernel (exact float32,
// dronesim_mlp_forward with DroneMlp.w2_layout = 2) and, further down, mlp3_rt16_kernel (f16x2, dronesim_mlp_forward_f16x2_rt).
// The two share the ownership (kRtChunks, rt_passes, rt_per_pass) and dma_to_lds; which kernel serves which shape, the LDS layouts and the launch plan: policy_common.hpp.
// mlp3_rt_kernel, exact float32: the register-fused formulation of the split kernels on
// v_mfma_f32_32x32x2_f32, with the work split the other way round.  A wave owns 32 env rows of one agent and ALL output chunks
// of layer 2 for them (up to kRtChunks = 7 accumulator tiles = 112 registers per pass; h2 > 224 takes two passes and recomputes
// layer 1 in the second: 52 of 2900 matrix instructions at h = 400), so
//   * nothing is computed twice across waves and every wave issues the same number of matrix instructions (whole chunks dealt
//     to waves leave 13 / 10 / 7 chunks at 4-3-3-3 / 3-3-2-2 / 2-2-2-1: 0.70 / 0.70 / 0.62 of the matrix peak at best);
//   * layers 1 -> 2 -> 3 meet in REGISTERS: D^T[feature][row] of v_mfma_f32_32x32x2_f32 puts feature 8 (r >> 2) + 4 (lane >> 5)
//     + (r & 3) of row (lane & 31) into register r, and register r of the two lane halves IS the B operand of k-step r of the
//     next layer once the weights' k order is permuted to match on the host (policies.py: pack_f32_rowtile_stream) -- no
//     activation touches LDS, no barrier after the prologue, layer 3 is complete inside the wave;
//   * the vector ALU -- which the float32 matrix instructions run on -- sees 16 v_max per 32-feature chunk and nothing else in the
//     loop: weights travel global -> LDS by DMA into a ring PRIVATE to the wave (4 blocks of 4 KiB = the sixteen A operands of
//     one (in-chunk, out-chunk) pair, four blocks ahead) and LDS -> registers as one ds_read_b128 per four matrix instructions.
// Matrix instructions per wave and 32 rows: 840 / 1740 / 2912 at h = 200 / 300 / 400 = 0.77 / 0.87 / 0.88 of the peak if none stalls.
// One agent's stream, in consumption order (blocks of 4 pieces of 1 KiB = [64 lanes][4 floats]):
//   per pass p (output chunks S_p):  for c1: L1(c1), L2(c1, c2) for c2 in S_p;  then L3(c2) for c2 in S_p;  kRtPad zero blocks.
//   L1(c1): piece 0 = W1[2 r + half][32 c1 + i], r = 0..3; piece 1 = the same for r = 4..6, then b1[32 c1 + i] (lanes < 32);
//   L2(c1, c2): piece q = W2[32 c1 + 8 q + 4 half + j][32 c2 + i], j = 0..3;   L3(c2): piece q = W3[32 c2 + 8 q + 4 half + j][i]
//   (lane = 32 half + i; zero beyond d_in / h1 / h2 / nout).
#include <type_traits>
#include "policy_common.hpp"

namespace {
struct MArgsR {
    int E, N, d_in, h1, h2, nout, nc1, nc2, blocks;
    const float *x, *ws, *b2, *b3;
    const float *w3;                     // VL3: the plain [N][h2][nout] output layer (nout <= 4)
    FinishArgs fin;
    unsigned rb_magic;
};

#define RT_PIN() __builtin_amdgcn_sched_barrier(0)

// VL3 (nout <= 4: the Gaussian actor's 4 moments, the critic's value): layer 3 on the VECTOR ALU from the same registers -- a lane
// multiplies its 16 features of a chunk with their nout weights (LDS table, one ds_read_b128 per feature) and the two lane halves'
// partial sums meet through one permute per output: 64 fused multiply-adds per chunk instead of 16 matrix instructions of 64 cycles
// whose 32 output rows hold nout <= 4 values (7 % of the kernel's matrix time at h = 400, 13 % at h = 200).  The stream then holds
// no L3 blocks.
template <bool VL3>
__global__ void __launch_bounds__(256, 2) mlp3_rt_kernel(const float *x, int E, int N, int d_in, const MArgsR rest)
{
    MArgsR a = rest;
    a.x = x; a.E = E; a.N = N; a.d_in = d_in;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int agent, row_block;
    xcd_work_item((a.E + kRtRows - 1) / kRtRows, agent, row_block, a.rb_magic);
    const int e0 = row_block * kRtRows + 32 * wave;                // this wave's 32 env rows
    const int half = lane >> 5;
    const int nc1 = a.nc1, nc2 = a.nc2, ks1 = (a.d_in + 1) >> 1;
    float *sb2 = reinterpret_cast<float *>(smem);                  // b2, zero padded to whole chunks
    f32x4 *sw3 = reinterpret_cast<f32x4 *>(smem + rt_b2_bytes(nc2));   // VL3: W3[f][0..3] (zero beyond h2 / nout)
    char *ring = smem + rt_tables_bytes(nc2, VL3) + wave * rt_ring_bytes();

    // ---- the weight stream.  Everything about it is scalar except the lane's 16-byte slot: the float32 matrix instructions run
    // on the vector ALUs, so every vector instruction in the loop is matrix time lost -- the DMA requests are issued by name with a
    // scalar base and a constant 32-bit lane offset (hipcc forms 64-bit per-lane addresses with two v_lshl_add_u64 per request), and
    // the ring reads by name with counted waits (hipcc waits for ALL outstanding LDS reads in front of a block's first instruction).
    const unsigned long long sbase0 = reinterpret_cast<unsigned long long>(a.ws) + (unsigned long long)agent * a.blocks * 4096ull;
    const unsigned voff = (unsigned)lane * 16u;                    // this lane's slot of a 1-KiB piece (global and LDS alike)
    const unsigned ring_a = lds_addr(ring);
    const unsigned rd_a = ring_a + voff;                           // LDS address of this lane's slot in ring block 0, piece 0
    int cur = 0;                                                   // block being consumed; its ring slot = cur & 3
    auto dma = [&](int blk, int q) {                               // piece q of stream block blk -> its ring slot
        const unsigned long long src = sbase0 + (unsigned long long)(unsigned)blk * 4096ull + (unsigned)q * 1024u;
        const unsigned dst = ring_a + (unsigned)(blk & (kRtRing - 1)) * 4096u + (unsigned)q * 1024u;
        dma_to_lds(dst, voff, src);
    };
    f32x4 w[4];                                                    // the current block's sixteen A operands
    // the ring is primed FIRST, ahead of the prologue's own loads: the first four blocks travel while b2 / x / W3 are fetched and
    // the workgroup meets at its barrier (one global round trip less at the head of every wave: 5-10 % of a wave's life at h = 200)
    if (e0 < a.E) {
#pragma unroll 1
        for (int b = 0; b < kRtRing; ++b) {
#pragma unroll
            for (int q = 0; q < 4; ++q) dma(b, q);
        }
    }
    for (int i = tid; i < nc2 * 32; i += 256) {                    // (clamped address, masked value: no branch around the load)
        const float v = a.b2[(size_t)agent * a.h2 + min(i, a.h2 - 1)];
        sb2[i] = __uint_as_float(__float_as_uint(v) & (i < a.h2 ? 0xffffffffu : 0u));
        if (VL3) {
            f32x4 wv;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const float t = a.w3[((size_t)agent * a.h2 + min(i, a.h2 - 1)) * a.nout + min(o, a.nout - 1)];
                wv[o] = __uint_as_float(__float_as_uint(t) & ((i < a.h2 && o < a.nout) ? 0xffffffffu : 0u));
            }
            sw3[i] = wv;
        }
    }
    // the x operand of layer 1: k-step r = inputs 2 r + half of row (lane & 31)
    float xb[7];
    {
        const int e = min(e0 + (lane & 31), a.E - 1);
        const float *xr = a.x + ((size_t)e * a.N + agent) * a.d_in;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const int k = 2 * r + half;
            const float v = xr[min(k, a.d_in - 1)];
            xb[r] = __uint_as_float(__float_as_uint(v) & (k < a.d_in ? 0xffffffffu : 0u));
        }
    }
    // the output stage's inputs: four lanes per env row, two rounds of 16 rows
    uint32_t tval[2] = {0u, 0u}, epval[2] = {0u, 0u};
    float b3v[2][kQ];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int e = e0 + 16 * it + (lane >> 2);
        if (e < a.E && a.fin.sample_kind != 0) {
            if (a.fin.t_dev) tval[it] = (uint32_t)a.fin.t_dev[e];
            if (a.fin.episode_dev) epval[it] = (uint32_t)a.fin.episode_dev[e];
        }
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int j = (lane & 3) + 4 * i;
            const float v = a.b3[(size_t)agent * a.nout + min(j, a.nout - 1)];
            b3v[it][i] = j < a.nout ? v : 0.0f;
        }
    }
    __syncthreads();                                               // b2 is in LDS; the only barrier of the kernel
    if (e0 >= a.E) return;                                         // a wave without rows (ragged last workgroup)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // every load above AND the ring's first four blocks have landed:
                                                                   // from here vmcnt counts the DMA pieces requested in the loop only

    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\t"
                 "ds_read_b128 %3, %4 offset:3072" : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]) : "v"(rd_a) : "memory");
    // one group = the four matrix instructions of piece q (`mf`) -- the piece was requested from LDS a block ago: at most three
    // younger reads may still be out -- then the piece's ring slot is refilled with block cur + 4, and piece q of block cur + 1
    // (landed: twelve DMA requests were issued behind it) takes its place in the registers
    auto group = [&](auto Q, auto &&mf) {
        constexpr int q = decltype(Q)::value;
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(w[q]) :: "memory");
        mf(w[q]);
        RT_PIN();
        dma(cur + kRtRing, q);
        const unsigned ra = rd_a + (unsigned)((cur + 1) & (kRtRing - 1)) * 4096u;
        asm volatile("s_waitcnt vmcnt(12)\n\tds_read_b128 %0, %1 offset:%2" : "=v"(w[q]) : "v"(ra), "n"(q * 1024) : "memory");
        RT_PIN();
    };
    typedef std::integral_constant<int, 0> Q0; typedef std::integral_constant<int, 1> Q1;
    typedef std::integral_constant<int, 2> Q2; typedef std::integral_constant<int, 3> Q3;
    auto nothing = [](const f32x4 &) {};

    f32x16 y = {0}, y1 = {0};
    const float one = lane < 32 ? 1.0f : 0.0f;
    const int passes = rt_passes(nc2), per = rt_per_pass(nc2);
    for (int p = 0; p < passes; ++p) {
        const int c2_0 = p * per, npc = min(per, nc2 - c2_0);      // this pass's output chunks (wave-uniform)
        f32x16 acc2[kRtChunks];
#pragma unroll
        for (int i = 0; i < kRtChunks; ++i) acc2[i] = bias_tile(sb2 + min(c2_0 + i, nc2 - 1) * 32, lane);
        for (int c1 = 0; c1 < nc1; ++c1) {
            // layer 1 of chunk c1: K = d_in <= 14, then the bias on one more matrix instruction (A = b1 in lanes 0..31, B = 1 there)
            f32x16 a1 = {0};
            group(Q0{}, [&](const f32x4 &v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < ks1) a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], xb[j], a1, 0, 0, 0);
            });
            group(Q1{}, [&](const f32x4 &v) {
#pragma unroll
                for (int j = 0; j < 3; ++j) if (4 + j < ks1) a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], xb[4 + j], a1, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[3], one, a1, 0, 0, 0);
            });
            group(Q2{}, nothing);
            group(Q3{}, nothing);
            ++cur;
#pragma unroll
            for (int r = 0; r < 16; ++r) a1[r] = fmaxf(a1[r], 0.0f);
            // layer 2: every output chunk of the pass takes this chunk's 32 features -- 16 k-steps, B = register r of a1.  Group q holds
            // the features 8 q .. 8 q + 7 of the chunk: the groups of a ragged last chunk that hold none are skipped (h = 400 / 300 /
            // 200 end in chunks of 16 / 12 / 8 features: 8 / 8 / 12 of the 16 instructions of each of that chunk's blocks)
            const int kv = a.h1 - 32 * c1;                     // features of this in-chunk (wave-uniform)
#pragma unroll
            for (int i = 0; i < kRtChunks; ++i) {
                if (i < npc) {
                    group(Q0{}, [&](const f32x4 &v) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], a1[j], acc2[i], 0, 0, 0);
                    });
                    group(Q1{}, [&](const f32x4 &v) {
                        if (kv > 8) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], a1[4 + j], acc2[i], 0, 0, 0);
                        }
                    });
                    group(Q2{}, [&](const f32x4 &v) {
                        if (kv > 16) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], a1[8 + j], acc2[i], 0, 0, 0);
                        }
                    });
                    group(Q3{}, [&](const f32x4 &v) {
                        if (kv > 24) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], a1[12 + j], acc2[i], 0, 0, 0);
                        }
                    });
                    ++cur;
                }
            }
        }
        // layer 3 from the finished chunks of this pass: two accumulation chains (even / odd chunks) that are added at the end --
        // half the roundings in a row on the outputs' own scale (every instruction rounds once; the 16-column instruction of the
        // LDS-staged kernel takes four products per rounding, this one two)
        auto layer3 = [&](f32x16 &yy, f32x16 &h, int kv3, int c2) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) h[r] = fmaxf(h[r], 0.0f);
            if constexpr (VL3) {                             // registers 0..3 of yy = this lane's partial sums of the nout <= 4 outputs
                const f32x4 *wp = sw3 + 32 * c2 + 4 * half;  // this lane's features: 8 q + 4 half + j
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 wv = wp[8 * q + j];
#pragma unroll
                        for (int o = 0; o < 4; ++o) yy[o] = fmaf(wv[o], h[4 * q + j], yy[o]);
                    }
                }
                return;
            }
            group(Q0{}, [&](const f32x4 &v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) yy = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], h[j], yy, 0, 0, 0);
            });
            group(Q1{}, [&](const f32x4 &v) {
                if (kv3 > 8) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) yy = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], h[4 + j], yy, 0, 0, 0);
                }
            });
            group(Q2{}, [&](const f32x4 &v) {
                if (kv3 > 16) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) yy = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], h[8 + j], yy, 0, 0, 0);
                }
            });
            group(Q3{}, [&](const f32x4 &v) {
                if (kv3 > 24) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) yy = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], h[12 + j], yy, 0, 0, 0);
                }
            });
            ++cur;
        };
#pragma unroll
        for (int i = 0; i < kRtChunks; ++i) {
            if (i < npc) {
                const int kv3 = a.h2 - 32 * (c2_0 + i);      // features of this chunk (the same skipping as in layer 2)
                if (i & 1) layer3(y1, acc2[i], kv3, c2_0 + i); else layer3(y, acc2[i], kv3, c2_0 + i);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the output tile reuses the ring: no DMA may land late

    // ---- output activation + sampling: the wave's 32 x nout tile through its own LDS region, four lanes per env row
    float *st = reinterpret_cast<float *>(ring);                   // [32 rows][33]
    if constexpr (VL3) {                                           // the two lane halves of a row hold the two halves of its features
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float p = y[o] + y1[o];
            const float other = __shfl_xor(p, 32, 64);
            if (half == 0) st[(lane & 31) * 33 + o] = p + other;
        }
    } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) st[(lane & 31) * 33 + cd_row(r, lane)] = y[r] + y1[r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int row = 16 * it + (lane >> 2), part = lane & 3;
        const int e = e0 + row;
        if (e < a.E) {
            float yv[kQ];
#pragma unroll
            for (int i = 0; i < kQ; ++i) {
                const int j = part + 4 * i;
                yv[i] = j < a.nout ? st[row * 33 + j] + b3v[it][i] : 0.0f;
            }
            finish_quad(a.fin, yv, e, agent, part, tval[it], epval[it]);
        }
    }
}
#undef RT_PIN

// ---------------------------------------------------------------------------------------------------------
// Two-part float16 split (f16x2), ROW-TILE ownership with ONE weight ring per workgroup (round 6; dronesim_mlp_forward_f16x2_rt).
// The formulation of mlp3_rt_kernel on v_mfma_f32_32x32x16_f16: a wave owns 32 env rows of one agent and every output chunk of layer 2
// for them (kRtChunks accumulator tiles per pass, layer 1 recomputed in the second pass), layers meet in registers through the
// float16 split of the accumulator tile, layer 3 runs on the vector ALU in exact float32 (VL3: nout <= 4) or takes the split, relu'd
// layer-2 tiles as the B operand of its own blocks.  Against mlp3_split_kernel
// (wave w owns output chunks w, w + 4, ... of two row tiles): no layer-1 work and no relu + split repeated by four waves, no
// 4-3-3-3 dealing of 13 chunks -- 1053 instead of 1500 matrix instructions per 32 rows at h = 400 -- and HALF the weight bytes per
// matrix instruction, because the four waves of a workgroup consume the SAME stream: it travels global -> LDS once per workgroup,
// into a ring of kR16Depth = 4 super-stages of four 4-KiB blocks; wave w requests piece w of every block.  One s_barrier per
// super-stage (24 matrix instructions) orders it: a wave that is about to read the first block of super-stage S has waited for its own
// pieces of S (counted vmcnt), so behind the barrier S is complete in LDS; and every wave has consumed all of S - 2 (its reads of
// S - 1's last block may still be in flight: nobody drains its LDS queue for the barrier), so the slot of S - 2 takes super-stage
// S + 2.  No other barrier after the prologue.
// One agent's stream (blocks of four 1-KiB pieces [64 lanes][8 float16]; policies.py: pack_f16_rowtile_stream):
//   per pass p (output chunks S_p):  for c1:  L1(c1) = (W1 hi, W1 lo, 0, 0) of chunk c1 (one 16-wide k-step, linear k order),
//                                             L2(c1, c2) = (hi, lo of k-step 2 c1), (hi, lo of k-step 2 c1 + 1) for c2 in S_p
//                                             (accumulator k order: 16 s + 8 (j >> 2) + 4 half + (j & 3));
//                                    nout > 4 (layer 3 on the matrix cores), after the pass's in-chunks:  L3(c2) = (hi, lo of k-step 2 c2),
//                                             (hi, lo of k-step 2 c2 + 1) of W3^T, outputs zero-padded to 32, for c2 in S_p;
//   padded to whole super-stages, then three empty super-stages (the requests run two super-stages ahead, the reads one block).  Weights carry DroneMlpBf16.wscale like the split kernel's.
struct MArgsR16 {
    int E, N, d_in, h1, h2, nout, nc1, nc2, blocks;
    const float *x, *b1, *b2, *b3, *w3, *wscale;
    const char *ws;
    FinishArgs fin;
    unsigned rb_magic;
    long long *trace;                                             // developer trace builds only (tools/trace_rt16.py)
};

template <bool VL3>
__global__ void __launch_bounds__(256, 2) mlp3_rt16_kernel(const float *x, int E, int N, int d_in, const MArgsR16 rest)
{
    typedef SchemeF16x2 S;
    constexpr int P = 2;
    MArgsR16 a = rest;
    a.x = x; a.E = E; a.N = N; a.d_in = d_in;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int agent, row_block;
    xcd_work_item((a.E + kRtRows - 1) / kRtRows, agent, row_block, a.rb_magic);
    const int e0 = row_block * kRtRows + 32 * wave;                // this wave's 32 env rows (a wave without rows runs on clamped ones:
    const int half = lane >> 5;                                    // every wave takes part in every barrier)
    const int nc1 = a.nc1, nc2 = a.nc2;
    PT64(0);
    if (kTrace && a.trace && lane == 0) a.trace[((size_t)blockIdx.x * 4 + wave) * 64 + 32] = __builtin_amdgcn_s_memrealtime();
    if (kTrace && a.trace && lane == 0) {                          // where the workgroup runs: HW_ID (wave, simd, cu, sh, se ...) and the XCC
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
        a.trace[((size_t)blockIdx.x * 4 + wave) * 64 + 34] = (long long)hw | ((long long)xcc << 32);
    }
    float ws1 = 1.0f, ws2 = 1.0f, wi1 = 1.0f, wi2 = 1.0f, wi3 = 1.0f;
    if (a.wscale != nullptr) {
        ws1 = a.wscale[3 * (size_t)agent]; ws2 = a.wscale[3 * (size_t)agent + 1];
        wi1 = __builtin_amdgcn_rcpf(ws1); wi2 = __builtin_amdgcn_rcpf(ws2);
        if constexpr (!VL3) wi3 = __builtin_amdgcn_rcpf(a.wscale[3 * (size_t)agent + 2]);
    }
    float *sb1 = reinterpret_cast<float *>(smem);                  // b1 * ws1 | b2 * ws2, zero padded to whole chunks
    float *sb2 = sb1 + rt16_bias_floats(nc1);
    f32x4 *sw3 = reinterpret_cast<f32x4 *>(sb2 + rt16_bias_floats(nc2));   // VL3: W3[f][0..3] / layer 2's weight factor (zero beyond h2 / nout)
    char *ring = reinterpret_cast<char *>(sw3 + rt16_w3_rows(nc2, VL3));   // [kR16Depth][4 blocks][4 pieces][1 KiB], shared by the workgroup

    // ---- the weight stream: wave w requests piece w of every block (scalar base + this lane's 16-byte slot, by name)
    const unsigned long long sbase0 = reinterpret_cast<unsigned long long>(a.ws) + (unsigned long long)agent * a.blocks * 4096ull +
                                      (unsigned long long)wave * 1024ull;
    const unsigned voff = (unsigned)lane * 16u;
    const unsigned ring_a = lds_addr(ring);
    const unsigned rd_a = ring_a + voff;
    auto dma_super = [&](int sst) {                                // this wave's four pieces of super-stage sst
        const unsigned slot = ring_a + (unsigned)(sst & (kR16Depth - 1)) * 16384u + (unsigned)wave * 1024u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned long long src = sbase0 + (unsigned long long)(unsigned)(4 * sst + b) * 4096ull;
            const unsigned dst = slot + (unsigned)b * 4096u;
            dma_to_lds(dst, voff, src);
        }
    };
    dma_super(0);                                                  // primed ahead of the prologue's own loads

    // Prologue loads, all requested before anything waits: biases and W3 (at most four table entries per thread: h1, h2 <= 512; clamped
    // addresses, masked values: no branch around the loads), the x rows, the sampling counters, b3 -- then super-stages 1 and 2, so
    // that ONE counted wait (all but those eight requests) covers what the prologue needs and the first super-stage.
    const int total = (nc1 + nc2) * 32;
    float bv[4];
    f32x4 wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = min(tid + 256 * u, total - 1);
        const bool l1 = i < nc1 * 32;
        const int j = l1 ? i : i - nc1 * 32, h = l1 ? a.h1 : a.h2;
        bv[u] = (l1 ? a.b1 : a.b2)[(size_t)agent * h + min(j, h - 1)];
        if constexpr (VL3) {
            const size_t row = (size_t)agent * a.h2 + (l1 ? 0 : min(j, a.h2 - 1));
#pragma unroll
            for (int o = 0; o < 4; ++o) wv[u][o] = a.w3[row * a.nout + min(o, a.nout - 1)];
        }
    }
    float xv[8];
    {
        const int e = min(e0 + (lane & 31), a.E - 1);
        const float *xr = a.x + ((size_t)e * a.N + agent) * a.d_in;
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = xr[min(8 * half + j, a.d_in - 1)];
    }
    uint32_t tval[2] = {0u, 0u}, epval[2] = {0u, 0u};
    float b3v[2][kQ];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int e = e0 + 16 * it + (lane >> 2);
        if (e < a.E && a.fin.sample_kind != 0) {
            if (a.fin.t_dev) tval[it] = (uint32_t)a.fin.t_dev[e];
            if (a.fin.episode_dev) epval[it] = (uint32_t)a.fin.episode_dev[e];
        }
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int j = (lane & 3) + 4 * i;
            const float v = a.b3[(size_t)agent * a.nout + min(j, a.nout - 1)];
            b3v[it][i] = j < a.nout ? v : 0.0f;
        }
    }
    dma_super(1);
    dma_super(2);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    // the tables -> LDS (the W3 rows carry 1 / (layer 2's weight factor), a power of two)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid + 256 * u;
        if (i < total) {
            const bool l1 = i < nc1 * 32;
            const int j = l1 ? i : i - nc1 * 32, h = l1 ? a.h1 : a.h2;
            sb1[i] = __uint_as_float(__float_as_uint(bv[u]) & (j < h ? 0xffffffffu : 0u)) * (l1 ? ws1 : ws2);
            if constexpr (VL3) {
                if (!l1) {
                    f32x4 w;
#pragma unroll
                    for (int o = 0; o < 4; ++o) w[o] = __uint_as_float(__float_as_uint(wv[u][o]) & ((j < a.h2 && o < a.nout) ? 0xffffffffu : 0u)) * wi2;
                    sw3[j] = w;
                }
            }
        }
    }
    // the x operand of layer 1 (one 16-wide k-step, linear order: inputs 8 half + j of row lane & 31), split once
    Parts<P> xB;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v2[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) v2[t] = __uint_as_float(__float_as_uint(xv[2 * q + t]) & (8 * half + 2 * q + t < a.d_in ? 0xffffffffu : 0u));
        unsigned d[P];
        S::template split_pair<false>(v2[0], v2[1], d);
#pragma unroll
        for (int p = 0; p < P; ++p) xB.p[p][q] = d[p];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // this wave's table entries are in LDS (its pieces of super-stage 0 as well)
    __builtin_amdgcn_s_barrier();                                  // ... and everybody else's
    PT64(1);

    // ---- consumption.  wf[0..3] = the current block's pieces (k-step 0 hi, lo; k-step 1 hi, lo); a piece is re-read with the NEXT
    // block's bytes right behind its last product.  `cur` = index of the block whose pieces are being (re)loaded.
    u32x4 wf[4];
    int cur = 0;
    unsigned ra = rd_a;                                            // this lane's address of block `cur` in the ring
    // (requested in the order the pieces are consumed -- lo, hi of k-step 0, then lo, hi of k-step 1 -- so that the piece about to
    // be used is always the OLDEST of at most four reads in flight: every wait below is lgkmcnt(3))
    asm volatile("ds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %0, %4\n\tds_read_b128 %3, %4 offset:3072\n\tds_read_b128 %2, %4 offset:2048"
                 : "=&v"(wf[0]), "=&v"(wf[1]), "=&v"(wf[2]), "=&v"(wf[3]) : "v"(rd_a) : "memory");
    // the first read of a block: when it opens super-stage sst >= 1, the workgroup meets first (see the header)
    auto open_block = [&]() {
        ++cur;
        ra = rd_a + ((unsigned)cur & (4u * kR16Depth - 1u)) * 4096u;
        if ((cur & 3) == 0) {
            const int sst = cur >> 2;
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // this wave's pieces of sst have landed (sst + 1's four may be out)
            __builtin_amdgcn_s_barrier();
            dma_super(sst + 2);                                    // the slot of sst - 2: every wave is past its last block
        }
    };
    // (immediate offsets per piece: four variants by name)
    auto ring_read_p = [&](u32x4 &dst, auto PIECE) {
        constexpr int piece = decltype(PIECE)::value;
        const unsigned at = ra;
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(at), "n"(piece * 1024) : "memory");
    };
    typedef std::integral_constant<int, 0> P0; typedef std::integral_constant<int, 1> P1;
    typedef std::integral_constant<int, 2> P2; typedef std::integral_constant<int, 3> P3;
    // one k-step of a block: the scheme's three products (lo.hi, hi.lo, hi.hi) of pieces (hiP, loP) with the B parts `b`; each piece is
    // reloaded with the next block's bytes behind its last product; FIRST: this k-step opens the next block (k-step 0)
    // `live` (wave-uniform): false = the k-step holds no feature (ragged last chunk): its pieces only make way for the next block's.
    // NOTE the reads are UNCONDITIONAL and only the matrix instructions sit under the branch: a register that an asynchronous read
    // issued by name is still filling must never meet a control-flow join -- hipcc resolves the join with register copies and does
    // not know that the value is not there yet (the first cut of this kernel copied stale pieces that way).
    auto kstep = [&](f32x16 &acc, const Parts<P> &b, auto HI, auto LO, auto FIRST, bool live) {
        constexpr int hi = decltype(HI)::value, lo = decltype(LO)::value;
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(wf[lo]) :: "memory");
        if (live) acc = S::mfma(wf[lo], b.p[0], acc);              // lo . hi
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (decltype(FIRST)::value) open_block();
        ring_read_p(wf[lo], LO);
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(wf[hi]) :: "memory");
        if (live) {
            acc = S::mfma(wf[hi], b.p[1], acc);                    // hi . lo
            acc = S::mfma(wf[hi], b.p[0], acc);                    // hi . hi
        }
        __builtin_amdgcn_sched_barrier(0);
        ring_read_p(wf[hi], HI);
    };

    // layer 3 (vector ALU): this lane's partial sums of the outputs as two packed pairs (v_pk_fma_f32: two outputs per instruction),
    // two chains (even / odd chunks)
    f32x2 ya[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, yb[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    // nout > 4: layer 3 on the matrix cores, out^T[output][row] in two accumulator tiles (even / odd chunks)
    f32x16 y3a, y3b;
#pragma unroll
    for (int r = 0; r < 16; ++r) { y3a[r] = 0.0f; y3b[r] = 0.0f; }
    const int passes = rt_passes(nc2), per = rt_per_pass(nc2);
    for (int p = 0; p < passes; ++p) {
        const int c2_0 = p * per, npc = min(per, nc2 - c2_0);
        f32x16 acc2[kRtChunks];
#pragma unroll
        for (int i = 0; i < kRtChunks; ++i) acc2[i] = bias_tile(sb2 + min(c2_0 + i, nc2 - 1) * 32, lane);
        // in-chunk c1: layer 1 (block L1: pieces 0, 1 = W1 hi, lo; 2, 3 unused), relu + split -> the two k-steps' B operands, then its
        // two k-steps of every output chunk of the pass.  FULL: the chunk holds 32 features (every chunk but a ragged last one, whose
        // second k-step is empty when it has <= 16: the test is compiled only into the last chunk's copy of the code)
        auto in_chunk = [&](int c1, auto FULL) {
            f32x16 a1 = bias_tile(sb1 + c1 * 32, lane);
            kstep(a1, xB, P0{}, P1{}, std::true_type{}, true);
            kstep(a1, xB, P2{}, P3{}, std::false_type{}, false);
            Parts<P> hB0, hB1;
            { SplitJob<S, 0, 1> j(a1, hB0, wi1); j.all(); }
            { SplitJob<S, 1, 1> j(a1, hB1, wi1); j.all(); }
            const bool second = decltype(FULL)::value ? true : a.h1 - 32 * c1 > 16;
#pragma unroll
            for (int i = 0; i < kRtChunks; ++i) {
                if (i < npc) {
                    kstep(acc2[i], hB0, P0{}, P1{}, std::true_type{}, true);
                    kstep(acc2[i], hB1, P2{}, P3{}, std::false_type{}, second);
                }
            }
        };
        for (int c1 = 0; c1 < nc1 - 1; ++c1) { in_chunk(c1, std::true_type{}); PT64(2 + 14 * min(p, 1) + min(c1, 12)); }
        in_chunk(nc1 - 1, std::false_type{});
        PT64(2 + 14 * min(p, 1) + min(nc1 - 1, 12));
        // layer 3 on the vector ALU, exact float32: relu (the weight factor of layer 2 is undone by the table), 16 features x nout <= 4
        // per chunk and lane: per feature pair two v_max and four packed multiply-adds (the pair's relu'd values are the low / high
        // half of one 64-bit operand)
        if constexpr (!VL3) {
            // the pass's blocks L3(c2): the relu'd, split chunk is the B operand of its two k-steps, W3^T (outputs zero-padded to 32) the A
#pragma unroll
            for (int i = 0; i < kRtChunks; ++i) {
                if (i < npc) {
                    Parts<P> gB0, gB1;
                    { SplitJob<S, 0, 1> j(acc2[i], gB0, wi2); j.all(); }
                    { SplitJob<S, 1, 1> j(acc2[i], gB1, wi2); j.all(); }
                    const bool second = a.h2 - 32 * (c2_0 + i) > 16;
                    if (i & 1) {
                        kstep(y3b, gB0, P0{}, P1{}, std::true_type{}, true);
                        kstep(y3b, gB1, P2{}, P3{}, std::false_type{}, second);
                    } else {
                        kstep(y3a, gB0, P0{}, P1{}, std::true_type{}, true);
                        kstep(y3a, gB1, P2{}, P3{}, std::false_type{}, second);
                    }
                }
            }
        } else {
#pragma unroll
        for (int i = 0; i < kRtChunks; ++i) {
            if (i < npc) {
                const f32x4 *wp = sw3 + 32 * (c2_0 + i) + 4 * half;
                f32x2 (&y)[2] = (i & 1) ? yb : ya;
                f32x4 w3r[16];                                    // the chunk's 16 table rows of this lane, requested together
#pragma unroll
                for (int k = 0; k < 16; ++k) w3r[k] = wp[8 * (k >> 2) + (k & 3)];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int j = 0; j < 4; j += 2) {
                        f32x2 hv;
                        asm("v_max_f32 %0, 0, %1" : "=v"(hv.x) : "v"(acc2[i][4 * q + j]));
                        asm("v_max_f32 %0, 0, %1" : "=v"(hv.y) : "v"(acc2[i][4 * q + j + 1]));
                        const f32x4 w0 = w3r[4 * q + j], w1 = w3r[4 * q + j + 1];
                        const f32x2 w0a = {w0[0], w0[1]}, w0b = {w0[2], w0[3]}, w1a = {w1[0], w1[1]}, w1b = {w1[2], w1[3]};
                        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(y[0]) : "v"(w0a), "v"(hv));
                        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(y[1]) : "v"(w0b), "v"(hv));
                        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(y[0]) : "v"(w1a), "v"(hv));
                        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(y[1]) : "v"(w1b), "v"(hv));
                    }
                }
            }
        }
        }
        PT64(15 + 14 * min(p, 1));
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");    // no DMA may land late: the output tile reuses the ring
    __syncthreads();                                               // ... and no wave may still be reading it
    PT64(30);

    float *st = reinterpret_cast<float *>(ring) + wave * kRtTileFloats;
    if constexpr (VL3) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float pv = ya[o >> 1][o & 1] + yb[o >> 1][o & 1];
            const float other = __shfl_xor(pv, 32, 64);
            if (half == 0) st[(lane & 31) * 33 + o] = pv + other;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[(lane & 31) * 33 + cd_row(r, lane)] = (y3a[r] + y3b[r]) * wi3;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int row = 16 * it + (lane >> 2), part = lane & 3;
        const int e = e0 + row;
        if (e < a.E) {
            float yv[kQ];
#pragma unroll
            for (int i = 0; i < kQ; ++i) {
                const int j = part + 4 * i;
                yv[i] = j < a.nout ? st[row * 33 + j] + b3v[it][i] : 0.0f;
            }
            finish_quad(a.fin, yv, e, agent, part, tval[it], epval[it]);
        }
    }
    PT64(31);
    if (kTrace && a.trace && lane == 0) a.trace[((size_t)blockIdx.x * 4 + wave) * 64 + 33] = __builtin_amdgcn_s_memrealtime();   // (100 MHz)
}

}   // namespace

long long *dronesim_policy_trace = nullptr;
// developer hook (tools/trace_policy.py / trace_x3.py with a -DDRONESIM_TRACE build; not declared in include/dronesim.h)
extern "C" void dronesim_debug_set_policy_trace(long long *p) { dronesim_policy_trace = p; }

// developer hook (tests/test_policy_plan_host.py; not declared in include/dronesim.h): the plan of the launch that entry point `entry`
// (0 dronesim_mlp_forward with w2_layout = `layout`, 1 _f16x2_rt, 2 _bf16x3, 3 _f16x2, 4 _bf16) would make for a network of these
// dimensions with DroneMlpBf16.reserved = `reserved`, its arrays there or not (`arrays`) and its stream at `stream_addr` ->
// out[9] = (return code, PolicyFamily, variant, grid, threads, LDS bytes, opt-in, stream length, rb_magic); a refused launch and E = 0
// report the code only.  No HIP call is made.
extern "C" void dronesim_debug_policy_plan(int entry, int N, int d_in, int h1, int h2, int nout, int layout, int reserved, int arrays,
                                           uint64_t stream_addr, int E, int64_t *out)
{
    const int family = entry == 0 ? (layout == 2 ? kFamRt : kFamStaged) : entry == 1 ? kFamRt16 : entry == 4 ? kFamBf16 : kFamSplit;
    PolicyPlan p{};
    if ((p.rc = check_mlp(N, d_in, h1, h2, nout, 0, 0, E)) == 0)
        p = plan_policy_launch(family, N, d_in, h1, h2, nout, family == kFamSplit ? entry - 2 : layout, reserved, arrays != 0, (uintptr_t)stream_addr, E);
    const int64_t plan[9] = {p.rc, family, p.variant, p.grid, p.threads, (int64_t)p.lds, p.opt_in, p.stream, p.rb_magic};
    for (int i = 0; i < 9; ++i) out[i] = (i == 0 || (p.rc == 0 && E != 0)) ? plan[i] : 0;
}

// blocks (4 KiB each) of one agent's row-tile weight stream, zero padding included (DroneMlp.w2_layout = 2; see mlp3_rt_kernel)
// (nout <= 4: layer 3 runs on the vector ALU from the plain w3 array and the stream holds no L3 blocks)
extern "C" int dronesim_mlp_rt_blocks(int h1, int h2, int nout) { return (h1 < 1 || h2 < 1 || nout < 1) ? 0 : rt_blocks(chunks32(h1), chunks32(h2), nout); }

// blocks (4 KiB) of one agent's float16 row-tile stream (dronesim_mlp_forward_f16x2_rt): the real blocks rounded up to whole
// super-stages of four, plus kR16PadSupers super-stages of padding for the run-ahead of the DMA requests
extern "C" int dronesim_mlp_rt16_blocks(int h1, int h2, int nout) { return (h1 < 1 || h2 < 1 || nout < 1) ? 0 : rt16_blocks(chunks32(h1), chunks32(h2), nout); }

extern "C" int dronesim_mlp_forward_f16x2_rt(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                                             uint64_t seed, uint64_t counter, int64_t env_base,
                                             const int32_t *t, const int32_t *episode, int E, void *stream)
{
    static const PolicyLaunch<MArgsR16> variants[2] = {launch_policy<mlp3_rt16_kernel<false>>, launch_policy<mlp3_rt16_kernel<true>>};   // [VL3]
    // VL3 (nout <= 4): layer 3 on the vector ALU, from the plain float32 array in w3p
    return policy_forward("dronesim_mlp_forward_f16x2_rt", "mlp3_rt16_kernel", kFamRt16, variants, m, {x, out, act, act_idx, seed, counter, env_base, t, episode, E, stream},
                          0, m ? m->reserved : 0, m && m->w1p && (m->nout > 4 || m->w3p) && m->b1 && m->b2 && m->b3, m ? m->w1p : nullptr,
                          [m](MArgsR16 &r, const PolicyPlan &p) {
        r.nout = m->nout; r.nc1 = chunks32(m->h1); r.nc2 = chunks32(m->h2);
        r.blocks = p.stream; r.rb_magic = p.rb_magic;
        r.b1 = m->b1; r.b2 = m->b2; r.b3 = m->b3; r.w3 = reinterpret_cast<const float *>(m->w3p); r.wscale = m->wscale;
        r.ws = reinterpret_cast<const char *>(m->w1p);
    });
}

extern "C" int dronesim_mlp_forward(const DroneMlp *m, const float *x, float *out, float *act, int32_t *act_idx,
                                    uint64_t seed, uint64_t counter, int64_t env_base,
                                    const int32_t *t, const int32_t *episode, int E, void *stream)
{
    const PolicyCall c{x, out, act, act_idx, seed, counter, env_base, t, episode, E, stream};
    if (m && m->w2_layout != 2) return dronesim_mlp_forward_staged(m, &c);     // w2_layout = 0 / 1: the LDS-staged kernel (policy_f32.hip)
    // the row-tile stream: w2 = [N][dronesim_mlp_rt_blocks(h1, h2, nout)][4][64][4] float32 holding W1, b1, W2 and W3 in the
    // kernel's consumption order; w1 / b1 are not read, w3 (the plain array) only by VL3 (nout <= 4: layer 3 on the vector ALU)
    static const PolicyLaunch<MArgsR> variants[2] = {launch_policy<mlp3_rt_kernel<false>>, launch_policy<mlp3_rt_kernel<true>>};         // [VL3]
    return policy_forward("dronesim_mlp_forward", "mlp3_rt_kernel", kFamRt, variants, m, c, 2, 0, m && m->w2 && m->b2 && m->b3 && (m->nout > 4 || m->w3),
                          m ? m->w2 : nullptr, [m](MArgsR &r, const PolicyPlan &p) {
        r.nout = m->nout; r.nc1 = chunks32(m->h1); r.nc2 = chunks32(m->h2);
        r.blocks = p.stream; r.rb_magic = p.rb_magic;
        r.ws = m->w2; r.b2 = m->b2; r.b3 = m->b3; r.w3 = m->w3;
    });
}
