// policy_f32.hip -- the exact-float32 policy forward of rounds 2-5: mlp3_kernel, activations staged through LDS (dronesim_mlp_forward
// with DroneMlp.w2_layout = 0 / 1; the default is mlp3_rt_kernel in policy_rowtile.hip; which kernel serves which shape: policy_common.hpp).
// Arithmetic: exact float32 on the matrix cores -- v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain
// (no reduced precision), so results match a float32 torch reference to round-off.
// Decomposition: ceil(E/32) x N workgroups (XCD-aware order, see xcd_work_item): one workgroup = 32 env rows of ONE agent, 4 waves.
//   wave w owns every fourth 32-column chunk of the hidden layers (one 32x32 accumulator tile).
//   32 rows keep the workgroup at ~57 KiB of LDS, so two workgroups share a CU and one's prologue, barriers
//   and output stage overlap the other's MFMAs (64-row workgroups -- one per CU -- measured 6-12 % slower).
//   layer 1: x tile (LDS) x W1 (global/L2)                   -> relu -> h1 tile in LDS [32][ld1]
//   layer 2 chunk (32 columns): h1 (LDS) x W2 (fragment-packed, L2) -> relu -> per-wave LDS staging [32][36]
//   layer 3 partial: staged chunk x W3 rows of the chunk (v_mfma_f32_16x16x4_f32 when nout <= 16) -> registers
//   the four waves' partials are summed through LDS, then activation + sampling.
// With packed W2 (w2_layout = 1) and nout <= 16 layers 1 and 2 are
// computed transposed -- weights as the A operand -- so that tiles leave the accumulators as 16-byte row pieces
// (store_tile_tr); the plain-layout path (w2_layout = 0, or nout > 16) keeps the row-major tiles and odd LDS strides
// (h1 + 1, 33) of rounds 2-3.
#include "policy_common.hpp"

namespace {
struct MArgs {
    int E, N, d_in, h1, h2, nout;
    const float *x, *w1, *b1, *w2, *b2, *w3, *b3;
    FinishArgs fin;
    long long *trace;                    // developer trace builds only (NULL otherwise)
    unsigned rb_magic;                   // xcd_work_item: ceil(2^32 / row blocks), or 0
};

// acc += A[32 x K] * B[K x 32].  A row-major in LDS (lda floats per row, odd stride -> conflict-free), B row-major
// in global / L2 (ldb floats per row); B columns >= ncols_valid read a clamped column (never stored), k >= K reads
// as zero.  Operand loads of the next 8 k-steps are issued before the 8 MFMAs of the current ones.
constexpr int kU = 8;                  // k-steps (of 2) per pipeline stage

struct Frag { float b[kU], a[kU]; };

template <bool CHECK>                                   // CHECK: k >= K reads as zero (the ragged last stage)
__device__ __forceinline__ void load_frag(Frag &f, const float *Arow, const float *__restrict__ Bcol, int ldb, int kbase, int K)
{
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const int k = kbase + 2 * u;
        const int kc = CHECK ? min(k, K - 1) : k;          // clamped address, value masked below: no branches
        const float b = Bcol[(size_t)kc * ldb], av = Arow[kc];
        f.b[u] = (!CHECK || k < K) ? b : 0.0f;
        f.a[u] = (!CHECK || k < K) ? av : 0.0f;
    }
}

__device__ __forceinline__ void tile_gemm(f32x16 &acc, const float *A, int lda, const float *__restrict__ B, int ldb,
                                          int K, int ncols_valid, int lane)
{
    const int ar = lane & 31, kk = lane >> 5;
    const float *Bcol = B + min(ar, ncols_valid - 1);
    const float *Arow = A + ar * lda;
    const int Kmain = K - K % (2 * kU);                    // whole pipeline stages, no bounds checks inside
    if (Kmain > 0) {
        Frag cur, nxt;
        load_frag<false>(cur, Arow, Bcol, ldb, kk, K);
        // The first stage's operands are waited for HERE, once, ahead of the loop.  Left pending into the loop, they make
        // hipcc place counted waits (vmcnt(7) ... vmcnt(0)) in front of the eight MFMAs of the loop body -- needed on
        // the first trip, where the MFMAs' operands are those loads, but the same instructions then also wait on every
        // later trip, where the only loads in flight are the NEXT stage's: the prefetch distance collapsed from a full
        // stage (512 cycles of MFMAs) to the position inside the stage, and every stage stalled on the L2 latency
        // (round 2: 0.46 of the matrix peak).  With nothing pending at the loop's entry the only wait left is the one
        // in front of the `cur = nxt` copies, a whole stage after the loads were issued.
        __builtin_amdgcn_s_waitcnt(0x0070);                // vmcnt(0) lgkmcnt(0)
        for (int k0 = 0; k0 < Kmain; k0 += 2 * kU) {
            const bool more = k0 + 2 * kU < Kmain;         // wave-uniform
            if (more) load_frag<false>(nxt, Arow, Bcol, ldb, k0 + 2 * kU + kk, K);
#pragma unroll
            for (int u = 0; u < kU; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[u], cur.b[u], acc, 0, 0, 0);
            if (more) cur = nxt;
        }
    }
    if (Kmain < K) {                                       // ragged rest (and all of a K < 16 layer) as ONE masked stage:
        Frag t;                                            // its loads are in flight together instead of one per MFMA
        load_frag<true>(t, Arow, Bcol, ldb, Kmain + kk, K);
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (Kmain + 2 * u < K) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t.a[u], t.b[u], acc, 0, 0, 0);   // wave-uniform
    }
}

// ---- layer 2 on fragment-packed weights (DroneMlp.w2_layout = 1, what the host class passes) ------------------------
// One pipeline stage = 16 k-values = 8 MFMAs.  Lane (col = lane & 31, half = lane >> 5) feeds MFMA u of stage s with
// k = 16 s + 8 half + u: its eight A values are CONSECUTIVE floats of its h1 row in LDS (two ds_read_b128; the row
// stride is a multiple of 4 floats with an odd quotient, so the 16 lanes of a read phase hit 16 different bank
// quads), its eight B values two 16-byte pieces of the packed chunk
//     w2p[agent][chunk c][stage s][q][lane][4] = W2[16 s + 8 half + 4 q + jj][32 c + col]       (zero beyond h1 / h2)
// which the wave reads as two fully coalesced 1 KiB loads (scalar base + lane * 16 + immediate).  The reference-layout
// loop above needs 8 dword loads, 4 LDS reads, 16 64-bit address additions and 16 register copies per stage (4 VALU
// per MFMA -- round-3 counters: 7 VALU instructions per MFMA over the kernel, the matrix pipe 54-60 % busy with two
// waves per SIMD); this one 2 + 2 loads, no copies (R register sets, the loop unrolled R times) and scalar address
// updates, with the loads R - 1 stages ahead of their use.  Measured at the C5 shard (Gaussian actor, h = 400):
// reference layout 521 us; R = 1 / 2 / 3 / 4: 505 / 417-424 / 436-445 / 460 us -- one stage (512 matrix cycles) of
// distance is enough with a second wave on the SIMD, deeper only keeps more loads and registers in flight.  Requesting
// the next chunk's first stages and the chunk's W3 rows early (across the layer-3 part) was measured too: +-1 %.
// Per-wave trace of this kernel (tools/trace_policy.py gaussian c5 f32): layer 2 is 72 % of a wave's life, layer 1 20 %
// (8.4k ticks waiting for W1 / b1 / x, 13.7k for ~200 instructions: while the OTHER workgroup's wave on the SIMD streams
// matrix instructions, this one gets about one issue slot per matrix instruction); raising the issue priority of the
// waves outside their layer-2 loop (s_setprio 2 / 3) costs 2.4 % instead of helping.  Matrix pipe busy 70 % (54 %).
#define POLICY_SETS 2         // register sets of the pipeline (see tile_gemm_packed)
struct FragSet { f32x4 a0, a1, b0, b1; };

__device__ __forceinline__ void load_set(FragSet &t, const float *Arow, const f32x4 *Bp, int s)
{
    const f32x4 *ap = reinterpret_cast<const f32x4 *>(Arow + 16 * s);
    const f32x4 *bp = Bp + (size_t)s * 128;
    t.b0 = bp[0]; t.b1 = bp[64];
    t.a0 = ap[0]; t.a1 = ap[1];
}
template <bool TR>                        // TR: the transposed product D^T[feature][row] (the weights as the A operand)
__device__ __forceinline__ void mfma_set(f32x16 &acc, const FragSet &t)
{
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(TR ? t.b0[u] : t.a0[u], TR ? t.a0[u] : t.b0[u], acc, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(TR ? t.b1[u] : t.a1[u], TR ? t.a1[u] : t.b1[u], acc, 0, 0, 0);
}

// Transposed tiles (TR).  D[i][j] of v_mfma_f32_32x32x2_f32 puts FOUR CONSECUTIVE i (registers 4 q .. 4 q + 3 = rows
// 8 q + 4 (lane >> 5) + 0..3) of column j = lane & 31 into a lane.  With the weights as the A operand i is the feature and
// j the env row, so a lane's registers are contiguous pieces of its row of the next layer's input: the relu'd tile goes
// to LDS as four ds_write_b128 instead of sixteen ds_write_b32, and the bias -- one value per feature, i.e. per A row
// -- rides on one more matrix instruction (A = bias in the k slot of lanes 0..31, B = 1 there, 0 in the other k slot:
// fmaf(bias, 1, acc), rounded exactly like acc + bias) instead of sixteen v_add.  Per 32 x 32 tile: 16 v_max + 4 wide
// writes instead of 16 x (v_add, v_max, ds_write_b32).  Every instruction saved here is an issue slot the OTHER
// workgroup's wave on the SIMD gets for its matrix stream (the float32 matrix instructions run on the vector ALUs).
__device__ __forceinline__ f32x16 bias_mfma(f32x16 acc, float bias, int lane)
{
    return __builtin_amdgcn_mfma_f32_32x32x2f32(lane < 32 ? bias : 0.0f, lane < 32 ? 1.0f : 0.0f, acc, 0, 0, 0);
}
template <bool RELU>
__device__ __forceinline__ void store_tile_tr(float *rowp, const f32x16 &acc, int lane)     // rowp: this lane's row + chunk offset
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = RELU ? fmaxf(acc[4 * q + t], 0.0f) : acc[4 * q + t];
        *reinterpret_cast<f32x4 *>(rowp + 8 * q + 4 * (lane >> 5)) = v;
    }
}

// acc += (h1 tile, stages [sb, sb + n)) x (packed chunk).  Arow: this lane's LDS row + 8 half; Bp: chunk base + lane.
template <int R, bool TR>
__device__ __forceinline__ void tile_gemm_packed(f32x16 &acc, const float *Arow, const f32x4 *Bp, int sb, int n)
{
    FragSet set[R];
    if (n < R - 1) {                                         // (a hidden layer of <= 16 (R - 2) units)
        for (int s1 = 0; s1 < n; ++s1) { load_set(set[0], Arow, Bp, sb + s1); mfma_set<TR>(acc, set[0]); }
        return;
    }
#pragma unroll
    for (int r = 0; r < R - 1; ++r) load_set(set[r], Arow, Bp, sb + r);
    int s = 0;
    // steady state: R stages per trip, every load unconditional (a conditional one makes hipcc wait for one stage more
    // than needed at the join, which costs a whole stage of prefetch distance)
    for (const int last = n - (2 * R - 1); s <= last; s += R) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            load_set(set[(r + R - 1) % R], Arow, Bp, sb + s + r + R - 1);
            mfma_set<TR>(acc, set[r]);
        }
    }
    // the last <= 2 R - 2 stages
#pragma unroll
    for (int r = 0; r < 2 * R - 2; ++r) {
        if (s + r < n) {                                     // wave-uniform
            if (s + r + R - 1 < n) load_set(set[(r + R - 1) % R], Arow, Bp, sb + s + r + R - 1);
            mfma_set<TR>(acc, set[r % R]);
        }
    }
}

// ---- layer 3 of a chunk for nout <= 16 (every network of the reference: 16 action probabilities, 4 Gaussian moments, 1
// value) on v_mfma_f32_16x16x4_f32.  The 32x32x2 form spends 16 matrix instructions of 64 cycles per chunk on 32 output
// columns of which at most 16 exist (8 % of the kernel's matrix time at h = 400); two 16-row tiles x 8 k-steps of the
// 16-column instruction are 16 x 32 cycles.  Lane (i = lane & 15, g = lane >> 4) feeds k-step ks with k = 8 g + ks (any
// assignment of the chunk's 32 k values to (g, ks) is a valid contraction order; this one makes a lane's eight A values
// CONSECUTIVE floats of its staged row: two ds_read_b128 per tile instead of eight ds_read_b32; kStN = 36 floats per
// row = a multiple of 4 with an odd quotient, so the 8 lanes of a read phase hit different bank quads) and reads its
// eight W3 values once for both tiles.  D: reg r of lane l = (row 4 (l >> 4) + r, col l & 15).
__device__ __forceinline__ void layer3_narrow(f32x4 (&y)[2], const float *st, const float *__restrict__ w3c, int nout, int kvalid, int lane)
{
    const int g = lane >> 4, i = lane & 15, c = min(i, nout - 1);
    float b[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int k = 8 * g + ks;
        const float w = w3c[(size_t)min(k, kvalid - 1) * nout + c];                 // clamped address, masked value
        b[ks] = k < kvalid ? w : 0.0f;
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const f32x4 *ap = reinterpret_cast<const f32x4 *>(st + (mt * 16 + i) * kStN + 8 * g);
        const f32x4 a0 = ap[0], a1 = ap[1];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) y[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[ks], b[ks], y[mt], 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) y[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[ks], b[4 + ks], y[mt], 0, 0, 0);
    }
}

// kRows env rows of one agent per workgroup, 4 waves per 32-row tile: wave w owns feature chunks (w & 3),
// (w & 3) + 4, ... of the rows of tile (w >> 2).
// NU: k-steps (of 2) of layer 1 that are loaded and issued when d_in <= 16 (3 for the reference's simplified observation,
// d_in = 6; compile-time so that the loads stay unconditional -- wave-uniform `if (u < nu)` around them was measured +2 %:
// hipcc drains the loads at every join)
template <bool PACKED, bool NARROW, int NU = kU>      // PACKED: W2 in the fragment layout of tile_gemm_packed; NARROW: nout <= 16
__global__ void __launch_bounds__(kThreadsF, 2) mlp3_kernel(const float *x, int E, int N, int d_in, const MArgs rest)
{
    MArgs a = rest;                      // leading scalars are preloaded into SGPRs at wave launch (csrc/Makefile)
    a.x = x; a.E = E; a.N = N; a.d_in = d_in;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int agent, row_block;
    xcd_work_item((a.E + kRows - 1) / kRows, agent, row_block, a.rb_magic);
    // (rotating which wave owns the chunks 0, 4, 8, ... -- one more chunk than the others at h = 400 -- with the row block,
    // so that the heavy waves of the two workgroups on a CU sit on different SIMDs, was measured in round 3: +-1 %)
    const int cw = wave & 3, rh = wave >> 2;
    const int e0 = row_block * kRows;
    const int ldx = a.d_in + 1, ld1 = PACKED ? packed_row_stride(a.h1) : a.h1 + 1;
    float *sx = reinterpret_cast<float *>(smem);                 // [rows][d_in+1]
    float *sh1 = sx + f32_tile_floats(ldx);                      // [rows][h1+1]
    constexpr int kSt = NARROW ? kStN : kStW;
    constexpr bool TR = PACKED && NARROW;                        // transposed tiles (see store_tile_tr)
    float *sst = sh1 + f32_tile_floats(ld1);                     // [waves][32][kSt] layer-2 chunk staging,
                                                                 // reused for the layer-3 partials
    const float *w1 = a.w1 + (size_t)agent * a.d_in * a.h1, *b1 = a.b1 + (size_t)agent * a.h1;
    const int nst = (a.h1 + 15) >> 4;                            // PACKED: 16-k stages of layer 2
    const float *w2 = a.w2 + (PACKED ? (size_t)agent * ((a.h2 + 31) >> 5) * nst * 512 : (size_t)agent * a.h1 * a.h2);
    const float *b2 = a.b2 + (size_t)agent * a.h2;
    const float *w3 = a.w3 + (size_t)agent * a.h2 * a.nout, *b3 = a.b3 + (size_t)agent * a.nout;

    PT(0);
    const unsigned long long rt0 = kTrace ? __builtin_amdgcn_s_memrealtime() : 0ull;   // trace builds: 100 MHz clock at entry
    const int col = lane & 31;
    constexpr int kL1 = 4;
    float wb[kL1][NU], bias[kL1];
    const bool small_k = NU < kU || a.d_in <= 2 * kU;            // (the NU = 3 instance is only launched with d_in <= 6)
    if (small_k) {                                               // layer 1's weights travel together with the x tile
#pragma unroll
    for (int i = 0; i < kL1; ++i) {
        // no branch around these loads, not even the wave-uniform `chunk exists`: hipcc drains the loads of a
        // conditional block at its join (s_waitcnt vmcnt(0) per chunk: four round trips in series, 10k cycles of a wave's
        // 100k); a chunk that does not exist re-reads the last column and is never used
        const int c0 = cw * 32 + 128 * i, cc = min(c0 + col, a.h1 - 1);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int k = (lane >> 5) + 2 * u;
            const float w = w1[(size_t)min(k, a.d_in - 1) * a.h1 + cc];            // clamped address, masked value
            wb[i][u] = k < a.d_in ? w : 0.0f;
        }
        const float bv = b1[cc];
        bias[i] = c0 + col < a.h1 ? bv : 0.0f;
    }
    }
    // ---- x tile -> LDS (rows beyond E are zero)
    if (a.d_in <= 8) {                                       // eight lanes per row: no per-thread division
        const int r = tid >> 3, c = tid & 7, e = e0 + r;
        if (c < a.d_in) sx[r * ldx + c] = e < a.E ? a.x[((size_t)e * a.N + agent) * a.d_in + c] : 0.0f;
    } else
    for (int idx = tid; idx < kRows * a.d_in; idx += kThreadsF) {
        const int r = idx / a.d_in, c = idx - r * a.d_in;
        const int e = e0 + r;
        sx[r * ldx + c] = e < a.E ? a.x[((size_t)e * a.N + agent) * a.d_in + c] : 0.0f;
    }
    __syncthreads();
    PT(1);

    // ---- layer 1: K = d_in is tiny, so the operands of ALL of this wave's chunks (<= 4: h1 <= 512) and their
    //      biases are requested together -- one global round trip for the layer instead of two per chunk
    if (small_k) {
        const float *Arow = sx + (rh * 32 + (lane & 31)) * ldx;
        float xa[NU];                                            // the x operand is the same for every chunk
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int k = (lane >> 5) + 2 * u;
            const float v = Arow[min(k, a.d_in - 1)];
            xa[u] = k < a.d_in ? v : 0.0f;
        }
        if (kTrace) {
            __builtin_amdgcn_s_waitcnt(0x0070);                  // trace builds: stamp 7 = layer 1's operands have arrived
            PT(7);
        }
#pragma unroll
        for (int i = 0; i < kL1; ++i) {
            const int c0 = cw * 32 + 128 * i;
            if (c0 < a.h1) {
                f32x16 acc = {0};
                if (TR) {
                    const bool ok = c0 + col < a.h1;             // features beyond h1 (the k padding of layer 2) come out as zero
#pragma unroll
                    for (int u = 0; u < NU; ++u)
                        if (2 * u < a.d_in) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? wb[i][u] : 0.0f, xa[u], acc, 0, 0, 0);
                    acc = bias_mfma(acc, bias[i], lane);
                    store_tile_tr<true>(sh1 + (rh * 32 + col) * ld1 + c0, acc, lane);
                    continue;
                }
#pragma unroll
                for (int u = 0; u < NU; ++u)
                    if (2 * u < a.d_in) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u], wb[i][u], acc, 0, 0, 0);
                if (c0 + col < a.h1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        sh1[(rh * 32 + cd_row(r, lane)) * ld1 + c0 + col] = fmaxf(acc[r] + bias[i], 0.0f);
                } else if (PACKED) {                             // the k padding of the last stage reads as zero
#pragma unroll
                    for (int r = 0; r < 16; ++r) sh1[(rh * 32 + cd_row(r, lane)) * ld1 + c0 + col] = 0.0f;
                }
            }
        }
    } else {
        for (int c0 = cw * 32; c0 < a.h1; c0 += 128) {
            const bool ok = c0 + col < a.h1;
            const float bias = ok ? b1[c0 + col] : 0.0f;
            f32x16 acc = {0};
            tile_gemm(acc, sx + rh * 32 * ldx, ldx, w1 + c0, a.h1, a.d_in, a.h1 - c0, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (ok) sh1[(rh * 32 + cd_row(r, lane)) * ld1 + c0 + col] = fmaxf(acc[r] + bias, 0.0f);
                else if (PACKED) sh1[(rh * 32 + cd_row(r, lane)) * ld1 + c0 + col] = 0.0f;
            }
        }
    }
    PT(2);
    __syncthreads();
    PT(3);

    // the output stage's inputs (4 lanes per row), requested now so that their latency hides behind layers 2 + 3
    uint32_t tval = 0u, epval = 0u;
    float b3v[kQ];
    {
        const int e = e0 + (tid >> 2);
        if (tid < 4 * kRows && e < a.E && a.fin.sample_kind != 0) {
            if (a.fin.t_dev) tval = (uint32_t)a.fin.t_dev[e];
            if (a.fin.episode_dev) epval = (uint32_t)a.fin.episode_dev[e];
        }
#pragma unroll
        for (int i = 0; i < kQ; ++i) b3v[i] = (tid & 3) + 4 * i < a.nout ? b3[(tid & 3) + 4 * i] : 0.0f;
    }

    // ---- layers 2 + 3 fused over this wave's column chunks.  The chunk count is rarely a multiple of four (13 at
    // h = 400, 10 at h = 300, 7 at h = 200): dealt whole, one wave gets a chunk more than the others, runs 4 : 3 longer and
    // the other three wait for it holding their slots (round 3 trace: 140k against 110-116k cycles per wave, the matrix
    // pipe 54 % busy).  So only whole rounds of four chunks are dealt, and the leftover chunks are SPLIT BY K in one more
    // trip: one leftover chunk over the four waves (a quarter of the h1 range each), two leftover chunks over two pairs of
    // waves (half the range each); the partial tiles meet in LDS and one wave per chunk finishes it.
    f32x16 y = {0};
    f32x4 yn[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    float *st = sst + wave * f32_stage_floats(kSt);
    const int nch = (a.h2 + 31) >> 5;
    // Measured at the C5 shard: one leftover (13 chunks at h = 400) -5.5 %, -4.3 % at C3; two leftovers (10 chunks at h = 300)
    // as pairs -8.7 % (round 4; as two quarter-split trips, i.e. four barriers, +1.5 %); three leftovers (7 chunks at
    // h = 200) lose either way (three quarter-split trips +19 %, a pair trip + a quarter trip +4 %) and are dealt whole
    const int rem = (nch & 3) == 3 ? 0 : (nch & 3);              // leftover chunks that are split (3: dealt whole)
    const int nch_even = rem ? (nch & ~3) : nch;
    const int split = rem == 2 ? 2 : 4;                          // waves sharing a leftover chunk
    const int ntrips = rem ? 1 : 0;
    // ONE loop over both kinds of trips (one inlined copy of each GEMM: a second copy of the layer-2 loop took the kernel
    // from 244 to 272 registers, i.e. from two workgroups per CU to one): first the whole rounds, then the leftover chunks
    const int rounds = (nch_even + 3) >> 2;                      // (whole dealing: the last round may be ragged)
    const int kpad = PACKED ? 16 * nst : a.h1;
    for (int it = 0; it < rounds + ntrips; ++it) {               // wave-uniform trip count (barriers inside)
        const bool left = it >= rounds;                          // leftover trip: this wave's K part of a leftover chunk
        const int part = cw & (split - 1);                       // this wave's K part
        const int lch = nch_even + (rem == 2 ? cw >> 1 : 0);
        const int c0 = (left ? lch : cw + 4 * it) * 32;
        if (!left && c0 >= nch_even * 32) continue;              // ragged last round of the whole dealing (no barrier in it)
        const int kq = PACKED ? 16 * ((nst + split - 1) / split) : (((a.h1 + split - 1) / split) + 1) & ~1;   // 1/split of K (even; PACKED: whole stages)
        const int kb = left ? min(part * kq, kpad) : 0, kn = left ? min(kq, kpad - kb) : kpad;
        const bool ok = c0 + col < a.h2;
        const float bias = ok ? b2[c0 + col] : 0.0f;             // issued before the k-loop, needed after it
        f32x16 acc = {0};
        // A single leftover chunk with at most 16 features (h2 = 400: the 13th chunk holds 16) is computed on the 16-column
        // instruction: D[16 features][16 rows] x two row tiles x 4 k per step = 8 instructions of 32 cycles per 16 k
        // instead of 8 of 64 on a tile whose other 16 feature rows are padding.  Lane (i = lane & 15, g = lane >> 4) takes
        // k = 16 s + 4 g + t at step t of stage s: its four weights are ONE 16-byte piece of the chunk's ordinary packed
        // stage ([q = g & 1][lane i + 32 (g >> 1)]: no other layout needed), its four h1 values one ds_read_b128 per row tile.
        const bool half16 = TR && left && split == 4 && a.h2 - c0 <= 16;     // wave-uniform
        if (half16) {
            const int i16 = lane & 15, g4 = lane >> 4;
            const f32x4 *Wp = reinterpret_cast<const f32x4 *>(w2 + (size_t)(c0 >> 5) * nst * 512) + (g4 & 1) * 64 + i16 + 32 * (g4 >> 1);
            const float *hr0 = sh1 + i16 * ld1 + 4 * g4, *hr1 = hr0 + 16 * ld1;
            const float bh = (part == 0 && c0 + i16 < a.h2) ? b2[c0 + i16] : 0.0f;
            f32x4 ha[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
            const int s0 = kb >> 4, sn = kn >> 4;
            if (sn > 0) {
                f32x4 wv = Wp[(size_t)s0 * 128];
                f32x4 x0 = *reinterpret_cast<const f32x4 *>(hr0 + 16 * s0), x1 = *reinterpret_cast<const f32x4 *>(hr1 + 16 * s0);
                for (int s1 = 0; s1 < sn; ++s1) {
                    const int sx2 = s0 + min(s1 + 1, sn - 1);                     // next stage (the last one re-reads itself: no branch)
                    const f32x4 wn = Wp[(size_t)sx2 * 128];
                    const f32x4 y0 = *reinterpret_cast<const f32x4 *>(hr0 + 16 * sx2), y1 = *reinterpret_cast<const f32x4 *>(hr1 + 16 * sx2);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        ha[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], x0[t], ha[0], 0, 0, 0);
                        ha[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], x1[t], ha[1], 0, 0, 0);
                    }
                    wv = wn; x0 = y0; x1 = y1;
                }
            }
            if (part == 0) {                                     // bias on the matrix pipe (k slot of lanes 0..15), as in bias_mfma
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    ha[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g4 == 0 ? bh : 0.0f, g4 == 0 ? 1.0f : 0.0f, ha[rt], 0, 0, 0);
            }
            // D: register r of lane (i, g) = (feature 4 g + r, row 16 rt + i) -> this wave's partial tile [row][feature]
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) *reinterpret_cast<f32x4 *>(st + (rt * 16 + i16) * kSt + 4 * g4) = ha[rt];
            __syncthreads();
            if (part == 0) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    f32x4 *p = reinterpret_cast<f32x4 *>(st + (rt * 16 + i16) * kSt + 4 * g4);
                    f32x4 v = ((p[0] + p[32 * kSt / 4]) + p[2 * 32 * kSt / 4]) + p[3 * 32 * kSt / 4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.0f);
                    p[0] = v;
                    p[4] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};      // features 16 .. 31 of the staged chunk read as zero in layer 3
                }
            }
        } else
        if (PACKED) {
            if (kn > 0)
                tile_gemm_packed<POLICY_SETS, TR>(acc, sh1 + (rh * 32 + col) * ld1 + 8 * (lane >> 5),
                                    reinterpret_cast<const f32x4 *>(w2 + (size_t)(c0 >> 5) * nst * 512) + lane, kb >> 4, kn >> 4);
        } else if (kn > 0)
            tile_gemm(acc, sh1 + rh * 32 * ld1 + kb, ld1, w2 + c0 + (size_t)kb * a.h2, a.h2, kn, a.h2 - c0, lane);
        bool l3 = true;                                          // this wave feeds the chunk to layer 3
        if (half16) l3 = part == 0;
        else if (TR) {                                           // (packed W2 and the masked bias are zero beyond h2)
            if (!left || part == 0) acc = bias_mfma(acc, bias, lane);
            if (!left) store_tile_tr<true>(st + col * kSt, acc, lane);
            else {
                store_tile_tr<false>(st + col * kSt, acc, lane);                     // this wave's partial tile (part 0: + bias)
                __syncthreads();
                l3 = part == 0;                                  // one wave per chunk adds the partials in a fixed order
                if (l3) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 *p = reinterpret_cast<f32x4 *>(st + col * kSt + 8 * q + 4 * (lane >> 5));
                        f32x4 v = p[0] + p[32 * kSt / 4];
                        if (split == 4) v = (v + p[2 * 32 * kSt / 4]) + p[3 * 32 * kSt / 4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.0f);
                        p[0] = v;
                    }
                }
            }
        } else if (!left) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[cd_row(r, lane) * kSt + col] = ok ? fmaxf(acc[r] + bias, 0.0f) : 0.0f;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[cd_row(r, lane) * kSt + col] = acc[r];     // this wave's partial tile
            __syncthreads();
            l3 = part == 0;                                      // one wave per chunk adds the partials in a fixed order
            if (l3) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = cd_row(r, lane) * kSt + col;
                    float v = st[o] + st[32 * kSt + o];
                    if (split == 4) v = (v + st[2 * 32 * kSt + o]) + st[3 * 32 * kSt + o];
                    st[o] = ok ? fmaxf(v + bias, 0.0f) : 0.0f;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (l3) {
            if (NARROW) layer3_narrow(yn, st, w3 + (size_t)c0 * a.nout, a.nout, min(32, a.h2 - c0), lane);
            else tile_gemm(y, st, kStW, w3 + (size_t)c0 * a.nout, a.nout, min(32, a.h2 - c0), a.nout, lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (left) __syncthreads();                               // the partial regions are free again
    }
    PT(4);
    if (NARROW) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[(mt * 16 + 4 * (lane >> 4) + r) * kSt + (lane & 15)] = yn[mt][r];
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[cd_row(r, lane) * kSt + col] = y[r];   // this wave's partial outputs
    }
    __syncthreads();
    PT(5);
    if (kTrace && a.trace && lane == 0 && wave >= 2)             // (slot 6 of waves 2, 3 is free: the finish stamp is waves 0, 1)
        a.trace[((size_t)blockIdx.x * 4 + wave) * 8 + 6] = (long long)(__builtin_amdgcn_s_memrealtime() - rt0);

    // ---- output activation + sampling: four lanes per env row
    if (tid < 4 * kRows) {
        const int row = tid >> 2, part = tid & 3;
        const int e = e0 + row;
        if (e >= a.E) return;
        const int rhh = row >> 5, rr = row & 31;
        float yv[kQ];
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int j = part + 4 * i;
            float v = 0.0f;
            if (j < a.nout) {
                v = b3v[i];
#pragma unroll
                for (int w = 0; w < 4; ++w) v += sst[((rhh * 4 + w) * 32 + rr) * kSt + j];
            }
            yv[i] = v;
        }
        finish_quad(a.fin, yv, e, agent, part, tval, epval);
        PT(6);
    }
}

}   // namespace

extern "C" int dronesim_mlp_forward_staged(const DroneMlp *m, const PolicyCall *c)
{
    static const PolicyLaunch<MArgs> variants[5] = {launch_policy<mlp3_kernel<false, false>>, launch_policy<mlp3_kernel<false, true>>,    // [2 PACKED + NARROW]
                                                    launch_policy<mlp3_kernel<true, false>>, launch_policy<mlp3_kernel<true, true>>,
                                                    launch_policy<mlp3_kernel<true, true, 3>>};                                          // d_in <= 6
    return policy_forward("dronesim_mlp_forward", "mlp3_kernel", kFamStaged, variants, m, *c, m->w2_layout, 0,
                          m->w1 && m->b1 && m->w2 && m->b2 && m->w3 && m->b3, m->w2, [m](MArgs &a, const PolicyPlan &p) {
        a.nout = m->nout; a.rb_magic = p.rb_magic;
        a.w1 = m->w1; a.b1 = m->b1; a.w2 = m->w2; a.b2 = m->b2; a.w3 = m->w3; a.b3 = m->b3;
    });
}
