// policy_common.hpp -- what the translation units of the batched policy forward share (policy_*.hip; not part of the C ABI).
//
// The reference evaluates one small torch MLP per agent per step in a Python loop
// (SAC_agents.py:170-180 -> utils.py:304-309 / 110-117 / 40-53): with the environment on the device this
// is the whole rollout time.  Here ALL agents' networks run in one launch over the
// batched observation z[E][N][d_in]:
//     h1 = relu(x W1_i + b1_i)        utils.py:291-292 / 91-92 / 42-43
//     h2 = relu(h1 W2_i + b2_i)       utils.py:295-296 / 95-99 / 46-47
//     y  = h2 W3_i + b3_i             utils.py:299 / 102-106 / 50
//     out = softmax(y) | (tanh, sigmoid) | y       utils.py:300 / 103,106 / --
// plus the sampling of sample_action (categorical over unit-circle actions utils.py:262-269,304-309;
// Gaussian utils.py:110-117) from a counter-based Philox stream (finish_quad below, shared by every kernel).
//
// Five kernel generations sit behind the six entry points of include/dronesim.h, one file per family (DEFAULT = what the host class runs):
//   policy_rowtile.hip  mlp3_rt_kernel     exact f32, a wave owns 32 rows and every output chunk (round 6): dronesim_mlp_forward, w2_layout = 2, DEFAULT
//                       mlp3_rt16_kernel   f16x2 split, same ownership, one ring per workgroup (round 6): dronesim_mlp_forward_f16x2_rt, DEFAULT of "f16x2"
//   policy_f32.hip      mlp3_kernel        exact f32, activations staged through LDS (rounds 2-5): dronesim_mlp_forward, w2_layout = 0 / 1
//   policy_split.hip    mlp3_split_kernel  bf16x3 / f16x2 splits, a wave owns output chunks w, w + 4, ... (rounds 2-5): dronesim_mlp_forward_bf16x3, _f16x2
//   policy_bf16.hip     mlp3_bf16_kernel   plain bf16, float32 accumulation (opt-in): dronesim_mlp_forward_bf16
// The superseded generations stay: they are part of the C ABI and the tests drive them.  Everything here lives in an unnamed
// namespace -- every translation unit gets its own copy, and the kernels keep the names they had in one file.
#pragma once
#include <stdio.h>
#include <mutex>
#include "common.hpp"
#include "dronesim.h"

// developer trace builds (kTrace, common.hpp) only: the stamps' buffer, set through dronesim_debug_set_policy_trace (policy_rowtile.hip)
extern __attribute__((visibility("hidden"))) long long *dronesim_policy_trace;
// w2_layout = 0 / 1 of dronesim_mlp_forward (policy_rowtile.hip) -> the LDS-staged kernel (policy_f32.hip); m, x, dimensions are checked
extern "C" __attribute__((visibility("hidden"))) int dronesim_mlp_forward_staged(
    const DroneMlp *m, const float *x, float *out, float *act, int32_t *act_idx, uint64_t seed, uint64_t counter, int64_t env_base,
    const int32_t *t, const int32_t *episode, int E, void *stream);

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int kMaxOut = 32;

// per-wave phase stamps of the trace builds: a.trace[workgroups][4 waves][8] (mlp3_rt16_kernel: [64] stamps -- tools/trace_rt16.py)
#define PT64(k) do { if (kTrace && a.trace && lane == 0) a.trace[((size_t)blockIdx.x * 4 + wave) * 64 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define PT(k) do { if (kTrace && a.trace && lane == 0) a.trace[((size_t)blockIdx.x * 4 + wave) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)

struct FinishArgs {
    int N, nout, out_kind, sample_kind;
    float *out, *act;
    int *act_idx;
    uint32_t key0, key1, ctr2, ctr3;
    long long env_base;
    const int *t_dev, *episode_dev;
};

// Workgroup -> (agent, row block).  The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs,
// each with its own 4 MiB L2; all agents' weights together (12.8 MiB in bf16 / 23 MiB in f32 at N = 64,
// h = 300) do not fit one L2, a few agents' do.  So the work list is ordered agent-major and cut into 8
// contiguous pieces, one per XCD: XCD x walks its own agents one after the other, the ~64 workgroups resident
// on it at any time share one or two agents' weights, and every weight byte leaves HBM once per launch.
// `magic` = ceil(2^32 / row_blocks) from the host when total x row_blocks < 2^32 (then umulhi(v, magic) = v / row_blocks
// exactly for every v < total), else 0: a run-time integer division is ~25 instructions of this prologue, each of which
// waits for an issue slot next to the other workgroup's matrix stream.
__host__ inline unsigned div_magic(unsigned long long total, unsigned d)
{
    return (d > 1 && total * d < (1ull << 32)) ? (unsigned)(((1ull << 32) + d - 1) / d) : 0u;
}
// (`magic` travels by reference ON PURPOSE: by value, a translation unit whose kernels all pass 0 -- policy_bf16.hip, policy_split.hip -- has the constant
// propagated into this function ahead of inlining, and those kernels' prologues come out in another instruction order than when all generations shared a file)
__device__ __forceinline__ void xcd_work_item(int row_blocks, int &agent, int &row_block, const unsigned &magic = 0u)
{
    const int total = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int q = total >> 3, r = total & 7;
    const int v = xcd * q + min(xcd, r) + slot;            // XCD x owns q + (x < r) items
    agent = magic ? (int)__umulhi((unsigned)v, magic) : v / row_blocks;
    row_block = v - agent * row_blocks;
}

// C/D layout of v_mfma_f32_32x32x2_f32: element reg r of lane l is (row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31)
__device__ __forceinline__ int cd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Output activation + sampling of ONE env row by the 4 adjacent lanes of a quad: lane `part` holds the
// pre-activation outputs j = part + 4 i (i < 8) in y[i].  Reductions over the row (softmax max / sum, the
// categorical cdf) run on DPP quad permutes, so the serial tail of the kernel is a quarter as long and the
// probabilities leave as 16-byte segments.  tval / epval: the env's step and episode counters (0 if absent).
constexpr int kQ = kMaxOut / 4;

template <int CTRL> __device__ __forceinline__ float quad_perm(float v)     // CTRL = quad_perm:[a,b,c,d] = a | b<<2 | c<<4 | d<<6
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kQuadUp1 = 0x90, kQuadUp2 = 0x40, kQuadLast = 0xFF;

__device__ __forceinline__ void finish_quad(const FinishArgs &a, float (&y)[kQ], int e, int agent, int part,
                                            uint32_t tval, uint32_t epval)
{
    const int nout = a.nout;
    if (a.out_kind == 1) {                                   // softmax (utils.py:286, dim = 0 of one sample)
        float m = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < kQ; ++i) if (part + 4 * i < nout) m = fmaxf(m, y[i]);
        m = fmaxf(m, quad_perm<kQuadXor1>(m));
        m = fmaxf(m, quad_perm<kQuadXor2>(m));
        float ssum = 0.0f;
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            // (v_exp_f32 = 2^x, 1 ulp: the library expf is ~15 instructions of range reduction for arguments that are <= 0
            // here, and every vector instruction of this tail waits for an issue slot next to the other workgroup's
            // matrix stream -- about one per 64 cycles, DESIGN_LOG round 5)
            if (4 * i < nout) { y[i] = part + 4 * i < nout ? __builtin_amdgcn_exp2f((y[i] - m) * 1.4426950408889634f) : 0.0f; ssum += y[i]; }
            else y[i] = 0.0f;
        }
        ssum += quad_perm<kQuadXor1>(ssum);
        ssum += quad_perm<kQuadXor2>(ssum);
        const float inv = __builtin_amdgcn_rcpf(ssum);             // ssum in [1, nout]: v_rcp_f32, 1 ulp
#pragma unroll
        for (int i = 0; i < kQ; ++i) y[i] *= inv;
    } else if (a.out_kind == 2) {                            // tanh means, sigmoid variances (utils.py:74-77)
        const int half = nout / 2;
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int j = part + 4 * i;
            if (j < nout) {                                      // tanh = 1 - 2 / (e^2y + 1), sigmoid = 1 / (1 + e^-y): absolute 1e-7
                const float ex = __builtin_amdgcn_exp2f(y[i] * (j < half ? 2.8853900817779268f : -1.4426950408889634f));
                const float rc = __builtin_amdgcn_rcpf(ex + 1.0f);
                y[i] = j < half ? fmaf(-2.0f, rc, 1.0f) : rc;
            }
        }
    }
    const size_t row = (size_t)e * a.N + agent;
    if (a.out) {
#pragma unroll
        for (int i = 0; i < kQ; ++i) if (part + 4 * i < nout) a.out[row * nout + part + 4 * i] = y[i];
    }
    if (a.sample_kind != 0) {
        uint32_t rnd[4];
        philox4x32_10((uint32_t)agent, (uint32_t)(a.env_base + e), a.ctr2 + tval, a.ctr3 + epval, a.key0, a.key1, rnd);
        if (a.sample_kind == 1) {                            // categorical -> unit vector (utils.py:262-269, 304-309)
            const float u = (float)(rnd[0] >> 8) * (1.0f / 16777216.0f);
            float base = 0.0f;                               // cdf up to the previous group of 4 outputs
            int below = 0;                                   // outputs j with cdf_j <= u: the pick is the first j with u < cdf_j
#pragma unroll
            for (int i = 0; i < kQ; ++i) {
                if (4 * i < nout) {
                    const bool valid = part + 4 * i < nout;
                    float incl = valid ? y[i] : 0.0f;        // inclusive scan over the quad
                    const float n1 = quad_perm<kQuadUp1>(incl);
                    if (part >= 1) incl += n1;
                    const float n2 = quad_perm<kQuadUp2>(incl);
                    if (part >= 2) incl += n2;
                    const float cdf = base + incl;
                    if (valid && !(u < cdf)) ++below;
                    base = quad_perm<kQuadLast>(cdf);
                }
            }
            below += __builtin_amdgcn_update_dpp(0, below, kQuadXor1, 0xF, 0xF, true);
            below += __builtin_amdgcn_update_dpp(0, below, kQuadXor2, 0xF, 0xF, true);
            const int pick = min(below, nout - 1);
            if (part == 0) {
                if (a.act_idx) a.act_idx[row] = pick;
                if (a.act) {                                    // v_cos_f32 / v_sin_f32 take REVOLUTIONS: cos(2 pi pick / nout) directly
                    const float rev = (float)pick * __builtin_amdgcn_rcpf((float)nout);
                    *reinterpret_cast<float2 *>(a.act + row * 2) = make_float2(__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev));
                }
            }
        } else {                                             // Gaussian, Box-Muller (utils.py:110-117); nout = 4:
            const float var = quad_perm<kQuadXor2>(y[0]);    // lane d < 2 holds mu_d, lane d + 2 its variance
            if (part < 2 && a.act) {
                const uint32_t r0 = part == 0 ? rnd[0] : rnd[2], r1 = part == 0 ? rnd[1] : rnd[3];
                const float u1 = ((float)(r0 >> 8) + 1.0f) * (1.0f / 16777216.0f);            // (0, 1]
                const float u2 = (float)(r1 >> 8) * (1.0f / 16777216.0f);
                // Box-Muller on the hardware's log2 / sqrt / cos(2 pi x): v_log_f32, v_sqrt_f32, v_cos_f32 (input in revolutions)
                const float n01 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1)) * __builtin_amdgcn_cosf(u2);
                a.act[row * 2 + part] = fmaf(__builtin_amdgcn_sqrtf(var), n01, y[0]);
            }
        }
    }
}

// ---- shared by the split kernel (policy_split.hip) and the float16 row-tile kernel (policy_rowtile.hip): the parts of a lane's
//      operand, the f16x2 scheme (the schemes' contract is spelled out in policy_split.hip) and the relu + split of accumulators
template <int P> struct Parts { u32x4 p[P]; };     // the P parts of a lane's 8 k-slots (two 16-bit values per dword, low half first)

struct SchemeF16x2 {                                   // v = hi + lo to 2^-22 (float16 parts, subnormals honoured by the
    static constexpr int kParts = 2, kProducts = 3;    // matrix unit), products hi.hi, hi.lo, lo.hi; |v| < 65504
    // the packed weights of a layer carry a power-of-two factor (DroneMlpBf16.wscale) that keeps their low parts out of the
    // float16 subnormals; a layer's accumulators are multiplied by its inverse where they are split for the next layer
    static constexpr bool kScaled = true;
    __device__ static constexpr int w_part(int q) { constexpr int t[3] = {1, 0, 0}; return t[q]; }            // lo.hi hi.lo hi.hi
    __device__ static constexpr int b_part(int q) { constexpr int t[3] = {0, 1, 0}; return t[q]; }
    __device__ static constexpr int last_use(int p) { constexpr int t[2] = {2, 0}; return t[p]; }
    __device__ static constexpr int request_slot(int p) { constexpr int t[2] = {2, 4}; return t[p]; }
    __device__ static __forceinline__ f32x16 mfma(const u32x4 &w, const u32x4 &b, const f32x16 &acc)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    }
    template <bool RELU> __device__ static __forceinline__ void split_pair(float v0, float v1, unsigned (&d)[2])
    {
        if (RELU) { v0 = fmaxf(v0, 0.0f); v1 = fmaxf(v1, 0.0f); }
        typedef float f32x2v __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
        const f32x2v v = {v0, v1};                                             // round to nearest twice (v_cvt_pk_f16_f32):
        const f16x2v h = __builtin_convertvector(v, f16x2v);                   // |v - hi| <= 2^-11 |v|, v - hi exact in float32,
        const f16x2v l = __builtin_convertvector(v - __builtin_convertvector(h, f32x2v), f16x2v);   // |v - hi - lo| <= 2^-22 |v|
        d[0] = __builtin_bit_cast(unsigned, h); d[1] = __builtin_bit_cast(unsigned, l);
    }
};

// relu + split of half an accumulator tile (registers 8 HALF .. 8 HALF + 7 = the k slots of k-step HALF of the next
// layer's B operand), dealt out over the slots between a stage's matrix instructions: one call per slot.
template <class S, int HALF, int TILES>
struct SplitJob {
    static constexpr int kSlots = TILES * S::kProducts;
    static constexpr int kStride = (kSlots - 2) / 4 > 0 ? (kSlots - 2) / 4 : 1;    // pairs behind slots 1, 1 + stride, ...
    const f32x16 &src;
    Parts<S::kParts> &dst;
    const float mul;                                                               // S::kScaled: 1 / (the producing layer's weight factor)
    __device__ __forceinline__ SplitJob(const f32x16 &s, Parts<S::kParts> &d, float m = 1.0f) : src(s), dst(d), mul(m) {}
    template <int Q> __device__ __forceinline__ void pair()                        // values 2 Q, 2 Q + 1 -> dword Q
    {
        unsigned d[S::kParts];
        if constexpr (S::kScaled) S::template split_pair<true>(src[8 * HALF + 2 * Q] * mul, src[8 * HALF + 2 * Q + 1] * mul, d);
        else
        S::template split_pair<true>(src[8 * HALF + 2 * Q], src[8 * HALF + 2 * Q + 1], d);
#pragma unroll
        for (int p = 0; p < S::kParts; ++p) dst.p[p][Q] = d[p];
    }
    template <int SLOT> __device__ __forceinline__ void slot()
    {
        if constexpr (SLOT >= 1 && (SLOT - 1) % kStride == 0 && (SLOT - 1) / kStride < 4) pair<(SLOT - 1) / kStride>();
    }
    __device__ __forceinline__ void all() { pair<0>(); pair<1>(); pair<2>(); pair<3>(); }
};

// LDS reads the compiler must NOT see: hipcc orders every LDS read it can see behind ALL pending global_load_lds of
// the wave (s_waitcnt vmcnt(0)), which would drain the weight ring; the bytes read this way (biases, the x operand)
// were written before the first DMA was issued.
__device__ __forceinline__ uint32_t lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}
// The 32 biases of a chunk in accumulator layout (register 4 q + j of a lane = feature 8 q + 4 (lane >> 5) + j): the
// initial value of the chunk's accumulators.  `bias` = the chunk's 32 floats in LDS.
__device__ __forceinline__ f32x16 bias_tile(const float *bias, int lane)
{
    const uint32_t addr = lds_addr(bias + 4 * (lane >> 5));
    float4 q0, q1, q2, q3;
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:32\n\tds_read_b128 %2, %4 offset:64\n\t"
                 "ds_read_b128 %3, %4 offset:96\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3) : "v"(addr) : "memory");
    return f32x16{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
}

// One DMA request global -> LDS of the row-tile kernels, by name: every lane's 16 bytes at `src` (scalar base) + voff travel to
// the LDS address `dst` (scalar, through m0) + the lane's slot of the 1-KiB piece.
__device__ __forceinline__ void dma_to_lds(unsigned dst, unsigned voff, unsigned long long src)
{
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(dst), "v"(voff), "s"(src) : "memory", "m0");
}

// > 64 KiB of dynamic LDS must be opted into once per (kernel, device): a bit mask of device ordinals per kernel,
// guarded by a mutex (the library may be driven from several host threads / devices of one process)
int enable_big_lds(const void *kernel, unsigned long long (&opted)[4], std::mutex &mu, const char *what)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 255) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (opted[dev >> 6] >> (dev & 63) & 1ull) return DRONESIM_OK;
    hipFuncAttributes fa{};                                        // 160 KiB per CU, minus what the kernel holds statically
    hipError_t e = hipFuncGetAttributes(&fa, kernel);
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)fa.sharedSizeBytes);
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof(msg), "cannot enable 160 KiB of dynamic LDS for %s: %s", what, hipGetErrorString(e));
        return dronesim_fail(DRONESIM_ELAUNCH, msg);
    }
    opted[dev >> 6] |= 1ull << (dev & 63);
    return DRONESIM_OK;
}

FinishArgs make_finish(int N, int nout, int out_kind, int sample_kind, float *out, float *act, int32_t *act_idx,
                       uint64_t seed, uint64_t counter, int64_t env_base, const int32_t *t, const int32_t *episode)
{
    return FinishArgs{N, nout, out_kind, sample_kind, out, act, act_idx, (uint32_t)seed, (uint32_t)(seed >> 32),
                      (uint32_t)counter, (uint32_t)(counter >> 32), env_base, t, episode};
}

int check_mlp(int N, int d_in, int h1, int h2, int nout, int out_kind, int sample_kind, int E)
{
    if (N < 1 || d_in < 1 || d_in > 64 || h1 < 1 || h1 > 512 || h2 < 1 || h2 > 512 || nout < 1 || nout > kMaxOut)
        return dronesim_fail(DRONESIM_EUNSUPPORTED, "mlp forward: need d_in<=64, h1,h2<=512, nout<=32");
    if (out_kind < 0 || out_kind > 2 || sample_kind < 0 || sample_kind > 2)
        return dronesim_fail(DRONESIM_EINVAL, "mlp forward: bad out_kind / sample_kind");
    if (sample_kind == 2 && (out_kind != 2 || nout != 4))
        return dronesim_fail(DRONESIM_EINVAL, "Gaussian sampling needs out_kind 2 with nout = 4 (mu_x, mu_y, var_x, var_y)");
    if (E < 0) return dronesim_fail(DRONESIM_EINVAL, "E < 0");
    return DRONESIM_OK;
}

// THE launch sequence of every policy kernel: opt `Kernel` in for the big LDS on this device when `lds` exceeds `opt_in_above`
// (0 = always; 48 KiB for the bf16 and split kernels), launch, report.  One instantiation per kernel: the opt-in state lives
// here.  Every kernel takes (x, E, N, d_in, its argument block): the leading scalars are preloaded into SGPRs.
template <auto Kernel, class Args>
int launch_policy(const char *what, size_t opt_in_above, dim3 grid, unsigned threads, size_t lds, void *stream, const Args &a)
{
    if (lds > opt_in_above) {
        static std::mutex mu;
        static unsigned long long opted[4] = {0ull, 0ull, 0ull, 0ull};
        const int rc = enable_big_lds(reinterpret_cast<const void *>(Kernel), opted, mu, what);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(Kernel, grid, dim3(threads), lds, static_cast<hipStream_t>(stream), a.x, a.E, a.N, a.d_in, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}

}   // namespace
