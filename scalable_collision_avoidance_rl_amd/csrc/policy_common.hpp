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
// Which kernel serves which shape (h1, h2 <= 512 throughout; BatchedMLP: host class, policies.py; one file per kernel family).
// plan_policy_launch below makes the choice; tests/test_policy_plan_host.py restates this table and checks it against the plan:
//   precision  constructor switches           d_in    nout    entry point (include/dronesim.h)           kernel, variant
//   "f32"      (default), d_in <= 14          1..14   1..4    dronesim_mlp_forward, w2_layout = 2        mlp3_rt_kernel<VL3 = true>         policy_rowtile.hip
//                                             1..14   5..32     "                                        mlp3_rt_kernel<false>
//   "f32"      pack_w2="fragments", or the    1..6    1..16   dronesim_mlp_forward, w2_layout = 1        mlp3_kernel<PACKED, NARROW, NU = 3>  policy_f32.hip
//              default with d_in > 14         7..64   1..16     "                                        mlp3_kernel<true, true>
//                                             1..64   17..32    "                                        mlp3_kernel<true, false>
//   "f32"      pack_w2=False (the plain ABI)  1..64   1..16   dronesim_mlp_forward, w2_layout = 0        mlp3_kernel<false, true>
//                                             1..64   17..32    "                                        mlp3_kernel<false, false>
//   "f16x2"    (default)                      1..16   1..4    dronesim_mlp_forward_f16x2_rt              mlp3_rt16_kernel<VL3 = true>       policy_rowtile.hip
//                                             1..16   5..32     "                                        mlp3_rt16_kernel<false>
//   "f16x2"    split_kernel=True              1..16   1..32   dronesim_mlp_forward_f16x2                 mlp3_split_kernel<SchemeF16x2, 2>  policy_split.hip
//   "bf16x3"                                  1..16   1..32   dronesim_mlp_forward_bf16x3                mlp3_split_kernel<SchemeBf16x3, 2>
//   "bf16"                                    1..16   1..32   dronesim_mlp_forward_bf16                  mlp3_bf16_kernel<NC1 = ceil(h1 / 32)>  policy_bf16.hip
// The row-tile kernels are the product for every shape they take; mlp3_kernel stays as the only exact-f32 path for d_in > 14 and for the
// plain C ABI, the split f16x2 path because the C ABI has it and the tests drive it.  Everything here lives in an unnamed namespace --
// every translation unit gets its own copy, and the kernels keep the names they had in one file.
#pragma once
#include <stdio.h>
#include <mutex>
#include "common.hpp"
#include "dronesim.h"

// developer trace builds (kTrace, common.hpp) only: the stamps' buffer, set through dronesim_debug_set_policy_trace (policy_rowtile.hip)
extern __attribute__((visibility("hidden"))) long long *dronesim_policy_trace;
// what a policy call carries besides the network: the tail of every entry point's signature
struct PolicyCall {
    const float *x; float *out, *act; int32_t *act_idx; uint64_t seed, counter; int64_t env_base; const int32_t *t, *episode; int E; void *stream;
};
// w2_layout = 0 / 1 of dronesim_mlp_forward (policy_rowtile.hip) -> the LDS-staged kernel (policy_f32.hip); m is not NULL
extern "C" __attribute__((visibility("hidden"))) int dronesim_mlp_forward_staged(const DroneMlp *m, const PolicyCall *c);

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

int failf(int code, const char *fmt, const char *arg) { char msg[200]; snprintf(msg, sizeof(msg), fmt, arg); return dronesim_fail(code, msg); }

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

// ---- The LDS layout of every kernel family: one function per region, next to the family's constants.  The kernel carves its dynamic
//      LDS with them and the host's *_lds adds the same calls up -- no layout has a second definition.  Each function keeps the
//      arithmetic in the spelling the kernel had as a literal: hipcc schedules `b + w` differently from `b * (vl3 ? 5 : 1)`.
__host__ __device__ constexpr int chunks32(int h) { return (h + 31) / 32; }                  // 32-feature chunks of a layer
constexpr size_t larger(size_t a, size_t b) { return a > b ? a : b; }                         // the size of a region two tenants share
// b1 | b2 (zero padded to whole chunks: nb floats) | b3 (32): the bias table of the split and the bf16 kernel
__host__ __device__ constexpr int bias_table_floats(int nb) { return nb + 32; }

// mlp3_rt_kernel / mlp3_rt16_kernel (policy_rowtile.hip): kRtRows env rows per workgroup, a wave keeps kRtChunks output chunks per pass
constexpr int kRtChunks = 7, kRtRing = 4, kRtPad = kRtRing, kRtRows = 128, kRtTileFloats = 32 * 33;    // (the [32 rows][33] output tile of a wave)
__host__ __device__ constexpr int rt_passes(int nc2) { return (nc2 + kRtChunks - 1) / kRtChunks; }
__host__ __device__ constexpr int rt_per_pass(int nc2) { return (nc2 + rt_passes(nc2) - 1) / rt_passes(nc2); }
// blocks of one agent's stream that hold weights: per pass L1(c1) and L2(c1, c2 of the pass) for every c1, then (`l3`) L3(c2)
__host__ __device__ constexpr int rt_weight_blocks(int nc1, int nc2, bool l3) { return rt_passes(nc2) * nc1 + nc1 * nc2 + (l3 ? nc2 : 0); }
__host__ __device__ constexpr int rt_b2_bytes(int nc2) { return nc2 * 32 * 4; }                              // b2, zero padded to whole chunks
__host__ __device__ constexpr int rt_tables_bytes(int nc2, bool vl3) { return nc2 * 32 * 4 * (vl3 ? 5 : 1); }   // b2, then (VL3) W3[f][0..3]
__host__ __device__ constexpr int rt_ring_bytes() { return kRtRing * 4096; }                                 // per wave; later its output tile
constexpr size_t rt_lds(int nc2, bool vl3) { return (size_t)rt_tables_bytes(nc2, vl3) + 4 * (size_t)rt_ring_bytes(); }
constexpr int rt_blocks(int nc1, int nc2, int nout) { return rt_weight_blocks(nc1, nc2, nout > 4) + kRtPad; }

constexpr int kR16Depth = 4, kR16PadSupers = 3;      // super-stages (four 4-KiB blocks) of the workgroup's ring; empty ones behind a stream
__host__ __device__ constexpr int rt16_bias_floats(int nc) { return nc * 32; }                               // b1 * ws1, then b2 * ws2
__host__ __device__ constexpr int rt16_w3_rows(int nc2, bool vl3) { return vl3 ? nc2 * 32 : 0; }             // VL3: W3[f][0..3], 16 bytes a row
__host__ __device__ constexpr int rt16_ring_bytes() { return kR16Depth * 16384; }                            // later the four waves' output tiles
constexpr size_t rt16_lds(int nc1, int nc2, bool vl3) { return sizeof(float) * (size_t)(rt16_bias_floats(nc1) + rt16_bias_floats(nc2)) + sizeof(f32x4) * (size_t)rt16_w3_rows(nc2, vl3) + rt16_ring_bytes(); }
constexpr int rt16_blocks(int nc1, int nc2, int nout) { return ((rt_weight_blocks(nc1, nc2, nout > 4) + 3) / 4 + kR16PadSupers) * 4; }

// mlp3_kernel (policy_f32.hip): kRows env rows per workgroup (32-row tiles x 4 feature waves each)
constexpr int kRows = 32, kThreadsF = kRows * 8;
constexpr int kStW = 33, kStN = 36;      // floats per row of the per-wave staging tile (wide / narrow layer 3)
// LDS row stride (floats) of the h1 tile for the packed layer 2: whole 32-column chunks (the k padding is written as
// zeros by layer 1), a multiple of 4 (16-byte aligned rows) whose quotient is odd (ds_read_b128 phases conflict-free)
__host__ __device__ constexpr int packed_row_stride(int h1)
{
    const int w = ((h1 + 31) >> 5) * 32;
    return ((w >> 2) & 1) ? w : w + 4;
}
__host__ __device__ constexpr int f32_tile_floats(int ld) { return kRows * ld; }                            // the x tile (ld = d_in + 1), the h1 tile
__host__ __device__ constexpr int f32_stage_floats(int kst) { return 32 * kst; }                             // per wave; later the layer-3 partials
constexpr size_t f32_lds(int d_in, int h1, bool packed, bool narrow)
{
    return sizeof(float) * ((size_t)f32_tile_floats(d_in + 1) + f32_tile_floats(packed ? packed_row_stride(h1) : h1 + 1) + (kThreadsF / 64) * f32_stage_floats(narrow ? kStN : kStW));
}

// mlp3_split_kernel<S, TILES> (policy_split.hip): 32 TILES env rows per workgroup, `parts` = S::kParts pieces of 1 KiB per stage
constexpr int kStreamPadX = 8;             // zero stages behind every stream: the run-ahead requests of the deepest ring
__host__ __device__ constexpr int split_ring_depth(int tiles) { return tiles <= 2 ? 4 : 8; }   // stages of the per-wave weight ring in LDS
__host__ __device__ constexpr int split_parts(int scheme) { return scheme == 0 ? 3 : 2; }      // 0: SchemeBf16x3, 1: SchemeF16x2
__host__ __device__ constexpr int split_x_bytes(int tiles, int parts) { return tiles * parts * 1024; }      // x operand [tile][part][lane] x 16 B
__host__ __device__ constexpr int split_ring_bytes(int tiles, int parts) { return split_ring_depth(tiles) * parts * 1024; }   // per wave
__host__ __device__ constexpr int split_part_bytes(int tiles) { return 4 * 32 * tiles * 33 * 4; }            // partials [4 waves][rows][33]: share the rings' LDS
constexpr size_t split_lds(int nc1, int nc2, int tiles, int parts)
{
    return sizeof(float) * bias_table_floats((nc1 + nc2) * 32) + split_x_bytes(tiles, parts) + larger(split_part_bytes(tiles), 4 * split_ring_bytes(tiles, parts));
}
// stages per (agent, wave) stream: wave 0 owns the most chunks; + padding for the run-ahead requests
constexpr int split_stages(int nc1, int nc2) { return nc1 * (1 + 2 * ((nc2 + 3) / 4)) + 2 * ((nc2 + 3) / 4) + kStreamPadX; }

// mlp3_bf16_kernel<NC1> (policy_bf16.hip): 64 env rows (2 row tiles) per workgroup
constexpr int kRowsB = 64, kTiles = 2;
constexpr int kLdx = 24;                 // bf16 per row of the x tile
__host__ __device__ constexpr int bf16_x_elems() { return kRowsB * kLdx; }
__host__ __device__ constexpr int bf16_h1_stride(int nc1) { return nc1 * 32 + 8; }                           // bf16 per row of the h1 tile
__host__ __device__ constexpr int bf16_part_bytes() { return 4 * kRowsB * 33 * 4; }                         // partials [4 waves][64][33]: share the h1 tile's LDS
constexpr size_t bf16_lds(int nc1, int nc2)
{
    return sizeof(__bf16) * bf16_x_elems() + sizeof(float) * bias_table_floats((nc1 + nc2) * 32) + larger(sizeof(__bf16) * kRowsB * bf16_h1_stride(nc1), bf16_part_bytes());
}

// The layouts' promises over nc1, nc2 = 1..16 and every variant: a region that a 16-byte access or a DMA request lands in starts on a
// 16-byte boundary; the rings are whole power-of-two slot counts where `& (depth - 1)` picks the slot, and hold the output tiles
// that reuse them; regions that share LDS are sized by the larger tenant.
constexpr bool policy_lds_regions_ok()
{
    bool ok = (kRtRing & (kRtRing - 1)) == 0 && (kR16Depth & (kR16Depth - 1)) == 0 && rt_ring_bytes() % 4096 == 0 && rt16_ring_bytes() % 16384 == 0 &&
              sizeof(float) * kRtTileFloats <= (size_t)rt_ring_bytes() && 4 * sizeof(float) * kRtTileFloats <= (size_t)rt16_ring_bytes() &&
              (split_ring_depth(2) & (split_ring_depth(2) - 1)) == 0 && bf16_x_elems() * sizeof(__bf16) % 16 == 0 && kStN % 4 == 0;
    for (int nc1 = 1; nc1 <= 16; ++nc1) {
        ok = ok && sizeof(__bf16) * bf16_h1_stride(nc1) % 16 == 0 && (sizeof(__bf16) * bf16_h1_stride(nc1) / 16) % 2 == 1;
        for (int h1 = 32 * nc1 - 31; h1 <= 32 * nc1; ++h1)
            ok = ok && packed_row_stride(h1) % 4 == 0 && (packed_row_stride(h1) / 4) % 2 == 1 && packed_row_stride(h1) >= 32 * nc1;
        for (int nc2 = 1; nc2 <= 16; ++nc2) {
            for (int vl3 = 0; vl3 < 2; ++vl3) {
                ok = ok && rt_b2_bytes(nc2) % 16 == 0 && rt_tables_bytes(nc2, vl3) % 16 == 0 &&
                     rt_tables_bytes(nc2, vl3) == rt_b2_bytes(nc2) + (vl3 ? 16 * nc2 * 32 : 0) && rt_lds(nc2, vl3) <= 160 * 1024;
                ok = ok && sizeof(float) * (rt16_bias_floats(nc1) + rt16_bias_floats(nc2)) % 16 == 0 &&
                     rt16_lds(nc1, nc2, vl3) == sizeof(float) * 32 * (nc1 + nc2) + (vl3 ? 16 * 32 * nc2 : 0) + rt16_ring_bytes() && rt16_lds(nc1, nc2, vl3) <= 160 * 1024;
            }
            for (int scheme = 0; scheme < 2; ++scheme) {
                const int parts = split_parts(scheme), shared = (int)(split_lds(nc1, nc2, 2, parts) - sizeof(float) * bias_table_floats((nc1 + nc2) * 32) - split_x_bytes(2, parts));
                ok = ok && sizeof(float) * bias_table_floats((nc1 + nc2) * 32) % 16 == 0 && split_x_bytes(2, parts) % 16 == 0 && split_ring_bytes(2, parts) % 1024 == 0 &&
                     shared >= split_part_bytes(2) && shared >= 4 * split_ring_bytes(2, parts) && (shared == split_part_bytes(2) || shared == 4 * split_ring_bytes(2, parts)) &&
                     split_lds(nc1, nc2, 2, parts) <= 160 * 1024;
            }
            const int shared = (int)(bf16_lds(nc1, nc2) - sizeof(__bf16) * bf16_x_elems() - sizeof(float) * bias_table_floats((nc1 + nc2) * 32));
            ok = ok && shared >= bf16_part_bytes() && shared >= (int)sizeof(__bf16) * kRowsB * bf16_h1_stride(nc1) &&
                 (shared == bf16_part_bytes() || shared == (int)sizeof(__bf16) * kRowsB * bf16_h1_stride(nc1));
        }
    }
    return ok;
}
static_assert(policy_lds_regions_ok(), "an LDS region of a policy kernel is misaligned, a ring is no power-of-two slot count, or a shared region is not its larger tenant's size");

// ---- The plan of a policy launch, without a HIP call: the refusals an entry point makes after check_mlp (in its own order, with its own
//      texts), the instance that runs (`variant`: index into the family's table of launch_policy instantiations), its grid and LDS, and
//      the stream length and division magic the kernel is told.  `layout`: DroneMlp.w2_layout (kFamRt, kFamStaged) or the scheme
//      (kFamSplit: 0 bf16x3, 1 f16x2); `reserved`: DroneMlpBf16.reserved; `arrays`: the arrays the family reads are there;
//      `stream_addr`: the array that must be 16-byte aligned.  E = 0 (nothing to launch) comes back accepted with grid = 0.
enum PolicyFamily { kFamRt, kFamRt16, kFamStaged, kFamSplit, kFamBf16 };
constexpr size_t kPolicyLdsMax = 160 * 1024;               // LDS of a CU: the most a workgroup can ask for
// opt_in: the kernel must be opted in for this much dynamic LDS (enable_big_lds); stream: blocks / stages of one weight stream (0: the
// family reads arrays); rb_magic: xcd_work_item's ceil(2^32 / row blocks), or 0
struct PolicyPlan { int rc, variant; unsigned grid, threads; size_t lds; bool opt_in; int stream; unsigned rb_magic; };

inline PolicyPlan plan_policy_launch(int family, int N, int d_in, int h1, int h2, int nout, int layout, int reserved, bool arrays,
                                     uintptr_t stream_addr, int E)
{
    PolicyPlan p{};
    const int nc1 = chunks32(h1), nc2 = chunks32(h2);
    const bool aligned = (stream_addr & 15u) == 0, vl3 = nout <= 4;          // vl3: the row-tile kernels run layer 3 on the vector ALU
    const char *const scheme = layout == 0 ? "bf16x3" : "f16x2";
    auto refuse = [&p, scheme](int code, const char *fmt) { p.rc = failf(code, fmt, scheme); return p; };
    // env rows per workgroup; LDS above which the kernel is opted in (0: always -- the opt-in is remembered per kernel and device); rb_magic in use
    static constexpr struct { int rows; size_t opt_in_above; bool magic; } kFam[5] = {{kRtRows, 0, true}, {kRtRows, 0, true}, {kRows, 0, true},
                                                                                      {32 * 2, 48 * 1024, false}, {kRowsB, 48 * 1024, false}};
    static_assert(kThreadsF == 256, "every policy kernel runs four waves");
    p.threads = 256;
    switch (family) {
    case kFamRt:
        if (!arrays) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward: NULL weight array");
        if (d_in > 14) return refuse(DRONESIM_EUNSUPPORTED, "dronesim_mlp_forward: w2_layout = 2 needs d_in <= 14");
        if (!aligned) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward: the row-tile stream (w2_layout = 2) must be 16-byte aligned");
        if (E == 0) return p;
        p.variant = vl3; p.lds = rt_lds(nc2, vl3); p.stream = rt_blocks(nc1, nc2, nout);
        break;
    case kFamRt16:
        if (d_in > 16) return refuse(DRONESIM_EUNSUPPORTED, "dronesim_mlp_forward_f16x2_rt: d_in <= 16");
        if (!arrays) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward_f16x2_rt: NULL weight array");
        if (reserved != rt16_blocks(nc1, nc2, nout))
            return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward_f16x2_rt: DroneMlpBf16.reserved must hold dronesim_mlp_rt16_blocks(h1, h2, nout)");
        if (!aligned) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward_f16x2_rt: the stream must be 16-byte aligned");
        if (E == 0) return p;
        p.variant = vl3; p.lds = rt16_lds(nc1, nc2, vl3); p.stream = reserved;
        break;
    case kFamStaged: {
        if (!arrays) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward: NULL weight array");
        if (layout != 0 && layout != 1) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward: w2_layout must be 0, 1 or 2");
        if (layout == 1 && !aligned)                                         // read with 16-byte vector loads
            return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward: fragment-packed w2 (w2_layout = 1) must be 16-byte aligned");
        if (E == 0) return p;
        const bool packed = layout == 1, narrow = nout <= 16;               // narrow: layer 3 on the 16-column matrix instruction
        p.lds = f32_lds(d_in, h1, packed, narrow);
        // mlp3_kernel<PACKED, NARROW>: 0 .. 3 = 2 PACKED + NARROW; 4 = <true, true, NU = 3> (d_in <= 6: three k-steps of layer 1)
        p.variant = (packed && narrow && d_in <= 6) ? 4 : (packed ? 2 : 0) + (narrow ? 1 : 0);
        break;
    }
    case kFamSplit:
        if (d_in > 16) return refuse(DRONESIM_EUNSUPPORTED, "%s path: d_in <= 16");
        if (!arrays) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward_%s: NULL weight array");
        if (E == 0) return p;
        if (reserved != split_stages(nc1, nc2))
            return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward_%s: DroneMlpBf16.reserved must hold dronesim_mlp_bf16x3_stages(h1, h2), "
                                           "the stages per stream of w1p");
        p.variant = layout; p.lds = split_lds(nc1, nc2, 2, split_parts(layout)); p.stream = reserved;      // TILES = 2
        break;
    case kFamBf16:
        if (d_in > 16) return refuse(DRONESIM_EUNSUPPORTED, "bf16 path: d_in <= 16");
        if (!arrays) return refuse(DRONESIM_EINVAL, "dronesim_mlp_forward_bf16: NULL weight array");
        if (E == 0) return p;
        p.lds = bf16_lds(nc1, nc2);
        p.variant = nc1 - 1;                                                 // mlp3_bf16_kernel<NC1>: the h1 tile's register residency is compile-time
        break;
    }
    // (mlp3_kernel's and bf16's tiles grow with h1; check_mlp's caps keep them at 92800 and 73856 bytes, the other families' are asserted above)
    if (p.lds > kPolicyLdsMax) return refuse(DRONESIM_EUNSUPPORTED, "hidden layer too wide for the LDS tile");
    const unsigned rb = (unsigned)((E + kFam[family].rows - 1) / kFam[family].rows);
    p.grid = rb * N;
    p.rb_magic = kFam[family].magic ? div_magic(p.grid, rb) : 0u;
    p.opt_in = p.lds > kFam[family].opt_in_above;
    return p;
}

// THE launch sequence of every policy kernel: opt `Kernel` in for the big LDS on this device where the plan says so, launch,
// report.  One instantiation per kernel: the opt-in state lives here.  Every kernel takes (x, E, N, d_in, its argument block): the
// leading scalars are preloaded into SGPRs.  A family's variants are one table of these, indexed by PolicyPlan.variant.
template <auto Kernel, class Args>
int launch_policy(const char *what, const PolicyPlan &p, void *stream, const Args &a)
{
    if (p.opt_in) {
        static std::mutex mu;
        static unsigned long long opted[4] = {0ull, 0ull, 0ull, 0ull};
        const int rc = enable_big_lds(reinterpret_cast<const void *>(Kernel), opted, mu, what);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(Kernel, dim3(p.grid), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a.x, a.E, a.N, a.d_in, a);
    return dronesim_launched();
}

// The front door of the five entry points: the NULL m / x check, check_mlp and the plan's refusals, E = 0, the fields every argument
// block has, make_finish and the trace pointer; `fill(a, plan)` then sets what is the family's own, and the plan's variant of the
// family's table is launched.  `entry`: the entry point's name for the NULL message; `aligned16`: the plan's `stream_addr`.
template <class A> auto set_trace(A &a, int) -> decltype((void)a.trace) { a.trace = kTrace ? dronesim_policy_trace : nullptr; }
template <class A> void set_trace(A &, long) {}                                // (mlp3_rt_kernel's block carries none)
template <class Args> using PolicyLaunch = int (*)(const char *, const PolicyPlan &, void *, const Args &);

template <class Args, size_t V, class M, class Fill>
int policy_forward(const char *entry, const char *kernel, int family, const PolicyLaunch<Args> (&variants)[V], const M *m, const PolicyCall &c,
                   int layout, int reserved, bool arrays, const void *aligned16, Fill fill)
{
    if (!m || !c.x) return failf(DRONESIM_EINVAL, "%s: NULL argument", entry);
    const int rc = check_mlp(m->N, m->d_in, m->h1, m->h2, m->nout, m->out_kind, m->sample_kind, c.E);
    if (rc) return rc;
    const PolicyPlan p = plan_policy_launch(family, m->N, m->d_in, m->h1, m->h2, m->nout, layout, reserved, arrays, reinterpret_cast<uintptr_t>(aligned16), c.E);
    if (p.rc || c.E == 0) return p.rc;
    Args a{};
    a.E = c.E; a.N = m->N; a.d_in = m->d_in; a.h1 = m->h1; a.h2 = m->h2; a.x = c.x;
    a.fin = make_finish(m->N, m->nout, m->out_kind, m->sample_kind, c.out, c.act, c.act_idx, c.seed, c.counter, c.env_base, c.t, c.episode);
    set_trace(a, 0);
    fill(a, p);
    return variants[p.variant](kernel, p, c.stream, a);
}

}   // namespace
