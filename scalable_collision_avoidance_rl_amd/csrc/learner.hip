// Per-agent learner step of the batched MLPs (SAC_agents.py:280-357, SA2CAgents.train_NN): gradients of the critic / actor
// losses over a window of rows, then clip_grad_norm_ + Adam per agent (include/dronesim.h: dronesim_mlp_grad, dronesim_adam_step).
//
// Exact float32.  Rows are processed in chunks of Rc (a multiple of 64); per chunk and for all N agents at once (one batch
// index per agent) the chain is
//   H1 = relu(X W1 + b1), H2 = relu(H1 W2 + b2), O = H2 W3 + b3          forward, on the matrix cores
//   dO, per-row loss                                                     head kernel (three kinds)
//   dW3 += H2^T dO (+ db3);  dH2 = (dO W3^T) . [H2 > 0]   (in place of H2)
//   dW2 += H1^T dH2 (+ db2); dH1 = (dH2 W2^T) . [H1 > 0]  (in place of H1)
//   dW1 += X^T dH1 (+ db1)
//   loss += sum of the chunk's per-row losses
// Every GEMM is one launch of ONE tiled kernel on v_mfma_f32_32x32x2f32 (a k-ordered fmaf chain per output element).  A
// weight-gradient element is owned by one lane that adds the chunk's partial sum into the gradient buffer, chunks in order:
// no float atomics, bit-identical run to run.  The window's first chunk WRITES the gradient and loss buffers instead of
// adding to a cleared buffer: the entry point enqueues kernels only (no memset node), which keeps a captured graph's
// replays identical to eager calls.  Bias gradients are one more output row of the same GEMM, fed by a virtual
// row of ones.
//
// PPO (SAC_agents.py:410-573, SPPOAgents.train; include/dronesim.h: dronesim_mlp_logp, dronesim_mlp_grad_ppo) is the same chain
// around another head: ppo_head_kernel computes log pi(a | x) with the expressions of the actor kinds above and either stops there
// (the forward-only pass: the old policy's log-probabilities) or forms the ratio to a stored logp_old, the clipped surrogate's
// per-row loss and dLoss/dO, plus three per-row diagnostics that ppo_stats_kernel reduces per agent in a fixed order.
//
// Two opt-in parts of the learners (include/dronesim.h): the entropy bonus -- head_ent_kernel / ppo_head_ent_kernel, the two actor
// heads with the policy's entropy in the loss, kernels of their own behind the same chain (dronesim_mlp_grad_ent,
// dronesim_mlp_grad_ppo_ent) -- and dronesim_standardize, the per-agent standardisation of a window's advantages (float64 sums,
// two launches, fixed order).
//
// Two guards of the PPO learner's repeated steps on one window (include/dronesim.h), through the SAME chain and kernels: every
// kernel of the chain takes a nullable per-agent gate `active` (int32 [N], device memory; NULL from the older entry points) --
// gemm_kernel's batch index is the agent, so a workgroup of a gated agent returns at entry, before any barrier, uniformly; the
// heads skip its rows and the per-agent sums write NaN for it.  dronesim_mlp_grad_ppo_gated is the PPO-with-entropy chain with
// that gate and one more per-row plane, the non-negative KL estimate k = expm1(dl) - dl (kl_sum_kernel: float64 partial sums,
// fixed order); dronesim_kl_gate decides the stop on the device; dronesim_adam_step_gated obeys it.  dronesim_mlp_grad_vclip is
// the critic chain with PPO's clipped value loss in head_kernel (one more per-row plane of zero-gradient flags).
#include "common.hpp"
#include "../../include/dronesim.h"

#include <math.h>
#include <stdio.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBM = 64, kBN = 64, kBK = 16, kThreads = 256;

enum Epilogue : int {
    kReluBias = 0,      // C = relu(acc + bias[n])
    kBias = 1,          // C = acc + bias[n]
    kMask = 2,          // C = C > 0 ? acc : 0           (C holds the forward activation it replaces)
    kAccumulate = 3,    // C += acc (C = acc when `first`); the row `ones_row` goes to Cb[n] (bias gradient)
};

struct GemmArgs {
    const float *A; long long sAm, sAk, bA;      // A(m, k) = A[b * bA + m * sAm + k * sAk]
    const float *B; long long sBk, sBn, bB;      // B(k, n) = B[b * bB + k * sBk + n * sBn]
    float *C; long long ldc, bC;                 // C(m, n) = C[b * bC + m * ldc + n]
    const float *bias; long long bBias;          // kReluBias / kBias: bias[b * bBias + n]
    float *Cb; long long bCb;                    // kAccumulate: the ones row's outputs
    int M, N, K;
    int ones_row;                                // -1: none; else A(ones_row, k) = 1 for k < K
    int mode;
    int half_m, half_n;                          // kAccumulate, > 0: outputs with (m < half_m) != (n < half_n) are 0
    int first;                                   // kAccumulate: the window's first chunk WRITES (no separate zeroing)
    const int32_t *active;                       // NULL, or [batch] in device memory: a batch index with active[b] == 0 is skipped
};

// 64 x 64 output tile per workgroup, four waves of one 32 x 32 accumulator each; the tile's k-slices go through LDS in k-major
// order, so a lane reads A(m = l & 31, k = l >> 5) and B(k = l >> 5, n = l & 31) -- the operand maps of the 32x32x2 form.
__global__ __launch_bounds__(kThreads) void gemm_kernel(GemmArgs g)
{
    __shared__ float As[kBK][kBM + 4];
    __shared__ float Bs[kBK][kBN + 4];
    const int b = blockIdx.z;
    if (g.active && g.active[b] == 0) return;    // the whole workgroup, before any barrier: a gated agent costs no matrix work
    const float *A = g.A + (long long)b * g.bA;
    const float *B = g.B + (long long)b * g.bB;
    const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * kBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const bool a_m_fast = g.sAm == 1, b_n_fast = g.sBn == 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int k0 = 0; k0 < g.K; k0 += kBK) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // the thread walks the operand's contiguous axis (coalesced loads)
            const int m = a_m_fast ? (tid & 63) : (tid >> 4) + 16 * j;
            const int k = a_m_fast ? (tid >> 6) + 4 * j : (tid & 15);
            const int gm = m0 + m, gk = k0 + k;
            float v = 0.f;
            if (gk < g.K && gm < g.M)
                v = gm == g.ones_row ? 1.f : A[(long long)gm * g.sAm + (long long)gk * g.sAk];
            As[k][m] = v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = b_n_fast ? (tid & 63) : (tid >> 4) + 16 * j;
            const int k = b_n_fast ? (tid >> 6) + 4 * j : (tid & 15);
            const int gn = n0 + n, gk = k0 + k;
            float v = 0.f;
            if (gk < g.K && gn < g.N) v = B[(long long)gk * g.sBk + (long long)gn * g.sBn];
            Bs[k][n] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 2) {
            const float a = As[kk + (lane >> 5)][wm + (lane & 31)];
            const float bv = Bs[kk + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int n = n0 + wn + (lane & 31);
    if (n >= g.N) return;
    float *C = g.C + (long long)b * g.bC;
    const float bias = (g.mode == kReluBias || g.mode == kBias) ? g.bias[(long long)b * g.bBias + n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.M) continue;
        const float v = acc[r];
        float *c = C + (long long)m * g.ldc + n;
        if (g.mode == kReluBias) {
            *c = fmaxf(v + bias, 0.f);
        } else if (g.mode == kBias) {
            *c = v + bias;
        } else if (g.mode == kMask) {
            *c = *c > 0.f ? v : 0.f;
        } else if (m == g.ones_row) {
            float *cb = g.Cb + (long long)b * g.bCb + n;
            *cb = g.first ? v : *cb + v;
        } else if (g.half_m > 0 && ((m < g.half_m) != (n < g.half_n))) {
            if (g.first) *c = 0.f;
        } else {
            *c = g.first ? v : *c + v;
        }
    }
}

// The loss head of one (row, agent): per-row loss (times `scale`) into L, dLoss/dO (pre-activation outputs) in place of O.
//   kind 0 (critic):       l = (o - G)^2
//   kind 1 (softmax):      l = -w log softmax(o)[a],  a = the action list's entry nearest to the stored unit action
//   kind 2 (Gaussian):     l = -w sum_d [-0.5 log(2 pi var_d) - (a_d - mu_d)^2 / (2 var_d)],  mu = tanh, var = sigmoid
// kind 0 with `v_old` set (dronesim_mlp_grad_vclip) is PPO's clipped value loss: Vc = V clamped to v_old +- vf_clip,
//   l = max((V - G)^2, (Vc - G)^2); where the clipped term is the STRICT maximum V is clamped and dl/dV = 0, and the row's flag
//   (0 / 1) goes to the plane Cp [N][Rc].  An unclamped row has Vc = V itself (not v_old + (V - v_old), which rounds): it forms
//   the plain head's expressions and gives its bits.
__global__ __launch_bounds__(kThreads) void head_kernel(float *O, float *L, long long Rc, int rc, long long r0, int N, int nout,
                                                        int kind, float scale, const float *target, const float *act,
                                                        const float *weight, const float *v_old, float vf_clip, float *Cp)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float loss;
    if (kind == 0) {
        const float d = o[0] - target[src];
        bool zero = false;
        float dc = d;
        if (v_old) {
            const float vo = v_old[src], dv = o[0] - vo;
            const float vc = dv > vf_clip ? vo + vf_clip : (dv < -vf_clip ? vo - vf_clip : o[0]);
            dc = vc - target[src];
            zero = dc * dc > d * d;
            Cp[(long long)i * Rc + m] = zero ? 1.f : 0.f;
        }
        if (zero) {
            loss = scale * dc * dc;
            o[0] = 0.f;
        } else {
            loss = scale * d * d;
            o[0] = 2.f * scale * d;
        }
    } else if (kind == 1) {
        const float ax = act[2 * src], ay = act[2 * src + 1];
        int a = (int)rintf(atan2f(ay, ax) * (float)nout * 0.15915494309189535f);
        a = ((a % nout) + nout) % nout;
        float mx = o[0];
        for (int j = 1; j < nout; ++j) mx = fmaxf(mx, o[j]);
        float s = 0.f;
        for (int j = 0; j < nout; ++j) s += expf(o[j] - mx);
        const float lse = mx + logf(s);
        const float c = -scale * weight[src];
        loss = c * (o[a] - lse);
        for (int j = 0; j < nout; ++j) {
            const float p = expf(o[j] - lse);
            o[j] = c * ((j == a ? 1.f : 0.f) - p);
        }
    } else {
        const float c = -scale * weight[src];
        float lp = 0.f;
        for (int d = 0; d < 2; ++d) {
            const float mu = tanhf(o[d]);
            const float e = expf(-o[2 + d]);
            const float var = 1.f / (1.f + e), omv = e / (1.f + e);
            const float diff = act[2 * src + d] - mu;
            lp += -0.5f * logf(6.283185307179586f * var) - diff * diff / (2.f * var);
            o[d] = c * (diff / var) * (1.f - mu * mu);
            o[2 + d] = c * (-0.5f + diff * diff / (2.f * var)) * omv;
        }
        loss = c * lp;
    }
    L[(long long)i * Rc + m] = loss;
}

// loss[i] (+)= the chunk's per-row losses of agent i, in a fixed order (strided partial sums, then a fixed tree); the first
// chunk writes.  A gated agent (active[i] == 0, uniform over the workgroup) sums nothing: its loss is NaN.
__global__ __launch_bounds__(kThreads) void loss_sum_kernel(const float *L, long long Rc, int rc, int first, float *loss,
                                                            const int32_t *active)
{
    __shared__ float part[kThreads];
    const int i = blockIdx.x;
    if (active && active[i] == 0) {
        if (threadIdx.x == 0) loss[i] = __builtin_nanf("");
        return;
    }
    float s = 0.f;
    for (int m = threadIdx.x; m < rc; m += kThreads) s += L[(long long)i * Rc + m];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[i] = first ? part[0] : loss[i] + part[0];
}

// The PPO head of one (row, agent) of an actor (kinds 1 and 2; SAC_agents.py:494, :541-549): logp = log pi_i(a | x) with the
// expressions of head_kernel's kinds; with `logp_out` set that is all it writes (the forward-only pass).  Otherwise
//   r = exp(logp - logp_old),  l = -min(r Adv, clamp(r, lo, hi) Adv)  (times `scale`) into L,
//   dLoss/dO = -scale Adv r dlogp/dO in place of O -- 0 where the clipped branch is the strict minimum (Adv > 0 and r > hi, or
//   Adv < 0 and r < lo) --, and the row's diagnostics into S: [0] clipped (0 / 1), [1] logp_old - logp, [2] r, each [N][Rc].
// Both modes are ONE kernel and share the instructions up to `lp`: on the same O they give the same bits, so r is exactly 1
// until the actor moves.
__global__ __launch_bounds__(kThreads) void ppo_head_kernel(float *O, float *L, float *S, long long Rc, int rc, long long r0, int N,
                                                            int nout, int kind, float scale, const float *act,
                                                            const float *logp_old, const float *adv, float lo, float hi,
                                                            float *logp_out)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float lp, lse = 0.f;
    int a = 0;
    float mu[2], var[2], omv[2], diff[2];
    if (kind == 1) {
        const float ax = act[2 * src], ay = act[2 * src + 1];
        a = (int)rintf(atan2f(ay, ax) * (float)nout * 0.15915494309189535f);
        a = ((a % nout) + nout) % nout;
        float mx = o[0];
        for (int j = 1; j < nout; ++j) mx = fmaxf(mx, o[j]);
        float s = 0.f;
        for (int j = 0; j < nout; ++j) s += expf(o[j] - mx);
        lse = mx + logf(s);
        lp = o[a] - lse;
    } else {
        lp = 0.f;
        for (int d = 0; d < 2; ++d) {
            mu[d] = tanhf(o[d]);
            const float e = expf(-o[2 + d]);
            var[d] = 1.f / (1.f + e);
            omv[d] = e / (1.f + e);
            diff[d] = act[2 * src + d] - mu[d];
            lp += -0.5f * logf(6.283185307179586f * var[d]) - diff[d] * diff[d] / (2.f * var[d]);
        }
    }
    if (logp_out) {
        logp_out[src] = lp;
        return;
    }
    const float dl = lp - logp_old[src];
    const float r = expf(dl);
    const float A = adv[src];
    const bool clipped = (A > 0.f && r > hi) || (A < 0.f && r < lo);
    const float c = clipped ? 0.f : -scale * A * r;
    if (kind == 1) {
        for (int j = 0; j < nout; ++j) {
            const float p = expf(o[j] - lse);
            o[j] = c * ((j == a ? 1.f : 0.f) - p);
        }
    } else {
        for (int d = 0; d < 2; ++d) {
            o[d] = c * (diff[d] / var[d]) * (1.f - mu[d] * mu[d]);
            o[2 + d] = c * (-0.5f + diff[d] * diff[d] / (2.f * var[d])) * omv[d];
        }
    }
    const long long dst = (long long)i * Rc + m, plane = (long long)N * Rc;
    L[dst] = -scale * fminf(r * A, fminf(fmaxf(r, lo), hi) * A);
    S[dst] = clipped ? 1.f : 0.f;
    S[plane + dst] = -dl;
    S[2 * plane + dst] = r;
}

// stats [4][N] of agent i over the chunks, in loss_sum_kernel's fixed order (strided partials, then a fixed tree): the clipped
// rows' count, the sum of logp_old - logp, min r, max r; the first chunk writes, the last divides the two sums by R
// (a gated agent: four NaN)
__global__ __launch_bounds__(kThreads) void ppo_stats_kernel(const float *S, long long Rc, int rc, int N, int first, int last,
                                                             float rows, float *stats, const int32_t *active)
{
    __shared__ float part[4][kThreads];
    const int i = blockIdx.x;
    if (active && active[i] == 0) {
        if (threadIdx.x < 4) stats[threadIdx.x * N + i] = __builtin_nanf("");
        return;
    }
    const long long plane = (long long)N * Rc;
    const float inf = __builtin_inff();
    float nc = 0.f, kl = 0.f, lo = inf, hi = -inf;
    for (int m = threadIdx.x; m < rc; m += kThreads) {
        const long long at = (long long)i * Rc + m;
        nc += S[at];
        kl += S[plane + at];
        const float r = S[2 * plane + at];
        lo = fminf(lo, r);
        hi = fmaxf(hi, r);
    }
    part[0][threadIdx.x] = nc; part[1][threadIdx.x] = kl; part[2][threadIdx.x] = lo; part[3][threadIdx.x] = hi;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            part[0][threadIdx.x] += part[0][threadIdx.x + w];
            part[1][threadIdx.x] += part[1][threadIdx.x + w];
            part[2][threadIdx.x] = fminf(part[2][threadIdx.x], part[2][threadIdx.x + w]);
            part[3][threadIdx.x] = fmaxf(part[3][threadIdx.x], part[3][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        nc = first ? part[0][0] : stats[i] + part[0][0];
        kl = first ? part[1][0] : stats[N + i] + part[1][0];
        stats[i] = last ? nc / rows : nc;
        stats[N + i] = last ? kl / rows : kl;
        stats[2 * N + i] = first ? part[2][0] : fminf(stats[2 * N + i], part[2][0]);
        stats[3 * N + i] = first ? part[3][0] : fmaxf(stats[3 * N + i], part[3][0]);
    }
}

// The entropy bonus (include/dronesim.h: dronesim_mlp_grad_ent, dronesim_mlp_grad_ppo_ent): the two actor heads above with the
// policy's entropy H of the row in the loss, L_i - es sum_r H_i(x_r).  Kernels of their own -- the heads above keep their code
// -- that form every value the siblings form with the same expressions and ADD the entropy's part, so with es = 0 they give
// the siblings' values (an exact zero is added) and the log-probability is the one dronesim_mlp_logp computes.
//   softmax:   lq_j = o_j - lse,  p_j = exp(lq_j),  H = -sum_j p_j lq_j;    dO_j += es p_j (lq_j + H)
//              (from lq, never log p: a logit 120 below the maximum has p = 0 in float32 and 0 log 0 is NaN)
//   Gaussian:  H = sum_d 0.5 log(2 pi e var_d);                             dO_{2+d} += -0.5 es (1 - var_d)  (the head's omv)
// The per-row loss is the whole objective (the sibling's l - es H); H itself goes to the plane E [N][Rc].
__global__ __launch_bounds__(kThreads) void head_ent_kernel(float *O, float *L, float *E, long long Rc, int rc, long long r0, int N,
                                                            int nout, int kind, float scale, float es, const float *act,
                                                            const float *weight)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float loss, H = 0.f;
    if (kind == 1) {
        const float ax = act[2 * src], ay = act[2 * src + 1];
        int a = (int)rintf(atan2f(ay, ax) * (float)nout * 0.15915494309189535f);
        a = ((a % nout) + nout) % nout;
        float mx = o[0];
        for (int j = 1; j < nout; ++j) mx = fmaxf(mx, o[j]);
        float s = 0.f;
        for (int j = 0; j < nout; ++j) s += expf(o[j] - mx);
        const float lse = mx + logf(s);
        const float c = -scale * weight[src];
        loss = c * (o[a] - lse);
        for (int j = 0; j < nout; ++j) {
            const float lq = o[j] - lse;
            H -= expf(lq) * lq;
        }
        for (int j = 0; j < nout; ++j) {
            const float p = expf(o[j] - lse);
            const float g = c * ((j == a ? 1.f : 0.f) - p);
            o[j] = g + es * (p * ((o[j] - lse) + H));
        }
    } else {
        const float c = -scale * weight[src];
        float lp = 0.f;
        for (int d = 0; d < 2; ++d) {
            const float mu = tanhf(o[d]);
            const float e = expf(-o[2 + d]);
            const float var = 1.f / (1.f + e), omv = e / (1.f + e);
            const float diff = act[2 * src + d] - mu;
            lp += -0.5f * logf(6.283185307179586f * var) - diff * diff / (2.f * var);
            H += 0.5f * logf(17.079468445347132f * var);
            o[d] = c * (diff / var) * (1.f - mu * mu);
            const float g = c * (-0.5f + diff * diff / (2.f * var)) * omv;
            o[2 + d] = g - 0.5f * es * omv;
        }
        loss = c * lp;
    }
    L[(long long)i * Rc + m] = loss - es * H;
    E[(long long)i * Rc + m] = H;
}

// ppo_head_kernel's gradient mode with the entropy (no forward-only mode: dronesim_mlp_logp stays the sibling's).  The entropy's
// gradient is added on EVERY row, the rows on the clipped branch included (there the surrogate's part is 0).
// The gated form (dronesim_mlp_grad_ppo_gated) passes `active` and the plane Kp [N][Rc]: the rows of an agent with
// active[i] == 0 are skipped, and every other row also stores k = expm1(dl) - dl >= 0, Schulman's (r - 1) - log r formed
// without the cancellation of r - 1 (exactly 0 at dl = 0).
__global__ __launch_bounds__(kThreads) void ppo_head_ent_kernel(float *O, float *L, float *S, float *E, long long Rc, int rc,
                                                                long long r0, int N, int nout, int kind, float scale, float es,
                                                                const float *act, const float *logp_old, const float *adv,
                                                                float lo, float hi, const int32_t *active, float *Kp)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    if (active && active[i] == 0) return;
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float lp, lse = 0.f, H = 0.f;
    int a = 0;
    float mu[2], var[2], omv[2], diff[2];
    if (kind == 1) {
        const float ax = act[2 * src], ay = act[2 * src + 1];
        a = (int)rintf(atan2f(ay, ax) * (float)nout * 0.15915494309189535f);
        a = ((a % nout) + nout) % nout;
        float mx = o[0];
        for (int j = 1; j < nout; ++j) mx = fmaxf(mx, o[j]);
        float s = 0.f;
        for (int j = 0; j < nout; ++j) s += expf(o[j] - mx);
        lse = mx + logf(s);
        lp = o[a] - lse;
        for (int j = 0; j < nout; ++j) {
            const float lq = o[j] - lse;
            H -= expf(lq) * lq;
        }
    } else {
        lp = 0.f;
        for (int d = 0; d < 2; ++d) {
            mu[d] = tanhf(o[d]);
            const float e = expf(-o[2 + d]);
            var[d] = 1.f / (1.f + e);
            omv[d] = e / (1.f + e);
            diff[d] = act[2 * src + d] - mu[d];
            lp += -0.5f * logf(6.283185307179586f * var[d]) - diff[d] * diff[d] / (2.f * var[d]);
        }
        for (int d = 0; d < 2; ++d) H += 0.5f * logf(17.079468445347132f * var[d]);
    }
    const float dl = lp - logp_old[src];
    const float r = expf(dl);
    const float A = adv[src];
    const bool clipped = (A > 0.f && r > hi) || (A < 0.f && r < lo);
    const float c = clipped ? 0.f : -scale * A * r;
    if (kind == 1) {
        for (int j = 0; j < nout; ++j) {
            const float p = expf(o[j] - lse);
            const float g = c * ((j == a ? 1.f : 0.f) - p);
            o[j] = g + es * (p * ((o[j] - lse) + H));
        }
    } else {
        for (int d = 0; d < 2; ++d) {
            o[d] = c * (diff[d] / var[d]) * (1.f - mu[d] * mu[d]);
            const float g = c * (-0.5f + diff[d] * diff[d] / (2.f * var[d])) * omv[d];
            o[2 + d] = g - 0.5f * es * omv[d];
        }
    }
    const long long dst = (long long)i * Rc + m, plane = (long long)N * Rc;
    const float l = -scale * fminf(r * A, fminf(fmaxf(r, lo), hi) * A);
    L[dst] = l - es * H;
    S[dst] = clipped ? 1.f : 0.f;
    S[plane + dst] = -dl;
    S[2 * plane + dst] = r;
    E[dst] = H;
    if (Kp) Kp[dst] = fmaxf(expm1f(dl) - dl, 0.f);
}

// entropy[i] = the mean row entropy of agent i over the chunks, in loss_sum_kernel's fixed order (strided partials, then a fixed
// tree); the first chunk writes, the last divides by R
// (a gated agent: NaN; dronesim_mlp_grad_vclip reduces its plane of zero-gradient flags with it)
__global__ __launch_bounds__(kThreads) void entropy_sum_kernel(const float *E, long long Rc, int rc, int first, int last, float rows,
                                                               float *entropy, const int32_t *active)
{
    __shared__ float part[kThreads];
    const int i = blockIdx.x;
    if (active && active[i] == 0) {
        if (threadIdx.x == 0) entropy[i] = __builtin_nanf("");
        return;
    }
    float s = 0.f;
    for (int m = threadIdx.x; m < rc; m += kThreads) s += E[(long long)i * Rc + m];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        s = first ? part[0] : entropy[i] + part[0];
        entropy[i] = last ? s / rows : s;
    }
}

// kl[i] = the mean of the head's k plane of agent i over the chunks, in the same fixed order with float64 partial sums: the
// running sum stays in acc [N] (float64, workspace) between the chunks, the last chunk writes the float32 mean.  A gated
// agent: NaN.
__global__ __launch_bounds__(kThreads) void kl_sum_kernel(const float *Kp, long long Rc, int rc, int first, int last, double rows,
                                                          double *acc, float *kl, const int32_t *active)
{
    __shared__ double part[kThreads];
    const int i = blockIdx.x;
    if (active && active[i] == 0) {
        if (threadIdx.x == 0) kl[i] = __builtin_nanf("");
        return;
    }
    double s = 0.0;
    for (int m = threadIdx.x; m < rc; m += kThreads) s += (double)Kp[(long long)i * Rc + m];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        s = first ? part[0] : acc[i] + part[0];
        acc[i] = s;
        if (last) kl[i] = (float)(s / rows);
    }
}

// dronesim_kl_gate: one thread per agent.  reset: every agent active, no step taken.  Otherwise an active agent whose estimate
// is not <= target_kl (NaN included) stops, and stays stopped; an agent that is still active has one more step counted.
__global__ __launch_bounds__(kThreads) void kl_gate_kernel(const float *kl, float target_kl, int32_t *active, int32_t *taken, int N,
                                                           int reset)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    if (reset) {
        active[i] = 1;
        taken[i] = 0;
        return;
    }
    int a = active[i];
    if (a && !(kl[i] <= target_kl)) active[i] = a = 0;
    if (a) taken[i] = taken[i] + 1;
}

struct Tensors {
    long long size[6];      // per agent: w1, b1, w2, b2, w3, b3
    long long off[6];       // of the [N, ...] tensor in the flat buffer
    long long per_agent;
};

Tensors tensors_of(const DroneMlp *m)
{
    Tensors t;
    const long long s[6] = {(long long)m->d_in * m->h1, m->h1, (long long)m->h1 * m->h2, m->h2, (long long)m->h2 * m->nout, m->nout};
    long long off = 0, pa = 0;
    for (int j = 0; j < 6; ++j) { t.size[j] = s[j]; t.off[j] = off; off += s[j] * m->N; pa += s[j]; }
    t.per_agent = pa;
    return t;
}

struct Params { float *p[6]; };

// the pre-clip gradient norm of agent i over its six tensors (double partial sums, fixed order); advances the step counter
// (dronesim_adam_step_gated: an agent with active[i] == 0 keeps its counter and reports NaN)
__global__ __launch_bounds__(kThreads) void grad_norm_kernel(const float *grad, Tensors t, int32_t *step, float *grad_norm,
                                                             const int32_t *active)
{
    __shared__ double part[kThreads];
    const int i = blockIdx.x;
    if (active && active[i] == 0) {
        if (threadIdx.x == 0) grad_norm[i] = __builtin_nanf("");
        return;
    }
    double s = 0.0;
    for (int j = 0; j < 6; ++j) {
        const float *g = grad + t.off[j] + (long long)i * t.size[j];
        for (long long e = threadIdx.x; e < t.size[j]; e += kThreads) s += (double)g[e] * (double)g[e];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        grad_norm[i] = (float)sqrt(part[0]);
        step[i] = step[i] + 1;
    }
}

// clip (coef = min(1, max_norm / (norm + 1e-6)), the clipped gradient is written back) and one Adam step, torch's formulas
__global__ __launch_bounds__(kThreads) void adam_kernel(float *grad, float *m1, float *m2, Params prm, Tensors t,
                                                        const int32_t *step, const float *grad_norm, float lr, float beta1,
                                                        float beta2, float eps, float max_norm, const int32_t *active)
{
    const int i = blockIdx.y;
    if (active && active[i] == 0) return;        // weights, moments and the gradient slice stay as they are
    // the agent's bias corrections (torch: step_size = lr / (1 - beta1^step), sqrt(1 - beta2^step)), once per workgroup
    __shared__ float corr[2];
    if (threadIdx.x == 0) {
        const double s = (double)step[i];
        corr[0] = (float)((double)lr / (1.0 - pow((double)beta1, s)));
        corr[1] = (float)sqrt(1.0 - pow((double)beta2, s));
    }
    __syncthreads();
    long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= t.per_agent) return;
    int j = 0;
    while (e >= t.size[j]) { e -= t.size[j]; ++j; }
    const long long f = t.off[j] + (long long)i * t.size[j] + e;
    const float coef = fminf(max_norm / (grad_norm[i] + 1e-6f), 1.f);
    const float g = grad[f] * coef;
    grad[f] = g;
    const float m = m1[f] + (g - m1[f]) * (1.f - beta1);
    const float v = m2[f] * beta2 + (1.f - beta2) * g * g;
    m1[f] = m;
    m2[f] = v;
    const float step_size = corr[0], bc2_sqrt = corr[1];
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    float *p = prm.p[j] + (long long)i * t.size[j] + e;
    *p = *p - step_size * (m / denom);
}

int launch_gemm(GemmArgs g, int batch, hipStream_t st, const int32_t *active)
{
    if (g.M <= 0 || g.N <= 0) return DRONESIM_OK;
    g.active = active;
    dim3 grid((g.N + kBN - 1) / kBN, (g.M + kBM - 1) / kBM, batch);
    hipLaunchKernelGGL(gemm_kernel, grid, dim3(kThreads), 0, st, g);
    return DRONESIM_OK;
}

GemmArgs gemm(const float *A, long long sAm, long long sAk, long long bA, const float *B, long long sBk, long long sBn, long long bB,
              float *C, long long ldc, long long bC, int M, int N, int K, int mode)
{
    GemmArgs g = {};
    g.A = A; g.sAm = sAm; g.sAk = sAk; g.bA = bA;
    g.B = B; g.sBk = sBk; g.sBn = sBn; g.bB = bB;
    g.C = C; g.ldc = ldc; g.bC = bC;
    g.M = M; g.N = N; g.K = K; g.ones_row = -1; g.mode = mode;
    return g;
}

int check_mlp(const DroneMlp *m, const char *where)
{
    char msg[160];
    if (!m) { snprintf(msg, sizeof msg, "%s: NULL DroneMlp", where); return dronesim_fail(DRONESIM_EINVAL, msg); }
    if (m->w2_layout != 0) {
        snprintf(msg, sizeof msg, "%s: the learner reads the plain weight arrays (w2_layout = 0)", where);
        return dronesim_fail(DRONESIM_EINVAL, msg);
    }
    if (m->N < 1 || m->d_in < 1 || m->d_in > 64 || m->h1 < 1 || m->h1 > 4096 || m->h2 < 1 || m->h2 > 4096 || m->nout < 1 || m->nout > 32) {
        snprintf(msg, sizeof msg, "%s: need N >= 1, 1 <= d_in <= 64, 1 <= h1, h2 <= 4096, 1 <= nout <= 32", where);
        return dronesim_fail(DRONESIM_EINVAL, msg);
    }
    if ((m->out_kind == 0 && m->nout != 1) || (m->out_kind == 1 && m->nout < 2) ||
        (m->out_kind == 2 && (m->nout != 4 || m->h2 % 2 != 0)) || m->out_kind < 0 || m->out_kind > 2) {
        snprintf(msg, sizeof msg, "%s: out_kind 0 needs nout = 1, 1 nout >= 2, 2 nout = 4 and an even h2", where);
        return dronesim_fail(DRONESIM_EINVAL, msg);
    }
    if (!m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->w3 || !m->b3) {
        snprintf(msg, sizeof msg, "%s: NULL weight array", where);
        return dronesim_fail(DRONESIM_EINVAL, msg);
    }
    return DRONESIM_OK;
}

size_t workspace_bytes(const DroneMlp *m, int rc)
{
    return sizeof(float) * (size_t)m->N * (size_t)rc * (size_t)(m->h1 + m->h2 + m->nout + 1);
}

// what the PPO entry points add to the chain (all NULL / 0 for dronesim_mlp_grad)
struct PpoArgs {
    const float *logp_old, *adv;
    float lo, hi;
    float *stats;          // [4][N]
    float *logp_out;       // set: forward + log-probabilities only
};

// what the entropy entry points add to the chain (NULL for the others): the heads with the entropy term, one more per-row plane
struct EntArgs {
    float scale;           // ent_scale
    float *entropy;        // [N]: the mean row entropy (dronesim_mlp_grad_ppo_ent: stats + 4 N)
};

// what dronesim_mlp_grad_ppo_gated adds to the PPO-with-entropy chain (NULL for the others): the per-agent gate every kernel of
// the chain obeys, and the k plane + its float64 running sums behind the sibling's workspace
struct GateArgs {
    const int32_t *active; // [N], device memory; may be NULL (nothing gated)
    float *kl;             // [N]: stats + 5 N
};

// what dronesim_mlp_grad_vclip adds to the critic chain (NULL for the others): the plane of zero-gradient flags sits at S
struct VclipArgs {
    const float *v_old;
    float vf_clip;
    float *clip_fraction;  // [N]
};

// The chunked chain of the header comment over all R rows; arguments validated by the entry points.
int run_chain(const DroneMlp *m, const float *x, int R, float row_scale, const float *target, const float *act, const float *weight,
              const PpoArgs *ppo, const EntArgs *ent, const GateArgs *gate, const VclipArgs *vc, float *grad, float *loss,
              int rows_per_chunk, void *ws, hipStream_t st)
{
    const int N = m->N, din = m->d_in, h1 = m->h1, h2 = m->h2, no = m->nout;
    const long long Rc = rows_per_chunk;
    const Tensors t = tensors_of(m);
    float *gw1 = grad + t.off[0], *gb1 = grad + t.off[1], *gw2 = grad + t.off[2];
    float *gb2 = grad + t.off[3], *gw3 = grad + t.off[4], *gb3 = grad + t.off[5];
    float *H1 = (float *)ws, *H2 = H1 + N * Rc * h1, *O = H2 + N * Rc * h2, *L = O + N * Rc * no, *S = L + N * Rc;
    float *En = ppo ? S + 3 * N * Rc : S;         // the row entropies, behind the sibling's workspace
    float *Kp = gate ? En + N * Rc : nullptr;     // the gated form's k plane, then its float64 running sums [N]
    double *Kacc = gate ? (double *)(Kp + N * Rc) : nullptr;
    const int32_t *active = gate ? gate->active : nullptr;

    const long long xs = (long long)N * din;      // row stride of x
    for (long long r0 = 0; r0 < R; r0 += Rc) {
        const int rc = (int)((R - r0) < Rc ? (R - r0) : Rc);
        const float *X = x + r0 * xs;
        GemmArgs g;
        // forward
        g = gemm(X, xs, 1, din, m->w1, h1, 1, (long long)din * h1, H1, h1, Rc * h1, rc, h1, din, kReluBias);
        g.bias = m->b1; g.bBias = h1;
        launch_gemm(g, N, st, active);
        g = gemm(H1, h1, 1, Rc * h1, m->w2, h2, 1, (long long)h1 * h2, H2, h2, Rc * h2, rc, h2, h1, kReluBias);
        g.bias = m->b2; g.bBias = h2;
        launch_gemm(g, N, st, active);
        g = gemm(H2, h2, 1, Rc * h2, m->w3, no, 1, (long long)h2 * no, O, no, Rc * no, rc, no, h2, kBias);
        g.bias = m->b3; g.bBias = no;
        launch_gemm(g, N, st, active);
        // head
        const long long items = (long long)rc * N;
        const dim3 hgrid((unsigned)((items + kThreads - 1) / kThreads));
        if (ent && ppo)
            hipLaunchKernelGGL(ppo_head_ent_kernel, hgrid, dim3(kThreads), 0, st, O, L, S, En, Rc, rc, r0, N, no, m->out_kind, row_scale,
                               ent->scale, act, ppo->logp_old, ppo->adv, ppo->lo, ppo->hi, active, Kp);
        else if (ent)
            hipLaunchKernelGGL(head_ent_kernel, hgrid, dim3(kThreads), 0, st, O, L, En, Rc, rc, r0, N, no, m->out_kind, row_scale,
                               ent->scale, act, weight);
        else if (ppo)
            hipLaunchKernelGGL(ppo_head_kernel, hgrid, dim3(kThreads), 0, st, O, L, S, Rc, rc, r0, N, no, m->out_kind, row_scale, act,
                               ppo->logp_old, ppo->adv, ppo->lo, ppo->hi, ppo->logp_out);
        else
            hipLaunchKernelGGL(head_kernel, hgrid, dim3(kThreads), 0, st, O, L, Rc, rc, r0, N, no, m->out_kind, row_scale, target, act,
                               weight, vc ? vc->v_old : nullptr, vc ? vc->vf_clip : 0.f, S);
        if (ppo && ppo->logp_out) continue;
        // layer 3: dW3 += H2^T dO (+ db3), then dH2 = (dO W3^T) . [H2 > 0] in place of H2
        g = gemm(H2, 1, h2, Rc * h2, O, no, 1, Rc * no, gw3, no, (long long)h2 * no, h2 + 1, no, rc, kAccumulate);
        g.ones_row = h2; g.Cb = gb3; g.bCb = no; g.first = r0 == 0;
        if (m->out_kind == 2) { g.half_m = h2 / 2; g.half_n = no / 2; }
        launch_gemm(g, N, st, active);
        g = gemm(O, no, 1, Rc * no, m->w3, 1, no, (long long)h2 * no, H2, h2, Rc * h2, rc, h2, no, kMask);
        launch_gemm(g, N, st, active);
        // layer 2: dW2 += H1^T dH2 (+ db2), then dH1 = (dH2 W2^T) . [H1 > 0] in place of H1
        g = gemm(H1, 1, h1, Rc * h1, H2, h2, 1, Rc * h2, gw2, h2, (long long)h1 * h2, h1 + 1, h2, rc, kAccumulate);
        g.ones_row = h1; g.Cb = gb2; g.bCb = h2; g.first = r0 == 0;
        launch_gemm(g, N, st, active);
        g = gemm(H2, h2, 1, Rc * h2, m->w2, 1, h2, (long long)h1 * h2, H1, h1, Rc * h1, rc, h1, h2, kMask);
        launch_gemm(g, N, st, active);
        // layer 1: dW1 += X^T dH1 (+ db1)
        g = gemm(X, 1, xs, din, H1, h1, 1, Rc * h1, gw1, h1, (long long)din * h1, din + 1, h1, rc, kAccumulate);
        g.ones_row = din; g.Cb = gb1; g.bCb = h1; g.first = r0 == 0;
        launch_gemm(g, N, st, active);
        hipLaunchKernelGGL(loss_sum_kernel, dim3(N), dim3(kThreads), 0, st, L, Rc, rc, (int)(r0 == 0), loss, active);
        if (ppo)
            hipLaunchKernelGGL(ppo_stats_kernel, dim3(N), dim3(kThreads), 0, st, S, Rc, rc, N, (int)(r0 == 0), (int)(r0 + Rc >= R),
                               (float)R, ppo->stats, active);
        if (ent)
            hipLaunchKernelGGL(entropy_sum_kernel, dim3(N), dim3(kThreads), 0, st, En, Rc, rc, (int)(r0 == 0), (int)(r0 + Rc >= R),
                               (float)R, ent->entropy, active);
        if (gate)
            hipLaunchKernelGGL(kl_sum_kernel, dim3(N), dim3(kThreads), 0, st, Kp, Rc, rc, (int)(r0 == 0), (int)(r0 + Rc >= R),
                               (double)R, Kacc, gate->kl, active);
        if (vc)
            hipLaunchKernelGGL(entropy_sum_kernel, dim3(N), dim3(kThreads), 0, st, S, Rc, rc, (int)(r0 == 0), (int)(r0 + Rc >= R),
                               (float)R, vc->clip_fraction, active);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}

int fail_at(const char *where, const char *what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", where, what);
    return dronesim_fail(DRONESIM_EINVAL, msg);
}

// the checks the actor-only entry points share: an actor, R, the chunk size
int check_actor_call(const DroneMlp *m, int R, int rows_per_chunk, const char *where)
{
    const int rc = check_mlp(m, where);
    if (rc != DRONESIM_OK) return rc;
    if (m->out_kind == 0) return fail_at(where, "needs an actor (out_kind 1 or 2), not a critic");
    if (R < 1) return fail_at(where, "R < 1");
    if (rows_per_chunk < 64 || rows_per_chunk % 64 != 0) return fail_at(where, "rows_per_chunk must be a positive multiple of 64");
    return DRONESIM_OK;
}

// the PPO head's three per-row diagnostics behind the gradient workspace
size_t ppo_workspace_bytes(const DroneMlp *m, int rc)
{
    return workspace_bytes(m, rc) + sizeof(float) * (size_t)m->N * (size_t)rc * 3;
}

// the entropy heads' row-entropy plane behind the sibling's workspace
size_t ent_workspace_bytes(const DroneMlp *m, int rc, bool ppo)
{
    return (ppo ? ppo_workspace_bytes(m, rc) : workspace_bytes(m, rc)) + sizeof(float) * (size_t)m->N * (size_t)rc;
}

// the gated PPO form's k plane and the N float64 running sums behind the entropy form's workspace (a multiple of 256 bytes)
size_t gated_workspace_bytes(const DroneMlp *m, int rc)
{
    return ent_workspace_bytes(m, rc, true) + sizeof(float) * (size_t)m->N * (size_t)rc + sizeof(double) * (size_t)m->N;
}

// the clipped value head's plane of zero-gradient flags behind the gradient workspace
size_t vclip_workspace_bytes(const DroneMlp *m, int rc)
{
    return workspace_bytes(m, rc) + sizeof(float) * (size_t)m->N * (size_t)rc;
}

// Per-agent standardisation of x [R][N] (include/dronesim.h: dronesim_standardize), two launches over one decomposition that
// depends on (R, N) only:
//   lane group   V = 4 adjacent columns where N % 4 == 0 (one 16-byte access where the pointers allow it), else 1
//   column tile  `tw` lane groups: 16 (64 floats, 256 contiguous bytes per row) where N % 64 == 0 -- at N = 64 the whole row --,
//                else the whole row, capped so that a tile has at most 1024 columns
//   iteration    a workgroup of 1024 lanes covers q = 1024 / tw rows of its tile at once: lane t holds row t / tw, group t % tw,
//                i.e. flat position t of the q x tw block (with one tile per row: of the flat array) -- N = 5 or 70 walk the
//                array contiguously with 1020 / 980 lanes, and a lane meets the same columns in every iteration
//   slab         `rps` rows (a multiple of q); S slabs x tiles workgroups aim at kStdBlocks, one per CU
// Pass 1: every lane of a column shifts by the same K, the column's value in the slab's first row (a value of the column: no
// cancellation at -500 +- 0.5), and accumulates in double the sums of d = x - K and of d^2; the q lanes of a column are folded
// through LDS by ONE fixed tree (both sums per level) into the slab's sum rows K + sum d and its second moment about the slab's
// own mean, sum d^2 - (sum d)^2 / rows: ws [S][2][N].  Nothing but the tree and one division per column follows the loop.
// Pass 2: every workgroup requests its first kStdPre iterations of rows, then folds the S partials of its tile's columns in ONE
// sweep -- up to kStdRuns contiguous runs of slabs, one lane each, ascending, then the runs ascending: the plain sums (mean), and the
// moments about slab 0's mean m0, sum_s (m2_s + e_s^2 / n_s) with e_s = sum_s - n_s m0, which - (sum_s e_s)^2 / R is the moment
// about the mean -- into mean and 1 / (std + eps), and maps its rows.  An all-equal column has K = c, d = 0, sum = rows c and
// e_s = 0 exactly.  The tile rule keeps that fold at S x 64 x 16 bytes per workgroup for the wide shapes (C5 shard: 64 KiB).
constexpr int kStdThreads = 1024, kStdBlocks = 256, kStdRuns = 32, kStdPre = 4;

struct StdPlan {
    int V, tw, tiles, q, S;
    long long rps;
};

StdPlan std_plan(int R, int N)
{
    StdPlan p;
    p.V = N % 4 == 0 ? 4 : 1;
    const int nv = N / p.V, cap = kStdThreads / p.V;
    p.tw = (p.V == 4 && N % 64 == 0) ? 16 : (nv <= cap ? nv : cap);
    p.tiles = (nv + p.tw - 1) / p.tw;
    p.q = kStdThreads / p.tw;
    const long long iters = ((long long)R + p.q - 1) / p.q;
    long long want = kStdBlocks / p.tiles;
    want = want < 1 ? 1 : (want > iters ? iters : want);
    p.rps = ((iters + want - 1) / want) * p.q;
    p.S = (int)(((long long)R + p.rps - 1) / p.rps);
    return p;
}

typedef float std_f4 __attribute__((ext_vector_type(4)));

// NT: the last use of the element (pass 2 reads a row once more and writes it once), as the return scans do
template <int V, bool VEC, bool NT>
__device__ __forceinline__ void std_load(const float *p, float (&v)[V])
{
    if (VEC) {
        const std_f4 f = NT ? __builtin_nontemporal_load(reinterpret_cast<const std_f4 *>(p)) : *reinterpret_cast<const std_f4 *>(p);
        v[0] = f.x; v[V > 1 ? 1 : 0] = f.y; v[V > 2 ? 2 : 0] = f.z; v[V > 3 ? 3 : 0] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = NT ? __builtin_nontemporal_load(p + k) : p[k];
    }
}

template <int V, bool VEC>
__device__ __forceinline__ void std_store(float *o, const float (&v)[V])
{
    if (VEC) {
        std_f4 f;
        f.x = v[0]; f.y = v[V > 1 ? 1 : 0]; f.z = v[V > 2 ? 2 : 0]; f.w = v[V > 3 ? 3 : 0];
        __builtin_nontemporal_store(f, reinterpret_cast<std_f4 *>(o));
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) __builtin_nontemporal_store(v[k], o + k);
    }
}

template <int V, bool VEC>
__global__ __launch_bounds__(kStdThreads) void standardize_sums_kernel(const float *__restrict__ x, double *__restrict__ ws, int R,
                                                                       int N, int tw, int q, int qp, long long rps)
{
    __shared__ double b1[kStdThreads][V], b2[kStdThreads][V];
    const int t = threadIdx.x, rl = t / tw, g = blockIdx.y * tw + t % tw;
    const bool lane_on = rl < q && g * V < N;
    const long long r_begin = (long long)blockIdx.x * rps;
    const long long r_end = r_begin + rps < R ? r_begin + rps : R;
    double sd[V], sd2[V], k0[V];
#pragma unroll
    for (int k = 0; k < V; ++k) sd[k] = sd2[k] = k0[k] = 0.0;
    if (lane_on) {
        float v[V];
        std_load<V, VEC, false>(x + (size_t)r_begin * N + (size_t)g * V, v);   // K: the slab's first row (cached: one read per
                                                                                 // column tile; its owners meet it again at j = 0)
#pragma unroll
        for (int k = 0; k < V; ++k) k0[k] = (double)v[k];
        if (r_begin + rl < r_end) {
            const float *p = x + (size_t)(r_begin + rl) * N + (size_t)g * V;
            const size_t step = (size_t)q * N;
            const long long n = (r_end - r_begin - rl + q - 1) / q;
#pragma unroll 4
            for (long long j = 0; j < n; ++j) {
                std_load<V, VEC, false>(p + j * step, v);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const double d = (double)v[k] - k0[k];
                    sd[k] += d;
                    sd2[k] = fma(d, d, sd2[k]);
                }
            }
        }
    }
    // fixed tree over the q lanes (rows) of a column: b[t] += b[t + w tw], w = qp / 2 .. 1 (qp = q rounded up to 2^n)
#pragma unroll
    for (int k = 0; k < V; ++k) { b1[t][k] = sd[k]; b2[t][k] = sd2[k]; }
    for (int w = qp >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (lane_on && rl < w && rl + w < q) {
#pragma unroll
            for (int k = 0; k < V; ++k) { b1[t][k] += b1[t + w * tw][k]; b2[t][k] += b2[t + w * tw][k]; }
        }
    }
    if (lane_on && rl == 0) {                                            // (its own sums: the last level's writer)
        const double rows = (double)(r_end - r_begin);
        double *o = ws + (size_t)blockIdx.x * 2 * N + (size_t)g * V;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double s = b1[t][k];
            o[k] = fma(rows, k0[k], s);
            o[N + k] = fmax(b2[t][k] - s * s / rows, 0.0);
        }
    }
}

template <int V, bool VEC>
__global__ __launch_bounds__(kStdThreads) void standardize_apply_kernel(const float *x, float *y, const double *__restrict__ ws,
                                                                        float *__restrict__ stats, int R, int N, int tw, int q,
                                                                        long long rps, int S, float eps)
{
    __shared__ double part[3][kStdThreads], mean_s[kStdThreads], inv_s[kStdThreads];
    const int t = threadIdx.x;
    // the map's first rows, requested before the fold: lane t at row t / tw, group t % tw, as in pass 1
    const int rl = t / tw, gl = t % tw, g = blockIdx.y * tw + gl;
    const long long r_begin = (long long)blockIdx.x * rps;
    const long long r_end = r_begin + rps < R ? r_begin + rps : R;
    const bool map_on = rl < q && g * V < N && r_begin + rl < r_end;
    const long long n = map_on ? (r_end - r_begin - rl + q - 1) / q : 0;
    const size_t at = (size_t)(r_begin + rl) * N + (size_t)g * V, step = (size_t)q * N;
    float pv[kStdPre][V];
#pragma unroll
    for (int u = 0; u < kStdPre; ++u) {
#pragma unroll
        for (int k = 0; k < V; ++k) pv[u][k] = 0.f;
        if (u < n) std_load<V, VEC, true>(x + at + u * step, pv[u]);
    }
    const int c0 = blockIdx.y * tw * V;                                  // the tile's first column
    const int nc = (N - c0) < tw * V ? (N - c0) : tw * V;                // its columns (<= 1024)
    // the fold: lane (run, column) takes the slabs [run ch, (run + 1) ch) in ascending order, lane (0, column) then the runs
    const int runs = kStdThreads / nc < kStdRuns ? kStdThreads / nc : kStdRuns, run = t / nc, col = t % nc;
    const int ch = (S + runs - 1) / runs;
    const int s_lo = run * ch, s_hi = (s_lo + ch) < S ? (s_lo + ch) : S;
    const double n_full = (double)(rps < R ? rps : R), n_last = (double)(R - (long long)(S - 1) * rps);
    double a = 0.0, b = 0.0, e1 = 0.0;
    if (run < runs && s_lo < s_hi) {
        const double m0 = ws[c0 + col] / n_full, inv_full = 1.0 / n_full, inv_last = 1.0 / n_last;
#pragma unroll 8
        for (int s = s_lo; s < s_hi; ++s) {
            const double sum = ws[(size_t)s * 2 * N + c0 + col], m2 = ws[(size_t)s * 2 * N + N + c0 + col];
            const double ns = s == S - 1 ? n_last : n_full, e = fma(-ns, m0, sum);
            a += sum;
            e1 += e;
            b += fma(e * e, s == S - 1 ? inv_last : inv_full, m2);
        }
    }
    part[0][t] = a;
    part[1][t] = b;
    part[2][t] = e1;
    __syncthreads();
    if (t < nc) {
        double tot = 0.0, m2 = 0.0, es = 0.0;
        for (int u = 0; u < runs; ++u) {
            tot += part[0][u * nc + t];
            m2 += part[1][u * nc + t];
            es += part[2][u * nc + t];
        }
        const double mean = tot / (double)R;
        const double sd = sqrt(fmax(m2 - es * es / (double)R, 0.0) / (double)R), den = sd + (double)eps;
        mean_s[t] = mean;
        inv_s[t] = den > 0.0 ? 1.0 / den : 0.0;                          // (an all-equal column at eps = 0: y = 0, not 0 / 0)
        if (stats && blockIdx.x == 0) {
            stats[c0 + t] = (float)mean;
            stats[N + c0 + t] = (float)sd;
        }
    }
    __syncthreads();
    // the map: y = (x - mean) * (1 / (std + eps)) in double (within 2^-52 of the quotient before the rounding to float)
    if (!map_on) return;
    double mean[V], inv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { mean[k] = mean_s[gl * V + k]; inv[k] = inv_s[gl * V + k]; }
#pragma unroll
    for (int u = 0; u < kStdPre; ++u) {
        if (u < n) {
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = (float)(((double)pv[u][k] - mean[k]) * inv[k]);
            std_store<V, VEC>(y + at + u * step, v);
        }
    }
#pragma unroll 4
    for (long long j = kStdPre; j < n; ++j) {
        float v[V];
        std_load<V, VEC, true>(x + at + j * step, v);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (float)(((double)v[k] - mean[k]) * inv[k]);
        std_store<V, VEC>(y + at + j * step, v);
    }
}

}  // namespace

extern "C" int dronesim_standardize_workspace(int R, int N, size_t *bytes)
{
    if (R < 1 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize_workspace: R < 1 or N < 1");
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize_workspace: NULL bytes");
    *bytes = sizeof(double) * 2 * (size_t)std_plan(R, N).S * (size_t)N;
    return DRONESIM_OK;
}

extern "C" int dronesim_standardize(const float *x, float *y, float *stats, int R, int N, float eps, void *ws, size_t ws_bytes,
                                    void *stream)
{
    if (R < 1 || N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: R < 1 or N < 1");
    if (!x || !y || !ws) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: NULL x / y / workspace");
    if (!(eps >= 0.f)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: eps must be >= 0");
    const StdPlan p = std_plan(R, N);
    if (ws_bytes < sizeof(double) * 2 * (size_t)p.S * (size_t)N)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: workspace smaller than dronesim_standardize_workspace()");
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return dronesim_fail(DRONESIM_EINVAL, "dronesim_standardize: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int qp = 1;
    while (qp < p.q) qp <<= 1;
    const dim3 grid((unsigned)p.S, (unsigned)p.tiles), block(kStdThreads);
    double *w = (double *)ws;
    // 16-byte accesses where every lane group starts 16-byte aligned; the lanes' columns and rows do not depend on it
    const bool vec = p.V == 4 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
    if (vec) {
        hipLaunchKernelGGL((standardize_sums_kernel<4, true>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<4, true>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    } else if (p.V == 4) {
        hipLaunchKernelGGL((standardize_sums_kernel<4, false>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<4, false>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    } else {
        hipLaunchKernelGGL((standardize_sums_kernel<1, false>), grid, block, 0, st, x, w, R, N, p.tw, p.q, qp, p.rps);
        hipLaunchKernelGGL((standardize_apply_kernel<1, false>), grid, block, 0, st, x, y, w, stats, R, N, p.tw, p.q, p.rps, p.S, eps);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_grad_ent_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_actor_call(m, 1, rows_per_chunk, "dronesim_mlp_grad_ent_workspace");
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ent_workspace: NULL bytes");
    *bytes = ent_workspace_bytes(m, rows_per_chunk, false);
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_grad_ppo_ent_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_actor_call(m, 1, rows_per_chunk, "dronesim_mlp_grad_ppo_ent_workspace");
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_ent_workspace: NULL bytes");
    *bytes = ent_workspace_bytes(m, rows_per_chunk, true);
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_grad_ent(const DroneMlp *m, const float *x, int R, float row_scale, const float *act, const float *weight,
                                     float ent_scale, float *grad, float *loss, float *entropy, int rows_per_chunk, void *ws,
                                     size_t ws_bytes, void *stream)
{
    const int rc = check_actor_call(m, R, rows_per_chunk, "dronesim_mlp_grad_ent");
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !weight || !grad || !loss || !entropy || !ws)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ent: NULL x / act / weight / grad / loss / entropy / workspace");
    if (!(ent_scale >= 0.f) || isinf(ent_scale)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ent: ent_scale must be finite and >= 0");
    if (ws_bytes < ent_workspace_bytes(m, rows_per_chunk, false))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ent: workspace smaller than dronesim_mlp_grad_ent_workspace()");
    EntArgs en = {ent_scale, entropy};
    return run_chain(m, x, R, row_scale, nullptr, act, weight, nullptr, &en, nullptr, nullptr, grad, loss, rows_per_chunk, ws, (hipStream_t)stream);
}

extern "C" int dronesim_mlp_grad_ppo_ent(const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
                                         const float *logp_old, const float *adv, float clip_eps, float ent_scale, float *grad,
                                         float *loss, float *stats, int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    const int rc = check_actor_call(m, R, rows_per_chunk, "dronesim_mlp_grad_ppo_ent");
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !logp_old || !adv || !grad || !loss || !stats || !ws)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_ent: NULL x / act / logp_old / adv / grad / loss / stats / workspace");
    if (!(clip_eps > 0.f && clip_eps < 1.f)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_ent: clip_eps must be in (0, 1)");
    if (!(ent_scale >= 0.f) || isinf(ent_scale))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_ent: ent_scale must be finite and >= 0");
    if (ws_bytes < ent_workspace_bytes(m, rows_per_chunk, true))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_ent: workspace smaller than dronesim_mlp_grad_ppo_ent_workspace()");
    PpoArgs p = {};
    p.logp_old = logp_old; p.adv = adv; p.lo = 1.f - clip_eps; p.hi = 1.f + clip_eps; p.stats = stats;
    EntArgs en = {ent_scale, stats + 4 * (size_t)m->N};
    return run_chain(m, x, R, row_scale, nullptr, act, nullptr, &p, &en, nullptr, nullptr, grad, loss, rows_per_chunk, ws, (hipStream_t)stream);
}

extern "C" int dronesim_mlp_grad_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_mlp(m, "dronesim_mlp_grad_workspace");
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_workspace: NULL bytes");
    if (rows_per_chunk < 64 || rows_per_chunk % 64 != 0)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_workspace: rows_per_chunk must be a positive multiple of 64");
    *bytes = workspace_bytes(m, rows_per_chunk);
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_grad(const DroneMlp *m, const float *x, int R, float row_scale, const float *target, const float *act,
                                 const float *weight, float *grad, float *loss, int rows_per_chunk, void *ws, size_t ws_bytes,
                                 void *stream)
{
    int rc0 = check_mlp(m, "dronesim_mlp_grad");
    if (rc0 != DRONESIM_OK) return rc0;
    if (!x || !grad || !loss || !ws) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad: NULL x / grad / loss / workspace");
    if (m->out_kind == 0 && !target) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad: the critic loss needs target");
    if (m->out_kind != 0 && (!act || !weight))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad: the actor loss needs act and weight");
    if (R < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad: R < 1");
    if (rows_per_chunk < 64 || rows_per_chunk % 64 != 0)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad: rows_per_chunk must be a positive multiple of 64");
    if (ws_bytes < workspace_bytes(m, rows_per_chunk))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad: workspace smaller than dronesim_mlp_grad_workspace()");
    return run_chain(m, x, R, row_scale, target, act, weight, nullptr, nullptr, nullptr, nullptr, grad, loss, rows_per_chunk, ws, (hipStream_t)stream);
}

extern "C" int dronesim_mlp_grad_ppo_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_actor_call(m, 1, rows_per_chunk, "dronesim_mlp_grad_ppo_workspace");
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_workspace: NULL bytes");
    *bytes = ppo_workspace_bytes(m, rows_per_chunk);
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_logp(const DroneMlp *m, const float *x, int R, const float *act, float *logp, int rows_per_chunk,
                                 void *ws, size_t ws_bytes, void *stream)
{
    const int rc = check_actor_call(m, R, rows_per_chunk, "dronesim_mlp_logp");
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !logp || !ws) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_logp: NULL x / act / logp / workspace");
    if (ws_bytes < workspace_bytes(m, rows_per_chunk))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_logp: workspace smaller than dronesim_mlp_grad_workspace()");
    PpoArgs p = {};
    p.logp_out = logp;
    // (grad and loss are not touched by the forward-only chain; the workspace stands in for their base address)
    return run_chain(m, x, R, 1.f, nullptr, act, nullptr, &p, nullptr, nullptr, nullptr, (float *)ws, nullptr, rows_per_chunk, ws, (hipStream_t)stream);
}

extern "C" int dronesim_mlp_grad_ppo(const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
                                     const float *logp_old, const float *adv, float clip_eps, float *grad, float *loss, float *stats,
                                     int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    const int rc = check_actor_call(m, R, rows_per_chunk, "dronesim_mlp_grad_ppo");
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !logp_old || !adv || !grad || !loss || !stats || !ws)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo: NULL x / act / logp_old / adv / grad / loss / stats / workspace");
    if (!(clip_eps > 0.f && clip_eps < 1.f)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo: clip_eps must be in (0, 1)");
    if (ws_bytes < ppo_workspace_bytes(m, rows_per_chunk))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo: workspace smaller than dronesim_mlp_grad_ppo_workspace()");
    PpoArgs p = {};
    p.logp_old = logp_old; p.adv = adv; p.lo = 1.f - clip_eps; p.hi = 1.f + clip_eps; p.stats = stats;
    return run_chain(m, x, R, row_scale, nullptr, act, nullptr, &p, nullptr, nullptr, nullptr, grad, loss, rows_per_chunk, ws, (hipStream_t)stream);
}

namespace {

int adam_step(const char *where, const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
              float beta2, float eps, float max_norm, float *grad_norm, const int32_t *active, void *stream)
{
    int rc = check_mlp(m, where);
    if (rc != DRONESIM_OK) return rc;
    if (!grad || !m1 || !m2 || !step || !grad_norm) return fail_at(where, "NULL grad / m1 / m2 / step / grad_norm");
    if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(max_norm > 0.f))
        return fail_at(where, "need lr >= 0, 0 <= beta < 1, eps > 0, max_norm > 0");
    hipStream_t st = (hipStream_t)stream;
    const Tensors t = tensors_of(m);
    Params p;
    const float *w[6] = {m->w1, m->b1, m->w2, m->b2, m->w3, m->b3};
    for (int j = 0; j < 6; ++j) p.p[j] = const_cast<float *>(w[j]);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(m->N), dim3(kThreads), 0, st, grad, t, step, grad_norm, active);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((t.per_agent + kThreads - 1) / kThreads), m->N), dim3(kThreads), 0, st,
                       grad, m1, m2, p, t, step, grad_norm, lr, beta1, beta2, eps, max_norm, active);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}

}  // namespace

extern "C" int dronesim_adam_step(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                                  float beta2, float eps, float max_norm, float *grad_norm, void *stream)
{
    return adam_step("dronesim_adam_step", m, grad, m1, m2, step, lr, beta1, beta2, eps, max_norm, grad_norm, nullptr, stream);
}

extern "C" int dronesim_adam_step_gated(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                                        float beta2, float eps, float max_norm, float *grad_norm, const int32_t *active,
                                        void *stream)
{
    if (!active) return dronesim_fail(DRONESIM_EINVAL, "dronesim_adam_step_gated: NULL active");
    return adam_step("dronesim_adam_step_gated", m, grad, m1, m2, step, lr, beta1, beta2, eps, max_norm, grad_norm, active, stream);
}

extern "C" int dronesim_mlp_grad_ppo_gated_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_actor_call(m, 1, rows_per_chunk, "dronesim_mlp_grad_ppo_gated_workspace");
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_ppo_gated_workspace: NULL bytes");
    *bytes = gated_workspace_bytes(m, rows_per_chunk);
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_grad_ppo_gated(const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
                                           const float *logp_old, const float *adv, float clip_eps, float ent_scale,
                                           const int32_t *active, float *grad, float *loss, float *stats, int rows_per_chunk,
                                           void *ws, size_t ws_bytes, void *stream)
{
    const char *where = "dronesim_mlp_grad_ppo_gated";
    const int rc = check_actor_call(m, R, rows_per_chunk, where);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !logp_old || !adv || !grad || !loss || !stats || !ws)
        return fail_at(where, "NULL x / act / logp_old / adv / grad / loss / stats / workspace");
    if (!(clip_eps > 0.f && clip_eps < 1.f)) return fail_at(where, "clip_eps must be in (0, 1)");
    if (!(ent_scale >= 0.f) || isinf(ent_scale)) return fail_at(where, "ent_scale must be finite and >= 0");
    if (ws_bytes < gated_workspace_bytes(m, rows_per_chunk))
        return fail_at(where, "workspace smaller than dronesim_mlp_grad_ppo_gated_workspace()");
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return fail_at(where, "workspace not 8-byte aligned");
    PpoArgs p = {};
    p.logp_old = logp_old; p.adv = adv; p.lo = 1.f - clip_eps; p.hi = 1.f + clip_eps; p.stats = stats;
    EntArgs en = {ent_scale, stats + 4 * (size_t)m->N};
    GateArgs ga = {active, stats + 5 * (size_t)m->N};
    return run_chain(m, x, R, row_scale, nullptr, act, nullptr, &p, &en, &ga, nullptr, grad, loss, rows_per_chunk, ws,
                     (hipStream_t)stream);
}

extern "C" int dronesim_kl_gate(const float *kl, float target_kl, int32_t *active, int32_t *taken, int N, int reset, void *stream)
{
    if (N < 1) return dronesim_fail(DRONESIM_EINVAL, "dronesim_kl_gate: N < 1");
    if (!active || !taken) return dronesim_fail(DRONESIM_EINVAL, "dronesim_kl_gate: NULL active / taken");
    if (!reset && !kl) return dronesim_fail(DRONESIM_EINVAL, "dronesim_kl_gate: NULL kl (only reset may omit it)");
    if (!(target_kl > 0.f) || isinf(target_kl)) return dronesim_fail(DRONESIM_EINVAL, "dronesim_kl_gate: target_kl must be finite and > 0");
    hipLaunchKernelGGL(kl_gate_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, kl,
                       target_kl, active, taken, N, reset);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}

namespace {

int check_vclip_call(const DroneMlp *m, int R, int rows_per_chunk, const char *where)
{
    const int rc = check_mlp(m, where);
    if (rc != DRONESIM_OK) return rc;
    if (m->out_kind != 0) return fail_at(where, "needs a critic (out_kind 0), not an actor");
    if (R < 1) return fail_at(where, "R < 1");
    if (rows_per_chunk < 64 || rows_per_chunk % 64 != 0) return fail_at(where, "rows_per_chunk must be a positive multiple of 64");
    return DRONESIM_OK;
}

}  // namespace

extern "C" int dronesim_mlp_grad_vclip_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_vclip_call(m, 1, rows_per_chunk, "dronesim_mlp_grad_vclip_workspace");
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_mlp_grad_vclip_workspace: NULL bytes");
    *bytes = vclip_workspace_bytes(m, rows_per_chunk);
    return DRONESIM_OK;
}

extern "C" int dronesim_mlp_grad_vclip(const DroneMlp *m, const float *x, int R, float row_scale, const float *target,
                                       const float *v_old, float vf_clip, float *grad, float *loss, float *clip_fraction,
                                       int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    const char *where = "dronesim_mlp_grad_vclip";
    const int rc = check_vclip_call(m, R, rows_per_chunk, where);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !target || !v_old || !grad || !loss || !clip_fraction || !ws)
        return fail_at(where, "NULL x / target / v_old / grad / loss / clip_fraction / workspace");
    if (!(vf_clip > 0.f)) return fail_at(where, "vf_clip must be > 0 (finite, or +inf: never clamped)");
    if (ws_bytes < vclip_workspace_bytes(m, rows_per_chunk))
        return fail_at(where, "workspace smaller than dronesim_mlp_grad_vclip_workspace()");
    VclipArgs vc = {v_old, vf_clip, clip_fraction};
    return run_chain(m, x, R, row_scale, target, nullptr, nullptr, nullptr, nullptr, nullptr, &vc, grad, loss, rows_per_chunk, ws,
                     (hipStream_t)stream);
}
