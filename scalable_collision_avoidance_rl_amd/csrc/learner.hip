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
};

// 64 x 64 output tile per workgroup, four waves of one 32 x 32 accumulator each; the tile's k-slices go through LDS in k-major
// order, so a lane reads A(m = l & 31, k = l >> 5) and B(k = l >> 5, n = l & 31) -- the operand maps of the 32x32x2 form.
__global__ __launch_bounds__(kThreads) void gemm_kernel(GemmArgs g)
{
    __shared__ float As[kBK][kBM + 4];
    __shared__ float Bs[kBK][kBN + 4];
    const int b = blockIdx.z;
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
__global__ __launch_bounds__(kThreads) void head_kernel(float *O, float *L, long long Rc, int rc, long long r0, int N, int nout,
                                                        int kind, float scale, const float *target, const float *act,
                                                        const float *weight)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float loss;
    if (kind == 0) {
        const float d = o[0] - target[src];
        loss = scale * d * d;
        o[0] = 2.f * scale * d;
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
// chunk writes
__global__ __launch_bounds__(kThreads) void loss_sum_kernel(const float *L, long long Rc, int rc, int first, float *loss)
{
    __shared__ float part[kThreads];
    const int i = blockIdx.x;
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
__global__ __launch_bounds__(kThreads) void ppo_stats_kernel(const float *S, long long Rc, int rc, int N, int first, int last,
                                                             float rows, float *stats)
{
    __shared__ float part[4][kThreads];
    const int i = blockIdx.x;
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
__global__ __launch_bounds__(kThreads) void grad_norm_kernel(const float *grad, Tensors t, int32_t *step, float *grad_norm)
{
    __shared__ double part[kThreads];
    const int i = blockIdx.x;
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
                                                        float beta2, float eps, float max_norm)
{
    const int i = blockIdx.y;
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

int launch_gemm(const GemmArgs &g, int batch, hipStream_t st)
{
    if (g.M <= 0 || g.N <= 0) return DRONESIM_OK;
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

// The chunked chain of the header comment over all R rows; arguments validated by the entry points.
int run_chain(const DroneMlp *m, const float *x, int R, float row_scale, const float *target, const float *act, const float *weight,
              const PpoArgs *ppo, float *grad, float *loss, int rows_per_chunk, void *ws, hipStream_t st)
{
    const int N = m->N, din = m->d_in, h1 = m->h1, h2 = m->h2, no = m->nout;
    const long long Rc = rows_per_chunk;
    const Tensors t = tensors_of(m);
    float *gw1 = grad + t.off[0], *gb1 = grad + t.off[1], *gw2 = grad + t.off[2];
    float *gb2 = grad + t.off[3], *gw3 = grad + t.off[4], *gb3 = grad + t.off[5];
    float *H1 = (float *)ws, *H2 = H1 + N * Rc * h1, *O = H2 + N * Rc * h2, *L = O + N * Rc * no, *S = L + N * Rc;

    const long long xs = (long long)N * din;      // row stride of x
    for (long long r0 = 0; r0 < R; r0 += Rc) {
        const int rc = (int)((R - r0) < Rc ? (R - r0) : Rc);
        const float *X = x + r0 * xs;
        GemmArgs g;
        // forward
        g = gemm(X, xs, 1, din, m->w1, h1, 1, (long long)din * h1, H1, h1, Rc * h1, rc, h1, din, kReluBias);
        g.bias = m->b1; g.bBias = h1;
        launch_gemm(g, N, st);
        g = gemm(H1, h1, 1, Rc * h1, m->w2, h2, 1, (long long)h1 * h2, H2, h2, Rc * h2, rc, h2, h1, kReluBias);
        g.bias = m->b2; g.bBias = h2;
        launch_gemm(g, N, st);
        g = gemm(H2, h2, 1, Rc * h2, m->w3, no, 1, (long long)h2 * no, O, no, Rc * no, rc, no, h2, kBias);
        g.bias = m->b3; g.bBias = no;
        launch_gemm(g, N, st);
        // head
        const long long items = (long long)rc * N;
        const dim3 hgrid((unsigned)((items + kThreads - 1) / kThreads));
        if (ppo)
            hipLaunchKernelGGL(ppo_head_kernel, hgrid, dim3(kThreads), 0, st, O, L, S, Rc, rc, r0, N, no, m->out_kind, row_scale, act,
                               ppo->logp_old, ppo->adv, ppo->lo, ppo->hi, ppo->logp_out);
        else
            hipLaunchKernelGGL(head_kernel, hgrid, dim3(kThreads), 0, st, O, L, Rc, rc, r0, N, no, m->out_kind, row_scale, target, act,
                               weight);
        if (ppo && ppo->logp_out) continue;
        // layer 3: dW3 += H2^T dO (+ db3), then dH2 = (dO W3^T) . [H2 > 0] in place of H2
        g = gemm(H2, 1, h2, Rc * h2, O, no, 1, Rc * no, gw3, no, (long long)h2 * no, h2 + 1, no, rc, kAccumulate);
        g.ones_row = h2; g.Cb = gb3; g.bCb = no; g.first = r0 == 0;
        if (m->out_kind == 2) { g.half_m = h2 / 2; g.half_n = no / 2; }
        launch_gemm(g, N, st);
        g = gemm(O, no, 1, Rc * no, m->w3, 1, no, (long long)h2 * no, H2, h2, Rc * h2, rc, h2, no, kMask);
        launch_gemm(g, N, st);
        // layer 2: dW2 += H1^T dH2 (+ db2), then dH1 = (dH2 W2^T) . [H1 > 0] in place of H1
        g = gemm(H1, 1, h1, Rc * h1, H2, h2, 1, Rc * h2, gw2, h2, (long long)h1 * h2, h1 + 1, h2, rc, kAccumulate);
        g.ones_row = h1; g.Cb = gb2; g.bCb = h2; g.first = r0 == 0;
        launch_gemm(g, N, st);
        g = gemm(H2, h2, 1, Rc * h2, m->w2, 1, h2, (long long)h1 * h2, H1, h1, Rc * h1, rc, h1, h2, kMask);
        launch_gemm(g, N, st);
        // layer 1: dW1 += X^T dH1 (+ db1)
        g = gemm(X, 1, xs, din, H1, h1, 1, Rc * h1, gw1, h1, (long long)din * h1, din + 1, h1, rc, kAccumulate);
        g.ones_row = din; g.Cb = gb1; g.bCb = h1; g.first = r0 == 0;
        launch_gemm(g, N, st);
        hipLaunchKernelGGL(loss_sum_kernel, dim3(N), dim3(kThreads), 0, st, L, Rc, rc, (int)(r0 == 0), loss);
        if (ppo)
            hipLaunchKernelGGL(ppo_stats_kernel, dim3(N), dim3(kThreads), 0, st, S, Rc, rc, N, (int)(r0 == 0), (int)(r0 + Rc >= R),
                               (float)R, ppo->stats);
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

}  // namespace

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
    return run_chain(m, x, R, row_scale, target, act, weight, nullptr, grad, loss, rows_per_chunk, ws, (hipStream_t)stream);
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
    return run_chain(m, x, R, 1.f, nullptr, act, nullptr, &p, (float *)ws, nullptr, rows_per_chunk, ws, (hipStream_t)stream);
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
    return run_chain(m, x, R, row_scale, nullptr, act, nullptr, &p, grad, loss, rows_per_chunk, ws, (hipStream_t)stream);
}

extern "C" int dronesim_adam_step(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                                  float beta2, float eps, float max_norm, float *grad_norm, void *stream)
{
    int rc = check_mlp(m, "dronesim_adam_step");
    if (rc != DRONESIM_OK) return rc;
    if (!grad || !m1 || !m2 || !step || !grad_norm)
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_adam_step: NULL grad / m1 / m2 / step / grad_norm");
    if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(max_norm > 0.f))
        return dronesim_fail(DRONESIM_EINVAL, "dronesim_adam_step: need lr >= 0, 0 <= beta < 1, eps > 0, max_norm > 0");
    hipStream_t st = (hipStream_t)stream;
    const Tensors t = tensors_of(m);
    Params p;
    const float *w[6] = {m->w1, m->b1, m->w2, m->b2, m->w3, m->b3};
    for (int j = 0; j < 6; ++j) p.p[j] = const_cast<float *>(w[j]);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(m->N), dim3(kThreads), 0, st, grad, t, step, grad_norm);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((t.per_agent + kThreads - 1) / kThreads), m->N), dim3(kThreads), 0, st,
                       grad, m1, m2, p, t, step, grad_norm, lr, beta1, beta2, eps, max_norm);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dronesim_fail(DRONESIM_ELAUNCH, hipGetErrorString(e));
    return DRONESIM_OK;
}
