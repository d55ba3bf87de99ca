// Per-agent learner step of the batched MLPs (SAC_agents.py:280-357, SA2CAgents.train_NN; :410-573, SPPOAgents.train): gradients
// of the critic / actor losses over a window of rows, then clip_grad_norm_ + Adam per agent (include/dronesim.h: dronesim_mlp_grad
// and its forms, dronesim_mlp_logp, dronesim_adam_step, dronesim_kl_gate).
//
// The chain.  Exact float32.  Rows are processed in chunks of Rc (a multiple of 64); per chunk and for all N agents at once (one
// batch index per agent) run_chain enqueues
//   H1 = relu(X W1 + b1), H2 = relu(H1 W2 + b2), O = H2 W3 + b3          forward, on the matrix cores
//   dO, per-row loss (and the form's per-row planes)                     one head kernel
//   dW3 += H2^T dO (+ db3);  dH2 = (dO W3^T) . [H2 > 0]   (in place of H2)
//   dW2 += H1^T dH2 (+ db2); dH1 = (dH2 W2^T) . [H1 > 0]  (in place of H1)
//   dW1 += X^T dH1 (+ db1)
//   loss += sum of the chunk's per-row losses, and the form's other per-agent results from its planes
// Every GEMM is one launch of ONE tiled kernel on v_mfma_f32_32x32x2f32 (a k-ordered fmaf chain per output element).  A
// weight-gradient element is owned by one lane that adds the chunk's partial sum into the gradient buffer, chunks in order:
// no float atomics, bit-identical run to run.  The window's first chunk WRITES the gradient and result buffers instead of
// adding to a cleared buffer: the entry points enqueue kernels only (no memset node), which keeps a captured graph's
// replays identical to eager calls.  Bias gradients are one more output row of the same GEMM, fed by a virtual row of ones.
//
// The heads are two templates on the entropy bonus, a2c_head_kernel<kEnt> (critic with the optional clipped value loss, softmax
// actor, Gaussian actor) and ppo_head_kernel<kEnt> (the clipped surrogate of both actor kinds; <false> is also the forward-only
// log-probability pass, <true> also the gated form with the KL plane); action_of, log_sum_exp, softmax_grad and the two
// cancellation-free factors one_minus_tanh2 / one_minus_sigmoid are shared by all four instantiations.  The per-agent results are block_sum reductions in one fixed order: row_sum_kernel (loss, mean entropy, share
// of zero-gradient rows), kl_sum_kernel and grad_norm_kernel (float64), and ppo_stats_kernel (four values per level).
//
// An entry point describes its call as a ChainJob -- the form (which options), the pointers and scalars that form reads -- after
// check_call has validated it; the table of legal forms stands at the struct.  layout_of is the workspace of a form: run_chain
// takes its pointers from it and the *_workspace queries their byte count.
//
// The gate of the PPO learner's KL early stop goes through the SAME chain and kernels: every kernel of the chain takes a nullable
// per-agent gate `active` (int32 [N], device memory; NULL for every form but the gated one) -- gemm_kernel's batch index is the
// agent, so a workgroup of a gated agent returns at entry, before any barrier, uniformly; the head skips its rows and the
// per-agent results are NaN for it.  dronesim_kl_gate decides the stop on the device; dronesim_adam_step_gated obeys it.
//
// Parameter sharing (dronesim_adam_step_shared, dronesim_kl_gate_shared, dronesim_mlp_tie): a sharing map in CSR form (group_ptr
// [n_groups + 1], members [N], ascending inside a group, so a group's first member is its leader) ties the weights of a group's
// members.  The step is three launches around the two of the unshared step: group_mean_kernel leaves the float64 mean of the
// members' gradients in the leader's slice, grad_norm_kernel and adam_kernel -- the SAME kernels, one workgroup row per group
// instead of per agent (agent_of) -- update the leader, group_broadcast_kernel copies the leader's weights, counter and norm to
// the other members.  Every kernel skips a map entry outside [0, N) (group_range, agent_ok): the device arrays cannot be checked
// by the host without a synchronisation.
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

// The index of a softmax actor's stored action: the action list's entry nearest to the unit vector act[src].
__device__ __forceinline__ int action_of(const float *act, long long src, int nout)
{
    const float ax = act[2 * src], ay = act[2 * src + 1];
    const int a = (int)rintf(atan2f(ay, ax) * (float)nout * 0.15915494309189535f);
    return ((a % nout) + nout) % nout;
}

// log sum_j exp(o_j) of one row of logits in two parts, the row's maximum `mx` (its first occurrence) and the returned
// ls = log1p(sum of the OTHER logits' exp(o_j - mx)): a log-probability is lq_j = (o_j - mx) - ls.  The sum mx + ls is never formed:
// it rounds at ulp(mx), which at a saturated policy (ls ~ 1e-7 and below) is all of log p_max.
__device__ __forceinline__ float log_sum_exp(const float *o, int nout, float &mx)
{
    int jm = 0;
    mx = o[0];
    for (int j = 1; j < nout; ++j)
        if (o[j] > mx) { mx = o[j]; jm = j; }
    float s = 0.f;
    for (int j = 0; j < nout; ++j)
        if (j != jm) s += expf(o[j] - mx);
    return log1pf(s);
}

// The softmax head's dLoss/dO in place of the logits o: c (onehot_a - p) (+ the entropy's es p_j (lq_j + H) with kEnt).  The chosen
// logit's 1 - p_a is the sum of the other probabilities, not a difference of two numbers near 1.
template <bool kEnt>
__device__ __forceinline__ void softmax_grad(float *o, int nout, int a, float mx, float ls, float c, float es, float H)
{
    float others = 0.f;
    for (int j = 0; j < nout; ++j)
        if (j != a) others += expf((o[j] - mx) - ls);
    for (int j = 0; j < nout; ++j) {
        const float lq = (o[j] - mx) - ls;
        const float p = expf(lq);
        const float g = c * (j == a ? others : -p);
        o[j] = kEnt ? g + es * (p * (lq + H)) : g;
    }
}

// The two factors of the Gaussian head's chain rule that cancel when formed from mu and var: 1 - tanh^2(o) = 4 t / (1 + t)^2 with
// t = exp(-2 |o|) (1 - mu mu is 0 from |o| = 9 on, and noise well before), and 1 - sigmoid(s) = sigmoid(-s) from its own
// exponential (e / (1 + e) with e = exp(-s) is inf / inf for s < -88).
__device__ __forceinline__ float one_minus_tanh2(float o)
{
    const float t = expf(-2.f * fabsf(o));
    return 4.f * t / ((1.f + t) * (1.f + t));
}

__device__ __forceinline__ float one_minus_sigmoid(float s) { return 1.f / (1.f + expf(s)); }

// The A2C loss head of one (row, agent): per-row loss (times `scale`) into L, dLoss/dO (pre-activation outputs) in place of O.
//   kind 0 (critic, <false> only):  l = (o - G)^2
//   kind 1 (softmax):               l = -w log softmax(o)[a],  a = action_of the stored unit action
//   kind 2 (Gaussian):              l = -w sum_d [-0.5 log(2 pi var_d) - (a_d - mu_d)^2 / (2 var_d)],  mu = tanh, var = sigmoid
// kind 0 with `v_old` set is PPO's clipped value loss: Vc = V clamped to v_old +- vf_clip, l = max((V - G)^2, (Vc - G)^2); where
//   the clipped term is the STRICT maximum V is clamped and dl/dV = 0, and the row's flag (0 / 1) goes to the plane P [N][Rc].
//   An unclamped row has Vc = V itself (not v_old + (V - v_old), which rounds): it forms the plain expressions and gives their bits.
// <true> is the entropy bonus of the two actor kinds, L_i - es sum_r H_i(x_r): every value of <false> is formed by the same
//   expressions and the entropy's part is ADDED, so es = 0 gives <false>'s values (an exact zero is added).
//     softmax:   lq_j = (o_j - max) - ls,  p_j = exp(lq_j),  H = -sum_j p_j lq_j;    dO_j += es p_j (lq_j + H)
//                (from lq, never log p: a logit 120 below the maximum has p = 0 in float32 and 0 log 0 is NaN)
//     Gaussian:  H = sum_d 0.5 log(2 pi e var_d);                             dO_{2+d} += -0.5 es (1 - var_d)  (the head's omv)
//   The per-row loss is the whole objective l - es H; H itself goes to the plane P [N][Rc].
// The heads stay accurate at saturated policies (p_max = 0.999..., a mean against tanh's +-1): the factors that cancel there come
// from log_sum_exp's two parts, softmax_grad, one_minus_tanh2 and one_minus_sigmoid; mu = tanh(o), var and the Gaussian log pi are
// formed as they always were.
template <bool kEnt>
__global__ __launch_bounds__(kThreads) void a2c_head_kernel(float *O, float *L, float *P, long long Rc, int rc, long long r0, int N,
                                                            int nout, int kind, float scale, float es, const float *target,
                                                            const float *act, const float *weight, const float *v_old,
                                                            float vf_clip)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float loss, H = 0.f;
    if (!kEnt && kind == 0) {
        const float d = o[0] - target[src];
        bool zero = false;
        float dc = d;
        if (v_old) {
            const float vo = v_old[src], dv = o[0] - vo;
            const float vc = dv > vf_clip ? vo + vf_clip : (dv < -vf_clip ? vo - vf_clip : o[0]);
            dc = vc - target[src];
            zero = dc * dc > d * d;
            P[(long long)i * Rc + m] = zero ? 1.f : 0.f;
        }
        if (zero) {
            loss = scale * dc * dc;
            o[0] = 0.f;
        } else {
            loss = scale * d * d;
            o[0] = 2.f * scale * d;
        }
    } else if (kind == 1) {
        const int a = action_of(act, src, nout);
        float mx;
        const float ls = log_sum_exp(o, nout, mx);
        const float c = -scale * weight[src];
        loss = c * ((o[a] - mx) - ls);
        if (kEnt) {
            for (int j = 0; j < nout; ++j) {
                const float lq = (o[j] - mx) - ls;
                H -= expf(lq) * lq;
            }
        }
        softmax_grad<kEnt>(o, nout, a, mx, ls, c, es, H);
    } else {
        const float c = -scale * weight[src];
        float lp = 0.f;
        for (int d = 0; d < 2; ++d) {
            const float mu = tanhf(o[d]), omm = one_minus_tanh2(o[d]);
            const float var = 1.f / (1.f + expf(-o[2 + d])), omv = one_minus_sigmoid(o[2 + d]);
            const float diff = act[2 * src + d] - mu;
            lp += -0.5f * logf(6.283185307179586f * var) - diff * diff / (2.f * var);
            if (kEnt) H += 0.5f * logf(17.079468445347132f * var);
            o[d] = c * (diff / var) * omm;
            const float g = c * (-0.5f + diff * diff / (2.f * var)) * omv;
            o[2 + d] = kEnt ? g - 0.5f * es * omv : g;
        }
        loss = c * lp;
    }
    L[(long long)i * Rc + m] = kEnt ? loss - es * H : loss;
    if (kEnt) P[(long long)i * Rc + m] = H;
}

// The PPO head of one (row, agent) of an actor (kinds 1 and 2; SAC_agents.py:494, :541-549): lp = log pi_i(a | x) with the
// expressions of a2c_head_kernel's kinds.  <false> with `logp_out` set writes that and nothing else (the forward-only pass).
// Otherwise
//   r = exp(lp - logp_old),  l = -min(r Adv, clamp(r, lo, hi) Adv)  (times `scale`) into L,
//   dLoss/dO = -scale Adv r dlp/dO in place of O -- 0 where the clipped branch is the strict minimum (Adv > 0 and r > hi, or
//   Adv < 0 and r < lo) --, and the row's diagnostics into S: [0] clipped (0 / 1), [1] logp_old - lp, [2] r, each [N][Rc].
// Both modes of <false> are ONE kernel and share the instructions up to `lp`: on the same O they give the same bits, so r is
// exactly 1 until the actor moves.
// <true> adds the entropy as a2c_head_kernel<true> does (H to the plane E, l - es H to L; es = 0 gives <false>'s values).  The
// entropy's gradient is added on EVERY row, the rows on the clipped branch included (there the surrogate's part is 0).  Only
// <true> knows the gate and the plane Kp [N][Rc]: the rows of an agent with active[i] == 0 are skipped, and with Kp set every
// other row also stores k = expm1(dl) - dl >= 0, Schulman's (r - 1) - log r formed without the cancellation of r - 1 (exactly 0
// at dl = 0).
template <bool kEnt>
__global__ __launch_bounds__(kThreads) void ppo_head_kernel(float *O, float *L, float *S, float *E, long long Rc, int rc, long long r0,
                                                            int N, int nout, int kind, float scale, float es, const float *act,
                                                            const float *logp_old, const float *adv, float lo, float hi,
                                                            const int32_t *active, float *Kp, float *logp_out)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)rc * N) return;
    const int i = (int)(id / rc), m = (int)(id % rc);
    if (kEnt && active && active[i] == 0) return;
    float *o = O + ((long long)i * Rc + m) * nout;
    const long long src = (r0 + m) * N + i;
    float lp, mx = 0.f, ls = 0.f, H = 0.f;
    int a = 0;
    float omm[2], var[2], omv[2], diff[2];
    if (kind == 1) {
        a = action_of(act, src, nout);
        ls = log_sum_exp(o, nout, mx);
        lp = (o[a] - mx) - ls;
        if (kEnt) {
            for (int j = 0; j < nout; ++j) {
                const float lq = (o[j] - mx) - ls;
                H -= expf(lq) * lq;
            }
        }
    } else {
        lp = 0.f;
        for (int d = 0; d < 2; ++d) {
            omm[d] = one_minus_tanh2(o[d]);
            var[d] = 1.f / (1.f + expf(-o[2 + d]));
            omv[d] = one_minus_sigmoid(o[2 + d]);
            diff[d] = act[2 * src + d] - tanhf(o[d]);
            lp += -0.5f * logf(6.283185307179586f * var[d]) - diff[d] * diff[d] / (2.f * var[d]);
        }
        if (kEnt) {
            for (int d = 0; d < 2; ++d) H += 0.5f * logf(17.079468445347132f * var[d]);
        }
    }
    if (!kEnt && logp_out) {
        logp_out[src] = lp;
        return;
    }
    const float dl = lp - logp_old[src];
    const float r = expf(dl);
    const float A = adv[src];
    const bool clipped = (A > 0.f && r > hi) || (A < 0.f && r < lo);
    const float c = clipped ? 0.f : -scale * A * r;
    if (kind == 1) {
        softmax_grad<kEnt>(o, nout, a, mx, ls, c, es, H);
    } else {
        for (int d = 0; d < 2; ++d) {
            o[d] = c * (diff[d] / var[d]) * omm[d];
            const float g = c * (-0.5f + diff[d] * diff[d] / (2.f * var[d])) * omv[d];
            o[2 + d] = kEnt ? g - 0.5f * es * omv[d] : g;
        }
    }
    const long long dst = (long long)i * Rc + m, plane = (long long)N * Rc;
    const float l = -scale * fminf(r * A, fminf(fmaxf(r, lo), hi) * A);
    L[dst] = kEnt ? l - es * H : l;
    S[dst] = clipped ? 1.f : 0.f;
    S[plane + dst] = -dl;
    S[2 * plane + dst] = r;
    if (kEnt) {
        E[dst] = H;
        if (Kp) Kp[dst] = fmaxf(expm1f(dl) - dl, 0.f);
    }
}

// The per-agent reductions' fixed order: every lane brings the partial sum of its strided elements, then ONE tree over the
// workgroup's kThreads partials (level w adds part[t + w] into part[t], w = kThreads / 2 .. 1), which leaves the total in part[0].
template <typename T>
__device__ __forceinline__ void block_sum(T (&part)[kThreads], T s)
{
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
}

// out[i] (+)= the chunk's sum over the rows of agent i of one per-row plane P [N][Rc], in block_sum's order; the first chunk
// writes, and with `last` the last chunk divides by `rows`: the per-agent loss (a sum: last = 0), the mean row entropy, the share
// of zero-gradient rows.  A gated agent (active[i] == 0, uniform over the workgroup) sums nothing: its value is NaN.
__global__ __launch_bounds__(kThreads) void row_sum_kernel(const float *P, long long Rc, int rc, int first, int last, float rows,
                                                           float *out, const int32_t *active)
{
    __shared__ float part[kThreads];
    const int i = blockIdx.x;
    if (active && active[i] == 0) {
        if (threadIdx.x == 0) out[i] = __builtin_nanf("");
        return;
    }
    float s = 0.f;
    for (int m = threadIdx.x; m < rc; m += kThreads) s += P[(long long)i * Rc + m];
    block_sum(part, s);
    if (threadIdx.x == 0) {
        s = first ? part[0] : out[i] + part[0];
        out[i] = last ? s / rows : s;
    }
}

// stats [4][N] of agent i over the chunks, in block_sum's order for all four values under one barrier per level: the clipped
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

// kl[i] = the mean of the head's k plane of agent i over the chunks, in block_sum's order with float64 partial sums: the
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
    block_sum(part, s);
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

// The sharing map's guards.  The members [beg, end) of group g, clamped to the N entries of `members`; false for an empty range.
__device__ __forceinline__ bool group_range(const int32_t *group_ptr, int g, int N, int &beg, int &end)
{
    beg = group_ptr[g];
    end = group_ptr[g + 1];
    if (beg < 0) beg = 0;
    if (end > N) end = N;
    return beg < end;
}

__device__ __forceinline__ bool agent_ok(int i, int N) { return (unsigned)i < (unsigned)N; }

// The agent that workgroup row b of the norm / Adam kernels serves: b itself, or under a sharing map (group_ptr set) the leader
// of group b; -1 for a map entry outside [0, N).
__device__ __forceinline__ int agent_of(int b, int N, const int32_t *group_ptr, const int32_t *members)
{
    if (!group_ptr) return b;
    const int at = group_ptr[b];
    if (!agent_ok(at, N)) return -1;
    const int i = members[at];
    return agent_ok(i, N) ? i : -1;
}

// dronesim_kl_gate_shared: one thread per group, kl_gate_kernel's rule on the group's estimate -- the mean of the members' kl,
// float64 partial sums in ascending member order from the leader's value -- with the verdict written to every member.  A
// singleton's mean is its own kl: kl_gate_kernel's test.
__global__ __launch_bounds__(kThreads) void kl_gate_shared_kernel(const float *kl, float target_kl, int32_t *active, int32_t *taken,
                                                                  int N, int reset, const int32_t *group_ptr, const int32_t *members,
                                                                  int n_groups)
{
    const int g = blockIdx.x * kThreads + threadIdx.x;
    int beg, end;
    if (g >= n_groups || !group_range(group_ptr, g, N, beg, end)) return;
    const int lead = members[beg];
    if (!agent_ok(lead, N)) return;
    int a = 1, tk = 0;
    if (!reset) {
        a = active[lead];
        tk = taken[lead];
        if (a) {
            double s = (double)kl[lead];
            for (int k = beg + 1; k < end; ++k) {
                const int i = members[k];
                if (agent_ok(i, N)) s += (double)kl[i];
            }
            if (!(s / (double)(end - beg) <= (double)target_kl)) a = 0;
        }
        if (a) tk += 1;
    }
    for (int k = beg; k < end; ++k) {
        const int i = members[k];
        if (!agent_ok(i, N)) continue;
        active[i] = a;
        taken[i] = tk;
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

// the pre-clip gradient norm of agent i over its six tensors (double partial sums, block_sum's order); advances the step counter
// (dronesim_adam_step_gated: an agent with active[i] == 0 keeps its counter and reports NaN).  Under a sharing map the agents
// are the groups' leaders (agent_of).
__global__ __launch_bounds__(kThreads) void grad_norm_kernel(const float *grad, Tensors t, int32_t *step, float *grad_norm,
                                                             const int32_t *active, int N, const int32_t *group_ptr,
                                                             const int32_t *members)
{
    __shared__ double part[kThreads];
    const int i = agent_of(blockIdx.x, N, group_ptr, members);
    if (i < 0) return;                           // (the whole workgroup, before any barrier)
    if (active && active[i] == 0) {
        if (threadIdx.x == 0) grad_norm[i] = __builtin_nanf("");
        return;
    }
    // Each lane adds the squares of its strided elements in element order.  The loads of kNormUnroll of them are issued before
    // the first is added: under a sharing map ONE workgroup walks a whole network, and the walk is bound by memory latency.
    // The order of the additions, and with it every bit of the sum, is that of the plain loop (a float's square is exact in
    // float64, so neither the batching nor a fused multiply-add can change a rounding).
    constexpr int kNormUnroll = 16;
    double s = 0.0;
    for (int j = 0; j < 6; ++j) {
        const float *g = grad + t.off[j] + (long long)i * t.size[j];
        long long e = threadIdx.x;
        for (; e + (kNormUnroll - 1) * kThreads < t.size[j]; e += kNormUnroll * kThreads) {
            float v[kNormUnroll];
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) v[u] = g[e + u * kThreads];
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) s += (double)v[u] * (double)v[u];
        }
        for (; e < t.size[j]; e += kThreads) s += (double)g[e] * (double)g[e];
    }
    block_sum(part, s);
    if (threadIdx.x == 0) {
        grad_norm[i] = (float)sqrt(part[0]);
        step[i] = step[i] + 1;
    }
}

// clip (coef = min(1, max_norm / (norm + 1e-6)), the clipped gradient is written back) and one Adam step, torch's formulas;
// the shared step's leaders go through this same kernel (agent_of): one set of instructions for both
__global__ __launch_bounds__(kThreads) void adam_kernel(float *grad, float *m1, float *m2, Params prm, Tensors t,
                                                        const int32_t *step, const float *grad_norm, float lr, float beta1,
                                                        float beta2, float eps, float max_norm, const int32_t *active, int N,
                                                        const int32_t *group_ptr, const int32_t *members)
{
    const int i = agent_of(blockIdx.y, N, group_ptr, members);
    if (i < 0) return;                           // (the whole workgroup, before the barrier)
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

// The element quads of the per-agent layout, the work items of the two group kernels: tensor j has ceil(size[j] / 4) of them,
// the last one possibly short.  quad q -> tensor j, first element e, cnt elements.
__host__ __device__ __forceinline__ long long quads_of(const Tensors &t)
{
    long long n = 0;
    for (int j = 0; j < 6; ++j) n += (t.size[j] + 3) >> 2;
    return n;
}

__device__ __forceinline__ void quad_at(const Tensors &t, long long q, int &j, long long &e, int &cnt)
{
    for (j = 0; j < 5; ++j) {
        const long long nq = (t.size[j] + 3) >> 2;
        if (q < nq) break;
        q -= nq;
    }
    e = 4 * q;
    const long long left = t.size[j] - e;
    cnt = left < 4 ? (int)left : 4;
}

// One quad from / to an agent's slice: <true> one 16-byte access (a whole quad at an aligned address), <false> element by
// element (a tensor's short last quad; slices that do not start on a 16-byte boundary).
template <bool kVec>
__device__ __forceinline__ float4 load_quad(const float *p, int cnt)
{
    if (kVec) return *reinterpret_cast<const float4 *>(p);
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (cnt == 4) {
        v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
        return v;
    }
    v.x = p[0];
    if (cnt > 1) v.y = p[1];
    if (cnt > 2) v.z = p[2];
    return v;
}

template <bool kVec>
__device__ __forceinline__ void store_quad(float *p, int cnt, float4 v)
{
    if (kVec) {
        *reinterpret_cast<float4 *>(p) = v;
        return;
    }
    p[0] = v.x;
    if (cnt > 1) p[1] = v.y;
    if (cnt > 2) p[2] = v.z;
    if (cnt > 3) p[3] = v.w;
}

// Whether the quad at `p` of EVERY agent's slice is one aligned 16-byte access: the quad is whole, this one is aligned, and the
// slices are a multiple of four floats apart.
__device__ __forceinline__ bool quad_is_vector(const float *p, long long stride, int cnt)
{
    return cnt == 4 && (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

constexpr int kGroupThreads = 64;       // small workgroups: one large group's quads still reach every compute unit
constexpr int kGroupUnroll = 8;         // members whose loads are in flight together (the sum itself stays in member order)

// The sum of one quad over the members [beg + 1, end) of a group on top of the leader's: float64 partial sums in ascending member
// order.  The loads of kGroupUnroll members are issued before the first of them is added -- the walk is bound by memory
// latency, the order of the additions is untouched.  A member outside [0, N) is read at the leader's address and not added.
template <bool kVec>
__device__ __forceinline__ void sum_quad(const float *base, long long stride, int cnt, int N, const int32_t *members, int beg, int end,
                                         int lead, double (&s)[4])
{
    const float4 v0 = load_quad<kVec>(base + (long long)lead * stride, cnt);
    s[0] = (double)v0.x; s[1] = (double)v0.y; s[2] = (double)v0.z; s[3] = (double)v0.w;
    int k = beg + 1;
    for (; k + kGroupUnroll <= end; k += kGroupUnroll) {
        float4 v[kGroupUnroll];
        bool ok[kGroupUnroll];
#pragma unroll
        for (int u = 0; u < kGroupUnroll; ++u) {
            const int i = members[k + u];
            ok[u] = agent_ok(i, N);
            v[u] = load_quad<kVec>(base + (long long)(ok[u] ? i : lead) * stride, cnt);
        }
#pragma unroll
        for (int u = 0; u < kGroupUnroll; ++u) {
            if (!ok[u]) continue;
            s[0] += (double)v[u].x; s[1] += (double)v[u].y; s[2] += (double)v[u].z; s[3] += (double)v[u].w;
        }
    }
    for (; k < end; ++k) {
        const int i = members[k];
        if (!agent_ok(i, N)) continue;
        const float4 v = load_quad<kVec>(base + (long long)i * stride, cnt);
        s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
    }
}

// The group mean of the shared step.  Grid (quad blocks, group): a thread owns one quad of the per-agent layout at a time
// (grid-stride over the quads) and walks the group's members for it -- consecutive lanes read consecutive quads of one member's
// slice --, so a group of any size is spread over the whole grid.  Per element: float64 partial sums in ascending member order
// from the first member's value, divided by (double)|G|, rounded once to float32, written into the LEADER's slice; the other
// members' slices are only read.  No atomics: one owner per element.  A singleton's mean is its own value (nothing to do); a
// stopped group (active[leader] == 0) is skipped.
__global__ __launch_bounds__(kGroupThreads) void group_mean_kernel(float *grad, Tensors t, int N, const int32_t *active,
                                                                   const int32_t *group_ptr, const int32_t *members)
{
    int beg, end;
    if (!group_range(group_ptr, blockIdx.y, N, beg, end)) return;
    const int lead = members[beg];
    if (end - beg == 1 || !agent_ok(lead, N)) return;
    if (active && active[lead] == 0) return;
    const double n = (double)(end - beg);
    const long long quads = quads_of(t);
    for (long long q = (long long)blockIdx.x * kGroupThreads + threadIdx.x; q < quads; q += (long long)gridDim.x * kGroupThreads) {
        int j, cnt;
        long long e;
        quad_at(t, q, j, e, cnt);
        float *base = grad + t.off[j] + e;
        float *out = base + (long long)lead * t.size[j];
        const bool vec = quad_is_vector(out, t.size[j], cnt);
        double s[4];
        if (vec) sum_quad<true>(base, t.size[j], cnt, N, members, beg, end, lead, s);
        else sum_quad<false>(base, t.size[j], cnt, N, members, beg, end, lead, s);
        const float4 mean = {(float)(s[0] / n), (float)(s[1] / n), (float)(s[2] / n), (float)(s[3] / n)};
        if (vec) store_quad<true>(out, cnt, mean);
        else store_quad<false>(out, cnt, mean);
    }
}

// The broadcast of the shared step and dronesim_mlp_tie: the leader's six weight tensors to every other member of its group, on
// group_mean_kernel's grid and quads; the group's first workgroup also mirrors the leader's pre-clip norm and step counter
// (either may be NULL: dronesim_mlp_tie).  A stopped group keeps its weights and counters, and all its members report the
// leader's NaN norm.
__global__ __launch_bounds__(kGroupThreads) void group_broadcast_kernel(Params prm, Tensors t, int N, int32_t *step, float *grad_norm,
                                                                        const int32_t *active, const int32_t *group_ptr,
                                                                        const int32_t *members)
{
    int beg, end;
    if (!group_range(group_ptr, blockIdx.y, N, beg, end)) return;
    const int lead = members[beg];
    if (end - beg == 1 || !agent_ok(lead, N)) return;
    const bool stopped = active && active[lead] == 0;
    if (blockIdx.x == 0) {
        for (int k = beg + 1 + (int)threadIdx.x; k < end; k += kGroupThreads) {
            const int i = members[k];
            if (!agent_ok(i, N)) continue;
            if (grad_norm) grad_norm[i] = grad_norm[lead];
            if (step && !stopped) step[i] = step[lead];
        }
    }
    if (stopped) return;
    const long long quads = quads_of(t);
    for (long long q = (long long)blockIdx.x * kGroupThreads + threadIdx.x; q < quads; q += (long long)gridDim.x * kGroupThreads) {
        int j, cnt;
        long long e;
        quad_at(t, q, j, e, cnt);
        float *base = prm.p[j] + e;
        const float *from = base + (long long)lead * t.size[j];
        const bool vec = quad_is_vector(from, t.size[j], cnt);
        const float4 v = vec ? load_quad<true>(from, cnt) : load_quad<false>(from, cnt);
        for (int k = beg + 1; k < end; ++k) {
            const int i = members[k];
            if (!agent_ok(i, N)) continue;
            if (vec) store_quad<true>(base + (long long)i * t.size[j], cnt, v);
            else store_quad<false>(base + (long long)i * t.size[j], cnt, v);
        }
    }
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

// One call of the chain: what to run (`form`) and every pointer and scalar the form reads; the rest stays zero.  The forms, i.e.
// the legal combinations of the option bits, and the network each takes:
//   0                        dronesim_mlp_grad             any kind     target (critic) or act + weight (actors)
//   kVclip                   dronesim_mlp_grad_vclip       critic       target, v_old, vf_clip -> clip_fraction [N]
//   kEnt                     dronesim_mlp_grad_ent         actor        act, weight, ent_scale -> entropy [N]
//   kLogp                    dronesim_mlp_logp             actor        act -> logp_out; forward + head only: no grad, no loss
//   kPpo                     dronesim_mlp_grad_ppo         actor        act, logp_old, adv, lo, hi -> stats [4][N]
//   kPpo | kEnt              dronesim_mlp_grad_ppo_ent     actor        + ent_scale -> stats [5][N]  (row 4: the mean row entropy)
//   kPpo | kEnt | kGate      dronesim_mlp_grad_ppo_gated   actor        + active (may be NULL) -> stats [6][N]  (row 5: kl)
enum Form : unsigned { kPpo = 1, kEnt = 2, kGate = 4, kVclip = 8, kLogp = 16 };

struct ChainJob {
    unsigned form;
    const DroneMlp *m;
    const float *x;
    int R, rows_per_chunk;
    float row_scale;
    float *grad, *loss;
    const float *target, *act, *weight;
    const float *v_old; float vf_clip; float *clip_fraction;
    float ent_scale; float *entropy;
    float *logp_out;
    const float *logp_old, *adv; float lo, hi; float *stats;
    const int32_t *active;
    void *ws;
    hipStream_t st;
};

// The workspace of a form at Rc rows per chunk, offsets in floats: the activations H1 [N][Rc][h1], H2 [N][Rc][h2], O [N][Rc][nout],
// the per-row losses L [N][Rc], and behind them the form's per-row planes [N][Rc] -- S: the PPO head's three diagnostics, or the
// one plane of kVclip's zero-gradient flags; En: the row entropies; Kp: the gated form's k, and Kacc: its N float64 running sums
// (Rc is a multiple of 64, so Kacc is 8-byte aligned where the workspace is).  A plane the form lacks has no extent.
struct Layout {
    size_t H1, H2, O, L, S, En, Kp, Kacc;
    size_t bytes;
};

Layout layout_of(const DroneMlp *m, int rows_per_chunk, unsigned form)
{
    const size_t plane = (size_t)m->N * (size_t)rows_per_chunk;
    Layout y;
    size_t at = 0;
    y.H1 = at; at += plane * (size_t)m->h1;
    y.H2 = at; at += plane * (size_t)m->h2;
    y.O = at; at += plane * (size_t)m->nout;
    y.L = at; at += plane;
    y.S = at; at += plane * ((form & kPpo) ? 3 : (form & kVclip) ? 1 : 0);
    y.En = at; at += (form & kEnt) ? plane : 0;
    y.Kp = at; at += (form & kGate) ? plane : 0;
    y.Kacc = at;
    y.bytes = sizeof(float) * at + ((form & kGate) ? sizeof(double) * (size_t)m->N : 0);
    return y;
}

// The chunked chain of the header comment over all R rows; the job validated by the entry points.
int run_chain(const ChainJob &j)
{
    const DroneMlp *m = j.m;
    const int N = m->N, din = m->d_in, h1 = m->h1, h2 = m->h2, no = m->nout, R = j.R;
    const long long Rc = j.rows_per_chunk;
    const bool ppo = j.form & (kPpo | kLogp), ent = j.form & kEnt, gate = j.form & kGate, vclip = j.form & kVclip;
    const Tensors t = tensors_of(m);
    // (kLogp touches neither grad nor loss; the workspace stands in for the gradient's base address)
    float *grad = (j.form & kLogp) ? (float *)j.ws : j.grad;
    float *gw1 = grad + t.off[0], *gb1 = grad + t.off[1], *gw2 = grad + t.off[2];
    float *gb2 = grad + t.off[3], *gw3 = grad + t.off[4], *gb3 = grad + t.off[5];
    const Layout y = layout_of(m, j.rows_per_chunk, j.form);
    float *W = (float *)j.ws;
    float *H1 = W + y.H1, *H2 = W + y.H2, *O = W + y.O, *L = W + y.L, *S = W + y.S, *En = W + y.En;
    float *Kp = gate ? W + y.Kp : nullptr;
    double *Kacc = (double *)(W + y.Kacc);
    // the three PPO forms keep their per-agent results in one array: stats [4][N], then the entropy row, then the kl row
    float *entropy = (j.form & kPpo) ? j.stats + 4 * (size_t)N : j.entropy, *kl = gate ? j.stats + 5 * (size_t)N : nullptr;
    const int32_t *active = gate ? j.active : nullptr;
    hipStream_t st = j.st;

    const long long xs = (long long)N * din;      // row stride of x
    for (long long r0 = 0; r0 < R; r0 += Rc) {
        const int rc = (int)((R - r0) < Rc ? (R - r0) : Rc);
        const int first = r0 == 0, last = r0 + Rc >= R;
        const float *X = j.x + r0 * xs;
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
        if (ppo)
            hipLaunchKernelGGL((ent ? ppo_head_kernel<true> : ppo_head_kernel<false>), hgrid, dim3(kThreads), 0, st, O, L, S, En, Rc,
                               rc, r0, N, no, m->out_kind, j.row_scale, j.ent_scale, j.act, j.logp_old, j.adv, j.lo, j.hi, active, Kp,
                               j.logp_out);
        else
            hipLaunchKernelGGL((ent ? a2c_head_kernel<true> : a2c_head_kernel<false>), hgrid, dim3(kThreads), 0, st, O, L,
                               ent ? En : S, Rc, rc, r0, N, no, m->out_kind, j.row_scale, j.ent_scale, j.target, j.act, j.weight,
                               j.v_old, j.vf_clip);
        if (j.form & kLogp) continue;
        // layer 3: dW3 += H2^T dO (+ db3), then dH2 = (dO W3^T) . [H2 > 0] in place of H2
        g = gemm(H2, 1, h2, Rc * h2, O, no, 1, Rc * no, gw3, no, (long long)h2 * no, h2 + 1, no, rc, kAccumulate);
        g.ones_row = h2; g.Cb = gb3; g.bCb = no; g.first = first;
        if (m->out_kind == 2) { g.half_m = h2 / 2; g.half_n = no / 2; }
        launch_gemm(g, N, st, active);
        g = gemm(O, no, 1, Rc * no, m->w3, 1, no, (long long)h2 * no, H2, h2, Rc * h2, rc, h2, no, kMask);
        launch_gemm(g, N, st, active);
        // layer 2: dW2 += H1^T dH2 (+ db2), then dH1 = (dH2 W2^T) . [H1 > 0] in place of H1
        g = gemm(H1, 1, h1, Rc * h1, H2, h2, 1, Rc * h2, gw2, h2, (long long)h1 * h2, h1 + 1, h2, rc, kAccumulate);
        g.ones_row = h1; g.Cb = gb2; g.bCb = h2; g.first = first;
        launch_gemm(g, N, st, active);
        g = gemm(H2, h2, 1, Rc * h2, m->w2, 1, h2, (long long)h1 * h2, H1, h1, Rc * h1, rc, h1, h2, kMask);
        launch_gemm(g, N, st, active);
        // layer 1: dW1 += X^T dH1 (+ db1)
        g = gemm(X, 1, xs, din, H1, h1, 1, Rc * h1, gw1, h1, (long long)din * h1, din + 1, h1, rc, kAccumulate);
        g.ones_row = din; g.Cb = gb1; g.bCb = h1; g.first = first;
        launch_gemm(g, N, st, active);
        // the per-agent results
        const dim3 agents(N), block(kThreads);
        hipLaunchKernelGGL(row_sum_kernel, agents, block, 0, st, L, Rc, rc, first, 0, (float)R, j.loss, active);
        if (j.form & kPpo) hipLaunchKernelGGL(ppo_stats_kernel, agents, block, 0, st, S, Rc, rc, N, first, last, (float)R, j.stats, active);
        if (ent) hipLaunchKernelGGL(row_sum_kernel, agents, block, 0, st, En, Rc, rc, first, last, (float)R, entropy, active);
        if (gate) hipLaunchKernelGGL(kl_sum_kernel, agents, block, 0, st, Kp, Rc, rc, first, last, (double)R, Kacc, kl, active);
        if (vclip) hipLaunchKernelGGL(row_sum_kernel, agents, block, 0, st, S, Rc, rc, first, last, (float)R, j.clip_fraction, active);
    }
    return dronesim_launched();
}

int check_mlp(const DroneMlp *m, const char *where)
{
    if (!m) return fail_at(where, "NULL DroneMlp");
    if (m->w2_layout != 0) return fail_at(where, "the learner reads the plain weight arrays (w2_layout = 0)");
    if (m->N < 1 || m->d_in < 1 || m->d_in > 64 || m->h1 < 1 || m->h1 > 4096 || m->h2 < 1 || m->h2 > 4096 || m->nout < 1 || m->nout > 32)
        return fail_at(where, "need N >= 1, 1 <= d_in <= 64, 1 <= h1, h2 <= 4096, 1 <= nout <= 32");
    if ((m->out_kind == 0 && m->nout != 1) || (m->out_kind == 1 && m->nout < 2) ||
        (m->out_kind == 2 && (m->nout != 4 || m->h2 % 2 != 0)) || m->out_kind < 0 || m->out_kind > 2)
        return fail_at(where, "out_kind 0 needs nout = 1, 1 nout >= 2, 2 nout = 4 and an even h2");
    if (!m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->w3 || !m->b3) return fail_at(where, "NULL weight array");
    return DRONESIM_OK;
}

// The checks every chain entry point shares: the network and its kind for the form (ChainJob's table), R, the chunk size, and --
// with `ws_bytes` set, i.e. for a call and not a workspace query -- the workspace's size and, where the form keeps float64 in
// it, its alignment.
int check_call(const char *where, const DroneMlp *m, unsigned form, int R, int rows_per_chunk, const void *ws, const size_t *ws_bytes)
{
    const int rc = check_mlp(m, where);
    if (rc != DRONESIM_OK) return rc;
    if ((form & kVclip) && m->out_kind != 0) return fail_at(where, "needs a critic (out_kind 0), not an actor");
    if ((form & ~kVclip) && m->out_kind == 0) return fail_at(where, "needs an actor (out_kind 1 or 2), not a critic");
    if (R < 1) return fail_at(where, "R < 1");
    if (rows_per_chunk < 64 || rows_per_chunk % 64 != 0) return fail_at(where, "rows_per_chunk must be a positive multiple of 64");
    if (!ws_bytes) return DRONESIM_OK;
    if (*ws_bytes < layout_of(m, rows_per_chunk, form).bytes) {
        char what[120];
        snprintf(what, sizeof what, "workspace smaller than %s_workspace()", form == kLogp ? "dronesim_mlp_grad" : where);
        return fail_at(where, what);
    }
    if ((form & kGate) && (reinterpret_cast<uintptr_t>(ws) & 7u)) return fail_at(where, "workspace not 8-byte aligned");
    return DRONESIM_OK;
}

int workspace_query(const char *where, const DroneMlp *m, unsigned form, int rows_per_chunk, size_t *bytes)
{
    const int rc = check_call(where, m, form, 1, rows_per_chunk, nullptr, nullptr);
    if (rc != DRONESIM_OK) return rc;
    if (!bytes) return fail_at(where, "NULL bytes");
    *bytes = layout_of(m, rows_per_chunk, form).bytes;
    return DRONESIM_OK;
}

bool bad_ent_scale(float ent_scale) { return !(ent_scale >= 0.f) || isinf(ent_scale); }

// the three PPO gradient forms: dronesim_mlp_grad_ppo (form kPpo), _ppo_ent (| kEnt) and _ppo_gated (| kEnt | kGate)
int ppo_grad(const char *where, unsigned form, const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
             const float *logp_old, const float *adv, float clip_eps, float ent_scale, const int32_t *active, float *grad, float *loss,
             float *stats, int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    const int rc = check_call(where, m, form, R, rows_per_chunk, ws, &ws_bytes);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !logp_old || !adv || !grad || !loss || !stats || !ws)
        return fail_at(where, "NULL x / act / logp_old / adv / grad / loss / stats / workspace");
    if (!(clip_eps > 0.f && clip_eps < 1.f)) return fail_at(where, "clip_eps must be in (0, 1)");
    if ((form & kEnt) && bad_ent_scale(ent_scale)) return fail_at(where, "ent_scale must be finite and >= 0");
    ChainJob j = {};
    j.form = form; j.m = m; j.x = x; j.R = R; j.rows_per_chunk = rows_per_chunk; j.row_scale = row_scale;
    j.grad = grad; j.loss = loss; j.act = act; j.logp_old = logp_old; j.adv = adv; j.lo = 1.f - clip_eps; j.hi = 1.f + clip_eps;
    j.stats = stats; j.ent_scale = ent_scale; j.active = active; j.ws = ws; j.st = (hipStream_t)stream;
    return run_chain(j);
}

Params params_of(const DroneMlp *m)
{
    Params p;
    const float *w[6] = {m->w1, m->b1, m->w2, m->b2, m->w3, m->b3};
    for (int j = 0; j < 6; ++j) p.p[j] = const_cast<float *>(w[j]);
    return p;
}

// the grid of the two group kernels: x over the quads of the per-agent layout in workgroups of kGroupThreads -- capped so that
// all groups together stay near 8192 of them, the kernels stride over the rest --, y the group
dim3 group_grid(const Tensors &t, int n_groups)
{
    const long long want = (quads_of(t) + kGroupThreads - 1) / kGroupThreads, cap = (8192 + n_groups - 1) / n_groups;
    return dim3((unsigned)(want < cap ? want : cap), (unsigned)n_groups);
}

int check_groups(const char *where, int N, const int32_t *group_ptr, const int32_t *members, int n_groups)
{
    if (!group_ptr || !members) return fail_at(where, "NULL group_ptr / members");
    if (n_groups < 1 || n_groups > N) return fail_at(where, "n_groups must be in [1, N]");
    return DRONESIM_OK;
}

// The three Adam entry points.  group_ptr NULL: one norm and one Adam workgroup row per agent; else one per group (its leader),
// between the group mean and the broadcast.
int adam_step(const char *where, const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
              float beta2, float eps, float max_norm, float *grad_norm, const int32_t *active, const int32_t *group_ptr,
              const int32_t *members, int n_groups, void *stream)
{
    int rc = check_mlp(m, where);
    if (rc != DRONESIM_OK) return rc;
    if (!grad || !m1 || !m2 || !step || !grad_norm) return fail_at(where, "NULL grad / m1 / m2 / step / grad_norm");
    if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(max_norm > 0.f))
        return fail_at(where, "need lr >= 0, 0 <= beta < 1, eps > 0, max_norm > 0");
    hipStream_t st = (hipStream_t)stream;
    const Tensors t = tensors_of(m);
    const Params p = params_of(m);
    const int rows = group_ptr ? n_groups : m->N;
    if (group_ptr)
        hipLaunchKernelGGL(group_mean_kernel, group_grid(t, n_groups), dim3(kGroupThreads), 0, st, grad, t, m->N, active, group_ptr, members);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(rows), dim3(kThreads), 0, st, grad, t, step, grad_norm, active, m->N, group_ptr, members);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((t.per_agent + kThreads - 1) / kThreads), rows), dim3(kThreads), 0, st,
                       grad, m1, m2, p, t, step, grad_norm, lr, beta1, beta2, eps, max_norm, active, m->N, group_ptr, members);
    if (group_ptr)
        hipLaunchKernelGGL(group_broadcast_kernel, group_grid(t, n_groups), dim3(kGroupThreads), 0, st, p, t, m->N, step, grad_norm, active,
                           group_ptr, members);
    return dronesim_launched();
}

}  // namespace

extern "C" int dronesim_mlp_grad_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    return workspace_query("dronesim_mlp_grad_workspace", m, 0, rows_per_chunk, bytes);
}

extern "C" int dronesim_mlp_grad_vclip_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    return workspace_query("dronesim_mlp_grad_vclip_workspace", m, kVclip, rows_per_chunk, bytes);
}

extern "C" int dronesim_mlp_grad_ent_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    return workspace_query("dronesim_mlp_grad_ent_workspace", m, kEnt, rows_per_chunk, bytes);
}

extern "C" int dronesim_mlp_grad_ppo_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    return workspace_query("dronesim_mlp_grad_ppo_workspace", m, kPpo, rows_per_chunk, bytes);
}

extern "C" int dronesim_mlp_grad_ppo_ent_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    return workspace_query("dronesim_mlp_grad_ppo_ent_workspace", m, kPpo | kEnt, rows_per_chunk, bytes);
}

extern "C" int dronesim_mlp_grad_ppo_gated_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes)
{
    return workspace_query("dronesim_mlp_grad_ppo_gated_workspace", m, kPpo | kEnt | kGate, rows_per_chunk, bytes);
}

extern "C" int dronesim_mlp_grad(const DroneMlp *m, const float *x, int R, float row_scale, const float *target, const float *act,
                                 const float *weight, float *grad, float *loss, int rows_per_chunk, void *ws, size_t ws_bytes,
                                 void *stream)
{
    const char *where = "dronesim_mlp_grad";
    const int rc = check_call(where, m, 0, R, rows_per_chunk, ws, &ws_bytes);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !grad || !loss || !ws) return fail_at(where, "NULL x / grad / loss / workspace");
    if (m->out_kind == 0 && !target) return fail_at(where, "the critic loss needs target");
    if (m->out_kind != 0 && (!act || !weight)) return fail_at(where, "the actor loss needs act and weight");
    ChainJob j = {};
    j.m = m; j.x = x; j.R = R; j.rows_per_chunk = rows_per_chunk; j.row_scale = row_scale; j.grad = grad; j.loss = loss;
    j.target = target; j.act = act; j.weight = weight; j.ws = ws; j.st = (hipStream_t)stream;
    return run_chain(j);
}

extern "C" int dronesim_mlp_grad_vclip(const DroneMlp *m, const float *x, int R, float row_scale, const float *target,
                                       const float *v_old, float vf_clip, float *grad, float *loss, float *clip_fraction,
                                       int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    const char *where = "dronesim_mlp_grad_vclip";
    const int rc = check_call(where, m, kVclip, R, rows_per_chunk, ws, &ws_bytes);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !target || !v_old || !grad || !loss || !clip_fraction || !ws)
        return fail_at(where, "NULL x / target / v_old / grad / loss / clip_fraction / workspace");
    if (!(vf_clip > 0.f)) return fail_at(where, "vf_clip must be > 0 (finite, or +inf: never clamped)");
    ChainJob j = {};
    j.form = kVclip; j.m = m; j.x = x; j.R = R; j.rows_per_chunk = rows_per_chunk; j.row_scale = row_scale; j.grad = grad;
    j.loss = loss; j.target = target; j.v_old = v_old; j.vf_clip = vf_clip; j.clip_fraction = clip_fraction; j.ws = ws;
    j.st = (hipStream_t)stream;
    return run_chain(j);
}

extern "C" int dronesim_mlp_grad_ent(const DroneMlp *m, const float *x, int R, float row_scale, const float *act, const float *weight,
                                     float ent_scale, float *grad, float *loss, float *entropy, int rows_per_chunk, void *ws,
                                     size_t ws_bytes, void *stream)
{
    const char *where = "dronesim_mlp_grad_ent";
    const int rc = check_call(where, m, kEnt, R, rows_per_chunk, ws, &ws_bytes);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !weight || !grad || !loss || !entropy || !ws)
        return fail_at(where, "NULL x / act / weight / grad / loss / entropy / workspace");
    if (bad_ent_scale(ent_scale)) return fail_at(where, "ent_scale must be finite and >= 0");
    ChainJob j = {};
    j.form = kEnt; j.m = m; j.x = x; j.R = R; j.rows_per_chunk = rows_per_chunk; j.row_scale = row_scale; j.grad = grad;
    j.loss = loss; j.act = act; j.weight = weight; j.ent_scale = ent_scale; j.entropy = entropy; j.ws = ws;
    j.st = (hipStream_t)stream;
    return run_chain(j);
}

extern "C" int dronesim_mlp_logp(const DroneMlp *m, const float *x, int R, const float *act, float *logp, int rows_per_chunk,
                                 void *ws, size_t ws_bytes, void *stream)
{
    const char *where = "dronesim_mlp_logp";
    const int rc = check_call(where, m, kLogp, R, rows_per_chunk, ws, &ws_bytes);
    if (rc != DRONESIM_OK) return rc;
    if (!x || !act || !logp || !ws) return fail_at(where, "NULL x / act / logp / workspace");
    ChainJob j = {};
    j.form = kLogp; j.m = m; j.x = x; j.R = R; j.rows_per_chunk = rows_per_chunk; j.row_scale = 1.f; j.act = act;
    j.logp_out = logp; j.ws = ws; j.st = (hipStream_t)stream;
    return run_chain(j);
}

extern "C" int dronesim_mlp_grad_ppo(const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
                                     const float *logp_old, const float *adv, float clip_eps, float *grad, float *loss, float *stats,
                                     int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    return ppo_grad("dronesim_mlp_grad_ppo", kPpo, m, x, R, row_scale, act, logp_old, adv, clip_eps, 0.f, nullptr, grad, loss, stats,
                    rows_per_chunk, ws, ws_bytes, stream);
}

extern "C" int dronesim_mlp_grad_ppo_ent(const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
                                         const float *logp_old, const float *adv, float clip_eps, float ent_scale, float *grad,
                                         float *loss, float *stats, int rows_per_chunk, void *ws, size_t ws_bytes, void *stream)
{
    return ppo_grad("dronesim_mlp_grad_ppo_ent", kPpo | kEnt, m, x, R, row_scale, act, logp_old, adv, clip_eps, ent_scale, nullptr,
                    grad, loss, stats, rows_per_chunk, ws, ws_bytes, stream);
}

extern "C" int dronesim_mlp_grad_ppo_gated(const DroneMlp *m, const float *x, int R, float row_scale, const float *act,
                                           const float *logp_old, const float *adv, float clip_eps, float ent_scale,
                                           const int32_t *active, float *grad, float *loss, float *stats, int rows_per_chunk,
                                           void *ws, size_t ws_bytes, void *stream)
{
    return ppo_grad("dronesim_mlp_grad_ppo_gated", kPpo | kEnt | kGate, m, x, R, row_scale, act, logp_old, adv, clip_eps, ent_scale,
                    active, grad, loss, stats, rows_per_chunk, ws, ws_bytes, stream);
}

extern "C" int dronesim_adam_step(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                                  float beta2, float eps, float max_norm, float *grad_norm, void *stream)
{
    return adam_step("dronesim_adam_step", m, grad, m1, m2, step, lr, beta1, beta2, eps, max_norm, grad_norm, nullptr, nullptr, nullptr,
                     0, stream);
}

extern "C" int dronesim_adam_step_gated(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                                        float beta2, float eps, float max_norm, float *grad_norm, const int32_t *active,
                                        void *stream)
{
    const char *where = "dronesim_adam_step_gated";
    if (!active) return fail_at(where, "NULL active");
    return adam_step(where, m, grad, m1, m2, step, lr, beta1, beta2, eps, max_norm, grad_norm, active, nullptr, nullptr, 0, stream);
}

extern "C" int dronesim_adam_step_shared(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                                         float beta2, float eps, float max_norm, float *grad_norm, const int32_t *active,
                                         const int32_t *group_ptr, const int32_t *members, int n_groups, void *stream)
{
    const char *where = "dronesim_adam_step_shared";
    int rc = check_mlp(m, where);
    if (rc == DRONESIM_OK) rc = check_groups(where, m->N, group_ptr, members, n_groups);
    if (rc != DRONESIM_OK) return rc;
    return adam_step(where, m, grad, m1, m2, step, lr, beta1, beta2, eps, max_norm, grad_norm, active, group_ptr, members, n_groups,
                     stream);
}

extern "C" int dronesim_mlp_tie(const DroneMlp *m, const int32_t *group_ptr, const int32_t *members, int n_groups, void *stream)
{
    const char *where = "dronesim_mlp_tie";
    int rc = check_mlp(m, where);
    if (rc == DRONESIM_OK) rc = check_groups(where, m->N, group_ptr, members, n_groups);
    if (rc != DRONESIM_OK) return rc;
    const Tensors t = tensors_of(m);
    hipLaunchKernelGGL(group_broadcast_kernel, group_grid(t, n_groups), dim3(kGroupThreads), 0, (hipStream_t)stream, params_of(m), t, m->N,
                       (int32_t *)nullptr, (float *)nullptr, (const int32_t *)nullptr, group_ptr, members);
    return dronesim_launched();
}

extern "C" int dronesim_kl_gate(const float *kl, float target_kl, int32_t *active, int32_t *taken, int N, int reset, void *stream)
{
    const char *where = "dronesim_kl_gate";
    if (N < 1) return fail_at(where, "N < 1");
    if (!active || !taken) return fail_at(where, "NULL active / taken");
    if (!reset && !kl) return fail_at(where, "NULL kl (only reset may omit it)");
    if (!(target_kl > 0.f) || isinf(target_kl)) return fail_at(where, "target_kl must be finite and > 0");
    hipLaunchKernelGGL(kl_gate_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, kl,
                       target_kl, active, taken, N, reset);
    return dronesim_launched();
}

extern "C" int dronesim_kl_gate_shared(const float *kl, float target_kl, int32_t *active, int32_t *taken, int N, int reset,
                                       const int32_t *group_ptr, const int32_t *members, int n_groups, void *stream)
{
    const char *where = "dronesim_kl_gate_shared";
    if (N < 1) return fail_at(where, "N < 1");
    if (!active || !taken) return fail_at(where, "NULL active / taken");
    if (!reset && !kl) return fail_at(where, "NULL kl (only reset may omit it)");
    if (!(target_kl > 0.f) || isinf(target_kl)) return fail_at(where, "target_kl must be finite and > 0");
    const int rc = check_groups(where, N, group_ptr, members, n_groups);
    if (rc != DRONESIM_OK) return rc;
    hipLaunchKernelGGL(kl_gate_shared_kernel, dim3((unsigned)((n_groups + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, kl, target_kl, active, taken, N, reset, group_ptr, members, n_groups);
    return dronesim_launched();
}
