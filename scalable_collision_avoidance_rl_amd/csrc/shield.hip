// Action shield (dronesim_action_shield): a local collision-avoidance filter between the policy and the step.  Per record (e, i)
// the nominal action u is replaced by its Euclidean projection u* onto the intersection of at most 12 half-planes a.x <= b, in
// this fixed order (include/dronesim.h states the rule; DESIGN.md the guarantee):
//   0..3       the box (+1,0), (-1,0), (0,+1), (0,-1), b = u_max  (the per-component clip of the controllers and policies)
//   4..4+k-1   slot s = 1..k of the agent's own observation: j = nbr[s], p = floats 0, 1 of row s (x_j - x_i), d = |p|; skipped
//              unless 0 <= j < N, j != i, d finite and > 0;  a = p / d,  b = rate max(d - radius[i] - radius[j] - margin, 0) / dt
// 0 satisfies every constraint, so the set is never empty.
//
// One thread per record, consecutive threads on consecutive records: every 64-byte segment of z, nbr and act is fetched once.  The
// loads of a record are as wide as c, the parity of k + 1 and the base address allow -- episode_safety_kernel<W>'s rule
// (evaluate.hip):
//   W = 4   c = 2, k1 even, z 16-byte aligned: the record (8 k1 bytes) as k1 / 2 16-byte loads, rows 2h and 2h + 1 each
//   W = 2   c = 2, z 8-byte aligned: one 8-byte load per row 1..k
//   W = 1   anything else: two dword loads per row (c = 5: rows start at multiples of 20 bytes)
// The solve inserts the constraints one at a time (Seidel's order, the objective |x - u|^2 instead of a linear one): while the
// current point satisfies the new half-plane nothing happens; where it violates it, the new optimum lies on the new line, and it is
// the projection of u onto that line clipped to the interval the earlier half-planes leave there.  At most 66 interval updates of
// a few instructions each, only in the lanes that violate, instead of 66 vertices x 12 tests in every lane of the wave.  A lane
// whose u satisfies all constraints leaves before the solve with u's own bits.  Every array below is indexed by unrolled loop
// counters only: registers, no scratch, no LDS.
// dronesim_action_shield_obstacles appends up to four half-planes of static discs (slots of dronesim_obstacle_sense's list, csrc/
// obstacles.hip) behind the neighbour slots: the set-up and the solve are device functions templated on the capacity of the
// constraint set (12 and 16), so both entries run ONE solver and the plain entry keeps its bits.
// dronesim_shield_totals folds the per-call planes into per-agent running totals in a fixed order, without float atomics.
#include "record_entry.hpp"

namespace {

constexpr int kShieldSlots = DRONESIM_MAX_K;                   // neighbour constraints a record can hold
constexpr int kShieldBox = 4;
constexpr int kShieldM = kShieldBox + kShieldSlots;
constexpr int kShieldObstacles = DRONESIM_MAX_SENSE;           // obstacle constraints a record can hold (dronesim_action_shield_obstacles)
constexpr int kShieldAll = kShieldM + kShieldObstacles;
// |a_j . t_i| at or below this counts as parallel (2^-21): such a line bounds nothing on line i that it did not bound before
// (both b >= 0: see DESIGN.md), and dividing by it would turn rounding noise into an interval end
constexpr float kShieldParallel = 4.76837158203125e-07f;
// Every earlier neighbour half-plane is relaxed on line m by kShieldNoise (4 b_m + min(|ux| + |uy|, 2 u_max)) -- 2 eps32 of the terms that num
// and s den are computed from at the ends that can clip s0 wrongly or be the answer inside the box: a violation of that size is
// rounding, not geometry, and at a small angle its end num / den lies anywhere on the line
constexpr float kShieldNoise = 1.1920928955078125e-07f;

typedef float sh_f4 __attribute__((ext_vector_type(4)));
typedef float sh_f2 __attribute__((ext_vector_type(2)));

struct ShieldArgs {
    const float *z;
    const int32_t *nbr;
    const float *act, *radius;
    float *act_out;
    uint8_t *intervened;
    float *correction;
    float rate_dt, margin, u_max;                              // rate_dt = rate / dt, rounded once on the host
    int N, k1, c, act8;                                        // act8: act and act_out are 8-byte aligned
    unsigned long long records;
};

// floats 0, 1 of rows 1..k of one record -> px[s - 1], py[s - 1]; rows at or beyond k1 stay 0 (d = 0: skipped)
template <int W>
__device__ __forceinline__ void shield_rows(const float *__restrict__ rec, int k1, int c, float (&px)[kShieldSlots], float (&py)[kShieldSlots])
{
#pragma unroll
    for (int q = 0; q < kShieldSlots; ++q) px[q] = py[q] = 0.0f;
    if (W == 4) {                                              // k1 even, at most 8: row 0 comes with row 1
#pragma unroll
        for (int h = 0; h < kShieldSlots / 2; ++h) {
            if (2 * h < k1) {                                  // (wave-uniform)
                const sh_f4 v = *reinterpret_cast<const sh_f4 *>(rec + 4 * h);
                if (h > 0) { px[2 * h - 1] = v.x; py[2 * h - 1] = v.y; }
                px[2 * h] = v.z; py[2 * h] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int s = 1; s <= kShieldSlots; ++s) {
            if (s < k1) {
                if (W == 2) {
                    const sh_f2 v = *reinterpret_cast<const sh_f2 *>(rec + 2 * s);
                    px[s - 1] = v.x; py[s - 1] = v.y;
                } else {
                    px[s - 1] = rec[s * c]; py[s - 1] = rec[s * c + 1];
                }
            }
        }
    }
}

// The first 4 + kShieldSlots half-planes of a record -- the box, then slots 1..k of its observation -- into a set of capacity CAP;
// a slot the record does not have is a = 0, b = +inf: never violated, never clips.  Returns radius[i].
template <int W, int CAP>
__device__ __forceinline__ float shield_constraints(const ShieldArgs &a, unsigned long long r, int i, float (&ax)[CAP],
                                                    float (&ay)[CAP], float (&b)[CAP])
{
    static_assert(CAP >= kShieldM, "the box and the neighbour slots come first");
    const int N = a.N, k1 = a.k1;
    float px[kShieldSlots], py[kShieldSlots];
    int nj[kShieldSlots];
    shield_rows<W>(a.z + r * (unsigned long long)(k1 * a.c), k1, a.c, px, py);
    const int32_t *nb = a.nbr + r * (unsigned long long)k1;
#pragma unroll
    for (int s = 1; s <= kShieldSlots; ++s) nj[s - 1] = s < k1 ? nb[s] : -1;
    const float ri = a.radius[i];

    const float inf = __builtin_inff();
    ax[0] = 1.0f; ay[0] = 0.0f; ax[1] = -1.0f; ay[1] = 0.0f; ax[2] = 0.0f; ay[2] = 1.0f; ax[3] = 0.0f; ay[3] = -1.0f;
    b[0] = b[1] = b[2] = b[3] = a.u_max;
#pragma unroll
    for (int q = 0; q < kShieldSlots; ++q) {
        ax[kShieldBox + q] = ay[kShieldBox + q] = 0.0f;                               // a = 0, b = +inf: never violated, never clips
        b[kShieldBox + q] = inf;
        if (q + 1 < k1) {                                                             // (wave-uniform: rows the record has)
            const int j = nj[q];
            const float d = __builtin_sqrtf(fmaf(py[q], py[q], px[q] * px[q]));
            const bool on = (unsigned)j < (unsigned)N && j != i && d > 0.0f && d < inf;   // a ghost id never indexes radius; NaN: off
            const float rj = a.radius[on ? j : i];
            const float inv = 1.0f / d;
            const float g = ((d - ri) - rj) - a.margin;
            ax[kShieldBox + q] = on ? px[q] * inv : 0.0f;
            ay[kShieldBox + q] = on ? py[q] * inv : 0.0f;
            b[kShieldBox + q] = on ? a.rate_dt * fmaxf(g, 0.0f) : inf;
        }
    }
    return ri;
}

// Slots 0..m-1 of the record's obstacle list (dronesim_obstacle_sense: (p.x, p.y, r) and the disc's id) into entries kShieldM +
// s: a disc is a neighbour that does not move, with a rate of its own.
struct ShieldObstacles {
    const float *orow;
    const int32_t *oid;
    float rate_dt;                                             // obstacle_rate / dt, rounded once on the host
    int m, M;
};

template <int CAP>
__device__ __forceinline__ void shield_obstacle_constraints(const ShieldObstacles &ob, unsigned long long r, float ri, float margin,
                                                            float (&ax)[CAP], float (&ay)[CAP], float (&b)[CAP])
{
    static_assert(CAP == kShieldM + kShieldObstacles, "the obstacle slots come behind the neighbour slots");
    const float inf = __builtin_inff();
    const float *row = ob.orow + r * (unsigned long long)(3 * ob.m);
    const int32_t *id = ob.oid + r * (unsigned long long)ob.m;
#pragma unroll
    for (int s = 0; s < kShieldObstacles; ++s) {
        ax[kShieldM + s] = ay[kShieldM + s] = 0.0f;                                   // a = 0, b = +inf: never violated, never clips
        b[kShieldM + s] = inf;
        if (s < ob.m) {                                                               // (wave-uniform)
            const float px = row[3 * s], py = row[3 * s + 1], ro = row[3 * s + 2];
            const int o = id[s];
            const float d = __builtin_sqrtf(fmaf(py, py, px * px));
            const bool on = (unsigned)o < (unsigned)ob.M && d > 0.0f && d < inf;
            const float inv = 1.0f / d;
            const float g = ((d - ri) - ro) - margin;
            ax[kShieldM + s] = on ? px * inv : 0.0f;
            ay[kShieldM + s] = on ? py * inv : 0.0f;
            b[kShieldM + s] = on ? ob.rate_dt * fmaxf(g, 0.0f) : inf;
        }
    }
}

// The projection of (ux, uy) onto the entries m < M and kShieldM <= m < kShieldM + MO of a set of capacity CAP (the entries in
// between are rows the record does not have), and the stores of one record.
template <int CAP>
__device__ __forceinline__ void shield_solve_store(const ShieldArgs &a, unsigned long long r, float ux, float uy, const int M, const int MO,
                                                   const float (&ax)[CAP], const float (&ay)[CAP], const float (&b)[CAP])
{
    const float inf = __builtin_inff();
    const bool finite = __builtin_fabsf(ux) < inf && __builtin_fabsf(uy) < inf;
    bool violated = false;
#pragma unroll
    for (int m = 0; m < CAP; ++m)
        if (m < M || (m >= kShieldM && m < kShieldM + MO)) violated |= fmaf(ax[m], ux, ay[m] * uy) > b[m];
    float x = ux, y = uy, corr = finite ? 0.0f : __builtin_nanf("");
    if (finite && violated) {
        // |s0| <= |ux| + |uy| + b_m on every line m; inside the box |s| <= 2 u_max + b_m (+inf: no box)
        const float noise_u = kShieldNoise * fminf(__builtin_fabsf(ux) + __builtin_fabsf(uy), 2.0f * a.u_max);
#pragma unroll
        for (int m = 0; m < CAP; ++m) {
            if ((m < M || (m >= kShieldM && m < kShieldM + MO)) && fmaf(ax[m], x, ay[m] * y) > b[m]) {
                const float qx = b[m] * ax[m], qy = b[m] * ay[m];                      // the line's point closest to 0 (|a| = 1)
                const float tx = -ay[m], ty = ax[m];
                const float s0 = fmaf(tx, ux, ty * uy);                                 // t . (u - q), and t . q = 0
                const float slack = fmaf(4.0f * kShieldNoise, b[m], noise_u);
                float lo = -inf, hi = inf;
#pragma unroll
                for (int n = 0; n < m; ++n) {
                    const float den = fmaf(ax[n], tx, ay[n] * ty);
                    const float num = fmaf(-ax[n], qx, fmaf(-ay[n], qy, b[n])) + (n < kShieldBox ? 0.0f : slack);   // (the box stays exact)
                    const float at = num * __builtin_amdgcn_rcpf(den);
                    hi = den > kShieldParallel ? fminf(hi, at) : hi;
                    lo = den < -kShieldParallel ? fmaxf(lo, at) : lo;
                }
                const float s = fminf(fmaxf(s0, lo), hi);
                x = fmaf(s, tx, qx); y = fmaf(s, ty, qy);
            }
        }
        // |u* - u|; where the squares overflow (|u* - u| > 2^64), of the components scaled by 2^-64: the value is a float32
        const float dx = x - ux, dy = y - uy;
        corr = __builtin_sqrtf(fmaf(dy, dy, dx * dx));
        if (corr == inf) {
            const float sx = dx * 0x1p-64f, sy = dy * 0x1p-64f;
            corr = __builtin_sqrtf(fmaf(sy, sy, sx * sx)) * 0x1p+64f;
        }
    }
    if (a.act8) {
        sh_f2 o; o.x = x; o.y = y;
        *reinterpret_cast<sh_f2 *>(a.act_out + 2 * r) = o;
    } else {
        a.act_out[2 * r] = x; a.act_out[2 * r + 1] = y;
    }
    if (a.intervened) a.intervened[r] = finite && violated ? 1 : 0;
    if (a.correction) a.correction[r] = corr;
}

__device__ __forceinline__ void shield_action(const ShieldArgs &a, unsigned long long r, float &ux, float &uy)
{
    if (a.act8) {
        const sh_f2 u = *reinterpret_cast<const sh_f2 *>(a.act + 2 * r);
        ux = u.x; uy = u.y;
    } else {
        ux = a.act[2 * r]; uy = a.act[2 * r + 1];
    }
}

template <int W>
__global__ void __launch_bounds__(256) action_shield_kernel(const ShieldArgs a)
{
    const unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (r >= a.records) return;
    const int i = (int)(r % (unsigned)a.N);
    float ux, uy;
    shield_action(a, r, ux, uy);
    float ax[kShieldM], ay[kShieldM], b[kShieldM];
    shield_constraints<W>(a, r, i, ax, ay, b);
    shield_solve_store(a, r, ux, uy, kShieldBox + a.k1 - 1, 0, ax, ay, b);
}

// dronesim_action_shield_obstacles: the same record, the same solve, up to four half-planes more
template <int W>
__global__ void __launch_bounds__(256) action_shield_obstacles_kernel(const ShieldArgs a, const ShieldObstacles ob)
{
    const unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (r >= a.records) return;
    const int i = (int)(r % (unsigned)a.N);
    float ux, uy;
    shield_action(a, r, ux, uy);
    float ax[kShieldAll], ay[kShieldAll], b[kShieldAll];
    const float ri = shield_constraints<W>(a, r, i, ax, ay, b);
    shield_obstacle_constraints(ob, r, ri, a.margin, ax, ay, b);
    shield_solve_store(a, r, ux, uy, kShieldBox + a.k1 - 1, ob.m, ax, ay, b);
}

// Per-agent running totals of the planes [E][N].  A workgroup of 1024 lanes owns 4 adjacent agents: lane t holds agent t % 4 of
// the tile and the envs t / 4, t / 4 + 256, ... in ascending order (a row of the tile is 4 bytes of `intervened` and 16 of
// `correction`; narrow tiles, because one plane is small -- 1.3 MB at 64 agents x 4096 envs -- and the launch is bound by how many
// rows a lane must wait for one after the other, not by bytes), then ONE fixed LDS tree folds the 256 lanes of an agent and the
// agent's first lane adds the result to the totals with plain loads and stores: the order never changes, so the totals are
// bit-identical run to run.
constexpr int kTotalsTile = 4, kTotalsRows = 256, kTotalsThreads = kTotalsTile * kTotalsRows, kTotalsUnroll = 8;

__global__ void __launch_bounds__(kTotalsThreads) shield_totals_kernel(const uint8_t *__restrict__ intervened, const float *__restrict__ correction,
                                                                       int E, int N, long long *interventions, long long *nonfinite,
                                                                       double *correction_sum, float *correction_max)
{
    __shared__ double s_sum[kTotalsThreads];
    __shared__ float s_max[kTotalsThreads];
    __shared__ int s_cnt[kTotalsThreads], s_nan[kTotalsThreads];
    const int t = threadIdx.x, rl = t / kTotalsTile, col = blockIdx.x * kTotalsTile + t % kTotalsTile;
    const bool on = col < N;
    double sum = 0.0;
    float mx = 0.0f;
    int cnt = 0, nan = 0;
    if (on) {
        // eight rows requested before the first is folded (a lane's rows are 256 apart: one at a time the loop waits out a
        // memory latency per row); the fold keeps the ascending order, so the unrolling does not change a bit
        for (long long e0 = rl; e0 < E; e0 += (long long)kTotalsUnroll * kTotalsRows) {
            float cv[kTotalsUnroll];
            uint8_t iv[kTotalsUnroll];
#pragma unroll
            for (int u = 0; u < kTotalsUnroll; ++u) {
                const long long e = e0 + (long long)u * kTotalsRows;
                const size_t at = (size_t)(e < E ? e : e0) * N + col;
                cv[u] = correction[at];
                iv[u] = intervened[at];
            }
#pragma unroll
            for (int u = 0; u < kTotalsUnroll; ++u) {
                if (e0 + (long long)u * kTotalsRows < E) {
                    const bool isnan = cv[u] != cv[u];
                    cnt += iv[u] != 0 ? 1 : 0;
                    nan += isnan ? 1 : 0;
                    sum += isnan ? 0.0 : (double)cv[u];
                    mx = isnan ? mx : fmaxf(mx, cv[u]);
                }
            }
        }
    }
    s_sum[t] = sum; s_max[t] = mx; s_cnt[t] = cnt; s_nan[t] = nan;
    for (int w = kTotalsRows / 2; w > 0; w >>= 1) {
        __syncthreads();
        if (rl < w) {
            const int o = t + w * kTotalsTile;
            s_sum[t] += s_sum[o]; s_max[t] = fmaxf(s_max[t], s_max[o]); s_cnt[t] += s_cnt[o]; s_nan[t] += s_nan[o];
        }
    }
    if (on && rl == 0) {                                       // (the lane's own LDS entries: written by itself in the last level)
        interventions[col] += (long long)s_cnt[t];
        nonfinite[col] += (long long)s_nan[t];
        correction_sum[col] += s_sum[t];
        correction_max[col] = fmaxf(correction_max[col], s_max[t]);
    }
}

// Host: the arguments of both shield entries, validated in ONE order and marshalled.  ob: nullptr for the plain entry; for the
// obstacle entry its list as the caller gave it, rate_dt still holding obstacle_rate -- divided by dt here, behind the checks.  The
// obstacle entry's own checks stand between the shared ones, so they are made here, where the order is stated once.
int shield_args(const char *where, const float *z, const int32_t *nbr, const float *act, const float *radius, float rate, float margin,
                float u_max, float dt, int E, int N, int k1, int c, float *act_out, uint8_t *intervened, float *correction,
                ShieldObstacles *ob, ShieldArgs &a)
{
    if (!z || !nbr || !act || !radius || !act_out) return fail_at(where, "NULL z / nbr / act / radius / act_out");
    if (ob && (!ob->orow || !ob->oid)) return fail_at(where, "NULL orow / oid");
    if (E < 0) return fail_at(where, "E < 0");
    int rc = check_records(where, N, k1, 2, DRONESIM_MAX_K + 1, c);
    if (rc == DRONESIM_OK && ob) rc = check_slots(where, ob->m);
    if (rc == DRONESIM_OK && ob) rc = check_discs(where, ob->M, nullptr, false);  // (the kernel reads the sensed rows, not the list)
    if (rc != DRONESIM_OK) return rc;
    if (!(rate > 0.0f && rate <= 0.5f)) return fail_at(where, "rate must be in (0, 0.5]");
    if (ob && !(ob->rate_dt > 0.0f && ob->rate_dt <= 1.0f)) return fail_at(where, "obstacle_rate must be in (0, 1]");
    if (!(margin >= 0.0f) || !(margin < __builtin_inff())) return fail_at(where, "margin must be finite and >= 0");
    if (!(u_max > 0.0f)) return fail_at(where, "u_max must be > 0 (+inf: no box; not NaN)");
    if (!(dt > 0.0f) || !(dt < __builtin_inff())) return fail_at(where, "dt must be finite and > 0");
    a.z = z; a.nbr = nbr; a.act = act; a.radius = radius; a.act_out = act_out; a.intervened = intervened; a.correction = correction;
    a.rate_dt = rate / dt; a.margin = margin; a.u_max = u_max;
    a.N = N; a.k1 = k1; a.c = c;
    a.act8 = ((reinterpret_cast<uintptr_t>(act) | reinterpret_cast<uintptr_t>(act_out)) & 7u) == 0 ? 1 : 0;
    a.records = (unsigned long long)E * (unsigned long long)N;
    if (ob) ob->rate_dt /= dt;
    return DRONESIM_OK;
}

}   // namespace

extern "C" {

int dronesim_action_shield(const float *z, const int32_t *nbr, const float *act, const float *radius, float rate, float margin,
                           float u_max, float dt, int E, int N, int k1, int c, float *act_out, uint8_t *intervened,
                           float *correction, void *stream)
{
    ShieldArgs a;
    const int rc = shield_args("dronesim_action_shield", z, nbr, act, radius, rate, margin, u_max, dt, E, N, k1, c, act_out, intervened,
                               correction, nullptr, a);
    if (rc != DRONESIM_OK || E == 0) return rc;
    const int W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
    if (W == 4) hipLaunchKernelGGL(action_shield_kernel<4>, grid, dim3(256), 0, s, a);
    else if (W == 2) hipLaunchKernelGGL(action_shield_kernel<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(action_shield_kernel<1>, grid, dim3(256), 0, s, a);
    return dronesim_launched();
}

int dronesim_action_shield_obstacles(const float *z, const int32_t *nbr, const float *act, const float *radius, float rate, float margin,
                                     float u_max, float dt, int E, int N, int k1, int c, float *act_out, uint8_t *intervened,
                                     float *correction, const float *orow, const int32_t *oid, int m, int M, float obstacle_rate,
                                     void *stream)
{
    ShieldObstacles ob{orow, oid, obstacle_rate, m, M};
    ShieldArgs a;
    const int rc = shield_args("dronesim_action_shield_obstacles", z, nbr, act, radius, rate, margin, u_max, dt, E, N, k1, c, act_out,
                               intervened, correction, &ob, a);
    if (rc != DRONESIM_OK || E == 0) return rc;
    const int W = record_load_width(k1, c, reinterpret_cast<uintptr_t>(z));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.records + 255) / 256));
    if (W == 4) hipLaunchKernelGGL(action_shield_obstacles_kernel<4>, grid, dim3(256), 0, s, a, ob);
    else if (W == 2) hipLaunchKernelGGL(action_shield_obstacles_kernel<2>, grid, dim3(256), 0, s, a, ob);
    else hipLaunchKernelGGL(action_shield_obstacles_kernel<1>, grid, dim3(256), 0, s, a, ob);
    return dronesim_launched();
}

int dronesim_shield_totals(const uint8_t *intervened, const float *correction, int E, int N, int64_t *interventions,
                           int64_t *nonfinite, double *correction_sum, float *correction_max, void *stream)
{
    const char *where = "dronesim_shield_totals";
    if (!intervened || !correction || !interventions || !nonfinite || !correction_sum || !correction_max) return fail_at(where, "NULL pointer");
    if (E < 0 || N < 1 || N > DRONESIM_MAX_AGENTS) return fail_at(where, "E < 0 or N outside 1..1024");
    if (E == 0) return DRONESIM_OK;
    hipLaunchKernelGGL(shield_totals_kernel, dim3((unsigned)((N + kTotalsTile - 1) / kTotalsTile)), dim3(kTotalsThreads), 0,
                       static_cast<hipStream_t>(stream), intervened, correction, E, N, reinterpret_cast<long long *>(interventions),
                       reinterpret_cast<long long *>(nonfinite), correction_sum, correction_max);
    return dronesim_launched();
}

}   // extern "C"
