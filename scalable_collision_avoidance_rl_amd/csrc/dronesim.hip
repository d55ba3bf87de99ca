// dronesim.hip -- C ABI (include/dronesim.h) of the batched drone_env hot path on gfx950 (MI355X / CDNA4), plus the
// small kernels around the step kernel: reset, classical controllers, episode reductions (learner-side scans: scans.hip).
// The step / observe / rollout kernel itself lives in drone_kernel.hpp and is instantiated per k_closest value in
// drone_kernel_k.hip; this file fills its arguments and dispatches.
#include "drone_kernel.hpp"

namespace {

// ---------------------------------------------------------------------------------------
// reset: N distinct lattice nodes per env by parallel rejection on a Philox4x32-10 stream
// (restated integer-exactly on the CPU in oracle/drone_oracle.c:oracle_reset).

struct RArgs {
    int N, E, P, epb, div_y, nt, shift;     // nt: sampling-table entries per env (2^k >= 2 N), shift = 32 - k
    uint32_t M, key0, key1;
    long long env_base;
    float pitch;
    const uint8_t *mask;
    float *pos, *vel;
    int *t, *episode, *node_out;
    double *acc;                    // DroneEpisodeAcc[E] (8 x 8 bytes per env) or nullptr: retire the episode in progress
};

__global__ void __launch_bounds__(1024) reset_kernel(const RArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N;
    int2 *sst = reinterpret_cast<int2 *>(smem);            // [epb][nt] open-addressing table of (node, owner)
    const int tid = threadIdx.x;
    int slot, agent;
    bool valid;
    if (a.P > 0) {                                           // same lane -> (slot, agent) map as drone_kernel
        const int lane = tid & (kWave - 1);
        const int sub = lane / N;
        slot = (tid >> 6) * a.P + sub;
        agent = lane - sub * N;
        valid = sub < a.P;
    } else {
        slot = 0; agent = tid; valid = tid < N;
    }
    const int env = blockIdx.x * a.epb + slot;
    valid = valid && env < a.E;
    if (valid && a.mask != nullptr) valid = a.mask[env] != 0;
    const uint32_t gid = (uint32_t)(a.env_base + env);
    const uint32_t epi = valid ? (uint32_t)a.episode[env] : 0u;   // resets this env has seen so far
    // Round r: unsettled agent i proposes node mulhi(philox(i, r, env, episode), M) and settles on it iff no settled
    // agent holds that node and no lower-index agent proposed it this round.  The rule is evaluated through an
    // open-addressing table per env (2^k >= 2 N entries, keys compared exactly): settled agents enter their node as
    // blockers (owner -1), proposers enter theirs with owner = min(agent index); a proposer wins iff it owns its entry.
    const int nt = a.nt;
    int2 *tbl = sst + (size_t)slot * nt;

    int node = -1;
    int remaining;
    uint32_t round = 0;
    do {
        if (valid)
            for (int o = agent; o < nt; o += N) tbl[o] = make_int2(-1, 0x7fffffff);
        __syncthreads();
        int cand = node, h = 0;
        if (valid) {
            if (node < 0) {
                const uint32_t w = philox4x32_10_word0((uint32_t)agent, round, gid, epi, a.key0, a.key1);
                cand = (int)__umulhi(w, a.M);
            }
            h = (int)(((uint32_t)cand * 0x9E3779B1u) >> a.shift);
            for (;;) {                                                // linear probing, load factor <= 1/2
                const int old = atomicCAS(&tbl[h].x, -1, cand);
                if (old == -1 || old == cand) break;
                h = (h + 1) & (nt - 1);
            }
            atomicMin(&tbl[h].y, node >= 0 ? -1 : agent);
        }
        __syncthreads();
        if (valid && node < 0 && tbl[h].y == agent) node = cand;
        remaining = __syncthreads_count(valid && node < 0);
        ++round;
    } while (remaining > 0 && round < (1u << 20));

    if (valid && node >= 0) {
        const size_t ga = (size_t)env * N + agent;
        const int idx = node / a.div_y, jdx = node - idx * a.div_y;
        reinterpret_cast<float2 *>(a.pos)[ga] = make_float2((float)idx * a.pitch, (float)jdx * a.pitch);
        reinterpret_cast<float2 *>(a.vel)[ga] = make_float2(0.f, 0.f);   // drone_env.py:189
        if (a.node_out) a.node_out[ga] = node;
        if (agent == 0) {
            a.t[env] = 0;                                                // drone_env.py:100
            a.episode[env] = (int)(epi + 1u);
            if (a.acc != nullptr) {                                      // train_problem.py:118-121: log, then reset
                double *rec = a.acc + 8 * (size_t)env;
                int *reci = reinterpret_cast<int *>(rec);
                if (reci[5] > 0) {                                       // ep_len: an episode was in progress
                    rec[4] += rec[0]; rec[5] += rec[1];
                    reinterpret_cast<long long *>(rec)[6] += reci[4];
                    reinterpret_cast<long long *>(rec)[7] += reci[5];
                    reci[6] += 1;
                    rec[0] = 0.0; rec[1] = 0.0; reci[4] = 0; reci[5] = 0;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Classical controllers (drone_env.py:609-679), same lane <-> agent geometry as drone_kernel.
// gradient_control sums a repulsion term over the partners inside dhat_i + l_i + l_j (:641-644).  Envs of >= kBucketMinN
// agents find them the way the step kernel's far filter does (round 6): every agent ORs its bit into the mask of its x
// cell and of its y cell (64 hashed cells per axis, at least one reach wide), an agent's candidates are
// (3 x masks) & (3 y masks), and only those get the exact test -- in ascending partner order, so the sum is the one the
// all-partner loop forms (far partners never contributed a term): C3 12.8 -> see DESIGN.md section 7.  Smaller envs keep the loop.
struct CArgs {
    int N, E, P, epb, kind;
    float u_max;
    const float *xF, *xF_lo, *d_hat, *radius, *pos;
    float *act;
    int bucket, tab_off;            // cell-mask filter in use; byte offset of its tables in LDS
    float inv_cell;                 // 1 / cell width
};

// (the controllers' arithmetic -- control_proportional, gradient_pair, control_gradient -- lives in drone_kernel.hpp: the
// closed-loop rollout evaluates the same expressions inside its launch)

template <bool WL>
__global__ void __launch_bounds__(1024) control_kernel(const CArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N;
    const int tid = threadIdx.x;
    const unsigned lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
    int slot, agent, env0, nval;
    if (WL) {
        const int sub = (int)lane / N;
        slot = wave * a.P + sub;
        agent = (int)lane - sub * N;
        env0 = blockIdx.x * a.epb + wave * a.P;
        nval = max(0, min(a.P, a.E - env0)) * N;
    } else {
        slot = 0; agent = tid; env0 = blockIdx.x;
        nval = max(0, min(kWave, N - wave * kWave));
    }
    const size_t wga0 = (size_t)env0 * N + (WL ? 0 : wave * kWave);
    const bool valid = (int)lane < nval;
    const bool gradient = a.kind == DRONESIM_CONTROL_GRADIENT;               // launch-uniform
    const bool bucket = gradient && a.bucket != 0;
    float2 *spos = reinterpret_cast<float2 *>(smem);                         // [epb][N]
    float *srad = reinterpret_cast<float *>(spos + (size_t)a.epb * N);       // [WL ? nwaves : 1][N]
    float *srad_w = srad + (WL ? (size_t)wave * N : 0);
    // cell tables (bucket): [axis][W words of 64 agents][64 cells]; one env per wave (WL: N >= kBucketMinN) or per workgroup
    const int W = WL ? 1 : nwaves;
    unsigned long long *tb = reinterpret_cast<unsigned long long *>(smem + a.tab_off) + (WL ? (size_t)wave * 2 * kCells : 0);
    float xi = 0.f, yi = 0.f, xFx = 0.f, xFy = 0.f, xLx = 0.f, xLy = 0.f, dhat = 1.f, ri = 0.f;
    if (valid) {
        const float2 p = (reinterpret_cast<const float2 *>(a.pos) + wga0)[lane];
        const float2 g = reinterpret_cast<const float2 *>(a.xF)[(unsigned)agent];
        if (a.xF_lo) { const float2 gl = reinterpret_cast<const float2 *>(a.xF_lo)[(unsigned)agent]; xLx = gl.x; xLy = gl.y; }
        dhat = a.d_hat[(unsigned)agent];
        ri = a.radius[(unsigned)agent];
        xi = p.x; yi = p.y; xFx = g.x; xFy = g.y;
        if (gradient) spos[(size_t)slot * N + agent] = p;
    }
    if (gradient) {
        if (WL) { if ((int)lane < N) srad_w[lane] = a.radius[lane]; }
        else for (int s = tid; s < N; s += blockDim.x) srad_w[s] = a.radius[s];
        if (bucket) {
            if (WL) { for (int o = lane; o < 2 * kCells; o += kWave) tb[o] = 0ull; }
            else for (int o = tid; o < 2 * kCells * W; o += blockDim.x) tb[o] = 0ull;
        }
        group_sync<WL>();
    }
    float2 u;
    if (!gradient) {
        u = control_proportional(xi, yi, xFx, xFy, xLx, xLy, a.u_max);       // :652-679
    } else {
        const float2 *pe = spos + (size_t)slot * N;
        float t2x = 0.f, t2y = 0.f;
        if (bucket) {
            const int cx = (int)__builtin_floorf(xi * a.inv_cell) & (kCells - 1), cy = (int)__builtin_floorf(yi * a.inv_cell) & (kCells - 1);
            if (valid) {
                atomicOr(&tb[(agent >> 6) * kCells + cx], 1ull << (agent & 63));
                atomicOr(&tb[(W + (agent >> 6)) * kCells + cy], 1ull << (agent & 63));
            }
            group_sync<WL>();
            if (valid) {
                const int cxm = (cx - 1) & (kCells - 1), cxp = (cx + 1) & (kCells - 1);
                const int cym = (cy - 1) & (kCells - 1), cyp = (cy + 1) & (kCells - 1);
                for (int w = 0; w < W; ++w) {                                // ascending partner order, like the loop below
                    const unsigned long long *tx = tb + w * kCells, *ty = tb + (W + w) * kCells;
                    unsigned long long m = (tx[cxm] | tx[cx] | tx[cxp]) & (ty[cym] | ty[cy] | ty[cyp]);
                    if (w == (agent >> 6)) m &= ~(1ull << (agent & 63));
                    while (m) {
                        const int j = 64 * w + __builtin_ctzll(m);
                        m &= m - 1ull;
                        gradient_pair(xi, yi, ri, dhat, pe[j], srad_w[j], t2x, t2y);
                    }
                }
            }
        } else if (valid) {
            for (int j = 0; j < N; ++j)
                if (j != agent) gradient_pair(xi, yi, ri, dhat, pe[j], srad_w[j], t2x, t2y);
        }
        u = control_gradient(xi, yi, xFx, xFy, xLx, xLy, t2x, t2y, a.u_max);   // :633, :646-647
    }
    if (valid) (reinterpret_cast<float2 *>(a.act) + wga0)[lane] = u;
}

// ---------------------------------------------------------------------------------------
// The logged statistic of one step (train_problem.py:98-100: sums of rewards, true rewards and collisions),
// accumulated in float64 into acc[5] = (sum r, sum true r, sum collisions, agent-steps, env-steps).
// One launch: every workgroup reduces a slice to three partial sums in `scratch` (fixed LDS tree); the workgroup that
// arrives last reduces the partials with the same fixed tree over the block index: bit-reproducible run to run.
constexpr int kStatBlocks = 256;

__global__ void __launch_bounds__(256) stats_kernel(const float *__restrict__ reward, const float *__restrict__ true_reward,
                                                    const int *__restrict__ n_coll, int E, int N, double *acc,
                                                    double *scratch)
{
    __shared__ double sh[3][256];
    __shared__ bool last;
    const int tid = threadIdx.x;
    const size_t n = (size_t)E * N;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    // 16 bytes per lane when the arrays allow it (E * N a multiple of 4 and 16-byte aligned bases), else 4
    const bool wide = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(true_reward)) & 15u) == 0;
    if (wide) {
        const float4 *r4 = reinterpret_cast<const float4 *>(reward), *t4 = reinterpret_cast<const float4 *>(true_reward);
        for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n / 4; i += (size_t)gridDim.x * 256) {
            const float4 a = r4[i], b = t4[i];
            s0 += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
            s1 += ((double)b.x + (double)b.y) + ((double)b.z + (double)b.w);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n; i += (size_t)gridDim.x * 256) {
            s0 += (double)reward[i];
            s1 += (double)true_reward[i];
        }
    }
    for (int e = blockIdx.x * 256 + tid; e < E; e += gridDim.x * 256) s2 += (double)n_coll[e];
    sh[0][tid] = s0; sh[1][tid] = s1; sh[2][tid] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {                       // fixed tree: the order depends on nothing but (E, N)
        if (tid < w) { sh[0][tid] += sh[0][tid + w]; sh[1][tid] += sh[1][tid + w]; sh[2][tid] += sh[2][tid + w]; }
        __syncthreads();
    }
    unsigned *ticket = reinterpret_cast<unsigned *>(scratch + 3 * kStatBlocks);
    if (tid == 0) {
        for (int k = 0; k < 3; ++k) scratch[k * kStatBlocks + blockIdx.x] = sh[k][0];
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last) {                                               // the workgroup that arrives last adds the partials,
        __threadfence();                                      // again as a fixed tree over the block index
        for (int k = 0; k < 3; ++k) sh[k][tid] = tid < (int)gridDim.x ? __builtin_nontemporal_load(scratch + k * kStatBlocks + tid) : 0.0;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) { sh[0][tid] += sh[0][tid + w]; sh[1][tid] += sh[1][tid + w]; sh[2][tid] += sh[2][tid + w]; }
            __syncthreads();
        }
        if (tid < 3) acc[tid] += sh[tid][0];
        if (tid == 0) { acc[3] += (double)E * N; acc[4] += (double)E; *ticket = 0u; }
    }
}

// Sum of the E episode records of a rank -> out[8] (include/dronesim.h).  ONE workgroup: thread i adds the records
// i, i + 1024, ... in order, then a fixed LDS tree: the summation order does not depend on anything but E.
__global__ void __launch_bounds__(1024) episode_reduce_kernel(const double *__restrict__ acc, int E, double *__restrict__ out)
{
    __shared__ double sh[8][1024];
    const int tid = threadIdx.x;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = tid; e < E; e += 1024) {
        const double *rec = acc + 8 * (size_t)e;
        const int *reci = reinterpret_cast<const int *>(rec);
        const long long *recl = reinterpret_cast<const long long *>(rec);
        v[0] += rec[4]; v[1] += rec[5]; v[2] += (double)recl[6]; v[3] += (double)recl[7]; v[4] += (double)reci[6];
        v[5] += rec[0]; v[6] += rec[1]; v[7] += (double)reci[5];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k][tid] = v[k];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 8; ++k) sh[k][tid] += sh[k][tid + w];
        }
        __syncthreads();
    }
    if (tid < 8) out[tid] = sh[tid][0];
}

// ---------------------------------------------------------------------------------------
thread_local char g_err[256] = "";
long long *g_trace = nullptr;         // developer trace builds (kTrace): per-wave stamp buffer of the step kernel

int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
}   // namespace

// shared with the other translation units of the library (csrc/common.hpp); not part of the C ABI
__attribute__((visibility("hidden"))) int dronesim_fail(int code, const char *msg) { return fail(code, msg); }

namespace {

constexpr Geometry geometry(int N, int E)
{
    Geometry g{};
    if (N <= kWave) {                  // 4 (or 2) independent waves per workgroup, floor(64/N) envs per wave
        g.P = kWave / N;
        // one env per wave (N > 32): two waves per workgroup -- measured against 4 (the round-1 choice), 8 and 16 at C3:
        // 5.33 / 5.40 / 5.42 / 5.71 us per launch (a single wave per workgroup doubles the cost of an empty launch);
        // several small envs per wave keep 4 (C2: 3.85 us against 4.13 with 2)
        const int wpb = g.P == 1 ? 2 : 4;
        g.threads = wpb * kWave;
        g.epb = wpb * g.P;
        g.geo = kPacked;
    } else {                           // (P = 0)
        g.threads = ((N + kWave - 1) / kWave) * kWave;
        g.epb = 1;
        g.geo = g.threads <= 256 ? kBlock256 : kBlock1024;
    }
    g.blocks = (E + g.epb - 1) / g.epb;
    return g;
}

constexpr size_t kLdsTile = 160 * 1024;                                   // LDS of a CU: the most a workgroup can ask for
constexpr size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// Dynamic LDS of drone_kernel: the sum of the region functions the kernel carves with (drone_kernel.hpp) -- the total, and the
// offsets the kernel is told (KArgs.lds_vel, lds_tail) with the choice that moves them (KArgs.stage5).
//   [positions][(Delta_j, l_j) tables][verdict words][staging area][cell tables]   or kSym64's block per wave
//   [velocities]   c = 5 with staged rows (stage5): the rows of the k nearest carry them
//   [tail]         episode layer (`epi_regions`): per-wave partial sums, then the in-kernel reset's sampling tables -- unless the
//                  tables share the cell tables' region (`shared_table`: workgroup-per-env geometries, single-step launches, round 5;
//                  a reset runs behind the step's last use of the cell tables: 25.8 -> 21.7 KiB per workgroup at N = 256, 7 instead
//                  of 6 workgroups per CU, 256 x 4096 envs 20.0 -> 19.5 us; the fused rollouts keep the table in the tail, sharing
//                  measured +2 % there: profiles/r5_abtest_sampling_table_alias.log)
struct StepLds { size_t total; int lds_vel, lds_tail, stage5; };

constexpr StepLds step_lds(int geo, int P, int epb, int threads, int N, int k, int c, bool rollout, bool epi_regions, bool tail_table,
                           bool shared_table)
{
    const size_t nwaves = (size_t)threads / kWave;
    const size_t samp = sizeof(int2) * (size_t)epb * samp_table_entries(N);
    const size_t tail = epi_regions ? sizeof(float) * tail_part_floats((int)nwaves) + (tail_table ? samp : 0) : 0;
    // bucket filter tables: per env slot, or the floor of 66 x 16 bytes per wave the packed geometries keep (whichever is larger)
    size_t tables = (P > 0 && N < kBucketMinN) ? 0 : sizeof(unsigned long long) * (P > 0 ? (size_t)epb : 1) * table_words(geo, rollout, P > 0 ? 1 : (int)nwaves);
    if (shared_table && samp > tables) tables = samp;
    if (P > 0 && sizeof(ulonglong2) * nwaves * kBucketRows > tables) tables = sizeof(ulonglong2) * nwaves * kBucketRows;
    const size_t fixed = sizeof(float2) * ((P > 0 ? packed_pos_entries(epb, N) : (size_t)block_pos_entries(N)) + (P > 0 ? nwaves : 1) * const_entries(N)) +
                         sizeof(int) * red_words(epb) + tables;
    // zc: columns of a staged z row (2, or 5 when those fit)
    const auto body = [=](int zc) { return geo == kSym64 ? nwaves * sym_wave_bytes(k, zc) : fixed + sizeof(unsigned) * nwaves * stage_words(zc, k); };
    // c = 5 rows: staged through LDS like the c = 2 ones, and the agents' velocities kept in LDS for the rows of the k nearest,
    // when the env's tile still fits (it does up to N = 1024 at k <= 3, and always in kSym64's; the rows leave as 4-byte stores
    // at a 60-byte stride otherwise, as they all did through round 2)
    // (the velocity region is rounded up to 16 bytes: the episode layer reads its per-wave partial sums behind it as
    // ds_read_b128 -- 8 N bytes with odd N left `lds_tail` 8-byte aligned)
    const size_t vel = round16(sizeof(float2) * (size_t)epb * (size_t)N);
    StepLds r{};
    r.stage5 = (c == 5 && (geo == kSym64 || body(5) + vel + tail <= kLdsTile)) ? 1 : 0;
    size_t b = body(r.stage5 ? 5 : 2);
    if (r.stage5) { r.lds_vel = (int)b; b += vel; }
    r.lds_tail = (int)round16(b);                          // the tail's float4 reads (per-wave partial sums) need 16 bytes
    r.total = (size_t)r.lds_tail + tail;
    return r;
}

// The layout's promises, over every launchable (N, k): each region a whole number of 16-byte units (the carve-up relies on it
// for its 16-byte LDS accesses), and kSym64's block the sum of its parts.
constexpr bool step_lds_regions_ok()
{
    bool ok = sym_stage_offset() % 16 == 0;
    for (int k = 1; k <= DRONESIM_MAX_K; ++k)              // (no region depends on both N and k: one loop each)
        for (int zc = 2; zc <= 5; zc += 3)
            ok = ok && sizeof(unsigned) * stage_words(zc, k) % 16 == 0 && sym_cells_offset(k, zc) % 16 == 0 && sym_wave_bytes(k, zc) % 16 == 0 &&
                 sym_wave_bytes(k, zc) == sym_stage_offset() + 4 * stage_words(zc, k) + 2 * kCells * 8;
    for (int N = 2; N <= DRONESIM_MAX_AGENTS; ++N) {
        const Geometry g = geometry(N, 1);
        const int nwaves = g.threads / kWave, W = g.P > 0 ? 1 : nwaves;
        const size_t regions[] = {sizeof(float2) * pos_stride(N), sizeof(float2) * block_pos_entries(N), sizeof(float2) * const_entries(N),
                                  sizeof(int) * red_words(g.epb), sizeof(float) * tail_part_floats(nwaves), sizeof(int2) * samp_table_entries(N),
                                  sizeof(unsigned long long) * table_words(g.geo, false, W), sizeof(unsigned long long) * table_words(g.geo, true, W)};
        for (const size_t r : regions) ok = ok && r % 16 == 0;
    }
    return ok;
}
static_assert(step_lds_regions_ok(), "an LDS region of drone_kernel is not a multiple of 16 bytes, or sym_wave_bytes is not the sum of its parts");

int check_params(const DroneParams *p, int E)
{
    if (!p) return fail(DRONESIM_EINVAL, "params is NULL");
    if (E < 0) return fail(DRONESIM_EINVAL, "E < 0");
    if (p->N < 2 || p->N > DRONESIM_MAX_AGENTS) return fail(DRONESIM_EUNSUPPORTED, "N must be in 2..1024");
    if (p->k < 1 || p->k > p->N - 1) return fail(DRONESIM_EINVAL, "k_closest must be in 1..N-1");
    if (p->k > DRONESIM_MAX_K) return fail(DRONESIM_EUNSUPPORTED, "k_closest > DRONESIM_MAX_K");
    if (p->c != 2 && p->c != 5) return fail(DRONESIM_EINVAL, "c must be 2 or 5");
    if (!p->xF || !p->d_hat || !p->delta || !p->radius) return fail(DRONESIM_EINVAL, "constant array is NULL");
    if (!(p->d_hat_min > 0.0f) || !(p->d_hat_max >= p->d_hat_min))
        return fail(DRONESIM_EINVAL, "need 0 < d_hat_min <= d_hat_max");
    return DRONESIM_OK;
}

}   // namespace

// drone_kernel_k.hip, one translation unit per k: dronesim_launch_k<k>(mode, KArgs, Geometry, stream)
#define DRONESIM_EACH_K(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#define DRONESIM_DECLARE_K(k) extern "C" int dronesim_launch_k##k(int, const void *, const void *, void *);
DRONESIM_EACH_K(DRONESIM_DECLARE_K)

namespace {

// the lattice a reset draws from: div_x x div_y nodes, at least N of them, fewer than 2^32 (`bad_size`: the caller's text for div < 1)
int check_lattice(int div_x, int div_y, int N, const char *bad_size, uint32_t *M_out)
{
    if (div_x < 1 || div_y < 1) return fail(DRONESIM_EINVAL, bad_size);
    const uint64_t M = (uint64_t)div_x * (uint64_t)div_y;
    if (M < (uint64_t)N) return fail(DRONESIM_EINVAL, "lattice has fewer nodes than agents (random.sample would raise)");
    if (M > 0xFFFFFFFFull) return fail(DRONESIM_EUNSUPPORTED, "lattice larger than 2^32 nodes");
    *M_out = (uint32_t)M;
    return DRONESIM_OK;
}

// the Philox stream of an env's resets and in-kernel actions (DroneEpisodeCtl -> kernel arguments)
void set_stream(const DroneEpisodeCtl *ctl, KArgs &a)
{
    a.episode = ctl->episode; a.gid_base = (uint32_t)ctl->env_base;
    a.key0 = (uint32_t)ctl->seed; a.key1 = (uint32_t)(ctl->seed >> 32);
}

// DroneEpisodeCtl -> kernel arguments (include/dronesim.h)
int apply_ctl(const DroneParams *p, const DroneEpisodeCtl *ctl, bool rand_act, KArgs &a)
{
    a.rand_act = rand_act ? 1 : 0;
    if (!ctl) return DRONESIM_OK;
    a.acc = reinterpret_cast<double *>(ctl->acc);
    a.auto_reset = ctl->auto_reset != 0 ? 1 : 0;
    if (a.auto_reset || rand_act) {
        if (!ctl->episode) return fail(DRONESIM_EINVAL, "DroneEpisodeCtl.episode is NULL");
        set_stream(ctl, a);
    }
    if (a.auto_reset) {
        const int rc = check_lattice(ctl->div_x, ctl->div_y, p->N, "DroneEpisodeCtl: bad lattice size", &a.lat_M);
        if (rc) return rc;
        a.div_y = ctl->div_y; a.pitch = ctl->pitch;
        a.z_final = ctl->z_final; a.nbr_final = ctl->nbr_final; a.pos_final = ctl->pos_final;
    }
    return DRONESIM_OK;
}

// state and output buffers of a launch -> kernel arguments (observe: `vel` is read, and t / act / done stay NULL)
KArgs step_args(float *pos, float *vel, int32_t *t, const float *act, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                int32_t *n_coll, uint8_t *done, int T)
{
    KArgs a{};
    a.pos = pos; a.vel = vel; a.t = t; a.act = act; a.reward = reward; a.true_reward = true_reward;
    a.z = z; a.nbr_idx = nbr_idx; a.n_coll = n_coll; a.done = done; a.T = T;
    return a;
}

int reset_impl(const DroneParams *p, int div_x, int div_y, float pitch, uint64_t seed, int64_t env_base,
               const uint8_t *mask, float *pos, float *vel, int32_t *t, int32_t *episode, int32_t *node_out,
               double *acc, int E, void *stream)
{
    if (!p) return fail(DRONESIM_EINVAL, "params is NULL");
    if (p->N < 1 || p->N > DRONESIM_MAX_AGENTS) return fail(DRONESIM_EUNSUPPORTED, "N must be in 1..1024");
    if (E < 0 || div_x < 1 || div_y < 1) return fail(DRONESIM_EINVAL, "bad E / lattice size");
    if (!pos || !vel || !t || !episode) return fail(DRONESIM_EINVAL, "dronesim_reset: required buffer is NULL");
    RArgs a{};
    const int rc = check_lattice(div_x, div_y, p->N, "bad E / lattice size", &a.M);   // (its size test: made above, ahead of the buffers')
    if (rc) return rc;
    if (E == 0) return DRONESIM_OK;
    const Geometry g = geometry(p->N, E);
    a.N = p->N; a.E = E; a.P = g.P; a.epb = g.epb; a.div_y = div_y;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.env_base = env_base; a.pitch = pitch; a.mask = mask;
    a.pos = pos; a.vel = vel; a.t = t; a.episode = episode; a.node_out = node_out; a.acc = acc;
    a.nt = samp_table_entries(p->N);
    a.shift = 32 - __builtin_ctz((unsigned)a.nt);
    const size_t lds = sizeof(int2) * (size_t)g.epb * a.nt;
    hipLaunchKernelGGL(reset_kernel, dim3(g.blocks), dim3(g.threads), lds, static_cast<hipStream_t>(stream), a);
    return dronesim_launched();
}

// the reach of an agent's partners, d_hat + 2 l at their largest; the fused rollouts' candidate list keeps kSkin of it as slack
float reach_max(const DroneParams *p) { return p->d_hat_max + 2.0f * p->radius_max; }
float skin(const DroneParams *p) { return kSkin * reach_max(p); }

// The plan of a step / observe / rollout launch, without a HIP call: which instance runs (g.geo, g.far, g.epi, g.ctrl: closed-loop
// rollout of mode kRollout, 1 + DRONESIM_CONTROL_*), its grid and LDS, and every kernel argument that follows from the
// parameters -- or the refusal.  `a` arrives with its buffers and the episode layer's fields (apply_ctl) set.
int plan_step_launch(int mode, const DroneParams *p, KArgs &a, int E, int ctrl, Geometry &g)
{
    const int N = p->N;
    const bool rollout = mode == kRollout;
    g = geometry(N, E);
    g.ctrl = ctrl;
    // far agents matter when a z row carries (v, l) of a tie-ordered agent (c = 5) or
    // when a clipped distance can pass a Delta mask (Delta_j >= dhat_i possible)
    a.far_inm = !(p->delta_max < p->d_hat_min) ? 1 : 0;
    g.far = (p->c == 5 || a.far_inm) ? 1 : 0;
    g.epi = (a.acc != nullptr || a.auto_reset != 0 || a.rand_act != 0) ? 1 : 0;   // DroneEpisodeCtl in use
    a.uniform = (p->d_hat_min == p->d_hat_max && p->delta_min == p->delta_max && p->radius_min == p->radius_max) ? 1 : 0;
    const bool wide_rows = ((reinterpret_cast<uintptr_t>(a.z) | reinterpret_cast<uintptr_t>(a.nbr_idx)) & 15u) == 0;
    // one env per wave, uniform (d_hat, Delta, radius) only; its fixed-shape copy-out of c = 2 rows stores 16 bytes per lane.
    // Round 4: also the FAR variant -- the reference's DEFAULT construction (deltas=None, simplify_zstate=False) at N = 64
    if (N == 64 && a.uniform && wide_rows) g.geo = kSym64;
    // N = 256 with uniform constants (BASELINE configs[4]), fused rollouts: the workgroup-per-env kernel with four full waves known at compile time
    if (rollout && g.geo == kBlock256 && N == 256 && !g.far && a.uniform && wide_rows) g.geo = kBlockU256;
    // the episode layer's regions: only when in use (dronesim_reset_observe: the sampling table of its draw, kept in the tail)
    const bool epi_regions = g.epi || a.do_reset != 0;
    const bool share = g.P == 0 && !rollout;               // workgroup-per-env, single step: the sampling table shares the cell tables' region
    const StepLds l = step_lds(g.geo, g.P, g.epb, g.threads, N, p->k, p->c, rollout, epi_regions, !share || a.do_reset, share && a.auto_reset);
    // closed-loop rollout: the c = 5 rows of the k nearest carry the partners' velocities = their actions, which exist in LDS only
    if (ctrl != 0 && p->c == 5 && !l.stage5)
        return fail(DRONESIM_EUNSUPPORTED, "dronesim_rollout_control: c = 5 rows of this n_agents x k_closest do not fit the LDS tile");
    if (l.total > kLdsTile) return fail(DRONESIM_EUNSUPPORTED, "n_agents x k_closest too large for the 160 KiB LDS tile");
    g.lds = l.total;
    a.stage5 = l.stage5; a.lds_vel = l.lds_vel; a.lds_tail = l.lds_tail;
    if (epi_regions) {
        a.samp_tbl = samp_table_entries(N);
        a.samp_shift = 32 - __builtin_ctz((unsigned)a.samp_tbl);
    }
    a.N = N; a.c = p->c; a.max_steps = p->max_steps; a.E = E; a.P = g.P; a.epb = g.epb;
    a.dt = p->dt; a.q = p->q; a.b = p->b; a.done_radius = p->done_radius;
    a.ghost_factor = p->ghost_factor; a.radius_max = p->radius_max; a.reach_max = reach_max(p);
    a.dhat_u = p->d_hat_max; a.delta_u = p->delta_max; a.radius_u = p->radius_max;
    a.xF = p->xF; a.xF_lo = p->xF_lo; a.d_hat = p->d_hat; a.delta = p->delta; a.radius = p->radius;
    a.bucket = (g.P > 0 && N >= kBucketMinN) ? 1 : 0;
    return DRONESIM_OK;
}

int launch(int mode, const DroneParams *p, KArgs &a, int E, void *stream, int ctrl = 0)
{
    if (E == 0) return DRONESIM_OK;
    Geometry g;
    const int rc = plan_step_launch(mode, p, a, E, ctrl, g);
    if (rc) return rc;
    a.trace = ((kTrace || kTraceSpan) && (mode == kStep || (mode == kObserve && a.do_reset))) ? g_trace : nullptr;
    static_assert(DRONESIM_MAX_K == 8, "eight translation units, one k value each");
#define DRONESIM_NAME_K(k) dronesim_launch_k##k,
    static constexpr int (*launch_k[DRONESIM_MAX_K])(int, const void *, const void *, void *) = {DRONESIM_EACH_K(DRONESIM_NAME_K)};
    const int le = launch_k[p->k - 1](mode, &a, &g, stream);            // (check_params: 1 <= k <= DRONESIM_MAX_K)
    if (le != 0) {
        char msg[200];
        snprintf(msg, sizeof(msg), "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for %zu bytes of LDS: %s",
                 g.lds, hipGetErrorString(static_cast<hipError_t>(le)));
        return fail(DRONESIM_ELAUNCH, msg);
    }
    return dronesim_launched();
}

}   // namespace

extern "C" {

int dronesim_step_ex(const DroneParams *p, const DroneEpisodeCtl *ctl, float *pos, float *vel, int32_t *t,
                     const float *act, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                     int32_t *n_coll, uint8_t *done, int E, void *stream)
{
    int rc = check_params(p, E);
    if (rc) return rc;
    if (!pos || !vel || !t || !act || !z || !nbr_idx || !done)
        return fail(DRONESIM_EINVAL, "dronesim_step: required buffer is NULL");
    KArgs a = step_args(pos, vel, t, act, reward, true_reward, z, nbr_idx, n_coll, done, 1);
    if ((rc = apply_ctl(p, ctl, false, a)) != 0) return rc;
    return launch(kStep, p, a, E, stream);
}

int dronesim_step_call(const DroneStepCall *c, const float *act, void *stream)
{
    if (!c) return fail(DRONESIM_EINVAL, "dronesim_step_call: call is NULL");
    return dronesim_step_ex(c->p, c->ctl, c->pos, c->vel, c->t, act, c->reward, c->true_reward, c->z, c->nbr_idx,
                            c->n_coll, c->done, c->E, stream);
}

int dronesim_step(const DroneParams *p, float *pos, float *vel, int32_t *t, const float *act,
                  float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                  int32_t *n_coll, uint8_t *done, int E, void *stream)
{
    return dronesim_step_ex(p, nullptr, pos, vel, t, act, reward, true_reward, z, nbr_idx, n_coll, done, E, stream);
}

int dronesim_observe(const DroneParams *p, const float *pos, const float *vel,
                     float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                     int32_t *n_coll, const uint8_t *mask, int E, void *stream)
{
    const int rc = check_params(p, E);
    if (rc) return rc;
    if (!pos || !vel || !z || !nbr_idx) return fail(DRONESIM_EINVAL, "dronesim_observe: required buffer is NULL");
    KArgs a = step_args(const_cast<float *>(pos), const_cast<float *>(vel), nullptr, nullptr, reward, true_reward, z, nbr_idx, n_coll, nullptr, 1);
    a.mask = mask;
    return launch(kObserve, p, a, E, stream);
}

int dronesim_reset_observe(const DroneParams *p, const DroneEpisodeCtl *ctl, const uint8_t *mask, float *pos, float *vel,
                           int32_t *t, int32_t *node_out, float *z, int32_t *nbr_idx, int E, void *stream)
{
    int rc = check_params(p, E);
    if (rc) return rc;
    if (!ctl || !ctl->episode) return fail(DRONESIM_EINVAL, "dronesim_reset_observe: ctl with the lattice, seed / env_base and episode is required");
    if (!pos || !vel || !t || !z || !nbr_idx) return fail(DRONESIM_EINVAL, "dronesim_reset_observe: required buffer is NULL");
    KArgs a = step_args(pos, vel, t, nullptr, nullptr, nullptr, z, nbr_idx, nullptr, nullptr, 1);
    if ((rc = check_lattice(ctl->div_x, ctl->div_y, p->N, "bad E / lattice size", &a.lat_M)) != 0) return rc;
    a.mask = mask; a.do_reset = 1; a.node_out = node_out;
    a.acc = reinterpret_cast<double *>(ctl->acc);             // retire the episode in progress (as dronesim_reset_ex does)
    set_stream(ctl, a);
    a.div_y = ctl->div_y; a.pitch = ctl->pitch;
    return launch(kObserve, p, a, E, stream);
}

int dronesim_rollout_ex(const DroneParams *p, const DroneEpisodeCtl *ctl, float *pos, float *vel, int32_t *t,
                        const float *act, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                        int32_t *n_coll, uint8_t *done, int E, int T, void *stream)
{
    int rc = check_params(p, E);
    if (rc) return rc;
    if (T < 0) return fail(DRONESIM_EINVAL, "T < 0");
    if (!pos || !vel || !t || !act || !z || !nbr_idx || !done)
        return fail(DRONESIM_EINVAL, "dronesim_rollout: required buffer is NULL");
    if (T == 0) return DRONESIM_OK;
    KArgs a = step_args(pos, vel, t, act, reward, true_reward, z, nbr_idx, n_coll, done, T);
    a.skin = skin(p);
    if ((rc = apply_ctl(p, ctl, false, a)) != 0) return rc;
    return launch(kRollout, p, a, E, stream);
}

int dronesim_rollout(const DroneParams *p, float *pos, float *vel, int32_t *t, const float *act,
                     float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                     int32_t *n_coll, uint8_t *done, int E, int T, void *stream)
{
    return dronesim_rollout_ex(p, nullptr, pos, vel, t, act, reward, true_reward, z, nbr_idx, n_coll, done, E, T, stream);
}

int dronesim_rollout_random(const DroneParams *p, const DroneEpisodeCtl *ctl, float *pos, float *vel, int32_t *t,
                            float *act_out, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                            int32_t *n_coll, uint8_t *done, int E, int T, void *stream)
{
    int rc = check_params(p, E);
    if (rc) return rc;
    if (T < 0) return fail(DRONESIM_EINVAL, "T < 0");
    if (!ctl || !ctl->episode) return fail(DRONESIM_EINVAL, "dronesim_rollout_random: ctl with seed / env_base / episode is required");
    if (!pos || !vel || !t || !z || !nbr_idx || !done)
        return fail(DRONESIM_EINVAL, "dronesim_rollout_random: required buffer is NULL");
    if (T == 0) return DRONESIM_OK;
    KArgs a = step_args(pos, vel, t, nullptr, reward, true_reward, z, nbr_idx, n_coll, done, T);
    a.skin = skin(p);
    a.act_out = act_out;
    if ((rc = apply_ctl(p, ctl, true, a)) != 0) return rc;
    return launch(kRollout, p, a, E, stream);
}

int dronesim_rollout_control(const DroneParams *p, const DroneEpisodeCtl *ctl, int kind, float u_max,
                             float *pos, float *vel, int32_t *t, float *act_out, float *reward, float *true_reward,
                             float *z, int32_t *nbr_idx, int32_t *n_coll, uint8_t *done, int E, int T, void *stream)
{
    int rc = check_params(p, E);
    if (rc) return rc;
    if (T < 0) return fail(DRONESIM_EINVAL, "T < 0");
    if (kind != DRONESIM_CONTROL_PROPORTIONAL && kind != DRONESIM_CONTROL_GRADIENT)
        return fail(DRONESIM_EINVAL, "unknown controller kind");
    if (!(u_max > 0.0f)) return fail(DRONESIM_EINVAL, "dronesim_rollout_control: u_max must be > 0 (and not NaN)");
    if (!pos || !vel || !t || !z || !nbr_idx || !done)
        return fail(DRONESIM_EINVAL, "dronesim_rollout_control: required buffer is NULL");
    if (T == 0) return DRONESIM_OK;
    KArgs a = step_args(pos, vel, t, nullptr, reward, true_reward, z, nbr_idx, n_coll, done, T);
    a.skin = skin(p);
    a.act_out = act_out;
    a.u_max = u_max;
    if ((rc = apply_ctl(p, ctl, false, a)) != 0) return rc;
    return launch(kRollout, p, a, E, stream, 1 + kind);
}

int dronesim_reset(const DroneParams *p, int div_x, int div_y, float pitch,
                   uint64_t seed, int64_t env_base, const uint8_t *mask,
                   float *pos, float *vel, int32_t *t, int32_t *episode, int32_t *node_out,
                   int E, void *stream)
{
    return reset_impl(p, div_x, div_y, pitch, seed, env_base, mask, pos, vel, t, episode, node_out, nullptr, E, stream);
}

int dronesim_reset_ex(const DroneParams *p, const DroneEpisodeCtl *ctl, const uint8_t *mask,
                      float *pos, float *vel, int32_t *t, int32_t *node_out, int E, void *stream)
{
    if (!ctl) return fail(DRONESIM_EINVAL, "dronesim_reset_ex: ctl is NULL");
    return reset_impl(p, ctl->div_x, ctl->div_y, ctl->pitch, ctl->seed, ctl->env_base, mask, pos, vel, t, ctl->episode,
                      node_out, reinterpret_cast<double *>(ctl->acc), E, stream);
}

int dronesim_episode_reduce(const DroneEpisodeAcc *acc, int E, double *out, void *stream)
{
    if (!acc || !out || E < 0) return fail(DRONESIM_EINVAL, "dronesim_episode_reduce: bad argument");
    hipLaunchKernelGGL(episode_reduce_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const double *>(acc), E, out);
    return dronesim_launched();
}

int dronesim_control(const DroneParams *p, int kind, const float *pos, float *act, float u_max,
                     int E, void *stream)
{
    if (!p) return fail(DRONESIM_EINVAL, "params is NULL");
    if (p->N < 1 || p->N > DRONESIM_MAX_AGENTS) return fail(DRONESIM_EUNSUPPORTED, "N must be in 1..1024");
    if (kind != DRONESIM_CONTROL_PROPORTIONAL && kind != DRONESIM_CONTROL_GRADIENT)
        return fail(DRONESIM_EINVAL, "unknown controller kind");
    if (E < 0 || !pos || !act || !p->xF || !p->d_hat || !p->radius)
        return fail(DRONESIM_EINVAL, "dronesim_control: bad E or NULL buffer");
    if (E == 0) return DRONESIM_OK;
    const Geometry g = geometry(p->N, E);
    CArgs a{};
    a.N = p->N; a.E = E; a.P = g.P; a.epb = g.epb; a.kind = kind; a.u_max = u_max;
    a.xF = p->xF; a.xF_lo = p->xF_lo; a.d_hat = p->d_hat; a.radius = p->radius; a.pos = pos; a.act = act;
    const size_t nw = (size_t)g.threads / kWave;
    size_t lds = sizeof(float2) * (size_t)g.epb * p->N + sizeof(float) * (g.P > 0 ? nw : 1) * p->N;
    // gradient: the cell-mask far filter for envs of >= kBucketMinN agents (one env per wave, or one per workgroup)
    // (needs the bounds d_hat_max / radius_max of DroneParams: a caller that left them unset keeps the all-partner loop)
    const float cell_w = reach_max(p) * 1.001f;
    a.bucket = (kind == DRONESIM_CONTROL_GRADIENT && p->N >= kBucketMinN && g.P <= 1 && p->d_hat_max > 0.0f && p->radius_max >= 0.0f &&
                cell_w > 0.0f && cell_w < 3.0e38f) ? 1 : 0;
    if (a.bucket) {
        lds = (lds + 7) & ~(size_t)7;
        a.tab_off = (int)lds;
        a.inv_cell = 1.0f / cell_w;
        lds += sizeof(unsigned long long) * 2 * kCells * nw;                 // [wave | word][axis][cell]
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (g.P > 0) hipLaunchKernelGGL(control_kernel<true>, dim3(g.blocks), dim3(g.threads), lds, s, a);
    else hipLaunchKernelGGL(control_kernel<false>, dim3(g.blocks), dim3(g.threads), lds, s, a);
    return dronesim_launched();
}

int dronesim_episode_stats(const float *reward, const float *true_reward, const int32_t *n_coll, int E, int N,
                           double *acc, double *scratch, void *stream)
{
    if (!reward || !true_reward || !n_coll || !acc || !scratch || E < 0 || N < 1)
        return fail(DRONESIM_EINVAL, "dronesim_episode_stats: bad argument");
    if (E == 0) return DRONESIM_OK;
    hipLaunchKernelGGL(stats_kernel, dim3(kStatBlocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reward, true_reward, n_coll, E, N, acc, scratch);
    return dronesim_launched();
}

// developer hook (tools/trace_*.py with a -DDRONESIM_TRACE build; not declared in include/dronesim.h): without that build
// the buffer is never handed to a kernel
void dronesim_debug_set_trace(long long *buf) { g_trace = buf; }

// developer hook (tests/test_step_plan_host.py; not declared in include/dronesim.h): the plan of the launch an entry point of mode
// `mode` (enum Mode) would make for these parameters, with the episode layer's parts in use as flagged and z / nbr_idx at
// `z_addr` -> out[12] = (return code, geo, far, epi, threads, epb, LDS bytes, lds_tail, lds_vel, stage5, samp_tbl, bucket); a
// refused launch reports its code only.  No HIP call is made.
void dronesim_debug_step_plan(const DroneParams *p, int mode, int ctrl, int records, int auto_reset, int rand_act, int do_reset,
                              uint64_t z_addr, int E, int64_t *out)
{
    KArgs a{};
    a.acc = records ? reinterpret_cast<double *>(out) : nullptr;      // (never dereferenced: only tested)
    a.auto_reset = auto_reset; a.rand_act = rand_act; a.do_reset = do_reset;
    a.z = reinterpret_cast<float *>(z_addr); a.nbr_idx = reinterpret_cast<int *>(z_addr);
    Geometry g;
    const int rc = plan_step_launch(mode, p, a, E, ctrl, g);
    const int64_t plan[12] = {rc, g.geo, g.far, g.epi, g.threads, g.epb, (int64_t)g.lds, a.lds_tail, a.lds_vel, a.stage5, a.samp_tbl, a.bucket};
    for (int i = 0; i < 12; ++i) out[i] = (i == 0 || rc == 0) ? plan[i] : 0;
}

const char *dronesim_last_error(void) { return g_err; }

const char *dronesim_error_string(int code)
{
    switch (code) {
    case DRONESIM_OK: return "ok";
    case DRONESIM_EINVAL: return "invalid argument";
    case DRONESIM_EUNSUPPORTED: return "unsupported size (N or k beyond the compiled kernels)";
    case DRONESIM_ELAUNCH: return "HIP launch failure";
    default: return "unknown error";
    }
}

int dronesim_version(void) { return DRONESIM_VERSION; }

}   // extern "C"
