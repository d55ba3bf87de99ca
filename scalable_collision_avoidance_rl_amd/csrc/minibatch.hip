// Shuffled minibatches for the PPO learner (include/dronesim.h: dronesim_row_permutation, dronesim_gather_rows): a row
// permutation computed on the device from a counter that lives in device memory, and ONE launch that copies the permuted rows of
// up to eight row-major arrays into minibatch-ordered, block-padded buffers.  Both only enqueue a kernel: no memset node, no
// allocation, no host synchronisation, no atomics -- the results are a pure function of the inputs, and a captured graph replays
// to a fresh permutation whenever the counter has moved.
//
// row_permutation_kernel: one thread per row.  A 4-round balanced Feistel network over [0, 2^(2h)) with Philox4x32-10 as the round
// function, cycle-walked into [0, R): no sort, no scratch, no communication between threads.  The domain is below 4 R, so a thread
// applies the network fewer than four times on average; every application costs four Philox calls (40 rounds).
//
// gather_rows_kernel: the mapping of lanes to bytes.  The learner's rows are short (12 bytes to a few hundred; 1536 at N = 64,
// d_in = 6), so neither a lane per row (a 64-lane request that touches 64 lines for 12 useful bytes each, and a store of the same
// shape) nor a wave per row (3 of 64 lanes busy on a 12-byte row) fits.  Here a lane owns one UNIT -- 16 bytes where the array's
// rows, blocks and base addresses are all multiples of 16, 4 bytes otherwise -- and consecutive lanes own consecutive units of
// the DESTINATION, running on from the end of one row into the next position's row.  A workgroup takes a tile of kTilePos = 64
// consecutive positions of every array: the 64 permutation entries (and the block number of each position) are read once into
// LDS, then the 256 threads sweep the tile's units array by array.  So every store instruction writes 64 consecutive units (1 KiB,
// or 256 B in the 4-byte form: whole lines apart from a block's padding gap), and every load instruction reads whole source rows
// back to back: a wave covers 64 / (units per row) rows per instruction, each row one contiguous segment.  Four units per
// thread are loaded before the first is stored, to keep several scattered reads in flight per lane.
#include "common.hpp"
#include "dronesim.h"

namespace {

constexpr int kMaxArrays = 8;
constexpr int kTilePos = 64;          // positions per workgroup
constexpr int kGatherThreads = 256;
constexpr int kInFlight = 4;          // units per thread loaded ahead of their stores
typedef uint32_t Unit16 __attribute__((ext_vector_type(4)));

// one application of the 4-round network on [0, 2^(2h))
__device__ __forceinline__ uint32_t feistel4(uint32_t v, int h, uint32_t mask, uint32_t ctr, uint32_t k0, uint32_t k1)
{
    uint32_t L = v >> h, Rr = v & mask;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        uint32_t w[4];
        philox4x32_10(Rr, k, ctr, 0u, k0, k1, w);
        const uint32_t n = L ^ (w[0] & mask);
        L = Rr; Rr = n;
    }
    return (L << h) | Rr;
}

__global__ void __launch_bounds__(256) row_permutation_kernel(uint32_t R, int h, uint32_t k0, uint32_t k1,
                                                              const int32_t *__restrict__ counter, int32_t *__restrict__ perm)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;          // (R <= 2^31 - 1: the grid's last thread index is below 2^32)
    if (r >= R) return;
    const uint32_t ctr = (uint32_t)counter[0];
    const uint32_t mask = (1u << h) - 1u;
    uint32_t v = r;
    do {
        v = feistel4(v, h, mask, ctr, k0, k1);
    } while (v >= R);                                            // cycle-walking: r < R lies on a cycle that returns below R
    perm[r] = (int32_t)v;
}

struct GatherArgs {
    const char *src[kMaxArrays];
    char *dst[kMaxArrays];
    long long row_bytes[kMaxArrays];
    long long pad_bytes[kMaxArrays];      // block_bytes - M row_bytes: what every block boundary adds to a destination offset
    uint32_t units_per_row[kMaxArrays];
    uint32_t wide;                        // bit a: array a moves in 16-byte units
    const int32_t *perm;
    int R, M, n_arrays;
};

template <typename Unit>
__device__ __forceinline__ void gather_tile(const char *__restrict__ src, char *__restrict__ dst, long long row_bytes, long long pad,
                                            uint32_t upr, uint32_t units, long long p0, const int *s_row, const int *s_blk)
{
    for (uint32_t u0 = threadIdx.x; u0 < units; u0 += kGatherThreads * kInFlight) {
        Unit val[kInFlight];
        long long to[kInFlight];
#pragma unroll
        for (int q = 0; q < kInFlight; ++q) {
            const uint32_t u = u0 + (uint32_t)q * kGatherThreads;
            const uint32_t pl = u < units ? u / upr : 0u, c = u - pl * upr;
            const int row = u < units ? s_row[pl] : -1;           // (an entry outside [0, R) is skipped, never dereferenced)
            const long long in_row = (long long)c * (long long)sizeof(Unit);
            to[q] = row >= 0 ? (p0 + pl) * row_bytes + (long long)s_blk[pl] * pad + in_row : -1;
            val[q] = row >= 0 ? *reinterpret_cast<const Unit *>(src + (long long)row * row_bytes + in_row) : Unit(0);
        }
#pragma unroll
        for (int q = 0; q < kInFlight; ++q)
            if (to[q] >= 0) *reinterpret_cast<Unit *>(dst + to[q]) = val[q];
    }
}

__global__ void __launch_bounds__(kGatherThreads) gather_rows_kernel(const GatherArgs a)
{
    __shared__ int s_row[kTilePos], s_blk[kTilePos];
    const long long p0 = (long long)blockIdx.x * kTilePos;
    const int npos = (int)((long long)a.R - p0 < kTilePos ? (long long)a.R - p0 : kTilePos);
    if (threadIdx.x < kTilePos) {
        int row = -1, blk = 0;
        if ((int)threadIdx.x < npos) {
            const uint32_t p = (uint32_t)(p0 + threadIdx.x);
            const uint32_t v = (uint32_t)a.perm[p];
            row = v < (uint32_t)a.R ? (int)v : -1;
            blk = (int)(p / (uint32_t)a.M);
        }
        s_row[threadIdx.x] = row; s_blk[threadIdx.x] = blk;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kMaxArrays; ++i) {
        if (i < a.n_arrays) {                                     // (uniform)
            const uint32_t upr = a.units_per_row[i], units = (uint32_t)npos * upr;
            if ((a.wide >> i) & 1u) gather_tile<Unit16>(a.src[i], a.dst[i], a.row_bytes[i], a.pad_bytes[i], upr, units, p0, s_row, s_blk);
            else gather_tile<uint32_t>(a.src[i], a.dst[i], a.row_bytes[i], a.pad_bytes[i], upr, units, p0, s_row, s_blk);
        }
    }
}

}   // namespace

extern "C" {

int dronesim_row_permutation(int R, uint64_t seed, const int32_t *counter, int32_t *perm, void *stream)
{
    if (R < 1 || !counter || !perm) return dronesim_fail(DRONESIM_EINVAL, "dronesim_row_permutation: bad argument (R < 1 or a NULL pointer)");
    int bits = 0;                                                  // bitlen(R - 1)
    for (uint32_t x = (uint32_t)R - 1u; x; x >>= 1) ++bits;
    const int h = bits <= 2 ? 1 : (bits + 1) / 2;                 // max(1, ceil(bits / 2))
    hipLaunchKernelGGL(row_permutation_kernel, dim3((unsigned)(((uint32_t)R + 255u) / 256u)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (uint32_t)R, h, (uint32_t)seed, (uint32_t)(seed >> 32), counter, perm);
    return dronesim_launched();
}

int dronesim_gather_rows(const int32_t *perm, int R, int M, int n_arrays, const void *const *src, void *const *dst,
                         const int64_t *row_bytes, const int64_t *block_bytes, void *stream)
{
    if (!perm || !src || !dst || !row_bytes || !block_bytes) return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: NULL pointer");
    if (R < 1 || M < 1 || R % M != 0) return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: R and M must be >= 1 with R a multiple of M");
    if (n_arrays < 1 || n_arrays > kMaxArrays) return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: n_arrays must be in 1..8");
    GatherArgs a = {};
    a.perm = perm; a.R = R; a.M = M; a.n_arrays = n_arrays;
    for (int i = 0; i < n_arrays; ++i) {
        const int64_t rb = row_bytes[i], bb = block_bytes[i];
        if (!src[i] || !dst[i]) return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: NULL array pointer");
        if (rb < 4 || rb % 4 != 0 || rb > DRONESIM_GATHER_MAX_ROW_BYTES)
            return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: a row size must be a positive multiple of 4 (at most DRONESIM_GATHER_MAX_ROW_BYTES)");
        if (bb < (int64_t)M * rb) return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: block_bytes below M * row_bytes");
        if ((reinterpret_cast<uintptr_t>(src[i]) | reinterpret_cast<uintptr_t>(dst[i]) | (uintptr_t)bb) & 3u)
            return dronesim_fail(DRONESIM_EINVAL, "dronesim_gather_rows: arrays and block sizes must be 4-byte aligned");
        const bool wide = ((reinterpret_cast<uintptr_t>(src[i]) | reinterpret_cast<uintptr_t>(dst[i]) | (uintptr_t)bb | (uintptr_t)rb) & 15u) == 0;
        a.src[i] = static_cast<const char *>(src[i]); a.dst[i] = static_cast<char *>(dst[i]);
        a.row_bytes[i] = rb; a.pad_bytes[i] = bb - (int64_t)M * rb;
        a.units_per_row[i] = (uint32_t)(rb / (wide ? 16 : 4));    // (kTilePos units_per_row < 2^32 by the row-size limit)
        a.wide |= (wide ? 1u : 0u) << i;
    }
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(((int64_t)R + kTilePos - 1) / kTilePos)), dim3(kGatherThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return dronesim_launched();
}

}   // extern "C"
