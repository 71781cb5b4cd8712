// dist_readout.hip — readout of a sharded state (dist.hip): the kernels that sample a state which
// is permuted (logical -> physical map `perm`) and split by rank, without gathering it.
//
// A chunk is the 2^c amplitudes that share all LOGICAL index bits >= c (c = min(12, L), the
// logical-order counterpart of reduce.hip's kChunkLog).  The sampler (qsim_dist_sample) first
// brings logical qubits 0 .. c-1 to local positions, so every chunk lies wholly on one rank; then
//   k_dist_chunk_partials + k_dist_chunk_finish : |a|^2 summed per chunk, one streaming pass over
//       the shard in physically contiguous 1 KiB runs (64 lanes x 16 B), no floating-point
//       atomics, every addition in a fixed order (bitwise reproducible, transport-independent);
//   k_dist_chunk_search : one wavefront per shot scans its chunk in logical order (the scan of
//       reduce.hip's k_chunk_search, addressed through the map).
// The chunk CDF and the per-shot targets in between are the host step the single-GPU sampler
// uses (chunk_targets, reduce.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "qsim_hip.h"

namespace qsim_hip {

// ---- host-only layout decisions ---------------------------------------------------------------

int dist_chunk_log(int L) { return std::min(L, kDistChunkLog); }

uint64_t dist_localize_mask(int n, int L, int c, const int* perm) {
    (void)n;
    uint64_t m = 0;
    for (int q = 0; q < c; ++q)
        if (perm[q] >= L) m |= 1ull << q;
    return m;
}

ChunkMap make_chunk_map(int n, int L, int c, int rank, const int* perm) {
    ChunkMap m{};
    m.L = L;
    m.c = c;
    std::vector<int> inv(n, -1);
    for (int q = 0; q < n; ++q) {
        if (perm[q] < 0 || perm[q] >= n || inv[perm[q]] >= 0) fail(QSIM_ERR_RUNTIME, "qubit map is not a permutation");
        inv[perm[q]] = q;
    }
    for (int q = 0; q < c; ++q) {
        if (perm[q] >= L) fail(QSIM_ERR_RUNTIME, "chunk qubit left on a rank position");
        m.amask |= 1ull << perm[q];
        m.pos[q] = (int8_t)perm[q];
    }
    int k = 0;  // slot bit k: the k-th local position (ascending) outside amask
    for (int p = 0; p < L; ++p)
        if (!((m.amask >> p) & 1ull)) m.dst[k++] = (int8_t)(inv[p] - c);
    if (k != L - c) fail(QSIM_ERR_RUNTIME, "chunk slot count mismatch");
    for (int p = L; p < n; ++p)
        if ((rank >> (p - L)) & 1) m.rank_or |= 1ull << (inv[p] - c);
    return m;
}

// ---- chunk sums -----------------------------------------------------------------------------
//
// Local positions split four ways: lane bits (positions 0..5: one 1 KiB run per wave load) inside
// or outside amask, and positions >= 6 inside (I: iterated, the same chunk) or outside (G: the
// block's group, other chunks).  Block (g, s) sums, for group g, the s-th share of the 2^|I| runs:
// its 4 waves take consecutive quarters, accumulate per lane, fold the lane bits inside amask with
// an xor butterfly (both partners add the same two numbers: the same result), and the block adds
// its 4 wave sums in wave order.  Lanes whose amask lane bits are 0 then hold one partial each,
// for slot (g, lane bits outside amask).  k_dist_chunk_finish adds a slot's partials in split
// order and stores the total at the slot's global chunk id.
__device__ __forceinline__ uint64_t deposit_dev(uint64_t v, uint64_t mask) {
    uint64_t r = 0;
    for (; mask && v; mask &= mask - 1, v >>= 1)
        if (v & 1ull) r |= mask & (0 - mask);
    return r;
}

__global__ __launch_bounds__(256) void k_dist_chunk_partials(const double2* st, int L, uint64_t amask,
                                                             int splits_log, uint64_t nslots,
                                                             double* partials) {
    __shared__ double wsum[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lane_bits = L < 6 ? L : 6;
    const uint64_t all = (1ull << L) - 1ull;
    const uint64_t imask = amask & ~63ull;          // iterated: same chunk
    const uint64_t gmask = ~amask & ~63ull & all;   // group: other chunks
    const uint64_t runs = 1ull << __popcll(imask);  // runs of one group
    const uint64_t per_block = runs >> splits_log;  // (the launcher keeps splits <= runs)
    uint64_t first, count;  // this wave's share of the block's runs
    if (per_block >= 4) {
        count = per_block >> 2;
        first = (uint64_t)blockIdx.y * per_block + (uint64_t)wave * count;
    } else {
        count = (uint64_t)wave < per_block ? 1 : 0;
        first = (uint64_t)blockIdx.y * per_block + (uint64_t)wave;
    }
    const uint64_t gbase = deposit_dev((uint64_t)blockIdx.x, gmask);
    double acc = 0.0;
    if (lane < (1 << lane_bits) && count) {
        uint64_t it = deposit_dev(first, imask);
#pragma unroll 4
        for (uint64_t k = 0; k < count; ++k) {
            const double2 a = st[gbase | it | (uint64_t)lane];
            acc += a.x * a.x + a.y * a.y;
            it = ((it | ~imask) + 1ull) & imask;  // next value of the iterated bits
        }
    }
#pragma unroll
    for (int b = 0; b < 6; ++b)
        if ((amask >> b) & 1ull) acc += __shfl_xor(acc, 1 << b);
    wsum[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && lane < (1 << lane_bits) && !((uint64_t)lane & amask)) {
        const uint64_t out_lanes = ~amask & ((1ull << lane_bits) - 1ull);
        uint64_t sub = 0;  // the lane bits outside amask, compacted
        int j = 0;
        for (uint64_t m = out_lanes; m; m &= m - 1, ++j) {
            const int b = __ffsll((long long)m) - 1;
            sub |= (((uint64_t)lane >> b) & 1ull) << j;
        }
        const uint64_t slot = ((uint64_t)blockIdx.x << __popcll(out_lanes)) | sub;
        if (slot < nslots)
            partials[(uint64_t)blockIdx.y * nslots + slot] =
                (wsum[0][lane] + wsum[1][lane]) + (wsum[2][lane] + wsum[3][lane]);
    }
}

__global__ __launch_bounds__(256) void k_dist_chunk_finish(const double* partials, uint64_t nslots, int splits,
                                                           ChunkMap m, uint64_t nchunks, double* sums) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nslots; j += step) {
        double acc = 0.0;
        for (int s = 0; s < splits; ++s) acc += partials[(uint64_t)s * nslots + j];
        uint64_t id = m.rank_or;
        for (int k = 0; k < m.L - m.c; ++k) id |= ((j >> k) & 1ull) << m.dst[k];
        if (id < nchunks) sums[id] = acc;
    }
}

size_t dist_chunk_partials_count(const ChunkMap& m, int* splits_log_out) {
    const uint64_t all = (1ull << m.L) - 1ull;
    const int ni = __builtin_popcountll(m.amask & ~63ull);
    const int ng = __builtin_popcountll(~m.amask & ~63ull & all);
    // enough blocks to fill the device, at least 4 runs (one per wave) each
    int sl = 0;
    while (ng + sl < 11 && sl + 2 < ni) ++sl;
    if (splits_log_out) *splits_log_out = sl;
    return ((size_t)1 << sl) << (m.L - m.c);
}

void launch_dist_chunk_sums(const double2* st, const ChunkMap& m, uint64_t nchunks, double* d_partials,
                            double* d_sums, hipStream_t s) {
    int sl = 0;
    (void)dist_chunk_partials_count(m, &sl);
    const uint64_t all = (1ull << m.L) - 1ull;
    const int ng = __builtin_popcountll(~m.amask & ~63ull & all);
    const uint64_t nslots = 1ull << (m.L - m.c);
    if (ng > 30) fail(QSIM_ERR_RUNTIME, "too many chunk groups for one launch");
    hipLaunchKernelGGL(k_dist_chunk_partials, dim3(1u << ng, 1u << sl), dim3(256), 0, s, st, m.L, m.amask, sl,
                       nslots, d_partials);
    QSIM_HIPCHK(hipGetLastError());
    const unsigned blocks = (unsigned)std::min<uint64_t>((nslots + 255) / 256, 4096);
    hipLaunchKernelGGL(k_dist_chunk_finish, dim3(blocks), dim3(256), 0, s, d_partials, nslots, 1 << sl, m, nchunks,
                       d_sums);
    QSIM_HIPCHK(hipGetLastError());
}

// ---- in-chunk search ------------------------------------------------------------------------
//
// One wavefront per job: the first logical in-chunk index i whose prefix of |a|^2 reaches the
// target (k_chunk_search's scan: 2^c / 64 consecutive indices per lane, a wave scan of the lane
// sums, then the first lane that reaches the target walks its own indices).  Logical index i sits
// at local offset base | deposit(i): bit k of i at position pos[k].  The result, hi | i, is stored
// as a double (exact: below 2^53) so the ranks' outputs combine in one all-reduce.
__device__ __forceinline__ uint64_t chunk_offset(const ChunkMap& m, uint64_t i) {
    uint64_t r = 0;
    for (int k = 0; k < m.c; ++k) r |= ((i >> k) & 1ull) << m.pos[k];
    return r;
}

__global__ __launch_bounds__(64) void k_dist_chunk_search(const double2* st, ChunkMap m, const ShotJob* jobs,
                                                          int count, int shots, double* out) {
    const int s = blockIdx.x;
    if (s >= count) return;
    const ShotJob job = jobs[s];
    const int lane = threadIdx.x;
    const uint64_t chunk = 1ull << m.c;
    const uint64_t per = (chunk + 63) / 64;  // consecutive logical indices per lane
    if (job.base >> m.L || job.shot < 0 || job.shot >= shots) return;  // (never: host-built jobs)
    double mine = 0.0;
    for (uint64_t k = 0; k < per; ++k) {
        const uint64_t i = (uint64_t)lane * per + k;
        if (i < chunk) {
            const double2 a = st[job.base | chunk_offset(m, i)];
            mine += a.x * a.x + a.y * a.y;
        }
    }
    double incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    const double r = job.target;
    const unsigned long long ball = __ballot(incl >= r);
    const int first = ball ? __ffsll((long long)ball) - 1 : 63;  // rounding: clamp to last lane
    if (lane == first) {
        double acc = incl - mine;
        uint64_t found = (uint64_t)lane * per + per - 1;
        for (uint64_t k = 0; k < per; ++k) {
            const uint64_t i = (uint64_t)lane * per + k;
            if (i >= chunk) break;
            const double2 a = st[job.base | chunk_offset(m, i)];
            acc += a.x * a.x + a.y * a.y;
            if (acc >= r) {
                found = i;
                break;
            }
        }
        if (found >= chunk) found = chunk - 1;
        out[job.shot] = (double)(job.hi | found);
    }
}

void launch_dist_chunk_search(const double2* st, const ChunkMap& m, const ShotJob* d_jobs, int count, int shots,
                              double* d_out, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_dist_chunk_search, dim3((unsigned)count), dim3(64), 0, s, st, m, d_jobs, count, shots,
                       d_out);
    QSIM_HIPCHK(hipGetLastError());
}

}  // namespace qsim_hip
