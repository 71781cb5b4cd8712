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
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "device_ops.hpp"
#include "dist_state.hpp"

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

// Physical (rank-major) amplitudes -> logical index order (dst: 2 * 2^n doubles).  The map
// i -> p(i) moves bit q to perm[q], so p is the OR of per-11-bit-chunk tables; threads split i.
template <typename Put>
void unpermute_each(const qsim_dist* d, Put&& put) {
    const int n = d->n, nch = (n + 10) / 11;
    std::vector<uint64_t> tab((size_t)nch << 11, 0);
    for (int c = 0; c < nch; ++c)
        for (uint64_t v = 0; v < 2048; ++v)
            for (int b = 0; b < 11 && c * 11 + b < n; ++b)
                if ((v >> b) & 1ull) tab[((size_t)c << 11) + v] |= 1ull << d->perm[c * 11 + b];
    const uint64_t N = 1ull << n;
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(16, N >> 16));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            for (uint64_t i = N * t / T; i < N * (t + 1) / T; ++i) {
                uint64_t p = 0;
                for (int c = 0; c < nch; ++c) p |= tab[((size_t)c << 11) + ((i >> (11 * c)) & 2047)];
                put(i, p);
            }
        });
    for (auto& x : th) x.join();
}
void unpermute(const qsim_dist* d, const std::vector<double2>& phys, double* dst) {
    unpermute_each(d, [&](uint64_t i, uint64_t p) {
        dst[2 * i] = phys[p].x;
        dst[2 * i + 1] = phys[p].y;
    });
}

static double prob_bit_zero(qsim_dist* d, int q) {
    const int p = d->perm[q];
    double local = 0.0;
    for (const Shard& s : d->shards) {
        if (p < d->L) local += reduce_norm(s.d, d->L, p, d->d_partials, d->d_result, d->stream);
        else if (!((s.rank >> (p - d->L)) & 1))
            local += reduce_norm(s.d, d->L, -1, d->d_partials, d->d_result, d->stream);
    }
    return allreduce_sum(d, local);
}

// Zero the amplitudes whose logical bit q != result, scale the rest; the layout stays.
static void collapse_bit(qsim_dist* d, int q, int result, double scale) {
    const int p = d->perm[q];
    for (const Shard& s : d->shards) {
        if (p < d->L) {
            launch_collapse(s.d, d->L, p, result, scale, d->stream);
            continue;
        }
        // the whole shard shares the bit: k_collapse on a bit above the shard reads 0 everywhere,
        // so result 0 scales every amplitude and result 1 zeroes every amplitude
        const int mine = (s.rank >> (p - d->L)) & 1;
        launch_collapse(s.d, d->L, 63, mine == result ? 0 : 1, scale, d->stream);
    }
    stream_wait(d, d->stream);
}

// Bring logical qubits 0 .. c-1 to local positions with one remap: each one on a rank position
// trades places with a logical qubit >= c on the highest local positions (long pack runs).  Pure
// copies (pack, transfer, unpack): amplitudes keep their bits, only the map changes.
static void localize_low(qsim_dist* d, int c) {
    std::vector<int> out;
    for (int q = 0; q < c; ++q)
        if (d->perm[q] >= d->L) out.push_back(q);
    if (out.empty()) return;
    std::vector<int> inv(d->n);
    for (int q = 0; q < d->n; ++q) inv[d->perm[q]] = q;
    std::vector<int> in;
    for (int p = d->L - 1; p >= 0 && in.size() < out.size(); --p)
        if (inv[p] >= c) in.push_back(inv[p]);
    if (in.size() != out.size() || out.size() > 8) fail(QSIM_ERR_RUNTIME, "sampler: no remap localizes the chunk qubits");
    DStep ex;
    ex.kind = 1;
    ex.k = (int)out.size();
    for (int j = 0; j < ex.k; ++j) {
        ex.gpos[j] = d->perm[out[j]];
        ex.lpos[j] = d->perm[in[j]];
    }
    exchange(d, ex, std::vector<char>(d->shards.size(), 0));
    for (int j = 0; j < ex.k; ++j) {
        d->perm[out[j]] = ex.lpos[j];
        d->perm[in[j]] = ex.gpos[j];
    }
    stream_wait(d, d->stream);
}

// The sampler (qsim_dist_sample; see the top of this file).  Every rank computes the same chunk
// totals (all-reduced), hence the same chunk and target per shot; a shot's chunk is searched by
// the rank that owns it, and the indices are combined by a second all-reduce.
static void sample_dist(qsim_dist* d, const double* uniforms, int shots, int64_t* out) {
    const int n = d->n, L = d->L, c = dist_chunk_log(L);
    localize_low(d, c);
    const uint64_t nchunks = 1ull << (n - c);
    std::vector<ChunkMap> maps;
    size_t npart = 0;
    for (const Shard& sh : d->shards) {
        maps.push_back(make_chunk_map(n, L, c, sh.rank, d->perm.data()));
        npart = std::max(npart, dist_chunk_partials_count(maps.back()));
    }
    // scratch = [chunk sums][partials][jobs][index of shot (double)]
    const size_t b_sums = nchunks * sizeof(double), b_part = npart * sizeof(double);
    const size_t b_jobs = (size_t)shots * sizeof(ShotJob), b_out = (size_t)shots * sizeof(double);
    char* base = (char*)d->readout.get(b_sums + b_part + b_jobs + b_out, d->stream);
    double* d_sums = (double*)base;
    double* d_part = (double*)(base + b_sums);
    ShotJob* d_jobs = (ShotJob*)(base + b_sums + b_part);
    double* d_out = (double*)(base + b_sums + b_part + b_jobs);
    QSIM_HIPCHK(hipMemsetAsync(d_sums, 0, b_sums, d->stream));
    for (size_t i = 0; i < d->shards.size(); ++i) {
        TimedLaunch tl(&d->timer, "dist_chunk_sums", 16.0 * (double)(1ull << L), d->stream);
        launch_dist_chunk_sums(d->shards[i].d, maps[i], nchunks, d_part, d_sums, d->stream);
    }
    std::vector<double> sums(nchunks);
    allreduce_vec(d, d_sums, nchunks, sums.data());
    std::vector<int64_t> chunk_of(shots);
    std::vector<double> target(shots);
    chunk_targets(sums.data(), nchunks, uniforms, shots, chunk_of.data(), target.data());
    // jobs grouped by owning shard (shard order), one upload
    std::vector<std::vector<ShotJob>> per(d->shards.size());
    for (int s = 0; s < shots; ++s) {
        if (chunk_of[s] < 0) continue;
        uint64_t phys = 0;
        for (int b = 0; b < n - c; ++b)
            if (((uint64_t)chunk_of[s] >> b) & 1ull) phys |= 1ull << d->perm[c + b];
        const int owner = (int)(phys >> L);
        for (size_t i = 0; i < d->shards.size(); ++i)
            if (d->shards[i].rank == owner)
                per[i].push_back({phys & ((1ull << L) - 1ull), (uint64_t)chunk_of[s] << c, target[s], (int64_t)s});
    }
    std::vector<ShotJob> jobs;
    for (const auto& v : per) jobs.insert(jobs.end(), v.begin(), v.end());
    if (!jobs.empty())
        QSIM_HIPCHK(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(ShotJob), hipMemcpyHostToDevice, d->stream));
    QSIM_HIPCHK(hipMemsetAsync(d_out, 0, b_out, d->stream));
    size_t at = 0;
    for (size_t i = 0; i < d->shards.size(); ++i) {
        TimedLaunch tl(&d->timer, "dist_chunk_search", 0.0, d->stream);
        launch_dist_chunk_search(d->shards[i].d, maps[i], d_jobs + at, (int)per[i].size(), shots, d_out, d->stream);
        at += per[i].size();
    }
    std::vector<double> idx(shots);
    allreduce_vec(d, d_out, (size_t)shots, idx.data());
    for (int s = 0; s < shots; ++s) out[s] = chunk_of[s] < 0 ? (int64_t)(1ull << n) : (int64_t)idx[s];
}

}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_dist_total_probability(qsim_dist* d, double* out) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        double local = 0.0;
        for (const Shard& s : d->shards)
            local += reduce_norm(s.d, d->L, -1, d->d_partials, d->d_result, d->stream);
        *out = allreduce_sum(d, local);
    });
}

int qsim_dist_prob_bit_zero(qsim_dist* d, int q, double* out) {
    return dguard_comm(d, [&] {
        need(d);
        QSIM_HIPCHK(hipSetDevice(d->device));
        flush_carry(d);  // (the previous run's last step, if it was left pending)
        if (q < 0 || q >= d->n) fail(QSIM_ERR_INVALID_ARGUMENT, "bit out of range");
        QSIM_HIPCHK(hipSetDevice(d->device));
        *out = prob_bit_zero(d, q);
    });
}

int qsim_dist_probabilities(qsim_dist* d, double* dst) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        const uint64_t shard = 1ull << d->L;
        const bool root = d->virt || d->shards[0].rank == 0;
        // |a|^2 per shard on the device, then the gather of qsim_dist_gather_state at 8 B per
        // amplitude: rank 0 collects the shards in rank order (physical order) and un-permutes
        const bool staged = root && !d->virt && d->transport != qsim_dist::T_HOSTED && d->world > 1;
        double* dp = (double*)d->readout.get(sizeof(double) * (staged ? (shard << d->g) : shard), d->stream);
        std::vector<double> phys(root ? (1ull << d->n) : shard);
        if (d->virt) {
            for (const Shard& s : d->shards) {
                launch_probabilities(s.d, shard, dp, d->stream);
                QSIM_HIPCHK(hipMemcpyAsync(phys.data() + s.rank * shard, dp, sizeof(double) * shard,
                                           hipMemcpyDeviceToHost, d->stream));
            }
            stream_wait(d, d->stream);
        } else if (d->transport == qsim_dist::T_HOSTED) {
            launch_probabilities(d->shards[0].d, shard, dp, d->stream);
            QSIM_HIPCHK(hipMemcpyAsync(phys.data(), dp, sizeof(double) * shard, hipMemcpyDeviceToHost, d->stream));
            QSIM_HIPCHK(hipStreamSynchronize(d->stream));
            std::vector<qsim_dist_post> hp;
            if (root)
                for (int r = 1; r < d->world; ++r)
                    hp.push_back({r, 0, sizeof(double) * shard, nullptr, phys.data() + r * shard});
            else
                hp.push_back({0, 0, sizeof(double) * shard, phys.data(), nullptr});
            if (!hp.empty()) host_call(d, hp, "gather of probabilities");
        } else {
            launch_probabilities(d->shards[0].d, shard, dp, d->stream);
            if (d->world > 1) {
                QSIM_NCCLCHK(ncclGroupStart());
                if (root)
                    for (int r = 1; r < d->world; ++r)
                        QSIM_NCCLCHK(ncclRecv(dp + r * shard, shard, ncclDouble, r, d->comm, d->stream));
                else
                    QSIM_NCCLCHK(ncclSend(dp, shard, ncclDouble, 0, d->comm, d->stream));
                QSIM_NCCLCHK(ncclGroupEnd());
                comm_settle(d, "gather of probabilities");
            }
            if (root)
                QSIM_HIPCHK(hipMemcpyAsync(phys.data(), dp, sizeof(double) << d->n, hipMemcpyDeviceToHost, d->stream));
            stream_wait(d, d->stream);
        }
        if (root && dst) unpermute_each(d, [&](uint64_t i, uint64_t p) { dst[i] = phys[p]; });
    });
}

int qsim_dist_sample(qsim_dist* d, const double* uniforms, int shots, int64_t* out) {
    return dguard_comm(d, [&] {
        need(d);
        if (shots <= 0) return;
        if (!uniforms || !out) fail(QSIM_ERR_INVALID_ARGUMENT, "null buffer");
        flush_on_device(d);
        sample_dist(d, uniforms, shots, out);
    });
}

int qsim_dist_collapse(qsim_dist* d, int logical_bit, int result, double scale) {
    return dguard_comm(d, [&] {
        need(d);
        if (logical_bit < 0 || logical_bit >= d->n) fail(QSIM_ERR_INVALID_ARGUMENT, "bit out of range");
        if (result != 0 && result != 1) fail(QSIM_ERR_INVALID_ARGUMENT, "result must be 0 or 1");
        flush_on_device(d);
        d->fresh = false;
        collapse_bit(d, logical_bit, result, scale);
    });
}

int qsim_dist_measure(qsim_dist* d, int logical_bit, double u, int* result) {
    return dguard_comm(d, [&] {
        need(d);
        if (!result) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (logical_bit < 0 || logical_bit >= d->n) fail(QSIM_ERR_INVALID_ARGUMENT, "bit out of range");
        flush_on_device(d);
        // p0 is all-reduced (the same on every rank) and u is the same by contract: every rank
        // decides alike
        const double p0 = prob_bit_zero(d, logical_bit);
        const int r = u < p0 ? 0 : 1;
        const double pr = r == 0 ? p0 : 1.0 - p0;
        if (pr < 1e-15)
            fail(QSIM_ERR_RUNTIME, "Measurement result " + std::to_string(r) + " has zero probability");
        d->fresh = false;
        collapse_bit(d, logical_bit, r, 1.0 / std::sqrt(pr));
        *result = r;
    });
}

int qsim_dist_sample_plan(int n_qubits, int world, const int32_t* perm, int* chunk_log, uint64_t* localize_mask) {
    return guarded([&] {
        const int L = HostPlanArgs(n_qubits, world).L, c = dist_chunk_log(L);
        if (!perm) fail(QSIM_ERR_INVALID_ARGUMENT, "null qubit map");
        const std::vector<int> p = checked_perm(n_qubits, perm);
        if (chunk_log) *chunk_log = c;
        if (localize_mask) *localize_mask = dist_localize_mask(n_qubits, L, c, p.data());
    });
}

}  // extern "C"
