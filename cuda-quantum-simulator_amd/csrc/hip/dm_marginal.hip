// dm_marginal.hip — marginal probabilities and reduced density matrices of a subset of qubits, and
// the fidelity <psi|rho|psi>, of a density matrix, computed where rho lies (no readback, no layout
// restore).  No reference counterpart: a caller of the reference copies the 4^n elements to the host.
//
// rho of n qubits lives in a 2n-bit state: amplitude i * 2^n + j holds rho[i][j].  Logical index bit
// q is the column bit of qubit q, logical bit q + n its row bit (as in dm_expect.hip); the state's
// permutation maps these 2n logical bits to physical positions.  Qubit q is index bit q (the gates'
// and PauliSum's convention); for the k listed qubits (any order, distinct), bit j of an output
// index is qubit qubits[j]:
//     marginal:  out[m]       = sum_b Re rho[(m, b)][(m, b)]
//     matrix:    rho_A[a][a'] = sum_b rho[(a, b)][(a', b)]
//     fidelity:  F            = Re sum_ij conj(psi_i) rho[i][j] psi_j
// All three are linear functionals of whatever the buffer holds: every element the formula names is
// summed, nothing is mirrored or symmetrised, Hermiticity is not assumed.  Every sum is added in an
// order fixed by (n, k, the physical positions): no floating-point atomics, two calls return
// identical doubles.
//
// The subset readers are one gather-reduce (engine.hpp: DmMarginalPlan).  The host lowering turns a
// request into address generators, masks over the 2n physical positions: one per output index bit
// (the matrix: 2k single positions, the row position of q_j for bit j of a and its column position
// for bit j of a'; the marginal: k masks of both positions) and one per unselected qubit (both
// positions).  The address of term b of output o is the OR of the generators at the set bits of o
// and of b.  All generators are sorted by their lowest position; the lowest (at most 8) are the bits
// of the thread index, so where positions 0, 1, ... are single-position generators neighbouring lanes
// read neighbouring 16 B (a two-position generator is never contiguous).  Of the others, the sum
// generators are looped over by each thread into one accumulator (cut into slices over work-groups)
// and the out generators choose the work-group.  The work-group then adds, per output it holds, the
// threads that differ in sum generators, in ascending order through LDS, and writes its partial
// outputs once; k_fold_partials (marginal.hip) adds the slices in a fixed order and stores each
// output at its place in the caller's bit order.  At most 2^(n+k) <= 2^21 elements are read.
//
// The fidelity is the streaming kernel: one pass over all 4^n elements in physical address order.  A
// run is 2^c contiguous elements (c = min(2n, 12)); thread t of the 256 reads elements j * 256 + t
// of a run, j < 16, so every load instruction of a wave moves 1 KiB of consecutive addresses (as
// k_marginal_partial).  Of a run's c low positions t_r are row bits and t_c column bits, so it
// touches 2^t_r values of i and 2^t_c of j: those entries of psi (a 2^n * 16 B table in device
// scratch, at most 512 KiB: it stays in L2) are staged in LDS per run, and an element costs two
// LDS reads instead of two table reads.  The in-run part of both table indices is fixed per thread
// and j (computed before the loop), the part from the run's high positions is uniform in the
// work-group.  Each thread accumulates Re(conj(psi_i) rho_ij psi_j); block_sum and
// launch_sum_partials add the threads and the work-groups as k_dm_expect_partial's are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"

namespace qsim_hip {

// perm (null: identity) as positions of the 2n logical bits, checked.
static std::vector<int> dm_positions(int n, const int* perm) {
    if (n < 1 || n > QSIM_DM_MAX_QUBITS) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
    std::vector<int> pos(2 * n);
    uint64_t seen = 0;
    for (int b = 0; b < 2 * n; ++b) {
        const int p = perm ? perm[b] : b;
        if (p < 0 || p >= 2 * n || (seen >> p & 1ull))
            fail(QSIM_ERR_INVALID_ARGUMENT, "perm is not a permutation of the 2n index bits");
        seen |= 1ull << p;
        pos[b] = p;
    }
    return pos;
}

DmMarginalPlan lower_dm_marginal(int n, const int32_t* qubits, int k, const int* perm, bool rdm) {
    const std::vector<int> pos = dm_positions(n, perm);
    if (k < 0 || k > (rdm ? kRdmMaxQubits : kMarginalMaxQubits) || k > n)
        fail(QSIM_ERR_INVALID_ARGUMENT, "too many qubits for this reader");
    if (k > 0 && !qubits) fail(QSIM_ERR_INVALID_ARGUMENT, "null qubit list");
    DmMarginalPlan p;
    p.n = n;
    p.k = k;
    p.rdm = rdm;
    p.out_gen.resize(rdm ? 2 * k : k);
    uint32_t seen = 0;
    for (int j = 0; j < k; ++j) {
        const int q = qubits[j];
        if (q < 0 || q >= n) fail(QSIM_ERR_OUT_OF_RANGE, "qubit index out of range");
        if (seen >> q & 1u) fail(QSIM_ERR_INVALID_ARGUMENT, "duplicate qubit");
        seen |= 1u << q;
        const uint64_t col = 1ull << pos[q], row = 1ull << pos[q + n];
        if (rdm) {
            p.out_gen[j] = col;
            p.out_gen[k + j] = row;
        } else {
            p.out_gen[j] = row | col;
        }
    }
    for (size_t j = 0; j < p.out_gen.size(); ++j) p.sorted.push_back(DmGatherGen{p.out_gen[j], (int)j});
    for (int q = 0; q < n; ++q) {
        if (seen >> q & 1u) continue;
        p.sum_gen.push_back(1ull << pos[q] | 1ull << pos[q + n]);
        p.sorted.push_back(DmGatherGen{p.sum_gen.back(), -1});
    }
    // (the generators' positions are disjoint, so the lowest positions are distinct)
    std::sort(p.sorted.begin(), p.sorted.end(), [](const DmGatherGen& a, const DmGatherGen& b) {
        return __builtin_ctzll(a.mask) < __builtin_ctzll(b.mask);
    });
    p.nt = std::min<int>((int)p.sorted.size(), kDmGatherThreadBits);
    int nloop = 0, nhigh = 0;
    for (size_t i = p.nt; i < p.sorted.size(); ++i) ++(p.sorted[i].out_bit < 0 ? nloop : nhigh);
    p.s_log = std::min(nloop, std::max(0, kDmGatherGroupsLog - nhigh));
    p.groups = 1ull << (nhigh + p.s_log);
    p.elements = 1ull << (n - k + (int)p.out_gen.size());
    p.scratch_bytes = ((uint64_t)(rdm ? 2 : 1) * sizeof(double) << p.out_gen.size()) << p.s_log;
    return p;
}

DmFidelityPlan lower_dm_fidelity(int n, const int* perm) {
    const std::vector<int> pos = dm_positions(n, perm);
    DmFidelityPlan p;
    p.n = n;
    for (int b = 0; b < 2 * n; ++b) {
        p.qubit[pos[b]] = (int8_t)(b < n ? b : b - n);
        if (b >= n) p.row_mask |= 1u << pos[b];
    }
    p.c = std::min(2 * n, 12);
    for (;;) {
        p.t_r = __builtin_popcount(p.row_mask & ((1u << p.c) - 1u));
        p.t_c = p.c - p.t_r;
        if ((1 << p.t_r) + (1 << p.t_c) <= kDmFidelityTable) break;
        --p.c;  // (all twelve low positions of one kind: eleven of them)
    }
    p.runs = 1ull << (2 * n - p.c);
    p.groups = (unsigned)std::min<uint64_t>(p.runs, kDmFidelityGroups);
    return p;
}

namespace {

struct GatherArgs {
    int nt, no_t, nloop, nhigh, s_log;
    uint32_t t_sum;     // the thread bits that are sum generators
    uint64_t tgen[8];   // thread bits
    uint64_t lgen[16];  // the looped sum generators
    uint64_t hgen[16];  // the out generators that choose the work-group
};

__device__ __forceinline__ uint64_t gen_or(uint32_t v, int count, const uint64_t* gen) {
    uint64_t a = 0;
    for (int i = 0; i < count; ++i)
        if (v >> i & 1u) a |= gen[i];
    return a;
}

// Bit i of v moved to the i-th lowest set bit of mask.
__device__ __forceinline__ uint32_t spread_bits(uint32_t v, uint32_t mask) {
    uint32_t r = 0;
    for (; mask; mask &= mask - 1u, v >>= 1)
        if (v & 1u) r |= mask & (0u - mask);
    return r;
}

// Work-group (h, slice): partials[slice][h << no_t | o] for the 2^no_t outputs o its threads hold.
template <bool CPLX>
__global__ __launch_bounds__(256) void k_dm_gather(const double2* __restrict__ rho, GatherArgs a,
                                                   double* __restrict__ partials) {
    __shared__ double2 part[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t slice = blockIdx.x & ((1u << a.s_log) - 1u);
    const uint32_t h = blockIdx.x >> a.s_log;
    const uint32_t per = 1u << (a.nloop - a.s_log);
    double2 acc = make_double2(0.0, 0.0);
    if (tid < (1u << a.nt)) {
        // every generator holds positions below 2n only, so every address is below 4^n
        const uint64_t base = gen_or(tid, a.nt, a.tgen) | gen_or(h, a.nhigh, a.hgen);
        const uint32_t end = (slice + 1u) * per;
        for (uint32_t b = slice * per; b < end; b += 4u) {
            double2 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                v[i] = b + i < end ? rho[base | gen_or(b + i, a.nloop, a.lgen)] : make_double2(0.0, 0.0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc.x += v[i].x;
                if (CPLX) acc.y += v[i].y;
            }
        }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < (1u << a.no_t)) {
        const uint32_t t_out = ((1u << a.nt) - 1u) & ~a.t_sum;
        const uint32_t r0 = spread_bits(tid, t_out);
        double2 v = part[r0];
        for (uint32_t sb = 1; sb < (1u << (a.nt - a.no_t)); ++sb) {
            const double2 w = part[r0 | spread_bits(sb, a.t_sum)];
            v.x += w.x;
            if (CPLX) v.y += w.y;
        }
        const size_t o = (((((size_t)slice << a.nhigh) + h)) << a.no_t) + tid;
        if (CPLX) ((double2*)partials)[o] = v;
        else partials[o] = v.x;
    }
}

struct FidArgs {
    int n, c, t_r, t_c, n_hi;
    uint32_t row_lo;      // the run positions (< c) that are row bits
    uint32_t row_hi;      // bit m: position c + m is a row bit
    uint16_t lo_bit[12];  // run position -> its bit of the row / column table index
    int8_t r_q[12];       // bit of the row table index -> the bit of i (the qubit)
    int8_t c_q[12];       // ... column table, bit of j
    int8_t hi_q[32];      // position c + m -> its qubit
};

__global__ __launch_bounds__(256) void k_dm_fidelity_partial(const double2* __restrict__ rho,
                                                             const double2* __restrict__ psi, FidArgs a,
                                                             uint64_t runs, double* __restrict__ partials) {
    __shared__ double2 tab[kDmFidelityTable];  // psi_i of the run's rows, then psi_j of its columns
    __shared__ double wsum[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t R = 1u << a.c, nr = 1u << a.t_r, nc = 1u << a.t_c;
    // table indices of in-run offset j * 256 + tid: the thread's part, then the part of j
    uint32_t xr_t = 0, xc_t = 0;
    for (int p = 0; p < 8 && p < a.c; ++p)
        if (tid >> p & 1u) {
            if (a.row_lo >> p & 1u) xr_t |= a.lo_bit[p];
            else xc_t |= a.lo_bit[p];
        }
    uint32_t xr_j[4], xc_j[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const bool in = 8 + b < a.c, row = a.row_lo >> (8 + b) & 1u;
        xr_j[b] = in && row ? a.lo_bit[8 + b] : 0u;
        xc_j[b] = in && !row ? a.lo_bit[8 + b] : 0u;
    }
    double acc = 0.0;
    for (uint64_t u = blockIdx.x; u < runs; u += gridDim.x) {
        const double2* src = rho + (u << a.c);
        double2 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t r = j * 256 + tid;  // r < 2^c: inside the run
            v[j] = r < R ? src[r] : make_double2(0.0, 0.0);
        }
        uint32_t i_hi = 0, j_hi = 0;
        for (int m = 0; m < a.n_hi; ++m)
            if (u >> m & 1ull) {
                if (a.row_hi >> m & 1u) i_hi |= 1u << a.hi_q[m];
                else j_hi |= 1u << a.hi_q[m];
            }
        __syncthreads();  // the tables of the run before have been consumed
        for (uint32_t x = tid; x < nr + nc; x += 256) {
            const bool is_row = x < nr;
            const uint32_t y = is_row ? x : x - nr;
            uint32_t idx = is_row ? i_hi : j_hi;  // < 2^n: qubits only
            for (int m = 0; m < (is_row ? a.t_r : a.t_c); ++m)
                if (y >> m & 1u) idx |= 1u << (is_row ? a.r_q[m] : a.c_q[m]);
            tab[x] = psi[idx];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t xr = xr_t, xc = xc_t;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (j >> b & 1) {
                    xr |= xr_j[b];
                    xc |= xc_j[b];
                }
            if ((uint32_t)(j * 256) + tid < R) {
                const double2 pi = tab[xr], pj = tab[nr + xc], e = v[j];
                const double tx = e.x * pj.x - e.y * pj.y, ty = e.x * pj.y + e.y * pj.x;  // rho_ij psi_j
                acc += pi.x * tx + pi.y * ty;  // Re(conj(psi_i) ...)
            }
        }
    }
    acc = block_sum(acc, wsum);
    if (tid == 0) partials[blockIdx.x] = acc;
}

}  // namespace

void launch_dm_marginal(const double2* rho, const DmMarginalPlan& p, double* d_partials, double* d_out,
                        hipStream_t s, Timer* tm) {
    // (both kernels of a call under one timer entry)
    TimedLaunch tl(tm, p.rdm ? "dm_reduced_density" : "dm_marginal", 16.0 * (double)p.elements, s);
    GatherArgs a{};
    FoldMap map{};
    const int shift = p.rdm ? 1 : 0;  // (the matrix: bit 0 of a partial's index is re / im)
    if (p.rdm) map.dst[map.nbits++] = 0;
    a.nt = p.nt;
    a.s_log = p.s_log;
    // the kernel numbers an output by its out generators among the thread bits, then the others
    for (int pass = 0; pass < 2; ++pass)
        for (size_t i = pass ? p.nt : 0; i < (pass ? p.sorted.size() : (size_t)p.nt); ++i) {
            const DmGatherGen& g = p.sorted[i];
            if (!pass) a.tgen[i] = g.mask;
            if (g.out_bit < 0) {
                if (!pass) a.t_sum |= 1u << i;
                else a.lgen[a.nloop++] = g.mask;
                continue;
            }
            if (!pass) ++a.no_t;
            else a.hgen[a.nhigh++] = g.mask;
            map.dst[map.nbits++] = (int8_t)(g.out_bit + shift);
        }
    const uint32_t outs = 1u << p.out_gen.size();
    if (p.rdm) hipLaunchKernelGGL(k_dm_gather<true>, dim3((unsigned)p.groups), dim3(256), 0, s, rho, a, d_partials);
    else hipLaunchKernelGGL(k_dm_gather<false>, dim3((unsigned)p.groups), dim3(256), 0, s, rho, a, d_partials);
    QSIM_HIPCHK(hipGetLastError());
    launch_fold(d_partials, outs << shift, 1u << p.s_log, map, d_out, s);
}

void launch_dm_fidelity(const double2* rho, const double2* d_psi, const DmFidelityPlan& p, double* d_partials,
                        double* d_out, hipStream_t s, Timer* tm) {
    FidArgs a{};
    a.n = p.n;
    a.c = p.c;
    a.t_r = p.t_r;
    a.t_c = p.t_c;
    a.n_hi = 2 * p.n - p.c;
    a.row_lo = p.row_mask & ((1u << p.c) - 1u);
    a.row_hi = p.row_mask >> p.c;
    int nr = 0, nc = 0;
    for (int pos = 0; pos < p.c; ++pos) {
        if (p.row_mask >> pos & 1u) {
            a.lo_bit[pos] = (uint16_t)(1u << nr);
            a.r_q[nr++] = p.qubit[pos];
        } else {
            a.lo_bit[pos] = (uint16_t)(1u << nc);
            a.c_q[nc++] = p.qubit[pos];
        }
    }
    for (int m = 0; m < a.n_hi; ++m) a.hi_q[m] = p.qubit[p.c + m];
    {
        TimedLaunch tl(tm, "dm_fidelity", 16.0 * (double)(1ull << (2 * p.n)), s);
        hipLaunchKernelGGL(k_dm_fidelity_partial, dim3(p.groups), dim3(256), 0, s, rho, d_psi, a, p.runs, d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    launch_sum_partials(d_partials, (int)p.groups, 1, d_out, false, s);
}

}  // namespace qsim_hip

// ---- the C entries ----
using namespace qsim_hip;

// All three read s->d under s->perm as they are: no prep() / canonicalize(), nothing of the state
// changes.
static void run_dm_marginal(qsim_state* s, int n, const int32_t* qubits, int k, bool rdm, double* out) {
    check_dm(s, n);
    QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
    DeviceGuard dg(s->device);
    share_flush(s);  // (pending gates of a run-sharing cycle; the layout may change with them)
    const DmMarginalPlan plan = lower_dm_marginal(n, qubits, k, s->perm.empty() ? nullptr : s->perm.data(), rdm);
    const size_t out_bytes = (rdm ? (size_t)2 << (2 * k) : (size_t)1 << k) * sizeof(double);
    const size_t part_bytes = (plan.scratch_bytes + 255) & ~(size_t)255;
    char* buf = (char*)s->scratch.get(part_bytes + out_bytes, s->stream);
    double* d_out = (double*)(buf + part_bytes);
    launch_dm_marginal(s->d, plan, (double*)buf, d_out, s->stream, &s->timer);
    QSIM_HIPCHK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s->stream));
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
}

extern "C" int qsim_dm_marginal_probabilities(qsim_state* s, int n, const int32_t* qubits, int k, double* out) {
    return guarded([&] { run_dm_marginal(s, n, qubits, k, false, out); });
}

extern "C" int qsim_dm_reduced_density_matrix(qsim_state* s, int n, const int32_t* qubits, int k, double* out) {
    return guarded([&] { run_dm_marginal(s, n, qubits, k, true, out); });
}

extern "C" int qsim_dm_fidelity(qsim_state* s, int n, const double* psi, double* out) {
    return guarded([&] {
        check_dm(s, n);
        QSIM_REQUIRE(psi, QSIM_ERR_INVALID_ARGUMENT, "null state");
        QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
        DeviceGuard dg(s->device);
        share_flush(s);
        const DmFidelityPlan plan = lower_dm_fidelity(n, s->perm.empty() ? nullptr : s->perm.data());
        const size_t psi_bytes = sizeof(double2) << n;
        char* buf = (char*)s->scratch.get(psi_bytes + plan.groups * sizeof(double), s->stream);
        double* d_partials = (double*)(buf + psi_bytes);
        QSIM_HIPCHK(hipMemcpyAsync(buf, psi, psi_bytes, hipMemcpyHostToDevice, s->stream));
        launch_dm_fidelity(s->d, (const double2*)buf, plan, d_partials, s->d_result, s->stream, &s->timer);
        QSIM_HIPCHK(hipMemcpyAsync(out, s->d_result, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

extern "C" int qsim_dm_marginal_plan(int n, const int32_t* qubits, int k, const int32_t* perm, int rdm,
                                     int32_t info[8], uint64_t* out_gen, uint64_t* sum_gen) {
    return guarded([&] {
        QSIM_REQUIRE(info, QSIM_ERR_INVALID_ARGUMENT, "null out");
        const DmMarginalPlan p = lower_dm_marginal(n, qubits, k, perm, rdm != 0);
        info[0] = (int32_t)(p.elements & 0xffffffffull);
        info[1] = (int32_t)(p.elements >> 32);
        info[2] = (int32_t)p.groups;
        info[3] = p.launches;
        info[4] = (int32_t)p.scratch_bytes;  // (at most 16 MiB)
        info[5] = 1 << p.s_log;
        info[6] = p.nt;
        info[7] = 0;
        if (out_gen) std::copy(p.out_gen.begin(), p.out_gen.end(), out_gen);
        if (sum_gen) std::copy(p.sum_gen.begin(), p.sum_gen.end(), sum_gen);
    });
}
