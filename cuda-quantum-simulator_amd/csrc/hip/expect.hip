// expect.hip — Pauli-sum expectation values <psi|H|psi>, H = sum_t c_t P_t, computed where the
// state lies (no readback, no layout restore).  No reference counterpart: the reference has no
// observable API; a caller copies the 2^n amplitudes to the host.
//
// A Pauli string is two masks: x (bit set where the factor is X or Y) and z (Z or Y), nY =
// popcount(x & z).  With index bit q == qubit q,
//     P|i> = i^nY (-1)^popcount(i & z) |i ^ x>
//     <psi|P|psi> = sum_i psi_i conj(psi_{i^x}) i^nY (-1)^popcount(i & z).
// x == 0: sum_i |psi_i|^2 s(i), s(i) = (-1)^popcount(i & z).  x != 0: pair i (highest x bit 0)
// with j = i ^ x, a = conj(psi_j) psi_i; the two terms of the pair add up to
//     nY even:  2 (-1)^(nY/2) s(i) Re a        nY odd:  -2 (-1)^((nY-1)/2) s(i) Im a
// (s(j) = s(i) (-1)^nY).  Terms with the same x share the pairing and Re a / Im a, so a group of
// them is ONE pass over the state that accumulates W_re(i) Re a + W_im(i) Im a with
// W_re = sum_t s_t(i) cr_t, W_im = sum_t s_t(i) ci_t, the real weights cr / ci prepared on the
// host.  Every Z/I-only term falls in the x == 0 group (Re a = |psi_i|^2): an Ising or MaxCut
// Hamiltonian of any size is one read of the state.
//
// Masks are mapped from logical to physical bits through the state's qubit permutation on the
// host, so the pass reads the amplitudes under whatever layout the last run left.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"

namespace qsim_hip {

void check_qubit_perm(int n, const int* perm) {
    if (n < 1 || n > 63) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
    if (!perm) return;
    uint64_t seen = 0;
    for (int q = 0; q < n; ++q) {
        if (perm[q] < 0 || perm[q] >= n || (seen >> perm[q] & 1ull))
            fail(QSIM_ERR_INVALID_ARGUMENT, "perm is not a permutation of the qubits");
        seen |= 1ull << perm[q];
    }
}

uint64_t mask_to_physical(uint64_t m, int n, const int* perm) {
    if (!perm) return m;
    uint64_t p = 0;
    for (int q = 0; q < n; ++q)
        if (m >> q & 1ull) p |= 1ull << perm[q];
    return p;
}

ExpectPlan lower_pauli_terms(int n, const qsim_pauli_term* terms, size_t count, const int* perm,
                             const std::function<void(uint64_t, uint64_t, double, ExpectTerm&)>& weight) {
    check_qubit_perm(n, perm);
    if (count && !terms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
    const uint64_t valid = (1ull << n) - 1ull;
    auto to_phys = [&](uint64_t m) { return mask_to_physical(m, n, perm); };
    // merged coefficients keyed by the physical (x, z): iteration order is by x, then z
    std::map<std::pair<uint64_t, uint64_t>, double> merged;
    for (size_t t = 0; t < count; ++t) {
        if ((terms[t].x_mask | terms[t].z_mask) & ~valid)
            fail(QSIM_ERR_OUT_OF_RANGE, "Pauli term acts on a qubit index out of range");
        merged[{to_phys(terms[t].x_mask), to_phys(terms[t].z_mask)}] += terms[t].coeff;
    }
    ExpectPlan plan;
    for (const auto& kv : merged) {
        const uint64_t x = kv.first.first, z = kv.first.second;
        const double c = kv.second;
        if (c == 0.0) continue;
        if (plan.groups.empty() || plan.groups.back().x != x) {
            plan.groups.push_back(ExpectGroup{x, plan.terms.size(), plan.terms.size()});
        }
        ExpectTerm e{z, 0.0, 0.0};
        weight(x, z, c, e);
        plan.terms.push_back(e);
        plan.groups.back().end = plan.terms.size();
    }
    for (const ExpectGroup& g : plan.groups)
        plan.launches += (g.end - g.begin + kExpectTerms - 1) / kExpectTerms;
    return plan;
}

ExpectPlan lower_expectation(int n, const qsim_pauli_term* terms, size_t count, const int* perm) {
    return lower_pauli_terms(n, terms, count, perm, [](uint64_t x, uint64_t z, double c, ExpectTerm& e) {
        e.cr = c;
        if (x != 0) {
            const int ny = __builtin_popcountll(x & z);
            if (ny & 1) {
                e.cr = 0.0;
                e.ci = ((ny - 1) / 2) & 1 ? 2.0 * c : -2.0 * c;
            } else {
                e.cr = (ny / 2) & 1 ? -2.0 * c : 2.0 * c;
            }
        }
    });
}

size_t expect_chunks(uint64_t batch) {
    return (size_t)std::min<uint64_t>(2048, std::max<uint64_t>(8, 16384 / std::max<uint64_t>(batch, 1)));
}

namespace {

// One launch of one group over `gridDim.y` trajectories: work-group (c, t) adds the pairs
// k = c * 256 + thread, + gridDim.x * 256, ... < count of trajectory t.  PAIR: x != 0, pair k is
// i = insert0(k, hbit) with i ^ x (hbit: the highest x bit); else i = k on its own.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_expect_partial(const double2* st, uint64_t stride, uint64_t count,
                                                        int hbit, uint64_t x, const ExpectTerm* terms, int nterms,
                                                        double* partials) {
    __shared__ ExpectTerm tab[kExpectTerms];
    __shared__ double wsum[4];
    for (int t = threadIdx.x; t < nterms; t += 256) tab[t] = terms[t];
    __syncthreads();
    const double2* v = st + (uint64_t)blockIdx.y * stride;
    const uint64_t lomask = PAIR ? (1ull << hbit) - 1ull : 0ull;
    double acc = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        uint64_t i = k;
        double re, im = 0.0;
        if (PAIR) {
            const uint64_t lo = k & lomask;
            i = ((k ^ lo) << 1) | lo;
            const double2 a = v[i], b = v[i ^ x];
            re = b.x * a.x + b.y * a.y;  // a = conj(psi_j) psi_i
            im = b.x * a.y - b.y * a.x;
        } else {
            const double2 a = v[i];
            re = a.x * a.x + a.y * a.y;
        }
        double wr = 0.0, wi = 0.0;
        for (int t = 0; t < nterms; ++t) {  // (same LDS address in every lane: broadcast reads)
            const ExpectTerm e = tab[t];
            const bool neg = __popcll(i & e.z) & 1;
            wr += neg ? -e.cr : e.cr;
            if (PAIR) wi += neg ? -e.ci : e.ci;
        }
        acc += PAIR ? wr * re + wi * im : wr * re;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// The same launch with each z split in two (groups of many terms are instruction-bound on the
// per-amplitude, per-term sign: a 64-bit AND, two population counts and a select).  A work-group's
// 256 consecutive pairs differ only in index bits 0-8 (bit 8: the inserted zero may fall below
// it), so (-1)^popcount(i & z) = (-1)^popcount(i & z & ~511) (-1)^popcount(i & z & 511): thread t
// evaluates the first factor of term t once per 256-pair run and stores the signed weights in
// LDS; per amplitude and term there remain a 32-bit AND, one population count and a sign-bit XOR.
// The trip count depends on blockIdx only, so every thread reaches both barriers.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_expect_partial_split(const double2* st, uint64_t stride, uint64_t count,
                                                              int hbit, uint64_t x, const ExpectTerm* terms,
                                                              int nterms, double* partials) {
    __shared__ uint32_t zlo[kExpectTerms];
    __shared__ double swr[kExpectTerms];
    __shared__ double swi[PAIR ? kExpectTerms : 1];
    __shared__ double wsum[4];
    constexpr uint64_t kLow = 511;
    ExpectTerm mine{0, 0.0, 0.0};
    if ((int)threadIdx.x < nterms) {
        mine = terms[threadIdx.x];
        zlo[threadIdx.x] = (uint32_t)(mine.z & kLow);
    }
    const double2* v = st + (uint64_t)blockIdx.y * stride;
    const uint64_t lomask = PAIR ? (1ull << hbit) - 1ull : 0ull;
    double acc = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k0 = (uint64_t)blockIdx.x * blockDim.x; k0 < count; k0 += step) {
        const uint64_t k = k0 + threadIdx.x;
        const bool active = k < count;
        uint64_t i = k;
        if (PAIR) {
            const uint64_t lo = k & lomask;
            i = ((k ^ lo) << 1) | lo;
        }
        double re = 0.0, im = 0.0;
        if (active) {
            if (PAIR) {
                const double2 a = v[i], b = v[i ^ x];
                re = b.x * a.x + b.y * a.y;  // a = conj(psi_j) psi_i
                im = b.x * a.y - b.y * a.x;
            } else {
                const double2 a = v[i];
                re = a.x * a.x + a.y * a.y;
            }
        }
        __syncthreads();  // the run before has read its weights
        if ((int)threadIdx.x < nterms) {
            const bool neg = __popcll(i & ~kLow & mine.z) & 1;  // i & ~511: the same in every thread
            swr[threadIdx.x] = neg ? -mine.cr : mine.cr;
            if (PAIR) swi[threadIdx.x] = neg ? -mine.ci : mine.ci;
        }
        __syncthreads();
        const uint32_t ilo = (uint32_t)(i & kLow);
        double wr = 0.0, wi = 0.0;
#pragma unroll 4
        for (int t = 0; t < nterms; ++t) {  // (same LDS address in every lane: broadcast reads)
            const unsigned long long flip = (unsigned long long)(__popc(ilo & zlo[t]) & 1) << 63;
            wr += __longlong_as_double(__double_as_longlong(swr[t]) ^ flip);
            if (PAIR) wi += __longlong_as_double(__double_as_longlong(swi[t]) ^ flip);
        }
        acc += PAIR ? wr * re + wi * im : wr * re;  // (re = im = 0 past the end)
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

}  // namespace

// QSIM_EXPECT_SPLIT (default 1; read at every call, so a benchmark can time both kernels in one
// process): 0 runs every group through the plain kernel.
bool expect_split_on() {
    const char* e = std::getenv("QSIM_EXPECT_SPLIT");
    return e == nullptr || std::atoi(e) != 0;
}

void launch_expectation(const double2* st, int n, uint64_t batch, const ExpectPlan& plan, DevBuf& terms,
                        double* d_partials, double* d_out, hipStream_t s, Timer* tm) {
    if (plan.terms.empty() || batch == 0) return;
    terms.upload(plan.terms.data(), plan.terms.size() * sizeof(ExpectTerm), s);
    const ExpectTerm* d_terms = (const ExpectTerm*)terms.ptr;
    const uint64_t N = 1ull << n;
    const uint64_t max_chunks = expect_chunks(batch);
    constexpr uint64_t kMaxGridY = 65535;
    const bool split_on = expect_split_on();
    bool first = true;
    for (const ExpectGroup& g : plan.groups) {
        const bool pair = g.x != 0;
        const int hbit = pair ? 63 - __builtin_clzll(g.x) : -1;
        const uint64_t count = pair ? N / 2 : N;
        const unsigned chunks = (unsigned)std::min<uint64_t>((count + 255) / 256, max_chunks);
        for (size_t t0 = g.begin; t0 < g.end; t0 += kExpectTerms) {
            const int nterms = (int)std::min<size_t>(kExpectTerms, g.end - t0);
            const bool split = split_on && nterms >= kExpectSplitMin;
            auto kernel = pair ? (split ? k_expect_partial_split<true> : k_expect_partial<true>)
                               : (split ? k_expect_partial_split<false> : k_expect_partial<false>);
            for (uint64_t b0 = 0; b0 < batch; b0 += kMaxGridY) {
                const unsigned nb = (unsigned)std::min<uint64_t>(kMaxGridY, batch - b0);
                {
                    TimedLaunch tl(tm, pair ? "expect_pair" : "expect_diag", 16.0 * (double)N * nb, s);
                    hipLaunchKernelGGL(kernel, dim3(chunks, nb), dim3(256), 0, s, st + b0 * N, N, count, hbit, g.x,
                                       d_terms + t0, nterms, d_partials);
                    QSIM_HIPCHK(hipGetLastError());
                }
                launch_sum_partials(d_partials, (int)chunks, nb, d_out + b0, !first, s);
            }
            first = false;
        }
    }
}

}  // namespace qsim_hip
