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
#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"

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

void check_pauli_masks(int n, const qsim_pauli_term* terms, size_t count, const char* what) {
    const uint64_t valid = (1ull << n) - 1ull;
    for (size_t t = 0; t < count; ++t)
        if ((terms[t].x_mask | terms[t].z_mask) & ~valid)
            fail(QSIM_ERR_OUT_OF_RANGE, std::string(what) + " acts on a qubit index out of range");
}

ExpectPlan lower_pauli_terms(int n, const qsim_pauli_term* terms, size_t count, const int* perm,
                             const std::function<void(uint64_t, uint64_t, double, ExpectTerm&)>& weight) {
    check_qubit_perm(n, perm);
    if (count && !terms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
    check_pauli_masks(n, terms, count, "Pauli term");
    auto to_phys = [&](uint64_t m) { return mask_to_physical(m, n, perm); };
    // merged coefficients keyed by the physical (x, z): iteration order is by x, then z
    std::map<std::pair<uint64_t, uint64_t>, double> merged;
    for (size_t t = 0; t < count; ++t)
        merged[{to_phys(terms[t].x_mask), to_phys(terms[t].z_mask)}] += terms[t].coeff;
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

// Addressing policies of the two kernels below: how pair number k of a launch turns into the sign
// index i (sign_index) and into Re a / Im a (product; off: the trajectory's offset).  kLow: the
// index bits in which the 256 consecutive k of a work-group's run differ.

// re + i im = conj(b) a
__device__ __forceinline__ void conj_product(double2 a, double2 b, double& re, double& im) {
    re = b.x * a.x + b.y * a.y;
    im = b.x * a.y - b.y * a.x;
}

// x == 0: amplitude i = k on its own, Re a = |psi_i|^2.
struct DiagAddr {
    static constexpr bool kPair = false;
    static constexpr uint64_t kLow = 511;
    const double2* st;
    __device__ uint64_t sign_index(uint64_t k) const { return k; }
    __device__ void product(uint64_t off, uint64_t, uint64_t i, double& re, double& im) const {
        const double2 a = st[off + i];
        re = a.x * a.x + a.y * a.y;
        im = 0.0;
    }
};

// x != 0 inside one state: i = insert0(k, hbit) (hbit: the highest x bit) with i ^ x,
// a = conj(psi_j) psi_i.  (kLow has bit 8: the inserted zero may fall below it.)
struct PairAddr {
    static constexpr bool kPair = true;
    static constexpr uint64_t kLow = 511;
    const double2* st;
    int hbit;
    uint64_t x;
    __device__ uint64_t sign_index(uint64_t k) const {
        const uint64_t lo = k & ((1ull << hbit) - 1ull);
        return ((k ^ lo) << 1) | lo;
    }
    __device__ void product(uint64_t off, uint64_t, uint64_t i, double& re, double& im) const {
        const double2* v = st + off;
        conj_product(v[i], v[i ^ x], re, im);
    }
};

// A cross-rank group of a sharded state (dist_expect.hip) on two base pointers: own[k] with
// peer[k ^ xl], a = conj(psi_J) psi_I (count = 2^(L-1): a power of two, and xl < count, so
// k ^ xl < count as well).  ibase: the dropped bit b of the own half, for the sign.  No zero is
// inserted into k, so the k of a run differ in index bits 0-7 only.  (One state: gridDim.y == 1.)
struct TwoStreamAddr {
    static constexpr bool kPair = true;
    static constexpr uint64_t kLow = 255;
    const double2 *own, *peer;
    uint64_t ibase, xl;
    __device__ uint64_t sign_index(uint64_t k) const { return k | ibase; }
    __device__ void product(uint64_t, uint64_t k, uint64_t, double& re, double& im) const {
        conj_product(own[k], peer[k ^ xl], re, im);
    }
};

// One launch of one group over `gridDim.y` trajectories: work-group (c, t) adds the pairs
// k = c * 256 + thread, + gridDim.x * 256, ... < count of trajectory t.
template <class Addr>
__global__ __launch_bounds__(256) void k_expect_partial(Addr addr, uint64_t stride, uint64_t count,
                                                        const ExpectTerm* terms, int nterms, double* partials) {
    __shared__ ExpectTerm tab[kExpectTerms];
    __shared__ double wsum[4];
    for (int t = threadIdx.x; t < nterms; t += 256) tab[t] = terms[t];
    __syncthreads();
    const uint64_t off = (uint64_t)blockIdx.y * stride;
    double acc = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        const uint64_t i = addr.sign_index(k);
        double re, im, wr, wi;
        addr.product(off, k, i, re, im);
        term_weight<Addr::kPair>(tab, nterms, i, wr, wi);
        acc += Addr::kPair ? wr * re + wi * im : wr * re;
    }
    acc = block_sum(acc, wsum);
    if (threadIdx.x == 0) partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// The same launch with each z split in two (groups of many terms are instruction-bound on the
// per-amplitude, per-term sign: a 64-bit AND, two population counts and a select).  A work-group's
// 256 consecutive pairs differ only in the index bits of kLow, so (-1)^popcount(i & z) =
// (-1)^popcount(i & z & ~kLow) (-1)^popcount(i & z & kLow): thread t evaluates the first factor of
// term t once per 256-pair run and stores the signed weights in LDS; per amplitude and term there
// remain a 32-bit AND, one population count and a sign-bit XOR.  The trip count depends on
// blockIdx only, so every thread reaches both barriers.
template <class Addr>
__global__ __launch_bounds__(256) void k_expect_partial_split(Addr addr, uint64_t stride, uint64_t count,
                                                              const ExpectTerm* terms, int nterms,
                                                              double* partials) {
    __shared__ uint32_t zlo[kExpectTerms];
    __shared__ double swr[kExpectTerms];
    __shared__ double swi[Addr::kPair ? kExpectTerms : 1];
    __shared__ double wsum[4];
    constexpr uint64_t kLow = Addr::kLow;
    ExpectTerm mine{0, 0.0, 0.0};
    if ((int)threadIdx.x < nterms) {
        mine = terms[threadIdx.x];
        zlo[threadIdx.x] = (uint32_t)(mine.z & kLow);
    }
    const uint64_t off = (uint64_t)blockIdx.y * stride;
    double acc = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k0 = (uint64_t)blockIdx.x * blockDim.x; k0 < count; k0 += step) {
        const uint64_t k = k0 + threadIdx.x;
        const uint64_t i = addr.sign_index(k);
        double re = 0.0, im = 0.0;
        if (k < count) addr.product(off, k, i, re, im);
        __syncthreads();  // the run before has read its weights
        if ((int)threadIdx.x < nterms) {
            const bool neg = __popcll(i & ~kLow & mine.z) & 1;  // i & ~kLow: the same in every thread
            swr[threadIdx.x] = neg ? -mine.cr : mine.cr;
            if (Addr::kPair) swi[threadIdx.x] = neg ? -mine.ci : mine.ci;
        }
        __syncthreads();
        const uint32_t ilo = (uint32_t)(i & kLow);
        double wr = 0.0, wi = 0.0;
#pragma unroll 4
        for (int t = 0; t < nterms; ++t) {  // (same LDS address in every lane: broadcast reads)
            const unsigned long long flip = (unsigned long long)(__popc(ilo & zlo[t]) & 1) << 63;
            wr += __longlong_as_double(__double_as_longlong(swr[t]) ^ flip);
            if (Addr::kPair) wi += __longlong_as_double(__double_as_longlong(swi[t]) ^ flip);
        }
        acc += Addr::kPair ? wr * re + wi * im : wr * re;  // (re = im = 0 past the end)
    }
    acc = block_sum(acc, wsum);
    if (threadIdx.x == 0) partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// One launch of at most kExpectTerms terms of one group: the split kernel from kExpectSplitMin
// terms on, unless QSIM_EXPECT_SPLIT says otherwise.
template <class Addr>
void launch_partial(const Addr& addr, dim3 grid, uint64_t stride, uint64_t count, const ExpectTerm* d_terms,
                    int nterms, bool split_on, double* d_partials, hipStream_t s) {
    const bool split = split_on && nterms >= kExpectSplitMin;
    hipLaunchKernelGGL(split ? k_expect_partial_split<Addr> : k_expect_partial<Addr>, grid, dim3(256), 0, s, addr,
                       stride, count, d_terms, nterms, d_partials);
    QSIM_HIPCHK(hipGetLastError());
}

}  // namespace

// QSIM_EXPECT_SPLIT (default 1; read at every call, so a benchmark can time both kernels in one
// process): 0 runs every group through the plain kernel.
bool expect_split_on() { return env_switch("QSIM_EXPECT_SPLIT", true); }

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
            for (uint64_t b0 = 0; b0 < batch; b0 += kMaxGridY) {
                const unsigned nb = (unsigned)std::min<uint64_t>(kMaxGridY, batch - b0);
                const double2* v = st + b0 * N;
                {
                    TimedLaunch tl(tm, pair ? "expect_pair" : "expect_diag", 16.0 * (double)N * nb, s);
                    if (pair)
                        launch_partial(PairAddr{v, hbit, g.x}, dim3(chunks, nb), N, count, d_terms + t0, nterms,
                                       split_on, d_partials, s);
                    else
                        launch_partial(DiagAddr{v}, dim3(chunks, nb), N, count, d_terms + t0, nterms, split_on,
                                       d_partials, s);
                }
                launch_sum_partials(d_partials, (int)chunks, nb, d_out + b0, !first, s);
            }
            first = false;
        }
    }
}

// A cross-rank group of a sharded state (dist_expect.hip): the same kernels on two streams.
void launch_dist_expectation(const double2* own, const double2* peer, int L, int half, uint64_t x_loc,
                             const ExpectTerm* d_terms, size_t count, double* d_partials, double* d_out,
                             bool accumulate, hipStream_t s, Timer* tm) {
    if (count == 0) return;
    if (L < 1 || (half != 0 && half != 1)) fail(QSIM_ERR_RUNTIME, "bad half-shard of a cross-rank expectation");
    const uint64_t H = 1ull << (L - 1);
    const TwoStreamAddr addr{own, peer, half ? H : 0ull, x_loc & (H - 1ull)};
    const unsigned chunks = (unsigned)std::min<uint64_t>((H + 255) / 256, expect_chunks(1));
    const bool split_on = expect_split_on();
    for (size_t t0 = 0; t0 < count; t0 += kExpectTerms) {
        const int nterms = (int)std::min<size_t>(kExpectTerms, count - t0);
        {
            TimedLaunch tl(tm, "dist_expect_cross", 2.0 * 16.0 * (double)H, s);
            launch_partial(addr, dim3(chunks), 0, H, d_terms + t0, nterms, split_on, d_partials, s);
        }
        launch_sum_partials(d_partials, (int)chunks, 1, d_out, accumulate || t0 != 0, s);
    }
}

}  // namespace qsim_hip

// ---- the C entries ----
using namespace qsim_hip;

// Reads s->d under s->perm as they are: no prep() / canonicalize(), nothing of the state changes.
extern "C" int qsim_state_expectation(qsim_state* s, const qsim_pauli_term* terms, size_t count, double* out) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
        QSIM_REQUIRE(terms || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        DeviceGuard dg(s->device);
        share_flush(s);  // (pending gates of a run-sharing cycle; the layout may change with them)
        const ExpectPlan plan = lower_expectation(s->n, terms, count, s->perm.empty() ? nullptr : s->perm.data());
        *out = 0.0;
        if (plan.terms.empty()) return;
        launch_expectation(s->d, s->n, 1, plan, s->expect_terms, s->d_partials, s->d_result, s->stream, &s->timer);
        QSIM_HIPCHK(hipMemcpyAsync(out, s->d_result, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

extern "C" int qsim_expectation_plan(int n_qubits, const qsim_pauli_term* terms, size_t count, const int32_t* perm,
                                     int* passes, int* launches) {
    return guarded([&] {
        QSIM_REQUIRE(terms || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        QSIM_REQUIRE(passes && launches, QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        const ExpectPlan plan = lower_expectation(n_qubits, terms, count, perm);
        *passes = (int)plan.groups.size();
        *launches = (int)plan.launches;
    });
}
