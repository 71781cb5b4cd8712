// dist_expect.hip — Pauli-sum expectation values <psi|H|psi> of a sharded state (dist.hip), read
// where the state lies: no remap, no layout restore, no gather.  No reference counterpart.
//
// expect.hip's lowering runs over all n physical positions.  A group's physical x mask splits
// into local bits and rank bits, x = x_loc | x_rank << L (z alike).  On shard r the sign of a term
// is (-1)^popcount(i & z_loc) (-1)^popcount(r & z_rank); the second factor is constant on the
// shard and folded into its cr / ci on the host, so the kernels only see local bits and n = L.
//
// x_rank == 0: the pair lies inside the shard — launch_expectation on each shard.
// x_rank != 0: amplitude I = (r, i) pairs with J = (r ^ x_rank, i ^ x_loc).  expect.hip's pair rule
//     nY even:  2 (-1)^(nY/2) s(I) Re a        nY odd:  -2 (-1)^((nY-1)/2) s(I) Im a
// holds with either member taken as I, as long as s(I) and a = conj(psi_J) psi_I come from that
// member (a -> conj a flips Im a, s(J) = s(I) (-1)^nY flips the sign for odd nY: the two cancel).
// Each unordered pair is taken once, and only half a shard crosses the link.  b = L - 1:
//   b in x_loc:     every rank takes its own i with bit b = 0; J then has bit b = 1, so every rank
//                   receives its peer's UPPER half (both send their upper half);
//   b not in x_loc: i and i ^ x_loc agree in bit b.  The lower rank of the pair takes the pairs
//                   with bit b = 0 and receives the peer's lower half; the higher rank takes those
//                   with bit b = 1 and receives the peer's upper half (so the lower rank sends its
//                   upper half, the higher rank its lower half).
// Either way a rank reads one half of its own shard at k = i with bit b dropped, and the received
// half at k ^ (x_loc without bit b): two streams of 2^(L-1) amplitudes, contiguous below the
// lowest set bit of x_loc.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"

namespace qsim_hip {

// ---- host-only lowering ---------------------------------------------------------------------

DistExpectPlan lower_dist_expectation(int n, int L, const qsim_pauli_term* terms, size_t count, const int* perm) {
    DistExpectPlan p;
    p.all = lower_expectation(n, terms, count, perm);
    const uint64_t lmask = (1ull << L) - 1ull;
    for (size_t gi = 0; gi < p.all.groups.size(); ++gi) {
        const ExpectGroup& g = p.all.groups[gi];
        const size_t launches = (g.end - g.begin + kExpectTerms - 1) / kExpectTerms;
        p.launches += launches;
        const uint64_t x_rank = g.x >> L, x_loc = g.x & lmask;
        if (x_rank == 0) {
            p.local.push_back(gi);
            continue;
        }
        // (groups come ordered by x = x_loc | x_rank << L: by x_rank, then x_loc — and x_loc holds
        // position L-1 exactly when it is >= 2^(L-1): the order by transfer key)
        const bool top = (x_loc >> (L - 1)) & 1ull;
        if (p.transfers.empty() || p.transfers.back().x_rank != x_rank || p.transfers.back().top != top)
            p.transfers.push_back(DistExpectTransfer{x_rank, top});
        p.cross.push_back(DistExpectCross{x_rank, x_loc, g.begin, g.end, p.cross_terms, p.transfers.size() - 1});
        p.cross_terms += g.end - g.begin;
    }
    return p;
}

ExpectTerm dist_shard_term(const ExpectTerm& e, int L, int rank) {
    const uint64_t lmask = (1ull << L) - 1ull;
    const bool neg = __builtin_popcountll((uint64_t)rank & (e.z >> L)) & 1;
    return ExpectTerm{e.z & lmask, neg ? -e.cr : e.cr, neg ? -e.ci : e.ci};
}

ExpectPlan dist_expect_local(const DistExpectPlan& p, int L, int rank) {
    ExpectPlan out;
    for (size_t gi : p.local) {
        const ExpectGroup& g = p.all.groups[gi];
        ExpectGroup lg{g.x, out.terms.size(), out.terms.size()};
        for (size_t t = g.begin; t < g.end; ++t) out.terms.push_back(dist_shard_term(p.all.terms[t], L, rank));
        lg.end = out.terms.size();
        out.groups.push_back(lg);
        out.launches += (lg.end - lg.begin + kExpectTerms - 1) / kExpectTerms;
    }
    return out;
}

std::vector<ExpectTerm> dist_expect_cross_terms(const DistExpectPlan& p, int L, int rank) {
    std::vector<ExpectTerm> out;
    out.reserve(p.cross_terms);
    for (const DistExpectCross& c : p.cross)
        for (size_t t = c.begin; t < c.end; ++t) out.push_back(dist_shard_term(p.all.terms[t], L, rank));
    return out;
}

int dist_expect_own_half(const DistExpectTransfer& t, int rank) {
    if (t.top) return 0;
    return (uint64_t)rank < ((uint64_t)rank ^ t.x_rank) ? 0 : 1;
}

int dist_expect_send_half(const DistExpectTransfer& t, int rank) {
    // what the peer pairs with: its partner's index has bit b flipped (top) or equal
    const int peer_half = dist_expect_own_half(t, (int)((uint64_t)rank ^ t.x_rank));
    return t.top ? 1 - peer_half : peer_half;
}

// ---- kernels --------------------------------------------------------------------------------
//
// k_expect_partial<PAIR>'s scheme on two base pointers: work-group c adds the pairs k = c * 256 +
// thread, + gridDim.x * 256, ... < count (count = 2^(L-1): a power of two, and xl < count, so
// k ^ xl < count as well).  ibase: the dropped bit b of the own half, for the sign.
namespace {

__global__ __launch_bounds__(256) void k_dist_expect_partial(const double2* own, const double2* peer,
                                                             uint64_t count, uint64_t ibase, uint64_t xl,
                                                             const ExpectTerm* terms, int nterms,
                                                             double* partials) {
    __shared__ ExpectTerm tab[kExpectTerms];
    __shared__ double wsum[4];
    for (int t = threadIdx.x; t < nterms; t += 256) tab[t] = terms[t];
    __syncthreads();
    double acc = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        const uint64_t i = k | ibase;
        const double2 a = own[k], b = peer[k ^ xl];
        const double re = b.x * a.x + b.y * a.y;  // a = conj(psi_J) psi_I
        const double im = b.x * a.y - b.y * a.x;
        double wr = 0.0, wi = 0.0;
        for (int t = 0; t < nterms; ++t) {  // (same LDS address in every lane: broadcast reads)
            const ExpectTerm e = tab[t];
            const bool neg = __popcll(i & e.z) & 1;
            wr += neg ? -e.cr : e.cr;
            wi += neg ? -e.ci : e.ci;
        }
        acc += wr * re + wi * im;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// The z lane/run split of k_expect_partial_split.  No zero is inserted into k here, so the 256
// consecutive k of a run differ in index bits 0-7 only: thread t evaluates term t's sign over
// i & ~255 once per run, per amplitude and term there remain a 32-bit AND, one population count
// and a sign-bit XOR.  The trip count depends on blockIdx only, so every thread reaches both
// barriers.
__global__ __launch_bounds__(256) void k_dist_expect_partial_split(const double2* own, const double2* peer,
                                                                   uint64_t count, uint64_t ibase, uint64_t xl,
                                                                   const ExpectTerm* terms, int nterms,
                                                                   double* partials) {
    __shared__ uint32_t zlo[kExpectTerms];
    __shared__ double swr[kExpectTerms];
    __shared__ double swi[kExpectTerms];
    __shared__ double wsum[4];
    constexpr uint64_t kLow = 255;
    ExpectTerm mine{0, 0.0, 0.0};
    if ((int)threadIdx.x < nterms) {
        mine = terms[threadIdx.x];
        zlo[threadIdx.x] = (uint32_t)(mine.z & kLow);
    }
    double acc = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k0 = (uint64_t)blockIdx.x * blockDim.x; k0 < count; k0 += step) {
        const uint64_t k = k0 + threadIdx.x;
        const uint64_t i = k | ibase;
        double re = 0.0, im = 0.0;
        if (k < count) {
            const double2 a = own[k], b = peer[k ^ xl];
            re = b.x * a.x + b.y * a.y;  // a = conj(psi_J) psi_I
            im = b.x * a.y - b.y * a.x;
        }
        __syncthreads();  // the run before has read its weights
        if ((int)threadIdx.x < nterms) {
            const bool neg = __popcll(i & ~kLow & mine.z) & 1;  // i & ~255: the same in every thread
            swr[threadIdx.x] = neg ? -mine.cr : mine.cr;
            swi[threadIdx.x] = neg ? -mine.ci : mine.ci;
        }
        __syncthreads();
        const uint32_t ilo = (uint32_t)(i & kLow);
        double wr = 0.0, wi = 0.0;
#pragma unroll 4
        for (int t = 0; t < nterms; ++t) {  // (same LDS address in every lane: broadcast reads)
            const unsigned long long flip = (unsigned long long)(__popc(ilo & zlo[t]) & 1) << 63;
            wr += __longlong_as_double(__double_as_longlong(swr[t]) ^ flip);
            wi += __longlong_as_double(__double_as_longlong(swi[t]) ^ flip);
        }
        acc += wr * re + wi * im;  // (re = im = 0 past the end)
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

}  // namespace

void launch_dist_expectation(const double2* own, const double2* peer, int L, int half, uint64_t x_loc,
                             const ExpectTerm* d_terms, size_t count, double* d_partials, double* d_out,
                             bool accumulate, hipStream_t s, Timer* tm) {
    if (count == 0) return;
    if (L < 1 || (half != 0 && half != 1)) fail(QSIM_ERR_RUNTIME, "bad half-shard of a cross-rank expectation");
    const uint64_t H = 1ull << (L - 1);
    const uint64_t xl = x_loc & (H - 1ull);
    const uint64_t ibase = half ? H : 0ull;
    const unsigned chunks = (unsigned)std::min<uint64_t>((H + 255) / 256, expect_chunks(1));
    const bool split_on = expect_split_on();
    for (size_t t0 = 0; t0 < count; t0 += kExpectTerms) {
        const int nterms = (int)std::min<size_t>(kExpectTerms, count - t0);
        const bool split = split_on && nterms >= kExpectSplitMin;
        {
            TimedLaunch tl(tm, "dist_expect_cross", 2.0 * 16.0 * (double)H, s);
            hipLaunchKernelGGL(split ? k_dist_expect_partial_split : k_dist_expect_partial, dim3(chunks), dim3(256),
                               0, s, own, peer, H, ibase, xl, d_terms + t0, nterms, d_partials);
            QSIM_HIPCHK(hipGetLastError());
        }
        launch_sum_partials(d_partials, (int)chunks, 1, d_out, accumulate || t0 != 0, s);
    }
}

}  // namespace qsim_hip
