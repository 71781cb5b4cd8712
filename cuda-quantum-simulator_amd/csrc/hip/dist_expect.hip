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
//
// This file is the host lowering.  The kernels are expect.hip's k_expect_partial pair under the
// two-stream addressing policy (launch_dist_expectation, there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "engine.hpp"

namespace qsim_hip {

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

}  // namespace qsim_hip
