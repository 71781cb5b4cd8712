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
// This file is the host lowering, the transfers around the kernels (expectation_dist) and the C
// entries.  The kernels are expect.hip's k_expect_partial pair under the
// two-stream addressing policy (launch_dist_expectation, there).
#include <algorithm>
#include <vector>

#include "dist_state.hpp"

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

// QSIM_DIST_EXPECT_OVERLAP (default 1; read at every call): 0 lands every transfer of an
// expectation value in the one receive buffer and waits for it before its kernels start.
static bool expect_overlap_on() { return env_switch("QSIM_DIST_EXPECT_OVERLAP", true); }

// <psi|H|psi> of the sharded state (qsim_dist_expectation), lowered as the top of this file says.  Everything
// computes on d->stream; transfer t of the plan lands in the receive buffer (t even) or, while the
// kernels of transfer t-1 still read that one, in the send buffer (t odd) — both are free outside
// remaps.  Events 0 .. 4 of d->events (free outside remaps too): the state is ready (0), transfer
// landed in buffer j (1 + j), the kernels that read buffer j are done (3 + j).
// Every (group, shard) sum gets a slot of its own on the device; the host adds the slots in a
// fixed order — the local groups shard by shard, then the cross groups in plan order, each shard
// by shard — and one all-reduce adds the ranks' totals.
double expectation_dist(qsim_dist* d, const qsim_pauli_term* terms, size_t count) {
    const int L = d->L;
    const DistExpectPlan plan = lower_dist_expectation(d->n, L, terms, count, d->perm.data());
    const size_t S = d->shards.size();
    const uint64_t H = L >= 1 ? 1ull << (L - 1) : 0;
    if (!plan.cross.empty() && d->world == 1) fail(QSIM_ERR_RUNTIME, "cross-rank Pauli group in a world of one");
    while (d->expect_local.size() < S) d->expect_local.emplace_back(new DevBuf());
    while (d->expect_cross.size() < S) d->expect_cross.emplace_back(new DevBuf());
    // slots: [shard] for the local groups, then [cross group][shard]
    const size_t nslots = S * (1 + plan.cross.size());
    double* d_slots = (double*)d->readout.get(nslots * sizeof(double), d->stream);
    QSIM_HIPCHK(hipMemsetAsync(d_slots, 0, nslots * sizeof(double), d->stream));
    const bool overlap = expect_overlap_on();
    const double sent_before = d->sent_bytes;  // (remapBytes() stays the last run's)
    if (!plan.transfers.empty()) ensure_events(d, 5);
    auto buffer_of = [&](size_t t) { return overlap ? (int)(t & 1) : 0; };
    auto post = [&](size_t t) {  // transfer t on comm_stream, into buffer_of(t)
        const DistExpectTransfer& tr = plan.transfers[t];
        const int j = buffer_of(t);
        // the buffer's last readers: the kernels of transfer t-2 (overlap) or t-1
        if (t >= (overlap ? 2u : 1u)) QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[3 + j], 0));
        std::vector<Post> posts;
        for (const Shard& sh : d->shards) {
            const int half = dist_expect_send_half(tr, sh.rank);
            posts.push_back({sh.rank, (int)((uint64_t)sh.rank ^ tr.x_rank), sh.d + (uint64_t)half * H,
                             j ? sh.sendbuf : sh.recvbuf, H});
        }
        post_transfers(d, posts, "expectation half-shard send/recv");
        QSIM_HIPCHK(hipEventRecord(d->events[1 + j], d->comm_stream));
        if (!overlap) stream_wait(d, d->comm_stream);
    };
    if (!plan.transfers.empty()) {
        QSIM_HIPCHK(hipEventRecord(d->events[0], d->stream));  // (the state's last writers)
        QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[0], 0));
        if (overlap) post(0);  // in flight while the local groups run
    }
    if (!plan.local.empty())
        for (size_t i = 0; i < S; ++i) {
            const ExpectPlan lp = dist_expect_local(plan, L, d->shards[i].rank);
            launch_expectation(d->shards[i].d, L, 1, lp, *d->expect_local[i], d->d_partials, d_slots + i, d->stream,
                               &d->timer);
        }
    if (!plan.cross.empty())
        for (size_t i = 0; i < S; ++i) {
            const std::vector<ExpectTerm> xt = dist_expect_cross_terms(plan, L, d->shards[i].rank);
            d->expect_cross[i]->upload(xt.data(), xt.size() * sizeof(ExpectTerm), d->stream);
        }
    size_t c = 0;
    for (size_t t = 0; t < plan.transfers.size(); ++t) {
        if (!overlap) post(t);
        else if (t + 1 < plan.transfers.size()) post(t + 1);
        const int j = buffer_of(t);
        QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[1 + j], 0));
        for (; c < plan.cross.size() && plan.cross[c].transfer == t; ++c) {
            const DistExpectCross& g = plan.cross[c];
            for (size_t i = 0; i < S; ++i) {
                const Shard& sh = d->shards[i];
                const int half = dist_expect_own_half(plan.transfers[t], sh.rank);
                launch_dist_expectation(sh.d + (uint64_t)half * H, j ? sh.sendbuf : sh.recvbuf, L, half, g.x_loc,
                                        (const ExpectTerm*)d->expect_cross[i]->ptr + g.xbegin, g.end - g.begin,
                                        d->d_partials, d_slots + (1 + c) * S + i, false, d->stream, &d->timer);
            }
        }
        QSIM_HIPCHK(hipEventRecord(d->events[3 + j], d->stream));
    }
    d->sent_bytes = sent_before;
    std::vector<double> slots(nslots, 0.0);
    if (!plan.all.terms.empty()) {
        QSIM_HIPCHK(hipMemcpyAsync(slots.data(), d_slots, nslots * sizeof(double), hipMemcpyDeviceToHost, d->stream));
        stream_wait(d, d->stream);
    }
    double local = 0.0;
    for (double v : slots) local += v;  // (slot order: local groups, then plan order; shards in rank order)
    return allreduce_sum(d, local);
}

}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_dist_expectation(qsim_dist* d, const qsim_pauli_term* terms, size_t count, double* out) {
    return dguard_comm(d, [&] {
        need(d);
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (!terms && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
        flush_on_device(d);
        *out = expectation_dist(d, terms, count);
    });
}

int qsim_dist_expectation_plan(int n_qubits, int world, const int32_t* perm, const qsim_pauli_term* terms,
                               size_t count, int* local_groups, int* cross_groups, int* transfers, int* launches,
                               uint64_t* bytes_sent_per_rank) {
    return guarded([&] {
        const int L = HostPlanArgs(n_qubits, world).L;
        if (!terms && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
        if (!local_groups || !cross_groups || !transfers || !launches || !bytes_sent_per_rank)
            fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        std::vector<int> p;
        if (perm) p.assign(perm, perm + n_qubits);
        const DistExpectPlan plan = lower_dist_expectation(n_qubits, L, terms, count, perm ? p.data() : nullptr);
        *local_groups = (int)plan.local.size();
        *cross_groups = (int)plan.cross.size();
        *transfers = (int)plan.transfers.size();
        *launches = (int)plan.launches;
        *bytes_sent_per_rank = (uint64_t)plan.transfers.size() * (sizeof(double2) << (L - 1));
    });
}

}  // extern "C"
