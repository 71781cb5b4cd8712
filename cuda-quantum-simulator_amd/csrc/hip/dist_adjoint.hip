// dist_adjoint.hip — adjoint-method gradients of <psi|H|psi> on a sharded state (dist.hip): the
// host lowering and the kernels the single-GPU sweep (adjoint.hip) lacks.  No reference counterpart.
//
// The sweep keeps two sharded work states, phi and lambda = H phi, under a qubit map of their own
// (the driver, gradient_dist at the end of this file, walks the circuit backwards as qsim_state_gradient does).
// With L local positions, a physical position p >= L is bit p - L of the rank.
//
// lambda = H phi.  lower_pauli_apply runs over all n physical positions; a group's x mask splits
// into x_loc | x_rank << L and, as in dist_expect.hip, the z bits on rank positions are a sign that
// is constant on a shard and folded into the shard's term table.  (P phi)[(r, i)] reads
// phi[(r ^ x_rank, i ^ x_loc)]: a group with x_rank == 0 is adjoint.hip's k_pauli_apply on the shard,
// one with x_rank != 0 the same kernel reading the whole phi shard of rank r ^ x_rank from a
// staging buffer.  Groups come ordered by x, hence by x_rank: groups of one x_rank share a transfer.
//
// A rotation exp(-i theta/2 G) contributes Im <lambda| G |phi>, then U^† is applied to both states.
// Classes, by the physical positions of the target t and the control c:
//   t local, c local or absent   adjoint.hip's step on each shard;
//   t local, c on a rank bit     the uncontrolled step on the shards whose rank has that bit set;
//   diagonal (Rz, CRZ), t rank   G and U^† are constant on a shard: k_dist_adjoint_diag, no transfer;
//   Rx / Ry / CRY, t rank        rank r pairs with r ^ tbit.  With v = this rank's target bit and
//                                U^† = [[m0, m1], [m2, m3]], row v of the pair update reads
//                                  new_own = a own + b peer,  (a, b) = v ? (m3, m2) : (m0, m1)
//                                and (G phi)_own = phi_peer (X), -i phi_peer (Y, v = 0), +i phi_peer
//                                (Y, v = 1).  k_dist_adjoint_step<.., BRAKET = true> adds
//                                Im conj(lambda_own) (G phi)_own and overwrites phi_own from the peer's
//                                old phi shard; a second launch (BRAKET = false) overwrites lambda_own
//                                from the peer's old lambda shard.  The two ranks' partial sums add up
//                                to the whole bra-ket.
// A control on a local position restricts either kernel to the indices with that bit set.
// Partial sums: double, wave_sum then the four waves of a work-group in a fixed order, one partial
// per work-group, launch_sum_partials — no atomics, bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device_ops.hpp"
#include "dist_state.hpp"

namespace qsim_hip {

// ---- host-only lowering ---------------------------------------------------------------------

DistApplyPlan lower_dist_apply(int n, int L, const qsim_pauli_term* terms, size_t count, const int* perm) {
    DistApplyPlan p;
    p.all = lower_pauli_apply(n, terms, count, perm);
    const uint64_t lmask = (1ull << L) - 1ull;
    uint64_t last_rank = 0;
    for (const ExpectGroup& g : p.all.groups) {
        const uint64_t x_rank = g.x >> L;
        p.groups.push_back(DistApplyGroup{x_rank, g.x & lmask, g.begin, g.end});
        p.launches += (g.end - g.begin + kExpectTerms - 1) / kExpectTerms;
        if (x_rank == 0) {
            ++p.local_groups;
            continue;
        }
        ++p.cross_groups;
        if (x_rank != last_rank) ++p.transfers;  // (ordered by x: one run of groups per x_rank)
        last_rank = x_rank;
    }
    return p;
}

std::vector<ExpectTerm> dist_apply_terms(const DistApplyPlan& p, int L, int rank) {
    std::vector<ExpectTerm> out;
    out.reserve(p.all.terms.size());
    for (const ExpectTerm& e : p.all.terms) out.push_back(dist_shard_term(e, L, rank));
    return out;
}

int dist_gradient_class(const qsim_gate& g, const int* perm, int L) {
    const Generator gen = gate_generator(g);
    const int t = perm[gen.t], c = gen.c >= 0 ? perm[gen.c] : -1;
    const bool crank = c >= L;
    if (t < L) return crank ? DG_LOCAL_CRANK : DG_LOCAL;
    if (gen.pauli == 3) return crank ? DG_DIAG_CRANK : DG_DIAG;
    return crank ? DG_CROSS_CRANK : DG_CROSS;
}

// ---- kernels --------------------------------------------------------------------------------
namespace {

// conj(a) g
__device__ __forceinline__ double2 cjmul(double2 a, double2 g) {
    return make_double2(a.x * g.x + a.y * g.y, a.x * g.y - a.y * g.x);
}

// Index k of the active subspace: the whole shard, or (CTRL) the indices with bit cpos set.
template <bool CTRL>
__device__ __forceinline__ uint64_t active_index(uint64_t k, int cpos) {
    if (!CTRL) return k;
    const uint64_t lo = k & ((1ull << cpos) - 1ull);
    return (((k ^ lo) << 1) | lo) | (1ull << cpos);
}

// Diagonal rotation whose target is a rank bit: on this shard G = sgn (+1: bit 0, -1: bit 1) and
// U^† = d.  partials[block] = the block's share of sgn Im <lam|phi>; phi *= d, lam *= d.
template <bool CTRL>
__global__ __launch_bounds__(256) void k_dist_adjoint_diag(double2* __restrict__ phi, double2* __restrict__ lam,
                                                           uint64_t count, int cpos, double sgn, double2 d,
                                                           double* partials) {
    __shared__ double wim[4];
    double im = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        const uint64_t i = active_index<CTRL>(k, cpos);
        const double2 p = phi[i], l = lam[i];
        im += cjmul(l, p).y;
        phi[i] = cmul(d, p);
        lam[i] = cmul(d, l);
    }
    im = block_sum(im, wim);
    if (threadIdx.x == 0) partials[blockIdx.x] = sgn * im;
}

// One work state of a rotation (X or Y generator) whose target is a rank bit: own <- a own + b peer
// over the active indices, peer = the partner rank's old shard.  BRAKET (own = phi, lam = this
// rank's lambda, not yet updated): partials[block] = the block's share of Im conj(lam) (G phi)_own,
// (G phi)_own = peer (X), -i peer (Y, v = 0), +i peer (Y, v = 1).
template <int PAULI, bool BRAKET, bool CTRL>
__global__ __launch_bounds__(256) void k_dist_adjoint_step(double2* __restrict__ own, const double2* __restrict__ peer,
                                                           const double2* __restrict__ lam, uint64_t count, int cpos,
                                                           int v, double2 a, double2 b, double* partials) {
    __shared__ double wim[4];
    double im = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        const uint64_t i = active_index<CTRL>(k, cpos);
        const double2 o = own[i], p = peer[i];
        if (BRAKET) {
            double2 g = p;
            if (PAULI == 2) g = v ? make_double2(-p.y, p.x) : make_double2(p.y, -p.x);
            im += cjmul(lam[i], g).y;
        }
        own[i] = cadd(cmul(a, o), cmul(b, p));
    }
    if (BRAKET) {
        im = block_sum(im, wim);
        if (threadIdx.x == 0) partials[blockIdx.x] = im;
    }
}

struct ShardGeom {
    uint64_t count;
    unsigned chunks;
};
ShardGeom shard_geom(int L, int cpos) {
    if (L < 1 || cpos >= L) fail(QSIM_ERR_INVALID_ARGUMENT, "bad control position of a cross-rank gradient step");
    ShardGeom g;
    g.count = (1ull << L) >> (cpos >= 0 ? 1 : 0);  // (every index it forms is below 2^L)
    g.chunks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((g.count + 255) / 256, expect_chunks(1)));
    return g;
}

}  // namespace

void launch_dist_adjoint_diag(double2* phi, double2* lam, int L, int cpos, int v, const Op& inv, double* d_partials,
                              double* d_out, hipStream_t s, Timer* tm) {
    if (inv.kind != K_DIAG) fail(QSIM_ERR_INVALID_ARGUMENT, "the inverse of a diagonal rotation is not diagonal");
    const ShardGeom g = shard_geom(L, cpos);
    const double2 d = v ? make_double2(inv.m[2], inv.m[3]) : make_double2(inv.m[0], inv.m[1]);
    {
        TimedLaunch tl(tm, "dist_adjoint_diag", 64.0 * (double)g.count, s);
        hipLaunchKernelGGL(cpos >= 0 ? k_dist_adjoint_diag<true> : k_dist_adjoint_diag<false>, dim3(g.chunks), dim3(256),
                           0, s, phi, lam, g.count, cpos, v ? -1.0 : 1.0, d, d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    launch_sum_partials(d_partials, (int)g.chunks, 1, d_out, false, s);
}

void launch_dist_adjoint_step(double2* own, const double2* peer, const double2* lam, int L, int pauli, int cpos, int v,
                              const Op& inv, double* d_partials, double* d_out, hipStream_t s, Timer* tm) {
    if (inv.kind != K_M1 || (pauli != 1 && pauli != 2))
        fail(QSIM_ERR_INVALID_ARGUMENT, "a cross-rank gradient step needs an X or Y rotation");
    const ShardGeom g = shard_geom(L, cpos);
    // row v of U^† = [[m0, m1], [m2, m3]]: the own amplitude's coefficient, then the peer's
    const double2 a = v ? make_double2(inv.m[6], inv.m[7]) : make_double2(inv.m[0], inv.m[1]);
    const double2 b = v ? make_double2(inv.m[4], inv.m[5]) : make_double2(inv.m[2], inv.m[3]);
    const bool braket = lam != nullptr, ctrl = cpos >= 0;
    auto kernel = braket ? (pauli == 1 ? (ctrl ? k_dist_adjoint_step<1, true, true> : k_dist_adjoint_step<1, true, false>)
                                       : (ctrl ? k_dist_adjoint_step<2, true, true> : k_dist_adjoint_step<2, true, false>))
                         : (ctrl ? k_dist_adjoint_step<1, false, true> : k_dist_adjoint_step<1, false, false>);
    {
        TimedLaunch tl(tm, "dist_adjoint_step", (braket ? 64.0 : 48.0) * (double)g.count, s);
        hipLaunchKernelGGL(kernel, dim3(g.chunks), dim3(256), 0, s, own, peer, lam, g.count, cpos, v, a, b, d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    if (braket) launch_sum_partials(d_partials, (int)g.chunks, 1, d_out, false, s);
}

// The work shards (allocated on first use) and room for nparams x (shards + 1) slots.
qsim_dist::GradWork& ensure_grad(qsim_dist* d, size_t nparams) {
    if (!d->grad) d->grad = std::make_unique<qsim_dist::GradWork>();
    qsim_dist::GradWork& w = *d->grad;
    const size_t S = d->shards.size();
    auto grab = [&](void** p, size_t b) {
        if (*p) return;
        if (hipMalloc(p, b) != hipSuccess) {
            (void)hipGetLastError();  // (clear the sticky error: the state itself is intact)
            *p = nullptr;
            (void)hipStreamSynchronize(d->stream);
            d->grad.reset();
            fail(QSIM_ERR_DEVICE, "out of device memory for the gradient work shards");
        }
    };
    w.phi.resize(S, nullptr);
    w.lam.resize(S, nullptr);
    for (size_t i = 0; i < S; ++i) {
        grab((void**)&w.phi[i], sizeof(double2) << d->L);
        grab((void**)&w.lam[i], sizeof(double2) << d->L);
    }
    const size_t need = nparams * (S + 1);
    if (need > w.slots_cap) {
        if (w.d_slots) {
            QSIM_HIPCHK(hipStreamSynchronize(d->stream));
            (void)hipFree(w.d_slots);
            w.d_slots = nullptr;
            w.slots_cap = 0;
        }
        const size_t cap = std::max<size_t>(need, 256);
        grab((void**)&w.d_slots, cap * sizeof(double));
        w.slots_cap = cap;
    }
    while (w.terms.size() < S) w.terms.emplace_back(new DevBuf());
    return w;
}

// The sweep's two work states from the state where it lies: phi = the state, lambda = H phi under
// the same map (events 0 and 1 of d->events: free outside remaps).
void grad_load_work(qsim_dist* d, qsim_dist::GradWork& w, const DistApplyPlan& ap) {
    const int L = d->L;
    const size_t S = d->shards.size();
    if (ap.cross_groups && d->world == 1) fail(QSIM_ERR_RUNTIME, "cross-rank Pauli group in a world of one");
    ensure_events(d, 5);
    const uint64_t amps = 1ull << L;
    for (size_t i = 0; i < S; ++i) {
        QSIM_HIPCHK(hipMemcpyAsync(w.phi[i], d->shards[i].d, amps * sizeof(double2), hipMemcpyDeviceToDevice, d->stream));
        const std::vector<ExpectTerm> tab = dist_apply_terms(ap, L, d->shards[i].rank);
        w.terms[i]->upload(tab.data(), tab.size() * sizeof(ExpectTerm), d->stream);
    }
    std::vector<char> first(S, 1);
    uint64_t landed = 0;  // x_rank of the phi shards in the receive buffers
    for (const DistApplyGroup& g : ap.groups) {
        if (g.x_rank != 0 && g.x_rank != landed) {
            QSIM_HIPCHK(hipEventRecord(d->events[0], d->stream));  // phi written, the buffer's readers done
            QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[0], 0));
            std::vector<Post> posts;
            for (size_t i = 0; i < S; ++i) {
                const Shard& sh = d->shards[i];
                posts.push_back({sh.rank, (int)((uint64_t)sh.rank ^ g.x_rank), w.phi[i], sh.recvbuf, amps});
            }
            post_transfers(d, posts, "gradient H phi shard send/recv");
            QSIM_HIPCHK(hipEventRecord(d->events[1], d->comm_stream));
            QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[1], 0));
            landed = g.x_rank;
        }
        for (size_t i = 0; i < S; ++i) {
            const double2* src = g.x_rank ? d->shards[i].recvbuf : w.phi[i];
            launch_pauli_apply_group(src, w.lam[i], L, g.x_loc, (const ExpectTerm*)w.terms[i]->ptr + g.begin,
                                     g.end - g.begin, first[i] != 0, d->stream, &d->timer);
            first[i] = 0;
        }
    }
}

// grad[j] for j < P from the slots [parameter j][shard i]: the shards of this process in rank
// order, then the ranks: one vector all-reduce.
void grad_reduce(qsim_dist* d, qsim_dist::GradWork& w, size_t P, double* out) {
    const size_t S = d->shards.size();
    double* d_tot = w.d_slots + P * S;
    launch_sum_partials(w.d_slots, (int)S, (unsigned)P, d_tot, false, d->stream);
    allreduce_vec(d, d_tot, P, out);
    stream_wait(d, d->comm_stream);
}

// One inverted run of non-parameterised gates (execution order, logical qubits) on both work
// states, from work map wperm (updated).  The sharded planner without its overlap marks: ops
// steps as fused plans or per gate (flags), remaps whole, phi first, then lambda — the plan is a
// function of (gates, start map), so both end under the same map.  Nothing of the state's own run
// bookkeeping (map, counters, run plans, carry) is read or written.
static void grad_run_segment(qsim_dist* d, qsim_dist::GradWork& w, const std::vector<qsim_gate>& seg,
                             std::vector<int>& wperm, int flags) {
    if (seg.empty()) return;
    const size_t S = d->shards.size();
    ShardPlans* gs = nullptr;
    for (auto& c : w.segments)
        if (c->is(seg.data(), seg.size(), wperm)) gs = c.get();
    if (!gs) {
        if (w.segments.size() >= 64) {  // (their compiled kernels may still be queued)
            QSIM_HIPCHK(hipStreamSynchronize(d->stream));
            w.segments.clear();
        }
        auto c = std::make_unique<ShardPlans>();
        c->build(d->shards, seg.data(), seg.size(), wperm, [&](int rank, std::vector<int>& perm) {
            return plan_dist_core(seg.data(), seg.size(), d->n, d->g, rank, perm);
        });
        w.segments.push_back(std::move(c));
        gs = w.segments.back().get();
    }
    const std::vector<char> unfused(S, 0);
    for (const std::vector<double2*>* bufs : {&w.phi, &w.lam}) {
        std::vector<Shard> ws = d->shards;  // (the state's staging buffers, the work state's amplitudes)
        for (size_t i = 0; i < S; ++i) ws[i].d = (*bufs)[i];
        for (size_t k = 0; k < gs->steps[0].size(); ++k) {
            if (gs->steps[0][k].kind == 1) {
                exchange(d, gs->steps[0][k], unfused, &ws);
                continue;
            }
            for (size_t i = 0; i < S; ++i) {
                const std::vector<Op>& ops = gs->steps[i][k].ops;
                if (ops.empty()) continue;
                const StepRun r = prepare_step(d, ops, flags, *gs->fplans[i][k], 0, 0);
                run_part(d, ws[i], ops, r, 0, r.plan ? r.np : 1);
            }
        }
    }
    wperm = gs->perm_out;
}

// One parameterised step of the sweep: slots[i] = shard i's share of Im <lambda| G |phi>, then
// U^† on both work states (last: the circuit's first rotation, after which nothing is read —
// lambda is left as it is).  inv_gate: the inverse rotation on logical qubits.
static void grad_step(qsim_dist* d, qsim_dist::GradWork& w, const qsim_gate& inv_gate, const std::vector<int>& wperm,
                      double* slots, bool last, bool fused_step) {
    const int L = d->L;
    const size_t S = d->shards.size();
    qsim_gate pg = inv_gate;  // physical positions over all n
    for (int j = 0; j < pg.nqubits; ++j) pg.qubits[j] = wperm[inv_gate.qubits[j]];
    const int cls = dist_gradient_class(inv_gate, wperm.data(), L);
    const Generator gen = gate_generator(pg);
    const bool crank = cls == DG_LOCAL_CRANK || cls == DG_DIAG_CRANK || cls == DG_CROSS_CRANK;
    auto takes_part = [&](const Shard& sh) { return !crank || ((sh.rank >> (gen.c - L)) & 1); };
    const int cpos = gen.c >= 0 && gen.c < L ? gen.c : -1;
    if (cls == DG_LOCAL || cls == DG_LOCAL_CRANK) {
        qsim_gate lg = pg;
        Generator lgen = gen;
        if (crank) {  // the control reads 1 on every amplitude of a shard that takes part
            lg.type = pg.type == QSIM_GATE_CRY ? QSIM_GATE_RY : QSIM_GATE_RZ;
            lg.nqubits = 1;
            lg.qubits[0] = gen.t;
            lgen.c = -1;
        }
        const Op inv = lower_gate(lg, L);
        for (size_t i = 0; i < S; ++i) {
            if (!takes_part(d->shards[i])) continue;
            if (last || !fused_step)
                launch_braket(w.lam[i], w.phi[i], L, lgen, d->d_partials, nullptr, slots + i, d->stream, &d->timer);
            else
                launch_adjoint_step(w.phi[i], w.lam[i], L, lgen, inv, d->d_partials, slots + i, d->stream, &d->timer);
            if (!last && !fused_step) {
                launch_op(w.phi[i], L, 1, inv, d->stream, &d->timer);
                launch_op(w.lam[i], L, 1, inv, d->stream, &d->timer);
            }
        }
        return;
    }
    const Op inv = lower_gate(pg, d->n);
    const int tb = gen.t - L;  // the target's rank bit
    if (cls == DG_DIAG || cls == DG_DIAG_CRANK) {
        for (size_t i = 0; i < S; ++i)
            if (takes_part(d->shards[i]))
                launch_dist_adjoint_diag(w.phi[i], w.lam[i], L, cpos, (d->shards[i].rank >> tb) & 1, inv, d->d_partials,
                                         slots + i, d->stream, &d->timer);
        return;
    }
    // Rx / Ry / CRY across ranks.  Events 0 .. 2 of d->events (free outside remaps): the work
    // states' last writers and the staging buffers' last readers are done (0), the peer's phi has
    // landed in the receive buffer (1), its lambda in the send buffer (2).  Both transfers are
    // queued before the first kernel, so lambda crosses while phi is updated; a shard is updated
    // only after the transfer that sends it has completed.
    if (d->world == 1) fail(QSIM_ERR_RUNTIME, "cross-rank gradient step in a world of one");
    const uint64_t amps = 1ull << L;
    QSIM_HIPCHK(hipEventRecord(d->events[0], d->stream));
    QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[0], 0));
    for (int which = 0; which < (last ? 1 : 2); ++which) {
        std::vector<Post> posts;
        for (size_t i = 0; i < S; ++i) {
            const Shard& sh = d->shards[i];
            if (!takes_part(sh)) continue;
            posts.push_back({sh.rank, sh.rank ^ (1 << tb), which ? w.lam[i] : w.phi[i], which ? sh.sendbuf : sh.recvbuf,
                             amps});
        }
        post_transfers(d, posts, which ? "gradient lambda shard send/recv" : "gradient phi shard send/recv");
        QSIM_HIPCHK(hipEventRecord(d->events[1 + which], d->comm_stream));
    }
    QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[1], 0));
    for (size_t i = 0; i < S; ++i) {
        const Shard& sh = d->shards[i];
        if (takes_part(sh))
            launch_dist_adjoint_step(w.phi[i], sh.recvbuf, w.lam[i], L, gen.pauli, cpos, (sh.rank >> tb) & 1, inv,
                                     d->d_partials, slots + i, d->stream, &d->timer);
    }
    if (last) return;
    QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[2], 0));
    for (size_t i = 0; i < S; ++i) {
        const Shard& sh = d->shards[i];
        if (takes_part(sh))
            launch_dist_adjoint_step(w.lam[i], sh.sendbuf, nullptr, L, gen.pauli, cpos, (sh.rank >> tb) & 1, inv,
                                     d->d_partials, nullptr, d->stream, &d->timer);
    }
}

// The value and the sweep of qsim_dist_gradient, on the state the forward run left.
static void gradient_dist(qsim_dist* d, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                          size_t nterms, int flags, double* value, double* grad) {
    const int n = d->n, L = d->L;
    const size_t S = d->shards.size();
    *value = 0.0;
    for (size_t k = 0; k < count; ++k) grad[k] = 0.0;
    flush_carry(d);  // (the run's last step, if it was left pending)
    const DistApplyPlan ap = lower_dist_apply(n, L, terms, nterms, d->perm.data());
    if (ap.all.terms.empty()) {  // H = 0 (no terms, or every coefficient cancels): no sweep
        stream_wait(d, d->stream);
        return;
    }
    std::vector<size_t> params;
    for (size_t k = 0; k < count; ++k)
        if (gate_is_parameterised(gates[k].type)) params.push_back(k);
    // (the work shards first: a failed allocation leaves nothing queued)
    qsim_dist::GradWork* wp = params.empty() ? nullptr : &ensure_grad(d, params.size());
    *value = expectation_dist(d, terms, nterms);
    if (!wp) return;
    qsim_dist::GradWork& w = *wp;
    const double sent_before = d->sent_bytes;  // (remapBytes() stays the forward run's)
    std::vector<int> wperm = d->perm;
    grad_load_work(d, w, ap);
    // the sweep: slot [parameter j][shard i]
    const size_t P = params.size();
    QSIM_HIPCHK(hipMemsetAsync(w.d_slots, 0, P * (S + 1) * sizeof(double), d->stream));
    const bool fused_step = adjoint_fused_on();
    const size_t first_param = params.front();
    std::vector<qsim_gate> seg;
    size_t j = P;
    for (size_t k = count; k-- > first_param;) {
        const qsim_gate inv_gate = gate_inverse(gates[k]);
        if (!gate_is_parameterised(gates[k].type)) {
            seg.push_back(inv_gate);
            continue;
        }
        grad_run_segment(d, w, seg, wperm, flags);
        seg.clear();
        --j;
        grad_step(d, w, inv_gate, wperm, w.d_slots + j * S, k == first_param, fused_step);
    }
    std::vector<double> tot(P, 0.0);
    grad_reduce(d, w, P, tot.data());
    for (size_t q = 0; q < P; ++q) grad[params[q]] = tot[q];
    d->sent_bytes = sent_before;
}

// Host-only mirror of gradient_dist (qsim_dist_gradient_plan): the same classification and the
// same planner calls, from map `perm`.
static void gradient_plan_host(int n, int g, std::vector<int> perm, const qsim_gate* gates, size_t count,
                               const qsim_pauli_term* terms, size_t nterms, qsim_dist_gradient_info* out) {
    const int L = n - g;
    std::memset(out, 0, sizeof(*out));
    if (count) (void)plan_dist_core(gates, count, n, g, 0, perm);  // the forward run's end map
    for (int q = 0; q < n; ++q) out->perm_after_run[q] = out->perm_after_sweep[q] = perm[q];
    std::vector<size_t> params;
    for (size_t k = 0; k < count; ++k)
        if (gate_is_parameterised(gates[k].type)) params.push_back(k);
    out->params = (int32_t)params.size();
    const DistApplyPlan ap = lower_dist_apply(n, L, terms, nterms, perm.data());
    if (ap.all.terms.empty() || params.empty()) return;  // no sweep
    out->apply_groups_local = (int32_t)ap.local_groups;
    out->apply_groups_cross = (int32_t)ap.cross_groups;
    out->apply_transfers = (int32_t)ap.transfers;
    out->apply_launches = (int32_t)ap.launches;
    std::vector<qsim_gate> seg;
    const size_t first_param = params.front();
    for (size_t k = count; k-- > first_param;) {
        const qsim_gate inv_gate = gate_inverse(gates[k]);
        if (!gate_is_parameterised(gates[k].type)) {
            seg.push_back(inv_gate);
            continue;
        }
        if (!seg.empty()) {
            int remaps = 0;
            for (const DStep& st : plan_dist_core(seg.data(), seg.size(), n, g, 0, perm)) remaps += st.kind == 1;
            ++out->segments;
            out->remap_segments += remaps > 0;
            out->segment_remaps += remaps;
            seg.clear();
        }
        const Generator gen = gate_generator(inv_gate);
        const int cls = dist_gradient_class(inv_gate, perm.data(), L);
        switch (cls) {
            case DG_LOCAL:
                ++out->steps_local;
                if (gen.c >= 0) ++(perm[gen.c] < perm[gen.t] ? out->local_ctrl_below : out->local_ctrl_above);
                break;
            case DG_LOCAL_CRANK: ++out->steps_local_crank; break;
            case DG_DIAG: ++out->steps_diag; break;
            case DG_DIAG_CRANK: ++out->steps_diag_crank; break;
            default:
                ++(cls == DG_CROSS ? out->steps_cross : out->steps_cross_crank);
                ++(inv_gate.type == QSIM_GATE_RX   ? out->cross_rx
                   : inv_gate.type == QSIM_GATE_RY ? out->cross_ry
                                                   : out->cross_cry);
                out->step_transfers += k == first_param ? 1 : 2;  // (the first rotation needs phi alone)
                break;
        }
    }
    for (int q = 0; q < n; ++q) out->perm_after_sweep[q] = perm[q];
    out->bytes_sent_per_rank =
        (uint64_t)(out->apply_transfers + out->step_transfers) * ((uint64_t)sizeof(double2) << L);
}

}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_dist_gradient(qsim_dist* d, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                       size_t nterms, int flags, double* value, double* grad) {
    int rc = guarded([&] {
        need(d);
        if (!value) fail(QSIM_ERR_INVALID_ARGUMENT, "null value");
        if (!grad && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null gradient");
        check_gradient_args(d->n, gates, count, terms, nterms);
    });
    if (rc != QSIM_OK) return rc;
    // The forward run is qsim_dist_run itself: the state ends exactly as a plain run leaves it, and
    // nothing below writes to it.
    if (count > 0 && (rc = qsim_dist_run(d, gates, count, flags)) != QSIM_OK) return rc;
    return dguard_comm(d, [&] {
        QSIM_HIPCHK(hipSetDevice(d->device));
        gradient_dist(d, gates, count, terms, nterms, flags, value, grad);
    });
}

int qsim_dist_gradient_release(qsim_dist* d) {
    return guarded([&] {
        need(d);
        if (!d->grad) return;
        QSIM_HIPCHK(hipSetDevice(d->device));
        QSIM_HIPCHK(hipStreamSynchronize(d->stream));
        d->grad.reset();
    });
}

int qsim_dist_gradient_memory_bytes(qsim_dist* d, uint64_t* bytes) {
    return guarded([&] {
        need(d);
        if (!bytes) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        *bytes = 0;
        if (!d->grad) return;
        for (const auto* v : {&d->grad->phi, &d->grad->lam})
            for (const double2* p : *v)
                if (p) *bytes += sizeof(double2) << d->L;
    });
}

int qsim_dist_gradient_plan(int n_qubits, int world, const int32_t* perm, const qsim_gate* gates, size_t count,
                            const qsim_pauli_term* terms, size_t nterms, qsim_dist_gradient_info* out) {
    return guarded([&] {
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        const int g = HostPlanArgs(n_qubits, world).g;
        check_gradient_args(n_qubits, gates, count, terms, nterms);
        gradient_plan_host(n_qubits, g, checked_perm(n_qubits, perm), gates, count, terms, nterms, out);
    });
}

}  // extern "C"
