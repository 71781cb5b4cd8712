// dist_pauli_rot.hip — Pauli-string rotations exp(-i theta/2 P) and the backward step of their
// adjoint-method gradient on a sharded state (dist.hip): the host lowering and the one kernel
// family the single-GPU kernels (pauli_rot.hip) lack.  No reference counterpart.
//
// pauli_rot.hip's lowering runs over all n physical positions.  With L local positions, position
// p >= L is bit p - L of the rank, and a rotation's masks split as x = x_loc | x_rank << L, z alike:
//     (P psi)[(r, i)] = i^nY (-1)^popcount((r ^ x_rank) & z_rank) (-1)^popcount((i ^ x_loc) & z_loc)
//                       psi[(r ^ x_rank, i ^ x_loc)],   nY = popcount(x & z) over all n positions.
// The rank factor is constant on a shard and folded in on the host.  Classes:
//   phase  x == 0            P = s (-1)^popcount(i & z_loc) on shard r, s = (-1)^popcount(r & z_rank):
//                            pauli_rot.hip's k_pauli_phase with theta -> s theta in the shard's table;
//   local  x_rank == 0       exp(-i theta/2 s P_loc) = exp(-i (s theta)/2 P_loc): k_pauli_rot on the
//                            shard with theta -> s theta;
//   cross  x_rank != 0       rank r pairs with the single peer r ^ x_rank and reads its whole old
//                            shard from a staging buffer:
//                              own[i] <- c own[i] + w sg(i) peer[i ^ x_loc],
//                            sg(i) = (-1)^popcount((i ^ x_loc) & z_loc), w = -i sin(theta/2) g,
//                            g = i^nY (-1)^popcount((r ^ x_rank) & z_rank).  One thread per amplitude:
//                            32 B read, 16 B written (and 16 B per direction over the link).  The low
//                            bits of x_loc permute lanes inside aligned runs, so the peer stream
//                            stays coalesced (the argument of k_pauli_apply).
// The sweep's cross step (U^† = c + i sn P) is the same kernel with w = +i sn g, once per work
// state; the launch on phi first adds the work-group's share of Im conj(lam_own[i]) (P phi)_own[i],
// (P phi)_own[i] = g sg(i) peer[i ^ x_loc].  The two ranks' partial sums add up to the whole bra-ket.
// Without the store it is that sum alone (the sweep's last step).  No floating-point atomics:
// wave_sum, the four waves of a work-group in a fixed order, launch_sum_partials.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <cmath>
#include <vector>

#include "device_ops.hpp"
#include "dist_state.hpp"

namespace qsim_hip {

// ---- host-only lowering ---------------------------------------------------------------------

DistPauliRotPlan lower_dist_pauli_rotations(int n, int L, const qsim_pauli_term* rots, size_t count,
                                            const int* perm) {
    if (L < 1 || L > n) fail(QSIM_ERR_INVALID_ARGUMENT, "bad shard size");
    const PauliRotPlan all = lower_pauli_rotations(n, rots, count, perm);
    const uint64_t lmask = (1ull << L) - 1ull;
    DistPauliRotPlan p;
    p.rots.reserve(count);
    size_t run = 0;  // length of the current run of phase rotations
    auto close_run = [&] {
        if (run == 0) return;
        p.phase_passes += 1;
        p.launches += (run + kExpectTerms - 1) / kExpectTerms;
        run = 0;
    };
    for (const PauliRot& r : all.rots) {
        DistPauliRot d{DPR_PHASE, r.x & lmask, r.z & lmask, r.x >> L, r.z >> L, r.theta,
                       __builtin_popcountll(r.x & r.z)};
        if (r.x == 0) {
            ++p.phase;
            ++run;
        } else {
            close_run();
            p.launches += 1;
            if (d.x_rank == 0) {
                d.cls = DPR_LOCAL;
                ++p.local;
            } else {
                d.cls = DPR_CROSS;
                ++p.cross;
                if (d.x_loc == 0) ++p.cross_pure;
            }
        }
        p.rots.push_back(d);
    }
    close_run();
    return p;
}

PauliRot dist_pauli_shard_rot(const DistPauliRot& r, int rank) {
    if (r.cls == DPR_CROSS) fail(QSIM_ERR_INVALID_ARGUMENT, "a cross-rank rotation has no shard-local form");
    return PauliRot{r.x_loc, r.z_loc, dist_pauli_rank_neg(r, rank) ? -r.theta : r.theta};
}

// ---- kernels --------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ double2 cneg_if(bool neg, double2 w) {
    return neg ? make_double2(-w.x, -w.y) : w;
}

// own[i] <- c own[i] + w sg(i) peer[i ^ x] over the shard's `count` amplitudes (STORE);
// BRAKET (own = phi, lam = this rank's lambda): partials[block] = the block's share of
// Im conj(lam[i]) g sg(i) peer[i ^ x].  x, z: the local masks (x < count: i ^ x stays in the shard).
template <bool BRAKET, bool STORE>
__global__ __launch_bounds__(256) void k_dist_pauli_rot(double2* __restrict__ own, const double2* __restrict__ peer,
                                                        const double2* __restrict__ lam, uint64_t count, uint64_t x,
                                                        uint64_t z, double c, double2 w, double2 g,
                                                        double* partials) {
    __shared__ double wim[4];
    double im = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step) {
        const uint64_t j = i ^ x;
        const double2 b = peer[j];
        const bool neg = __popcll(j & z) & 1;
        if (BRAKET) {
            const double2 l = lam[i], gp = cmul(cneg_if(neg, g), b);  // (P phi)_own[i]
            im += l.x * gp.y - l.y * gp.x;
        }
        if (STORE) {
            const double2 a = own[i], p = cmul(cneg_if(neg, w), b);
            own[i] = make_double2(c * a.x + p.x, c * a.y + p.y);
        }
    }
    if (BRAKET) {
        im = block_sum(im, wim);
        if (threadIdx.x == 0) partials[blockIdx.x] = im;
    }
}

// i^k
double2 i_pow(int k) {
    switch (k & 3) {
        case 0: return make_double2(1.0, 0.0);
        case 1: return make_double2(0.0, 1.0);
        case 2: return make_double2(-1.0, 0.0);
        default: return make_double2(0.0, -1.0);
    }
}

}  // namespace

void launch_dist_pauli_rot(double2* own, const double2* peer, const double2* lam, int L, const DistPauliRot& r,
                           int rank, bool adjoint, bool store, double* d_partials, double* d_out, hipStream_t s,
                           Timer* tm) {
    // Guards of a launch that indexes with a mask: x_loc outside the shard would address past it.
    if (L < 1 || L > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad shard size");
    if ((r.x_loc | r.z_loc) >> L) fail(QSIM_ERR_INVALID_ARGUMENT, "local mask of a cross-rank rotation outside the shard");
    if (r.cls != DPR_CROSS || r.x_rank == 0) fail(QSIM_ERR_INVALID_ARGUMENT, "dist_pauli_rot needs a rank x mask");
    if (!own || !peer) fail(QSIM_ERR_INVALID_ARGUMENT, "null shard");
    const bool braket = lam != nullptr;
    if (!braket && !store) fail(QSIM_ERR_INVALID_ARGUMENT, "a cross-rank step that neither sums nor stores");
    const uint64_t count = 1ull << L;
    double2 g = i_pow(r.ny);
    if (dist_pauli_rank_neg(r, rank)) g = make_double2(-g.x, -g.y);
    const double c = std::cos(0.5 * r.theta), sn = std::sin(0.5 * r.theta);
    // forward -i sn g, adjoint +i sn g
    const double2 w = adjoint ? make_double2(-sn * g.y, sn * g.x) : make_double2(sn * g.y, -sn * g.x);
    uint64_t blocks = std::min<uint64_t>((count + 255) / 256, pauli_stream_blocks());
    if (braket) blocks = std::min<uint64_t>(blocks, expect_chunks(1));  // (one partial per work-group)
    auto kernel = braket ? (store ? k_dist_pauli_rot<true, true> : k_dist_pauli_rot<true, false>)
                         : k_dist_pauli_rot<false, true>;
    {
        TimedLaunch tl(tm, "dist_pauli_rot", ((braket ? 16.0 : 0.0) + (store ? 48.0 : 16.0)) * (double)count, s);
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, own, peer, lam, count, r.x_loc, r.z_loc, c,
                           w, g, d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    if (braket) launch_sum_partials(d_partials, (int)blocks, 1, d_out, false, s);
}

// The peers' whole shards `src` (one per shard of this process, this rank's own data) into the
// staging buffers (recv: the receive buffers, else the send buffers) for the pairing r <-> r ^ x_rank,
// on the comm stream after everything queued on d->stream so far (event 0: src written, the
// buffer's last readers done); `landed` is recorded when the shards have arrived.
static void post_peer_shards(qsim_dist* d, const std::vector<double2*>& src, uint64_t x_rank, bool recv,
                             hipEvent_t landed, const char* what) {
    QSIM_HIPCHK(hipEventRecord(d->events[0], d->stream));
    QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[0], 0));
    std::vector<Post> posts;
    for (size_t i = 0; i < d->shards.size(); ++i) {
        const Shard& sh = d->shards[i];
        posts.push_back({sh.rank, (int)((uint64_t)sh.rank ^ x_rank), src[i], recv ? sh.recvbuf : sh.sendbuf,
                         1ull << d->L});
    }
    post_transfers(d, posts, what);
    QSIM_HIPCHK(hipEventRecord(landed, d->comm_stream));
}

// The sequence on the state's shards, in order (qsim_dist_apply_pauli_rotations).  A cross rotation
// sends each shard itself; its kernel, the shard's next writer, waits for the transfer (event 1),
// which has then read the shard on this rank and landed the peer's in the receive buffer.
static void pauli_rotations_dist(qsim_dist* d, const DistPauliRotPlan& plan) {
    const int L = d->L;
    const size_t S = d->shards.size();
    if (plan.cross && d->world == 1) fail(QSIM_ERR_RUNTIME, "cross-rank Pauli rotation in a world of one");
    if (plan.cross) ensure_events(d, 5);
    const double sent_before = d->sent_bytes;  // (remapBytes() stays the last run's)
    // every phase run's table in one upload per shard (sequence order), before the first launch
    if (plan.phase) {
        while (d->rot_terms.size() < S) d->rot_terms.emplace_back(new DevBuf());
        for (size_t i = 0; i < S; ++i) {
            std::vector<ExpectTerm> tab;
            tab.reserve(plan.phase);
            for (const DistPauliRot& r : plan.rots)
                if (r.cls == DPR_PHASE) tab.push_back(ExpectTerm{r.z_loc, dist_pauli_shard_rot(r, d->shards[i].rank).theta, 0.0});
            d->rot_terms[i]->upload(tab.data(), tab.size() * sizeof(ExpectTerm), d->stream);
        }
    }
    std::vector<double2*> own(S);
    for (size_t i = 0; i < S; ++i) own[i] = d->shards[i].d;
    size_t done = 0;  // phase rotations launched so far
    for (size_t k = 0; k < plan.rots.size();) {
        const DistPauliRot& r = plan.rots[k];
        if (r.cls == DPR_PHASE) {
            size_t end = k;
            while (end < plan.rots.size() && plan.rots[end].cls == DPR_PHASE) ++end;
            for (size_t i = 0; i < S; ++i)
                launch_pauli_phase(own[i], L, (const ExpectTerm*)d->rot_terms[i]->ptr + done, end - k, d->stream, &d->timer);
            done += end - k;
            k = end;
            continue;
        }
        if (r.cls == DPR_LOCAL) {
            for (size_t i = 0; i < S; ++i)
                launch_pauli_rot(own[i], L, dist_pauli_shard_rot(r, d->shards[i].rank), d->stream, &d->timer);
        } else {
            post_peer_shards(d, own, r.x_rank, true, d->events[1], "Pauli rotation shard send/recv");
            QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[1], 0));
            for (size_t i = 0; i < S; ++i)
                launch_dist_pauli_rot(own[i], d->shards[i].recvbuf, nullptr, L, r, d->shards[i].rank, false, true,
                                      d->d_partials, nullptr, d->stream, &d->timer);
        }
        ++k;
    }
    d->sent_bytes = sent_before;
}

// One step of the rotation sweep (pauli_gradient_dist): slots[i] = shard i's share of
// Im <lambda| P |phi>, then exp(+i theta/2 P) on both work states; last (the sequence's first
// rotation): the bra-ket alone.  A cross step receives the peer's old phi shard (receive buffer,
// event 1), then its old lambda shard (send buffer, event 2): both transfers are queued before
// the first kernel, so lambda crosses while phi is updated, and each work shard is overwritten
// only after the transfer that sends it has completed.
static void pauli_grad_step(qsim_dist* d, qsim_dist::GradWork& w, const DistPauliRot& r, double* slots, bool last) {
    const int L = d->L;
    const size_t S = d->shards.size();
    if (r.cls != DPR_CROSS) {
        for (size_t i = 0; i < S; ++i) {
            const int rank = d->shards[i].rank;
            launch_pauli_adjoint_step(w.phi[i], w.lam[i], L, PauliRot{r.x_loc, r.z_loc, r.theta}, !last, d->d_partials,
                                      slots + i, d->stream, &d->timer, dist_pauli_rank_neg(r, rank));
        }
        return;
    }
    if (d->world == 1) fail(QSIM_ERR_RUNTIME, "cross-rank gradient step in a world of one");
    post_peer_shards(d, w.phi, r.x_rank, true, d->events[1], "Pauli gradient phi shard send/recv");
    if (!last) {
        std::vector<Post> posts;
        for (size_t i = 0; i < S; ++i) {
            const Shard& sh = d->shards[i];
            posts.push_back({sh.rank, (int)((uint64_t)sh.rank ^ r.x_rank), w.lam[i], sh.sendbuf, 1ull << L});
        }
        post_transfers(d, posts, "Pauli gradient lambda shard send/recv");
        QSIM_HIPCHK(hipEventRecord(d->events[2], d->comm_stream));
    }
    QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[1], 0));
    for (size_t i = 0; i < S; ++i)
        launch_dist_pauli_rot(w.phi[i], d->shards[i].recvbuf, w.lam[i], L, r, d->shards[i].rank, true, !last,
                              d->d_partials, slots + i, d->stream, &d->timer);
    if (last) return;
    QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[2], 0));
    for (size_t i = 0; i < S; ++i)
        launch_dist_pauli_rot(w.lam[i], d->shards[i].sendbuf, nullptr, L, r, d->shards[i].rank, true, true,
                              d->d_partials, nullptr, d->stream, &d->timer);
}

// The value and the sweep of qsim_dist_pauli_gradient, on the state the sequence left.  Rotations
// never change the map: no segments, no remaps, the work map stays the state's.
static void pauli_gradient_dist(qsim_dist* d, const DistPauliRotPlan& plan, const qsim_pauli_term* terms,
                                size_t nterms, double* value, double* grad) {
    const size_t S = d->shards.size(), P = plan.rots.size();
    *value = 0.0;
    for (size_t k = 0; k < P; ++k) grad[k] = 0.0;
    const DistApplyPlan ap = lower_dist_apply(d->n, d->L, terms, nterms, d->perm.data());
    if (ap.all.terms.empty()) {  // H = 0 (no terms, or every coefficient cancels): no sweep
        stream_wait(d, d->stream);
        return;
    }
    // (the work shards first: a failed allocation leaves nothing queued)
    qsim_dist::GradWork* wp = P ? &ensure_grad(d, P) : nullptr;
    *value = expectation_dist(d, terms, nterms);
    if (!wp) return;
    qsim_dist::GradWork& w = *wp;
    const double sent_before = d->sent_bytes;  // (remapBytes() stays the last run's)
    grad_load_work(d, w, ap);
    // the sweep: slot [rotation k][shard i], every rotation its own step, last to first
    QSIM_HIPCHK(hipMemsetAsync(w.d_slots, 0, P * (S + 1) * sizeof(double), d->stream));
    for (size_t k = P; k-- > 0;) pauli_grad_step(d, w, plan.rots[k], w.d_slots + k * S, k == 0);
    grad_reduce(d, w, P, grad);
    d->sent_bytes = sent_before;
}

// Host-only mirror of pauli_rotations_dist (qsim_dist_pauli_rotation_plan).
static void pauli_rotation_info(const DistPauliRotPlan& plan, int L, qsim_dist_pauli_rotation_info* out) {
    std::memset(out, 0, sizeof(*out));
    out->rotations = (int32_t)plan.rots.size();
    out->phase_rotations = (int32_t)plan.phase;
    out->phase_passes = (int32_t)plan.phase_passes;
    out->local_rotations = (int32_t)plan.local;
    out->cross_rotations = (int32_t)plan.cross;
    out->cross_pure = (int32_t)plan.cross_pure;
    out->launches = (int32_t)plan.launches;
    out->transfers = (int32_t)plan.cross;
    out->bytes_sent_per_rank = (uint64_t)plan.cross * ((uint64_t)sizeof(double2) << L);
}

}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_dist_apply_pauli_rotations(qsim_dist* d, const qsim_pauli_term* rots, size_t count) {
    return dguard_comm(d, [&] {
        need(d);
        if (!rots && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        if (count == 0) return;
        // (the lowering checks every mask of the sequence: nothing is launched or posted before)
        const DistPauliRotPlan plan = lower_dist_pauli_rotations(d->n, d->L, rots, count, d->perm.data());
        QSIM_HIPCHK(hipSetDevice(d->device));
        flush_carry(d);  // (the previous run's last step, if it was left pending)
        d->fresh = false;
        pauli_rotations_dist(d, plan);
    });
}

int qsim_dist_pauli_rotation_plan(int n_qubits, int world, const int32_t* perm, const qsim_pauli_term* rots,
                                  size_t count, qsim_dist_pauli_rotation_info* out) {
    return guarded([&] {
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        const int L = HostPlanArgs(n_qubits, world).L;
        if (!rots && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        const std::vector<int> p = checked_perm(n_qubits, perm);
        pauli_rotation_info(lower_dist_pauli_rotations(n_qubits, L, rots, count, p.data()), L, out);
    });
}

int qsim_dist_pauli_gradient(qsim_dist* d, const qsim_pauli_term* rots, size_t count, const qsim_pauli_term* terms,
                             size_t nterms, double* value, double* grad) {
    int rc = guarded([&] {
        need(d);
        if (!value) fail(QSIM_ERR_INVALID_ARGUMENT, "null value");
        if (!grad && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null gradient");
        if (!rots && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        if (!terms && nterms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
        // (the observable before the sequence is applied; the sequence's masks: by that call)
        check_pauli_masks(d->n, terms, nterms, "Pauli term");
    });
    if (rc != QSIM_OK) return rc;
    // The forward pass is qsim_dist_apply_pauli_rotations itself: the state ends exactly as that
    // call alone leaves it, and nothing below writes to it.
    if ((rc = qsim_dist_apply_pauli_rotations(d, rots, count)) != QSIM_OK) return rc;
    return dguard_comm(d, [&] {
        QSIM_HIPCHK(hipSetDevice(d->device));
        flush_carry(d);  // (count == 0: nothing above has flushed)
        const DistPauliRotPlan plan = lower_dist_pauli_rotations(d->n, d->L, rots, count, d->perm.data());
        pauli_gradient_dist(d, plan, terms, nterms, value, grad);
    });
}

int qsim_dist_pauli_gradient_plan(int n_qubits, int world, const int32_t* perm, const qsim_pauli_term* rots,
                                  size_t count, const qsim_pauli_term* terms, size_t nterms,
                                  qsim_dist_pauli_gradient_info* out) {
    return guarded([&] {
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        const int L = HostPlanArgs(n_qubits, world).L;
        if (!rots && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        if (!terms && nterms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
        check_pauli_masks(n_qubits, terms, nterms, "Pauli term");
        const std::vector<int> p = checked_perm(n_qubits, perm);
        const DistPauliRotPlan plan = lower_dist_pauli_rotations(n_qubits, L, rots, count, p.data());
        const DistApplyPlan ap = lower_dist_apply(n_qubits, L, terms, nterms, p.data());
        std::memset(out, 0, sizeof(*out));
        pauli_rotation_info(plan, L, &out->forward);
        out->first_class = -1;
        out->bytes_sent_per_rank = out->forward.bytes_sent_per_rank;
        if (ap.all.terms.empty() || plan.rots.empty()) return;  // no sweep
        out->apply_groups_local = (int32_t)ap.local_groups;
        out->apply_groups_cross = (int32_t)ap.cross_groups;
        out->apply_transfers = (int32_t)ap.transfers;
        out->apply_launches = (int32_t)ap.launches;
        out->steps = (int32_t)plan.rots.size();
        out->steps_phase = (int32_t)plan.phase;
        out->steps_local = (int32_t)plan.local;
        out->steps_cross = (int32_t)plan.cross;
        out->first_class = plan.rots.front().cls;
        // (phi and lambda per cross step; the sequence's first rotation needs phi alone)
        out->step_transfers = (int32_t)(2 * plan.cross) - (plan.rots.front().cls == DPR_CROSS ? 1 : 0);
        out->bytes_sent_per_rank +=
            (uint64_t)(out->apply_transfers + out->step_transfers) * ((uint64_t)sizeof(double2) << L);
    });
}

}  // extern "C"
