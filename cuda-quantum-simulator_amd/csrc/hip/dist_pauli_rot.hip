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
#include <cmath>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"

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

}  // namespace qsim_hip
