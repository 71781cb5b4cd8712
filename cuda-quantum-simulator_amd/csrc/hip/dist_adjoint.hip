// dist_adjoint.hip — adjoint-method gradients of <psi|H|psi> on a sharded state (dist.hip): the
// host lowering and the kernels the single-GPU sweep (adjoint.hip) lacks.  No reference counterpart.
//
// The sweep keeps two sharded work states, phi and lambda = H phi, under a qubit map of their own
// (the driver, gradient_dist in dist.hip, walks the circuit backwards as qsim_state_gradient does).
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
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"

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

}  // namespace qsim_hip
