// pauli_rot.hip — Pauli-string rotations exp(-i theta/2 P) and the backward step of their
// adjoint-method gradient (no reference counterpart: the reference has neither observables nor
// multi-qubit rotations).
//
// P is a string of X / Y / Z factors given as two masks (x: X or Y, z: Z or Y), with the convention
// of adjoint.hip:
//     (P psi)[i] = i^nY (-1)^popcount((i ^ x) & z) psi[i ^ x],   nY = popcount(x & z).
// P^2 = 1, so exp(-i theta/2 P) = cos(theta/2) - i sin(theta/2) P: whatever the string's weight, a
// rotation pairs amplitude i with j = i ^ x and is one streaming pass over the state (32 B per
// amplitude).  With sg(i) = (-1)^popcount(i & z) the pair update is
//     psi'[i] = c psi[i] + w (-1)^nY sg(i) psi[j],   psi'[j] = c psi[j] + w sg(i) psi[i],
// w = -i sin(theta/2) i^nY: the host prepares both complex weights, the kernel evaluates sg alone.
// Three kernels:
//   pauli_rot           x != 0, one thread per pair; i comes from the pair number by inserting a
//                       zero at the highest bit of x, so the low bits of x only permute lanes inside
//                       aligned runs (the coalescing argument of k_pauli_apply)
//   pauli_phase         x == 0: a run of consecutive Z/I-only rotations (they commute) as one pass,
//                       psi[i] *= exp(-i/2 sum_t theta_t (-1)^popcount(i & z_t)); the terms sit in
//                       LDS (broadcast reads), one sincos per amplitude and launch
//   pauli_adjoint_step  one step of the backward sweep for a generator G = P: the work-group's share
//                       of Im <lam| P |phi>, then exp(+i theta/2 P) on both work states in the same
//                       pass (64 B per amplitude); a pair form (x != 0) and a per-amplitude form
//                       (x == 0); without the stores it is the bra-ket alone (the sweep's last step)
// All of them work on physical positions under the state's current layout: the host maps the
// logical masks through perm (lower_pauli_rotations).  No floating-point atomics: partial sums are
// added in a fixed order (wave, work-group, launch_sum_partials), so results are bitwise
// reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"

namespace qsim_hip {

PauliRotPlan lower_pauli_rotations(int n, const qsim_pauli_term* rots, size_t count, const int* perm) {
    check_qubit_perm(n, perm);
    if (count && !rots) fail(QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
    check_pauli_masks(n, rots, count, "Pauli rotation");  // (the whole sequence: a caller lowers before it launches)
    auto to_phys = [&](uint64_t m) { return mask_to_physical(m, n, perm); };
    PauliRotPlan plan;
    plan.rots.reserve(count);
    size_t run = 0;  // length of the current run of x == 0 rotations
    auto close_run = [&] {
        if (run == 0) return;
        plan.passes += 1;
        plan.launches += (run + kExpectTerms - 1) / kExpectTerms;
        run = 0;
    };
    for (size_t t = 0; t < count; ++t) {
        const PauliRot r{to_phys(rots[t].x_mask), to_phys(rots[t].z_mask), rots[t].coeff};
        plan.rots.push_back(r);
        if (r.x == 0) {
            ++run;
        } else {
            close_run();
            plan.passes += 1;
            plan.launches += 1;
        }
    }
    close_run();
    return plan;
}

// QSIM_PAULI_BLOCKS (default and most 65536, the cap of k_pauli_apply; read at every call, so a test
// runs several grid-stride trips on a small state): the most work-groups of pauli_rot and
// pauli_phase.  Larger states take further trips, by default from 2^24 pairs or amplitudes on.
// Measured at 28 qubits against a cap of 2048 (one resident set): pauli_rot 1.68 against 1.79 ms,
// pauli_phase 2.42 against 2.79 ms.
uint64_t pauli_stream_blocks() {
    const char* e = std::getenv("QSIM_PAULI_BLOCKS");
    const long v = e ? std::atol(e) : 0;
    return v >= 1 && v <= 65536 ? (uint64_t)v : 65536;
}

namespace {

// Pair k: a zero inserted at position hbit (lomask = 2^hbit - 1).
__device__ __forceinline__ uint64_t insert0(uint64_t k, uint64_t lomask) {
    const uint64_t lo = k & lomask;
    return ((k ^ lo) << 1) | lo;
}

__device__ __forceinline__ double2 cneg_if(bool neg, double2 w) {
    return neg ? make_double2(-w.x, -w.y) : w;
}

// i u
__device__ __forceinline__ double2 times_i(double2 u) { return make_double2(-u.y, u.x); }

// st <- (c + w P) st over the pairs (i, j = i ^ x), bit hbit of i clear: wi / wj are the weights
// of the partner in the i half and in the j half, up to the sign (-1)^popcount(i & z).
__global__ __launch_bounds__(256) void k_pauli_rot(double2* __restrict__ st, uint64_t pairs, uint64_t lomask,
                                                   uint64_t x, uint64_t z, double c, double2 wi, double2 wj) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < pairs; k += step) {
        const uint64_t i = insert0(k, lomask), j = i ^ x;
        const double2 a = st[i], b = st[j];
        const bool neg = __popcll(i & z) & 1;
        const double2 pi = cmul(cneg_if(neg, wi), b), pj = cmul(cneg_if(neg, wj), a);
        st[i] = make_double2(c * a.x + pi.x, c * a.y + pi.y);
        st[j] = make_double2(c * b.x + pj.x, c * b.y + pj.y);
    }
}

// st[i] *= exp(-i/2 sum_t theta_t (-1)^popcount(i & z_t)) over the nterms <= kExpectTerms terms
// (ExpectTerm: z and cr = theta).
__global__ __launch_bounds__(256) void k_pauli_phase(double2* __restrict__ st, uint64_t N, const ExpectTerm* terms,
                                                     int nterms) {
    __shared__ uint64_t zs[kExpectTerms];
    __shared__ double th[kExpectTerms];
    for (int t = threadIdx.x; t < nterms; t += 256) {
        zs[t] = terms[t].z;
        th[t] = terms[t].cr;
    }
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += step) {
        const double2 v = st[i];
        double a = 0.0;
        for (int t = 0; t < nterms; ++t) {  // (same LDS address in every lane: broadcast reads)
            const bool neg = __popcll(i & zs[t]) & 1;
            a += neg ? -th[t] : th[t];
        }
        double sn, cs;
        sincos(-0.5 * a, &sn, &cs);
        st[i] = make_double2(cs * v.x - sn * v.y, cs * v.y + sn * v.x);
    }
}

// One step of the backward sweep for G = P: partials[block] = the block's share of Im <lam| P |phi>,
// then, with APPLY, (phi, lam) <- (c + i sn P) (phi, lam).  PAIR: x != 0, one (i, j = i ^ x) pair
// per thread, gi / gj = i^nY (-1)^nY and i^nY (the weights of P in the i and the j half, up to the
// sign (-1)^popcount(i & z)); else one amplitude per thread, P = that sign.
template <bool PAIR, bool APPLY>
__global__ __launch_bounds__(256) void k_pauli_adjoint_step(double2* __restrict__ phi, double2* __restrict__ lam,
                                                            uint64_t count, uint64_t lomask, uint64_t x, uint64_t z,
                                                            double c, double sn, double2 gi, double2 gj,
                                                            double* partials) {
    __shared__ double wim[4];
    double im = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        if (PAIR) {
            const uint64_t i = insert0(k, lomask), j = i ^ x;
            const double2 p0 = phi[i], p1 = phi[j], l0 = lam[i], l1 = lam[j];
            const bool neg = __popcll(i & z) & 1;
            const double2 si = cneg_if(neg, gi), sj = cneg_if(neg, gj);
            const double2 gp0 = cmul(si, p1), gp1 = cmul(sj, p0);  // P phi
            im += (l0.x * gp0.y - l0.y * gp0.x) + (l1.x * gp1.y - l1.y * gp1.x);
            if (APPLY) {
                const double2 gl0 = cmul(si, l1), gl1 = cmul(sj, l0);  // P lam
                const double2 up0 = times_i(gp0), up1 = times_i(gp1), ul0 = times_i(gl0), ul1 = times_i(gl1);
                phi[i] = make_double2(c * p0.x + sn * up0.x, c * p0.y + sn * up0.y);
                phi[j] = make_double2(c * p1.x + sn * up1.x, c * p1.y + sn * up1.y);
                lam[i] = make_double2(c * l0.x + sn * ul0.x, c * l0.y + sn * ul0.y);
                lam[j] = make_double2(c * l1.x + sn * ul1.x, c * l1.y + sn * ul1.y);
            }
        } else {
            const double2 p = phi[k], l = lam[k];
            const bool neg = __popcll(k & z) & 1;
            const double b = l.x * p.y - l.y * p.x;  // Im conj(lam) phi
            im += neg ? -b : b;
            if (APPLY) {
                const double s = neg ? -sn : sn;  // the factor c + i s
                phi[k] = make_double2(c * p.x - s * p.y, c * p.y + s * p.x);
                lam[k] = make_double2(c * l.x - s * l.y, c * l.y + s * l.x);
            }
        }
    }
    im = block_sum(im, wim);
    if (threadIdx.x == 0) partials[blockIdx.x] = im;
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

// Guard of the launches that index with a mask: x outside the state would address past it.
void check_masks(int n, const PauliRot& r) {
    if (n < 1 || n > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
    if ((r.x | r.z) >> n) fail(QSIM_ERR_INVALID_ARGUMENT, "mask of a Pauli rotation outside the state");
}

}  // namespace

void launch_pauli_rot(double2* st, int n, const PauliRot& r, hipStream_t s, Timer* tm) {
    check_masks(n, r);
    if (r.x == 0) fail(QSIM_ERR_INVALID_ARGUMENT, "pauli_rot needs an x mask");
    const uint64_t N = 1ull << n, pairs = N >> 1;
    const int hbit = 63 - __builtin_clzll(r.x);
    const int ny = __builtin_popcountll(r.x & r.z);
    const double c = std::cos(0.5 * r.theta), sn = std::sin(0.5 * r.theta);
    const double2 g = i_pow(ny);
    const double2 wj = make_double2(sn * g.y, -sn * g.x);  // -i sin(theta/2) i^nY
    const double2 wi = ny & 1 ? make_double2(-wj.x, -wj.y) : wj;
    const unsigned blocks = (unsigned)std::min<uint64_t>((pairs + 255) / 256, pauli_stream_blocks());
    TimedLaunch tl(tm, "pauli_rot", 32.0 * (double)N, s);
    hipLaunchKernelGGL(k_pauli_rot, dim3(blocks), dim3(256), 0, s, st, pairs, (1ull << hbit) - 1ull, r.x, r.z, c, wi,
                       wj);
    QSIM_HIPCHK(hipGetLastError());
}

void launch_pauli_phase(double2* st, int n, const ExpectTerm* d_terms, size_t count, hipStream_t s, Timer* tm) {
    if (n < 1 || n > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
    const uint64_t N = 1ull << n;
    const unsigned blocks = (unsigned)std::min<uint64_t>((N + 255) / 256, pauli_stream_blocks());
    for (size_t t0 = 0; t0 < count; t0 += kExpectTerms) {
        const int nterms = (int)std::min<size_t>(kExpectTerms, count - t0);
        TimedLaunch tl(tm, "pauli_phase", 32.0 * (double)N, s);
        hipLaunchKernelGGL(k_pauli_phase, dim3(blocks), dim3(256), 0, s, st, N, d_terms + t0, nterms);
        QSIM_HIPCHK(hipGetLastError());
    }
}

void launch_pauli_rotations(double2* st, int n, const PauliRotPlan& plan, DevBuf& terms, hipStream_t s, Timer* tm) {
    // every run's table in one upload (sequence order), before the first launch
    std::vector<ExpectTerm> tab;
    for (const PauliRot& r : plan.rots)
        if (r.x == 0) tab.push_back(ExpectTerm{r.z, r.theta, 0.0});
    terms.upload(tab.data(), tab.size() * sizeof(ExpectTerm), s);
    const ExpectTerm* d_terms = (const ExpectTerm*)terms.ptr;
    size_t done = 0;  // x == 0 rotations launched so far
    for (size_t k = 0; k < plan.rots.size();) {
        if (plan.rots[k].x != 0) {
            launch_pauli_rot(st, n, plan.rots[k], s, tm);
            ++k;
            continue;
        }
        size_t end = k;
        while (end < plan.rots.size() && plan.rots[end].x == 0) ++end;
        launch_pauli_phase(st, n, d_terms + done, end - k, s, tm);
        done += end - k;
        k = end;
    }
}

void launch_pauli_adjoint_step(double2* phi, double2* lam, int n, const PauliRot& r, bool apply, double* d_partials,
                               double* d_out, hipStream_t s, Timer* tm, bool negate) {
    check_masks(n, r);
    const uint64_t N = 1ull << n;
    const bool pair = r.x != 0;
    const uint64_t count = pair ? N >> 1 : N;
    const uint64_t lomask = pair ? (1ull << (63 - __builtin_clzll(r.x))) - 1ull : 0ull;
    const int ny = __builtin_popcountll(r.x & r.z);
    double2 gj = i_pow(ny);
    double c = std::cos(0.5 * r.theta), sn = std::sin(0.5 * r.theta);  // U^† = c + i sn P
    if (negate) {
        // Generator -P.  Pair form: the sign goes into the two weights of P.  Amplitude form (no
        // weights): Im <phi|P|lam> = -Im <lam|P|phi> and both states get the same update, so the
        // states swap roles and the update's angle flips.
        if (pair) {
            gj = make_double2(-gj.x, -gj.y);
        } else {
            std::swap(phi, lam);
            sn = -sn;
        }
    }
    const double2 gi = ny & 1 ? make_double2(-gj.x, -gj.y) : gj;
    const unsigned chunks = (unsigned)std::min<uint64_t>((count + 255) / 256, expect_chunks(1));
    auto kernel = pair ? (apply ? k_pauli_adjoint_step<true, true> : k_pauli_adjoint_step<true, false>)
                       : (apply ? k_pauli_adjoint_step<false, true> : k_pauli_adjoint_step<false, false>);
    {
        TimedLaunch tl(tm, "pauli_adjoint_step", (apply ? 64.0 : 32.0) * (double)N, s);
        hipLaunchKernelGGL(kernel, dim3(chunks), dim3(256), 0, s, phi, lam, count, lomask, r.x, r.z, c, sn, gi, gj,
                           d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    launch_sum_partials(d_partials, (int)chunks, 1, d_out, false, s);
}

}  // namespace qsim_hip

// ---- the C entries: rotations and their adjoint gradient on a single-GPU state ----
using namespace qsim_hip;

extern "C" {

int qsim_state_apply_pauli_rotations(qsim_state* s, const qsim_pauli_term* rots, size_t count) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(rots || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        if (count == 0) return;
        DeviceGuard dg(s->device);
        share_flush(s);  // (pending gates of a run-sharing cycle; the layout may change with them)
        // (the lowering checks every mask of the sequence: nothing of it is launched before)
        const PauliRotPlan plan =
            lower_pauli_rotations(s->n, rots, count, s->perm.empty() ? nullptr : s->perm.data());
        s->basis = false;
        launch_pauli_rotations(s->d, s->n, plan, s->expect_terms, s->stream, &s->timer);
    });
}

int qsim_pauli_rotation_plan(int n_qubits, const qsim_pauli_term* rots, size_t count, const int32_t* perm,
                             int* passes, int* launches) {
    return guarded([&] {
        QSIM_REQUIRE(rots || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        QSIM_REQUIRE(passes && launches, QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        const PauliRotPlan plan = lower_pauli_rotations(n_qubits, rots, count, perm);
        *passes = (int)plan.passes;
        *launches = (int)plan.launches;
    });
}

int qsim_pauli_gradient_plan(int n_qubits, const qsim_pauli_term* rots, size_t count,
                             const qsim_pauli_term* terms, size_t nterms, const int32_t* perm, int* steps,
                             int* apply_passes) {
    return guarded([&] {
        QSIM_REQUIRE(rots || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        QSIM_REQUIRE(terms || nterms == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        QSIM_REQUIRE(steps && apply_passes, QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        const PauliRotPlan plan = lower_pauli_rotations(n_qubits, rots, count, perm);
        const ExpectPlan aplan = lower_pauli_apply(n_qubits, terms, nterms, perm);
        *steps = aplan.terms.empty() ? 0 : (int)plan.rots.size();  // (H == 0: no sweep)
        *apply_passes = (int)aplan.launches;
    });
}

int qsim_state_pauli_gradient(qsim_state* s, const qsim_pauli_term* rots, size_t count,
                              const qsim_pauli_term* terms, size_t nterms, double* value, double* grad) {
    int rc = guarded([&] {
        check_state(s);
        QSIM_REQUIRE(value, QSIM_ERR_INVALID_ARGUMENT, "null value");
        QSIM_REQUIRE(grad || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gradient");
        QSIM_REQUIRE(rots || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null rotation list");
        QSIM_REQUIRE(terms || nterms == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        // (the observable before the sequence is applied; the sequence's masks: by that call)
        check_pauli_masks(s->n, terms, nterms, "Pauli term");
    });
    if (rc != QSIM_OK) return rc;
    // The forward pass is qsim_state_apply_pauli_rotations itself: the state ends exactly as that
    // call alone leaves it, and nothing below writes to it.
    if ((rc = qsim_state_apply_pauli_rotations(s, rots, count)) != QSIM_OK) return rc;
    return guarded([&] {
        DeviceGuard dg(s->device);
        share_flush(s);  // (count == 0: nothing above has flushed)
        const int n = s->n;
        GradWork* wp = gradient_prologue(s, terms, nterms, count, count > 0, value, grad);
        if (!wp) return;  // H = 0, or no rotation: the value alone
        GradWork& w = *wp;
        const PauliRotPlan plan =
            lower_pauli_rotations(n, rots, count, s->perm.empty() ? nullptr : s->perm.data());
        // every rotation its own step, last to first; the first rotation undoes nothing
        for (size_t k = count; k-- > 0;)
            launch_pauli_adjoint_step(w.phi, w.lam, n, plan.rots[k], k > 0, s->d_partials, w.d_out + k, s->stream,
                                      &s->timer);
        QSIM_HIPCHK(hipMemcpyAsync(grad, w.d_out, count * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

}  // extern "C"
