// adjoint.hip — the kernels of adjoint-method gradients of <psi|H|psi> (no reference counterpart:
// the reference has no observable API).
//
// With phi_k = U_k ... U_1 |psi0>, lambda_k = U_{k+1}^† ... U_N^† H |phi_N> and, for a rotation
// U_k = exp(-i theta/2 G_k) (G_k = P_target, or |1><1|_control (x) P_target for CRY / CRZ),
//     dE/dtheta_k = Im <lambda_k| G_k |phi_k>.
// The backward sweep (capi.hip: qsim_state_gradient) starts from phi = phi_N, lambda = H phi_N and
// walks the circuit from its last gate to its first: at a rotation it accumulates the bra-ket, then
// applies U_k^† to both states.  Three kernels serve it:
//   pauli_apply   dst = H src out of place, one streaming pass per group of terms sharing an x mask
//   braket        <a| G |b> (Re and Im), a fixed-order two-stage reduction
//   adjoint_step  the bra-ket and the U^† of both states in one pass over the (i0, i1) pairs:
//                 64 B per amplitude of the active subspace, against 96 B for braket + two gates
// All of them read the amplitudes under the state's current qubit layout: the host maps gates,
// generators and Pauli masks from logical to physical positions.  Partial sums are added in a
// fixed order (wave, work-group, launch_sum_partials): results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"

namespace qsim_hip {

bool gate_is_parameterised(int type) {
    return type == QSIM_GATE_RX || type == QSIM_GATE_RY || type == QSIM_GATE_RZ || type == QSIM_GATE_CRY ||
           type == QSIM_GATE_CRZ;
}

qsim_gate gate_inverse(const qsim_gate& g) {
    qsim_gate r = g;
    switch (g.type) {
        case QSIM_GATE_S: r.type = QSIM_GATE_SDAG; break;
        case QSIM_GATE_SDAG: r.type = QSIM_GATE_S; break;
        case QSIM_GATE_T: r.type = QSIM_GATE_TDAG; break;
        case QSIM_GATE_TDAG: r.type = QSIM_GATE_T; break;
        default:
            if (gate_is_parameterised(g.type)) r.parameter = -g.parameter;
            break;  // every other gate is its own inverse
    }
    return r;
}

Generator gate_generator(const qsim_gate& g) {
    Generator gen;
    switch (g.type) {
        case QSIM_GATE_RX: gen.pauli = 1; gen.t = g.qubits[0]; break;
        case QSIM_GATE_RY: gen.pauli = 2; gen.t = g.qubits[0]; break;
        case QSIM_GATE_RZ: gen.pauli = 3; gen.t = g.qubits[0]; break;
        case QSIM_GATE_CRY: gen.pauli = 2; gen.c = g.qubits[0]; gen.t = g.qubits[1]; break;
        case QSIM_GATE_CRZ: gen.pauli = 3; gen.c = g.qubits[0]; gen.t = g.qubits[1]; break;
        default: fail(QSIM_ERR_INVALID_ARGUMENT, "gate has no parameter");
    }
    return gen;
}

// QSIM_ADJOINT_FUSED (default 1; read at every call, so a test or a benchmark runs both paths in
// one process): 0 composes a parameterised step from braket and two per-gate launches.
bool adjoint_fused_on() { return env_switch("QSIM_ADJOINT_FUSED", true); }

void check_gradient_args(int n, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms, size_t nterms) {
    if (!gates && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null gate list");
    if (!terms && nterms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
    for (size_t i = 0; i < count; ++i) validate_gate(gates[i], n);
    check_pauli_masks(n, terms, nterms, "Pauli term");
}

// The terms of dst = H src: (P src)[i] = i^nY (-1)^popcount((i ^ x) & z) src[i ^ x].  The sign is
// (-1)^popcount(i & z) (-1)^nY, so a term's complex weight c i^nY (-1)^nY = c (-i)^nY is prepared
// here (cr + i ci; one of the two is zero) and the kernel evaluates (-1)^popcount(i & z) alone.
ExpectPlan lower_pauli_apply(int n, const qsim_pauli_term* terms, size_t count, const int* perm) {
    return lower_pauli_terms(n, terms, count, perm, [](uint64_t x, uint64_t z, double c, ExpectTerm& e) {
        switch (__builtin_popcountll(x & z) & 3) {  // c (-i)^nY
            case 0: e.cr = c; break;
            case 1: e.ci = -c; break;
            case 2: e.cr = -c; break;
            default: e.ci = c; break;
        }
    });
}

namespace {

// conj(a) g
__device__ __forceinline__ double2 cjmul(double2 a, double2 g) {
    return make_double2(a.x * g.x + a.y * g.y, a.x * g.y - a.y * g.x);
}

// Pair k of the active subspace: zeros inserted at the ascending positions f0 (< f1), the control
// bit set.  f1 < 0: no control.
template <bool CTRL>
__device__ __forceinline__ uint64_t pair_index(uint64_t k, int f0, int f1, uint64_t cbit) {
    uint64_t lo = k & ((1ull << f0) - 1ull);
    k = ((k ^ lo) << 1) | lo;
    if (CTRL) {
        lo = k & ((1ull << f1) - 1ull);
        k = (((k ^ lo) << 1) | lo) | cbit;
    }
    return k;
}

// G b on one pair: (b0, b1) -> (g0, g1), G = X (1), Y (2) or Z (3) on the target.
template <int PAULI>
__device__ __forceinline__ void pauli_pair(double2 b0, double2 b1, double2& g0, double2& g1) {
    if (PAULI == 1) {
        g0 = b1;
        g1 = b0;
    } else if (PAULI == 2) {  // Y|0> = i|1>, Y|1> = -i|0>
        g0 = make_double2(b1.y, -b1.x);
        g1 = make_double2(-b0.y, b0.x);
    } else {
        g0 = b0;
        g1 = make_double2(-b1.x, -b1.y);
    }
}

// dst[i] (+)= W(i) src[i ^ x], W(i) = sum_t (-1)^popcount(i & z_t) (cr_t + i ci_t): one group of
// terms (one x mask), at most kExpectTerms of them per launch.  Lanes read i ^ x: consecutive i
// stay inside their aligned 2^k-amplitude block for the low bits of x, so a wave still covers
// whole 1 KiB runs.
template <bool ACC>
__global__ __launch_bounds__(256) void k_pauli_apply(const double2* __restrict__ src, double2* __restrict__ dst,
                                                     uint64_t N, uint64_t x, const ExpectTerm* terms, int nterms) {
    __shared__ ExpectTerm tab[kExpectTerms];
    for (int t = threadIdx.x; t < nterms; t += 256) tab[t] = terms[t];
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += step) {
        const double2 v = src[i ^ x];
        double wr, wi;
        term_weight<true>(tab, nterms, i, wr, wi);
        // (explicit fma: which product of a sum of two is rounded on its own is otherwise the
        // compiler's choice, and the gradients' last bit with it)
        double2 o = make_double2(fma(wr, v.x, -(wi * v.y)), fma(wi, v.x, wr * v.y));
        if (ACC) {
            const double2 d = dst[i];
            o.x += d.x;
            o.y += d.y;
        }
        dst[i] = o;
    }
}

// <a| G |b>: partials[block] = Re, partials[gridDim.x + block] = Im of the block's share.
// PAULI == 0: G = 1, one amplitude per thread and trip; else one (i0, i1) pair.
template <int PAULI, bool CTRL>
__global__ __launch_bounds__(256) void k_braket(const double2* __restrict__ a, const double2* __restrict__ b,
                                                uint64_t count, int f0, int f1, uint64_t cbit, uint64_t tbit,
                                                double* partials) {
    __shared__ double wre[4], wim[4];
    double re = 0.0, im = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        if (PAULI == 0) {
            const double2 p = cjmul(a[k], b[k]);
            re += p.x;
            im += p.y;
        } else {
            const uint64_t i0 = pair_index<CTRL>(k, f0, f1, cbit), i1 = i0 | tbit;
            double2 g0, g1;
            pauli_pair<PAULI>(b[i0], b[i1], g0, g1);
            const double2 p0 = cjmul(a[i0], g0), p1 = cjmul(a[i1], g1);
            re += p0.x + p1.x;
            im += p0.y + p1.y;
        }
    }
    re = block_sum(re, wre);
    im = block_sum(im, wim);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = re;
        partials[gridDim.x + blockIdx.x] = im;
    }
}

// One parameterised step of the backward sweep: partials[block] = the block's share of
// Im <lam| G |phi>, then (phi, lam) <- U^† (phi, lam) with U^† = [[m0, m1], [m2, m3]] on the
// target, over the pairs of the control == 1 subspace (the whole state without a control).
template <int PAULI, bool CTRL>
__global__ __launch_bounds__(256) void k_adjoint_step(double2* __restrict__ phi, double2* __restrict__ lam,
                                                      uint64_t count, int f0, int f1, uint64_t cbit, uint64_t tbit,
                                                      double2 m0, double2 m1, double2 m2, double2 m3,
                                                      double* partials) {
    __shared__ double wim[4];
    double im = 0.0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) {
        const uint64_t i0 = pair_index<CTRL>(k, f0, f1, cbit), i1 = i0 | tbit;
        double2 p0 = phi[i0], p1 = phi[i1], l0 = lam[i0], l1 = lam[i1];
        double2 g0, g1;
        pauli_pair<PAULI>(p0, p1, g0, g1);
        im += cjmul(l0, g0).y + cjmul(l1, g1).y;
        m1_pair(S_GEN, m0, m1, m2, m3, p0, p1);
        m1_pair(S_GEN, m0, m1, m2, m3, l0, l1);
        phi[i0] = p0;
        phi[i1] = p1;
        lam[i0] = l0;
        lam[i1] = l1;
    }
    im = block_sum(im, wim);
    if (threadIdx.x == 0) partials[blockIdx.x] = im;
}

struct PairGeom {
    uint64_t count, cbit, tbit;
    int f0, f1;
    unsigned chunks;
};
PairGeom pair_geom(int n, const Generator& g) {
    if (g.t < 0 || g.t >= n || g.c >= n || g.c == g.t) fail(QSIM_ERR_INVALID_ARGUMENT, "bad generator qubits");
    PairGeom p;
    const bool ctrl = g.c >= 0;
    p.count = (1ull << n) >> (ctrl ? 2 : 1);
    p.tbit = 1ull << g.t;
    p.cbit = ctrl ? 1ull << g.c : 0ull;
    p.f0 = ctrl ? std::min(g.t, g.c) : g.t;
    p.f1 = ctrl ? std::max(g.t, g.c) : -1;
    p.chunks = (unsigned)std::min<uint64_t>((p.count + 255) / 256, expect_chunks(1));
    return p;
}

}  // namespace

void launch_pauli_apply(const double2* src, double2* dst, int n, const ExpectPlan& plan, DevBuf& terms,
                        hipStream_t s, Timer* tm) {
    const uint64_t N = 1ull << n;
    if (plan.terms.empty()) {  // H = 0
        QSIM_HIPCHK(hipMemsetAsync(dst, 0, sizeof(double2) * N, s));
        return;
    }
    terms.upload(plan.terms.data(), plan.terms.size() * sizeof(ExpectTerm), s);
    const ExpectTerm* d_terms = (const ExpectTerm*)terms.ptr;
    bool first = true;
    for (const ExpectGroup& g : plan.groups) {
        launch_pauli_apply_group(src, dst, n, g.x, d_terms + g.begin, g.end - g.begin, first, s, tm);
        first = false;
    }
}

void launch_pauli_apply_group(const double2* src, double2* dst, int n, uint64_t x, const ExpectTerm* d_terms,
                              size_t count, bool first, hipStream_t s, Timer* tm) {
    const uint64_t N = 1ull << n;
    if (x >= N) fail(QSIM_ERR_INVALID_ARGUMENT, "x mask of a Pauli group outside the state");
    const unsigned blocks = (unsigned)std::min<uint64_t>((N + 255) / 256, 1u << 16);
    for (size_t t0 = 0; t0 < count; t0 += kExpectTerms) {
        const int nterms = (int)std::min<size_t>(kExpectTerms, count - t0);
        TimedLaunch tl(tm, "pauli_apply", (first ? 32.0 : 48.0) * (double)N, s);
        hipLaunchKernelGGL(first ? k_pauli_apply<false> : k_pauli_apply<true>, dim3(blocks), dim3(256), 0, s, src, dst, N,
                           x, d_terms + t0, nterms);
        QSIM_HIPCHK(hipGetLastError());
        first = false;
    }
}

void launch_braket(const double2* a, const double2* b, int n, const Generator& g, double* d_partials, double* d_re,
                   double* d_im, hipStream_t s, Timer* tm) {
    unsigned chunks;
    if (g.pauli == 0) {
        const uint64_t N = 1ull << n;
        chunks = (unsigned)std::min<uint64_t>((N + 255) / 256, expect_chunks(1));
        TimedLaunch tl(tm, "braket", 32.0 * (double)N, s);
        hipLaunchKernelGGL((k_braket<0, false>), dim3(chunks), dim3(256), 0, s, a, b, N, 0, -1, 0ull, 0ull,
                           d_partials);
        QSIM_HIPCHK(hipGetLastError());
    } else {
        if (g.pauli < 1 || g.pauli > 3) fail(QSIM_ERR_INVALID_ARGUMENT, "bad generator");
        const PairGeom p = pair_geom(n, g);
        const bool ctrl = g.c >= 0;
        chunks = p.chunks;
        auto kernel = g.pauli == 1 ? (ctrl ? k_braket<1, true> : k_braket<1, false>)
                      : g.pauli == 2 ? (ctrl ? k_braket<2, true> : k_braket<2, false>)
                                     : (ctrl ? k_braket<3, true> : k_braket<3, false>);
        TimedLaunch tl(tm, "braket", 64.0 * (double)p.count, s);
        hipLaunchKernelGGL(kernel, dim3(chunks), dim3(256), 0, s, a, b, p.count, p.f0, p.f1, p.cbit, p.tbit,
                           d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    if (d_re) launch_sum_partials(d_partials, (int)chunks, 1, d_re, false, s);
    if (d_im) launch_sum_partials(d_partials + chunks, (int)chunks, 1, d_im, false, s);
}

void launch_adjoint_step(double2* phi, double2* lam, int n, const Generator& g, const Op& inv, double* d_partials,
                         double* d_out, hipStream_t s, Timer* tm) {
    if (g.pauli < 1 || g.pauli > 3) fail(QSIM_ERR_INVALID_ARGUMENT, "bad generator");
    const PairGeom p = pair_geom(n, g);
    const bool ctrl = g.c >= 0;
    if (inv.t0 != g.t || inv.cmask != p.cbit || (inv.kind != K_M1 && inv.kind != K_DIAG))
        fail(QSIM_ERR_INVALID_ARGUMENT, "the inverse op does not act where the generator does");
    double2 m0, m1, m2, m3;
    if (inv.kind == K_M1) {
        m0 = make_double2(inv.m[0], inv.m[1]);
        m1 = make_double2(inv.m[2], inv.m[3]);
        m2 = make_double2(inv.m[4], inv.m[5]);
        m3 = make_double2(inv.m[6], inv.m[7]);
    } else {  // diagonal (d0, d1)
        m0 = make_double2(inv.m[0], inv.m[1]);
        m1 = m2 = make_double2(0.0, 0.0);
        m3 = make_double2(inv.m[2], inv.m[3]);
    }
    auto kernel = g.pauli == 1 ? (ctrl ? k_adjoint_step<1, true> : k_adjoint_step<1, false>)
                  : g.pauli == 2 ? (ctrl ? k_adjoint_step<2, true> : k_adjoint_step<2, false>)
                                 : (ctrl ? k_adjoint_step<3, true> : k_adjoint_step<3, false>);
    {
        TimedLaunch tl(tm, "adjoint_step", 128.0 * (double)p.count, s);
        hipLaunchKernelGGL(kernel, dim3(p.chunks), dim3(256), 0, s, phi, lam, p.count, p.f0, p.f1, p.cbit, p.tbit, m0,
                           m1, m2, m3, d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    launch_sum_partials(d_partials, (int)p.chunks, 1, d_out, false, s);
}

}  // namespace qsim_hip
