// adjoint.hip — the kernels of adjoint-method gradients of <psi|H|psi> (no reference counterpart:
// the reference has no observable API).
//
// With phi_k = U_k ... U_1 |psi0>, lambda_k = U_{k+1}^† ... U_N^† H |phi_N> and, for a rotation
// U_k = exp(-i theta/2 G_k) (G_k = P_target, or |1><1|_control (x) P_target for CRY / CRZ),
//     dE/dtheta_k = Im <lambda_k| G_k |phi_k>.
// The backward sweep (qsim_state_gradient below) starts from phi = phi_N, lambda = H phi_N and
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
#include <memory>
#include <string>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"

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
                        hipStream_t s, Timer* tm, uint64_t batch) {
    const uint64_t N = batch << n;
    if (plan.terms.empty()) {  // H = 0
        QSIM_HIPCHK(hipMemsetAsync(dst, 0, sizeof(double2) * N, s));
        return;
    }
    terms.upload(plan.terms.data(), plan.terms.size() * sizeof(ExpectTerm), s);
    const ExpectTerm* d_terms = (const ExpectTerm*)terms.ptr;
    bool first = true;
    for (const ExpectGroup& g : plan.groups) {
        launch_pauli_apply_group(src, dst, n, g.x, d_terms + g.begin, g.end - g.begin, first, s, tm, batch);
        first = false;
    }
}

void launch_pauli_apply_group(const double2* src, double2* dst, int n, uint64_t x, const ExpectTerm* d_terms,
                              size_t count, bool first, hipStream_t s, Timer* tm, uint64_t batch) {
    // (the masks lie below 2^n: i ^ x never leaves a member, and a member's index bits above n
    // meet no z bit — the launch over batch x 2^n amplitudes is the single state's, longer)
    if (batch < 1 || (batch << n) >> n != batch) fail(QSIM_ERR_INVALID_ARGUMENT, "bad member count of a Pauli-sum apply");
    if (x >> n) fail(QSIM_ERR_INVALID_ARGUMENT, "x mask of a Pauli group outside the state");
    const uint64_t N = batch << n;
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

// ---- the gradient on a single-GPU state ----
// The work states of the backward sweep and room for `count` per-gate results.
static GradWork& ensure_grad(qsim_state* s, size_t count) {
    if (!s->grad) s->grad = std::make_unique<GradWork>();
    GradWork& w = *s->grad;
    const size_t bytes = sizeof(double2) << s->n;
    auto grab = [&](void** p, size_t b) {
        if (*p) return;
        if (hipMalloc(p, b) != hipSuccess) {
            (void)hipGetLastError();  // (clear the sticky error: the state itself is intact)
            *p = nullptr;
            s->grad.reset();
            fail(QSIM_ERR_DEVICE, "out of device memory for the gradient work states");
        }
    };
    grab((void**)&w.phi, bytes);
    grab((void**)&w.lam, bytes);
    if (count > w.out_cap) {
        if (w.d_out) {
            QSIM_HIPCHK(hipStreamSynchronize(s->stream));
            (void)hipFree(w.d_out);
            w.d_out = nullptr;
            w.out_cap = 0;
        }
        const size_t cap = std::max<size_t>(count, 256);
        grab((void**)&w.d_out, cap * sizeof(double));
        w.out_cap = cap;
    }
    return w;
}

// Inverted non-parameterised gates (execution order) on both work states, the way `flags` says.
static void grad_apply_segment(qsim_state* s, GradWork& w, const std::vector<Op>& seg, int flags) {
    if (seg.empty()) return;
    if (flags & QSIM_RUN_FUSED) {
        PlanCache::Entry& pe = w.plans.get(seg, s->n, s->stream);
        const Plan& plan = pe.plan;
        w.ops.upload(plan.ops.data(), plan.ops.size() * sizeof(TileOp), s->stream);
        w.stages.upload(plan.stages.data(), plan.stages.size() * sizeof(Stage), s->stream);
        for (double2* buf : {w.phi, w.lam}) {
            double2* r = launch_fused(buf, s->n, 1, plan, (const TileOp*)w.ops.ptr, (const Stage*)w.stages.ptr,
                                      s->stream, &s->timer);
            if (r != buf) fail(QSIM_ERR_RUNTIME, "a gradient segment planned a relayout pass");
        }
    } else {
        for (const Op& op : seg) {
            launch_op(w.phi, s->n, 1, op, s->stream, &s->timer);
            launch_op(w.lam, s->n, 1, op, s->stream, &s->timer);
        }
    }
}

// What the two gradient entry points (here and in pauli_rot.hip) do once the forward pass has run:
// the outputs zeroed, *value = <psi|H|psi> queued and, with `sweep` (there is something to
// differentiate), the work states of the backward sweep queued as well: phi = a copy of the state
// where it lies, lambda = H phi under that layout.  Returns them, or null when the call is already
// complete (H = 0, or no sweep): the stream is then drained.
GradWork* gradient_prologue(qsim_state* s, const qsim_pauli_term* terms, size_t nterms, size_t count, bool sweep,
                            double* value, double* grad) {
    const int n = s->n;
    *value = 0.0;
    for (size_t k = 0; k < count; ++k) grad[k] = 0.0;
    const int* perm = s->perm.empty() ? nullptr : s->perm.data();
    const ExpectPlan eplan = lower_expectation(n, terms, nterms, perm);
    if (eplan.terms.empty()) {  // H = 0 (no terms, or every coefficient cancels): no sweep
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
        return nullptr;
    }
    // (the work states first: a failed allocation leaves nothing queued)
    GradWork* w = sweep ? &ensure_grad(s, count) : nullptr;
    launch_expectation(s->d, n, 1, eplan, s->expect_terms, s->d_partials, s->d_result, s->stream, &s->timer);
    QSIM_HIPCHK(hipMemcpyAsync(value, s->d_result, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (!w) {  // the value alone
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
        return nullptr;
    }
    QSIM_HIPCHK(hipMemcpyAsync(w->phi, s->d, sizeof(double2) << n, hipMemcpyDeviceToDevice, s->stream));
    launch_pauli_apply(s->d, w->lam, n, lower_pauli_apply(n, terms, nterms, perm), w->terms, s->stream, &s->timer);
    return w;
}

}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_gate_inverse(const qsim_gate* g, qsim_gate* out) {
    return guarded([&] {
        QSIM_REQUIRE(g && out, QSIM_ERR_INVALID_ARGUMENT, "null gate");
        if (g->type < 0 || g->type >= QSIM_GATE_COUNT)
            fail(QSIM_ERR_RUNTIME, "Unknown gate type " + std::to_string(g->type));
        *out = gate_inverse(*g);
    });
}

int qsim_gradient_plan(int n_qubits, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                       size_t nterms, int* n_params, int* n_segments, int* apply_passes) {
    return guarded([&] {
        QSIM_REQUIRE(n_params && n_segments && apply_passes, QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        check_gradient_args(n_qubits, gates, count, terms, nterms);
        int params = 0, segments = 0;
        bool in_segment = false;
        for (size_t k = 0; k < count; ++k) {
            if (gate_is_parameterised(gates[k].type)) {
                ++params;
                in_segment = false;
            } else if (params > 0 && !in_segment) {  // (gates before the first parameter are never undone)
                ++segments;
                in_segment = true;
            }
        }
        *n_params = params;
        *n_segments = segments;
        *apply_passes = (int)lower_pauli_apply(n_qubits, terms, nterms, nullptr).launches;
    });
}

int qsim_state_apply_pauli_sum(qsim_state* src, qsim_state* dst, const qsim_pauli_term* terms, size_t count) {
    return guarded([&] {
        check_state(src);
        check_state(dst);
        QSIM_REQUIRE(terms || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        if (src == dst) fail(QSIM_ERR_INVALID_ARGUMENT, "the Pauli sum is applied out of place: src == dst");
        if (src->n != dst->n) fail(QSIM_ERR_INVALID_ARGUMENT, "states have different qubit counts");
        if (src->device != dst->device) fail(QSIM_ERR_INVALID_ARGUMENT, "states live on different devices");
        DeviceGuard dg(src->device);
        share_flush(src);
        // (a handed-out device pointer always sees the identity layout)
        if (dst->pinned) prep(src, false);
        const ExpectPlan plan =
            lower_pauli_apply(src->n, terms, count, src->perm.empty() ? nullptr : src->perm.data());
        drop_layout(dst);
        dst->perm = src->perm;
        QSIM_HIPCHK(hipStreamSynchronize(src->stream));  // src's writes done; dst's stream orders the rest
        launch_pauli_apply(src->d, dst->d, src->n, plan, dst->expect_terms, dst->stream, &dst->timer);
        QSIM_HIPCHK(hipStreamSynchronize(dst->stream));
    });
}

int qsim_state_inner_product(qsim_state* a, qsim_state* b, double out[2]) {
    return guarded([&] {
        check_state(a);
        check_state(b);
        QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (a->n != b->n) fail(QSIM_ERR_INVALID_ARGUMENT, "states have different qubit counts");
        if (a->device != b->device) fail(QSIM_ERR_INVALID_ARGUMENT, "states live on different devices");
        DeviceGuard dg(a->device);
        share_flush(a);
        share_flush(b);
        if (a->perm != b->perm) {  // one common layout: the identity
            prep(a, false);
            prep(b, false);
        }
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));  // b's writes done; a's stream orders the rest
        double* d_out = (double*)a->scratch.get(2 * sizeof(double), a->stream);
        launch_braket(a->d, b->d, a->n, Generator{}, a->d_partials, d_out, d_out + 1, a->stream, &a->timer);
        QSIM_HIPCHK(hipMemcpyAsync(out, d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, a->stream));
        QSIM_HIPCHK(hipStreamSynchronize(a->stream));
    });
}

int qsim_state_gradient_release(qsim_state* s) {
    return guarded([&] {
        check_state(s);
        if (!s->grad) return;
        DeviceGuard dg(s->device);
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
        s->grad.reset();
    });
}

int qsim_state_gradient(qsim_state* s, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                        size_t nterms, int flags, double* value, double* grad) {
    int rc = guarded([&] {
        check_state(s);
        QSIM_REQUIRE(value, QSIM_ERR_INVALID_ARGUMENT, "null value");
        QSIM_REQUIRE(grad || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gradient");
        check_gradient_args(s->n, gates, count, terms, nterms);
        DeviceGuard dg(s->device);
        share_flush(s);
    });
    if (rc != QSIM_OK) return rc;
    // (the sweep below reads the state this run leaves: it runs its own plan whole)
    struct ShareBlock {
        qsim_state* s;
        explicit ShareBlock(qsim_state* st) : s(st) { s->share_block = true; }
        ~ShareBlock() { s->share_block = false; }
    } share_block(s);
    // The forward run is qsim_run itself: the state ends exactly as a plain run leaves it, and
    // nothing below writes to it.
    if (count > 0 && (rc = qsim_run(s, gates, count, flags)) != QSIM_OK) return rc;
    return guarded([&] {
        DeviceGuard dg(s->device);
        const int n = s->n;
        size_t first_param = count;
        for (size_t k = count; k-- > 0;)
            if (gate_is_parameterised(gates[k].type)) first_param = k;
        GradWork* wp = gradient_prologue(s, terms, nterms, count, first_param < count, value, grad);
        if (!wp) return;  // H = 0, or no parameter: the value alone
        GradWork& w = *wp;
        QSIM_HIPCHK(hipMemsetAsync(w.d_out, 0, count * sizeof(double), s->stream));
        const int th = state_tile_height(s);
        const TileHeightScope tile_h(th, tile_rb_for(n, th));  // the segments' plans
        const bool fused_step = adjoint_fused_on();
        std::vector<Op> seg;
        for (size_t k = count; k-- > first_param;) {
            const qsim_gate inv_gate = map_gate(s, gate_inverse(gates[k]));
            Op inv = lower_gate(inv_gate, n);
            if (!gate_is_parameterised(gates[k].type)) {
                inv.src = (int)seg.size();
                seg.push_back(inv);
                continue;
            }
            grad_apply_segment(s, w, seg, flags);
            seg.clear();
            const Generator gen = gate_generator(inv_gate);  // (physical positions)
            if (k == first_param) {  // nothing is left to differentiate: no un-apply
                launch_braket(w.lam, w.phi, n, gen, s->d_partials, nullptr, w.d_out + k, s->stream, &s->timer);
            } else if (fused_step) {
                launch_adjoint_step(w.phi, w.lam, n, gen, inv, s->d_partials, w.d_out + k, s->stream, &s->timer);
            } else {
                launch_braket(w.lam, w.phi, n, gen, s->d_partials, nullptr, w.d_out + k, s->stream, &s->timer);
                launch_op(w.phi, n, 1, inv, s->stream, &s->timer);
                launch_op(w.lam, n, 1, inv, s->stream, &s->timer);
            }
        }
        QSIM_HIPCHK(hipMemcpyAsync(grad, w.d_out, count * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

}  // extern "C"
