// batch_adjoint.hip — the backward sweep of adjoint-method gradients over the B members of a
// batched parameter sweep (qsim_batch_gradient_sweep, batched.hip): member t holds its own angle
// set, so every member differentiates its own circuit.
//
// The recurrence is adjoint.hip's, per member: phi = the member's state after the sweep,
// lambda = H phi, and walking the gate list backwards, at the parameterised gate of slot j
//     grad[t, j] = Im <lambda_t| G |phi_t>,   then (phi_t, lambda_t) <- U(theta_tj)^† (phi_t, lambda_t).
// One launch covers all members (batch_adjoint_step; batch_braket at the first parameterised gate,
// where nothing is left to un-apply).  Member t's U^† is derived in the kernel from the FORWARD
// coefficients the sweep uploaded (coef[t * 8], Op::m layout): for the general 2x2
// m0' = conj m0, m1' = conj m2, m2' = conj m1, m3' = conj m3, for the diagonal d' = conj d — no
// second table exists on this path.
//
// Access pattern: batch_sweep.hip's, not the strided pairs of the single-state k_adjoint_step.  The
// member is the work-group's position (work-groups never straddle members; its eight coefficients
// are one uniform load), the low six index bits are the lanes, so every global access of a wave is
// a contiguous 1 KiB run:
//   * 2x2, target < 6 ("lane"): a thread owns one amplitude of phi and one of lambda, the partners
//     arrive by shfl_xor;
//   * 2x2, target >= 6 ("slice"): a thread owns one pair of each;
//   * diagonal (Rz / CRZ: G = Z needs no partner either): a thread owns one amplitude of each.
// A control is a per-lane predicate: lanes outside control == 1 neither load nor store and add
// nothing to the sum.  n < 6 leaves surplus lanes idle; they still take part in the shuffles.
// Sums are added per member in a fixed order — wave, work-group (block_sum), then the member's
// work-groups (launch_sum_partials, one row per member) — so out[member] is bitwise reproducible
// and does not depend on the other members' angles.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"

namespace qsim_hip {

namespace {

constexpr int kLaneU = 4;   // amplitudes of each work state per thread (lane, diagonal): 8 loads in flight
constexpr int kSliceU = 2;  // pairs of each work state per thread (slice): 8 loads in flight

struct BaArgs {
    double2* phi;
    double2* lam;
    const double* coef;  // [batch][8], the forward gate (read only with APPLY)
    double* partials;    // [batch << log_bpm]
    uint64_t cmask;
    uint64_t items;      // per member: amplitudes (lane, diagonal) or pairs (slice)
    int n, t0;
    int log_bpm;         // work-groups per member (a power of two)
};

template <int U>
__device__ __forceinline__ uint64_t ba_member(const BaArgs& a, uint64_t& first) {
    const uint64_t b = blockIdx.x;
    first = (b & ((1ull << a.log_bpm) - 1ull)) * (256ull * U) + threadIdx.x;
    return b >> a.log_bpm;
}

__device__ __forceinline__ double2 conj2(double2 v) { return make_double2(v.x, -v.y); }

// Im(conj(l) g)  (explicit fma: which product is rounded on its own is otherwise the compiler's
// choice, and the gradients' last bit with it)
__device__ __forceinline__ double im_cj(double2 l, double2 g) { return fma(l.x, g.y, -(l.y * g.x)); }

// (G b) on the side with target bit `bit`: self / other are b there and at the partner index.
template <int PAULI>
__device__ __forceinline__ double2 gen_half(int bit, double2 self, double2 other) {
    if (PAULI == 1) return other;
    if (PAULI == 2)  // Y|0> = i|1>, Y|1> = -i|0>
        return bit ? make_double2(-other.y, other.x) : make_double2(other.y, -other.x);
    return bit ? make_double2(-self.x, -self.y) : self;
}

template <int PAULI, bool APPLY>
__global__ __launch_bounds__(256) void k_ba_lane(BaArgs a) {
    __shared__ double wim[4];
    uint64_t first;
    const uint64_t member = ba_member<kLaneU>(a, first);
    double2 u0, u1, u2, u3;  // U^† of this member
    if (APPLY) {
        const double* c = a.coef + 8ull * member;  // uniform
        u0 = conj2(make_double2(ldc(c, 0), ldc(c, 1)));
        u2 = conj2(make_double2(ldc(c, 2), ldc(c, 3)));
        u1 = conj2(make_double2(ldc(c, 4), ldc(c, 5)));
        u3 = conj2(make_double2(ldc(c, 6), ldc(c, 7)));
    }
    double2* const phi = a.phi + (member << a.n);
    double2* const lam = a.lam + (member << a.n);
    double2 p[kLaneU], l[kLaneU];
    bool ok[kLaneU];
#pragma unroll
    for (int u = 0; u < kLaneU; ++u) {
        const uint64_t i = first + 256ull * u;
        ok[u] = i < a.items && (i & a.cmask) == a.cmask;  // (the partner shares the control bits)
        p[u] = l[u] = make_double2(0.0, 0.0);
        if (ok[u]) {
            p[u] = phi[i];
            l[u] = lam[i];
        }
    }
    const int tm = 1 << a.t0;
    const int bit = (int)((threadIdx.x >> a.t0) & 1u);  // (256 | work-group base: lane bits = index bits)
    double im = 0.0;
#pragma unroll
    for (int u = 0; u < kLaneU; ++u) {
        const double2 po = shfl_xor2(p[u], tm);  // every lane takes part
        if (ok[u]) im += im_cj(l[u], gen_half<PAULI>(bit, p[u], po));
        if (APPLY) {
            const double2 lo = shfl_xor2(l[u], tm);
            if (ok[u]) {
                const uint64_t i = first + 256ull * u;
                phi[i] = m1_half(S_GEN, u0, u1, u2, u3, bit, p[u], po);
                lam[i] = m1_half(S_GEN, u0, u1, u2, u3, bit, l[u], lo);
            }
        }
    }
    im = block_sum(im, wim);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = im;
}

template <int PAULI, bool APPLY>
__global__ __launch_bounds__(256) void k_ba_slice(BaArgs a) {
    __shared__ double wim[4];
    uint64_t first;
    const uint64_t member = ba_member<kSliceU>(a, first);
    double2 u0, u1, u2, u3;
    if (APPLY) {
        const double* c = a.coef + 8ull * member;
        u0 = conj2(make_double2(ldc(c, 0), ldc(c, 1)));
        u2 = conj2(make_double2(ldc(c, 2), ldc(c, 3)));
        u1 = conj2(make_double2(ldc(c, 4), ldc(c, 5)));
        u3 = conj2(make_double2(ldc(c, 6), ldc(c, 7)));
    }
    double2* const phi = a.phi + (member << a.n);
    double2* const lam = a.lam + (member << a.n);
    const uint64_t tb = 1ull << a.t0, lo_mask = tb - 1ull;
    double2 p0[kSliceU], p1[kSliceU], l0[kSliceU], l1[kSliceU];
    uint64_t i0[kSliceU];
    bool ok[kSliceU];
#pragma unroll
    for (int u = 0; u < kSliceU; ++u) {
        const uint64_t k = first + 256ull * u;
        const uint64_t lo = k & lo_mask;
        i0[u] = ((k ^ lo) << 1) | lo;  // target bit 0
        ok[u] = k < a.items && (i0[u] & a.cmask) == a.cmask;
        if (ok[u]) {
            p0[u] = phi[i0[u]];
            p1[u] = phi[i0[u] | tb];
            l0[u] = lam[i0[u]];
            l1[u] = lam[i0[u] | tb];
        }
    }
    double im = 0.0;
#pragma unroll
    for (int u = 0; u < kSliceU; ++u) {
        if (ok[u]) {
            im += im_cj(l0[u], gen_half<PAULI>(0, p0[u], p1[u])) + im_cj(l1[u], gen_half<PAULI>(1, p1[u], p0[u]));
            if (APPLY) {
                m1_pair(S_GEN, u0, u1, u2, u3, p0[u], p1[u]);
                m1_pair(S_GEN, u0, u1, u2, u3, l0[u], l1[u]);
                phi[i0[u]] = p0[u];
                phi[i0[u] | tb] = p1[u];
                lam[i0[u]] = l0[u];
                lam[i0[u] | tb] = l1[u];
            }
        }
    }
    im = block_sum(im, wim);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = im;
}

// G = Z and U^† = diag(conj d0, conj d1): no partner.
template <bool APPLY>
__global__ __launch_bounds__(256) void k_ba_diag(BaArgs a) {
    __shared__ double wim[4];
    uint64_t first;
    const uint64_t member = ba_member<kLaneU>(a, first);
    double2 d0, d1;
    if (APPLY) {
        const double* c = a.coef + 8ull * member;
        d0 = conj2(make_double2(ldc(c, 0), ldc(c, 1)));
        d1 = conj2(make_double2(ldc(c, 2), ldc(c, 3)));
    }
    double2* const phi = a.phi + (member << a.n);
    double2* const lam = a.lam + (member << a.n);
    double2 p[kLaneU], l[kLaneU];
    bool ok[kLaneU];
#pragma unroll
    for (int u = 0; u < kLaneU; ++u) {
        const uint64_t i = first + 256ull * u;
        ok[u] = i < a.items && (i & a.cmask) == a.cmask;
        if (ok[u]) {
            p[u] = phi[i];
            l[u] = lam[i];
        }
    }
    double im = 0.0;
#pragma unroll
    for (int u = 0; u < kLaneU; ++u) {
        if (ok[u]) {
            const uint64_t i = first + 256ull * u;
            const int bit = (int)((i >> a.t0) & 1ull);
            im += im_cj(l[u], gen_half<3>(bit, p[u], p[u]));
            if (APPLY) {
                const double2 d = bit ? d1 : d0;
                phi[i] = cmul(d, p[u]);
                lam[i] = cmul(d, l[u]);
            }
        }
    }
    im = block_sum(im, wim);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = im;
}

// dst[t] = the coefficients of member t's U^† in Op::m layout, from the forward ones at src[t]
// (the table of the cross-check path, QSIM_ADJOINT_FUSED=0).
__global__ __launch_bounds__(256) void k_ba_conj_table(const double* src, double* dst, uint64_t batch, int diag) {
    const uint64_t t = (uint64_t)blockIdx.x * 256ull + threadIdx.x;
    if (t >= batch) return;
    const double* c = src + 8ull * t;
    double* o = dst + 8ull * t;
    const int from[4] = {0, diag ? 1 : 2, diag ? 2 : 1, 3};  // the transpose swaps m1 and m2
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[2 * k] = c[2 * from[k]];
        o[2 * k + 1] = -c[2 * from[k] + 1];
    }
}

template <bool APPLY>
void ba_dispatch(int pauli, int kind, bool slice, unsigned blocks, const BaArgs& a, hipStream_t s) {
    if (kind == K_DIAG) hipLaunchKernelGGL(k_ba_diag<APPLY>, dim3(blocks), dim3(256), 0, s, a);
    else if (slice && pauli == 1) hipLaunchKernelGGL((k_ba_slice<1, APPLY>), dim3(blocks), dim3(256), 0, s, a);
    else if (slice) hipLaunchKernelGGL((k_ba_slice<2, APPLY>), dim3(blocks), dim3(256), 0, s, a);
    else if (pauli == 1) hipLaunchKernelGGL((k_ba_lane<1, APPLY>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_ba_lane<2, APPLY>), dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

size_t batch_adjoint_partials(int n, uint64_t batch) { return (size_t)(batch << (n > 10 ? n - 10 : 0)); }

void launch_batch_adjoint_step(double2* phi, double2* lam, int n, uint64_t batch, const Generator& g, int kind,
                               const double* coef, bool apply, double* d_partials, double* d_out, hipStream_t s,
                               Timer* tm) {
    if (n < 1 || g.t < 0 || g.t >= n || g.c >= n || g.c == g.t) fail(QSIM_ERR_INVALID_ARGUMENT, "bad generator qubits");
    // Rz / CRZ lower to the diagonal and generate Z; Rx / Ry / CRY to the 2x2 and generate X / Y
    if (!((kind == K_DIAG && g.pauli == 3) || (kind == K_M1 && (g.pauli == 1 || g.pauli == 2))))
        fail(QSIM_ERR_INVALID_ARGUMENT, "bad generator");
    if (apply && !coef) fail(QSIM_ERR_RUNTIME, "a batched adjoint step needs the sweep's table");
    const bool slice = kind == K_M1 && g.t >= 6;
    BaArgs a{};
    a.phi = phi;
    a.lam = lam;
    a.coef = coef;
    a.partials = d_partials;
    a.cmask = g.c >= 0 ? 1ull << g.c : 0ull;
    a.n = n;
    a.t0 = g.t;
    a.items = slice ? 1ull << (n - 1) : 1ull << n;
    const uint64_t per_block = 256ull * (slice ? kSliceU : kLaneU);
    a.log_bpm = 0;
    while ((per_block << a.log_bpm) < a.items) ++a.log_bpm;
    const uint64_t blocks = batch << a.log_bpm;
    if (blocks == 0 || blocks > 0x7fffffffull || batch > 0x7fffffffull) fail(QSIM_ERR_RUNTIME, "sweep grid too large");
    if (blocks > batch_adjoint_partials(n, batch)) fail(QSIM_ERR_RUNTIME, "partial sums of a batched adjoint step");
    {
        const double pairs = std::ldexp((double)batch, n - (g.c >= 0 ? 2 : 1));
        TimedLaunch tl(tm, apply ? "batch_adjoint_step" : "batch_braket", (apply ? 128.0 : 64.0) * pairs, s);
        if (apply) ba_dispatch<true>(g.pauli, kind, slice, (unsigned)blocks, a, s);
        else ba_dispatch<false>(g.pauli, kind, slice, (unsigned)blocks, a, s);
        QSIM_HIPCHK(hipGetLastError());
    }
    launch_sum_partials(d_partials, 1 << a.log_bpm, (unsigned)batch, d_out, false, s);
}

BatchGradWork::~BatchGradWork() {
    for (void* p : {(void*)phi, (void*)lam, (void*)d_out, (void*)d_partials, (void*)d_conj})
        if (p) (void)hipFree(p);
}

BatchGradWork& batch_grad_ensure(std::unique_ptr<BatchGradWork>& slot, int n, uint64_t batch, size_t n_slots,
                                 hipStream_t s) {
    if (!slot) slot = std::make_unique<BatchGradWork>();
    BatchGradWork& w = *slot;
    auto grab = [&](void** p, size_t b) {
        if (*p) return;
        if (hipMalloc(p, b) != hipSuccess) {
            (void)hipGetLastError();  // (clear the sticky error: the members themselves are intact)
            *p = nullptr;
            slot.reset();
            fail(QSIM_ERR_DEVICE, "out of device memory for the gradient work ensembles");
        }
    };
    const size_t bytes = ((size_t)batch * sizeof(double2)) << n;
    grab((void**)&w.phi, bytes);
    grab((void**)&w.lam, bytes);
    grab((void**)&w.d_partials, batch_adjoint_partials(n, batch) * sizeof(double));
    grab((void**)&w.d_conj, 8 * (size_t)batch * sizeof(double));
    const size_t outs = n_slots * (size_t)batch;
    if (outs > w.out_cap) {
        if (w.d_out) {
            QSIM_HIPCHK(hipStreamSynchronize(s));
            (void)hipFree(w.d_out);
            w.d_out = nullptr;
            w.out_cap = 0;
        }
        const size_t cap = std::max<size_t>(outs, 256);
        grab((void**)&w.d_out, cap * sizeof(double));
        w.out_cap = cap;
    }
    return w;
}

// Inverted non-parameterised gates (execution order) on both work ensembles.
static void batch_grad_segment(BatchGradWork& w, int n, uint64_t batch, const std::vector<Op>& seg, bool fused,
                               hipStream_t s, Timer* tm) {
    if (seg.empty()) return;
    if (!fused) {
        for (const Op& op : seg) {
            launch_op(w.phi, n, batch, op, s, tm);
            launch_op(w.lam, n, batch, op, s, tm);
        }
        return;
    }
    const CtrlOutOff ctrl_off;  // (every control is a tile bit, as in the members' own passes)
    const Plan& plan = w.plans.get(seg, n, s).plan;
    w.ops.upload(plan.ops.data(), plan.ops.size() * sizeof(TileOp), s);
    w.stages.upload(plan.stages.data(), plan.stages.size() * sizeof(Stage), s);
    for (double2* buf : {w.phi, w.lam}) {
        double2* r = launch_fused(buf, n, batch, plan, (const TileOp*)w.ops.ptr, (const Stage*)w.stages.ptr, s, tm);
        if (r != buf) fail(QSIM_ERR_RUNTIME, "a gradient segment planned a relayout pass");
    }
}

void batch_adjoint_sweep(BatchGradWork& w, int n, uint64_t batch, const std::vector<BatchBackStep>& steps,
                         const double* d_tab, bool fused_segments, hipStream_t s, Timer* tm) {
    const bool fused_step = adjoint_fused_on();
    std::vector<Op> seg;
    for (size_t i = 0; i < steps.size(); ++i) {
        const BatchBackStep& st = steps[i];
        if (st.pauli == 0) {
            seg.push_back(st.op);
            continue;
        }
        batch_grad_segment(w, n, batch, seg, fused_segments, s, tm);
        seg.clear();
        const Op& op = st.op;
        if (op.src < 0 || (size_t)(op.src + 1) * batch > w.out_cap || __builtin_popcountll(op.cmask) > 1)
            fail(QSIM_ERR_RUNTIME, "bad slot of a batched adjoint step");
        Generator gen;
        gen.pauli = st.pauli;
        gen.t = op.t0;
        gen.c = op.cmask ? __builtin_ctzll(op.cmask) : -1;
        const double* coef = d_tab + 8 * (size_t)batch * (size_t)op.src;
        double* out = w.d_out + (size_t)op.src * batch;
        const bool last = i + 1 == steps.size();  // nothing is left to differentiate: no un-apply
        launch_batch_adjoint_step(w.phi, w.lam, n, batch, gen, op.kind, coef, !last && fused_step, w.d_partials, out,
                                  s, tm);
        if (last || fused_step) continue;
        hipLaunchKernelGGL(k_ba_conj_table, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, coef, w.d_conj, batch,
                           op.kind == K_DIAG ? 1 : 0);
        QSIM_HIPCHK(hipGetLastError());
        launch_sweep_op(w.phi, n, batch, op, w.d_conj, s, tm);
        launch_sweep_op(w.lam, n, batch, op, w.d_conj, s, tm);
    }
    if (!seg.empty()) fail(QSIM_ERR_RUNTIME, "a backward sweep ends at a parameterised gate");
}

}  // namespace qsim_hip
