// batch_sweep.hip — per-gate kernels of a batched parameter sweep (qsim_batch_run_sweep,
// batched.hip): one circuit, one angle set per member of a BatchedSimulator.
//
// A parameterised gate (Rx, Ry, Rz, CRY, CRZ) is one launch over all B members; member t applies
// the general 2x2 (K_M1) or the general diagonal (K_DIAG) whose eight coefficients (Op::m layout,
// lowered on the host by lower_gate) sit at coef[t * 8].  The member is the work-group's position
// (work-groups never straddle two members), so the coefficients are one uniform scalar load per
// work-group.  Used where the fused tile passes are not: n < 10, QSIM_BATCH_PER_GATE,
// QSIM_BATCH_FUSED=0.
//
// Access pattern (as the per-gate kernels of gates.hip): the low six index bits are the 64 lanes,
// so every global access of a wave is one contiguous 1 KiB run of 16-B amplitudes.
//   * target < 6 ("lane"): a thread owns one amplitude, its partner sits in lane ^ (1 << t) of the
//     same wave and arrives by shuffle — never a strided 16-B access per lane;
//   * target >= 6 ("slice"): a thread owns one pair, the wave reads the 1 KiB run with the target
//     bit 0 and the run with it 1;
//   * diagonal: a thread owns one amplitude, no partner.
// Controls (any mask) are a per-lane predicate on the index: lanes outside the control == 1
// subspace neither load nor store.  States smaller than a wave (n < 6) leave the surplus lanes
// idle; they still take part in the shuffle, whose partners all lie below 2^n.
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_ops.hpp"
#include "engine.hpp"

namespace qsim_hip {

namespace {

constexpr int kSweepU = 4;                        // items per thread
constexpr uint64_t kSweepBlock = 256 * kSweepU;   // items per work-group

struct SwArgs {
    double2* st;
    const double* coef;  // [batch][8]
    uint64_t cmask;
    uint64_t items;      // per member: amplitudes (lane, diagonal) or pairs (slice)
    int n, t0;
    int log_bpm;         // work-groups per member (a power of two)
};

__device__ __forceinline__ uint64_t sweep_member(const SwArgs& a, uint64_t& first) {
    const uint64_t b = blockIdx.x;
    first = (b & ((1ull << a.log_bpm) - 1ull)) * kSweepBlock + threadIdx.x;
    return b >> a.log_bpm;
}

__global__ __launch_bounds__(256) void k_sweep_m1_lane(SwArgs a) {
    uint64_t first;
    const uint64_t member = sweep_member(a, first);
    const double* c = a.coef + 8ull * member;  // uniform
    const double2 m0 = make_double2(ldc(c, 0), ldc(c, 1)), m1 = make_double2(ldc(c, 2), ldc(c, 3));
    const double2 m2 = make_double2(ldc(c, 4), ldc(c, 5)), m3 = make_double2(ldc(c, 6), ldc(c, 7));
    double2* const st = a.st + (member << a.n);
    double2 v[kSweepU];
    bool ok[kSweepU];
#pragma unroll
    for (int u = 0; u < kSweepU; ++u) {
        const uint64_t i = first + 256ull * u;
        ok[u] = i < a.items && (i & a.cmask) == a.cmask;  // (the partner shares the control bits)
        v[u] = make_double2(0.0, 0.0);
        if (ok[u]) v[u] = st[i];
    }
    const int tm = 1 << a.t0;
    const int bit = (int)((threadIdx.x >> a.t0) & 1u);  // (256 | work-group base: lane bits = index bits)
#pragma unroll
    for (int u = 0; u < kSweepU; ++u) {
        const double2 p = shfl_xor2(v[u], tm);  // every lane takes part
        if (ok[u]) st[first + 256ull * u] = m1_half(S_GEN, m0, m1, m2, m3, bit, v[u], p);
    }
}

__global__ __launch_bounds__(256) void k_sweep_m1_slice(SwArgs a) {
    uint64_t first;
    const uint64_t member = sweep_member(a, first);
    const double* c = a.coef + 8ull * member;
    const double2 m0 = make_double2(ldc(c, 0), ldc(c, 1)), m1 = make_double2(ldc(c, 2), ldc(c, 3));
    const double2 m2 = make_double2(ldc(c, 4), ldc(c, 5)), m3 = make_double2(ldc(c, 6), ldc(c, 7));
    double2* const st = a.st + (member << a.n);
    const uint64_t tb = 1ull << a.t0, lo_mask = tb - 1ull;
    double2 v0[kSweepU], v1[kSweepU];
    uint64_t i0[kSweepU];
    bool ok[kSweepU];
#pragma unroll
    for (int u = 0; u < kSweepU; ++u) {
        const uint64_t p = first + 256ull * u;
        const uint64_t lo = p & lo_mask;
        i0[u] = ((p ^ lo) << 1) | lo;  // target bit 0
        ok[u] = p < a.items && (i0[u] & a.cmask) == a.cmask;
        if (ok[u]) {
            v0[u] = st[i0[u]];
            v1[u] = st[i0[u] | tb];
        }
    }
#pragma unroll
    for (int u = 0; u < kSweepU; ++u) {
        if (ok[u]) {
            m1_pair(S_GEN, m0, m1, m2, m3, v0[u], v1[u]);
            st[i0[u]] = v0[u];
            st[i0[u] | tb] = v1[u];
        }
    }
}

__global__ __launch_bounds__(256) void k_sweep_diag(SwArgs a) {
    uint64_t first;
    const uint64_t member = sweep_member(a, first);
    const double* c = a.coef + 8ull * member;
    const double2 d0 = make_double2(ldc(c, 0), ldc(c, 1)), d1 = make_double2(ldc(c, 2), ldc(c, 3));
    double2* const st = a.st + (member << a.n);
    double2 v[kSweepU];
    bool ok[kSweepU];
#pragma unroll
    for (int u = 0; u < kSweepU; ++u) {
        const uint64_t i = first + 256ull * u;
        ok[u] = i < a.items && (i & a.cmask) == a.cmask;
        if (ok[u]) v[u] = st[i];
    }
#pragma unroll
    for (int u = 0; u < kSweepU; ++u) {
        const uint64_t i = first + 256ull * u;
        if (ok[u]) st[i] = cmul(((i >> a.t0) & 1ull) ? d1 : d0, v[u]);
    }
}

}  // namespace

void launch_sweep_op(double2* st, int n, uint64_t batch, const Op& op, const double* coef, hipStream_t s, Timer* tm) {
    if (op.kind != K_M1 && op.kind != K_DIAG) fail(QSIM_ERR_RUNTIME, "sweep op must be a 2x2 or a diagonal");
    if (n < 1 || op.t0 < 0 || op.t0 >= n || (op.cmask >> n) != 0 || ((op.cmask >> op.t0) & 1ull))
        fail(QSIM_ERR_RUNTIME, "sweep op out of range");
    const bool slice = op.kind == K_M1 && op.t0 >= 6;
    SwArgs a{};
    a.st = st;
    a.coef = coef;
    a.cmask = op.cmask;
    a.n = n;
    a.t0 = op.t0;
    a.items = slice ? 1ull << (n - 1) : 1ull << n;
    a.log_bpm = 0;
    while ((kSweepBlock << a.log_bpm) < a.items) ++a.log_bpm;
    const uint64_t blocks = batch << a.log_bpm;
    if (blocks == 0 || blocks > 0x7fffffffull) fail(QSIM_ERR_RUNTIME, "sweep grid too large");
    TimedLaunch tl(tm, op.kind == K_DIAG ? "sweep_diag" : "sweep_m1", op_alg_bytes(op, std::ldexp((double)batch, n)), s);
    if (op.kind == K_DIAG) hipLaunchKernelGGL(k_sweep_diag, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else if (slice) hipLaunchKernelGGL(k_sweep_m1_slice, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_sweep_m1_lane, dim3((unsigned)blocks), dim3(256), 0, s, a);
    QSIM_HIPCHK(hipGetLastError());
}

}  // namespace qsim_hip
