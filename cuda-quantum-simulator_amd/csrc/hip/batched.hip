// batched.hip — B independent trajectories of 2^n amplitudes (reference BatchedSimulator,
// include/NoiseModel.cuh:231-297, src/NoiseModel.cu:653-972) with Monte-Carlo Pauli noise.
//
// Layout: trajectory-major [B][2^n] like the reference (d_states_, NoiseModel.cu:657-673), so
// each gate is the single-state kernel with a batch dimension (launch_op(..., batch, ...)).
//
// Noise (deliberate redesign): the reference draws one curand number per amplitude
// PAIR and keeps a 48-B curandState per pair (1.5 GiB at 16q x 1024).  Here each trajectory
// draws once per channel per gate from a stateless counter hash keyed by (seed, step, channel,
// trajectory); the Pauli picks of all channels of one gate are composed into one Pauli string
// i^e X^x Z^z per trajectory, and only trajectories whose string is not the identity are
// touched (one read+write of that trajectory).  This is the physical depolarizing channel on a
// pure-state trajectory; statistics, not per-trajectory realizations, match the reference.
// Channel types the reference batched mode ignores (F5: only Depolarizing) are Pauli-free here
// too: BitFlip/PhaseFlip/BitPhaseFlip are applied (X/Z/Y), damping channels are ignored.
//
// qsim_batch_run validates, decides the path and lowers; the paths are run_reference_noise (the
// reference's per-pair process: run_pulled, run_tile with split_tile_run, or step by step — the
// schedules and their side kit, NoiseSide, are noise.hip's), run_frames (fused passes under Pauli
// frames) and run_per_gate.  Every fused run — those, a sweep's, canonicalize's SWAP network —
// goes through run_planned.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"
#include "qsim_hip.h"

using namespace qsim_hip;

namespace qsim_hip {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// uniform double in [0,1) from 53 bits
__device__ __forceinline__ double u01(uint64_t h) { return (double)(h >> 11) * 0x1.0p-53; }

struct DevChannel {
    int type;
    int qubit;
    double p;
};

// This step's Pauli picks of trajectory b, composed into i^e X^x Z^z (channels in order).
// b is the GLOBAL trajectory index (qsim_batch_set_trajectory_offset): a sharded ensemble draws
// exactly what one object holding every trajectory draws.
__device__ __forceinline__ void draw_step(const DevChannel* ch, int nch, uint64_t seed, uint64_t step,
                                          uint64_t b, uint64_t& x, uint64_t& z, int& e) {
    x = 0;
    z = 0;
    e = 0;
    for (int c = 0; c < nch; ++c) {
        const uint64_t key = mix64(seed ^ mix64(step * 0x100000001b3ull + (uint64_t)c) ^
                                   (b << 20));
        const double r1 = u01(mix64(key));
        int pauli = 0;  // 1 X, 2 Y, 3 Z
        const int t = ch[c].type;
        if (r1 < ch[c].p) {
            if (t == 0) {  // depolarizing: uniform X/Y/Z (reference thresholds 1/3, 2/3)
                const double r2 = u01(mix64(key ^ 0x5bd1e995ull));
                pauli = r2 < 1.0 / 3.0 ? 1 : (r2 < 2.0 / 3.0 ? 2 : 3);
            } else if (t == 3) pauli = 1;       // bit flip
            else if (t == 4) pauli = 3;         // phase flip
            else if (t == 5) pauli = 2;         // bit-phase flip
        }
        if (!pauli) continue;
        const uint64_t q = 1ull << ch[c].qubit;
        if (pauli == 1) {
            x ^= q;
        } else if (pauli == 3) {
            if (x & q) e += 2;
            z ^= q;
        } else {  // Y = i X Z
            e += 1 + ((x & q) ? 2 : 0);
            x ^= q;
            z ^= q;
        }
    }
    e &= 3;
}

// One thread per trajectory: compose this step's Pauli picks into (e, x, z).
__global__ void k_pauli_draw(const DevChannel* ch, int nch, uint64_t seed, uint64_t step,
                             int batch, uint64_t traj0, uint64_t* xz, int* ephase) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    uint64_t x, z;
    int e;
    draw_step(ch, nch, seed, step, traj0 + (uint64_t)b, x, z, e);
    xz[2 * b] = x;
    xz[2 * b + 1] = z;
    ephase[b] = e;
}

// Pauli frames for a whole run.  With the frame Phi = i^E X^F Z^G (state = Phi * stored vector),
// the noise P = i^e X^x Z^z after step s updates Phi <- P Phi = i^(e+E) (-1)^popc(z & F)
// X^(x^F) Z^(z^G); frames[s] is the frame in force BEFORE gate s (gates are applied to the stored
// vector conjugated by it, fused.hip), fin the frame after the last step (materialised with
// k_pauli_apply).  Same draws as k_pauli_draw.  Two kernels: every (step, trajectory) draw in
// parallel (written into frames[s] as (x, z) plus ephase[s]), then one thread per trajectory
// scans the steps in order, replacing each draw by the frame before it.
__global__ void k_draw_steps(const DevChannel* ch, int nch, uint64_t seed, uint64_t step0,
                             int count, int batch, uint64_t traj0, uint64_t* frames, int* ephase) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)count * batch) return;
    const int s = (int)(i / batch), b = (int)(i - (uint64_t)s * batch);
    uint64_t x, z;
    int e;
    draw_step(ch, nch, seed, step0 + (uint64_t)s, traj0 + (uint64_t)b, x, z, e);
    frames[2 * i] = x;
    frames[2 * i + 1] = z;
    ephase[i] = e;
}

// Clifford gates move the frame instead of being conjugated by it (Pauli-frame propagation):
// for a Clifford U, U Phi = (U Phi U^dag) U, so U runs on the stored vector unchanged and the
// frame becomes U Phi U^dag — again a Pauli.  Per step: {code, q0, q1}; code 0 = not Clifford (the
// gate is conjugated by the frame in the pass kernels instead).  Rules for Phi = i^E X^F Z^G:
//   X_q: E += 2 G_q            Z_q: E += 2 F_q              Y_q: E += 2 (F_q ^ G_q)
//   H_q: swap F_q, G_q; E += 2 (F_q & G_q)
//   S_q: G_q ^= F_q; E += F_q   Sdag_q: G_q ^= F_q; E += 3 F_q
//   CNOT(c, t): F_t ^= F_c; G_c ^= G_t      CZ(a, b): G_a ^= F_b; G_b ^= F_a; E += 2 (F_a & F_b)
//   SWAP(a, b): exchange bits a and b of F and of G.
enum CliffordCode : int { CL_NONE = 0, CL_X, CL_Y, CL_Z, CL_H, CL_S, CL_SDG, CL_CNOT, CL_CZ, CL_SWAP };
struct StepClifford {
    int code, q0, q1, _pad;
};

__device__ __forceinline__ void clifford_update(const StepClifford& c, uint64_t& F, uint64_t& G, int& E) {
    const uint64_t a = 1ull << c.q0, bm = 1ull << (c.q1 < 0 ? 0 : c.q1);
    const int fa = (F & a) != 0, ga = (G & a) != 0;
    switch (c.code) {
        case CL_X: E += 2 * ga; break;
        case CL_Z: E += 2 * fa; break;
        case CL_Y: E += 2 * (fa ^ ga); break;
        case CL_H:
            E += 2 * (fa & ga);
            F = (F & ~a) | (ga ? a : 0ull);
            G = (G & ~a) | (fa ? a : 0ull);
            break;
        case CL_S: E += fa; if (fa) G ^= a; break;
        case CL_SDG: E += 3 * fa; if (fa) G ^= a; break;
        case CL_CNOT: {  // q0 control, q1 target
            if (fa) F ^= bm;
            if (G & bm) G ^= a;
            break;
        }
        case CL_CZ: {
            const int fb = (F & bm) != 0;
            E += 2 * (fa & fb);
            if (fb) G ^= a;
            if (fa) G ^= bm;
            break;
        }
        case CL_SWAP: {
            const int fb = (F & bm) != 0, gb = (G & bm) != 0;
            F = (F & ~(a | bm)) | (fb ? a : 0ull) | (fa ? bm : 0ull);
            G = (G & ~(a | bm)) | (gb ? a : 0ull) | (ga ? bm : 0ull);
            break;
        }
        default: break;
    }
}

// carry: start from the frame in fin_xz / fin_e (the last run's, not materialised) instead of 1.
__global__ void k_frame_build(int count, int batch, uint64_t* frames, const int* ephase,
                              const StepClifford* cl, uint64_t* fin_xz, int* fin_e, int carry) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    uint64_t F = carry ? fin_xz[2 * b] : 0ull, G = carry ? fin_xz[2 * b + 1] : 0ull;
    int E = carry ? fin_e[b] : 0;
    for (int s = 0; s < count; ++s) {
        const uint64_t i = (uint64_t)s * batch + b;
        uint64_t* fr = frames + 2 * i;
        const uint64_t x = fr[0], z = fr[1];
        fr[0] = F;  // the frame gate s is conjugated by (when it is not Clifford)
        fr[1] = G;
        clifford_update(cl[s], F, G, E);
        E += ephase[i] + ((__popcll(z & F) & 1) ? 2 : 0);  // then this step's noise: P Phi
        F ^= x;
        G ^= z;
    }
    fin_xz[2 * b] = F;
    fin_xz[2 * b + 1] = G;
    fin_e[b] = E & 3;
}

__device__ __forceinline__ double2 mul_ipow(double2 a, int e) {
    switch (e & 3) {
        case 1: return make_double2(-a.y, a.x);
        case 2: return make_double2(-a.x, -a.y);
        case 3: return make_double2(a.y, -a.x);
        default: return a;
    }
}

// new[j] = i^e (-1)^{popc(z & (j^x))} old[j^x]; pairs (j, j^x) with bit h of j == 0.
__global__ __launch_bounds__(256) void k_pauli_apply(double2* st, int n, const uint64_t* xz,
                                                     const int* ephase, uint64_t items_per_traj,
                                                     uint64_t batch) {
    const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b = item / items_per_traj;
    if (b >= batch) return;  // (the last block's surplus threads)
    const uint64_t k = item - b * items_per_traj;
    const uint64_t x = xz[2 * b], z = xz[2 * b + 1];
    const int e = ephase[b];
    if (x == 0 && z == 0 && e == 0) return;
    double2* s = st + (b << n);
    if (x == 0) {  // diagonal: k enumerates all 2^n amplitudes (items_per_traj == 2^(n-1)): 2 each
        for (int r = 0; r < 2; ++r) {
            const uint64_t j = 2 * k + r;
            const double2 a = s[j];
            const int sign = __popcll(z & j) & 1;
            double2 v = mul_ipow(a, e + 2 * sign);
            s[j] = v;
        }
        return;
    }
    const int h = 63 - __clzll(x);
    const uint64_t lo = k & ((1ull << h) - 1ull);
    const uint64_t j = ((k ^ lo) << 1) | lo;  // bit h == 0
    const uint64_t jp = j ^ x;
    const double2 a = s[j], ap = s[jp];
    // new[j] uses old[jp]; sign from z & (j ^ x) = z & jp
    const double2 nj = mul_ipow(ap, e + 2 * (__popcll(z & jp) & 1));
    const double2 njp = mul_ipow(a, e + 2 * (__popcll(z & j) & 1));
    s[j] = nj;
    s[jp] = njp;
}

}  // namespace qsim_hip

struct qsim_batch {
    int n = 0, batch = 0, device = 0;
    double2* d = nullptr;
    hipStream_t stream = nullptr;
    uint64_t seed = 0, step = 0;
    uint64_t traj0 = 0;     // global index of trajectory 0 (trajectory-sharded ensembles)
    uint64_t ncounter = 0;  // per-pair noise passes so far (QSIM_BATCH_REFERENCE_NOISE)
    uint64_t* d_xz = nullptr;
    int* d_e = nullptr;
    DevChannel* d_ch = nullptr;
    size_t ch_cap = 0;
    uint64_t* d_frames = nullptr;  // Pauli frames of the current run, [steps][batch][2]
    int* d_fe = nullptr;           // per-(step, trajectory) draw phases (frame build scratch)
    size_t frames_cap = 0;
    DevBuf ops, stages;             // fused-plan descriptors
    DevBuf cliff;                   // per-step Clifford codes of the current run (frame build)
    DevBuf expect_terms;            // term table of the last expectation value (expect.hip)
    // coefficient table of the last parameter sweep (qsim_batch_run_sweep): [slot][member][8]
    // doubles, grown on demand like d_frames
    DevBuf sweep_table;
    // adjoint gradients of a sweep (qsim_batch_gradient_sweep): the two work ensembles and the
    // plans of the inverted segments (null until used; qsim_batch_gradient_release drops them)
    std::unique_ptr<BatchGradWork> grad;
    PlanCache plans;
    Timer timer;
    Scratch scratch, scratch2;
    int last_passes = 0, last_jit_passes = 0;
    // Layout-aware relabeling (relabel.hip) of the qubits inside every trajectory: logical q at
    // physical perm[q] (empty: identity); basis: every trajectory is |0..0> (create / reset).
    std::vector<int> perm;
    bool basis = true;
    // The Pauli frames of the last fused noisy run (d_xz, d_e; physical positions) are not yet
    // materialised: every trajectory's state is Phi * stored vector.  The next fused run starts
    // its frame build from them (frames compose: no Pauli pass per run); everything that reads
    // or writes amplitudes otherwise materialises them first (materialize), and so does sync.
    bool frame_pending = false;
    // Pulled reference noise (noise.hip: launch_pull_noise_run) writes out of place: the
    // ensemble alternates between d0 (allocated at create) and d1 (allocated on the first pulled
    // run when the device has room; otherwise the push kernels run).  d is the current one.
    // pinned: a raw pointer to d0 was handed out, so a run that ends in d1 copies back.
    double2* d0 = nullptr;
    double2* d1 = nullptr;
    bool pinned = false;
    // The side stream, events, code words and flip lists of the pulled and in-tile runs (both
    // build one or two steps ahead of the passes that read them).
    NoiseSide noise;
    // QSIM_NOISE_SPLIT=k (default 2, at most 4): the in-tile path runs the ensemble as k trajectory
    // parts on k streams (part 0 on `stream` with `noise`), so one part's tile pass can overlap
    // another's suffix push; split[j - 1] is part j
    struct SplitPart {
        hipStream_t s = nullptr;
        hipEvent_t fork = nullptr, join = nullptr;
        NoiseSide side;
        void destroy() noexcept {
            if (s) (void)hipStreamSynchronize(s);
            side.destroy();
            for (hipEvent_t* e : {&fork, &join}) {
                if (*e) (void)hipEventDestroy(*e);
                *e = nullptr;
            }
            if (s) (void)hipStreamDestroy(s);
            s = nullptr;
        }
        ~SplitPart() { destroy(); }
    };
    SplitPart split[3];
    ~qsim_batch() {
        if (stream) (void)hipStreamSynchronize(stream);
        grad.reset();
        noise.destroy();
        if (d0) (void)hipFree(d0);
        if (d1) (void)hipFree(d1);
        for (SplitPart& p : split) p.destroy();
        if (d_xz) (void)hipFree(d_xz);
        if (d_e) (void)hipFree(d_e);
        if (d_ch) (void)hipFree(d_ch);
        if (d_frames) (void)hipFree(d_frames);
        if (d_fe) (void)hipFree(d_fe);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {
void need(const qsim_batch* b) {
    if (!b) fail(QSIM_ERR_INVALID_ARGUMENT, "null batch handle");
}
// The ensemble back in its first buffer (after a pulled run that ended in the second one).
void settle_in_d0(qsim_batch* b) {
    if (b->d == b->d0) return;
    QSIM_HIPCHK(hipMemcpyAsync(b->d0, b->d, ((uint64_t)b->batch * sizeof(double2)) << b->n,
                               hipMemcpyDeviceToDevice, b->stream));
    b->d = b->d0;
}
// The qubit count whose state has as many amplitudes as the whole ensemble (rounded up): what the
// relabeling and JIT size thresholds are applied to.
int batch_eff_qubits(const qsim_batch* b) {
    int eff = b->n;
    while ((1ll << (eff - b->n)) < (long long)b->batch) ++eff;
    return eff;
}
// QSIM_NOISE_STREAM_PRIO (experiments): 1 = the side stream at the lowest priority, so the
// list builds yield the CUs to the main stream's kernels
void ensure_side_stream(qsim_batch* b) { b->noise.ensure_stream(env_switch("QSIM_NOISE_STREAM_PRIO", false)); }
// The in-tile run over k trajectory parts on k streams (QSIM_NOISE_SPLIT, default 2): part 0 on the object's
// stream with its list sets (the caller has ensured them), part j > 0 on a stream of its own with its
// own side kit; every part draws with the global pair index, so the states are the one-part run's.
// false (nothing launched): a part's lists do not fit beside the margin NoiseSide::ensure_lists
// keeps — the caller runs the ensemble as one part instead (a near-full device must not
// turn a run that fits as one part into an error).
bool split_tile_run(qsim_batch* b, const std::vector<Op>& ops, const std::vector<NoiseChan>& dep, int k) {
    const uint64_t B = (uint64_t)b->batch;
    std::vector<uint64_t> first(k + 1);
    for (int j = 0; j <= k; ++j) first[j] = B * (uint64_t)j / (uint64_t)k;
    for (int j = 1; j < k; ++j) {  // every part's list buffers first, so a refusal launches nothing
        qsim_batch::SplitPart& p = b->split[j - 1];
        if (!p.side.ensure_lists(gate_noise_lists_bytes(b->n, first[j + 1] - first[j], dep), p.s)) return false;
    }
    std::vector<GnLists> Ls(k);
    Ls[0] = b->noise.view();
    for (int j = 1; j < k; ++j) {
        qsim_batch::SplitPart& p = b->split[j - 1];
        if (!p.s) {
            QSIM_HIPCHK(hipStreamCreateWithFlags(&p.s, hipStreamNonBlocking));
            for (hipEvent_t* e : {&p.fork, &p.join}) QSIM_HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        }
        p.side.ensure_stream(false);
        Ls[j] = p.side.view();
        QSIM_HIPCHK(hipEventRecord(p.fork, b->stream));  // (after everything before this run)
        QSIM_HIPCHK(hipStreamWaitEvent(p.s, p.fork, 0));
    }
    const uint64_t c0 = b->ncounter;
    uint64_t c_end = c0;
    for (int j = 0; j < k; ++j) {
        hipStream_t sj = j == 0 ? b->stream : b->split[j - 1].s;
        uint64_t c = c0;
        launch_gate_noise_run(b->d + (first[j] << b->n), b->n, first[j + 1] - first[j], b->traj0 + first[j], ops, dep,
                              b->seed, c, sj, &b->timer, &Ls[j]);
        c_end = c;
    }
    for (int j = 1; j < k; ++j) {
        QSIM_HIPCHK(hipEventRecord(b->split[j - 1].join, b->split[j - 1].s));
        QSIM_HIPCHK(hipStreamWaitEvent(b->stream, b->split[j - 1].join, 0));
    }
    b->ncounter = c_end;
    return true;
}
// Buffers of the pulled noise path (second ensemble buffer, two sets of code words), allocated
// when the device has room for them beside a margin; false: run the push kernels instead.
bool ensure_pull_buffers(qsim_batch* b, size_t nch) {
    const size_t state_b = ((uint64_t)b->batch * sizeof(double2)) << b->n;
    const size_t codes_b = pull_noise_codes_bytes(b->n, (uint64_t)b->batch, nch);
    const size_t need_b = (b->d1 ? 0 : state_b) + (codes_b > b->noise.codes_cap ? 2 * codes_b : 0);
    if (need_b == 0) return true;
    if (device_free_bytes() < need_b + kAltMarginBytes) return false;
    if (!b->d1 && !(b->d1 = (double2*)device_alloc_or_null(state_b))) return false;
    if (!b->noise.ensure_codes(codes_b, b->stream)) return false;
    ensure_side_stream(b);
    return true;
}
// One Pauli pass: every trajectory's string (d_xz, d_e) applied to its stored vector.
void apply_frames(qsim_batch* b) {
    const uint64_t N = 1ull << b->n;
    const uint64_t items_per_traj = N / 2 > 0 ? N / 2 : 1;
    const uint64_t total = items_per_traj * (uint64_t)b->batch;
    TimedLaunch tl(&b->timer, "pauli_apply", 0.0, b->stream);
    hipLaunchKernelGGL(k_pauli_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, b->stream, b->d, b->n,
                       b->d_xz, b->d_e, items_per_traj, (uint64_t)b->batch);
    QSIM_HIPCHK(hipGetLastError());
}
// Apply the carried Pauli frames to the stored vectors (one pass), frames back to 1.
void materialize(qsim_batch* b) {
    if (!b->frame_pending) return;
    b->frame_pending = false;
    apply_frames(b);
}
// `ops` over every member as fused tile passes, through the plan cache.  frames: the Pauli frames
// its ops with a step are conjugated by (null: none); table: a sweep's coefficient table (null:
// none) — the passes that read it run in the interpreter, so circuit-specialised kernels are
// looked up only when another pass exists and only those are counted.  counted = false (the SWAP
// network of canonicalize): no circuit-specialised kernels, and the last run's figures stay.
void run_planned(qsim_batch* b, const std::vector<Op>& ops, const uint64_t* frames, const double* table,
                 bool counted = true) {
    PlanCache::Entry& pe = b->plans.get(ops, b->n, b->stream);
    const Plan& plan = pe.plan;
    std::vector<char> tabled(plan.passes.size(), 0);
    bool any_plain = table == nullptr;
    for (size_t p = 0; table && p < plan.passes.size(); ++p) {
        tabled[p] = pass_has_step_op(plan, p);
        any_plain = any_plain || !tabled[p];
    }
    // (the JIT threshold counts the whole batch)
    const JitModule* jm = counted && any_plain ? jit_for(pe.jit, plan, batch_eff_qubits(b)) : nullptr;
    b->ops.upload(plan.ops.data(), plan.ops.size() * sizeof(TileOp), b->stream);
    b->stages.upload(plan.stages.data(), plan.stages.size() * sizeof(Stage), b->stream);
    launch_fused(b->d, b->n, (uint64_t)b->batch, plan, (const TileOp*)b->ops.ptr, (const Stage*)b->stages.ptr,
                 b->stream, &b->timer, jm, frames, FusedRange(), table);
    if (!counted) return;
    b->last_passes = (int)plan.passes.size();
    b->last_jit_passes = 0;
    if (jm)
        for (size_t p = 0; p < jm->fn.size(); ++p)
            b->last_jit_passes += jm->fn[p] != nullptr && !(p < tabled.size() && tabled[p]);
}
// The layout of the first fused run of |0..0> members: the one the model prefers for the circuit
// (lower_under: its ops under a candidate labeling), memoised per (kind, key).  The tile-control
// rule in force (CtrlOutOff) is the caller's: the choice is made and memoised under it.
void choose_first_layout(qsim_batch* b, int kind, const void* key, size_t key_bytes,
                         const std::function<std::vector<Op>(const std::vector<int>&)>& lower_under) {
    // relabel for the plan's tile layouts when the whole batch is HBM-sized
    if (!relabel_enabled(batch_eff_qubits(b))) return;
    if (layout_memo_get(b->n, kind, key, key_bytes, b->perm)) return;
    b->perm = choose_layout(b->n, lower_under, relabel_tries()).perm;
    layout_memo_put(b->n, kind, key, key_bytes, b->perm);
}
// Undo the relabeling in every trajectory (fused SWAP network over the batch, exact data
// movement) before anything reads or writes amplitudes by index; carried frames first.
void canonicalize(qsim_batch* b) {
    materialize(b);
    if (b->perm.empty()) return;
    const int n = b->n;
    std::vector<int> p = b->perm, inv(n);
    for (int q = 0; q < n; ++q) inv[p[q]] = q;
    std::vector<Op> swaps;
    for (int q = 0; q < n; ++q) {
        if (p[q] == q) continue;
        const int at = p[q], r = inv[q];
        qsim_gate g{};
        g.type = QSIM_GATE_SWAP;
        g.nqubits = 2;
        g.qubits[0] = q;
        g.qubits[1] = at;
        swaps.push_back(lower_gate(g, n));
        swaps.back().src = -1;
        p[r] = at;
        inv[at] = r;
        p[q] = q;
        inv[q] = q;
    }
    b->perm.clear();
    if (swaps.empty()) return;
    run_planned(b, swaps, nullptr, nullptr, false);
}
// ---- parameter sweeps (qsim_batch_run_sweep / qsim_batch_sweep_plan) ----
// The checks both entries share.  Returns the gate list with every parameterised gate's angle
// replaced by the placeholder — what is validated, planned and keyed, so neither the plan nor the
// qubit layout depends on the members' angles — and the slots (gate indices, list order).
std::vector<qsim_gate> sweep_arguments(int n, const qsim_gate* gates, size_t count, int flags,
                                       std::vector<size_t>& slots) {
    if (!gates && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null gate list");
    if (flags & ~QSIM_BATCH_PER_GATE)
        fail(QSIM_ERR_INVALID_ARGUMENT, "a parameter sweep takes flags 0 or QSIM_BATCH_PER_GATE");
    std::vector<qsim_gate> pg(gates, gates + count);
    slots.clear();
    for (size_t i = 0; i < count; ++i) {
        if (gate_is_parameterised(pg[i].type)) {
            pg[i].parameter = kSweepPlaceholderAngle;
            slots.push_back(i);
        }
        validate_gate(pg[i], n);
    }
    return pg;
}
bool sweep_fused_path(int n, int flags) {
    return n >= 10 && env_switch("QSIM_BATCH_FUSED", true) && !(flags & QSIM_BATCH_PER_GATE);
}
// The placeholder list lowered under `perm`; a parameterised gate's op carries its slot in src.
std::vector<Op> sweep_lower(int n, const std::vector<qsim_gate>& pg, const std::vector<int>& perm, bool slots) {
    std::vector<Op> ops = lower_gates(n, pg.data(), pg.size(), perm);
    int k = 0;
    for (size_t i = 0; i < ops.size(); ++i) ops[i].src = slots && gate_is_parameterised(pg[i].type) ? k++ : -1;
    return ops;
}
// ---- the paths of qsim_batch_run ----
// Reference noise, pulled: the noise after gate i is applied by gate i+1's pass (out of place), the
// noise after the last gate by one identity pass; same draws, same states as the push kernels.
// false: not this run (unsupported channels, or no room for the buffers): nothing launched.
bool run_pulled(qsim_batch* b, const std::vector<Op>& ops, const std::vector<NoiseChan>& dep) {
    if (!pull_noise_supported(b->n, dep, false) || !ensure_pull_buffers(b, dep.size())) return false;
    // QSIM_NOISE_MAP_OVERLAP=0: the word maps on the object's stream, one set in turn (read per run)
    const bool overlap = env_switch("QSIM_NOISE_MAP_OVERLAP", true);
    const uint64_t c0 = b->ncounter;
    b->ncounter += (uint64_t)ops.size() * dep.size();  // (one pass counter per channel entry, as the push path)
    double2* const buf[2] = {b->d0, b->d1};
    b->d = buf[launch_pull_noise_run(buf, b->d == b->d0 ? 0 : 1, b->n, (uint64_t)b->batch, b->traj0, ops, dep, b->seed,
                                     c0, b->noise, b->stream, &b->timer, overlap)];
    if (b->pinned) settle_in_d0(b);
    return true;
}
// Reference noise, in-tile (noise.hip: gate + in-tile channels in LDS per step, each step's flip
// lists built on the side stream during the step before, when the device has room for them).
// false: a gate the tile kernel does not take: nothing launched.
bool run_tile(qsim_batch* b, const std::vector<Op>& ops, const std::vector<NoiseChan>& dep) {
    bool all_tile = !ops.empty();
    for (const Op& op : ops) all_tile = all_tile && gate_noise_tile_supported(b->n, op.kind >= 0 ? &op : nullptr);
    if (!all_tile) return false;
    const size_t lb = gate_noise_lists_bytes(b->n, (uint64_t)b->batch, dep);
    GnLists L{};
    const bool lists = lb && b->noise.ensure_lists(lb, b->stream);
    if (lists) {
        ensure_side_stream(b);
        L = b->noise.view();
    }
    // two trajectory halves on two streams (QSIM_NOISE_SPLIT, read per run; default 2):
    // one half's tile pass overlaps the other's DRAM-random suffix push — W-BATCH config 4
    // 57.8 -> 54.1 ms per step (3 parts 62.5, 4 parts 58.6)
    const int k = std::max(1, std::min(4, env_int("QSIM_NOISE_SPLIT", 2)));
    if (k > 1 && b->batch >= k && lists && split_tile_run(b, ops, dep, k)) return true;
    launch_gate_noise_run(b->d, b->n, (uint64_t)b->batch, b->traj0, ops, dep, b->seed, b->ncounter, b->stream,
                          &b->timer, lists ? &L : nullptr);
    return true;
}
// The reference's process (src/NoiseModel.cu:815-892): each gate, then for every Depolarizing
// channel entry (the only type batched mode applies, F5) one pass over all B x 2^(n-1) amplitude
// pairs; every pair draws its own uniform (counter hash of (seed, pass, global pair index) in
// place of its curandState) and, below p, a second one picks X / Y / Z at 1/3, 2/3 — applied to
// that pair only (F7).  Three schedules of the same draws: pulled, in-tile, or step by step.
void run_reference_noise(qsim_batch* b, const std::vector<Op>& ops, const std::vector<NoiseChan>& dep) {
    if (run_pulled(b, ops, dep) || run_tile(b, ops, dep)) return;
    for (const Op& op : ops) {
        const Op* o = op.kind >= 0 ? &op : nullptr;
        if (gate_noise_tile_supported(b->n, o)) {  // (noise.hip: gate + in-tile channels in LDS)
            launch_gate_noise_step(b->d, b->n, (uint64_t)b->batch, b->traj0, o, dep, b->seed, b->ncounter, b->stream,
                                   &b->timer);
            continue;
        }
        if (o) launch_op(b->d, b->n, (uint64_t)b->batch, op, b->stream, &b->timer);
        launch_noise_after_gate(b->d, b->n, dep, b->seed, b->ncounter, b->stream, &b->timer, (uint64_t)b->batch,
                                b->traj0);
    }
}
// The Pauli frames of a run of `count` steps with `nch` channels (in d_ch): every draw, then per
// trajectory the frame in force before each step (cl: the steps whose Clifford gate moves it).
void build_frames(qsim_batch* b, size_t count, size_t nch, const std::vector<StepClifford>& cl) {
    const size_t need_frames = 2 * count * (size_t)b->batch;
    if (need_frames > b->frames_cap) {
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
        if (b->d_frames) QSIM_HIPCHK(hipFree(b->d_frames));
        if (b->d_fe) QSIM_HIPCHK(hipFree(b->d_fe));
        b->d_frames = nullptr;
        b->d_fe = nullptr;
        QSIM_HIPCHK(hipMalloc((void**)&b->d_frames, need_frames * sizeof(uint64_t)));
        QSIM_HIPCHK(hipMalloc((void**)&b->d_fe, need_frames / 2 * sizeof(int)));
        b->frames_cap = need_frames;
    }
    TimedLaunch tl(&b->timer, "pauli_frames", 0.0, b->stream);
    const uint64_t draws = (uint64_t)count * b->batch;
    hipLaunchKernelGGL(k_draw_steps, dim3((unsigned)((draws + 255) / 256)), dim3(256), 0, b->stream, b->d_ch, (int)nch,
                       b->seed, b->step, (int)count, b->batch, b->traj0, b->d_frames, b->d_fe);
    b->cliff.upload(cl.data(), cl.size() * sizeof(StepClifford), b->stream);
    hipLaunchKernelGGL(k_frame_build, dim3((b->batch + 63) / 64), dim3(64), 0, b->stream, (int)count, b->batch,
                       b->d_frames, b->d_fe, (const StepClifford*)b->cliff.ptr, b->d_xz, b->d_e,
                       b->frame_pending ? 1 : 0);
    QSIM_HIPCHK(hipGetLastError());
}
// Fused tile passes over all trajectories (a tile never straddles two).  Noise is carried as
// per-trajectory Pauli frames: no noise kernel per gate, one frame build before the circuit and
// one materialising Pauli pass when something next reads the amplitudes.  gates: the caller's
// list (ops[i] is gates[i] lowered; kind < 0: ignored by the reference gate set); nch channels.
void run_frames(qsim_batch* b, const qsim_gate* gates, const std::vector<Op>& ops, size_t nch) {
    const size_t count = ops.size();
    // a carried frame must be propagated (Cliffords) and conjugated (the rest) like noise
    const bool noisy = (nch > 0 || b->frame_pending) && count > 0;
    std::vector<Op> fops;
    std::vector<StepClifford> cl(count, StepClifford{CL_NONE, 0, -1, 0});
    for (size_t i = 0; i < count; ++i) {
        if (ops[i].kind < 0) continue;
        const qsim_gate g = map_gate(b, gates[i]);
        static const int code_of[QSIM_GATE_COUNT] = {
            CL_X, CL_Y, CL_Z, CL_H, CL_S, CL_NONE /*T*/, CL_SDG, CL_NONE /*Tdag*/,
            CL_NONE, CL_NONE, CL_NONE /*Rx Ry Rz*/, CL_CNOT, CL_CZ, CL_NONE, CL_NONE /*CRY CRZ*/,
            CL_SWAP, CL_NONE /*Toffoli*/};
        cl[i] = StepClifford{code_of[g.type], g.qubits[0], g.nqubits > 1 ? g.qubits[1] : -1, 0};
        fops.push_back(ops[i]);
        // circuit step = frame index for ops conjugated by the frame; Clifford gates move the
        // frame instead and run unconjugated (src -1)
        fops.back().src = (noisy && cl[i].code == CL_NONE) ? (int)i : -1;
    }
    if (noisy) build_frames(b, count, nch, cl);
    if (!fops.empty()) {
        // every control is a tile bit; circuit-specialised kernels for the passes no frame
        // conjugation reaches (all of them for a Clifford circuit)
        const CtrlOutOff ctrl_off;
        run_planned(b, fops, noisy ? b->d_frames : nullptr, nullptr);
    }
    if (noisy) {
        if (nch > 0) b->step += count;
        b->frame_pending = true;  // materialised by the next reader (or composed by the next run)
    }
}
// One launch per gate over all trajectories; after each, this step's Pauli string per trajectory
// (nch channels in d_ch) drawn and applied.
void run_per_gate(qsim_batch* b, const std::vector<Op>& ops, size_t nch) {
    for (const Op& op : ops) {
        if (op.kind >= 0) launch_op(b->d, b->n, (uint64_t)b->batch, op, b->stream, &b->timer);
        if (nch == 0) continue;
        {
            TimedLaunch tl(&b->timer, "pauli_draw", 0.0, b->stream);
            hipLaunchKernelGGL(k_pauli_draw, dim3((b->batch + 255) / 256), dim3(256), 0, b->stream, b->d_ch, (int)nch,
                               b->seed, b->step, b->batch, b->traj0, b->d_xz, b->d_e);
            QSIM_HIPCHK(hipGetLastError());
        }
        ++b->step;
        apply_frames(b);
    }
}
}  // namespace

extern "C" {

int qsim_batch_run_sweep(qsim_batch* b, const qsim_gate* gates, size_t count, const double* angles,
                         size_t n_slots, int flags) {
    bool plain = false;  // no parameterised gate: qsim_batch_run without channels
    const int rc = guarded([&] {
        need(b);
        std::vector<size_t> slots;
        const std::vector<qsim_gate> pg = sweep_arguments(b->n, gates, count, flags, slots);
        const size_t P = slots.size();
        if (n_slots != P) fail(QSIM_ERR_INVALID_ARGUMENT, "n_slots must be the number of parameterised gates");
        if (P && !angles) fail(QSIM_ERR_INVALID_ARGUMENT, "null angles");
        if (count == 0) return;
        if (P == 0) {
            plain = true;
            return;
        }
        // the table first: a bad angle or a failed allocation leaves the states as they are
        const size_t B = (size_t)b->batch;
        std::vector<double> tab(8 * B * P);
        for (size_t k = 0; k < P; ++k) {
            qsim_gate g = pg[slots[k]];
            for (size_t t = 0; t < B; ++t) {
                g.parameter = angles[t * P + k];
                const Op op = lower_gate(g, b->n);  // (one definition of each rotation)
                std::memcpy(&tab[8 * (k * B + t)], op.m, sizeof(op.m));
            }
        }
        try {
            b->sweep_table.upload(tab.data(), tab.size() * sizeof(double), b->stream);
        } catch (...) {  // (a refused growth left no block behind)
            if (!b->sweep_table.ptr) {
                b->sweep_table.cap = 0;
                b->sweep_table.shadow.clear();
            }
            throw;
        }
        const double* d_tab = (const double*)b->sweep_table.ptr;
        materialize(b);  // a sweep is noise-free: carried Pauli frames are applied first
        const bool fused_path = sweep_fused_path(b->n, flags);
        if (fused_path && b->basis && b->perm.empty()) {
            // first fused run of |0..0> members: the layout qsim_batch_run would choose for the
            // placeholder circuit (the same rule, memoised under the same kind)
            const CtrlOutOff ctrl_off;
            choose_first_layout(b, 1, pg.data(), count * sizeof(qsim_gate),
                                [&](const std::vector<int>& pi) { return sweep_lower(b->n, pg, pi, false); });
        }
        b->basis = false;
        const std::vector<Op> ops = sweep_lower(b->n, pg, b->perm, true);
        if (!fused_path) {  // one launch per gate over all members (batch_sweep.hip for the slots)
            for (const Op& op : ops) {
                if (op.src >= 0) launch_sweep_op(b->d, b->n, B, op, d_tab + 8 * B * (size_t)op.src, b->stream, &b->timer);
                else launch_op(b->d, b->n, B, op, b->stream, &b->timer);
            }
            return;
        }
        const CtrlOutOff ctrl_off;  // (every control is a tile bit, as in the Pauli-frame passes)
        run_planned(b, ops, nullptr, d_tab);
    });
    if (rc == QSIM_OK && plain) return qsim_batch_run(b, gates, count, nullptr, 0, flags);
    return rc;
}

int qsim_batch_sweep_plan(int n_qubits, int batch, const qsim_gate* gates, size_t count, int flags,
                          int32_t info[8]) {
    return guarded([&] {
        if (!info) fail(QSIM_ERR_INVALID_ARGUMENT, "null info");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > QSIM_MAX_QUBITS_SINGLE)
            fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits must be between 1 and 30");
        if (batch < 1) fail(QSIM_ERR_INVALID_ARGUMENT, "batch_size must be positive");
        std::vector<size_t> slots;
        const std::vector<qsim_gate> pg = sweep_arguments(n_qubits, gates, count, flags, slots);
        for (int i = 0; i < 8; ++i) info[i] = 0;
        info[0] = (int32_t)slots.size();
        info[3] = (int32_t)count;
        const uint64_t bytes = 64ull * (uint64_t)batch * (uint64_t)slots.size();
        info[4] = (int32_t)(uint32_t)(bytes & 0xffffffffull);
        info[5] = (int32_t)(uint32_t)(bytes >> 32);
        const bool fused_path = sweep_fused_path(n_qubits, flags);
        info[6] = fused_path ? 1 : 0;
        if (!fused_path || count == 0) return;
        const CtrlOutOff ctrl_off;
        const Plan plan = plan_fused(sweep_lower(n_qubits, pg, {}, true), n_qubits);
        info[1] = (int32_t)plan.passes.size();
        for (size_t p = 0; p < plan.passes.size(); ++p) info[2] += pass_has_step_op(plan, p) ? 1 : 0;
    });
}

// ---- adjoint gradients of a sweep (the kernels and the backward walk: batch_adjoint.hip) ----
int qsim_batch_gradient_sweep(qsim_batch* b, const qsim_gate* gates, size_t count, const double* angles,
                              size_t n_slots, const qsim_pauli_term* terms, size_t nterms, int flags, double* values,
                              double* grads) {
    bool backward = false;  // there is something to differentiate: P > 0 and H != 0
    int rc = guarded([&] {
        need(b);
        std::vector<size_t> slots;
        sweep_arguments(b->n, gates, count, flags, slots);
        const size_t P = slots.size();
        if (n_slots != P) fail(QSIM_ERR_INVALID_ARGUMENT, "n_slots must be the number of parameterised gates");
        if (P && !angles) fail(QSIM_ERR_INVALID_ARGUMENT, "null angles");
        if (!terms && nterms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
        check_pauli_masks(b->n, terms, nterms, "Pauli term");
        if (!values || (P && !grads)) fail(QSIM_ERR_INVALID_ARGUMENT, "null output");
        backward = P > 0 && !lower_expectation(b->n, terms, nterms, nullptr).terms.empty();
        // (the work ensembles before the forward run: a failed allocation leaves the members as they were)
        if (backward) batch_grad_ensure(b->grad, b->n, (uint64_t)b->batch, P, b->stream);
    });
    if (rc != QSIM_OK) return rc;
    // The forward run is the sweep itself (its angle checks come before its first launch): the
    // members end exactly as it leaves them, and nothing below writes to them.
    if (count > 0 && (rc = qsim_batch_run_sweep(b, gates, count, angles, n_slots, flags)) != QSIM_OK) return rc;
    return guarded([&] {
        const int n = b->n;
        const size_t B = (size_t)b->batch, P = n_slots;
        std::fill(values, values + B, 0.0);
        if (P) std::fill(grads, grads + B * P, 0.0);
        const int* perm = b->perm.empty() ? nullptr : b->perm.data();
        // the values: what qsim_batch_expectation computes, the same way
        const ExpectPlan eplan = lower_expectation(n, terms, nterms, perm);
        if (eplan.terms.empty()) {  // H = 0 (no terms, or every coefficient cancels)
            QSIM_HIPCHK(hipStreamSynchronize(b->stream));
            return;
        }
        materialize(b);
        double* d_val = (double*)b->scratch.get((B + B * expect_chunks(B)) * sizeof(double), b->stream);
        launch_expectation(b->d, n, B, eplan, b->expect_terms, d_val + B, d_val, b->stream, &b->timer);
        QSIM_HIPCHK(hipMemcpyAsync(values, d_val, B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        if (!backward) {
            QSIM_HIPCHK(hipStreamSynchronize(b->stream));
            return;
        }
        // phi = a copy of the ensemble where it lies, lambda = H phi under that layout
        BatchGradWork& w = *b->grad;
        QSIM_HIPCHK(hipMemcpyAsync(w.phi, b->d, (B * sizeof(double2)) << n, hipMemcpyDeviceToDevice, b->stream));
        launch_pauli_apply(b->d, w.lam, n, lower_pauli_apply(n, terms, nterms, perm), w.terms, b->stream, &b->timer, B);
        QSIM_HIPCHK(hipMemsetAsync(w.d_out, 0, P * B * sizeof(double), b->stream));
        // the walk: the sweep's own placeholder ops at the slots, the other gates inverted, all under b->perm
        std::vector<size_t> slots;
        const std::vector<qsim_gate> pg = sweep_arguments(n, gates, count, flags, slots);
        const std::vector<Op> ops = sweep_lower(n, pg, b->perm, true);
        std::vector<BatchBackStep> steps;
        for (size_t k = count; k-- > slots[0];) {  // (gates before the first parameter are never undone)
            BatchBackStep st;
            if (ops[k].src >= 0) {
                st.op = ops[k];
                st.pauli = gate_generator(gates[k]).pauli;
            } else {
                const qsim_gate inv = gate_inverse(gates[k]);
                st.op = lower_gates(n, &inv, 1, b->perm)[0];
                st.op.src = -1;
            }
            steps.push_back(st);
        }
        batch_adjoint_sweep(w, n, B, steps, (const double*)b->sweep_table.ptr, sweep_fused_path(n, flags), b->stream,
                            &b->timer);
        std::vector<double> by_slot(P * B);  // [slot][member] on the device, member-major for the caller
        QSIM_HIPCHK(hipMemcpyAsync(by_slot.data(), w.d_out, P * B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
        for (size_t t = 0; t < B; ++t)
            for (size_t j = 0; j < P; ++j) grads[t * P + j] = by_slot[j * B + t];
    });
}

int qsim_batch_gradient_release(qsim_batch* b) {
    return guarded([&] {
        need(b);
        if (!b->grad) return;
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
        b->grad.reset();
    });
}

int qsim_batch_gradient_plan(int n_qubits, int batch, const qsim_gate* gates, size_t count,
                             const qsim_pauli_term* terms, size_t nterms, int flags, int32_t info[8]) {
    return guarded([&] {
        if (!info) fail(QSIM_ERR_INVALID_ARGUMENT, "null info");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > QSIM_MAX_QUBITS_SINGLE)
            fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits must be between 1 and 30");
        if (batch < 1) fail(QSIM_ERR_INVALID_ARGUMENT, "batch_size must be positive");
        std::vector<size_t> slots;
        sweep_arguments(n_qubits, gates, count, flags, slots);
        if (!terms && nterms) fail(QSIM_ERR_INVALID_ARGUMENT, "null term list");
        check_pauli_masks(n_qubits, terms, nterms, "Pauli term");
        for (int i = 0; i < 8; ++i) info[i] = 0;
        info[0] = (int32_t)slots.size();
        bool in_segment = false;
        for (size_t k = slots.empty() ? count : slots[0]; k < count; ++k) {
            if (gate_is_parameterised(gates[k].type)) {
                in_segment = false;
            } else if (!in_segment) {  // (gates before the first parameter are never undone)
                ++info[1];
                in_segment = true;
            }
        }
        info[2] = (int32_t)lower_pauli_apply(n_qubits, terms, nterms, nullptr).launches;
        info[3] = sweep_fused_path(n_qubits, flags) ? 1 : 0;
        const uint64_t bytes = (2ull * (uint64_t)batch * sizeof(double2)) << n_qubits;
        info[4] = (int32_t)(uint32_t)(bytes & 0xffffffffull);
        info[5] = (int32_t)(uint32_t)(bytes >> 32);
    });
}

int qsim_batch_create(int n_qubits, int batch_size, qsim_batch** out) {
    return guarded([&] {
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        *out = nullptr;
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > QSIM_MAX_QUBITS_SINGLE)
            fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits must be between 1 and 30");
        if (batch_size < 1) fail(QSIM_ERR_INVALID_ARGUMENT, "batch_size must be positive");
        auto b = std::make_unique<qsim_batch>();
        b->n = n_qubits;
        b->batch = batch_size;
        QSIM_HIPCHK(hipGetDevice(&b->device));
        QSIM_HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->timer.stream = b->stream;
        QSIM_HIPCHK(hipMalloc((void**)&b->d0, ((uint64_t)batch_size * sizeof(double2)) << n_qubits));
        b->d = b->d0;
        QSIM_HIPCHK(hipMalloc((void**)&b->d_xz, 2 * sizeof(uint64_t) * batch_size));
        QSIM_HIPCHK(hipMalloc((void**)&b->d_e, sizeof(int) * batch_size));
        b->seed = std::random_device{}();  // reference seeds from random_device (NoiseModel.cu:663)
        launch_init_basis(b->d, n_qubits, batch_size, 0, b->stream);
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
        *out = b.release();
    });
}

int qsim_batch_destroy(qsim_batch* b) {
    return guarded([&] { delete b; });
}

int qsim_batch_reset(qsim_batch* b) {
    return guarded([&] {
        need(b);
        launch_init_basis(b->d, b->n, b->batch, 0, b->stream);
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
        b->frame_pending = false;
        b->perm.clear();
        b->basis = true;
    });
}

int qsim_batch_set_seed(qsim_batch* b, uint64_t seed) {
    return guarded([&] {
        need(b);
        b->seed = seed;
        b->step = 0;
        b->ncounter = 0;
    });
}

int qsim_batch_set_trajectory_offset(qsim_batch* b, uint64_t first) {
    return guarded([&] {
        need(b);
        if (first > (1ull << 40)) fail(QSIM_ERR_INVALID_ARGUMENT, "trajectory offset out of range");
        b->traj0 = first;
    });
}

int qsim_batch_run(qsim_batch* b, const qsim_gate* gates, size_t count,
                   const qsim_noise_channel* channels, size_t n_channels, int flags) {
    return guarded([&] {
        need(b);
        if (!gates && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        std::vector<DevChannel> ch;
        for (size_t i = 0; i < n_channels; ++i) {
            const auto& c = channels[i];
            if (c.qubit < 0 || c.qubit >= b->n) fail(QSIM_ERR_OUT_OF_RANGE, "noise qubit out of range");
            if (c.type == 0 || c.type == 3 || c.type == 4 || c.type == 5)
                ch.push_back(DevChannel{c.type, c.qubit, c.probability});
        }
        for (size_t i = 0; i < count; ++i) validate_gate(gates[i], b->n);
        static const bool fused_env = env_switch("QSIM_BATCH_FUSED", true);
        const bool reference_noise = (flags & QSIM_BATCH_REFERENCE_NOISE) != 0;
        const bool fused_path = b->n >= 10 && fused_env && !(flags & QSIM_BATCH_PER_GATE) && !reference_noise;
        if (reference_noise) canonicalize(b);  // per-pair draws name positions
        const bool frame_path = fused_path && b->n >= 10;  // (the Pauli-frame passes below)
        if (!frame_path) materialize(b);  // per-gate paths act on the plain vectors
        auto reference_gate = [](const qsim_gate& g) { return g.type <= QSIM_GATE_H || g.type == QSIM_GATE_CNOT; };
        if (fused_path && b->basis && b->perm.empty() && count > 0) {
            // First fused run of |0..0> trajectories: relabel for the plan's tile layouts (chosen
            // under the tile-control rule the frame path plans with, and memoised under it)
            std::unique_ptr<CtrlOutOff> ctrl_off;
            if (frame_path) ctrl_off = std::make_unique<CtrlOutOff>();
            choose_first_layout(b, 1 + (flags & QSIM_BATCH_REFERENCE_GATESET ? 1 : 0), gates, count * sizeof(qsim_gate),
                                [&](const std::vector<int>& pi) {
                                    std::vector<Op> lops;
                                    for (size_t i = 0; i < count; ++i) {
                                        qsim_gate g = gates[i];
                                        if ((flags & QSIM_BATCH_REFERENCE_GATESET) && !reference_gate(g)) continue;
                                        for (int j = 0; j < g.nqubits && j < 3; ++j) g.qubits[j] = pi[g.qubits[j]];
                                        lops.push_back(lower_gate(g, b->n));
                                        lops.back().src = -1;
                                    }
                                    return lops;
                                });
        }
        b->basis = false;
        for (DevChannel& c : ch)
            if (!b->perm.empty()) c.qubit = b->perm[c.qubit];
        if (ch.size() > b->ch_cap) {
            if (b->d_ch) {
                QSIM_HIPCHK(hipStreamSynchronize(b->stream));
                QSIM_HIPCHK(hipFree(b->d_ch));
            }
            QSIM_HIPCHK(hipMalloc((void**)&b->d_ch, ch.size() * sizeof(DevChannel)));
            b->ch_cap = ch.size();
        }
        if (!ch.empty())
            QSIM_HIPCHK(hipMemcpyAsync(b->d_ch, ch.data(), ch.size() * sizeof(DevChannel),
                                       hipMemcpyHostToDevice, b->stream));
        std::vector<Op> ops;
        for (size_t i = 0; i < count; ++i) {
            const qsim_gate g = map_gate(b, gates[i]);
            if (flags & QSIM_BATCH_REFERENCE_GATESET) {
                // src/NoiseModel.cu:742-763, 808-812, 821-825: only X/Y/Z/H and CNOT act.
                validate_gate(g, b->n);
                ops.push_back(reference_gate(g) ? lower_gate(g, b->n) : Op{});
                if (!reference_gate(g)) ops.back().kind = -1;
            } else {
                ops.push_back(lower_gate(g, b->n));
            }
        }
        if (reference_noise) {
            std::vector<NoiseChan> dep;
            for (size_t i = 0; i < n_channels; ++i)
                if (channels[i].type == 0) dep.push_back(NoiseChan{0, channels[i].qubit, channels[i].probability});
            run_reference_noise(b, ops, dep);
        } else if (frame_path) {
            run_frames(b, gates, ops, ch.size());
        } else {
            run_per_gate(b, ops, ch.size());
        }
    });
}

int qsim_batch_avg_probabilities(qsim_batch* b, double* dst) {
    return guarded([&] {
        need(b);
        canonicalize(b);
        const uint64_t N = 1ull << b->n;
        double* d_p = (double*)b->scratch.get(N * sizeof(double), b->stream);
        launch_avg_probabilities(b->d, b->n, (uint64_t)b->batch, d_p, b->stream);
        QSIM_HIPCHK(hipMemcpyAsync(dst, d_p, N * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int qsim_batch_traj_probabilities(qsim_batch* b, int traj, double* dst) {
    return guarded([&] {
        need(b);
        canonicalize(b);
        if (traj < 0 || traj >= b->batch) fail(QSIM_ERR_OUT_OF_RANGE, "Invalid trajectory index");
        const uint64_t N = 1ull << b->n;
        double* d_p = (double*)b->scratch.get(N * sizeof(double), b->stream);
        launch_probabilities(b->d + (uint64_t)traj * N, N, d_p, b->stream);
        QSIM_HIPCHK(hipMemcpyAsync(dst, d_p, N * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int qsim_batch_sample(qsim_batch* b, const double* uniforms, int shots, int64_t* out) {
    return guarded([&] {
        need(b);
        canonicalize(b);
        if (shots < 0) fail(QSIM_ERR_INVALID_ARGUMENT, "n_shots must be non-negative");
        if (shots > 0 && (!uniforms || !out)) fail(QSIM_ERR_INVALID_ARGUMENT, "null buffer");
        sample_indices(b->d, b->n, (uint64_t)b->batch, uniforms, shots, out, b->stream, b->scratch);
    });
}

int qsim_batch_histogram(qsim_batch* b, const double* uniforms, int shots, int64_t* hist) {
    return guarded([&] {
        need(b);
        canonicalize(b);
        if (shots < 0) fail(QSIM_ERR_INVALID_ARGUMENT, "n_shots must be non-negative");
        if (!hist || (shots > 0 && !uniforms)) fail(QSIM_ERR_INVALID_ARGUMENT, "null buffer");
        const uint64_t N = 1ull << b->n, nshots = (uint64_t)shots * (uint64_t)b->batch;
        std::vector<int64_t> idx(nshots);
        sample_indices(b->d, b->n, (uint64_t)b->batch, uniforms, shots, idx.data(), b->stream,
                       b->scratch);
        // counts on the device: scratch2 = [hist N x u64][indices nshots x i64]
        char* base = (char*)b->scratch2.get(N * 8 + std::max<uint64_t>(1, nshots) * 8, b->stream);
        unsigned long long* d_h = (unsigned long long*)base;
        int64_t* d_idx = (int64_t*)(base + N * 8);
        QSIM_HIPCHK(hipMemsetAsync(d_h, 0, N * sizeof(unsigned long long), b->stream));
        if (nshots) {
            QSIM_HIPCHK(hipMemcpyAsync(d_idx, idx.data(), nshots * sizeof(int64_t),
                                       hipMemcpyHostToDevice, b->stream));
            launch_histogram(d_idx, nshots, N, d_h, b->stream);
        }
        QSIM_HIPCHK(hipMemcpyAsync(hist, d_h, N * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int qsim_batch_traj_state(qsim_batch* b, int traj, double* dst) {
    return guarded([&] {
        need(b);
        canonicalize(b);
        if (traj < 0 || traj >= b->batch) fail(QSIM_ERR_OUT_OF_RANGE, "Invalid trajectory index");
        const uint64_t N = 1ull << b->n;
        QSIM_HIPCHK(hipMemcpyAsync(dst, b->d + (uint64_t)traj * N, N * sizeof(double2),
                                   hipMemcpyDeviceToHost, b->stream));
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
    });
}

// Reads b->d under b->perm: carried frames are applied (materialize), the layout is not restored.
int qsim_batch_expectation(qsim_batch* b, const qsim_pauli_term* terms, size_t count, double* per_traj) {
    return guarded([&] {
        need(b);
        if (!per_traj || (count && !terms)) fail(QSIM_ERR_INVALID_ARGUMENT, "null buffer");
        const ExpectPlan plan = lower_expectation(b->n, terms, count, b->perm.empty() ? nullptr : b->perm.data());
        const uint64_t B = (uint64_t)b->batch;
        std::fill(per_traj, per_traj + B, 0.0);
        if (plan.terms.empty()) return;
        materialize(b);
        // scratch = [per-trajectory sums B][partials B x chunks]
        double* d_out = (double*)b->scratch.get((B + B * expect_chunks(B)) * sizeof(double), b->stream);
        launch_expectation(b->d, b->n, B, plan, b->expect_terms, d_out + B, d_out, b->stream, &b->timer);
        QSIM_HIPCHK(hipMemcpyAsync(per_traj, d_out, B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
    });
}

// ---- overlap matrices (the kernels: batch_overlap.hip) ----
static bool overlap_mfma_enabled() { return env_switch("QSIM_OVERLAP_MFMA", true); }
static bool same_layout(const std::vector<int>& p, const std::vector<int>& q) {
    const size_t n = std::max(p.size(), q.size());
    for (size_t i = 0; i < n; ++i)
        if ((p.empty() ? (int)i : p[i]) != (q.empty() ? (int)i : q[i])) return false;
    return true;
}
// The partial tiles and the Ba x Bb result in a's scratch, before anything is launched: a refused
// allocation is QSIM_ERR_DEVICE with the HIP error cleared and every amplitude where it was.
static double2* overlap_scratch(qsim_batch* a, const OverlapPlan& p, uint64_t entries) {
    const size_t bytes = p.scratch_bytes + entries * sizeof(double2);
    Scratch& sc = a->scratch;
    if (bytes > sc.cap) {
        if (sc.ptr) {
            QSIM_HIPCHK(hipStreamSynchronize(a->stream));
            QSIM_HIPCHK(hipFree(sc.ptr));
            sc.ptr = nullptr;
            sc.cap = 0;
        }
        if (!(sc.ptr = device_alloc_or_null(bytes))) fail(QSIM_ERR_DEVICE, "no device memory for the overlap scratch");
        sc.cap = bytes;
    }
    return (double2*)sc.ptr;
}
// out = the Ba x Bb overlaps of a's members with the Bb vectors at d_b (null: a's own, the self
// case), both already in one layout and complete on their streams.
static void overlap_into(qsim_batch* a, const double2* d_b, uint64_t Bb, const OverlapPlan& p, double2* d_work, double* out) {
    const uint64_t Ba = (uint64_t)a->batch;
    const bool self = d_b == nullptr;
    double2* d_out = d_work + p.scratch_bytes / sizeof(double2);
    launch_batch_overlap(a->d, self ? a->d : d_b, a->n, Ba, Bb, self, p, d_work, d_out, a->stream, &a->timer);
    QSIM_HIPCHK(hipMemcpyAsync(out, d_out, Ba * Bb * sizeof(double2), hipMemcpyDeviceToHost, a->stream));
    QSIM_HIPCHK(hipStreamSynchronize(a->stream));
}

// Self: reads a->d under a->perm like qsim_batch_expectation (G does not depend on a relabeling all
// members share).  Cross: in place when the two layouts agree, else both are restored.
int qsim_batch_overlaps(qsim_batch* a, qsim_batch* b, double* out) {
    return guarded([&] {
        need(a);
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        const bool self = !b || b == a;
        if (!self && a->n != b->n) fail(QSIM_ERR_INVALID_ARGUMENT, "ensembles have different qubit counts");
        if (!self && a->device != b->device) fail(QSIM_ERR_INVALID_ARGUMENT, "ensembles live on different devices");
        const uint64_t Ba = (uint64_t)a->batch, Bb = self ? Ba : (uint64_t)b->batch;
        const OverlapPlan p = overlap_plan(a->n, Ba, Bb, self, overlap_mfma_enabled());
        double2* d_work = overlap_scratch(a, p, Ba * Bb);
        if (self) {
            materialize(a);
        } else if (same_layout(a->perm, b->perm)) {
            materialize(a);
            materialize(b);
        } else {  // one common layout: the identity
            canonicalize(a);
            canonicalize(b);
        }
        if (!self) QSIM_HIPCHK(hipStreamSynchronize(b->stream));  // b's writes done; a's stream orders the rest
        overlap_into(a, self ? nullptr : b->d, Bb, p, d_work, out);
    });
}

int qsim_batch_state_overlaps(qsim_batch* a, qsim_state* s, double* out) {
    return guarded([&] {
        need(a);
        check_state(s);
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (a->n != s->n) fail(QSIM_ERR_INVALID_ARGUMENT, "ensemble and state have different qubit counts");
        if (a->device != s->device) fail(QSIM_ERR_INVALID_ARGUMENT, "ensemble and state live on different devices");
        const OverlapPlan p = overlap_plan(a->n, (uint64_t)a->batch, 1, false, false);
        double2* d_work = overlap_scratch(a, p, (uint64_t)a->batch);
        share_flush(s);
        if (same_layout(a->perm, s->perm)) {
            materialize(a);
        } else {
            canonicalize(a);
            prep(s, false);
        }
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
        overlap_into(a, s->d, 1, p, d_work, out);
    });
}

int qsim_batch_overlap_plan(int n_qubits, int batch_a, int batch_b, int self, int32_t info[8]) {
    return guarded([&] {
        if (!info) fail(QSIM_ERR_INVALID_ARGUMENT, "null info");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > QSIM_MAX_QUBITS_SINGLE)
            fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits must be between 1 and 30");
        if (batch_a < 1 || batch_b < 1) fail(QSIM_ERR_INVALID_ARGUMENT, "batch_size must be positive");
        if (self && batch_a != batch_b) fail(QSIM_ERR_INVALID_ARGUMENT, "the self case has one batch size");
        const OverlapPlan p =
            overlap_plan(n_qubits, (uint64_t)batch_a, (uint64_t)batch_b, self != 0, overlap_mfma_enabled());
        if (p.tiles > 0x7fffffffull) fail(QSIM_ERR_INVALID_ARGUMENT, "too many members for one overlap launch");
        info[0] = p.mfma ? 1 : 0;
        info[1] = (int32_t)p.tiles_a;
        info[2] = (int32_t)p.tiles_b;
        info[3] = (int32_t)p.tiles;
        info[4] = (int32_t)p.chunks;
        info[5] = (int32_t)(uint32_t)(p.scratch_bytes & 0xffffffffull);
        info[6] = (int32_t)(uint32_t)(p.scratch_bytes >> 32);
        info[7] = 0;
    });
}

int qsim_batch_device_ptr(qsim_batch* b, void** dptr) {
    return guarded([&] {
        need(b);
        canonicalize(b);
        b->basis = false;  // the caller may write through the pointer
        settle_in_d0(b);   // (pulled runs copy their result back to this buffer from now on)
        b->pinned = true;
        *dptr = b->d;
    });
}

int qsim_batch_perm(qsim_batch* b, int32_t* perm) {
    return guarded([&] {
        need(b);
        if (!perm) fail(QSIM_ERR_INVALID_ARGUMENT, "null perm");
        for (int q = 0; q < b->n; ++q) perm[q] = b->perm.empty() ? q : b->perm[q];
    });
}

int qsim_batch_last_run(qsim_batch* b, int* passes, int* jit_passes) {
    return guarded([&] {
        need(b);
        if (passes) *passes = b->last_passes;
        if (jit_passes) *jit_passes = b->last_jit_passes;
    });
}

int qsim_batch_sync(qsim_batch* b) {
    return guarded([&] {
        need(b);
        materialize(b);  // the carried frames are queued work too
        QSIM_HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int qsim_batch_profile(qsim_batch* b, int enable) {
    return guarded([&] {
        need(b);
        b->timer.enabled = enable != 0;
    });
}

int qsim_batch_profile_count(qsim_batch* b, int* n) {
    return guarded([&] {
        need(b);
        b->timer.resolve();
        *n = (int)b->timer.stats.size();
    });
}

int qsim_batch_profile_get(qsim_batch* b, int i, char* name, size_t name_len, double* total_ms,
                           int64_t* launches, double* alg_bytes) {
    return guarded([&] {
        need(b);
        b->timer.resolve();
        if (i < 0 || i >= (int)b->timer.stats.size()) fail(QSIM_ERR_OUT_OF_RANGE, "bad index");
        const auto& st = b->timer.stats[i];
        if (name && name_len) {
            std::strncpy(name, st.name.c_str(), name_len - 1);
            name[name_len - 1] = 0;
        }
        if (total_ms) *total_ms = st.ms;
        if (launches) *launches = st.launches;
        if (alg_bytes) *alg_bytes = st.bytes;
    });
}

}  // extern "C"
