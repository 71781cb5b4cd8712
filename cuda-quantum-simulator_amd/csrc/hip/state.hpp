// state.hpp — the single-GPU state's object (struct qsim_state) and what the files that work on it
// share: the C entries' guard, the device guard and the state helpers that cross files (file map:
// DESIGN.md).  The single-GPU counterpart of dist_state.hpp.
//
// Each qsim_state owns its device buffer (2^n x 16 B) and a non-blocking HIP stream; gate
// application is asynchronous on that stream (as the reference's launches are on the legacy
// stream, src/Simulator.cu:95-97) and every readout synchronizes it (src/StateVector.cu:204-233).
#pragma once

#include <hip/hip_runtime.h>

#include <exception>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "engine.hpp"
#include "qsim_hip.h"

#define QSIM_REQUIRE(cond, code, msg) \
    do {                              \
        if (!(cond)) fail(code, msg); \
    } while (0)

namespace qsim_hip {

// The guard of every extern "C" entry of the library: the exception becomes the thread's last
// error (qsim_last_error) and a QSIM_ERR_* return code.
template <typename F>
int guarded(F&& f) {
    try {
        f();
        return QSIM_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return QSIM_ERR_RUNTIME;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return QSIM_ERR_RUNTIME;
    }
}

// A gate under the labels of a state or an ensemble (anything with n and perm; empty: identity).
template <typename S>
qsim_gate map_gate(const S* s, const qsim_gate& g) {
    qsim_gate m = g;
    if (!s->perm.empty())
        for (int j = 0; j < g.nqubits && j < 3; ++j)
            if (g.qubits[j] >= 0 && g.qubits[j] < s->n) m.qubits[j] = s->perm[g.qubits[j]];
    return m;
}

// Adjoint gradients (adjoint.hip, qsim_state_gradient): the two 2^n work states of the backward
// sweep, the per-gate results and the descriptors of the sweep's own plans.  Kept on the state
// between calls (an optimiser asks for hundreds of gradients); qsim_state_gradient_release and
// qsim_state_destroy free it.  Nothing here is shared with qsim_run: the state's plan cache,
// descriptor buffers and last-run figures stay what the forward run left.
struct GradWork {
    double2* phi = nullptr;
    double2* lam = nullptr;
    double* d_out = nullptr;  // out_cap doubles: dE/dtheta per gate
    size_t out_cap = 0;
    DevBuf ops, stages, terms;
    PlanCache plans;
    ~GradWork() {
        if (phi) (void)hipFree(phi);
        if (lam) (void)hipFree(lam);
        if (d_out) (void)hipFree(d_out);
    }
};

// Run sharing (engine.hpp SharePlan; the contract: include/qsim_hip.h qsim_set_run_share): the
// joint plan of `copies` runs of one circuit, its compiled kernels, and how far the current cycle
// has come.  armed: the state lies in one of the joint plan's layouts and identical fused runs are
// executed as calls of the cycle; calls > 0: gates may be pending (share_flush).
struct ShareState {
    std::vector<qsim_gate> gates;  // the circuit sp was planned for
    SharePlan sp;
    JitState jit;
    bool have = false;     // sp holds a joint plan for `gates`
    bool refused = false;  // no joint plan pays for `gates`: never tried again
    bool armed = false;
    bool completed = false;  // a whole cycle has run since the state was armed
    int calls = 0;         // calls of the current cycle so far
    size_t next = 0;       // the first joint pass not yet launched
};

}  // namespace qsim_hip

struct qsim_state {
    int n = 0;
    int device = 0;
    double2* d = nullptr;
    void* base = nullptr;  // the allocation d lies in
    hipStream_t stream = nullptr;
    double* d_partials = nullptr;
    double* d_result = nullptr;
    qsim_hip::DevBuf ops, stages;  // fused-plan descriptors, re-uploaded only when the plan changes
    qsim_hip::DevBuf expect_terms;  // term table of the last expectation value (expect.hip)
    qsim_hip::PlanCache plans;
    qsim_hip::Timer timer;
    int last_passes = 0, last_jit_passes = 0;  // of the last fused run (qsim_state_last_run)
    qsim_hip::Scratch scratch;
    // Layout-aware relabeling (relabel.hip): logical qubit q lives at physical position perm[q]
    // (empty: identity).  basis: the amplitudes are the computational basis state basis_idx
    // (physical index) — set by create / init, cleared by anything else that writes them.
    std::vector<int> perm;
    bool basis = true;
    uint64_t basis_idx = 0;
    // tile height chosen for this state by the first-run calibration (-1: the size rule), and
    // whether its layout was chosen by timing candidates on the device
    int tile_h = -1;
    bool calibrated = false;
    bool relayout = false;  // the first-run choice is a relayout plan (relayout.hip)
    // Relayout passes write out of place: the state alternates between two buffers (d is the
    // current one; alt_base is allocated on the first relayout run).  pinned: a raw device
    // pointer was handed out, so the amplitudes are copied back to it after such a run.
    void* alt_base = nullptr;
    double2* alt = nullptr;
    double2* base_d = nullptr;  // the amplitudes' address inside `base` (d == base_d or alt_base)
    bool pinned = false;
    // Noisy runs (noisy_run.hip): the side stream, events, flip lists and code words of the pulled
    // (noise.hip launch_pull_noise_run) and in-tile (launch_gate_noise_run) schedules
    qsim_hip::NoiseSide noise;
    std::unique_ptr<qsim_hip::GradWork> grad;  // adjoint gradients: work states and plans (null until used)
    // run sharing: the gate list of the last fused qsim_run (cleared by every reader and writer of
    // amplitudes in between), the cycle, and share_block (a caller that reads right after its run)
    std::vector<qsim_gate> last_gates;
    std::unique_ptr<qsim_hip::ShareState> share;
    bool share_block = false;
    // back-off: cycles in a row that a reader ended before one whole cycle had run, and the
    // identical repeats to let pass unshared before arming again (2^strikes - 1, at most 63) — a
    // loop of "run twice, read" must not pay the arming (a gate-free pass, a flush plan) each time
    int share_strikes = 0, share_wait = 0;
    ~qsim_state() {
        if (stream) (void)hipStreamSynchronize(stream);
        grad.reset();
        noise.destroy();
        if (base) (void)hipFree(base);
        if (alt_base) (void)hipFree(alt_base);
        if (d_partials) (void)hipFree(d_partials);
        if (d_result) (void)hipFree(d_result);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace qsim_hip {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) QSIM_HIPCHK(hipSetDevice(dev));
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

inline void check_state(const qsim_state* s) {
    if (!s) fail(QSIM_ERR_INVALID_ARGUMENT, "null state handle");
}
void check_dm(const qsim_state* s, int n);  // s holds rho of n qubits (density.hip)
// The tile height this state's plans are made at: its first-run choice, else the size rule.
inline int state_tile_height(const qsim_state* s) { return s->tile_h >= 0 ? s->tile_h : tile_height_for(s->n); }

// ---- the state core (state.hip) ---------------------------------------------------------------
bool ensure_alt(qsim_state* s);   // false: no room (or refused): the caller stays in place
void release_alt(qsim_state* s);  // free the buffer the amplitudes are not in
void canonicalize(qsim_state* s);      // undo the relabeling (flushes a run-sharing cycle first)
void drop_layout(qsim_state* s);       // before an entry that overwrites every amplitude
void prep(qsim_state* s, bool touch);  // before an entry that reads amplitudes by index (touch: and writes)
// ---- the run (run.hip) ------------------------------------------------------------------------
// A pinned state (handed-out device pointer `home`) whose amplitudes a run left in the other
// buffer: copied back, so the pointer keeps seeing them.
void settle_home(qsim_state* s, double2* home);
void launch_plan(qsim_state* s, const Plan& plan, Timer* tm, const JitModule* jm, size_t first = 0,
                 size_t last = SIZE_MAX);
void run_fused(qsim_state* s, const std::vector<Op>& ops, bool jit = true);
void share_flush(qsim_state* s);    // run the pending gates of a run-sharing cycle; ends the cycle
void share_discard(qsim_state* s);  // drop them (the amplitudes are about to be overwritten)
// ---- the first run's layout choice (first_layout.hip) -------------------------------------------
// One timed candidate: a tile height and the labels chosen under it, with the circuit lowered
// under those labels and its plan at that height.
struct LayoutCandidate {
    int h = kTileHDefault;
    std::vector<int> perm;  // empty: identity
    std::vector<Op> ops;
    Plan plan;
    bool relayout = false;  // a relayout plan (relayout.hip)
};
size_t calibrate_candidates(qsim_state* s, std::vector<LayoutCandidate>& cands);
void choose_first_layout(qsim_state* s, const qsim_gate* gates, size_t count);
// ---- adjoint gradients (adjoint.hip; pauli_rot.hip sweeps with the same prologue) ----------------
GradWork* gradient_prologue(qsim_state* s, const qsim_pauli_term* terms, size_t nterms, size_t count, bool sweep,
                            double* value, double* grad);

}  // namespace qsim_hip
