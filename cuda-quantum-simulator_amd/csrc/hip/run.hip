// run.hip — running gates on a single-GPU state: one fused plan on the state's two buffers, the
// run-sharing cycle driver, and the extern "C" entries that apply gates and matrices and describe
// the last run and the layout it left (include/qsim_hip.h).  The counterpart of dist_run.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "state.hpp"

using namespace qsim_hip;

namespace qsim_hip {

void settle_home(qsim_state* s, double2* home) {
    if (!s->pinned || s->d == home) return;
    QSIM_HIPCHK(hipMemcpyAsync(home, s->d, sizeof(double2) << s->n, hipMemcpyDeviceToDevice, s->stream));
    s->alt = s->d;
    s->d = home;
}

// One fused plan on the state: relayout passes alternate between the state's two buffers.
// [first, last): the passes to launch (run sharing launches a joint plan piecewise).
void launch_plan(qsim_state* s, const Plan& plan, Timer* tm, const JitModule* jm, size_t first, size_t last) {
    FusedRange range;
    range.first = first;
    range.last = last;
    bool relayout = false;
    for (const FusedPass& p : plan.passes) relayout = relayout || p.relayout;
    if (relayout) {
        // (choose_first_layout only takes relayout plans once the buffer exists)
        if (!ensure_alt(s)) fail(QSIM_ERR_DEVICE, "out of device memory for the relayout buffer");
        range.alt = s->alt;
    }
    double2* const home = s->d;
    double2* r = launch_fused(s->d, s->n, 1, plan, (const TileOp*)s->ops.ptr, (const Stage*)s->stages.ptr,
                              s->stream, tm, jm, nullptr, range);
    if (r == home) return;
    s->alt = home;
    s->d = r;
    settle_home(s, home);
}

// jit = false: the pass interpreter only (a one-off network — the layout restore — would wait
// longer for its compile than its passes take).
void run_fused(qsim_state* s, const std::vector<Op>& ops, bool jit) {
    PlanCache::Entry& pe = s->plans.get(ops, s->n, s->stream);
    const Plan& plan = pe.plan;
    const JitModule* jm = jit ? jit_for(pe.jit, plan, s->n) : nullptr;
    s->ops.upload(plan.ops.data(), plan.ops.size() * sizeof(TileOp), s->stream);
    s->stages.upload(plan.stages.data(), plan.stages.size() * sizeof(Stage), s->stream);
    launch_plan(s, plan, &s->timer, jm);
    s->last_passes = (int)plan.passes.size();
    s->last_jit_passes = 0;
    if (jm)
        for (hipFunction_t f : jm->fn) s->last_jit_passes += f != nullptr;
}

// ---- run sharing ----
static bool same_gates(const std::vector<qsim_gate>& a, const qsim_gate* b, size_t nb) {
    if (a.size() != nb || nb == 0) return false;
    for (size_t i = 0; i < nb; ++i) {
        const qsim_gate &x = a[i], &y = b[i];
        if (x.type != y.type || x.nqubits != y.nqubits || x.parameter != y.parameter) return false;
        for (int j = 0; j < x.nqubits && j < 3; ++j)
            if (x.qubits[j] != y.qubits[j]) return false;
    }
    return true;
}
// Pending gates are dropped (the amplitudes are about to be overwritten, or the state destroyed).
void share_discard(qsim_state* s) {
    s->last_gates.clear();
    if (!s->share) return;
    s->share->armed = false;
    s->share->calls = 0;
    s->share->next = 0;
}
// Before anything but the next identical fused run touches the amplitudes: the requested gates
// of the cycle that no launched pass held, lowered under the layout the state is in and run in
// circuit order as an ordinary fused plan.  Ends the cycle (its plan stays for the next one).
void share_flush(qsim_state* s) {
    s->last_gates.clear();
    if (!s->share || !s->share->armed) return;
    ShareState& sh = *s->share;
    const int calls = sh.calls;
    const size_t next = sh.next;
    if (sh.completed) {
        s->share_strikes = 0;
    } else {
        s->share_strikes = std::min(6, s->share_strikes + 1);
        s->share_wait = (1 << s->share_strikes) - 1;
    }
    sh.armed = false;
    sh.calls = 0;
    sh.next = 0;
    if (calls == 0) return;
    std::vector<Op> ops;
    for (int g : share_pending(sh.sp, next, calls)) {  // (src: the position in this list)
        ops.push_back(lower_gate(map_gate(s, sh.gates[(size_t)g % sh.sp.count]), s->n));
        ops.back().src = (int)ops.size() - 1;
    }
    if (ops.empty()) return;
    const int th = state_tile_height(s);
    const TileHeightScope tile_h(th, tile_rb_for(s->n, th));
    const int passes = s->last_passes, jit_passes = s->last_jit_passes;
    run_fused(s, ops);
    s->last_passes = passes;  // (qsim_state_last_run keeps describing the last qsim_run call)
    s->last_jit_passes = jit_passes;
}
// A fused run has just executed the gate list of the fused run before it: plan `copies` of it as
// one relayout plan (once per circuit), bring the state to that plan's first layout with one
// gate-free pass and arm the cycle; the next identical runs are its calls (share_call).
static void share_arm_impl(qsim_state* s, const qsim_gate* gates, size_t count) {
    const int n = s->n;
    if (s->pinned || s->share_block || !run_share_enabled(n) || !relabel_mode_on() || tile_height_is_set()) return;
    if (!s->share) s->share = std::make_unique<ShareState>();
    const int copies = run_share_copies(n);
    if (!(s->share->have || s->share->refused) || !same_gates(s->share->gates, gates, count) ||
        (s->share->have && s->share->sp.copies != copies)) {
        if (s->share->jit.mod) QSIM_HIPCHK(hipStreamSynchronize(s->stream));  // its kernels may be queued
        s->share = std::make_unique<ShareState>();
        ShareState& sh = *s->share;
        sh.gates.assign(gates, gates + count);
        sh.have = plan_share(n, gates, count, copies, (size_t)std::max(1, s->last_passes), sh.sp);
        sh.refused = !sh.have;
    }
    ShareState& sh = *s->share;
    if (!sh.have || !ensure_alt(s)) return;
    const TileHeightScope scope(6, tile_rb_for(n, 6));
    // (inline compilation compiles the joint plan's kernels here, not in the cycle's first call)
    (void)jit_for(sh.jit, sh.sp.plan, n);
    if (s->perm != sh.sp.layouts[0]) {
        const Plan move = plan_permutation_pass(n, s->perm, sh.sp.layouts[0]);
        s->stages.upload(move.stages.data(), move.stages.size() * sizeof(Stage), s->stream);
        launch_plan(s, move, &s->timer, nullptr);
        s->perm = sh.sp.layouts[0];
    }
    s->relayout = true;  // (the state keeps its second buffer)
    sh.armed = true;
    sh.completed = false;
    sh.calls = 0;
    sh.next = 0;
}
static void share_arm(qsim_state* s, const qsim_gate* gates, size_t count) {
    if (s->share_wait > 0) {  // (back-off after cycles that readers cut short)
        --s->share_wait;
        return;
    }
    // The run's own plan has been launched already: a failure here (planning, the compile, the
    // gate-free pass's launch) must not fail the run — the state stays unarmed and runs unshared.
    try {
        share_arm_impl(s, gates, count);
    } catch (const std::exception&) {
        (void)hipGetLastError();
        if (s->share) {
            s->share->armed = false;
            s->share->have = false;
            s->share->refused = true;  // (not tried again for this circuit on this state)
        }
    }
}
// One call of the armed cycle: the longest prefix of not-yet-launched joint passes whose gates
// all belong to the copies requested so far.
static void share_call(qsim_state* s) {
    ShareState& sh = *s->share;
    const TileHeightScope scope(6, tile_rb_for(s->n, 6));
    const Plan& plan = sh.sp.plan;
    const JitModule* jm = jit_for(sh.jit, plan, s->n);
    s->ops.upload(plan.ops.data(), plan.ops.size() * sizeof(TileOp), s->stream);
    s->stages.upload(plan.stages.data(), plan.stages.size() * sizeof(Stage), s->stream);
    size_t first = 0, last = 0, next = sh.next;
    int calls = sh.calls;
    const bool done = share_advance(sh.sp, calls, next, first, last);
    if (last > first) launch_plan(s, plan, &s->timer, jm, first, last);
    sh.calls = calls;  // (only now: a failed launch leaves the bookkeeping where the state is)
    sh.next = next;
    sh.completed = sh.completed || done;
    s->perm = sh.sp.layouts[done ? 0 : last];
    s->basis = false;
    s->last_passes = (int)(last - first);
    s->last_jit_passes = 0;
    for (size_t k = first; k < last && jm && k < jm->fn.size(); ++k) s->last_jit_passes += jm->fn[k] != nullptr;
}
}  // namespace qsim_hip

// Range checks of the matrix entries: every target and control in [0, n), all distinct.
static void check_qubit(int q, int n) {
    if (q < 0 || q >= n) fail(QSIM_ERR_OUT_OF_RANGE, "Qubit index " + std::to_string(q) + " out of range");
}

extern "C" {

int qsim_state_last_run(qsim_state* s, int* passes, int* jit_passes) {
    return guarded([&] {
        check_state(s);
        if (passes) *passes = s->last_passes;
        if (jit_passes) *jit_passes = s->last_jit_passes;
    });
}

int qsim_state_layout_info(qsim_state* s, int* tile_h, int* calibrated, int* relabeled) {
    return guarded([&] {
        check_state(s);
        if (tile_h) *tile_h = state_tile_height(s);
        if (calibrated) *calibrated = s->calibrated ? 1 : 0;
        if (relabeled) *relabeled = s->perm.empty() ? 0 : 1;
    });
}

int qsim_state_relayout(qsim_state* s, int* relayout) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(relayout, QSIM_ERR_INVALID_ARGUMENT, "null out");
        *relayout = s->relayout ? 1 : 0;
    });
}

int qsim_state_restore_layout(qsim_state* s) {
    return guarded([&] {
        check_state(s);
        DeviceGuard dg(s->device);
        canonicalize(s);
    });
}

int qsim_state_perm(qsim_state* s, int32_t* perm) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(perm, QSIM_ERR_INVALID_ARGUMENT, "null perm");
        for (int q = 0; q < s->n; ++q) perm[q] = s->perm.empty() ? q : s->perm[q];
    });
}

int qsim_apply_gate(qsim_state* s, const qsim_gate* g) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(g, QSIM_ERR_INVALID_ARGUMENT, "null gate");
        DeviceGuard dg(s->device);
        validate_gate(*g, s->n);
        share_flush(s);
        const Op op = lower_gate(map_gate(s, *g), s->n);
        s->basis = false;
        launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
    });
}

int qsim_run(qsim_state* s, const qsim_gate* gates, size_t count, int flags) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(gates || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        DeviceGuard dg(s->device);
        for (size_t i = 0; i < count; ++i) validate_gate(gates[i], s->n);
        const bool fused = (flags & QSIM_RUN_FUSED) != 0;
        if (s->share && s->share->armed) {
            // the armed cycle's circuit again: its next call; anything else flushes first
            if (fused && !s->share_block && same_gates(s->share->gates, gates, count)) {
                share_call(s);
                return;
            }
            share_flush(s);
        }
        // the gate list of the fused run before this one, with no reader or writer in between?
        const bool repeat = fused && same_gates(s->last_gates, gates, count);
        // First run on a basis state: choose the qubit labels (and, with cross-height calibration,
        // the tile height) for fewer passes and faster pass layouts (relabel.hip: choose_layout).
        // A state whose raw device pointer was handed out (devicePtr) is never relabeled: the
        // pointer must always see the canonical amplitudes (reference include/StateVector.cuh:
        // devicePtr() is the state itself), and a relabeled run would leave them qubit-permuted
        // there until the next index-based reader.  So pinned states run the identity layout in
        // place (no relayout plan, no second buffer, no copy-back).
        if (fused && !s->pinned && s->basis && s->perm.empty() && count > 0 &&
            (relabel_enabled(s->n) || (relayout_enabled(s->n) && relabel_mode_on() && !tile_height_is_set()))) {
            choose_first_layout(s, gates, count);
            if (!s->perm.empty() && s->basis_idx) {  // relabel the basis state itself
                uint64_t k = 0;
                for (int q = 0; q < s->n; ++q)
                    if ((s->basis_idx >> q) & 1ull) k |= 1ull << s->perm[q];
                launch_init_basis(s->d, s->n, 1, k, s->stream);
            }
        }
        const int th = state_tile_height(s);
        const TileHeightScope tile_h(th, tile_rb_for(s->n, th));  // plans of this run
        const std::vector<Op> ops = lower_gates(s->n, gates, count, s->perm);
        s->basis = false;
        if (fused) {
            run_fused(s, ops);
            if (!repeat) s->last_gates.assign(gates, gates + count);
            else share_arm(s, gates, count);
        } else {
            s->last_gates.clear();
            for (const Op& op : ops) launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
        }
    });
}

int qsim_apply_matrix1q(qsim_state* s, int target, const double m[8], const int* controls,
                        int n_controls) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(m, QSIM_ERR_INVALID_ARGUMENT, "null matrix");
        check_qubit(target, s->n);
        Op op;
        op.kind = K_M1;
        op.sub = S_GEN;
        op.t0 = target;
        for (int i = 0; i < 8; ++i) op.m[i] = m[i];
        for (int i = 0; i < n_controls; ++i) {
            const int c = controls[i];
            check_qubit(c, s->n);
            if (c == target || ((op.cmask >> c) & 1ull))
                fail(QSIM_ERR_INVALID_ARGUMENT, "control qubits must be distinct from target");
            op.cmask |= 1ull << c;
        }
        DeviceGuard dg(s->device);
        prep(s, true);
        launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
    });
}

int qsim_apply_matrix2q(qsim_state* s, int q0, int q1, const double m[32], const int* controls,
                        int n_controls) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(m, QSIM_ERR_INVALID_ARGUMENT, "null matrix");
        QSIM_REQUIRE(controls || n_controls == 0, QSIM_ERR_INVALID_ARGUMENT, "null controls");
        for (int q : {q0, q1}) check_qubit(q, s->n);
        if (q0 == q1) fail(QSIM_ERR_INVALID_ARGUMENT, "Two-qubit gate requires distinct qubits");
        uint64_t cm = 0;
        for (int i = 0; i < n_controls; ++i) {
            const int c = controls[i];
            check_qubit(c, s->n);
            if (c == q0 || c == q1 || ((cm >> c) & 1ull))
                fail(QSIM_ERR_INVALID_ARGUMENT, "control qubits must be distinct from the targets");
            cm |= 1ull << c;
        }
        DeviceGuard dg(s->device);
        prep(s, true);
        launch_matrix2q(s->d, s->n, q0, q1, m, cm, s->stream, &s->timer);
    });
}

int qsim_apply_matrix(qsim_state* s, const int* targets, int k, const double* m,
                      const int* controls, int n_controls) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(m && targets, QSIM_ERR_INVALID_ARGUMENT, "null matrix or targets");
        QSIM_REQUIRE(controls || n_controls == 0, QSIM_ERR_INVALID_ARGUMENT, "null controls");
        if (k < 1 || k > 8) fail(QSIM_ERR_INVALID_ARGUMENT, "matrix must act on 1 to 8 qubits");
        uint64_t used = 0, cm = 0;
        for (int j = 0; j < k; ++j) {
            const int q = targets[j];
            check_qubit(q, s->n);
            if ((used >> q) & 1ull) fail(QSIM_ERR_INVALID_ARGUMENT, "target qubits must be distinct");
            used |= 1ull << q;
        }
        for (int i = 0; i < n_controls; ++i) {
            const int c = controls[i];
            check_qubit(c, s->n);
            if ((used >> c) & 1ull)
                fail(QSIM_ERR_INVALID_ARGUMENT, "control qubits must be distinct from the targets");
            used |= 1ull << c;
            cm |= 1ull << c;
        }
        DeviceGuard dg(s->device);
        prep(s, true);
        const int dim = 1 << k;
        std::vector<double> mt(2 * (size_t)dim * dim);  // transpose: mt[c][r] = M[r][c]
        for (int r = 0; r < dim; ++r)
            for (int c = 0; c < dim; ++c) {
                mt[2 * ((size_t)c * dim + r)] = m[2 * ((size_t)r * dim + c)];
                mt[2 * ((size_t)c * dim + r) + 1] = m[2 * ((size_t)r * dim + c) + 1];
            }
        double2* d_mt = (double2*)s->scratch.get(mt.size() * sizeof(double), s->stream);
        QSIM_HIPCHK(hipMemcpyAsync(d_mt, mt.data(), mt.size() * sizeof(double), hipMemcpyHostToDevice,
                                   s->stream));
        launch_matrixk(s->d, s->n, targets, k, d_mt, cm, s->stream, &s->timer);
        // the matrix lives in the state's scratch: wait before the next user may reuse it
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

int qsim_apply_diagonal_layer(qsim_state* s, const double* gp, uint64_t active) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(gp || active == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate_params");
        if (s->n < 64 && (active >> s->n)) fail(QSIM_ERR_OUT_OF_RANGE, "active mask names a qubit >= n");
        std::vector<Op> ops;
        for (int q = 0; q < s->n; ++q) {
            if (!((active >> q) & 1ull)) continue;
            Op o;
            o.kind = K_DIAG;
            o.sub = S_GEN;
            o.t0 = q;
            o.m[0] = gp[8 * q + 0];
            o.m[1] = gp[8 * q + 1];
            o.m[2] = gp[8 * q + 6];
            o.m[3] = gp[8 * q + 7];
            o.d0_one = o.m[0] == 1.0 && o.m[1] == 0.0;
            o.src = (int)ops.size();
            ops.push_back(o);
        }
        DeviceGuard dg(s->device);
        prep(s, true);
        if (!ops.empty()) run_fused(s, ops);
    });
}

int qsim_apply_gate_raw(void* dstate, int n_qubits, const qsim_gate* g, void* stream) {
    return guarded([&] {
        QSIM_REQUIRE(dstate && g, QSIM_ERR_INVALID_ARGUMENT, "null argument");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40)
            fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        const Op op = lower_gate(*g, n_qubits);
        launch_op((double2*)dstate, n_qubits, 1, op, (hipStream_t)stream, nullptr);
    });
}

int qsim_apply_hadamard_optimized(void* dstate, int n_qubits, int target, void* stream) {
    qsim_gate g{};
    g.type = QSIM_GATE_H;
    g.nqubits = 1;
    g.qubits[0] = target;
    return qsim_apply_gate_raw(dstate, n_qubits, &g, stream);
}

int qsim_apply_cnot_optimized(void* dstate, int n_qubits, int control, int target, void* stream) {
    qsim_gate g{};
    g.type = QSIM_GATE_CNOT;
    g.nqubits = 2;
    g.qubits[0] = control;
    g.qubits[1] = target;
    return qsim_apply_gate_raw(dstate, n_qubits, &g, stream);
}

int qsim_apply_matrix1q_raw(void* dstate, int n_qubits, int target, const double m[8], void* stream) {
    return guarded([&] {
        QSIM_REQUIRE(dstate && m, QSIM_ERR_INVALID_ARGUMENT, "null argument");
        if (n_qubits < 1 || n_qubits > QSIM_MAX_QUBITS_SINGLE)
            fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits must be between 1 and 30");
        check_qubit(target, n_qubits);
        Op op;
        op.kind = K_M1;
        op.sub = S_GEN;
        op.t0 = target;
        for (int i = 0; i < 8; ++i) op.m[i] = m[i];
        launch_op((double2*)dstate, n_qubits, 1, op, (hipStream_t)stream, nullptr);
    });
}

}  // extern "C"
