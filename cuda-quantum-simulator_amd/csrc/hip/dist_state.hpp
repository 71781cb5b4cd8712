// dist_state.hpp — the sharded state's object (struct qsim_dist) and what the files that work on it
// share: the communicator watchdogs and the functions that cross files (file map: top of dist.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "dist_plan.hpp"

// ncclInProgress is the normal return of a non-blocking communicator (the call is queued; the
// communicator settles before the next use, comm_settle below).
#define QSIM_NCCLCHK(call)                                                              \
    do {                                                                                \
        ncclResult_t r_ = (call);                                                       \
        if (r_ != ncclSuccess && r_ != ncclInProgress)                                  \
            fail(QSIM_ERR_DEVICE, std::string("RCCL error: ") + ncclGetErrorString(r_)); \
    } while (0)

namespace qsim_hip {

// A prepared ops step (see prepare_step): its plan, kernels and the pass ranges around pivots.
struct StepRun : PassSplit {
    const Plan* plan = nullptr;
    const JitModule* jm = nullptr;
};

// One rank's share: its amplitudes and the exchange staging buffers.
struct Shard {
    int rank = 0;
    double2 *d = nullptr, *sendbuf = nullptr, *recvbuf = nullptr;
};

// The plans of one gate list from one start map, for every shard of this process (ranks differ
// only in which global controls / phases apply): what a run plan and an inverted gradient segment
// both are.  plan(rank, perm) is the planner call: it returns the rank's steps and updates perm.
struct ShardPlans {
    std::vector<qsim_gate> gates;
    std::vector<int> perm_in, perm_out;
    std::vector<std::vector<DStep>> steps;                        // per shard
    std::vector<std::vector<std::unique_ptr<PlanCache>>> fplans;  // per shard, per ops step
    bool is(const qsim_gate* g, size_t count, const std::vector<int>& perm) const {
        return perm_in == perm && gates.size() == count &&
               (count == 0 || std::memcmp(gates.data(), g, count * sizeof(qsim_gate)) == 0);
    }
    template <typename PlanFn>
    void build(const std::vector<Shard>& shards, const qsim_gate* g, size_t count, const std::vector<int>& perm,
               PlanFn&& plan) {
        gates.assign(g, g + count);
        perm_in = perm;
        for (const Shard& sh : shards) {
            perm_out = perm;
            steps.push_back(plan(sh.rank, perm_out));
            fplans.emplace_back();
            for (const DStep& s : steps.back())
                fplans.back().push_back(s.kind == 0 ? std::make_unique<PlanCache>() : nullptr);
        }
        // Every shard's plan has the same step skeleton (the planner decides from rank-independent
        // data): the walk over the steps is in lockstep.
        for (size_t i = 1; i < steps.size(); ++i) {
            if (steps[i].size() != steps[0].size()) fail(QSIM_ERR_RUNTIME, "exchange skeleton mismatch");
            for (size_t k = 0; k < steps[0].size(); ++k)
                if (steps[i][k].kind != steps[0][k].kind || steps[i][k].role != steps[0][k].role)
                    fail(QSIM_ERR_RUNTIME, "exchange skeleton mismatch");
        }
    }
};

}  // namespace qsim_hip

// Every mode runs the same per-shard code (planning per rank, pack / unpack, the slab posts of
// one remap part); only the transport that carries the posts differs:
//   T_RCCL    one shard per process, grouped ncclSend / ncclRecv over xGMI (production);
//   T_VIRTUAL all W shards in this process on one GPU (qsim_dist_create_virtual): the posts of
//             the W shards are paired by RCCL's matching rule and moved by device copies, or by
//             ncclSend / ncclRecv to rank 0 of a world-1 communicator (qsim_dist_virtual_rccl);
//   T_HOSTED  one shard per process, the posts staged through host memory and handed to a
//             caller-supplied function (qsim_dist_create_hosted: multi-process runs without RCCL,
//             e.g. several ranks on one GPU in tests).
struct qsim_dist {
    enum Transport { T_RCCL = 0, T_VIRTUAL = 1, T_HOSTED = 2 };
    int n = 0, g = 0, L = 0, world = 1, device = 0;
    bool virt = false;
    Transport transport = T_RCCL;
    qsim_dist_transport_fn host_fn = nullptr;
    void* host_ctx = nullptr;
    char* h_stage = nullptr;  // hosted: pinned staging (send half, receive half), grow-only
    size_t h_stage_bytes = 0;
    std::vector<qsim_hip::Shard> shards;
    double* d_partials = nullptr;
    double* d_result = nullptr;
    hipStream_t stream = nullptr;       // compute: passes, pack / unpack
    hipStream_t comm_stream = nullptr;  // remap transfers (RCCL or, virtual, device copies)
    hipStream_t copy_stream = nullptr;  // pack / unpack of overlapped (half) remaps
    std::vector<hipEvent_t> events;     // remap pipeline: packed part p, transferred part p
    // overlapped remap, per part h < kMaxParts: tail done (pev[h]), packed (kMaxParts + h), sent
    // (2 kMaxParts + h), unpacked (3 kMaxParts + h)
    hipEvent_t pev[4 * qsim_hip::kMaxParts] = {};
    int order[qsim_hip::kMaxParts] = {};  // exchange order of the pending overlapped remap's parts (part_order)
    int overlapped = 0;                 // remaps of the last run that overlapped local work
    ncclComm_t comm = nullptr;
    bool aborted = false;  // the communicator was aborted after an RCCL / HIP error or a timeout
    bool fresh = true;     // |0..0> with the identity map (create / reset): local labels are free
    std::vector<int> perm;
    qsim_hip::DevBuf ops, stages;
    // Plans of recent runs, keyed by (gate list, map at the start of the run): a repeated circuit
    // alternates between a few start maps, each with its own segment plans and compiled kernels.
    // Fused remap (QSIM_DIST_FUSED_PACK, default on): the last pass before an exchange stores
    // its tiles straight into the send buffer's slab layout and the step after it plans in that
    // layout, loading from the receive buffer, its last pass storing back to the standard one —
    // no pack / unpack kernels.  Per shard: the two plans, their compiled kernels, the decision.
    struct FusedVariant {
        qsim_hip::Plan plan;
        qsim_hip::JitState jit;
        bool ok = false;
    };
    struct RunPlan : qsim_hip::ShardPlans {
        uint64_t carry_in = 0;  // pivots of the previous run's exchange still in flight at the start
        bool in_use = false;    // a deferred step of this plan is pending (never evicted then)
        std::vector<std::unique_ptr<FusedVariant>> fpack, funpack;    // per shard (the first exchange)
        bool fused_decided = false;
        uint64_t used = 0;
    };
    int fused_remaps = 0;  // exchanges of the last run whose pack / unpack ran inside the passes
    // Cross-run overlap: a run whose last step is the per-part head of an overlapped remap (every
    // pass of it avoids the pivots) leaves that step pending; the next run of a circuit runs its
    // first step's leading passes per part too, interleaved with it (part h of both as soon as
    // part h has landed), so the remap also hides the next run's first passes.  Anything else
    // that touches the state runs it first (flush_carry).
    struct Carry {
        bool active = false;
        uint64_t pmask = 0;  // the remap's pivots (the run's standard positions)
        int parts = 0;
        RunPlan* rp = nullptr;
        size_t step = 0;
        std::vector<qsim_hip::StepRun> runs;
        std::vector<uint64_t> pbs;
        std::vector<double2*> homes, alts;
    } carry;
    int carried = 0;  // runs of this object whose first step merged a carried step
    std::vector<std::unique_ptr<RunPlan>> run_plans;
    uint64_t run_clock = 0;
    qsim_hip::Timer timer;
    ~qsim_dist() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        grad.reset();
        if (comm) {  // flush, bounded wait (non-blocking comm), then destroy; abort on trouble
            bool ok = ncclCommFinalize(comm) == ncclSuccess;
            if (!ok) {
                ncclResult_t st = ncclInProgress;
                const auto t0 = std::chrono::steady_clock::now();
                while (ncclCommGetAsyncError(comm, &st) == ncclSuccess && st == ncclInProgress &&
                       std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60))
                    std::this_thread::yield();
                ok = st == ncclSuccess;
            }
            if (ok) (void)ncclCommDestroy(comm);
            else (void)ncclCommAbort(comm);
        }
        for (qsim_hip::Shard& s : shards)
            for (void* p : {(void*)s.d, (void*)s.sendbuf, (void*)s.recvbuf})
                if (p) (void)hipFree(p);
        if (d_partials) (void)hipFree(d_partials);
        if (d_result) (void)hipFree(d_result);
        if (comm_stream) (void)hipStreamSynchronize(comm_stream);
        for (hipEvent_t e : events)
            if (e) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        for (hipEvent_t e : pev)
            if (e) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        if (comm_stream) (void)hipStreamDestroy(comm_stream);
        if (stream) (void)hipStreamDestroy(stream);
        if (h_stage) (void)hipHostFree(h_stage);
    }
    // this rank's remap traffic in the last run (bytes sent; the same are received)
    double sent_bytes = 0.0;
    qsim_hip::Scratch readout;  // sampling / probabilities / broadcast temporaries (dist readout entries)
    // per shard: the signed term tables of the last expectation value (dist_expect.hip)
    std::vector<std::unique_ptr<qsim_hip::DevBuf>> expect_local, expect_cross;
    // per shard: the signed angle tables of the last rotation sequence's phase runs (dist_pauli_rot.hip)
    std::vector<std::unique_ptr<qsim_hip::DevBuf>> rot_terms;
    // Adjoint-method gradients (gradient_dist): the two work shards per shard of this process, the
    // per-shard term tables of H, the (parameter, shard) slots, and the plans of the inverted
    // segments, keyed like run plans by (gate list, map at the start).  Absent until the first
    // sweep; freed by qsim_dist_gradient_release and with the object.
    struct GradWork {
        std::vector<double2*> phi, lam;
        std::vector<std::unique_ptr<qsim_hip::DevBuf>> terms;
        double* d_slots = nullptr;
        size_t slots_cap = 0;
        std::vector<std::unique_ptr<qsim_hip::ShardPlans>> segments;
        ~GradWork() {
            for (double2* p : phi)
                if (p) (void)hipFree(p);
            for (double2* p : lam)
                if (p) (void)hipFree(p);
            if (d_slots) (void)hipFree(d_slots);
        }
    };
    std::unique_ptr<GradWork> grad;
};

namespace qsim_hip {

// ---- guards and watchdogs (dist.hip) ------------------------------------------------------
void need(const qsim_dist* d);
// Entry points that touch the communicator: any RCCL / HIP failure (or a timeout) aborts it, so
// peers blocked in a collective with this rank are released instead of hanging.
template <typename F>
int dguard_comm(qsim_dist* d, F&& f) {
    const int rc = guarded(std::forward<F>(f));
    if (rc == QSIM_ERR_DEVICE && d && d->comm && !d->aborted) {
        (void)ncclCommAbort(d->comm);
        d->comm = nullptr;
        d->aborted = true;
    }
    return rc;
}
double env_seconds(const char* k, double dflt);
void comm_settle(ncclComm_t comm, const char* what, double timeout_s);
void comm_settle(qsim_dist* d, const char* what);
void stream_wait(qsim_dist* d, hipStream_t s);
// ---- transports (dist_exchange.hip) -------------------------------------------------------
// One point-to-point transfer posted by a shard: `amps` amplitudes at `send` go to rank `peer`
// and `amps` amplitudes from `peer` land at `recv` — one ncclSend / ncclRecv pair of a group on
// the multi-rank path.  Posts pair up by RCCL's rule: the k-th post of rank r naming q matches
// the k-th post of rank q naming r (and must carry the same count).
struct Post {
    int rank, peer;
    const double2* send;
    double2* recv;
    uint64_t amps;
};
void post_transfers(qsim_dist* d, const std::vector<Post>& posts, const char* what);
void host_call(qsim_dist* d, const std::vector<qsim_dist_post>& hp, const char* what);
// on: the shards to remap instead of the state's (the gradient's work states: their own
// amplitudes, the state's staging buffers); null: the state.
void exchange(qsim_dist* d, const DStep& ex, const std::vector<char>& fused, const std::vector<Shard>* on = nullptr);
void exchange_parts(qsim_dist* d, const DStep& ex, const std::vector<char>& fused);
double allreduce_sum(qsim_dist* d, double local);
void allreduce_vec(qsim_dist* d, double* d_vec, size_t count, double* h_out);
void ensure_events(qsim_dist* d, size_t count);
// ---- the run (dist_run.hip) -----------------------------------------------------------------
StepRun prepare_step(qsim_dist* d, const std::vector<Op>& ops, int flags, PlanCache& pc, uint64_t pb, uint64_t pa,
                     uint64_t cb = 0, bool head = true);
void run_part(qsim_dist* d, Shard& sh, const std::vector<Op>& ops, const StepRun& r, size_t first, size_t last,
              uint64_t pmask = 0, int part = -1, double2* home = nullptr, double2* alt = nullptr);
void flush_carry(qsim_dist* d);
void flush_on_device(qsim_dist* d);  // what an entry that touches the state does first
void run_dist(qsim_dist* d, const qsim_gate* gates, size_t count, int flags);
// ---- features, where one calls another ----------------------------------------------------
void unpermute(const qsim_dist* d, const std::vector<double2>& phys, double* dst);       // dist_readout.hip
double expectation_dist(qsim_dist* d, const qsim_pauli_term* terms, size_t count);       // dist_expect.hip
qsim_dist::GradWork& ensure_grad(qsim_dist* d, size_t nparams);                          // dist_adjoint.hip
void grad_load_work(qsim_dist* d, qsim_dist::GradWork& w, const DistApplyPlan& ap);      // dist_adjoint.hip
void grad_reduce(qsim_dist* d, qsim_dist::GradWork& w, size_t P, double* out);           // dist_adjoint.hip

}  // namespace qsim_hip
