// dist_plan.hpp — the sharded state's remap planner and slab layout: host-only, no device handle,
// no communicator.  dist_plan.hip defines it; the run, the transports and the host-only C entries
// (which the CPU tests drive) all read the plan through these declarations.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <exception>
#include <vector>

#include "engine.hpp"
#include "state.hpp"
#include "qsim_hip.h"

namespace qsim_hip {

struct DStep {
    int kind = 0;  // 0 ops, 1 exchange
    int k = 0;
    int gpos[8] = {0}, lpos[8] = {0};
    std::vector<Op> ops;
    // Overlap of a remap with local work (mark_overlap): an exchange with pivots (pmask != 0, up
    // to kMaxPivots local physical positions) runs as 2^m part-exchanges, one per value of the
    // pivot bits.  An ops step with role bit 1 runs the trailing passes of its fused plan that
    // avoid the pivots of the exchange after it per part (so part j's transfer overlaps the later
    // parts' passes); role bit 2: the leading passes that avoid the pivots of the exchange before
    // it run per part, each as soon as its part has landed.  The step's plan is the same one-piece
    // fused plan either way (no extra passes).  `pivot`: the lowest pivot (-1: none).
    int pivot = -1, role = 0;
    uint64_t pmask = 0;
    // Coarse parts (round 5; exchange steps): a subset of pmask that the step before's passes just
    // ahead of its per-part tail leave untouched.  Those passes (which do touch the other pivots)
    // run per value of these bits, each coarse part followed at once by the tail of its fine parts,
    // so the first part can leave after 1/2^|coarse| of them instead of after all of them.  Parts
    // are exchanged in coarse-major order (part_order).  0: none.
    uint64_t coarse = 0;
    // planning only: the circuit gates emitted into this step (rank-independent), their physical
    // qubit masks, and for each op the index of the gate (in this list) it came from
    std::vector<uint64_t> gmask;
    std::vector<int> op_gate;
};

constexpr int kMaxPivots = 4;
constexpr int kMaxParts = 1 << kMaxPivots;  // part-exchanges of one overlapped remap

bool carry_enabled();  // QSIM_DIST_CARRY
// Whether pass p can run per part of pivots pmask: a tile pass of 4 free bits or more that touches
// none of them.
bool pass_avoids(const FusedPass& p, uint64_t pmask);
uint64_t deposit_bits(uint64_t v, uint64_t mask);  // bit j of v -> j-th set bit of mask
void part_order(uint64_t pmask, uint64_t cb, int* order);  // kMaxParts entries at most
// Part count of an overlapped remap with pivot mask pmask; the event array pev holds kMaxParts
// slots per kind, so a larger count is a planner bug, reported instead of overrunning it (round 4:
// a segfault when the pivot limit rose to 4 while pev still had 8 slots per kind).
int part_count(uint64_t pmask);
// The split of an ops step's fused plan around the remaps next to it (pb: pivots of the exchange
// before it, pa: of the one after, cb: the coarse bits among pa).  The plan is the step's ordinary
// fused plan with tiles padded away from the pivots, so the split costs no extra HBM pass:
//   head   [0, j1)   passes that avoid pb: per part, each after its part of the exchange has landed;
//   middle [j1, jc)  whole shard, after every part has landed;
//   coarse [jc, j2)  passes that avoid cb: per coarse part, each followed by its fine parts' tails;
//   tail   [j2, np)  passes that avoid pa: per part, each followed by the event its part waits for.
// A pass counts once: head first, then tail.  head_runs: parts are pending, so the head does run
// per part and the coarse passes end at j1; else its passes run whole and may be coarse ones.
struct PassSplit { size_t j1 = 0, j2 = 0, jc = 0, np = 0; };
PassSplit split_passes(const Plan& pl, uint64_t pb, uint64_t pa, uint64_t cb, bool head_runs);
// The pivots a run with step skeleton `st` leaves in flight for the next run, or 0: its last step is
// the per-part head of its last remap and no tail.  Skeleton only, so the same on every rank.
uint64_t carried_pivots(const std::vector<DStep>& st);
// Host plan of one run for one rank, from map `perm` (updated to the run's end map): plan_dist_core
// without overlap marks, plan_dist with them (carry: the pivots still in flight at the start).
std::vector<DStep> plan_dist_core(const qsim_gate* gates, size_t count, int n, int g, int rank, std::vector<int>& perm);
std::vector<DStep> plan_dist(const qsim_gate* gates, size_t count, int n, int g, int rank, std::vector<int>& perm,
                             uint64_t carry = 0);
// The slab layout of exchange `ex` as a permutation of the local positions (the inverse of
// xlocal): positions outside lpos and the pivots ascending -> 0 .. L-k-m-1, lpos[j] -> L-m-k+j,
// the pivots ascending -> L-m .. L-1.  Part h of slab c is then the contiguous block at
// h * 2^(L-m) + c * 2^(L-m-k) of the send / receive buffers.
std::vector<int> slab_sigma(int L, const DStep& ex);

// ---- slab layout of an exchange ------------------------------------------------------------
struct XArgs {
    double2* st;
    double2* buf;
    uint64_t chunk;     // 2^(L-k) amplitudes
    int chunk_log;
    int k;
    int my_c;
    int nsorted;        // zero-insertion positions: lpos, plus the pivots of a part exchange
    int sorted[12];     // ascending
    int lpos[8];        // chunk bit j <-> lpos[j]
    uint64_t orval;     // part exchange: the pivot bits' values
};

// Local amplitude index of element e of the slab buffer (slab c = e >> chunk_log): the offset's
// bits are spread around the zero-inserted positions, then slab bits go to lpos and the part's
// pivot values are or-ed in.  Host and device: qsim_dist_slab_map exports the same map.
__host__ __device__ __forceinline__ uint64_t xlocal(const XArgs& a, uint64_t e) {
    const uint64_t c = e >> a.chunk_log;
    uint64_t off = e & (a.chunk - 1);
#pragma unroll
    for (int j = 0; j < 12; ++j)
        if (j < a.nsorted) {
            const uint64_t lo = off & ((1ull << a.sorted[j]) - 1ull);
            off = ((off ^ lo) << 1) | lo;
        }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < a.k) off |= ((c >> j) & 1ull) << a.lpos[j];
    return off | a.orval;
}

// The slab layout of one remap (or one part of an overlapped remap) on one rank: the pack /
// unpack map (XArgs) and the rank each slab goes to and comes from.  Host-only and rank-local;
// qsim_dist_slab_map exports it for the CPU tests.
struct XPlan {
    XArgs a;
    int peer_of[256];
};
// part < 0: the whole shard; part j: the amplitudes whose pivot bits hold the bits of j.
XPlan xplan(int L, int rank, const DStep& ex, int part = -1);

// ---- the C entries' prologues (their guard: state.hpp guarded) ---------------------------------
int log2_exact(int w);
void check_sizes(int n, int g);
std::vector<int> checked_perm(int n, const int32_t* perm);  // null: the identity
// Prologue of the host-only plan entries: world -> g, the size and rank checks, and the map the
// plan starts from (perm_inout, null: the identity), written back by store().
struct HostPlanArgs {
    int g, L;
    std::vector<int> perm;
    HostPlanArgs(int n, int world, int rank = 0, const int32_t* perm_inout = nullptr);
    void store(int32_t* perm_inout) const {
        if (perm_inout) std::copy(perm.begin(), perm.end(), perm_inout);
    }
};
}  // namespace qsim_hip
