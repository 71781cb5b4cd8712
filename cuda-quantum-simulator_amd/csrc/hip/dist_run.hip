// dist_run.hip — one run of a circuit on the sharded state (dist.hip): its plans per shard, each ops
// step split around its remaps, the fused remap, the carried step and the walk over the steps (run_dist).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "device_ops.hpp"
#include "dist_state.hpp"

namespace qsim_hip {

// One ops step on one shard: its fused plan, kernels and the split of its passes around the
// neighbouring exchanges (split_passes).  Per-gate mode (or an empty step) has no plan and runs whole.
StepRun prepare_step(qsim_dist* d, const std::vector<Op>& ops, int flags, PlanCache& pc, uint64_t pb, uint64_t pa,
                     uint64_t cb, bool head) {
    if (ops.empty() || !(flags & QSIM_RUN_FUSED)) return StepRun();
    PlanCache::Entry& pe = pc.get(ops, d->L, d->stream, pa, pb);
    return StepRun{split_passes(pe.plan, pb, pa, cb, head), &pe.plan, jit_for(pe.jit, pe.plan, d->L)};
}
// Launch passes [first, last) of a prepared step (part >= 0: the part whose pivot bits `pmask`
// hold the bits of part); per-gate mode: the whole op list when called for the middle part.
// home / alt: where the step's passes read, and where a relayout pass (fused remap) writes
// (null: the shard's state, no second buffer).
void run_part(qsim_dist* d, Shard& sh, const std::vector<Op>& ops, const StepRun& r, size_t first,
              size_t last, uint64_t pmask, int part, double2* home, double2* alt) {
    if (ops.empty() || first >= last) return;
    if (!r.plan) {
        for (const Op& op : ops) launch_op(sh.d, d->L, 1, op, d->stream, &d->timer);
        return;
    }
    d->ops.upload(r.plan->ops.data(), r.plan->ops.size() * sizeof(TileOp), d->stream);
    d->stages.upload(r.plan->stages.data(), r.plan->stages.size() * sizeof(Stage), d->stream);
    FusedRange rg;
    rg.first = first;
    rg.last = last;
    rg.alt = alt;
    if (part >= 0) {
        rg.fix_mask = pmask;
        rg.fix_val = deposit_bits((uint64_t)part, pmask);
    }
    launch_fused(home ? home : sh.d, d->L, 1, *r.plan, (const TileOp*)d->ops.ptr, (const Stage*)d->stages.ptr,
                 d->stream, &d->timer, r.jm, nullptr, rg);
}

static bool fused_pack_enabled() {
    const char* e = std::getenv("QSIM_DIST_FUSED_PACK");  // (read per run: tests switch it)
    return e == nullptr || std::atoi(e) != 0;
}
static Op map_op_positions(Op op, const std::vector<int>& sg) {
    op.t0 = sg[op.t0];
    if (op.kind == K_SWAP) op.t1 = sg[op.t1];
    uint64_t cm = 0;
    for (uint64_t m = op.cmask; m; m &= m - 1) cm |= 1ull << sg[__builtin_ctzll(m)];
    op.cmask = cm;
    return op;
}
// Per shard, whether the first exchange of run plan `rp` runs fused (steps [A, X, B] at the
// start of the run, fused ops plans on both sides; exchanged positions below 6 only cost the
// storing pass some coalescing: its lanes are the tile bits with the lowest store positions),
// and the two plans: A's with its last pass storing into
// the slab layout, B's planned on positions sigma(p) (the receive buffer's layout) with its last
// pass storing back to the standard positions.  The slab layout is the unfused exchange's, so
// shards decide independently.
// The variants are built the first time a run of this plan may use them (fused mode, fused pack
// on); whether a run uses them is decided per run from its own flags (fused_now), so a per-gate
// run of a cached plan never runs them and a fused run after a per-gate one still gets them.
static bool fused_now(int flags) {
    return (flags & QSIM_RUN_FUSED) && fused_pack_enabled();
}
static void decide_fused(qsim_dist* d, qsim_dist::RunPlan& rp, int flags) {
    const size_t S = d->shards.size();
    rp.fpack.resize(S);
    rp.funpack.resize(S);
    if (rp.fused_decided || !fused_now(flags)) return;
    rp.fused_decided = true;
    const std::vector<DStep>& st0 = rp.steps[0];
    if (st0.size() < 3 || st0[0].kind != 0 || st0[1].kind != 1 || st0[2].kind != 0 || (st0[2].role & 1))
        return;
    const DStep& ex = st0[1];
    if (ex.pmask & 0x3full) return;  // (pivots are >= 6 by construction)
    const std::vector<int> sg = slab_sigma(d->L, ex);
    std::vector<int> inv(d->L);
    for (int p = 0; p < d->L; ++p) inv[sg[p]] = p;
    uint64_t pm_sigma = 0;
    for (uint64_t m = ex.pmask; m; m &= m - 1) pm_sigma |= 1ull << sg[__builtin_ctzll(m)];
    for (size_t i = 0; i < S; ++i) {
        const DStep& A = rp.steps[i][0];
        const DStep& B = rp.steps[i][2];
        if (A.ops.empty() || B.ops.empty()) continue;
        auto pk = std::make_unique<qsim_dist::FusedVariant>();
        auto up = std::make_unique<qsim_dist::FusedVariant>();
        try {
            const uint64_t pa = (A.role & 1) ? ex.pmask : 0ull;
            const uint64_t pb = (A.role & 2) ? rp.carry_in : 0ull;
            pk->plan = plan_fused(A.ops, d->L, -1, pa, pb);
            const FusedPass& la = pk->plan.passes.back();
            if (la.single >= 0 || la.h < 4) continue;
            relayout_last_pass(pk->plan, d->L, sg.data());
            std::vector<Op> bops;
            for (const Op& op : B.ops) bops.push_back(map_op_positions(op, sg));
            up->plan = plan_fused(bops, d->L, -1, 0ull, (B.role & 2) ? pm_sigma : 0ull);
            const FusedPass& lb = up->plan.passes.back();
            if (lb.single >= 0 || lb.h < 4) continue;
            relayout_last_pass(up->plan, d->L, inv.data());
        } catch (const Error&) {
            continue;  // (this shard keeps the pack / unpack kernels)
        }
        pk->ok = up->ok = true;
        rp.fpack[i] = std::move(pk);
        rp.funpack[i] = std::move(up);
    }
}
static StepRun prepare_variant(qsim_dist* d, qsim_dist::FusedVariant& v, uint64_t pb, uint64_t pa, uint64_t cb,
                               bool head) {
    return StepRun{split_passes(v.plan, pb, pa, cb, head), &v.plan, jit_for(v.jit, v.plan, d->L)};
}
// The cached plan of this run (same gates, same start map, same carry), or a new one (LRU of 8).
static qsim_dist::RunPlan& run_plan(qsim_dist* d, const qsim_gate* gates, size_t count, uint64_t carry) {
    for (auto& rp : d->run_plans)
        if (rp->carry_in == carry && rp->is(gates, count, d->perm)) {
            rp->used = ++d->run_clock;
            return *rp;
        }
    auto rp = std::make_unique<qsim_dist::RunPlan>();
    rp->carry_in = carry;
    rp->build(d->shards, gates, count, d->perm, [&](int rank, std::vector<int>& perm) {
        return plan_dist(gates, count, d->n, d->g, rank, perm, carry);
    });
    rp->used = ++d->run_clock;
    if (d->run_plans.size() >= 8) {
        auto lru = std::min_element(d->run_plans.begin(), d->run_plans.end(), [](const auto& a, const auto& b) {
            return a->in_use != b->in_use ? !a->in_use : a->used < b->used;  // (a pending step's plan stays)
        });
        QSIM_HIPCHK(hipStreamSynchronize(d->stream));  // its compiled kernels may still be queued
        d->run_plans.erase(lru);
    }
    d->run_plans.push_back(std::move(rp));
    return *d->run_plans.back();
}
// The carried step on shard i: part h of its head, or (h < 0) its passes past the head, whole.
static void run_carried(qsim_dist* d, size_t i, int h) {
    const qsim_dist::Carry& c = d->carry;
    const StepRun& r = c.runs[i];
    if (!r.plan) return;
    const std::vector<Op>& ops = c.rp->steps[i][c.step].ops;
    if (h >= 0) run_part(d, d->shards[i], ops, r, 0, r.j1, c.pbs[i], h, c.homes[i], c.alts[i]);
    else run_part(d, d->shards[i], ops, r, r.j1, r.np, 0, -1, c.homes[i], c.alts[i]);
}
static void carry_done(qsim_dist* d) {
    d->carry.active = false;
    d->carry.rp->in_use = false;
    d->carry.rp = nullptr;
}
// Run the carried step (the per-part head of the previous run's last remap) now, part by part as
// each part lands; every entry that touches the state, or a run that cannot merge it, calls this.
// A shard whose carried step has passes that touch the pivots (j1 < np: its lowering differs from
// rank 0's, e.g. gates dropped by a global control) runs those whole once every part has landed.
void flush_carry(qsim_dist* d) {
    const qsim_dist::Carry& c = d->carry;
    if (!c.active) return;
    if (c.parts > kMaxParts) fail(QSIM_ERR_RUNTIME, "carried remap with too many parts");
    for (int oi = 0; oi < c.parts; ++oi) {
        const int h = d->order[oi];
        QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->pev[3 * kMaxParts + h], 0));
        for (size_t i = 0; i < d->shards.size(); ++i) run_carried(d, i, h);
    }
    for (size_t i = 0; i < d->shards.size(); ++i) run_carried(d, i, -1);
    carry_done(d);
}
void flush_on_device(qsim_dist* d) {
    QSIM_HIPCHK(hipSetDevice(d->device));
    flush_carry(d);  // (the previous run's last step, if it was left pending)
    QSIM_HIPCHK(hipSetDevice(d->device));
}

void run_dist(qsim_dist* d, const qsim_gate* gates, size_t count, int flags) {
    if ((flags & QSIM_RUN_FUSED) && d->fresh && count > 0 && relabel_enabled(d->L)) {
        // Layout-aware relabeling of the LOCAL positions (relabel.hip): |0..0> stays |0..0>
        // under any relabeling, so the map is free to choose now.  Decided from rank 0's plan,
        // which every rank can compute, so all ranks pick the same map (the exchanges need
        // identical positions everywhere).  Global positions are untouched.
        std::vector<int> p0 = d->perm;
        const std::vector<DStep> st0 = plan_dist(gates, count, d->n, d->g, 0, p0);
        std::vector<uint64_t> tiles;
        for (const DStep& st : st0)
            if (st.kind == 0 && !st.ops.empty())
                for (uint64_t t : plan_tiles(plan_fused(st.ops, d->L))) tiles.push_back(t);
        double before = 0.0, after = 0.0;
        const std::vector<int> pi = choose_relabel(tiles, d->L, &before, &after);
        if (!pi.empty())
            for (int q = 0; q < d->n; ++q)
                if (d->perm[q] < d->L) d->perm[q] = pi[d->perm[q]];
    }
    d->fresh = false;
    d->sent_bytes = 0.0;
    const bool carry_on = carry_enabled();
    if (!(flags & QSIM_RUN_FUSED) || !carry_on) flush_carry(d);
    const uint64_t carry_in = d->carry.active ? d->carry.pmask : 0ull;
    qsim_dist::RunPlan& rp = run_plan(d, gates, count, carry_in);
    const auto& plans = rp.steps;
    const size_t S = d->shards.size();
    // merge the carried step into this run's first one (its leading passes per part too)
    const bool merge = d->carry.active && !plans[0].empty() && plans[0][0].kind == 0 && (plans[0][0].role & 2);
    if (!merge) flush_carry(d);
    d->overlapped = 0;
    d->fused_remaps = 0;
    decide_fused(d, rp, flags);
    std::vector<char> fused(S, 0);  // per shard: the first exchange runs fused
    for (size_t i = 0; i < S; ++i) fused[i] = fused_now(flags) && rp.fpack[i] && rp.fpack[i]->ok;
    const std::vector<char> unfused(S, 0);
    static const bool dbg = std::getenv("QSIM_DIST_DEBUG") != nullptr;
    if (dbg) {  // the exchange skeleton this run executes (kind, k, pivot mask, role)
        std::string line = "[dist] rank " + std::to_string(d->shards[0].rank) + " perm_in";
        for (int q = 0; q < d->n; ++q) line += " " + std::to_string(rp.perm_in[q]);
        line += " |";
        for (const DStep& st : plans[0])
            line += st.kind == 1 ? " X" + std::to_string(st.k) + ":" + std::to_string(st.pmask)
                                 : " O" + std::to_string(st.ops.size()) + "r" + std::to_string(st.role);
        std::fprintf(stderr, "%s\n", line.c_str());
    }
    int pending = merge ? d->carry.parts : 0;  // parts of an overlapped remap still to be waited for
    if (merge) ++d->carried;
    auto wait_pending = [&]() {
        if (pending > kMaxParts) fail(QSIM_ERR_RUNTIME, "pending remap with too many parts");
        for (int oi = 0; oi < pending; ++oi)
            QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->pev[3 * kMaxParts + d->order[oi]], 0));
        pending = 0;
    };
    // Every rank's plan has the same step skeleton (checked when the plan was built): walk the
    // steps in lockstep.
    for (size_t k = 0; k < plans[0].size(); ++k) {
        const DStep& s0 = plans[0][k];
        if (s0.kind == 1) {
            const std::vector<char>& fz = k == 1 ? fused : unfused;
            for (char f : fz) d->fused_remaps += f ? 1 : 0;
            if (s0.pmask) {
                // the ops step before (role bit 1) recorded pev[j] after its tail part j;
                // otherwise every part is ready now
                const int K = part_count(s0.pmask);
                wait_pending();
                if (k == 0 || !(plans[0][k - 1].role & 1))
                    for (int h = 0; h < K; ++h) QSIM_HIPCHK(hipEventRecord(d->pev[h], d->stream));
                exchange_parts(d, s0, fz);
                pending = K;
                ++d->overlapped;
            } else {
                wait_pending();
                exchange(d, s0, fz);
            }
            continue;
        }
        // ops step: head per half (after the exchange before), middle, tail per half
        const uint64_t pb = (s0.role & 2) ? (k == 0 ? carry_in : plans[0][k - 1].pmask) : 0ull;
        const uint64_t pa = (s0.role & 1) ? plans[0][k + 1].pmask : 0ull;
        // coarse parts (DStep::coarse, rank-independent): this shard's passes just ahead of its
        // tail that avoid the coarse bits run per coarse part, each followed by the tails of its
        // fine parts, in the exchange's part order
        const uint64_t cb = pa ? (plans[0][k + 1].coarse & pa) : 0ull;
        const bool head = pb && pending;
        std::vector<StepRun> runs(S);
        // fused first exchange: step 0 stores its last pass into the send buffer (slab
        // layout), step 2 reads the receive buffer in that layout (pivots at sigma's top
        // positions) and stores its last pass back to the state
        std::vector<uint64_t> pbs(S, pb);
        std::vector<double2*> homes(S, nullptr), alts(S, nullptr);
        for (size_t i = 0; i < S; ++i) {
            if (fused[i] && k == 0) {
                runs[i] = prepare_variant(d, *rp.fpack[i], pb, pa, cb, head);
                alts[i] = d->shards[i].sendbuf;
            } else if (fused[i] && k == 2) {
                const std::vector<int> sg = slab_sigma(d->L, plans[0][1]);
                uint64_t ps = 0;
                for (uint64_t m = pb; m; m &= m - 1) ps |= 1ull << sg[__builtin_ctzll(m)];
                pbs[i] = ps;
                runs[i] = prepare_variant(d, *rp.funpack[i], ps, 0, 0, head);
                homes[i] = d->shards[i].recvbuf;
                alts[i] = d->shards[i].d;
            } else {
                runs[i] = prepare_step(d, plans[i][k].ops, flags, *rp.fplans[i][k], pb, pa, cb, head);
            }
        }
        // the run's last step, the per-part head of the run's last remap: leave it pending (the
        // next run merges it into its first step's head; anything else flushes it).  Decided on
        // the step skeleton alone (roles, pivots: the same on every rank), never on this rank's
        // own passes — the next run plans its pivots with the carried ones (carry_in), so ranks
        // that decided differently would plan different part counts for the same exchange
        // (round 5 required every shard's step to lie wholly in the head; at world 8 / 20 qubits
        // some shards' lowerings differ from rank 0's — gates dropped by a global control — so
        // no run ever carried, and separate rank processes could have disagreed).  A shard whose
        // step has passes that touch the pivots runs them whole after the last part (flush_carry
        // and the merged head below).
        if (head && carry_on && k + 1 == plans[0].size() && carried_pivots(plans[0]) && (flags & QSIM_RUN_FUSED) &&
            !(k == 0 && merge)) {
            d->carry = qsim_dist::Carry{true, pb, pending, &rp, k, runs, pbs, homes, alts};
            rp.in_use = true;
            pending = 0;
            continue;
        }
        // passes [first, last) of this step on shard i, if it has a plan (h < 0: the whole shard)
        auto launch = [&](size_t i, size_t first, size_t last, uint64_t mask, int h) {
            if (runs[i].plan)
                run_part(d, d->shards[i], plans[i][k].ops, runs[i], first, last, mask, h, homes[i], alts[i]);
        };
        if (head) {
            const bool carried = k == 0 && merge;
            const qsim_dist::Carry& c = d->carry;
            // a shard whose carried step is partial (see flush_carry) interleaves nothing: its
            // carried head per part, then after the last part the rest of that step whole and
            // this step's head whole
            auto partial = [&](size_t i) { return carried && c.runs[i].plan && c.runs[i].j1 < c.runs[i].np; };
            if (pending > kMaxParts) fail(QSIM_ERR_RUNTIME, "pending remap with too many parts");
            for (int oi = 0; oi < pending; ++oi) {
                const int h = d->order[oi];
                QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->pev[3 * kMaxParts + h], 0));
                if (carried)  // part h of the previous run's last step, then part h of this one
                    for (size_t i = 0; i < S; ++i) run_carried(d, i, h);
                for (size_t i = 0; i < S; ++i)
                    if (!partial(i)) launch(i, 0, runs[i].j1, pbs[i], h);
            }
            if (carried) {
                for (size_t i = 0; i < S; ++i)
                    if (partial(i)) {
                        run_carried(d, i, -1);
                        launch(i, 0, runs[i].j1, 0, -1);
                    }
                carry_done(d);
            }
        }
        wait_pending();
        for (size_t i = 0; i < S; ++i) {
            if (runs[i].plan) launch(i, head ? runs[i].j1 : 0, runs[i].jc, 0, -1);
            else run_part(d, d->shards[i], plans[i][k].ops, runs[i], 0, 1);  // per-gate: the whole list
        }
        if (pa) {  // the exchange after waits for pev[h]
            const int K = part_count(pa), Kc = 1 << __builtin_popcountll(cb), Kf = K / Kc;
            int ord[kMaxParts];
            part_order(pa, cb, ord);
            for (int cv = 0; cv < Kc; ++cv) {
                if (cb)
                    for (size_t i = 0; i < S; ++i) launch(i, runs[i].jc, runs[i].j2, cb, cv);
                for (int f = 0; f < Kf; ++f) {
                    const int h = ord[cv * Kf + f];
                    for (size_t i = 0; i < S; ++i) launch(i, runs[i].j2, runs[i].np, pa, h);
                    QSIM_HIPCHK(hipEventRecord(d->pev[h], d->stream));
                }
            }
        }
    }
    wait_pending();
    d->perm = rp.perm_out;
}

}  // namespace qsim_hip
