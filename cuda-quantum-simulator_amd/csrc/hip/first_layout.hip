// first_layout.hip — the layout of a state's first fused run: the qubit labels (s->perm), with
// cross-height calibration the tile height (s->tile_h), and whether the run is a relayout plan
// (relayout.hip).  Policy only: the planners are relabel.hip and relayout.hip, the decisions are
// memoised by cache.hip, and candidates are timed on the device by calibrate_candidates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

#include "state.hpp"

namespace qsim_hip {

// Time every candidate with its own circuit-specialised kernels on this device (each candidate's
// whole plan under its own tile height, the faster of two runs, the basis state restored after
// each) and return the fastest: the cost model ranks layouts from probes of other boxes, real
// pass times differ by a few per cent between devices, and whether 13-qubit tiles (fewer passes,
// slower streaming) beat 12-qubit ones depends on the circuit.  The plans stay cached
// (compiled).
size_t calibrate_candidates(qsim_state* s, std::vector<LayoutCandidate>& cands) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    QSIM_HIPCHK(hipEventCreate(&e0));
    QSIM_HIPCHK(hipEventCreate(&e1));
    size_t best = 0;
    float best_ms = 3.0e38f;
    try {
        for (size_t k = 0; k < cands.size(); ++k) {
            LayoutCandidate& c = cands[k];
            const TileHeightScope scope(c.h, tile_rb_for(s->n, c.h));
            s->plans.put(c.ops, s->n, c.plan, s->stream);
            PlanCache::Entry& pe = s->plans.get(c.ops, s->n, s->stream);
            const JitModule* jm = jit_for(pe.jit, pe.plan, s->n);
            s->ops.upload(pe.plan.ops.data(), pe.plan.ops.size() * sizeof(TileOp), s->stream);
            s->stages.upload(pe.plan.stages.data(), pe.plan.stages.size() * sizeof(Stage), s->stream);
            float ms = 3.0e38f;
            const int reps = s->n < 26 ? 5 : 2;  // (short runs: more repetitions against noise)
            for (int rep = 0; rep < reps; ++rep) {
                QSIM_HIPCHK(hipEventRecord(e0, s->stream));
                launch_plan(s, pe.plan, nullptr, jm);
                QSIM_HIPCHK(hipEventRecord(e1, s->stream));
                QSIM_HIPCHK(hipEventSynchronize(e1));
                float t = 0.0f;
                QSIM_HIPCHK(hipEventElapsedTime(&t, e0, e1));
                ms = std::min(ms, t);
            }
            launch_init_basis(s->d, s->n, 1, s->basis_idx, s->stream);  // the state as it was
            static const bool dbg = std::getenv("QSIM_RELABEL_DEBUG") != nullptr;
            if (dbg)
                std::fprintf(stderr, "[calibrate] candidate %zu (h=%d, %zu passes): %.3f ms per run\n", k, c.h,
                             pe.plan.passes.size(), ms);
            if (ms < best_ms) {
                best = k;
                best_ms = ms;
            }
        }
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        // a candidate may have run partway: put the basis state back (best effort) or, if even
        // that fails, stop treating the amplitudes as that basis state (no relabeling later)
        try {
            launch_init_basis(s->d, s->n, 1, s->basis_idx, s->stream);
            QSIM_HIPCHK(hipStreamSynchronize(s->stream));
        } catch (...) {
            s->basis = false;
        }
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    return best;
}

namespace {
// What every step of one first-run choice reads.
struct FirstRun {
    qsim_state* s;
    const qsim_gate* gates;
    size_t count;
    int n;
    size_t bytes;   // of the gate list: the memo key
    bool heights;   // cross-height calibration: the tile height is chosen too
    int th;         // the state's tile height going in
    bool relayout;  // relayout plans are candidates (and the second buffer exists)
    bool timing;    // candidates are timed on the device
    std::vector<Op> lower(const std::vector<int>& pi) const { return lower_gates(n, gates, count, pi); }
    // a fixed-layout decision (a single-height one is keyed by its height)
    void memo_put(const std::vector<int>& perm) const {
        const TileHeightScope scope(th);
        layout_memo_put(n, 0, gates, bytes, perm, heights ? s->tile_h : -1);
    }
    void memo_no_relayout() const { layout_memo_put(n, 2, gates, bytes, {}, -1); }
};

// The relayout variants of the circuit (12-qubit tiles, every pass stores under the next pass's
// layout), planned on a worker thread while the fixed-layout candidates are chosen; join() where
// the result is first needed.  best: the best predicted variant (timing compares all of them).
struct RelayoutWorker {
    RelayoutChoice best;
    std::vector<RelayoutChoice> all;
    bool have = false;
    std::thread t;
    void start(const FirstRun& c) {
        t = std::thread([this, &c] {
            try {
                const TileHeightScope scope(6, tile_rb_for(c.n, 6));
                have = plan_relayout_variants(
                           c.n, [&c](const std::vector<int>& pi) { return c.lower(pi); }, SIZE_MAX, all) > 0;
                if (have) best = all.front();
            } catch (...) {
                have = false;  // (no relayout candidate)
            }
        });
    }
    void join() {
        if (t.joinable()) t.join();
    }
    ~RelayoutWorker() { join(); }
};

// The state takes a relayout plan: cached, its labels kept and the decision memoised.
void take_relayout(const FirstRun& c, const std::vector<int>& perm, const std::vector<Op>& ops, Plan plan) {
    qsim_state* s = c.s;
    {
        const TileHeightScope scope(6, tile_rb_for(c.n, 6));
        s->plans.put(ops, c.n, std::move(plan), s->stream);
    }
    s->perm = perm;
    s->tile_h = 6;
    s->relayout = true;
    layout_memo_put(c.n, 2, c.gates, c.bytes, s->perm, c.timing ? 6 : -1);
}
void take_relayout(const FirstRun& c, RelayoutChoice& rc) { take_relayout(c, rc.perm, rc.ops, std::move(rc.plan)); }
// (a timed winner: re-put, the timing loop may have evicted it)
void take_relayout(const FirstRun& c, const LayoutCandidate& w) { take_relayout(c, w.perm, w.ops, w.plan); }

void add_candidate(std::vector<LayoutCandidate>& cands, int h, std::vector<int> perm, std::vector<Op> ops,
                   Plan plan, bool rl = false) {
    for (const LayoutCandidate& c : cands)
        if (c.h == h && c.perm == perm && c.relayout == rl) return;  // the same candidate twice
    cands.push_back(LayoutCandidate{h, std::move(perm), std::move(ops), std::move(plan), rl});
}

// A relayout choice made before for this circuit (by timing, or by pass count when candidates are
// not timed: memoised apart).  True: decided.
bool relayout_memo_decides(const FirstRun& c) {
    qsim_state* s = c.s;
    std::vector<int> memo;
    int mh = -1;
    if (!layout_memo_get(c.n, 2, c.gates, c.bytes, memo, c.timing ? &mh : nullptr) ||
        (memo.empty() && relayout_forced()))
        return false;
    if (memo.empty()) return true;  // (decided: no relayout plan, and no relabeling below)
    std::vector<RelayoutChoice> vs;
    plan_relayout_variants(c.n, [&c](const std::vector<int>& pi) { return c.lower(pi); }, SIZE_MAX, vs);
    for (RelayoutChoice& rc : vs) {
        if (rc.perm != memo) continue;
        const TileHeightScope scope(6, tile_rb_for(c.n, 6));
        s->plans.put(rc.ops, c.n, std::move(rc.plan), s->stream);
        s->perm = memo;
        s->tile_h = 6;
        s->relayout = true;
        s->calibrated = c.timing;
        return true;
    }
    return false;
}

// A fixed-layout choice made before for this circuit (its plan: the plan cache).  True: decided.
bool layout_memo_decides(const FirstRun& c) {
    qsim_state* s = c.s;
    std::vector<int> memo;
    int mh = -1;
    const TileHeightScope scope(c.th);
    // (a forced relayout plan does not take a fixed-layout decision made before)
    if (relayout_forced() || !layout_memo_get(c.n, 0, c.gates, c.bytes, memo, c.heights ? &mh : nullptr))
        return false;
    s->perm = memo;
    if (c.heights) s->tile_h = mh;
    s->calibrated = c.heights;  // (a cross-height decision is always a timed one)
    return true;
}

// States below the relabeling threshold: relayout only, taken when it needs fewer passes than
// the circuit's plan under the identity labels.
void choose_relayout_only(const FirstRun& c, RelayoutWorker& rw) {
    qsim_state* s = c.s;
    if (!c.relayout) return;  // (no room for the second buffer: nothing to decide, no memo)
    rw.join();
    std::vector<Op> ops0 = c.lower({});
    Plan p0;
    {
        const TileHeightScope scope(c.th, tile_rb_for(c.n, c.th));
        p0 = plan_fused(ops0, c.n, c.th);
    }
    // with inline compilation (the bench's mode) the identity-label plan and the relayout
    // variants are timed on the device, as at the first run of larger states
    static const bool time_small = env_switch("QSIM_RELAYOUT_TIME_SMALL", true);
    if (rw.have && !relayout_forced() && time_small && jit_mode() == 2 && calibrate_mode_on()) {
        std::vector<LayoutCandidate> cands;
        add_candidate(cands, c.th, {}, ops0, p0);
        for (const RelayoutChoice& v : rw.all)
            if (v.plan.passes.size() <= p0.passes.size()) add_candidate(cands, 6, v.perm, v.ops, v.plan, true);
        if (cands.size() > 1) {
            const LayoutCandidate& w = cands[calibrate_candidates(s, cands)];
            s->calibrated = true;
            if (w.relayout) take_relayout(c, w);
            else c.memo_no_relayout();
            return;
        }
    }
    if (rw.have && (relayout_forced() || rw.best.plan.passes.size() < p0.passes.size())) take_relayout(c, rw.best);
    else c.memo_no_relayout();
}

// One height's fixed-layout candidates: the layout model's choice and its next alternatives
// under tile height h and 13-qubit cost factor t13.
struct Gen {
    int h;
    double t13;
    size_t alts;
};
std::vector<Gen> candidate_gens(const FirstRun& c) {
    // QSIM_RELABEL_CALIBRATE_CANDIDATES (default 3) per height
    static const size_t alts = (size_t)std::max(1, env_int("QSIM_RELABEL_CALIBRATE_CANDIDATES", 3)) - 1;
    std::vector<Gen> gens{{c.th, layout_t13(), c.timing ? alts : 0}};
    if (c.heights) {
        if (c.th == 7) gens.push_back({6, 1.0, alts});
        else gens.insert(gens.end(), {{7, 1.25, alts}, {7, 1.0, 0}});
    }
    return gens;
}
// True: decided (the identity is this height's choice and there is nothing to time).
bool add_height_candidates(const FirstRun& c, const Gen& g, RelayoutWorker& rw, std::vector<LayoutCandidate>& cands) {
    const TileHeightScope scope(g.h, tile_rb_for(c.n, g.h));
    const LayoutT13Scope t13(g.t13);
    LayoutChoice lc =
        choose_layout(c.n, [&c](const std::vector<int>& pi) { return c.lower(pi); }, relabel_tries(), g.alts);
    if (lc.perm.empty()) {  // the identity is this height's choice
        rw.join();
        if (!c.heights && !(rw.have && c.timing)) {  // (nothing to time)
            if (rw.have && rw.best.plan.passes.size() < lc.passes_before) take_relayout(c, rw.best);
            else c.memo_put({});
            return true;
        }
        std::vector<Op> ops = c.lower({});
        Plan plan = plan_fused(ops, c.n, g.h);
        add_candidate(cands, g.h, {}, std::move(ops), std::move(plan));
    } else {
        add_candidate(cands, g.h, std::move(lc.perm), std::move(lc.ops), std::move(lc.plan));
    }
    for (LayoutChoice::Alt& a : lc.alts) add_candidate(cands, g.h, std::move(a.perm), std::move(a.ops), std::move(a.plan));
    return false;
}

// The pick among the fixed-layout candidates and the relayout variants: timed when there is more
// than one, else the relayout plan when it needs fewer passes.
void pick_candidate(const FirstRun& c, RelayoutWorker& rw, std::vector<LayoutCandidate>& cands) {
    qsim_state* s = c.s;
    if (rw.have) {
        if (c.timing) {
            for (const RelayoutChoice& v : rw.all) add_candidate(cands, 6, v.perm, v.ops, v.plan, true);
        } else if (rw.best.plan.passes.size() < cands[0].plan.passes.size()) {
            take_relayout(c, rw.best);
            return;
        }
    }
    size_t best = 0;
    if (cands.size() > 1) {
        best = calibrate_candidates(s, cands);  // (their plans stay cached, compiled)
    } else {
        const TileHeightScope scope(cands[0].h, tile_rb_for(c.n, cands[0].h));
        if (!cands[0].perm.empty()) s->plans.put(cands[0].ops, c.n, cands[0].plan, s->stream);
    }
    LayoutCandidate& w = cands[best];
    s->calibrated = cands.size() > 1;
    if (w.relayout) {
        take_relayout(c, w);
        return;
    }
    if (c.heights) s->tile_h = w.h;
    s->perm = std::move(w.perm);
    c.memo_put(s->perm);
}
}  // namespace

// The labels (s->perm) and, with cross-height calibration, the tile height (s->tile_h) for the
// first fused run of a basis state.  Candidates: the layout model's choice and its next
// alternatives at the state's default height; with cross-height calibration also at the other
// height (13-qubit tiles with the 13-qubit cost factor 1.25, which steers the labels toward
// mixed plans, and with factor 1) — every candidate timed on the device, the fastest kept.
void choose_first_layout(qsim_state* s, const qsim_gate* gates, size_t count) {
    const int n = s->n;
    FirstRun c{s, gates, count, n, count * sizeof(qsim_gate), false, 0, false, false};
    c.heights = calibrate_heights(n) && s->tile_h < 0;
    c.th = state_tile_height(s);
    // Relayout plans permute qubit labels, so they follow the relabeling mode (not its size
    // threshold), and they need the second buffer: without room for it, fixed layouts only.
    c.relayout = relayout_enabled(n) && relabel_mode_on() && !tile_height_is_set() && ensure_alt(s);
    struct AltRelease {  // a first run that does not end on a relayout plan keeps one buffer
        qsim_state* s;
        ~AltRelease() {
            if (!s->relayout) try {
                    release_alt(s);
                } catch (...) {
                }
        }
    } alt_release{s};
    c.timing = relabel_calibrate(n);
    if (c.relayout && relayout_memo_decides(c)) return;
    if (layout_memo_decides(c)) return;
    RelayoutWorker rw;
    if (c.relayout) rw.start(c);
    if (!relabel_enabled(n)) return choose_relayout_only(c, rw);
    if (relayout_forced()) {  // (tests: QSIM_RELAYOUT=2 / qsim_set_relayout(2): whenever one exists)
        rw.join();
        if (rw.have) return take_relayout(c, rw.best);
    }
    // The relayout planner keeps running on its worker while the fixed-layout candidates are
    // chosen; it is joined where its result is first needed.
    std::vector<LayoutCandidate> cands;
    for (const Gen& g : candidate_gens(c))
        if (add_height_candidates(c, g, rw, cands)) return;
    rw.join();
    pick_candidate(c, rw, cands);
}

}  // namespace qsim_hip
