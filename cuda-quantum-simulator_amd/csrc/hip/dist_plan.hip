// dist_plan.hip — the remap planner of the sharded state (dist.hip), the slab layout of its exchanges
// and the host-only C entries through which CPU tests read what a run will do.  No device, no communicator.
#include "dist_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>

namespace qsim_hip {

// QSIM_DIST_COARSE=0: no coarse parts (DStep::coarse; read once)
static bool coarse_enabled() {
    static const bool v = env_switch("QSIM_DIST_COARSE", true);
    return v;
}
// QSIM_DIST_CARRY=1 (experimental, off by default; read per call so tests can switch it): a run's
// last step is left pending and merged into the next run's first step (run_dist).
bool carry_enabled() {
    return env_switch("QSIM_DIST_CARRY", false);
}
// The positions of `mask` that pass p's tile touches (all of them for a per-gate step or a tile
// below 4 free bits: such passes never run as sub-space launches).
static uint64_t pass_touches(const FusedPass& p, uint64_t mask) {
    if (p.single >= 0 || p.h < 4) return mask;
    uint64_t t = 0;
    for (int i = 0; i < 6 + p.h - p.r0; ++i) t |= mask & (1ull << p.hpos[i]);
    return t;
}
// Coarse split of the passes [lo, hi) of a plan just ahead of its per-part tail, for pivots `set`:
// the count c of passes (ending at hi) and the coarse bits (pivots none of them touches) that
// minimise the exposed work (hi - lo - c) + c / 2^|coarse| (in passes).  *cb = 0, 0: none.
static int coarse_split(const Plan& pl, int lo, int hi, uint64_t set, uint64_t* cb) {
    int best_c = 0;
    uint64_t best_cb = 0, U = 0;
    double best = (double)(hi - lo);
    for (int c = 1; c <= hi - lo; ++c) {
        U |= pass_touches(pl.passes[hi - c], set);
        const uint64_t b = set & ~U;
        if (!b) break;
        const double e = (double)(hi - lo - c) + (double)c / (double)(1 << __builtin_popcountll(b));
        if (e < best - 1e-9) {
            best = e;
            best_c = c;
            best_cb = b;
        }
    }
    *cb = best_cb;
    return best_c;
}
// Exchange order of the K parts of an overlapped remap with pivots pmask and coarse bits cb:
// coarse-major (part index bit j = the j-th pivot; the coarse pivots' bits vary slowest), so the
// parts of the first coarse part, whose passes finish first, leave first.  Rank-independent.
void part_order(uint64_t pmask, uint64_t cb, int* order) {
    const int m = __builtin_popcountll(pmask), K = 1 << m;
    uint64_t ch = 0;  // coarse pivots as part-index bits
    {
        int j = 0;
        for (uint64_t mm = pmask; mm; mm &= mm - 1, ++j)
            if ((cb >> __builtin_ctzll(mm)) & 1ull) ch |= 1ull << j;
    }
    const int Kc = 1 << __builtin_popcountll(ch), Kf = K / Kc;
    int i = 0;
    for (int cv = 0; cv < Kc; ++cv)
        for (int f = 0; f < Kf; ++f) {
            uint64_t h = 0;
            int a = 0, b = 0;
            for (int j = 0; j < m; ++j) {
                if ((ch >> j) & 1ull) h |= (uint64_t)((cv >> a++) & 1) << j;
                else h |= (uint64_t)((f >> b++) & 1) << j;
            }
            order[i++] = (int)h;
        }
}
bool pass_avoids(const FusedPass& p, uint64_t pmask) {
    if (p.single >= 0 || p.h < 4) return false;
    for (int i = 0; i < 6 + p.h - p.r0; ++i)
        if ((pmask >> p.hpos[i]) & 1ull) return false;
    return true;
}
uint64_t deposit_bits(uint64_t v, uint64_t mask) {
    uint64_t r = 0;
    for (int j = 0; mask; mask &= mask - 1, ++j) r |= ((v >> j) & 1ull) << __builtin_ctzll(mask);
    return r;
}
int part_count(uint64_t pmask) {
    const int m = __builtin_popcountll(pmask);
    if (m > kMaxPivots) fail(QSIM_ERR_RUNTIME, "overlapped remap with " + std::to_string(m) + " pivots (at most " +
                                                   std::to_string(kMaxPivots) + ")");
    return 1 << m;
}
PassSplit split_passes(const Plan& pl, uint64_t pb, uint64_t pa, uint64_t cb, bool head_runs) {
    PassSplit r;
    r.np = pl.passes.size();
    if (pb)
        while (r.j1 < r.np && pass_avoids(pl.passes[r.j1], pb)) ++r.j1;
    r.j2 = r.np;
    if (pa)
        while (r.j2 > r.j1 && pass_avoids(pl.passes[r.j2 - 1], pa)) --r.j2;
    r.jc = r.j2;
    const size_t lo = head_runs ? r.j1 : 0;
    if (cb)
        while (r.jc > lo && pass_avoids(pl.passes[r.jc - 1], cb)) --r.jc;
    return r;
}
uint64_t carried_pivots(const std::vector<DStep>& st) {
    const size_t k = st.size() - 1;
    if (st.size() < 2 || st[k].kind != 0 || !(st[k].role & 2) || (st[k].role & 1)) return 0;
    return st[k - 1].pmask;
}
// cost(c) for every c < count, on up to 16 threads.  Worker threads must not throw: a candidate
// whose cost does scores 1e30 and just loses.
template <typename F>
static std::vector<double> score_parallel(size_t count, F&& cost) {
    std::vector<double> sc(count, 1e30);
    std::vector<std::thread> th;
    const size_t nt = std::min<size_t>(count, 16);
    for (size_t w = 0; w < nt; ++w)
        th.emplace_back([&, w] {
            for (size_t c = w; c < count; c += nt) try {
                    sc[c] = cost(c);
                } catch (...) {
                }
        });
    for (auto& t : th) t.join();
    return sc;
}

// Choose, for every exchange between two ops steps, its pivots (QSIM_DIST_OVERLAP=0 disables).
// The ops steps are not split: each rank plans a step as one fused plan (tiles padded away from
// the pivots) and runs per part only the passes at its ends that avoid them (qsim_dist_run).
// Time model of one remap between steps A and B (pass time 1, transfer time R, K = 2^m parts,
// t trailing passes of A and h leading passes of B avoiding the pivots):
//     T = max(R + (nA - t) + (nB - h) + (t + h) / K,  nA + nB + R / K)
// with R = 50 / world (an HBM pass at ~6 TB/s over a remap that sends 1/world of the shard per
// link at ~60 GB/s).  Pivots are local positions >= 6 (never a tile's contiguous run) outside the
// exchanged positions, added greedily (up to kMaxPivots) while T drops; each candidate set is
// scored by planning both steps with it avoided, in parallel, on RANK 0's ops (`ref`: the same
// skeleton on every rank), so every rank picks the same pivots.  Everything else the score reads
// is rank-independent too: the positions the step before must also avoid come from this rank's
// own marks (`steps`, set by the same decisions on every rank), never from `ref`'s roles (which
// are only marked when `ref` aliases `steps`, i.e. on rank 0).  QSIM_DIST_PIVOTS caps m
// (default kMaxPivots); QSIM_DIST_PIVOT_PLAN=0: one pivot by the cheaper gate-level score
// (trailing / leading gates that do not touch the position).
// carry: pivots of the previous run's last exchange whose parts are still in flight when this
// run starts (qsim_dist_run merges that run's last step into this one's first): the first ops
// step's leading passes that avoid them run per part too (role bit 2 on step 0).
// next_ops: the first ops step of the NEXT run of the circuit (from this run's end map, rank 0's
// lowering): the last remap's pivots are also scored by the passes of it they let run per part
// (carried into the next run, qsim_dist_run).
static void mark_overlap(std::vector<DStep>& steps, int L, int world, const std::vector<DStep>& ref,
                         uint64_t carry = 0, const std::vector<Op>* next_ops = nullptr) {
    static const int enabled = env_int("QSIM_DIST_OVERLAP", 1);
    static const int by_plan = env_int("QSIM_DIST_PIVOT_PLAN", 1);
    static const int max_piv = [] {
        const char* e = std::getenv("QSIM_DIST_PIVOTS");
        return e ? std::max(1, std::min(kMaxPivots, std::atoi(e))) : kMaxPivots;
    }();
    if (!enabled || L < 8) return;
    if (carry && !steps.empty() && steps[0].kind == 0) steps[0].role |= 2;
    const int min_gates = 4;
    static const double r_scale = [] {  // QSIM_DIST_MODEL_R (experiments): R x world, default 50
        const char* e = std::getenv("QSIM_DIST_MODEL_R");
        return e ? std::atof(e) : 50.0;
    }();
    const double R = r_scale / std::max(2, world);
    for (size_t i = 1; i + 1 < steps.size(); ++i) {
        DStep& ex = steps[i];
        DStep& A = steps[i - 1];
        DStep& B = steps[i + 1];
        if (ex.kind != 1 || A.kind != 0 || B.kind != 0) continue;
        uint64_t lmask = 0;
        for (int j = 0; j < ex.k; ++j) lmask |= 1ull << ex.lpos[j];
        int best_p = -1, best = 0;
        std::vector<int> cand;
        for (int p = 6; p < L; ++p) {
            if ((lmask >> p) & 1ull) continue;
            cand.push_back(p);
            const uint64_t bit = 1ull << p;
            int a = 0, b = 0;
            while (a < (int)A.gmask.size() && !(A.gmask[A.gmask.size() - 1 - a] & bit)) ++a;
            while (b < (int)B.gmask.size() && !(B.gmask[b] & bit)) ++b;
            if (a + b > best) {
                best_p = p;
                best = a + b;
            }
        }
        uint64_t pmask = best_p >= 0 && best >= min_gates ? 1ull << best_p : 0ull;
        const DStep& rA = ref[i - 1];
        const DStep& rB = ref[i + 1];
        if (by_plan && !rA.ops.empty() && !rB.ops.empty() && !cand.empty()) {
            const uint64_t avoidA0 = (A.role & 2) ? (i >= 2 ? steps[i - 2].pmask : carry) : 0ull;
            // T of a pivot set (pass counts in units of one pass); +inf when planning failed;
            // *cb_out: the coarse bits of that set (coarse_split)
            auto model = [&](uint64_t set, uint64_t* cb_out = nullptr) {
                const Plan pA = plan_fused(rA.ops, L, -1, set, avoidA0);
                const Plan pB = plan_fused(rB.ops, L, -1, 0, set);
                const int na = (int)pA.passes.size(), nb = (int)pB.passes.size();
                int t = 0, h = 0, ha = 0;
                // A's leading passes that run per part of the exchange before it (or of the
                // previous run's last one, `carry`) are hidden behind that exchange; the trailing
                // ones that avoid this set feed this one (a pass counts once: head first, as the
                // run splits a step)
                if (avoidA0)
                    while (ha < na && pass_avoids(pA.passes[ha], avoidA0)) ++ha;
                while (t < na - ha && pass_avoids(pA.passes[na - 1 - t], set)) ++t;
                while (h < nb && pass_avoids(pB.passes[h], set)) ++h;
                const double K = (double)(1 << __builtin_popcountll(set));
                if (t + h == 0) return 1e30;
                // The next run's first pass, if it avoids the set, is hidden behind this remap too
                // (carried, qsim_dist_run); at most one is credited — more would only shorten that
                // run's own tail, whose remap hides it anyway (crediting them all makes the greedy
                // pick few pivots: big parts, a long exposed last part).  A's leading `ha` passes
                // were hidden behind the remap before this one and cost nothing here.
                int hn = 0;
                if (next_ops && !next_ops->empty() && i + 2 == steps.size() && h == nb && !(B.role & 1)) {
                    const Plan pN = plan_fused(*next_ops, L, -1, set);
                    hn = !pN.passes.empty() && pass_avoids(pN.passes[0], set) ? 1 : 0;
                }
                // the passes just ahead of the tail run per coarse part (coarse_split)
                uint64_t cb = 0;
                const int c = coarse_enabled() ? coarse_split(pA, ha, na - t, set, &cb) : 0;
                if (cb_out) *cb_out = cb;
                const double exposed = (double)(na - t - ha - c) + (c ? (double)c / (double)(1 << __builtin_popcountll(cb)) : 0.0);
                return std::max(R + exposed + (nb - h) + (t + h + hn) / K - hn, na + nb + R / K);
            };
            // round 1: every single position; later rounds: a beam of the kBeam best sets, each
            // grown by one of the kPool best singles (the greedy of round 4 kept one set: it missed
            // sets whose first pass leaves a pivot untouched, i.e. coarse parts, round 5)
            constexpr size_t kBeam = 4, kPool = 10;
            std::vector<double> sc1 = score_parallel(cand.size(), [&](size_t c) { return model(1ull << cand[c]); });
            std::vector<size_t> order(cand.size());
            for (size_t c = 0; c < order.size(); ++c) order[c] = c;
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return sc1[a] < sc1[b]; });
            double bestT = sc1[order[0]];
            uint64_t set = bestT < 1e29 ? 1ull << cand[order[0]] : 0ull;
            std::vector<int> pool;
            std::vector<std::pair<double, uint64_t>> beam;
            for (size_t c = 0; c < order.size() && pool.size() < kPool; ++c)
                if (sc1[order[c]] < 1e29) {
                    pool.push_back(cand[order[c]]);
                    if (beam.size() < kBeam) beam.push_back({sc1[order[c]], 1ull << cand[order[c]]});
                }
            for (int m = 1; set && m < max_piv && !beam.empty(); ++m) {
                std::vector<uint64_t> sets;
                for (const auto& b : beam)
                    for (int q : pool) {
                        const uint64_t s2 = b.second | (1ull << q);
                        if (s2 != b.second && std::find(sets.begin(), sets.end(), s2) == sets.end()) sets.push_back(s2);
                    }
                std::vector<double> sc = score_parallel(sets.size(), [&](size_t c) { return model(sets[c]); });
                std::vector<size_t> o2(sets.size());
                for (size_t c = 0; c < o2.size(); ++c) o2[c] = c;
                std::sort(o2.begin(), o2.end(), [&](size_t a, size_t b) {
                    return sc[a] != sc[b] ? sc[a] < sc[b] : sets[a] < sets[b];  // (deterministic)
                });
                beam.clear();
                for (size_t c = 0; c < o2.size() && beam.size() < kBeam; ++c)
                    if (sc[o2[c]] < 1e29) beam.push_back({sc[o2[c]], sets[o2[c]]});
                if (!beam.empty() && beam[0].first < bestT - 1e-9) {
                    bestT = beam[0].first;
                    set = beam[0].second;
                }
            }
            if (set) {
                pmask = set;
                try {
                    (void)model(set, &ex.coarse);
                } catch (...) {
                    ex.coarse = 0;
                }
            }
        }
        if (!pmask) continue;
        ex.pmask = pmask;
        ex.pivot = __builtin_ctzll(pmask);
        A.role |= 1;
        B.role |= 2;
    }
}

// Logical target that must be local for gate g (2x2 ops), or -1 (diagonal, SWAP).
static int needs_local(const qsim_gate& g) {
    switch (g.type) {
        case QSIM_GATE_X: case QSIM_GATE_Y: case QSIM_GATE_H: case QSIM_GATE_RX: case QSIM_GATE_RY:
            return g.qubits[0];
        case QSIM_GATE_CNOT: case QSIM_GATE_CRY:
            return g.qubits[1];
        case QSIM_GATE_TOFFOLI:
            return g.qubits[2];
        default:
            return -1;
    }
}

// QSIM_DIST_FULL_REMAP=0 lets a remap move only the globals that must leave (fewer bytes, fewer
// links); the default swaps all of them (see plan_dist).
static bool full_remap() {
    static const bool v = env_switch("QSIM_DIST_FULL_REMAP", true);
    return v;
}

static uint64_t gate_qmask(const qsim_gate& g) {
    uint64_t m = 0;
    for (int j = 0; j < g.nqubits; ++j) m |= 1ull << g.qubits[j];
    return m;
}

// Gates of `window` (indices into `gates`, in program order) that can run before any further
// remap when the logical qubits in `glob` are global: a gate runs unless its target is global or
// an earlier gate that shares a qubit with it could not run.  SWAPs relabel `glob`.
static int count_runnable(const qsim_gate* gates, const std::vector<uint64_t>& qm,
                          const std::vector<int>& window, size_t upto, uint64_t glob) {
    uint64_t blocked = 0;
    int cnt = 0;
    for (size_t w = 0; w < upto; ++w) {
        const int i = window[w];
        const qsim_gate& gt = gates[i];
        if (qm[i] & blocked) {
            blocked |= qm[i];
            continue;
        }
        if (gt.type == QSIM_GATE_SWAP) {
            const uint64_t a = 1ull << gt.qubits[0], b = 1ull << gt.qubits[1];
            if (((glob & a) != 0) != ((glob & b) != 0)) glob ^= a | b;
            continue;
        }
        const int tq = needs_local(gt);
        if (tq >= 0 && ((glob >> tq) & 1ull)) {
            blocked |= qm[i];
            continue;
        }
        ++cnt;
    }
    return cnt;
}

// The logical qubits to make global at a remap.  Scored, in order, by the gates that can then run
// before the next remap (i) in the rest of this circuit and (ii) over the rest plus one more run
// of the circuit (a benchmark or trajectory loop re-runs it from the map this run ends with), then
// by the physical positions of the incoming qubits (high positions give long pack runs).
// Exhaustive over the candidate g-sets when that is cheap (C(27,3) = 2925 at 30 qubits on 8
// ranks), greedy one qubit at a time otherwise.
static uint64_t choose_globals(const qsim_gate* gates, size_t count, const std::vector<uint64_t>& qm,
                               const std::vector<char>& done, const std::vector<int>& perm, int n,
                               int g, int L, bool full) {
    std::vector<int> window;
    for (size_t i = 0; i < count; ++i)
        if (!done[i]) window.push_back((int)i);
    const size_t rest = window.size();
    const size_t cap = std::max<size_t>(rest, 1024);
    for (size_t i = 0; i < count && window.size() < cap; ++i) window.push_back((int)i);
    std::vector<int> cand;  // full remap: every current global leaves, so only locals may enter
    for (int q = 0; q < n; ++q)
        if (!full || perm[q] < L) cand.push_back(q);
    struct Score {
        int a = -1, b = -1, c = -1;
        bool operator<(const Score& o) const {
            return a != o.a ? a < o.a : (b != o.b ? b < o.b : c < o.c);
        }
    };
    auto score = [&](uint64_t set) {
        Score s;
        s.a = count_runnable(gates, qm, window, rest, set);
        s.b = count_runnable(gates, qm, window, window.size(), set);
        s.c = 0;
        for (int q = 0; q < n; ++q)
            if ((set >> q) & 1ull) s.c += perm[q];
        return s;
    };
    const int m = (int)cand.size();
    double combos = 1.0;
    for (int j = 0; j < g; ++j) combos = combos * (m - j) / (j + 1);
    uint64_t best_set = 0;
    Score best;
    if (combos <= 20000.0) {
        std::vector<int> idx(g);
        for (int j = 0; j < g; ++j) idx[j] = j;
        for (;;) {
            uint64_t set = 0;
            for (int j = 0; j < g; ++j) set |= 1ull << cand[idx[j]];
            const Score s = score(set);
            if (best < s) {
                best = s;
                best_set = set;
            }
            int j = g - 1;
            while (j >= 0 && idx[j] == m - g + j) --j;
            if (j < 0) break;
            ++idx[j];
            for (int k = j + 1; k < g; ++k) idx[k] = idx[k - 1] + 1;
        }
    } else {
        for (int j = 0; j < g; ++j) {
            uint64_t pick = 0;
            Score bj;
            for (int q : cand) {
                if ((best_set >> q) & 1ull) continue;
                const Score s = score(best_set | (1ull << q));
                if (bj < s) {
                    bj = s;
                    pick = 1ull << q;
                }
            }
            best_set |= pick;
        }
    }
    return best_set;
}

// Host plan of one run for one rank.  Gates are reordered only past gates on disjoint qubits
// (exact).  Each sweep in program order runs every gate whose target is local and whose earlier
// qubit-sharing gates have all run; when a sweep leaves gates, one remap brings in the targets
// (choose_globals) and the next sweep continues.  W-HC at 30 qubits on 8 ranks needs one remap
// per run this way (two in plain program order).
std::vector<DStep> plan_dist_core(const qsim_gate* gates, size_t count, int n, int g, int rank,
                                         std::vector<int>& perm) {
    const int L = n - g;
    auto rank_bit = [&](int p) { return (rank >> (p - L)) & 1; };
    std::vector<DStep> steps;
    DStep cur;
    auto flush = [&]() {
        if (!cur.ops.empty() || !cur.gmask.empty()) steps.push_back(cur);
        cur = DStep();
    };
    for (size_t i = 0; i < count; ++i) validate_gate(gates[i], n);
    std::vector<uint64_t> qm(count);
    for (size_t i = 0; i < count; ++i) qm[i] = gate_qmask(gates[i]);
    auto emit = [&](size_t i) {
        const qsim_gate& gt = gates[i];
        if (gt.type == QSIM_GATE_SWAP) {  // relabel only
            std::swap(perm[gt.qubits[0]], perm[gt.qubits[1]]);
            return;
        }
        uint64_t pm = 0;  // physical positions the gate touches (rank-independent)
        for (int j = 0; j < gt.nqubits; ++j) pm |= 1ull << perm[gt.qubits[j]];
        cur.gmask.push_back(pm);
        qsim_gate pg = gt;
        for (int j = 0; j < gt.nqubits; ++j) pg.qubits[j] = perm[gt.qubits[j]];
        Op op = lower_gate(pg, n);
        op.src = (int)i;
        bool skip = false;
        for (int c = L; c < n; ++c)
            if ((op.cmask >> c) & 1ull) {
                if (!rank_bit(c)) skip = true;
                op.cmask &= ~(1ull << c);
            }
        if (skip) return;
        if (op.kind == K_DIAG && op.t0 >= L) {
            const int b = rank_bit(op.t0);
            if (!b && op.d0_one) return;  // factor 1 on this rank
            const double fr = b ? op.m[2] : op.m[0], fi = b ? op.m[3] : op.m[1];
            int t = 0;
            while (t < L - 1 && ((op.cmask >> t) & 1ull)) ++t;
            op.t0 = t;
            op.sub = S_GEN;
            op.d0_one = false;
            op.m[0] = op.m[2] = fr;
            op.m[1] = op.m[3] = fi;
        }
        if (op.t0 >= L || (op.kind == K_SWAP && op.t1 >= L))
            fail(QSIM_ERR_RUNTIME, "distributed planner left a global target");
        cur.ops.push_back(op);
        cur.op_gate.push_back((int)cur.gmask.size() - 1);
    };
    std::vector<char> done(count, 0);
    size_t left = count;
    for (;;) {
        uint64_t blocked = 0;
        for (size_t i = 0; i < count; ++i) {
            if (done[i]) continue;
            if (qm[i] & blocked) {
                blocked |= qm[i];
                continue;
            }
            const int tq = needs_local(gates[i]);
            if (tq >= 0 && perm[tq] >= L) {
                blocked |= qm[i];
                continue;
            }
            emit(i);
            done[i] = 1;
            --left;
        }
        if (left == 0) break;
        flush();
        const bool full = full_remap();
        const uint64_t want = choose_globals(gates, count, qm, done, perm, n, g, L, full);
        std::vector<int> out, in;
        for (int q = 0; q < n; ++q) {
            const bool w = (want >> q) & 1ull;
            if (perm[q] >= L && !w) out.push_back(q);
            if (perm[q] < L && w) in.push_back(q);
        }
        if (out.empty() || out.size() != in.size())
            fail(QSIM_ERR_RUNTIME, "distributed planner: no remap makes progress");
        DStep ex;
        ex.kind = 1;
        ex.k = (int)out.size();
        for (int j = 0; j < ex.k; ++j) {
            ex.gpos[j] = perm[out[j]];
            ex.lpos[j] = perm[in[j]];
            perm[out[j]] = ex.lpos[j];
            perm[in[j]] = ex.gpos[j];
        }
        steps.push_back(ex);
    }
    flush();
    // an exchange needs an ops step on both sides to overlap with (possibly empty)
    std::vector<DStep> framed;
    for (size_t i = 0; i < steps.size(); ++i) {
        if (steps[i].kind == 1 && (framed.empty() || framed.back().kind == 1)) framed.push_back(DStep());
        framed.push_back(std::move(steps[i]));
    }
    if (!framed.empty() && framed.back().kind == 1) framed.push_back(DStep());
    steps.swap(framed);
    return steps;
}

// Pivots chosen for a (gate list, start map, n, g): every shard of a virtual run, and every run
// that starts from the same map, reuses the decision instead of re-planning the candidates.
namespace {
struct PivotMemo {
    int n, g;
    uint64_t carry;
    std::vector<qsim_gate> gates;
    std::vector<int> perm;
    std::vector<uint64_t> pmask;   // per step (0: none)
    std::vector<uint64_t> coarse;  // per step
    uint64_t used;
};
std::mutex g_pivot_mu;
std::vector<PivotMemo> g_pivots;
uint64_t g_pivot_clock = 0;
}  // namespace

// ---- steady-state cycle pivots (the cross-run carry, QSIM_DIST_CARRY) ---------------------
// A benchmark or trajectory loop re-runs one circuit, and the runs' start maps soon cycle (the remap
// planner is deterministic; W-HC 30q on 8 ranks: two maps).  With the carry on, run j's last step B_j
// and run j+1's leading passes run per part of run j's exchange X_j, so X_j's pivots P_j shape TWO
// runs: run j (A_j's tail and B_j avoid P_j) and run j+1 (A_{j+1}'s head avoids P_j).  mark_overlap
// chooses P_j for run j alone (at most one pass of the next run credited), and on the alternate
// runs of seed 42 A's first pass then touches the carried pivots and runs whole and exposed.  Here
// the pivots of every exchange of the cycle are chosen together: coordinate descent over the
// cycle, each P_j by the beam search of mark_overlap on the cost T_j + T_{j+1} (the run-time model
// of mark_overlap with the carry: per-part passes of both neighbouring runs, whole passes exposed),
// every plan from rank 0's lowering (rank-independent), plans memoised by (step, avoid sets).
namespace {
struct CycleMemo {
    int n, g;
    std::vector<qsim_gate> gates;
    std::vector<std::vector<int>> maps;  // start map of each run of the cycle
    std::vector<uint64_t> piv;           // pivots of each run's exchange
    uint64_t used;
};
std::vector<CycleMemo> g_cycles;  // (under g_pivot_mu)
}  // namespace

// The pass touch masks of step `ops` planned with tail avoid set `pa` and head avoid set `pb`
// (all ones for a pass that never runs per part).
static std::vector<uint64_t> pass_masks(const std::vector<Op>& ops, int L, uint64_t pa, uint64_t pb) {
    const Plan pl = plan_fused(ops, L, -1, pa, pb);
    std::vector<uint64_t> m;
    for (const FusedPass& fp : pl.passes) m.push_back(pass_touches(fp, ~0ull));
    return m;
}

// Per pass of the unconstrained plan of `ops`: the positions its gates act on (targets and
// controls; padding excluded — a tile may be padded elsewhere), all ones for a per-gate pass.
static std::vector<uint64_t> pass_forced(const std::vector<Op>& ops, int L) {
    const Plan pl = plan_fused(ops, L);
    std::vector<uint64_t> m;
    for (const FusedPass& fp : pl.passes) {
        if (fp.single >= 0 || fp.h < 4) {
            m.push_back(~0ull);
            continue;
        }
        int b = fp.op_begin, e = fp.op_end;
        if (fp.stage_end > fp.stage_begin) {
            b = pl.stages[fp.stage_begin].op_begin;
            e = pl.stages[fp.stage_end - 1].op_end;
        }
        uint64_t f = 0;
        for (int i = b; i < e; ++i) {
            const Op& o = ops[pl.order[i]];
            f |= (1ull << o.t0) | o.cmask;
            if (o.t1 >= 0) f |= 1ull << o.t1;
        }
        m.push_back(f);
    }
    return m;
}

static bool cycle_pivots(const qsim_gate* gates, size_t count, int n, int g, const std::vector<int>& perm_in,
                         uint64_t* piv_out) {
    const int L = n - g;
    auto same_gates = [&](const CycleMemo& m) {
        return m.n == n && m.g == g && m.gates.size() == count &&
               (count == 0 || std::memcmp(m.gates.data(), gates, count * sizeof(qsim_gate)) == 0);
    };
    {
        std::lock_guard<std::mutex> l(g_pivot_mu);
        for (CycleMemo& m : g_cycles)
            if (same_gates(m))
                for (size_t j = 0; j < m.maps.size(); ++j)
                    if (m.maps[j] == perm_in) {
                        m.used = ++g_pivot_clock;
                        *piv_out = m.piv[j];
                        return true;
                    }
    }
    // the runs from perm_in (rank 0's lowering), until a start map repeats
    std::vector<std::vector<int>> maps;
    std::vector<std::vector<DStep>> runs;
    std::vector<int> p = perm_in;
    int cyc = -1;
    for (int r = 0; r < 8 && cyc < 0; ++r) {
        maps.push_back(p);
        runs.push_back(plan_dist_core(gates, count, n, g, 0, p));
        for (size_t j = 0; j < maps.size(); ++j)
            if (maps[j] == p) cyc = (int)j;
    }
    if (cyc != 0) return false;  // (perm_in is a transient map, or no cycle within 8 runs)
    const int C = (int)runs.size();
    for (const std::vector<DStep>& st : runs)
        if (st.size() != 3 || st[0].kind != 0 || st[1].kind != 1 || st[2].kind != 0 || st[0].ops.empty() ||
            st[2].ops.empty())
            return false;  // (one remap per run between two ops steps: the case the model prices)
    static const double r_scale = [] {  // (mark_overlap's QSIM_DIST_MODEL_R)
        const char* e = std::getenv("QSIM_DIST_MODEL_R");
        return e ? std::atof(e) : 50.0;
    }();
    // a pass run per part (sub-space launches) costs rP whole-shard passes (virtual 30q / 8:
    // 5.15 vs 6.4 TB/s, profiles/r04/dist_virtual/)
    static const double rP = [] {
        const char* e = std::getenv("QSIM_DIST_MODEL_PART");
        return e ? std::atof(e) : 1.243;
    }();
    const double R = r_scale / std::max(2, 1 << g);
    std::mutex mu;
    std::map<std::tuple<int, int, uint64_t, uint64_t>, std::vector<uint64_t>> cache;
    auto masks = [&](int j, int which, uint64_t pa, uint64_t pb) {
        const auto key = std::make_tuple(j, which, pa, pb);
        {
            std::lock_guard<std::mutex> l(mu);
            auto it = cache.find(key);
            if (it != cache.end()) return it->second;
        }
        std::vector<uint64_t> m = pass_masks(runs[j][which].ops, L, pa, pb);
        std::lock_guard<std::mutex> l(mu);
        cache.emplace(key, m);
        return m;
    };
    // B_j's (passes, leading passes avoiding P_j, parts)
    struct BInfo {
        int nb, h;
        double K;
    };
    auto binfo = [&](int j, uint64_t P) {
        const std::vector<uint64_t> mb = masks(j, 2, 0, P);
        int h = 0;
        if (P)
            while (h < (int)mb.size() && !(mb[h] & P)) ++h;
        return BInfo{(int)mb.size(), h, (double)(1 << __builtin_popcountll(P))};
    };
    // T of a run from its A's pass masks, the previous run's B info, carried pivots Pp, own P
    auto t_of = [&](const std::vector<uint64_t>& ma, const BInfo& bp, uint64_t Pp, uint64_t P) {
        const int na = (int)ma.size();
        int hA = 0, t = 0;
        if (Pp)
            while (hA < na && !(ma[hA] & Pp)) ++hA;
        if (P)
            while (t < na - hA && !(ma[na - 1 - t] & P)) ++t;
        int c = 0;
        uint64_t cb = 0;
        if (P && coarse_enabled()) {  // (coarse_split on the masks)
            double best = (double)(na - t - hA);
            uint64_t U = 0;
            for (int cc = 1; cc <= na - t - hA; ++cc) {
                U |= ma[na - t - cc] & P;
                const uint64_t b = P & ~U;
                if (!b) break;
                const double e = (double)(na - t - hA - cc) + (double)cc / (double)(1 << __builtin_popcountll(b));
                if (e < best - 1e-9) {
                    best = e;
                    c = cc;
                    cb = b;
                }
            }
        }
        const double K = (double)(1 << __builtin_popcountll(P)), Kc = (double)(1 << __builtin_popcountll(cb));
        const int whole = (na - hA - t - c) + (bp.nb - bp.h);
        const double exposed = (bp.h + hA) * rP / bp.K + (na - hA - t - c) + c * rP / Kc + t * rP / K + (bp.nb - bp.h);
        return std::max(R + exposed, whole + (hA + t + c + bp.h) * rP + R / K);
    };
    // T_j: run j with carried pivots Pp (of X_{j-1}) and its own P, from the plans under those sets
    auto tj = [&](int j, uint64_t Pp, uint64_t P) {
        const int jp = (j + C - 1) % C;
        return t_of(masks(j, 0, P, Pp), binfo(jp, Pp), Pp, P);
    };
    std::vector<uint64_t> P(C, 0);
    auto cost_j = [&](int j, uint64_t Pj) {  // the terms P_j enters
        std::vector<uint64_t> Q = P;
        Q[j] = Pj;
        const int jn = (j + 1) % C;
        if (jn == j) return tj(j, Pj, Pj);
        return tj(j, Q[(j + C - 1) % C], Pj) + tj(jn, Pj, Q[jn]);
    };
    auto optimise = [&](int j) {
        uint64_t lmask = 0;
        for (int i = 0; i < runs[j][1].k; ++i) lmask |= 1ull << runs[j][1].lpos[i];
        std::vector<int> cand;
        for (int q = 6; q < L; ++q)
            if (!((lmask >> q) & 1ull)) cand.push_back(q);
        auto score = [&](const std::vector<uint64_t>& sets) {
            return score_parallel(sets.size(), [&](size_t c) { return cost_j(j, sets[c]); });
        };
        std::vector<uint64_t> singles;
        for (int q : cand) singles.push_back(1ull << q);
        std::vector<double> s1 = score(singles);
        double bestT = cost_j(j, 0);
        uint64_t best = 0;
        std::vector<size_t> o(singles.size());
        for (size_t c = 0; c < o.size(); ++c) o[c] = c;
        std::sort(o.begin(), o.end(), [&](size_t a, size_t b) { return s1[a] != s1[b] ? s1[a] < s1[b] : a < b; });
        constexpr size_t kBeam = 4, kPool = 10;
        std::vector<int> pool;
        std::vector<uint64_t> beam;
        for (size_t c = 0; c < o.size() && pool.size() < kPool; ++c)
            if (s1[o[c]] < 1e29) {
                pool.push_back(cand[o[c]]);
                if (beam.size() < kBeam) beam.push_back(singles[o[c]]);
                if (s1[o[c]] < bestT - 1e-9) {
                    bestT = s1[o[c]];
                    best = singles[o[c]];
                }
            }
        // (the current choice competes too: a sweep never makes P_j worse)
        if (P[j]) {
            const double cur = cost_j(j, P[j]);
            if (cur < bestT - 1e-9) {
                bestT = cur;
                best = P[j];
            }
        }
        for (int m = 1; m < kMaxPivots && !beam.empty(); ++m) {
            std::vector<uint64_t> sets;
            for (uint64_t b : beam)
                for (int q : pool) {
                    const uint64_t s2 = b | (1ull << q);
                    if (s2 != b && std::find(sets.begin(), sets.end(), s2) == sets.end()) sets.push_back(s2);
                }
            std::vector<double> sc = score(sets);
            std::vector<size_t> o2(sets.size());
            for (size_t c = 0; c < o2.size(); ++c) o2[c] = c;
            std::sort(o2.begin(), o2.end(),
                      [&](size_t a, size_t b) { return sc[a] != sc[b] ? sc[a] < sc[b] : sets[a] < sets[b]; });
            beam.clear();
            for (size_t c = 0; c < o2.size() && beam.size() < kBeam; ++c)
                if (sc[o2[c]] < 1e29) beam.push_back(sets[o2[c]]);
            if (!o2.empty() && sc[o2[0]] < bestT - 1e-9) {
                bestT = sc[o2[0]];
                best = sets[o2[0]];
            }
        }
        P[j] = best;
    };
    // Constructive start: every split of each run's A into a head (avoids the carried pivots) and a
    // tail (avoids its own), the passes between them whole or coarse.  Under fixed splits P_j may
    // take any position outside the exchanged ones, B_j's passes, A_j's tail and A_{j+1}'s head
    // (masks of the unconstrained plans); the up-to-4 such positions used by the fewest passes of
    // the cycle form P_j.  Splits are ranked by the model on the unconstrained masks, the best few
    // re-priced on the plans under their sets, and the best becomes the descent's start.
    // (QSIM_DIST_CYCLE_CONSTRUCT=1, measured not kept: W-HC 30q / 8, the carry model over seeds
    // 42 / 1-3 gives 4.03 / 3.98 / 4.11 / 3.97x with it against 4.18 / 4.00 / 4.11 / 4.22x from the
    // descent alone — W-HC tiles are dense, a split's free positions number one or two, and the
    // plans re-padded under the chosen sets lose the split anyway)
    static const bool construct = env_switch("QSIM_DIST_CYCLE_CONSTRUCT", false);
    if (C <= 3 && construct) {
        std::vector<std::vector<uint64_t>> mA(C), mB(C);
        std::vector<int> use(64, 0);
        for (int j = 0; j < C; ++j) {
            mA[j] = pass_forced(runs[j][0].ops, L);
            mB[j] = pass_forced(runs[j][2].ops, L);
            for (const auto* v : {&mA[j], &mB[j]})
                for (uint64_t x : *v)
                    for (int q = 0; q < L; ++q) use[q] += (int)((x >> q) & 1ull);
        }
        uint64_t all = 0;
        for (int q = 6; q < L; ++q) all |= 1ull << q;
        std::vector<std::vector<std::pair<int, int>>> splits(C);
        for (int j = 0; j < C; ++j)
            for (int h = 0; h <= std::min(1, (int)mA[j].size()); ++h)  // (the planner steers the first pass only)
                for (int t = 0; h + t <= (int)mA[j].size(); ++t) splits[j].push_back({h, t});
        struct Combo {
            double pred;
            std::vector<uint64_t> P;
        };
        std::vector<Combo> combos;
        std::vector<size_t> idx(C, 0);
        for (;;) {
            std::vector<uint64_t> Q(C, 0);
            for (int j = 0; j < C; ++j) {
                const int jn = (j + 1) % C;
                const int t = splits[j][idx[j]].second, hn = splits[jn][idx[jn]].first;
                uint64_t forbid = 0;
                for (int i = 0; i < runs[j][1].k; ++i) forbid |= 1ull << runs[j][1].lpos[i];
                for (uint64_t x : mB[j]) forbid |= x;
                for (int i = 0; i < t; ++i) forbid |= mA[j][mA[j].size() - 1 - i];
                for (int i = 0; i < hn; ++i) forbid |= mA[jn][i];
                std::vector<int> ok;
                for (int q = 6; q < L; ++q)
                    if (((all & ~forbid) >> q) & 1ull) ok.push_back(q);
                std::stable_sort(ok.begin(), ok.end(), [&](int a, int b) { return use[a] < use[b]; });
                for (size_t i = 0; i < ok.size() && i < (size_t)kMaxPivots; ++i) Q[j] |= 1ull << ok[i];
            }
            double pred = 0.0;
            for (int j = 0; j < C; ++j) {
                const int jp = (j + C - 1) % C;
                int hb = 0;
                if (Q[jp])
                    while (hb < (int)mB[jp].size() && !(mB[jp][hb] & Q[jp])) ++hb;
                pred += t_of(mA[j], BInfo{(int)mB[jp].size(), hb, (double)(1 << __builtin_popcountll(Q[jp]))},
                             Q[jp], Q[j]);
            }
            combos.push_back({pred, Q});
            int j = 0;
            while (j < C && ++idx[j] == splits[j].size()) idx[j++] = 0;
            if (j == C) break;
        }
        std::sort(combos.begin(), combos.end(), [](const Combo& a, const Combo& b) {
            return a.pred != b.pred ? a.pred < b.pred : a.P < b.P;
        });
        std::vector<std::vector<uint64_t>> tops;
        for (const Combo& cb : combos) {
            if (tops.size() >= 12) break;
            if (std::find(tops.begin(), tops.end(), cb.P) == tops.end()) tops.push_back(cb.P);
        }
        const std::vector<double> sc = score_parallel(tops.size(), [&](size_t c) {
            double tot = 0.0;
            for (int j = 0; j < C; ++j) tot += tj(j, tops[c][(j + C - 1) % C], tops[c][j]);
            return tot;
        });
        size_t bi = 0;
        for (size_t c = 1; c < tops.size(); ++c)
            if (sc[c] < sc[bi] - 1e-9) bi = c;
        if (std::getenv("QSIM_DIST_DEBUG_CYCLE"))
            for (size_t c = 0; c < tops.size(); ++c) {
                double pr = 0;
                for (const Combo& cb : combos)
                    if (cb.P == tops[c]) {
                        pr = cb.pred;
                        break;
                    }
                std::fprintf(stderr, "[cycle] combo %zu pred %.3f real %.3f:", c, pr, sc[c]);
                for (uint64_t x : tops[c]) std::fprintf(stderr, " %#llx", (unsigned long long)x);
                for (int j = 0; j < C; ++j) {
                    std::fprintf(stderr, " | A%d", j);
                    for (uint64_t x : masks(j, 0, tops[c][j], tops[c][(j + C - 1) % C]))
                        std::fprintf(stderr, " %#llx", (unsigned long long)x);
                    std::fprintf(stderr, " B%d", j);
                    for (uint64_t x : masks(j, 2, 0, tops[c][j])) std::fprintf(stderr, " %#llx", (unsigned long long)x);
                }
                std::fprintf(stderr, "\n");
            }
        if (!tops.empty() && sc[bi] < 1e29) P = tops[bi];
    }
    static const int sweeps = std::max(0, env_int("QSIM_DIST_CYCLE_SWEEPS", 2));
    for (int sw = 0; sw < sweeps; ++sw)
        for (int j = 0; j < C; ++j) optimise(j);
    static const bool dbg = std::getenv("QSIM_DIST_DEBUG_CYCLE") != nullptr;
    if (dbg) {
        double tot = 0.0;
        for (int j = 0; j < C; ++j) tot += tj(j, P[(j + C - 1) % C], P[j]);
        std::fprintf(stderr, "[cycle] %d runs, model %.3f passes per run, pivots", C, tot / C);
        for (uint64_t x : P) std::fprintf(stderr, " %#llx", (unsigned long long)x);
        std::fprintf(stderr, "\n");
        for (int j = 0; j < C; ++j) {
            const uint64_t Pp = P[(j + C - 1) % C];
            std::fprintf(stderr, "[cycle] run %d T %.3f | A (head %#llx, tail %#llx):", j, tj(j, Pp, P[j]),
                         (unsigned long long)Pp, (unsigned long long)P[j]);
            for (uint64_t x : masks(j, 0, P[j], Pp)) std::fprintf(stderr, " %#llx", (unsigned long long)x);
            std::fprintf(stderr, " | A free:");
            for (uint64_t x : masks(j, 0, 0, 0)) std::fprintf(stderr, " %#llx", (unsigned long long)x);
            std::fprintf(stderr, " | B:");
            for (uint64_t x : masks(j, 2, 0, P[j])) std::fprintf(stderr, " %#llx", (unsigned long long)x);
            std::fprintf(stderr, " | X lpos");
            for (int i = 0; i < runs[j][1].k; ++i) std::fprintf(stderr, " %d", runs[j][1].lpos[i]);
            std::fprintf(stderr, "\n");
        }
    }
    *piv_out = P[0];
    std::lock_guard<std::mutex> l(g_pivot_mu);
    CycleMemo m{n, g, std::vector<qsim_gate>(gates, gates + count), maps, P, ++g_pivot_clock};
    if (g_cycles.size() >= 8)
        g_cycles.erase(std::min_element(g_cycles.begin(), g_cycles.end(),
                                        [](const CycleMemo& a, const CycleMemo& b) { return a.used < b.used; }));
    g_cycles.push_back(std::move(m));
    return true;
}

std::vector<DStep> plan_dist(const qsim_gate* gates, size_t count, int n, int g, int rank,
                                    std::vector<int>& perm, uint64_t carry) {
    const std::vector<int> perm_in = perm;
    std::vector<DStep> steps = plan_dist_core(gates, count, n, g, rank, perm);
    const int L = n - g;
    static const int overlap = env_int("QSIM_DIST_OVERLAP", 1);
    if (!overlap || L < 8 || steps.empty() || steps[0].kind != 0) carry = 0;
    auto same = [&](const PivotMemo& m) {
        return m.n == n && m.g == g && m.carry == carry && m.perm == perm_in && m.gates.size() == count &&
               (count == 0 || std::memcmp(m.gates.data(), gates, count * sizeof(qsim_gate)) == 0);
    };
    {
        std::lock_guard<std::mutex> l(g_pivot_mu);
        for (PivotMemo& m : g_pivots)
            if (same(m) && m.pmask.size() == steps.size()) {
                m.used = ++g_pivot_clock;
                if (carry) steps[0].role |= 2;
                for (size_t k = 0; k < steps.size(); ++k)
                    if (m.pmask[k]) {
                        steps[k].pmask = m.pmask[k];
                        steps[k].coarse = m.coarse[k];
                        steps[k].pivot = __builtin_ctzll(m.pmask[k]);
                        steps[k - 1].role |= 1;
                        steps[k + 1].role |= 2;
                    }
                return steps;
            }
    }
    auto remember = [&]() {  // the marks of `steps` into the memo (16 entries, least recently used out)
        PivotMemo m{n, g, carry, std::vector<qsim_gate>(gates, gates + count), perm_in, {}, {}, 0};
        for (const DStep& st : steps) {
            m.pmask.push_back(st.kind == 1 ? st.pmask : 0ull);
            m.coarse.push_back(st.kind == 1 ? st.coarse : 0ull);
        }
        std::lock_guard<std::mutex> l(g_pivot_mu);
        m.used = ++g_pivot_clock;
        if (g_pivots.size() >= 16)
            g_pivots.erase(std::min_element(g_pivots.begin(), g_pivots.end(),
                                            [](const PivotMemo& a, const PivotMemo& b) { return a.used < b.used; }));
        g_pivots.push_back(std::move(m));
    };
    // carry on and the start map on a cycle of one-remap runs: the cycle's jointly chosen pivots
    uint64_t cyc_piv = 0;
    if (carry_enabled() && overlap && L >= 8 && steps.size() == 3 && steps[0].kind == 0 && steps[1].kind == 1 &&
        steps[2].kind == 0 && cycle_pivots(gates, count, n, g, perm_in, &cyc_piv) && cyc_piv) {
        DStep& A = steps[0];
        DStep& ex = steps[1];
        ex.pmask = cyc_piv;
        ex.pivot = __builtin_ctzll(cyc_piv);
        A.role |= 1;
        steps[2].role |= 2;
        if (carry) A.role |= 2;
        // coarse bits for this run's actual carry, on rank 0's lowering (rank-independent)
        ex.coarse = 0;
        if (coarse_enabled()) {
            std::vector<int> p0 = perm_in;
            const std::vector<DStep> ref = plan_dist_core(gates, count, n, g, 0, p0);
            if (ref.size() == 3 && !ref[0].ops.empty()) {
                const Plan pA = plan_fused(ref[0].ops, L, -1, cyc_piv, carry);
                const PassSplit sp = split_passes(pA, carry, cyc_piv, 0, true);
                (void)coarse_split(pA, (int)sp.j1, (int)sp.j2, cyc_piv, &ex.coarse);
            }
        }
        remember();
        return steps;
    }
    // the next run's first ops step (rank 0's lowering, from this run's end map: the same on every
    // rank), for scoring the last remap's pivots by the passes it can carry
    std::vector<Op> next_ops;
    if (carry_enabled() && overlap && L >= 8) {
        std::vector<int> pn = perm;
        const std::vector<DStep> nxt = plan_dist_core(gates, count, n, g, 0, pn);
        if (!nxt.empty() && nxt[0].kind == 0) next_ops = nxt[0].ops;
    }
    if (rank == 0) {
        mark_overlap(steps, L, 1 << g, steps, carry, &next_ops);
    } else {
        std::vector<int> p0 = perm_in;
        const std::vector<DStep> ref = plan_dist_core(gates, count, n, g, 0, p0);
        if (ref.size() != steps.size()) fail(QSIM_ERR_RUNTIME, "exchange skeleton mismatch");
        mark_overlap(steps, L, 1 << g, ref, carry, &next_ops);
    }
    remember();
    return steps;
}

// ---- slab layout -----------------------------------------------------------------------------
XPlan xplan(int L, int rank, const DStep& ex, int part) {
    XPlan x{};
    XArgs& a = x.a;
    a.k = ex.k;
    const bool h = part >= 0;
    a.chunk_log = L - ex.k - (h ? __builtin_popcountll(ex.pmask) : 0);
    a.chunk = 1ull << a.chunk_log;
    for (int j = 0; j < ex.k; ++j) {
        a.lpos[j] = ex.lpos[j];
        a.sorted[j] = ex.lpos[j];
        a.my_c |= ((rank >> (ex.gpos[j] - L)) & 1) << j;
    }
    a.nsorted = ex.k;
    if (h) {
        for (uint64_t m = ex.pmask; m; m &= m - 1) a.sorted[a.nsorted++] = __builtin_ctzll(m);
        a.orval = deposit_bits((uint64_t)part, ex.pmask);
    }
    std::sort(a.sorted, a.sorted + a.nsorted);
    for (int c = 0; c < (1 << ex.k); ++c) {
        int peer = rank;
        for (int j = 0; j < ex.k; ++j) {
            const int b = ex.gpos[j] - L;
            peer = (peer & ~(1 << b)) | (((c >> j) & 1) << b);
        }
        x.peer_of[c] = peer;
    }
    return x;
}

std::vector<int> slab_sigma(int L, const DStep& ex) {
    std::vector<int> s(L, -1);
    uint64_t moved = ex.pmask;
    for (int j = 0; j < ex.k; ++j) moved |= 1ull << ex.lpos[j];
    const int m = __builtin_popcountll(ex.pmask);
    int k = 0;
    for (int p = 0; p < L; ++p)
        if (!((moved >> p) & 1ull)) s[p] = k++;
    for (int j = 0; j < ex.k; ++j) s[ex.lpos[j]] = L - m - ex.k + j;
    int i = 0;
    for (uint64_t mm = ex.pmask; mm; mm &= mm - 1) s[__builtin_ctzll(mm)] = L - m + i++;
    return s;
}

// ---- the C entries' guards -------------------------------------------------------------------
int log2_exact(int w) {
    if (w < 1) fail(QSIM_ERR_INVALID_ARGUMENT, "world size must be positive");
    int g = 0;
    while ((1 << g) < w) ++g;
    if ((1 << g) != w) fail(QSIM_ERR_INVALID_ARGUMENT, "world size must be a power of two");
    return g;
}
void check_sizes(int n, int g) {
    if (n < QSIM_MIN_QUBITS || n > QSIM_MAX_QUBITS_DIST)
        fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits out of range");
    if (n - g < std::max(1, g))
        fail(QSIM_ERR_INVALID_ARGUMENT, "too few qubits per rank for this world size");
}
std::vector<int> checked_perm(int n, const int32_t* perm) {
    std::vector<int> p(n);
    uint64_t seen = 0;
    for (int q = 0; q < n; ++q) {
        p[q] = perm ? perm[q] : q;
        if (p[q] < 0 || p[q] >= n || ((seen >> p[q]) & 1ull)) fail(QSIM_ERR_INVALID_ARGUMENT, "qubit map is not a permutation");
        seen |= 1ull << p[q];
    }
    return p;
}
HostPlanArgs::HostPlanArgs(int n, int world, int rank, const int32_t* perm_inout) : g(log2_exact(world)), L(n - g) {
    check_sizes(n, g);
    if (rank < 0 || rank >= world) fail(QSIM_ERR_INVALID_ARGUMENT, "rank out of range");
    perm.resize(n);
    for (int q = 0; q < n; ++q) perm[q] = perm_inout ? perm_inout[q] : q;
}
}  // namespace qsim_hip

using namespace qsim_hip;
extern "C" {

int qsim_dist_plan(int n, int world, int rank, const qsim_gate* gates, size_t count,
                   int32_t* perm_inout, qsim_dist_step* steps, size_t step_cap, size_t* n_steps,
                   qsim_op* ops, size_t op_cap, size_t* n_ops) {
    return guarded([&] {
        HostPlanArgs a(n, world, rank, perm_inout);
        const std::vector<DStep> st = plan_dist(gates, count, n, a.g, rank, a.perm);
        size_t si = 0, oi = 0;
        for (const DStep& s : st) {
            if (si < step_cap) {
                qsim_dist_step& o = steps[si];
                std::memset(&o, 0, sizeof(o));
                o.kind = s.kind;
                o.k = s.k;
                o.op_begin = (int32_t)oi;
                o.op_end = (int32_t)(oi + s.ops.size());
                for (int j = 0; j < 8; ++j) {
                    o.gpos[j] = s.gpos[j];
                    o.lpos[j] = s.lpos[j];
                }
                o.pivot = s.pivot;
                o.pmask = s.pmask;
                o.coarse = s.coarse;
                o.role = s.role;
            }
            for (const Op& op : s.ops) {
                if (oi < op_cap) {
                    qsim_op& r = ops[oi];
                    r.kind = op.kind;
                    r.sub = op.sub;
                    r.t0 = op.t0;
                    r.t1 = op.t1;
                    r.cmask = op.cmask;
                    r.d0_one = op.d0_one ? 1 : 0;
                    r.src = op.src;
                    for (int j = 0; j < 8; ++j) r.m[j] = op.m[j];
                }
                ++oi;
            }
            ++si;
        }
        if (n_steps) *n_steps = si;
        if (n_ops) *n_ops = oi;
        a.store(perm_inout);
    });
}

static int plan_passes_impl(int n, int world, int rank, const qsim_gate* gates, size_t count, int32_t* perm_inout,
                            uint64_t* carry_inout, int32_t* passes, size_t cap, size_t* n_steps, int width) {
    return guarded([&] {
        HostPlanArgs a(n, world, rank, perm_inout);
        const uint64_t carry = carry_inout ? *carry_inout : 0ull;
        const std::vector<DStep> st = plan_dist(gates, count, n, a.g, rank, a.perm, carry);
        for (size_t k = 0; k < st.size(); ++k) {
            int np = 0, head = 0, tail = 0, coarse = 0, coarse_bits = 0;
            if (st[k].kind == 0 && !st[k].ops.empty()) {  // the plan and the split of the run (run_dist)
                const uint64_t pb = (st[k].role & 2) ? (k == 0 ? carry : st[k - 1].pmask) : 0ull;
                const uint64_t pa = (st[k].role & 1) ? st[k + 1].pmask : 0ull;
                const uint64_t cb = pa ? (st[k + 1].coarse & pa) : 0ull;
                const Plan pl = plan_fused(st[k].ops, a.L, -1, pa, pb);
                const PassSplit sp = split_passes(pl, pb, pa, cb, true);
                np = (int)sp.np;
                head = (int)sp.j1;
                tail = (int)(sp.np - sp.j2);
                coarse = (int)(sp.j2 - sp.jc);
                coarse_bits = __builtin_popcountll(cb);
                static const bool dbg = std::getenv("QSIM_DIST_DEBUG_PASSES") != nullptr;
                if (dbg && pa) {  // the exchange-after pivots each pass touches
                    std::string line = "[passes] step " + std::to_string(k) + " pa " + std::to_string(pa) + ":";
                    for (int j = 0; j < np; ++j)
                        line += " " + std::to_string(__builtin_popcountll(pass_touches(pl.passes[j], pa)));
                    std::fprintf(stderr, "%s\n", line.c_str());
                }
            }
            if (k < cap && passes) {
                passes[width * k] = st[k].kind == 1 ? -1 : np;
                passes[width * k + 1] = head;
                passes[width * k + 2] = tail;
                if (width >= 5) {
                    passes[width * k + 3] = coarse;
                    passes[width * k + 4] = coarse_bits;
                }
            }
        }
        if (n_steps) *n_steps = st.size();
        a.store(perm_inout);
        if (carry_inout) *carry_inout = carried_pivots(st);
    });
}

int qsim_dist_plan_passes_carry(int n, int world, int rank, const qsim_gate* gates, size_t count,
                                int32_t* perm_inout, uint64_t* carry_inout, int32_t* passes, size_t cap,
                                size_t* n_steps) {
    return plan_passes_impl(n, world, rank, gates, count, perm_inout, carry_inout, passes, cap, n_steps, 3);
}

int qsim_dist_plan_passes_coarse(int n, int world, int rank, const qsim_gate* gates, size_t count,
                                 int32_t* perm_inout, uint64_t* carry_inout, int32_t* passes, size_t cap,
                                 size_t* n_steps) {
    return plan_passes_impl(n, world, rank, gates, count, perm_inout, carry_inout, passes, cap, n_steps, 5);
}

int qsim_dist_plan_passes(int n, int world, int rank, const qsim_gate* gates, size_t count,
                          int32_t* perm_inout, int32_t* passes, size_t cap, size_t* n_steps) {
    return qsim_dist_plan_passes_carry(n, world, rank, gates, count, perm_inout, nullptr, passes, cap, n_steps);
}

int qsim_dist_plan_memo_clear(void) {
    return guarded([&] {
        std::lock_guard<std::mutex> l(g_pivot_mu);
        g_pivots.clear();
        g_cycles.clear();
    });
}

int qsim_dist_slab_map(int n, int world, int rank, const qsim_dist_step* step, int part,
                       int32_t* my_c, int32_t* peer_of, uint64_t* index, size_t index_cap) {
    return guarded([&] {
        const HostPlanArgs a(n, world, rank);
        if (!step || step->kind != 1 || step->k < 1 || step->k > a.g)
            fail(QSIM_ERR_INVALID_ARGUMENT, "not an exchange step");
        const int L = a.L;
        DStep ex;
        ex.kind = 1;
        ex.k = step->k;
        uint64_t used = 0;
        for (int j = 0; j < ex.k; ++j) {
            ex.gpos[j] = step->gpos[j];
            ex.lpos[j] = step->lpos[j];
            if (ex.gpos[j] < L || ex.gpos[j] >= n || ex.lpos[j] < 0 || ex.lpos[j] >= L ||
                ((used >> ex.lpos[j]) & 1ull))
                fail(QSIM_ERR_INVALID_ARGUMENT, "bad exchange positions");
            used |= 1ull << ex.lpos[j];
        }
        ex.pmask = step->pmask;
        if (ex.pmask & (used | ~((1ull << L) - 1)))
            fail(QSIM_ERR_INVALID_ARGUMENT, "bad pivot mask");
        const int m = __builtin_popcountll(ex.pmask);
        if (part >= (1 << m)) fail(QSIM_ERR_INVALID_ARGUMENT, "part out of range");
        const XPlan x = xplan(L, rank, ex, part < 0 ? -1 : part);
        if (my_c) *my_c = x.a.my_c;
        if (peer_of)
            for (int c = 0; c < (1 << ex.k); ++c) peer_of[c] = x.peer_of[c];
        const uint64_t count = (uint64_t)x.a.chunk << ex.k;
        if (index) {
            if (index_cap < count) fail(QSIM_ERR_INVALID_ARGUMENT, "index buffer too small");
            for (uint64_t e = 0; e < count; ++e) index[e] = xlocal(x.a, e);
        }
    });
}

}  // extern "C"
