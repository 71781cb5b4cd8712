// density.hip — DensityMatrix / DensityMatrixSimulator (reference include/DensityMatrix.cuh:63-224,
// src/DensityMatrix.cu) on the state-vector engine.
//
// Layout: rho (2^n x 2^n, row-major like the reference, src/DensityMatrix.cu:29-30) is the vector
// of a qsim_state with 2n index bits, v[i * 2^n + j] = rho[i][j]: bits 0..n-1 are the column j,
// bits n..2n-1 the row i.  U rho U^dag is U on row bit q+n and conj(U) on column bit q — two
// ordinary engine ops — and every channel of the reference is a short sequence of controlled 2x2 /
// diagonal ops on the bit pair (r = q+n, c = q): CNOT(c -> r) maps the element pairs
// (rho_rc, rho_r'c') (r' = 1-r, c' = 1-c) onto pairs along c and marks the off-diagonal elements
// by r ^ c.  A density-matrix circuit is therefore an op list for the same fused LDS tile passes,
// circuit-specialised kernels and per-gate kernels as a 2n-qubit state (no 4^n-thread kernels);
// 4^15 x 16 B = 16 GiB fits one MI355X (the reference stops at 14, :25-27).
//
// Reference semantics kept: gates X..Rz, CNOT, CZ, SWAP (others throw runtime_error, :264-266);
// after each gate, for each of its qubits, every channel that applies to the qubit (empty qubit
// list = all, :201-212, :269-296); depolarizing scales the off-diagonal by 1 - 4p/3 and leaves the
// diagonal (:978-1002); amplitude damping rho00 += g rho11, rho11 *= 1 - g, off-diagonal *=
// sqrt(1 - g) (:1004-1044; the reference reads rho11 racily, here the pre-channel value); phase
// damping / phase flip scale the off-diagonal by sqrt(1 - g) / 1 - 2p (:1046-1065, :1102-1122); bit
// flip mixes rho_rc with rho_r'c' (:1067-1100); bit-phase flip is the phase-flip channel
// (:343-356).  Divergence: Y acts as Y rho Y^dag; the reference kernel's phase table (:540-544)
// returns -(Y rho Y^dag) (trace -1; untested there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "engine.hpp"
#include "state.hpp"
#include "qsim_hip.h"

namespace qsim_hip {

static Op dm_row(Op o, int n) {  // the op on the row bits
    o.t0 += n;
    if (o.t1 >= 0) o.t1 += n;
    o.cmask <<= n;
    return o;
}
static Op dm_col(Op o) {  // conj(op) on the column bits
    for (int i = 1; i < 8; i += 2) o.m[i] = -o.m[i];
    if (o.kind == K_M1 && o.sub == S_Y) o.sub = S_GEN;  // conj(Y) = [[0, i], [-i, 0]]
    if (o.kind == K_DIAG) {
        if (o.sub == S_I) o.sub = S_MI;
        else if (o.sub == S_MI) o.sub = S_I;
        else if (o.sub == S_T) o.sub = S_TDG;
        else if (o.sub == S_TDG) o.sub = S_T;
    }
    return o;
}

static void dm_channel(std::vector<Op>& out, int n, int type, int q, double p) {
    const int r = q + n, c = q;
    auto m1 = [&](int t, uint64_t cm, double a, double b, double cc, double d, int sub = S_GEN) {
        Op o;
        o.kind = K_M1;
        o.sub = sub;
        o.t0 = t;
        o.cmask = cm;
        const double v[8] = {a, 0, b, 0, cc, 0, d, 0};
        for (int i = 0; i < 8; ++i) o.m[i] = v[i];
        out.push_back(o);
    };
    auto cx = [&]() { m1(r, 1ull << c, 0, 1, 1, 0, S_X); };
    auto diag = [&](double d0, double d1) {
        Op o;
        o.kind = K_DIAG;
        o.sub = S_GEN;
        o.t0 = r;
        o.d0_one = d0 == 1.0;
        o.m[0] = d0;
        o.m[2] = d1;
        out.push_back(o);
    };
    switch (type) {
        case 0: cx(); diag(1.0, 1.0 - 4.0 * p / 3.0); cx(); break;          // depolarizing (ref.)
        case 1:                                                              // amplitude damping
            cx();
            m1(r, 0, 0, 1, 1, 0, S_X);                   // r' = r ^ c ^ 1: 1 on the diagonal block
            m1(c, 1ull << r, 1.0, p, 0.0, 1.0 - p);      // [rho00, rho11] <- [[1, g], [0, 1-g]]
            diag(std::sqrt(1.0 - p), 1.0);               // off-diagonal elements
            m1(r, 0, 0, 1, 1, 0, S_X);
            cx();
            break;
        case 2: cx(); diag(1.0, std::sqrt(1.0 - p)); cx(); break;           // phase damping
        case 3: cx(); m1(c, 0, 1.0 - p, p, p, 1.0 - p); cx(); break;        // bit flip
        case 4: case 5: cx(); diag(1.0, 1.0 - 2.0 * p); cx(); break;       // phase / bit-phase flip
        default: fail(QSIM_ERR_INVALID_ARGUMENT, "unknown noise type");
    }
}

// tags (introspection, may be null): one entry per op pushed, the gate it follows and where it came
// from (the origin word of qsim_dm_plan_stage_info).
void dm_lower(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* ch,
              size_t nch, std::vector<Op>& out, bool reference_y, std::vector<StageInfoTag>* tags) {
    auto tag = [&](size_t gate, int origin, int qubit) {  // the ops pushed since the last call
        for (int seq = 0; tags && tags->size() < out.size(); ++seq)
            tags->push_back(StageInfoTag{(int32_t)gate, origin | (qubit << 8) | (seq << 16)});
    };
    for (size_t c = 0; c < nch; ++c) {
        if (ch[c].type < 0 || ch[c].type > 5) fail(QSIM_ERR_INVALID_ARGUMENT, "unknown noise type");
        if (ch[c].qubit < -1 || ch[c].qubit >= n)
            fail(QSIM_ERR_OUT_OF_RANGE, "Qubit index " + std::to_string(ch[c].qubit) + " out of range");
    }
    for (size_t i = 0; i < count; ++i) {
        const qsim_gate& g = gates[i];
        if (g.type == QSIM_GATE_CRY || g.type == QSIM_GATE_CRZ || g.type == QSIM_GATE_TOFFOLI)
            fail(QSIM_ERR_RUNTIME, "Gate not supported in density matrix simulation");
        Op o = lower_gate(g, n);
        o.src = (int)i;
        out.push_back(dm_row(o, n));
        tag(i, QSIM_DM_ORIGIN_ROW, g.qubits[g.nqubits - 1]);
        out.push_back(dm_col(o));
        tag(i, QSIM_DM_ORIGIN_COL, g.qubits[g.nqubits - 1]);
        if (reference_y && g.type == QSIM_GATE_Y) {  // dmApplyY's extra sign (-Y rho Y^dag)
            Op neg;
            neg.kind = K_DIAG;
            neg.sub = S_GEN;
            neg.t0 = 0;
            neg.d0_one = false;
            neg.m[0] = neg.m[2] = -1.0;
            neg.src = (int)i;
            out.push_back(neg);
            tag(i, QSIM_DM_ORIGIN_SIGN, 0);
        }
        for (int k = 0; k < g.nqubits; ++k)
            for (size_t c = 0; c < nch; ++c)
                if (ch[c].qubit < 0 || ch[c].qubit == g.qubits[k]) {
                    dm_channel(out, n, ch[c].type, g.qubits[k], ch[c].probability);
                    tag(i, QSIM_DM_ORIGIN_CHANNEL + ch[c].type, g.qubits[k]);
                }
    }
}

void dm_lower_channel(int n, int type, int qubit, double p, std::vector<Op>& out) {
    if (qubit < 0 || qubit >= n) fail(QSIM_ERR_OUT_OF_RANGE, "Qubit index " + std::to_string(qubit) + " out of range");
    dm_channel(out, n, type, qubit, p);
}

__global__ __launch_bounds__(256) void k_dm_diag(const double2* rho, uint64_t dim, double* out) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += step)
        out[i] = rho[i * (dim + 1)].x;
}

// rho[i][j] = psi_i conj(psi_j) (dmInitPure, src/DensityMatrix.cu:412-425) or, psi == null, I / dim.
__global__ __launch_bounds__(256) void k_dm_init(double2* rho, const double2* psi, int n) {
    const uint64_t dim = 1ull << n, total = dim << n;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        const uint64_t i = k >> n, j = k & (dim - 1);
        if (psi) {
            const double2 si = psi[i], sj = psi[j];
            rho[k] = make_double2(si.x * sj.x + si.y * sj.y, si.y * sj.x - si.x * sj.y);
        } else {
            rho[k] = make_double2(i == j ? 1.0 / (double)dim : 0.0, 0.0);
        }
    }
}

void launch_dm_diag(const double2* rho, int n, double* out, hipStream_t s) {
    const uint64_t dim = 1ull << n;
    const unsigned blocks = (unsigned)std::min<uint64_t>((dim + 255) / 256, 1024);
    hipLaunchKernelGGL(k_dm_diag, dim3(blocks), dim3(256), 0, s, rho, dim, out);
    QSIM_HIPCHK(hipGetLastError());
}

void launch_dm_init(double2* rho, const double2* psi, int n, hipStream_t s) {
    const uint64_t total = 1ull << (2 * n);
    const unsigned blocks = (unsigned)std::min<uint64_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(k_dm_init, dim3(blocks), dim3(256), 0, s, rho, psi, n);
    QSIM_HIPCHK(hipGetLastError());
}

}  // namespace qsim_hip

// ---- rho on a single-GPU state of 2n qubits: the relabeling policy and the C entries ----
namespace qsim_hip {
void check_dm(const qsim_state* s, int n) {
    check_state(s);
    if (n < 1 || n > QSIM_DM_MAX_QUBITS)
        fail(QSIM_ERR_INVALID_ARGUMENT, "Density matrix supports 1-" + std::to_string(QSIM_DM_MAX_QUBITS) + " qubits");
    if (s->n != 2 * n) fail(QSIM_ERR_INVALID_ARGUMENT, "density matrix state must have 2n qubits");
}

// An op with every index bit moved through pi (bit b -> position pi[b]).
static Op permute_op(Op o, const std::vector<int>& pi) {
    o.t0 = pi[o.t0];
    if (o.t1 >= 0) o.t1 = pi[o.t1];
    uint64_t m = 0;
    for (uint64_t c = o.cmask; c; c &= c - 1) m |= 1ull << pi[__builtin_ctzll(c)];
    o.cmask = m;
    return o;
}
// Density-matrix relabeling: the 2n index bits of rho under a permutation that plans the lowered
// circuit (dm_lower above) into fewer passes — the state-vector search (relabel.hip
// choose_layout: seeded random labelings, the fewest-pass ones annealed on the layout cost
// model) over bit positions rather than qubits, so row and column bits move independently.
// QSIM_DM_RELABEL_TRIES labelings (default 48, about 1 s of host planning at 14 qubits; 256 when
// the candidates are timed on the device — more fewest-pass candidates to time: 14q 9.19k ->
// 9.52k gates/s); 0 turns it off.
// Below 24 index bits (rho of <= 11 qubits: ~1 ms passes) a quarter of that (the search
// is paid on the first run of every new circuit structure).
static int dm_relabel_tries(int nbits, bool timed = false) {
    static const int v = [] {  // (-1: not set)
        const char* e = std::getenv("QSIM_DM_RELABEL_TRIES");
        return e ? std::max(0, std::atoi(e)) : -1;
    }();
    if (v >= 0) return v;
    const int full = timed ? 256 : 48;
    return nbits >= 24 ? full : full / 4;
}
// The DM relabeling follows the state-vector relabel policy (qsim_set_relabel / QSIM_RELABEL: mode
// 0 turns it off) with its own size floor in index bits (QSIM_DM_RELABEL_MIN_BITS, default 16:
// rho of 8 qubits).
static bool dm_relabel_enabled(int nbits) {
    static const int min_bits = std::max(2, env_int("QSIM_DM_RELABEL_MIN_BITS", 16));
    return relabel_mode_on() && nbits >= min_bits && dm_relabel_tries(nbits) > 0;
}
static LayoutChoice dm_choose_layout(int nbits, const std::vector<Op>& ops, size_t want_alts = 0) {
    auto lower = [&](const std::vector<int>& pi) {
        std::vector<Op> out;
        out.reserve(ops.size());
        for (const Op& o : ops) out.push_back(permute_op(o, pi));
        return out;
    };
    // QSIM_DM_STAGE_US (default 1000, layout-cost units per register stage; 0: cost alone): the
    // round-5 timed candidates at 14 qubits ran ~0.1 ms longer per stage and per 1 000 units of
    // predicted cost (profiles/r05/dm_relabel/sweep, stage counts from QSIM_DM_CAND_DEBUG)
    static const double stage_us = [] {
        const char* e = std::getenv("QSIM_DM_STAGE_US");
        return e ? std::max(0.0, std::atof(e)) : 1000.0;
    }();
    return choose_layout(nbits, lower, dm_relabel_tries(nbits, want_alts > 0), want_alts, stage_us);
}
// The checks and the lowering that the host-only entries below start with.
static std::vector<Op> dm_lower_checked(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                                        size_t n_channels, int flags, std::vector<StageInfoTag>* tags = nullptr) {
    if (n < 1 || n > QSIM_DM_MAX_QUBITS) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
    QSIM_REQUIRE(gates || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate list");
    QSIM_REQUIRE(channels || n_channels == 0, QSIM_ERR_INVALID_ARGUMENT, "null channel list");
    std::vector<Op> ops;
    dm_lower(n, gates, count, channels, n_channels, ops, (flags & QSIM_DM_REFERENCE_Y) != 0, tags);
    return ops;
}
// The plan qsim_dm_run's fused path executes for these ops when the state lies under the labels
// `perm` of the 2n index bits (logical -> physical; null: the identity).  pi: the labels checked.
static Plan dm_plan_under(int n, std::vector<Op>& ops, const int32_t* perm, std::vector<int>& pi) {
    pi.resize(2 * n);
    for (int b = 0; b < 2 * n; ++b) pi[b] = perm ? perm[b] : b;
    std::vector<int> chk(pi);
    std::sort(chk.begin(), chk.end());
    for (int b = 0; b < 2 * n; ++b)
        if (chk[b] != b) fail(QSIM_ERR_INVALID_ARGUMENT, "perm is not a permutation");
    if (perm)
        for (Op& o : ops) o = permute_op(o, pi);
    const int th = tile_height_for(2 * n);
    const TileHeightScope tile_h(th, tile_rb_for(2 * n, th));
    return plan_fused(ops, 2 * n);
}
}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_dm_run(qsim_state* s, int n, const qsim_gate* gates, size_t count,
                const qsim_noise_channel* channels, size_t n_channels, int flags) {
    return guarded([&] {
        check_dm(s, n);
        QSIM_REQUIRE(gates || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        QSIM_REQUIRE(channels || n_channels == 0, QSIM_ERR_INVALID_ARGUMENT, "null channel list");
        DeviceGuard dg(s->device);
        share_flush(s);
        std::vector<Op> ops;
        dm_lower(n, gates, count, channels, n_channels, ops, (flags & QSIM_DM_REFERENCE_Y) != 0);
        // the state-vector size rule for the 2n index bits (13-qubit tiles for 26-28 bits: DM 13-14
        // qubits; W-HC + depolarizing at 14 qubits 6.87 k -> 7.35 k gates/s, 8 -> 7 passes)
        const int th = tile_height_for(s->n);
        const TileHeightScope tile_h(th, tile_rb_for(s->n, th));
        // First fused run on |0><0| (a reset rho: basis index 0, which every labeling leaves at 0):
        // choose the index-bit labels (dm_choose_layout; W-HC + depolarizing 14q: 7 -> 6 passes),
        // memoised per (circuit, channels, flags).  Later runs keep the labels and map their ops
        // through them; readers restore the identity first (prep).  A pinned state (handed-out
        // device pointer) is never relabeled.
        const bool fresh = (flags & QSIM_RUN_FUSED) && !s->pinned && s->basis && s->basis_idx == 0 &&
                           s->perm.empty() && count > 0 && dm_relabel_enabled(s->n);
        if (fresh) {
            // memo key: the circuit's STRUCTURE (gate types and qubits, channel types and qubits,
            // flags) — not rotation angles or probabilities, so a parameter sweep (reset + run with
            // new angles) reuses the labels instead of searching again; any labels are exact, the
            // structure is what they were chosen for
            std::vector<int32_t> key;
            key.reserve(4 * count + 2 * n_channels + 2);
            for (size_t i = 0; i < count; ++i) {
                key.push_back(gates[i].type);
                for (int j = 0; j < 3; ++j) key.push_back(j < gates[i].nqubits ? gates[i].qubits[j] : -1);
            }
            for (size_t i = 0; i < n_channels; ++i) {
                key.push_back(channels[i].type);
                key.push_back(channels[i].qubit);
            }
            key.push_back((int32_t)count);
            key.push_back(flags);
            std::vector<int> memo;
            if (layout_memo_get(s->n, 3, key.data(), key.size() * sizeof(int32_t), memo, nullptr)) {
                s->perm = memo;
            } else {
                // with layout calibration (inline compilation, >= 26 index bits by default) the
                // fewest-pass candidates are timed on the device, as a state vector's are: the
                // cost model prices run lengths, not the register stages that DM passes spend
                // most of their time in (QSIM_DM_RELABEL_CANDIDATES, default 8; 14q: the 6-pass
                // candidates run 10.4-11.9 ms)
                static const size_t alts = (size_t)std::max(1, env_int("QSIM_DM_RELABEL_CANDIDATES", 8)) - 1;
                LayoutChoice lc = dm_choose_layout(s->n, ops, relabel_calibrate(s->n) ? alts : 0);
                if (!lc.perm.empty() && !lc.alts.empty()) {
                    std::vector<LayoutCandidate> cands;
                    cands.push_back(LayoutCandidate{th, lc.perm, std::move(lc.ops), std::move(lc.plan), false});
                    for (LayoutChoice::Alt& a : lc.alts)
                        cands.push_back(LayoutCandidate{th, a.perm, std::move(a.ops), std::move(a.plan), false});
                    s->perm = cands[calibrate_candidates(s, cands)].perm;  // (every plan stays cached)
                    s->calibrated = true;
                } else if (!lc.perm.empty()) {
                    s->plans.put(lc.ops, s->n, std::move(lc.plan), s->stream);
                    s->perm = lc.perm;
                }
                layout_memo_put(s->n, 3, key.data(), key.size() * sizeof(int32_t), s->perm, -1);
            }
        } else if (s->pinned || s->relayout) {
            prep(s, true);  // (identity labels; a relayout-plan layout is the state vector's own)
        }
        s->basis = false;
        if (!s->perm.empty())
            for (Op& o : ops) o = permute_op(o, s->perm);
        if (flags & QSIM_RUN_FUSED) run_fused(s, ops);
        else for (const Op& op : ops) launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
    });
}

int qsim_dm_plan_info(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                      size_t n_channels, int flags, int32_t* info, size_t cap, size_t* n_passes) {
    return guarded([&] {
        const std::vector<Op> ops = dm_lower_checked(n, gates, count, channels, n_channels, flags);
        const int th = tile_height_for(2 * n);
        const TileHeightScope tile_h(th, tile_rb_for(2 * n, th));
        Plan plan;
        LayoutChoice lc;
        if (flags & QSIM_DM_PLAN_RELABELED) {
            // (QSIM_DM_CAND_DEBUG: every candidate the timed first run would time, in its order:
            // passes, register stages per pass, layout cost)
            static const bool dbg = std::getenv("QSIM_DM_CAND_DEBUG") != nullptr;
            static const size_t nalt = (size_t)std::max(1, env_int("QSIM_DM_CAND_DEBUG", 1));
            lc = dm_choose_layout(2 * n, ops, dbg ? nalt - 1 : 0);
            if (dbg && !lc.perm.empty()) {
                auto show = [&](size_t k, const Plan& pl) {
                    int st = 0;
                    std::string per;
                    for (const FusedPass& fp : pl.passes) {
                        st += fp.stage_end - fp.stage_begin;
                        per += " " + std::to_string(fp.stage_end - fp.stage_begin);
                    }
                    std::fprintf(stderr, "[dmcand] %zu passes %zu stages %d (%s ) cost %.1f\n", k, pl.passes.size(), st,
                                 per.c_str(), plan_layout_cost_us(pl));
                };
                show(0, lc.plan);
                for (size_t a = 0; a < lc.alts.size(); ++a) show(a + 1, lc.alts[a].plan);
            }
        }
        if (!lc.perm.empty()) plan = std::move(lc.plan);
        else plan = plan_fused(ops, 2 * n);  // (as qsim_dm_run's run_fused plans it)
        for (size_t p = 0; p < plan.passes.size() && p < cap && info; ++p) {
            const FusedPass& fp = plan.passes[p];
            int nops = 0;
            for (int st = fp.stage_begin; st < fp.stage_end; ++st) nops += plan.stages[st].op_end - plan.stages[st].op_begin;
            if (fp.stage_end == fp.stage_begin) nops = fp.op_end - fp.op_begin;
            info[4 * p] = fp.single >= 0 ? -1 : fp.h;
            info[4 * p + 1] = nops;
            info[4 * p + 2] = fp.stage_end - fp.stage_begin;
            info[4 * p + 3] = fp.r0;
        }
        if (n_passes) *n_passes = plan.passes.size();
    });
}

int qsim_dm_jit_source(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                       size_t n_channels, int flags, char* buf, size_t cap, size_t* len) {
    return guarded([&] {
        const std::vector<Op> ops = dm_lower_checked(n, gates, count, channels, n_channels, flags);
        const int th = tile_height_for(2 * n);
        const TileHeightScope tile_h(th, tile_rb_for(2 * n, th));
        copy_source(jit_source(plan_fused(ops, 2 * n)), buf, cap, len);
    });
}

int qsim_dm_plan_stage_info(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                            size_t n_channels, int flags, const int32_t* perm, int32_t* ops, size_t op_cap,
                            size_t* n_ops, int32_t* passes, size_t pass_cap, size_t* n_passes, int32_t* stages,
                            size_t stage_cap, size_t* n_stages) {
    return guarded([&] {
        std::vector<StageInfoTag> tags;
        std::vector<Op> lowered = dm_lower_checked(n, gates, count, channels, n_channels, flags, &tags);
        // (an op's src is read by nothing but the Pauli-frame arms: here it names the lowered op)
        for (size_t k = 0; k < lowered.size(); ++k) lowered[k].src = (int)k;
        std::vector<int> pi;
        const Plan plan = dm_plan_under(n, lowered, perm, pi);
        write_stage_info(plan, &tags, ops, op_cap, n_ops, passes, pass_cap, n_passes, stages, stage_cap, n_stages);
    });
}

int qsim_dm_plan_exec_host(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                           size_t n_channels, int flags, const int32_t* perm, double* amps, int* passes) {
    return guarded([&] {
        QSIM_REQUIRE(amps, QSIM_ERR_INVALID_ARGUMENT, "null amplitudes");
        std::vector<Op> lowered = dm_lower_checked(n, gates, count, channels, n_channels, flags);
        if (2 * n < 10 || 2 * n > 26) fail(QSIM_ERR_INVALID_ARGUMENT, "host execution: 10..26 index bits");
        std::vector<int> pi;
        const Plan plan = dm_plan_under(n, lowered, perm, pi);
        exec_plan_on_host(plan, 2 * n, amps, perm ? pi.data() : nullptr);
        if (passes) *passes = (int)plan.passes.size();
    });
}

int qsim_dm_apply_channel(qsim_state* s, int n, int type, int qubit, double p) {
    return guarded([&] {
        check_dm(s, n);
        DeviceGuard dg(s->device);
        prep(s, true);
        std::vector<Op> ops;
        dm_lower_channel(n, type, qubit, p, ops);
        for (const Op& op : ops) launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
    });
}

int qsim_dm_diagonal(qsim_state* s, int n, double* dst) {
    return guarded([&] {
        check_dm(s, n);
        QSIM_REQUIRE(dst, QSIM_ERR_INVALID_ARGUMENT, "null destination");
        DeviceGuard dg(s->device);
        prep(s, false);
        double* d_p = (double*)s->scratch.get(sizeof(double) << n, s->stream);
        launch_dm_diag(s->d, n, d_p, s->stream);
        QSIM_HIPCHK(hipMemcpyAsync(dst, d_p, sizeof(double) << n, hipMemcpyDeviceToHost, s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

int qsim_dm_init_pure(qsim_state* s, int n, const double* psi) {
    return guarded([&] {
        check_dm(s, n);
        QSIM_REQUIRE(psi, QSIM_ERR_INVALID_ARGUMENT, "null state");
        DeviceGuard dg(s->device);
        drop_layout(s);
        double2* d_psi = (double2*)s->scratch.get(sizeof(double2) << n, s->stream);
        QSIM_HIPCHK(hipMemcpyAsync(d_psi, psi, sizeof(double2) << n, hipMemcpyHostToDevice, s->stream));
        launch_dm_init(s->d, d_psi, n, s->stream);
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

int qsim_dm_init_maximally_mixed(qsim_state* s, int n) {
    return guarded([&] {
        check_dm(s, n);
        DeviceGuard dg(s->device);
        drop_layout(s);
        launch_dm_init(s->d, nullptr, n, s->stream);
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

}  // extern "C"
