// capi.hip — the extern "C" entries of the fused planner (fused.hip): its view of a circuit and
// the tile settings.  They stay out of fused.hip, the largest file of the library; every other
// entry lives beside the code it calls (file map: DESIGN.md).
#include <vector>

#include "state.hpp"

namespace qsim_hip {
// The three record tables of qsim_plan_stage_info (include/qsim_hip.h) read out of `plan`.  tags
// (density.hip, may be null): Op::src indexes it; its entry gives the source gate index reported in
// field 0 and the origin word of field 15 (an op without a source, src < 0: -1 and 0).
void write_stage_info(const Plan& plan, const std::vector<StageInfoTag>* tags, int32_t* ops, size_t op_cap,
                      size_t* n_ops, int32_t* passes, size_t pass_cap, size_t* n_passes, int32_t* stages,
                      size_t stage_cap, size_t* n_stages) {
    static const uint32_t kFixed[4] = {0x10u, 0x20u, 0x40u, 0x80u};
    size_t ko = 0, ks = 0, kp = 0;
    auto put_op = [&](int pass, int stage, int pos, int src, int kind, int sub, int p0, int b0, int b1,
                      uint32_t cmask, uint32_t cm_reg, uint32_t cm_thr, uint64_t cm_out, int d0_one) {
        if (ops && ko < op_cap) {
            int32_t* r = ops + 16 * ko;
            int32_t origin = 0;
            if (tags) {
                const StageInfoTag t = src >= 0 ? (*tags)[src] : StageInfoTag{-1, 0};
                src = t.gate;
                origin = t.origin;
            }
            const int32_t v[16] = {src, pass, stage, pos, kind, sub, p0, b0, b1, (int32_t)cmask, (int32_t)cm_reg,
                                   (int32_t)cm_thr, (int32_t)(cm_out & 0xffffffffull), (int32_t)(cm_out >> 32),
                                   d0_one, origin};
            for (int i = 0; i < 16; ++i) r[i] = v[i];
        }
        ++ko;
    };
    for (size_t pi = 0; pi < plan.passes.size(); ++pi) {
        const FusedPass& p = plan.passes[pi];
        const bool single = p.single >= 0, staged = !single && p.stage_end > p.stage_begin;
        const size_t op0 = ko;
        int fixed = 0, searched = 0;
        if (single) {
            const Op& o = plan.singles[p.single];
            put_op((int)pi, -1, 3, o.src, o.kind, o.sub, -1, o.t0, o.t1, 0, 0, 0, 0, o.d0_one ? 1 : 0);
        } else if (staged) {
            const int ns = p.stage_end - p.stage_begin;
            for (int s = p.stage_begin; s < p.stage_end; ++s) {
                const Stage& sg = plan.stages[s];
                const int k = s - p.stage_begin;
                const int pos = ns == 1 ? 3 : k == 0 ? 0 : k == ns - 1 ? 2 : 1;
                // the LDS round trip after this stage: 0 none (it stores to HBM), 1 the fixed
                // swizzle, 2 a searched one
                int swz = 0;
                if (k + 1 < ns) {
                    swz = 1;
                    for (int i = 0; i < 4; ++i)
                        if (sg.trow_out[i] != kFixed[i]) swz = 2;
                    (swz == 1 ? fixed : searched) += 1;
                }
                uint32_t sbits = 0;
                for (int i = 0; i < p.rb; ++i) sbits |= 1u << sg.fix[i];
                if (stages && ks < stage_cap) {
                    int32_t* r = stages + 8 * ks;
                    const int32_t v[8] = {(int32_t)pi, k, pos, (int32_t)sbits, sg.op_end - sg.op_begin, swz,
                                          sg.tscatter, 0};
                    for (int i = 0; i < 8; ++i) r[i] = v[i];
                }
                ++ks;
                for (int o = sg.op_begin; o < sg.op_end; ++o) {
                    const TileOp& t = plan.ops[o];
                    put_op((int)pi, k, pos, plan.order[o], t.kind, t.sub, t.p0, t.b0, t.b1, t.cmask, t.cm_reg,
                           t.cm_thr, t.cm_out, t.d0_one);
                }
            }
        } else {
            for (int o = p.op_begin; o < p.op_end; ++o) {
                const TileOp& t = plan.ops[o];
                put_op((int)pi, -1, 3, plan.order[o], t.kind, t.sub, -1, t.b0, t.b1, t.cmask, 0, 0, t.cm_out,
                       t.d0_one);
            }
        }
        if (passes && kp < pass_cap) {
            int32_t* r = passes + 24 * kp;
            for (int i = 0; i < 24; ++i) r[i] = 0;
            r[0] = single ? 1 : 0;
            r[1] = p.h;
            r[2] = p.r0;
            r[3] = staged ? p.rb : 0;
            r[4] = p.hu_count;
            r[5] = p.relayout;
            r[6] = staged ? p.stage_end - p.stage_begin : 0;
            r[7] = (int32_t)(ko - op0);
            r[8] = fixed;
            r[9] = searched;
            r[10] = single ? 0 : 6 + p.h - p.r0;
            for (int i = 0; i < r[10] && i < 10; ++i) r[11 + i] = p.hpos[i];
        }
        ++kp;
    }
    if (n_ops) *n_ops = ko;
    if (n_passes) *n_passes = kp;
    if (n_stages) *n_stages = ks;
}
}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_set_tile_height(int h) {
    return guarded([&] { tile_height_configure(h); });
}

int qsim_set_tile_ctrl_out(int mode) {
    return guarded([&] { tile_ctrl_out_configure(mode); });
}

int qsim_set_tile_rb7(int rb) {
    return guarded([&] { tile_rb7_configure(rb); });
}

int qsim_plan_fused(int n_qubits, const qsim_gate* gates, size_t count, int hmax, int32_t* order,
                    int32_t* pass_of, int32_t* n_passes) {
    return guarded([&] {
        QSIM_REQUIRE(gates || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        if (hmax < 0 || hmax > kTileHMax) fail(QSIM_ERR_INVALID_ARGUMENT, "hmax out of range");
        const Plan plan = plan_fused(lower_gates(n_qubits, gates, count, {}), n_qubits, hmax);
        size_t k = 0;
        int32_t tile = 0;
        for (const FusedPass& p : plan.passes) {
            if (p.single >= 0) {
                if (order) order[k] = plan.singles[p.single].src;
                if (pass_of) pass_of[k] = -1;
                ++k;
                continue;
            }
            auto emit = [&](int o) {
                if (plan.order[o] < 0) return;  // 2nd/3rd controlled-X of a lowered SWAP
                if (order) order[k] = plan.order[o];
                if (pass_of) pass_of[k] = tile;
                ++k;
            };
            if (p.stage_end > p.stage_begin) {
                for (int s = p.stage_begin; s < p.stage_end; ++s)
                    for (int o = plan.stages[s].op_begin; o < plan.stages[s].op_end; ++o) emit(o);
            } else {
                for (int o = p.op_begin; o < p.op_end; ++o) emit(o);
            }
            ++tile;
        }
        if (n_passes) *n_passes = tile;
    });
}

int qsim_plan_stage_info(int n_qubits, const qsim_gate* gates, size_t count, int relayout, int32_t* ops,
                         size_t op_cap, size_t* n_ops, int32_t* passes, size_t pass_cap, size_t* n_passes,
                         int32_t* stages, size_t stage_cap, size_t* n_stages) {
    return guarded([&] {
        QSIM_REQUIRE(gates || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        const int n = n_qubits;
        for (size_t i = 0; i < count; ++i) validate_gate(gates[i], n);
        auto lower = [&](const std::vector<int>& pi) { return lower_gates(n, gates, count, pi); };
        // the plan qsim_run's fused path makes for a state of this size: its height and stage width
        // (run.hip), or the relayout plan of a first run (12-qubit tiles)
        Plan plan;
        if (relayout) {
            const TileHeightScope scope(6, tile_rb_for(n, 6));
            RelayoutChoice rc;
            if (!plan_relayout(n, lower, SIZE_MAX, rc)) fail(QSIM_ERR_RUNTIME, "no relayout plan");
            plan = std::move(rc.plan);
        } else {
            const int th = tile_height_for(n);
            const TileHeightScope scope(th, tile_rb_for(n, th));
            plan = plan_fused(lower({}), n);
        }
        write_stage_info(plan, nullptr, ops, op_cap, n_ops, passes, pass_cap, n_passes, stages, stage_cap, n_stages);
    });
}

}  // extern "C"
