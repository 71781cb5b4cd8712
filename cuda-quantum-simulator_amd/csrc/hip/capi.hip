// capi.hip — the extern "C" entries of the fused planner (fused.hip): its view of a circuit and
// the tile settings.  They stay out of fused.hip, the largest file of the library; every other
// entry lives beside the code it calls (file map: DESIGN.md).
#include <vector>

#include "state.hpp"

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

}  // extern "C"
