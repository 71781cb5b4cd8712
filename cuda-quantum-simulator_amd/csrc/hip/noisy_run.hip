// noisy_run.hip — the noisy trajectory run on a single-GPU state (qsim_noisy_run, qsim_noise_apply):
// which of noise.hip's paths a run takes (in-tile, pulled, pushed) and the buffers the first two
// keep on the state (its NoiseSide and the second 2^n buffer).  The kernels, their launchers and
// the schedules of the in-tile and pulled runs are noise.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "state.hpp"

using namespace qsim_hip;

// Buffers of the pulled noise path: the second state buffer, two sets of per-step code words.
static bool ensure_noise_buffers(qsim_state* s, size_t nch) {
    const size_t state_b = sizeof(double2) << s->n;
    const size_t codes_b = pull_noise_codes_bytes(s->n, 1, nch);
    // Allocate only when the device keeps room for another state of this size beside the new
    // buffers — the rule trim_noise_buffers keeps them by — so a device with between one and two
    // states of room runs the push kernels instead of allocating and freeing a second state on
    // every run.
    const size_t need = (s->alt ? 0 : state_b) + (codes_b > s->noise.codes_cap ? 2 * codes_b : 0);
    if (need && device_free_bytes() < need + state_b + kAltMarginBytes) return false;
    if (!ensure_alt(s) || !s->noise.ensure_codes(codes_b, s->stream)) return false;
    s->noise.ensure_stream(false);
    return true;
}

// After a pulled noisy run: free the second buffer (unless a relayout plan owns it) and the
// code words when the device no longer has room for another 2^n buffer beside a margin.
static void trim_noise_buffers(qsim_state* s) {
    // QSIM_NOISE_KEEP_BUFFERS: 1 always keep, 0 always free (tests)
    static const int keep = env_int("QSIM_NOISE_KEEP_BUFFERS", -1);
    if (keep == 1) return;
    if (keep != 0 && device_free_bytes() >= (sizeof(double2) << s->n) + kAltMarginBytes) return;
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    if (s->noise.stream) QSIM_HIPCHK(hipStreamSynchronize(s->noise.stream));
    s->noise.release_codes();
    s->noise.release_lists();
    if (!s->relayout) release_alt(s);
}

// QSIM_NOISY_TILE=1 (from 12 qubits, flip-only models): the in-tile path (noise.hip
// launch_gate_noise_run: the gate and the channel prefix whose qubits lie in its tile in one LDS
// pass, their flips from lists built one step ahead on the side stream — two sets, when they fit
// beside a margin, else the tile kernels walk the draws themselves — the rest pushed one launch
// per channel): the same draws, so the same states as the pulled and pushed paths.  Opt-in: at 26
// qubits with 26 channels the 14-15 per-channel suffix launches (0.04 ms each) outweigh the pull
// pass, 904 vs 1 024 gates/s.  false: not this run (nothing launched).
static bool run_tile(qsim_state* s, const std::vector<Op>& ops, const std::vector<NoiseChan>& chans, uint64_t seed,
                     uint64_t* counter) {
    bool tile = env_switch("QSIM_NOISY_TILE", false) && s->n >= 12;  // (read per run: tests switch it)
    for (const NoiseChan& ch : chans) tile = tile && (ch.type == 0 || ch.type >= 3);
    for (const Op& op : ops) tile = tile && gate_noise_tile_supported(s->n, &op);
    if (!tile) return false;
    const size_t lb = gate_noise_lists_bytes(s->n, 1, chans);
    GnLists L{};
    const bool lists = lb && s->noise.ensure_lists(lb, s->stream);
    if (lists) {
        s->noise.ensure_stream(false);
        L = s->noise.view();
    }
    launch_gate_noise_run(s->d, s->n, 1, 0, ops, chans, seed, *counter, s->stream, &s->timer, lists ? &L : nullptr);
    trim_noise_buffers(s);
    return true;
}

// QSIM_NOISE_MAP_FUSED=1 (opt-in): step i's pass also builds step i + 1's words (its hash-and-log
// walks meant to fill its own memory stalls; noise.hip k_pull_gate<..., MAP>), one stream.
// Measured slower at 26 qubits: 1.22 ms per fused pass against 0.70 + 0.24 ms apart, 815 vs 1 063
// gates/s (the walks and their LDS cost the pass its occupancy), so the default is the word map as
// a kernel of its own, beside the pass (overlap) or before it (launch_pull_noise_run).
static void run_pulled_map_fused(qsim_state* s, const std::vector<Op>& ops, const std::vector<NoiseChan>& chans,
                                 uint64_t seed, uint64_t c0) {
    const size_t G = ops.size();
    launch_noise_map(s->n, 1, 0, chans, seed, c0, s->noise.words(0), s->stream, &s->timer);
    launch_op(s->d, s->n, 1, ops[0], s->stream, &s->timer);
    for (size_t i = 0; i < G; ++i) {
        const PullMapNext nx{0, seed, c0 + (i + 1) * chans.size(), s->noise.words(i + 1)};
        launch_pull_gate(s->d, s->alt, s->n, 1, chans, i + 1 < G ? &ops[i + 1] : nullptr, s->noise.words(i),
                         s->stream, &s->timer, i + 1 < G ? &nx : nullptr);
        std::swap(s->d, s->alt);
    }
}

// Flip channels only: the noise after gate i is applied by gate i+1's pass (out of place), the
// noise after the last gate by one identity pass (noise.hip); the same draws as the per-channel
// passes, so the same state.  false: not this run (nothing launched).
static bool run_pulled(qsim_state* s, const std::vector<Op>& ops, const std::vector<NoiseChan>& chans, uint64_t seed,
                       uint64_t* counter) {
    if (!pull_noise_supported(s->n, chans, true) || !ensure_noise_buffers(s, chans.size())) return false;
    // where the amplitudes are now: a pinned state's handed-out pointer (prep() leaves the
    // amplitudes of a pinned state in the buffer that was handed out, which may be either one)
    double2* const home = s->d;
    // QSIM_NOISE_MAP_OVERLAP=0: the word maps on the state's stream (read per run, as the next
    // one: tests switch them)
    const bool overlap = env_switch("QSIM_NOISE_MAP_OVERLAP", true);
    const uint64_t c0 = *counter;
    *counter += (uint64_t)ops.size() * chans.size();
    if (env_switch("QSIM_NOISE_MAP_FUSED", false) && !ops.empty()) {
        run_pulled_map_fused(s, ops, chans, seed, c0);
    } else {
        double2* const buf[2] = {s->d, s->alt};
        const int at = launch_pull_noise_run(buf, 0, s->n, 1, 0, ops, chans, seed, c0, s->noise, s->stream, &s->timer,
                                             overlap);
        s->d = buf[at];
        s->alt = buf[at ^ 1];
    }
    settle_home(s, home);
    // The second buffer and the code words stay for the next run (qsim_state_memory_bytes counts
    // them) only while the device keeps room for another state of this size beside them;
    // otherwise they are freed now, so a later StateVector does not fail where the reference's
    // single-buffer one would not.
    trim_noise_buffers(s);
    return true;
}

extern "C" {

int qsim_noise_apply(qsim_state* s, int type, int qubit, double probability, uint64_t seed,
                     uint64_t counter) {
    return guarded([&] {
        check_state(s);
        DeviceGuard dg(s->device);
        prep(s, true);
        launch_noise(s->d, s->n, type, qubit, probability, seed, counter, s->stream, &s->timer);
    });
}

int qsim_noisy_run(qsim_state* s, const qsim_gate* gates, size_t count,
                   const qsim_noise_channel* channels, size_t n_channels, uint64_t seed,
                   uint64_t* counter, int flags) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(gates || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        QSIM_REQUIRE(channels || n_channels == 0, QSIM_ERR_INVALID_ARGUMENT, "null channel list");
        QSIM_REQUIRE(counter, QSIM_ERR_INVALID_ARGUMENT, "null counter");
        DeviceGuard dg(s->device);
        prep(s, true);
        const std::vector<Op> ops = lower_gates(s->n, gates, count, {});
        for (size_t c = 0; c < n_channels; ++c) {
            if (channels[c].type < 0 || channels[c].type > 5)
                fail(QSIM_ERR_INVALID_ARGUMENT, "unknown noise type");
            if (channels[c].qubit < 0 || channels[c].qubit >= s->n)
                fail(QSIM_ERR_OUT_OF_RANGE, "Qubit index " + std::to_string(channels[c].qubit) + " out of range");
        }
        if (n_channels == 0) {
            if (flags & QSIM_RUN_FUSED) run_fused(s, ops);
            else for (const Op& op : ops) launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
            return;
        }
        std::vector<NoiseChan> chans;
        for (size_t c = 0; c < n_channels; ++c)
            chans.push_back(NoiseChan{channels[c].type, channels[c].qubit, channels[c].probability});
        if (run_tile(s, ops, chans, seed, counter) || run_pulled(s, ops, chans, seed, counter)) return;
        for (const Op& op : ops) {
            launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
            for (size_t c = 0; c < n_channels; ++c)
                launch_noise(s->d, s->n, channels[c].type, channels[c].qubit, channels[c].probability,
                             seed, (*counter)++, s->stream, &s->timer);
        }
    });
}

}  // extern "C"
