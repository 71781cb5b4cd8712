// noisy_run.hip — the noisy trajectory run on a single-GPU state (qsim_noisy_run, qsim_noise_apply):
// which of noise.hip's paths a run takes (in-tile, pulled, pushed) and the buffers, side stream and
// events the first two keep on the state.  The kernels and their launchers are noise.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "state.hpp"

using namespace qsim_hip;

// The noise side stream and its events (the pulled path's code-word maps, the in-tile path's lists).
static void ensure_noise_stream(qsim_state* s) {
    if (s->noise_stream) return;
    QSIM_HIPCHK(hipStreamCreateWithFlags(&s->noise_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&s->nev_map[0], &s->nev_map[1], &s->nev_pull[0], &s->nev_pull[1], &s->nev_start})
        QSIM_HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
}
// Buffers of the pulled noise path: the second state buffer, two sets of per-step code words.
static bool ensure_noise_buffers(qsim_state* s, size_t nch) {
    const size_t codes_b = pull_noise_codes_bytes(s->n, 1, nch);
    // Allocate only when the device keeps room for another state of this size beside the new
    // buffers — the rule trim_noise_buffers keeps them by — so a device with between one and two
    // states of room runs the push kernels instead of allocating and freeing a second state on
    // every run.
    const size_t need = (s->alt ? 0 : (sizeof(double2) << s->n)) + (codes_b > s->noise_codes_cap ? 2 * codes_b : 0);
    if (need) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (free_b < need + (sizeof(double2) << s->n) + kAltMarginBytes) return false;
    }
    if (!ensure_alt(s)) return false;
    auto grab = [&](unsigned char** p, size_t bytes) {
        if (hipMalloc((void**)p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            return false;
        }
        return true;
    };
    if (codes_b > s->noise_codes_cap) {
        if (s->noise_codes) {
            QSIM_HIPCHK(hipStreamSynchronize(s->stream));
            (void)hipFree(s->noise_codes);
            s->noise_codes = nullptr;
            s->noise_codes_cap = 0;
        }
        if (!grab(&s->noise_codes, 2 * codes_b)) return false;
        s->noise_codes_cap = codes_b;
    }
    ensure_noise_stream(s);
    return true;
}

// Two sets of the in-tile path's flip lists, when they fit beside a margin (false: the tile
// kernels walk the draws themselves).
static bool ensure_noise_lists(qsim_state* s, size_t bytes) {
    if (bytes > s->noise_lists_cap) {
        if (s->noise_lists) {
            QSIM_HIPCHK(hipStreamSynchronize(s->stream));
            if (s->noise_stream) QSIM_HIPCHK(hipStreamSynchronize(s->noise_stream));
            (void)hipFree(s->noise_lists);
            s->noise_lists = nullptr;
            s->noise_lists_cap = 0;
        }
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (free_b < 2 * bytes + kAltMarginBytes) return false;
        if (hipMalloc((void**)&s->noise_lists, 2 * bytes) != hipSuccess) {
            (void)hipGetLastError();
            s->noise_lists = nullptr;
            return false;
        }
        s->noise_lists_cap = bytes;
    }
    ensure_noise_stream(s);
    return true;
}

// After a pulled noisy run: free the second buffer (unless a relayout plan owns it) and the
// code words when the device no longer has room for another 2^n buffer beside a margin.
static void trim_noise_buffers(qsim_state* s) {
    // QSIM_NOISE_KEEP_BUFFERS: 1 always keep, 0 always free (tests)
    static const int keep = env_int("QSIM_NOISE_KEEP_BUFFERS", -1);
    if (keep == 1) return;
    if (keep != 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            free_b = 0;
        }
        if (free_b >= (sizeof(double2) << s->n) + kAltMarginBytes) return;
    }
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    if (s->noise_stream) QSIM_HIPCHK(hipStreamSynchronize(s->noise_stream));
    if (s->noise_codes) (void)hipFree(s->noise_codes);
    s->noise_codes = nullptr;
    s->noise_codes_cap = 0;
    if (s->noise_lists) (void)hipFree(s->noise_lists);
    s->noise_lists = nullptr;
    s->noise_lists_cap = 0;
    if (!s->relayout) release_alt(s);
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
        // where the amplitudes are now: a pinned state's handed-out pointer (prep() leaves the
        // amplitudes of a pinned state in the buffer that was handed out, which may be either one)
        double2* const home = s->d;
        // QSIM_NOISY_TILE=1 (from 12 qubits, flip-only models): the in-tile path (noise.hip
        // launch_gate_noise_run: the gate and the channel prefix whose qubits lie in its tile in one
        // LDS pass, their flips from lists built one step ahead on noise_stream, the rest pushed one
        // launch per channel) — the same draws, so the same states as the pulled and pushed paths.
        // Opt-in: at 26 qubits with 26 channels the 14-15 per-channel suffix launches (0.04 ms
        // each) outweigh the pull pass, 904 vs 1 024 gates/s.
        {
            bool tile = env_switch("QSIM_NOISY_TILE", false) && s->n >= 12;  // (read per run: tests switch it)
            for (const NoiseChan& ch : chans) tile = tile && (ch.type == 0 || ch.type >= 3);
            for (const Op& op : ops) tile = tile && gate_noise_tile_supported(s->n, &op);
            if (tile) {
                const size_t lb = gate_noise_lists_bytes(s->n, 1, chans);
                GnLists L{};
                const bool lists = lb && ensure_noise_lists(s, lb);
                if (lists) {
                    L.buf[0] = s->noise_lists;
                    L.buf[1] = s->noise_lists + s->noise_lists_cap;
                    L.set_bytes = s->noise_lists_cap;
                    L.ms = s->noise_stream;
                    L.built[0] = s->nev_map[0];
                    L.built[1] = s->nev_map[1];
                    L.used[0] = s->nev_pull[0];
                    L.used[1] = s->nev_pull[1];
                    L.start = s->nev_start;
                }
                launch_gate_noise_run(s->d, s->n, 1, 0, ops, chans, seed, *counter, s->stream, &s->timer,
                                      lists ? &L : nullptr);
                trim_noise_buffers(s);
                return;
            }
        }
        if (pull_noise_supported(s->n, chans, true) && ensure_noise_buffers(s, chans.size())) {
            // Flip channels only: the noise after gate i is applied by gate i+1's pass (out of
            // place), the noise after the last gate by one identity pass (noise.hip); the same
            // draws as the per-channel passes below, so the same state.
            // The words of step i (set i & 1) are built on noise_stream while the pass of step
            // i - 1 runs; the pass of step i waits for them, the words of step i + 2 for that pass
            // (QSIM_NOISE_MAP_OVERLAP=0: one stream; read per run, as the next one: tests switch them).
            const bool overlap = env_switch("QSIM_NOISE_MAP_OVERLAP", true);
            const size_t G = ops.size();
            const uint64_t c0 = *counter;
            *counter += (uint64_t)G * n_channels;
            auto words = [&](size_t i) { return (void*)(s->noise_codes + (i & 1) * s->noise_codes_cap); };
            // QSIM_NOISE_MAP_FUSED=1 (opt-in): step i's pass also builds step i + 1's words (its
            // hash-and-log walks meant to fill its own memory stalls; noise.hip k_pull_gate<...,
            // MAP>), one stream.  Measured slower at 26 qubits: 1.22 ms per fused pass against
            // 0.70 + 0.24 ms apart, 815 vs 1 063 gates/s (the walks and their LDS cost the pass its
            // occupancy), so the default is the word map as a kernel of its own, beside the pass
            // (overlap) or before it.
            if (env_switch("QSIM_NOISE_MAP_FUSED", false) && G) {
                launch_noise_map(s->n, 1, 0, chans, seed, c0, words(0), s->stream, &s->timer);
                launch_op(s->d, s->n, 1, ops[0], s->stream, &s->timer);
                for (size_t i = 0; i < G; ++i) {
                    double2* dst = s->alt;
                    const PullMapNext nx{0, seed, c0 + (i + 1) * n_channels, words(i + 1)};
                    launch_pull_gate(s->d, dst, s->n, 1, chans, i + 1 < G ? &ops[i + 1] : nullptr, words(i), s->stream,
                                     &s->timer, i + 1 < G ? &nx : nullptr);
                    s->alt = s->d;
                    s->d = dst;
                }
                settle_home(s, home);
                trim_noise_buffers(s);
                return;
            }
            hipStream_t ms = overlap ? s->noise_stream : s->stream;
            auto map = [&](size_t i) {
                if (overlap && i >= 2) QSIM_HIPCHK(hipStreamWaitEvent(ms, s->nev_pull[i & 1], 0));
                launch_noise_map(s->n, 1, 0, chans, seed, c0 + i * n_channels, words(i), ms, &s->timer);
                if (overlap) QSIM_HIPCHK(hipEventRecord(s->nev_map[i & 1], ms));
            };
            if (overlap) {  // (the previous run's passes may still read both sets)
                QSIM_HIPCHK(hipEventRecord(s->nev_start, s->stream));
                QSIM_HIPCHK(hipStreamWaitEvent(ms, s->nev_start, 0));
                for (size_t i = 0; i < std::min<size_t>(G, 2); ++i) map(i);
            }
            if (G) launch_op(s->d, s->n, 1, ops[0], s->stream, &s->timer);
            for (size_t i = 0; i < G; ++i) {
                if (overlap) QSIM_HIPCHK(hipStreamWaitEvent(s->stream, s->nev_map[i & 1], 0));
                else map(i);
                double2* dst = s->alt;
                launch_pull_gate(s->d, dst, s->n, 1, chans, i + 1 < G ? &ops[i + 1] : nullptr, words(i), s->stream,
                                 &s->timer);
                s->alt = s->d;
                s->d = dst;
                if (overlap && i + 2 < G) {
                    QSIM_HIPCHK(hipEventRecord(s->nev_pull[i & 1], s->stream));
                    map(i + 2);
                }
            }
            settle_home(s, home);
            // The second buffer and the code words stay for the next run (qsim_state_memory_bytes
            // counts them) only while the device keeps room for another state of this size beside
            // them; otherwise they are freed now, so a later StateVector does not fail where the
            // reference's single-buffer one would not.
            trim_noise_buffers(s);
            return;
        }
        for (const Op& op : ops) {
            launch_op(s->d, s->n, 1, op, s->stream, &s->timer);
            for (size_t c = 0; c < n_channels; ++c)
                launch_noise(s->d, s->n, channels[c].type, channels[c].qubit, channels[c].probability,
                             seed, (*counter)++, s->stream, &s->timer);
        }
    });
}

}  // extern "C"
