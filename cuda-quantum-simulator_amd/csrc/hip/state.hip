// state.hip — the single-GPU state's core: the thread's last error, the timing and buffer classes
// of engine.hpp, the second buffer, the way back to the identity layout, and the extern "C"
// entries that create, fill, copy and describe a state (include/qsim_hip.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "state.hpp"

using namespace qsim_hip;

// ---------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

namespace qsim_hip {
void set_last_error(const char* msg) { g_last_error = msg; }

// ---------------------------------------------------------------------------------------
// Timer
// ---------------------------------------------------------------------------------------
int Timer::slot_of(const char* name) {
    for (size_t i = 0; i < stats.size(); ++i)
        if (stats[i].name == name) return (int)i;
    stats.push_back(Stat{name});
    return (int)stats.size() - 1;
}
static hipEvent_t take_event(std::vector<hipEvent_t>& pool) {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e;
    QSIM_HIPCHK(hipEventCreate(&e));
    return e;
}
void Timer::begin(const char* name, double, hipEvent_t* a_out, int* slot_out) {
    *slot_out = slot_of(name);
    *a_out = take_event(pool);
    QSIM_HIPCHK(hipEventRecord(*a_out, stream));
}
void Timer::end(int slot, hipEvent_t a, double bytes) {
    hipEvent_t b = take_event(pool);
    QSIM_HIPCHK(hipEventRecord(b, stream));
    pending.push_back(Pending{slot, a, b, bytes});
}
void Timer::begin_ext(const char* name, hipEvent_t* a_out, hipEvent_t* b_out, int* slot_out) {
    *slot_out = slot_of(name);
    *a_out = take_event(pool);
    *b_out = take_event(pool);
}
void Timer::finish(int slot, hipEvent_t a, hipEvent_t b, double bytes) {
    pending.push_back(Pending{slot, a, b, bytes});
}
void Timer::resolve() {
    for (auto& p : pending) {
        QSIM_HIPCHK(hipEventSynchronize(p.b));
        float ms = 0.f;
        QSIM_HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        stats[p.slot].ms += ms;
        stats[p.slot].launches += 1;
        stats[p.slot].bytes += p.bytes;
        pool.push_back(p.a);
        pool.push_back(p.b);
    }
    pending.clear();
}
void Timer::reset() {
    resolve();
    stats.clear();
}
Timer::~Timer() {
    for (auto& p : pending) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (auto e : pool) (void)hipEventDestroy(e);
}
void DevBuf::upload(const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return;
    if (shadow.size() == bytes && std::memcmp(shadow.data(), src, bytes) == 0) return;
    if (copied) QSIM_HIPCHK(hipEventSynchronize(copied));  // previous copy done reading shadow
    if (bytes > cap) {
        if (ptr) {
            QSIM_HIPCHK(hipStreamSynchronize(s));
            QSIM_HIPCHK(hipFree(ptr));
            ptr = nullptr;
        }
        cap = std::max<size_t>(bytes, 16384);
        QSIM_HIPCHK(hipMalloc(&ptr, cap));
    }
    shadow.assign((const unsigned char*)src, (const unsigned char*)src + bytes);
    QSIM_HIPCHK(hipMemcpyAsync(ptr, shadow.data(), bytes, hipMemcpyHostToDevice, s));
    if (!copied) QSIM_HIPCHK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    QSIM_HIPCHK(hipEventRecord(copied, s));
}
void* Scratch::get(size_t bytes, hipStream_t s) {
    bytes = std::max<size_t>(bytes, 256);
    if (bytes > cap) {
        if (ptr) {
            QSIM_HIPCHK(hipStreamSynchronize(s));
            QSIM_HIPCHK(hipFree(ptr));
            ptr = nullptr;
            cap = 0;
        }
        QSIM_HIPCHK(hipMalloc(&ptr, bytes));
        cap = bytes;
    }
    return ptr;
}
Scratch::~Scratch() {
    if (ptr) (void)hipFree(ptr);
}
DevBuf::~DevBuf() {
    if (copied) {
        (void)hipEventSynchronize(copied);
        (void)hipEventDestroy(copied);
    }
    if (ptr) (void)hipFree(ptr);
}
TimedLaunch::TimedLaunch(Timer* t, const char* name, double by, hipStream_t s, bool e)
    : tm(t), bytes(by), ext(e), stream(s) {
    if (tm && tm->enabled) {
        tm->stream = s;
        if (ext) tm->begin_ext(name, &a, &b, &slot);
        else tm->begin(name, by, &a, &slot);
    } else {
        tm = nullptr;
    }
}
TimedLaunch::~TimedLaunch() {
    if (tm) {
        try {
            tm->stream = stream;  // a nested launch on another stream may have moved it
            if (ext) tm->finish(slot, a, b, bytes);
            else tm->end(slot, a, bytes);
        } catch (...) {
        }
    }
}

// ---------------------------------------------------------------------------------------
// the second buffer
// ---------------------------------------------------------------------------------------
// The second 2^n buffer relayout passes write into (they run out of place).  Allocated only
// when the device has room for it beside a margin; a refused or failed allocation is cleared and
// reported as false, so the caller keeps the in-place fixed-layout plan (the reference's
// StateVector owns exactly one buffer, and coexisting states must not fail where it would not).
bool ensure_alt(qsim_state* s) {
    if (s->alt) return true;
    // QSIM_RELAYOUT_NO_ALT=1: behave as if it never fits (tests)
    static const bool off = env_switch("QSIM_RELAYOUT_NO_ALT", false);
    if (off) return false;
    const size_t bytes = sizeof(double2) << s->n;
    void* p = device_alloc_beside(bytes, kAltMarginBytes);
    if (!p) return false;
    s->alt_base = p;
    s->alt = reinterpret_cast<double2*>(p);
    return true;
}
// Free the buffer the amplitudes are not in (the state goes back to one 2^n buffer).
void release_alt(qsim_state* s) {
    if (!s->alt_base) return;
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    if (s->d != s->base_d) {  // the amplitudes live in alt_base: it becomes the state's buffer
        (void)hipFree(s->base);
        s->base = s->alt_base;
        s->base_d = s->d;
    } else {
        (void)hipFree(s->alt_base);
    }
    s->alt_base = nullptr;
    s->alt = nullptr;
}

// ---------------------------------------------------------------------------------------
// back to the identity layout
// ---------------------------------------------------------------------------------------
// Undo the relabeling: a fused network of physical SWAPs that brings logical qubit q back to
// position q (exact data movement), then the identity map.  Every entry that reads or writes
// amplitudes by index calls this first.
void canonicalize(qsim_state* s) {
    share_flush(s);
    if (s->perm.empty()) return;
    const int n = s->n;
    // One gate-free relayout pass (relayout.hip) from 16 qubits: every amplitude stored at its
    // identity-layout position in a single HBM round trip (QSIM_RESTORE_ONE_PASS=0: the SWAP
    // network below, a few passes).
    static const bool one_pass = env_switch("QSIM_RESTORE_ONE_PASS", true);
    // (it writes out of place: without room for the second buffer, the in-place SWAP network)
    if (one_pass && n >= 16 && n - 12 <= 32 && ensure_alt(s)) {
        const Plan plan = plan_permutation_pass(n, s->perm);
        s->stages.upload(plan.stages.data(), plan.stages.size() * sizeof(Stage), s->stream);
        launch_plan(s, plan, &s->timer, nullptr);
        s->perm.clear();  // (last_passes keeps describing the last circuit run)
        if (!s->relayout) release_alt(s);  // (only relayout plans keep the second buffer)
        return;
    }
    std::vector<int> p = s->perm, inv(n);
    for (int q = 0; q < n; ++q) inv[p[q]] = q;
    std::vector<Op> swaps;
    for (int q = 0; q < n; ++q) {
        if (p[q] == q) continue;
        const int b = p[q], r = inv[q];  // logical q sits at b, logical r at position q
        qsim_gate g{};
        g.type = QSIM_GATE_SWAP;
        g.nqubits = 2;
        g.qubits[0] = q;
        g.qubits[1] = b;
        swaps.push_back(lower_gate(g, n));
        swaps.back().src = (int)swaps.size() - 1;
        p[r] = b;
        inv[b] = r;
        p[q] = q;
        inv[q] = q;
    }
    s->perm.clear();
    if (!swaps.empty()) run_fused(s, swaps, false);
}
// Before an entry that overwrites every amplitude: the labels are dropped, not restored.
void drop_layout(qsim_state* s) {
    share_discard(s);  // (pending gates of a run-sharing cycle: overwritten with the rest)
    if (s->relayout) {  // (a relayout plan's second buffer: as canonicalize would leave it)
        canonicalize(s);
    }
    s->perm.clear();
    s->basis = false;
}
// Before an entry that reads amplitudes by index (touch: and writes them).
void prep(qsim_state* s, bool touch) {
    canonicalize(s);
    if (touch) s->basis = false;
}
}  // namespace qsim_hip

// A basis state written over the amplitudes: the state is as new (the next first run chooses its
// layout again: memo).
static void init_basis(qsim_state* s, uint64_t idx) {
    DeviceGuard g(s->device);
    share_discard(s);
    launch_init_basis(s->d, s->n, 1, idx, s->stream);
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    s->perm.clear();
    s->basis = true;
    s->basis_idx = idx;
    s->tile_h = -1;
    s->calibrated = false;
    s->relayout = false;
}

extern "C" {

const char* qsim_last_error(void) { return g_last_error.c_str(); }

int qsim_abi_version(void) { return QSIM_ABI_VERSION; }

int qsim_set_device(int device) {
    return guarded([&] {
        int c = 0;
        QSIM_HIPCHK(hipGetDeviceCount(&c));
        if (device < 0 || device >= c) fail(QSIM_ERR_INVALID_ARGUMENT, "device index out of range");
        QSIM_HIPCHK(hipSetDevice(device));
    });
}

int qsim_device_count(int* count) {
    return guarded([&] {
        QSIM_REQUIRE(count, QSIM_ERR_INVALID_ARGUMENT, "null count");
        int c = 0;
        hipError_t e = hipGetDeviceCount(&c);
        if (e != hipSuccess) c = 0;
        *count = c;
    });
}

int qsim_device_info(int device, char* name, size_t name_len, int* cu_count, size_t* total_mem) {
    return guarded([&] {
        hipDeviceProp_t p;
        QSIM_HIPCHK(hipGetDeviceProperties(&p, device));
        if (name && name_len) {
            std::strncpy(name, p.name, name_len - 1);
            name[name_len - 1] = 0;
        }
        if (cu_count) *cu_count = p.multiProcessorCount;
        if (total_mem) *total_mem = p.totalGlobalMem;
    });
}

int qsim_state_create_on(int device, int n_qubits, qsim_state** out) {
    return guarded([&] {
        QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
        *out = nullptr;
        // StateVector ctor validation (src/StateVector.cu:135-141, Constants.hpp:68-69)
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > QSIM_MAX_QUBITS_SINGLE)
            fail(QSIM_ERR_INVALID_ARGUMENT, "Number of qubits must be between " +
                                                std::to_string(QSIM_MIN_QUBITS) + " and " +
                                                std::to_string(QSIM_MAX_QUBITS_SINGLE));
        DeviceGuard g(device);
        auto s = std::make_unique<qsim_state>();
        s->n = n_qubits;
        s->device = device;
        QSIM_HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        s->timer.stream = s->stream;
        // QSIM_STATE_OFFSET_KB (experiments): the amplitudes start that far into their allocation
        static const size_t off = [] {
            const char* e = std::getenv("QSIM_STATE_OFFSET_KB");
            return e ? (size_t)std::max(0ll, std::atoll(e)) * 1024 : (size_t)0;
        }();
        static const int contiguous = env_int("QSIM_STATE_CONTIGUOUS", 0);  // (experiments)
        const size_t sbytes = ((sizeof(double2)) << n_qubits) + off;
        if (!contiguous || hipExtMallocWithFlags(&s->base, sbytes, hipDeviceMallocContiguous) != hipSuccess) {
            (void)hipGetLastError();
            s->base = nullptr;
            QSIM_HIPCHK(hipMalloc(&s->base, sbytes));
        }
        s->d = reinterpret_cast<double2*>(reinterpret_cast<char*>(s->base) + off);
        s->base_d = s->d;
        QSIM_HIPCHK(hipMalloc((void**)&s->d_partials, 4096 * sizeof(double)));
        QSIM_HIPCHK(hipMalloc((void**)&s->d_result, sizeof(double)));
        launch_init_basis(s->d, s->n, 1, 0, s->stream);
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
        *out = s.release();
    });
}

int qsim_state_create(int n_qubits, qsim_state** out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return qsim_state_create_on(dev, n_qubits, out);
}

int qsim_state_destroy(qsim_state* s) {
    return guarded([&] {
        if (!s) return;
        DeviceGuard g(s->device);
        delete s;
    });
}

int qsim_state_num_qubits(const qsim_state* s, int* n) {
    return guarded([&] {
        check_state(s);
        *n = s->n;
    });
}

int qsim_state_device_ptr(qsim_state* s, void** dptr) {
    return guarded([&] {
        check_state(s);
        DeviceGuard dg(s->device);
        prep(s, true);  // the caller may read or write through the pointer
        s->pinned = true;  // (relayout runs copy their result back to this buffer)
        *dptr = s->d;
    });
}

int qsim_state_stream(qsim_state* s, void** stream) {
    return guarded([&] {
        check_state(s);
        *stream = (void*)s->stream;
    });
}

int qsim_state_init_zero(qsim_state* s) {
    return guarded([&] {
        check_state(s);
        init_basis(s, 0);
    });
}

int qsim_state_init_basis(qsim_state* s, uint64_t idx) {
    return guarded([&] {
        check_state(s);
        if (idx >= (1ull << s->n)) fail(QSIM_ERR_INVALID_ARGUMENT, "Basis index out of range");
        init_basis(s, idx);
    });
}

int qsim_state_sync(qsim_state* s) {
    return guarded([&] {
        check_state(s);
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

int qsim_state_to_host(qsim_state* s, double* dst) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(dst, QSIM_ERR_INVALID_ARGUMENT, "null destination");
        DeviceGuard dg(s->device);
        prep(s, false);
        QSIM_HIPCHK(hipMemcpyAsync(dst, s->d, sizeof(double2) << s->n, hipMemcpyDeviceToHost,
                                   s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

int qsim_state_from_host(qsim_state* s, const double* src) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(src, QSIM_ERR_INVALID_ARGUMENT, "null source");
        DeviceGuard dg(s->device);
        share_discard(s);
        s->perm.clear();  // overwritten in logical order
        s->basis = false;
        QSIM_HIPCHK(hipMemcpyAsync(s->d, src, sizeof(double2) << s->n, hipMemcpyHostToDevice,
                                   s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

int qsim_state_memory_bytes(qsim_state* s, uint64_t* bytes) {
    return guarded([&] {
        check_state(s);
        QSIM_REQUIRE(bytes, QSIM_ERR_INVALID_ARGUMENT, "null out");
        const uint64_t amps = sizeof(double2) << s->n;
        *bytes = amps + (s->alt_base ? amps : 0) + 4096 * sizeof(double) + sizeof(double) + s->scratch.cap +
                 s->ops.cap + s->stages.cap + s->expect_terms.cap + 2 * s->noise.codes_cap + 2 * s->noise.lists_cap;
        if (s->grad)
            *bytes += 2 * amps + s->grad->out_cap * sizeof(double) + s->grad->ops.cap + s->grad->stages.cap +
                      s->grad->terms.cap;
    });
}

int qsim_state_profile(qsim_state* s, int enable) {
    return guarded([&] {
        check_state(s);
        s->timer.enabled = enable != 0;
        s->timer.stream = s->stream;
    });
}

int qsim_state_profile_count(qsim_state* s, int* n) {
    return guarded([&] {
        check_state(s);
        DeviceGuard dg(s->device);
        s->timer.resolve();
        *n = (int)s->timer.stats.size();
    });
}

int qsim_state_profile_get(qsim_state* s, int i, char* name, size_t name_len, double* total_ms,
                           int64_t* launches, double* alg_bytes) {
    return guarded([&] {
        check_state(s);
        DeviceGuard dg(s->device);
        s->timer.resolve();
        if (i < 0 || i >= (int)s->timer.stats.size()) fail(QSIM_ERR_OUT_OF_RANGE, "bad index");
        const auto& st = s->timer.stats[i];
        if (name && name_len) {
            std::strncpy(name, st.name.c_str(), name_len - 1);
            name[name_len - 1] = 0;
        }
        if (total_ms) *total_ms = st.ms;
        if (launches) *launches = st.launches;
        if (alg_bytes) *alg_bytes = st.bytes;
    });
}

int qsim_state_profile_reset(qsim_state* s) {
    return guarded([&] {
        check_state(s);
        DeviceGuard dg(s->device);
        s->timer.reset();
    });
}

}  // extern "C"
