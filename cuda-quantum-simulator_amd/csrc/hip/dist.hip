// dist.hip — state vector sharded over the GPUs of one node, one process per GPU, RCCL over xGMI.
//
// The reference is single-GPU (README.md:361-367); SURVEY §8(e) specifies this extension.
//
// Layout: W = 2^g ranks, L = n - g local qubits.  Rank r owns the 2^L amplitudes whose top g
// PHYSICAL index bits equal r.  Every rank keeps the same logical->physical qubit map `perm`:
//   * SWAP gates only exchange two map entries (zero data movement);
//   * controls on global (rank) bits are resolved per rank (the op is dropped on ranks whose bit
//     is 0, the control is dropped on the others); a diagonal gate whose target is global becomes a
//     uniform phase on the rank's shard;
//   * a gate whose TARGET is global needs data from another rank: before it, the planner remaps
//     qubits — the g logical qubits whose next use as a target lies furthest ahead become global —
//     and executes the remap as one all-to-all: pack (gather the 2^k - 1 outgoing chunks by their
//     local bits) -> grouped ncclSend/ncclRecv with the 2^k - 1 peers -> unpack.  With k = g all
//     W - 1 xGMI links of every GPU carry 1/W of its shard concurrently.
// Local work between remaps is the single-GPU engine (fused tile passes) on the 2^L shard.
//
// This file: the object's lifetime and the entries that only move state around.  The planner is
// dist_plan.hip, the transports dist_exchange.hip, the run dist_run.hip; each feature lives with its kernels
// (dist_readout.hip, dist_expect.hip, dist_adjoint.hip, dist_pauli_rot.hip).  They share dist_state.hpp.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "device_ops.hpp"
#include "dist_state.hpp"

using namespace qsim_hip;

namespace qsim_hip {

void need(const qsim_dist* d) {
    if (!d) fail(QSIM_ERR_INVALID_ARGUMENT, "null dist handle");
    if (d->aborted)
        fail(QSIM_ERR_DEVICE, "distributed state unusable: its RCCL communicator was aborted "
                              "after an earlier error");
}
double env_seconds(const char* k, double dflt) {
    const char* e = std::getenv(k);
    const double v = e ? std::atof(e) : dflt;
    return v > 0 ? v : dflt;
}
// Wait until a non-blocking communicator has finished queuing its last call (init, group end,
// collective); a communicator error or QSIM_DIST_TIMEOUT seconds without progress fails (the
// caller's dguard_comm then aborts the communicator).
void comm_settle(ncclComm_t comm, const char* what, double timeout_s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        ncclResult_t st = ncclSuccess;
        QSIM_NCCLCHK(ncclCommGetAsyncError(comm, &st));
        if (st == ncclSuccess) return;
        if (st != ncclInProgress)
            fail(QSIM_ERR_DEVICE, std::string("RCCL error during ") + what + ": " + ncclGetErrorString(st));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
            fail(QSIM_ERR_DEVICE, std::string("RCCL timeout during ") + what);
        std::this_thread::yield();
    }
}
void comm_settle(qsim_dist* d, const char* what) {
    if (d->comm) comm_settle(d->comm, what, env_seconds("QSIM_DIST_TIMEOUT", 600.0));
}
// hipStreamSynchronize with a watchdog: while the stream drains, a communicator error or
// QSIM_DIST_TIMEOUT seconds fail (and abort the communicator) instead of blocking forever.
void stream_wait(qsim_dist* d, hipStream_t s) {
    if (!d->comm) {
        QSIM_HIPCHK(hipStreamSynchronize(s));
        return;
    }
    const double timeout_s = env_seconds("QSIM_DIST_TIMEOUT", 600.0);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) return;
        if (q != hipErrorNotReady) QSIM_HIPCHK(q);
        ncclResult_t st = ncclSuccess;
        QSIM_NCCLCHK(ncclCommGetAsyncError(d->comm, &st));
        if (st != ncclSuccess && st != ncclInProgress)
            fail(QSIM_ERR_DEVICE, std::string("RCCL error while waiting: ") + ncclGetErrorString(st));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
            fail(QSIM_ERR_DEVICE, "timeout waiting for the distributed state's streams");
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

static void init_zero(qsim_dist* d) {
    for (int q = 0; q < d->n; ++q) d->perm[q] = q;
    d->fresh = true;
    for (Shard& s : d->shards) launch_init_basis(s.d, d->L, 1, s.rank == 0 ? 0 : ~0ull, d->stream);
    QSIM_HIPCHK(hipStreamSynchronize(d->stream));
}
// The object of every creator (its arguments checked by then), for a transport and the ranks whose
// shards this process holds.  The creator attaches its communicator, if any, and calls init_zero.
static std::unique_ptr<qsim_dist> make_dist(int n, int g, int world, int device, qsim_dist::Transport transport,
                                            const std::vector<int>& ranks) {
    auto d = std::make_unique<qsim_dist>();
    d->n = n;
    d->g = g;
    d->L = n - g;
    d->world = world;
    d->device = device;
    d->virt = transport == qsim_dist::T_VIRTUAL;
    d->transport = transport;
    d->perm.resize(n);
    QSIM_HIPCHK(hipSetDevice(device));
    QSIM_HIPCHK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    QSIM_HIPCHK(hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking));
    QSIM_HIPCHK(hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : d->pev) QSIM_HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    d->timer.stream = d->stream;
    const size_t bytes = sizeof(double2) << d->L;
    for (int r : ranks) {
        Shard s;
        s.rank = r;
        QSIM_HIPCHK(hipMalloc((void**)&s.d, bytes));
        if (d->world > 1) {
            QSIM_HIPCHK(hipMalloc((void**)&s.sendbuf, bytes));
            QSIM_HIPCHK(hipMalloc((void**)&s.recvbuf, bytes));
        }
        d->shards.push_back(s);
    }
    QSIM_HIPCHK(hipMalloc((void**)&d->d_partials, 4096 * sizeof(double)));
    QSIM_HIPCHK(hipMalloc((void**)&d->d_result, sizeof(double)));
    return d;
}
// Attach the communicator of (world, rank, id) to d.  Non-blocking (QSIM_RCCL_BLOCKING=1 selects a
// blocking one): the init and every later call can then be bounded by a timeout and aborted, so a
// rank that never arrives (or dies) makes its peers fail instead of hanging.
static void open_comm(qsim_dist* d, int world, int rank, const void* unique_id) {
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const char* bl = std::getenv("QSIM_RCCL_BLOCKING");
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = bl && std::atoi(bl) != 0 ? 1 : 0;
    const ncclResult_t ir = ncclCommInitRankConfig(&d->comm, world, id, rank, &cfg);
    if (ir != ncclSuccess && ir != ncclInProgress) {
        if (d->comm) (void)ncclCommAbort(d->comm);
        d->comm = nullptr;
        fail(QSIM_ERR_DEVICE, std::string("RCCL error: ") + ncclGetErrorString(ir));
    }
    try {
        comm_settle(d->comm, "communicator init", env_seconds("QSIM_DIST_INIT_TIMEOUT", 300.0));
    } catch (...) {
        (void)ncclCommAbort(d->comm);
        d->comm = nullptr;
        throw;
    }
}

}  // namespace qsim_hip

extern "C" {

int qsim_dist_unique_id(void* id_out) {
    return guarded([&] {
        if (!id_out) fail(QSIM_ERR_INVALID_ARGUMENT, "null id buffer");
        static_assert(sizeof(ncclUniqueId) <= QSIM_DIST_UNIQUE_ID_BYTES, "unique id size");
        ncclUniqueId id;
        QSIM_NCCLCHK(ncclGetUniqueId(&id));
        std::memset(id_out, 0, QSIM_DIST_UNIQUE_ID_BYTES);
        std::memcpy(id_out, &id, sizeof(id));
    });
}

int qsim_dist_create(int n_qubits, int rank, int world, const void* unique_id, int device,
                     qsim_dist** out) {
    return guarded([&] {
        if (!out || !unique_id) fail(QSIM_ERR_INVALID_ARGUMENT, "null argument");
        *out = nullptr;
        const int g = log2_exact(world);
        if (rank < 0 || rank >= world) fail(QSIM_ERR_INVALID_ARGUMENT, "rank out of range");
        check_sizes(n_qubits, g);
        auto d = make_dist(n_qubits, g, world, device, qsim_dist::T_RCCL, {rank});
        open_comm(d.get(), world, rank, unique_id);
        init_zero(d.get());
        *out = d.release();
    });
}

int qsim_dist_create_virtual(int n_qubits, int world, int device, qsim_dist** out) {
    return guarded([&] {
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null argument");
        *out = nullptr;
        const int g = log2_exact(world);
        check_sizes(n_qubits, g);
        std::vector<int> ranks(world);
        for (int r = 0; r < world; ++r) ranks[r] = r;
        auto d = make_dist(n_qubits, g, world, device, qsim_dist::T_VIRTUAL, ranks);
        init_zero(d.get());
        *out = d.release();
    });
}

int qsim_dist_create_hosted(int n_qubits, int rank, int world, int device, qsim_dist_transport_fn fn,
                            void* ctx, qsim_dist** out) {
    return guarded([&] {
        if (!out || !fn) fail(QSIM_ERR_INVALID_ARGUMENT, "null argument");
        *out = nullptr;
        const int g = log2_exact(world);
        if (rank < 0 || rank >= world) fail(QSIM_ERR_INVALID_ARGUMENT, "rank out of range");
        check_sizes(n_qubits, g);
        auto d = make_dist(n_qubits, g, world, device, qsim_dist::T_HOSTED, {rank});
        d->host_fn = fn;
        d->host_ctx = ctx;
        init_zero(d.get());
        *out = d.release();
    });
}

int qsim_dist_virtual_rccl(qsim_dist* d, const void* unique_id) {
    return guarded([&] {
        need(d);
        if (!d->virt || d->comm) fail(QSIM_ERR_INVALID_ARGUMENT, "needs a virtual object without a communicator");
        if (!unique_id) fail(QSIM_ERR_INVALID_ARGUMENT, "null argument");
        QSIM_HIPCHK(hipSetDevice(d->device));
        open_comm(d, 1, 0, unique_id);
    });
}

int qsim_dist_destroy(qsim_dist* d) {
    return guarded([&] { delete d; });
}

int qsim_dist_reset(qsim_dist* d) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        init_zero(d);
    });
}

int qsim_dist_run(qsim_dist* d, const qsim_gate* gates, size_t count, int flags) {
    return dguard_comm(d, [&] {
        need(d);
        if (!gates && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null gate list");
        QSIM_HIPCHK(hipSetDevice(d->device));
        run_dist(d, gates, count, flags);
    });
}

int qsim_dist_remap_bytes(qsim_dist* d, double* sent) {
    return guarded([&] {
        need(d);
        if (sent) *sent = d->sent_bytes;
    });
}

int qsim_dist_fused_remaps(qsim_dist* d, int* remaps) {
    return guarded([&] {
        need(d);
        if (!remaps) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        *remaps = d->fused_remaps;
    });
}

int qsim_dist_carried_runs(qsim_dist* d, int* runs) {
    return guarded([&] {
        need(d);
        if (!runs) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        *runs = d->carried;
    });
}

int qsim_dist_overlapped(qsim_dist* d, int* remaps) {
    return guarded([&] {
        need(d);
        if (remaps) *remaps = d->overlapped;
    });
}

int qsim_dist_sync(qsim_dist* d) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        for (hipStream_t s : {d->comm_stream, d->copy_stream, d->stream}) stream_wait(d, s);
    });
}

// Every rank's engine idle, then a one-double all-reduce on the communicator: the ranks leave it
// within the collective's latency of one another (the timing barrier of bench.py's N > 1 steps —
// a host-file barrier releases its pollers milliseconds apart).
int qsim_dist_barrier(qsim_dist* d) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        for (hipStream_t s : {d->comm_stream, d->copy_stream, d->stream}) stream_wait(d, s);
        (void)allreduce_sum(d, 0.0);
    });
}

int qsim_dist_perm(qsim_dist* d, int32_t* perm) {
    return guarded([&] {
        need(d);
        for (int q = 0; q < d->n; ++q) perm[q] = d->perm[q];
    });
}

int qsim_dist_local_state(qsim_dist* d, double* dst) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        const size_t bytes = sizeof(double2) << d->L;
        for (size_t i = 0; i < d->shards.size(); ++i)  // virtual mode: all shards, rank order
            QSIM_HIPCHK(hipMemcpyAsync((char*)dst + i * bytes, d->shards[i].d, bytes,
                                       hipMemcpyDeviceToHost, d->stream));
        QSIM_HIPCHK(hipStreamSynchronize(d->stream));
    });
}

int qsim_dist_gather_state(qsim_dist* d, double* dst) {
    return dguard_comm(d, [&] {
        need(d);
        flush_on_device(d);
        const uint64_t shard = 1ull << d->L;
        const bool root = d->virt || d->shards[0].rank == 0;
        if (d->transport == qsim_dist::T_HOSTED) {  // host-staged: rank 0 receives every shard
            std::vector<double2> phys(root ? (1ull << d->n) : shard);
            QSIM_HIPCHK(hipMemcpyAsync(phys.data(), d->shards[0].d,
                                       sizeof(double2) * shard, hipMemcpyDeviceToHost, d->stream));
            QSIM_HIPCHK(hipStreamSynchronize(d->stream));
            std::vector<qsim_dist_post> hp;
            if (root)
                for (int r = 1; r < d->world; ++r)
                    hp.push_back({r, 0, sizeof(double2) * shard, nullptr, phys.data() + r * shard});
            else
                hp.push_back({0, 0, sizeof(double2) * shard, phys.data(), nullptr});
            host_call(d, hp, "gather");
            if (root && dst) unpermute(d, phys, dst);
            return;
        }
        double2* all = nullptr;
        if (root) QSIM_HIPCHK(hipMalloc((void**)&all, (sizeof(double2) << d->n)));
        if (d->virt) {
            for (const Shard& s : d->shards)
                QSIM_HIPCHK(hipMemcpyAsync(all + s.rank * shard, s.d, sizeof(double2) * shard,
                                           hipMemcpyDeviceToDevice, d->stream));
        } else {
            QSIM_NCCLCHK(ncclGroupStart());
            if (root) {
                QSIM_HIPCHK(hipMemcpyAsync(all, d->shards[0].d, sizeof(double2) * shard,
                                           hipMemcpyDeviceToDevice, d->stream));
                for (int r = 1; r < d->world; ++r)
                    QSIM_NCCLCHK(ncclRecv(all + r * shard, shard * 2, ncclDouble, r, d->comm, d->stream));
            } else {
                QSIM_NCCLCHK(ncclSend(d->shards[0].d, shard * 2, ncclDouble, 0, d->comm, d->stream));
            }
            QSIM_NCCLCHK(ncclGroupEnd());
            comm_settle(d, "gather");
        }
        stream_wait(d, d->stream);
        if (root) {
            std::vector<double2> phys(1ull << d->n);
            QSIM_HIPCHK(hipMemcpy(phys.data(), all, sizeof(double2) << d->n, hipMemcpyDeviceToHost));
            QSIM_HIPCHK(hipFree(all));
            if (dst) unpermute(d, phys, dst);
        }
    });
}

int qsim_dist_bcast(qsim_dist* d, double* buf, size_t count) {
    return dguard_comm(d, [&] {
        need(d);
        if (!buf && count) fail(QSIM_ERR_INVALID_ARGUMENT, "null buffer");
        flush_on_device(d);
        if (count == 0 || d->virt || d->world == 1) return;
        const size_t bytes = count * sizeof(double);
        const int me = d->shards[0].rank;
        if (d->transport == qsim_dist::T_HOSTED) {
            std::vector<qsim_dist_post> hp;
            if (me == 0)
                for (int r = 1; r < d->world; ++r) hp.push_back({r, 0, (uint64_t)bytes, buf, nullptr});
            else
                hp.push_back({0, 0, (uint64_t)bytes, nullptr, buf});
            host_call(d, hp, "broadcast");
            return;
        }
        double* dv = (double*)d->readout.get(bytes, d->stream);
        if (me == 0) QSIM_HIPCHK(hipMemcpyAsync(dv, buf, bytes, hipMemcpyHostToDevice, d->stream));
        QSIM_NCCLCHK(ncclBroadcast(dv, dv, count, ncclDouble, 0, d->comm, d->stream));
        comm_settle(d, "broadcast");
        if (me != 0) QSIM_HIPCHK(hipMemcpyAsync(buf, dv, bytes, hipMemcpyDeviceToHost, d->stream));
        stream_wait(d, d->stream);
    });
}

int qsim_dist_profile(qsim_dist* d, int enable) {
    return guarded([&] {
        need(d);
        d->timer.enabled = enable != 0;
    });
}

int qsim_dist_profile_count(qsim_dist* d, int* n) {
    return guarded([&] {
        need(d);
        QSIM_HIPCHK(hipSetDevice(d->device));
        d->timer.resolve();
        *n = (int)d->timer.stats.size();
    });
}

int qsim_dist_profile_get(qsim_dist* d, int i, char* name, size_t name_len, double* total_ms,
                          int64_t* launches, double* alg_bytes) {
    return guarded([&] {
        need(d);
        QSIM_HIPCHK(hipSetDevice(d->device));
        d->timer.resolve();
        if (i < 0 || i >= (int)d->timer.stats.size()) fail(QSIM_ERR_OUT_OF_RANGE, "bad index");
        const auto& st = d->timer.stats[i];
        if (name && name_len) {
            std::strncpy(name, st.name.c_str(), name_len - 1);
            name[name_len - 1] = 0;
        }
        if (total_ms) *total_ms = st.ms;
        if (launches) *launches = st.launches;
        if (alg_bytes) *alg_bytes = st.bytes;
    });
}

}  // extern "C"
