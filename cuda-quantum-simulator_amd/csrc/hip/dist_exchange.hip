// dist_exchange.hip — the transports of the sharded state (dist.hip): the pack / unpack kernel of a remap,
// the posts of one part, the three ways to carry them and the collectives.  Slab layout: dist_plan.hpp.
#include <algorithm>
#include <map>

#include "device_ops.hpp"
#include "dist_state.hpp"

namespace qsim_hip {

// Pack (state -> send slabs) or unpack (receive slabs -> state) the offsets [lo, lo + 2^sub_log)
// of every slab (one pipeline part of a remap); the own slab never moves.
template <bool PACK>
__global__ __launch_bounds__(256) void k_exchange_copy(XArgs a, uint64_t lo, int sub_log) {
    const uint64_t total = (uint64_t)1 << (sub_log + a.k);
    const uint64_t sub_mask = ((uint64_t)1 << sub_log) - 1;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += step) {
        const uint64_t c = x >> sub_log;
        if ((int)c == a.my_c) continue;
        const uint64_t e = (c << a.chunk_log) | (lo + (x & sub_mask));
        const uint64_t i = xlocal(a, e);
        if (PACK) a.buf[e] = a.st[i];
        else a.st[i] = a.buf[e];
    }
}

XPlan xplan(const qsim_dist* d, const Shard& sh, const DStep& ex, int part = -1) {
    XPlan x = xplan(d->L, sh.rank, ex, part);
    x.a.st = sh.d;
    return x;
}
static void copy_kernel(bool pack, XArgs a, uint64_t lo, int sub_log, hipStream_t s) {
    const uint64_t total = (uint64_t)1 << (sub_log + a.k);
    const unsigned blocks = (unsigned)std::min<uint64_t>((total + 255) / 256, 256 * 64);
    if (pack) hipLaunchKernelGGL(k_exchange_copy<true>, dim3(blocks), dim3(256), 0, s, a, lo, sub_log);
    else hipLaunchKernelGGL(k_exchange_copy<false>, dim3(blocks), dim3(256), 0, s, a, lo, sub_log);
    QSIM_HIPCHK(hipGetLastError());
}
// Pipeline parts of a remap (QSIM_DIST_PIPELINE, default 4): slab offsets are split into parts
// so that part p's transfer overlaps the packing of later parts and the unpacking of earlier
// ones (pack and unpack run on the compute stream, transfers on the comm stream, ordered by
// events).  Parts below 1 MiB of amplitudes are not split further.
static int pipeline_parts(uint64_t chunk) {
    static const int want = [] {
        const char* e = std::getenv("QSIM_DIST_PIPELINE");
        const int v = e ? std::atoi(e) : 4;
        return v < 1 ? 1 : (v > 16 ? 16 : v);
    }();
    int parts = 1;
    while (parts * 2 <= want && (chunk / (uint64_t)(parts * 2)) >= (1ull << 16)) parts *= 2;
    return parts;
}
// Qubit remap: rank r sends its amplitudes with local bits lpos == c to the rank whose bits at
// gpos are c, and stores what that rank sends at local bits == c (the swap of the two qubit
// sets, SURVEY §8(e) "global<->local qubit swap by all-to-all").
// The posts of one remap part of shard `sh`: slab c (c != my_c) is the `amps` amplitudes at
// base + c * stride of the send / receive buffers; it goes to and comes from rank peer_of[c].
// Every transport runs this same per-shard loop (one shard per process, or all of them).
static void slab_posts(std::vector<Post>& out, const Shard& sh, const XPlan& x, int k, uint64_t base,
                       uint64_t stride, uint64_t amps) {
    for (int c = 0; c < (1 << k); ++c) {
        if (c == x.a.my_c) continue;
        const uint64_t at = base + (uint64_t)c * stride;
        out.push_back({sh.rank, x.peer_of[c], sh.sendbuf + at, sh.recvbuf + at, amps});
    }
}
// Virtual transport: move one matched slab inside this process — a device copy, or, with a
// world-1 communicator attached (qsim_dist_virtual_rccl), an ncclSend / ncclRecv pair to rank 0
// itself inside the caller's group (RCCL matches them in issue order).
static void virt_move(qsim_dist* d, double2* dst, const double2* src, uint64_t amps) {
    if (!d->comm) {
        QSIM_HIPCHK(hipMemcpyAsync(dst, src, amps * sizeof(double2), hipMemcpyDeviceToDevice, d->comm_stream));
        return;
    }
    QSIM_NCCLCHK(ncclSend(src, (size_t)amps * 2, ncclDouble, 0, d->comm, d->comm_stream));
    QSIM_NCCLCHK(ncclRecv(dst, (size_t)amps * 2, ncclDouble, 0, d->comm, d->comm_stream));
}
// Hosted transport: hand host-staged copies of this rank's posts to the caller's function (which
// must move them between the rank processes with the same matching rule) and copy what arrived
// back.  Synchronous on the comm stream; for tests, not for speed.
void host_call(qsim_dist* d, const std::vector<qsim_dist_post>& hp, const char* what) {
    const int rc = d->host_fn(d->host_ctx, hp.data(), hp.size());
    if (rc != 0) fail(QSIM_ERR_DEVICE, std::string("host transport failed (") + std::to_string(rc) + ") during " + what);
}
static char* host_stage(qsim_dist* d, size_t bytes) {
    if (bytes > d->h_stage_bytes) {
        if (d->h_stage) QSIM_HIPCHK(hipHostFree(d->h_stage));
        d->h_stage = nullptr;
        d->h_stage_bytes = 0;
        QSIM_HIPCHK(hipHostMalloc((void**)&d->h_stage, bytes, hipHostMallocDefault));
        d->h_stage_bytes = bytes;
    }
    return d->h_stage;
}
static void host_transfers(qsim_dist* d, const std::vector<Post>& posts, const char* what) {
    size_t total = 0;
    for (const Post& p : posts) total += p.amps * sizeof(double2);
    char* snd = host_stage(d, 2 * total);
    char* rcv = snd + total;
    std::vector<qsim_dist_post> hp(posts.size());
    size_t at = 0;
    for (size_t i = 0; i < posts.size(); ++i) {
        const size_t b = posts[i].amps * sizeof(double2);
        QSIM_HIPCHK(hipMemcpyAsync(snd + at, posts[i].send, b, hipMemcpyDeviceToHost, d->comm_stream));
        hp[i] = {posts[i].peer, 0, (uint64_t)b, snd + at, rcv + at};
        at += b;
    }
    QSIM_HIPCHK(hipStreamSynchronize(d->comm_stream));
    host_call(d, hp, what);
    at = 0;
    for (size_t i = 0; i < posts.size(); ++i) {
        const size_t b = posts[i].amps * sizeof(double2);
        QSIM_HIPCHK(hipMemcpyAsync(posts[i].recv, rcv + at, b, hipMemcpyHostToDevice, d->comm_stream));
        at += b;
    }
    QSIM_HIPCHK(hipStreamSynchronize(d->comm_stream));
}
// Carry the posts of one remap part on d->comm_stream (which has already waited for the packs).
void post_transfers(qsim_dist* d, const std::vector<Post>& posts, const char* what) {
    if (posts.empty()) return;
    double sent = 0.0;
    for (const Post& p : posts) sent += (double)p.amps * sizeof(double2);
    d->sent_bytes += sent / (double)d->shards.size();
    TimedLaunch tl(&d->timer, "xgmi_transfer", 2.0 * sent / (double)d->shards.size(), d->comm_stream);
    switch (d->transport) {
        case qsim_dist::T_RCCL:
            QSIM_NCCLCHK(ncclGroupStart());
            for (const Post& p : posts) {
                QSIM_NCCLCHK(ncclSend(p.send, (size_t)p.amps * 2, ncclDouble, p.peer, d->comm, d->comm_stream));
                QSIM_NCCLCHK(ncclRecv(p.recv, (size_t)p.amps * 2, ncclDouble, p.peer, d->comm, d->comm_stream));
            }
            QSIM_NCCLCHK(ncclGroupEnd());
            comm_settle(d, what);
            return;
        case qsim_dist::T_HOSTED:
            host_transfers(d, posts, what);
            return;
        case qsim_dist::T_VIRTUAL: {
            // pair shard r's k-th post naming q with shard q's k-th post naming r; what r sends
            // lands where q receives (a mismatch is exactly what would hang a multi-rank run)
            std::map<std::pair<int, int>, std::vector<size_t>> by_pair;
            for (size_t i = 0; i < posts.size(); ++i) by_pair[{posts[i].rank, posts[i].peer}].push_back(i);
            if (d->comm) QSIM_NCCLCHK(ncclGroupStart());
            for (const auto& kv : by_pair) {
                const auto it = by_pair.find({kv.first.second, kv.first.first});
                if (it == by_pair.end() || it->second.size() != kv.second.size())
                    fail(QSIM_ERR_RUNTIME, std::string("unmatched slab transfer during ") + what);
                for (size_t j = 0; j < kv.second.size(); ++j) {
                    const Post& s = posts[kv.second[j]];
                    const Post& r = posts[it->second[j]];
                    if (s.amps != r.amps) fail(QSIM_ERR_RUNTIME, std::string("slab size mismatch during ") + what);
                    virt_move(d, r.recv, s.send, s.amps);
                }
            }
            if (d->comm) {
                QSIM_NCCLCHK(ncclGroupEnd());
                comm_settle(d, what);
            }
            return;
        }
    }
}

// A fused shard's own slab of part `base`: the pass wrote it to the send buffer, the step after
// reads the receive buffer (the slab never leaves the GPU: one device copy of 1 / 2^k of it).
static void own_slab_copy(qsim_dist* d, const Shard& sh, const XPlan& x, uint64_t base, uint64_t stride,
                          uint64_t amps, hipStream_t s) {
    const uint64_t at = base + (uint64_t)x.a.my_c * stride;
    QSIM_HIPCHK(hipMemcpyAsync(sh.recvbuf + at, sh.sendbuf + at, amps * sizeof(double2), hipMemcpyDeviceToDevice, s));
}

void exchange(qsim_dist* d, const DStep& ex, const std::vector<char>& fused, const std::vector<Shard>* on) {
    if (ex.k == 0) return;
    const std::vector<Shard>& shards = on ? *on : d->shards;
    const uint64_t total = 1ull << d->L;
    const uint64_t chunk = total >> ex.k;
    const double bytes = 2.0 * 16.0 * (double)(total - chunk) * (double)shards.size();
    TimedLaunch tl(&d->timer, "alltoall_remap", bytes, d->stream);
    const int parts = pipeline_parts(chunk);
    int sub_log = d->L - ex.k;
    for (int p = parts; p > 1; p >>= 1) --sub_log;
    const uint64_t sub = 1ull << sub_log;
    ensure_events(d, 2 * (size_t)parts);
    std::vector<XPlan> xs;
    for (const Shard& sh : shards) xs.push_back(xplan(d, sh, ex));
    for (int p = 0; p < parts; ++p) {
        for (size_t i = 0; i < shards.size(); ++i) {
            if (fused[i]) {  // (the pass before stored the slabs; the own slab moves on the device)
                own_slab_copy(d, shards[i], xs[i], (uint64_t)p * sub, chunk, sub, d->stream);
                continue;
            }
            XArgs a = xs[i].a;
            a.buf = shards[i].sendbuf;
            copy_kernel(true, a, (uint64_t)p * sub, sub_log, d->stream);
        }
        QSIM_HIPCHK(hipEventRecord(d->events[p], d->stream));
    }
    for (int p = 0; p < parts; ++p) {
        QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[p], 0));
        std::vector<Post> posts;
        for (size_t i = 0; i < shards.size(); ++i)
            slab_posts(posts, shards[i], xs[i], ex.k, (uint64_t)p * sub, chunk, sub);
        post_transfers(d, posts, "remap send/recv");
        QSIM_HIPCHK(hipEventRecord(d->events[parts + p], d->comm_stream));
    }
    for (int p = 0; p < parts; ++p) {
        QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[parts + p], 0));
        for (size_t i = 0; i < shards.size(); ++i) {
            if (fused[i]) continue;  // (the step after loads the receive buffer itself)
            XArgs a = xs[i].a;
            a.buf = shards[i].recvbuf;
            copy_kernel(false, a, (uint64_t)p * sub, sub_log, d->stream);
        }
    }
}
// One overlapped remap: the K = 2^m parts of every shard (the values of the m pivot bits) are
// exchanged one after the other — pack and unpack on copy_stream, transfers on comm_stream —
// each part waiting for its local work (event pev[j], recorded on the compute stream after the
// role-1 step's part) and signalling pev[3 kMaxParts + j] when unpacked (the role-2 step's part waits for
// it).  Part j uses part j of the send / receive buffers, so all parts can be in flight.
void exchange_parts(qsim_dist* d, const DStep& ex, const std::vector<char>& fused) {
    const int K = part_count(ex.pmask);
    const uint64_t part_amps = 1ull << (d->L - __builtin_popcountll(ex.pmask));
    const uint64_t chunk = part_amps >> ex.k;
    const double bytes = 2.0 * 16.0 * (double)(part_amps - chunk) * (double)d->shards.size();
    part_order(ex.pmask, ex.coarse & ex.pmask, d->order);  // (the same on every rank: RCCL pairs posts in order)
    for (int oi = 0; oi < K; ++oi) {
        const int h = d->order[oi];
        TimedLaunch tl(&d->timer, "alltoall_remap", bytes, d->copy_stream);
        std::vector<XPlan> xs;
        for (Shard& sh : d->shards) xs.push_back(xplan(d, sh, ex, h));
        QSIM_HIPCHK(hipStreamWaitEvent(d->copy_stream, d->pev[h], 0));
        for (size_t i = 0; i < d->shards.size(); ++i) {
            if (fused[i]) {  // (the tail pass of part h stored its slabs; own slab on the device)
                own_slab_copy(d, d->shards[i], xs[i], (uint64_t)h * part_amps, chunk, chunk, d->copy_stream);
                continue;
            }
            XArgs a = xs[i].a;
            a.buf = d->shards[i].sendbuf + (uint64_t)h * part_amps;
            copy_kernel(true, a, 0, xs[i].a.chunk_log, d->copy_stream);
        }
        QSIM_HIPCHK(hipEventRecord(d->pev[kMaxParts + h], d->copy_stream));
        QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->pev[kMaxParts + h], 0));
        std::vector<Post> posts;
        for (size_t i = 0; i < d->shards.size(); ++i)
            slab_posts(posts, d->shards[i], xs[i], ex.k, (uint64_t)h * part_amps, chunk, chunk);
        post_transfers(d, posts, "overlapped remap send/recv");
        QSIM_HIPCHK(hipEventRecord(d->pev[2 * kMaxParts + h], d->comm_stream));
        QSIM_HIPCHK(hipStreamWaitEvent(d->copy_stream, d->pev[2 * kMaxParts + h], 0));
        for (size_t i = 0; i < d->shards.size(); ++i) {
            if (fused[i]) continue;  // (the step after loads part h from the receive buffer)
            XArgs a = xs[i].a;
            a.buf = d->shards[i].recvbuf + (uint64_t)h * part_amps;
            copy_kernel(false, a, 0, xs[i].a.chunk_log, d->copy_stream);
        }
        QSIM_HIPCHK(hipEventRecord(d->pev[3 * kMaxParts + h], d->copy_stream));
    }
}

// Sum of one double over the ranks (virtual: `local` already sums every shard; with a world-1
// communicator the all-reduce below runs anyway, as an identity).  Hosted: every rank sends its
// value to every other and sums in rank order (the same order, so the same result, everywhere).
double allreduce_sum(qsim_dist* d, double local) {
    if (d->transport == qsim_dist::T_HOSTED) {
        const int me = d->shards[0].rank;
        std::vector<double> vals(d->world, 0.0);
        vals[me] = local;
        std::vector<qsim_dist_post> hp;
        for (int r = 0; r < d->world; ++r)
            if (r != me) hp.push_back({r, 0, sizeof(double), &local, &vals[r]});
        host_call(d, hp, "all-reduce");
        double s = 0.0;
        for (double v : vals) s += v;
        return s;
    }
    if (!d->comm) return local;
    QSIM_HIPCHK(hipMemcpyAsync(d->d_result, &local, sizeof(double), hipMemcpyHostToDevice, d->stream));
    QSIM_NCCLCHK(ncclAllReduce(d->d_result, d->d_result, 1, ncclDouble, ncclSum, d->comm, d->stream));
    comm_settle(d, "all-reduce");
    double out = 0.0;
    QSIM_HIPCHK(hipMemcpyAsync(&out, d->d_result, sizeof(double), hipMemcpyDeviceToHost, d->stream));
    stream_wait(d, d->stream);
    return out;
}
// Element-wise sum over the ranks of `count` doubles at d_vec (device, on d->stream), result in
// h_out on every rank.  allreduce_sum's rules, per entry: virtual shards share d_vec (nothing to
// add; with a world-1 communicator the all-reduce runs anyway); hosted: every rank sends its
// vector to every other and adds them in rank order.
void allreduce_vec(qsim_dist* d, double* d_vec, size_t count, double* h_out) {
    if (d->transport == qsim_dist::T_HOSTED) {
        QSIM_HIPCHK(hipMemcpyAsync(h_out, d_vec, count * sizeof(double), hipMemcpyDeviceToHost, d->stream));
        QSIM_HIPCHK(hipStreamSynchronize(d->stream));
        if (d->world == 1) return;
        const int me = d->shards[0].rank;
        std::vector<double> mine(h_out, h_out + count);
        std::vector<std::vector<double>> got(d->world);
        std::vector<qsim_dist_post> hp;
        for (int r = 0; r < d->world; ++r)
            if (r != me) {
                got[r].assign(count, 0.0);
                hp.push_back({r, 0, (uint64_t)(count * sizeof(double)), mine.data(), got[r].data()});
            }
        host_call(d, hp, "vector all-reduce");
        for (size_t i = 0; i < count; ++i) {
            double s = 0.0;
            for (int r = 0; r < d->world; ++r) s += r == me ? mine[i] : got[r][i];
            h_out[i] = s;
        }
        return;
    }
    if (d->comm) {
        QSIM_NCCLCHK(ncclAllReduce(d_vec, d_vec, count, ncclDouble, ncclSum, d->comm, d->stream));
        comm_settle(d, "vector all-reduce");
    }
    QSIM_HIPCHK(hipMemcpyAsync(h_out, d_vec, count * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    stream_wait(d, d->stream);
}

// At least `count` events in d->events (the remap pipeline's; the readers below use the first few
// between remaps).
void ensure_events(qsim_dist* d, size_t count) {
    const size_t have = d->events.size();
    if (have >= count) return;
    d->events.resize(count, nullptr);
    for (size_t i = have; i < count; ++i) QSIM_HIPCHK(hipEventCreateWithFlags(&d->events[i], hipEventDisableTiming));
}

}  // namespace qsim_hip
