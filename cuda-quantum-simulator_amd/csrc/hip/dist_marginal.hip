// dist_marginal.hip — marginal probabilities and reduced density matrices of a sharded state
// (dist.hip), read where the shards lie: no remap, no localize, no gather of amplitudes.  No
// reference counterpart.  Conventions, caps and error codes are marginal.hip's.
//
// The k listed qubits are mapped through the state's permutation on the host.  A selected physical
// position is local (< L, k_loc of them) or a rank position (>= L, k_rank of them); the selected
// rank bits of rank r, packed in ascending position, are s(r).  Unselected rank bits belong to the
// environment.
//
// Marginal.  Every shard runs marginal.hip's launch_marginal with a plan lowered for n = L over
// its k_loc local positions (k_loc = 0: the shard's norm), which leaves 2^k_loc bins in ascending
// position order.  k_fold_accumulate then adds them into the process's zero-filled 2^k vector at
// the output indices whose rank-selected bits are s(r), in the caller's bit order — one launch per
// shard, the shards of a process in rank order on one stream, so no floating-point atomics.  One
// allreduce_vec adds the ranks (the other ranks' bins hold exact zeros or bins of the same s with
// another environment).
//
// Reduced density matrix.  With a over the selected local positions and b over the unselected,
//     rho[(s, a), (s', a')] = sum_e sum_b psi_(s,e)(a, b) conj psi_(s',e)(a', b).
// Diagonal blocks (s = s'): marginal.hip's matrix kernel on each shard at n = L, k = k_loc.
// Off-diagonal blocks: for every non-zero d inside the selected rank mask (ascending, at most 7
// steps) rank r pairs with r ^ d and the cross block C = M_r M_(r^d)^dagger (a full 2^k_loc x
// 2^k_loc complex matrix) is computed by k_rdm_cross, the two-source variant of the matrix kernel:
// rows from the own shard, columns from the received one.
// Pair rule (a function of (r, d, the positions) only):
//   * top local position L-1 unselected: it is an environment bit, so the sum over b splits in
//     two halves.  The lower rank of the pair takes b with bit L-1 = 0 and receives the peer's
//     lower half; the higher rank takes bit L-1 = 1 and receives the peer's upper half (the
//     half-shard rule of dist_expect.hip).  Half a shard moves each way, both ranks compute half of
//     the columns, and a half shard is simply a state of L-1 qubits with the same selected
//     positions.  The lower rank's sum lands in block (s, s'), the higher rank's — it is
//     M_(r^d) M_r^dagger over its half — in block (s', s); the finish adds the second's conjugate
//     transpose to the first.
//   * top local position selected: the lower rank computes all of C into block (s, s'); a whole
//     shard moves each way (a post is a send / receive pair), the higher rank launches nothing
//     and its block (s', s) stays zero, so the same finish applies.
// Summation order: the device adds into one zero-filled 2 * 4^k vector in a fixed order — the
// diagonal blocks shard by shard in rank order, then the cross steps in ascending d, each shard by
// shard — then one allreduce_vec over the 2 * 4^k doubles, then the host finish (dist_rdm_finish):
// blocks with s < s' take raw(s, s') + raw(s', s)^dagger, those with s > s' the conjugate
// transpose of that, and marginal.hip's rdm_finish takes the upper triangle in the caller's
// numbering, zeroes the diagonal's imaginary part and mirrors.
//
// k_rdm_cross stages two panels of 2^11 amplitudes (own and received, 32 KiB each: the 64 KiB of
// LDS of the one-source kernel, two work-groups per CU) and keeps its BLK x BLK register block.
//
// Transfers go through post_transfers and land in the receive buffer (even steps) or the send
// buffer (odd steps), both free outside remaps and a whole shard each (make_dist, dist.hip);
// events 0 .. 4 of d->events order them as in dist_expect.hip.  Scratch: the partial sums of one
// kernel at a time (<= 64 MiB, shared by the shards of a process one after the other), one block
// vector and the result vector.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_ops.hpp"
#include "dist_state.hpp"

namespace qsim_hip {

constexpr int kRdmCrossPanelBits = 11;  // two panels of 2^11 amplitudes: 64 KiB of LDS

struct DistMarginalPlan {
    MarginalPlan all;  // over all n positions: the checks, sel and dst (ascending position -> caller's bit)
    MarginalPlan loc;  // a shard's plan: n = L over the k_loc local positions, bins in ascending position
    int L = 0, k_loc = 0, k_rank = 0;
    uint64_t rank_sel = 0;        // the selected rank positions, as bits of a rank
    std::vector<int> steps;       // matrix: the non-zero d inside rank_sel, ascending
    bool half = false;            // matrix with steps: the half-shard rule (position L-1 unselected)
    int n_x = 0;                  // qubits of each of the cross kernel's two sources (L - 1 or L)
    uint64_t x_groups = 0;        // its work-groups
    uint64_t scratch_bytes = 0;   // partial sums: the larger of the local and the cross kernel's
    uint64_t bytes_per_step = 0;  // sent by one rank in one step
    int launches = 0;             // per shard, at most (a rank that is the lower one of all its pairs)
};

DistMarginalPlan lower_dist_marginal(int n, int L, const int32_t* qubits, int k, const int* perm, bool rdm) {
    DistMarginalPlan p;
    p.all = lower_marginal(n, qubits, k, perm, rdm);
    p.L = L;
    std::vector<int32_t> local;
    for (int pos = 0; pos < n; ++pos) {
        if (!(p.all.sel >> pos & 1ull)) continue;
        if (pos < L) local.push_back(pos);
        else p.rank_sel |= 1ull << (pos - L);
    }
    p.k_loc = (int)local.size();
    p.k_rank = k - p.k_loc;
    p.loc = lower_marginal(L, local.data(), p.k_loc, nullptr, rdm);
    p.scratch_bytes = p.loc.scratch_bytes;
    p.launches = p.loc.launches + 1;
    if (rdm && p.k_rank > 0) {
        for (uint64_t d = 1; d < (1ull << (n - L)); ++d)
            if ((d & ~p.rank_sel) == 0) p.steps.push_back((int)d);
        p.half = !(p.all.sel >> (L - 1) & 1ull);
        p.n_x = p.half ? L - 1 : L;
        const int px = std::min(p.n_x, kRdmCrossPanelBits);
        p.x_groups = std::min<uint64_t>(1ull << (p.n_x - px), kRdmGroups);
        p.scratch_bytes = std::max<uint64_t>(p.scratch_bytes, p.x_groups * (2ull << (2 * p.k_loc)) * sizeof(double));
        p.bytes_per_step = sizeof(double2) << p.n_x;
        p.launches += 2 * (int)p.steps.size();
    }
    return p;
}

// s(r): the bits of `rank` at the selected rank positions, packed in ascending position.
static uint32_t rank_selected_bits(const DistMarginalPlan& p, int rank) {
    uint32_t s = 0;
    int j = 0;
    for (int b = 0; b < 63; ++b)
        if (p.rank_sel >> b & 1ull) s |= (uint32_t)(rank >> b & 1) << j++;
    return s;
}

void dist_rdm_finish(const DistMarginalPlan& p, const double* raw, double* out) {
    const uint32_t D = 1u << p.all.k;
    std::vector<double> m((size_t)2 * D * D);
    auto at = [&](uint32_t r, uint32_t c) { return 2 * ((size_t)r * D + c); };
    for (uint32_t r = 0; r < D; ++r)
        for (uint32_t c = 0; c < D; ++c) {
            const uint32_t sr = r >> p.k_loc, sc = c >> p.k_loc;
            if (sr == sc) {
                m[at(r, c)] = raw[at(r, c)];
                m[at(r, c) + 1] = raw[at(r, c) + 1];
            } else if (sr < sc) {  // both ranks of a pair may hold a part: raw(s, s') + raw(s', s)^dagger
                m[at(r, c)] = raw[at(r, c)] + raw[at(c, r)];
                m[at(r, c) + 1] = raw[at(r, c) + 1] - raw[at(c, r) + 1];
            }
        }
    for (uint32_t r = 0; r < D; ++r)
        for (uint32_t c = 0; c < D; ++c)
            if ((r >> p.k_loc) > (c >> p.k_loc)) {
                m[at(r, c)] = m[at(c, r)];
                m[at(r, c) + 1] = -m[at(c, r) + 1];
            }
    rdm_finish(p.all, m.data(), out);
}

namespace {

// Bit i of v moved to position pos[i].
__device__ __forceinline__ uint64_t scatter_bits(uint64_t v, int count, const int8_t* pos) {
    uint64_t r = 0;
    for (int i = 0; i < count; ++i) r |= (v >> i & 1ull) << pos[i];
    return r;
}

// out[base | place(t)] += sum over s < S of partials[s * T + t], t < T: the accumulating variant
// of marginal.hip's k_fold_partials (the same fixed order over s: thread row y adds s = y, y + cy,
// ..., thread row 0 then adds the rows' sums in order).  place: bit i of t lands on bit dst[i].
// One thread owns one output element and launches into the same vector follow one another on one
// stream, so the additions into out happen in launch order.
struct PlaceMap {
    int nbits;
    int8_t dst[24];
    uint32_t base;
};
__global__ __launch_bounds__(256) void k_fold_accumulate(const double* __restrict__ partials, uint32_t T, uint32_t S,
                                                         int tx_log, PlaceMap map, double* __restrict__ out) {
    __shared__ double red[256];
    const uint32_t tx = 1u << tx_log, cy = 256u >> tx_log;
    const uint32_t x = threadIdx.x & (tx - 1u), y = threadIdx.x >> tx_log;
    const uint32_t t = blockIdx.x * tx + x;
    double acc = 0.0;
    if (t < T)
        for (uint32_t s = y; s < S; s += cy) acc += partials[(uint64_t)s * T + t];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (y == 0 && t < T) {
        double v = red[x];
        for (uint32_t yy = 1; yy < cy; ++yy) v += red[yy * tx + x];
        uint32_t o = map.base;  // (T == 2^nbits and base has no bit of place(): inside the result vector)
        for (int i = 0; i < map.nbits; ++i) o |= (t >> i & 1u) << map.dst[i];
        out[o] += v;
    }
}

void launch_fold_accumulate(const double* partials, uint32_t T, uint32_t S, const PlaceMap& map, double* out,
                            hipStream_t s) {
    int tx_log = 0;
    while (tx_log < 6 && (1u << (tx_log + 1)) <= T) ++tx_log;
    const uint32_t tx = 1u << tx_log;
    hipLaunchKernelGGL(k_fold_accumulate, dim3((T + tx - 1) / tx), dim3(256), 0, s, partials, T, S, tx_log, map, out);
    QSIM_HIPCHK(hipGetLastError());
}

// The panel geometry of marginal.hip's matrix kernel, for panels of 2^p amplitudes.
struct RdmCrossArgs {
    int p;            // panel bits
    uint64_t panels;  // 2^(n - p)
    int8_t pos[12];   // physical position of bit i of a panel element index (ascending)
    int8_t slot[12];  // LDS slot bit of it: a selected position's rank, or K + an unselected one's
    int8_t rest[52];  // the positions outside the panel, ascending
    int nrest;
};

// C = M_own M_oth^dagger over two sources of 2^n amplitudes each (M: rows over the K selected
// positions, columns over the others), as k_rdm_partial computes M M^dagger: a work-group stages
// the same panel of both sources in LDS as [column][row], every thread owns a BLK x BLK block of C
// (rows from the own panel, columns from the other one) and one of G column groups; the groups are
// added in a fixed order through LDS and the work-group writes its partial matrix once.
template <int K>
__global__ __launch_bounds__(256) void k_rdm_cross(const double2* __restrict__ own, const double2* __restrict__ oth,
                                                   RdmCrossArgs a, double2* __restrict__ partials) {
    constexpr int D = 1 << K;
    constexpr int BLK = D < 4 ? D : 4;
    constexpr int NB = D / BLK;      // blocks per side
    constexpr int NBLK = NB * NB;    // blocks of C
    constexpr int G = 256 / NBLK;    // column groups
    constexpr int PE = 1 << kRdmCrossPanelBits;
    constexpr int J = PE / 256;      // elements of a panel per thread
    __shared__ double2 lds[2 * PE];  // the own panel, the other one; afterwards the groups' blocks
    double2* pa = lds;
    double2* pb = lds + PE;
    const unsigned tid = threadIdx.x;
    const unsigned blk = tid % NBLK, g = tid / NBLK;
    const unsigned bi = blk / NB, bj = blk % NB;
    const uint32_t E = 1u << a.p;  // elements of a panel (<= PE)
    const uint32_t B = E >> K;     // its columns
    uint64_t off_t = 0;
    uint32_t slot_t = 0;
    for (int i = 0; i < 8 && i < a.p; ++i)
        if (tid >> i & 1u) {
            off_t |= 1ull << a.pos[i];
            slot_t |= 1u << a.slot[i];
        }
    double2 acc[BLK][BLK];
#pragma unroll
    for (int i = 0; i < BLK; ++i)
#pragma unroll
        for (int j = 0; j < BLK; ++j) acc[i][j] = make_double2(0.0, 0.0);
    for (uint64_t pan = blockIdx.x; pan < a.panels; pan += gridDim.x) {
        const uint64_t base = scatter_bits(pan, a.nrest, a.rest);
        double2 va[J], vb[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            uint64_t off = base | off_t;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if ((j >> b & 1) && 8 + b < a.p) off |= 1ull << a.pos[8 + b];
            // j * 256 + tid < 2^p: the offset has panel-position and rest bits only, all below n
            const bool in = (uint32_t)(j * 256) + tid < E;
            va[j] = in ? own[off] : make_double2(0.0, 0.0);
            vb[j] = in ? oth[off] : make_double2(0.0, 0.0);
        }
        __syncthreads();  // the panels before have been consumed
#pragma unroll
        for (int j = 0; j < J; ++j) {
            uint32_t sl = slot_t;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if ((j >> b & 1) && 8 + b < a.p) sl |= 1u << a.slot[8 + b];
            if ((uint32_t)(j * 256) + tid < E) {  // sl < 2^p <= PE
                pa[sl] = va[j];
                pb[sl] = vb[j];
            }
        }
        __syncthreads();
        for (uint32_t col = g; col < B; col += G) {
            const double2* ca = pa + ((size_t)col << K);
            const double2* cb = pb + ((size_t)col << K);
            double2 ra[BLK], rb[BLK];
#pragma unroll
            for (int i = 0; i < BLK; ++i) {
                ra[i] = ca[bi * BLK + i];
                rb[i] = cb[bj * BLK + i];
            }
#pragma unroll
            for (int i = 0; i < BLK; ++i)
#pragma unroll
                for (int j = 0; j < BLK; ++j) {  // += ra[i] * conj(rb[j])
                    acc[i][j].x += ra[i].x * rb[j].x + ra[i].y * rb[j].y;
                    acc[i][j].y += ra[i].y * rb[j].x - ra[i].x * rb[j].y;
                }
        }
    }
    __syncthreads();
    double2* red = lds;  // [g][D * D]: G * D * D = 256 * BLK * BLK <= 4096 = 2 * PE
#pragma unroll
    for (int i = 0; i < BLK; ++i)
#pragma unroll
        for (int j = 0; j < BLK; ++j) red[g * (D * D) + (bi * BLK + i) * D + bj * BLK + j] = acc[i][j];
    __syncthreads();
    for (unsigned o = tid; o < D * D; o += 256) {
        double2 v = red[o];
        for (int gg = 1; gg < G; ++gg) {
            v.x += red[gg * (D * D) + o].x;
            v.y += red[gg * (D * D) + o].y;
        }
        partials[(size_t)blockIdx.x * (D * D) + o] = v;
    }
}

template <int K>
void launch_cross_k(const double2* own, const double2* oth, const RdmCrossArgs& a, unsigned groups, double2* partials,
                    hipStream_t s) {
    hipLaunchKernelGGL(k_rdm_cross<K>, dim3(groups), dim3(256), 0, s, own, oth, a, partials);
}

// One cross block of two sources of 2^n_x amplitudes into partials (x_groups matrices).
void launch_rdm_cross(const double2* own, const double2* oth, const DistMarginalPlan& p, double* d_partials,
                      hipStream_t s, Timer* tm) {
    TimedLaunch tl(tm, "reduced_density_cross", 32.0 * (double)(1ull << p.n_x), s);
    const uint64_t sel = p.all.sel & ((1ull << p.L) - 1ull);
    const int K = p.k_loc;
    RdmCrossArgs a{};
    a.p = std::min(p.n_x, kRdmCrossPanelBits);
    a.panels = 1ull << (p.n_x - a.p);
    // the panel: every selected local position and the p - K lowest unselected ones
    uint64_t in_panel = sel;
    for (int pos = 0, need = a.p - K; pos < p.n_x && need > 0; ++pos)
        if (!(sel >> pos & 1ull)) {
            in_panel |= 1ull << pos;
            --need;
        }
    int ne = 0, nsel = 0, nuns = 0;
    for (int pos = 0; pos < p.n_x; ++pos) {
        if (in_panel >> pos & 1ull) {
            a.pos[ne] = (int8_t)pos;
            a.slot[ne] = (int8_t)((sel >> pos & 1ull) ? nsel++ : K + nuns++);
            ++ne;
        } else {
            a.rest[a.nrest++] = (int8_t)pos;
        }
    }
    double2* part = (double2*)d_partials;
    const unsigned groups = (unsigned)p.x_groups;
    switch (K) {
        case 0: launch_cross_k<0>(own, oth, a, groups, part, s); break;
        case 1: launch_cross_k<1>(own, oth, a, groups, part, s); break;
        case 2: launch_cross_k<2>(own, oth, a, groups, part, s); break;
        case 3: launch_cross_k<3>(own, oth, a, groups, part, s); break;
        case 4: launch_cross_k<4>(own, oth, a, groups, part, s); break;
        case 5: launch_cross_k<5>(own, oth, a, groups, part, s); break;
        // (a cross step has k_rank >= 1, so k_loc <= 5 under the cap k <= 6)
        default: fail(QSIM_ERR_RUNTIME, "cross block of more than 5 local qubits");
    }
    QSIM_HIPCHK(hipGetLastError());
}

// Where a shard's 2^k_loc bins go in the caller's 2^k vector.
PlaceMap marginal_place(const DistMarginalPlan& p, int rank) {
    PlaceMap m{};
    m.nbits = p.k_loc;
    for (int i = 0; i < p.k_loc; ++i) m.dst[i] = (int8_t)p.all.dst[i];
    const uint32_t s = rank_selected_bits(p, rank);
    for (int j = 0; j < p.k_rank; ++j) m.base |= (s >> j & 1u) << p.all.dst[p.k_loc + j];
    return m;
}

// Where block (s_row, s_col) of 2 * 4^k_loc doubles goes in the raw 2^k x 2^k matrix (rows and
// columns numbered by ascending physical position: local bits, then rank bits).
PlaceMap block_place(const DistMarginalPlan& p, uint32_t s_row, uint32_t s_col) {
    PlaceMap m{};
    const int kl = p.k_loc, k = p.all.k;
    m.nbits = 1 + 2 * kl;
    m.dst[0] = 0;  // re / im
    for (int i = 0; i < kl; ++i) {
        m.dst[1 + i] = (int8_t)(1 + i);           // column
        m.dst[1 + kl + i] = (int8_t)(1 + k + i);  // row
    }
    m.base = (s_col << (1 + kl)) | (s_row << (1 + k + kl));
    return m;
}

}  // namespace

// Both readers (qsim_dist_marginal_probabilities / qsim_dist_reduced_density_matrix), lowered as
// the top of this file says.  Everything computes on d->stream; step t's transfer lands in the
// receive buffer (t even) or the send buffer (t odd).  Events 0 .. 4 of d->events: the state is
// ready (0), a transfer landed in buffer j (1 + j), the kernels that read buffer j are done (3 + j).
static void marginal_dist(qsim_dist* d, const int32_t* qubits, int k, bool rdm, double* out) {
    const int L = d->L;
    const DistMarginalPlan plan = lower_dist_marginal(d->n, L, qubits, k, d->perm.data(), rdm);
    const size_t S = d->shards.size();
    const size_t out_count = rdm ? (size_t)2 << (2 * k) : (size_t)1 << k;
    const size_t blk_count = rdm ? (size_t)2 << (2 * plan.k_loc) : (size_t)1 << plan.k_loc;
    const size_t part_bytes = (plan.scratch_bytes + 255) & ~(size_t)255;
    char* buf = (char*)d->readout.get(part_bytes + (blk_count + out_count) * sizeof(double), d->stream);
    double* d_part = (double*)buf;
    double* d_blk = (double*)(buf + part_bytes);
    double* d_out = d_blk + blk_count;
    QSIM_HIPCHK(hipMemsetAsync(d_out, 0, out_count * sizeof(double), d->stream));
    const size_t T = plan.steps.size();
    const double sent_before = d->sent_bytes;  // (remapBytes() stays the last run's)
    const uint64_t H = 1ull << plan.n_x;       // amplitudes of a transfer
    auto post = [&](size_t t) {  // step t's transfer on comm_stream, into buffer t & 1
        const int j = (int)(t & 1);
        if (t >= 2) QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[3 + j], 0));  // the buffer's last readers
        std::vector<Post> posts;
        for (const Shard& sh : d->shards) {
            const int peer = sh.rank ^ plan.steps[t];
            // half-shard rule: the peer pairs my amplitudes of ITS half — the lower rank sends its upper half
            const uint64_t from = plan.half && sh.rank < peer ? H : 0;
            posts.push_back({sh.rank, peer, sh.d + from, j ? sh.sendbuf : sh.recvbuf, H});
        }
        post_transfers(d, posts, "reduced density matrix shard send/recv");
        QSIM_HIPCHK(hipEventRecord(d->events[1 + j], d->comm_stream));
    };
    if (T) {
        ensure_events(d, 5);
        QSIM_HIPCHK(hipEventRecord(d->events[0], d->stream));  // (the state's last writers)
        QSIM_HIPCHK(hipStreamWaitEvent(d->comm_stream, d->events[0], 0));
        post(0);  // in flight while the local kernels run
    }
    for (size_t i = 0; i < S; ++i) {
        const Shard& sh = d->shards[i];
        launch_marginal(sh.d, plan.loc, d_part, d_blk, d->stream, &d->timer);
        const uint32_t s = rank_selected_bits(plan, sh.rank);
        launch_fold_accumulate(d_blk, (uint32_t)blk_count, 1, rdm ? block_place(plan, s, s) : marginal_place(plan, sh.rank),
                               d_out, d->stream);
    }
    for (size_t t = 0; t < T; ++t) {
        if (t + 1 < T) post(t + 1);
        const int j = (int)(t & 1);
        QSIM_HIPCHK(hipStreamWaitEvent(d->stream, d->events[1 + j], 0));
        for (size_t i = 0; i < S; ++i) {
            const Shard& sh = d->shards[i];
            const int peer = sh.rank ^ plan.steps[t];
            const bool lower = sh.rank < peer;
            if (!plan.half && !lower) continue;  // the lower rank computes the whole block
            const double2* own = sh.d + (plan.half && !lower ? H : 0);
            launch_rdm_cross(own, j ? sh.sendbuf : sh.recvbuf, plan, d_part, d->stream, &d->timer);
            launch_fold_accumulate(d_part, (uint32_t)blk_count, (uint32_t)plan.x_groups,
                                   block_place(plan, rank_selected_bits(plan, sh.rank), rank_selected_bits(plan, peer)),
                                   d_out, d->stream);
        }
        QSIM_HIPCHK(hipEventRecord(d->events[3 + j], d->stream));
    }
    d->sent_bytes = sent_before;
    if (!rdm) {
        allreduce_vec(d, d_out, out_count, out);
        return;
    }
    std::vector<double> raw(out_count);
    allreduce_vec(d, d_out, out_count, raw.data());
    dist_rdm_finish(plan, raw.data(), out);
}

}  // namespace qsim_hip

using namespace qsim_hip;

extern "C" {

int qsim_dist_marginal_probabilities(qsim_dist* d, const int32_t* qubits, int k, double* out) {
    return dguard_comm(d, [&] {
        need(d);
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        (void)lower_marginal(d->n, qubits, k, nullptr, false);  // the argument checks, before anything runs
        QSIM_HIPCHK(hipSetDevice(d->device));
        flush_on_device(d);
        marginal_dist(d, qubits, k, false, out);
    });
}

int qsim_dist_reduced_density_matrix(qsim_dist* d, const int32_t* qubits, int k, double* out) {
    return dguard_comm(d, [&] {
        need(d);
        if (!out) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        (void)lower_marginal(d->n, qubits, k, nullptr, true);  // the argument checks, before anything runs
        QSIM_HIPCHK(hipSetDevice(d->device));
        flush_on_device(d);
        marginal_dist(d, qubits, k, true, out);
    });
}

int qsim_dist_marginal_plan(int n_qubits, int world, const int32_t* perm, const int32_t* qubits, int k, int rdm,
                            int32_t info[16]) {
    return guarded([&] {
        if (!info) fail(QSIM_ERR_INVALID_ARGUMENT, "null out");
        const int L = HostPlanArgs(n_qubits, world).L;
        const DistMarginalPlan p = lower_dist_marginal(n_qubits, L, qubits, k, perm, rdm != 0);
        const uint64_t bytes = (uint64_t)p.steps.size() * p.bytes_per_step;
        info[0] = p.k_loc;
        info[1] = p.k_rank;
        info[2] = p.loc.k_lo;
        info[3] = p.loc.k_hi;
        info[4] = (int32_t)p.loc.slices;
        info[5] = (int32_t)p.loc.groups;
        info[6] = (int32_t)p.steps.size();
        info[7] = (int32_t)p.steps.size();
        info[8] = (int32_t)(bytes & 0xffffffffull);
        info[9] = (int32_t)(bytes >> 32);
        info[10] = p.launches;
        info[11] = (int32_t)(rdm ? 2u << (2 * k) : 1u << k);
        info[12] = (int32_t)(p.scratch_bytes & 0xffffffffull);
        info[13] = (int32_t)(p.scratch_bytes >> 32);
        info[14] = p.steps.empty() ? 0 : (p.half ? 1 : 2);
        info[15] = (int32_t)p.x_groups;
    });
}

}  // extern "C"
