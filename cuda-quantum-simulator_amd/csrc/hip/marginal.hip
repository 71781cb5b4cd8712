// marginal.hip — marginal probabilities and reduced density matrices of a subset of qubits,
// computed where the state lies (no readback, no layout restore).  No reference counterpart: the
// reference copies 2^n probabilities to the host and leaves the reduction to the caller.
//
// Qubit convention: PauliSum's and the gates' — qubit q is index bit q (NOT measure(q)'s
// big-endian F2 mapping).  For the k listed qubits (any order, distinct),
//     marginal:  out[m]      = sum_i |psi_i|^2 over all i with bit qubits[j] of i == bit j of m
//     matrix:    rho[a][a']  = sum_b psi(a, b) conj(psi(a', b)),  bit j of a = qubit qubits[j]
// The qubits are mapped to physical positions through the state's permutation on the host
// (lower_marginal); the kernels see physical positions only and read the current buffer as it is.
// Every sum is added in an order fixed by the launch geometry, which depends only on (n, the
// physical positions): no floating-point atomics, two calls return identical doubles.
//
// Marginal (k <= 20).  A run is 2^c contiguous amplitudes, c = min(n, 12); thread t of the 256
// reads amplitudes j * 256 + t of a run, j < 16, so run bits 0-5 are lane bits, 6-7 wave bits and
// 8-11 per-thread bits, and every load instruction of a wave moves 1 KiB of consecutive
// addresses.  Selected positions below c (k_lo of them) are binned inside the run, those above
// (k_hi) choose runs: a work-group owns one value h of the selected high bits and one of S slices
// of the unselected high bits, loops over its runs with 16 accumulators per thread (one per j),
// then folds: unselected per-thread bits in registers, unselected lane bits by an xor butterfly
// (both operands of each add are the same two numbers in either lane), unselected wave bits as a
// fixed-order sum through LDS.  It writes its 2^k_lo bins once; k_fold_partials adds the S slices
// of a bin in a fixed order and stores the bin at its place in the caller's bit order.  S is the
// largest power of two with about kMarginalGroups work-groups and S * 2^k * 8 B <= 64 MiB.
//
// Reduced density matrix (k <= 6), rho = M M^dagger with M of shape 2^k x 2^(n-k), plain FP64 FMA.
// A panel is the 2^p amplitudes (p = min(n, 12)) spanned by the k selected positions and the
// p - k lowest unselected ones; a work-group stages one panel at a time in LDS as [column][row]
// (64 KiB) and loops over its share of the 2^(n-p) panels.  Coalescing: positions 0 .. p-k-1 are
// each either selected or among the p-k lowest unselected, so they all belong to the panel, and
// the loads walk the panel in address order — element e of a panel (bit i of e = the i-th lowest
// panel position) is read by thread e mod 256.  Which (row a, column b) that element is depends on
// the case: when low positions are unselected, consecutive lanes hold consecutive columns; when
// the selected positions are the lowest bits, consecutive lanes hold one column's rows.  Either
// way the lane -> (a, b) map is the bit table RdmArgs::slot, applied when the element is written
// to LDS, and the global loads are the same contiguous 1 KiB per wave.  Each thread owns a
// BLK x BLK block of rho in registers (4 x 4 complex at k = 6) and, when the matrix has fewer than
// 256 blocks, one of G column groups; the groups are added in a fixed order through LDS and the
// work-group writes its partial matrix once.  k_fold_partials adds the work-groups' partials.
// All of rho is accumulated (every thread busy); the host takes the upper triangle, zeroes the
// diagonal's imaginary part and mirrors, so rho == rho^dagger bitwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"

namespace qsim_hip {

MarginalPlan lower_marginal(int n, const int32_t* qubits, int k, const int* perm, bool rdm) {
    check_qubit_perm(n, perm);
    const int cap = rdm ? kRdmMaxQubits : kMarginalMaxQubits;
    if (k < 0 || k > cap || k > n) fail(QSIM_ERR_INVALID_ARGUMENT, "too many qubits for this reader");
    if (k > 0 && !qubits) fail(QSIM_ERR_INVALID_ARGUMENT, "null qubit list");
    MarginalPlan p;
    p.n = n;
    p.k = k;
    p.rdm = rdm;
    p.c = std::min(n, kMarginalRunBits);
    uint64_t seen = 0;
    int out_bit_of[64];  // physical position -> bit of the caller's index
    for (int j = 0; j < k; ++j) {
        const int q = qubits[j];
        if (q < 0 || q >= n) fail(QSIM_ERR_OUT_OF_RANGE, "qubit index out of range");
        if (seen >> q & 1ull) fail(QSIM_ERR_INVALID_ARGUMENT, "duplicate qubit");
        seen |= 1ull << q;
        const int pos = perm ? perm[q] : q;
        p.sel |= 1ull << pos;
        out_bit_of[pos] = j;
    }
    for (int pos = 0; pos < n; ++pos) {
        if (!(p.sel >> pos & 1ull)) continue;
        p.dst.push_back(out_bit_of[pos]);  // internal bin bit (ascending position) -> caller's bit
        if (pos < p.c) ++p.k_lo;
        else ++p.k_hi;
    }
    if (!rdm) {
        const int u_hi = n - p.c - p.k_hi;
        int s_log = std::max(0, kMarginalGroupsLog - p.k_hi);
        s_log = std::min(s_log, u_hi);
        s_log = std::min(s_log, kMarginalScratchLog - 3 - k);  // S * 2^k doubles <= 64 MiB (k <= 20)
        p.slices = 1u << s_log;
        p.groups = (uint64_t)p.slices << p.k_hi;
        p.scratch_bytes = ((uint64_t)p.slices << k) * sizeof(double);
    } else {
        const uint64_t panels = 1ull << (n - p.c);
        // (kRdmGroups partial matrices of 2 * 4^6 doubles are 64 MiB)
        p.groups = std::min<uint64_t>(panels, kRdmGroups);
        p.slices = (unsigned)p.groups;
        p.scratch_bytes = p.groups * (2ull << (2 * k)) * sizeof(double);
    }
    p.launches = 2;
    return p;
}

namespace {

struct MargArgs {
    int c, k, k_lo, k_hi, u_hi, s_log;
    uint32_t lo_mask;    // selected positions below c
    int8_t lo_pos[12];   // ... ascending
    int8_t hi_sel[52];   // selected positions >= c, ascending
    int8_t hi_uns[52];   // unselected positions >= c, ascending
};

// Bit i of v moved to position pos[i].
__device__ __forceinline__ uint64_t scatter_bits(uint64_t v, int count, const int8_t* pos) {
    uint64_t r = 0;
    for (int i = 0; i < count; ++i) r |= (v >> i & 1ull) << pos[i];
    return r;
}

__global__ __launch_bounds__(256) void k_marginal_partial(const double2* __restrict__ st, MargArgs a,
                                                          double* __restrict__ partials) {
    __shared__ double part[4096];
    const unsigned tid = threadIdx.x;
    const uint64_t slice = blockIdx.x & ((1u << a.s_log) - 1u);
    const uint64_t h = blockIdx.x >> a.s_log;
    const uint64_t base_h = scatter_bits(h, a.k_hi, a.hi_sel);
    const uint64_t per = 1ull << (a.u_hi - a.s_log);
    const uint32_t R = 1u << a.c;
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    for (uint64_t u = slice * per; u < (slice + 1) * per; ++u) {
        const double2* p = st + (base_h | scatter_bits(u, a.u_hi, a.hi_uns));
        double2 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t r = j * 256 + tid;  // r < 2^c: inside the run, base has no bit below c
            v[j] = r < R ? p[r] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] += v[j].x * v[j].x + v[j].y * v[j].y;
    }
    // unselected per-thread bits (run bits 8-11; bits >= c hold zeros and count as unselected)
    const uint32_t uns_t = ~(a.lo_mask >> 8) & 15u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (uns_t >> b & 1u) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (!(j >> b & 1)) acc[j] += acc[j | 1 << b];
        }
    }
    // unselected lane bits: xor butterfly, low bit first
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        if (!(a.lo_mask >> b & 1u)) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (!(j & uns_t)) acc[j] += __shfl_xor(acc[j], 1 << b);
        }
    }
    const bool lane_rep = (tid & 63u & ~a.lo_mask) == 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (lane_rep && !(j & uns_t)) part[j * 256 + tid] = acc[j];
    __syncthreads();
    // unselected wave bits (6, 7) in a fixed order, one bin per thread
    const bool u6 = !(a.lo_mask >> 6 & 1u), u7 = !(a.lo_mask >> 7 & 1u);
    const uint32_t bins = 1u << a.k_lo;
    for (uint32_t ml = tid; ml < bins; ml += 256) {
        const uint32_t r0 = (uint32_t)scatter_bits(ml, a.k_lo, a.lo_pos);
        double v = part[r0];
        if (u6 && u7) v = (part[r0] + part[r0 | 64]) + (part[r0 | 128] + part[r0 | 192]);
        else if (u6) v = part[r0] + part[r0 | 64];
        else if (u7) v = part[r0] + part[r0 | 128];
        partials[(slice << a.k) + (h << a.k_lo) + ml] = v;
    }
}

}  // namespace

// out[place(t)] = sum over s < S of partials[s * T + t], t < T, in a fixed order: a work-group
// takes tx = 2^tx_log consecutive t and splits the S rows over its 256 / tx thread rows, thread
// row y adding s = y, y + cy, ...; thread row 0 then adds the rows' sums in order.  place: bit i of
// t lands on bit dst[i] (nbits == 0: the identity).  (FoldMap, launch_fold: engine.hpp.)
namespace {
__global__ __launch_bounds__(256) void k_fold_partials(const double* __restrict__ partials, uint32_t T, uint32_t S,
                                                       int tx_log, FoldMap map, double* __restrict__ out) {
    __shared__ double red[256];
    const uint32_t tx = 1u << tx_log, cy = 256u >> tx_log;
    const uint32_t x = threadIdx.x & (tx - 1u), y = threadIdx.x >> tx_log;
    const uint32_t t = blockIdx.x * tx + x;
    double acc = 0.0;
    if (t < T)
        for (uint32_t s = y; s < S; s += cy) acc += partials[(uint64_t)s * T + t];
    red[threadIdx.x] = acc;  // (= red[y * tx + x])
    __syncthreads();
    if (y == 0 && t < T) {
        double v = red[x];
        for (uint32_t yy = 1; yy < cy; ++yy) v += red[yy * tx + x];
        uint32_t o = t;
        if (map.nbits) {
            o = 0;
            for (int i = 0; i < map.nbits; ++i) o |= (t >> i & 1u) << map.dst[i];
        }
        out[o] = v;
    }
}

}  // namespace

void launch_fold(const double* partials, uint32_t T, uint32_t S, const FoldMap& map, double* out, hipStream_t s) {
    int tx_log = 0;
    while (tx_log < 6 && (1u << (tx_log + 1)) <= T) ++tx_log;
    const uint32_t tx = 1u << tx_log;
    hipLaunchKernelGGL(k_fold_partials, dim3((T + tx - 1) / tx), dim3(256), 0, s, partials, T, S, tx_log, map, out);
    QSIM_HIPCHK(hipGetLastError());
}

namespace {

struct RdmArgs {
    int p;                // panel bits
    uint64_t panels;      // 2^(n - p)
    int8_t pos[12];       // physical position of bit i of a panel element index (ascending)
    int8_t slot[12];      // LDS slot bit of it: a selected position's rank, or K + an unselected one's
    int8_t rest[52];      // the positions outside the panel, ascending
    int nrest;
};

template <int K>
__global__ __launch_bounds__(256) void k_rdm_partial(const double2* __restrict__ st, RdmArgs a,
                                                     double2* __restrict__ partials) {
    constexpr int D = 1 << K;
    constexpr int BLK = D < 4 ? D : 4;
    constexpr int NB = D / BLK;       // blocks per side
    constexpr int NBLK = NB * NB;     // blocks of rho
    constexpr int G = 256 / NBLK;     // column groups
    __shared__ double2 panel[4096];   // [column][row]; afterwards the groups' blocks
    const unsigned tid = threadIdx.x;
    const unsigned blk = tid % NBLK, g = tid / NBLK;
    const unsigned bi = blk / NB, bj = blk % NB;
    const uint32_t E = 1u << a.p;     // elements of a panel
    const uint32_t B = E >> K;        // its columns
    // element e = j * 256 + tid: address offset and LDS slot are ORs of per-bit contributions
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
        const double2* src = st + scatter_bits(pan, a.nrest, a.rest);
        double2 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint64_t off = off_t;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if ((j >> b & 1) && 8 + b < a.p) off |= 1ull << a.pos[8 + b];
            // j * 256 + tid < 2^p: the offset has panel-position bits only, all below n
            v[j] = (uint32_t)(j * 256) + tid < E ? src[off] : make_double2(0.0, 0.0);
        }
        __syncthreads();  // the panel before has been consumed
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t sl = slot_t;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if ((j >> b & 1) && 8 + b < a.p) sl |= 1u << a.slot[8 + b];
            if ((uint32_t)(j * 256) + tid < E) panel[sl] = v[j];
        }
        __syncthreads();
        for (uint32_t col = g; col < B; col += G) {
            const double2* cp = panel + ((size_t)col << K);
            double2 ra[BLK], rb[BLK];
#pragma unroll
            for (int i = 0; i < BLK; ++i) {
                ra[i] = cp[bi * BLK + i];
                rb[i] = cp[bj * BLK + i];
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
    double2* red = panel;  // [g][D * D]: G * D * D = 256 * BLK * BLK <= 4096
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
void launch_rdm_k(const double2* st, const RdmArgs& a, unsigned groups, double2* partials, hipStream_t s) {
    hipLaunchKernelGGL(k_rdm_partial<K>, dim3(groups), dim3(256), 0, s, st, a, partials);
}

}  // namespace

void launch_marginal(const double2* st, const MarginalPlan& p, double* d_partials, double* d_out, hipStream_t s,
                     Timer* tm) {
    // (both kernels of a call under one timer entry)
    TimedLaunch tl(tm, p.rdm ? "reduced_density" : "marginal", 16.0 * (double)(1ull << p.n), s);
    FoldMap map{};
    if (!p.rdm) {
        MargArgs a{};
        a.c = p.c;
        a.k = p.k;
        a.k_lo = p.k_lo;
        a.k_hi = p.k_hi;
        a.u_hi = p.n - p.c - p.k_hi;
        a.s_log = 0;
        while ((1u << a.s_log) < p.slices) ++a.s_log;
        a.lo_mask = (uint32_t)(p.sel & ((1ull << p.c) - 1ull));
        int nl = 0, nh = 0, nu = 0;
        for (int pos = 0; pos < p.n; ++pos) {
            const bool sel = p.sel >> pos & 1ull;
            if (pos < p.c) {
                if (sel) a.lo_pos[nl++] = (int8_t)pos;
            } else if (sel) {
                a.hi_sel[nh++] = (int8_t)pos;
            } else {
                a.hi_uns[nu++] = (int8_t)pos;
            }
        }
        map.nbits = p.k;
        for (int i = 0; i < p.k; ++i) map.dst[i] = (int8_t)p.dst[i];
        hipLaunchKernelGGL(k_marginal_partial, dim3((unsigned)p.groups), dim3(256), 0, s, st, a, d_partials);
        QSIM_HIPCHK(hipGetLastError());
        launch_fold(d_partials, 1u << p.k, p.slices, map, d_out, s);
        return;
    }
    RdmArgs a{};
    a.p = p.c;
    a.panels = 1ull << (p.n - p.c);
    // the panel: every selected position and the p - k lowest unselected ones
    uint64_t in_panel = p.sel;
    for (int pos = 0, need = p.c - p.k; pos < p.n && need > 0; ++pos)
        if (!(p.sel >> pos & 1ull)) {
            in_panel |= 1ull << pos;
            --need;
        }
    int ne = 0, nsel = 0, nuns = 0;
    for (int pos = 0; pos < p.n; ++pos) {
        if (in_panel >> pos & 1ull) {
            a.pos[ne] = (int8_t)pos;
            a.slot[ne] = (int8_t)((p.sel >> pos & 1ull) ? nsel++ : p.k + nuns++);
            ++ne;
        } else {
            a.rest[a.nrest++] = (int8_t)pos;
        }
    }
    {
        double2* part = (double2*)d_partials;
        const unsigned groups = (unsigned)p.groups;
        switch (p.k) {
            case 0: launch_rdm_k<0>(st, a, groups, part, s); break;
            case 1: launch_rdm_k<1>(st, a, groups, part, s); break;
            case 2: launch_rdm_k<2>(st, a, groups, part, s); break;
            case 3: launch_rdm_k<3>(st, a, groups, part, s); break;
            case 4: launch_rdm_k<4>(st, a, groups, part, s); break;
            case 5: launch_rdm_k<5>(st, a, groups, part, s); break;
            case 6: launch_rdm_k<6>(st, a, groups, part, s); break;
            default: fail(QSIM_ERR_INVALID_ARGUMENT, "too many qubits for a reduced density matrix");
        }
        QSIM_HIPCHK(hipGetLastError());
    }
    // rows and columns of rho are numbered by ascending physical position here; the host maps them
    // to the caller's bit order when it mirrors the upper triangle (rdm_finish)
    launch_fold(d_partials, 2u << (2 * p.k), (uint32_t)p.groups, map, d_out, s);
}

void rdm_finish(const MarginalPlan& p, const double* raw, double* out) {
    const uint32_t D = 1u << p.k;
    auto place = [&](uint32_t t) {
        uint32_t o = 0;
        for (int i = 0; i < p.k; ++i) o |= (t >> i & 1u) << p.dst[i];
        return o;
    };
    for (uint32_t r = 0; r < D; ++r)
        for (uint32_t c = 0; c < D; ++c) {
            const uint32_t a = place(r), b = place(c);
            if (a > b) continue;  // the upper triangle in the caller's numbering
            const double re = raw[2 * ((size_t)r * D + c)], im = a == b ? 0.0 : raw[2 * ((size_t)r * D + c) + 1];
            out[2 * ((size_t)a * D + b)] = re;
            out[2 * ((size_t)a * D + b) + 1] = im;
            if (a == b) continue;
            out[2 * ((size_t)b * D + a)] = re;
            out[2 * ((size_t)b * D + a) + 1] = -im;
        }
}

}  // namespace qsim_hip

// ---- the C entries ----
using namespace qsim_hip;

// Both read s->d under s->perm as they are: no prep() / canonicalize(), nothing of the state changes.
static void run_marginal(qsim_state* s, const int32_t* qubits, int k, bool rdm, double* out) {
    check_state(s);
    QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
    DeviceGuard dg(s->device);
    share_flush(s);  // (pending gates of a run-sharing cycle; the layout may change with them)
    const MarginalPlan plan = lower_marginal(s->n, qubits, k, s->perm.empty() ? nullptr : s->perm.data(), rdm);
    const size_t out_bytes = (rdm ? (size_t)2 << (2 * k) : (size_t)1 << k) * sizeof(double);
    const size_t part_bytes = (plan.scratch_bytes + 255) & ~(size_t)255;
    char* buf = (char*)s->scratch.get(part_bytes + out_bytes, s->stream);
    double* d_out = (double*)(buf + part_bytes);
    launch_marginal(s->d, plan, (double*)buf, d_out, s->stream, &s->timer);
    std::vector<double> raw;
    if (rdm) raw.resize(out_bytes / sizeof(double));
    QSIM_HIPCHK(hipMemcpyAsync(rdm ? raw.data() : out, d_out, out_bytes, hipMemcpyDeviceToHost, s->stream));
    QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    if (rdm) rdm_finish(plan, raw.data(), out);
}

extern "C" int qsim_state_marginal_probabilities(qsim_state* s, const int32_t* qubits, int k, double* out) {
    return guarded([&] { run_marginal(s, qubits, k, false, out); });
}

extern "C" int qsim_state_reduced_density_matrix(qsim_state* s, const int32_t* qubits, int k, double* out) {
    return guarded([&] { run_marginal(s, qubits, k, true, out); });
}

extern "C" int qsim_marginal_plan(int n_qubits, const int32_t* qubits, int k, const int32_t* perm, int rdm,
                                  int32_t info[8]) {
    return guarded([&] {
        QSIM_REQUIRE(info, QSIM_ERR_INVALID_ARGUMENT, "null out");
        if (n_qubits < QSIM_MIN_QUBITS || n_qubits > 40) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
        const MarginalPlan p = lower_marginal(n_qubits, qubits, k, perm, rdm != 0);
        info[0] = p.k_lo;
        info[1] = p.k_hi;
        info[2] = (int32_t)p.slices;
        info[3] = (int32_t)p.groups;
        info[4] = (int32_t)(p.scratch_bytes & 0xffffffffull);
        info[5] = (int32_t)(p.scratch_bytes >> 32);
        info[6] = p.launches;
        info[7] = 0;
    });
}
