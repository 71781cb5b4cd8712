// dm_expect.hip — Pauli-sum expectation values Re Tr(rho H), H = sum_t c_t P_t, of a density
// matrix, computed where rho lies (no readback, no layout restore).  No reference counterpart: the
// reference has no observable API; a caller copies the 4^n elements to the host.
//
// rho of n qubits lives in a 2n-bit state: amplitude k = i * 2^n + j holds rho[i][j].  Logical
// index bit q is the column bit of qubit q, logical bit q + n its row bit; the state's qubit
// permutation maps these 2n logical bits to physical positions.  A Pauli string is two masks over
// the n qubits: x (X or Y) and z (Z or Y), nY = popcount(x & z).  With
//     P|i> = i^nY (-1)^popcount(i & z) |i ^ x>             (as in expect.hip)
// the only non-zero entry of column i of P is row i ^ x, so
//     Tr(rho P) = sum_{i < 2^n} rho[i][i ^ x] i^nY (-1)^popcount(i & z):
// one string reads 2^n of the 4^n elements, one generalised diagonal per x mask.  Every one of
// the 2^n values of i is summed: the entry is a linear functional of whatever the buffer holds
// (Hermitian or not), and it returns the real part of the weighted sum.
//
// Terms with the same x read the same elements, so they form a group; a group is cut into rows of
// at most kExpectTerms terms with complex weights w_t = c_t i^nY, and a row accumulates
//     Re(W(i) rho[i][i ^ x]),  W(i) = sum_t (-1)^popcount(i & z_t) w_t.
//
// Addresses under relabeled bits: with both[q] = 1 << perm[q + n] | 1 << perm[q] (row and column
// position of qubit q), D(i) = OR of both[q] over the set bits of i is the address of rho[i][i],
// and, as moving bits commutes with XOR, rho[i][i ^ x] lies at D(i) ^ xcol, xcol = the bits of x
// at their column positions.  D(i) = D(i & 255) | D(i & ~255): a thread keeps the first part, the
// second is the same in all 256 threads of a work-group.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device_ops.hpp"
#include "engine.hpp"
#include "state.hpp"

namespace qsim_hip {

DmExpectPlan lower_dm_expectation(int n, const qsim_pauli_term* terms, size_t count, const int* perm) {
    if (n < 1 || n > QSIM_DM_MAX_QUBITS) fail(QSIM_ERR_INVALID_ARGUMENT, "bad qubit count");
    DmExpectPlan plan;
    plan.n = n;
    uint64_t seen = 0;
    for (int b = 0; b < 2 * n; ++b) {
        const int p = perm ? perm[b] : b;
        if (p < 0 || p >= 2 * n || (seen >> p & 1ull))
            fail(QSIM_ERR_INVALID_ARGUMENT, "perm is not a permutation of the 2n index bits");
        seen |= 1ull << p;
    }
    uint64_t col[QSIM_DM_MAX_QUBITS];
    for (int q = 0; q < n; ++q) {
        col[q] = 1ull << (perm ? perm[q] : q);
        plan.map.both[q] = col[q] | 1ull << (perm ? perm[q + n] : q + n);
    }
    // merged and grouped by the LOGICAL x mask (the kernel reads the sign from the logical i)
    const ExpectPlan lowered =
        lower_pauli_terms(n, terms, count, nullptr, [](uint64_t x, uint64_t z, double c, ExpectTerm& e) {
            switch (__builtin_popcountll(x & z) & 3) {  // c * i^nY
                case 0: e.cr = c; break;
                case 1: e.ci = c; break;
                case 2: e.cr = -c; break;
                default: e.ci = -c; break;
            }
        });
    plan.terms = lowered.terms;
    plan.groups = lowered.groups.size();
    for (const ExpectGroup& g : lowered.groups) {
        uint64_t xcol = 0;
        for (int q = 0; q < n; ++q)
            if (g.x >> q & 1ull) xcol |= col[q];
        for (size_t t0 = g.begin; t0 < g.end; t0 += kExpectTerms)
            plan.rows.push_back(DmExpectRow{xcol, (uint32_t)t0, (uint32_t)std::min<size_t>(kExpectTerms, g.end - t0)});
    }
    plan.launches = (plan.rows.size() + kDmExpectMaxRows - 1) / kDmExpectMaxRows;
    return plan;
}

unsigned dm_expect_chunks(int n) {
    return (unsigned)std::min<uint64_t>(((1ull << n) + 255) / 256, kDmExpectChunks);
}

namespace {

__device__ __forceinline__ uint64_t dm_deposit(const DmExpectMap& m, uint32_t i, int from, int to) {
    uint64_t a = 0;
    for (int q = from; q < to; ++q)
        if (i >> q & 1u) a |= m.both[q];
    return a;
}

// Work-group (c, r) adds row r's share of the runs i = (c + k gridDim.x) * 256 + thread < 2^n and
// writes partials[r * gridDim.x + c].
__global__ __launch_bounds__(256) void k_dm_expect_partial(const double2* rho, int n, DmExpectMap map,
                                                           const DmExpectRow* rows, const ExpectTerm* terms,
                                                           double* partials) {
    __shared__ ExpectTerm tab[kExpectTerms];
    __shared__ double wsum[4];
    const DmExpectRow row = rows[blockIdx.y];
    const int nterms = (int)row.count;
    for (int t = threadIdx.x; t < nterms; t += 256) tab[t] = terms[row.begin + t];
    __syncthreads();
    const uint32_t dim = 1u << n;
    const uint64_t lo = dm_deposit(map, threadIdx.x, 0, n < 8 ? n : 8);
    double acc = 0.0;
    for (uint32_t i0 = blockIdx.x * 256u; i0 < dim; i0 += gridDim.x * 256u) {
        const uint32_t i = i0 + threadIdx.x;
        if (i >= dim) break;  // (n < 8: one run, its upper threads idle)
        const double2 a = rho[(dm_deposit(map, i0, 8, n) | lo) ^ row.xcol];
        double wr, wi;
        term_weight<true>(tab, nterms, i, wr, wi);  // (a 32-bit i: the 32-bit population count)
        acc += wr * a.x - wi * a.y;  // Re(W rho)
    }
    acc = block_sum(acc, wsum);
    if (threadIdx.x == 0) partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

}  // namespace

static size_t dm_expect_table_bytes(const DmExpectPlan& plan) {
    return plan.rows.size() * sizeof(DmExpectRow) + plan.terms.size() * sizeof(ExpectTerm);
}

size_t dm_expect_work_doubles(const DmExpectPlan& plan) {
    const size_t rows = std::min<size_t>(plan.rows.size(), kDmExpectMaxRows);
    return rows * dm_expect_chunks(plan.n) + rows;
}

void launch_dm_expectation(const double2* rho, const DmExpectPlan& plan, DevBuf& table, double* d_work,
                           double* d_out, hipStream_t s, Timer* tm) {
    if (plan.rows.empty()) return;
    // one table: the rows, then the terms (sizeof(DmExpectRow) keeps the terms 8-byte aligned)
    const size_t rows_b = plan.rows.size() * sizeof(DmExpectRow);
    std::vector<unsigned char> blob(dm_expect_table_bytes(plan));
    std::memcpy(blob.data(), plan.rows.data(), rows_b);
    std::memcpy(blob.data() + rows_b, plan.terms.data(), plan.terms.size() * sizeof(ExpectTerm));
    table.upload(blob.data(), blob.size(), s);
    const DmExpectRow* d_rows = (const DmExpectRow*)table.ptr;
    const ExpectTerm* d_terms = (const ExpectTerm*)((const unsigned char*)table.ptr + rows_b);
    const unsigned chunks = dm_expect_chunks(plan.n);
    for (size_t r0 = 0; r0 < plan.rows.size(); r0 += kDmExpectMaxRows) {
        const unsigned nr = (unsigned)std::min<size_t>(kDmExpectMaxRows, plan.rows.size() - r0);
        double* d_rowsum = d_work + (size_t)nr * chunks;
        {
            TimedLaunch tl(tm, "dm_expect", 16.0 * (double)(1ull << plan.n) * nr, s);
            hipLaunchKernelGGL(k_dm_expect_partial, dim3(chunks, nr), dim3(256), 0, s, rho, plan.n, plan.map,
                               d_rows + r0, d_terms, d_work);
            QSIM_HIPCHK(hipGetLastError());
        }
        // fixed order: each row's chunks, then the rows
        launch_sum_partials(d_work, (int)chunks, nr, d_rowsum, false, s);
        launch_sum_partials(d_rowsum, (int)nr, 1, d_out, r0 != 0, s);
    }
}

}  // namespace qsim_hip

// ---- the C entries ----
using namespace qsim_hip;

// Reads s->d (the current buffer) under s->perm as they are: no prep() / canonicalize(), nothing of
// the state changes.
extern "C" int qsim_dm_expectation(qsim_state* s, int n, const qsim_pauli_term* terms, size_t count, double* out) {
    return guarded([&] {
        check_dm(s, n);
        QSIM_REQUIRE(out, QSIM_ERR_INVALID_ARGUMENT, "null out");
        QSIM_REQUIRE(terms || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        DeviceGuard dg(s->device);
        share_flush(s);  // (pending gates of a run-sharing cycle; the layout may change with them)
        const DmExpectPlan plan = lower_dm_expectation(n, terms, count, s->perm.empty() ? nullptr : s->perm.data());
        *out = 0.0;
        if (plan.rows.empty()) return;
        double* d_work = (double*)s->scratch.get(dm_expect_work_doubles(plan) * sizeof(double), s->stream);
        launch_dm_expectation(s->d, plan, s->expect_terms, d_work, s->d_result, s->stream, &s->timer);
        QSIM_HIPCHK(hipMemcpyAsync(out, s->d_result, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        QSIM_HIPCHK(hipStreamSynchronize(s->stream));
    });
}

extern "C" int qsim_dm_expectation_plan(int n, const qsim_pauli_term* terms, size_t count, const int32_t* perm,
                                        int* groups, int* rows, int* launches, uint64_t* elements) {
    return guarded([&] {
        QSIM_REQUIRE(terms || count == 0, QSIM_ERR_INVALID_ARGUMENT, "null term list");
        QSIM_REQUIRE(groups && rows && launches && elements, QSIM_ERR_INVALID_ARGUMENT, "null out");
        const DmExpectPlan plan = lower_dm_expectation(n, terms, count, perm);
        *groups = (int)plan.groups;
        *rows = (int)plan.rows.size();
        *launches = (int)plan.launches;
        *elements = (uint64_t)plan.groups << n;
    });
}
