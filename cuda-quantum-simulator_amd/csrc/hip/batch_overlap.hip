// batch_overlap.hip — overlap (Gram) matrices of batched ensembles: out[i][j] = <a_i|b_j> for the
// members of two [B][2^n] ensembles, or of one with itself (qsim_batch_overlaps,
// qsim_batch_state_overlaps: batched.hip; no reference counterpart).
//
// The ensemble is a B x 2^n row-major complex matrix A, and G = conj(A) B^T with K = 2^n contiguous
// in both operands.  The work is cut into tiles of 64 x 64 members and chunks of K (overlap_plan:
// both depend on the shapes alone); one work-group owns one (tile, chunk), writes its partial tile
// to scratch, and k_overlap_reduce adds the partials of an entry in chunk order — no
// floating-point atomics, so the result is bitwise reproducible.
//
// Both tile kernels stage 16 k of the two 64-member panels through LDS as four real planes
// (Ar, Ai, Br, Bi; [64][18] doubles, padded so that the fragment reads below touch 32 different
// 8-byte banks per half-wave), the next stage's global loads in flight while the current one is
// multiplied.  k_overlap_mfma: four waves, each owning 32 x 32 of the tile as 2 x 2 blocks of
// v_mfma_f64_16x16x4_f64; per block and 4 k, Re += Ar Br + Ai Bi and Im += Ar Bi - Ai Br.  Lane l
// feeds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15] (one f64 each) and holds, in register
// r of the accumulator, D[row (l >> 4) + 4 r][col l & 15] — the f64 map, not the f32 one.  Blocks
// that lie wholly beyond Ba or Bb are skipped (the branch is uniform per wave).  k_overlap_vec:
// plain FMAs, thread (tx, ty) owning rows ty + 16 i and columns tx + 16 j; it runs the GEMV of
// qsim_batch_state_overlaps (a matrix core would idle 15 of 16 columns there) and, behind
// QSIM_OVERLAP_MFMA=0, everything else as a cross-check.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "engine.hpp"

namespace qsim_hip {

namespace {

constexpr int kOvTile = 64;      // members per tile side
constexpr int kOvStage = 16;     // k per LDS stage
constexpr int kOvLd = 18;        // doubles per plane row (16 + 2 of padding)
constexpr int kOvThreads = 256;  // per work-group, both tile kernels
constexpr int kOvLoads = kOvTile * kOvStage / kOvThreads;  // double2 per thread, panel and stage
constexpr uint64_t kOvTileEntries = (uint64_t)kOvTile * kOvTile;

typedef double v4d __attribute__((ext_vector_type(4)));

// Tile `idx` of the launch: row-major over Ta x Tb, or (self) over the upper triangle tj >= ti.
__device__ __forceinline__ void overlap_tile_of(uint64_t idx, uint32_t Tb, bool self, uint32_t& ti, uint32_t& tj) {
    if (!self) {
        ti = (uint32_t)(idx / Tb);
        tj = (uint32_t)(idx % Tb);
        return;
    }
    uint32_t i = 0;
    uint64_t row = Tb;  // tiles in tile-row i of the triangle
    while (idx >= row) {
        idx -= row;
        --row;
        ++i;
    }
    ti = i;
    tj = i + (uint32_t)idx;
}

// One stage of both panels in registers: element e = i * 256 + t is (member e >> 4, k e & 15), so 16
// lanes read 256 contiguous bytes of one member.  Members beyond the ensemble and k beyond k_end
// (<= 2^n) read as zero; nothing else is addressed.
struct OvRegs {
    double2 a[kOvLoads], b[kOvLoads];
};
__device__ __forceinline__ void overlap_load(OvRegs& r, const double2* __restrict__ A, const double2* __restrict__ Bm,
                                             int n, uint64_t row_a0, uint64_t row_b0, uint64_t Ba, uint64_t Bb,
                                             uint64_t k, uint64_t k_end, int t) {
#pragma unroll
    for (int i = 0; i < kOvLoads; ++i) {
        const int e = i * kOvThreads + t;
        const uint64_t ra = row_a0 + (uint64_t)(e >> 4), rb = row_b0 + (uint64_t)(e >> 4);
        const uint64_t kk = k + (uint64_t)(e & 15);
        const bool in_k = kk < k_end;
        r.a[i] = in_k && ra < Ba ? A[(ra << n) + kk] : make_double2(0.0, 0.0);
        r.b[i] = in_k && rb < Bb ? Bm[(rb << n) + kk] : make_double2(0.0, 0.0);
    }
}
__device__ __forceinline__ void overlap_store(const OvRegs& r, double (*sh)[kOvTile][kOvLd], int t) {
#pragma unroll
    for (int i = 0; i < kOvLoads; ++i) {
        const int e = i * kOvThreads + t;
        const int row = e >> 4, kk = e & 15;
        sh[0][row][kk] = r.a[i].x;
        sh[1][row][kk] = r.a[i].y;
        sh[2][row][kk] = r.b[i].x;
        sh[3][row][kk] = r.b[i].y;
    }
}

// grid (tiles, chunks); partials: [chunk][tile][64 x 64] complex, of which the entries inside
// Ba x Bb are written.
__global__ __launch_bounds__(kOvThreads) void k_overlap_mfma(const double2* __restrict__ A,
                                                             const double2* __restrict__ Bm, int n, uint64_t Ba,
                                                             uint64_t Bb, uint32_t Tb, int self, uint64_t chunk_len,
                                                             double2* __restrict__ partials) {
    __shared__ double sh[4][kOvTile][kOvLd];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);  // this wave's corner in the tile
    uint32_t ti, tj;
    overlap_tile_of(blockIdx.x, Tb, self != 0, ti, tj);
    const uint64_t row_a0 = (uint64_t)ti * kOvTile, row_b0 = (uint64_t)tj * kOvTile;
    const uint64_t K = 1ull << n, k0 = (uint64_t)blockIdx.y * chunk_len;
    const uint64_t k_end = k0 + chunk_len < K ? k0 + chunk_len : K;
    bool act[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            act[i][j] = row_a0 + (uint64_t)(wr + 16 * i) < Ba && row_b0 + (uint64_t)(wc + 16 * j) < Bb;
    v4d re[2][2], im[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            re[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
            im[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
        }
    OvRegs regs;
    overlap_load(regs, A, Bm, n, row_a0, row_b0, Ba, Bb, k0, k_end, t);
    for (uint64_t k = k0; k < k_end; k += kOvStage) {
        __syncthreads();  // (the stage before has been read)
        overlap_store(regs, sh, t);
        __syncthreads();
        if (k + kOvStage < k_end) overlap_load(regs, A, Bm, n, row_a0, row_b0, Ba, Bb, k + kOvStage, k_end, t);
#pragma unroll
        for (int k4 = 0; k4 < kOvStage / 4; ++k4) {
            const int kk = 4 * k4 + (lane >> 4);
            double ar[2], ai[2], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ar[i] = sh[0][wr + 16 * i + (lane & 15)][kk];
                ai[i] = sh[1][wr + 16 * i + (lane & 15)][kk];
                br[i] = sh[2][wc + 16 * i + (lane & 15)][kk];
                bi[i] = sh[3][wc + 16 * i + (lane & 15)][kk];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (!act[i][j]) continue;
                    re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], re[i][j], 0, 0, 0);
                    re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], bi[j], re[i][j], 0, 0, 0);
                    im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], bi[j], im[i][j], 0, 0, 0);
                    im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai[i], br[j], im[i][j], 0, 0, 0);
                }
        }
    }
    double2* dst = partials + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kOvTileEntries;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!act[i][j]) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr + 16 * i + (lane >> 4) + 4 * r, col = wc + 16 * j + (lane & 15);
                if (row_a0 + (uint64_t)row < Ba && row_b0 + (uint64_t)col < Bb)
                    dst[row * kOvTile + col] = make_double2(re[i][j][r], im[i][j][r]);
            }
        }
}

// The same tile and chunk with plain FMAs (same grid, same partials).
__global__ __launch_bounds__(kOvThreads) void k_overlap_vec(const double2* __restrict__ A,
                                                            const double2* __restrict__ Bm, int n, uint64_t Ba,
                                                            uint64_t Bb, uint32_t Tb, int self, uint64_t chunk_len,
                                                            double2* __restrict__ partials) {
    __shared__ double sh[4][kOvTile][kOvLd];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    uint32_t ti, tj;
    overlap_tile_of(blockIdx.x, Tb, self != 0, ti, tj);
    const uint64_t row_a0 = (uint64_t)ti * kOvTile, row_b0 = (uint64_t)tj * kOvTile;
    const uint64_t K = 1ull << n, k0 = (uint64_t)blockIdx.y * chunk_len;
    const uint64_t k_end = k0 + chunk_len < K ? k0 + chunk_len : K;
    int ni = 0, nj = 0;  // this thread's rows ty + 16 i, i < ni, and columns tx + 16 j, j < nj, exist
    for (int i = 0; i < 4; ++i) {
        ni += row_a0 + (uint64_t)(ty + 16 * i) < Ba;
        nj += row_b0 + (uint64_t)(tx + 16 * i) < Bb;
    }
    double re[4][4], im[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) re[i][j] = im[i][j] = 0.0;
    OvRegs regs;
    overlap_load(regs, A, Bm, n, row_a0, row_b0, Ba, Bb, k0, k_end, t);
    for (uint64_t k = k0; k < k_end; k += kOvStage) {
        __syncthreads();
        overlap_store(regs, sh, t);
        __syncthreads();
        if (k + kOvStage < k_end) overlap_load(regs, A, Bm, n, row_a0, row_b0, Ba, Bb, k + kOvStage, k_end, t);
        if (ni == 0 || nj == 0) continue;
        for (int kk = 0; kk < kOvStage; ++kk) {
            double ar[4], ai[4], br[4], bi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ar[i] = sh[0][ty + 16 * i][kk];
                ai[i] = sh[1][ty + 16 * i][kk];
                br[i] = sh[2][tx + 16 * i][kk];
                bi[i] = sh[3][tx + 16 * i][kk];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= nj) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    re[i][j] = fma(ar[i], br[j], re[i][j]);
                    re[i][j] = fma(ai[i], bi[j], re[i][j]);
                    im[i][j] = fma(ar[i], bi[j], im[i][j]);
                    im[i][j] = fma(-ai[i], br[j], im[i][j]);
                }
            }
        }
    }
    double2* dst = partials + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kOvTileEntries;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i < ni && j < nj) dst[(ty + 16 * i) * kOvTile + tx + 16 * j] = make_double2(re[i][j], im[i][j]);
}

// grid (tiles, 16): out[i][j] = the partials of the entry added in chunk order.  self: the entries
// of the upper triangle, the lower one written as their exact conjugates and the diagonal's
// imaginary part as +0.
__global__ __launch_bounds__(kOvThreads) void k_overlap_reduce(const double2* __restrict__ partials, uint32_t chunks,
                                                               uint32_t Tb, int self, uint64_t Ba, uint64_t Bb,
                                                               double2* __restrict__ out) {
    const int e = blockIdx.y * kOvThreads + threadIdx.x;
    const int r = e >> 6, c = e & 63;
    uint32_t ti, tj;
    overlap_tile_of(blockIdx.x, Tb, self != 0, ti, tj);
    const uint64_t gi = (uint64_t)ti * kOvTile + (uint64_t)r, gj = (uint64_t)tj * kOvTile + (uint64_t)c;
    if (gi >= Ba || gj >= Bb) return;
    if (self && gi > gj) return;  // (a diagonal tile's lower half: the mirror of its upper one)
    double sr = 0.0, si = 0.0;
    for (uint32_t ch = 0; ch < chunks; ++ch) {
        const double2 p = partials[((uint64_t)ch * gridDim.x + blockIdx.x) * kOvTileEntries + (uint64_t)e];
        sr += p.x;
        si += p.y;
    }
    if (!self) {
        out[gi * Bb + gj] = make_double2(sr, si);
    } else if (gi == gj) {
        out[gi * Bb + gj] = make_double2(sr, 0.0);
    } else {
        out[gi * Bb + gj] = make_double2(sr, si);
        out[gj * Bb + gi] = make_double2(sr, -si);
    }
}

}  // namespace

// The chunking rule: as many chunks (a power of two) as bring the launch to about 512 work-groups
// — two per CU — while a chunk keeps at least 256 k.
OverlapPlan overlap_plan(int n, uint64_t Ba, uint64_t Bb, bool self, bool mfma) {
    OverlapPlan p;
    p.mfma = mfma && Bb > 1;
    p.tiles_a = (Ba + kOvTile - 1) / kOvTile;
    p.tiles_b = (Bb + kOvTile - 1) / kOvTile;
    p.tiles = self ? p.tiles_a * (p.tiles_a + 1) / 2 : p.tiles_a * p.tiles_b;
    const uint64_t K = 1ull << n;
    uint64_t chunks = 1;
    while (chunks * p.tiles < 512 && K / (2 * chunks) >= 256) chunks *= 2;
    p.chunks = (uint32_t)chunks;
    p.chunk_len = K / chunks;
    p.scratch_bytes = chunks * p.tiles * kOvTileEntries * sizeof(double2);
    return p;
}

void launch_batch_overlap(const double2* a, const double2* b, int n, uint64_t Ba, uint64_t Bb, bool self,
                          const OverlapPlan& p, double2* d_partials, double2* d_out, hipStream_t s, Timer* tm) {
    if (p.tiles > 0x7fffffffull) fail(QSIM_ERR_INVALID_ARGUMENT, "too many members for one overlap launch");
    const dim3 grid((unsigned)p.tiles, p.chunks), block(kOvThreads);
    const double bytes = (double)((self ? Ba : Ba + Bb) * sizeof(double2)) * (double)(1ull << n);
    {
        TimedLaunch tl(tm, p.mfma ? "batch_overlap_mfma" : "batch_overlap_vec", bytes, s);
        if (p.mfma)
            hipLaunchKernelGGL(k_overlap_mfma, grid, block, 0, s, a, b, n, Ba, Bb, (uint32_t)p.tiles_b, self ? 1 : 0,
                               p.chunk_len, d_partials);
        else
            hipLaunchKernelGGL(k_overlap_vec, grid, block, 0, s, a, b, n, Ba, Bb, (uint32_t)p.tiles_b, self ? 1 : 0,
                               p.chunk_len, d_partials);
        QSIM_HIPCHK(hipGetLastError());
    }
    TimedLaunch tl(tm, "batch_overlap_reduce", 0.0, s);
    hipLaunchKernelGGL(k_overlap_reduce, dim3((unsigned)p.tiles, (unsigned)(kOvTileEntries / kOvThreads)), block, 0, s,
                       d_partials, p.chunks, (uint32_t)p.tiles_b, self ? 1 : 0, Ba, Bb, d_out);
    QSIM_HIPCHK(hipGetLastError());
}

}  // namespace qsim_hip
