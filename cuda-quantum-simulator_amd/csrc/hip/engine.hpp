// engine.hpp — internal declarations shared by the HIP translation units of libqsim_hip.so.
//
// Nothing here crosses the C ABI (include/qsim_hip.h).  Host code lowers each reference
// GateOp (include/Circuit.hpp:64-84) to an `Op`: a (multi-)controlled 2x2 unitary on one
// target, a (multi-)controlled diagonal, or a SWAP.  The kernels only know those three kinds.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "qsim_hip.h"

namespace qsim_hip {

// ---------------------------------------------------------------------------------------
// Errors (mapped to QSIM_ERR_* at the ABI boundary)
// ---------------------------------------------------------------------------------------
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
[[noreturn]] inline void fail(int code, const std::string& m) { throw Error(code, m); }
// Thread-local message returned by qsim_last_error() (state.hip).
void set_last_error(const char* msg);
// A boolean switch of the environment, read at every call (so a test or a benchmark runs both
// settings in one process): unset is `dflt`, else whether the value reads as a non-zero integer.
inline bool env_switch(const char* name, bool dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) != 0 : dflt;
}
// An integer of the environment (unset: `dflt`), read at every call likewise.  A setting that is
// fixed for the process keeps the value of either in a function-local static.
inline int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

#define QSIM_HIPCHK(call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            ::qsim_hip::fail(QSIM_ERR_DEVICE, std::string("HIP error: ") +                  \
                                                  hipGetErrorString(e_) + " at " __FILE__ ":" + \
                                                  std::to_string(__LINE__));                \
    } while (0)

// ---------------------------------------------------------------------------------------
// Lowered operations
// ---------------------------------------------------------------------------------------
enum Kind : int { K_M1 = 0, K_DIAG = 1, K_SWAP = 2 };

// Sub-kinds select exact reference arithmetic where the reference kernel has a closed form
// (src/Gates.cu:31-175), so per-gate results are bitwise those formulas.
enum Sub : int {
    S_GEN = 0,  // general complex 2x2 / general diagonal
    S_X = 1,    // swap                                   (Gates.cu:31-44)
    S_Y = 2,    // (im1,-re1),(-im0,re0)                  (Gates.cu:46-63)
    S_H = 3,    // (a0+-a1)*0.7071067811865476            (Gates.cu:79-104)
    S_NEG = 4,  // d1 = -1   (Z, CZ)                      (Gates.cu:65-77, 283-296)
    S_I = 5,    // d1 = +i   (S)                          (Gates.cu:106-119)
    S_MI = 6,   // d1 = -i   (Sdag)                       (Gates.cu:143-155)
    S_T = 7,    // d1 = (1+i)/sqrt2  as (re-im, re+im)*c  (Gates.cu:121-141)
    S_TDG = 8   // d1 = (1-i)/sqrt2  as (re+im, im-re)*c  (Gates.cu:157-175)
};

constexpr double kInvSqrt2 = 0.7071067811865476;  // literal used by src/Gates.cu:88

struct Op {
    int kind = K_M1;
    int sub = S_GEN;
    int t0 = 0, t1 = -1;   // target (t1: second SWAP qubit)
    uint64_t cmask = 0;    // control qubits, all must read 1
    bool d0_one = false;   // DIAG: d0 == 1 exactly -> only the |1> half is touched
    double m[8] = {0};     // M1: a,b,c,d ; DIAG: d0,d1 (re,im interleaved)
    int src = -1;          // index of the circuit gate this op came from
    int ncontrols() const { return __builtin_popcountll(cmask); }
};

// Lower one reference gate (validated) to an Op.  Throws Error on bad input.
Op lower_gate(const qsim_gate& g, int n_qubits);
// A gate list lowered under the labels `perm` (qubit q -> perm[q]; empty: the identity), op i
// from gate i (src = i).
std::vector<Op> lower_gates(int n, const qsim_gate* gates, size_t count, const std::vector<int>& perm);
// Validate a gate against n qubits with the reference's rules (src/Circuit.cpp:16-55).
void validate_gate(const qsim_gate& g, int n_qubits);
// Algorithmic HBM bytes of one op over `amps` amplitudes.
double op_alg_bytes(const Op& op, double amps);
const char* gate_name(int type);

// ---------------------------------------------------------------------------------------
// Kernel launch interface (gates.hip)
// ---------------------------------------------------------------------------------------
struct Timer;  // per-launch HIP-event attribution (state.hip)

// Apply one op to `batch` contiguous trajectories of 2^n amplitudes each.
void launch_op(double2* st, int n, uint64_t batch, const Op& op, hipStream_t s, Timer* tm);

// General 2^k x 2^k matrix (k <= 8) on `targets` (matrix-index bit j = targets[j]), d_mt the
// device copy of the transposed matrix, controlled on cmask.
void launch_matrixk(double2* st, int n, const int* targets, int k, const double2* d_mt,
                    uint64_t cmask, hipStream_t s, Timer* tm);
// General 4x4 on qubits (q0, q1) (m row-major over (b1 << 1) | b0, re/im interleaved), controlled.
void launch_matrix2q(double2* st, int n, int q0, int q1, const double* m, uint64_t cmask,
                     hipStream_t s, Timer* tm);

// Fused tile passes (fused.hip).
struct FusedPass {
    int single = -1;       // >= 0: not a tile pass but one per-gate op, Plan::singles[single]
    int h = 0;             // tile = 64 << h amplitudes (tile bits 0 .. 5 + h)
    int r0 = 6;            // tile bits 0 .. r0-1 are qubits 0 .. r0-1 (2^r0-amplitude HBM runs)
    int hpos[10] = {0};    // ascending physical qubits of tile bits r0 .. 5 + h (all >= r0)
    int rb = 4;            // staged: register bits per stage (threads per workgroup = 64 << h >> rb)
    int op_begin = 0, op_end = 0;  // range in the pass-op buffer (unstaged kernel)
    int stage_begin = 0, stage_end = 0;  // range in Plan::stages (staged kernel, h >= 4)
    int hu_count = 0;      // unnormalized H butterflies in the pass: store scales by 2^(-k/2)
    // Algorithmic HBM bytes per amplitude of the pass: min(32, sum of its gates' SURVEY §8(d)
    // bytes) — a pass of one CNOT is charged 16, not the 32 a full read+write would move.
    double alg_bpa = 32.0;
    // Relayout pass (plan_relayout, relayout.hip): the tile is loaded under this pass's layout
    // (r0 / hpos above) but stored under the next pass's: tile bit x goes to physical position
    // st_pos[x], tile-id bit i (the i-th non-tile position of the load layout, ascending) to
    // st_tid[i].  The last stage's lanes are the tile bits with the lowest store positions
    // (Stage::tmap), so the store still moves whole runs.
    int relayout = 0;
    int st_pos[13] = {0};
    int st_tid[32] = {0};
    int n_tid = 0;
};
struct TileOp {            // an Op re-expressed in tile-index bits
    int kind, sub, b0, b1;
    uint32_t cmask;
    int d0_one;
    int p0;                // staged kernel: register-bit position of the target (-1: thread bit)
    uint32_t cm_reg;       // staged kernel: controls among the stage bits, in register-bit space
    uint32_t cm_thr;       // staged kernel: controls among the other tile bits (tile space)
    // Pauli-frame fields (batched noisy runs, batched.hip): the op's circuit step, its target
    // qubit, and per control (<= 2) its qubit, register position in its stage (-1: thread bit)
    // and tile bit.
    int step, tq;
    int cq[2], cpos[2], cb[2];
    int _pad;
    // Tile-constant controls (tile_ctrl_out): physical positions outside the tile the op is
    // controlled on — the tile's non-tile bits are fixed, so the op runs on a whole tile or not
    // at all (a uniform branch on the tile's base address, no tile slot used).
    uint64_t cm_out;
    double m[8];
};
// A stage of a staged tile pass: every thread holds the 2^rb amplitudes spanned by `fix` (the
// stage's tile bits) in registers; ops in [op_begin, op_end) act on them with no LDS traffic.
// Register r of a stage holds tile element jb | offs(r), offs(r) = r spread over fix[].  Both
// address maps are XOR-linear in the element index, so their per-register parts are
// precomputed here and the kernel combines them with the thread part by one OR / XOR.
// LDS layout between two stages: element j lives at slot sigma(j) = j ^ sum_i parity(j & trow[i])
// << i (trow[i] only holds tile bits above i: triangular, so sigma is a bijection).  The planner
// picks trow per stage transition so that both the writes of the stage before (ds_write_b128:
// 8 groups of 8 lanes, slot mod 8) and the reads of the stage after (ds_read_b128: 4 groups of
// 16 lanes, slot mod 16) are bank-conflict-free (MI355X_MICROARCH.md §LDS); the fixed
// j ^ ((j >> 4) & 15) is 2-way conflicted whenever a stage's lanes span bits 0-3 and 4-7 unevenly.
struct Stage {
    uint64_t goff[16];     // HBM amplitude offset of offs(r) (its bits >= 6 spread over hpos)
    uint32_t lds[16];      // LDS byte offset 16 * sigma_in(offs(r)): this stage's reads
    uint32_t lds_w[16];    // LDS byte offset 16 * sigma_out(offs(r)): this stage's writes
    uint32_t trow_in[4], trow_out[4];  // the two layouts' sigma rows (see above)
    int fix[4];            // ascending stage tile bits
    int op_begin, op_end;
    // Thread bit i of the stage's element index jb sits at tile bit tmap[i] (the non-register
    // tile bits, ascending — the zero insertion at fix[] — except in the last stage of a
    // relayout pass, where they are ordered by store position).  tscatter != 0: use tmap.
    int tmap[10];
    int tscatter;
    int _pad;
};
// sigma of a layout (host and device)
__host__ __device__ __forceinline__ uint32_t lds_sigma(uint32_t j, const uint32_t* trow) {
    uint32_t s = j;
#pragma unroll
    for (int i = 0; i < 4; ++i) s ^= (uint32_t)(__builtin_popcount(j & trow[i]) & 1) << i;
    return s;
}
struct Plan {
    std::vector<FusedPass> passes;
    std::vector<TileOp> ops;
    std::vector<int> order;  // source gate index of each entry of `ops` (execution order)
    std::vector<Stage> stages;
    std::vector<Op> singles;  // ops run by the per-gate kernels (gate wider than the tile, n < 6)
    size_t fused_gate_count = 0;
    size_t tile_passes = 0;
};
constexpr int kTileHMax = 7;  // 64 << 7 = 8192 amplitudes = 128 KiB of LDS per workgroup
constexpr int kTileHDefault = 6;  // 12-qubit tiles unless QSIM_TILE_HMAX / qsim_set_tile_hmax
constexpr int kHposMax = 10;  // tile bits above the run: 6 + h - r0 <= 9
// Register bits per thread of a staged pass: 16 amplitudes per thread; 256 threads per workgroup
// up to h = 6, 512 at h = 7 (one 128 KiB workgroup per CU, the same 8 waves per CU).
constexpr int stage_rb(int h) { return h >= 6 ? 4 : h - 2; }
constexpr int stage_threads(int h) { return (64 << h) >> stage_rb(h); }
constexpr int kTileR0 = 6;    // contiguous run bits of a staged tile (QSIM_TILE_R0 in 4..6)
// hmax < 0: the process default (kTileHDefault, or QSIM_TILE_HMAX up to kTileHMax).
// avoid: qubits no tile may contain (ops never act on them; only tile padding is affected).
// avoid_first: the same for the plan's FIRST pass only (the sharded engine: the pivots of the
// remap before a step steer its leading pass, those of the remap after it every pass).
Plan plan_fused(const std::vector<Op>& ops, int n, int hmax = -1, uint64_t avoid = 0, uint64_t avoid_first = 0);
// Host-only introspection of a plan (tests).  write_stage_info (capi.hip): the record tables of
// qsim_plan_stage_info; tags (may be null) replaces an op's source index by (gate, origin word).
// exec_plan_on_host (relayout.hip): the plan's staged passes executed on 2^n interleaved re/im
// amplitudes with the kernels' index math (QSIM_ERR_RUNTIME on any other pass); amps is in logical
// order under the labels pi (bit b -> position pi[b]; null: the identity) the plan was made for.
struct StageInfoTag {
    int32_t gate, origin;
};
void write_stage_info(const Plan& plan, const std::vector<StageInfoTag>* tags, int32_t* ops, size_t op_cap,
                      size_t* n_ops, int32_t* passes, size_t pass_cap, size_t* n_passes, int32_t* stages,
                      size_t stage_cap, size_t* n_stages);
void exec_plan_on_host(const Plan& plan, int n, double* amps, const int* pi = nullptr);
// Rebuild the last pass of `plan` (staged) as a relayout pass that stores load position p at
// tau[p] (a permutation of 0..n-1; the sharded engine's fused remap pack / unpack).
void relayout_last_pass(Plan& plan, int n, const int* tau);
// One tile pass appended to a plan (fused.hip; plan_fused and the relayout planner use it).
// bit_of[q] < 0: op qubit q is not a tile qubit (a tile-constant control); phys_of (null: the
// identity) gives such a control's physical position under the pass's load layout.
void append_tile_pass(Plan& plan, const std::vector<Op>& ops, int n, int h, int r0, const int* hpos,
                      const int* bit_of, const int* st_pos, const int* st_tid, const int* phys_of = nullptr);
// Tile-constant controls (QSIM_TILE_CTRL_OUT, default 1; qsim_set_tile_ctrl_out): a control
// qubit need not be a tile qubit — planners then only require an op's targets in the tile.
// Off for the calling thread inside a CtrlOutOff scope (batched Pauli-frame plans).
bool tile_ctrl_out();
void tile_ctrl_out_configure(int mode);
struct CtrlOutOff {
    CtrlOutOff();
    ~CtrlOutOff();
    CtrlOutOff(const CtrlOutOff&) = delete;
    CtrlOutOff& operator=(const CtrlOutOff&) = delete;
  private:
    bool prev_;
};
// Relayout plans (relayout.hip): every pass stores its tile under the next pass's layout, so
// each pass may choose all of its tile qubits except the four of the contiguous run, which come
// from the pass before (the last pass restores the first layout, so re-runs need no restore).
// `lower` maps the circuit through a logical -> physical permutation exactly as the caller will.
// Returns false when no relayout plan beats `max_passes` passes.
struct RelayoutChoice {
    std::vector<int> perm;  // the first (and last) layout, logical -> physical
    std::vector<Op> ops;    // the circuit lowered under perm
    Plan plan;
    double cost_us = 0.0;   // predicted (layout model)
    // layouts[k] (logical -> physical) is what pass k loads and pass k - 1 stores; layouts[K] =
    // layouts[0] = perm.  pass_src[k]: the circuit gates (Op::src) pass k applies.
    std::vector<std::vector<int>> layouts;
    std::vector<std::vector<int>> pass_src;
};
bool plan_relayout(int n, const std::function<std::vector<Op>(const std::vector<int>&)>& lower,
                   size_t max_passes, RelayoutChoice& out);
// Up to QSIM_RELAYOUT_VARIANTS (default 3) closed tile sequences of the fewest passes, each with
// QSIM_RELAYOUT_LAYOUT_VARIANTS (default 2) position choices: relayout choices, best predicted first — the candidates a timed first run compares; memoised.
// rule.period > 0 (run sharing): the circuit is `copies` copies of `period` gates each, and the
// gates a pass may hoist from later copies are limited — cap_passes = 0: none more than one copy
// past its oldest gate's; cap_passes = P > 0: by the pass's position in a plan aimed at P passes
// (relayout.hip Search::copy_limit).
struct ShareRule {
    size_t period = 0, copies = 0, cap_passes = 0;
};
size_t plan_relayout_variants(int n, const std::function<std::vector<Op>(const std::vector<int>&)>& lower,
                              size_t max_passes, std::vector<RelayoutChoice>& out, const ShareRule& rule = {});
bool relayout_enabled(int n);  // QSIM_RELAYOUT (default 1), QSIM_RELAYOUT_MIN_QUBITS (default 20)
void relayout_configure(int mode, int min_qubits);  // qsim_set_relayout; < 0 leaves a setting
// A single gate-free relayout pass taking logical qubit q from physical perm[q] to q (n >= 12).
Plan plan_permutation_pass(int n, const std::vector<int>& perm);
// The same pass between any two layouts: logical qubit q goes from physical from[q] to to[q]
// (either may be empty: the identity).
Plan plan_permutation_pass(int n, const std::vector<int>& from, const std::vector<int>& to);
bool relayout_forced();  // mode 2: a relayout plan whenever one exists (tests)
// Run sharing (relayout.hip; driven by run.hip qsim_run): `copies` consecutive runs of one
// circuit planned as ONE relayout plan and executed piecewise, call by call.  Call j of a cycle
// launches the longest prefix of not-yet-launched passes whose gates all belong to copies <= j;
// the requested gates in later passes stay pending until the next call or the next reader.
struct SharePlan {
    int copies = 0;
    size_t count = 0;                        // gates per copy
    size_t cap_passes = 0;                   // the position cap P the plan was searched under (0: the tail rule)
    std::vector<Op> ops;                     // the copies in order, lowered under layouts[0]
    Plan plan;
    std::vector<std::vector<int>> layouts;   // RelayoutChoice::layouts of the joint plan
    std::vector<std::vector<int>> pass_src;  // joint gate indices (copy * count + gate) per pass
    std::vector<int> pass_copy;              // the highest copy a pass holds a gate of (-1: none)
};
// False when no joint plan needs fewer than copies * single_passes passes (memoised per circuit,
// in process and on disk, apart from single-run layout decisions: memo kind 4).
bool plan_share(int n, const qsim_gate* gates, size_t count, int copies, size_t single_passes, SharePlan& out);
// One more call of a cycle (calls: requested so far, next: the first pass not yet launched; both
// advanced): the passes [first, last) it launches.  True when the cycle is complete: every pass
// has run, nothing is pending, and calls / next are back at 0.
bool share_advance(const SharePlan& sp, int& calls, size_t& next, size_t& first, size_t& last);
// Requested gates (joint indices below calls * count) in passes >= next_pass, in circuit order.
std::vector<int> share_pending(const SharePlan& sp, size_t next_pass, int calls);
bool run_share_enabled(int n);  // QSIM_RUN_SHARE (default 1), from the relayout size threshold
// QSIM_RUN_SHARE_COPIES / qsim_set_run_share when set; else 4 below 26 qubits and 8 from there
int run_share_copies(int n);
void run_share_configure(int mode, int copies);  // qsim_set_run_share; negative: unchanged
int tile_height_default();             // the h that hmax < 0 means (scope, setting, env, 6)
int tile_height_for(int n);            // a single-GPU state's height (the setting, or by size)
bool tile_height_is_set();             // qsim_set_tile_height or QSIM_TILE_HMAX in force
void tile_height_configure(int h);     // qsim_set_tile_height: h < 0 restores the env default
int tile_rb_default(int heff);         // register bits per stage of a staged pass of height heff
int tile_rb7();                        // register bits per stage of 13-qubit tiles (4, or 3)
void tile_rb7_configure(int rb);       // qsim_set_tile_rb7: 3 or 4; else back to QSIM_TILE_RB7
int tile_rb_for(int n, int h);         // a single-GPU state's stage width (-1: stage_rb(h))
// Plans made by this thread while the scope lives default to height h and, for 12-qubit tiles,
// rb register bits per stage (qsim_run of a state).
struct TileHeightScope {
    explicit TileHeightScope(int h, int rb = -1);
    ~TileHeightScope();
    TileHeightScope(const TileHeightScope&) = delete;
    TileHeightScope& operator=(const TileHeightScope&) = delete;
  private:
    int prev_, prev_rb_;
};
// Layout-aware qubit relabeling (relabel.hip): predicted cost of a tile (qubit mask) in
// microseconds, the tiles of a plan's staged passes, and the permutation (logical -> physical)
// minimising the predicted cost of `tiles` (empty: keep the identity, < min_gain better).
bool relabel_enabled(int n);                        // policy (QSIM_RELABEL*, qsim_set_relabel)
bool relabel_mode_on();  // the mode alone (QSIM_RELABEL / qsim_set_relabel != 0), whatever the size
void relabel_configure(int mode, int min_qubits);   // < 0 leaves a setting unchanged
double layout_cost_us(uint64_t tile);
std::vector<uint64_t> plan_tiles(const Plan& plan);
double plan_layout_cost_us(const Plan& plan);
std::vector<int> choose_relabel(const std::vector<uint64_t>& tiles, int n, double* before, double* after,
                                double min_gain = 0.03);
// The layout for a whole circuit: labels chosen for fewer passes first, then the cheapest pass
// layouts (relabel.hip).  perm empty: keep the identity.  ops / plan: the circuit under perm as
// the caller's `lower` produced it, and its plan (for the caller's plan cache).
struct LayoutChoice {
    std::vector<int> perm;
    std::vector<Op> ops;
    Plan plan;
    size_t passes_before = 0;
    double cost_before = 0.0, cost_after = 0.0;
    // want_alts > 0: the next acceptable candidates (same pass count), predicted-cost order
    struct Alt {
        std::vector<int> perm;
        std::vector<Op> ops;
        Plan plan;
    };
    std::vector<Alt> alts;
};
// stage_us > 0: the fewest-pass candidates are ranked by their plans' layout cost plus stage_us per
// register stage (density-matrix passes spend their time in their stages) instead of by the
// annealed layout cost alone.
LayoutChoice choose_layout(int n, const std::function<std::vector<Op>(const std::vector<int>&)>& lower,
                           int tries, size_t want_alts = 0, double stage_us = 0.0);
// QSIM_RELABEL_CALIBRATE (default 1) / QSIM_RELABEL_CALIBRATE_MIN_QUBITS (default 26): with
// inline compilation (QSIM_JIT=2) the first run of a basis state times the model's choice and
// its alternatives with their circuit-specialised kernels and keeps the fastest (first_layout.hip).
bool relabel_calibrate(int n);
void calibrate_configure(int mode, int min_qubits);  // negative: unchanged
bool calibrate_mode_on();  // the calibration mode alone (QSIM_RELABEL_CALIBRATE / qsim_set_calibrate)
int relabel_tries();  // QSIM_RELABEL_TRIES (default 7): random labelings planned per choice
// Process-wide memo of layout choices per circuit (kind: 0 state, 1 batched with its run flags).
// h != null / h >= 0: a decision that also chose the tile height (cross-height calibration).
// On-disk cache across processes (cache.hip; QSIM_CACHE=0 off, QSIM_CACHE_DIR): hipRTC code objects
// keyed by their source and options, layout decisions keyed like the in-process memo.
std::string cache_dir();
uint64_t cache_hash(const void* p, size_t n, uint64_t seed);
bool jit_cache_load(const std::string& src, const std::string& opts, std::vector<char>& code);
void jit_cache_store(const std::string& src, const std::string& opts, const std::vector<char>& code);
bool layout_cache_load(int n, int kind, const void* key, size_t bytes, std::vector<int>& perm, int* h);
void layout_cache_store(int n, int kind, const void* key, size_t bytes, int h, const std::vector<int>& perm);
bool layout_memo_get(int n, int kind, const void* gates, size_t bytes, std::vector<int>& perm, int* h = nullptr);
void layout_memo_put(int n, int kind, const void* gates, size_t bytes, const std::vector<int>& perm, int h = -1);
bool calibrate_heights(int n);  // QSIM_CALIBRATE_HEIGHTS (first_layout.hip: choose_first_layout)
// Factor on the predicted cost of a 13-qubit tile (QSIM_LAYOUT_T13, default 1); a scope sets it
// for the calling thread (and choose_layout hands it to its worker threads).
double layout_t13();
struct LayoutT13Scope {
    explicit LayoutT13Scope(double f);
    ~LayoutT13Scope();
    LayoutT13Scope(const LayoutT13Scope&) = delete;
    LayoutT13Scope& operator=(const LayoutT13Scope&) = delete;
  private:
    double prev_;
};
// Circuit-specialised pass kernels (jit.hip): hipRTC code object of one plan on one device.
struct JitJob;
struct JitModule {
    hipModule_t mod = nullptr;
    std::vector<hipFunction_t> fn;  // per plan pass; null = run by the interpreter
    ~JitModule();
};
struct JitState {
    std::shared_ptr<JitJob> job;
    std::unique_ptr<JitModule> mod;
    bool failed = false;
};
int jit_mode();        // 0 off, 1 background compile (default), 2 compile on first use
bool jit_pass_pipelined(const FusedPass& p);  // persistent software-pipelined pass kernel (jit.hip)
int jit_min_qubits();  // smaller states never JIT (QSIM_JIT_MIN_QUBITS, default 20)
void jit_configure(int mode, int min_qubits);  // < 0 leaves a setting unchanged
void jit_shutdown();  // stop the background compiler (queued jobs dropped, running one joined)
std::string jit_source(const Plan& plan);      // empty when the plan has no staged pass
// A generated source copied out the way the *_jit_source entries return it (len: its length).
void copy_source(const std::string& src, char* buf, size_t cap, size_t* len);
bool jit_compile(const std::string& src, std::vector<char>& code, std::string& log);
// The loaded module for `plan`, or null while it compiles / when JIT does not apply.
const JitModule* jit_for(JitState& js, const Plan& plan, int n);

// The last few plans of one engine object (LRU): re-running a circuit (the benchmark loop,
// repeated trajectories, two circuits alternating on one state) skips the host planning and,
// once compiled, runs the specialised kernels.
struct PlanCache {
    struct Entry {
        int n = -1, h = -1;  // h: the tile height the plan was made for
        int ctrl_out = -1;   // tile_ctrl_out() when it was planned
        uint64_t avoid = 0, avoid_first = 0;
        std::vector<Op> key;
        Plan plan;
        JitState jit;
        uint64_t used = 0;
    };
    static constexpr size_t kEntries = 16;  // (first-run calibration keeps its candidates)
    std::vector<std::unique_ptr<Entry>> entries;
    uint64_t clock = 0;
    // stream: where the owner runs this cache's plans (drained before a plan is evicted)
    Entry& get(const std::vector<Op>& ops, int n_qubits, hipStream_t stream, uint64_t avoid = 0,
               uint64_t avoid_first = 0);
    // insert a plan computed elsewhere under `ops` (relabeling plans its candidates itself)
    void put(std::vector<Op> ops, int n_qubits, Plan plan, hipStream_t stream);
};
// Which part of a plan to launch: passes [first, last) over the sub-space whose qubits in
// fix_mask read fix_val (fix_mask = 0: the whole state).  Sub-space launches need staged passes.
struct FusedRange {
    size_t first = 0, last = SIZE_MAX;
    uint64_t fix_mask = 0, fix_val = 0;
    // relayout passes write out of place (a tile's store addresses are other tiles' load
    // addresses): they alternate between the state and `alt` (same size)
    double2* alt = nullptr;
};
// frames != null: batched noisy run under per-trajectory Pauli frames (FArgs::frames).
// sweep != null (never together with frames): batched parameter sweep — an op with step >= 0 takes
// its eight coefficients from sweep[(step * batch + member) * 8] (Op::m layout); a pass holding
// such an op always runs the interpreter, never a circuit-specialised kernel.
// Returns the buffer that holds the result (st, or range.alt after an odd number of relayout
// passes).
double2* launch_fused(double2* st, int n, uint64_t batch, const Plan& plan, const TileOp* d_ops,
                  const Stage* d_stages, hipStream_t s, Timer* tm, const JitModule* jm = nullptr,
                  const uint64_t* frames = nullptr, const FusedRange& range = FusedRange(),
                  const double* sweep = nullptr);
// Does pass `pidx` of the plan hold an op with step >= 0 (a frame-conjugated or member-dependent op)?
bool pass_has_step_op(const Plan& plan, size_t pidx);

// Per-gate kernels of a batched parameter sweep (batch_sweep.hip): `op` (K_M1 or K_DIAG, any
// control mask, any target, n >= 1) applied to every member of st ([batch][2^n]) with member t's
// eight coefficients at coef[t * 8] (Op::m layout) instead of op.m.  One launch.  Asynchronous.
void launch_sweep_op(double2* st, int n, uint64_t batch, const Op& op, const double* coef, hipStream_t s, Timer* tm);
// The angle every parameterised gate of a sweep is planned under (the plan and the qubit layout
// must not depend on the members' angles): no multiple of pi, so it lowers to S_GEN.
constexpr double kSweepPlaceholderAngle = 0.7390851332151607;

// Single-trajectory Monte-Carlo noise (noise.hip): one per-pair pass of channel `type`
// (reference NoiseType numbering) on `qubit`, uniforms from the hash of (seed, counter, pair);
// traj0: global trajectory index of trajectory 0 (the pair index hashed is the global one).
void launch_noise(double2* st, int n, int type, int qubit, double p, uint64_t seed,
                  uint64_t counter, hipStream_t s, Timer* tm, uint64_t batch = 1, uint64_t traj0 = 0);
// Every channel that follows one gate, passes counter, counter + 1, ... (counter is advanced):
// flip channels over a large batch run in one launch (work-group per unit of trajectories),
// otherwise one launch_noise per channel.  Same draws and results either way.
struct NoiseChan {
    int type, qubit;
    double p;
};
void launch_noise_after_gate(double2* st, int n, const std::vector<NoiseChan>& chans, uint64_t seed,
                             uint64_t& counter, hipStream_t s, Timer* tm, uint64_t batch, uint64_t traj0);
// Gate + in-tile noise (noise.hip): the gate and the prefix of `chans` whose qubits lie in its
// 4096-amplitude tile in one LDS pass, the rest by the push kernel; counter advances by
// chans.size().  Same states as launch_op + launch_noise_after_gate.  op == null: no gate.
bool gate_noise_tile_supported(int n, const Op* op);
void launch_gate_noise_step(double2* st, int n, uint64_t batch, uint64_t traj0, const Op* op,
                            const std::vector<NoiseChan>& chans, uint64_t seed, uint64_t& counter, hipStream_t s,
                            Timer* tm);
// A whole run of gate steps (ops[i].kind < 0: no gate) through the tile kernel, each step's
// prefix flip lists built by k_gn_lists on L->ms (two sets, event-ordered) during the step before;
// L == null or gate_noise_lists_bytes == 0: the tile kernels walk the blocks themselves.  Every
// op must pass gate_noise_tile_supported.  counter advances by ops.size() x chans.size().
struct GnLists {
    void* buf[2];
    size_t set_bytes;  // of one set (>= gate_noise_lists_bytes)
    hipStream_t ms;
    hipEvent_t built[2], used[2], start;
};
// Optional device blocks (a second 2^n buffer, code words, flip lists) are allocated only while
// the device keeps this much free beside them; a caller that is refused takes its in-place path.
constexpr size_t kAltMarginBytes = 256ull << 20;
size_t device_free_bytes();                // 0 when it cannot be read (the HIP error is cleared)
void* device_alloc_or_null(size_t bytes);  // null: the allocation failed (the HIP error is cleared)
// The block, when the device has `bytes + beside` free and the allocation succeeds; else null.
void* device_alloc_beside(size_t bytes, size_t beside);
// What a noisy run keeps beside the amplitudes for the pulled and in-tile schedules: the side
// stream their maps and lists are built on one or two steps ahead, its events, two sets of flip
// lists and two sets of code words.  Owned by a state, an ensemble, or one part of a split
// ensemble; nothing exists until the first run that needs it.
struct NoiseSide {
    hipStream_t stream = nullptr;
    hipEvent_t built[2] = {}, used[2] = {}, start = nullptr;
    char* lists = nullptr;
    size_t lists_cap = 0;  // bytes of ONE set
    unsigned char* codes = nullptr;
    size_t codes_cap = 0;  // bytes of ONE set
    NoiseSide() = default;
    NoiseSide(const NoiseSide&) = delete;
    NoiseSide& operator=(const NoiseSide&) = delete;
    // The stream and its events, once (low_priority: at the device's lowest stream priority).
    void ensure_stream(bool low_priority);
    // Two sets of `bytes` each; grow only (the old block is freed once `main` and the side stream
    // are idle).  false: the device has not 2 * bytes + kAltMarginBytes free, or refused.
    bool ensure_lists(size_t bytes, hipStream_t main);
    // Likewise (freed once `main` is idle: its passes are the words' last readers).  Whether the
    // device has room is the caller's rule; false: the allocation failed.
    bool ensure_codes(size_t bytes, hipStream_t main);
    void* words(size_t step) const { return codes + (step & 1) * codes_cap; }
    GnLists view() const;
    void release_lists();  // (the caller has synchronised every stream that used them)
    void release_codes();
    // Waits for the side stream, then drops everything; the owner calls it before it destroys the
    // main stream.
    void destroy() noexcept;
    ~NoiseSide() { destroy(); }
};
size_t gate_noise_lists_bytes(int n, uint64_t batch, const std::vector<NoiseChan>& chans);
void launch_gate_noise_run(double2* st, int n, uint64_t batch, uint64_t traj0, const std::vector<Op>& ops,
                           const std::vector<NoiseChan>& chans, uint64_t seed, uint64_t& counter, hipStream_t s,
                           Timer* tm, const GnLists* L);
// Pulled noise (noise.hip): the noise step after one gate (channels `chans`, passes counter0,
// counter0 + 1, ...; the push kernels' draws) applied by the NEXT gate's pass: dst = U (P src)
// out of place, op == null: the identity (the last step of a run).  words: >=
// pull_noise_codes_bytes (one code word per amplitude).  Supported when n >= 9, every channel
// flips (depolarizing / X / Y / Z) and at most 32 can fire; QSIM_NOISE_PULL=0 / 1 overrides the
// caller's default (NoisySimulator: on; BatchedSimulator: off — measured).
bool pull_noise_supported(int n, const std::vector<NoiseChan>& chans, bool default_on);
size_t pull_noise_codes_bytes(int n, uint64_t batch, size_t nch);
void launch_pull_noise_step(const double2* src, double2* dst, int n, uint64_t batch, uint64_t traj0,
                            const std::vector<NoiseChan>& chans, uint64_t seed, uint64_t counter0,
                            const Op* op, void* words, hipStream_t s, Timer* tm);
// Its two halves, for callers that build the next step's words on another stream while this
// step's pass runs (the map reads no amplitudes).
void launch_noise_map(int n, uint64_t batch, uint64_t traj0, const std::vector<NoiseChan>& chans, uint64_t seed,
                      uint64_t counter0, void* words, hipStream_t s, Timer* tm);
// next (optional): this pass also builds the NEXT step's code words (counter0: its first pass
// counter) — the word map fused into the pull pass (QSIM_NOISE_MAP_FUSED).
struct PullMapNext {
    uint64_t traj0, seed, counter0;
    void* words;
};
void launch_pull_gate(const double2* src, double2* dst, int n, uint64_t batch, const std::vector<NoiseChan>& chans,
                      const Op* op, const void* words, hipStream_t s, Timer* tm, const PullMapNext* next = nullptr);
// A whole pulled run of gate steps (ops[i].kind < 0: no gate): the first gate in place, then the
// noise after gate i and gate i + 1 in one pass out of place, the last noise step by an identity
// pass.  buf[cur] holds the amplitudes; the passes alternate between the two buffers; returns which
// one holds the result.  Step i's passes count from counter0 + i * chans.size().  overlap: the
// words of step i (set i & 1 of side.codes) are built on side.stream while the pass of step i - 1
// runs — the pass waits for them, the words of step i + 2 for that pass, the first two for whatever
// ran on `s` before; else every map on `s` right before its pass.  side: codes for these channels
// and (overlap) the stream are ensured by the caller.
int launch_pull_noise_run(double2* const buf[2], int cur, int n, uint64_t batch, uint64_t traj0,
                          const std::vector<Op>& ops, const std::vector<NoiseChan>& chans, uint64_t seed,
                          uint64_t counter0, NoiseSide& side, hipStream_t s, Timer* tm, bool overlap);

// Density matrices as 2n-index-bit states (density.hip).
void dm_lower(int n, const qsim_gate* gates, size_t count, const qsim_noise_channel* ch,
              size_t nch, std::vector<Op>& out, bool reference_y = false,
              std::vector<StageInfoTag>* tags = nullptr);
void dm_lower_channel(int n, int type, int qubit, double p, std::vector<Op>& out);
void launch_dm_diag(const double2* rho, int n, double* out, hipStream_t s);
void launch_dm_init(double2* rho, const double2* psi, int n, hipStream_t s);

// Reductions / readout helpers (reduce.hip)
void launch_init_basis(double2* st, int n, uint64_t batch, uint64_t basis, hipStream_t s);
void launch_probabilities(const double2* st, uint64_t count, double* out, hipStream_t s);
// sum over |a_i|^2 for i with ((i >> bit) & 1) == 0 (bit < 0: all), deterministic 2-pass.
double reduce_norm(const double2* st, int n, int bit, double* d_partials, double* d_result,
                   hipStream_t s);
// Second stage of the reductions: result[r] (+)= the `count` partials of row r < rows, added in a
// fixed order by one work-group per row (bitwise reproducible).
void launch_sum_partials(const double* partials, int count, unsigned rows, double* result, bool accumulate,
                         hipStream_t s);
void launch_collapse(double2* st, int n, int bit, int result, double scale, hipStream_t s);
// max over the 2^n amplitudes of the larger per-component |a - b| (d_partials: >= 2048 doubles).
double reduce_max_abs_diff(const double2* a, const double2* b, int n, double* d_partials, double* d_result,
                           hipStream_t s);
struct Scratch;
void launch_histogram(const int64_t* d_idx, uint64_t count, uint64_t N, unsigned long long* d_hist,
                      hipStream_t s);
// Host-only: chunk CDF of `sums` + per-shot (chunk, residual target); chunk -1: past the end.
void chunk_targets(const double* sums, uint64_t nchunks, const double* uniforms, int shots,
                   int64_t* chunk_of, double* target);
void sample_indices(const double2* st, int n, uint64_t batch, const double* uniforms, int shots,
                    int64_t* out, hipStream_t s, Scratch& scratch);
// ---- readout of a sharded state (dist_readout.hip; the collectives it uses: dist_exchange.hip) ----
// A chunk: the 2^c amplitudes sharing all logical index bits >= c, c = min(kDistChunkLog, L).
constexpr int kDistChunkLog = 12;
int dist_chunk_log(int L);
// Logical qubits below c that sit on a rank position (the sampler brings them local first).
uint64_t dist_localize_mask(int n, int L, int c, const int* perm);
// How one shard's chunks map to the state's: amask = the local positions of logical qubits
// 0 .. c-1 (pos[k]: of qubit k); a shard's chunk slot j numbers its chunks by the other local
// positions in ascending order, slot bit k landing on bit dst[k] of the global (logical) chunk id;
// rank_or: the id bits fixed by the shard's rank.
struct ChunkMap {
    int L, c;
    uint64_t amask, rank_or;
    int8_t dst[64];
    int8_t pos[kDistChunkLog];
};
ChunkMap make_chunk_map(int n, int L, int c, int rank, const int* perm);
// One shot's in-chunk search: the chunk's local offset (amask bits 0), its logical index bits
// >= c (hi), the residual target and where the result goes.
struct ShotJob {
    uint64_t base, hi;
    double target;
    int64_t shot;
};
// Doubles of partial sums launch_dist_chunk_sums needs for this map (d_partials).
size_t dist_chunk_partials_count(const ChunkMap& m, int* splits_log_out = nullptr);
// d_sums[global chunk id] = sum of |a|^2 over the chunk, for every chunk of shard `st`.
void launch_dist_chunk_sums(const double2* st, const ChunkMap& m, uint64_t nchunks, double* d_partials,
                            double* d_sums, hipStream_t s);
// d_out[job.shot] = (double)(job.hi | first in-chunk index whose prefix reaches job.target).
void launch_dist_chunk_search(const double2* st, const ChunkMap& m, const ShotJob* d_jobs, int count, int shots,
                              double* d_out, hipStream_t s);
// Average of |a|^2 over `batch` trajectories into out[2^n] (device).
void launch_avg_probabilities(const double2* st, int n, uint64_t batch, double* out,
                              hipStream_t s);

// Pauli-sum expectation values (expect.hip).  lower_expectation maps the terms' masks from logical
// to physical bits through perm (null: identity), merges duplicate strings, drops zero
// coefficients and groups the rest by physical x mask (one pass over the state per group; a
// group of more than kExpectTerms terms takes several launches).  Throws Error on a mask bit >= n.
constexpr int kExpectTerms = 256;  // capacity of a launch's term table in LDS
struct ExpectTerm {
    uint64_t z;     // physical z mask
    double cr, ci;  // weights of Re a / Im a of a pair (x == 0: cr = c, the weight of |psi_i|^2)
};
struct ExpectGroup {
    uint64_t x;  // physical x mask of every term in [begin, end)
    size_t begin, end;
};
struct ExpectPlan {
    std::vector<ExpectTerm> terms;
    std::vector<ExpectGroup> groups;
    size_t launches = 0;
};
ExpectPlan lower_expectation(int n, const qsim_pauli_term* terms, size_t count, const int* perm);
// The merge-and-group step shared by lower_expectation and lower_pauli_apply (adjoint.hip):
// weight(x, z, c, e) fills e.cr / e.ci of the merged term c * (physical x, z); e.z is set, the
// weights start at 0.
ExpectPlan lower_pauli_terms(int n, const qsim_pauli_term* terms, size_t count, const int* perm,
                             const std::function<void(uint64_t, uint64_t, double, ExpectTerm&)>& weight);
// The two host steps every Pauli lowering starts with (expect.hip): n in [1, 63] and perm (null:
// identity) a permutation of 0..n-1, else Error (invalid argument); a logical mask at its physical
// positions under perm.
void check_qubit_perm(int n, const int* perm);
uint64_t mask_to_physical(uint64_t m, int n, const int* perm);
// Every x / z mask of the list fits in n (< 64) qubits, else Error (out of range) whose message
// starts with `what`, the noun for the list's entries ("Pauli term", "Pauli rotation").
void check_pauli_masks(int n, const qsim_pauli_term* terms, size_t count, const char* what);
size_t expect_chunks(uint64_t batch);  // partials per trajectory a launch may write
// d_out[t] = the plan's sum on trajectory t of st ([batch][2^n]); terms: the owner's device copy of
// the term table (uploaded here), d_partials: batch * expect_chunks(batch) doubles.  Nothing is
// launched for an empty plan.  Asynchronous.
struct DevBuf;
void launch_expectation(const double2* st, int n, uint64_t batch, const ExpectPlan& plan, DevBuf& terms,
                        double* d_partials, double* d_out, hipStream_t s, Timer* tm);
// The z lane/run split of groups of at least kExpectSplitMin terms (QSIM_EXPECT_SPLIT, default 1).
constexpr int kExpectSplitMin = 16;
bool expect_split_on();

// Marginal probabilities and reduced density matrices of k qubits (marginal.hip).  The listed
// qubits are mapped to physical positions through perm (null: identity); positions below the run
// (c = min(n, kMarginalRunBits) bits) are binned inside a work-group, those above choose its runs.
constexpr int kMarginalMaxQubits = 20;   // 2^20 bins
constexpr int kRdmMaxQubits = 6;         // a 64 x 64 matrix
constexpr int kMarginalRunBits = 12;     // 4096 contiguous amplitudes, 16 per thread
constexpr int kMarginalGroupsLog = 12;   // work-groups aimed at when the state has that many runs
constexpr int kMarginalScratchLog = 26;  // partial sums never take more than 64 MiB
constexpr uint64_t kRdmGroups = 1024;    // work-groups (and partial matrices) of the matrix kernel
struct MarginalPlan {
    int n = 0, k = 0, c = 0;
    bool rdm = false;
    uint64_t sel = 0;        // selected physical positions
    int k_lo = 0, k_hi = 0;  // ... below / from position c
    unsigned slices = 1;     // marginal: slices of the unselected high bits; matrix: = groups
    uint64_t groups = 1;     // work-groups of the first kernel
    uint64_t scratch_bytes = 0;
    int launches = 0;
    std::vector<int> dst;    // bit i of a kernel-side index (ascending position) -> the caller's bit
};
// Throws Error: a duplicate qubit, k above the reader's cap or above n, a null list with k > 0, a
// perm that is no permutation (invalid argument); a qubit outside [0, n) (out of range).
MarginalPlan lower_marginal(int n, const int32_t* qubits, int k, const int* perm, bool rdm);
// d_out: 2^k doubles in the caller's bit order (marginal), or 2 * 4^k doubles of rho numbered by
// ascending physical position (matrix; rdm_finish makes the caller's matrix of it on the host).
// d_partials: plan.scratch_bytes.  Reads st only.  Asynchronous.
void launch_marginal(const double2* st, const MarginalPlan& plan, double* d_partials, double* d_out, hipStream_t s,
                     Timer* tm);
// Host: the upper triangle of raw in the caller's numbering, the diagonal's imaginary part zeroed,
// mirrored into the lower one (out == out^dagger bitwise).
void rdm_finish(const MarginalPlan& plan, const double* raw, double* out);
// The second kernel of these readers (marginal.hip), shared with dm_marginal.hip: out[place(t)] =
// sum over s < S of partials[s * T + t], t < T, added in a fixed order; place: bit i of t lands on
// bit dst[i] (nbits == 0: the identity).  Asynchronous.
struct FoldMap {
    int nbits;
    int8_t dst[24];
};
void launch_fold(const double* partials, uint32_t T, uint32_t S, const FoldMap& map, double* out, hipStream_t s);

// Marginals, reduced density matrices and the fidelity <psi|rho|psi> of a density matrix, read where
// rho lies (dm_marginal.hip).  rho of n qubits is a 2n-bit state: logical bit q is the column bit of
// qubit q, bit q + n its row bit; perm maps the 2n logical bits to physical positions (null:
// identity).  Both subset readers are one gather-reduce over address generators (masks over the 2n
// physical positions):
//     out[o] = sum over b < 2^(n-k) of buf[G_out(o) | G_sum(b)],  G(v) = OR of gen[i] over the set bits i of v
// complex for the matrix, the real part for the marginal.  Matrix: out index o = a << k | a' (row-
// major rho_A[a][a']), out_gen[j] = 1 << perm[q_j] (bit j of a'), out_gen[k + j] = 1 << perm[q_j + n]
// (bit j of a).  Marginal: out_gen[j] = both positions of q_j.  sum_gen: both positions of every
// unselected qubit, ascending.  All generators (n for the marginal, n + k for the matrix) are sorted by
// their lowest position: the lowest nt <= 8 are a work-group's thread bits, the other sum generators are looped
// over by each thread (2^s_log slices of them over work-groups), the other out generators choose
// the work-group.
constexpr int kDmGatherThreadBits = 8;  // 256 threads
constexpr int kDmGatherGroupsLog = 10;  // work-groups aimed at
struct DmGatherGen {
    uint64_t mask;
    int out_bit;  // bit of the caller's out index, -1: a sum generator
};
struct DmMarginalPlan {
    int n = 0, k = 0;
    bool rdm = false;
    std::vector<uint64_t> out_gen, sum_gen;  // in the caller's bit order / by ascending qubit
    std::vector<DmGatherGen> sorted;         // all of them by lowest position
    int nt = 0;                              // thread bits: sorted[0 .. nt)
    int s_log = 0;                           // slices of the looped sum generators
    uint64_t elements = 0, groups = 1, scratch_bytes = 0;
    int launches = 2;
};
// Throws Error as lower_marginal does (the same messages): n outside [1, QSIM_DM_MAX_QUBITS], a perm
// that is no permutation of the 2n bits, a duplicate qubit, k above kRdmMaxQubits (matrix) or n, a
// null list with k > 0 (invalid argument); a qubit outside [0, n) (out of range).
DmMarginalPlan lower_dm_marginal(int n, const int32_t* qubits, int k, const int* perm, bool rdm);
// d_out: 2^k doubles (marginal) or 2 * 4^k (matrix, row-major re/im) in the caller's bit order;
// d_partials: plan.scratch_bytes.  Reads rho only.  Asynchronous.
void launch_dm_marginal(const double2* rho, const DmMarginalPlan& plan, double* d_partials, double* d_out,
                        hipStream_t s, Timer* tm);
// Fidelity: *d_out = Re sum_ij conj(psi_i) rho[i][j] psi_j, one streaming pass over the 4^n elements
// in physical address order.  A run is 2^c contiguous elements; its t_r row bits and t_c column
// bits need 2^t_r + 2^t_c entries of psi, staged in LDS per run (c = min(2n, 12), one less when all
// twelve are of one kind so the tables stay within kDmFidelityTable entries).
constexpr unsigned kDmFidelityGroups = 512;  // work-groups (a state of more runs: several per group)
constexpr int kDmFidelityTable = 2052;       // >= 2^11 + 2^1
struct DmFidelityPlan {
    int n = 0, c = 0, t_r = 0, t_c = 0;
    int8_t qubit[2 * QSIM_DM_MAX_QUBITS];  // physical position -> its qubit
    uint32_t row_mask = 0;                  // physical positions that are row bits
    uint64_t runs = 1;
    unsigned groups = 1;
};
DmFidelityPlan lower_dm_fidelity(int n, const int* perm);
// d_psi: device copy of psi (2^n); d_partials: plan.groups doubles.
void launch_dm_fidelity(const double2* rho, const double2* d_psi, const DmFidelityPlan& plan, double* d_partials,
                        double* d_out, hipStream_t s, Timer* tm);

// Pauli-sum expectation values Re Tr(rho H) of a density matrix (dm_expect.hip).  Terms are merged
// and grouped by logical x mask (one generalised diagonal of rho, 2^n elements, per group) and a
// group is cut into rows of at most kExpectTerms terms with complex weights c i^nY (cr + i ci, z:
// the LOGICAL z mask); one launch runs a (chunks of i, rows) grid, at most kDmExpectMaxRows rows.
constexpr size_t kDmExpectMaxRows = 65535;  // the grid's y limit
constexpr unsigned kDmExpectChunks = 128;   // work-groups along i (256 values of i per run)
struct DmExpectMap {
    uint64_t both[QSIM_DM_MAX_QUBITS];  // physical row bit | column bit of qubit q
};
struct DmExpectRow {
    uint64_t xcol;          // the group's x mask at the physical column positions
    uint32_t begin, count;  // the row's terms in DmExpectPlan::terms
};
struct DmExpectPlan {
    int n = 0;
    DmExpectMap map{};
    std::vector<ExpectTerm> terms;
    std::vector<DmExpectRow> rows;
    size_t groups = 0, launches = 0;
};
// perm: the 2n index bits' logical -> physical map (null: identity).  Throws Error: n outside
// [1, QSIM_DM_MAX_QUBITS] or a perm that is no permutation (invalid argument), a mask bit >= n (out
// of range).
DmExpectPlan lower_dm_expectation(int n, const qsim_pauli_term* terms, size_t count, const int* perm);
unsigned dm_expect_chunks(int n);
size_t dm_expect_work_doubles(const DmExpectPlan& plan);  // doubles of d_work a plan's launches need
// *d_out = the plan's sum over rho (a 2n-bit state's current buffer); table: the owner's device copy
// of the rows and terms (uploaded here).  Partial sums are added in a fixed order (no atomics).
// Nothing is launched for a plan without rows.  Asynchronous.
void launch_dm_expectation(const double2* rho, const DmExpectPlan& plan, DevBuf& table, double* d_work,
                           double* d_out, hipStream_t s, Timer* tm);

// Pauli-sum expectation values on a sharded state (lowering: dist_expect.hip; the launch: expect.hip;
// the transfers and collectives it uses: dist_exchange.hip).  A physical x mask splits into local bits (< L) and rank bits:
// x = x_loc | x_rank << L.  Groups with x_rank == 0 pair inside a shard (launch_expectation on the
// shard, n = L); a group with x_rank != 0 pairs shard r with shard r ^ x_rank and needs half of
// the peer's shard.  Cross groups with the same key (x_rank, top local position in x_loc) share
// one transfer; lower_expectation's order by x is already the order by key.
struct DistExpectCross {
    uint64_t x_rank, x_loc;
    size_t begin, end;  // the group's terms in DistExpectPlan::all.terms
    size_t xbegin;      // the same terms in the cross table (dist_expect_cross_terms)
    size_t transfer;    // index of the transfer it reads
};
struct DistExpectTransfer {
    uint64_t x_rank;
    bool top;  // position L-1 is in x_loc
};
struct DistExpectPlan {
    ExpectPlan all;                // lower_expectation over the n physical positions
    std::vector<size_t> local;     // indices into all.groups with x_rank == 0
    std::vector<DistExpectCross> cross;
    std::vector<DistExpectTransfer> transfers;
    size_t cross_terms = 0, launches = 0;  // launches: kernel launches per shard, both kinds
};
DistExpectPlan lower_dist_expectation(int n, int L, const qsim_pauli_term* terms, size_t count, const int* perm);
// The tables of shard `rank`: z keeps its local bits, the sign (-1)^popcount(rank & z_rank) is
// folded into cr / ci.  Local: a plan for launch_expectation with n = L.  Cross: the terms of
// every cross group in plan order (group c at [xbegin, xbegin + end - begin)).
ExpectPlan dist_expect_local(const DistExpectPlan& p, int L, int rank);
std::vector<ExpectTerm> dist_expect_cross_terms(const DistExpectPlan& p, int L, int rank);
// The half of its own shard (0 lower, 1 upper: the value of local bit L-1) that rank `rank`
// pairs in a transfer's groups, and the half it sends to rank ^ x_rank.
int dist_expect_own_half(const DistExpectTransfer& t, int rank);
int dist_expect_send_half(const DistExpectTransfer& t, int rank);
// *d_out (+)= sum over k < 2^(L-1) of W_re(i) Re a + W_im(i) Im a, i = k | half << (L-1) the local
// index of own[k], a = conj(peer[k ^ (x_loc mod 2^(L-1))]) own[k]; W as in expect.hip over the
// group's terms (d_terms: device, count terms, several launches past kExpectTerms).  own / peer:
// 2^(L-1) amplitudes each; d_partials: expect_chunks(1) doubles.  Asynchronous.
void launch_dist_expectation(const double2* own, const double2* peer, int L, int half, uint64_t x_loc,
                             const ExpectTerm* d_terms, size_t count, double* d_partials, double* d_out,
                             bool accumulate, hipStream_t s, Timer* tm);

// Adjoint-method gradients (adjoint.hip).  A rotation's generator: pauli = 1 X, 2 Y, 3 Z on
// position t (0: the identity, a plain inner product), times |1><1| on position c when c >= 0.
struct Generator {
    int pauli = 0, t = -1, c = -1;
};
bool gate_is_parameterised(int type);
qsim_gate gate_inverse(const qsim_gate& g);    // S <-> Sdag, T <-> Tdag, rotations: angle negated
Generator gate_generator(const qsim_gate& g);  // of a parameterised gate, on the gate's own qubits
bool adjoint_fused_on();                       // QSIM_ADJOINT_FUSED (default 1), read at every call
// The arguments of a gradient call or plan (single state and sharded): null lists (invalid
// argument), every gate against n qubits (validate_gate), the observable's masks (out of range).
void check_gradient_args(int n, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms, size_t nterms);
// The terms of dst = H src, merged and grouped by physical x mask like lower_expectation; a term's
// (cr, ci) is its complex weight c (-i)^nY (the kernel adds the sign (-1)^popcount(i & z)).
ExpectPlan lower_pauli_apply(int n, const qsim_pauli_term* terms, size_t count, const int* perm);
// dst = H src out of place (src != dst), one streaming pass per launch of the plan; an empty plan
// zeroes dst.  terms: the owner's device copy of the term table.  batch: src and dst hold that many
// members of 2^n amplitudes, each multiplied by H on its own.  Asynchronous.
void launch_pauli_apply(const double2* src, double2* dst, int n, const ExpectPlan& plan, DevBuf& terms,
                        hipStream_t s, Timer* tm, uint64_t batch = 1);
// *d_re + i *d_im = <a| G |b> (either may be null), d_partials: 2 * expect_chunks(1) doubles.
void launch_braket(const double2* a, const double2* b, int n, const Generator& g, double* d_partials, double* d_re,
                   double* d_im, hipStream_t s, Timer* tm);
// *d_out = Im <lam| G |phi>, then inv (the lowered inverse of the rotation: K_M1 or K_DIAG on g's
// target and control) applied to both states, in one launch.
void launch_adjoint_step(double2* phi, double2* lam, int n, const Generator& g, const Op& inv, double* d_partials,
                         double* d_out, hipStream_t s, Timer* tm);

// One launch of it per kExpectTerms terms of one group: dst[i] (+)= W(i) src[i ^ x] over the
// `count` device terms at d_terms; first: the first launch writes dst, later ones accumulate.
void launch_pauli_apply_group(const double2* src, double2* dst, int n, uint64_t x, const ExpectTerm* d_terms,
                              size_t count, bool first, hipStream_t s, Timer* tm, uint64_t batch = 1);

// Pauli-string rotations exp(-i theta/2 P) (pauli_rot.hip).  A rotation under the state's layout:
// physical masks (the convention of qsim_pauli_term) and the angle.
struct PauliRot {
    uint64_t x, z;
    double theta;
};
// A sequence in application order.  passes: streaming passes over the state (one per x != 0
// rotation, one per maximal run of consecutive x == 0 rotations); launches: kernel launches (a run
// of more than kExpectTerms rotations takes several).
struct PauliRotPlan {
    std::vector<PauliRot> rots;
    size_t passes = 0, launches = 0;
};
// Maps the masks from logical to physical bits through perm (null: identity); nothing is merged or
// reordered.  Throws Error: a null list or a perm that is no permutation (invalid argument), a
// mask bit >= n anywhere in the sequence (out of range).
PauliRotPlan lower_pauli_rotations(int n, const qsim_pauli_term* rots, size_t count, const int* perm);
uint64_t pauli_stream_blocks();  // QSIM_PAULI_BLOCKS (default 65536), read at every call
// st <- exp(-i theta/2 P) st in place, x != 0: one thread per pair (i, i ^ x).  Asynchronous.
void launch_pauli_rot(double2* st, int n, const PauliRot& r, hipStream_t s, Timer* tm);
// st[i] *= exp(-i/2 sum_t theta_t (-1)^popcount(i & z_t)) over `count` device terms (z, cr = theta),
// one launch per kExpectTerms of them.
void launch_pauli_phase(double2* st, int n, const ExpectTerm* d_terms, size_t count, hipStream_t s, Timer* tm);
// The whole plan on st; terms: the owner's device copy of the x == 0 runs' tables (one upload).
void launch_pauli_rotations(double2* st, int n, const PauliRotPlan& plan, DevBuf& terms, hipStream_t s, Timer* tm);
// *d_out = Im <lam| P |phi>, then (apply) exp(+i theta/2 P) on both states, in one launch; without
// apply nothing is stored: the bra-ket alone.  d_partials: expect_chunks(1) doubles.  negate: the
// generator is -P (a shard on which the string's rank factors give -1), folded in on the host.
void launch_pauli_adjoint_step(double2* phi, double2* lam, int n, const PauliRot& r, bool apply, double* d_partials,
                               double* d_out, hipStream_t s, Timer* tm, bool negate = false);

// Pauli-string rotations on a sharded state (dist_pauli_rot.hip; the transfers and collectives
// they use: dist_exchange.hip).  A rotation's physical masks split as x = x_loc | x_rank << L, z alike.
enum {
    DPR_PHASE = 0,  // x == 0: part of a run of Z/I-only rotations, pauli_phase on each shard
    DPR_LOCAL = 1,  // x_rank == 0, x_loc != 0: pauli_rot on each shard
    DPR_CROSS = 2   // x_rank != 0: rank r pairs with r ^ x_rank, one whole-shard transfer
};
struct DistPauliRot {
    int cls;
    uint64_t x_loc, z_loc, x_rank, z_rank;
    double theta;
    int ny;  // popcount(x & z) over all n positions
};
struct DistPauliRotPlan {
    std::vector<DistPauliRot> rots;  // application order
    size_t phase = 0, local = 0, cross = 0, cross_pure = 0;  // rotations by class; cross with x_loc == 0
    size_t phase_passes = 0;                                 // maximal runs of consecutive phase rotations
    size_t launches = 0;                                     // kernel launches per shard
};
// lower_pauli_rotations over the n physical positions (its checks and errors), then the split.
DistPauliRotPlan lower_dist_pauli_rotations(int n, int L, const qsim_pauli_term* rots, size_t count, const int* perm);
// The sign of P's rank factors on shard `rank`, for the classes that read the shard itself (phase,
// local: (-1)^popcount(rank & z_rank)) and for a cross rotation, which reads rank ^ x_rank's.
inline bool dist_pauli_rank_neg(const DistPauliRot& r, int rank) {
    return __builtin_popcountll(((uint64_t)rank ^ r.x_rank) & r.z_rank) & 1;
}
// A phase or local rotation as shard `rank` runs it with n = L: the rank sign folded into theta.
PauliRot dist_pauli_shard_rot(const DistPauliRot& r, int rank);
// A cross rotation on one shard, peer = the whole old shard of rank ^ x_rank.  With
// (P v)_own[i] = g sg(i) peer[i ^ x_loc], sg(i) = (-1)^popcount((i ^ x_loc) & z_loc), g = i^nY times
// the rank sign:  own[i] <- cos(theta/2) own[i] + (-+) i sin(theta/2) (P v)_own[i], - forward,
// + adjoint (the sweep's U^†).  lam != null (own = phi): first *d_out = this rank's share of
// Im <lam| P |phi>; store = false (needs lam): that alone, nothing is written.  d_partials:
// expect_chunks(1) doubles.  Asynchronous.
void launch_dist_pauli_rot(double2* own, const double2* peer, const double2* lam, int L, const DistPauliRot& r,
                           int rank, bool adjoint, bool store, double* d_partials, double* d_out, hipStream_t s,
                           Timer* tm);

// Adjoint-method gradients on a sharded state (dist_adjoint.hip; the transfers, the inverted
// segments and the collectives it uses: dist_plan.hip, dist_run.hip, dist_exchange.hip).
// lambda = H phi on shards: lower_pauli_apply over the n physical positions, each group's x mask
// split into x_loc | x_rank << L.  Groups come ordered by x, so groups of one x_rank are adjacent
// and share the transfer of the peer's phi shard.
struct DistApplyGroup {
    uint64_t x_rank, x_loc;
    size_t begin, end;  // the group's terms in DistApplyPlan::all.terms (and in a shard's table)
};
struct DistApplyPlan {
    ExpectPlan all;
    std::vector<DistApplyGroup> groups;  // plan order
    size_t local_groups = 0, cross_groups = 0, transfers = 0, launches = 0;
};
DistApplyPlan lower_dist_apply(int n, int L, const qsim_pauli_term* terms, size_t count, const int* perm);
// A term as shard `rank` sees it: the local z bits, the sign of the rank's z bits folded into cr / ci.
ExpectTerm dist_shard_term(const ExpectTerm& e, int L, int rank);
std::vector<ExpectTerm> dist_apply_terms(const DistApplyPlan& p, int L, int rank);  // all.terms for that shard
// Class of a parameterised gate (logical qubits) under qubit map perm with L local positions.
enum {
    DG_LOCAL = 0,        // target local, control local or absent
    DG_LOCAL_CRANK = 1,  // target local, control on a rank position
    DG_DIAG = 2,         // Rz / CRZ, target on a rank position, control local or absent
    DG_DIAG_CRANK = 3,   // ... control on a rank position
    DG_CROSS = 4,        // Rx / Ry / CRY, target on a rank position, control local or absent
    DG_CROSS_CRANK = 5   // ... control on a rank position
};
int dist_gradient_class(const qsim_gate& g, const int* perm, int L);
// DG_DIAG step on one shard: *d_out = sgn Im <lam|phi> over the active indices (all 2^L, or those
// with local bit cpos set when cpos >= 0), then both states times the entry of inv (K_DIAG, the
// lowered inverse rotation) for this rank's target bit v.  d_partials: expect_chunks(1) doubles.
void launch_dist_adjoint_diag(double2* phi, double2* lam, int L, int cpos, int v, const Op& inv, double* d_partials,
                              double* d_out, hipStream_t s, Timer* tm);
// DG_CROSS step, one work state on one shard: own <- row v of inv (K_M1) applied to (own, peer),
// peer = the whole old shard of the rank whose target bit differs.  lam != null (own = phi):
// first *d_out = this rank's share of Im <lam| G |phi>, G = X (pauli 1) or Y (2); lam == null: the
// update alone (own = lambda, peer = the partner's old lambda).
void launch_dist_adjoint_step(double2* own, const double2* peer, const double2* lam, int L, int pauli, int cpos, int v,
                              const Op& inv, double* d_partials, double* d_out, hipStream_t s, Timer* tm);

// ---------------------------------------------------------------------------------------
// Timing (state.hip): per-launch HIP events grouped by kernel name.
// ---------------------------------------------------------------------------------------
struct Timer {
    struct Pending { int slot; hipEvent_t a, b; double bytes; };
    struct Stat { std::string name; double ms = 0; int64_t launches = 0; double bytes = 0; };
    bool enabled = false;
    std::vector<Stat> stats;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    hipStream_t stream = nullptr;
    int slot_of(const char* name);
    void begin(const char* name, double bytes, hipEvent_t* a_out, int* slot_out);
    void end(int slot, hipEvent_t a, double bytes);
    // ext mode: two events for a launch to time itself; finish() queues them for resolve()
    void begin_ext(const char* name, hipEvent_t* a_out, hipEvent_t* b_out, int* slot_out);
    void finish(int slot, hipEvent_t a, hipEvent_t b, double bytes);
    void resolve();   // synchronizes on outstanding events
    void reset();
    ~Timer();
};
// Device copy of a small host descriptor array (fused plans).  Uploads only when the bytes
// change (a re-run of the same circuit re-uses the resident plan); the host shadow stays alive
// until the async copy that reads it has completed.
struct DevBuf {
    void* ptr = nullptr;
    size_t cap = 0;
    std::vector<unsigned char> shadow;
    hipEvent_t copied = nullptr;
    void upload(const void* src, size_t bytes, hipStream_t s);
    ~DevBuf();
};

// Grow-only device scratch of one engine object (readback / sampling temporaries).  Every user
// synchronises its stream before returning, so the next user may reuse the memory; growing
// waits for the stream before the old block is freed.  (Plain hipMalloc memory: the
// stream-ordered pool is not used for buffers that pageable host copies read or write.)
struct Scratch {
    void* ptr = nullptr;
    size_t cap = 0;
    void* get(size_t bytes, hipStream_t s);
    ~Scratch();
};

// Adjoint gradients of a batched parameter sweep (batch_adjoint.hip; the entry points and what they
// share with the sweep: batched.hip).  The work of the backward sweep: two ensembles ([batch][2^n]
// each) kept across calls, one result per (slot, member), the per-work-group partial sums of a step
// and, on the cross-check path (QSIM_ADJOINT_FUSED=0) alone, one slot's conjugated coefficients.
struct BatchGradWork {
    double2* phi = nullptr;
    double2* lam = nullptr;
    double* d_out = nullptr;  // out_cap doubles: [slot][member]
    size_t out_cap = 0;
    double* d_partials = nullptr;  // batch_adjoint_partials doubles
    double* d_conj = nullptr;      // [batch][8]
    DevBuf ops, stages, terms;
    PlanCache plans;  // the inverted fixed segments
    BatchGradWork() = default;
    BatchGradWork(const BatchGradWork&) = delete;
    BatchGradWork& operator=(const BatchGradWork&) = delete;
    ~BatchGradWork();
};
// The work for `batch` members of n qubits and n_slots parameters, allocated on first use (d_out
// grows on demand; s: the stream its users run on).  A refused allocation clears the HIP error,
// drops the whole work (slot becomes null) and throws Error (QSIM_ERR_DEVICE).
BatchGradWork& batch_grad_ensure(std::unique_ptr<BatchGradWork>& slot, int n, uint64_t batch, size_t n_slots,
                                 hipStream_t s);
size_t batch_adjoint_partials(int n, uint64_t batch);  // doubles of d_partials a step may write
// d_out[t] = Im <lam_t| G |phi_t> for every member t < batch, then (apply) member t's U^† on both
// of its work states, in one launch; without apply nothing is stored (the bra-ket alone, coef may
// be null).  kind: how the rotation lowers (K_M1 with g.pauli 1 / 2, K_DIAG with 3); g: physical
// positions; coef: the FORWARD coefficients, [batch][8] in Op::m layout.  Asynchronous.
void launch_batch_adjoint_step(double2* phi, double2* lam, int n, uint64_t batch, const Generator& g, int kind,
                               const double* coef, bool apply, double* d_partials, double* d_out, hipStream_t s,
                               Timer* tm);
// One step of the backward walk (execution order: the circuit's last gate first).  pauli == 0: a
// non-parameterised gate, op = its lowered inverse; else a parameterised gate generating that
// Pauli, op = the sweep's placeholder op (kind, target, control; src = its slot).
struct BatchBackStep {
    Op op;
    int pauli = 0;
};
// The backward sweep over w.phi / w.lam (already holding phi and H phi): w.d_out[slot * batch + t]
// for every slot among `steps`, whose last entry is the first parameterised gate (bra-ket only).
// d_tab: the sweep's table, [slot][member][8].  fused_segments: runs of non-parameterised steps go
// through launch_fused and w.plans (a plan with a relayout pass is an error), else launch_op.
// QSIM_ADJOINT_FUSED=0 composes each step from the bra-ket and two launch_sweep_op calls.
void batch_adjoint_sweep(BatchGradWork& w, int n, uint64_t batch, const std::vector<BatchBackStep>& steps,
                         const double* d_tab, bool fused_segments, hipStream_t s, Timer* tm);

// Overlap matrices of batched ensembles (batch_overlap.hip; the entry points: batched.hip).  How
// out[i][j] = <a_i|b_j> (Ba x Bb members of n qubits) is cut up: tiles of 64 x 64 members — self:
// only those of the upper triangle — times chunks of K = 2^n, one work-group and one partial tile
// of scratch each.  A function of the arguments alone.
struct OverlapPlan {
    bool mfma = false;  // the matrix-core tile kernel (never for Bb == 1), else the FMA one
    uint64_t tiles_a = 0, tiles_b = 0, tiles = 0;
    uint32_t chunks = 1;
    uint64_t chunk_len = 0;      // k per chunk (K / chunks)
    uint64_t scratch_bytes = 0;  // chunks x tiles x 64 x 64 x 16
};
OverlapPlan overlap_plan(int n, uint64_t Ba, uint64_t Bb, bool self, bool mfma);
// d_out[i * Bb + j] = <a_i|b_j>, a: [Ba][2^n], b: [Bb][2^n] (self: b == a and Bb == Ba; the result
// is Hermitian bitwise with +0 imaginary parts on the diagonal).  d_partials: p.scratch_bytes.  The
// tile kernel and the reduction that adds the chunks of an entry in order.  Asynchronous.
void launch_batch_overlap(const double2* a, const double2* b, int n, uint64_t Ba, uint64_t Bb, bool self,
                          const OverlapPlan& p, double2* d_partials, double2* d_out, hipStream_t s, Timer* tm);

// RAII scope used around each launch.  Record mode: events recorded on the stream before and
// after the launch (two marker packets, ~8 us of serialisation per launch — 35 % of a 20-qubit
// circuit).  Ext mode (ext = true): the two events are handed to the launch itself through
// start() / stop() (hipExtLaunchKernel / hipExtModuleLaunchKernel), which time the dispatch
// packet with no extra packets; the launch site must pass them.
struct TimedLaunch {
    Timer* tm; int slot = -1; hipEvent_t a = nullptr, b = nullptr; double bytes; bool ext = false;
    hipStream_t stream;  // the end event goes on the stream the begin event went on
    TimedLaunch(Timer* t, const char* name, double b, hipStream_t s, bool ext = false);
    hipEvent_t start() const { return a; }  // null when profiling is off
    hipEvent_t stop() const { return b; }
    ~TimedLaunch();
};

}  // namespace qsim_hip
