/*
 * qsim_hip.h — C ABI of the MI355X (gfx950) state-vector engine.
 *
 * This is the drop-in boundary between host code (the C++17 API in
 * include/qsim/ headers, the Python ctypes mirror, or any FFI) and the
 * hand-written HIP kernels.  Plain C types only: opaque handles, pointers,
 * sizes, int status codes.  No HIP, torch or C++ types cross it.
 *
 * Amplitude layout: 2^n interleaved {double re, double im} (16 B each),
 * index bit q == qubit q (LSB-first; reference src/Gates.cu:19-25 and
 * tests/test_gates.cu:258-273 pin this convention).
 *
 * Every entry point returns QSIM_OK (0) or a QSIM_ERR_* code; the message of
 * the last failure on the calling thread is in qsim_last_error().
 *
 * Reference interfaces replaced (file:line in rylanmalarchick/cuda-quantum-simulator):
 *   StateVector ctor/alloc/init      include/StateVector.cuh:66-86, src/StateVector.cu:130-202
 *   Gates.cuh __global__ kernels     include/Gates.cuh:58-101 (launched per gate)
 *   Simulator::run / applyGate       include/Simulator.hpp:53-85, src/Simulator.cu:28-154
 *   toHost / getProbabilities        src/StateVector.cu:204-233
 *   measure (prob + collapse)        src/StateVector.cu:260-314
 *   sample                           src/Simulator.cu:164-185, src/StateVector.cu:316-342
 *   OptimizedGates applyGate1Q_opt   include/OptimizedGates.cuh:91-93
 *   BatchedSimulator                 include/NoiseModel.cuh:231-297, src/NoiseModel.cu:653-972
 *   DensityMatrix(Simulator)         include/DensityMatrix.cuh:63-224, src/DensityMatrix.cu
 *   NoisySimulator noise kernels     include/NoiseModel.cuh:139-214, src/NoiseModel.cu:115-577
 */
#ifndef QSIM_HIP_H
#define QSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSIM_ABI_VERSION 2

/* ---- status codes (mapped to the reference's exception types by the C++ layer) ---- */
enum {
    QSIM_OK = 0,
    QSIM_ERR_INVALID_ARGUMENT = 1, /* std::invalid_argument (src/StateVector.cu:135-141, :261-266) */
    QSIM_ERR_OUT_OF_RANGE = 2,     /* std::out_of_range (src/Circuit.cpp:26-31, src/NoiseModel.cu:917-919) */
    QSIM_ERR_RUNTIME = 3,          /* std::runtime_error (zero-probability measure, unknown gate) */
    QSIM_ERR_DEVICE = 4            /* std::runtime_error from a HIP/RCCL failure (CUDA_CHECK analogue) */
};

/* ---- gate types: numbering == reference enum class GateType (include/Circuit.hpp:42-59) ---- */
enum {
    QSIM_GATE_X = 0, QSIM_GATE_Y = 1, QSIM_GATE_Z = 2, QSIM_GATE_H = 3,
    QSIM_GATE_S = 4, QSIM_GATE_T = 5, QSIM_GATE_SDAG = 6, QSIM_GATE_TDAG = 7,
    QSIM_GATE_RX = 8, QSIM_GATE_RY = 9, QSIM_GATE_RZ = 10,
    QSIM_GATE_CNOT = 11, QSIM_GATE_CZ = 12, QSIM_GATE_CRY = 13, QSIM_GATE_CRZ = 14,
    QSIM_GATE_SWAP = 15, QSIM_GATE_TOFFOLI = 16,
    QSIM_GATE_COUNT = 17
};

/* One circuit operation, same meaning as the reference GateOp (include/Circuit.hpp:64-84):
 * qubits = [target] | [control, target] | [q1, q2] (SWAP) | [c1, c2, target]. */
typedef struct qsim_gate {
    int32_t type;      /* QSIM_GATE_* */
    int32_t nqubits;   /* 1, 2 or 3 */
    int32_t qubits[3];
    int32_t _pad;
    double  parameter; /* angle in radians for Rx/Ry/Rz/CRY/CRZ, else ignored */
} qsim_gate;

/* Execution flags for qsim_run / qsim_batch_run. */
enum {
    QSIM_RUN_PER_GATE = 0,   /* one kernel launch per gate (reference Simulator::run shape) */
    QSIM_RUN_FUSED = 1       /* host planner groups gates into LDS-tiled fused passes */
};

typedef struct qsim_state qsim_state; /* one 2^n state vector on one GPU + its HIP stream */
typedef struct qsim_batch qsim_batch; /* B trajectories of 2^n amplitudes (BatchedSimulator) */

/* ---- library ---- */
const char* qsim_last_error(void);
int qsim_abi_version(void);
int qsim_device_count(int* count);
/* Device of the calling thread's next objects (hipSetDevice; the reference always uses the
 * default device).  One process per GPU selects its LOCAL_RANK with this. */
int qsim_set_device(int device);
/* Name/bandwidth facts of the current device (for bench reports). name_len includes NUL. */
int qsim_device_info(int device, char* name, size_t name_len, int* cu_count, size_t* total_mem);

/* ---- state vector lifecycle (StateVector.cuh:66-86) ---- */
/* 1 <= n_qubits <= QSIM_MAX_QUBITS_SINGLE (30, Constants.hpp:68), else QSIM_ERR_INVALID_ARGUMENT.
 * The new state is |0...0> (src/StateVector.cu:130-143). */
int qsim_state_create(int n_qubits, qsim_state** out);
int qsim_state_create_on(int device, int n_qubits, qsim_state** out);
int qsim_state_destroy(qsim_state* s);
int qsim_state_num_qubits(const qsim_state* s, int* n);
/* Raw device address of amplitude 0 (StateVector::devicePtr, StateVector.cuh:89-90). */
int qsim_state_device_ptr(qsim_state* s, void** dptr);
/* hipStream_t of the state, as an opaque pointer. */
int qsim_state_stream(qsim_state* s, void** stream);
int qsim_state_init_zero(qsim_state* s);                      /* initializeZero */
int qsim_state_init_basis(qsim_state* s, uint64_t basis_idx);  /* initializeBasis; >= 2^n -> INVALID_ARGUMENT */
int qsim_state_sync(qsim_state* s);

/* ---- gate application ---- */
/* Validate + apply one gate (Simulator::applyGate, src/Simulator.cu:38-46).  Asynchronous. */
int qsim_apply_gate(qsim_state* s, const qsim_gate* g);
/* Whole circuit (Simulator::run, src/Simulator.cu:28-36).  flags = QSIM_RUN_*.  Asynchronous. */
int qsim_run(qsim_state* s, const qsim_gate* gates, size_t count, int flags);
/* General 2x2 unitary [[a,b],[c,d]] on `target`, m = {a.re,a.im,b.re,b.im,c.re,c.im,d.re,d.im}
 * (applyGate1Q_opt, include/OptimizedGates.cuh:91-93), optionally controlled on `controls`. */
int qsim_apply_matrix1q(qsim_state* s, int target, const double m[8],
                        const int* controls, int n_controls);
/* General 4x4 matrix on (q0, q1), m = 32 doubles, row-major over the index (bit q1 << 1) | bit q0,
 * optionally controlled (the k = 2 applyMatrix of SURVEY §8(f) rank 3).  Asynchronous. */
int qsim_apply_matrix2q(qsim_state* s, int q0, int q1, const double m[32], const int* controls,
                        int n_controls);
/* General 2^k x 2^k complex matrix on k <= 8 target qubits (generalises
 * applyGate1Q_opt, src/OptimizedGates.cu:165-183, and cuStateVec's applyMatrix used by
 * benchmarks/benchmark_custatevec.cu:131-135): m row-major, re/im interleaved, matrix-index bit j
 * = bit targets[j] of the amplitude index; applied on the control == 1 subspace of `controls`.
 * Asynchronous; synchronises before returning (the matrix is staged in device scratch). */
int qsim_apply_matrix(qsim_state* s, const int* targets, int k, const double* m,
                      const int* controls, int n_controls);
/* Named dispatchers of the reference (src/OptimizedGates.cu:388-413, declared in
 * include/OptimizedGates.cuh:161-166) on a raw device pointer and stream, routed to this build's
 * per-gate kernels; applyGate1Q_opt's general 2x2 as qsim_apply_matrix1q_raw. */
int qsim_apply_hadamard_optimized(void* dstate, int n_qubits, int target, void* stream);
int qsim_apply_cnot_optimized(void* dstate, int n_qubits, int control, int target, void* stream);
int qsim_apply_matrix1q_raw(void* dstate, int n_qubits, int target, const double m[8], void* stream);
/* applyFusedSingleQubitLayer (src/OptimizedGates.cu:344-382): for every qubit q in `active`,
 * amplitudes with bit q = 0 are scaled by gate_params[q*4+0] and those with bit q = 1 by
 * gate_params[q*4+3] (complex, re/im interleaved: 8 doubles per qubit).  Runs as fused passes. */
int qsim_apply_diagonal_layer(qsim_state* s, const double* gate_params, uint64_t active);
/* Host-only introspection of the fused-pass planner (no device needed).  Writes, for each gate
 * in execution order, its index in `gates` (order[count]) and its pass number (pass_of[count],
 * -1 for gates executed per-gate), and the number of passes.  Gates are only reordered past
 * gates on disjoint qubits. */
int qsim_plan_fused(int n_qubits, const qsim_gate* gates, size_t count, int hmax,
                    int32_t* order, int32_t* pass_of, int32_t* n_passes);
/* Host-only, read-only: the stages of the plan a fused qsim_run of this gate list would execute on
 * a state of n_qubits under the process settings in force (tile height, stage width, tile-constant
 * controls, QSIM_TILE_R0 and the planner pins), read out of that plan; relayout != 0: the relayout
 * plan of a first run instead (QSIM_ERR_RUNTIME when none exists).  Three tables of int32 records;
 * each is filled up to its capacity in records (the buffer may be null) and its full count is
 * returned, so a caller may ask for the counts first.
 *   ops, 16 per executed tile op, in execution order (a gate run per-gate gives one record too):
 *     0 source gate index (-1: the second and third controlled-X of a lowered SWAP), 1 pass,
 *     2 stage within the pass (-1: unstaged tile or per-gate), 3 stage position (0 first: straight
 *     from the HBM loads, 1 middle: LDS on both sides, 2 last: straight into the stores, 3 only),
 *     4 kind (0 2x2, 1 diagonal, 2 SWAP), 5 sub-kind as the kernel dispatches it (an H beyond the
 *     pass's unnormalised-butterfly cap is relabelled general), 6 p0 (register bit of the target,
 *     -1: a thread bit), 7 b0 and 8 b1 (tile bits of the targets; qubits for a per-gate op),
 *     9 controls inside the tile (tile bits), 10 cm_reg (those on register bits, register space),
 *     11 cm_thr (those on thread bits, tile space), 12 / 13 low / high word of cm_out (controls
 *     outside the tile, physical positions), 14 d0_one, 15 zero (qsim_dm_plan_stage_info: origin).
 *   passes, 24 per pass: 0 single (per-gate fallback), 1 h, 2 r0, 3 rb (0: unstaged), 4 hu_count,
 *     5 relayout, 6 stages, 7 op records, 8 / 9 LDS round trips under the fixed / a searched
 *     swizzle, 10 tile bits above the run, 11.. their physical positions (hpos).
 *   stages, 8 per stage: 0 pass, 1 stage, 2 position (as above), 3 register-bit mask (tile bits),
 *     4 ops, 5 the LDS round trip after it (0 none, 1 fixed swizzle, 2 searched), 6 tscatter, 7 zero. */
int qsim_plan_stage_info(int n_qubits, const qsim_gate* gates, size_t count, int relayout, int32_t* ops,
                         size_t op_cap, size_t* n_ops, int32_t* passes, size_t pass_cap, size_t* n_passes,
                         int32_t* stages, size_t stage_cap, size_t* n_stages);
/* Circuit-specialised pass kernels (hipRTC, no reference counterpart: the reference launches one
 * fixed kernel per gate, src/Simulator.cu:38-154).  mode 0 = off, 1 = compile in the background
 * on a plan's first run and switch to the compiled kernels when ready (default), 2 = compile on
 * the first run before launching; states below min_qubits always use the pass interpreter.
 * A negative argument leaves that setting unchanged (env defaults: QSIM_JIT, QSIM_JIT_MIN_QUBITS). */
int qsim_set_jit(int mode, int min_qubits);
/* Stop the background compiler: queued compiles are dropped (their plans stay on the
 * interpreter) and the one in progress is waited for.  Called at exit (the Python package
 * registers it with atexit; the library registers it after its first compile) so no compile runs
 * while the compiler's static state is destroyed; later background requests are refused. */
int qsim_jit_shutdown(void);
/* Layout-aware qubit relabeling (no reference counterpart; relabel.hip).  A fused pass's speed
 * depends on the physical qubit positions its tile spans (the memory system's address mapping).
 * On the first fused qsim_run of a state that holds a computational basis state (after create /
 * init), the engine may choose a logical -> physical qubit permutation for the circuit's plan and
 * keep running the state under it; every entry that reads or writes amplitudes by index first
 * restores the identity layout with a fused SWAP network, so results are unchanged.  mode 0 off,
 * 1 on (default, QSIM_RELABEL); states below min_qubits (default 26, QSIM_RELABEL_MIN_QUBITS)
 * are never relabeled; negative arguments leave a setting unchanged. */
int qsim_set_relabel(int mode, int min_qubits);
int qsim_state_perm(qsim_state* s, int32_t* perm);  /* current logical -> physical map, n entries */
/* First-run layout decision of a state (no reference counterpart): the tile height its fused
 * runs plan at, whether the layout was chosen by timing candidates on the device (layout and
 * cross-height calibration), whether the qubits are currently relabeled. */
int qsim_state_layout_info(qsim_state* s, int* tile_h, int* calibrated, int* relabeled);
/* Bring a relabeled state back to the identity qubit layout now (the fused SWAP network every
 * index-based reader runs first); a no-op when it is not relabeled. */
int qsim_state_restore_layout(qsim_state* s);
/* Whether the state's first fused run chose a relayout plan (no reference counterpart): every
 * 12-qubit tile pass stores its tile under the next pass's qubit layout, so each pass picks all
 * of its tile qubits except the four of the contiguous run (fewer passes); the last pass restores
 * the first layout.  QSIM_RELAYOUT=0 disables them (QSIM_RELAYOUT_MIN_QUBITS, default 20).
 * Relayout passes write out of place into a second 2^n buffer: a first run only considers them
 * when the device has room for it (otherwise the fixed-layout plan runs in place), and the buffer
 * is freed again unless the run keeps a relayout plan (qsim_state_memory_bytes). */
int qsim_state_relayout(qsim_state* s, int* relayout);
/* Relayout plans on (mode 1: when they need fewer passes, or win the device timing with
 * calibration) / off (0) / forced (2: whenever one exists — tests) for first runs from now on, for
 * states of at least min_qubits qubits; they permute qubit labels, so relabeling mode 0
 * (qsim_set_relabel / QSIM_RELABEL=0) turns them off too, whatever the state's size; negative
 * arguments leave a setting unchanged. */
int qsim_set_relayout(int mode, int min_qubits);
/* Host-only: compile the relayout plan's pass kernels with hipRTC for gfx950 (no GPU needed);
 * code_bytes: the code object's size.  QSIM_ERR_RUNTIME when there is no relayout plan. */
int qsim_jit_build_relayout(int n_qubits, const qsim_gate* gates, size_t count, size_t* code_bytes);
/* Host-only check of the planners' index math (tests; no GPU): plan the circuit (mode 0: the
 * fixed-layout planner under the identity labels; 1: the relayout planner) and execute the plan
 * on the host exactly as the staged pass kernels address the state (register stages, LDS slots,
 * store layouts).  amps: 2^n interleaved re/im in logical qubit order, updated in place.
 * perm (n entries, may be null): the layout the plan starts and ends in (logical -> physical);
 * passes: the plan's pass count.  QSIM_ERR_RUNTIME when mode 1 finds no relayout plan.
 * mode 2: the one-pass identity-layout restore instead (gates unused): amps holds the state in
 * the physical order of layout perm (input), and is returned in logical order. */
int qsim_plan_exec_host(int n_qubits, const qsim_gate* gates, size_t count, int mode, double* amps,
                        int32_t* perm, int* passes);
/* Host-only: the relayout plan of a circuit (what qsim_run would consider): its first/last layout
 * (perm, n entries, may be null), pass count and predicted time in microseconds (layout model);
 * *passes = 0 when none exists. */
int qsim_plan_relayout(int n_qubits, const qsim_gate* gates, size_t count, int32_t* perm, int* passes,
                       double* predicted_us);
/* Run sharing (no reference counterpart).  A caller that runs the same circuit again and again
 * before reading the state pays, per run, the edge effects a single plan cannot share.  When a
 * fused qsim_run receives exactly the gate list of the previous fused qsim_run on the state (the
 * lists are compared, not a hash), nothing is pending, the state's device pointer was not handed
 * out and relayout plans are allowed for it, that call still runs its own plan whole and then
 * arms a cycle: `copies` consecutive copies of the circuit are planned as ONE relayout plan (kept
 * only if it needs fewer passes than `copies` single runs; memoised per circuit) and the state is
 * brought to that plan's start layout by one gate-free pass.  Call j = 1..copies of the cycle then
 * launches the longest prefix of the joint plan's not-yet-launched passes whose gates all belong
 * to copies <= j; requested gates in later passes stay PENDING.  After call `copies` every pass
 * has run, nothing is pending, and the next identical call starts the next cycle on the same
 * plan with no planning and no upload.
 * Contract: gates are applied no later than the next reader.  Every entry that reads or writes
 * amplitudes (readout, sampling, measurement, expectation values, gradients, apply_gate / matrix
 * entries, noise / density entries on the state, restore_layout, device_ptr, a qsim_run with
 * another gate list or in per-gate mode) first flushes: the pending gates are lowered under the
 * layout the state is in and run, in circuit order, as an ordinary fused plan, which ends the
 * cycle.  qsim_state_init_zero / init_basis / from_host / destroy discard pending gates.
 * qsim_state_sync waits for launched work and does not flush; qsim_state_last_run (the passes the
 * last qsim_run call launched), layout_info, relayout, perm and the profile getters do not flush.
 * Cost of arming: joint planning (once per circuit), under inline compilation the joint kernels'
 * compile, and one extra pass over the state; a reader that ends a cycle early also pays the plan
 * of the pending gates.  A reader between two identical runs prevents arming, and a state whose
 * cycles are ended before one whole cycle has run backs off: after k such cycles in a row it lets
 * 2^k - 1 (at most 63) identical repeats run unshared before it arms again.  A failure while
 * arming (planning, compile, launch) leaves the run that triggered it successful and unshared.
 * mode 0 off (every run executes its own plan, as before), 1 on (default, QSIM_RUN_SHARE) for
 * states from the relayout size threshold; copies >= 2 (QSIM_RUN_SHARE_COPIES), or 0 (default):
 * 4 below 26 qubits and 8 from there, where a pass takes milliseconds and the longer cycle's
 * arming (joint planning: seconds at 30 qubits; about 21 kernels to compile instead of 12) pays
 * off; negative arguments leave a setting unchanged.  The joint plan is the better of the tail
 * rule's (below) and a sweep of position caps (the pass at position k of a plan aimed at P passes
 * takes gates of the copies below min(copies, k * copies / P + 1)): the fewest passes, then the
 * smallest largest call before the last.  The last call of a cycle launches what is left, up to
 * about twice a single run's passes.  QSIM_RUN_SHARE_TAIL (per cent, default 50, read
 * once): the share of a copy's gates that must have run before a joint pass may also take gates
 * of the next copy (100: from the start; fewer passes, but the first call of a cycle launches
 * none). */
int qsim_set_run_share(int mode, int copies);
/* Host-only view of run sharing (tests; no GPU): plays `calls` identical fused runs of the
 * circuit through the engine's cycle bookkeeping and executes every launched pass on the host
 * with the staged kernels' index math (qsim_plan_exec_host), flushes at the end and returns the
 * state in logical order.  amps: 2^n interleaved re/im, logical order, updated in place.
 * passes_per_call / pending_per_call (calls entries each, may be null): the circuit passes each
 * call launched and the gates pending after it.  copies <= 0: the configured count. */
int qsim_plan_share_host(int n_qubits, const qsim_gate* gates, size_t count, int copies, int calls,
                         double* amps, int32_t* passes_per_call, int32_t* pending_per_call);
/* Host-only: the joint plan a cycle of `copies` runs would execute: its pass count (0: no cycle
 * pays), the single-run plan's pass count, and per joint pass (up to cap entries, may be null) the
 * highest copy (0-based) the pass holds a gate of. */
int qsim_plan_share_info(int n_qubits, const qsim_gate* gates, size_t count, int copies, int* joint_passes,
                         int* single_passes, int32_t* pass_copy, size_t cap);
/* Layout calibration (with QSIM_JIT = 2, from min_qubits; defaults QSIM_RELABEL_CALIBRATE = 1,
 * QSIM_RELABEL_CALIBRATE_MIN_QUBITS = 26): the first run of a basis state times the layout
 * model's choice and two alternatives with their compiled pass kernels (the basis state is
 * restored after each) and keeps the fastest.  Negative arguments leave a setting unchanged. */
int qsim_set_calibrate(int mode, int min_qubits);
/* Tile height of fused passes planned from now on (no reference counterpart): a tile spans 6 + h
 * qubits (64 << h amplitudes in LDS).  h = 6 (12 qubits, 64 KiB, two workgroups per CU) is the
 * default; h = 7 (13 qubits, 128 KiB, one 512-thread workgroup per CU, persistent pipelined
 * kernels) needs fewer passes on some circuits but streams slower.  h < 0 restores
 * the default (QSIM_TILE_HMAX); plans already cached for a circuit keep their height. */
int qsim_set_tile_height(int h);
/* Tile-constant controls (no reference counterpart; default on, QSIM_TILE_CTRL_OUT): the fused
 * planners require only an op's TARGETS to be tile qubits; a control outside the tile is fixed for
 * the whole tile, so the op runs on the tiles where it reads 1 (a uniform branch on the tile's
 * base address) — a CNOT costs one tile slot, not two.  mode 0 off, 1 on, negative: unchanged;
 * plans made from now on.  Batched Pauli-frame passes always keep every control a tile qubit. */
int qsim_set_tile_ctrl_out(int mode);
/* Register bits per stage of 13-qubit tiles: 4 (16 amplitudes per thread, 512-thread workgroups,
 * the default) or 3 (8 per thread, 1024 threads); anything else restores QSIM_TILE_RB7. */
int qsim_set_tile_rb7(int rb);
/* Host-only: the permutation the engine would choose for this circuit (identity when none pays)
 * and the predicted pass-layout cost (microseconds, summed over the plan's passes) before/after. */
int qsim_plan_relabel(int n_qubits, const qsim_gate* gates, size_t count, int32_t* perm,
                      double* cost_before_us, double* cost_after_us);
/* Host-only: the generated source of a circuit's plan (len = its size; buf gets up to cap-1
 * bytes + NUL), and a hipRTC compile of it for gfx950 (code_bytes = code-object size). */
int qsim_jit_source(int n_qubits, const qsim_gate* gates, size_t count, char* buf, size_t cap,
                    size_t* len);
int qsim_jit_build(int n_qubits, const qsim_gate* gates, size_t count, size_t* code_bytes);
/* Kernel-level entry on a raw device pointer (the reference's Gates.cuh kernels, launched by
 * tests/test_statevector.cu:151-159).  stream may be NULL (the null stream). */
int qsim_apply_gate_raw(void* dstate, int n_qubits, const qsim_gate* g, void* stream);

/* ---- readout (each synchronizes the state's stream) ---- */
int qsim_state_to_host(qsim_state* s, double* dst);            /* 2*2^n doubles */
int qsim_state_from_host(qsim_state* s, const double* src);    /* 2*2^n doubles */
int qsim_state_probabilities(qsim_state* s, double* dst);      /* 2^n doubles, |a_i|^2 */
int qsim_state_total_probability(qsim_state* s, double* out);  /* device wave64 reduction */
/* P(index bit `bit` == 0), device reduction (qubitProbabilityKernel src/StateVector.cu:83-99
 * + host sum :280-287).  `bit` is an index bit: the C++ layer maps the reference's
 * big-endian measure(q) to bit n-1-q. */
int qsim_state_prob_bit_zero(qsim_state* s, int bit, double* out);
/* Zero amplitudes whose `bit` != result, scale the rest (collapseStateKernel :105-124). */
int qsim_state_collapse(qsim_state* s, int bit, int result, double scale);
/* Draw `shots` basis indices from |a|^2 with uniforms u[i] in [0,1) supplied by the caller
 * (host RNG keeps the reference's mt19937 stream): device CDF + binary search. */
int qsim_state_sample(qsim_state* s, const double* uniforms, int shots, int64_t* out);
/* max_i max(|Re a_i - Re b_i|, |Im a_i - Im b_i|) of two states of the same size on the same
 * device, both read in the identity qubit layout, computed on the device (no reference
 * counterpart: tests/test_gpu_cpu_equivalence.cu:26 compares per component on the host, which at
 * 30 qubits would copy 32 GiB).  NaN when any difference is NaN. */
int qsim_state_max_abs_diff(qsim_state* a, qsim_state* b, double* out);
/* Device bytes the state owns now: the 2^n x 16 B amplitudes, the second buffer a relayout plan
 * writes into (same size; allocated on a first run only when the device has room for it, freed
 * when the run does not keep a relayout plan), reduction and plan buffers, readout scratch. */
int qsim_state_memory_bytes(qsim_state* s, uint64_t* bytes);

/* ---- Pauli-sum expectation values (no reference counterpart: the reference has no observable
 * API, a caller reads the amplitudes back) ----
 * One term c * P of H = sum_t c_t P_t.  Bit q of x_mask: the factor on LOGICAL qubit q is X or Y;
 * bit q of z_mask: it is Z or Y (Y sets both; neither: identity). */
typedef struct qsim_pauli_term {
    uint64_t x_mask, z_mask;
    double coeff;
} qsim_pauli_term;
/* <psi|H|psi> by device reductions over the state where it lies: the masks are mapped through the
 * state's current qubit layout on the host, so the layout (qsim_state_perm), a relayout plan's
 * current buffer and the amplitudes are left exactly as they are.  Terms are grouped by x mask,
 * one streaming read of the state per group (every Z/I-only term shares one); partial sums are
 * added in a fixed order, so the value is bitwise reproducible.  A mask bit >= n ->
 * QSIM_ERR_OUT_OF_RANGE; count == 0 -> 0.0 with no launch.  Synchronises.  A group of 16 or more
 * terms evaluates the z bits above a work-group's 256-pair run once per run and term, the low
 * bits per amplitude (QSIM_EXPECT_SPLIT=0: the whole sign per amplitude; the same weights added in
 * the same order, so the same value). */
int qsim_state_expectation(qsim_state* s, const qsim_pauli_term* terms, size_t count, double* out);
/* Host-only (no GPU): the passes over the state (distinct physical x masks after duplicate
 * strings are merged and zero coefficients dropped) and the kernel launches (a pass of more terms
 * than one launch's table holds takes several) the lowering makes for these terms under the qubit
 * layout perm (logical -> physical, n entries; null: identity). */
int qsim_expectation_plan(int n_qubits, const qsim_pauli_term* terms, size_t count, const int32_t* perm,
                          int* passes, int* launches);

/* ---- marginal probabilities and reduced density matrices of a subset of qubits (no reference
 * counterpart: a caller copies 2^n probabilities to the host and reduces them there) ----
 * qubits: k distinct LOGICAL qubits in any order, in the convention of the gates and of
 * qsim_pauli_term: qubit q is index bit q (not the big-endian mapping of the C++ measure(q)).
 * Bit j of an output index is qubit qubits[j], so the order of the list decides the bit order.
 * Both readers work like qsim_state_expectation: pending gates of a run-sharing cycle are flushed,
 * the qubits are mapped through the state's current layout on the host, and ONE streaming read of
 * the state (16 B per amplitude) is made where it lies; the layout (qsim_state_perm), a relayout
 * plan's current buffer and the amplitudes are left exactly as they are.  Partial sums are added
 * in a fixed order (no floating-point atomics): bitwise reproducible.  Both synchronise.
 * A duplicate qubit, k above the cap (or above n), null out, a null handle, null qubits with
 * k > 0 -> QSIM_ERR_INVALID_ARGUMENT; a qubit < 0 or >= n -> QSIM_ERR_OUT_OF_RANGE.
 *
 * out[m] = sum of |psi_i|^2 over all i whose bit qubits[j] equals bit j of m, m < 2^k;
 * 0 <= k <= min(n, 20); k == 0: out[0] = the total probability.  Device scratch for partial sums
 * stays <= 64 MiB for every qubit choice. */
int qsim_state_marginal_probabilities(qsim_state* s, const int32_t* qubits, int k, double* out);
/* out = rho_A, 2^k x 2^k row-major, interleaved re/im (2 * 4^k doubles), 0 <= k <= min(n, 6):
 * rho_A[a][a'] = sum_b psi(a, b) conj(psi(a', b)), a over the listed qubits, b over the others.
 * The upper triangle is mirrored and the diagonal is real, so rho_A equals its conjugate
 * transpose bitwise; the diagonal is the marginal.  k == 0: the 1 x 1 matrix holding the norm. */
int qsim_state_reduced_density_matrix(qsim_state* s, const int32_t* qubits, int k, double* out);
/* Host-only (no GPU): how the lowering splits the work for these qubits under the layout perm
 * (logical -> physical, n entries; null: identity); rdm != 0: for the matrix.  info[0] = k_lo,
 * selected physical positions below the work-group's contiguous run of 2^min(n, 12) amplitudes;
 * [1] = k_hi, those above; [2] = slices of the unselected high positions (matrix: = [3]);
 * [3] = work-groups of the first kernel; [4], [5] = scratch bytes of the partial sums, low and high
 * word; [6] = kernel launches; [7] reserved (0).  The argument checks and error codes of the two
 * entries above; a perm that is no permutation -> QSIM_ERR_INVALID_ARGUMENT. */
int qsim_marginal_plan(int n_qubits, const int32_t* qubits, int k, const int32_t* perm, int rdm,
                       int32_t info[8]);

/* ---- adjoint-method gradients of <psi|H|psi> (no reference counterpart) ----
 * dst = H src out of place, one streaming pass per group of terms sharing an x mask (same qubit
 * count and device; src == dst -> QSIM_ERR_INVALID_ARGUMENT).  dst takes src's qubit layout.
 * A mask bit >= n -> QSIM_ERR_OUT_OF_RANGE.  Synchronises. */
int qsim_state_apply_pauli_sum(qsim_state* src, qsim_state* dst, const qsim_pauli_term* terms, size_t count);
/* out[0] + i out[1] = <a|b>, both read in one common layout (their own when the two layouts are
 * equal, else both are restored to the identity first); a == b gives the norm.  Partial sums are
 * added in a fixed order: bitwise reproducible.  Synchronises. */
int qsim_state_inner_product(qsim_state* a, qsim_state* b, double out[2]);
/* Host-only: the inverse of one gate (self-inverse types unchanged, S <-> Sdag, T <-> Tdag,
 * rotations with the angle negated).  An unknown type -> QSIM_ERR_RUNTIME. */
int qsim_gate_inverse(const qsim_gate* g, qsim_gate* out);
/* Host-only: what qsim_state_gradient would do for this circuit and observable: the parameterised
 * gates (Rx, Ry, Rz, CRY, CRZ), the runs of non-parameterised gates the backward sweep inverts
 * (those after the first parameterised gate; the gates before it are never undone), and the
 * passes over the state of the Pauli-sum apply.  Errors as qsim_state_gradient. */
int qsim_gradient_plan(int n_qubits, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                       size_t nterms, int* n_params, int* n_segments, int* apply_passes);
/* The state holds |psi0> (whatever it holds now).  Runs the circuit as qsim_run(s, gates, count,
 * flags) would, then *value = <psi|H|psi> and grad[k] = dE/d(parameter of gate k) for k < count
 * (0.0 for a gate without a parameter), by the adjoint method: one backward sweep over two 2^n
 * work states (a copy of the state and H times it), one pass over both per parameterised gate,
 * instead of the two circuit runs per parameter of a parameter shift.  After the
 * call the state holds U|psi0> exactly as qsim_run alone leaves it (amplitudes, qubit layout,
 * relayout buffer); the sweep never writes to it.  The work states stay on the state between
 * calls (counted by qsim_state_memory_bytes) until qsim_state_gradient_release or
 * qsim_state_destroy; if they cannot be allocated: QSIM_ERR_DEVICE, the state holding U|psi0>.
 * A parameterised step is one fused launch (bra-ket + U^dagger of both work states);
 * QSIM_ADJOINT_FUSED=0 (read at every call) composes it from a reduction and two per-gate
 * launches.  Runs of other gates are inverted as fused passes or per gate, as flags says.
 * count == 0: *value = <H> of the state as it is; nterms == 0: *value = 0, all-zero gradient, no
 * sweep.  Null pointers -> QSIM_ERR_INVALID_ARGUMENT, a mask bit >= n -> QSIM_ERR_OUT_OF_RANGE,
 * a bad gate -> the code of qsim_run.  Bitwise reproducible.  Synchronises. */
int qsim_state_gradient(qsim_state* s, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                        size_t nterms, int flags, double* value, double* grad);
int qsim_state_gradient_release(qsim_state* s); /* free the gradient work buffers now */

/* ---- Pauli-string rotations exp(-i theta/2 P) and their adjoint gradients (no reference
 * counterpart) ----
 * A rotation is a qsim_pauli_term whose coeff is the angle theta in radians; a sequence is an array
 * of them in application order.  Whatever its weight, a rotation with an X or Y factor is ONE
 * streaming pass over the state (amplitude i pairs with i ^ x_mask); a maximal run of consecutive
 * Z/I-only rotations (they commute; the identity string, a global phase, included) is one pass,
 * one kernel launch per 256 rotations of the run.  Nothing else is reordered or merged.
 * Behaves as qsim_apply_gate: pending gates of a run-sharing cycle are flushed first, the masks
 * are mapped through the state's current qubit layout on the host, the layout is neither restored
 * nor re-decided, and the figures of the last fused run stay.  Asynchronous.  count == 0 launches
 * nothing.  A mask bit >= n anywhere in the sequence -> QSIM_ERR_OUT_OF_RANGE before the first
 * launch; null rots with count > 0 -> QSIM_ERR_INVALID_ARGUMENT.  QSIM_PAULI_BLOCKS (1..65536,
 * default 65536, read at every call) caps the work-groups of the two streaming kernels; the
 * amplitudes do not depend on it. */
int qsim_state_apply_pauli_rotations(qsim_state* s, const qsim_pauli_term* rots, size_t count);
/* Host-only (no GPU): the passes over the state and the kernel launches the call above makes for
 * this sequence under the qubit layout perm (logical -> physical, n entries; null: identity).
 * The same error codes; a perm that is no permutation -> QSIM_ERR_INVALID_ARGUMENT. */
int qsim_pauli_rotation_plan(int n_qubits, const qsim_pauli_term* rots, size_t count, const int32_t* perm,
                             int* passes, int* launches);
/* Applies the sequence to the state as qsim_state_apply_pauli_rotations does, then
 * *value = <psi|H|psi> and grad[k] = dE/dtheta_k for k < count, by the adjoint method: one backward
 * sweep over the two work states of qsim_state_gradient (the same buffers, counted by
 * qsim_state_memory_bytes, freed by qsim_state_gradient_release), one fused launch per rotation
 * (Im <lambda|P|phi>, then exp(+i theta/2 P) on both work states: 64 B per amplitude); the last
 * step of the sweep, the sequence's first rotation, is the bra-ket alone.  Every rotation takes
 * its own step: Z-only runs are not merged in the sweep.  The sweep never writes the state: it
 * ends exactly as qsim_state_apply_pauli_rotations alone leaves it.  nterms == 0 or H == 0:
 * *value = 0, all-zero gradient, no sweep; count == 0: *value = <H> of the state as it is.  A
 * parameter shared between rotations is the caller's chain rule over grad.  Error codes and the
 * out-of-memory behaviour are those of qsim_state_gradient (every argument is checked before the
 * sequence is applied).  Bitwise reproducible.  Synchronises. */
int qsim_state_pauli_gradient(qsim_state* s, const qsim_pauli_term* rots, size_t count,
                              const qsim_pauli_term* terms, size_t nterms, double* value, double* grad);
/* Host-only: what qsim_state_pauli_gradient would do under the layout perm (null: identity): the
 * steps of the backward sweep (count; 0 when H == 0) and the passes over the state of the
 * Pauli-sum apply.  The same error codes. */
int qsim_pauli_gradient_plan(int n_qubits, const qsim_pauli_term* rots, size_t count,
                             const qsim_pauli_term* terms, size_t nterms, const int32_t* perm, int* steps,
                             int* apply_passes);

/* ---- timing (bench / profiling) ---- */
/* Enable per-launch HIP-event timing on the state's stream; kernels are attributed by name. */
int qsim_state_profile(qsim_state* s, int enable);
/* Number of distinct kernel names timed so far, and per-name stats (ms totals, launch counts). */
int qsim_state_profile_count(qsim_state* s, int* n);
int qsim_state_profile_get(qsim_state* s, int i, char* name, size_t name_len,
                           double* total_ms, int64_t* launches, double* alg_bytes);
int qsim_state_profile_reset(qsim_state* s);
/* Introspection of the last fused qsim_run on this state: tile passes planned and how many ran
 * as circuit-specialised (hipRTC) kernels rather than the pass interpreter. */
int qsim_state_last_run(qsim_state* s, int* passes, int* jit_passes);

/* ---- batched trajectories (BatchedSimulator, include/NoiseModel.cuh:231-297) ---- */
/* Noise channel on one qubit, NoiseType numbering == reference enum (NoiseModel.cuh:49-56). */
typedef struct qsim_noise_channel {
    int32_t type;   /* 0 Depolarizing, 1 AmplitudeDamping, 2 PhaseDamping, 3 BitFlip, 4 PhaseFlip, 5 BitPhaseFlip */
    int32_t qubit;
    double  probability;
} qsim_noise_channel;

int qsim_batch_create(int n_qubits, int batch_size, qsim_batch** out);
int qsim_batch_destroy(qsim_batch* b);
int qsim_batch_reset(qsim_batch* b);
int qsim_batch_set_seed(qsim_batch* b, uint64_t seed);
/* Trajectory sharding (SURVEY §8(e) "BatchedSimulator shards trivially by trajectory"; no
 * reference counterpart — the reference runs every trajectory on one GPU): this object's B
 * trajectories are trajectories [first, first + B) of a larger ensemble.  Noise draws are keyed
 * by the global trajectory index (both noise processes), so G objects with offsets 0, B, 2B, ...
 * and the same seed hold exactly the trajectories one object of G*B trajectories would. */
int qsim_batch_set_trajectory_offset(qsim_batch* b, uint64_t first);
/* Apply the circuit to every trajectory; after each gate apply every channel (reference
 * BatchedSimulator::run, src/NoiseModel.cu:815-831).  Gate semantics follow
 * src/NoiseModel.cu:717-801 when flags has QSIM_BATCH_REFERENCE_GATESET, else the full gate set.
 * For n >= 10 the gates run as fused tile passes with the noise carried as per-trajectory Pauli
 * frames (same draws, same trajectories); QSIM_BATCH_PER_GATE forces one kernel per gate plus
 * one Pauli pass per noisy step (the reference's structure). */
enum { QSIM_BATCH_FULL_GATESET = 0, QSIM_BATCH_REFERENCE_GATESET = 1, QSIM_BATCH_PER_GATE = 2,
       QSIM_BATCH_REFERENCE_NOISE = 4 };
/* QSIM_BATCH_REFERENCE_NOISE: the reference's noise process instead of the physical channel —
 * after every gate, one pass per Depolarizing channel entry (other types are ignored, as the
 * reference's batched mode does) over all B x 2^(n-1) amplitude pairs; each pair draws its own
 * uniform (float, compared with the double probability) and below p picks X/Y/Z at float
 * thresholds 1/3, 2/3 with a second draw, applied to that pair only
 * (applyBatchedDepolarizingKernel, src/NoiseModel.cu:834-892).  The draws come from the counter
 * hash of qsim_noise_apply keyed by (seed, pass counter, global pair index t*2^(n-1) + pair). */
int qsim_batch_run(qsim_batch* b, const qsim_gate* gates, size_t count,
                   const qsim_noise_channel* channels, size_t n_channels, int flags);
/* Parameter sweep (no reference counterpart): one circuit, one angle set per member.  P = number
 * of parameterised gates (Rx, Ry, Rz, CRY, CRZ) of the list, in list order ("slots").  angles is
 * member-major, B x P: member t applies its k-th parameterised gate with angles[t * P + k]; the
 * `parameter` field of those gates is ignored.  Every other gate is applied to all members as
 * qsim_batch_run applies it.
 * Noise-free: no channel list; carried Pauli frames of an earlier noisy run are applied to the
 * stored vectors first, as a reader of the state does; trajectory offset, seed and step counter are
 * neither read nor advanced.  Starts from whatever each member holds (|0..0> after reset, or the
 * result of an earlier run or sweep).  Asynchronous, like qsim_batch_run.  Bitwise reproducible.
 * flags: 0 or QSIM_BATCH_PER_GATE; QSIM_BATCH_REFERENCE_GATESET / QSIM_BATCH_REFERENCE_NOISE ->
 * QSIM_ERR_INVALID_ARGUMENT (the reference gate set has no rotations to sweep).  n_slots != P, or
 * null angles with P > 0, or an angle that is not finite -> QSIM_ERR_INVALID_ARGUMENT.  Gates are
 * validated as qsim_batch_run validates them, before the first launch.  P == 0 behaves exactly as
 * qsim_batch_run(b, gates, count, NULL, 0, flags) (angles may be null); count == 0 launches
 * nothing.
 * For n >= 10 (without QSIM_BATCH_PER_GATE, QSIM_BATCH_FUSED=0) the circuit runs as the fused tile
 * passes of qsim_batch_run; a pass that holds a parameterised gate always runs the pass
 * interpreter, which reads that gate's 2x2 per member from a coefficient table, the others run
 * what they run in qsim_batch_run (circuit-specialised kernels included).  Otherwise one launch
 * per gate over all members.  The plan and the qubit layout are made for the list with every
 * parameterised angle replaced by one fixed placeholder: a second sweep of the same circuit with
 * new angles plans nothing.
 * The coefficient table (64 bytes per slot and member: the gate's eight matrix doubles, lowered on
 * the host exactly as qsim_run lowers the rotation) lives on the batch object, grows on demand and
 * is freed with it; it is counted by no memory figure.  If it cannot be allocated:
 * QSIM_ERR_DEVICE, the states untouched. */
int qsim_batch_run_sweep(qsim_batch* b, const qsim_gate* gates, size_t count,
                         const double* angles, size_t n_slots, int flags);
/* Host-only (no GPU): what the call above would do for a batch of `batch` members, planned under
 * the identity layout and the tile height in force.  info[0] = P; [1] = tile passes; [2] = passes
 * holding at least one member-dependent op (always the interpreter); [3] = launches of the
 * per-gate path (one per gate); [4], [5] = table bytes (64 * batch * P), low and high word;
 * [6] = 1 if the fused path is taken (n >= 10, no QSIM_BATCH_PER_GATE), else 0 and [1] = [2] = 0;
 * [7] = 0.  The argument errors of the run. */
int qsim_batch_sweep_plan(int n_qubits, int batch, const qsim_gate* gates, size_t count, int flags,
                          int32_t info[8]);
/* Adjoint-method gradients of a sweep (no reference counterpart): the sweep above, then member t's
 * energy values[t] = <psi_t|H|psi_t> and grads[t * n_slots + j] = dE_t / d angles[t * n_slots + j],
 * indexed by slot like `angles` (not by gate as qsim_state_gradient), from one forward run and one
 * backward sweep over two work ensembles.
 * Arguments are checked as qsim_batch_run_sweep (gates, flags, angles, n_slots) and
 * qsim_state_gradient (terms) check them, with their error codes, before the first launch; null
 * values, or null grads with P > 0: QSIM_ERR_INVALID_ARGUMENT.
 * The forward run is qsim_batch_run_sweep itself: afterwards the members and qsim_batch_perm are
 * bitwise what it leaves, and the backward sweep does not write to them.  values are what
 * qsim_batch_expectation returns for that state, bitwise.
 * The backward sweep works on phi (a device copy of the ensemble where it lies) and lambda = H phi,
 * B * 2^n amplitudes each, kept on the object across calls until qsim_batch_gradient_release or
 * destroy; they are allocated before the forward run, and a failed allocation returns
 * QSIM_ERR_DEVICE with the members untouched.  Per member the recurrence is qsim_state_gradient's;
 * at a parameterised gate one launch covers all members (the bra-ket and U^† on both work states,
 * member t's U^† derived from the sweep's coefficient table), non-parameterised segments between
 * them are inverted and run as fused tile passes (n >= 10, no QSIM_BATCH_PER_GATE) or per gate.
 * QSIM_ADJOINT_FUSED=0 composes each step from a bra-ket and two per-gate launches (cross-check).
 * P == 0 or H == 0 (no terms, or all cancel): values only (zeros for H == 0), grads zero-filled.
 * count == 0: the values of the current states.  Synchronous; bitwise reproducible; member t's
 * outputs do not depend on the other members' angles. */
int qsim_batch_gradient_sweep(qsim_batch* b, const qsim_gate* gates, size_t count, const double* angles,
                              size_t n_slots, const qsim_pauli_term* terms, size_t nterms, int flags,
                              double* values /* B */, double* grads /* B * n_slots, row-major by member */);
/* Frees the work ensembles of qsim_batch_gradient_sweep (the next call allocates them again). */
int qsim_batch_gradient_release(qsim_batch* b);
/* Host-only (no GPU): what the call above would do.  info[0] = P; [1] = inverted non-parameterised
 * segments the backward sweep runs (gates before the first parameter are never undone); [2] =
 * launches of lambda = H phi; [3] = 1 if the fused path is taken; [4], [5] = work bytes
 * (2 * batch * 2^n * 16), low and high word; [6] = [7] = 0.  The argument errors of the call. */
int qsim_batch_gradient_plan(int n_qubits, int batch, const qsim_gate* gates, size_t count,
                             const qsim_pauli_term* terms, size_t nterms, int flags, int32_t info[8]);
int qsim_batch_avg_probabilities(qsim_batch* b, double* dst);           /* 2^n */
int qsim_batch_traj_probabilities(qsim_batch* b, int traj, double* dst);  /* 2^n */
int qsim_batch_traj_state(qsim_batch* b, int traj, double* dst);          /* 2*2^n */
/* BatchedSimulator::sample (src/NoiseModel.cu:938-957) on the device: uniforms and out are
 * trajectory-major, B x shots (shot s of trajectory t at t*shots + s — the reference's draw
 * order); out = lower_bound of the uniform over the trajectory's CDF, 2^n when past its end. */
int qsim_batch_sample(qsim_batch* b, const double* uniforms, int shots, int64_t* out);
/* BatchedSimulator::getHistogram (src/NoiseModel.cu:959-972): counts of the sampled outcomes
 * over every trajectory and shot, out-of-range outcomes skipped; hist has 2^n entries. */
int qsim_batch_histogram(qsim_batch* b, const double* uniforms, int shots, int64_t* hist);
/* qsim_state_expectation on every trajectory: per_traj[t] = <psi_t|H|psi_t>, t < B (no reference
 * counterpart).  Carried Pauli frames are applied first; the qubit layout is left as it is. */
int qsim_batch_expectation(qsim_batch* b, const qsim_pauli_term* terms, size_t count, double* per_traj);
/* Overlap (Gram) matrices of ensembles, computed where the members lie (no reference counterpart).
 * out: Ba x Bb complex, row-major, (re, im) interleaved: out[2 * (i * Bb + j)] = Re <a_i|b_j>.
 * b == NULL or b == a: the self matrix G of a.  Only the upper triangle is computed; the lower one
 * is written as its exact conjugate (G[j][i] == conj(G[i][j]) bitwise) and the diagonal's imaginary
 * parts are +0.0.  Carried Pauli frames are applied first.  The self case reads the ensemble under
 * whatever qsim_batch_perm the last run left (G does not depend on a relabeling that all members
 * share): the layout is not restored and the amplitudes are not written.  The cross case reads in
 * place when the two layouts are equal; otherwise both ensembles get the layout restore every
 * index-based reader applies — the one case that moves data.
 * The ensemble is a B x 2^n matrix and out = conj(A) B^T: tiles of 64 x 64 members times chunks of
 * 2^n (qsim_batch_overlap_plan), each on v_mfma_f64_16x16x4_f64, its partial tile written to scratch;
 * a second kernel adds an entry's partials in chunk order.  No floating-point atomics: the result is
 * bitwise reproducible, and an entry depends on its two members alone.  QSIM_OVERLAP_MFMA=0 runs
 * the same tiles with plain FMAs (cross-check).
 * Null out, different qubit counts or different devices: QSIM_ERR_INVALID_ARGUMENT before any
 * launch.  The scratch (a's) cannot be allocated: QSIM_ERR_DEVICE, nothing launched.  Synchronous. */
int qsim_batch_overlaps(qsim_batch* a, qsim_batch* b, double* out);
/* out: B complex, out[2 * t] = Re <a_t|s>: the call above with one column, always on the FMA kernel
 * (a GEMV is memory-bound).  In place when the ensemble's and the state's layouts are equal, else
 * both are restored.  The errors of the call above. */
int qsim_batch_state_overlaps(qsim_batch* a, qsim_state* s, double* out);
/* Host-only (no GPU): how the calls above cut their work up.  info[0] = path (0 FMA, 1 matrix
 * core; 0 whenever batch_b == 1 or QSIM_OVERLAP_MFMA=0), [1] = row tiles, [2] = column tiles, [3] =
 * tiles launched (self: the upper triangle only), [4] = K chunks, [5], [6] = partial-scratch bytes
 * (chunks x tiles x 64 x 64 x 16), low and high word, [7] = 0.  Everything but [0] depends on the
 * arguments alone.  self != 0 needs batch_a == batch_b.  Argument errors:
 * QSIM_ERR_INVALID_ARGUMENT. */
int qsim_batch_overlap_plan(int n_qubits, int batch_a, int batch_b, int self, int32_t info[8]);
/* Current logical -> physical qubit map inside every trajectory, n entries (as qsim_state_perm). */
int qsim_batch_perm(qsim_batch* b, int32_t* perm);
int qsim_batch_device_ptr(qsim_batch* b, void** dptr);
int qsim_batch_sync(qsim_batch* b);
/* Last fused batched run: tile passes and how many ran as circuit-specialised kernels. */
int qsim_batch_last_run(qsim_batch* b, int* passes, int* jit_passes);
int qsim_batch_profile(qsim_batch* b, int enable);
int qsim_batch_profile_count(qsim_batch* b, int* n);
int qsim_batch_profile_get(qsim_batch* b, int i, char* name, size_t name_len,
                           double* total_ms, int64_t* launches, double* alg_bytes);

/* ---- single-trajectory Monte-Carlo noise (NoisySimulator, include/NoiseModel.cuh:139-214) ----
 * One noise pass on `qubit` with the reference kernels' per-pair semantics
 * (applyBitFlipKernel ... applyPhaseDampingKernel, src/NoiseModel.cu:115-314): every amplitude
 * pair draws from a counter hash of (seed, counter, pair index).  Asynchronous. */
int qsim_noise_apply(qsim_state* s, int type, int qubit, double probability, uint64_t seed,
                     uint64_t counter);
/* Flips applied so far by range-checked noise launches (QSIM_NOISE_CHECK=1: the one-launch
 * reference noise kernel counts every access outside its work-group's pairs on the device and
 * fails the call if there is one; tests read this to see the check had work to do). */
int qsim_noise_check_flips(uint64_t* flips);
/* Tests: `draws` geometric gaps of a flip channel of probability p (keyed by `key`) taken the
 * engine's way (single precision first, the double log where that cannot decide) against
 * floor(ln u / ln(1 - P)) in double, both capped at one 256-pair block (a walk only needs to know
 * a gap is past its block): *mismatches (0 expected) and *fallbacks. */
int qsim_noise_gap_check(double p, uint64_t draws, uint64_t key, uint64_t* mismatches, uint64_t* fallbacks);
/* On-disk cache across processes of the first-run costs (no reference counterpart: the reference
 * compiles its kernels ahead of time and does no layout search): circuit-specialised pass kernels
 * (hipRTC code objects) and layout decisions, in QSIM_CACHE_DIR (default $XDG_CACHE_HOME/qsim_amd
 * or $HOME/.cache/qsim_amd; QSIM_CACHE=0 off).  Counters of this process: entries loaded / written. */
int qsim_cache_stats(uint64_t* jit_hits, uint64_t* jit_stores, uint64_t* layout_hits, uint64_t* layout_stores);
/* Tests: the same comparison on TARGETED draws — for every gap boundary m in [0, 256] (u_m =
 * exp(m ln(1 - P))) and both ends of the interval of doubles that round to the float nearest u_m,
 * 2 x half consecutive u values around each; *draws = how many were checked. */
int qsim_noise_gap_check_edges(double p, uint64_t half, uint64_t* mismatches, uint64_t* fallbacks,
                               uint64_t* draws);
/* NoisySimulator::run (src/NoiseModel.cu:369-382): each gate, then every channel entry in order,
 * one noise pass each; *counter advances by one per pass.  With no channel entries the circuit
 * runs as fused passes (flags = QSIM_RUN_*), else one kernel per gate (the noise interleaves). */
int qsim_noisy_run(qsim_state* s, const qsim_gate* gates, size_t count,
                   const qsim_noise_channel* channels, size_t n_channels, uint64_t seed,
                   uint64_t* counter, int flags);

/* ---- density matrices (DensityMatrix / DensityMatrixSimulator, include/DensityMatrix.cuh:63-224)
 * rho of n qubits (1 <= n <= QSIM_DM_MAX_QUBITS) lives in a qsim_state created with 2n qubits:
 * amplitude k = i * 2^n + j holds rho[i][j] (the reference's row-major layout,
 * src/DensityMatrix.cu:29-30); purity = qsim_state_total_probability, the matrix =
 * qsim_state_to_host, measurement collapse = qsim_state_collapse on bits q + n and q. */
#define QSIM_DM_MAX_QUBITS 15
/* DensityMatrixSimulator::run (src/DensityMatrix.cu:201-212): each gate as U rho U^dag, then for
 * each of its qubits every channel entry on that qubit or with qubit = -1 (a global channel).
 * CRY/CRZ/Toffoli -> QSIM_ERR_RUNTIME (:264-266).  flags = QSIM_RUN_* | QSIM_DM_REFERENCE_Y.
 * Asynchronous. */
/* QSIM_DM_REFERENCE_Y: Y acts as the reference's dmApplyY, rho -> -Y rho Y^dag
 * (src/DensityMatrix.cu:507-546: its phases are those of Y rho Y^dag times -1, so the trace
 * changes sign); default: Y rho Y^dag. */
#define QSIM_DM_REFERENCE_Y 8
int qsim_dm_run(qsim_state* rho, int n_qubits, const qsim_gate* gates, size_t count,
                const qsim_noise_channel* channels, size_t n_channels, int flags);
/* Host-only: the fused plan qsim_dm_run (QSIM_RUN_FUSED) would run for this circuit, four ints
 * per pass: tile height h (tile = 64 << h elements; -1: a per-gate step), ops, register stages,
 * contiguous run bits r0.  With QSIM_DM_PLAN_RELABELED in flags: the plan under the index-bit
 * labels a first run on |0><0| chooses. */
#define QSIM_DM_PLAN_RELABELED 0x100
int qsim_dm_plan_info(int n_qubits, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                      size_t n_channels, int flags, int32_t* info, size_t cap, size_t* n_passes);
/* Host-only: the circuit-specialised kernel source of that plan (as qsim_jit_source). */
int qsim_dm_jit_source(int n_qubits, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                       size_t n_channels, int flags, char* buf, size_t cap, size_t* len);
/* Host-only: the records of qsim_plan_stage_info for the plan qsim_dm_run (QSIM_RUN_FUSED) executes
 * for (n_qubits, gates, channels, flags) on a state that lies under the labels perm of the 2n index
 * bits (logical -> physical, column bit q, row bit q + n; null: the identity; qsim_state_perm of
 * the state): the lowered ops moved through perm, planned at the height and stage width of 2n index
 * bits.  Field 0 of an op record is the gate the op belongs to (a channel op: the gate it follows),
 * field 15 its origin: bits 0-7 QSIM_DM_ORIGIN_ROW (the gate on the row bits), _COL (its conjugate on
 * the column bits), _SIGN (the -1 of QSIM_DM_REFERENCE_Y) or _CHANNEL + noise type; bits 8-15 the
 * qubit (a gate: its target); bits 16-23 the op's place in its channel's sequence.  0 for the second
 * and third controlled-X of a lowered SWAP. */
#define QSIM_DM_ORIGIN_ROW 1
#define QSIM_DM_ORIGIN_COL 2
#define QSIM_DM_ORIGIN_SIGN 3
#define QSIM_DM_ORIGIN_CHANNEL 4
int qsim_dm_plan_stage_info(int n_qubits, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                            size_t n_channels, int flags, const int32_t* perm, int32_t* ops, size_t op_cap,
                            size_t* n_ops, int32_t* passes, size_t pass_cap, size_t* n_passes, int32_t* stages,
                            size_t stage_cap, size_t* n_stages);
/* Host-only: that plan executed on the host as qsim_plan_exec_host executes one (tests of the
 * lowering and of the planners' index math for its ops; no GPU).  amps: 4^n interleaved re/im,
 * rho row-major (logical order), updated in place; 10..26 index bits (n = 5..13), staged passes only
 * (QSIM_ERR_RUNTIME on a per-gate step or an unstaged tile).  passes: the plan's pass count. */
int qsim_dm_plan_exec_host(int n_qubits, const qsim_gate* gates, size_t count, const qsim_noise_channel* channels,
                           size_t n_channels, int flags, const int32_t* perm, double* amps, int* passes);
/* One channel (applyDepolarizing ... applyBitPhaseFlip, :298-356) on `qubit`. */
int qsim_dm_apply_channel(qsim_state* rho, int n_qubits, int type, int qubit, double p);
int qsim_dm_diagonal(qsim_state* rho, int n_qubits, double* dst);          /* 2^n: Re rho_ii */
int qsim_dm_init_pure(qsim_state* rho, int n_qubits, const double* psi);   /* rho = |psi><psi| */
int qsim_dm_init_maximally_mixed(qsim_state* rho, int n_qubits);          /* rho = I / 2^n */
/* Re Tr(rho H), H = sum_t c_t P_t over the n qubits (masks as in qsim_state_expectation), reduced
 * on the device where rho lies (no reference counterpart).  Tr(rho P) = sum_{i < 2^n}
 * rho[i][i ^ x] i^nY (-1)^popcount(i & z), nY = popcount(x & z): a string reads 2^n of the 4^n
 * elements, strings with the same x mask the same ones.  All 2^n values of i are summed (no use of
 * Hermiticity: the value is linear in whatever the buffer holds).  The element addresses are mapped
 * through the state's current index-bit layout on the host, so the layout (qsim_state_perm), the
 * current buffer and the amplitudes are left exactly as they are (the other readers of rho restore
 * the identity layout first).  Partial sums are added in a fixed order: bitwise reproducible.  A
 * mask bit >= n_qubits -> QSIM_ERR_OUT_OF_RANGE; count == 0 -> 0.0 with no launch.  Synchronises. */
int qsim_dm_expectation(qsim_state* rho, int n_qubits, const qsim_pauli_term* terms, size_t count, double* out);
/* Host-only (no GPU): what the lowering makes of these terms after duplicate strings are merged
 * and zero coefficients dropped: groups (distinct x masks), rows (a group of more terms than one
 * row's table holds takes several), kernel launches (all rows in one, up to the grid's limit of
 * 65535 rows) and elements of rho read (groups x 2^n).  perm: the layout of the 2n index bits
 * (logical -> physical, 2n entries; null: identity); anything but a permutation, or n_qubits
 * outside [1, QSIM_DM_MAX_QUBITS] -> QSIM_ERR_INVALID_ARGUMENT. */
int qsim_dm_expectation_plan(int n_qubits, const qsim_pauli_term* terms, size_t count, const int32_t* perm,
                             int* groups, int* rows, int* launches, uint64_t* elements);
/* Marginal probabilities and reduced density matrices of k distinct qubits of rho, and the fidelity
 * with a pure state, reduced on the device where rho lies (no reference counterpart).  Qubits as in
 * qsim_state_marginal_probabilities: qubit q is index bit q, the list may be in any order and bit j
 * of an output index is qubit qubits[j].  With b over the values of the n - k unlisted qubits:
 *   marginal: out[m] = sum_b Re rho[(m, b)][(m, b)], 2^k doubles, 0 <= k <= n (k == 0: the trace);
 *   matrix:   out = rho_A, 2^k x 2^k row-major, interleaved re/im (2 * 4^k doubles), 0 <= k <=
 *             min(n, 6): rho_A[a][a'] = sum_b rho[(a, b)][(a', b)];
 *   fidelity: *out = Re sum_ij conj(psi_i) rho[i][j] psi_j, psi: 2^n host amplitudes (re/im), used
 *             as given (not normalised).
 * Like qsim_dm_expectation all three are linear functionals of whatever the buffer holds: every
 * element the formula names is summed, nothing is mirrored or symmetrised (for k == n <= 6 the
 * matrix is the buffer itself and the marginal its diagonal).  The matrix reads 2^(n+k) of the 4^n
 * elements, the marginal 2^n, the fidelity streams all of them once.  Pending gates of a run-sharing
 * cycle are flushed, addresses are mapped through the state's current index-bit layout on the host,
 * and the layout (qsim_state_perm), the current buffer and the elements are left exactly as they
 * are.  Sums are added in a fixed order (no floating-point atomics): bitwise reproducible.  All
 * synchronise.  A duplicate qubit, k above the cap, a null pointer (qubits only with k > 0), a state
 * that is not rho of n_qubits -> QSIM_ERR_INVALID_ARGUMENT; a qubit < 0 or >= n ->
 * QSIM_ERR_OUT_OF_RANGE. */
int qsim_dm_marginal_probabilities(qsim_state* rho, int n_qubits, const int32_t* qubits, int k, double* out);
int qsim_dm_reduced_density_matrix(qsim_state* rho, int n_qubits, const int32_t* qubits, int k, double* out);
int qsim_dm_fidelity(qsim_state* rho, int n_qubits, const double* psi, double* out);
/* Host-only (no GPU): the lowering of the two subset readers under the layout perm of the 2n index
 * bits (logical -> physical, 2n entries; null: identity); rdm != 0: for the matrix.  Both readers
 * evaluate out[o] = sum over b < 2^(n-k) of buf[G_out(o) | G_sum(b)], G(v) = the OR of the address
 * generators (masks over the 2n physical positions) at the set bits of v.  out_gen (null: not
 * returned): one generator per bit of the out index — marginal: k masks, both positions of
 * qubits[j]; matrix: 2k single positions for o = a << k | a', [j] the column position of qubits[j]
 * (bit j of a'), [k + j] its row position (bit j of a).  sum_gen (null: not returned): both
 * positions of each of the n - k unlisted qubits, ascending.  info[0], [1] = elements of rho read
 * (2^n or 2^(n+k)), low and high word; [2] = work-groups of the first kernel; [3] = kernel launches;
 * [4] = scratch bytes of the partial sums; [5] = slices of the sum a work-group takes one of;
 * [6] = generators that are bits of the thread index; [7] reserved (0).  The argument checks and
 * error codes of the two readers; a perm that is no permutation or n_qubits outside
 * [1, QSIM_DM_MAX_QUBITS] -> QSIM_ERR_INVALID_ARGUMENT. */
int qsim_dm_marginal_plan(int n_qubits, const int32_t* qubits, int k, const int32_t* perm, int rdm,
                          int32_t info[8], uint64_t* out_gen, uint64_t* sum_gen);

/* ---- multi-GPU: state sharded by its high physical qubits, one process per GPU, RCCL ----
 * (the reference is single-GPU, README.md:361-367).  World size W = 2^g ranks;
 * rank r holds the 2^(n-g) amplitudes whose top g PHYSICAL index bits equal r.  A logical->
 * physical qubit map is kept on every rank: SWAP gates only relabel it, gates whose target sits
 * on a global (rank) bit trigger an all-to-all qubit remap over RCCL. */
typedef struct qsim_dist qsim_dist;
#define QSIM_DIST_UNIQUE_ID_BYTES 128
#define QSIM_MAX_QUBITS_DIST 36
/* Lowered operation record (host planner output, see qsim_dist_plan). kind: 0 controlled 2x2
 * (m = a,b,c,d), 1 controlled diagonal (m = d0,d1), 2 swap(t0,t1); qubits are PHYSICAL local
 * positions of the rank the plan was made for. */
typedef struct qsim_op {
    int32_t kind, sub, t0, t1;
    uint64_t cmask;
    int32_t d0_one, src;
    double m[8];
} qsim_op;
/* One plan step: kind 0 = ops[op_begin, op_end) on the local shard; kind 1 = exchange that
 * swaps global physical positions gpos[i] with local positions lpos[i], i < k.  Overlapped
 * remaps: an exchange with pivots (pmask != 0: up to 4 local physical positions; pivot = the
 * lowest, -1 if none) runs as 2^m part-exchanges, one per value of the pivot bits.  An ops step
 * with role bit 1 runs the trailing passes of its fused plan that avoid the pivots of the
 * exchange after it per part (each part's transfer then overlaps the later parts' passes); role
 * bit 2: its leading passes that avoid the pivots of the exchange before it run per part as each
 * part lands.  The step is planned as one fused plan either way (ops steps report pivot -1). */
typedef struct qsim_dist_step {
    int32_t kind, k;
    int32_t op_begin, op_end;
    int32_t gpos[8], lpos[8];
    int32_t pivot, role;
    uint64_t pmask;
    uint64_t coarse; /* exchange: pivots the step before's coarse passes leave untouched (0: none) */
} qsim_dist_step;

int qsim_dist_unique_id(void* id_out);  /* ncclGetUniqueId, on rank 0 */
int qsim_dist_create(int n_qubits, int rank, int world, const void* unique_id, int device,
                     qsim_dist** out);
/* Virtual ranks: all `world` shards in this process on one GPU, exchanged by device copies
 * (same planner and pack/unpack kernels, no RCCL) — for testing the sharded path on one GPU. */
int qsim_dist_create_virtual(int n_qubits, int world, int device, qsim_dist** out);
/* Attach a world-1 RCCL communicator (unique id from qsim_dist_unique_id) to a virtual object:
 * its slab moves then run as ncclSend / ncclRecv pairs to rank 0 itself in the same groups, and
 * its all-reduces through RCCL — the multi-rank call sequence (non-blocking init, groups,
 * settle, watchdog) on one GPU (tests). */
int qsim_dist_virtual_rccl(qsim_dist* d, const void* unique_id);
/* Exchanges of the last qsim_dist_run (summed over this process's shards) whose pack and unpack
 * ran inside the local passes: the last pass before the remap stored its tiles straight into the
 * send buffer's slab layout and the step after it planned in that layout, loading from the receive
 * buffer, its last pass storing back to the standard positions (no k_exchange_copy). */
int qsim_dist_fused_remaps(qsim_dist* d, int* remaps);
/* Host-staged transport (no RCCL): one shard per process like qsim_dist_create, but every
 * point-to-point transfer is handed to `fn` as host buffers.  A post sends `bytes` from `send` to
 * rank `peer` and receives `bytes` from `peer` into `recv` (either may be NULL for a one-sided
 * post); posts pair up as grouped ncclSend / ncclRecv do: the k-th post of rank r naming q
 * with the k-th post of q naming r.  `fn` returns 0 on success.  Used to run several rank
 * processes on one GPU (tests); no counterpart in the reference (single-GPU, README.md:361-367). */
typedef struct qsim_dist_post {
    int32_t peer, _pad;
    uint64_t bytes;
    const void* send;
    void* recv;
} qsim_dist_post;
typedef int (*qsim_dist_transport_fn)(void* ctx, const qsim_dist_post* posts, size_t count);
int qsim_dist_create_hosted(int n_qubits, int rank, int world, int device, qsim_dist_transport_fn fn,
                            void* ctx, qsim_dist** out);
int qsim_dist_destroy(qsim_dist* d);
int qsim_dist_run(qsim_dist* d, const qsim_gate* gates, size_t count, int flags);
int qsim_dist_sync(qsim_dist* d);
/* Collective: qsim_dist_sync, then a one-value all-reduce on the communicator, so every rank
 * returns within the collective's latency of the others (the per-step timing barrier of the
 * N > 1 bench; no reference counterpart: the reference is single-GPU, README.md:361-367). */
int qsim_dist_barrier(qsim_dist* d);
int qsim_dist_overlapped(qsim_dist* d, int* remaps); /* remaps of the last run that overlapped local work */
/* Runs of this object whose first step merged the previous run's carried last step (the
 * EXPERIMENTAL cross-run overlap, QSIM_DIST_CARRY=1, off by default; read per run). */
int qsim_dist_carried_runs(qsim_dist* d, int* runs);
int qsim_dist_remap_bytes(qsim_dist* d, double* sent); /* bytes this rank sent in its last run's remaps */
int qsim_dist_reset(qsim_dist* d);                         /* |0..0>, identity qubit map */
int qsim_dist_perm(qsim_dist* d, int32_t* perm);            /* logical -> physical, n entries */
/* This rank's 2*2^(n-g) doubles (virtual mode: all shards in rank order, 2*2^n doubles). */
int qsim_dist_local_state(qsim_dist* d, double* dst);
/* Full state in LOGICAL index order on rank 0 (collective; dst may be NULL on other ranks). */
int qsim_dist_gather_state(qsim_dist* d, double* dst);
int qsim_dist_total_probability(qsim_dist* d, double* out); /* collective */
int qsim_dist_prob_bit_zero(qsim_dist* d, int logical_bit, double* out);  /* collective */
/* ---- readout of the sharded state.  Every entry below is collective: every rank calls it with
 * the same arguments (virtual objects: one call covers all shards). ---- */
/* Rank 0's `count` doubles go to every rank (RCCL: ncclBroadcast; hosted: posts; virtual and
 * world 1: nothing to do).  How one host random draw becomes the same on every rank. */
int qsim_dist_bcast(qsim_dist* d, double* buf, size_t count);
/* 2^n doubles |a_i|^2 in LOGICAL index order on rank 0 (dst may be NULL on other ranks).  |a|^2
 * is computed per shard on the device, so 8 B per amplitude are gathered, not 16. */
int qsim_dist_probabilities(qsim_dist* d, double* dst);
/* qsim_state_sample on the sharded state: out[s] = lower_bound of uniforms[s] over the CDF in
 * logical index order, 2^n past the end; every rank passes the same uniforms and receives all
 * `shots` indices.  Nothing is gathered: per-chunk sums of |a|^2 (chunks of 2^min(12, L) logical
 * indices) are all-reduced, each shot's chunk is searched on the rank that owns it.  If one of
 * the chunk's logical qubits sits on a rank position, one remap brings them local first: the
 * amplitudes are unchanged, but the qubit map (qsim_dist_perm) may differ afterwards.
 * shots <= 0 returns at once. */
int qsim_dist_sample(qsim_dist* d, const double* uniforms, int shots, int64_t* out);
/* Zero the amplitudes whose logical bit != result and scale the rest (qsim_state_collapse). */
int qsim_dist_collapse(qsim_dist* d, int logical_bit, int result, double scale);
/* Measure a logical bit with the caller's uniform u (the same on every rank): result = u < p0 ?
 * 0 : 1 with p0 = qsim_dist_prob_bit_zero, then collapse with scale 1 / sqrt(p(result)).  An
 * outcome of probability below 1e-15 fails with QSIM_ERR_RUNTIME. */
int qsim_dist_measure(qsim_dist* d, int logical_bit, double u, int* result);
/* qsim_state_expectation on the sharded state: <psi|H|psi>, the same double on every rank.  The
 * state is read where it lies: the masks are mapped through the qubit map, no remap runs, and the
 * map, the amplitudes and the buffers are left exactly as they are.  A group of terms whose
 * physical x mask has no rank position is one read of each shard; one with rank positions x_rank
 * pairs rank r with rank r ^ x_rank, and HALF of the peer's shard crosses the link (each pair is
 * taken by one of the two ranks).  Groups with the same (x_rank, top local position in x) share a
 * transfer, so a call makes at most 2 (world - 1) of them; the local groups and the kernels of
 * one transfer run while the next transfer is in flight (QSIM_DIST_EXPECT_OVERLAP=0, read per
 * call: one receive buffer, every transfer waited for).  Sums are added in a fixed order (groups
 * in plan order, shards in rank order, one all-reduce of the ranks' totals per call): two calls on
 * the same state and layout return bitwise-equal values.  Error codes: qsim_state_expectation's. */
int qsim_dist_expectation(qsim_dist* d, const qsim_pauli_term* terms, size_t count, double* out);
/* Host-only: what qsim_dist_expectation would do for qubit map `perm` (n entries; null: the
 * identity) in a world of `world` ranks: the groups read inside a shard and across ranks, the
 * half-shard transfers, the kernel launches per shard and the bytes one rank sends. */
int qsim_dist_expectation_plan(int n_qubits, int world, const int32_t* perm, const qsim_pauli_term* terms,
                               size_t count, int* local_groups, int* cross_groups, int* transfers, int* launches,
                               uint64_t* bytes_sent_per_rank);
/* qsim_state_marginal_probabilities / qsim_state_reduced_density_matrix on the sharded state
 * (collective): their conventions, caps (k <= min(n, 20) / k <= min(n, 6)), argument checks and
 * error codes, all checked on the host before any launch or transfer; the same doubles on EVERY
 * rank.  Like qsim_dist_expectation they flush pending work, map the qubits through the qubit map
 * on the host and make one streaming read of every shard where it lies: no remap, no gather of
 * amplitudes; the map, the amplitudes and the gradient work states are left exactly as they are.
 * Both synchronise.  A selected qubit sits on a local position or on a rank position (the top
 * log2(world) ones).
 * Marginal: every shard bins its local positions and adds its 2^k_loc bins into the rank's
 * zero-filled 2^k vector at the indices of its own rank bits (shards of a process in rank order,
 * no floating-point atomics); one all-reduce of 2^k doubles adds the ranks.
 * Matrix: blocks between equal rank bits are one read of each shard.  For every non-zero d inside
 * the selected rank positions (at most 7 steps) rank r pairs with r ^ d and the block between the
 * two is computed from the own shard and the received one.  When the top local position is not
 * selected, half a shard moves each way and each rank of a pair sums half of the environment;
 * when it is selected, a whole shard moves each way and the lower rank computes the block.  Sums
 * are added in a fixed order (diagonal blocks shard by shard in rank order, then the steps in
 * ascending d), one all-reduce of 2 * 4^k doubles follows, and the host mirrors the upper triangle:
 * rho equals its conjugate transpose bitwise and two calls on the same state and layout return
 * identical doubles.  Device scratch beyond the state's staging buffers: at most 64 MiB of
 * partial sums, plus one block vector and the result vector. */
int qsim_dist_marginal_probabilities(qsim_dist* d, const int32_t* qubits, int k, double* out);
int qsim_dist_reduced_density_matrix(qsim_dist* d, const int32_t* qubits, int k, double* out);
/* Host-only (no GPU): what the two entries above do for qubit map `perm` (n entries; null: the
 * identity) in a world of `world` ranks; rdm != 0: for the matrix.  With L = n - log2(world):
 * info[0] = k_loc, selected physical positions below L; [1] = k_rank, those from L up;
 * [2], [3], [4], [5] = k_lo, k_hi, slices and work-groups of the shard's own plan, which are
 * qsim_marginal_plan's for n = L and the k_loc local positions; [6] = cross steps (2^k_rank - 1
 * for the matrix, 0 for the marginal); [7] = transfers per rank (one send / receive pair per
 * step); [8], [9] = bytes one rank sends in a call, low and high word; [10] = kernel launches per
 * shard, at most (a rank that is the lower one of all its pairs); [11] = doubles in the one
 * all-reduce; [12], [13] = scratch bytes of the partial sums, low and high word (<= 64 MiB; the
 * block vector and the result vector come on top); [14] = the pair rule: 0 no cross step, 1 half a
 * shard each way and both ranks compute, 2 a whole shard each way and the lower rank computes;
 * [15] = work-groups of the two-source kernel (0 without cross steps).  The argument checks and
 * error codes of the two entries above; a perm that is no permutation or a world that is no
 * power of two -> QSIM_ERR_INVALID_ARGUMENT. */
int qsim_dist_marginal_plan(int n_qubits, int world, const int32_t* perm, const int32_t* qubits, int k, int rdm,
                            int32_t info[16]);
/* qsim_state_gradient on the sharded state (collective).  Runs the circuit exactly as
 * qsim_dist_run(d, gates, count, flags) would (fresh-state relabel, plan cache; a carried step is
 * flushed first, as by every reader), then *value = <psi|H|psi> as qsim_dist_expectation computes
 * it and grad[k] = dE/d(parameter of gate k) for Rx / Ry / Rz / CRY / CRZ, 0.0 for any other gate,
 * by one backward sweep over two sharded work states phi and lambda = H phi.  Afterwards the
 * state, qsim_dist_perm and what the run getters report are what qsim_dist_run alone leaves, the
 * amplitudes bit for bit: the sweep never writes to the state's shards.
 * The work states are read under a qubit map of their own that starts as the state's.  H phi: a
 * group of terms whose physical x mask has no rank position is one pass over each shard; groups
 * with rank positions x_rank read the WHOLE phi shard of rank r ^ x_rank, one transfer per distinct
 * x_rank.  A parameterised step, by the physical positions of its target t and control c:
 *   t local, c local or absent: the single-GPU step on each shard (QSIM_ADJOINT_FUSED=0 composes
 *     it from a reduction and two per-gate launches, as there; the variable has no effect on the
 *     classes below, which always use their own kernels);
 *   t local, c on a rank position: the uncontrolled step on the ranks whose bit is 1;
 *   Rz / CRZ with t on a rank position: one streaming kernel per shard, no transfer;
 *   Rx / Ry / CRY with t on a rank position: rank r pairs with the rank whose t bit differs and
 *     receives its whole old phi shard, then its whole old lambda shard (two transfers, the second
 *     in flight while the first kernel runs; with a local control the whole shard still crosses,
 *     the kernel touches the c == 1 half); the circuit's first rotation needs phi alone.
 *   With c on a rank position only the ranks whose bit is 1 take part.
 * Runs of other gates between rotations are inverted and run on both work states through the
 * sharded planner (remaps included) from the work map, which they may change; they never touch the
 * state's map, counters or cached run plans.  The sweep stops at the circuit's first rotation.
 * Every (parameter, shard) sum has a slot of its own, the shards of a process are added in rank
 * order and ONE vector all-reduce adds the ranks: every rank returns the same doubles and two
 * calls return bitwise-equal results.  Work memory: two extra shards per rank, allocated by the
 * first call that sweeps, kept until qsim_dist_gradient_release or qsim_dist_destroy; the
 * exchange staging buffers serve the transfers (a world of one has and needs none).
 * count == 0: the value of the state as it is (no run); nterms == 0 (or H == 0): value 0, zero
 * gradient, no sweep, no allocation.  Null pointers -> QSIM_ERR_INVALID_ARGUMENT, a mask bit >= n
 * -> QSIM_ERR_OUT_OF_RANGE, a bad gate -> the code of qsim_dist_run, work shards that cannot be
 * allocated -> QSIM_ERR_DEVICE with the state holding U|psi0>.  Synchronises. */
int qsim_dist_gradient(qsim_dist* d, const qsim_gate* gates, size_t count, const qsim_pauli_term* terms,
                       size_t nterms, int flags, double* value, double* grad);
int qsim_dist_gradient_release(qsim_dist* d); /* free the work shards now */
/* Device bytes of the gradient work shards this process holds now (0 before the first sweep and
 * after a release). */
int qsim_dist_gradient_memory_bytes(qsim_dist* d, uint64_t* bytes);
/* Host-only: what qsim_dist_gradient would do, the qubit map simulated through the forward plan
 * and the sweep.  Valid when the call starts from a non-fresh state with map `perm` (null: the
 * identity): a fresh state (create / reset) may relabel its local positions first, which this
 * entry does not model.  A step transfer or an apply transfer moves one whole shard
 * (16 << (n - log2 world) bytes); bytes_sent_per_rank = (apply_transfers + step_transfers) x that:
 * what a rank whose control bits are all 1 sends outside the segments' remaps. */
typedef struct qsim_dist_gradient_info {
    int32_t params;             /* parameterised gates */
    int32_t steps_local;        /* t local, c local or absent */
    int32_t steps_local_crank;  /* t local, c on a rank position */
    int32_t steps_diag;         /* Rz / CRZ, t on a rank position, c local or absent */
    int32_t steps_diag_crank;   /* ... c on a rank position */
    int32_t steps_cross;        /* Rx / Ry / CRY, t on a rank position, c local or absent */
    int32_t steps_cross_crank;  /* ... c on a rank position */
    int32_t cross_rx, cross_ry, cross_cry;     /* the cross steps (both kinds) by gate type */
    int32_t local_ctrl_below, local_ctrl_above; /* steps_local with a control below / above the target */
    int32_t segments;           /* inverted runs of non-parameterised gates */
    int32_t remap_segments;     /* ... that need at least one remap */
    int32_t segment_remaps;     /* remaps of all segments, per work state */
    int32_t apply_groups_local, apply_groups_cross, apply_transfers, apply_launches; /* lambda = H phi */
    int32_t step_transfers;     /* whole-shard transfers of the cross steps */
    uint64_t bytes_sent_per_rank;
    int32_t perm_after_run[64]; /* the state's map after the forward run (the sweep's first map) */
    int32_t perm_after_sweep[64]; /* the work map when the sweep ends */
} qsim_dist_gradient_info;
int qsim_dist_gradient_plan(int n_qubits, int world, const int32_t* perm, const qsim_gate* gates, size_t count,
                            const qsim_pauli_term* terms, size_t nterms, qsim_dist_gradient_info* out);
/* qsim_state_apply_pauli_rotations on the sharded state (collective): term t of `rots` is
 * exp(-i coeff_t/2 P_t), applied in order where the state lies.  The masks are mapped through the
 * qubit map on the host; no remap ever runs for a rotation and qsim_dist_perm, the run getters,
 * the cached run plans and the gradient work shards are left as they are (a carried step is
 * flushed first, as by every entry that changes the state).  With L = n - log2 world local
 * positions the physical masks split as x = x_loc | x_rank << L, z alike, and the z bits on rank
 * positions are a sign that is constant on a shard and folded in on the host.  Classes:
 *   phase (x == 0): a maximal run of consecutive Z/I-only rotations is one pass per shard (one
 *     launch per 256 rotations), each shard with its own signed angle table; no transfer;
 *   local (x_rank == 0, x_loc != 0): the single-GPU pair kernel on each shard; no transfer;
 *   cross (x_rank != 0): rank r pairs with the single peer r ^ x_rank; both send their WHOLE old
 *     shard through the exchange staging buffers (every amplitude is updated, so the half-shard
 *     transfer of qsim_dist_expectation does not apply), then one kernel writes
 *     own[i] = cos(theta/2) own[i] + w sg(i) peer[i ^ x_loc]: 32 B read and 16 B written per
 *     amplitude, 16 B per amplitude and direction over the link.  The shard is overwritten only
 *     after the transfer that sends it has completed.  x_loc may be 0 (a pure rank flip).
 * Nothing is reordered or merged beyond Z-only runs.  Every argument of the whole sequence is
 * checked before the first launch or post, so a bad mask fails on all ranks alike: a mask bit >= n
 * -> QSIM_ERR_OUT_OF_RANGE, null rots with count > 0 -> QSIM_ERR_INVALID_ARGUMENT, the state
 * untouched.  count == 0 does nothing.  QSIM_PAULI_BLOCKS caps the work-groups of all three
 * streaming kernels.  A world of one runs exactly the launches of qsim_state_apply_pauli_rotations.
 * Asynchronous on virtual ranks and RCCL; the hosted transport completes each transfer on the host. */
int qsim_dist_apply_pauli_rotations(qsim_dist* d, const qsim_pauli_term* rots, size_t count);
/* Host-only: what the call above would do for qubit map `perm` (n entries; null: the identity) in
 * a world of `world` ranks.  A transfer moves one whole shard (16 << (n - log2 world) bytes). */
typedef struct qsim_dist_pauli_rotation_info {
    int32_t rotations;        /* count */
    int32_t phase_rotations;  /* x == 0 */
    int32_t phase_passes;     /* maximal runs of them: one pass over each shard per run */
    int32_t local_rotations;  /* x_rank == 0, x_loc != 0 */
    int32_t cross_rotations;  /* x_rank != 0 */
    int32_t cross_pure;       /* ... of which x_loc == 0 */
    int32_t launches;         /* kernel launches per shard */
    int32_t transfers;        /* whole-shard transfers: one per cross rotation */
    uint64_t bytes_sent_per_rank;
} qsim_dist_pauli_rotation_info;
int qsim_dist_pauli_rotation_plan(int n_qubits, int world, const int32_t* perm, const qsim_pauli_term* rots,
                                  size_t count, qsim_dist_pauli_rotation_info* out);
/* qsim_state_pauli_gradient on the sharded state (collective).  Applies the sequence exactly as
 * qsim_dist_apply_pauli_rotations does, then *value = <psi|H|psi> as qsim_dist_expectation computes
 * it and grad[k] = dE/dtheta_k for k < count by one backward sweep over the two sharded work
 * states of qsim_dist_gradient (the same buffers: counted by qsim_dist_gradient_memory_bytes, freed
 * by qsim_dist_gradient_release), phi copied from the state and lambda = H phi built as there.
 * Rotations never change the qubit map, so the sweep has no segments and no remaps.  One step per
 * rotation, last to first (Z-only runs are not merged in the sweep):
 *   phase and local: the single-GPU step on each shard (Im <lambda|P|phi>, then exp(+i theta/2 P)
 *     on both work states in one launch), the shard's rank sign folded in on the host;
 *   cross: the rank receives the peer's whole old phi shard, then its old lambda shard (the second
 *     transfer in flight while the first kernel runs); launch 1 adds this rank's share of
 *     Im conj(lambda_own)(P phi)_own and updates phi_own, launch 2 updates lambda_own.  The two
 *     ranks' shares add up to the whole bra-ket.
 * The sweep's last step, the sequence's first rotation, is the bra-ket alone: a cross step there
 * needs the peer's phi only and stores nothing.  No floating-point atomics: every (rotation, shard)
 * sum has a slot of its own, the shards of a process are added in rank order and ONE vector
 * all-reduce adds the ranks, so every rank returns the same doubles and two calls return
 * bitwise-equal results.  The sweep never writes the state's shards: the state ends exactly as
 * qsim_dist_apply_pauli_rotations alone leaves it.  count == 0: *value = <H> of the state as it is;
 * nterms == 0 or H == 0: value 0, zero gradient, no sweep, no allocation.  Every argument is checked
 * before the sequence is applied (the codes of the apply call; a mask bit >= n of the observable ->
 * QSIM_ERR_OUT_OF_RANGE); work shards that cannot be allocated -> QSIM_ERR_DEVICE with the state
 * holding the rotated state.  Synchronises. */
int qsim_dist_pauli_gradient(qsim_dist* d, const qsim_pauli_term* rots, size_t count, const qsim_pauli_term* terms,
                             size_t nterms, double* value, double* grad);
/* Host-only: what qsim_dist_pauli_gradient would do under qubit map `perm` (null: the identity).
 * bytes_sent_per_rank = (forward.transfers + apply_transfers + step_transfers) whole shards. */
typedef struct qsim_dist_pauli_gradient_info {
    qsim_dist_pauli_rotation_info forward; /* the sequence's application */
    int32_t steps;            /* steps of the sweep: count, or 0 when H == 0 (no sweep) */
    int32_t steps_phase, steps_local, steps_cross; /* ... by class */
    int32_t first_class;      /* class of the sequence's first rotation, the bra-ket-only step:
                                 0 phase, 1 local, 2 cross; -1 without a sweep */
    int32_t apply_groups_local, apply_groups_cross, apply_transfers, apply_launches; /* lambda = H phi */
    int32_t step_transfers;   /* whole-shard transfers of the cross steps: 2 each, 1 for the first rotation */
    uint64_t bytes_sent_per_rank;
} qsim_dist_pauli_gradient_info;
int qsim_dist_pauli_gradient_plan(int n_qubits, int world, const int32_t* perm, const qsim_pauli_term* rots,
                                  size_t count, const qsim_pauli_term* terms, size_t nterms,
                                  qsim_dist_pauli_gradient_info* out);
/* Host-only: what qsim_dist_sample would do for qubit map `perm` (n entries): the chunk size
 * (log2) and the set of logical qubits it must bring local first (0: no remap). */
int qsim_dist_sample_plan(int n_qubits, int world, const int32_t* perm, int* chunk_log,
                          uint64_t* localize_mask);
int qsim_dist_profile(qsim_dist* d, int enable);
int qsim_dist_profile_count(qsim_dist* d, int* n);
int qsim_dist_profile_get(qsim_dist* d, int i, char* name, size_t name_len, double* total_ms,
                          int64_t* launches, double* alg_bytes);
/* Host-only planner (no GPU, no RCCL): the exact step list qsim_dist_run executes on `rank`
 * starting from qubit map perm_inout (updated).  Call with caps = 0 to size the output. */
int qsim_dist_plan(int n_qubits, int world, int rank, const qsim_gate* gates, size_t count,
                   int32_t* perm_inout, qsim_dist_step* steps, size_t step_cap, size_t* n_steps,
                   qsim_op* ops, size_t op_cap, size_t* n_ops);

/* Host-only: per step of that plan, as qsim_dist_run would plan it, three ints: fused passes
 * (-1 for an exchange step), leading passes that run per half as the exchange before lands, and
 * trailing passes that run per half before the exchange after (the overlapped work);
 * `cap` counts steps.  perm_inout updated as by qsim_dist_plan. */
int qsim_dist_plan_passes(int n_qubits, int world, int rank, const qsim_gate* gates, size_t count,
                          int32_t* perm_inout, int32_t* passes, size_t cap, size_t* n_steps);
/* As qsim_dist_plan_passes, with the cross-run overlap of qsim_dist_run: *carry_inout (in) the
 * pivots of the previous run's last remap still in flight when this run starts (0: none; the first
 * step's leading passes that avoid them run per part), (out) the pivots this run carries into the
 * next (its last step runs wholly per part and is merged into the next run's first step). */
int qsim_dist_plan_passes_carry(int n, int world, int rank, const qsim_gate* gates, size_t count,
                                int32_t* perm_inout, uint64_t* carry_inout, int32_t* passes, size_t cap,
                                size_t* n_steps);
/* As qsim_dist_plan_passes_carry with five ints per step: passes, head, tail, then the coarse
 * passes (those just ahead of the tail that run per coarse part, DStep::coarse / qsim_dist_step
 * .coarse of the exchange after) and the number of coarse pivot bits. */
int qsim_dist_plan_passes_coarse(int n, int world, int rank, const qsim_gate* gates, size_t count,
                                 int32_t* perm_inout, uint64_t* carry_inout, int32_t* passes, size_t cap,
                                 size_t* n_steps);

/* Host-only: forget the process-wide memo of remap pivots (planning is then redone from scratch,
 * as in a fresh rank process). */
int qsim_dist_plan_memo_clear(void);
/* Host-only: the slab layout the pack / unpack kernels use for exchange step `step` on `rank`.
 * part < 0: the whole remap; part j: part j of an overlapped remap (its pivot bits hold j).
 * my_c: the slab that stays; peer_of[c], c < 2^k: the rank slab c goes to and comes from;
 * index[c * chunk + e] (e < chunk = 2^(L - k - m), m = pivots of a part, 0 for part < 0): the
 * local amplitude index of element e of slab c.  index_cap counts entries (2^(L - m) needed). */
int qsim_dist_slab_map(int n_qubits, int world, int rank, const qsim_dist_step* step, int part,
                       int32_t* my_c, int32_t* peer_of, uint64_t* index, size_t index_cap);

#define QSIM_MAX_QUBITS_SINGLE 30
#define QSIM_MIN_QUBITS 1

#ifdef __cplusplus
}
#endif
#endif /* QSIM_HIP_H */
