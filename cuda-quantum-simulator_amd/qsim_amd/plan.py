"""Host-side view of the engine's fused-pass planner (qsim_plan_fused, include/qsim_hip.h)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .circuit import Circuit


def plan_fused(circuit: Circuit, hmax: int = 6):
    """Return (order, pass_of, n_passes): execution order of the circuit's gates (indices into
    circuit.getGates()), the pass each runs in (-1 = per-gate), and the number of fused passes."""
    arr, cnt = circuit.to_abi()
    order = np.zeros(max(1, cnt), np.int32)
    pass_of = np.zeros(max(1, cnt), np.int32)
    npass = ctypes.c_int32(0)
    _lib.check(_lib.hip.qsim_plan_fused(circuit.getNumQubits(), arr, cnt, hmax,
                                        order.ctypes.data_as(ctypes.c_void_p),
                                        pass_of.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(npass)))
    return order[:cnt], pass_of[:cnt], npass.value


_STAGE_POS = ("first", "middle", "last", "only")
_SWIZZLE = (None, "fixed", "searched")


def plan_stage_info(circuit: Circuit, relayout: bool = False) -> dict:
    """The stages of the plan run(circuit, Fused) would execute under the process settings in force
    (qsim_plan_stage_info, host only; relayout: the relayout plan of a first run).  Returns
    {"ops": [...], "passes": [...]}: one dict per executed tile op in execution order (src: source
    gate index, -1 for the second and third op of a lowered SWAP; pass, stage, pos in first / middle
    / last / only; kind, sub, p0, b0, b1, cmask, cm_reg, cm_thr, cm_out, d0_one) and one per pass
    (single, h, r0, rb, hpos, hu_count, relayout, stages, ops, lds_fixed, lds_searched, swizzle: per
    LDS round trip "fixed" or "searched", stage_bits: the register-bit mask of every stage)."""
    arr, cnt = circuit.to_abi()
    n = circuit.getNumQubits()
    return _stage_info(lambda *args: _lib.hip.qsim_plan_stage_info(n, arr, cnt, 1 if relayout else 0, *args))


def _stage_info(entry) -> dict:
    """The three record tables of qsim_plan_stage_info / qsim_dm_plan_stage_info as dicts; entry
    takes the nine table arguments (buffer, capacity, count of each)."""
    sizes = [ctypes.c_size_t(0) for _ in range(3)]

    def call(bufs, caps):
        args = []
        for b, c, s in zip(bufs, caps, sizes):
            args += [b.ctypes.data_as(ctypes.c_void_p) if b is not None else None, c, ctypes.byref(s)]
        _lib.check(entry(*args))

    call([None] * 3, [0] * 3)
    caps = [s.value for s in sizes]
    bufs = [np.zeros(max(1, c) * w, np.int32) for c, w in zip(caps, (16, 24, 8))]
    call(bufs, caps)
    ops_t, pass_t, stage_t = (b.reshape(-1, w)[:c].tolist() for b, c, w in zip(bufs, caps, (16, 24, 8)))
    u32 = lambda x: x & 0xffffffff
    ops = [{"src": r[0], "pass": r[1], "stage": r[2], "pos": _STAGE_POS[r[3]], "kind": r[4], "sub": r[5],
            "p0": r[6], "b0": r[7], "b1": r[8], "cmask": u32(r[9]), "cm_reg": u32(r[10]), "cm_thr": u32(r[11]),
            "cm_out": u32(r[12]) | (u32(r[13]) << 32), "d0_one": r[14], "origin": r[15]} for r in ops_t]
    passes = [{"single": bool(r[0]), "h": r[1], "r0": r[2], "rb": r[3], "hu_count": r[4], "relayout": r[5],
               "stages": r[6], "ops": r[7], "lds_fixed": r[8], "lds_searched": r[9], "hpos": r[11:11 + r[10]],
               "swizzle": [], "stage_bits": []} for r in pass_t]
    for r in stage_t:
        passes[r[0]]["stage_bits"].append(u32(r[3]))
        if r[5]:
            passes[r[0]]["swizzle"].append(_SWIZZLE[r[5]])
    return {"ops": ops, "passes": passes}


_DM_ORIGINS = ("", "row", "col", "sign", "ch0", "ch1", "ch2", "ch3", "ch4", "ch5")


def _dm_args(n: int, circuit: Circuit, channels, perm):
    arr, cnt = circuit.to_abi()
    ch = (_lib.qsim_noise_channel * max(1, len(channels)))()
    for i, (t, q, p) in enumerate(channels):
        ch[i].type, ch[i].qubit, ch[i].probability = int(t), int(q), float(p)
    return arr, cnt, ch, len(channels), _perm_arg(2 * n, perm)


def dm_plan_stage_info(circuit: Circuit, channels=(), flags: int = 1, perm=None) -> dict:
    """plan_stage_info of the plan DensityMatrixSimulator.run executes for (circuit, channels as
    (type, qubit or -1, p), flags) on a state under the labels perm of the 2n index bits (logical ->
    physical, StateVector.perm() of the density matrix's state; None: identity), host only
    (qsim_dm_plan_stage_info).  Every op record also names where it came from: src is the gate it
    belongs to or follows, origin "row" / "col" (the gate and its conjugate), "sign" (the -1 of the
    reference's Y), "ch0".."ch5" (a channel of that noise type) or "" (the second and third op of a
    lowered SWAP); qubit: the gate's target or the channel's qubit; seq: the op's place in its
    channel's sequence."""
    n = circuit.getNumQubits()
    arr, cnt, ch, nch, pi = _dm_args(n, circuit, channels, perm)
    info = _stage_info(lambda *args: _lib.hip.qsim_dm_plan_stage_info(n, arr, cnt, ch, nch, flags, pi, *args))
    for r in info["ops"]:
        word = r["origin"]
        r["origin"], r["qubit"], r["seq"] = _DM_ORIGINS[word & 0xff], (word >> 8) & 0xff, (word >> 16) & 0xff
    return info


def dm_plan_exec_host(circuit: Circuit, rho, channels=(), flags: int = 1, perm=None):
    """That plan executed on the host with the staged kernels' index math on the 2^n x 2^n matrix
    rho (qsim_dm_plan_exec_host; 10..26 index bits, staged passes only; no GPU).  Returns (rho after
    the run, pass count)."""
    n = circuit.getNumQubits()
    arr, cnt, ch, nch, pi = _dm_args(n, circuit, channels, perm)
    st = np.array(rho, dtype=np.complex128).reshape(-1)
    if st.shape != (1 << (2 * n),):
        raise ValueError("rho must hold 4^n elements")
    passes = ctypes.c_int(0)
    _lib.check(_lib.hip.qsim_dm_plan_exec_host(n, arr, cnt, ch, nch, flags, pi, st.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.byref(passes)))
    return st.reshape(1 << n, 1 << n), passes.value


def set_jit(mode: int = -1, min_qubits: int = -1) -> None:
    """Circuit-specialised pass kernels: mode 0 off, 1 background compile (default), 2 compile
    on a plan's first run; states below `min_qubits` use the pass interpreter (qsim_set_jit)."""
    _lib.check(_lib.hip.qsim_set_jit(mode, min_qubits))


def jit_source(circuit: Circuit) -> str:
    """The HIP source the engine generates for this circuit's fused plan ('' if no staged pass)."""
    arr, cnt = circuit.to_abi()
    n = ctypes.c_size_t(0)
    _lib.check(_lib.hip.qsim_jit_source(circuit.getNumQubits(), arr, cnt, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value + 1)
    _lib.check(_lib.hip.qsim_jit_source(circuit.getNumQubits(), arr, cnt, buf, n.value + 1,
                                        ctypes.byref(n)))
    return buf.value.decode()


def jit_build(circuit: Circuit) -> int:
    """Compile the circuit's generated pass kernels with hipRTC for gfx950 (no GPU needed);
    returns the code-object size in bytes (0 when nothing is specialised)."""
    arr, cnt = circuit.to_abi()
    n = ctypes.c_size_t(0)
    _lib.check(_lib.hip.qsim_jit_build(circuit.getNumQubits(), arr, cnt, ctypes.byref(n)))
    return n.value


def set_relabel(mode: int = -1, min_qubits: int = -1) -> None:
    """Layout-aware qubit relabeling of fused runs (qsim_set_relabel): mode 0 off, 1 on; states
    below `min_qubits` are never relabeled; negative arguments leave a setting unchanged."""
    _lib.check(_lib.hip.qsim_set_relabel(mode, min_qubits))


def set_relayout(mode: int = -1, min_qubits: int = -1) -> None:
    """Relayout plans (every pass stores its tile under the next pass's qubit layout) for first
    runs of states from `min_qubits` on (qsim_set_relayout): mode 0 off, 1 on (when they need
    fewer passes or win the device timing), 2 forced (tests); negative arguments leave a setting
    unchanged."""
    _lib.check(_lib.hip.qsim_set_relayout(mode, min_qubits))


def set_run_share(mode: int = -1, copies: int = -1) -> None:
    """Run sharing (qsim_set_run_share): repeated fused runs of one circuit executed as calls of
    ONE joint relayout plan of `copies` runs (0, the default: 4 below 26 qubits, 8 from there); gates
    a call could not yet run stay
    pending until the next call or the next reader of the state.  mode 0 off, 1 on (default, for
    states from the relayout size threshold); negative arguments leave a setting unchanged."""
    _lib.check(_lib.hip.qsim_set_run_share(mode, copies))


def set_calibrate(mode: int = -1, min_qubits: int = -1) -> None:
    """Time the layout model's top candidates on the device at a basis state's first run and
    keep the fastest (qsim_set_calibrate; needs set_jit(2)): mode 0 off, 1 on."""
    _lib.check(_lib.hip.qsim_set_calibrate(mode, min_qubits))


def set_tile_height(h: int = -1) -> None:
    """Tile height of fused passes planned from now on (qsim_set_tile_height): tiles of 6 + h
    qubits, h in 0..7 (default 6); h < 0 restores the default."""
    _lib.check(_lib.hip.qsim_set_tile_height(h))


def set_tile_rb7(rb: int = -1) -> None:
    """Register bits per stage of 13-qubit tiles (4: 512-thread workgroups, default; 3: 1024
    threads with 8 amplitudes each); -1 restores QSIM_TILE_RB7."""
    _lib.check(_lib.hip.qsim_set_tile_rb7(rb))


def set_tile_ctrl_out(mode: int = -1) -> None:
    """Tile-constant controls (qsim_set_tile_ctrl_out): 1 (default) a control qubit need not be a
    tile qubit (the op runs per tile where it reads 1), 0 every control is a tile qubit."""
    _lib.check(_lib.hip.qsim_set_tile_ctrl_out(mode))


# The shipped policy (include/qsim_hip.h; environment variables unset).
DEFAULTS = {"jit": (1, 20), "relabel": (1, 26), "relayout": (1, 20), "calibrate": (1, 26),
            "run_share": (1, 0)}


def restore_defaults() -> None:
    """Put every process-wide planning policy back to the shipped defaults: background JIT from
    20 qubits, relabeling from 26, relayout plans from 20, calibrated first runs from 26 (with
    inline compilation), run sharing on with its cycle length by state size, the size rule for tile heights (tests call this after changing any)."""
    set_jit(*DEFAULTS["jit"])
    set_relabel(*DEFAULTS["relabel"])
    set_relayout(*DEFAULTS["relayout"])
    set_calibrate(*DEFAULTS["calibrate"])
    set_run_share(*DEFAULTS["run_share"])
    set_tile_height(-1)
    set_tile_ctrl_out(1)


def plan_relabel(circuit: Circuit):
    """(perm, predicted_us_before, predicted_us_after): the logical -> physical qubit map the
    engine would choose for this circuit's fused plan (identity when none pays), host only."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    perm = (ctypes.c_int32 * n)()
    b, a = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.hip.qsim_plan_relabel(n, arr, cnt, perm, ctypes.byref(b), ctypes.byref(a)))
    return list(perm), b.value, a.value


def plan_exec_host(circuit: Circuit, mode: int = 1, state=None):
    """Plan the circuit (mode 0: fixed-layout planner under the identity labels, 1: relayout
    planner) and execute the plan on the host exactly as the staged pass kernels address the
    state (qsim_plan_exec_host; tests of the planners' index math, no GPU).  Returns
    (state in logical order, start/end layout, pass count)."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    if state is None:
        st = np.zeros(1 << n, np.complex128)
        st[0] = 1.0
    else:
        st = np.array(state, dtype=np.complex128)
    st = np.ascontiguousarray(st)
    perm = (ctypes.c_int32 * n)()
    passes = ctypes.c_int(0)
    _lib.check(_lib.hip.qsim_plan_exec_host(n, arr, cnt, mode, st.ctypes.data_as(ctypes.c_void_p),
                                            perm, ctypes.byref(passes)))
    return st, list(perm), passes.value


def plan_relayout(circuit: Circuit):
    """(perm, passes, predicted_us) of the circuit's relayout plan (qsim_plan_relayout, host
    only); passes = 0 when no relayout plan exists."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    perm = (ctypes.c_int32 * n)()
    passes = ctypes.c_int(0)
    pred = ctypes.c_double(0.0)
    _lib.check(_lib.hip.qsim_plan_relayout(n, arr, cnt, perm, ctypes.byref(passes), ctypes.byref(pred)))
    return list(perm), passes.value, pred.value


def gate_inverse(op):
    """The inverse of one GateOp (qsim_gate_inverse, host only): self-inverse types unchanged,
    S <-> Sdag, T <-> Tdag, rotations with the angle negated."""
    from .circuit import GateOp, GateType
    g, out = _lib.qsim_gate(), _lib.qsim_gate()
    g.type = int(op.type)
    g.nqubits = len(op.qubits)
    for j, q in enumerate(op.qubits):
        g.qubits[j] = q
    g.parameter = op.parameter
    _lib.check(_lib.hip.qsim_gate_inverse(ctypes.byref(g), ctypes.byref(out)))
    return GateOp(GateType(out.type), [out.qubits[j] for j in range(out.nqubits)], out.parameter)


def gradient_plan(circuit: Circuit, observable):
    """(parameterised gates, inverted non-parameterised segments, Pauli-sum apply passes) of the
    backward sweep Simulator.gradient would run (qsim_gradient_plan, host only)."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    terms, nterms = observable.to_abi(n)
    p, s, a = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.hip.qsim_gradient_plan(n, arr, cnt, terms, nterms, ctypes.byref(p), ctypes.byref(s),
                                           ctypes.byref(a)))
    return p.value, s.value, a.value


def parameterised_slots(circuit: Circuit):
    """Gate indices of the circuit's parameterised gates (Rx, Ry, Rz, CRY, CRZ) in gate order: slot
    k of BatchedSimulator.runSweep, i.e. column k of its angles, is gate parameterised_slots()[k]."""
    from .circuit import PARAMETRIC
    return [i for i, op in enumerate(circuit.getGates()) if op.type in PARAMETRIC]


def batch_sweep_plan(circuit: Circuit, batch_size: int, per_gate: bool = False) -> dict:
    """What BatchedSimulator.runSweep would do for this circuit on batch_size members, planned
    under the identity layout (qsim_batch_sweep_plan, host only): slots, passes, member_passes (the
    passes holding a member-dependent op; they run the pass interpreter), per_gate_launches,
    table_bytes (64 per slot and member) and fused (False: one launch per gate)."""
    arr, cnt = circuit.to_abi()
    info = (ctypes.c_int32 * 8)()
    flags = _lib.QSIM_BATCH_PER_GATE if per_gate else 0
    _lib.check(_lib.hip.qsim_batch_sweep_plan(circuit.getNumQubits(), int(batch_size), arr, cnt, flags, info))
    return {"slots": info[0], "passes": info[1], "member_passes": info[2], "per_gate_launches": info[3],
            "table_bytes": (info[4] & 0xffffffff) | ((info[5] & 0xffffffff) << 32), "fused": bool(info[6])}


def batch_gradient_plan(circuit: Circuit, batch_size: int, observable, per_gate: bool = False) -> dict:
    """What BatchedSimulator.gradientSweep would do for this circuit and observable on batch_size
    members (qsim_batch_gradient_plan, host only): slots, segments (inverted runs of non-parameterised
    gates the backward sweep applies; gates before the first parameter are never undone),
    apply_launches (of lambda = H phi), fused (False: the segments run gate by gate) and work_bytes
    (the two work ensembles: 2 x batch_size x 2^n x 16)."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    terms, nterms = observable.to_abi(n)
    info = (ctypes.c_int32 * 8)()
    flags = _lib.QSIM_BATCH_PER_GATE if per_gate else 0
    _lib.check(_lib.hip.qsim_batch_gradient_plan(n, int(batch_size), arr, cnt, terms, nterms, flags, info))
    return {"slots": info[0], "segments": info[1], "apply_launches": info[2], "fused": bool(info[3]),
            "work_bytes": (info[4] & 0xffffffff) | ((info[5] & 0xffffffff) << 32)}


def batch_overlap_plan(n: int, batch: int, other_batch=None) -> dict:
    """How BatchedSimulator.overlapMatrix cuts its work up for `batch` members of n qubits against
    other_batch members (None: the ensemble's own Gram matrix) (qsim_batch_overlap_plan, host
    only): mfma (False: the FMA kernel — one column, or QSIM_OVERLAP_MFMA=0), row_tiles,
    col_tiles, tiles (launched; the self case computes the upper triangle only), chunks (of
    K = 2^n; one work-group per tile and chunk) and scratch_bytes (chunks x tiles x 64 x 64 x 16).
    Everything but mfma depends on the arguments alone."""
    self_case = other_batch is None
    info = (ctypes.c_int32 * 8)()
    _lib.check(_lib.hip.qsim_batch_overlap_plan(int(n), int(batch), int(batch if self_case else other_batch),
                                                1 if self_case else 0, info))
    return {"mfma": bool(info[0]), "row_tiles": info[1], "col_tiles": info[2], "tiles": info[3], "chunks": info[4],
            "scratch_bytes": (info[5] & 0xffffffff) | ((info[6] & 0xffffffff) << 32)}


def _perm_arg(n: int, perm):
    if perm is None:
        return None
    if len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    return (ctypes.c_int32 * n)(*[int(p) for p in perm])


def pauli_rotation_plan(seq, perm=None):
    """(passes over the state, kernel launches) applyPauliRotations(seq) makes under the qubit
    layout perm (logical -> physical; None: identity): one pass per rotation with an X or Y factor,
    one per maximal run of consecutive Z/I-only rotations, one launch per 256 rotations of a run
    (qsim_pauli_rotation_plan, host only)."""
    n = seq.getNumQubits()
    rots, count = seq.to_abi(n)
    p, l = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.hip.qsim_pauli_rotation_plan(n, rots, count, _perm_arg(n, perm), ctypes.byref(p),
                                                 ctypes.byref(l)))
    return p.value, l.value


def marginal_plan(n: int, qubits, perm=None, rdm: bool = False) -> dict:
    """How marginalProbabilities (rdm: reducedDensityMatrix) of these qubits on an n-qubit state
    splits its work under the qubit layout perm (logical -> physical; None: identity): k_lo / k_hi
    selected physical positions below / above a work-group's contiguous run, slices of the
    unselected high positions, work-groups of the first kernel, scratch bytes of the partial sums
    and kernel launches (qsim_marginal_plan, host only).  The readers' argument checks."""
    qs = [int(q) for q in qubits]
    arr = (ctypes.c_int32 * len(qs))(*qs) if qs else None
    info = (ctypes.c_int32 * 8)()
    _lib.check(_lib.hip.qsim_marginal_plan(n, arr, len(qs), _perm_arg(n, perm), 1 if rdm else 0, info))
    return {"k_lo": info[0], "k_hi": info[1], "slices": info[2], "work_groups": info[3],
            "scratch_bytes": (info[4] & 0xffffffff) | (info[5] << 32), "launches": info[6]}


def dm_marginal_plan(n: int, qubits, perm=None, rdm: bool = False) -> dict:
    """How DensityMatrix.marginalProbabilities (rdm: reducedDensityMatrix) of these qubits lowers
    under the layout perm of the 2n index bits (logical -> physical, column bit q, row bit q + n;
    None: identity), host only (qsim_dm_marginal_plan).  Both readers evaluate
    out[o] = sum_b buf[G_out(o) | G_sum(b)], G(v) the OR of the generators at the set bits of v:
    out_gen, one address mask per bit of the out index (the matrix: o = a << k | a'), sum_gen, one per
    unlisted qubit; elements of rho read, work_groups of the first kernel, kernel launches,
    scratch_bytes of the partial sums, slices of the sum and thread_bits.  The readers' argument
    checks."""
    qs = [int(q) for q in qubits]
    arr = (ctypes.c_int32 * len(qs))(*qs) if qs else None
    info = (ctypes.c_int32 * 8)()
    out_gen = (ctypes.c_uint64 * max(1, 2 * len(qs)))()
    sum_gen = (ctypes.c_uint64 * max(1, n))()
    _lib.check(_lib.hip.qsim_dm_marginal_plan(n, arr, len(qs), _perm_arg(2 * n, perm), 1 if rdm else 0, info,
                                              out_gen, sum_gen))
    return {"elements": (info[0] & 0xffffffff) | (info[1] << 32), "work_groups": info[2], "launches": info[3],
            "scratch_bytes": info[4], "slices": info[5], "thread_bits": info[6],
            "out_gen": [int(g) for g in out_gen[:(2 if rdm else 1) * len(qs)]],
            "sum_gen": [int(g) for g in sum_gen[:n - len(qs)]]}


def hermitian_entropy(rho, renyi2: bool = False) -> float:
    """The entropy in bits of a density matrix (at most 64 x 64) by the C++ layer's host routine,
    the cyclic Jacobi sweep behind qsim::StateVector::entanglementEntropy (qsim_hermitian_entropy;
    host only)."""
    m = np.ascontiguousarray(rho, dtype=np.complex128)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("rho must be a square matrix")
    out = ctypes.c_double()
    _lib.raise_for(_lib.api.qsim_hermitian_entropy(m.ctypes.data_as(ctypes.c_void_p), m.shape[0],
                                                   1 if renyi2 else 0, ctypes.byref(out)),
                   lambda: "bad density matrix")
    return out.value


def pauli_gradient_plan(seq, observable, perm=None):
    """(steps of the backward sweep, Pauli-sum apply passes) of Simulator.pauliGradient under the
    qubit layout perm (qsim_pauli_gradient_plan, host only): every rotation its own step, no step
    when H = 0."""
    n = seq.getNumQubits()
    rots, count = seq.to_abi(n)
    terms, nterms = observable.to_abi(n)
    s, a = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.hip.qsim_pauli_gradient_plan(n, rots, count, terms, nterms, _perm_arg(n, perm),
                                                 ctypes.byref(s), ctypes.byref(a)))
    return s.value, a.value


def jit_build_relayout(circuit: Circuit) -> int:
    """Compile the circuit's relayout plan (qsim_jit_build_relayout, hipRTC for gfx950, no GPU
    needed); returns the code-object size in bytes."""
    arr, cnt = circuit.to_abi()
    n = ctypes.c_size_t(0)
    _lib.check(_lib.hip.qsim_jit_build_relayout(circuit.getNumQubits(), arr, cnt, ctypes.byref(n)))
    return n.value


def plan_share_host(circuit: Circuit, calls: int, copies: int = 0, state=None):
    """Play `calls` identical fused runs of the circuit through the engine's run-sharing
    bookkeeping, every launched pass executed on the host with the staged kernels' index math,
    flushed at the end (qsim_plan_share_host; no GPU).  Returns (state in logical order, circuit
    passes launched per call, gates pending after each call)."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    if state is None:
        st = np.zeros(1 << n, np.complex128)
        st[0] = 1.0
    else:
        st = np.array(state, dtype=np.complex128)
    st = np.ascontiguousarray(st)
    passes = np.zeros(max(1, calls), np.int32)
    pending = np.zeros(max(1, calls), np.int32)
    _lib.check(_lib.hip.qsim_plan_share_host(n, arr, cnt, copies, calls, st.ctypes.data_as(ctypes.c_void_p),
                                             passes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             pending.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return st, [int(x) for x in passes[:calls]], [int(x) for x in pending[:calls]]


def plan_share_info(circuit: Circuit, copies: int = 0):
    """(joint passes, single-run passes, highest copy per joint pass) of the joint plan a cycle of
    `copies` runs would execute (qsim_plan_share_info, host only); joint passes = 0 and an empty
    list when no cycle pays."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    joint, single = ctypes.c_int(0), ctypes.c_int(0)
    cap = 256
    pc = (ctypes.c_int32 * cap)()
    _lib.check(_lib.hip.qsim_plan_share_info(n, arr, cnt, copies, ctypes.byref(joint), ctypes.byref(single),
                                             pc, cap))
    return joint.value, single.value, [int(pc[k]) for k in range(min(cap, joint.value))]
