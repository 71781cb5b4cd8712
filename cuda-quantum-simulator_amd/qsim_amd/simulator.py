"""StateVector / Simulator / NoiseModel / BatchedSimulator over the C ABI.

Mirrors the reference C++ classes (include/StateVector.cuh:66-124, include/Simulator.hpp:53-85,
include/NoiseModel.cuh:46-297) with the same method names, argument meanings and exception
classes (ValueError ~ std::invalid_argument, IndexError ~ std::out_of_range,
RuntimeError ~ std::runtime_error).  All compute runs in the HIP engine; nothing here falls back
to the CPU.
"""
from __future__ import annotations

import ctypes
import enum
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .circuit import Circuit, GateOp, is_valid_qubit_count, MAX_QUBITS, MIN_QUBITS, PARAMETRIC
from .observable import PauliSum, trotter_sequence

_c = ctypes


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_c.c_void_p)


class RunMode(enum.IntEnum):
    PerGate = _lib.QSIM_RUN_PER_GATE
    Fused = _lib.QSIM_RUN_FUSED


def device_count() -> int:
    c = _c.c_int(0)
    _lib.check(_lib.hip.qsim_device_count(_c.byref(c)))
    return c.value


def set_device(device: int) -> None:
    """Device the calling thread's next objects are created on (one process per GPU)."""
    _lib.check(_lib.hip.qsim_set_device(int(device)))


def device_info(device: int = 0):
    name = _c.create_string_buffer(256)
    cus = _c.c_int(0)
    mem = _c.c_size_t(0)
    _lib.check(_lib.hip.qsim_device_info(device, name, 256, _c.byref(cus), _c.byref(mem)))
    return {"name": name.value.decode(), "cu_count": cus.value, "total_mem": mem.value}


def sequence_circuit(circuits, n: int) -> Circuit:
    """The gates of `circuits` (each of n qubits) in order, as one circuit."""
    seq = Circuit(n)
    for c in circuits:
        if c.getNumQubits() != n:
            raise ValueError("Circuit qubit count doesn't match simulator")
        seq.extend(c)
    return seq


class StateVector:
    def __init__(self, num_qubits: int, device: Optional[int] = None):
        if not is_valid_qubit_count(num_qubits):
            raise ValueError(f"Number of qubits must be between {MIN_QUBITS} and {MAX_QUBITS}")
        self._h = _c.c_void_p()
        if device is None:
            _lib.check(_lib.hip.qsim_state_create(num_qubits, _c.byref(self._h)))
        else:
            _lib.check(_lib.hip.qsim_state_create_on(device, num_qubits, _c.byref(self._h)))
        self._n = num_qubits
        self._rng: Optional[np.random.Generator] = None

    def __del__(self):
        self.close()

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _lib.hip.qsim_state_destroy(h)
            self._h = _c.c_void_p()

    @property
    def handle(self):
        return self._h

    def getNumQubits(self) -> int: return self._n
    def getSize(self) -> int: return 1 << self._n

    def initializeZero(self) -> None:
        _lib.check(_lib.hip.qsim_state_init_zero(self._h))

    def initializeBasis(self, idx: int) -> None:
        if idx < 0 or idx >= (1 << self._n):
            raise ValueError("Basis index out of range")
        _lib.check(_lib.hip.qsim_state_init_basis(self._h, idx))

    def devicePtr(self) -> int:
        p = _c.c_void_p()
        _lib.check(_lib.hip.qsim_state_device_ptr(self._h, _c.byref(p)))
        return p.value

    def stream(self) -> int:
        p = _c.c_void_p()
        _lib.check(_lib.hip.qsim_state_stream(self._h, _c.byref(p)))
        return p.value

    def synchronize(self) -> None:
        _lib.check(_lib.hip.qsim_state_sync(self._h))

    def toHost(self) -> np.ndarray:
        out = np.empty(1 << self._n, dtype=np.complex128)
        _lib.check(_lib.hip.qsim_state_to_host(self._h, _ptr(out)))
        return out

    def fromHost(self, amps) -> None:
        a = np.ascontiguousarray(amps, dtype=np.complex128)
        if a.shape != (1 << self._n,):
            raise ValueError("amplitude count does not match 2^n")
        _lib.check(_lib.hip.qsim_state_from_host(self._h, _ptr(a)))

    def getProbabilities(self) -> np.ndarray:
        out = np.empty(1 << self._n, dtype=np.float64)
        _lib.check(_lib.hip.qsim_state_probabilities(self._h, _ptr(out)))
        return out

    def getTotalProbability(self) -> float:
        t = _c.c_double()
        _lib.check(_lib.hip.qsim_state_total_probability(self._h, _c.byref(t)))
        return t.value

    def isNormalized(self, tolerance: float = 1e-10) -> bool:
        return abs(self.getTotalProbability() - 1.0) <= tolerance

    def assertNormalized(self, tolerance: float = 1e-10) -> None:
        t = self.getTotalProbability()
        if abs(t - 1.0) > tolerance:
            raise RuntimeError(f"State vector not normalized: total probability = {t}")

    def maxAbsDiff(self, other: "StateVector") -> float:
        """Larger per-component |a - b| against another state of the same size, computed on the
        device in the identity layout (qsim_state_max_abs_diff; the reference's 1e-12 per-component
        bar, tests/test_gpu_cpu_equivalence.cu:26, without a host copy)."""
        d = _c.c_double()
        _lib.check(_lib.hip.qsim_state_max_abs_diff(self._h, other._h, _c.byref(d)))
        return d.value

    def getDeviceMemoryBytes(self) -> int:
        """Device bytes this state owns now, the relayout plans' second buffer included."""
        b = _c.c_uint64()
        _lib.check(_lib.hip.qsim_state_memory_bytes(self._h, _c.byref(b)))
        return b.value

    def expectation(self, observable) -> float:
        """<psi|H|psi> of a PauliSum, reduced on the device where the state lies: no readback and
        no layout restore (qsim_state_expectation; no reference counterpart)."""
        terms, count = observable.to_abi(self._n)
        e = _c.c_double()
        _lib.check(_lib.hip.qsim_state_expectation(self._h, terms, count, _c.byref(e)))
        return e.value

    def _qubit_list(self, qubits, cap: int):
        qs = [int(q) for q in qubits]
        if len(qs) > cap:
            raise ValueError(f"at most {cap} qubits")
        return (_c.c_int32 * len(qs))(*qs) if qs else None, len(qs)

    def marginalProbabilities(self, qubits) -> np.ndarray:
        """The 2^k marginal probabilities of k <= 20 distinct qubits (any order; k = 0: the total
        probability): out[m] = sum of |psi_i|^2 over the i whose bit qubits[j] equals bit j of m.
        Qubit q is index bit q, the gates' and PauliSum's convention (not measure(q)'s big-endian
        one).  One streaming read where the state lies: no readback of the amplitudes, no layout
        restore, bitwise reproducible (qsim_state_marginal_probabilities; no reference
        counterpart).  ValueError on a duplicate or too many qubits, IndexError on a bad qubit."""
        arr, k = self._qubit_list(qubits, 20)
        out = np.empty(1 << k, dtype=np.float64)
        _lib.check(_lib.hip.qsim_state_marginal_probabilities(self._h, arr, k, _ptr(out)))
        return out

    def reducedDensityMatrix(self, qubits) -> np.ndarray:
        """rho_A of k <= 6 qubits as a 2^k x 2^k complex128 array, rho_A[a, a'] = sum_b psi(a, b)
        conj(psi(a', b)) with bit j of a = qubit qubits[j]; equal to its conjugate transpose
        bitwise, its diagonal the marginal (qsim_state_reduced_density_matrix).  Reads the state
        where it lies; errors as marginalProbabilities."""
        arr, k = self._qubit_list(qubits, 6)
        out = np.empty((1 << k, 1 << k), dtype=np.complex128)
        _lib.check(_lib.hip.qsim_state_reduced_density_matrix(self._h, arr, k, _ptr(out)))
        return out

    def subsystemPurity(self, qubits) -> float:
        """Tr rho_A^2 of the k <= 6 qubits."""
        rho = self.reducedDensityMatrix(qubits)
        return float(np.sum(rho.real ** 2 + rho.imag ** 2))

    def entanglementEntropy(self, qubits, renyi2: bool = False) -> float:
        """Von Neumann entropy of rho_A in bits, -sum l log2 l over numpy.linalg.eigvalsh(rho_A)
        (eigenvalues below 1e-300 contribute 0); renyi2: -log2 Tr rho_A^2 instead."""
        rho = self.reducedDensityMatrix(qubits)
        if renyi2:
            return float(-np.log2(np.sum(rho.real ** 2 + rho.imag ** 2)))
        ev = np.linalg.eigvalsh(rho)
        ev = ev[ev >= 1e-300]
        return float(-np.sum(ev * np.log2(ev)))

    def applyPauliSum(self, observable, dst: "StateVector") -> None:
        """dst = H |self> out of place on the device (qsim_state_apply_pauli_sum); dst takes this
        state's qubit layout.  ValueError when dst is self or of another size."""
        terms, count = observable.to_abi(self._n)
        _lib.check(_lib.hip.qsim_state_apply_pauli_sum(self._h, dst._h, terms, count))

    def applyPauliRotation(self, factors, theta: float) -> None:
        """exp(-i theta/2 P) in place, P the product of the factors {qubit: 'X' | 'Y' | 'Z'} (as
        PauliSum.add takes them; none: the global phase exp(-i theta/2)): one streaming pass over
        the state whatever the string's weight.  IndexError on a bad qubit, before anything is
        applied."""
        self.applyPauliRotations(PauliSum(self._n).add(theta, factors))

    def applyPauliRotations(self, seq) -> None:
        """A PauliSum read as an ordered sequence: term t is exp(-i coeff_t/2 P_t), applied in
        add() order where the state lies, no layout restore (qsim_state_apply_pauli_rotations; no
        reference counterpart).  Every rotation with an X or Y factor is one pass; a run of
        consecutive Z/I-only rotations shares one.  Asynchronous.  ValueError on a qubit-count
        mismatch."""
        rots, count = seq.to_abi(self._n)
        _lib.check(_lib.hip.qsim_state_apply_pauli_rotations(self._h, rots, count))

    def innerProduct(self, other: "StateVector") -> complex:
        """<self|other> by a fixed-order device reduction (qsim_state_inner_product)."""
        out = (_c.c_double * 2)()
        _lib.check(_lib.hip.qsim_state_inner_product(self._h, other._h, out))
        return complex(out[0], out[1])

    def probBitZero(self, bit: int) -> float:
        p = _c.c_double()
        _lib.check(_lib.hip.qsim_state_prob_bit_zero(self._h, bit, _c.byref(p)))
        return p.value

    def collapse(self, bit: int, result: int, scale: float) -> None:
        _lib.check(_lib.hip.qsim_state_collapse(self._h, bit, result, scale))

    def setSeed(self, seed: int) -> None:
        self._rng = np.random.default_rng(seed)

    def _uniforms(self, k: int) -> np.ndarray:
        rng = self._rng if self._rng is not None else np.random.default_rng()
        return rng.random(k)

    def measureBit(self, bit: int) -> int:
        if bit < 0 or bit >= self._n:
            raise ValueError(f"Qubit index {bit} out of range [0, {self._n - 1}]")
        p0 = self.probBitZero(bit)
        r = float(self._uniforms(1)[0])
        result = 0 if r < p0 else 1
        pr = p0 if result == 0 else 1.0 - p0
        if pr < 1e-15:
            raise RuntimeError(f"Measurement result {result} has zero probability")
        self.collapse(bit, result, 1.0 / np.sqrt(pr))
        return result

    def measure(self, qubit: int) -> int:
        """Reference semantics: big-endian index bit n-1-qubit (src/StateVector.cu:87-89, F2)."""
        if qubit < 0 or qubit >= self._n:
            raise ValueError(f"Qubit index {qubit} out of range [0, {self._n - 1}]")
        return self.measureBit(self._n - 1 - qubit)

    def sampleWith(self, uniforms) -> np.ndarray:
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.size <= 0:
            raise ValueError("n_shots must be positive")
        out = np.empty(u.size, dtype=np.int64)
        _lib.check(_lib.hip.qsim_state_sample(self._h, _ptr(u), int(u.size), _ptr(out)))
        return out

    def sample(self, n_shots: int) -> np.ndarray:
        if n_shots <= 0:
            raise ValueError("n_shots must be positive")
        return self.sampleWith(self._uniforms(n_shots))

    # -- direct gate application (kernel-level entry, Gates.cuh analogue)
    def applyGate(self, op: GateOp) -> None:
        g = _lib.qsim_gate()
        g.type = int(op.type)
        g.nqubits = len(op.qubits)
        for j, q in enumerate(op.qubits):
            g.qubits[j] = q
        g.parameter = op.parameter
        _lib.check(_lib.hip.qsim_apply_gate(self._h, _c.byref(g)))

    def applyMatrix1Q(self, target: int, m, controls: Sequence[int] = ()) -> None:
        mm = np.asarray(m, dtype=np.complex128).reshape(4)
        buf = (_c.c_double * 8)(*[v for z in mm for v in (z.real, z.imag)])
        ctl = (_c.c_int * max(1, len(controls)))(*controls)
        _lib.check(_lib.hip.qsim_apply_matrix1q(self._h, target, buf, ctl, len(controls)))

    def applyMatrix2Q(self, q0: int, q1: int, m, controls: Sequence[int] = ()) -> None:
        """General 4x4 on (q0, q1), row-major over (bit q1 << 1) | bit q0 (qsim_apply_matrix2q)."""
        mm = np.asarray(m, dtype=np.complex128).reshape(16)
        buf = (_c.c_double * 32)(*[v for z in mm for v in (z.real, z.imag)])
        ctl = (_c.c_int * max(1, len(controls)))(*controls)
        _lib.check(_lib.hip.qsim_apply_matrix2q(self._h, q0, q1, buf, ctl, len(controls)))

    def applyMatrix(self, targets: Sequence[int], m, controls: Sequence[int] = ()) -> None:
        """General 2^k x 2^k matrix, k = len(targets) <= 8, row-major; matrix-index bit j is
        qubit targets[j]; applied on the control == 1 subspace (qsim_apply_matrix)."""
        k = len(targets)
        mm = np.asarray(m, dtype=np.complex128)
        if k < 1 or k > 8 or mm.size != (1 << k) ** 2:
            raise ValueError("matrix must be 2^k x 2^k for 1 <= k <= 8 targets")
        buf = np.ascontiguousarray(mm.reshape(-1)).view(np.float64)
        tg = (_c.c_int * k)(*targets)
        ctl = (_c.c_int * max(1, len(controls)))(*controls)
        _lib.check(_lib.hip.qsim_apply_matrix(self._h, tg, k,
                                              buf.ctypes.data_as(_c.POINTER(_c.c_double)),
                                              ctl, len(controls)))

    def applyDiagonalLayer(self, gate_params, active_qubits: int) -> None:
        """applyFusedSingleQubitLayer (src/OptimizedGates.cu:344-382): gate_params[q][0] / [q][3]
        scale the bit-q = 0 / 1 amplitudes of every active qubit."""
        gp = np.ascontiguousarray(np.asarray(gate_params, dtype=np.complex128).reshape(-1, 4))
        if gp.shape[0] < self._n:
            raise ValueError("gate_params needs 4 entries per qubit")
        flat = gp.view(np.float64).reshape(-1)
        _lib.check(_lib.hip.qsim_apply_diagonal_layer(
            self._h, flat.ctypes.data_as(_c.POINTER(_c.c_double)), active_qubits))

    def run(self, circuit: Circuit, mode: RunMode = RunMode.Fused) -> None:
        arr, n = circuit.to_abi()
        _lib.check(_lib.hip.qsim_run(self._h, arr, n, int(mode)))

    def runSequence(self, circuits, mode: RunMode = RunMode.Fused) -> None:
        """Apply `circuits` one after the other as ONE engine run (no reference counterpart): the
        planner sees their gates together, so a pass may hold the end of one circuit and the
        start of the next — consecutive 100-gate W-HC circuits at 30 qubits plan into 2.5-2.75
        passes each instead of 4.  The same state as run() on each in turn."""
        seq = sequence_circuit(circuits, self._n)
        self.run(seq, mode)

    def perm(self):
        """Current logical -> physical qubit map (identity unless a fused run relabeled)."""
        p = (_c.c_int32 * self._n)()
        _lib.check(_lib.hip.qsim_state_perm(self._h, p))
        return list(p)

    def layoutInfo(self) -> dict:
        """The first-run layout decision: tile height of the fused runs, whether it was chosen by
        timing candidates on the device, whether the qubits are relabeled now."""
        h, c, r = _c.c_int(0), _c.c_int(0), _c.c_int(0)
        _lib.check(_lib.hip.qsim_state_layout_info(self._h, _c.byref(h), _c.byref(c), _c.byref(r)))
        rl = _c.c_int(0)
        _lib.check(_lib.hip.qsim_state_relayout(self._h, _c.byref(rl)))
        return {"tile_qubits": 6 + h.value, "calibrated": bool(c.value), "relabeled": bool(r.value),
                "relayout": bool(rl.value)}

    def restoreLayout(self) -> None:
        """Undo a relabeling now (the SWAP network every index-based reader runs first)."""
        _lib.check(_lib.hip.qsim_state_restore_layout(self._h))

    # -- profiling
    def profile(self, enable: bool = True) -> None:
        _lib.check(_lib.hip.qsim_state_profile(self._h, 1 if enable else 0))

    def profileReset(self) -> None:
        _lib.check(_lib.hip.qsim_state_profile_reset(self._h))

    def lastRunInfo(self):
        """(tile passes, passes run by circuit-specialised kernels) of the last fused run."""
        p, j = _c.c_int(0), _c.c_int(0)
        _lib.check(_lib.hip.qsim_state_last_run(self._h, _c.byref(p), _c.byref(j)))
        return p.value, j.value

    def profileStats(self):
        n = _c.c_int(0)
        _lib.check(_lib.hip.qsim_state_profile_count(self._h, _c.byref(n)))
        out = []
        for i in range(n.value):
            name = _c.create_string_buffer(64)
            ms, cnt, by = _c.c_double(), _c.c_int64(), _c.c_double()
            _lib.check(_lib.hip.qsim_state_profile_get(self._h, i, name, 64, _c.byref(ms),
                                                       _c.byref(cnt), _c.byref(by)))
            out.append({"name": name.value.decode(), "ms": ms.value, "launches": cnt.value,
                        "alg_bytes": by.value})
        return out


class Simulator:
    """Reference Simulator (src/Simulator.cu:22-189).  run() defaults to fused passes."""

    def __init__(self, num_qubits: int, mode: RunMode = RunMode.Fused, device: Optional[int] = None):
        self._state = StateVector(num_qubits, device)
        self._mode = RunMode(mode)

    @property
    def state(self) -> StateVector:
        return self._state

    def setRunMode(self, mode: RunMode) -> None: self._mode = RunMode(mode)
    def getRunMode(self) -> RunMode: return self._mode
    def setSeed(self, seed: int) -> None: self._state.setSeed(seed)
    def reset(self) -> None: self._state.initializeZero()

    def run(self, circuit: Circuit) -> None:
        if circuit.getNumQubits() != self._state.getNumQubits():
            raise ValueError("Circuit qubit count doesn't match simulator")
        self._state.run(circuit, self._mode)

    def runSequence(self, circuits) -> None:
        """run() of each circuit in turn, planned as one (StateVector.runSequence)."""
        self._state.runSequence(circuits, self._mode)

    def applyGate(self, op: GateOp) -> None: self._state.applyGate(op)
    def getStateVector(self) -> np.ndarray: return self._state.toHost()
    def getProbabilities(self) -> np.ndarray: return self._state.getProbabilities()

    def sample(self, n_shots: int) -> np.ndarray:
        if n_shots == 0:
            return np.empty(0, dtype=np.int64)
        return self._state.sample(n_shots)

    def measureQubit(self, qubit: int) -> int: return self._state.measure(qubit)
    # no reference counterpart: StateVector.expectation
    def expectation(self, observable) -> float: return self._state.expectation(observable)
    def marginalProbabilities(self, qubits) -> np.ndarray: return self._state.marginalProbabilities(qubits)
    def reducedDensityMatrix(self, qubits) -> np.ndarray: return self._state.reducedDensityMatrix(qubits)
    def subsystemPurity(self, qubits) -> float: return self._state.subsystemPurity(qubits)

    def entanglementEntropy(self, qubits, renyi2: bool = False) -> float:
        return self._state.entanglementEntropy(qubits, renyi2)

    def gradient(self, circuit: Circuit, observable, mode: RunMode = RunMode.Fused):
        """(value, gradient): runs `circuit` on the state as it is, as run() would in `mode`, then
        <psi|H|psi> and its derivative with respect to the angle of every gate (numpy array, one
        entry per gate, 0 for a gate without a parameter) by the adjoint method: one backward
        sweep on the device, one pass over two work states per angle, instead of two circuit runs
        per angle (qsim_state_gradient; no reference counterpart).  The state is left as run()
        leaves it."""
        n = self._state.getNumQubits()
        if circuit.getNumQubits() != n:
            raise ValueError("Circuit qubit count doesn't match simulator")
        arr, cnt = circuit.to_abi()
        terms, nterms = observable.to_abi(n)
        value = _c.c_double()
        grad = np.zeros(max(1, cnt), dtype=np.float64)
        _lib.check(_lib.hip.qsim_state_gradient(self._state.handle, arr, cnt, terms, nterms, int(mode),
                                                _c.byref(value), grad.ctypes.data_as(_c.POINTER(_c.c_double))))
        return value.value, grad[:cnt]

    # Pauli-string rotations (no reference counterpart): StateVector.applyPauliRotation(s)
    def applyPauliRotation(self, factors, theta: float) -> None:
        self._state.applyPauliRotation(factors, theta)

    def applyPauliRotations(self, seq) -> None: self._state.applyPauliRotations(seq)

    def evolve(self, H, time: float, steps: int = 1, order: int = 1) -> None:
        """The Trotter product for exp(-i H time) on the state as it is: nothing but
        applyPauliRotations(trotter_sequence(H, time, steps, order)) (observable.trotter_sequence
        defines both orders).  ValueError when steps < 1, order is not 1 or 2 or the qubit counts
        differ."""
        self.applyPauliRotations(trotter_sequence(H, time, steps, order))

    def pauliGradient(self, seq, observable):
        """(value, gradient): applies the rotation sequence `seq` (a PauliSum read in add() order,
        as applyPauliRotations does) to the state as it is, then <psi|H|psi> and its derivative
        with respect to the angle of every rotation (numpy array, one entry per term of seq) by
        the adjoint method: one backward sweep on the device, one fused pass over two work states
        per rotation (qsim_state_pauli_gradient).  The state is left as applyPauliRotations(seq)
        leaves it.  The angles are independent parameters here: a parameter shared between
        rotations (a QAOA gamma, a Trotter time) is the caller's chain rule over the returned
        gradient, d E / d gamma = sum_k grad[k] d theta_k / d gamma.  The work states are those
        of gradient() (releaseGradientBuffers frees them)."""
        n = self._state.getNumQubits()
        rots, count = seq.to_abi(n)
        terms, nterms = observable.to_abi(n)
        value = _c.c_double()
        grad = np.zeros(max(1, count), dtype=np.float64)
        _lib.check(_lib.hip.qsim_state_pauli_gradient(self._state.handle, rots, count, terms, nterms,
                                                      _c.byref(value), grad.ctypes.data_as(_c.POINTER(_c.c_double))))
        return value.value, grad[:count]

    def releaseGradientBuffers(self) -> None:
        """Free the two work states gradient() keeps on the state between calls."""
        _lib.check(_lib.hip.qsim_state_gradient_release(self._state.handle))

    def getNumQubits(self) -> int: return self._state.getNumQubits()
    def getStateSize(self) -> int: return self._state.getSize()
    def synchronize(self) -> None: self._state.synchronize()


class NoiseType(enum.IntEnum):
    Depolarizing = 0
    AmplitudeDamping = 1
    PhaseDamping = 2
    BitFlip = 3
    PhaseFlip = 4
    BitPhaseFlip = 5


class NoiseChannel:
    def __init__(self, type: NoiseType, qubits: Sequence[int], probability: float):
        self.type = NoiseType(type)
        self.qubits = list(qubits)
        self.probability = float(probability)


class NoiseModel:
    """Reference NoiseModel (src/NoiseModel.cu:24-101), incl. the empty-qubit 'global' form (F6)."""

    def __init__(self):
        self._ch: List[NoiseChannel] = []

    def _per(self, t, qubits, p):
        for q in qubits:
            self._ch.append(NoiseChannel(t, [q], p))

    def addDepolarizing(self, qubits_or_p, p=None):
        if p is None:
            self._ch.append(NoiseChannel(NoiseType.Depolarizing, [], qubits_or_p))
        else:
            self._per(NoiseType.Depolarizing, qubits_or_p, p)

    def addBitFlip(self, qubits_or_p, p=None):
        if p is None:
            self._ch.append(NoiseChannel(NoiseType.BitFlip, [], qubits_or_p))
        else:
            self._per(NoiseType.BitFlip, qubits_or_p, p)

    def addPhaseFlip(self, qubits_or_p, p=None):
        if p is None:
            self._ch.append(NoiseChannel(NoiseType.PhaseFlip, [], qubits_or_p))
        else:
            self._per(NoiseType.PhaseFlip, qubits_or_p, p)

    def addBitPhaseFlip(self, qubits_or_p, p=None):
        if p is None:
            self._ch.append(NoiseChannel(NoiseType.BitPhaseFlip, [], qubits_or_p))
        else:
            self._per(NoiseType.BitPhaseFlip, qubits_or_p, p)

    def addAmplitudeDamping(self, qubits_or_g, g=None):
        if g is None:
            self._ch.append(NoiseChannel(NoiseType.AmplitudeDamping, [], qubits_or_g))
        else:
            self._per(NoiseType.AmplitudeDamping, qubits_or_g, g)

    def addPhaseDamping(self, qubits_or_g, g=None):
        if g is None:
            self._ch.append(NoiseChannel(NoiseType.PhaseDamping, [], qubits_or_g))
        else:
            self._per(NoiseType.PhaseDamping, qubits_or_g, g)

    def addDepolarizingAll(self, n, p): self._per(NoiseType.Depolarizing, range(n), p)
    def addAmplitudeDampingAll(self, n, g): self._per(NoiseType.AmplitudeDamping, range(n), g)
    def addPhaseDampingAll(self, n, g): self._per(NoiseType.PhaseDamping, range(n), g)
    def getChannels(self) -> List[NoiseChannel]: return list(self._ch)
    def hasNoise(self) -> bool: return bool(self._ch)
    def clear(self) -> None: self._ch.clear()

    def to_abi(self):
        flat = [(c.type, q, c.probability) for c in self._ch for q in c.qubits]
        arr = (_lib.qsim_noise_channel * max(1, len(flat)))()
        for i, (t, q, p) in enumerate(flat):
            arr[i].type, arr[i].qubit, arr[i].probability = int(t), q, p
        return arr, len(flat)


class NoisySimulator:
    """Reference NoisySimulator (include/NoiseModel.cuh:139-214, src/NoiseModel.cu:320-651):
    Monte-Carlo noise on one state vector.  run() applies each gate and then every channel entry
    of the model (one per-pair noise pass each, noise.hip); global channels act on no qubit (F6).
    measureQubit measures index bit `qubit` (LSB-first, src/NoiseModel.cu:615-651) unlike
    StateVector.measure (F2).  Seeded from os.urandom like the reference's random_device."""

    def __init__(self, num_qubits: int, noise_model: Optional[NoiseModel] = None):
        self._state = StateVector(num_qubits)
        self._noise = noise_model or NoiseModel()
        self.setSeed(int.from_bytes(os.urandom(4), "little"))

    def setNoiseModel(self, nm: NoiseModel) -> None: self._noise = nm
    def getNoiseModel(self) -> NoiseModel: return self._noise

    def setSeed(self, seed: int) -> None:
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._counter = 0
        self._rng = np.random.default_rng(seed)

    @property
    def state(self) -> StateVector:
        return self._state

    def reset(self) -> None: self._state.initializeZero()

    def run(self, circuit: Circuit, mode: RunMode = RunMode.Fused) -> None:
        if circuit.getNumQubits() != self._state.getNumQubits():
            raise ValueError("Circuit qubit count doesn't match simulator")
        g, ng = circuit.to_abi()
        ch, nch = self._noise.to_abi()
        ctr = _c.c_uint64(self._counter)
        _lib.check(_lib.hip.qsim_noisy_run(self._state.handle, g, ng, ch, nch, self._seed,
                                           _c.byref(ctr), int(mode)))
        self._counter = ctr.value

    def applyGate(self, op: GateOp) -> None: self._state.applyGate(op)

    def applyNoise(self, channel: NoiseChannel) -> None:
        for q in channel.qubits:
            self.applyNoiseToQubit(channel.type, q, channel.probability)

    def applyNoiseToQubit(self, type: NoiseType, qubit: int, probability: float) -> None:
        _lib.check(_lib.hip.qsim_noise_apply(self._state.handle, int(type), qubit, probability,
                                             self._seed, self._counter))
        self._counter += 1

    def getStateVector(self) -> np.ndarray: return self._state.toHost()
    def getProbabilities(self) -> np.ndarray: return self._state.getProbabilities()

    def sample(self, n_shots: int) -> np.ndarray:
        """CDF + lower_bound like the reference (src/NoiseModel.cu:599-613), on the device."""
        if n_shots <= 0:
            return np.empty(0, dtype=np.int64)
        return self._state.sampleWith(self._rng.random(n_shots))

    def measureQubit(self, qubit: int) -> int:
        p0 = self._state.probBitZero(qubit)
        result = 0 if float(self._rng.random()) < p0 else 1
        kept = p0 if result == 0 else self._state.getTotalProbability() - p0
        self._state.collapse(qubit, result, 1.0 / np.sqrt(kept))
        return result

    # no reference counterpart: StateVector.expectation
    def expectation(self, observable) -> float: return self._state.expectation(observable)
    def marginalProbabilities(self, qubits) -> np.ndarray: return self._state.marginalProbabilities(qubits)
    def reducedDensityMatrix(self, qubits) -> np.ndarray: return self._state.reducedDensityMatrix(qubits)
    def subsystemPurity(self, qubits) -> float: return self._state.subsystemPurity(qubits)

    def entanglementEntropy(self, qubits, renyi2: bool = False) -> float:
        return self._state.entanglementEntropy(qubits, renyi2)

    def getNumQubits(self) -> int: return self._state.getNumQubits()
    def getStateSize(self) -> int: return self._state.getSize()
    def synchronize(self) -> None: self._state.synchronize()


class BatchedGateSet(enum.IntEnum):
    Full = _lib.QSIM_BATCH_FULL_GATESET
    Reference = _lib.QSIM_BATCH_REFERENCE_GATESET


class BatchedNoise(enum.IntEnum):
    """Reference (the default, as the reference behaves): the per-amplitude-pair depolarizing
    process after every gate (src/NoiseModel.cu:834-892; Depolarizing entries only, SURVEY
    F5/F7).  Physical (opt-in): one draw per trajectory, channel and gate (the Kraus channel on a
    pure-state trajectory), run as Pauli frames inside fused passes."""
    Physical = 0
    Reference = _lib.QSIM_BATCH_REFERENCE_NOISE


class BatchedSimulator:
    """Reference BatchedSimulator (src/NoiseModel.cu:653-972)."""

    def __init__(self, num_qubits: int, batch_size: int, noise_model: Optional[NoiseModel] = None,
                 gate_set: BatchedGateSet = BatchedGateSet.Full,
                 noise: BatchedNoise = BatchedNoise.Reference):
        self._h = _c.c_void_p()
        _lib.check(_lib.hip.qsim_batch_create(num_qubits, batch_size, _c.byref(self._h)))
        self._n, self._b = num_qubits, batch_size
        self._noise = noise_model or NoiseModel()
        self._gate_set = BatchedGateSet(gate_set)
        self._noise_sem = BatchedNoise(noise)
        self._rng = np.random.default_rng()

    def __del__(self):
        self.close()

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _lib.hip.qsim_batch_destroy(h)
            self._h = _c.c_void_p()

    def setNoiseModel(self, nm: NoiseModel) -> None: self._noise = nm
    def setGateSet(self, g: BatchedGateSet) -> None: self._gate_set = BatchedGateSet(g)
    def setNoiseSemantics(self, m: BatchedNoise) -> None: self._noise_sem = BatchedNoise(m)

    def setReferenceCompatible(self) -> None:
        """Both reference behaviours: gate set X/Y/Z/H/CNOT and per-pair depolarizing noise."""
        self._gate_set = BatchedGateSet.Reference
        self._noise_sem = BatchedNoise.Reference

    def setSeed(self, seed: int) -> None:
        self._rng = np.random.default_rng(seed)
        _lib.check(_lib.hip.qsim_batch_set_seed(self._h, seed))

    def setTrajectoryOffset(self, first: int) -> None:
        """This object's trajectories are [first, first + batch_size) of a larger ensemble: noise
        draws are keyed by the global trajectory index, so shards of an ensemble (one per GPU)
        reproduce the single-object run exactly (qsim_batch_set_trajectory_offset)."""
        _lib.check(_lib.hip.qsim_batch_set_trajectory_offset(self._h, int(first)))

    def reset(self) -> None: _lib.check(_lib.hip.qsim_batch_reset(self._h))

    def run(self, circuit: Circuit, per_gate: bool = False) -> None:
        """per_gate: one kernel per gate and one Pauli pass per noisy step (the reference's
        structure) instead of fused passes under Pauli frames; identical trajectories."""
        if circuit.getNumQubits() != self._n:
            raise ValueError("Circuit qubit count doesn't match simulator")
        g, ng = circuit.to_abi()
        ch, nch = self._noise.to_abi()
        flags = int(self._gate_set) | int(self._noise_sem) | \
            (_lib.QSIM_BATCH_PER_GATE if per_gate else 0)
        _lib.check(_lib.hip.qsim_batch_run(self._h, g, ng, ch, nch, flags))

    def runSweep(self, circuit: Circuit, angles, per_gate: bool = False) -> None:
        """One circuit, one angle set per member (qsim_batch_run_sweep; no reference counterpart).
        angles: array-like of shape (B, P), or (P,) given to every member; P = the circuit's
        parameterised gates (Rx, Ry, Rz, CRY, CRZ) in gate order (plan.parameterised_slots): member
        t applies its k-th one with angles[t, k], the angles stored in the circuit are ignored.
        Noise-free, from whatever every member holds; one planned run whatever the angles.
        ValueError: a shape mismatch, a non-empty noise model, the reference gate set or the
        reference noise semantics selected (construct with noise=BatchedNoise.Physical)."""
        a, n_slots = self._sweep_angles(circuit, angles)
        g, ng = circuit.to_abi()
        flags = _lib.QSIM_BATCH_PER_GATE if per_gate else 0
        _lib.check(_lib.hip.qsim_batch_run_sweep(self._h, g, ng, a.ctypes.data_as(_c.POINTER(_c.c_double)),
                                                 n_slots, flags))

    def _sweep_angles(self, circuit: Circuit, angles):
        """The checks of a sweep made on this side of the ABI; returns the contiguous (B, P) angles
        and P."""
        if circuit.getNumQubits() != self._n:
            raise ValueError("Circuit qubit count doesn't match simulator")
        if self._noise.to_abi()[1] > 0:
            raise ValueError("runSweep is noise-free: the noise model must be empty")
        if self._gate_set != BatchedGateSet.Full or self._noise_sem != BatchedNoise.Physical:
            raise ValueError("runSweep needs the full gate set and the physical noise semantics")
        n_slots = sum(1 for op in circuit.getGates() if op.type in PARAMETRIC)
        a = np.asarray(angles, dtype=np.float64)
        if a.ndim == 1:
            a = np.broadcast_to(a, (self._b, a.shape[0]))
        if a.ndim != 2 or a.shape != (self._b, n_slots):
            raise ValueError(f"angles must have shape ({self._b}, {n_slots}) or ({n_slots},)")
        return np.ascontiguousarray(a), n_slots

    def gradientSweep(self, circuit: Circuit, angles, observable, per_gate: bool = False):
        """runSweep(circuit, angles, per_gate), then every member's energy and its gradient by the
        adjoint method (qsim_batch_gradient_sweep; no reference counterpart): returns (values[B],
        grads[B, P]), grads[t, k] = d values[t] / d angles[t, k] — indexed by slot like angles, not
        by gate as Simulator.gradient.  One forward run and one backward sweep over two work
        ensembles of the batch's size, which stay on the object until releaseGradientBuffers().
        The members are left exactly as runSweep leaves them; values are what getExpectations then
        returns.  angles and the ValueErrors are those of runSweep."""
        a, n_slots = self._sweep_angles(circuit, angles)
        g, ng = circuit.to_abi()
        terms, nterms = observable.to_abi(self._n)
        values = np.zeros(self._b, dtype=np.float64)
        grads = np.zeros((self._b, n_slots), dtype=np.float64)
        dp = _c.POINTER(_c.c_double)
        flags = _lib.QSIM_BATCH_PER_GATE if per_gate else 0
        _lib.check(_lib.hip.qsim_batch_gradient_sweep(self._h, g, ng, a.ctypes.data_as(dp), n_slots, terms, nterms,
                                                      flags, values.ctypes.data_as(dp), grads.ctypes.data_as(dp)))
        return values, grads

    def releaseGradientBuffers(self) -> None:
        """Free the work ensembles of gradientSweep (the next call allocates them again)."""
        _lib.check(_lib.hip.qsim_batch_gradient_release(self._h))

    def synchronize(self) -> None: _lib.check(_lib.hip.qsim_batch_sync(self._h))

    def getAverageProbabilities(self) -> np.ndarray:
        out = np.empty(1 << self._n, dtype=np.float64)
        _lib.check(_lib.hip.qsim_batch_avg_probabilities(self._h, _ptr(out)))
        return out

    def getProbabilities(self, t: int) -> np.ndarray:
        if t < 0 or t >= self._b:
            raise IndexError("Invalid trajectory index")
        out = np.empty(1 << self._n, dtype=np.float64)
        _lib.check(_lib.hip.qsim_batch_traj_probabilities(self._h, t, _ptr(out)))
        return out

    def getStateVector(self, t: int) -> np.ndarray:
        if t < 0 or t >= self._b:
            raise IndexError("Invalid trajectory index")
        out = np.empty(1 << self._n, dtype=np.complex128)
        _lib.check(_lib.hip.qsim_batch_traj_state(self._h, t, _ptr(out)))
        return out

    def perm(self):
        """Current logical -> physical qubit map inside every trajectory (qsim_batch_perm)."""
        p = (_c.c_int32 * self._n)()
        _lib.check(_lib.hip.qsim_batch_perm(self._h, p))
        return list(p)

    def getExpectations(self, observable) -> np.ndarray:
        """Per-trajectory <psi_t|H|psi_t> of a PauliSum, reduced on the device
        (qsim_batch_expectation; no reference counterpart)."""
        terms, count = observable.to_abi(self._n)
        out = np.empty(self._b, dtype=np.float64)
        _lib.check(_lib.hip.qsim_batch_expectation(self._h, terms, count,
                                                   out.ctypes.data_as(_c.POINTER(_c.c_double))))
        return out

    def overlapMatrix(self, other: Optional["BatchedSimulator"] = None) -> np.ndarray:
        """G[i, j] = <psi_i|phi_j> over this ensemble's members and other's, complex128 (B, B'),
        computed where the members lie (qsim_batch_overlaps; no reference counterpart).  other
        None (or self): the ensemble's own Gram matrix, Hermitian bitwise with +0 imaginary parts
        on the diagonal, read under whatever layout the last run left (perm() and the amplitudes
        stay as they are).  With another ensemble the two are read in place when their layouts
        agree, else both layouts are restored first.  Bitwise reproducible; QSIM_OVERLAP_MFMA=0
        selects the FMA kernel (cross-check).  ValueError: different qubit counts."""
        cross = other is not None and other is not self
        out = np.empty((self._b, other._b if cross else self._b), dtype=np.complex128)
        _lib.check(_lib.hip.qsim_batch_overlaps(self._h, other._h if cross else None,
                                                out.ctypes.data_as(_c.POINTER(_c.c_double))))
        return out

    def kernelMatrix(self, other: Optional["BatchedSimulator"] = None) -> np.ndarray:
        """|overlapMatrix(other)|^2, float64: the fidelity kernel of the members.  Over a noisy
        trajectory ensemble its mean is the purity Tr rho^2 of the average state."""
        g = self.overlapMatrix(other)
        return g.real * g.real + g.imag * g.imag

    def overlapsWith(self, state) -> np.ndarray:
        """<psi_t|s> for every member t, complex128 (B,) (qsim_batch_state_overlaps): one streaming
        pass over the ensemble.  state: a StateVector, a Simulator, or a host array of 2^n
        amplitudes (uploaded into a temporary StateVector)."""
        tmp = None
        if isinstance(state, Simulator):
            state = state.state
        elif not isinstance(state, StateVector):
            tmp = StateVector(self._n)
            tmp.fromHost(state)
            state = tmp
        out = np.empty(self._b, dtype=np.complex128)
        try:
            _lib.check(_lib.hip.qsim_batch_state_overlaps(self._h, state._h,
                                                          out.ctypes.data_as(_c.POINTER(_c.c_double))))
        finally:
            if tmp is not None:
                tmp.close()
        return out

    def getAverageExpectation(self, observable) -> float:
        """Host mean of getExpectations, added in index order."""
        total = 0.0
        for v in self.getExpectations(observable):
            total += float(v)
        return total / self._b

    def sampleWith(self, uniforms: np.ndarray) -> np.ndarray:
        """Device sampling with given uniforms, shape (B, shots) trajectory-major; returns the
        (B, shots) outcomes (lower_bound over each trajectory's CDF, 2^n past its end)."""
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.ndim != 2 or u.shape[0] != self._b:
            raise ValueError("uniforms must have shape (batch_size, shots)")
        out = np.empty(u.shape, dtype=np.int64)
        _lib.check(_lib.hip.qsim_batch_sample(self._h, _ptr(u), int(u.shape[1]), _ptr(out)))
        return out

    def _draw(self, n_shots: int) -> np.ndarray:
        if n_shots < 0:
            raise ValueError("n_shots must be non-negative")
        # the reference draws shot by shot inside the trajectory loop (NoiseModel.cu:944-954)
        return self._rng.random((self._b, n_shots))

    def sample(self, n_shots: int) -> np.ndarray:
        """[shot][trajectory] outcomes: per-trajectory CDF + lower_bound (NoiseModel.cu:938-957),
        on the device."""
        return np.ascontiguousarray(self.sampleWith(self._draw(n_shots)).T)

    def getHistogram(self, n_shots: int) -> np.ndarray:
        """Counts over every trajectory and shot, out-of-range outcomes skipped
        (NoiseModel.cu:959-972); sampling and counting on the device."""
        u = np.ascontiguousarray(self._draw(n_shots))
        hist = np.empty(1 << self._n, dtype=np.int64)
        _lib.check(_lib.hip.qsim_batch_histogram(self._h, _ptr(u), int(n_shots), _ptr(hist)))
        return hist

    def getNumQubits(self) -> int: return self._n
    def getBatchSize(self) -> int: return self._b
    def getTotalMemoryBytes(self) -> int: return self._b * (1 << self._n) * 16

    def lastRunInfo(self):
        """(tile passes, passes run by circuit-specialised kernels) of the last fused run."""
        p, j = _c.c_int(0), _c.c_int(0)
        _lib.check(_lib.hip.qsim_batch_last_run(self._h, _c.byref(p), _c.byref(j)))
        return p.value, j.value

    def profile(self, enable: bool = True) -> None:
        _lib.check(_lib.hip.qsim_batch_profile(self._h, 1 if enable else 0))

    def profileStats(self):
        n = _c.c_int(0)
        _lib.check(_lib.hip.qsim_batch_profile_count(self._h, _c.byref(n)))
        out = []
        for i in range(n.value):
            name = _c.create_string_buffer(64)
            ms, cnt, by = _c.c_double(), _c.c_int64(), _c.c_double()
            _lib.check(_lib.hip.qsim_batch_profile_get(self._h, i, name, 64, _c.byref(ms),
                                                       _c.byref(cnt), _c.byref(by)))
            out.append({"name": name.value.decode(), "ms": ms.value, "launches": cnt.value,
                        "alg_bytes": by.value})
        return out
