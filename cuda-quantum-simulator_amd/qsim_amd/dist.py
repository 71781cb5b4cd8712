"""Sharded multi-GPU state (qsim_dist_* of include/qsim_hip.h).

One process per GPU: `DistributedSimulator(n, rank, world, unique_id, device)`; rank 0 creates the
RCCL unique id with `unique_id()` and the launcher (torch.distributed over gloo, see
dist_bench.py) broadcasts it.  `DistributedSimulator.virtual(n, world)` keeps all `world` shards in
one process on one GPU (exchanges by device copies) — the same planner and kernels, used to test
the sharded path on a single GPU.  `plan()` exposes the host planner (no GPU needed).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .circuit import Circuit
from .observable import PauliSum, trotter_sequence

_c = ctypes
UNIQUE_ID_BYTES = 128


def unique_id() -> bytes:
    buf = _c.create_string_buffer(UNIQUE_ID_BYTES)
    _lib.check(_lib.hip.qsim_dist_unique_id(buf))
    return buf.raw


class DistributedSimulator:
    def __init__(self, num_qubits: int, rank: int = 0, world: int = 1,
                 uid: Optional[bytes] = None, device: int = 0, _virtual: bool = False):
        self._h = _c.c_void_p()
        self._n, self._world, self._rank = num_qubits, world, rank
        self._virtual = _virtual
        if _virtual:
            _lib.check(_lib.hip.qsim_dist_create_virtual(num_qubits, world, device,
                                                         _c.byref(self._h)))
        else:
            if uid is None:
                if world != 1:
                    raise ValueError("a unique id from rank 0 is required for world > 1")
                uid = unique_id()
            buf = _c.create_string_buffer(uid, UNIQUE_ID_BYTES)
            _lib.check(_lib.hip.qsim_dist_create(num_qubits, rank, world, buf, device,
                                                 _c.byref(self._h)))

    @classmethod
    def virtual(cls, num_qubits: int, world: int, device: int = 0,
                rccl: bool = False) -> "DistributedSimulator":
        """`world` shards in this process on one GPU.  rccl: move the slabs with ncclSend /
        ncclRecv pairs to rank 0 of a world-1 communicator (qsim_dist_virtual_rccl) instead of
        device copies — the multi-rank RCCL call sequence, on one GPU."""
        sim = cls(num_qubits, 0, world, None, device, _virtual=True)
        if rccl:
            buf = _c.create_string_buffer(unique_id(), UNIQUE_ID_BYTES)
            _lib.check(_lib.hip.qsim_dist_virtual_rccl(sim._h, buf))
        return sim

    @classmethod
    def hosted(cls, num_qubits: int, rank: int, world: int, transport, device: int = 0
               ) -> "DistributedSimulator":
        """One shard per process, as the RCCL path, but every transfer goes through the Python
        callable `transport(posts)` (qsim_dist_create_hosted): `posts` is a list of
        (peer, send, recv) with `send` / `recv` memoryviews of host staging (either may be None
        for a one-sided post); the k-th post naming q must meet q's k-th post naming this rank.
        An exception in `transport` fails the engine call.  Lets several rank processes share
        one GPU (tests: the per-rank planning and exchange of the multi-rank path without RCCL)."""
        sim = cls.__new__(cls)
        sim._h = _c.c_void_p()
        sim._n, sim._world, sim._rank, sim._virtual = num_qubits, world, rank, False
        sim._transport_error = None

        def cb(_ctx, posts, count):
            try:
                items = []
                for i in range(count):
                    p = posts[i]
                    snd = (memoryview((_c.c_char * p.bytes).from_address(p.send)).cast("B")
                           if p.send else None)
                    rcv = (memoryview((_c.c_char * p.bytes).from_address(p.recv)).cast("B")
                           if p.recv else None)
                    items.append((p.peer, snd, rcv))
                transport(items)
                return 0
            except BaseException as e:  # noqa: BLE001 — reported through the engine's error
                sim._transport_error = e
                return 1
        sim._cb = _lib.qsim_dist_transport_fn(cb)  # kept alive with the object
        _lib.check(_lib.hip.qsim_dist_create_hosted(num_qubits, rank, world, device, sim._cb, None,
                                                    _c.byref(sim._h)))
        return sim

    def __del__(self):
        self.close()

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _lib.hip.qsim_dist_destroy(h)
            self._h = _c.c_void_p()

    def getNumQubits(self) -> int: return self._n
    def getWorldSize(self) -> int: return self._world

    def run(self, circuit: Circuit, fused: bool = True) -> None:
        if circuit.getNumQubits() != self._n:
            raise ValueError("Circuit qubit count doesn't match simulator")
        arr, cnt = circuit.to_abi()
        _lib.check(_lib.hip.qsim_dist_run(self._h, arr, cnt,
                                          _lib.QSIM_RUN_FUSED if fused else _lib.QSIM_RUN_PER_GATE))

    def runSequence(self, circuits, fused: bool = True) -> None:
        """run() of each circuit in turn as ONE sharded run (Simulator.runSequence): passes and
        global<->local remaps are planned over all of their gates."""
        from .simulator import sequence_circuit
        self.run(sequence_circuit(circuits, self._n), fused)

    def synchronize(self) -> None: _lib.check(_lib.hip.qsim_dist_sync(self._h))

    def barrier(self) -> None:
        """Collective: this rank's engine idle, then a one-value all-reduce over the communicator
        (the ranks leave within its latency of one another: bench.py's per-step timing barrier)."""
        _lib.check(_lib.hip.qsim_dist_barrier(self._h))

    def overlappedRemaps(self) -> int:
        """Remaps of the last run that were split in halves overlapping local work."""
        v = _c.c_int(0)
        _lib.check(_lib.hip.qsim_dist_overlapped(self._h, _c.byref(v)))
        return v.value
    def carriedRuns(self) -> int:
        """Runs whose first step merged the previous run's carried last step (QSIM_DIST_CARRY=1,
        experimental)."""
        v = _c.c_int(0)
        _lib.check(_lib.hip.qsim_dist_carried_runs(self._h, _c.byref(v)))
        return v.value
    def fusedRemaps(self) -> int:
        """Exchanges of the last run whose pack / unpack ran inside the local passes (the pass
        before stored into the slab layout, the step after loaded from it), summed over shards."""
        v = _c.c_int(0)
        _lib.check(_lib.hip.qsim_dist_fused_remaps(self._h, _c.byref(v)))
        return v.value

    def remapBytes(self) -> float:
        """Bytes this rank sent in the last run's remaps (it received as many)."""
        v = _c.c_double(0)
        _lib.check(_lib.hip.qsim_dist_remap_bytes(self._h, _c.byref(v)))
        return v.value

    def reset(self) -> None: _lib.check(_lib.hip.qsim_dist_reset(self._h))

    def perm(self) -> List[int]:
        p = (_c.c_int32 * self._n)()
        _lib.check(_lib.hip.qsim_dist_perm(self._h, p))
        return list(p)

    def getStateVector(self) -> Optional[np.ndarray]:
        """Full logical-order state on rank 0 (collective); None on other ranks."""
        out = np.empty(1 << self._n, dtype=np.complex128)
        root = self._virtual or self._rank == 0
        _lib.check(_lib.hip.qsim_dist_gather_state(self._h, out.ctypes.data_as(_c.c_void_p)
                                                   if root else None))
        return out if root else None

    def localState(self) -> np.ndarray:
        shards = self._world if self._virtual else 1
        out = np.empty(shards << (self._n - (self._world.bit_length() - 1)), dtype=np.complex128)
        _lib.check(_lib.hip.qsim_dist_local_state(self._h, out.ctypes.data_as(_c.c_void_p)))
        return out

    def getTotalProbability(self) -> float:
        t = _c.c_double()
        _lib.check(_lib.hip.qsim_dist_total_probability(self._h, _c.byref(t)))
        return t.value

    def probBitZero(self, q: int) -> float:
        t = _c.c_double()
        _lib.check(_lib.hip.qsim_dist_prob_bit_zero(self._h, q, _c.byref(t)))
        return t.value

    # -- readout without a gather of amplitudes (collective: every rank calls with the same
    #    arguments; the semantics are StateVector's)
    def getProbabilities(self) -> Optional[np.ndarray]:
        """|a_i|^2 in logical index order on rank 0 (collective); None on other ranks."""
        root = self._virtual or self._rank == 0
        out = np.empty(1 << self._n, dtype=np.float64) if root else None
        _lib.check(_lib.hip.qsim_dist_probabilities(self._h, out.ctypes.data_as(_c.c_void_p)
                                                    if root else None))
        return out

    def expectation(self, observable) -> float:
        """<psi|H|psi> of a PauliSum on the sharded state, the same float on every rank
        (qsim_dist_expectation): each shard is read where it lies — no gather, no remap, perm()
        unchanged; a string with X or Y on a qubit that sits on a rank position moves half a
        shard between the two ranks it pairs."""
        terms, count = observable.to_abi(self._n)
        e = _c.c_double()
        _lib.check(_lib.hip.qsim_dist_expectation(self._h, terms, count, _c.byref(e)))
        return e.value

    # -- readout of a subset of qubits where the shards lie (collective; StateVector's conventions:
    #    qubit q is index bit q, bit j of an output index is qubits[j]; ValueError on a duplicate
    #    or too many qubits, IndexError on a bad qubit).  The same floats on every rank.
    def _qubit_list(self, qubits, cap: int):
        qs = [int(q) for q in qubits]
        if len(qs) > cap:
            raise ValueError(f"at most {cap} qubits")
        return (_c.c_int32 * len(qs))(*qs) if qs else None, len(qs)

    def marginalProbabilities(self, qubits) -> np.ndarray:
        """The 2^k marginal probabilities of k <= 20 distinct qubits (k = 0: the total probability)
        of the sharded state (qsim_dist_marginal_probabilities): every shard bins its local
        positions and one all-reduce of 2^k doubles adds the ranks — no gather, no remap, perm()
        unchanged, bitwise reproducible."""
        arr, k = self._qubit_list(qubits, 20)
        out = np.empty(1 << k, dtype=np.float64)
        _lib.check(_lib.hip.qsim_dist_marginal_probabilities(self._h, arr, k,
                                                             out.ctypes.data_as(_c.c_void_p)))
        return out

    def reducedDensityMatrix(self, qubits) -> np.ndarray:
        """rho_A of k <= 6 qubits as a 2^k x 2^k complex128 array, bitwise equal to its conjugate
        transpose (qsim_dist_reduced_density_matrix).  A selected qubit that sits on a rank
        position pairs ranks: each of the 2^k_rank - 1 steps moves half a shard each way (a whole
        one when the top local position is selected too)."""
        arr, k = self._qubit_list(qubits, 6)
        out = np.empty((1 << k, 1 << k), dtype=np.complex128)
        _lib.check(_lib.hip.qsim_dist_reduced_density_matrix(self._h, arr, k,
                                                             out.ctypes.data_as(_c.c_void_p)))
        return out

    def subsystemPurity(self, qubits) -> float:
        """Tr rho_A^2 of the k <= 6 qubits."""
        rho = self.reducedDensityMatrix(qubits)
        return float(np.sum(rho.real ** 2 + rho.imag ** 2))

    def entanglementEntropy(self, qubits, renyi2: bool = False) -> float:
        """Von Neumann entropy of rho_A in bits (the host Jacobi routine plan.hermitian_entropy;
        eigenvalues below 1e-300 contribute 0); renyi2: -log2 Tr rho_A^2 instead."""
        from .plan import hermitian_entropy
        return hermitian_entropy(self.reducedDensityMatrix(qubits), renyi2)

    def gradient(self, circuit: Circuit, observable, fused: bool = True):
        """(value, gradient) on the sharded state (collective, qsim_dist_gradient): runs `circuit`
        as run() would, then <psi|H|psi> and its derivative with respect to the angle of every
        gate (numpy array, one entry per gate, 0 for a gate without a parameter) by one backward
        sweep over two sharded work states.  A rotation whose target sits on a rank position
        pairs each rank with one peer (two whole-shard transfers) instead of a remap.  The state,
        perm() and the run counters are left as run() alone leaves them; every rank gets the
        same floats."""
        if circuit.getNumQubits() != self._n:
            raise ValueError("Circuit qubit count doesn't match simulator")
        arr, cnt = circuit.to_abi()
        terms, nterms = observable.to_abi(self._n)
        value = _c.c_double()
        grad = np.zeros(max(1, cnt), dtype=np.float64)
        _lib.check(_lib.hip.qsim_dist_gradient(
            self._h, arr, cnt, terms, nterms, _lib.QSIM_RUN_FUSED if fused else _lib.QSIM_RUN_PER_GATE,
            _c.byref(value), grad.ctypes.data_as(_c.POINTER(_c.c_double))))
        return value.value, grad[:cnt]

    # Pauli-string rotations on the sharded state (collective; Simulator's signatures and exceptions)
    def applyPauliRotation(self, factors, theta: float) -> None:
        """exp(-i theta/2 P) in place, P the product of the factors {qubit: 'X' | 'Y' | 'Z'} (as
        PauliSum.add takes them; none: the global phase).  IndexError on a bad qubit, before
        anything is applied."""
        self.applyPauliRotations(PauliSum(self._n).add(theta, factors))

    def applyPauliRotations(self, seq) -> None:
        """A PauliSum read as an ordered sequence: term t is exp(-i coeff_t/2 P_t), applied in
        add() order where the shards lie (qsim_dist_apply_pauli_rotations): no remap, perm()
        unchanged.  A run of consecutive Z/I-only rotations is one pass per shard; a rotation with
        X or Y factors on local positions only is one pass per shard; one with an X or Y factor on
        a qubit that sits on a rank position pairs each rank with one peer and moves a whole
        shard each way.  ValueError on a qubit-count mismatch."""
        rots, count = seq.to_abi(self._n)
        _lib.check(_lib.hip.qsim_dist_apply_pauli_rotations(self._h, rots, count))

    def evolve(self, H, time: float, steps: int = 1, order: int = 1) -> None:
        """The Trotter product for exp(-i H time) on the state as it is: nothing but
        applyPauliRotations(trotter_sequence(H, time, steps, order)).  ValueError when steps < 1,
        order is not 1 or 2 or the qubit counts differ."""
        self.applyPauliRotations(trotter_sequence(H, time, steps, order))

    def pauliGradient(self, seq, observable):
        """(value, gradient) as Simulator.pauliGradient, on the sharded state (collective,
        qsim_dist_pauli_gradient): applies `seq` as applyPauliRotations does, then <psi|H|psi> and
        its derivative with respect to the angle of every rotation by one backward sweep over the
        two sharded work states of gradient() (releaseGradientBuffers frees them).  The state is
        left as applyPauliRotations(seq) leaves it; every rank gets the same floats."""
        rots, count = seq.to_abi(self._n)
        terms, nterms = observable.to_abi(self._n)
        value = _c.c_double()
        grad = np.zeros(max(1, count), dtype=np.float64)
        _lib.check(_lib.hip.qsim_dist_pauli_gradient(self._h, rots, count, terms, nterms, _c.byref(value),
                                                     grad.ctypes.data_as(_c.POINTER(_c.c_double))))
        return value.value, grad[:count]

    def releaseGradientBuffers(self) -> None:
        """Free the two work shards per rank gradient() keeps between calls."""
        _lib.check(_lib.hip.qsim_dist_gradient_release(self._h))

    def gradientMemoryBytes(self) -> int:
        """Device bytes of the gradient work shards this process holds now."""
        v = _c.c_uint64(0)
        _lib.check(_lib.hip.qsim_dist_gradient_memory_bytes(self._h, _c.byref(v)))
        return v.value

    def setSeed(self, seed: int) -> None:
        """Seed this rank's generator (StateVector.setSeed).  sample / measure* draw on rank 0 and
        broadcast, so the shots are rank 0's; with the same seed on every rank all generators
        also stay in step."""
        self._rng = np.random.default_rng(seed)

    def _uniforms(self, k: int) -> np.ndarray:
        rng = getattr(self, "_rng", None)
        u = np.ascontiguousarray((rng if rng is not None else np.random.default_rng()).random(k))
        _lib.check(_lib.hip.qsim_dist_bcast(self._h, u.ctypes.data_as(_c.c_void_p), u.size))
        return u

    def sampleWith(self, uniforms) -> np.ndarray:
        """StateVector.sampleWith on the sharded state: every rank passes the same uniforms and
        gets all the shots.  May change the qubit map (perm()): the logical qubits of a sampling
        chunk are brought to local positions first; the amplitudes are untouched."""
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.size <= 0:
            raise ValueError("n_shots must be positive")
        out = np.empty(u.size, dtype=np.int64)
        _lib.check(_lib.hip.qsim_dist_sample(self._h, u.ctypes.data_as(_c.c_void_p), int(u.size),
                                             out.ctypes.data_as(_c.c_void_p)))
        return out

    def sample(self, n_shots: int) -> np.ndarray:
        if n_shots <= 0:
            raise ValueError("n_shots must be positive")
        return self.sampleWith(self._uniforms(n_shots))

    def collapse(self, bit: int, result: int, scale: float) -> None:
        _lib.check(_lib.hip.qsim_dist_collapse(self._h, bit, result, scale))

    def measureBit(self, bit: int, uniform: Optional[float] = None) -> int:
        """StateVector.measureBit; `uniform`: the draw to use (the same on every rank) instead
        of one from rank 0's generator."""
        if bit < 0 or bit >= self._n:
            raise ValueError(f"Qubit index {bit} out of range [0, {self._n - 1}]")
        u = float(self._uniforms(1)[0]) if uniform is None else float(uniform)
        r = _c.c_int(0)
        _lib.check(_lib.hip.qsim_dist_measure(self._h, bit, u, _c.byref(r)))
        return r.value

    def measureQubit(self, qubit: int, uniform: Optional[float] = None) -> int:
        """Reference semantics: big-endian index bit n-1-qubit (F2, as StateVector.measure)."""
        if qubit < 0 or qubit >= self._n:
            raise ValueError(f"Qubit index {qubit} out of range [0, {self._n - 1}]")
        return self.measureBit(self._n - 1 - qubit, uniform)

    def profile(self, enable: bool = True) -> None:
        _lib.check(_lib.hip.qsim_dist_profile(self._h, 1 if enable else 0))

    def profileStats(self):
        n = _c.c_int(0)
        _lib.check(_lib.hip.qsim_dist_profile_count(self._h, _c.byref(n)))
        out = []
        for i in range(n.value):
            name = _c.create_string_buffer(64)
            ms, cnt, by = _c.c_double(), _c.c_int64(), _c.c_double()
            _lib.check(_lib.hip.qsim_dist_profile_get(self._h, i, name, 64, _c.byref(ms),
                                                      _c.byref(cnt), _c.byref(by)))
            out.append({"name": name.value.decode(), "ms": ms.value, "launches": cnt.value,
                        "alg_bytes": by.value})
        return out


def plan(circuit: Circuit, world: int, rank: int, perm: Optional[List[int]] = None):
    """Host planner output for `rank`: (steps, ops, perm_after).  steps are dicts
    {kind: 'ops'|'exchange', ...}; ops are dicts with the lowered op fields."""
    n = circuit.getNumQubits()
    arr, cnt = circuit.to_abi()
    p = (_c.c_int32 * n)(*(perm if perm is not None else range(n)))
    ns, no = _c.c_size_t(0), _c.c_size_t(0)
    p_size = (_c.c_int32 * n)(*p)  # size the output for the SAME start map (the call updates it)
    _lib.check(_lib.hip.qsim_dist_plan(n, world, rank, arr, cnt, p_size, None, 0, _c.byref(ns),
                                       None, 0, _c.byref(no)))
    steps = (_lib.qsim_dist_step * max(1, ns.value))()
    ops = (_lib.qsim_op * max(1, no.value))()
    _lib.check(_lib.hip.qsim_dist_plan(n, world, rank, arr, cnt, p, steps, ns.value, _c.byref(ns),
                                       ops, no.value, _c.byref(no)))
    out_ops = [{"kind": o.kind, "sub": o.sub, "t0": o.t0, "t1": o.t1, "cmask": o.cmask,
                "d0_one": o.d0_one, "src": o.src,
                "m": [complex(o.m[2 * i], o.m[2 * i + 1]) for i in range(4)]}
               for o in ops[:no.value]]
    out_steps = []
    for s in steps[:ns.value]:
        if s.kind == 1:
            out_steps.append({"kind": "exchange", "k": s.k, "gpos": list(s.gpos[:s.k]),
                              "lpos": list(s.lpos[:s.k]), "pivot": s.pivot, "pmask": s.pmask, "coarse": s.coarse,
                              "pivots": [b for b in range(64) if (s.pmask >> b) & 1]})
        else:
            out_steps.append({"kind": "ops", "ops": out_ops[s.op_begin:s.op_end],
                              "role": s.role, "pivot": s.pivot})
    return out_steps, list(p)


def sample_plan(n: int, world: int, perm: List[int]) -> Tuple[int, int]:
    """Host-only (qsim_dist_sample_plan): (chunk_log, localize_mask) of sampling a sharded state
    whose qubit map is `perm` — the chunk size and the logical qubits brought local first."""
    p = (_c.c_int32 * len(perm))(*perm)
    if len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    c, m = _c.c_int(0), _c.c_uint64(0)
    _lib.check(_lib.hip.qsim_dist_sample_plan(n, world, p, _c.byref(c), _c.byref(m)))
    return c.value, m.value


def expectation_plan(n: int, world: int, perm: Optional[List[int]], observable) -> dict:
    """Host-only (qsim_dist_expectation_plan): what DistributedSimulator.expectation does for a
    PauliSum (or a list of (x_mask, z_mask, coeff)) under qubit map `perm` (None: the identity):
    {local_groups, cross_groups, transfers, launches, bytes_sent_per_rank}."""
    if perm is not None and len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    if hasattr(observable, "to_abi"):
        terms, count = observable.to_abi(n)
    else:
        items = list(observable)
        count = len(items)
        terms = (_lib.qsim_pauli_term * max(1, count))()
        for i, (x, z, c) in enumerate(items):
            terms[i].x_mask, terms[i].z_mask, terms[i].coeff = x, z, c
    p = (_c.c_int32 * n)(*perm) if perm is not None else None
    lg, cg, tr, la = _c.c_int(0), _c.c_int(0), _c.c_int(0), _c.c_int(0)
    by = _c.c_uint64(0)
    _lib.check(_lib.hip.qsim_dist_expectation_plan(n, world, p, terms, count, _c.byref(lg), _c.byref(cg),
                                                   _c.byref(tr), _c.byref(la), _c.byref(by)))
    return {"local_groups": lg.value, "cross_groups": cg.value, "transfers": tr.value,
            "launches": la.value, "bytes_sent_per_rank": by.value}


def marginal_plan(n: int, world: int, perm: Optional[List[int]], qubits, rdm: bool = False) -> dict:
    """Host-only (qsim_dist_marginal_plan): what DistributedSimulator.marginalProbabilities (rdm:
    reducedDensityMatrix) does for these qubits under qubit map `perm` (None: the identity):
    k_loc / k_rank selected local / rank positions; k_lo, k_hi, slices, work_groups of a shard's
    own plan (plan.marginal_plan at n = L); cross_steps, transfers and bytes_sent_per_rank;
    launches per shard (at most), allreduce_doubles, scratch_bytes of the partial sums, pair_rule
    (0 none, 1 half a shard each way, 2 a whole shard and the lower rank computes) and
    cross_work_groups.  The readers' argument checks."""
    if perm is not None and len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    qs = [int(q) for q in qubits]
    arr = (_c.c_int32 * len(qs))(*qs) if qs else None
    p = (_c.c_int32 * n)(*perm) if perm is not None else None
    info = (_c.c_int32 * 16)()
    _lib.check(_lib.hip.qsim_dist_marginal_plan(n, world, p, arr, len(qs), 1 if rdm else 0, info))
    return {"k_loc": info[0], "k_rank": info[1], "k_lo": info[2], "k_hi": info[3], "slices": info[4],
            "work_groups": info[5], "cross_steps": info[6], "transfers": info[7],
            "bytes_sent_per_rank": (info[8] & 0xffffffff) | (info[9] << 32), "launches": info[10],
            "allreduce_doubles": info[11],
            "scratch_bytes": (info[12] & 0xffffffff) | (info[13] << 32), "pair_rule": info[14],
            "cross_work_groups": info[15]}


def gradient_plan(circuit: Circuit, world: int, observable, perm: Optional[List[int]] = None) -> dict:
    """Host-only (qsim_dist_gradient_plan): what DistributedSimulator.gradient does for `circuit`
    and a PauliSum (or a list of (x_mask, z_mask, coeff)) when the call starts from a non-fresh
    state with qubit map `perm` (None: the identity; a fresh state may relabel first, which is not
    modelled): the parameterised steps by class, the inverted segments and their remaps, the
    groups and transfers of lambda = H phi, the steps' transfers, bytes sent per rank, and the map
    after the forward run and after the sweep."""
    n = circuit.getNumQubits()
    if perm is not None and len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    arr, cnt = circuit.to_abi()
    if hasattr(observable, "to_abi"):
        terms, count = observable.to_abi(n)
    else:
        items = list(observable)
        count = len(items)
        terms = (_lib.qsim_pauli_term * max(1, count))()
        for i, (x, z, c) in enumerate(items):
            terms[i].x_mask, terms[i].z_mask, terms[i].coeff = x, z, c
    p = (_c.c_int32 * n)(*perm) if perm is not None else None
    info = _lib.qsim_dist_gradient_info()
    _lib.check(_lib.hip.qsim_dist_gradient_plan(n, world, p, arr, cnt, terms, count, _c.byref(info)))
    out = {k: getattr(info, k) for k, _ in info._fields_ if not k.startswith("perm_")}
    out["perm_after_run"] = list(info.perm_after_run[:n])
    out["perm_after_sweep"] = list(info.perm_after_sweep[:n])
    return out


def _terms_arg(n: int, items):
    """A PauliSum, or a list of (x_mask, z_mask, coeff), as the ABI's term array and its count."""
    if hasattr(items, "to_abi"):
        return items.to_abi(n)
    items = list(items)
    terms = (_lib.qsim_pauli_term * max(1, len(items)))()
    for i, (x, z, c) in enumerate(items):
        terms[i].x_mask, terms[i].z_mask, terms[i].coeff = x, z, c
    return terms, len(items)


def _info_dict(info) -> dict:
    out = {}
    for k, _ in info._fields_:
        v = getattr(info, k)
        if hasattr(v, "_fields_"):
            out.update({f"{k}_{kk}": vv for kk, vv in _info_dict(v).items()})
        else:
            out[k] = v
    return out


def pauli_rotation_plan(n: int, world: int, perm: Optional[List[int]], seq) -> dict:
    """Host-only (qsim_dist_pauli_rotation_plan): what DistributedSimulator.applyPauliRotations
    does for a sequence (a PauliSum, or a list of (x_mask, z_mask, theta)) under qubit map `perm`
    (None: the identity): {rotations, phase_rotations, phase_passes, local_rotations,
    cross_rotations, cross_pure, launches, transfers, bytes_sent_per_rank}."""
    if perm is not None and len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    rots, count = _terms_arg(n, seq)
    p = (_c.c_int32 * n)(*perm) if perm is not None else None
    info = _lib.qsim_dist_pauli_rotation_info()
    _lib.check(_lib.hip.qsim_dist_pauli_rotation_plan(n, world, p, rots, count, _c.byref(info)))
    return _info_dict(info)


def pauli_gradient_plan(n: int, world: int, perm: Optional[List[int]], seq, observable) -> dict:
    """Host-only (qsim_dist_pauli_gradient_plan): what DistributedSimulator.pauliGradient does
    under qubit map `perm` (None: the identity): the application's figures as forward_*, the
    sweep's steps by class, the class of the bra-ket-only step (first_class), the groups and
    transfers of lambda = H phi, the steps' transfers and the bytes one rank sends."""
    if perm is not None and len(perm) != n:
        raise ValueError("perm needs one entry per qubit")
    rots, count = _terms_arg(n, seq)
    terms, nterms = _terms_arg(n, observable)
    p = (_c.c_int32 * n)(*perm) if perm is not None else None
    info = _lib.qsim_dist_pauli_gradient_info()
    _lib.check(_lib.hip.qsim_dist_pauli_gradient_plan(n, world, p, rots, count, terms, nterms, _c.byref(info)))
    return _info_dict(info)


def plan_memo_clear() -> None:
    """Forget the process-wide pivot memo: the next plan() decides as a fresh rank process."""
    _lib.check(_lib.hip.qsim_dist_plan_memo_clear())


def slab_map(n: int, world: int, rank: int, step: dict, part: int = -1):
    """The pack / unpack layout of exchange `step` (a plan() dict) on `rank`, as the engine's
    kernels use it (qsim_dist_slab_map): (my_c, peer_of, index) where slab c goes to and comes
    from rank peer_of[c] and index[c * chunk + e] is the local amplitude index of its element e.
    part >= 0: part `part` of an overlapped remap (the pivot bits hold `part`)."""
    st = _lib.qsim_dist_step()
    st.kind, st.k = 1, step["k"]
    for j in range(step["k"]):
        st.gpos[j], st.lpos[j] = step["gpos"][j], step["lpos"][j]
    st.pmask = step.get("pmask", 0)
    g = world.bit_length() - 1
    m = bin(st.pmask).count("1") if part >= 0 else 0
    count = 1 << (n - g - m)
    my_c = _c.c_int32(0)
    peer_of = (_c.c_int32 * (1 << st.k))()
    index = np.empty(count, dtype=np.uint64)
    _lib.check(_lib.hip.qsim_dist_slab_map(n, world, rank, _c.byref(st), part, _c.byref(my_c), peer_of,
                                           index.ctypes.data_as(_c.POINTER(_c.c_uint64)), count))
    return my_c.value, list(peer_of), index.astype(np.int64)
