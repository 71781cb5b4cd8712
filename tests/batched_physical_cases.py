"""Cases of the batched physical-noise tests (csrc/hip/batched.hip, the Pauli-frame path).

Helper module (no tests here), shared by tests/test_batched_physical_cpu.py (which checks on the
CPU that every case really draws X, Y and Z picks around non-Clifford gates) and
tests/test_batched_physical_gpu.py (which runs the cases on the engine against
oracle/numpy_oracle.py: batched_physical_run).  Everything here is plain data: gates are
(type, qubits, parameter) tuples and channels (type, qubit, p) tuples, as the oracle takes them.
"""
import itertools

import numpy as np

X, Y, Z, H, S, T, SDAG, TDAG, RX, RY, RZ, CNOT, CZ, CRY, CRZ, SWAP, TOFFOLI = range(17)
NAMES = ["X", "Y", "Z", "H", "S", "T", "Sdag", "Tdag", "Rx", "Ry", "Rz", "CNOT", "CZ", "CRY", "CRZ",
         "SWAP", "Toffoli"]
ARITY = [1] * 11 + [2] * 5 + [3]
# the gates the frame path propagates its Pauli frame through instead of conjugating them
# (batched.hip: CliffordCode); every other gate consumes the frame inside a fused pass
CLIFFORD = frozenset({X, Y, Z, H, S, SDAG, CNOT, CZ, SWAP})
DEPOLARIZING, AMPLITUDE_DAMPING, PHASE_DAMPING, BIT_FLIP, PHASE_FLIP, BIT_PHASE_FLIP = range(6)
# p = 1 channel type that applies a given Pauli ('I': no entry), and that Pauli as a gate type
CHANNEL_OF = {"X": BIT_FLIP, "Y": BIT_PHASE_FLIP, "Z": PHASE_FLIP}
GATE_OF = {"X": X, "Y": Y, "Z": Z}


def mixed_gates(n, depth, seed):
    """`depth` gates drawn uniformly from the gate types an n-qubit register can hold (all 17
    from 3 qubits on) on distinct random operands."""
    rng = np.random.default_rng(seed)
    kinds = [k for k in range(17) if ARITY[k] <= n]
    out = []
    for _ in range(depth):
        k = kinds[int(rng.integers(0, len(kinds)))]
        qs = [int(x) for x in rng.choice(n, ARITY[k], replace=False)]
        th = float(rng.uniform(-3.0, 3.0)) if k in (RX, RY, RZ, CRY, CRZ) else 0.0
        out.append((k, qs, th))
    return out


def mixed_channels(n, seed):
    """All four Pauli channel types on several qubits, p in [0.1, 0.5], two damping entries
    interleaved (the physical process ignores them; they shift the model's indices only)."""
    rng = np.random.default_rng(1000 + seed)
    p = lambda: float(rng.uniform(0.1, 0.5))
    q = lambda: int(rng.integers(0, n))
    ch = [(DEPOLARIZING, 0, p()), (BIT_FLIP, q(), p()), (AMPLITUDE_DAMPING, q(), 0.3),
          (PHASE_FLIP, q(), p()), (DEPOLARIZING, n - 1, p()), (BIT_PHASE_FLIP, q(), p()),
          (PHASE_DAMPING, q(), 0.2), (DEPOLARIZING, n // 2, p()), (PHASE_FLIP, n - 1, p()),
          (BIT_FLIP, 0, p())]
    return ch


def circuit_of(q, n, gates):
    c = q.Circuit(n)
    for t, qs, th in gates:
        c.append(q.GateOp(q.GateType(t), list(qs), th))
    return c


def model_of(q, channels):
    nm = q.NoiseModel()
    add = [nm.addDepolarizing, nm.addAmplitudeDamping, nm.addPhaseDamping, nm.addBitFlip,
           nm.addPhaseFlip, nm.addBitPhaseFlip]
    for t, qubit, p in channels:
        add[t]([qubit], p)
    return nm


# ---- (a) random draws -------------------------------------------------------------------------
# name -> n, B, depth, circuit/model seed, simulator seed(s) of the two consecutive runs (a second
# seed: setSeed between the runs, which restarts the step counter), trajectory offset, gate set.
# n < 10 runs one kernel per gate whatever is asked (the small Pauli-pass launch shapes, odd B);
# n >= 10 runs fused passes under Pauli frames; at 13 one qubit lies outside the 12-qubit tile.
def _case(n, B, depth, cseed, seed, seed2=None, traj0=0, refset=False):
    return dict(n=n, B=B, depth=depth, cseed=cseed, seed=seed, seed2=seed2, traj0=traj0, refset=refset)


RANDOM_CASES = {
    "n1_B7": _case(1, 7, 20, 101, 11),
    "n3_B5": _case(3, 5, 20, 103, 12),
    "n6_B9": _case(6, 9, 20, 106, 13),
    "n8_B3": _case(8, 3, 20, 108, 14),
    "n10_B5": _case(10, 5, 40, 110, 15),
    "n12_B4": _case(12, 4, 40, 112, 16),
    "n13_B3": _case(13, 3, 40, 113, 17),
    "n10_B5_reseed": _case(10, 5, 40, 210, 18, seed2=19),
    "n11_B4_offset3": _case(11, 4, 40, 211, 20, traj0=3),
    "n11_B4_refset": _case(11, 4, 40, 311, 21, refset=True),
}


def case_runs(case):
    """[(gates, channels, seed, first step)] of the two consecutive runs of a random-draw case."""
    gates = mixed_gates(case["n"], case["depth"], case["cseed"])
    channels = mixed_channels(case["n"], case["cseed"])
    if case["seed2"] is None:
        return [(gates, channels, case["seed"], 0), (gates, channels, case["seed"], len(gates))]
    return [(gates, channels, case["seed"], 0), (gates, channels, case["seed2"], 0)]


def clifford_gates(n, depth, seed):
    rng = np.random.default_rng(seed)
    kinds = sorted(CLIFFORD)
    out = []
    for _ in range(depth):
        k = kinds[int(rng.integers(0, len(kinds)))]
        out.append((k, [int(x) for x in rng.choice(n, ARITY[k], replace=False)], 0.0))
    return out


# The further fused scenarios of the GPU file: n, B, simulator seed and the stages in order, each
# (gates, channels, how) with how = "fused" | "per_gate" (a run) or "sync" (synchronize()).
def scenario(name):
    if name == "carried":  # frames carried through noisy, noise-free and per-gate runs and a sync
        n = 11
        c1, c2, ch = mixed_gates(n, 40, 401), mixed_gates(n, 30, 402), mixed_channels(n, 401)
        stages = [(c1, ch, "fused"), (c2, [], "fused"), (c1, ch, "per_gate"), (c2, ch, "fused"),
                  (None, None, "sync"), (c1, ch, "fused")]
        return dict(n=n, B=5, seed=31, stages=stages)
    if name == "relabel":  # first run from |0..0> under forced relabeling, then a second run
        # no gate on qubit 2 (noise only): the 12 busy qubits fit one tile only under other labels
        # than the identity, whose tiles always hold qubits 0..3 — so the planner relabels
        n = 13
        live = [q for q in range(n) if q != 2]
        c = [(t, [live[q] for q in qs], th) for t, qs, th in mixed_gates(n - 1, 60, 412)]
        ch = mixed_channels(n, 412)
        return dict(n=n, B=3, seed=32, stages=[(c, ch, "fused"), (c, ch, "fused")])
    if name == "jit":
        # Clifford gates, closed by two CNOT rings over all 13 qubits: whichever qubit the first
        # pass's 12-qubit tile leaves out, the rings stop it before the mixed gates behind them,
        # so the first pass is Clifford-only (a specialised kernel) and the frame-conjugated
        # gates run in later passes (the interpreter)
        n = 13
        ring = [(CNOT, [q, (q + 1) % n], 0.0) for q in range(n)]
        c = clifford_gates(n, 30, 420) + ring + ring + mixed_gates(n, 40, 421)
        ch = mixed_channels(n, 420)
        return dict(n=n, B=3, seed=33, stages=[(c, ch, "fused"), (c, ch, "fused")])
    if name == "readers":  # one fused noisy run; every reader then meets a pending frame
        n = 10  # (the rotation layer first: probability on every basis state, generic phases)
        c = prep_gates(n, 431) + mixed_gates(n, 40, 430)
        return dict(n=n, B=4, seed=34, stages=[(c, mixed_channels(n, 430), "fused")])
    raise KeyError(name)


SCENARIOS = ("carried", "relabel", "jit", "readers")


# ---- (b) deterministic frame matrix -----------------------------------------------------------
FRAME_SIZES = {10: dict(operands=(0, 1, 4, 7, 9), spare=2), 13: dict(operands=(0, 6, 11, 12), spare=3)}
# placements: every role (target / control / second control) sees a lowest, a middle and the top qubit
_PLACEMENTS = {
    (10, 1): [(0,), (1,), (4,), (7,), (9,)],
    (10, 2): [(0, 4), (4, 9), (9, 0), (1, 7), (7, 1)],
    (10, 3): [(0, 4, 9), (9, 0, 4), (4, 9, 0), (7, 1, 4)],
    (13, 1): [(0,), (6,), (11,), (12,)],
    (13, 2): [(0, 12), (12, 6), (6, 11), (11, 0)],
    (13, 3): [(0, 6, 12), (12, 0, 11), (11, 12, 0), (6, 11, 12)],
}
# reduced frame sets: every operand under each of I, X, Y, Z, and mixed strings
_REDUCED = {
    2: ["II", "XX", "YY", "ZZ", "XZ", "ZY", "YX", "IX", "ZI"],
    3: ["III", "XXX", "YYY", "ZZZ", "XYZ", "YZX", "ZXY", "IXZ", "ZIY"],
}


def frame_cases(n, gate_type):
    """[(operands, frame string, fillers)]: all 4^k frames at n = 10 for one- and two-qubit gates
    and at Toffoli's first placement; the reduced set at Toffoli's other placements and for
    multi-qubit gates at n = 13."""
    k = ARITY[gate_type]
    out = []
    for i, ops in enumerate(_PLACEMENTS[(n, k)]):
        full = k == 1 or (n == 10 and (k == 2 or i == 0))
        frames = ["".join(f) for f in itertools.product("IXYZ", repeat=k)] if full else _REDUCED[k]
        for fr in frames:
            for fillers in (1, 2):
                out.append((ops, fr, fillers))
    return out


def prep_gates(n, seed=77):
    """A product of seeded Ry / Rz rotations on every qubit, entangled by a CZ chain: every
    amplitude non-zero with a generic phase."""
    rng = np.random.default_rng(seed)
    g = []
    for q in range(n):
        g.append((RY, [q], float(rng.uniform(0.4, 2.7))))
        g.append((RZ, [q], float(rng.uniform(-3.0, 3.0))))
    for q in range(n - 1):
        g.append((CZ, [q, q + 1], 0.0))
    return g


def frame_circuit(n, gate_type, operands, fillers, theta=0.83):
    """[fillers x H on the spare qubit, G on the operands, T on G's target]."""
    spare = FRAME_SIZES[n]["spare"]
    th = theta if gate_type in (RX, RY, RZ, CRY, CRZ) else 0.0
    target = operands[-1]  # one-qubit gates: the qubit; (control, target); (c1, c2, target)
    return [(H, [spare], 0.0)] * fillers + [(gate_type, list(operands), th), (T, [target], 0.0)]


def frame_channels(operands, frame):
    return [(CHANNEL_OF[p], q, 1.0) for q, p in zip(operands, frame) if p != "I"]


def frame_expected_gates(n, gate_type, operands, frame, fillers):
    """The circuit with the frame's Paulis as explicit gates after every step, in channel order."""
    paulis = [(GATE_OF[p], [q], 0.0) for q, p in zip(operands, frame) if p != "I"]
    out = []
    for g in frame_circuit(n, gate_type, operands, fillers):
        out.append(g)
        out.extend(paulis)
    return out
