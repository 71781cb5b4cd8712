"""Batched parameter sweeps (BatchedSimulator.runSweep -> qsim_batch_run_sweep): one circuit, one
angle set per member.  The oracle is oracle/numpy_oracle.run_cpu per member with that member's
angles written into the gate list; the tolerance is the project's 1e-12 per component
(test_batched_gpu.py).  Every test handles at most 4 MiB of state."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12
PARAM_TYPES = (8, 9, 10, 13, 14)  # Rx Ry Rz CRY CRZ
FIXED_ROWS = (0.0, math.pi, 2.0 * math.pi, -0.3)


def _add(c, k, a, b, d, th):
    if k < 8:
        getattr(c, ("x", "y", "z", "h", "s", "t", "sdag", "tdag")[k])(a)
    elif k < 11:
        getattr(c, ("rx", "ry", "rz")[k - 8])(a, th)
    elif k == 11:
        c.cnot(a, b)
    elif k == 12:
        c.cz(a, b)
    elif k == 13:
        c.cry(a, b, th)
    elif k == 14:
        c.crz(a, b, th)
    elif k == 15:
        c.swap(a, b)
    else:
        c.toffoli(a, b, d)


def _random_circuit(q, n, depth, seed, min_slots=12, extra_pairs=()):
    """depth gates over the full gate set, at least min_slots of them parameterised, CRY and CRZ with
    the control above and below the target among them; extra_pairs: CRY(control, target) gates
    spread through the circuit."""
    rng = np.random.default_rng(seed)
    kinds = [int(k) for k in rng.integers(0, 17, size=depth)]
    forced = [8, 9, 10, 13, 14, 13, 14, 9, 10, 8, 13, 14]
    where = rng.choice(depth, size=len(forced), replace=False)
    for w, k in zip(where, forced):
        kinds[int(w)] = k
    assert sum(k in PARAM_TYPES for k in kinds) >= min_slots
    c = q.Circuit(n)
    extra = list(extra_pairs)
    flip = 0
    for i, k in enumerate(kinds):
        a, b, d = (int(x) for x in rng.choice(n, 3, replace=False))
        if k in (13, 14):  # alternate the control above / below the target
            lo, hi = min(a, b), max(a, b)
            a, b = (hi, lo) if flip & 1 else (lo, hi)
            flip += 1
        _add(c, k, a, b, d, float(rng.uniform(-3.0, 3.0)))
        if extra and i % 3 == 0:
            ctrl, tgt = extra.pop()
            c.cry(ctrl, tgt, 0.5)
    for ctrl, tgt in extra:
        c.cry(ctrl, tgt, 0.5)
    return c


def _slots(c):
    return [i for i, g in enumerate(c.getGates()) if int(g.type) in PARAM_TYPES]


def _oracle_states(oracle, c, angles, start=None):
    """The per-member oracle states: member t's angles written into the gate list."""
    n = c.getNumQubits()
    base = oracle.gates_of(c)
    slots = _slots(c)
    out = []
    for t, row in enumerate(angles):
        gates = list(base)
        for k, i in enumerate(slots):
            gates[i] = (gates[i][0], gates[i][1], float(row[k]))
        out.append(oracle.run_cpu(n, gates, None if start is None else start[t]))
    return out


def _err(got, want):
    d = got - want
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


def _check(sim, want, what=""):
    for t, w in enumerate(want):
        e = _err(sim.getStateVector(t), w)
        assert e < TOL, f"{what} member {t}: max component error {e}"


def _batch(q, n, B):
    return q.BatchedSimulator(n, B, noise=q.BatchedNoise.Physical)


def _angle_sets(rng, B, P):
    """One drawn (B, P) set, then sets whose rows go through the fixed rows (all 0, all pi, all
    2 pi, all -0.3) until every one of them has been a member's row (B = 1: four sweeps)."""
    sets = [rng.uniform(-math.pi, math.pi, size=(B, P))]
    k = 0
    while k < len(FIXED_ROWS):
        a = rng.uniform(-math.pi, math.pi, size=(B, P))
        for t in range(B):
            if k < len(FIXED_ROWS):
                a[t, :] = FIXED_ROWS[k]
                k += 1
        sets.append(a)
    return sets


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n", [10, 12, 14])
def test_fused_matches_oracle(qsim, oracle, gpu_ready, n, B):
    """At n = 14 a member spans several tiles (a wrong member derivation fails here) and every
    ordered (control, target) pair over {0, 6, 12, 13} is a CRY: whatever 12 or 13 of the 14 qubits
    a pass's tile holds, some control lies outside some candidate tile."""
    from qsim_amd import plan
    pairs = [(a, b) for a in (0, 6, 12, 13) for b in (0, 6, 12, 13) if a != b] if n == 14 else []
    c = _random_circuit(qsim, n, 40, 100 + n, extra_pairs=pairs)
    P = len(_slots(c))
    assert P >= 12 and plan.batch_sweep_plan(c, B)["fused"]
    rng = np.random.default_rng(7 * n + B)
    sim = _batch(qsim, n, B)
    for a in _angle_sets(rng, B, P):
        sim.reset()
        sim.runSweep(c, a)
        _check(sim, _oracle_states(oracle, c, a), f"n={n} B={B}")


def test_thirteen_qubit_tiles(qsim, oracle, gpu_ready):
    from qsim_amd import plan
    n, B = 14, 2
    c = _random_circuit(qsim, n, 40, 77)
    a = np.random.default_rng(5).uniform(-3, 3, size=(B, len(_slots(c))))
    plan.set_tile_height(7)
    try:
        for rb7 in (4, 3):
            plan.set_tile_rb7(rb7)
            sim = _batch(qsim, n, B)
            sim.runSweep(c, a)
            _check(sim, _oracle_states(oracle, c, a), f"h=7 rb={rb7}")
    finally:
        plan.set_tile_rb7(-1)
        plan.set_tile_height(-1)


def _per_gate_circuit(q, n):
    """Every slot type on target 0, the middle and n - 1; controlled types with the control above
    and below (every ordered pair at n = 3)."""
    c = q.Circuit(n)
    for k in range(n):
        c.h(k)
        c.t(k)
    targets = sorted({0, n // 2, n - 1})
    th = iter(0.1 * k for k in range(1, 1000))
    for t in targets:
        c.rx(t, next(th))
        c.ry(t, next(th))
        c.rz(t, next(th))
    if n >= 2:
        pairs = [(a, b) for a in range(n) for b in range(n) if a != b] if n <= 3 else \
            [(a, b) for b in targets for a in sorted({0, n // 2, n - 1, (b + 1) % n, (b - 1) % n}) if a != b]
        for a, b in pairs:
            c.cry(a, b, next(th))
            c.h(b)
            c.crz(a, b, next(th))
        if n >= 3:
            c.toffoli(0, 1, n - 1)
            c.swap(0, n - 1)
            c.ry(n - 1, next(th))
    return c


@pytest.mark.parametrize("n,per_gate", [(1, False), (3, False), (6, False), (9, False), (12, True)])
def test_per_gate_matches_oracle(qsim, oracle, gpu_ready, n, per_gate):
    from qsim_amd import plan
    B = 3
    c = _per_gate_circuit(qsim, n)
    P = len(_slots(c))
    assert not plan.batch_sweep_plan(c, B, per_gate=per_gate)["fused"]
    rng = np.random.default_rng(n)
    sim = _batch(qsim, n, B)
    for a in _angle_sets(rng, B, P):
        sim.reset()
        sim.runSweep(c, a, per_gate=per_gate)
        _check(sim, _oracle_states(oracle, c, a), f"per-gate n={n}")


def test_fused_equals_per_gate(qsim, gpu_ready):
    n, B = 12, 3
    c = _random_circuit(qsim, n, 40, 31)
    a = np.random.default_rng(9).uniform(-3, 3, size=(B, len(_slots(c))))
    fused, per = _batch(qsim, n, B), _batch(qsim, n, B)
    fused.runSweep(c, a)
    per.runSweep(c, a, per_gate=True)
    for t in range(B):
        assert _err(fused.getStateVector(t), per.getStateVector(t)) < TOL


def test_composition(qsim, oracle, gpu_ready):
    n, B = 11, 3
    c1, c2 = _random_circuit(qsim, n, 30, 41), _random_circuit(qsim, n, 40, 42)
    P = len(_slots(c2))
    rng = np.random.default_rng(3)
    a1, a2 = rng.uniform(-3, 3, size=(B, P)), rng.uniform(-3, 3, size=(B, P))
    sim = _batch(qsim, n, B)
    sim.run(c1)
    sim.runSweep(c2, a1)
    sim.runSweep(c2, a2)
    start = [oracle.run_cpu(n, oracle.gates_of(c1))] * B
    want = _oracle_states(oracle, c2, a2, _oracle_states(oracle, c2, a1, start))
    _check(sim, want, "run, sweep, sweep")
    # every row the circuit's own angles: what run() computes; a 1-d angle set goes to every member
    own = [g.parameter for g in c2.getGates() if int(g.type) in PARAM_TYPES]
    a, b = _batch(qsim, n, B), _batch(qsim, n, B)
    a.runSweep(c2, own)
    b.run(c2)
    for t in range(B):
        assert _err(a.getStateVector(t), b.getStateVector(t)) < TOL
    # no parameterised gate: exactly run()
    cliff = qsim.createRandomHCCircuit(n, 60, 5)
    if _slots(cliff):
        cliff = qsim.createGHZCircuit(n)
    assert not _slots(cliff)
    a, b = _batch(qsim, n, B), _batch(qsim, n, B)
    a.runSweep(cliff, np.zeros((B, 0)))
    b.run(cliff)
    for t in range(B):
        assert a.getStateVector(t).tobytes() == b.getStateVector(t).tobytes()


def test_after_a_noisy_run(qsim, oracle, gpu_ready):
    """Two objects run the same noisy trajectories (one seed).  The first is read (its carried
    Pauli frames materialised by the reader); the second goes straight into a noise-free sweep,
    which has to materialise them itself."""
    n, B = 10, 4
    c1, c2 = _random_circuit(qsim, n, 30, 51), _random_circuit(qsim, n, 40, 52)
    nm = qsim.NoiseModel()
    nm.addDepolarizingAll(n, 0.15)
    nm.addBitFlip([0, n - 1], 0.2)
    a = np.random.default_rng(8).uniform(-3, 3, size=(B, len(_slots(c2))))
    read, swept = (qsim.BatchedSimulator(n, B, nm, noise=qsim.BatchedNoise.Physical) for _ in range(2))
    for s in (read, swept):
        s.setSeed(2024)
        s.run(c1)
    start = [read.getStateVector(t) for t in range(B)]
    assert any(_err(start[t], start[0]) > 1e-3 for t in range(1, B)), "the noise did nothing"
    swept.setNoiseModel(qsim.NoiseModel())
    swept.runSweep(c2, a)
    _check(swept, _oracle_states(oracle, c2, a, start), "after noise")


def _pauli_expectation(psi, x, z):
    """<psi|P|psi>, P = i^(#Y) X^x Z^z (masks)."""
    idx = np.arange(psi.size, dtype=np.int64)
    par = np.zeros(psi.size, dtype=np.int64)
    for q in range(int(z).bit_length()):
        if z >> q & 1:
            par ^= (idx >> q) & 1
    out = np.empty_like(psi)
    out[idx ^ x] = (1j ** bin(x & z).count("1")) * (1 - 2 * par) * psi
    return float(np.vdot(psi, out).real)


def expectation_np(psi, terms):
    return sum(c * _pauli_expectation(psi, x, z) for x, z, c in terms)


def pauli_sum(qsim, n, terms):
    h = qsim.PauliSum(n)
    for x, z, c in terms:
        h.add(c, {q: "Y" if (x >> q & 1) and (z >> q & 1) else ("X" if x >> q & 1 else "Z")
                  for q in range(n) if (x | z) >> q & 1})
    return h


def test_expectations(qsim, oracle, gpu_ready):
    n, B = 12, 5
    c = _random_circuit(qsim, n, 40, 61)
    a = np.random.default_rng(4).uniform(-3, 3, size=(B, len(_slots(c))))
    terms = [(0, 0b101, 0.7), (0b11, 0b10, -0.4), (1 << 11, 1 << 11, 0.3), (0b1000001, 0b0100000, 0.25),
             ((1 << 6) | (1 << 9), (1 << 9) | 1, -0.6)]  # Z.Z, X.Y, Y, X.Z.X, X.Y.Z
    sim = _batch(qsim, n, B)
    sim.runSweep(c, a)
    got = sim.getExpectations(pauli_sum(qsim, n, terms))
    bound = TOL * sum(abs(t[2]) for t in terms)
    for t, psi in enumerate(_oracle_states(oracle, c, a)):
        assert abs(got[t] - expectation_np(psi, terms)) < bound


def test_reproducible(qsim, gpu_ready):
    for n, per_gate in ((13, False), (8, False), (11, True)):
        B = 3
        c = _random_circuit(qsim, n, 40, 71)
        a = np.random.default_rng(6).uniform(-3, 3, size=(B, len(_slots(c))))
        runs = []
        for _ in range(2):
            sim = _batch(qsim, n, B)
            sim.runSweep(c, a, per_gate=per_gate)
            runs.append([sim.getStateVector(t).tobytes() for t in range(B)])
        assert runs[0] == runs[1]


def test_errors_leave_the_states(qsim, gpu_ready):
    n, B = 10, 3
    c = _random_circuit(qsim, n, 40, 81)
    P = len(_slots(c))
    sim = _batch(qsim, n, B)
    sim.run(qsim.createGHZCircuit(n))
    before = [sim.getStateVector(t).tobytes() for t in range(B)]
    good = np.full((B, P), 0.3)
    for bad in (np.zeros((B, P + 1)), np.zeros((B + 1, P)), np.zeros(P - 1), np.zeros((B, P, 1)), np.zeros((P, B))):
        with pytest.raises(ValueError):
            sim.runSweep(c, bad)
    with pytest.raises(ValueError):
        sim.runSweep(qsim.Circuit(n + 1), np.zeros((B, 0)))
    nm = qsim.NoiseModel()
    nm.addBitFlip([1], 0.1)
    sim.setNoiseModel(nm)
    with pytest.raises(ValueError):
        sim.runSweep(c, good)
    sim.setNoiseModel(qsim.NoiseModel())
    sim.setGateSet(qsim.BatchedGateSet.Reference)
    with pytest.raises(ValueError):
        sim.runSweep(c, good)
    sim.setGateSet(qsim.BatchedGateSet.Full)
    sim.setNoiseSemantics(qsim.BatchedNoise.Reference)
    with pytest.raises(ValueError):
        sim.runSweep(c, good)
    sim.setNoiseSemantics(qsim.BatchedNoise.Physical)
    with pytest.raises(ValueError):  # an angle that is not finite: refused by the engine before any launch
        sim.runSweep(c, np.full((B, P), np.nan))
    assert [sim.getStateVector(t).tobytes() for t in range(B)] == before
    sim.runSweep(c, good)  # and the object still sweeps
    assert [sim.getStateVector(t).tobytes() for t in range(B)] != before
