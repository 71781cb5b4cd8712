"""Adjoint gradients of a batched parameter sweep (BatchedSimulator.gradientSweep ->
qsim_batch_gradient_sweep; csrc/hip/batch_adjoint.hip): one circuit, one angle set per member, every
member's energy and its gradient with respect to its own angles.

The oracle is tests/gradient_cases.adjoint_gradient per member with that member's angles written
into the gate list (itself checked against the exact parameter shift in tests/test_gradient_cpu.py);
the tolerance is the project's gradient_cases.bound(terms) = 1e-12 * sum |c| for values and
gradients.  Every test handles at most a few MiB of state."""
import math

import numpy as np
import pytest

import gradient_cases as gc
from test_batch_sweep_gpu import _angle_sets, _batch, _random_circuit, _slots

pytestmark = pytest.mark.gpu


def _gates(c):
    return [(int(g.type), list(g.qubits), float(g.parameter)) for g in c.getGates()]


def _oracle(c, angles, terms, start=None):
    """(values[B], grads[B, P]) of the dense recurrence, member by member; start: the members' states
    before the circuit (default |0..0>)."""
    n = c.getNumQubits()
    base, slots = _gates(c), _slots(c)
    values, grads = [], []
    for t, row in enumerate(np.atleast_2d(angles)):
        gates = list(base)
        for k, i in enumerate(slots):
            gates[i] = (gates[i][0], gates[i][1], float(row[k]))
        v, g = gc.adjoint_gradient(gc.basis_state(n) if start is None else start[t], n, gates, terms)
        values.append(v)
        grads.append(g[slots] if slots else np.zeros(0))
    return np.array(values), np.array(grads).reshape(len(values), len(slots))


def _check(got, want, terms, what=""):
    (gv, gg), (wv, wg) = got, want
    assert gv.shape == wv.shape and gg.shape == wg.shape, (what, gv.shape, gg.shape)
    ev = np.abs(gv - wv).max()
    assert ev < gc.bound(terms), (what, "values", float(ev))
    if gg.size:
        err = np.abs(gg - wg)
        assert err.max() < gc.bound(terms), (what, np.unravel_index(int(err.argmax()), err.shape), float(err.max()))


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- closed forms at n = 1, 2 ----
@pytest.mark.parametrize("fused", ["1", "0"])
def test_closed_forms(qsim, gpu_ready, monkeypatch, fused):
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
    B, tol = 3, 1e-12
    th = np.array([0.61, -1.2, 2.5])

    def run(n, gates, terms, slot):
        """The members' values and their gradients at `slot`, whose angle is th[t]; other slots 0.3."""
        c = gc.to_circuit(qsim, n, gates)
        P = len(_slots(c))
        a = np.full((B, P), 0.3)
        a[:, slot] = th
        for k, g in enumerate(g for g in gates if g[0] in gc.PARAMETRIC):
            if k != slot:
                a[:, k] = g[2]
        v, g = _batch(qsim, n, B).gradientSweep(c, a, gc.to_pauli_sum(qsim, n, terms))
        assert v.shape == (B,) and g.shape == (B, P)
        return v, g

    z0 = [(0, 1, 1.0)]
    # The circuit's first parameterised gate is the sweep's last step, a reduction with nothing to
    # undo; behind a leading RZ(0) the gate under test takes the step proper.
    for t, want in ((gc.RY, (np.cos(th), -np.sin(th))), (gc.RX, (np.cos(th), -np.sin(th))),
                    (gc.RZ, (np.ones(B), np.zeros(B)))):
        for head in ([], [(gc.RZ, [0], 0.0)]):
            v, g = run(1, head + [(t, [0], 0.0)], z0, len(head))
            assert np.abs(v - want[0]).max() < tol and np.abs(g[:, len(head)] - want[1]).max() < tol, (t, head, v, g)
    z1 = [(0, 2, 1.0)]
    for head in ([], [(gc.RZ, [1], 0.0)]):
        k = len(head)
        v, g = run(2, head + [(gc.X, [0], 0.0), (gc.CRY, [0, 1], 0.0), (gc.RZ, [0], 0.3)], z1, k)
        assert np.abs(v - np.cos(th)).max() < tol and np.abs(g[:, k] + np.sin(th)).max() < tol
        assert np.abs(g[:, k + 1]).max() < tol
        v, g = run(2, head + [(gc.CRY, [0, 1], 0.0), (gc.RY, [0], 0.0)], z1, k)  # control at |0>
        assert np.abs(v - 1.0).max() < tol
        assert (g[:, k] == 0.0).all()  # exactly: the control == 1 half is all zeros


# ---- every operand class of the step kernels, on the per-gate path ----
def _operand_circuit(q, n):
    """An H layer (a dense state), then every generator (X, Y, Z, controlled Y, controlled Z) on
    targets 0, 5, 6 (where n allows) and n - 1, the controlled ones with the control above and below
    the target, fixed gates between them."""
    c = q.Circuit(n)
    for k in range(n):
        c.h(k)
    th = iter(0.1 * k for k in range(1, 1000))
    for t in sorted({t for t in (0, 5, 6, n - 1) if t < n}):
        c.rx(t, next(th))
        c.t(t)
        c.ry(t, next(th))
        c.rz(t, next(th))
        c.cnot(t, (t + 2) % n)
        for ctrl in sorted({x for x in (t - 1, t + 1, 0, n - 1) if 0 <= x < n and x != t}):
            c.cry(ctrl, t, next(th))
            c.crz(ctrl, t, next(th))
            c.h(ctrl)
    return c


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n", [5, 7, 9])
def test_operand_matrix_per_gate(qsim, gpu_ready, n, B):
    from qsim_amd import plan
    c = _operand_circuit(qsim, n)
    P = len(_slots(c))
    rng = np.random.default_rng(100 * n + B)
    terms = gc.random_terms(rng, n, 12, 5)
    h = gc.to_pauli_sum(qsim, n, terms)
    assert not plan.batch_gradient_plan(c, B, h)["fused"]
    a = rng.uniform(-math.pi, math.pi, size=(B, P))
    _check(_batch(qsim, n, B).gradientSweep(c, a, h), _oracle(c, a, terms), terms, f"n={n} B={B}")


# ---- the fused path ----
def _fused_case(qsim, n, seed=None):
    pairs = [(a, b) for a in (0, 6, 12, 13) for b in (0, 6, 12, 13) if a != b] if n == 14 else []
    c = _random_circuit(qsim, n, 40, (100 + n) if seed is None else seed, extra_pairs=pairs)
    terms = gc.random_terms(np.random.default_rng(n), n, 12, 5)
    return c, terms, gc.to_pauli_sum(qsim, n, terms)


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n", [10, 12, 14])
def test_fused_matches_oracle(qsim, gpu_ready, n, B):
    """At n = 14 a member spans several tiles and every ordered (control, target) pair over
    {0, 6, 12, 13} is a CRY: some control lies outside some tile."""
    from qsim_amd import plan
    c, terms, h = _fused_case(qsim, n)
    P = len(_slots(c))
    assert P >= 12 and plan.batch_gradient_plan(c, B, h)["fused"]
    rng = np.random.default_rng(7 * n + B)
    sim = _batch(qsim, n, B)
    for a in _angle_sets(rng, B, P):
        sim.reset()
        _check(sim.gradientSweep(c, a, h), _oracle(c, a, terms), terms, f"n={n} B={B}")


def test_paths_agree(qsim, gpu_ready, monkeypatch):
    n, B = 12, 3
    c, terms, h = _fused_case(qsim, n, seed=31)
    a = np.random.default_rng(9).uniform(-3, 3, size=(B, len(_slots(c))))
    want = _batch(qsim, n, B).gradientSweep(c, a, h)
    _check(_batch(qsim, n, B).gradientSweep(c, a, h, per_gate=True), want, terms, "per_gate")
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", "0")
    _check(_batch(qsim, n, B).gradientSweep(c, a, h), want, terms, "composed step")
    _check(_batch(qsim, n, B).gradientSweep(c, a, h, per_gate=True), want, terms, "composed step, per_gate")


def test_thirteen_qubit_tiles(qsim, gpu_ready):
    from qsim_amd import plan
    n, B = 14, 2
    c, terms, h = _fused_case(qsim, n, seed=77)
    a = np.random.default_rng(5).uniform(-3, 3, size=(B, len(_slots(c))))
    want = _batch(qsim, n, B).gradientSweep(c, a, h)
    plan.set_tile_height(7)
    try:
        for rb7 in (4, 3):
            plan.set_tile_rb7(rb7)
            _check(_batch(qsim, n, B).gradientSweep(c, a, h), want, terms, f"h=7 rb={rb7}")
    finally:
        plan.set_tile_rb7(-1)
        plan.set_tile_height(-1)


# ---- bitwise properties ----
def test_members_are_independent_bitwise(qsim, gpu_ready):
    n, B = 12, 5
    c, terms, h = _fused_case(qsim, n, seed=61)
    P = len(_slots(c))
    rng = np.random.default_rng(4)
    a = rng.uniform(-3, 3, size=(B, P))
    v, g = _batch(qsim, n, B).gradientSweep(c, a, h)
    v_again, g_again = _batch(qsim, n, B).gradientSweep(c, a, h)  # reproducible on a fresh object
    assert v.tobytes() == v_again.tobytes() and g.tobytes() == g_again.tobytes()
    order = np.array([3, 0, 4, 1, 2])
    vp, gp = _batch(qsim, n, B).gradientSweep(c, a[order], h)
    assert vp.tobytes() == v[order].tobytes() and gp.tobytes() == np.ascontiguousarray(g[order]).tobytes()
    other = a.copy()
    other[2] = rng.uniform(-3, 3, size=P)
    vo, go = _batch(qsim, n, B).gradientSweep(c, other, h)
    keep = [0, 1, 3, 4]
    assert vo[keep].tobytes() == v[keep].tobytes() and go[keep].tobytes() == g[keep].tobytes()
    assert vo[2] != v[2] and (go[2] != g[2]).any()


def test_agrees_with_the_single_state_gradient(qsim, gpu_ready):
    n, B = 10, 3
    c, terms, h = _fused_case(qsim, n)
    slots = _slots(c)
    a = np.random.default_rng(2).uniform(-3, 3, size=(B, len(slots)))
    v, g = _batch(qsim, n, B).gradientSweep(c, a, h)
    for t in range(B):
        gates = _gates(c)
        for k, i in enumerate(slots):
            gates[i] = (gates[i][0], gates[i][1], float(a[t, k]))
        sv, sg = qsim.Simulator(n).gradient(gc.to_circuit(qsim, n, gates), h)
        assert abs(v[t] - sv) < gc.bound(terms)
        assert np.abs(g[t] - np.asarray(sg)[slots]).max() < gc.bound(terms)


@pytest.mark.parametrize("n,per_gate", [(12, False), (8, False), (11, True)])
def test_state_left_behind(qsim, gpu_ready, n, per_gate):
    """The members and the qubit layout are what runSweep leaves; the values are what getExpectations
    then returns."""
    B = 3
    c, terms, h = _fused_case(qsim, n, seed=71)
    a = np.random.default_rng(6).uniform(-3, 3, size=(B, len(_slots(c))))
    grad, swept = _batch(qsim, n, B), _batch(qsim, n, B)
    v, _ = grad.gradientSweep(c, a, h, per_gate=per_gate)
    swept.runSweep(c, a, per_gate=per_gate)
    assert grad.perm() == swept.perm()
    assert grad.getExpectations(h).tobytes() == v.tobytes() == swept.getExpectations(h).tobytes()
    assert _same_bits([grad.getStateVector(t) for t in range(B)], [swept.getStateVector(t) for t in range(B)])


def test_non_basis_start(qsim, gpu_ready):
    n, B = 11, 3
    c0 = _random_circuit(qsim, n, 30, 41)
    c, terms, h = _fused_case(qsim, n, seed=42)
    a = np.random.default_rng(3).uniform(-3, 3, size=(B, len(_slots(c))))
    sim = _batch(qsim, n, B)
    sim.run(c0)
    start = [gc.run(gc.basis_state(n), n, _gates(c0))] * B
    _check(sim.gradientSweep(c, a, h), _oracle(c, a, terms, start), terms, "after run()")


def test_edges(qsim, gpu_ready):
    n, B = 10, 3
    c, terms, h = _fused_case(qsim, n, seed=81)
    P = len(_slots(c))
    a = np.random.default_rng(8).uniform(-3, 3, size=(B, P))
    # P = 0: the values alone
    ghz = qsim.createGHZCircuit(n)
    assert not _slots(ghz)
    sim, plain = _batch(qsim, n, B), _batch(qsim, n, B)
    v, g = sim.gradientSweep(ghz, np.zeros((B, 0)), h)
    plain.run(ghz)
    assert g.shape == (B, 0) and v.tobytes() == plain.getExpectations(h).tobytes()
    # an empty circuit: the values of the current states
    v, g = sim.gradientSweep(qsim.Circuit(n), np.zeros((B, 0)), h)
    assert g.shape == (B, 0) and v.tobytes() == plain.getExpectations(h).tobytes()
    # H = 0: zeros (no terms; terms that cancel)
    for empty in (qsim.PauliSum(n), gc.to_pauli_sum(qsim, n, [(6, 1, 0.4), (6, 1, -0.4)])):
        v, g = _batch(qsim, n, B).gradientSweep(c, a, empty)
        assert v.shape == (B,) and g.shape == (B, P) and not v.any() and not g.any()
    # a (P,) row goes to every member
    sim = _batch(qsim, n, B)
    v, g = sim.gradientSweep(c, a[1], h)
    want = _batch(qsim, n, B).gradientSweep(c, np.tile(a[1], (B, 1)), h)
    assert v.tobytes() == want[0].tobytes() and g.tobytes() == want[1].tobytes()
    assert (v == v[0]).all() and (g == g[0]).all()
    _check((v, g), _oracle(c, np.tile(a[1], (B, 1)), terms), terms, "broadcast row")
    # the work ensembles released and allocated again: the same bits
    sim.releaseGradientBuffers()
    sim.releaseGradientBuffers()
    sim.reset()
    v2, g2 = sim.gradientSweep(c, a[1], h)
    assert v2.tobytes() == v.tobytes() and g2.tobytes() == g.tobytes()


def test_errors_leave_the_states(qsim, gpu_ready):
    n, B = 10, 3
    c, terms, h = _fused_case(qsim, n, seed=81)
    P = len(_slots(c))
    sim = _batch(qsim, n, B)
    sim.run(qsim.createGHZCircuit(n))
    before = [sim.getStateVector(t).tobytes() for t in range(B)]
    good = np.full((B, P), 0.3)
    for bad in (np.zeros((B, P + 1)), np.zeros((B + 1, P)), np.zeros(P - 1), np.zeros((B, P, 1)), np.zeros((P, B))):
        with pytest.raises(ValueError):
            sim.gradientSweep(c, bad, h)
    with pytest.raises(ValueError):
        sim.gradientSweep(qsim.Circuit(n + 1), np.zeros((B, 0)), h)
    with pytest.raises(ValueError):
        sim.gradientSweep(c, good, qsim.PauliSum(n + 1))
    nm = qsim.NoiseModel()
    nm.addBitFlip([1], 0.1)
    sim.setNoiseModel(nm)
    with pytest.raises(ValueError):
        sim.gradientSweep(c, good, h)
    sim.setNoiseModel(qsim.NoiseModel())
    sim.setGateSet(qsim.BatchedGateSet.Reference)
    with pytest.raises(ValueError):
        sim.gradientSweep(c, good, h)
    sim.setGateSet(qsim.BatchedGateSet.Full)
    sim.setNoiseSemantics(qsim.BatchedNoise.Reference)
    with pytest.raises(ValueError):
        sim.gradientSweep(c, good, h)
    sim.setNoiseSemantics(qsim.BatchedNoise.Physical)
    with pytest.raises(ValueError):  # an angle that is not finite: refused by the engine before any launch
        sim.gradientSweep(c, np.full((B, P), np.nan), h)
    assert [sim.getStateVector(t).tobytes() for t in range(B)] == before
    start = [np.frombuffer(b, dtype=np.complex128) for b in before]
    _check(sim.gradientSweep(c, good, h), _oracle(c, good, terms, start), terms, "after the refusals")


def test_profile_names(qsim, gpu_ready):
    n, B = 10, 2
    c, terms, h = _fused_case(qsim, n)
    sim = _batch(qsim, n, B)
    sim.profile(True)
    sim.gradientSweep(c, np.full((B, len(_slots(c))), 0.4), h)
    stats = {s["name"]: s for s in sim.profileStats()}
    P = len(_slots(c))
    assert stats["batch_adjoint_step"]["launches"] == P - 1
    assert stats["batch_braket"]["launches"] == 1  # the first slot: nothing left to un-apply
    ctrl = [len(g.qubits) == 2 for g in c.getGates() if int(g.type) in gc.PARAMETRIC]
    pairs = [B * (1 << n) / (4 if k else 2) for k in ctrl]
    assert stats["batch_adjoint_step"]["alg_bytes"] == 128 * sum(pairs[1:])
    assert stats["batch_braket"]["alg_bytes"] == 64 * pairs[0]
