"""Host-side pieces of the adjoint-method gradients (no GPU): qsim_gate_inverse, qsim_gradient_plan,
and the numpy restatement of the recurrence (tests/gradient_cases.py) that the GPU tests compare
against, itself checked against the exact parameter shift and central differences."""
import ctypes

import numpy as np
import pytest

import gradient_cases as gc


def test_gate_inverse_all_types(qsim, oracle):
    """Oracle forward, then the engine's inverses in reverse order: back to the start state."""
    from qsim_amd.plan import gate_inverse
    n = 5
    rng = np.random.default_rng(5)
    gates = []
    for t in range(17):  # every type, twice, on random operands
        for _ in range(2):
            gates += gc.random_gates(rng, n, 1, [t])
    assert {g[0] for g in gates} == set(range(17))
    psi0 = gc.random_state(rng, n)
    inv = []
    for t, q, th in reversed(gates):
        op = gate_inverse(qsim.GateOp(qsim.GateType(t), q, th))
        assert op.qubits == q
        inv.append((int(op.type), op.qubits, op.parameter))
    back = oracle.run_cpu(n, gates + inv, psi0)
    assert np.abs(back - psi0).max() < 1e-12
    assert np.abs(oracle.run_cpu(n, gates, psi0) - psi0).max() > 1e-3  # (the circuit does something)
    # the pairs, explicitly
    G = qsim.GateType
    assert gate_inverse(qsim.GateOp(G.S, [1])).type == G.Sdag
    assert gate_inverse(qsim.GateOp(G.Sdag, [1])).type == G.S
    assert gate_inverse(qsim.GateOp(G.T, [1])).type == G.Tdag
    assert gate_inverse(qsim.GateOp(G.Tdag, [1])).type == G.T
    assert gate_inverse(qsim.GateOp(G.CRZ, [1, 0], 0.25)) == qsim.GateOp(G.CRZ, [1, 0], -0.25)
    assert gate_inverse(qsim.GateOp(G.Toffoli, [2, 1, 0])) == qsim.GateOp(G.Toffoli, [2, 1, 0])


def test_gate_inverse_error_codes(qsim):
    from qsim_amd import _lib
    g, out = _lib.qsim_gate(), _lib.qsim_gate()
    f = _lib.hip.qsim_gate_inverse
    assert f(None, ctypes.byref(out)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(ctypes.byref(g), None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    g.type = 17
    assert f(ctypes.byref(g), ctypes.byref(out)) == _lib.QSIM_ERR_RUNTIME


def test_gradient_plan_counts(qsim):
    from qsim_amd.plan import gradient_plan
    n = 4
    c = qsim.Circuit(n)
    c.h(0).cnot(0, 1)            # before the first parameter: never undone
    c.ry(0, 0.1).rz(1, 0.2)      # two parameters back to back: no segment between them
    c.cnot(1, 2).s(2).swap(2, 3)  # segment 1
    c.crz(0, 3, 0.3)
    c.t(1)                       # segment 2
    c.cry(2, 1, 0.4).rx(3, 0.5)
    c.h(2).toffoli(0, 1, 2)      # segment 3 (after the last parameter)
    h = qsim.PauliSum(n)
    h.add(1.0, {0: "Z"}).add(0.5, {1: "Z", 2: "Z"}).add(0.25, {})   # x = 0: one pass
    h.add(0.3, {0: "X"}).add(0.2, {0: "Y", 3: "Z"})                  # x = 1: one pass
    h.add(0.1, {1: "X", 2: "Y"})                                     # x = 6
    h.add(0.7, {3: "X"}).add(-0.7, {3: "X"})                         # cancels: dropped
    assert gradient_plan(c, h) == (5, 3, 3)
    assert gradient_plan(qsim.Circuit(n).h(0).cnot(0, 1), h) == (0, 0, 3)
    assert gradient_plan(c, qsim.PauliSum(n)) == (5, 3, 0)
    # a group larger than one launch's term table takes two passes
    big = qsim.PauliSum(10)
    for z in range(300):
        big.add(1.0 + z, {q: "Z" for q in range(10) if z >> q & 1})
    assert gradient_plan(qsim.Circuit(10).rx(0, 0.1), big) == (1, 0, 2)


def test_gradient_plan_error_codes(qsim):
    from qsim_amd import _lib
    n = 4
    arr, cnt = qsim.Circuit(n).rx(0, 0.1).cnot(0, 1).to_abi()
    terms = (_lib.qsim_pauli_term * 1)()
    terms[0].x_mask, terms[0].z_mask, terms[0].coeff = 0, 1, 1.0
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out = (ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    f = _lib.hip.qsim_gradient_plan
    assert f(n, arr, cnt, terms, 1, *out) == 0 and (a.value, b.value, c.value) == (1, 1, 1)
    assert f(n, None, cnt, terms, 1, *out) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(n, arr, cnt, None, 1, *out) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(n, arr, cnt, terms, 1, None, out[1], out[2]) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(0, arr, cnt, terms, 1, *out) == _lib.QSIM_ERR_INVALID_ARGUMENT
    terms[0].z_mask = 1 << n
    assert f(n, arr, cnt, terms, 1, *out) == _lib.QSIM_ERR_OUT_OF_RANGE
    terms[0].z_mask = 1
    arr[1].qubits[1] = n  # qubit out of range: the code qsim_run gives
    assert f(n, arr, cnt, terms, 1, *out) == _lib.QSIM_ERR_OUT_OF_RANGE
    arr[1].qubits[1] = 0  # control == target
    assert f(n, arr, cnt, terms, 1, *out) == _lib.QSIM_ERR_INVALID_ARGUMENT
    arr[1].qubits[1] = 1
    arr[1].type = 99
    assert f(n, arr, cnt, terms, 1, *out) == _lib.QSIM_ERR_RUNTIME


def test_numpy_gates_match_the_oracle(oracle):
    n = 5
    rng = np.random.default_rng(1)
    gates = gc.random_gates(rng, n, 80)
    assert {g[0] for g in gates} == set(range(17))
    psi0 = gc.random_state(rng, n)
    assert np.abs(gc.run(psi0, n, gates) - oracle.run_cpu(n, gates, psi0)).max() < 1e-13


def test_numpy_adjoint_against_shift_and_central_differences():
    n = 6
    rng = np.random.default_rng(6)
    gates = gc.random_gates(rng, n, 40)
    # (make sure both controlled rotations and all three plain ones are among them)
    gates += [(gc.CRY, [4, 1], 0.7), (gc.CRZ, [0, 5], -1.1), (gc.RX, [2], 0.3), (gc.RY, [3], 2.0), (gc.RZ, [0], -0.4)]
    gates += gc.random_gates(rng, n, 10)
    assert {gc.RX, gc.RY, gc.RZ, gc.CRY, gc.CRZ} <= {g[0] for g in gates}
    terms = gc.random_terms(rng, n, 12, 5)
    psi0 = gc.basis_state(n)
    value, grad = gc.adjoint_gradient(psi0, n, gates, terms)
    assert abs(value - gc.expectation(gc.run(psi0, n, gates), terms)) < gc.bound(terms, 1e-13)
    shift = gc.shift_gradient(psi0, n, gates, terms)
    central = gc.central_gradient(psi0, n, gates, terms)
    exact = [k for k, g in enumerate(gates) if g[0] in (gc.RX, gc.RY, gc.RZ)]
    assert len(exact) >= 5
    assert np.abs(grad[exact] - shift[exact]).max() < gc.bound(terms, 1e-13)
    assert np.abs(grad - central).max() < gc.bound(terms, 1e-7)
    assert np.abs(grad).max() > 1e-2
    assert all(grad[k] == 0.0 for k, g in enumerate(gates) if g[0] not in gc.PARAMETRIC)


def test_random_cases_cover_the_full_gate_set():
    """The three random circuits of tests/test_gradient_gpu.py hold all 17 gate types between them."""
    seen = set()
    for seed in (1, 2, 3):
        seen |= {g[0] for g in gc.random_case(seed)[0]}
    assert seen == set(range(17))
