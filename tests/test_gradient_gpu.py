"""Adjoint-method gradients on the device (csrc/hip/adjoint.hip; qsim_state_gradient,
qsim_state_apply_pauli_sum, qsim_state_inner_product).

Reference: the dense numpy restatement of the recurrence in tests/gradient_cases.py (itself checked
against the exact parameter shift and central differences in tests/test_gradient_cpu.py).  Values
and gradients are compared at 1e-12 * sum |c_t|, amplitudes of H src at the same bar per component.
"""
import ctypes
import functools

import numpy as np
import pytest

import gradient_cases as gc

pytestmark = pytest.mark.gpu


def gradient(qsim, n, gates, terms, mode=None, psi0=None):
    """(value, grad, simulator) of Simulator.gradient from |0..0> or a loaded start state."""
    sim = qsim.Simulator(n)
    if psi0 is not None:
        sim.state.fromHost(psi0)
    mode = qsim.RunMode.Fused if mode is None else mode
    value, grad = sim.gradient(gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms), mode)
    return value, grad, sim


def check(got, want, terms, what=""):
    (gv, gg), (wv, wg) = got, want
    assert gg.shape == wg.shape
    assert abs(gv - wv) < gc.bound(terms), (what, gv, wv)
    err = np.abs(gg - wg)
    assert err.max() < gc.bound(terms), (what, int(err.argmax()), float(err.max()))


# ---- closed forms at n = 1, 2 ----
@pytest.mark.parametrize("fused", ["1", "0"])
def test_closed_forms(qsim, gpu_ready, monkeypatch, fused):
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
    th, tol = 0.61, 1e-12
    z0 = [(0, 1, 1.0)]
    # The circuit's first parameterised gate is the sweep's last step, a reduction with nothing to
    # undo; behind a leading RZ(0) the gate under test takes the step proper.
    for t, want in ((gc.RY, (np.cos(th), -np.sin(th))), (gc.RX, (np.cos(th), -np.sin(th))), (gc.RZ, (1.0, 0.0))):
        for head in ([], [(gc.RZ, [0], 0.0)]):
            v, g, _ = gradient(qsim, 1, head + [(t, [0], th)], z0)
            assert abs(v - want[0]) < tol and abs(g[len(head)] - want[1]) < tol, (t, head, v, g)
    z1 = [(0, 2, 1.0)]
    for head in ([], [(gc.RZ, [1], 0.0)]):
        k = len(head)
        v, g, _ = gradient(qsim, 2, head + [(gc.X, [0], 0.0), (gc.CRY, [0, 1], th), (gc.RZ, [0], 0.3)], z1)
        assert abs(v - np.cos(th)) < tol and g[k] == 0.0 and abs(g[k + 1] + np.sin(th)) < tol
        assert abs(g[k + 2]) < tol
        v, g, _ = gradient(qsim, 2, head + [(gc.CRY, [0, 1], th), (gc.RY, [0], 0.0)], z1)  # control at |0>
        assert abs(v - 1.0) < tol and g[k] == 0.0  # exactly: the control == 1 half is all zeros


# ---- applyPauliSum against numpy at n = 10 ----
@pytest.fixture(scope="module")
def ten(qsim, gpu_ready):
    n = 10
    psi = gc.random_state(np.random.default_rng(10), n)
    psi.setflags(write=False)
    sv = qsim.StateVector(n)
    sv.fromHost(psi)
    return sv, psi


def _apply_cases():
    rng = np.random.default_rng(3)
    cases = {
        "x0": [(0, 0b1011, 0.8), (0, 0, -0.3), (0, 1 << 9, 0.5)],
        "x_bit0": [(1, 0, 0.9), (1, 0b110, -0.2)],
        "x_bit9": [(1 << 9, 0, 0.9), (1 << 9, 0b11, 0.4)],
        "y1": [(0b100001, 0b000001 | 1 << 7, 0.7)],
        "y2": [(0b1100000011, 0b0100000001 | 1 << 4, -0.6)],
        "y3": [(0b1000011001, 0b1000010001 | 1 << 2, 0.5)],
        "mixed": gc.random_terms(rng, 10, 30, 6),
        "merged_and_cancelled": [(5, 3, 0.5), (5, 3, 0.25), (6, 1, 0.4), (6, 1, -0.4)],
    }
    assert [bin(x & z).count("1") for x, z, _ in cases["y1"] + cases["y2"] + cases["y3"]] == [1, 2, 3]
    return cases


@pytest.mark.parametrize("name", sorted(_apply_cases()))
def test_apply_pauli_sum_n10(qsim, ten, name):
    sv, psi = ten
    terms = _apply_cases()[name]
    dst = qsim.StateVector(10)
    sv.applyPauliSum(gc.to_pauli_sum(qsim, 10, terms), dst)
    d = dst.toHost() - gc.apply_h(psi, terms)
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) < gc.bound(terms)
    assert np.array_equal(sv.toHost(), psi)  # the source is only read


def test_apply_group_larger_than_the_term_table(qsim, ten):
    from qsim_amd.plan import gradient_plan
    sv, psi = ten
    rng = np.random.default_rng(9)
    for x in (0, 0b1000100001):
        terms = [(x, z, float(rng.uniform(-1, 1))) for z in range(1, 601)]
        h = gc.to_pauli_sum(qsim, 10, terms)
        assert gradient_plan(qsim.Circuit(10).rx(0, 0.1), h)[2] == 3  # 600 terms, 256 per launch
        dst = qsim.StateVector(10)
        sv.applyPauliSum(h, dst)
        d = dst.toHost() - gc.apply_h(psi, terms)
        assert max(np.abs(d.real).max(), np.abs(d.imag).max()) < gc.bound(terms)


def test_apply_empty_sum_and_rejections(qsim, ten):
    from qsim_amd import _lib
    sv, psi = ten
    dst = qsim.StateVector(10)
    sv.applyPauliSum(qsim.PauliSum(10), dst)
    assert not dst.toHost().any()
    h = gc.to_pauli_sum(qsim, 10, [(1, 0, 1.0)])
    with pytest.raises(ValueError):
        sv.applyPauliSum(h, sv)  # src == dst
    with pytest.raises(ValueError):
        sv.applyPauliSum(h, qsim.StateVector(9))
    arr = (_lib.qsim_pauli_term * 1)()
    arr[0].x_mask, arr[0].z_mask, arr[0].coeff = 1 << 10, 0, 1.0
    f = _lib.hip.qsim_state_apply_pauli_sum
    assert f(sv.handle, dst.handle, arr, 1) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert f(sv.handle, dst.handle, None, 1) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(None, dst.handle, arr, 1) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(sv.handle, None, arr, 1) == _lib.QSIM_ERR_INVALID_ARGUMENT


# ---- innerProduct ----
@pytest.mark.parametrize("n", [10, 21])  # 21: the grid-stride loop takes more than one trip
def test_inner_product(qsim, gpu_ready, n):
    from qsim_amd import _lib
    rng = np.random.default_rng(n)
    a, b = gc.random_state(rng, n), gc.random_state(rng, n)
    sa, sb = qsim.StateVector(n), qsim.StateVector(n)
    sa.fromHost(a)
    sb.fromHost(b)
    got = sa.innerProduct(sb)
    want = np.vdot(a, b)
    assert abs(got.real - want.real) < 1e-12 and abs(got.imag - want.imag) < 1e-12
    again = sa.innerProduct(sb)
    assert got.real == again.real and got.imag == again.imag  # bitwise
    norm = sa.innerProduct(sa)
    assert abs(norm.real - sa.getTotalProbability()) < 1e-12 and abs(norm.imag) < 1e-12
    if n == 10:
        out = (ctypes.c_double * 2)()
        f = _lib.hip.qsim_state_inner_product
        assert f(sa.handle, sb.handle, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
        assert f(None, sb.handle, out) == _lib.QSIM_ERR_INVALID_ARGUMENT
        assert f(sa.handle, qsim.StateVector(9).handle, out) == _lib.QSIM_ERR_INVALID_ARGUMENT


# ---- the operand matrix of the step kernel ----
def _frame(n):
    """A fixed entangling prefix and suffix: both work states are dense at the gate under test."""
    pre = [(gc.H, [q], 0.0) for q in range(n)] + [(gc.CNOT, [q, q + 1], 0.0) for q in range(n - 1)]
    pre += [(gc.RY, [q], 0.3 + 0.2 * q) for q in (0, n // 2, n - 1)]
    post = [(gc.CNOT, [q + 1, q], 0.0) for q in range(n - 1)]
    post += [(gc.RY, [q], -0.4 + 0.1 * q) for q in (1, n - 2)] + [(gc.H, [n // 3], 0.0)]
    return pre, post


def _matrix_terms(n):
    return [(1 | 1 << (n - 1), 1 << 2, 0.6), (1 << (n // 2), 1 << (n // 2) | 1, -0.5), (0, 1 << (n - 1) | 2, 0.8),
            (0b110, 0b011, 0.3), (0, 1, -0.7), (1 << (n - 2), 0, 0.4)]


def _matrix_gates(n):
    out = [(t, [q], 0.9 - 0.13 * q) for t in (gc.RX, gc.RY, gc.RZ) for q in range(n)]
    out += [(t, [c, q], 0.5 + 0.07 * c - 0.05 * q) for t in (gc.CRY, gc.CRZ) for c in range(n) for q in range(n)
            if c != q]
    return out


@functools.lru_cache(maxsize=None)
def _matrix_reference(n):
    """numpy value and whole gradient vector (prefix rotations, the gate under test, suffix) of
    every circuit of the matrix, computed once and shared by both paths."""
    pre, post = _frame(n)
    terms = _matrix_terms(n)
    psi0 = gc.basis_state(n)
    after = (len(pre), gc.run(psi0, n, pre))  # the forward run through the prefix, once
    return [gc.adjoint_gradient(psi0, n, pre + [g] + post, terms, after) for g in _matrix_gates(n)]


@pytest.mark.parametrize("n", [7, 10, 13])
def test_step_operand_matrix(qsim, gpu_ready, monkeypatch, n):
    """Every operand in both paths, the whole gradient vector each time: the entries from the gate
    under test on check its bra-ket, the prefix rotations' entries check its U^† write-back to
    both work states (nothing else depends on it)."""
    pre, post = _frame(n)
    terms = _matrix_terms(n)
    gates = _matrix_gates(n)
    assert len(gates) == 3 * n + 2 * n * (n - 1)
    ref = _matrix_reference(n)
    npre = len(pre)
    prefix_rot = [k for k, g in enumerate(pre) if g[0] in gc.PARAMETRIC]
    # (the reference is not trivially zero: nearly every gate under test has a gradient, and so do
    # the prefix rotations behind it)
    assert sum(abs(wg[npre]) > 1e-6 for _, wg in ref) >= 0.9 * len(gates)
    assert len(prefix_rot) == 3 and all(np.abs(wg[prefix_rot]).max() > 1e-3 for _, wg in ref)
    h = gc.to_pauli_sum(qsim, n, terms)
    sim = qsim.Simulator(n)
    for fused in (None, "0"):
        if fused is None:
            monkeypatch.delenv("QSIM_ADJOINT_FUSED", raising=False)
        else:
            monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
        for g, want in zip(gates, ref):
            sim.reset()
            got = sim.gradient(gc.to_circuit(qsim, n, pre + [g] + post), h)
            check(got, want, terms, (fused, g))


# ---- random circuits over the full gate set ----
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_circuits_n10(qsim, gpu_ready, monkeypatch, seed):
    n = 10
    gates, terms = gc.random_case(seed)
    assert len(gates) == 60 and len(terms) == 12
    want = gc.adjoint_gradient(gc.basis_state(n), n, gates, terms)
    assert np.abs(want[1]).max() > 1e-3 and np.count_nonzero(np.abs(want[1]) > 1e-6) >= 8
    for fused in ("1", "0"):
        monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
        for mode in (qsim.RunMode.Fused, qsim.RunMode.PerGate):
            v, g, _ = gradient(qsim, n, gates, terms, mode)
            check((v, g), want, terms, (fused, mode))
            assert all(g[k] == 0.0 for k, gate in enumerate(gates) if gate[0] not in gc.PARAMETRIC)


def test_arbitrary_start_state(qsim, gpu_ready):
    n = 9
    rng = np.random.default_rng(99)
    psi0 = gc.random_state(rng, n)
    gates = gc.random_gates(rng, n, 40)
    terms = gc.random_terms(rng, n, 10, 4)
    want = gc.adjoint_gradient(psi0, n, gates, terms)
    for mode in (qsim.RunMode.Fused, qsim.RunMode.PerGate):
        v, g, _ = gradient(qsim, n, gates, terms, mode, psi0)
        check((v, g), want, terms, mode)


# ---- the state after gradient ----
@pytest.mark.parametrize("mode_name", ["Fused", "PerGate"])
def test_state_after_gradient_is_what_run_leaves(qsim, gpu_ready, mode_name):
    n = 12
    mode = getattr(qsim.RunMode, mode_name)
    rng = np.random.default_rng(12)
    gates = gc.random_gates(rng, n, 50)
    terms = gc.random_terms(rng, n, 8, 4)
    c = gc.to_circuit(qsim, n, gates)
    sim, twin = qsim.Simulator(n, mode), qsim.Simulator(n, mode)
    v, _ = sim.gradient(c, gc.to_pauli_sum(qsim, n, terms), mode)
    twin.run(c)
    assert sim.state.perm() == twin.state.perm()
    assert sim.state.layoutInfo() == twin.state.layoutInfo()
    assert sim.state.lastRunInfo() == twin.state.lastRunInfo()
    assert v == twin.expectation(gc.to_pauli_sum(qsim, n, terms))
    assert sim.state.maxAbsDiff(twin.state) == 0.0


# ---- layouts at n = 16 ----
def _hc_ansatz(qsim, n, seed):
    """The relabel-prone H / CNOT workload with rotations (plain and controlled) spliced in."""
    rng = np.random.default_rng(seed)
    gates = []
    for k, g in enumerate(qsim.createRandomHCCircuit(n, 100, 1).getGates()):
        gates.append((int(g.type), list(g.qubits), float(g.parameter)))
        if k % 9 == 4:
            gates += gc.random_gates(rng, n, 1, gc.PARAMETRIC)
    return gates


def _layout_terms(n):
    """A ZZ chain with X and Y fields."""
    return ([(0, 3 << k, 1.0) for k in range(n - 1)] + [(1 << k, 0, 0.7) for k in range(n)] +
            [(1 << k, 1 << k, 0.3) for k in range(0, n, 3)])


@pytest.mark.parametrize("relayout", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_layouts_n16(qsim, gpu_ready, monkeypatch, relayout, fused):
    from qsim_amd.plan import set_calibrate, set_relabel, set_relayout
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
    n = 16
    set_relabel(1, 14)
    if relayout:
        set_relayout(2, 16)  # forced: a relayout plan whenever one exists
        set_calibrate(0, -1)
    gates = _hc_ansatz(qsim, n, 16)
    terms = _layout_terms(n)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    sim, twin = qsim.Simulator(n), qsim.Simulator(n)
    v, g = sim.gradient(c, h)
    perm = sim.state.perm()
    assert perm != list(range(n)), "expected the planner to relabel this circuit"
    twin.run(c)
    assert twin.state.perm() == perm and twin.state.layoutInfo() == sim.state.layoutInfo()
    if relayout:
        assert sim.state.layoutInfo()["relayout"]
    want = _layout_reference(n)
    check((v, g), want, terms, (relayout, fused))
    sim.gradient(c, h)  # a second circuit run on the relabeled, non-basis state
    assert sim.state.perm() == perm
    twin.run(c)
    assert sim.state.maxAbsDiff(twin.state) == 0.0  # (restores both layouts: after the perm checks)


@functools.lru_cache(maxsize=None)
def _layout_reference(n):
    import qsim_amd
    gates = _hc_ansatz(qsim_amd, n, 16)
    terms = _layout_terms(n)
    value, grad = gc.adjoint_gradient(gc.basis_state(n), n, gates, terms)
    # (an H / CNOT state annihilates most random Pauli strings: this H is chosen so that it does not)
    assert abs(value) > 0.1 and np.count_nonzero(np.abs(grad) > 1e-3) >= 4
    return value, grad


# ---- multi-trip at n = 21 ----
@pytest.mark.parametrize("fused", ["1", "0"])
def test_multi_trip_n21(qsim, gpu_ready, monkeypatch, fused):
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
    n = 21
    gates = [(gc.H, [0], 0.0), (gc.H, [20], 0.0), (gc.RY, [10], 0.7), (gc.CNOT, [10, 0], 0.0),
             (gc.RX, [20], 0.4), (gc.CRY, [0, 20], 1.1), (gc.RZ, [0], -0.8), (gc.CRZ, [20, 10], 0.6)]
    terms = [(1, 0, 0.5), (1 << 20, 1 << 20 | 1 << 10, -0.7), (0, 1 << 10 | 1, 0.9)]
    want = _trip_reference()
    v, g, _ = gradient(qsim, n, gates, terms)
    check((v, g), want, terms, fused)


@functools.lru_cache(maxsize=None)
def _trip_reference():
    n = 21
    gates = [(gc.H, [0], 0.0), (gc.H, [20], 0.0), (gc.RY, [10], 0.7), (gc.CNOT, [10, 0], 0.0),
             (gc.RX, [20], 0.4), (gc.CRY, [0, 20], 1.1), (gc.RZ, [0], -0.8), (gc.CRZ, [20, 10], 0.6)]
    terms = [(1, 0, 0.5), (1 << 20, 1 << 20 | 1 << 10, -0.7), (0, 1 << 10 | 1, 0.9)]
    return gc.adjoint_gradient(gc.basis_state(n), n, gates, terms)


# ---- reproducibility, memory, edge cases ----
@pytest.mark.parametrize("fused", ["1", "0"])
def test_bitwise_reproducible(qsim, gpu_ready, monkeypatch, fused):
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", fused)
    n = 14
    rng = np.random.default_rng(14)
    gates = gc.random_gates(rng, n, 40)
    terms = gc.random_terms(rng, n, 10, 4)
    v1, g1, sim = gradient(qsim, n, gates, terms)
    v2, g2, _ = gradient(qsim, n, gates, terms)
    assert v1 == v2 and np.array_equal(g1, g2)
    sim.reset()  # the same simulator again, its work buffers reused
    v3, g3 = sim.gradient(gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms))
    assert v1 == v3 and np.array_equal(g1, g3)


def test_memory_is_counted_and_released(qsim, gpu_ready):
    n = 16
    state_bytes = 16 << n
    rng = np.random.default_rng(2)
    c = gc.to_circuit(qsim, n, gc.random_gates(rng, n, 20, [gc.H, gc.CNOT, gc.RY, gc.CRZ]))
    h = gc.to_pauli_sum(qsim, n, gc.random_terms(rng, n, 6, 3))
    sim = qsim.Simulator(n)
    sim.run(c)
    sim.expectation(h)
    before = sim.state.getDeviceMemoryBytes()
    sim.gradient(c, h)
    during = sim.state.getDeviceMemoryBytes()
    assert 2 * state_bytes <= during - before < 2 * state_bytes + (1 << 18)  # + descriptors, results
    sim.gradient(c, h)
    assert sim.state.getDeviceMemoryBytes() == during  # kept between calls, not grown
    sim.releaseGradientBuffers()
    assert sim.state.getDeviceMemoryBytes() == before
    sim.releaseGradientBuffers()  # idempotent


def test_edge_cases_and_error_codes(qsim, gpu_ready):
    from qsim_amd import _lib
    n = 4
    sim = qsim.Simulator(n)
    sim.run(qsim.Circuit(n).h(0).cnot(0, 1))
    h = gc.to_pauli_sum(qsim, n, [(0, 3, 1.0), (3, 0, 0.5)])
    # count == 0: <H> of the state as it is
    v, g = sim.gradient(qsim.Circuit(n), h)
    assert g.shape == (0,) and v == sim.expectation(h) and abs(v - 1.5) < 1e-12
    # nterms == 0: zeros, and the circuit still ran
    twin = qsim.Simulator(n)
    twin.run(qsim.Circuit(n).h(0).cnot(0, 1))
    twin.run(qsim.Circuit(n).ry(2, 0.4))
    v, g = sim.gradient(qsim.Circuit(n).ry(2, 0.4), qsim.PauliSum(n))
    assert v == 0.0 and list(g) == [0.0]
    assert sim.state.maxAbsDiff(twin.state) == 0.0
    # no parameters: all zeros, the value alone; no work buffers are allocated for it
    fresh = qsim.Simulator(n)
    noparam = qsim.Circuit(n).h(0).cnot(0, 1).s(2)
    fresh.run(noparam)
    fresh.expectation(h)
    before = fresh.state.getDeviceMemoryBytes()
    fresh.reset()
    v, g = fresh.gradient(noparam, h)
    assert list(g) == [0.0, 0.0, 0.0] and abs(v - 1.5) < 1e-12
    assert fresh.state.getDeviceMemoryBytes() == before
    with pytest.raises(ValueError):
        sim.gradient(qsim.Circuit(5), h)
    with pytest.raises(ValueError):
        sim.gradient(qsim.Circuit(n), qsim.PauliSum(5))
    arr, cnt = qsim.Circuit(n).rx(0, 0.1).cnot(0, 1).to_abi()
    terms, nterms = h.to_abi(n)
    value = ctypes.c_double(7.0)
    grad = (ctypes.c_double * 2)()
    f = _lib.hip.qsim_state_gradient
    hdl = sim.state.handle
    assert f(None, arr, cnt, terms, nterms, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, None, cnt, terms, nterms, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, arr, cnt, None, nterms, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, arr, cnt, terms, nterms, 1, None, grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, arr, cnt, terms, nterms, 1, ctypes.byref(value), None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    bad = (_lib.qsim_pauli_term * 1)()
    bad[0].x_mask, bad[0].z_mask, bad[0].coeff = 0, 1 << n, 1.0
    assert f(hdl, arr, cnt, bad, 1, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_OUT_OF_RANGE
    arr[1].qubits[1] = n
    assert f(hdl, arr, cnt, terms, nterms, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_OUT_OF_RANGE
    arr[1].qubits[1] = 0
    assert f(hdl, arr, cnt, terms, nterms, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    arr[1].qubits[1] = 1
    arr[1].type = 99
    assert f(hdl, arr, cnt, terms, nterms, 1, ctypes.byref(value), grad) == _lib.QSIM_ERR_RUNTIME
    assert sim.state.maxAbsDiff(twin.state) == 0.0  # rejected calls ran nothing
    assert _lib.hip.qsim_state_gradient_release(None) == _lib.QSIM_ERR_INVALID_ARGUMENT


def test_profile_attributes_the_new_kernels(qsim, gpu_ready, monkeypatch):
    n = 10
    rng = np.random.default_rng(4)
    gates = gc.random_gates(rng, n, 30)
    terms = gc.random_terms(rng, n, 8, 3)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    sim = qsim.Simulator(n)
    sim.state.profile(True)
    sim.gradient(c, h)
    names = {s["name"] for s in sim.state.profileStats()}
    assert {"pauli_apply", "adjoint_step", "braket"} <= names  # braket: the first parameter's step
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", "0")
    sim.state.profileReset()
    sim.reset()
    sim.gradient(c, h)
    stats = {s["name"]: s["launches"] for s in sim.state.profileStats()}
    nparam = sum(g[0] in gc.PARAMETRIC for g in gates)
    assert "adjoint_step" not in stats and stats["braket"] == nparam
