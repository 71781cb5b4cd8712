"""Pauli-string rotations, Trotter evolution and their adjoint gradients on the device
(csrc/hip/pauli_rot.hip; qsim_state_apply_pauli_rotations, qsim_state_pauli_gradient).

Reference: the dense numpy restatement in tests/pauli_rotation_cases.py (itself checked against
the RX / RY / RZ matrices, the exact parameter shift and the exact evolution in
tests/test_pauli_rotation_cpu.py).  Amplitudes are compared at 1e-12 per component (the bar of the
bench-path parity tests), values and gradients at 1e-12 * sum |c_t|.
"""
import functools

import numpy as np
import pytest

import gradient_cases as gc
import pauli_rotation_cases as pc

pytestmark = pytest.mark.gpu
TOL = 1e-12


def factors(n, x, z):
    f = {}
    for q in range(n):
        xb, zb = x >> q & 1, z >> q & 1
        if xb or zb:
            f[q] = "Y" if xb and zb else ("X" if xb else "Z")
    return f


def loaded(qsim, n, psi):
    sim = qsim.Simulator(n)
    sim.state.fromHost(psi)
    return sim


def check_grad(got, want, terms, what=""):
    (gv, gg), (wv, wg) = got, want
    assert gg.shape == wg.shape
    assert abs(gv - wv) < gc.bound(terms), (what, gv, wv)
    if len(wg):
        err = np.abs(gg - wg)
        assert err.max() < gc.bound(terms), (what, int(err.argmax()), float(err.max()))


# ---- closed forms at n = 1, 2, 3 (fewer pairs than one work-group) ----
@pytest.mark.parametrize("n", [1, 2, 3])
def test_weight_one_rotations_are_the_circuit_gates(qsim, gpu_ready, n):
    psi = gc.random_state(np.random.default_rng(n), n)
    th = 0.83
    for q in range(n):
        for letter, gate in (("X", "rx"), ("Y", "ry"), ("Z", "rz")):
            a, b = loaded(qsim, n, psi), loaded(qsim, n, psi)
            a.applyPauliRotation({q: letter}, th)
            c = qsim.Circuit(n)
            getattr(c, gate)(q, th)
            b.state.run(c, qsim.RunMode.PerGate)
            # (exp(-i theta/2 P) exactly: the global phase of Rz included)
            assert pc.max_component_diff(a.getStateVector(), b.getStateVector()) < TOL, (q, letter)


def test_closed_forms(qsim, gpu_ready):
    th = 0.61
    c, s = np.cos(th / 2), np.sin(th / 2)
    sim = loaded(qsim, 2, np.full(4, 0.5, dtype=np.complex128))  # |++>
    sim.applyPauliRotation({0: "Z", 1: "Z"}, th)
    want = 0.5 * np.array([c - 1j * s, c + 1j * s, c + 1j * s, c - 1j * s])
    assert pc.max_component_diff(sim.getStateVector(), want) < TOL
    sim = qsim.Simulator(2)
    sim.applyPauliRotation({0: "X", 1: "X"}, th)
    assert pc.max_component_diff(sim.getStateVector(), [c, 0, 0, -1j * s]) < TOL
    for n in (1, 3):
        psi = gc.random_state(np.random.default_rng(30 + n), n)
        sim = loaded(qsim, n, psi)
        sim.applyPauliRotation({}, th)  # the identity string: a global phase
        assert pc.max_component_diff(sim.getStateVector(), (c - 1j * s) * psi) < TOL
    sim = qsim.Simulator(3)
    sim.applyPauliRotation({0: "Y", 1: "X", 2: "Y"}, th)  # YXY|000> = i^2 |111>
    want = np.zeros(8, dtype=np.complex128)
    want[0], want[7] = c, 1j * s
    assert pc.max_component_diff(sim.getStateVector(), want) < TOL


# ---- one rotation each at n = 10 ----
@pytest.fixture(scope="module")
def psi10():
    psi = gc.random_state(np.random.default_rng(10), 10)
    psi.setflags(write=False)
    return psi


def _single_cases():
    from test_gradient_gpu import _apply_cases
    ys = _apply_cases()
    th = 0.77
    cases = {
        "x_bit0": (1, 0b110, th),
        "x_bit9": (1 << 9, 0b11, th),
        "x_low": (0b1011, 1 << 5 | 1, th),
        "x_across_bit8": (1 << 9 | 1 << 4, 1 << 8 | 1 << 2, th),
        "x_bit8_and_low": (1 << 8 | 0b11, 1 << 9, th),
        "y1": ys["y1"][0][:2] + (th,),
        "y2": ys["y2"][0][:2] + (th,),
        "y3": ys["y3"][0][:2] + (th,),
        "weight10": (0b1111111111, 0b1010110011, th),
        "z1": (0, 1 << 4, th),
        "z3": (0, 0b1000100001, th),
        "z10": (0, 0b1111111111, th),
        "theta0": (0b1000100110, 0b0000100011, 0.0),
        "theta2pi": (0b1000100110, 0b0000100011, 2 * np.pi),
        "z_theta2pi": (0, 0b101, 2 * np.pi),
    }
    assert [bin(cases[k][0] & cases[k][1]).count("1") for k in ("y1", "y2", "y3")] == [1, 2, 3]
    return cases


@pytest.mark.parametrize("name", sorted(_single_cases()))
def test_single_rotation_n10(qsim, gpu_ready, psi10, name):
    x, z, th = _single_cases()[name]
    sim = loaded(qsim, 10, psi10)
    sim.applyPauliRotation(factors(10, x, z), th)
    got = sim.getStateVector()
    assert pc.max_component_diff(got, pc.rotate(psi10, x, z, th)) < TOL
    if name.endswith("theta2pi"):
        assert pc.max_component_diff(got, -psi10) < TOL
    if name == "theta0":
        assert pc.max_component_diff(got, psi10) < TOL


# ---- sequences at n = 10 ----
def _z_run_sequence():
    """Z-only runs of length 1, 5 and 300 between X rotations."""
    rng = np.random.default_rng(5)

    def zs(k):
        return [(0, int(rng.integers(0, 1 << 10)), float(rng.uniform(-np.pi, np.pi))) for _ in range(k)]

    def xr():
        return [(int(rng.integers(1, 1 << 10)), int(rng.integers(0, 1 << 10)), float(rng.uniform(-np.pi, np.pi)))]
    return xr() + zs(1) + xr() + zs(5) + xr() + zs(300) + xr()


def test_random_sequence_n10(qsim, gpu_ready, psi10):
    seq = pc.random_rotations(np.random.default_rng(40), 10, 40)
    assert any(x == 0 for x, _, _ in seq) and any(x != 0 for x, _, _ in seq)
    sim = loaded(qsim, 10, psi10)
    sim.applyPauliRotations(gc.to_pauli_sum(qsim, 10, seq))
    assert pc.max_component_diff(sim.getStateVector(), pc.run_sequence(psi10, seq)) < TOL


def test_z_runs_share_a_pass_and_repeat_bitwise(qsim, gpu_ready, psi10):
    seq = _z_run_sequence()
    assert len(seq) == 310
    ps = gc.to_pauli_sum(qsim, 10, seq)
    sim = loaded(qsim, 10, psi10)
    sim.state.profile(True)
    sim.applyPauliRotations(ps)
    first = sim.getStateVector()
    stats = {s["name"]: s["launches"] for s in sim.state.profileStats()}
    assert stats["pauli_rot"] == 4 and stats["pauli_phase"] == 1 + 1 + 2  # the 300-run: two launches
    assert pc.max_component_diff(first, pc.run_sequence(psi10, seq)) < TOL
    again = loaded(qsim, 10, psi10)
    again.applyPauliRotations(ps)
    assert np.array_equal(again.getStateVector(), first)


# ---- Trotter evolution ----
@pytest.mark.parametrize("order", [1, 2])
def test_evolve_is_the_trotter_sequence(qsim, gpu_ready, order):
    n, time, steps = 8, 0.9, 3
    terms = pc.tfim_terms(n)
    psi = gc.random_state(np.random.default_rng(8), n)
    sim = loaded(qsim, n, psi)
    sim.evolve(gc.to_pauli_sum(qsim, n, terms), time, steps, order)
    want = pc.run_sequence(psi, pc.trotter_sequence(terms, time, steps, order))
    assert pc.max_component_diff(sim.getStateVector(), want) < TOL
    for bad in ((0, 1), (1, 3)):
        with pytest.raises(ValueError):
            sim.evolve(gc.to_pauli_sum(qsim, n, terms), time, *bad)


def test_evolve_of_a_commuting_h_is_exact(qsim, gpu_ready):
    n, time = 8, 1.3
    rng = np.random.default_rng(12)
    terms = [(0, int(rng.integers(1, 1 << n)), float(rng.uniform(-1, 1))) for _ in range(12)]
    psi = gc.random_state(rng, n)
    want = pc.exact_evolve(psi, n, terms, time)
    for steps, order in ((1, 1), (2, 2)):
        sim = loaded(qsim, n, psi)
        sim.evolve(gc.to_pauli_sum(qsim, n, terms), time, steps, order)
        assert pc.max_component_diff(sim.getStateVector(), want) < TOL, (steps, order)


# ---- pauliGradient ----
def test_gradient_closed_form(qsim, gpu_ready):
    th = 0.61
    z = gc.to_pauli_sum(qsim, 1, [(0, 1, 1.0)])
    # behind a leading rotation by 0 the rotation under test takes the step proper (the sequence's
    # first rotation is the sweep's last step, a bra-ket with nothing to undo)
    for head in ([], [(0, 1, 0.0)], [(1, 1, 0.0)]):
        for x, zz in ((1, 0), (1, 1)):  # E = cos theta for X and for Y rotations of |0>
            v, g = qsim.Simulator(1).pauliGradient(gc.to_pauli_sum(qsim, 1, head + [(x, zz, th)]), z)
            assert abs(v - np.cos(th)) < TOL and abs(g[len(head)] + np.sin(th)) < TOL, (head, x, zz, v, g)
        v, g = qsim.Simulator(1).pauliGradient(gc.to_pauli_sum(qsim, 1, head + [(0, 1, th)]), z)
        assert abs(v - 1.0) < TOL and abs(g[len(head)]) < TOL


def _gradient_case(seed):
    n = 10
    rng = np.random.default_rng(100 + seed)
    psi0 = gc.random_state(rng, n)
    seq = pc.random_rotations(rng, n, 12)
    zrot = (0, int(rng.integers(1, 1 << n)), float(rng.uniform(-np.pi, np.pi)))
    if seed == 1:
        seq[0] = zrot  # starts with a Z-only rotation
    elif seed == 2:
        seq[-1] = zrot  # ends with one
    elif seed == 3:
        seq = [s for s in seq if s[0] != 0][:1]  # a single rotation
    elif seed == 4:
        seq = [zrot]
    elif seed == 5:
        seq = [(0, 0, 0.4)] + seq[:6] + [zrot, (0, 3, 0.2), (0, 0, -1.1)]  # identity strings, a Z run
    return psi0, seq, gc.random_terms(rng, n, 8, 4)


@pytest.mark.parametrize("seed", range(1, 11))
def test_gradient_n10(qsim, gpu_ready, seed):
    psi0, seq, terms = _gradient_case(seed)
    want = pc.sequence_gradient(psi0, seq, terms)
    assert np.abs(want[1]).max() > 1e-3
    sim = loaded(qsim, 10, psi0)
    got = sim.pauliGradient(gc.to_pauli_sum(qsim, 10, seq), gc.to_pauli_sum(qsim, 10, terms))
    check_grad(got, want, terms, seed)


def test_gradient_edge_cases(qsim, gpu_ready, psi10):
    n = 10
    rng = np.random.default_rng(77)
    seq = pc.random_rotations(rng, n, 6)
    terms = gc.random_terms(rng, n, 6, 3)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    sim = loaded(qsim, n, psi10)
    v, g = sim.pauliGradient(qsim.PauliSum(n), h)  # count == 0: <H> of the state as it is
    assert g.shape == (0,) and v == sim.expectation(h) and abs(v - gc.expectation(psi10, terms)) < gc.bound(terms)
    assert np.array_equal(sim.getStateVector(), psi10)
    rotated = pc.run_sequence(psi10, seq)
    for zero in (qsim.PauliSum(n), gc.to_pauli_sum(qsim, n, [(5, 3, 0.4), (5, 3, -0.4)])):
        sim = loaded(qsim, n, psi10)
        v, g = sim.pauliGradient(ps, zero)  # H = 0: zeros, and the sequence was still applied
        assert v == 0.0 and list(g) == [0.0] * 6
        assert pc.max_component_diff(sim.getStateVector(), rotated) < TOL


def test_gradient_repeats_bitwise_and_leaves_the_rotated_state(qsim, gpu_ready, psi10):
    n = 10
    rng = np.random.default_rng(78)
    seq = pc.random_rotations(rng, n, 16)
    terms = gc.random_terms(rng, n, 8, 4)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    a, b, plain = loaded(qsim, n, psi10), loaded(qsim, n, psi10), loaded(qsim, n, psi10)
    v1, g1 = a.pauliGradient(ps, h)
    v2, g2 = b.pauliGradient(ps, h)
    assert v1 == v2 and np.array_equal(g1, g2)
    plain.applyPauliRotations(ps)
    assert a.state.maxAbsDiff(plain.state) == 0.0
    assert v1 == plain.expectation(h)
    a.state.fromHost(psi10)  # the same simulator again, its work states reused
    v3, g3 = a.pauliGradient(ps, h)
    assert v1 == v3 and np.array_equal(g1, g3)
    a.state.profile(True)
    a.state.fromHost(psi10)
    a.pauliGradient(ps, h)
    stats = {s["name"]: s["launches"] for s in a.state.profileStats()}
    assert stats["pauli_adjoint_step"] == 16  # every rotation its own step


# ---- layouts at n = 16 ----
def _layout_sequences(n):
    rng = np.random.default_rng(16)
    a = pc.random_rotations(rng, n, 12)
    b = pc.random_rotations(rng, n, 12)
    a[3] = (1 | 1 << (n - 1), 1 << 7, 0.9)
    a[4], a[5] = (0, 0b11, 0.7), (0, 1 << (n - 1) | 1 << 5, -0.4)  # a Z run
    terms = ([(0, 3 << k, 1.0) for k in range(n - 1)] + [(1 << k, 0, 0.7) for k in range(n)] +
             [(1 << k, 1 << k, 0.3) for k in range(0, n, 3)])
    return a, b, terms


@functools.lru_cache(maxsize=None)
def _layout_reference(n):
    import numpy_oracle as orc
    import qsim_amd
    g = orc.gates_of(qsim_amd.createRandomHCCircuit(n, 100, 1))
    a, b, terms = _layout_sequences(n)
    psi_a = pc.run_sequence(orc.run_cpu(n, g), a)
    value, grad = pc.sequence_gradient(psi_a, b, terms)
    assert np.count_nonzero(np.abs(grad) > 1e-3) >= 4
    final = orc.run_cpu(n, g, state=pc.run_sequence(psi_a, b))
    return psi_a, (value, grad), final


@pytest.mark.parametrize("relayout", [False, True])
def test_layouts_n16(qsim, gpu_ready, relayout):
    from qsim_amd.plan import set_calibrate, set_relabel, set_relayout
    n = 16
    set_relabel(1, 14)
    if relayout:
        set_relayout(2, 16)  # forced: a relayout plan whenever one exists
        set_calibrate(0, -1)
    c = qsim.createRandomHCCircuit(n, 100, 1)  # the relabel-prone workload
    a, b, terms = _layout_sequences(n)
    psi_a, want, final = _layout_reference(n)
    sim, twin = qsim.Simulator(n), qsim.Simulator(n)
    sim.run(c)
    twin.run(c)
    perm, info = sim.state.perm(), sim.state.layoutInfo()
    assert perm != list(range(n)), "expected the planner to relabel this circuit"
    if relayout:
        assert info["relayout"]
    last = sim.state.lastRunInfo()
    sim.applyPauliRotations(gc.to_pauli_sum(qsim, n, a))
    got = sim.pauliGradient(gc.to_pauli_sum(qsim, n, b), gc.to_pauli_sum(qsim, n, terms))
    check_grad(got, want, terms, relayout)
    assert sim.state.perm() == perm and sim.state.layoutInfo() == info and sim.state.lastRunInfo() == last
    # the rotated amplitudes themselves, on a twin (reading them restores the layout)
    twin.applyPauliRotations(gc.to_pauli_sum(qsim, n, a))
    assert twin.state.perm() == perm
    assert pc.max_component_diff(twin.getStateVector(), psi_a) < TOL
    # a further run of the circuit on the relabeled, rotated state
    sim.run(c)
    assert pc.max_component_diff(sim.getStateVector(), final) < TOL


# ---- run sharing: pending gates are flushed before a rotation ----
def test_rotation_flushes_a_run_sharing_cycle(qsim, oracle, gpu_ready):
    from qsim_amd.plan import set_relayout
    set_relayout(1, 16)
    n = 16
    c = qsim.createRandomHCCircuit(n, 100, 42)
    g = oracle.gates_of(c)
    ref = oracle.run_cpu(n, g)
    for _ in range(2):
        ref = oracle.run_cpu(n, g, state=ref)
    x, z, th = 1 << 15 | 1 << 3 | 1, 1 << 9 | 1 << 3, 0.7
    sim = qsim.Simulator(n)
    for _ in range(3):  # identical fused runs: the second arms a cycle, the third is a call of it
        sim.run(c)
    sim.applyPauliRotation(factors(n, x, z), th)
    assert pc.max_component_diff(sim.getStateVector(), pc.rotate(ref, x, z, th)) < TOL


# ---- more than one grid-stride trip at n = 21 ----
def test_multi_trip_n21(qsim, gpu_ready):
    n = 21
    prep = qsim.Circuit(n)
    for q in (0, 7, 20):
        prep.h(q)
    prep.cnot(7, 12).ry(12, 0.4)
    psi = gc.run(gc.basis_state(n), n, [(gc.H, [0], 0.0), (gc.H, [7], 0.0), (gc.H, [20], 0.0),
                                        (gc.CNOT, [7, 12], 0.0), (gc.RY, [12], 0.4)])
    x, z, th = 1 << 20 | 1, 1 << 20 | 1 << 12, 0.9  # x bits {0, 20}, nY = 1
    sim = qsim.Simulator(n)
    sim.state.run(prep, qsim.RunMode.PerGate)
    sim.applyPauliRotation(factors(n, x, z), th)
    psi = pc.rotate(psi, x, z, th)
    seq = [(1 << 12, 1 << 12 | 1, 0.5), (0, 1 << 20 | 1 << 7, -0.8), (1 << 20 | 1 << 7, 1, 1.1)]
    terms = [(1, 0, 0.5), (1 << 20, 1 << 20 | 1 << 12, -0.7), (0, 1 << 12 | 1, 0.9)]
    want = pc.sequence_gradient(psi, seq, terms)
    assert np.abs(want[1]).min() > 1e-3
    got = sim.pauliGradient(gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms))
    check_grad(got, want, terms)
    assert pc.max_component_diff(sim.getStateVector(), pc.run_sequence(psi, seq)) < TOL


# ---- the grid-stride loops of pauli_rot and pauli_phase ----
@pytest.mark.parametrize("blocks", ["3", "1"])
def test_streaming_kernels_take_several_trips(qsim, gpu_ready, monkeypatch, blocks):
    """By default a second trip starts at 2^24 pairs; QSIM_PAULI_BLOCKS (read at every call) caps the
    grid, so 12 qubits take 2048 / (3 * 256) = 2.7 trips of pairs (a ragged last one) and 5.3 of
    amplitudes, or 8 and 16 with one work-group.  The amplitudes do not depend on the grid."""
    n = 12
    rng = np.random.default_rng(120)
    psi = gc.random_state(rng, n)
    seq = [(1 << 11 | 1, 1 << 11 | 1 << 5, 0.9), (0, 0b101000000011, -0.6), (0, 1 << 11, 0.3),
           (0b11, 1 << 9, 1.2), (1 << 8 | 1 << 7, 1 << 8 | 1 << 7 | 1, -0.4)]
    ps = gc.to_pauli_sum(qsim, n, seq)
    plain = loaded(qsim, n, psi)
    plain.applyPauliRotations(ps)
    monkeypatch.setenv("QSIM_PAULI_BLOCKS", blocks)
    sim = loaded(qsim, n, psi)
    sim.applyPauliRotations(ps)
    got = sim.getStateVector()
    assert pc.max_component_diff(got, pc.run_sequence(psi, seq)) < TOL
    assert np.array_equal(got, plain.getStateVector())


# ---- errors: raised before anything is applied ----
def test_errors_leave_the_state_unchanged(qsim, gpu_ready, psi10):
    import ctypes
    from qsim_amd import _lib
    n = 10
    sim = loaded(qsim, n, psi10)
    h = gc.to_pauli_sum(qsim, n, [(0, 3, 1.0)])
    with pytest.raises(IndexError):
        sim.applyPauliRotation({0: "X", n: "Z"}, 0.3)
    with pytest.raises(IndexError):
        sim.applyPauliRotation({-1: "X"}, 0.3)
    with pytest.raises(ValueError):
        sim.applyPauliRotations(qsim.PauliSum(n - 1).add(0.3, {0: "X"}))
    with pytest.raises(ValueError):
        sim.pauliGradient(qsim.PauliSum(n + 1).add(0.3, {0: "X"}), h)
    with pytest.raises(ValueError):
        sim.pauliGradient(qsim.PauliSum(n).add(0.3, {0: "X"}), qsim.PauliSum(n - 1))
    with pytest.raises(ValueError):
        sim.evolve(qsim.PauliSum(n - 1).add(1.0, {0: "Z"}), 1.0)
    # the ABI itself: a bad mask at the END of a sequence is found before the first launch
    rots = (_lib.qsim_pauli_term * 3)()
    for k, (x, z, c) in enumerate([(1, 0, 0.4), (0, 5, 0.3), (1 << n, 0, 0.2)]):
        rots[k].x_mask, rots[k].z_mask, rots[k].coeff = x, z, c
    hdl = sim.state.handle
    f = _lib.hip.qsim_state_apply_pauli_rotations
    assert f(hdl, rots, 3) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert f(hdl, None, 3) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(None, rots, 2) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, rots, 0) == _lib.QSIM_OK and f(hdl, None, 0) == _lib.QSIM_OK
    terms, nterms = h.to_abi(n)
    value, grad = ctypes.c_double(7.0), (ctypes.c_double * 3)()
    gf = _lib.hip.qsim_state_pauli_gradient
    assert gf(hdl, rots, 3, terms, nterms, ctypes.byref(value), grad) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert gf(hdl, rots, 2, rots, 3, ctypes.byref(value), grad) == _lib.QSIM_ERR_OUT_OF_RANGE  # a bad TERM
    assert gf(hdl, None, 2, terms, nterms, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gf(hdl, rots, 2, None, nterms, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gf(hdl, rots, 2, terms, nterms, None, grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gf(hdl, rots, 2, terms, nterms, ctypes.byref(value), None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gf(None, rots, 2, terms, nterms, ctypes.byref(value), grad) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert np.array_equal(sim.getStateVector(), psi10)
