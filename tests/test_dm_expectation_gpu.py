"""Density-matrix expectation values on the device (qsim_dm_expectation, csrc/hip/dm_expect.hip):
DensityMatrix.expectation / DensityMatrixSimulator.expectation against the dense Kronecker checker
of tests/dm_expectation_cases.py.

Tolerances (S = sum_t |c_t|):
  A, the reduction alone: against the checker on the matrix the same object holds.  1e-12 S — a
     fixed-order sum of 2^n products stays below 4 * 2^n * 2^-52 per unit weight, 4.5e-13 at n = 9.
  B, the whole path: against the checker on the oracle's rho (oracle/numpy_oracle.py dm_run).
     2^n * 1e-12 S — the project's 1e-12 per component of rho over the 2^n elements a string reads.
"""
import numpy as np
import pytest

from dm_expectation_cases import (abs_sum, add_all, dense_expectation, heisenberg, random_strings, tfim,
                                  z_only_strings)
from test_density import _circuit, _noise

pytestmark = pytest.mark.gpu


def relabeled_channels(n):  # the channel list of test_density._relabeled_runs
    return [(0, -1, 0.03), (2, 1, 0.2), (1, 2, 0.1), (3, n - 1, 0.05), (4, 0, 0.1)]


def tol_a(obs):
    return 1e-12 * abs_sum(obs)


def tol_b(obs):
    return (1 << obs.getNumQubits()) * 1e-12 * abs_sum(obs)


def check(got, rho, obs, tol, what):
    want = dense_expectation(rho, obs)
    print(f"{what}: got {got!r} want {want!r} |diff| {abs(got - want):.3e} tol {tol:.3e}")
    assert abs(got - want) <= tol, what


@pytest.mark.parametrize("n", [1, 2, 3])
def test_loaded_non_hermitian_matrix_identity_layout(qsim, gpu_ready, n):
    """A random complex NON-Hermitian matrix loaded as it is: every single-qubit Pauli on every
    qubit and XY / YY / YZ / XYZ strings pin the Y phase, the row / column orientation and that all
    2^n values of i are summed (no Hermiticity shortcut); the identity string is the trace."""
    rng = np.random.default_rng(100 + n)
    d = 1 << n
    m = rng.uniform(-1, 1, (d, d)) + 1j * rng.uniform(-1, 1, (d, d))
    assert np.abs(m - m.conj().T).max() > 0.1
    rho = qsim.DensityMatrix(n)
    rho.state.fromHost(m.reshape(-1))
    strings = [{k: letter} for k in range(n) for letter in "XYZ"]
    if n >= 2:
        strings += [{0: "X", 1: "Y"}, {0: "Y", 1: "X"}, {0: "Y", 1: "Y"}, {0: "Y", 1: "Z"}, {n - 1: "Y", 0: "Z"}]
    if n >= 3:
        strings += [{0: "X", 1: "Y", 2: "Z"}, {2: "X", 0: "Y", 1: "Z"}, {0: "Y", 1: "Y", 2: "Y"}]
    for k, f in enumerate(strings):
        obs = qsim.PauliSum(n).add(0.5 + 0.25 * k, f)
        check(rho.expectation(obs), m, obs, tol_a(obs), f"n={n} {f}")
    allsum = qsim.PauliSum(n)
    for k, f in enumerate(strings):
        allsum.add((-1) ** k * (0.3 + 0.1 * k), f)
    allsum.add(0.7, {})
    check(rho.expectation(allsum), m, allsum, tol_a(allsum), f"n={n} all strings")
    ident = qsim.PauliSum(n).add(1.0, {})
    assert abs(rho.expectation(ident) - np.trace(m).real) <= tol_a(ident)
    np.testing.assert_array_equal(rho.getMatrix(), m)  # the buffer is as it was loaded


@pytest.fixture(scope="module")
def relabeled_case(qsim, oracle):
    """n = 8: the circuits, the channel list of test_density._relabeled_runs, the oracle's rho after
    one and after two runs, and the three observables."""
    n = 8
    channels = relabeled_channels(n)
    c1 = _circuit(qsim, n, 30, 21)
    c2 = _circuit(qsim, n, 15, 121)
    want1 = oracle.dm_run(n, oracle.gates_of(c1), channels)
    want2 = oracle.dm_run(n, oracle.gates_of(c2), channels, rho=want1)
    obs = {"tfim": tfim(qsim, n), "heisenberg": heisenberg(qsim, n),
           "random": random_strings(qsim, n, 40, 4, 77)}
    for w in (want1, want2):
        w.setflags(write=False)
    return n, channels, c1, c2, want1, want2, obs


def test_relabeled_layout_is_read_in_place(qsim, gpu_ready, relabeled_case):
    """The first fused run of a reset rho relabels the 16 index bits; expectation() reads rho
    under those labels and leaves perm, layoutInfo and lastRunInfo alone.  A against the matrix read
    back afterwards, B against the oracle; then a second run with no reader in between, B again."""
    n, channels, c1, c2, want1, want2, obs = relabeled_case
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c1)
    st = sim.density.state
    assert st.layoutInfo()["relabeled"]
    before = (st.perm(), st.layoutInfo(), st.lastRunInfo())
    assert before[0] != list(range(2 * n))
    got = {k: sim.expectation(h) for k, h in obs.items()}
    assert (st.perm(), st.layoutInfo(), st.lastRunInfo()) == before
    assert sim.density.expectation(obs["tfim"]) == got["tfim"]
    m = sim.getDensityMatrix()  # (only now: this reader restores the identity layout)
    for k, h in obs.items():
        check(got[k], m, h, tol_a(h), f"A {k}")
        check(got[k], want1, h, tol_b(h), f"B {k}")
        check(sim.expectation(h), m, h, tol_a(h), f"A {k}, identity layout")
    sim.run(c2)
    for k, h in obs.items():
        check(sim.expectation(h), want2, h, tol_b(h), f"B {k}, second run")
    # the same two runs with no reader at all: the second one keeps the first one's labels
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c1)
    sim.run(c2)
    assert sim.density.state.layoutInfo()["relabeled"]
    for k, h in obs.items():
        check(sim.expectation(h), want2, h, tol_b(h), f"B {k}, two runs under the labels")
    assert sim.density.state.layoutInfo()["relabeled"]


def test_row_chunking_300_z_strings(qsim, oracle, gpu_ready):
    """n = 9, one group of 300 terms: two rows (256 + 44) of one launch, after a short noisy run."""
    n = 9
    channels = [(0, -1, 0.02), (1, 3, 0.1)]
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(_circuit(qsim, n, 12, 5))
    obs = z_only_strings(qsim, n, 300, 5)
    assert obs.size() == 300
    got = sim.expectation(obs)
    check(got, sim.getDensityMatrix(), obs, tol_a(obs), "A 300 Z strings")
    # with X / Y strings of several groups beside them: rows of different groups in one launch,
    # read under the relabeled bits of a fresh run
    for k in range(n):
        obs.add(0.1 * (k + 1), {k: "X", (k + 4) % n: "Y"})
    add_all(obs, random_strings(qsim, n, 30, 4, 6))
    sim.reset()
    sim.run(_circuit(qsim, n, 12, 5))
    print("layout:", sim.density.state.layoutInfo())
    got = sim.expectation(obs)
    check(got, sim.getDensityMatrix(), obs, tol_a(obs), "A 300 Z strings + 39 X/Y strings")


def test_index_bits_above_a_work_group_run(qsim, gpu_ready):
    """n = 9: a work-group's 256 values of i share bit 8, so X / Y / Z on qubit 8 (and 7, the top
    bit inside a run) take the kernel's other address part.  A random non-Hermitian matrix makes
    every string's value generic (no term is zero by symmetry); each is checked on its own."""
    n = 9
    d = 1 << n
    rng = np.random.default_rng(9)
    m = rng.uniform(-1, 1, (d, d)) + 1j * rng.uniform(-1, 1, (d, d))
    rho = qsim.DensityMatrix(n)
    rho.state.fromHost(m.reshape(-1))
    strings = [{8: "X"}, {8: "Y"}, {8: "Z"}, {7: "X"}, {7: "Y"}, {8: "X", 7: "X"}, {8: "Y", 7: "Z"},
               {8: "X", 0: "Y"}, {8: "Z", 3: "X"}, {8: "Y", 7: "X", 2: "Z", 0: "Y"}, {8: "Z", 7: "Z", 1: "X"}]
    total = qsim.PauliSum(n)
    for k, f in enumerate(strings):
        obs = qsim.PauliSum(n).add(1.0 + 0.1 * k, f)
        assert abs(dense_expectation(m, obs)) > 1e-3  # the string is visible in this matrix
        check(rho.expectation(obs), m, obs, tol_a(obs), f"n=9 {f}")
        total.add(0.5 - 0.1 * k, f)
    check(rho.expectation(total), m, total, tol_a(total), "n=9 all strings")


def test_maximally_mixed_gives_identity_coefficient(qsim, gpu_ready):
    n = 6
    rho = qsim.DensityMatrix(n)
    rho.initMaximallyMixed()
    for obs in (tfim(qsim, n), heisenberg(qsim, n), random_strings(qsim, n, 20, 4, 3)):
        assert abs(rho.expectation(obs)) <= tol_a(obs)
        obs.add(-1.75, {})
        assert abs(rho.expectation(obs) + 1.75) <= tol_a(obs)


def test_pure_product_state_matches_state_vector(qsim, gpu_ready):
    n = 7
    c = qsim.Circuit(n)
    for k in range(n):
        c.ry(k, 0.3 + 0.4 * k)
        c.rz(k, 1.1 - 0.3 * k)
        c.rx(k, 0.2 * k - 0.5)
    sv = qsim.Simulator(n)
    sv.run(c)
    rho = qsim.DensityMatrix(n)
    rho.initFromPureState(sv.getStateVector())
    for obs in (tfim(qsim, n), heisenberg(qsim, n), random_strings(qsim, n, 30, 4, 9)):
        got, want = rho.expectation(obs), sv.expectation(obs)
        print(f"pure: rho {got!r} psi {want!r} |diff| {abs(got - want):.3e} tol {tol_a(obs):.3e}")
        assert abs(got - want) <= tol_a(obs)


def test_reference_y_sign_is_read_as_stored(qsim, oracle, gpu_ready):
    """setReferenceCompatible(): Y as the reference computes it (-Y rho Y^dag, trace -1 after one
    Y): the value is linear in the stored rho, so it follows the oracle's reference-Y run."""
    n = 8
    channels = [(0, -1, 0.02), (4, 2, 0.1)]
    c = _circuit(qsim, n, 14, 31)
    c.y(3)
    want = oracle.dm_run(n, oracle.gates_of(c), channels, reference_y=True)
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.setReferenceCompatible()
    sim.run(c)
    for obs in (tfim(qsim, n), random_strings(qsim, n, 20, 4, 13), qsim.PauliSum(n).add(1.0, {})):
        check(sim.expectation(obs), want, obs, tol_b(obs), "B reference Y")


def test_reproducible_and_edges(qsim, oracle, gpu_ready):
    n = 7
    channels = [(0, -1, 0.04), (1, 1, 0.2), (3, 5, 0.1)]
    c = _circuit(qsim, n, 25, 8)
    want = oracle.dm_run(n, oracle.gates_of(c), channels)
    obs = random_strings(qsim, n, 30, 4, 21)
    for k in range(n - 1):
        obs.add(-1.0, {k: "Z", k + 1: "Z"}).add(-0.7, {k: "X"})
    sim =qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c)
    a, b = sim.expectation(obs), sim.expectation(obs)
    assert a == b  # bitwise: fixed-order sums, no atomics
    assert sim.expectation(qsim.PauliSum(n)) == 0.0
    # a qubit-count mismatch raises what StateVector.expectation raises for it
    for bad in (qsim.PauliSum(n + 1).add(1.0, {0: "Z"}), qsim.PauliSum(n - 1)):
        with pytest.raises(ValueError) as sv_err:
            qsim.StateVector(n).expectation(bad)
        for holder in (sim, sim.density):
            with pytest.raises(ValueError) as dm_err:
                holder.expectation(bad)
            assert str(dm_err.value) == str(sv_err.value)
    # per-gate mode: the same value from the per-gate kernels' rho
    per_gate = qsim.DensityMatrixSimulator(n, _noise(qsim, channels), mode=qsim.RunMode.PerGate)
    per_gate.run(c)
    check(per_gate.expectation(obs), want, obs, tol_b(obs), "B per-gate mode")
    check(a, want, obs, tol_b(obs), "B fused mode")
    # a collapsed, renormalised rho
    sim.setSeed(3)
    bit = sim.measureQubit(2)
    got = sim.expectation(obs)
    m = sim.getDensityMatrix()
    check(got, m, obs, tol_a(obs), f"A after measureQubit -> {bit}")
    z2 = qsim.PauliSum(n).add(1.0, {2: "Z"})
    assert abs(sim.expectation(z2) - (1 - 2 * bit)) <= 1e-12
