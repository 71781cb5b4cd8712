"""Density-matrix marginals, partial traces and fidelity on the device (qsim_dm_marginal_probabilities,
qsim_dm_reduced_density_matrix, qsim_dm_fidelity; csrc/hip/dm_marginal.hip) against the dense einsum
checker of tests/dm_marginal_cases.py.

Tolerances are derived, not measured (dm_marginal_cases.tol_*):
  A, the reduction alone: against the checker on the matrix the same object holds.  A fixed-order sum
     of T terms of weight W = sum |terms| stays within 4 T 2^-52 W: T = 2^(n-k) for the subset
     readers (per output, W from that output's terms), T = 4^n and W = sum |psi_i| |rho_ij| |psi_j|
     for the fidelity.
  B, the whole path: against the checker on the oracle's rho (oracle/numpy_oracle.py dm_run): the
     project's 1e-12 per component of rho times the 2^(n-k) components summed; for the fidelity
     1e-12 (sum |psi_i|)^2.
"""
import itertools

import numpy as np
import pytest

import dm_marginal_cases as dc
from test_density import _circuit, _noise
from test_dm_expectation_gpu import relabeled_channels

pytestmark = pytest.mark.gpu


def loaded(qsim, m):
    n = m.shape[0].bit_length() - 1
    rho = qsim.DensityMatrix(n)
    rho.state.fromHost(m.reshape(-1))
    return rho


def tol_purity(want, tol):
    """d sum |z|^2 <= sum 2 |z| |dz| with |dz| <= sqrt 2 * the per-component bound, plus the host
    sum of 4^k squares."""
    return float(np.sum(2 * np.abs(want) * np.sqrt(2) * tol)) + 4 * want.size * dc.U * dc.purity_np(want)


def check_subset_a(holder, m, qs, what):
    """Matrix (k <= 6) and marginal of one subset at A against the matrix m."""
    if len(qs) <= 6:
        dc.check_rdm(holder.reducedDensityMatrix(qs), m, qs, dc.tol_a_rdm(m, qs), what)
    dc.check_marginal(holder.marginalProbabilities(qs), m, qs, dc.tol_a_marginal(m, qs), what)


def check_subset_b(holder, want, qs, what):
    n = want.shape[0].bit_length() - 1
    if len(qs) <= 6:
        dc.check_rdm(holder.reducedDensityMatrix(qs), want, qs, dc.tol_b_subset(n, qs), what)
    dc.check_marginal(holder.marginalProbabilities(qs), want, qs, dc.tol_b_subset(n, qs), what)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_loaded_non_hermitian_matrix_identity_layout(qsim, gpu_ready, n):
    """A random NON-Hermitian matrix loaded as it is pins the row / column orientation and the bit
    order: every subset in every order, k = 0 .. n; k = 0 is the trace, k = n the buffer itself."""
    m = dc.random_matrix(n, 200 + n)
    assert np.abs(m - m.conj().T).max() > 0.1
    rho = loaded(qsim, m)
    for k in range(n + 1):
        for combo in itertools.combinations(range(n), k):
            for qs in itertools.permutations(combo):
                qs = list(qs)
                check_subset_a(rho, m, qs, f"n={n}")
                want = dc.dm_rdm_np(m, qs)
                got = rho.subsystemPurity(qs)
                assert abs(got - dc.purity_np(want)) <= tol_purity(want, dc.tol_a_rdm(m, qs)), (qs, got)
    assert abs(rho.reducedDensityMatrix([])[0, 0] - np.trace(m)) <= 2 * dc.tol_a_rdm(m, [])[0, 0]
    assert abs(rho.marginalProbabilities([])[0] - np.trace(m).real) <= dc.tol_a_marginal(m, [])[0]
    np.testing.assert_array_equal(rho.reducedDensityMatrix(list(range(n))), rho.getMatrix())
    np.testing.assert_array_equal(rho.marginalProbabilities(list(range(n))), rho.getProbabilities())
    np.testing.assert_array_equal(rho.getMatrix(), m)  # the buffer is as it was loaded


@pytest.fixture(scope="module")
def relabeled_case(qsim, oracle):
    """n = 8: the circuits and the channel list of test_dm_expectation_gpu.relabeled_case, the
    oracle's rho after one and after two runs."""
    n = 8
    channels = relabeled_channels(n)
    c1 = _circuit(qsim, n, 30, 21)
    c2 = _circuit(qsim, n, 15, 121)
    want1 = oracle.dm_run(n, oracle.gates_of(c1), channels)
    want2 = oracle.dm_run(n, oracle.gates_of(c2), channels, rho=want1)
    for w in (want1, want2):
        w.setflags(write=False)
    return n, channels, c1, c2, want1, want2


SUBSETS_8 = [[0], [7], [3, 1], [7, 0, 4], [5, 4, 3, 2, 1, 0], [2, 7, 5, 0, 6, 1]]
MARGINALS_8 = [list(range(8)), [6, 2, 7]]


def test_basis_vector_fidelity_is_the_diagonal(qsim, gpu_ready, relabeled_case):
    """fidelity(e_i) == getProbabilities()[i] exactly: every other product is an exact zero.  n = 3
    on a loaded matrix; n = 8 under the relabeled layout for 32 random i."""
    n = 3
    m = dc.random_matrix(n, 31)
    rho = loaded(qsim, m)
    probs = rho.getProbabilities()
    for i in range(1 << n):
        e = np.zeros(1 << n, complex)
        e[i] = 1.0
        assert rho.fidelity(e) == probs[i], i
    psi = dc.random_psi(n, 32)
    dc.check_fidelity(rho.fidelity(psi), m, psi, dc.tol_a_fidelity(m, psi), "n=3 loaded")
    n, channels, c1, _, want1, _ = relabeled_case
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c1)
    assert sim.density.state.layoutInfo()["relabeled"]
    picks = [int(i) for i in np.random.default_rng(8).choice(1 << n, 32, replace=False)]
    got = []
    for i in picks:
        e = np.zeros(1 << n, complex)
        e[i] = 1.0
        got.append(sim.fidelity(e))
    psi = dc.random_psi(n, 33)
    f = sim.fidelity(psi)
    assert sim.density.state.layoutInfo()["relabeled"]
    probs = sim.getProbabilities()  # (only now: this reader restores the identity layout)
    assert got == [probs[i] for i in picks]
    dc.check_fidelity(f, sim.getDensityMatrix(), psi, dc.tol_a_fidelity(sim.getDensityMatrix(), psi), "A n=8 relabeled")
    dc.check_fidelity(f, want1, psi, dc.tol_b_fidelity(psi), "B n=8 relabeled")


def test_relabeled_layout_is_read_in_place(qsim, gpu_ready, relabeled_case):
    """The first fused run of a reset rho relabels the 16 index bits; the readers read rho under
    those labels and leave perm, layoutInfo and lastRunInfo alone.  A against the matrix read back
    afterwards, B against the oracle; then a second run with no restoring reader in between, B again."""
    n, channels, c1, c2, want1, want2 = relabeled_case
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c1)
    st = sim.density.state
    assert st.layoutInfo()["relabeled"]
    before = (st.perm(), st.layoutInfo(), st.lastRunInfo())
    assert before[0] != list(range(2 * n))
    psi = dc.random_psi(n, 34)
    mats = [sim.reducedDensityMatrix(qs) for qs in SUBSETS_8]
    margs = [sim.marginalProbabilities(qs) for qs in SUBSETS_8 + MARGINALS_8]
    fid = sim.fidelity(psi)
    pur = sim.subsystemPurity(SUBSETS_8[3])
    assert (st.perm(), st.layoutInfo(), st.lastRunInfo()) == before
    np.testing.assert_array_equal(sim.density.reducedDensityMatrix(SUBSETS_8[2]), mats[2])
    m = sim.getDensityMatrix()  # (only now: this reader restores the identity layout)
    for qs, got in zip(SUBSETS_8, mats):
        dc.check_rdm(got, m, qs, dc.tol_a_rdm(m, qs), "A")
        dc.check_rdm(got, want1, qs, dc.tol_b_subset(n, qs), "B")
    for qs, got in zip(SUBSETS_8 + MARGINALS_8, margs):
        dc.check_marginal(got, m, qs, dc.tol_a_marginal(m, qs), "A")
        dc.check_marginal(got, want1, qs, dc.tol_b_subset(n, qs), "B")
    dc.check_fidelity(fid, m, psi, dc.tol_a_fidelity(m, psi), "A")
    dc.check_fidelity(fid, want1, psi, dc.tol_b_fidelity(psi), "B")
    want = dc.dm_rdm_np(m, SUBSETS_8[3])
    assert abs(pur - dc.purity_np(want)) <= tol_purity(want, dc.tol_a_rdm(m, SUBSETS_8[3]))
    for qs in SUBSETS_8 + MARGINALS_8:
        check_subset_a(sim, m, qs, "A identity layout")
    sim.run(c2)
    for qs in SUBSETS_8 + MARGINALS_8:
        check_subset_b(sim, want2, qs, "B second run")
    dc.check_fidelity(sim.fidelity(psi), want2, psi, dc.tol_b_fidelity(psi), "B second run")
    # the same two runs with no reader at all: the second one keeps the first one's labels
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c1)
    sim.run(c2)
    assert sim.density.state.layoutInfo()["relabeled"]
    for qs in SUBSETS_8 + MARGINALS_8:
        check_subset_b(sim, want2, qs, "B two runs under the labels")
    dc.check_fidelity(sim.fidelity(psi), want2, psi, dc.tol_b_fidelity(psi), "B two runs under the labels")
    assert sim.density.state.layoutInfo()["relabeled"]


def test_index_bits_above_a_run(qsim, gpu_ready):
    """n = 9, a loaded random matrix: 18 index bits, so qubit 8's row bit (17) and qubit 7's (16) lie
    far above the fidelity kernel's 12-bit run and the gather kernel's 8 thread bits, qubit 8's
    column bit (8) just above the thread bits.  Subsets with qubit 8, qubit 7, both, neither; each
    checked on its own."""
    n = 9
    m = dc.random_matrix(n, 9)
    rho = loaded(qsim, m)
    for qs in ([8], [7], [8, 7], [7, 8], [3, 1], [0, 8, 4], [7, 2, 5], [8, 0, 7, 3], [5, 4, 3, 2, 1, 0],
               [8, 7, 6, 5, 4, 3], [2, 8, 5, 0, 7, 1], [4, 6, 0, 2, 8, 7, 1], list(range(9)), []):
        check_subset_a(rho, m, qs, "n=9")
    for seed, support in ((1, None), (2, [8]), (3, [7]), (4, [8, 7]), (5, [0, 3])):
        psi = dc.random_psi(n, 90 + seed)
        if support is not None:  # amplitudes only where these qubits are 1: one block of rho
            idx = np.arange(1 << n)
            for q in support:
                psi[(idx >> q & 1) == 0] = 0
        dc.check_fidelity(rho.fidelity(psi), m, psi, dc.tol_a_fidelity(m, psi), f"n=9 support {support}")


def test_fidelity_multi_trip_loop(qsim, gpu_ready):
    """n = 11 is the smallest n at which a work-group of the fidelity kernel takes more than one trip
    of its loop: rho has 2^22 elements = 1024 runs of 2^12, the grid is capped at 512 work-groups
    (kDmFidelityGroups), so each takes two runs; at n = 10 the 256 runs get a work-group each."""
    n = 11
    m = dc.random_matrix(n, 11)
    rho = loaded(qsim, m)
    psi = dc.random_psi(n, 111)
    dc.check_fidelity(rho.fidelity(psi), m, psi, dc.tol_a_fidelity(m, psi), "n=11")
    i = 1234
    e = np.zeros(1 << n, complex)
    e[i] = 1.0
    assert rho.fidelity(e) == m[i, i].real
    for qs in ([10, 0, 5], [9, 10, 3, 4, 1, 0]):
        check_subset_a(rho, m, qs, "n=11")


def test_largest_matrix(qsim, gpu_ready):
    """k = 6 at n = 7 (each entry a sum of two elements) and at n = 10, loaded matrices."""
    for n, subsets in ((7, ([0, 1, 2, 3, 4, 5], [6, 5, 4, 3, 2, 1], [3, 6, 0, 5, 1, 4])),
                       (10, ([0, 1, 2, 3, 4, 5], [9, 8, 7, 6, 5, 4], [9, 2, 7, 0, 5, 3]))):
        m = dc.random_matrix(n, 70 + n)
        rho = loaded(qsim, m)
        for qs in subsets:
            check_subset_a(rho, m, qs, f"n={n} k=6")


def test_maximally_mixed(qsim, gpu_ready):
    n = 6
    rho = qsim.DensityMatrix(n)
    rho.initMaximallyMixed()
    psi = dc.random_psi(n, 6)
    for qs in ([], [2], [5, 0], [1, 3, 4], [0, 1, 2, 3, 4, 5], [5, 3, 1, 0, 2, 4]):
        k = len(qs)
        np.testing.assert_allclose(rho.marginalProbabilities(qs), np.full(1 << k, 2.0 ** -k), atol=1e-15, rtol=0)
        np.testing.assert_allclose(rho.reducedDensityMatrix(qs), np.eye(1 << k) / (1 << k), atol=1e-15, rtol=0)
        assert abs(rho.subsystemEntropy(qs) - k) <= 1e-10
        assert abs(rho.subsystemEntropy(qs, renyi2=True) - k) <= 1e-10
        assert abs(rho.subsystemPurity(qs) - 2.0 ** -k) <= 1e-15
    want = float(np.vdot(psi, psi).real) / (1 << n)
    assert abs(rho.fidelity(psi) - want) <= dc.tol_a_fidelity(np.eye(1 << n) / (1 << n), psi)


def test_pure_entangled_state_matches_the_state_vector_readers(qsim, gpu_ready):
    n = 7
    sim = qsim.Simulator(n)
    sim.run(qsim.createRandomCircuit(n, 60, 5))
    psi = sim.getStateVector()
    m = np.outer(psi, psi.conj())
    rho = qsim.DensityMatrix(n, psi)
    for qs in ([0], [6, 2], [1, 3, 5], [4, 0, 6, 2], [0, 1, 2, 3, 4]):
        ta, tm = dc.tol_a_rdm(m, qs), dc.tol_a_marginal(m, qs)
        got, want = rho.reducedDensityMatrix(qs), sim.reducedDensityMatrix(qs)
        assert np.all(np.abs(got.real - want.real) <= ta) and np.all(np.abs(got.imag - want.imag) <= ta), qs
        assert np.all(np.abs(rho.marginalProbabilities(qs) - sim.marginalProbabilities(qs)) <= tm), qs
        assert abs(rho.subsystemEntropy(qs) - sim.entanglementEntropy(qs)) <= 1e-10, qs
        assert abs(rho.subsystemEntropy(qs, True) - sim.entanglementEntropy(qs, True)) <= 1e-10, qs
    f = rho.fidelity(psi)
    assert abs(f - 1.0) <= dc.tol_a_fidelity(m, psi)
    assert rho.fidelity(sim.state) == f  # the StateVector itself: its toHost()


def test_reproducible_modes_measurement_and_errors(qsim, oracle, gpu_ready):
    n = 7
    channels = [(0, -1, 0.04), (1, 1, 0.2), (3, 5, 0.1)]
    c = _circuit(qsim, n, 25, 8)
    want = oracle.dm_run(n, oracle.gates_of(c), channels)
    psi = dc.random_psi(n, 71)
    subsets = ([2], [6, 0, 3], [5, 1, 4, 2, 0, 6], list(range(n)))
    sim = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    sim.run(c)
    for qs in subsets:  # bitwise: fixed-order sums, no atomics
        np.testing.assert_array_equal(sim.marginalProbabilities(qs), sim.marginalProbabilities(qs))
        if len(qs) <= 6:
            np.testing.assert_array_equal(sim.reducedDensityMatrix(qs), sim.reducedDensityMatrix(qs))
    assert sim.fidelity(psi) == sim.fidelity(psi)
    per_gate = qsim.DensityMatrixSimulator(n, _noise(qsim, channels), mode=qsim.RunMode.PerGate)
    per_gate.run(c)
    for holder, what in ((sim, "B fused mode"), (per_gate, "B per-gate mode")):
        for qs in subsets:
            check_subset_b(holder, want, qs, what)
        dc.check_fidelity(holder.fidelity(psi), want, psi, dc.tol_b_fidelity(psi), what)
    # a collapsed, renormalised rho
    sim.setSeed(3)
    bit = sim.measureQubit(2)
    got = [(qs, sim.marginalProbabilities(qs), sim.reducedDensityMatrix(qs)) for qs in subsets[:3]]
    f = sim.fidelity(psi)
    m = sim.getDensityMatrix()
    for qs, marg, mat in got:
        dc.check_marginal(marg, m, qs, dc.tol_a_marginal(m, qs), f"A after measureQubit -> {bit}")
        dc.check_rdm(mat, m, qs, dc.tol_a_rdm(m, qs), f"A after measureQubit -> {bit}")
    dc.check_fidelity(f, m, psi, dc.tol_a_fidelity(m, psi), "A after measureQubit")
    np.testing.assert_allclose(sim.marginalProbabilities([2]), [1 - bit, bit], atol=1e-12, rtol=0)
    # reference-compatible Y: the readers are linear in the stored rho, so they follow the oracle
    cy = _circuit(qsim, n, 14, 31)
    cy.y(3)
    want_y = oracle.dm_run(n, oracle.gates_of(cy), channels, reference_y=True)
    ref = qsim.DensityMatrixSimulator(n, _noise(qsim, channels))
    ref.setReferenceCompatible()
    ref.run(cy)
    for qs in subsets:
        check_subset_b(ref, want_y, qs, "B reference Y")
    dc.check_fidelity(ref.fidelity(psi), want_y, psi, dc.tol_b_fidelity(psi), "B reference Y")
    # errors: what StateVector raises for the same mistake, on both holder classes
    sv = qsim.StateVector(n)
    mistakes = [("marginalProbabilities", [1, 4, 1], ValueError), ("reducedDensityMatrix", [1, 4, 1], ValueError),
                ("marginalProbabilities", [0, n], IndexError), ("reducedDensityMatrix", [-1], IndexError),
                ("reducedDensityMatrix", list(range(7)), ValueError), ("subsystemPurity", list(range(7)), ValueError),
                ("marginalProbabilities", list(range(n)) + [0], ValueError),
                ("marginalProbabilities", list(range(21)), ValueError)]
    for name, qs, exc in mistakes:
        with pytest.raises(exc) as sv_err:
            getattr(sv, name)(qs)
        for holder in (sim, sim.density):
            with pytest.raises(exc) as dm_err:
                getattr(holder, name)(qs)
            assert str(dm_err.value) == str(sv_err.value), (name, qs)
    for holder in (sim, sim.density):
        with pytest.raises(ValueError):
            holder.subsystemEntropy([3, 3])
        for bad in (np.ones(1 << (n - 1)), np.ones((1 << n) + 1), qsim.StateVector(n + 1)):
            with pytest.raises(ValueError, match="State vector size mismatch"):
                holder.fidelity(bad)
