"""Marginal probabilities, reduced density matrices, subsystem purity and entanglement entropy on
the device (csrc/hip/marginal.hip) against numpy on the simulator's own amplitudes, read back after
the call under test."""
import ctypes

import numpy as np
import pytest

import marginal_cases as mc

pytestmark = pytest.mark.gpu


def check_marginal(sim, psi, qubits):
    got = sim.marginalProbabilities(qubits)
    want = mc.marginal_np(psi, qubits)
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    assert err <= mc.ATOL, f"marginal of {qubits}: max error {err}"
    return got


def check_rdm(sim, psi, qubits):
    got = sim.reducedDensityMatrix(qubits)
    want = mc.rdm_np(psi, qubits)
    assert got.shape == want.shape and got.dtype == np.complex128
    err = float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))
    assert err <= mc.ATOL, f"reduced density matrix of {qubits}: max component error {err}"
    assert np.array_equal(got, got.conj().T), "rho_A is not bitwise Hermitian"
    assert not got.diagonal().imag.any()
    return got


# ---- known answers ----
def test_bell(qsim, gpu_ready):
    sim = qsim.Simulator(2)
    sim.run(qsim.createBellCircuit())
    for q in (0, 1):
        np.testing.assert_allclose(sim.marginalProbabilities([q]), [0.5, 0.5], atol=mc.ATOL, rtol=0)
        np.testing.assert_allclose(sim.reducedDensityMatrix([q]), np.eye(2) / 2, atol=mc.ATOL, rtol=0)
        assert abs(sim.entanglementEntropy([q]) - 1.0) <= mc.ENT_ATOL
        assert abs(sim.entanglementEntropy([q], renyi2=True) - 1.0) <= mc.ENT_ATOL
        assert abs(sim.subsystemPurity([q]) - 0.5) <= mc.ATOL
    np.testing.assert_allclose(sim.marginalProbabilities([0, 1]), [0.5, 0, 0, 0.5], atol=mc.ATOL, rtol=0)
    assert abs(sim.state.entanglementEntropy([0, 1])) <= mc.ENT_ATOL  # the whole state is pure


def test_ghz3(qsim, gpu_ready):
    sim = qsim.Simulator(3)
    sim.run(qsim.createGHZCircuit(3))
    np.testing.assert_allclose(sim.marginalProbabilities([0, 2]), [0.5, 0, 0, 0.5], atol=mc.ATOL, rtol=0)
    for q in range(3):
        assert abs(sim.entanglementEntropy([q]) - 1.0) <= mc.ENT_ATOL
    np.testing.assert_allclose(sim.reducedDensityMatrix([2, 0]), np.diag([0.5, 0, 0, 0.5]), atol=mc.ATOL, rtol=0)


def test_product_state(qsim, gpu_ready):
    n = 4
    c = qsim.Circuit(n)
    for q in range(n):
        c.ry(q, 0.3 + 0.7 * q)
    sim = qsim.Simulator(n)
    sim.run(c)
    for qs in ([0], [2], [1, 3], [3, 0, 2]):
        assert abs(sim.entanglementEntropy(qs)) <= mc.ENT_ATOL
        assert abs(sim.subsystemPurity(qs) - 1.0) <= mc.ATOL
    want = [np.cos((0.3 + 0.7 * 1) / 2) ** 2, np.sin((0.3 + 0.7 * 1) / 2) ** 2]
    np.testing.assert_allclose(sim.marginalProbabilities([1]), want, atol=mc.ATOL, rtol=0)


def test_no_qubits_gives_the_norm(qsim, gpu_ready):
    sim = qsim.Simulator(7)
    sim.run(qsim.createRandomCircuit(7, 40, 3))
    sim.state.fromHost(0.6 * sim.getStateVector())  # (an unnormalised state: the norm is 0.36)
    psi = sim.getStateVector()
    norm = float(np.sum(np.abs(psi) ** 2))
    assert abs(norm - 0.36) < 1e-9
    m = sim.marginalProbabilities([])
    rho = sim.reducedDensityMatrix([])
    assert m.shape == (1,) and rho.shape == (1, 1)
    assert abs(m[0] - norm) <= mc.ATOL and abs(rho[0, 0] - norm) <= mc.ATOL and rho[0, 0].imag == 0.0


# ---- exhaustive at n = 6, and one partly filled work-group at n = 5 ----
@pytest.fixture(scope="module")
def six(qsim, gpu_ready):
    sim = qsim.Simulator(6)
    sim.run(qsim.createRandomCircuit(6, 60, 11))
    psi = sim.getStateVector()
    psi.setflags(write=False)
    return sim, psi


def test_every_subset_n6(six):
    sim, psi = six
    subsets = mc.all_subsets(6)
    assert len(subsets) == 64
    for qs in subsets:
        check_marginal(sim, psi, qs)
        check_rdm(sim, psi, qs)
    full = sim.reducedDensityMatrix(list(range(6)))
    assert np.max(np.abs(full - np.outer(psi, psi.conj()))) <= mc.ATOL  # k = n: |psi><psi|


def test_qubit_order_decides_bit_order_n6(six):
    sim, psi = six
    base = sim.marginalProbabilities([0, 2, 3, 5])
    for order in ([3, 0, 5, 2], [5, 3, 2, 0]):
        got = check_marginal(sim, psi, order)
        assert not np.allclose(got, base, atol=1e-6), "the bit-permuted array, not the sorted one"
        rho = check_rdm(sim, psi, order)
        assert np.max(np.abs(rho.diagonal().real - got)) <= mc.ATOL


def test_partly_filled_work_group_n5(qsim, gpu_ready):
    sim = qsim.Simulator(5)
    sim.run(qsim.createRandomCircuit(5, 50, 4))
    psi = sim.getStateVector()
    for qs in mc.all_subsets(5):
        check_marginal(sim, psi, qs)
        check_rdm(sim, psi, qs)
    for qs in ([4, 1], [0, 2, 3]):
        rho = mc.rdm_np(psi, qs)
        if mc.spectrum_is_safe(rho):
            assert abs(sim.entanglementEntropy(qs) - mc.entropy_np(rho)) <= mc.ENT_ATOL


# ---- n = 10 and n = 14 under the identity layout: every class of position ----
@pytest.fixture(scope="module", params=[10, 14])
def pergate(request, qsim, gpu_ready):
    n = request.param
    sim = qsim.Simulator(n, mode=qsim.RunMode.PerGate)
    sim.run(qsim.createRandomCircuit(n, 150, 100 + n))
    assert sim.state.perm() == list(range(n))
    psi = sim.getStateVector()
    psi.setflags(write=False)
    return n, sim, psi


def test_position_classes_marginal(pergate):
    from qsim_amd.plan import marginal_plan
    n, sim, psi = pergate
    sliced = 0
    for name, qs in mc.MARGINAL_CLASSES[n].items():
        check_marginal(sim, psi, qs)
        info = marginal_plan(n, qs)
        assert info["k_lo"] + info["k_hi"] == len(qs), name
        sliced += info["slices"] > 1
    if n == 14:
        assert sliced >= 1, "no case exercises the second-stage reduce over several slices"
        assert marginal_plan(n, mc.MARGINAL_CLASSES[n]["above"])["k_hi"] == 2
    assert sim.state.perm() == list(range(n))


def test_position_classes_matrix(pergate):
    n, sim, psi = pergate
    for name, qs in mc.RDM_CLASSES[n].items():
        rho = check_rdm(sim, psi, qs)
        marg = sim.marginalProbabilities(qs)
        assert np.max(np.abs(rho.diagonal().real - marg)) <= mc.ATOL, name
        want = mc.rdm_np(psi, qs)
        assert abs(sim.subsystemPurity(qs) - float(np.sum(np.abs(want) ** 2))) <= mc.ATOL * want.size
        if mc.spectrum_is_safe(want):
            assert abs(sim.entanglementEntropy(qs) - mc.entropy_np(want)) <= mc.ENT_ATOL, name
            assert abs(sim.entanglementEntropy(qs, True) - mc.entropy_np(want, True)) <= mc.ENT_ATOL, name


def test_single_qubit_marginal_is_prob_bit_zero(pergate):
    n, sim, psi = pergate
    for q in range(n):
        p0 = sim.state.probBitZero(q)
        got = sim.marginalProbabilities([q])
        assert np.max(np.abs(got - np.array([p0, 1.0 - p0]))) <= mc.ATOL


# ---- n = 16: read where the state lies ----
@pytest.mark.parametrize("relayout", [False, True])
def test_reads_the_state_where_it_lies_n16(qsim, gpu_ready, relayout):
    from qsim_amd.plan import marginal_plan, set_calibrate, set_relabel, set_relayout
    n = 16
    set_relabel(1, 14)
    if relayout:
        set_relayout(2, 16)  # forced: a relayout plan whenever one exists
        set_calibrate(0, -1)
    sim = qsim.Simulator(n)
    sim.run(qsim.createRandomHCCircuit(n, 100, 1))
    perm = sim.state.perm()
    info = sim.state.layoutInfo()
    assert perm != list(range(n)), "expected the planner to relabel this circuit"
    if relayout:
        assert info["relayout"]
    marg_sets = [[0], [15, 3, 8], list(range(0, 16, 2)), list(range(4, 16)), [1, 2, 13, 14, 6]]
    rdm_sets = [[5], [14, 0, 7], [0, 1, 2, 3, 4, 5], [10, 11, 12, 13, 14, 15], [15, 9, 4, 2]]
    margs = [sim.marginalProbabilities(qs) for qs in marg_sets]
    rhos = [sim.reducedDensityMatrix(qs) for qs in rdm_sets]
    assert sim.state.perm() == perm and sim.state.layoutInfo() == info  # nothing was restored
    for qs, m in zip(marg_sets, margs):
        assert np.array_equal(m, sim.marginalProbabilities(qs)), "not bitwise reproducible"
        assert marginal_plan(n, qs, perm)["k_lo"] + marginal_plan(n, qs, perm)["k_hi"] == len(qs)
    for qs, r in zip(rdm_sets, rhos):
        assert np.array_equal(r, sim.reducedDensityMatrix(qs)), "not bitwise reproducible"
    assert sim.state.perm() == perm and sim.state.layoutInfo() == info
    psi = sim.getStateVector()  # only now
    for qs, m in zip(marg_sets, margs):
        assert np.max(np.abs(m - mc.marginal_np(psi, qs))) <= mc.ATOL
    for qs, r in zip(rdm_sets, rhos):
        want = mc.rdm_np(psi, qs)
        assert max(np.max(np.abs(r.real - want.real)), np.max(np.abs(r.imag - want.imag))) <= mc.ATOL
        assert np.array_equal(r, r.conj().T)


def test_noisy_simulator_forward(qsim, gpu_ready):
    n = 8
    nm = qsim.NoiseModel()
    nm.addDepolarizingAll(n, 0.02)
    sim = qsim.NoisySimulator(n, nm)
    sim.setSeed(5)
    sim.run(qsim.createRandomCircuit(n, 60, 21))
    got = sim.marginalProbabilities([6, 1, 3])
    rho = sim.reducedDensityMatrix([6, 1, 3])
    psi = sim.getStateVector()
    assert np.max(np.abs(got - mc.marginal_np(psi, [6, 1, 3]))) <= mc.ATOL
    assert np.max(np.abs(rho - mc.rdm_np(psi, [6, 1, 3]))) <= mc.ATOL
    assert abs(sim.subsystemPurity([6, 1, 3]) - float(np.sum(np.abs(rho) ** 2))) <= mc.ATOL * 64
    assert abs(sim.entanglementEntropy([6, 1, 3], True) + np.log2(np.sum(np.abs(rho) ** 2))) <= mc.ENT_ATOL


# ---- the entropy the C++ harness recomputes (tests/test_marginal_cpp.py passes it on) ----
def test_cpp_entropy_case_matches_numpy(qsim, gpu_ready):
    case = mc.CPP_ENTROPY_CASE
    sim = qsim.Simulator(case["n"])
    sim.run(qsim.createRandomCircuit(case["n"], case["depth"], case["seed"]))
    got = sim.entanglementEntropy(case["qubits"])
    want = mc.rdm_np(sim.getStateVector(), case["qubits"])
    assert mc.spectrum_is_safe(want)
    print(f"entropy of the C++ case: {got!r}")
    assert abs(got - mc.entropy_np(want)) <= mc.ENT_ATOL


# ---- argument checks: the raw ABI and Python ----
def test_argument_checks(qsim, gpu_ready):
    from qsim_amd import _lib
    n = 22
    sim = qsim.Simulator(n)
    h = sim.state.handle
    h = h() if callable(h) else h
    out = np.zeros(2 * 4 ** 6 + (1 << 20))
    optr = out.ctypes.data_as(ctypes.c_void_p)

    def arr(*qs):
        return (ctypes.c_int32 * len(qs))(*qs)

    marg, rdm = _lib.hip.qsim_state_marginal_probabilities, _lib.hip.qsim_state_reduced_density_matrix
    for fn in (marg, rdm):
        assert fn(h, arr(1, 4, 1), 3, optr) == _lib.QSIM_ERR_INVALID_ARGUMENT  # duplicate
        assert fn(h, arr(0, n), 2, optr) == _lib.QSIM_ERR_OUT_OF_RANGE
        assert fn(h, arr(-1), 1, optr) == _lib.QSIM_ERR_OUT_OF_RANGE
        assert fn(h, arr(0, 1), 2, None) == _lib.QSIM_ERR_INVALID_ARGUMENT  # null out
        assert fn(None, arr(0, 1), 2, optr) == _lib.QSIM_ERR_INVALID_ARGUMENT  # null handle
        assert fn(h, None, 1, optr) == _lib.QSIM_ERR_INVALID_ARGUMENT  # null list, k > 0
        assert fn(h, None, 0, optr) == _lib.QSIM_OK  # null list with k == 0 is valid
        assert out[0] == 1.0
    assert marg(h, arr(*range(21)), 21, optr) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert marg(h, arr(*range(20)), 20, optr) == _lib.QSIM_OK
    assert out[0] == 1.0 and not out[1:1 << 20].any()
    assert rdm(h, arr(*range(7)), 7, optr) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert rdm(h, arr(*range(6)), 6, optr) == _lib.QSIM_OK

    for name in ("marginalProbabilities", "reducedDensityMatrix", "subsystemPurity", "entanglementEntropy"):
        f = getattr(sim, name)
        with pytest.raises(ValueError):
            f([1, 4, 1])
        with pytest.raises(IndexError):
            f([0, n])
        with pytest.raises(IndexError):
            f([-1])
    with pytest.raises(ValueError):
        sim.marginalProbabilities(list(range(21)))
    with pytest.raises(ValueError):
        sim.reducedDensityMatrix(list(range(7)))
    small = qsim.Simulator(3)
    with pytest.raises((ValueError, IndexError)):
        small.marginalProbabilities([0, 1, 2, 3])
