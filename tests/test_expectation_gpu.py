"""Pauli-sum expectation values on the device (csrc/hip/expect.hip; qsim_state_expectation,
qsim_batch_expectation).

Primary check: the GPU value against numpy on the SAME simulator's amplitudes, read back AFTER
the expectation call (so a relabeled / relayout state really is read where it lies), at
1e-12 * sum |c_t| — only the summation order differs.  Secondary: against numpy on the oracle's
state at the same bar.  The numpy reference (apply_pauli / expectation_np) is the one
tests/test_expectation_cpu.py checks against dense Kronecker products.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def apply_pauli(psi, x, z):
    """P|psi> for the string with masks (x, z): P|i> = i^nY (-1)^popcount(i & z) |i ^ x>."""
    idx = np.arange(psi.size, dtype=np.uint64)
    par = np.zeros(psi.size, dtype=np.int64)
    t = idx & np.uint64(z)
    while t.any():
        par ^= (t & np.uint64(1)).astype(np.int64)
        t >>= np.uint64(1)
    ny = bin(x & z).count("1")
    out = np.empty_like(psi)
    out[(idx ^ np.uint64(x)).astype(np.int64)] = (1j ** ny) * (1 - 2 * par) * psi
    return out


def expectation_np(psi, terms):
    return sum(c * np.vdot(psi, apply_pauli(psi, x, z)).real for x, z, c in terms)


def pauli_sum(qsim, n, terms):
    """PauliSum of (x, z, c) mask terms through the public add()."""
    h = qsim.PauliSum(n)
    for x, z, c in terms:
        f = {}
        for q in range(n):
            xb, zb = x >> q & 1, z >> q & 1
            if xb or zb:
                f[q] = "Y" if xb and zb else ("X" if xb else "Z")
        h.add(c, f)
    return h


def random_terms(rng, n, count, n_x):
    """count terms over n_x distinct x masks (0 among them), random z, coefficients in [-1, 1)."""
    xs = [0] + [int(v) for v in rng.integers(1, 1 << n, size=n_x - 1)]
    return [(xs[int(rng.integers(0, len(xs)))], int(rng.integers(0, 1 << n)), float(rng.uniform(-1, 1)))
            for _ in range(count)]


def bound(terms):
    return 1e-12 * sum(abs(c) for _, _, c in terms)


def single(qsim, sim, x, z):
    return sim.expectation(pauli_sum(qsim, sim.getNumQubits(), [(x, z, 1.0)]))


def test_known_answers(qsim, gpu_ready):
    X, Y, Z = "XYZ"

    def ev(sim, factors):
        return sim.expectation(qsim.PauliSum(sim.getNumQubits()).add(1.0, factors))

    s = qsim.Simulator(1)
    assert abs(ev(s, {0: Z}) - 1.0) < 1e-12
    s.run(qsim.Circuit(1).h(0))
    assert abs(ev(s, {0: X}) - 1.0) < 1e-12
    assert abs(ev(s, {0: Z})) < 1e-12
    s = qsim.Simulator(1)
    s.run(qsim.Circuit(1).h(0).s(0))
    assert abs(ev(s, {0: Y}) - 1.0) < 1e-12
    s = qsim.Simulator(2)
    s.run(qsim.createBellCircuit())
    assert abs(ev(s, {0: X, 1: X}) - 1.0) < 1e-12
    assert abs(ev(s, {0: Y, 1: Y}) + 1.0) < 1e-12
    assert abs(ev(s, {0: Z, 1: Z}) - 1.0) < 1e-12
    assert abs(ev(s, {0: X, 1: Z})) < 1e-12
    assert abs(ev(s, {}) - 1.0) < 1e-12  # identity: the norm
    s = qsim.Simulator(3)
    s.run(qsim.createGHZCircuit(3))
    assert abs(ev(s, {0: X, 1: X, 2: X}) - 1.0) < 1e-12
    assert abs(ev(s, {0: X, 1: Y, 2: Y}) + 1.0) < 1e-12
    assert abs(ev(s, {0: Z, 1: Z}) - 1.0) < 1e-12


@pytest.fixture(scope="module")
def ten(qsim, oracle, gpu_ready):
    n = 10
    c = qsim.createRandomCircuit(n, 120, 77)
    sim = qsim.Simulator(n)
    sim.run(c)
    ref = oracle.run_cpu(n, oracle.gates_of(c))
    ref.setflags(write=False)
    return sim, ref


def _pairing_cases(n):
    """Single strings whose highest x bit is 0 (lane), 5, 6 (wave), 7, 8 (block) and 9 (top), each
    with nY = 0..3 where x has room for it, with z reaching outside x and with z inside x only."""
    rng = np.random.default_rng(4)
    cases = []
    for hb in (0, 5, 6, 7, 8, 9):
        for ny in range(4):
            if ny > hb + 1:
                continue  # x has hb + 1 bits at most
            lower = [int(q) for q in rng.permutation(hb)[:max(ny - 1, min(hb, 2))]]
            xbits = [hb] + lower
            x = sum(1 << q for q in xbits)
            ybits = sum(1 << q for q in xbits[:ny])
            free = [q for q in range(n) if not x >> q & 1]
            outside = sum(1 << int(q) for q in rng.permutation(free)[:3])
            cases.append((x, ybits | outside))
            cases.append((x, ybits))
    return cases


def test_pairing_cases_n10(qsim, ten):
    sim, ref = ten
    cases = _pairing_cases(10)
    assert {x.bit_length() - 1 for x, _ in cases} == {0, 5, 6, 7, 8, 9}
    assert {bin(x & z).count("1") for x, z in cases} == {0, 1, 2, 3}
    got = [single(qsim, sim, x, z) for x, z in cases]
    own = sim.getStateVector()  # after the expectation calls
    for (x, z), g in zip(cases, got):
        assert abs(g - expectation_np(own, [(x, z, 1.0)])) < 1e-12, (hex(x), hex(z))
        assert abs(g - expectation_np(ref, [(x, z, 1.0)])) < 1e-12, (hex(x), hex(z))


def test_mixed_sum_and_reproducibility_n10(qsim, ten):
    sim, ref = ten
    terms = random_terms(np.random.default_rng(8), 10, 40, 9)
    h = pauli_sum(qsim, 10, terms)
    a = sim.expectation(h)
    b = sim.expectation(h)
    assert a == b  # fixed summation order: bitwise reproducible
    own = sim.getStateVector()
    assert abs(a - expectation_np(own, terms)) < bound(terms)
    assert abs(a - expectation_np(ref, terms)) < bound(terms)


def test_group_larger_than_the_term_table(qsim, ten):
    """A group of more terms than one launch's LDS table holds (several launches of the kernel)
    equals the same sum split by the caller into two calls."""
    from qsim_amd import _lib
    sim, ref = ten
    rng = np.random.default_rng(9)
    for x in (0, 0b1000100001):
        terms = [(x, z, float(rng.uniform(-1, 1))) for z in range(1, 701)]
        arr, cnt = pauli_sum(qsim, 10, terms).to_abi(10)
        passes, launches = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.hip.qsim_expectation_plan(10, arr, cnt, None, ctypes.byref(passes), ctypes.byref(launches)))
        assert passes.value == 1 and launches.value > 1
        whole = sim.expectation(pauli_sum(qsim, 10, terms))
        halves = sim.expectation(pauli_sum(qsim, 10, terms[:350])) + sim.expectation(pauli_sum(qsim, 10, terms[350:]))
        assert abs(whole - halves) < bound(terms)
        assert abs(whole - expectation_np(ref, terms)) < bound(terms)


@pytest.mark.parametrize("relayout", [False, True])
def test_reads_the_state_where_it_lies_n16(qsim, oracle, gpu_ready, relayout):
    from qsim_amd.plan import set_calibrate, set_relabel, set_relayout
    n = 16
    set_relabel(1, 14)
    if relayout:
        set_relayout(2, 16)  # forced: a relayout plan whenever one exists
        set_calibrate(0, -1)
    c = qsim.createRandomHCCircuit(n, 100, 1)
    sim = qsim.Simulator(n)
    sim.run(c)
    perm = sim.state.perm()
    assert perm != list(range(n)), "expected the planner to relabel this circuit"
    if relayout:  # (three passes: the run ends in the second buffer)
        assert sim.state.layoutInfo()["relayout"]
    terms = random_terms(np.random.default_rng(16), n, 60, 12)
    got = sim.expectation(pauli_sum(qsim, n, terms))
    assert sim.state.perm() == perm  # read in place: the layout was not restored
    assert got == sim.expectation(pauli_sum(qsim, n, terms))
    own = sim.getStateVector()  # only now
    assert abs(got - expectation_np(own, terms)) < bound(terms)
    ref = oracle.run_cpu(n, oracle.gates_of(c))
    assert abs(got - expectation_np(ref, terms)) < bound(terms)


@pytest.mark.parametrize("noisy", [False, True])
def test_noisy_simulator(qsim, gpu_ready, noisy):
    n = 10
    nm = qsim.NoiseModel()
    if noisy:
        nm.addDepolarizingAll(n, 0.02)
    sim = qsim.NoisySimulator(n, nm)
    sim.setSeed(5)
    sim.run(qsim.createRandomCircuit(n, 60, 21))
    terms = random_terms(np.random.default_rng(2), n, 30, 6)
    got = sim.expectation(pauli_sum(qsim, n, terms))
    own = sim.getStateVector()
    assert abs(got - expectation_np(own, terms)) < bound(terms)


def test_batched_noise_free(qsim, ten):
    sim, ref = ten
    n, B = 10, 5
    b = qsim.BatchedSimulator(n, B)
    b.run(qsim.createRandomCircuit(n, 120, 77))
    terms = random_terms(np.random.default_rng(12), n, 30, 6)
    h = pauli_sum(qsim, n, terms)
    e = b.getExpectations(h)
    assert e.shape == (B,)
    one = sim.expectation(h)
    for t in range(B):
        assert abs(e[t] - one) < bound(terms)
        assert abs(e[t] - expectation_np(ref, terms)) < bound(terms)


@pytest.mark.parametrize("physical", [False, True])
def test_batched_noisy_trajectories(qsim, gpu_ready, physical):
    n, B = 12, 8
    nm = qsim.NoiseModel()
    nm.addDepolarizingAll(n, 0.05)
    b = qsim.BatchedSimulator(n, B, nm)
    if physical:
        b.setNoiseSemantics(qsim.BatchedNoise.Physical)  # carries Pauli frames past the run
    b.setSeed(31)
    b.run(qsim.createRandomCircuit(n, 60, 13))
    terms = random_terms(np.random.default_rng(3), n, 30, 6)
    h = pauli_sum(qsim, n, terms)
    e = b.getExpectations(h)  # before any getStateVector: carried frames are still pending
    avg = b.getAverageExpectation(h)
    exp = []
    for t in range(B):
        psi = b.getStateVector(t)
        exp.append(expectation_np(psi, terms))
        assert abs(e[t] - exp[t]) < bound(terms), t
    assert len({round(v, 9) for v in exp}) > 1, "the trajectories should differ under noise"
    mean = 0.0
    for v in e:
        mean += float(v)
    assert avg == mean / B


def test_error_codes(qsim, gpu_ready):
    from qsim_amd import _lib
    sim = qsim.Simulator(4)
    out = ctypes.c_double(7.0)
    arr = (_lib.qsim_pauli_term * 1)()
    arr[0].x_mask, arr[0].z_mask, arr[0].coeff = 1 << 4, 0, 1.0
    hdl = sim.state.handle
    f = _lib.hip.qsim_state_expectation
    assert f(hdl, arr, 1, ctypes.byref(out)) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert f(hdl, None, 1, ctypes.byref(out)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, arr, 1, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(None, arr, 1, ctypes.byref(out)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(hdl, None, 0, ctypes.byref(out)) == 0 and out.value == 0.0
    with pytest.raises(ValueError):
        sim.expectation(qsim.PauliSum(5))
    b = qsim.BatchedSimulator(4, 3)
    res = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    g = _lib.hip.qsim_batch_expectation
    assert g(b._h, arr, 1, res) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert g(b._h, None, 1, res) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert g(b._h, arr, 1, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert g(None, arr, 1, res) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert g(b._h, None, 0, res) == 0 and list(res) == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        b.getExpectations(qsim.PauliSum(5))


@pytest.mark.parametrize("n", [5, 10])
def test_z_split_kernel_matches_plain_kernel(qsim, oracle, gpu_ready, monkeypatch, n):
    """Groups of 16 or more terms run the kernel that splits each z into a per-run and a
    per-amplitude part (QSIM_EXPECT_SPLIT, default on): the same weights added in the same order
    as the plain kernel, so the same double.  n = 5: one partly filled work-group (the tail);
    n = 10: several work-groups; x with its highest bit below, at and above bit 8 of the index."""
    c = qsim.createRandomCircuit(n, 60, 3)
    sim = qsim.Simulator(n)
    sim.run(c)
    ref = oracle.run_cpu(n, oracle.gates_of(c))
    rng = np.random.default_rng(n)
    for x in (0, 0b01001, 1 << (n - 2) | 3, 1 << (n - 1) | 1 << 3):
        zs = rng.permutation(1 << n)[:24]
        terms = [(x, int(z), float(rng.uniform(-1, 1))) for z in zs]
        h = pauli_sum(qsim, n, terms)
        monkeypatch.setenv("QSIM_EXPECT_SPLIT", "1")
        split = sim.expectation(h)
        monkeypatch.setenv("QSIM_EXPECT_SPLIT", "0")
        plain = sim.expectation(h)
        assert split == plain, hex(x)
        assert abs(split - expectation_np(ref, terms)) < bound(terms), hex(x)


def test_batched_reads_under_its_qubit_layout(qsim, gpu_ready):
    """A relabeled ensemble (Physical noise: fused frame passes keep the layout the first run chose)
    is read under b->perm: the layout is still there after the call, the values match numpy on the
    trajectories read back afterwards."""
    from qsim_amd.plan import set_relabel
    n, B = 16, 2
    set_relabel(1, 14)
    nm = qsim.NoiseModel()
    nm.addDepolarizingAll(n, 0.01)
    b = qsim.BatchedSimulator(n, B, nm, noise=qsim.BatchedNoise.Physical)
    b.setSeed(7)
    b.run(qsim.createRandomHCCircuit(n, 100, 1))
    perm = b.perm()
    assert perm != list(range(n)), "expected the planner to relabel this circuit"
    terms = random_terms(np.random.default_rng(21), n, 40, 8)
    e = b.getExpectations(pauli_sum(qsim, n, terms))
    assert b.perm() == perm  # read in place
    for t in range(B):
        assert abs(e[t] - expectation_np(b.getStateVector(t), terms)) < bound(terms), t
