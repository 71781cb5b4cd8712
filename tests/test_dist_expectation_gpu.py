"""GPU: Pauli-sum expectation values on the sharded state (DistributedSimulator.expectation,
qsim_dist_expectation; csrc/hip/dist_expect.hip) on virtual ranks.

The circuits and run counts are those of tests/test_dist_readout_gpu.py, so the qubit map has left
the identity; every string is chosen by PHYSICAL position (local / rank, lane / above, top local
position in or out of x) and translated to logical qubits through perm() read before the call.
Reference: the numpy restatement apply_pauli / expectation_np and the bar 1e-12 * sum |c| of
tests/test_expectation_gpu.py (copied), on the oracle's state and on the simulator's own
amplitudes gathered AFTER the calls.  After every case the map and the amplitudes must be
bit-identical to what they were and the state must still run.
"""
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


def bound(terms):
    return 1e-12 * sum(abs(c) for _, _, c in terms)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _circuit(qsim, n, name):
    return qsim.createRandomHCCircuit(n, 100, 42) if name == "hc" else qsim.createRandomCircuit(n, 100, 5)


_REF = {}


def _reference(qsim, oracle, n, name, runs):
    """Oracle state of `runs` runs of the circuit; computed once, read-only."""
    key = (n, name, runs)
    if key not in _REF:
        st = oracle.run_cpu(n, oracle.gates_of(_circuit(qsim, n, name)) * runs)
        st.setflags(write=False)
        _REF[key] = st
    return _REF[key]


# (world, n, circuit, runs): L = 7 (half a shard = 64 amplitudes, less than a work-group), 8 (128),
# 9 (256: one work-group) and 13 (4096: several work-groups)
SHAPES = [(2, 8, "hc", 1), (4, 10, "hc", 2), (8, 12, "hc", 3), (8, 16, "hc", 2)]


def _make(qsim, world, n, name, runs, d=None):
    from qsim_amd.dist import DistributedSimulator
    c = _circuit(qsim, n, name)
    d = d if d is not None else DistributedSimulator.virtual(n, world)
    for _ in range(runs):
        d.run(c)
    assert d.perm() != list(range(n))                          # the map has left the identity
    return d, c


def _mask(positions):
    m = 0
    for p in positions:
        assert not m >> p & 1
        m |= 1 << p
    return m


def _to_logical(perm, m):
    """Physical mask -> logical mask (bit perm[q] of m -> bit q)."""
    return sum(1 << q for q in range(len(perm)) if m >> perm[q] & 1)


def _single_strings(n, world):
    """Physical (x, z) of the single-string set, with the class of each for the coverage check."""
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    rank_pos = list(range(L, n))
    rank_sets = [[L]] + ([[L, n - 1]] if g >= 2 else []) + ([rank_pos] if g >= 3 else [])
    locs = [[], [b], [b, 2], [1], [0, 3]]
    if b > 6:
        locs += [[b, 6], [6]]
    out = []
    for R in rank_sets:
        free_rank = [p for p in rank_pos if p not in R]
        for xl in locs:
            x = _mask(R + xl)
            z_out = _mask([p for p in (0, 4, b - 1) if p not in xl] + free_rank[:1])
            out.append((x, 0))
            out.append((x, z_out))                             # z outside x, on a rank position if one is free
            out.append((x, _mask(R[:1]) | z_out))              # one Y, on a rank position
    # nY = 0..3, the first Y on a rank position
    x = _mask(rank_pos + [1, 3, b])
    for ny in range(4):
        out.append((x, _mask([rank_pos[0], 1, b][:ny]) | 1))
    x = _mask(rank_pos + [2, 5])
    for ny in range(1, 4):
        out.append((x, _mask([rank_pos[-1], 5, 2][:ny]) | _mask([b])))
    # purely local (z reaching a rank position) and purely Z
    out += [(_mask([1]), _mask([L])), (_mask([b, 2]), _mask([2, 0, n - 1])), (_mask([b]), 0),
            (_mask([0, 5]), _mask([0, 5, n - 1])), (0, _mask([L])), (0, _mask([0, b, n - 1])), (0, 0)]
    return out


@pytest.mark.parametrize("world,n,name,runs", SHAPES)
def test_single_strings(qsim, oracle, gpu_ready, world, n, name, runs):
    d, c = _make(qsim, world, n, name, runs)
    ref = _reference(qsim, oracle, n, name, runs)
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    lmask = (1 << L) - 1
    phys = _single_strings(n, world)
    # what the set covers, by physical position
    cross = [(x, z) for x, z in phys if x >> L]
    assert {bin(x >> L).count("1") for x, _ in cross} >= {1, g}
    assert any(x & lmask == 0 for x, _ in cross)                               # x_loc empty
    assert any(x >> b & 1 for x, _ in cross) and any(x & lmask and not x >> b & 1 for x, _ in cross)
    low = {(x & lmask) & -(x & lmask) for x, _ in cross if x & lmask}
    assert any(v < 64 for v in low) and any(v >= 64 for v in low)              # lane bit / above
    assert {bin(x & z).count("1") for x, z in cross if (x & z) >> L} >= {1, 2, 3}
    assert any(bin(x & z).count("1") == 0 for x, z in cross)
    assert any((z & ~x) >> L for x, z in cross) or g == 1                      # z on a rank position outside x
    assert any((z & ~x) >> L for x, z in phys if not x >> L and x)
    assert any(x and not x >> L for x, _ in phys) and any(x == 0 for x, _ in phys)
    perm = d.perm()
    before = d.getStateVector()
    cases = [(_to_logical(perm, x), _to_logical(perm, z)) for x, z in phys]
    got = [d.expectation(pauli_sum(qsim, n, [(x, z, 1.0)])) for x, z in cases]
    assert d.perm() == perm
    own = d.getStateVector()                                   # after the calls
    assert np.array_equal(_bits(before), _bits(own))
    for (x, z), (px, pz), v in zip(cases, phys, got):
        assert abs(v - expectation_np(own, [(x, z, 1.0)])) < 1e-12, (hex(px), hex(pz))
        assert abs(v - expectation_np(ref, [(x, z, 1.0)])) < 1e-12, (hex(px), hex(pz))
    d.run(c)                                                   # and the state still runs
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def _mixed_terms(n, world, perm, seed=3):
    """60 terms over 9 distinct physical x masks: Z-only, two local ones, and six cross ones of
    which three share the transfer key (rank position L, top local position out of x) and differ
    only in x_loc — one of them a group of 40 terms — and two share the key with it in x."""
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    last = _mask(list(range(L, n))) | 2 if g >= 2 else _mask([L, 4])
    xs = [0, _mask([1]), _mask([b, 2]), _mask([L]), _mask([L, 1]), _mask([L, 0, 3]), _mask([L, b]),
          _mask([L, b, 2]), last]
    assert len(set(xs)) == 9
    counts = [3, 3, 3, 3, 40, 2, 2, 2, 2]
    rng = np.random.default_rng(seed)
    terms = []
    for x, k in zip(xs, counts):
        zs = set()
        while len(zs) < k:
            zs.add(int(rng.integers(0, 1 << n)))
        terms += [(_to_logical(perm, x), _to_logical(perm, z), float(rng.uniform(-1, 1))) for z in sorted(zs)]
    assert len(terms) == 60
    return terms


@pytest.mark.parametrize("world,n,name,runs", SHAPES)
def test_mixed_sum(qsim, oracle, gpu_ready, monkeypatch, world, n, name, runs):
    from qsim_amd.dist import expectation_plan
    d, c = _make(qsim, world, n, name, runs)
    sim = qsim.Simulator(n)
    for _ in range(runs):
        sim.run(c)
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    terms = _mixed_terms(n, world, perm)
    h = pauli_sum(qsim, n, terms)
    plan = expectation_plan(n, world, perm, h)
    assert (plan["local_groups"], plan["cross_groups"]) == (3, 6)
    assert plan["transfers"] == (3 if world > 2 else 2)
    before = d.getStateVector()
    a = d.expectation(h)
    assert d.expectation(h) == a                               # fixed-order sums: bit for bit
    monkeypatch.setenv("QSIM_EXPECT_SPLIT", "0")
    plain = d.expectation(h)                                   # (the 40-term cross group: split by default)
    monkeypatch.delenv("QSIM_EXPECT_SPLIT")
    assert plain == a
    monkeypatch.setenv("QSIM_DIST_EXPECT_OVERLAP", "0")
    serial = d.expectation(h)
    monkeypatch.delenv("QSIM_DIST_EXPECT_OVERLAP")
    assert abs(serial - a) <= bound(terms)
    assert d.expectation(h) == a
    assert d.perm() == perm
    own = d.getStateVector()
    assert np.array_equal(_bits(before), _bits(own))
    assert abs(a - expectation_np(own, terms)) <= bound(terms)
    assert abs(a - expectation_np(ref, terms)) <= bound(terms)
    assert abs(a - sim.expectation(h)) <= bound(terms)
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def test_cross_group_of_several_launches(qsim, oracle, gpu_ready, monkeypatch):
    """kExpectTerms + 5 = 261 terms with one physical x mask on two rank positions."""
    from qsim_amd.dist import expectation_plan
    world, n, name, runs = 8, 12, "hc", 3
    d, c = _make(qsim, world, n, name, runs)
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    L = n - 3
    x = _mask([L, n - 1, L - 1, 2])
    rng = np.random.default_rng(12)
    zs = sorted(int(v) for v in rng.choice(1 << n, size=261, replace=False))
    terms = [(_to_logical(perm, x), _to_logical(perm, z), float(rng.uniform(-1, 1))) for z in zs]
    h = pauli_sum(qsim, n, terms)
    plan = expectation_plan(n, world, perm, h)
    assert (plan["cross_groups"], plan["transfers"], plan["launches"]) == (1, 1, 2)
    before = d.getStateVector()
    a = d.expectation(h)
    assert d.expectation(h) == a
    monkeypatch.setenv("QSIM_EXPECT_SPLIT", "0")
    assert d.expectation(h) == a
    monkeypatch.delenv("QSIM_EXPECT_SPLIT")
    assert d.perm() == perm
    own = d.getStateVector()
    assert np.array_equal(_bits(before), _bits(own))
    assert abs(a - expectation_np(own, terms)) <= bound(terms)
    assert abs(a - expectation_np(ref, terms)) <= bound(terms)
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def _few_terms(n, world, perm):
    g = world.bit_length() - 1
    L = n - g
    phys = [(0, _mask([0, L]), 0.7), (_mask([1]), _mask([n - 1]), -0.4), (_mask([L, 2]), _mask([L, 5]), 1.1),
            (_mask([L, L - 1]), _mask([0]), 0.3), (_mask([n - 1]), _mask([n - 1, 3]), -0.9),
            (_mask(list(range(L, n)) + [L - 1, 4]), _mask([4, 6]), 0.5)]
    return [(_to_logical(perm, x), _to_logical(perm, z), c) for x, z, c in phys]


def test_after_run_sequence_with_carry(qsim, oracle, gpu_ready, monkeypatch):
    """QSIM_DIST_CARRY=1 (read per run) can leave a run's last step pending; the expectation
    value flushes it first, as every reader does.  Shape and circuit of
    tests/test_dist_gpu.py::test_cross_run_carry_matches_oracle."""
    from qsim_amd.dist import DistributedSimulator
    world, n = 8, 20
    monkeypatch.setenv("QSIM_DIST_CARRY", "1")
    c = qsim.createRandomHCCircuit(n, 100, 42)
    d = DistributedSimulator.virtual(n, world)
    for _ in range(3):
        d.runSequence([c])
    perm = d.perm()
    terms = _few_terms(n, world, perm)
    a = d.expectation(pauli_sum(qsim, n, terms))               # (a carried step, if any, runs first)
    assert d.perm() == perm
    own = d.getStateVector()
    ref = oracle.run_cpu(n, oracle.gates_of(c) * 3)
    np.testing.assert_allclose(own, ref, atol=1e-12, rtol=0)
    assert abs(a - expectation_np(own, terms)) <= bound(terms)
    assert abs(a - expectation_np(ref, terms)) <= bound(terms)
    assert d.expectation(pauli_sum(qsim, n, terms)) == a
    assert d.carriedRuns() >= 1, "the carry never merged"


def test_virtual_ranks_over_rccl(qsim, oracle, gpu_ready):
    """The half-shard posts as ncclSend / ncclRecv pairs and the final all-reduce through a
    world-1 RCCL communicator (tests/test_dist_readout_gpu.py::test_virtual_ranks_over_rccl)."""
    from qsim_amd.dist import DistributedSimulator
    world, n, name, runs = 4, 14, "hc", 2
    d, c = _make(qsim, world, n, name, runs, DistributedSimulator.virtual(n, world, rccl=True))
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    terms = _few_terms(n, world, perm) + _mixed_terms(n, world, perm, seed=9)
    before = d.getStateVector()
    a = d.expectation(pauli_sum(qsim, n, terms))
    assert d.expectation(pauli_sum(qsim, n, terms)) == a
    assert d.perm() == perm
    own = d.getStateVector()
    assert np.array_equal(_bits(before), _bits(own))
    assert abs(a - expectation_np(own, terms)) <= bound(terms)
    assert abs(a - expectation_np(ref, terms)) <= bound(terms)
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def test_world_one_equals_single_gpu(qsim, oracle, gpu_ready):
    """World 1: no second buffers, no cross groups — the single-GPU kernels on the one shard.
    Observed: within `bound` of Simulator.expectation, not bitwise (0.0348345360792086 against
    0.03483453607920852 under the same qubit map): the two engines plan their passes differently,
    so the amplitudes themselves differ in the last bits."""
    from qsim_amd.dist import DistributedSimulator, expectation_plan
    n = 12
    c = _circuit(qsim, n, "rand")
    d = DistributedSimulator(n, 0, 1)
    sim = qsim.Simulator(n)
    for _ in range(2):
        d.run(c)
        sim.run(c)
    rng = np.random.default_rng(21)
    xs = [0] + [int(v) for v in rng.integers(1, 1 << n, size=8)]
    terms = [(xs[int(rng.integers(0, 9))], int(rng.integers(0, 1 << n)), float(rng.uniform(-1, 1)))
             for _ in range(60)]
    h = pauli_sum(qsim, n, terms)
    plan = expectation_plan(n, 1, d.perm(), h)
    assert plan["cross_groups"] == 0 and plan["transfers"] == 0
    perm = d.perm()
    a = d.expectation(h)
    s = sim.expectation(h)
    print(f"world 1: dist {a!r} single {s!r} bitwise {a == s} same map {perm == sim.state.perm()}")
    assert abs(a - s) <= bound(terms)
    assert d.expectation(h) == a and d.perm() == perm
    own = d.getStateVector()
    assert abs(a - expectation_np(own, terms)) <= bound(terms)
    assert abs(a - expectation_np(oracle.run_cpu(n, oracle.gates_of(c) * 2), terms)) <= bound(terms)


def test_errors(qsim, gpu_ready):
    from qsim_amd import _lib
    from qsim_amd.dist import DistributedSimulator
    import ctypes
    d = DistributedSimulator.virtual(10, 4)
    with pytest.raises(ValueError):
        d.expectation(qsim.PauliSum(9).add(1.0, {0: "X"}))
    assert d.expectation(qsim.PauliSum(10)) == 0.0             # no terms: 0.0
    assert abs(d.expectation(qsim.PauliSum(10).add(1.0, {9: "Z", 0: "Z"})) - 1.0) < 1e-15   # |0..0>
    assert d.expectation(qsim.PauliSum(10).add(1.0, {9: "X"})) == 0.0
    t = (_lib.qsim_pauli_term * 1)()
    t[0].x_mask, t[0].z_mask, t[0].coeff = 1 << 10, 0, 1.0
    e = ctypes.c_double(0)
    assert _lib.hip.qsim_dist_expectation(d._h, t, 1, ctypes.byref(e)) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert _lib.hip.qsim_dist_expectation(d._h, None, 1, ctypes.byref(e)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert d.perm() == list(range(10))
