"""GPU: marginal probabilities, reduced density matrices, purity and entropies on the sharded state
(DistributedSimulator.marginalProbabilities / reducedDensityMatrix / subsystemPurity /
entanglementEntropy; csrc/hip/dist_marginal.hip) on virtual ranks.

Shapes, circuits and run counts are those of tests/test_dist_expectation_gpu.py, so the qubit map
has left the identity; the qubits are chosen by PHYSICAL position (local: lane / wave / per-thread
/ above the run; rank positions; the top local position in or out) and translated to logical
qubits through perm() read before the call.  Reference: tests/marginal_cases.py on the oracle's
state, at its tolerances.  After every case perm() and every shard's amplitudes must be
bit-identical to what they were, and the state must still run.

The cap k <= 6 leaves k_loc <= 5 to a matrix with a selected rank position, so the matrix classes
are k_loc = 0, 1 and 5 with k_rank >= 1, and k_loc = 6 with k_rank = 0.
"""
import ctypes

import numpy as np
import pytest

import marginal_cases as mc

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, "hc", 1), (4, 10, "hc", 2), (8, 12, "hc", 3), (8, 16, "hc", 2)]


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


def _make(qsim, world, n, name, runs, d=None, moved=True):
    from qsim_amd.dist import DistributedSimulator
    c = _circuit(qsim, n, name)
    d = d if d is not None else DistributedSimulator.virtual(n, world)
    for _ in range(runs):
        d.run(c)
    if moved:
        assert d.perm() != list(range(n))                      # the map has left the identity
    return d, c


def _uniq(positions, n):
    return [p for p in dict.fromkeys(positions) if 0 <= p < n]


def _marginal_positions(n, world):
    """{class: physical positions}."""
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    ranks = list(range(L, n))
    out = {
        "lane": [0, 2, 5],
        "wave": [6] if L == 7 else [6, 7],
        "rank1": [L],
        "mixed": [1, L],
        "mixed_all_kinds": _uniq([0, 6, b, n - 1], n),
        "top_local": [b],
        "top_local_and_rank": [b, L],
        "below_top_and_rank": [b - 1, n - 1],
        "shuffled": _uniq([n - 1, 0, b, 3, L], n),
        "none": [],
        "every_amplitude": list(range(n)),
    }
    if L >= 9:
        out["thread"] = [8] if L < 12 else [8, 11]
    if L > 12:
        out["above"] = [12]
        out["above_and_rank"] = [12, 3, n - 1]
    if g >= 2:
        out["rank2"] = [L, n - 1]
    if g >= 3:
        out["rank3"] = ranks
        out["rank3_shuffled_with_local"] = [n - 2, 4, n - 1, L, b]
    return out


def _rdm_positions(n, world):
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    ranks = list(range(L, n))
    out = {
        "local6": [0, 1, 2, 3, 4, 5],                          # k_loc = 6, k_rank = 0
        "local_top": [b, 2],
        "none": [],
        "rank1": [L],                                          # k_loc = 0
        "loc1_rank1": [3, L],                                  # k_loc = 1, half-shard rule
        "top_rank1": [b, L],                                   # k_loc = 1, whole shard (top selected)
        "loc5_rank1": [0, 1, 3, 5, 6, n - 1],                  # k_loc = 5 (L = 7: 6 is the top position)
        "loc5_top_rank1": _uniq([b, 0, 2, 4, 5, L], n),
        "shuffled": _uniq([n - 1, 0, L, 4], n),
    }
    if L > 12:
        out["above_rank"] = [12, 3, L]
    if g >= 2:
        out["rank2"] = [n - 1, L]
        out["loc2_rank2"] = [2, L, 6, n - 1]
    if g >= 3:
        out["rank3"] = ranks
        out["loc3_rank3"] = [1, n - 1, b - 1, L, 4, L + 1]
        out["top_rank3"] = [L + 1, b, L, n - 1]
    return out


def _logical(perm, positions):
    inv = {p: q for q, p in enumerate(perm)}
    return [inv[p] for p in positions]


def _unchanged(d, perm, shards):
    assert d.perm() == perm
    assert np.array_equal(_bits(d.localState()), _bits(shards))


@pytest.mark.parametrize("world,n,name,runs", SHAPES)
def test_marginal_by_position_class(qsim, oracle, gpu_ready, world, n, name, runs):
    d, c = _make(qsim, world, n, name, runs)
    ref = _reference(qsim, oracle, n, name, runs)
    g = world.bit_length() - 1
    L = n - g
    classes = _marginal_positions(n, world)
    # what the set covers, by physical position
    sets = [set(p) for p in classes.values()]
    assert {sum(1 for p in s if p >= L) for s in sets if s and min(s) >= L} == set(range(1, g + 1))
    assert any(s and max(s) < L for s in sets) and any(s and min(s) < L <= max(s) for s in sets)
    assert any(L - 1 in s for s in sets) and any(s and L - 1 not in s for s in sets)
    assert any(s and max(s) < 6 for s in sets) and any(s & {6, 7} for s in sets)
    assert L < 9 or any(s & {8, 9, 10, 11} for s in sets)
    assert L <= 12 or any(12 in s for s in sets)
    perm = d.perm()
    shards = d.localState()
    for cls, positions in classes.items():
        qubits = _logical(perm, positions)
        got = d.marginalProbabilities(qubits)
        want = mc.marginal_np(ref, qubits)
        err = float(np.max(np.abs(got - want)))
        print(f"marginal {world}x{n} {cls}: max err {err:.3e}")
        assert got.shape == (1 << len(qubits),)
        assert err <= mc.ATOL, cls
        assert np.array_equal(_bits(d.marginalProbabilities(qubits)), _bits(got)), cls   # fixed-order sums
        _unchanged(d, perm, shards)
    # k = n in logical order is getProbabilities()
    full = d.marginalProbabilities(list(range(n)))
    assert np.max(np.abs(full - d.getProbabilities())) <= 1e-12
    _unchanged(d, perm, shards)
    d.run(c)                                                   # and the state still runs
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


@pytest.mark.parametrize("world,n,name,runs", SHAPES)
def test_rdm_by_position_class(qsim, oracle, gpu_ready, world, n, name, runs):
    from qsim_amd.dist import marginal_plan
    d, c = _make(qsim, world, n, name, runs)
    ref = _reference(qsim, oracle, n, name, runs)
    g = world.bit_length() - 1
    L = n - g
    classes = _rdm_positions(n, world)
    perm = d.perm()
    shards = d.localState()
    seen, rules = set(), set()
    for cls, positions in classes.items():
        qubits = _logical(perm, positions)
        plan = marginal_plan(n, world, perm, qubits, rdm=True)
        k_loc, k_rank = sum(1 for p in positions if p < L), sum(1 for p in positions if p >= L)
        assert (plan["k_loc"], plan["k_rank"], plan["cross_steps"]) == (k_loc, k_rank, (1 << k_rank) - 1)
        seen.add((k_loc, k_rank))
        rules.add(plan["pair_rule"])
        rho = d.reducedDensityMatrix(qubits)
        want = mc.rdm_np(ref, qubits)
        err = float(np.max(np.abs(rho - want)))
        print(f"rdm {world}x{n} {cls}: k_loc {k_loc} k_rank {k_rank} rule {plan['pair_rule']} max err {err:.3e}")
        assert err <= mc.ATOL, cls
        assert np.array_equal(rho, rho.conj().T), cls             # rho == rho^dagger, as tests/test_marginal_gpu.py checks it
        assert not rho.diagonal().imag.any()
        assert np.array_equal(_bits(d.reducedDensityMatrix(qubits)), _bits(rho)), cls
        assert np.max(np.abs(rho.diagonal().real - d.marginalProbabilities(qubits))) <= mc.ATOL, cls
        assert abs(d.subsystemPurity(qubits) - float(np.sum(np.abs(want) ** 2))) <= mc.ATOL * want.size, cls
        _unchanged(d, perm, shards)
    assert {kl for kl, kr in seen if kr >= 1} >= {0, 1, 5}
    assert (6, 0) in seen and {kr for _, kr in seen} == set(range(g + 1))
    assert rules == {0, 1, 2}
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def _entropy_positions(n, world):
    L = n - (world.bit_length() - 1)
    return [[0, L], [3, L - 1, n - 1], [1, 2, L], [L], [5, 1]]


@pytest.mark.parametrize("world,n,name,runs", SHAPES)
def test_purity_and_entropies(qsim, oracle, gpu_ready, world, n, name, runs):
    d, _ = _make(qsim, world, n, name, runs)
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    for positions in _entropy_positions(n, world):
        qubits = _logical(perm, _uniq(positions, n))
        want = mc.rdm_np(ref, qubits)
        assert mc.spectrum_is_safe(want), positions            # (checked on the oracle's rho beforehand)
        assert abs(d.subsystemPurity(qubits) - float(np.sum(np.abs(want) ** 2))) <= mc.ATOL * want.size
        vn, r2 = d.entanglementEntropy(qubits), d.entanglementEntropy(qubits, renyi2=True)
        print(f"entropy {world}x{n} {positions}: {vn!r} (numpy {mc.entropy_np(want)!r}), Renyi-2 {r2!r}")
        assert abs(vn - mc.entropy_np(want)) <= mc.ENT_ATOL, positions
        assert abs(r2 - mc.entropy_np(want, True)) <= mc.ENT_ATOL, positions
    assert d.perm() == perm


@pytest.mark.parametrize("world,runs", [(2, 1), (4, 2)])
def test_every_subset_of_8_qubits(qsim, oracle, gpu_ready, world, runs):
    n, name = 8, "hc"
    d, c = _make(qsim, world, n, name, runs, moved=False)
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    shards = d.localState()
    worst_m = worst_r = 0.0
    for qubits in mc.all_subsets(n):
        got = d.marginalProbabilities(qubits)
        worst_m = max(worst_m, float(np.max(np.abs(got - mc.marginal_np(ref, qubits)))))
        assert worst_m <= mc.ATOL, qubits
        if len(qubits) <= 6:
            rho = d.reducedDensityMatrix(qubits)
            worst_r = max(worst_r, float(np.max(np.abs(rho - mc.rdm_np(ref, qubits)))))
            assert worst_r <= mc.ATOL, qubits
            assert np.array_equal(rho, rho.conj().T), qubits
        _unchanged(d, perm, shards)
    print(f"world {world}, 8 qubits, every subset: marginal max err {worst_m:.3e}, matrix max err {worst_r:.3e}")
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def test_virtual_ranks_over_rccl(qsim, oracle, gpu_ready):
    """The shard posts as ncclSend / ncclRecv pairs and the vector all-reduce through a world-1
    RCCL communicator (tests/test_dist_readout_gpu.py::test_virtual_ranks_over_rccl)."""
    from qsim_amd.dist import DistributedSimulator
    world, n, name, runs = 4, 14, "hc", 2
    d, c = _make(qsim, world, n, name, runs, DistributedSimulator.virtual(n, world, rccl=True))
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    shards = d.localState()
    for cls in ("lane", "rank2", "mixed_all_kinds", "shuffled", "none", "every_amplitude"):
        qubits = _logical(perm, _marginal_positions(n, world)[cls])
        got = d.marginalProbabilities(qubits)
        assert np.max(np.abs(got - mc.marginal_np(ref, qubits))) <= mc.ATOL, cls
        assert np.array_equal(_bits(d.marginalProbabilities(qubits)), _bits(got)), cls
        _unchanged(d, perm, shards)
    for cls in ("local6", "rank2", "loc1_rank1", "top_rank1", "loc5_rank1", "loc2_rank2", "shuffled"):
        qubits = _logical(perm, _rdm_positions(n, world)[cls])
        rho = d.reducedDensityMatrix(qubits)
        assert np.max(np.abs(rho - mc.rdm_np(ref, qubits))) <= mc.ATOL, cls
        assert np.array_equal(rho, rho.conj().T), cls
        assert np.array_equal(_bits(d.reducedDensityMatrix(qubits)), _bits(rho)), cls
        _unchanged(d, perm, shards)
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(ref))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


def test_random_circuit_amplitudes(qsim, oracle, gpu_ready):
    """The W-HC states above have few distinct amplitude magnitudes; a random circuit's state has
    generic ones, so every rounding of the sums shows."""
    world, n, name, runs = 8, 12, "rand", 2
    d, _ = _make(qsim, world, n, name, runs, moved=False)
    ref = _reference(qsim, oracle, n, name, runs)
    perm = d.perm()
    shards = d.localState()
    for cls, positions in _marginal_positions(n, world).items():
        qubits = _logical(perm, positions)
        assert np.max(np.abs(d.marginalProbabilities(qubits) - mc.marginal_np(ref, qubits))) <= mc.ATOL, cls
    for cls, positions in _rdm_positions(n, world).items():
        qubits = _logical(perm, positions)
        rho = d.reducedDensityMatrix(qubits)
        assert np.max(np.abs(rho - mc.rdm_np(ref, qubits))) <= mc.ATOL, cls
        assert np.array_equal(rho, rho.conj().T), cls
        assert np.array_equal(_bits(d.reducedDensityMatrix(qubits)), _bits(rho)), cls
    _unchanged(d, perm, shards)


def test_world_one(qsim, oracle, gpu_ready):
    """World 1: no second buffers and no rank positions — the single-GPU kernels on the one shard."""
    from qsim_amd.dist import DistributedSimulator
    n = 12
    c = _circuit(qsim, n, "rand")
    d = DistributedSimulator(n, 0, 1)
    d.run(c)
    d.run(c)
    ref = oracle.run_cpu(n, oracle.gates_of(c) * 2)
    for qubits in ([0, 11], [7, 2, 9, 4], []):
        assert np.max(np.abs(d.marginalProbabilities(qubits) - mc.marginal_np(ref, qubits))) <= mc.ATOL
        assert np.max(np.abs(d.reducedDensityMatrix(qubits) - mc.rdm_np(ref, qubits))) <= mc.ATOL


def test_errors(qsim, gpu_ready):
    from qsim_amd import _lib
    from qsim_amd.dist import DistributedSimulator
    n = 10
    d = DistributedSimulator.virtual(n, 4)
    d.run(qsim.createRandomHCCircuit(n, 100, 42))
    perm = d.perm()
    shards = d.localState()
    marg, rdm = _lib.hip.qsim_dist_marginal_probabilities, _lib.hip.qsim_dist_reduced_density_matrix
    arr = lambda *q: (ctypes.c_int32 * max(1, len(q)))(*q)
    out = np.full(2 << 12, 7.0)
    optr = out.ctypes.data_as(ctypes.c_void_p)
    bad, oor = _lib.QSIM_ERR_INVALID_ARGUMENT, _lib.QSIM_ERR_OUT_OF_RANGE
    for f in (marg, rdm):
        assert f(d._h, arr(1, 4, 1), 3, optr) == bad
        assert f(d._h, None, 2, optr) == bad
        assert f(d._h, arr(0, 1), 2, None) == bad
        assert f(None, arr(0, 1), 2, optr) == bad
        assert f(d._h, arr(0, n), 2, optr) == oor
        assert f(d._h, arr(-1), 1, optr) == oor
    assert marg(d._h, arr(*range(n)), n + 1, optr) == bad      # k above n
    assert rdm(d._h, arr(*range(7)), 7, optr) == bad           # k above the cap
    assert not (out != 7.0).any()                              # nothing written
    _unchanged(d, perm, shards)
    for name in ("marginalProbabilities", "reducedDensityMatrix", "subsystemPurity", "entanglementEntropy"):
        f = getattr(d, name)
        with pytest.raises(ValueError):
            f([1, 4, 1])
        with pytest.raises(IndexError):
            f([0, n])
    with pytest.raises(ValueError):
        d.reducedDensityMatrix(list(range(7)))
    _unchanged(d, perm, shards)
    assert abs(d.marginalProbabilities([])[0] - 1.0) <= mc.ATOL
    assert abs(d.reducedDensityMatrix([])[0, 0] - 1.0) <= mc.ATOL
