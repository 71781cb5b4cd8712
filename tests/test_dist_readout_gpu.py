"""GPU: readout of the sharded state without gathering it — sampleWith, getProbabilities,
collapse / measureBit / measureQubit of DistributedSimulator — on virtual ranks.

Sampling follows tests/test_sampling_gpu.py: the sharded sampler must return the reference's
lower_bound over the sequential CDF in logical index order, and may differ from it (and from the
single-GPU sampler) only at rounding ties, proven per mismatching shot by _assert_tie_only (copied
from that file).  The cases run the circuits one to three times so the qubit map has left the
identity; the run counts were chosen on the CPU with the host planner (qsim_amd.dist.plan +
sample_plan) so that all but one case start sampling with one of the chunk's logical qubits on a
rank position (the localization remap), and one starts with none (the direct path); each case
asserts which of the two it is from perm() before the call.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _assert_tie_only(probs, u, got, exp):
    seq = np.add.accumulate(probs)  # sequential left-to-right, == std::partial_sum
    bad = np.nonzero(got != exp)[0]
    for i in bad:
        a, b = int(min(got[i], exp[i])), int(max(got[i], exp[i]))
        # lower_bound semantics: every index in [a, b) has its CDF step straddling u
        assert b - a == 1 or np.all(probs[a + 1:b] == 0.0), \
            f"shot {i}: indices {got[i]} vs {exp[i]} are not adjacent steps"
        k = a
        exact = math.fsum(probs[:k + 1])
        lo, hi = min(seq[k], exact), max(seq[k], exact)
        tol = 4 * np.spacing(u[i])
        assert lo - tol <= u[i] <= hi + tol, \
            f"shot {i}: u={u[i]!r} is not between C_seq={seq[k]!r} and C_exact={exact!r} at {k}"
    return len(bad)


def _circuit(qsim, n, name):
    return qsim.createRandomHCCircuit(n, 100, 42) if name == "hc" else qsim.createRandomCircuit(n, 100, 5)


_REF = {}


def _reference(qsim, oracle, n, name, runs):
    """(oracle state, its probabilities) of `runs` runs of the circuit; computed once, read-only."""
    key = (n, name, runs)
    if key not in _REF:
        g = oracle.gates_of(_circuit(qsim, n, name))
        st = oracle.run_cpu(n, g * runs)
        st.setflags(write=False)
        p = np.abs(st) ** 2
        p.setflags(write=False)
        _REF[key] = (st, p)
    return _REF[key]


def _uniforms(probs, seed, k_random=6000, k_steps=600):
    """Random uniforms, uniforms within an ulp of CDF steps, and one past the end."""
    rng = np.random.default_rng(seed)
    seq = np.add.accumulate(probs)
    steps = rng.integers(0, probs.size - 1, k_steps)
    u = np.concatenate([rng.random(k_random), np.nextafter(seq[steps], 0.0), seq[steps],
                        np.nextafter(seq[steps], 2.0)])
    u = u[(u > 0) & (u < 1)]
    return np.concatenate([u, [1.5]]), k_random


def _low_qubit_on_rank_position(d, n, world):
    L = n - (world.bit_length() - 1)
    c = min(12, L)
    perm = d.perm()
    return any(perm[q] >= L for q in range(c))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# (world, n, circuit, runs, a chunk qubit starts on a rank position).  (4, 10) and (8, 12): c = L <
# 12; (8, 16): 16 chunks of 2^12; (2, 20): 256 chunks of 2^12.
SAMPLING_CASES = [
    (2, 8, "hc", 1, True), (2, 8, "rand", 2, True),
    (4, 10, "hc", 2, True), (4, 10, "rand", 3, True),
    (8, 12, "hc", 3, True), (8, 12, "rand", 1, True),
    (8, 16, "hc", 2, True), (8, 16, "rand", 3, True),
    (2, 20, "hc", 2, False), (2, 20, "rand", 1, True),
]


@pytest.mark.parametrize("world,n,name,runs,localizes", SAMPLING_CASES)
def test_sampling_matches_sequential_cdf(qsim, oracle, gpu_ready, world, n, name, runs, localizes):
    from qsim_amd.dist import DistributedSimulator, sample_plan
    c = _circuit(qsim, n, name)
    st, probs = _reference(qsim, oracle, n, name, runs)
    d = DistributedSimulator.virtual(n, world)
    sim = qsim.Simulator(n)
    for _ in range(runs):
        d.run(c)
        sim.run(c)
    assert d.perm() != list(range(n))
    # which path this case takes, read from the layout before the call
    assert _low_qubit_on_rank_position(d, n, world) == localizes
    assert (sample_plan(n, world, d.perm())[1] != 0) == localizes
    before = d.getStateVector()
    perm_before = d.perm()
    # (each tie is proven with an exactly rounded prefix sum over up to 2^n terms, and at 20 qubits
    # most step-aimed uniforms are ties of the sequential CDF: fewer of them there)
    u, k_random = _uniforms(probs, 1000 + n, k_steps=600 if n <= 16 else 40)
    got = d.sampleWith(u)
    assert got.dtype == np.int64 and got.shape == u.shape
    assert got[-1] == 1 << n                                   # past the end
    exp = oracle.sample_cpu(n, st, u)
    _assert_tie_only(probs, u, got, exp)
    assert np.count_nonzero(got[:k_random] != exp[:k_random]) <= 2
    single = sim.state.sampleWith(u)
    _assert_tie_only(probs, u, got, single)
    # the sampler moved qubits (or not), never amplitudes
    assert not _low_qubit_on_rank_position(d, n, world)
    assert (d.perm() != perm_before) == localizes
    after = d.getStateVector()
    assert np.array_equal(_bits(before), _bits(after))
    np.testing.assert_allclose(after, st, atol=1e-12, rtol=0)
    # same state, same layout, same uniforms: the same shots, bit for bit (fixed-order sums)
    assert np.array_equal(d.sampleWith(u), got)
    # and the state still runs: one more circuit on the new layout
    d.run(c)
    ref2 = oracle.run_cpu(n, oracle.gates_of(c), state=np.array(st))
    np.testing.assert_allclose(d.getStateVector(), ref2, atol=1e-12, rtol=0)


@pytest.mark.parametrize("world,n,name,runs", [(2, 8, "hc", 1), (8, 12, "rand", 1), (8, 16, "hc", 2), (4, 14, "rand", 2)])
def test_probabilities_match_oracle(qsim, oracle, gpu_ready, world, n, name, runs):
    from qsim_amd.dist import DistributedSimulator
    c = _circuit(qsim, n, name)
    _, probs = _reference(qsim, oracle, n, name, runs)
    d = DistributedSimulator.virtual(n, world)
    for _ in range(runs):
        d.run(c)
    assert d.perm() != list(range(n))
    p = d.getProbabilities()
    assert p.dtype == np.float64 and p.shape == (1 << n,)
    np.testing.assert_allclose(p, probs, atol=1e-12, rtol=0)


def _pick_bit(d, sim, n, world, where):
    """A logical bit whose physical position is local / on a rank bit, read from perm(); among
    those, the one whose outcomes are most balanced (both must be possible)."""
    L = n - (world.bit_length() - 1)
    perm = d.perm()
    bits = [q for q in range(n) if (perm[q] >= L) == (where == "global")]
    assert bits
    return min(bits, key=lambda q: abs(sim.state.probBitZero(q) - 0.5))


def _pair(qsim, n, world, runs=2):
    from qsim_amd.dist import DistributedSimulator
    c = _circuit(qsim, n, "rand")
    d = DistributedSimulator.virtual(n, world)
    sim = qsim.Simulator(n)
    for _ in range(runs):
        d.run(c)
        sim.run(c)
    return d, sim


@pytest.mark.parametrize("where", ["local", "global"])
@pytest.mark.parametrize("result", [0, 1])
def test_collapse_matches_single_gpu(qsim, gpu_ready, where, result):
    n, world = 12, 4
    d, sim = _pair(qsim, n, world)
    bit = _pick_bit(d, sim, n, world, where)
    p0 = sim.state.probBitZero(bit)
    assert abs(d.probBitZero(bit) - p0) < 1e-12
    scale = 1.0 / math.sqrt(p0 if result == 0 else 1.0 - p0)
    perm = d.perm()
    d.collapse(bit, result, scale)
    sim.state.collapse(bit, result, scale)
    assert d.perm() == perm                                    # the layout is left as it is
    np.testing.assert_allclose(d.getStateVector(), sim.getStateVector(), atol=1e-12, rtol=0)
    assert abs(d.getTotalProbability() - 1.0) < 1e-12


@pytest.mark.parametrize("where", ["local", "global"])
@pytest.mark.parametrize("result", [0, 1])
def test_measure_bit_with_supplied_uniform(qsim, gpu_ready, where, result):
    n, world = 12, 4
    d, sim = _pair(qsim, n, world)
    bit = _pick_bit(d, sim, n, world, where)
    p0 = sim.state.probBitZero(bit)
    assert 1e-3 < p0 < 1 - 1e-3
    u = p0 / 2 if result == 0 else (1 + p0) / 2
    assert d.measureBit(bit, uniform=u) == result
    sim.state.collapse(bit, result, 1.0 / math.sqrt(p0 if result == 0 else 1.0 - p0))
    np.testing.assert_allclose(d.getStateVector(), sim.getStateVector(), atol=1e-12, rtol=0)
    assert abs(d.getTotalProbability() - 1.0) < 1e-12
    assert abs(d.probBitZero(bit) - (1.0 if result == 0 else 0.0)) < 1e-12
    for u2 in (0.01, 0.5, 0.99):                               # measured again: the same result
        assert d.measureBit(bit, uniform=u2) == result
    assert abs(d.getTotalProbability() - 1.0) < 1e-12


def test_measure_qubit_is_bit_n_minus_1_minus_q(qsim, gpu_ready):
    n, world = 12, 4
    for q in (0, 5, 11):
        a, _ = _pair(qsim, n, world)
        b, _ = _pair(qsim, n, world)
        ra = a.measureQubit(q, uniform=0.37)
        rb = b.measureBit(n - 1 - q, uniform=0.37)
        assert ra == rb
        assert np.array_equal(_bits(a.getStateVector()), _bits(b.getStateVector()))
        assert abs(a.probBitZero(n - 1 - q) - (1.0 if ra == 0 else 0.0)) < 1e-12


def test_measure_with_generator_and_seed(qsim, gpu_ready):
    n, world = 10, 4
    outs = []
    for _ in range(2):
        d, _ = _pair(qsim, n, world, runs=1)
        d.setSeed(11)
        outs.append(([d.measureQubit(q) for q in range(4)], d.sample(50)))
        assert abs(d.getTotalProbability() - 1.0) < 1e-12
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1])
    # the seeded draws are StateVector._uniforms' draws
    d, _ = _pair(qsim, n, world, runs=1)
    d.setSeed(5)
    u = np.random.default_rng(5).random(64)
    want = d.sampleWith(u)
    d.setSeed(5)
    assert np.array_equal(d.sample(64), want)


def test_zero_probability_outcome_raises(qsim, gpu_ready):
    from qsim_amd.dist import DistributedSimulator
    n, world = 10, 4
    d = DistributedSimulator.virtual(n, world)                 # |0..0>: bit = 1 has probability 0
    for bit in (0, n - 1):                                     # a local and a rank position
        with pytest.raises(RuntimeError, match="Measurement result 1 has zero probability"):
            d.measureBit(bit, uniform=1.0)
        assert d.measureBit(bit, uniform=0.5) == 0
    np.testing.assert_allclose(d.getStateVector()[0], 1.0, atol=1e-15)
    with pytest.raises(ValueError):
        d.collapse(n, 0, 1.0)
    with pytest.raises(ValueError):
        d.collapse(0, 2, 1.0)
    with pytest.raises(ValueError):
        d.probBitZero(-1)


def _sample_and_measure(qsim, oracle, d, n, world):
    c = _circuit(qsim, n, "hc")
    st, probs = _reference(qsim, oracle, n, "hc", 2)
    d.run(c)
    d.run(c)
    u, _ = _uniforms(probs, 77, k_random=3000, k_steps=300)
    got = d.sampleWith(u)
    assert got[-1] == 1 << n
    _assert_tie_only(probs, u, got, oracle.sample_cpu(n, st, u))
    np.testing.assert_allclose(d.getProbabilities(), probs, atol=1e-12, rtol=0)
    np.testing.assert_allclose(d.getStateVector(), st, atol=1e-12, rtol=0)
    L = n - (world.bit_length() - 1)
    perm = d.perm()
    bit = max(range(n), key=lambda q: perm[q])                 # the highest position (a rank bit if any)
    assert world == 1 or perm[bit] >= L
    p0 = float(probs[((np.arange(1 << n) >> bit) & 1) == 0].sum())
    r = d.measureBit(bit, uniform=(1 + p0) / 2)
    assert r == 1
    want = np.where(((np.arange(1 << n) >> bit) & 1) == 1, st, 0.0) / math.sqrt(1.0 - p0)
    np.testing.assert_allclose(d.getStateVector(), want, atol=1e-12, rtol=0)
    assert abs(d.getTotalProbability() - 1.0) < 1e-12
    assert d.measureBit(bit, uniform=0.2) == 1


def test_virtual_ranks_over_rccl(qsim, oracle, gpu_ready):
    """The collectives of the readout (vector all-reduce) through a world-1 RCCL communicator."""
    from qsim_amd.dist import DistributedSimulator
    _sample_and_measure(qsim, oracle, DistributedSimulator.virtual(14, 4, rccl=True), 14, 4)


def test_world_one_communicator(qsim, oracle, gpu_ready):
    from qsim_amd.dist import DistributedSimulator
    _sample_and_measure(qsim, oracle, DistributedSimulator(14, 0, 1), 14, 1)
