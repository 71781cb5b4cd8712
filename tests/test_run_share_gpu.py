"""GPU: run sharing (qsim_set_run_share) — repeated fused runs of one circuit executed as calls of
one joint relayout plan, gates applied no later than the next reader.

16 and 18 qubits with the relayout threshold lowered to 16; W-HC depth 100.  Every state is compared
with the numpy oracle of as many copies of the circuit at 1e-12 per component (the suite's
amplitude bound).  The second identical run arms the cycle (it still runs its own plan whole), so
after 4 runs two calls of a 4-call cycle are done and gates are pending."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M = 4


@pytest.fixture
def relayout_low(qsim):
    from qsim_amd.plan import set_relayout
    set_relayout(1, 16)
    yield


_refs = {}


def _ref(qsim, oracle, n, seed, copies):
    """The oracle's state after `copies` runs of W-HC(n, 100, seed) from |0..0> (computed once)."""
    key = (n, seed)
    lst = _refs.setdefault(key, [])
    g = oracle.gates_of(qsim.createRandomHCCircuit(n, 100, seed))
    while len(lst) < copies:
        lst.append(oracle.run_cpu(n, g, state=lst[-1]) if lst else oracle.run_cpu(n, g))
    return lst[copies - 1]


def _err(a, b):
    d = np.asarray(a) - np.asarray(b)
    return float(np.max(np.abs(np.concatenate([d.real, d.imag]))))


def _mid_cycle(qsim, n, seed=42):
    """A simulator 2 calls into a 4-call cycle (4 runs requested), gates pending."""
    c = qsim.createRandomHCCircuit(n, 100, seed)
    sim = qsim.Simulator(n)
    for _ in range(4):
        sim.run(c)
    return sim, c


@pytest.mark.parametrize("n", [16, 18])
@pytest.mark.parametrize("seed", [42, 1, 2, 3, 4])
def test_repeated_runs(qsim, oracle, gpu_ready, relayout_low, n, seed):
    c = qsim.createRandomHCCircuit(n, 100, seed)
    for k in range(1, 7):
        sim = qsim.Simulator(n)
        for _ in range(k):
            sim.run(c)
        assert _err(sim.getStateVector(), _ref(qsim, oracle, n, seed, k)) < 1e-12, (n, seed, k)


@pytest.mark.parametrize("n", [16, 18])
@pytest.mark.parametrize("kind", ["toHost", "getProbabilities", "measureQubit", "sample", "applyGate",
                                  "applyMatrix1Q", "expectation", "gradient", "restoreLayout",
                                  "other_circuit", "per_gate_run"])
def test_flush_mid_cycle(qsim, oracle, gpu_ready, relayout_low, n, kind):
    from qsim_amd.circuit import GateOp, GateType
    sim, c = _mid_cycle(qsim, n)
    ref = _ref(qsim, oracle, n, 42, 4)
    if kind == "toHost":
        assert _err(sim.state.toHost(), ref) < 1e-12
    elif kind == "getProbabilities":
        assert float(np.max(np.abs(sim.getProbabilities() - np.abs(ref) ** 2))) < 1e-12
    elif kind == "measureQubit":
        sim.setSeed(5)
        r = sim.measureQubit(3)  # (reference semantics: index bit n - 1 - qubit)
        keep = ((np.arange(1 << n) >> (n - 1 - 3)) & 1) == r
        ref = np.where(keep, ref, 0)
        ref = ref / np.linalg.norm(ref)
    elif kind == "sample":
        u = np.random.default_rng(3).random(64)
        twin = qsim.Simulator(n)
        twin.state.fromHost(ref)
        assert np.count_nonzero(sim.state.sampleWith(u) != twin.state.sampleWith(u)) <= 1
    elif kind == "applyGate":
        sim.applyGate(GateOp(GateType.H, [5]))
        h = qsim.Circuit(n)
        h.h(5)
        ref = oracle.run_cpu(n, oracle.gates_of(h), state=ref)
    elif kind == "applyMatrix1Q":
        sim.state.applyMatrix1Q(2, [0, 1, 1, 0])
        x = qsim.Circuit(n)
        x.x(2)
        ref = oracle.run_cpu(n, oracle.gates_of(x), state=ref)
    elif kind == "expectation":
        h = qsim.PauliSum(n)
        h.add(1.0, {0: "Z", 3: "Z"})
        idx = np.arange(1 << n)
        sign = 1.0 - 2.0 * (((idx >> 0) ^ (idx >> 3)) & 1)
        assert abs(sim.expectation(h) - float(np.sum(sign * np.abs(ref) ** 2))) < 1e-10
    elif kind == "gradient":
        h = qsim.PauliSum(n)
        h.add(1.0, {1: "Z"})
        c2 = qsim.Circuit(n)
        c2.ry(1, 0.3)
        value, _ = sim.gradient(c2, h)
        ref = oracle.run_cpu(n, oracle.gates_of(c2), state=ref)
        sign = 1.0 - 2.0 * ((np.arange(1 << n) >> 1) & 1)
        assert abs(value - float(np.sum(sign * np.abs(ref) ** 2))) < 1e-10
    elif kind == "restoreLayout":
        sim.state.restoreLayout()
        assert not sim.state.layoutInfo()["relabeled"]
    elif kind == "other_circuit":
        o = qsim.createRandomHCCircuit(n, 100, 9)
        sim.run(o)
        ref = oracle.run_cpu(n, oracle.gates_of(o), state=ref)
    elif kind == "per_gate_run":
        sim.state.run(c, qsim.RunMode.PerGate)
        ref = oracle.run_cpu(n, oracle.gates_of(c), state=ref)
    assert _err(sim.getStateVector(), ref) < 1e-12, kind
    for _ in range(2):  # two more runs (the second arms a cycle again), then read
        sim.run(c)
        ref = oracle.run_cpu(n, oracle.gates_of(c), state=ref)
    assert _err(sim.getStateVector(), ref) < 1e-12, kind


@pytest.mark.parametrize("n", [16, 18])
def test_circuit_for_which_no_cycle_pays(qsim, oracle, gpu_ready, relayout_low, n):
    """20 gates on qubits 0..7 (one pass): the joint plan is refused, every run executes the single
    plan and nothing is ever pending (sync alone makes the state readable through the twin check)."""
    from qsim_amd.plan import plan_share_info
    c = qsim.Circuit(n)
    for k in range(5):
        c.h(k)
        c.cnot(k, k + 1)
        c.ry(k + 2, 0.1 * (k + 1))
        c.cz(k + 1, k + 3)
    assert plan_share_info(c, M)[0] == 0
    g = oracle.gates_of(c)
    sim = qsim.Simulator(n)
    ref = None
    for k in range(1, 7):
        sim.run(c)
        ref = oracle.run_cpu(n, g, state=ref) if ref is not None else oracle.run_cpu(n, g)
        assert sim.state.lastRunInfo()[0] == 1, k
    assert _err(sim.getStateVector(), ref) < 1e-12
    for k in range(3):  # and again after a reader
        sim.run(c)
        ref = oracle.run_cpu(n, g, state=ref)
        assert sim.state.lastRunInfo()[0] == 1
    assert _err(sim.getStateVector(), ref) < 1e-12


@pytest.mark.parametrize("n", [16, 18])
@pytest.mark.parametrize("runs", [2, 3])
def test_short_repeat_loops(qsim, oracle, gpu_ready, relayout_low, n, runs):
    """'run twice (or three times), read' never completes a cycle, so the state backs off (it arms
    after 1, then 3, then 7 ... further repeats); armed or not, every read equals the oracle."""
    c = qsim.createRandomHCCircuit(n, 100, 42)
    sim = qsim.Simulator(n)
    for it in range(6):
        for _ in range(runs):
            sim.run(c)
        assert _err(sim.getStateVector(), _ref(qsim, oracle, n, 42, (it + 1) * runs)) < 1e-12, it


@pytest.mark.parametrize("n", [16, 18])
def test_device_ptr_mid_cycle(qsim, oracle, gpu_ready, relayout_low, n):
    sim, c = _mid_cycle(qsim, n)
    ptr = sim.state.devicePtr()
    sim.synchronize()
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(1 << n, dtype=np.complex128)

    def read():
        sim.synchronize()
        assert hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes, 2) == 0
        return out

    assert _err(read(), _ref(qsim, oracle, n, 42, 4)) < 1e-12
    single = None
    for k in (5, 6, 7):  # later runs do not defer: the pointer sees every run at once
        sim.run(c)
        assert _err(read(), _ref(qsim, oracle, n, 42, k)) < 1e-12
        single = single or sim.state.lastRunInfo()[0]
        assert sim.state.lastRunInfo()[0] == single


@pytest.mark.parametrize("n", [16, 18])
def test_discarding_pending_gates(qsim, oracle, gpu_ready, relayout_low, n):
    sim, c = _mid_cycle(qsim, n)
    sim.state.initializeZero()
    sim.run(c)
    assert _err(sim.getStateVector(), _ref(qsim, oracle, n, 42, 1)) < 1e-12
    sim2, _ = _mid_cycle(qsim, n)
    sim2.state.close()  # destroying a state with pending gates


@pytest.mark.parametrize("n", [16, 18])
def test_pass_counts_and_agreement(qsim, oracle, gpu_ready, relayout_low, n):
    from qsim_amd.plan import plan_share_info, set_run_share
    c = qsim.createRandomHCCircuit(n, 100, 42)
    joint, _, _ = plan_share_info(c, M)
    assert joint > 0
    sim = qsim.Simulator(n)
    counts = []
    for _ in range(2 + 2 * M):
        sim.run(c)
        counts.append(sim.state.lastRunInfo()[0])
    assert counts[0] == counts[1]  # the single-run plan, twice
    assert sum(counts[2:2 + M]) == joint and counts[2 + M:] == counts[2:2 + M]
    shared = sim.getStateVector()
    set_run_share(0, -1)
    plain = qsim.Simulator(n)
    for _ in range(2 + 2 * M):
        plain.run(c)
        assert plain.state.lastRunInfo()[0] == counts[0]
    assert _err(shared, plain.getStateVector()) < 1e-12
    assert _err(shared, _ref(qsim, oracle, n, 42, 2 + 2 * M)) < 1e-12
