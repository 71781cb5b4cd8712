"""GPU: 8-copy run-sharing cycles planned under the position cap (qsim_set_run_share(1, 8)).

20 and 22 qubits with the relayout threshold lowered to 16; W-HC depth 100, seed 42.  Every state
is compared with the numpy oracle of as many copies of the circuit at 1e-12 per component (the
suite's amplitude bound).  The second identical run arms the cycle (it still runs its own plan
whole), so run 2 + j is call j of a cycle; up to about one and a half copies are pending mid-cycle
and a reader there flushes them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M = 8
ARM = 2
SEED = 42


@pytest.fixture
def eight_copies(qsim):
    from qsim_amd.plan import set_relayout, set_run_share
    set_relayout(1, 16)
    set_run_share(1, M)
    yield


_refs = {}


def _ref(qsim, oracle, n, copies):
    """The oracle's state after `copies` runs of W-HC(n, 100, SEED) from |0..0> (computed once)."""
    lst = _refs.setdefault(n, [])
    g = oracle.gates_of(qsim.createRandomHCCircuit(n, 100, SEED))
    while len(lst) < copies:
        lst.append(oracle.run_cpu(n, g, state=lst[-1]) if lst else oracle.run_cpu(n, g))
    return lst[copies - 1]


def _err(a, b):
    d = np.asarray(a) - np.asarray(b)
    return float(np.max(np.abs(np.concatenate([d.real, d.imag]))))


def _per_call(pass_copy, copies):
    """Passes each call of a cycle launches: the longest prefix of passes of copies < call."""
    out, k = [], 0
    for call in range(1, copies + 1):
        first = k
        while k < len(pass_copy) and pass_copy[k] < call:
            k += 1
        out.append(k - first)
    return out


@pytest.mark.parametrize("n", [20, 22])
def test_two_cycles_and_pass_counts(qsim, oracle, gpu_ready, eight_copies, n):
    from qsim_amd.plan import plan_share_info
    c = qsim.createRandomHCCircuit(n, 100, SEED)
    joint, single, pass_copy = plan_share_info(c, M)
    assert 0 < joint < M * single
    sim = qsim.Simulator(n)
    counts = []
    for _ in range(ARM + 2 * M):
        sim.run(c)
        counts.append(sim.state.lastRunInfo()[0])
    print(f"{n} qubits: joint {joint}, single {single}, passes per run {counts}")
    assert counts[:ARM] == [single] * ARM  # the single-run plan, twice
    assert counts[ARM:ARM + M] == _per_call(pass_copy, M)  # the host view's launches
    assert counts[ARM + M:] == counts[ARM:ARM + M]
    assert _err(sim.getStateVector(), _ref(qsim, oracle, n, ARM + 2 * M)) < 1e-12


@pytest.mark.parametrize("n", [20, 22])
def test_read_after_every_run(qsim, oracle, gpu_ready, eight_copies, n):
    """Every one of the 2 + 2 * 8 runs against the oracle.  A read flushes and ends the cycle, so
    each prefix is run on a state of its own (the pass counts are the test above's)."""
    c = qsim.createRandomHCCircuit(n, 100, SEED)
    for runs in range(1, ARM + 2 * M + 1):
        sim = qsim.Simulator(n)
        for _ in range(runs):
            sim.run(c)
        assert _err(sim.state.toHost(), _ref(qsim, oracle, n, runs)) < 1e-12, (n, runs)
        sim.state.close()


@pytest.mark.parametrize("n", [20, 22])
@pytest.mark.parametrize("call", [3, 6])
def test_read_mid_cycle(qsim, oracle, gpu_ready, eight_copies, n, call):
    c = qsim.createRandomHCCircuit(n, 100, SEED)
    sim = qsim.Simulator(n)
    for _ in range(ARM + call):
        sim.run(c)
    assert _err(sim.state.toHost(), _ref(qsim, oracle, n, ARM + call)) < 1e-12
    for _ in range(2):  # two more runs after the flush, then read again
        sim.run(c)
    assert _err(sim.getStateVector(), _ref(qsim, oracle, n, ARM + call + 2)) < 1e-12
