"""CPU: run sharing (include/qsim_hip.h qsim_set_run_share) through its host-only view.

qsim_plan_share_host plays identical fused runs of one circuit through the engine's cycle
bookkeeping (the second identical run arms a cycle of `copies` runs planned as ONE relayout plan;
each later call launches the longest prefix of joint passes whose gates were all requested; the
rest is flushed at the end) and executes every launched pass on the host with the staged kernels'
index math.  The state after k calls must be the oracle's after k copies of the circuit
(1e-12 per component, the suite's amplitude bound; the host arithmetic is the oracle's, so the
errors are rounding only)."""
import numpy as np
import pytest

M = 4        # copies per cycle (the default)
ARM = 2      # the first two calls run the single-run plan whole (the second arms the cycle)
CALLS = 9


@pytest.fixture
def relayout_low(qsim):
    from qsim_amd.plan import set_relayout
    set_relayout(1, 16)  # relayout plans (and with them run sharing) from 16 qubits
    yield


_refs = {}


def _oracle_states(qsim, oracle, n, seed, depth):
    """States after 1..CALLS copies of the circuit from |0..0> (computed once per circuit)."""
    key = (n, seed, depth)
    if key not in _refs:
        c = qsim.createRandomHCCircuit(n, depth, seed)
        g = oracle.gates_of(c)
        out, st = [], None
        for _ in range(CALLS):
            st = oracle.run_cpu(n, g, state=st) if st is not None else oracle.run_cpu(n, g)
            out.append(st)
        _refs[key] = out
    return _refs[key]


def _err(a, b):
    d = a - b
    return float(np.max(np.abs(np.concatenate([d.real, d.imag]))))


@pytest.mark.parametrize("n", [16, 18])
@pytest.mark.parametrize("seed", [42, 1, 2, 3, 4])
def test_cycle_bookkeeping_and_states(qsim, oracle, relayout_low, n, seed):
    from qsim_amd.plan import plan_share_host, plan_share_info
    c = qsim.createRandomHCCircuit(n, 100, seed)
    joint, single, pass_copy = plan_share_info(c, M)
    assert 0 < joint < M * single, (joint, single)
    assert max(pass_copy) == M - 1 and min(pass_copy) >= 0
    refs = _oracle_states(qsim, oracle, n, seed, 100)
    # calls = 1 .. 9: the state after every number of calls (a flush ends each play)
    for calls in range(1, CALLS + 1):
        st, passes, pending = plan_share_host(c, calls, M)
        assert _err(st, refs[calls - 1]) < 1e-12, (n, seed, calls)
    assert passes[:ARM] == [single] * ARM and pending[:ARM] == [0] * ARM
    cyc_passes, cyc_pending = passes[ARM:], pending[ARM:]
    # per cycle the calls launch the joint plan's passes, and nothing is pending after its last call
    assert sum(cyc_passes[:M]) == joint
    assert cyc_pending[M - 1] == 0
    assert cyc_passes[M:] == cyc_passes[:CALLS - ARM - M]  # the next cycle repeats the first
    # no launched pass holds a gate of a copy that was not yet requested
    done = 0
    for j in range(M):
        done += cyc_passes[j]
        assert all(pc <= j for pc in pass_copy[:done]), (j, pass_copy, cyc_passes)
        if done < joint:
            assert pass_copy[done] > j  # and the prefix is the longest one
        assert cyc_pending[j] <= (j + 1) * 100


def _small_circuit(qsim, n):
    """20 gates on qubits 0..7: the single plan is one pass, so four copies cannot need fewer
    than four single runs and the joint plan is refused."""
    c = qsim.Circuit(n)
    for k in range(5):
        c.h(k)
        c.cnot(k, k + 1)
        c.ry(k + 2, 0.1 * (k + 1))
        c.cz(k + 1, k + 3)
    return c


@pytest.mark.parametrize("n", [16, 18])
def test_circuit_for_which_no_cycle_pays(qsim, oracle, relayout_low, n):
    from qsim_amd.plan import plan_share_host, plan_share_info
    c = _small_circuit(qsim, n)
    assert c.getGateCount() == 20
    g = oracle.gates_of(c)
    for _ in range(2):  # the second time the refusal comes from the memo
        joint, single, pass_copy = plan_share_info(c, M)
        assert (joint, single, pass_copy) == (0, 1, [])
    ref = None
    for calls in range(1, CALLS + 1):
        ref = oracle.run_cpu(n, g, state=ref) if ref is not None else oracle.run_cpu(n, g)
        st, passes, pending = plan_share_host(c, calls, M)
        assert passes == [single] * calls and pending == [0] * calls
        assert _err(st, ref) < 1e-12, calls


def test_mode_0_runs_the_single_plan_every_call(qsim, oracle, relayout_low):
    from qsim_amd.plan import plan_share_host, plan_share_info, set_run_share
    n = 16
    c = qsim.createRandomHCCircuit(n, 100, 42)
    _, single, _ = plan_share_info(c, M)
    set_run_share(0, -1)
    st, passes, pending = plan_share_host(c, 6, M)
    assert passes == [single] * 6 and pending == [0] * 6
    assert _err(st, _oracle_states(qsim, oracle, n, 42, 100)[5]) < 1e-12


def test_copies_knob(qsim, oracle, relayout_low):
    from qsim_amd.plan import plan_share_host, plan_share_info
    n = 16
    c = qsim.createRandomHCCircuit(n, 100, 42)
    joint, single, pass_copy = plan_share_info(c, 2)
    assert 0 < joint < 2 * single and max(pass_copy) == 1
    st, passes, pending = plan_share_host(c, 6, 2)
    assert sum(passes[2:4]) == joint and pending[3] == 0 and pending[5] == 0
    assert _err(st, _oracle_states(qsim, oracle, n, 42, 100)[5]) < 1e-12
