"""CPU: run-sharing cycles planned under the position cap (relayout.hip Search::copy_limit,
plan_share), through the host-only view (qsim_plan_share_host / qsim_plan_share_info).

plan_share keeps the better of the tail rule's joint plan and a sweep of position caps: the fewest
joint passes, then the smallest largest call among the calls before the last.  An 8-copy cycle is
played here call by call on the host: every state must be the oracle's after as many copies of the
circuit (1e-12 per component, the suite's amplitude bound; the host arithmetic is the oracle's),
and the cycle's bookkeeping must close as a 4-copy cycle's does."""
import numpy as np
import pytest

M = 8                  # copies per cycle (the default from 26 qubits)
ARM = 2                # the first two calls run the single-run plan whole (the second arms the cycle)
CALLS = ARM + 2 * M    # two whole cycles


@pytest.fixture
def relayout_low(qsim):
    from qsim_amd.plan import set_relayout
    set_relayout(1, 16)  # relayout plans (and with them run sharing) from 16 qubits
    yield


def _err(a, b):
    d = a - b
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


@pytest.mark.parametrize("n", [16, 18])
@pytest.mark.parametrize("seed", [42, 1, 2, 3, 4])
def test_eight_copy_cycle_states_and_bookkeeping(qsim, oracle, relayout_low, n, seed):
    from qsim_amd.plan import plan_share_host, plan_share_info
    c = qsim.createRandomHCCircuit(n, 100, seed)
    g = oracle.gates_of(c)
    joint, single, pass_copy = plan_share_info(c, M)
    assert 0 < joint < M * single, (joint, single)
    assert max(pass_copy) == M - 1 and min(pass_copy) >= 0
    ref = None
    for calls in range(1, CALLS + 1):  # the state after every number of calls (a flush ends each play)
        ref = oracle.run_cpu(n, g, state=ref) if ref is not None else oracle.run_cpu(n, g)
        st, passes, pending = plan_share_host(c, calls, M)
        assert _err(st, ref) < 1e-12, (n, seed, calls)
    assert passes[:ARM] == [single] * ARM and pending[:ARM] == [0] * ARM
    cyc_passes, cyc_pending = passes[ARM:], pending[ARM:]
    assert sum(cyc_passes[:M]) == joint
    assert cyc_pending[M - 1] == 0 and cyc_pending[2 * M - 1] == 0
    assert cyc_passes[M:] == cyc_passes[:M]  # the second cycle repeats the first
    assert cyc_passes[:M] == _per_call(pass_copy, M)
    # no launched pass holds a gate of a copy that was not yet requested
    done = 0
    for j in range(M):
        done += cyc_passes[j]
        assert all(pc <= j for pc in pass_copy[:done]), (j, pass_copy, cyc_passes)
        assert cyc_pending[j] <= (j + 1) * 100


# Joint passes of the 8-copy plan under the tail rule alone (the planner before the position cap),
# W-HC 30 qubits depth 100.
TAIL_RULE_JOINT = {42: 23, 1: 26, 3: 23}


@pytest.mark.parametrize("seed", [42, 1, 3])
def test_30_qubit_cycle_is_shorter_and_evenly_paced(qsim, seed):
    """Obtained (joint passes, passes per call): seed 42: 21, 2 2 2 2 2 3 1 7; seed 1: 23,
    3 2 2 2 2 2 2 8; seed 3: 22, 2 2 2 2 2 2 2 8 (tail rule alone: 23, 26, 23 passes)."""
    from qsim_amd.plan import plan_share_info
    c = qsim.createRandomHCCircuit(30, 100, seed)
    joint, single, pass_copy = plan_share_info(c, M)
    per_call = _per_call(pass_copy, M)
    print(f"seed {seed}: joint {joint}, single {single}, per call {per_call}")
    assert sum(per_call) == joint == len(pass_copy)
    assert 0 < joint < TAIL_RULE_JOINT[seed], (joint, per_call)
    assert sum(1 for p in per_call if p <= 2) >= 4, per_call
    assert max(per_call[:-1]) <= 3, per_call
    if seed == 42:  # unset, a 30-qubit state's cycle is this one: 8 copies
        assert plan_share_info(c) == (joint, single, pass_copy)


def test_30_qubit_four_copy_cycle_is_never_worse(qsim):
    from qsim_amd.plan import plan_share_info
    c = qsim.createRandomHCCircuit(30, 100, 42)
    joint, single, pass_copy = plan_share_info(c, 4)
    per_call = _per_call(pass_copy, 4)
    print(f"joint {joint}, single {single}, per call {per_call}")
    assert 0 < joint <= 12 and sum(per_call) == joint  # (the tail rule alone: 12, launched 2 3 3 4)
    assert max(per_call[:-1]) <= 3


def test_default_cycle_length_by_state_size(qsim, relayout_low):
    """Unset (copies 0), the cycle is 4 copies below 26 qubits; an explicit count wins."""
    from qsim_amd.plan import plan_share_info, set_run_share
    c = qsim.createRandomHCCircuit(16, 100, 42)
    set_run_share(1, 0)
    assert max(plan_share_info(c)[2]) == 3
    set_run_share(1, 8)
    assert max(plan_share_info(c)[2]) == 7
    set_run_share(1, 0)
    assert max(plan_share_info(c)[2]) == 3
    # the boundary: at exactly 26 qubits an unset count means 8 copies, at 25 still 4
    assert max(plan_share_info(qsim.createRandomHCCircuit(26, 100, 42))[2]) == 7
    assert max(plan_share_info(qsim.createRandomHCCircuit(25, 100, 42))[2]) == 3
