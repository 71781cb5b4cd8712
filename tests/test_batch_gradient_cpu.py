"""Host-side pieces of the batched sweep gradient (no GPU): qsim_batch_gradient_plan through
qsim_amd.plan.batch_gradient_plan — slots, the inverted segments, the launches of lambda = H phi,
the fused / per-gate decision, the work bytes, the plan's independence of the angles, and the
argument errors (those of qsim_batch_sweep_plan, plus the observable's)."""
import ctypes
import math

import gradient_cases as gc


def _mixed(q, n, angles):
    """All five parameterised types between H / CNOT / T / Toffoli: gate 0 precedes the first
    parameter; behind it lie the fixed runs [cnot], [t], [toffoli] and [h] (rz and cry are adjacent)."""
    a = iter(angles)
    c = q.Circuit(n)
    c.h(0)
    c.rx(1, next(a))
    c.cnot(0, 2)
    c.ry(2, next(a))
    c.t(3)
    c.crz(n - 1, 0, next(a))
    c.toffoli(0, 1, n - 1)
    c.rz(n - 2, next(a))
    c.cry(1, n - 1, next(a))
    c.h(n - 1)
    return c


# x masks 0, 2 and 8: three groups, one launch each
TERMS = [(0, 1, 0.5), (2, 0, -0.25), (2, 4, 0.75), (8, 8, 1.0)]


def test_plan_contents(qsim):
    from qsim_amd import plan
    for n, per_gate, fused in ((9, False, False), (10, False, True), (12, True, False), (12, False, True)):
        c = _mixed(qsim, n, [0.3] * 5)
        h = gc.to_pauli_sum(qsim, n, TERMS)
        for B in (1, 3, 1000):
            info = plan.batch_gradient_plan(c, B, h, per_gate=per_gate)
            assert info == {"slots": 5, "segments": 4, "apply_launches": 3, "fused": fused,
                            "work_bytes": 2 * B * 16 << n}, (n, per_gate, B, info)
    # the byte count needs both words
    c = _mixed(qsim, 10, [0.3] * 5)
    assert plan.batch_gradient_plan(c, 1 << 20, gc.to_pauli_sum(qsim, 10, TERMS))["work_bytes"] == 32 << 30
    # 600 terms of one x mask: 256 per launch
    many = gc.to_pauli_sum(qsim, 10, [(5, z, 0.01) for z in range(1, 601)])
    assert plan.batch_gradient_plan(c, 2, many)["apply_launches"] == 3
    assert plan.batch_gradient_plan(c, 2, qsim.PauliSum(10))["apply_launches"] == 0


def test_plan_does_not_depend_on_angles(qsim):
    from qsim_amd import plan
    n = 14
    infos = []
    for angles in ([0.3, -1.1, 2.2, 0.9, -0.4], [0.0] * 5, [math.pi] * 5, [2 * math.pi, 0.0, math.pi, -math.pi, 1.0]):
        c = _mixed(qsim, n, angles)
        for k in range(n):
            c.cnot(k, (k + 3) % n)
        infos.append(plan.batch_gradient_plan(c, 5, gc.to_pauli_sum(qsim, n, TERMS)))
    assert all(i == infos[0] for i in infos), infos
    assert infos[0]["segments"] == 4  # (the CNOT layer joins the trailing h)


def test_leading_gates_add_no_segment(qsim):
    from qsim_amd import plan
    n = 10
    h = gc.to_pauli_sum(qsim, n, TERMS)
    base = plan.batch_gradient_plan(_mixed(qsim, n, [0.3] * 5), 3, h)
    c = qsim.Circuit(n)
    for k in range(n):
        c.h(k)
        c.cnot(k, (k + 1) % n)
    for g in _mixed(qsim, n, [0.3] * 5).getGates():
        c.append(g)
    assert plan.batch_gradient_plan(c, 3, h) == base
    # no parameter at all: nothing is undone
    info = plan.batch_gradient_plan(qsim.createGHZCircuit(n), 3, h)
    assert info["slots"] == 0 and info["segments"] == 0
    # a parameter first and last: one segment between them
    c = qsim.Circuit(n)
    c.ry(0, 0.1)
    c.h(1)
    c.cnot(1, 2)
    c.rz(3, 0.2)
    assert plan.batch_gradient_plan(c, 3, h)["segments"] == 1


def test_errors(qsim):
    from qsim_amd import _lib
    f = _lib.hip.qsim_batch_gradient_plan
    c = _mixed(qsim, 10, [0.3] * 5)
    arr, cnt = c.to_abi()
    terms, nterms = gc.to_pauli_sum(qsim, 10, TERMS).to_abi(10)
    info = (ctypes.c_int32 * 8)()
    assert f(10, 3, arr, cnt, terms, nterms, 0, info) == _lib.QSIM_OK
    assert f(10, 3, arr, cnt, terms, nterms, _lib.QSIM_BATCH_PER_GATE, info) == _lib.QSIM_OK
    for flags in (_lib.QSIM_BATCH_REFERENCE_GATESET, _lib.QSIM_BATCH_REFERENCE_NOISE,
                  _lib.QSIM_BATCH_REFERENCE_NOISE | _lib.QSIM_BATCH_PER_GATE, 8):
        assert f(10, 3, arr, cnt, terms, nterms, flags, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 0, arr, cnt, terms, nterms, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(0, 3, arr, cnt, terms, nterms, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, None, cnt, terms, nterms, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, arr, cnt, terms, nterms, 0, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    # a qubit out of range for a 9-qubit batch: the code qsim_run gives
    assert f(9, 3, arr, cnt, terms, nterms, 0, info) == _lib.QSIM_ERR_OUT_OF_RANGE
    bad = (_lib.qsim_gate * 1)()
    bad[0].type, bad[0].nqubits = int(qsim.GateType.CRY), 2
    bad[0].qubits[0] = bad[0].qubits[1] = 4
    assert f(10, 3, bad, 1, terms, nterms, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT  # control == target
    bad[0].type = 99
    assert f(10, 3, bad, 1, terms, nterms, 0, info) == _lib.QSIM_ERR_RUNTIME  # unknown type
    # the observable: a mask bit >= n (the code qsim_state_gradient gives), a null list
    for x, z in ((1 << 10, 0), (0, 1 << 10), (1 << 63, 1)):
        wide = (_lib.qsim_pauli_term * 2)()
        wide[0].x_mask, wide[0].z_mask, wide[0].coeff = 1, 1, 0.5
        wide[1].x_mask, wide[1].z_mask, wide[1].coeff = x, z, 0.5
        assert f(10, 3, arr, cnt, wide, 2, 0, info) == _lib.QSIM_ERR_OUT_OF_RANGE
        assert f(10, 3, arr, cnt, wide, 1, 0, info) == _lib.QSIM_OK
    assert f(10, 3, arr, cnt, None, 2, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, arr, cnt, None, 0, 0, info) == _lib.QSIM_OK
    assert f(10, 3, None, 0, None, 0, 0, info) == _lib.QSIM_OK and list(info) == [0, 0, 0, 1, 3 * 32 << 10, 0, 0, 0]


def test_abi_version_unchanged(qsim):
    from qsim_amd import _lib
    assert _lib.hip.qsim_abi_version() == 2
