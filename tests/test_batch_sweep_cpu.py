"""Host-side pieces of the batched parameter sweep (no GPU): qsim_batch_sweep_plan through
qsim_amd.plan.batch_sweep_plan — slots, the fused / per-gate decision, the coefficient table's
size, the member-dependent passes, the plan's independence of the angles, and the argument errors."""
import ctypes
import math

import pytest


def _mixed(q, n, angles):
    """All five parameterised types between H / CNOT / T / Toffoli; returns (circuit, slot indices)."""
    a = iter(angles)
    c = q.Circuit(n)
    c.h(0)
    c.rx(1, next(a))        # 1
    c.cnot(0, 2)
    c.ry(2, next(a))        # 3
    c.t(3)
    c.crz(n - 1, 0, next(a))  # 5
    c.toffoli(0, 1, n - 1)
    c.rz(n - 2, next(a))    # 7
    c.cry(1, n - 1, next(a))  # 8
    c.h(n - 1)
    return c, [1, 3, 5, 7, 8]


def test_slots_and_order(qsim):
    from qsim_amd import plan
    c, want = _mixed(qsim, 12, [0.1, 0.2, 0.3, 0.4, 0.5])
    assert plan.parameterised_slots(c) == want
    info = plan.batch_sweep_plan(c, 7)
    assert info["slots"] == 5
    assert info["per_gate_launches"] == len(c.getGates())
    assert plan.parameterised_slots(qsim.createGHZCircuit(5)) == []
    assert plan.batch_sweep_plan(qsim.createGHZCircuit(5), 3)["slots"] == 0


def test_fused_flag_and_table_bytes(qsim):
    from qsim_amd import plan
    for n, per_gate, fused in ((9, False, False), (10, False, True), (12, True, False), (12, False, True)):
        c, slots = _mixed(qsim, n, [0.3] * 5)
        for B in (1, 3, 1000):
            info = plan.batch_sweep_plan(c, B, per_gate=per_gate)
            assert info["fused"] is fused, (n, per_gate)
            assert info["table_bytes"] == 64 * B * len(slots)
            assert info["member_passes"] <= info["passes"]
            if fused:
                assert 1 <= info["member_passes"]
            else:
                assert info["passes"] == 0 and info["member_passes"] == 0
    # the byte count needs both words: 2^26 members x 5 slots x 64 B
    c, _ = _mixed(qsim, 10, [0.3] * 5)
    assert plan.batch_sweep_plan(c, 1 << 26)["table_bytes"] == 64 * 5 << 26


def test_rotations_in_first_layer_only(qsim):
    """Rotations on qubits 0..3 (always tile qubits), then CNOT layers pairing every qubit with far
    ones: more passes than one tile covers, the rotations in the first of them only."""
    from qsim_amd import plan
    n = 18
    c = qsim.Circuit(n)
    for k in range(4):
        c.ry(k, 0.1 * (k + 1))
    for stride in (1, 5, 7, 11, 13):
        for k in range(n):
            c.cnot(k, (k + stride) % n)
        for k in range(n):
            c.h(k)
    info = plan.batch_sweep_plan(c, 4)
    assert info["fused"] and info["slots"] == 4
    assert info["passes"] >= 2
    assert 1 <= info["member_passes"] < info["passes"]


def test_plan_does_not_depend_on_angles(qsim):
    """Angles 0 and pi lower to the identity / a closed-form sub-kind in qsim_run; a sweep plans under
    one placeholder angle, so the plan is the same whatever the circuit's angles are."""
    from qsim_amd import plan
    n = 14
    infos = []
    for angles in ([0.3, -1.1, 2.2, 0.9, -0.4], [0.0] * 5, [math.pi] * 5, [2 * math.pi, 0.0, math.pi, -math.pi, 1.0]):
        c, _ = _mixed(qsim, n, angles)
        for stride in (3, 5):
            for k in range(n):
                c.cnot(k, (k + stride) % n)
        infos.append(plan.batch_sweep_plan(c, 5))
    assert all(i == infos[0] for i in infos), infos


def test_errors(qsim):
    from qsim_amd import _lib
    f = _lib.hip.qsim_batch_sweep_plan
    c, _ = _mixed(qsim, 10, [0.3] * 5)
    arr, cnt = c.to_abi()
    info = (ctypes.c_int32 * 8)()
    assert f(10, 3, arr, cnt, 0, info) == _lib.QSIM_OK
    assert f(10, 3, arr, cnt, _lib.QSIM_BATCH_PER_GATE, info) == _lib.QSIM_OK
    for flags in (_lib.QSIM_BATCH_REFERENCE_GATESET, _lib.QSIM_BATCH_REFERENCE_NOISE,
                  _lib.QSIM_BATCH_REFERENCE_NOISE | _lib.QSIM_BATCH_PER_GATE, 8):
        assert f(10, 3, arr, cnt, flags, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 0, arr, cnt, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(0, 3, arr, cnt, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, None, cnt, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, arr, cnt, 0, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    # a qubit out of range for a 9-qubit batch: the code qsim_run gives
    assert f(9, 3, arr, cnt, 0, info) == _lib.QSIM_ERR_OUT_OF_RANGE
    bad = (_lib.qsim_gate * 1)()
    bad[0].type, bad[0].nqubits = int(qsim.GateType.CRY), 2
    bad[0].qubits[0] = bad[0].qubits[1] = 4
    assert f(10, 3, bad, 1, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT  # control == target
    bad[0].type = 99
    assert f(10, 3, bad, 1, 0, info) == _lib.QSIM_ERR_RUNTIME  # unknown type
    assert f(10, 3, None, 0, 0, info) == _lib.QSIM_OK and list(info) == [0] * 6 + [1, 0]


def test_abi_version_unchanged(qsim):
    from qsim_amd import _lib
    assert _lib.hip.qsim_abi_version() == 2
