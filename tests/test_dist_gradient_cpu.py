"""CPU: the host-only plan entry of sharded adjoint gradients (qsim_dist_gradient_plan,
qsim_amd.dist.gradient_plan): the class of every parameterised step, the inverted segments and their
remaps, the groups and transfers of lambda = H phi, the steps' transfers and the bytes a rank sends
— worked out by hand on hand-written maps, and re-derived gate by gate in Python from the map the
entry reports after the forward run.  Also the entry's error codes and the C++ test binary's build.
"""
import ctypes as c
import os
import subprocess

import numpy as np
import pytest

import gradient_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(qsim, n, world, gates, terms, perm=None):
    from qsim_amd.dist import gradient_plan
    return gradient_plan(gc.to_circuit(qsim, n, gates), world, terms, perm)


def test_symbols_and_struct(qsim):
    from qsim_amd import _lib
    for name in ("qsim_dist_gradient", "qsim_dist_gradient_release", "qsim_dist_gradient_plan",
                 "qsim_dist_gradient_memory_bytes"):
        assert hasattr(_lib.hip, name)
    assert c.sizeof(_lib.qsim_dist_gradient_info) == 20 * 4 + 8 + 2 * 64 * 4


def test_hand_worked_no_forward_remap(qsim):
    """World 4 at 10 qubits (L = 8) under a hand-written map.  Every Rx / Ry / CRY target is local,
    so the forward run never remaps and the sweep reads the circuit under the same map:
    logical 9 -> position 0, 0 -> 9 (rank bit 1), 5 -> 8 (rank bit 0), 8 -> 5, the rest in place."""
    n, world = 10, 4
    perm = [9, 1, 2, 3, 4, 8, 6, 7, 5, 0]
    gates = [
        (gc.RY, [1], 0.3),        # local
        (gc.RX, [9], 0.2),        # local (position 0)
        (gc.CRY, [2, 3], 0.1),    # local, control (2) below target (3)
        (gc.CRZ, [7, 4], 0.5),    # local, control (7) above target (4)
        (gc.CRY, [0, 6], 0.7),    # target local, control on a rank position
        (gc.CRZ, [5, 2], 0.4),    # target local, control on a rank position
        (gc.RZ, [0], 0.6),        # diagonal on a rank position
        (gc.CRZ, [3, 5], 0.8),    # diagonal on a rank position, control local
        (gc.CRZ, [0, 5], 0.9),    # diagonal on a rank position, control on the other one
        (gc.RZ, [8], -0.2),       # local (position 5)
    ]
    terms = [(0, 0b11, 1.0), (0, 1 << 9, 0.5), (1 << 9, 1 << 1, 0.25)]   # x: none, none, logical 9 = position 0
    info = _plan(qsim, n, world, gates, terms, perm)
    assert info["perm_after_run"] == perm == info["perm_after_sweep"]
    assert info["params"] == 10
    assert (info["steps_local"], info["steps_local_crank"]) == (5, 2)
    assert (info["local_ctrl_below"], info["local_ctrl_above"]) == (1, 1)
    assert (info["steps_diag"], info["steps_diag_crank"]) == (2, 1)
    assert (info["steps_cross"], info["steps_cross_crank"]) == (0, 0)
    assert (info["cross_rx"], info["cross_ry"], info["cross_cry"]) == (0, 0, 0)
    assert (info["segments"], info["remap_segments"], info["segment_remaps"]) == (0, 0, 0)
    assert (info["apply_groups_local"], info["apply_groups_cross"], info["apply_transfers"]) == (2, 0, 0)
    assert info["step_transfers"] == 0 and info["bytes_sent_per_rank"] == 0


def test_hand_worked_apply_groups(qsim):
    """H under the same map: x masks by physical position.  logical 0 -> position 9 and 5 -> 8 are
    the rank positions: x on {0} and on {0, 1} share x_rank = 2 (one transfer), x on {5} has
    x_rank = 1, x on {0, 5} x_rank = 3; x on {1} and the Z-only strings stay inside a shard."""
    n, world = 10, 4
    perm = [9, 1, 2, 3, 4, 8, 6, 7, 5, 0]
    gates = [(gc.RZ, [1], 0.3), (gc.RY, [2], 0.1)]
    X = lambda *qs: sum(1 << q for q in qs)
    terms = [(0, X(0, 5), 1.0), (0, X(3), 0.5), (X(1), 0, 0.2), (X(0), X(0), 0.3), (X(0, 1), X(2), 0.4),
             (X(5), 0, 0.6), (X(0, 5), X(5), 0.7)]
    info = _plan(qsim, n, world, gates, terms, perm)
    assert (info["apply_groups_local"], info["apply_groups_cross"], info["apply_transfers"]) == (2, 4, 3)
    assert info["apply_launches"] == 6 and info["step_transfers"] == 0
    assert info["bytes_sent_per_rank"] == 3 * 16 * (1 << 8)      # whole shards: 16 B x 2^L
    # Z-only H: nothing crosses
    z_only = [(0, X(0, 5), 1.0), (0, X(0), -0.5), (0, X(9, 3), 0.25)]
    info = _plan(qsim, n, world, gates, z_only, perm)
    assert (info["apply_groups_local"], info["apply_groups_cross"], info["apply_transfers"]) == (1, 0, 0)
    assert info["bytes_sent_per_rank"] == 0


def _classify(gates, perm, L):
    """The sweep's classes of a rotations-only circuit, re-derived from the map after the run."""
    out = dict(steps_local=0, steps_local_crank=0, steps_diag=0, steps_diag_crank=0, steps_cross=0,
               steps_cross_crank=0, cross_rx=0, cross_ry=0, cross_cry=0, local_ctrl_below=0, local_ctrl_above=0,
               step_transfers=0)
    for k, (t, q, _) in enumerate(gates):
        tp = perm[q[-1]]
        cp = perm[q[0]] if len(q) == 2 else None
        crank = cp is not None and cp >= L
        if tp < L:
            out["steps_local_crank" if crank else "steps_local"] += 1
            if cp is not None and not crank:
                out["local_ctrl_below" if cp < tp else "local_ctrl_above"] += 1
        elif t in (gc.RZ, gc.CRZ):
            out["steps_diag_crank" if crank else "steps_diag"] += 1
        else:
            out["steps_cross_crank" if crank else "steps_cross"] += 1
            out[{gc.RX: "cross_rx", gc.RY: "cross_ry", gc.CRY: "cross_cry"}[t]] += 1
            out["step_transfers"] += 1 if k == 0 else 2          # the first rotation needs phi alone
    return out


@pytest.mark.parametrize("world,n", [(2, 8), (4, 9), (4, 10), (8, 11), (8, 12)])
def test_rotations_only(qsim, world, n):
    """Rotations only: no segment, no remap in the sweep, so the map after the run classifies every
    gate; the counts must be the ones re-derived here, and the bytes the documented whole shards."""
    L = n - (world.bit_length() - 1)
    rng = np.random.default_rng(500 + n + world)
    perm = [int(v) for v in rng.permutation(n)]
    seen = set()
    for seed in range(12):
        r = np.random.default_rng(seed)
        gates = gc.random_gates(r, n, 40, types=gc.PARAMETRIC)
        terms = gc.random_terms(r, n, 8, 3)
        info = _plan(qsim, n, world, gates, terms, perm)
        assert (info["segments"], info["remap_segments"], info["segment_remaps"]) == (0, 0, 0)
        assert info["perm_after_sweep"] == info["perm_after_run"] and sorted(info["perm_after_run"]) == list(range(n))
        want = _classify(gates, info["perm_after_run"], L)
        assert {k: info[k] for k in want} == want
        assert info["params"] == 40 == sum(want[k] for k in want if k.startswith("steps_"))
        assert info["bytes_sent_per_rank"] == (info["apply_transfers"] + info["step_transfers"]) * 16 * (1 << L)
        pa = info["perm_after_run"]
        xr = {sum(1 << pa[q] for q in range(n) if x >> q & 1) >> L for x, _, _ in terms}
        assert info["apply_transfers"] == len(xr - {0})
        seen |= {k for k in want if want[k]}
    assert {"steps_local", "steps_local_crank", "steps_diag", "steps_cross"} <= seen


def test_segments(qsim):
    """Segments are the runs of other gates AFTER the first rotation (the single-GPU rule); a SWAP
    only relabels the work map; a random circuit over all 17 gate types has segments that remap."""
    n, world = 10, 4
    gates = [(gc.H, [0], 0.0), (gc.RY, [0], 0.1), (gc.CZ, [0, 1], 0.0), (gc.S, [2], 0.0), (gc.RZ, [1], 0.2),
             (gc.T, [3], 0.0), (gc.RY, [2], 0.3), (gc.H, [1], 0.0)]
    terms = [(0, 1, 1.0)]
    info = _plan(qsim, n, world, gates, terms)
    assert (info["params"], info["segments"], info["remap_segments"]) == (3, 3, 0)
    gates3 = [(gc.RZ, [0], 0.2), (gc.SWAP, [0, 9], 0.0), (gc.RZ, [0], 0.1)]       # a SWAP only relabels
    info = _plan(qsim, n, world, gates3, terms)
    assert (info["segments"], info["segment_remaps"]) == (1, 0)
    assert info["perm_after_sweep"] == list(range(n)) and info["perm_after_run"][0] == 9
    # random circuits with all 17 gate types: some segment remaps
    gates4, terms4 = gc.random_case(0, n)
    info = _plan(qsim, n, world, gates4, terms4)
    assert info["remap_segments"] >= 1 and info["segment_remaps"] >= info["remap_segments"]
    assert info["segments"] >= info["remap_segments"]


def test_world_one_is_all_local(qsim):
    n = 10
    gates, terms = gc.random_case(4, n)
    info = _plan(qsim, n, 1, gates, terms)
    assert info["params"] == info["steps_local"] > 0
    for k in ("steps_local_crank", "steps_diag", "steps_diag_crank", "steps_cross", "steps_cross_crank",
              "apply_groups_cross", "apply_transfers", "step_transfers", "segment_remaps", "bytes_sent_per_rank"):
        assert info[k] == 0, k
    assert info["apply_groups_local"] >= 1 and info["segments"] >= 1


def test_no_sweep_cases(qsim):
    n = 10
    gates, terms = gc.random_case(1, n)
    info = _plan(qsim, n, 4, gates, [])                       # H = 0: the run alone
    assert info["params"] > 0 and info["apply_launches"] == 0 and info["segments"] == 0
    info = _plan(qsim, n, 4, [(gc.H, [0], 0.0), (gc.CNOT, [0, 9], 0.0)], terms)   # no parameter: the value alone
    assert info["params"] == 0 and info["segments"] == 0 and info["step_transfers"] == 0


def test_plan_error_codes(qsim):
    from qsim_amd import _lib
    f = _lib.hip.qsim_dist_gradient_plan
    n = 10
    circ = gc.to_circuit(qsim, n, [(gc.RY, [0], 0.1)])
    arr, cnt = circ.to_abi()
    t = (_lib.qsim_pauli_term * 1)()
    t[0].x_mask, t[0].z_mask, t[0].coeff = 0, 1, 1.0
    info = _lib.qsim_dist_gradient_info()
    assert f(n, 4, None, arr, cnt, t, 1, c.byref(info)) == _lib.QSIM_OK
    assert f(n, 4, None, arr, cnt, t, 1, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(n, 3, None, arr, cnt, t, 1, c.byref(info)) == _lib.QSIM_ERR_INVALID_ARGUMENT       # not a power of two
    assert f(n, 0, None, arr, cnt, t, 1, c.byref(info)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(n, 4, None, None, cnt, t, 1, c.byref(info)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(n, 4, None, arr, cnt, None, 1, c.byref(info)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    t[0].z_mask = 1 << n
    assert f(n, 4, None, arr, cnt, t, 1, c.byref(info)) == _lib.QSIM_ERR_OUT_OF_RANGE
    t[0].z_mask, t[0].x_mask = 1, 1 << 40
    assert f(n, 4, None, arr, cnt, t, 1, c.byref(info)) == _lib.QSIM_ERR_OUT_OF_RANGE
    t[0].x_mask = 0
    bad = (_lib.qsim_gate * 1)()
    bad[0].type, bad[0].nqubits, bad[0].qubits[0], bad[0].parameter = 8, 1, n, 0.1              # Rx on qubit n
    plan_rc = _lib.hip.qsim_dist_plan(n, 4, 0, bad, 1, (c.c_int32 * n)(*range(n)), None, 0,
                                      c.byref(c.c_size_t()), None, 0, c.byref(c.c_size_t()))
    assert plan_rc != _lib.QSIM_OK and f(n, 4, None, bad, 1, t, 1, c.byref(info)) == plan_rc     # the run's code
    bad[0].type = 99
    assert f(n, 4, None, bad, 1, t, 1, c.byref(info)) == _lib.QSIM_ERR_RUNTIME
    dup = (c.c_int32 * n)(*([0] * n))
    assert f(n, 4, dup, arr, cnt, t, 1, c.byref(info)) == _lib.QSIM_ERR_INVALID_ARGUMENT        # not a permutation
    with pytest.raises(ValueError):
        from qsim_amd.dist import gradient_plan
        gradient_plan(circ, 4, [(0, 1, 1.0)], perm=[0, 1])


def test_cpp_dist_gradient_builds():
    """The header compiles with g++ alone and the method links."""
    cpp = os.path.join(ROOT, "tests", "cpp_dist_gradient")
    subprocess.run(["make", "-C", cpp], check=True, capture_output=True, text=True)
    assert os.path.exists(os.path.join(cpp, "build", "test_dist_gradient"))
