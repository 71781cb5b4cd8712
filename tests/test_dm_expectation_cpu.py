"""Density-matrix expectation values, host side (csrc/hip/dm_expect.hip lower_dm_expectation through
qsim_dm_expectation_plan): groups, rows, launches and elements read of the lowering, the argument
errors, the unchanged ABI version; and the dense checker of the GPU tests against a hand-written
case.  No GPU needed."""
import ctypes

import numpy as np

from dm_expectation_cases import dense_expectation, dense_string, tfim, z_only_strings


def _plan(n, terms, perm=None):
    from qsim_amd import _lib
    arr = (_lib.qsim_pauli_term * max(1, len(terms)))()
    for i, (x, z, c) in enumerate(terms):
        arr[i].x_mask, arr[i].z_mask, arr[i].coeff = x, z, c
    p = (ctypes.c_int32 * len(perm))(*perm) if perm is not None else None
    groups, rows, launches = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    elements = ctypes.c_uint64(0)
    rc = _lib.hip.qsim_dm_expectation_plan(n, arr, len(terms), p, ctypes.byref(groups), ctypes.byref(rows),
                                           ctypes.byref(launches), ctypes.byref(elements))
    return rc, groups.value, rows.value, launches.value, elements.value


def test_checker_on_hand_written_cases():
    """Qubit 0 is the low index bit; Tr(rho Y) = i rho[0][1] - i rho[1][0] (a non-Hermitian
    rho tells the two apart)."""
    import qsim_amd as q
    np.testing.assert_array_equal(dense_string(["X", "Z"]), np.kron(np.diag([1, -1]), [[0, 1], [1, 0]]))
    rho = np.array([[0.25, 2 + 3j], [5 - 1j, 0.75]])
    assert dense_expectation(rho, q.PauliSum(1).add(1.0, {0: "Y"})) == (1j * (2 + 3j) - 1j * (5 - 1j)).real
    assert dense_expectation(rho, q.PauliSum(1).add(2.0, {0: "X"})) == 2.0 * 7.0
    assert dense_expectation(rho, q.PauliSum(1).add(1.0, {0: "Z"}).add(3.0, {})) == -0.5 + 3.0


def test_plan_tfim_8():
    import qsim_amd as q
    n = 8
    terms = tfim(q, n).terms()
    assert len(terms) == 15
    want = (0, 9, 9, 1, 9 * 256)  # the ZZ bonds share x = 0; every X field is a group of its own
    assert _plan(n, terms) == want
    perm = [int(p) for p in np.random.default_rng(3).permutation(2 * n)]
    assert _plan(n, terms, perm) == want


def test_plan_duplicates_merge_and_zeros_drop():
    n = 6
    assert _plan(n, [(5, 2, 0.25), (5, 2, 0.5)]) == (0, 1, 1, 1, 64)
    assert _plan(n, [(5, 2, 0.25), (5, 2, -0.25)]) == (0, 0, 0, 0, 0)  # cancels: nothing to launch
    assert _plan(n, [(5, 2, 0.25), (5, 2, -0.25), (0, 7, 1.0)]) == (0, 1, 1, 1, 64)
    assert _plan(n, [(5, 2, 0.0), (0, 7, 1.0), (0, 3, 1.0)]) == (0, 1, 1, 1, 64)
    assert _plan(n, [(5, 2, 1.0), (5, 3, 1.0), (4, 2, 1.0)]) == (0, 2, 2, 1, 128)
    assert _plan(n, []) == (0, 0, 0, 0, 0)


def test_plan_300_z_only_strings_take_two_rows():
    import qsim_amd as q
    n = 9
    terms = z_only_strings(q, n, 300, 5).terms()
    assert len({z for _, z, _ in terms}) == 300 and not any(x for x, _, _ in terms)
    assert _plan(n, terms) == (0, 1, 2, 1, 512)


def test_plan_errors():
    from qsim_amd import _lib
    bad_arg, bad_range = _lib.QSIM_ERR_INVALID_ARGUMENT, _lib.QSIM_ERR_OUT_OF_RANGE
    assert _plan(4, [(1 << 4, 0, 1.0)])[0] == bad_range
    assert _plan(4, [(0, 1 << 4, 1.0)])[0] == bad_range  # (bit 4 is a row bit of the state, no qubit)
    assert _plan(4, [(0, 1 << 63, 1.0)])[0] == bad_range
    assert _plan(4, [(1, 0, 1.0)], [0] * 8)[0] == bad_arg
    assert _plan(4, [(1, 0, 1.0)], [0, 1, 2, 3, 4, 5, 6, 8])[0] == bad_arg
    assert _plan(4, [(1, 0, 1.0)], [0, 1, 2, 3, 4, 5, 6, -1])[0] == bad_arg
    assert _plan(4, [(1, 0, 1.0)], [7, 6, 5, 4, 3, 2, 1, 0])[0] == 0
    assert _plan(0, [(0, 0, 1.0)])[0] == bad_arg
    assert _plan(16, [(0, 0, 1.0)])[0] == bad_arg
    assert _plan(15, [(1 << 14, 0, 1.0)]) == (0, 1, 1, 1, 1 << 15)
    one = (_lib.qsim_pauli_term * 1)()
    i, e = ctypes.c_int(), ctypes.c_uint64()
    f = _lib.hip.qsim_dm_expectation_plan
    assert f(4, None, 1, None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(e)) == bad_arg
    assert f(4, one, 1, None, None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(e)) == bad_arg
    assert f(4, one, 1, None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), None) == bad_arg


def test_abi_version_unchanged():
    from qsim_amd import _lib
    assert _lib.hip.qsim_abi_version() == 2
