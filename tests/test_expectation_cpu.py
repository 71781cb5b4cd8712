"""Pauli-sum expectation values, host side (csrc/hip/expect.hip lower_expectation through
qsim_expectation_plan, qsim::PauliSum in libqsim.so, qsim_amd.PauliSum): the numpy reference the
GPU tests use, checked against dense Kronecker products; the grouping rule of the lowering; the
argument errors.  No GPU needed."""
import ctypes
import itertools

import numpy as np
import pytest


def apply_pauli(psi, x, z):
    """P|psi> for the string with masks (x, z): P|i> = i^nY (-1)^popcount(i & z) |i ^ x>."""
    idx = np.arange(psi.size, dtype=np.uint64)
    par = np.zeros(psi.size, dtype=np.int64)
    t = idx & np.uint64(z)
    while t.any():
        par ^= (t & np.uint64(1)).astype(np.int64)
        t >>= np.uint64(1)
    ny = bin(x & z).count("1")
    out = np.empty_like(psi)
    out[(idx ^ np.uint64(x)).astype(np.int64)] = (1j ** ny) * (1 - 2 * par) * psi
    return out


def expectation_np(psi, terms):
    """E = sum_t c_t vdot(psi, P_t psi).real for terms (x, z, c)."""
    return sum(c * np.vdot(psi, apply_pauli(psi, x, z)).real for x, z, c in terms)


_PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]),
          "Z": np.array([[1, 0], [0, -1]])}


def test_numpy_helper_matches_dense_kron():
    rng = np.random.default_rng(11)
    n = 3
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    psi /= np.linalg.norm(psi)
    for letters in itertools.product("IXYZ", repeat=n):  # letters[q]: the factor on qubit q
        dense = np.array([[1.0]])
        for q in range(n):  # qubit q is index bit q: the last kron factor is qubit 0
            dense = np.kron(_PAULI[letters[q]], dense)
        x = sum(1 << q for q in range(n) if letters[q] in "XY")
        z = sum(1 << q for q in range(n) if letters[q] in "ZY")
        np.testing.assert_allclose(apply_pauli(psi, x, z), dense @ psi, atol=1e-15, rtol=0)
        assert abs(expectation_np(psi, [(x, z, 0.7)]) - 0.7 * np.vdot(psi, dense @ psi).real) < 1e-15


def _plan(n, terms, perm=None):
    from qsim_amd import _lib
    arr = (_lib.qsim_pauli_term * max(1, len(terms)))()
    for i, (x, z, c) in enumerate(terms):
        arr[i].x_mask, arr[i].z_mask, arr[i].coeff = x, z, c
    p = (ctypes.c_int32 * n)(*perm) if perm is not None else None
    passes, launches = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.hip.qsim_expectation_plan(n, arr, len(terms), p, ctypes.byref(passes), ctypes.byref(launches))
    return rc, passes.value, launches.value


def test_plan_all_diagonal_terms_share_one_pass():
    n = 16
    zz = [((0), (1 << a) | (1 << b), 0.5) for a, b in itertools.combinations(range(n), 2)]
    assert len(zz) == 120
    assert _plan(n, zz) == (0, 1, 1)


def test_plan_chain_plus_x_fields():
    n = 12
    terms = [(0, 3 << q, 1.0) for q in range(n - 1)] + [(1 << q, 0, 0.3) for q in range(n)]
    assert _plan(n, terms) == (0, 1 + n, 1 + n)


def test_plan_duplicates_merge_and_zeros_drop():
    n = 8
    assert _plan(n, [(5, 2, 0.25), (5, 2, 0.5)]) == (0, 1, 1)
    assert _plan(n, [(5, 2, 0.25), (5, 2, -0.25)]) == (0, 0, 0)  # cancels: nothing to launch
    assert _plan(n, [(5, 2, 0.0), (0, 7, 1.0)]) == (0, 1, 1)
    assert _plan(n, []) == (0, 0, 0)


def test_plan_large_group_takes_several_launches():
    n = 10
    terms = [(0, z, 1.0) for z in range(1, 601)]
    rc, passes, launches = _plan(n, terms)
    assert (rc, passes) == (0, 1) and launches > 1
    # same x, distinct z: a second group with its own launches
    rc, passes2, launches2 = _plan(n, terms + [(3, z, 1.0) for z in range(5)])
    assert (rc, passes2, launches2) == (0, 2, launches + 1)


def test_plan_perm_keeps_the_pass_count():
    n = 12
    rng = np.random.default_rng(5)
    terms = [(int(rng.integers(0, 8)) << 4, int(rng.integers(0, 1 << n)), 1.0) for _ in range(60)]
    ident = _plan(n, terms)
    assert ident[0] == 0 and ident[1] == len({x for x, _, _ in terms})
    perm = [int(p) for p in rng.permutation(n)]
    assert _plan(n, terms, perm) == ident
    assert _plan(n, terms, [0] * n)[0] == 1  # not a permutation: invalid argument


def test_plan_errors():
    from qsim_amd import _lib
    assert _plan(4, [(1 << 4, 0, 1.0)])[0] == _lib.QSIM_ERR_OUT_OF_RANGE
    assert _plan(4, [(0, 1 << 63, 1.0)])[0] == _lib.QSIM_ERR_OUT_OF_RANGE
    one = (_lib.qsim_pauli_term * 1)()
    out = ctypes.c_int()
    assert _lib.hip.qsim_expectation_plan(4, None, 1, None, ctypes.byref(out), ctypes.byref(out)) == \
        _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_expectation_plan(4, one, 1, None, None, ctypes.byref(out)) == _lib.QSIM_ERR_INVALID_ARGUMENT


def test_python_pauli_sum():
    import qsim_amd as q
    h = q.PauliSum(4)
    h.add(0.5, {0: "X", 2: "Y"}).add(-1.0, {3: "Z"}).add(2.0, {})
    assert h.size() == 3 and len(h) == 3
    assert h.terms() == [(0b0101, 0b0100, 0.5), (0, 0b1000, -1.0), (0, 0, 2.0)]
    with pytest.raises(IndexError):
        h.add(1.0, {4: "X"})
    with pytest.raises(IndexError):
        h.add(1.0, {-1: "X"})
    with pytest.raises(ValueError):
        h.add(1.0, [(1, "X"), (1, "Z")])
    with pytest.raises(ValueError):
        h.add(1.0, {1: "Q"})
    with pytest.raises(ValueError):
        q.PauliSum(0)
    with pytest.raises(ValueError):
        h.to_abi(5)
    assert h.size() == 3  # a rejected term is not added


def _make(n, qubits, letters, coeff=1.0):
    from qsim_amd import _lib
    qs = (ctypes.c_int32 * max(1, len(qubits)))(*qubits)
    out = _lib.qsim_pauli_term()
    rc = _lib.api.qsim_pauli_term_make(n, qs, letters.encode(), len(qubits), coeff, ctypes.byref(out))
    return rc, out.x_mask, out.z_mask, out.coeff


def test_cpp_pauli_sum_through_libqsim():
    from qsim_amd import _lib
    assert _make(5, [0, 2, 4], "XYZ", 0.5) == (0, 0b00101, 0b10100, 0.5)
    assert _make(5, [], "", 2.0) == (0, 0, 0, 2.0)
    assert _make(5, [5], "X")[0] == _lib.QSIM_ERR_OUT_OF_RANGE
    assert _make(5, [-1], "Z")[0] == _lib.QSIM_ERR_OUT_OF_RANGE
    assert _make(5, [1, 1], "XZ")[0] == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _make(5, [1], "x")[0] == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _make(0, [], "")[0] == _lib.QSIM_ERR_INVALID_ARGUMENT
