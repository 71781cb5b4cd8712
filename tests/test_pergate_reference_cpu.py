"""CPU: the dense numpy reference of tests/pergate_cases.py against the oracle, before any GPU test
relies on it.  Every case of the operand matrix at n = 3, 7, 10: dense_apply equals
oracle.run_cpu (the CPUSimulator restatement) at 1e-14 per component, and changes nothing outside
its may_change mask.  Pins the control / target conventions of both a second time."""
import numpy as np
import pytest

import pergate_cases as pc


def test_case_counts():
    # 7 positions: 11 x 7 one-qubit, 4 x 42 controlled + 21 SWAP, 7 x C(6, 2) Toffoli + 3 reversed
    assert pc.default_positions(10) == [0, 2, 3, 5, 6, 7, 9]
    assert len(pc.operand_cases(10)) == 77 + 168 + 21 + 105 + 3 == 374
    assert len(pc.operand_cases(7)) == 374
    assert len(pc.operand_cases(3)) == 33 + 24 + 3 + 3 + 3
    assert pc.operand_cases(10) == pc.operand_cases(10)  # deterministic (parent and child agree)
    tof = [qs for t, qs, _ in pc.operand_cases(10) if t == pc.TOFFOLI]
    assert sum(1 for qs in tof if qs[0] > qs[1]) == 3  # both control orders of a few triples
    for t, qs, p in pc.operand_cases(10):
        if t in (pc.RX, pc.RY, pc.RZ, pc.CRY, pc.CRZ):  # no angle near a multiple of pi/2
            assert abs(p / (np.pi / 2) - round(p / (np.pi / 2))) > 0.05, p
    for want in [(0, [6]), (6, [0, 5]), (9, [6, 7]), (2, [3, 6, 7]), (7, [2, 6, 9])]:
        assert want in pc.matrix_cases(10)


@pytest.mark.parametrize("n", [3, 7, 10])
def test_dense_reference_equals_oracle(oracle, n):
    psi = pc.random_state(n, 300 + n)
    cases = pc.operand_cases(n)
    if n == 10:
        assert len(cases) == 374
    seen = set()
    for t, qs, p in cases:
        want, may = pc.dense_apply(n, psi, t, qs, p)
        ref = oracle.run_cpu(n, [(t, qs, p)], state=psi)
        err = max(np.max(np.abs(want.real - ref.real)), np.max(np.abs(want.imag - ref.imag)))
        assert err <= 1e-14, (pc.NAMES[t], qs, p, err)
        changed = want.view(np.uint64).reshape(-1, 2) != psi.view(np.uint64).reshape(-1, 2)
        assert not changed.any(axis=1)[~may].any(), (pc.NAMES[t], qs)
        # (a dense random state and an angle off the multiples of pi/2: the gate moves all it may)
        assert changed.any(axis=1)[may].all(), (pc.NAMES[t], qs)
        seen.add(t)
    assert seen == set(range(17))


def test_controlled_matrix_reference_equals_oracle(oracle):
    """dense_matrix1q with the Ry matrix under 0, 1 and 2 controls is Ry, CRY and, with X, Toffoli."""
    n = 10
    psi = pc.random_state(n, 41)
    c, s = np.cos(0.35), np.sin(0.35)
    ry = np.array([[c, -s], [s, c]])
    for t, cs in pc.matrix_cases(n):
        got, may = pc.dense_matrix1q(n, psi, t, ry, cs[:1])
        ref = oracle.run_cpu(n, [(pc.CRY, [cs[0], t], 0.7)], state=psi)
        assert np.max(np.abs(got - ref)) <= 1e-14
        assert np.array_equal(got[~may], psi[~may])
        if len(cs) >= 2:
            got, may = pc.dense_matrix1q(n, psi, t, [[0, 1], [1, 0]], cs[:2])
            assert np.array_equal(got, oracle.run_cpu(n, [(pc.TOFFOLI, cs[:2] + [t], 0.0)], state=psi))
            assert np.count_nonzero(may) == 1 << (n - 2)


def test_check_case_catches_what_it_should():
    n = 7
    psi = pc.random_state(n, 1)
    want, may = pc.dense_apply(n, psi, pc.CZ, [6, 2])
    assert pc.check_case(want.copy(), psi, want, may, True) == 0.0
    bad = want.copy()
    k = int(np.flatnonzero(~may)[5])
    bad[k] = bad[k] * (1.0 + 2.0 ** -52)  # one ulp outside the subspace
    with pytest.raises(AssertionError, match="outside"):
        pc.check_case(bad, psi, want, may, True)
    bad = want.copy()
    k = int(np.flatnonzero(may)[3])
    bad[k] = bad[k] * (1.0 + 2.0 ** -52)
    with pytest.raises(AssertionError, match="exact"):
        pc.check_case(bad, psi, want, may, True)
    assert pc.check_case(bad, psi, want, may, False) < 1e-15
    bad[k] += 2e-12
    with pytest.raises(AssertionError, match="max component"):
        pc.check_case(bad, psi, want, may, False)
