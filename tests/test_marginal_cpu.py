"""Host-only checks of the marginal / reduced-density-matrix lowering (qsim_marginal_plan) and of
the C++ layer's entropy routine (qsim_hermitian_entropy); no GPU."""
import numpy as np
import pytest

import marginal_cases as mc

MIB = 1 << 20
RUN_BITS = 12  # a work-group's contiguous run is 2^min(n, 12) amplitudes


def test_plan_validation(qsim):
    from qsim_amd.plan import marginal_plan
    for rdm in (False, True):
        with pytest.raises(ValueError):
            marginal_plan(10, [1, 4, 1], rdm=rdm)  # duplicate
        with pytest.raises(IndexError):
            marginal_plan(10, [0, 10], rdm=rdm)
        with pytest.raises(IndexError):
            marginal_plan(10, [-1], rdm=rdm)
        with pytest.raises(ValueError):
            marginal_plan(10, [0, 1], perm=[0] * 10, rdm=rdm)  # no permutation
        assert marginal_plan(10, [], rdm=rdm)["k_lo"] == 0
    with pytest.raises(ValueError):
        marginal_plan(30, list(range(21)))
    with pytest.raises(ValueError):
        marginal_plan(30, list(range(7)), rdm=True)
    assert marginal_plan(30, list(range(20)))["launches"] == 2
    assert marginal_plan(30, list(range(6)), rdm=True)["launches"] == 2


def test_plan_splits_low_and_high_under_random_perms(qsim):
    from qsim_amd.plan import marginal_plan
    rng = np.random.default_rng(3)
    for n in (5, 12, 14, 20, 30):
        for _ in range(20):
            perm = [int(p) for p in rng.permutation(n)]
            k = int(rng.integers(0, min(n, 20) + 1))
            qs = [int(q) for q in rng.choice(n, size=k, replace=False)]
            info = marginal_plan(n, qs, perm)
            c = min(n, RUN_BITS)
            assert info["k_lo"] == sum(perm[q] < c for q in qs)
            assert info["k_hi"] == sum(perm[q] >= c for q in qs)
            assert info["k_lo"] + info["k_hi"] == k
            assert info["work_groups"] == info["slices"] << info["k_hi"]
            assert info["scratch_bytes"] == info["slices"] * 8 << k
            if k <= 6:
                r = marginal_plan(n, qs, perm, rdm=True)
                assert r["k_lo"] + r["k_hi"] == k and r["scratch_bytes"] == r["work_groups"] * 16 * 4 ** k


def _selections(n, k):
    lowest = list(range(k))
    highest = list(range(n - k, n))
    lo = RUN_BITS - k // 2
    straddle = list(range(lo, lo + k))
    return [lowest, highest, straddle]


def test_scratch_cap_and_work_groups_n30(qsim):
    from qsim_amd.plan import marginal_plan
    n = 30
    rng = np.random.default_rng(8)
    perms = [None] + [[int(p) for p in rng.permutation(n)] for _ in range(5)]
    for k in range(21):
        for qs in _selections(n, k):
            for perm in perms:
                info = marginal_plan(n, qs, perm)
                assert info["scratch_bytes"] <= 64 * MIB, (k, qs, perm, info)
                assert info["work_groups"] >= 1024, (k, qs, perm, info)  # 2^30 / 2^12 runs
    for qs in _selections(n, 6):
        for perm in perms:
            info = marginal_plan(n, qs, perm, rdm=True)
            assert info["scratch_bytes"] <= 64 * MIB and info["work_groups"] >= 1


def test_work_groups_whenever_the_state_has_the_runs(qsim):
    from qsim_amd.plan import marginal_plan
    rng = np.random.default_rng(9)
    for n in range(2, 31):
        c = min(n, RUN_BITS)
        runs = (1 << n) >> c
        for k in {0, 1, min(n, 7), min(n, 20)}:
            for _ in range(4):
                qs = [int(q) for q in rng.choice(n, size=k, replace=False)]
                info = marginal_plan(n, qs)
                assert 1 <= info["work_groups"] <= runs
                if runs >= 1024:
                    assert info["work_groups"] >= 1024, (n, qs, info)
                assert info["scratch_bytes"] <= 64 * MIB


def _random_density_matrix(rng, d):
    a = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    rho = a @ a.conj().T
    rho /= np.trace(rho).real
    return 0.7 * rho + 0.3 * np.eye(d) / d  # spectrum bounded away from 0


@pytest.mark.parametrize("d", [2, 8, 64])
def test_host_entropy_matches_eigvalsh(qsim, d):
    from qsim_amd.plan import hermitian_entropy
    rng = np.random.default_rng(d)
    for _ in range(3):
        rho = _random_density_matrix(rng, d)
        assert np.linalg.eigvalsh(rho).min() > 1e-6
        assert abs(hermitian_entropy(rho) - mc.entropy_np(rho)) <= mc.ENT_ATOL
        assert abs(hermitian_entropy(rho, renyi2=True) - mc.entropy_np(rho, renyi2=True)) <= mc.ENT_ATOL
    assert abs(hermitian_entropy(np.eye(d) / d) - np.log2(d)) <= mc.ENT_ATOL
    pure = np.zeros((d, d), complex)
    pure[d - 1, d - 1] = 1.0
    assert abs(hermitian_entropy(pure)) <= mc.ENT_ATOL


def test_numpy_reference_conventions():
    """The helper itself: bit j of an output index is qubits[j], qubit q is index bit q."""
    n = 4
    psi = np.zeros(1 << n, complex)
    psi[0b0110] = 1.0  # qubits 1 and 2 set
    assert mc.marginal_np(psi, [1])[1] == 1.0 and mc.marginal_np(psi, [0])[0] == 1.0
    assert mc.marginal_np(psi, [0, 1])[0b10] == 1.0 and mc.marginal_np(psi, [1, 0])[0b01] == 1.0
    assert mc.rdm_np(psi, [3, 2, 1])[0b110, 0b110] == 1.0
    rng = np.random.default_rng(0)
    psi = rng.normal(size=16) + 1j * rng.normal(size=16)
    assert np.allclose(mc.rdm_np(psi, [2, 0]).diagonal().real, mc.marginal_np(psi, [2, 0]))
