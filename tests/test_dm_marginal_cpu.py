"""Host-only checks of the density-matrix subset readers' lowering (qsim_dm_marginal_plan,
csrc/hip/dm_marginal.hip) and of the dense checker tests/dm_marginal_cases.py; no GPU."""
import numpy as np
import pytest

import dm_marginal_cases as dc


def test_checker_orientation_on_a_hand_written_matrix():
    """2 qubits, non-Hermitian: rho[i][j] = 10 i + j + 0.5i (i - j), so every entry names its row and
    its column.  a is the ROW index, a' the COLUMN index, qubit 0 the LOW bit."""
    m = np.array([[10 * i + j + 0.5j * (i - j) for j in range(4)] for i in range(4)])
    assert np.abs(m - m.conj().T).max() > 0.1
    # tracing out qubit 1 (the high bit): rho_A[a][a'] = m[a][a'] + m[a + 2][a' + 2]
    want0 = np.array([[m[a, b] + m[a + 2, b + 2] for b in range(2)] for a in range(2)])
    np.testing.assert_array_equal(dc.dm_rdm_np(m, [0]), want0)
    assert dc.dm_rdm_np(m, [0])[0, 1] == m[0, 1] + m[2, 3]  # row 0, column 1: not its transpose
    # tracing out qubit 0 (the low bit): rho_A[a][a'] = m[2a][2a'] + m[2a + 1][2a' + 1]
    want1 = np.array([[m[2 * a, 2 * b] + m[2 * a + 1, 2 * b + 1] for b in range(2)] for a in range(2)])
    np.testing.assert_array_equal(dc.dm_rdm_np(m, [1]), want1)
    np.testing.assert_array_equal(dc.dm_rdm_np(m, [0, 1]), m)
    swapped = m.reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4)  # bit 0 of an index = qubit 1
    np.testing.assert_array_equal(dc.dm_rdm_np(m, [1, 0]), swapped)
    assert dc.dm_rdm_np(m, []).shape == (1, 1) and dc.dm_rdm_np(m, [])[0, 0] == np.trace(m)
    d = np.diag(m).real
    np.testing.assert_array_equal(dc.dm_marginal_np(m, [0]), [d[0] + d[2], d[1] + d[3]])
    np.testing.assert_array_equal(dc.dm_marginal_np(m, [1]), [d[0] + d[1], d[2] + d[3]])
    np.testing.assert_array_equal(dc.dm_marginal_np(m, [0, 1]), d)
    np.testing.assert_array_equal(dc.dm_marginal_np(m, [1, 0]), d[[0, 2, 1, 3]])
    np.testing.assert_array_equal(dc.dm_marginal_np(m, []), [d.sum()])
    psi = np.array([1, 2j, -1, 0.5])
    assert dc.fidelity_np(m, psi) == pytest.approx(sum((np.conj(psi[i]) * m[i, j] * psi[j]).real
                                                       for i in range(4) for j in range(4)), abs=1e-12)
    e2 = np.zeros(4)
    e2[2] = 1
    assert dc.fidelity_np(m, e2) == d[2]


def test_plan_counts(qsim):
    """Elements read: 2^n for the marginal, 2^(n+k) for the matrix; two launches (the gather and the
    fold); scratch = slices x outputs; the readers never read more than 2^21 elements."""
    from qsim_amd.plan import dm_marginal_plan
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 8, 12, 15):
        for trial in range(6):
            perm = None if trial == 0 else [int(p) for p in rng.permutation(2 * n)]
            for k in sorted({0, 1, min(n, 3), min(n, 6), n}):
                qs = [int(q) for q in rng.choice(n, size=k, replace=False)]
                info = dm_marginal_plan(n, qs, perm)
                assert info["elements"] == 1 << n and info["launches"] == 2
                assert len(info["out_gen"]) == k and len(info["sum_gen"]) == n - k
                assert info["scratch_bytes"] == info["slices"] * 8 << k
                assert 1 <= info["work_groups"] <= max(1, (1 << n) >> info["thread_bits"])
                assert info["thread_bits"] == min(n, 8)
                if k <= 6:
                    info = dm_marginal_plan(n, qs, perm, rdm=True)
                    assert info["elements"] == 1 << (n + k) <= 1 << 21 and info["launches"] == 2
                    assert len(info["out_gen"]) == 2 * k and len(info["sum_gen"]) == n - k
                    assert info["scratch_bytes"] == info["slices"] * 16 << (2 * k)
                    assert info["scratch_bytes"] <= 16 << 20
                    assert info["thread_bits"] == min(n + k, 8)
                    assert info["work_groups"] * (1 << info["thread_bits"]) <= info["elements"]


def test_generators_under_the_identity_layout(qsim):
    from qsim_amd.plan import dm_marginal_plan
    n = 5
    info = dm_marginal_plan(n, [3, 0], rdm=True)
    # o = a << 2 | a': column positions of qubits 3, 0, then their row positions (q + n)
    assert info["out_gen"] == [1 << 3, 1 << 0, 1 << 8, 1 << 5]
    assert info["sum_gen"] == [1 << 1 | 1 << 6, 1 << 2 | 1 << 7, 1 << 4 | 1 << 9]
    info = dm_marginal_plan(n, [3, 0])
    assert info["out_gen"] == [1 << 3 | 1 << 8, 1 << 0 | 1 << 5]


def _host_replay(buf, out_gen, sum_gen):
    """out[o] = sum_b buf[G_out(o) | G_sum(b)], G(v) the OR of the generators at v's set bits."""
    def addr(v, gens):
        a = 0
        for i, g in enumerate(gens):
            if v >> i & 1:
                a |= g
        return a
    sums = np.array([addr(b, sum_gen) for b in range(1 << len(sum_gen))], dtype=np.int64)
    return np.array([buf[addr(o, out_gen) | sums].sum() for o in range(1 << len(out_gen))])


def _scatter_under_perm(m, perm):
    """The buffer a state under the index-bit layout perm (logical bit -> physical position) holds
    for the matrix m: element i * 2^n + j lies where every set logical bit is moved to perm[bit]."""
    flat = np.asarray(m).reshape(-1)
    idx = np.arange(flat.size)
    phys = np.zeros_like(idx)
    for b, p in enumerate(perm):
        phys |= (idx >> b & 1) << p
    buf = np.empty_like(flat)
    buf[phys] = flat
    return buf


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_host_replay_of_the_generators(qsim, n):
    """A random non-Hermitian matrix scattered into a buffer under random 2n-bit layouts; the sum the
    kernels evaluate, replayed in numpy from the returned generators, is the checker's partial trace
    and marginal for subsets in scrambled order."""
    from qsim_amd.plan import dm_marginal_plan
    rng = np.random.default_rng(40 + n)
    m = dc.random_matrix(n, 60 + n)
    assert np.abs(m - m.conj().T).max() > 0.1
    subsets = [[], [0], [n - 1], list(range(n)), list(range(n))[::-1]]
    for _ in range(5):
        k = int(rng.integers(1, n + 1))
        subsets.append([int(q) for q in rng.permutation(n)[:k]])
    for trial in range(4):
        perm = list(range(2 * n)) if trial == 0 else [int(p) for p in rng.permutation(2 * n)]
        buf = _scatter_under_perm(m, perm)
        for qs in subsets:
            info = dm_marginal_plan(n, qs, perm, rdm=True)
            got = _host_replay(buf, info["out_gen"], info["sum_gen"]).reshape(1 << len(qs), 1 << len(qs))
            np.testing.assert_allclose(got, dc.dm_rdm_np(m, qs), atol=1e-13 * (1 << n), rtol=0)
            info = dm_marginal_plan(n, qs, perm)
            got = _host_replay(buf, info["out_gen"], info["sum_gen"]).real
            np.testing.assert_allclose(got, dc.dm_marginal_np(m, qs), atol=1e-13 * (1 << n), rtol=0)
    # the identity layout through perm=None is the identity list
    for qs in subsets[:5]:
        assert dm_marginal_plan(n, qs, None, rdm=True) == dm_marginal_plan(n, qs, list(range(2 * n)), rdm=True)


def test_argument_errors(qsim):
    from qsim_amd.plan import dm_marginal_plan, marginal_plan
    n = 8
    for rdm in (False, True):
        with pytest.raises(ValueError) as dup:
            dm_marginal_plan(n, [1, 4, 1], rdm=rdm)
        with pytest.raises(ValueError) as sv_dup:
            marginal_plan(n, [1, 4, 1], rdm=rdm)
        assert str(dup.value) == str(sv_dup.value)
        for bad in ([0, n], [-1]):
            with pytest.raises(IndexError) as rng_err:
                dm_marginal_plan(n, bad, rdm=rdm)
            with pytest.raises(IndexError) as sv_rng:
                marginal_plan(n, bad, rdm=rdm)
            assert str(rng_err.value) == str(sv_rng.value)
        with pytest.raises(ValueError):
            dm_marginal_plan(n, [0, 1], perm=[0] * (2 * n), rdm=rdm)  # no permutation
        with pytest.raises(ValueError):
            dm_marginal_plan(n, [0, 1], perm=list(range(n)), rdm=rdm)  # n entries, not 2n
        with pytest.raises(ValueError):
            dm_marginal_plan(0, [], rdm=rdm)
        with pytest.raises(ValueError):
            dm_marginal_plan(16, [], rdm=rdm)
    with pytest.raises(ValueError) as many:
        dm_marginal_plan(n, list(range(7)), rdm=True)  # k > 6 for the matrix
    with pytest.raises(ValueError) as sv_many:
        marginal_plan(n, list(range(7)), rdm=True)
    assert str(many.value) == str(sv_many.value)
    assert dm_marginal_plan(n, list(range(8)))["elements"] == 256  # k == n is fine for the marginal
    with pytest.raises(ValueError):
        dm_marginal_plan(3, [0, 1, 2, 0])  # k > n (and so a duplicate)
    with pytest.raises(ValueError) as over:
        dm_marginal_plan(3, [0, 1, 2, 3], rdm=True)  # k > n
    with pytest.raises(ValueError) as sv_over:
        marginal_plan(3, [0, 1, 2, 3], rdm=True)
    assert str(over.value) == str(sv_over.value)


def test_python_layer_has_the_readers(qsim):
    for cls in (qsim.DensityMatrix, qsim.DensityMatrixSimulator):
        for name in ("marginalProbabilities", "reducedDensityMatrix", "subsystemPurity", "subsystemEntropy",
                     "fidelity"):
            assert callable(getattr(cls, name))
        assert not hasattr(cls, "entanglementEntropy")


def test_abi_version_is_still_2(qsim):
    from qsim_amd import _lib
    assert _lib.hip.qsim_abi_version() == 2
    for name in ("qsim_dm_marginal_probabilities", "qsim_dm_reduced_density_matrix", "qsim_dm_fidelity",
                 "qsim_dm_marginal_plan"):
        assert hasattr(_lib.hip, name)
