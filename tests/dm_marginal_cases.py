"""Dense checker of the density-matrix subset readers and the fidelity (helper of
tests/test_dm_marginal_*.py; no reference counterpart).

rho is reshaped to 2n axes of size 2 and reduced with einsum: no address or mask arithmetic, so it
shares nothing with the generators csrc/hip/dm_marginal.hip evaluates.  Convention: qubit q is index
bit q of the row index i and of the column index j of rho[i][j]; bit j of an output index is
qubits[j]; rho_A[a][a'] has a on the rows.
"""
import numpy as np

U = 2.0 ** -52


def _axes(rho):
    rho = np.asarray(rho)
    n = rho.shape[0].bit_length() - 1
    assert rho.shape == (1 << n, 1 << n)
    # axis x of the row half is row bit n - 1 - x; the column half follows
    row = {q: n - 1 - q for q in range(n)}
    col = {q: 2 * n - 1 - q for q in range(n)}
    return n, rho.reshape((2,) * (2 * n)), row, col


def dm_rdm_np(rho, qubits):
    """rho_A[a][a'] = sum_b rho[(a, b)][(a', b)]: the other qubits' row and column axes share a
    label (a trace), the listed ones keep theirs."""
    n, t, row, col = _axes(rho)
    qubits = list(qubits)
    k = len(qubits)
    labels = [0] * (2 * n)
    for q in range(n):
        labels[row[q]] = q
        labels[col[q]] = q + n if q in qubits else q
    out = [q for q in reversed(qubits)] + [q + n for q in reversed(qubits)]  # most significant bit first
    return np.einsum(t, labels, out).reshape(1 << k, 1 << k)


def dm_marginal_np(rho, qubits):
    """out[m] = sum_b Re rho[(m, b)][(m, b)]: every qubit's row and column axes share a label (the
    diagonal), the listed ones are kept."""
    n, t, row, col = _axes(rho)
    qubits = list(qubits)
    labels = [0] * (2 * n)
    for q in range(n):
        labels[row[q]] = labels[col[q]] = q
    return np.einsum(t, labels, [q for q in reversed(qubits)]).reshape(1 << len(qubits)).real.copy()


def fidelity_np(rho, psi):
    psi = np.asarray(psi, dtype=np.complex128)
    return float(np.vdot(psi, np.asarray(rho) @ psi).real)


def purity_np(rho_a):
    return float(np.sum(np.abs(rho_a) ** 2))


# Tolerance A (the reduction alone): a fixed-order sum of T terms of weight W = sum |terms| stays
# within 4 T 2^-52 W of the exact sum — the sequential-sum bound the expectation tests use.
def tol_a_rdm(rho, qubits):
    """Per entry (each component): T = 2^(n-k) elements, W = sum_b |rho[(a, b)][(a', b)]|."""
    n = np.asarray(rho).shape[0].bit_length() - 1
    return 4.0 * (1 << (n - len(list(qubits)))) * U * dm_rdm_np(np.abs(rho), qubits).real


def tol_a_marginal(rho, qubits):
    n = np.asarray(rho).shape[0].bit_length() - 1
    return 4.0 * (1 << (n - len(list(qubits)))) * U * dm_marginal_np(np.abs(np.asarray(rho).real), qubits)


def tol_a_fidelity(rho, psi):
    """T = 4^n products, W = sum_ij |psi_i| |rho_ij| |psi_j|."""
    a = np.abs(np.asarray(psi, dtype=np.complex128))
    return 4.0 * np.asarray(rho).size * U * float(a @ (np.abs(rho) @ a))


# Tolerance B (the whole path, against the oracle's rho): the project's 1e-12 per component of rho
# times the number of components summed; for the fidelity times (sum |psi_i|)^2.
def tol_b_subset(n, qubits):
    return 1e-12 * (1 << (n - len(list(qubits))))


def tol_b_fidelity(psi):
    return 1e-12 * float(np.sum(np.abs(psi))) ** 2


def random_matrix(n, seed):
    """A random complex matrix that is visibly NOT Hermitian."""
    rng = np.random.default_rng(seed)
    d = 1 << n
    m = rng.uniform(-1, 1, (d, d)) + 1j * rng.uniform(-1, 1, (d, d))
    return m


def random_psi(n, seed):
    rng = np.random.default_rng(seed)
    d = 1 << n
    return rng.uniform(-1, 1, d) + 1j * rng.uniform(-1, 1, d)


def check_rdm(got, rho, qubits, tol, what):
    want = dm_rdm_np(rho, qubits)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    print(f"{what} matrix {list(qubits)}: max err {err.max():.3e} min tol {np.min(tol):.3e}")
    assert got.shape == want.shape and np.all(err <= tol), what


def check_marginal(got, rho, qubits, tol, what):
    want = dm_marginal_np(rho, qubits)
    err = np.abs(got - want)
    print(f"{what} marginal {list(qubits)}: max err {err.max():.3e} min tol {np.min(tol):.3e}")
    assert got.shape == want.shape and np.all(err <= tol), what


def check_fidelity(got, rho, psi, tol, what):
    want = fidelity_np(rho, psi)
    print(f"{what} fidelity: got {got!r} want {want!r} |diff| {abs(got - want):.3e} tol {tol:.3e}")
    assert abs(got - want) <= tol, what
