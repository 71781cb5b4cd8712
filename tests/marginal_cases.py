"""Dense numpy restatement of marginal probabilities, reduced density matrices and their entropies,
and the shared case lists (helper of tests/test_marginal_*.py; no reference counterpart).

Convention: qubit q is index bit q of an amplitude index (the gates' and PauliSum's); bit j of an
output index is qubits[j].
"""
import itertools

import numpy as np

ATOL = 1e-12      # every bin and matrix component: only the summation order differs
ENT_ATOL = 1e-10  # entropies, on spectra with no eigenvalue in (0, 1e-6)


def _split(psi, qubits):
    """psi as a matrix M[a, b]: a over `qubits` (bit j of a = qubits[j]), b over the others."""
    psi = np.asarray(psi, dtype=np.complex128)
    n = psi.size.bit_length() - 1
    qubits = list(qubits)
    k = len(qubits)
    t = psi.reshape((2,) * n)  # axis i is index bit n-1-i
    rest = [q for q in range(n) if q not in qubits]
    # row index a: its most significant bit is qubits[k-1]; columns: any fixed order of the rest
    axes = [n - 1 - q for q in reversed(qubits)] + [n - 1 - q for q in reversed(rest)]
    return np.transpose(t, axes).reshape(1 << k, 1 << (n - k))


def marginal_np(psi, qubits):
    m = _split(psi, qubits)
    return np.sum(m.real ** 2 + m.imag ** 2, axis=1)


def rdm_np(psi, qubits):
    m = _split(psi, qubits)
    return m @ m.conj().T


def entropy_np(rho, renyi2=False):
    if renyi2:
        return float(-np.log2(np.sum(np.abs(rho) ** 2)))
    ev = np.linalg.eigvalsh(rho)
    ev = ev[ev >= 1e-300]
    return float(-np.sum(ev * np.log2(ev)))


def spectrum_is_safe(rho):
    """No eigenvalue in (0, 1e-6): -l log2 l has unbounded slope at 0.  Eigenvalues within
    rounding of 0 (|l| < 1e-13, a rank-deficient rho_A) count as exact zeros."""
    ev = np.linalg.eigvalsh(rho)
    return not np.any((ev > 1e-13) & (ev < 1e-6))


def all_subsets(n, kmax=None):
    kmax = n if kmax is None else kmax
    return [list(c) for k in range(kmax + 1) for c in itertools.combinations(range(n), k)]


# Selections by the class of physical position they fall in under the identity layout (a run is
# min(n, 12) bits: 0-5 lane bits, 6-7 wave bits, 8-11 per-thread bits; above: run-choosing bits).
MARGINAL_CLASSES = {
    10: {
        "lane": [0, 2, 5],
        "wave": [6, 7],
        "thread": [8, 9],
        "one_of_each": [3, 6, 9],
        "all_run_bits": list(range(10)),
        "shuffled": [9, 0, 6, 4],
        "one_lane": [1],
        "one_wave": [7],
        "none": [],
    },
    14: {
        "lane": [0, 2, 5],
        "wave": [6, 7],
        "thread": [8, 11, 9],
        "above": [12, 13],
        "one_above": [13],
        "one_of_each": [3, 6, 9, 12],
        "all_run_bits": list(range(12)),
        "every_amplitude": list(range(14)),
        "shuffled": [13, 0, 7, 10, 4],
        "one_lane": [4],
        "none": [],
    },
}
RDM_CLASSES = {
    10: {"contiguous_columns": [0, 1, 2, 3, 4, 5], "mixed": [0, 3, 7, 9], "high": [8, 9], "shuffled": [7, 1, 9]},
    14: {"contiguous_columns": [0, 1, 2, 3, 4, 5], "high": [8, 9, 10, 11, 12, 13], "mixed": [0, 3, 7, 9, 12, 13],
         "shuffled": [13, 2, 8], "one_above": [12], "k5": [1, 4, 6, 10, 13], "k4": [5, 6, 11, 12]},
}

# The 12-qubit random circuit whose 6-qubit entropy the C++ harness recomputes with its Jacobi sweep
CPP_ENTROPY_CASE = {"n": 12, "depth": 120, "seed": 31, "qubits": [0, 2, 5, 7, 8, 11]}
