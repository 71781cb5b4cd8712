"""Dense numpy restatement of Pauli-string rotations, Trotter sequences and their adjoint-method
gradient (helper of tests/test_pauli_rotation_*.py; no reference counterpart).

A rotation is a tuple (x_mask, z_mask, theta) and means exp(-i theta/2 P) = cos(theta/2) -
i sin(theta/2) P with the string convention of gradient_cases.apply_pauli; a sequence is a list of
them in application order.  With phi_k = U_k ... U_1 psi0 and lambda_k = U_{k+1}^† ... U_N^† H phi_N,
    dE/dtheta_k = Im <lambda_k| P_k |phi_k>.
"""
import numpy as np

import gradient_cases as gc


def rotate(psi, x, z, theta):
    return np.cos(theta / 2) * psi - 1j * np.sin(theta / 2) * gc.apply_pauli(psi, x, z)


def run_sequence(psi0, seq):
    psi = np.array(psi0, dtype=np.complex128)
    for x, z, th in seq:
        psi = rotate(psi, x, z, th)
    return psi


def trotter_sequence(terms, time, steps, order):
    """The Trotter product for exp(-i H time), H = terms (x, z, c), written slice by slice: order 1
    is the terms in order at angle 2 c dt; order 2 is every term but the last at angle c dt, the
    last at 2 c dt, the others again backwards, with the two term-0 rotations that meet between
    steps merged into one."""
    dt = time / steps
    if order == 1:
        return [(x, z, 2 * c * dt) for _ in range(steps) for x, z, c in terms]
    assert order == 2
    if len(terms) < 2:
        return [(x, z, 2 * c * dt) for _ in range(steps) for x, z, c in terms]
    seq = []
    for _ in range(steps):
        step = [(x, z, c * dt) for x, z, c in terms[:-1]]
        x, z, c = terms[-1]
        step = step + [(x, z, 2 * c * dt)] + step[::-1]
        if seq and seq[-1][:2] == step[0][:2]:
            x, z, th = seq.pop()
            step[0] = (x, z, th + step[0][2])
        seq += step
    return seq


def sequence_gradient(psi0, seq, terms):
    """(value, gradient per rotation) by the backward sweep, in complex128."""
    phi = run_sequence(psi0, seq)
    lam = gc.apply_h(phi, terms)
    value = float(np.vdot(phi, lam).real)
    grad = np.zeros(len(seq))
    for k in range(len(seq) - 1, -1, -1):
        x, z, th = seq[k]
        grad[k] = np.vdot(lam, gc.apply_pauli(phi, x, z)).imag
        if k > 0:
            phi = rotate(phi, x, z, -th)
            lam = rotate(lam, x, z, -th)
    return value, grad


def shift_gradient(psi0, seq, terms):
    """The exact two-point rule of a Pauli rotation: dE/dtheta = (E(theta + pi/2) - E(theta - pi/2)) / 2."""
    grad = np.zeros(len(seq))
    for k, (x, z, th) in enumerate(seq):
        ep = gc.expectation(run_sequence(psi0, seq[:k] + [(x, z, th + np.pi / 2)] + seq[k + 1:]), terms)
        em = gc.expectation(run_sequence(psi0, seq[:k] + [(x, z, th - np.pi / 2)] + seq[k + 1:]), terms)
        grad[k] = (ep - em) / 2
    return grad


def dense_h(n, terms):
    """The 2^n x 2^n matrix of H (column i = H e_i); small n only."""
    dim = 1 << n
    m = np.zeros((dim, dim), dtype=np.complex128)
    for i in range(dim):
        e = np.zeros(dim, dtype=np.complex128)
        e[i] = 1.0
        m[:, i] = gc.apply_h(e, terms)
    return m


def exact_evolve(psi0, n, terms, time):
    """exp(-i H time) psi0 through the eigendecomposition of the dense H."""
    w, v = np.linalg.eigh(dense_h(n, terms))
    return v @ (np.exp(-1j * w * time) * (v.conj().T @ np.asarray(psi0, dtype=np.complex128)))


def random_rotations(rng, n, count, p_diag=0.3):
    """count rotations: random masks (x = 0 with probability p_diag), angles in (-pi, pi)."""
    out = []
    for _ in range(count):
        x = 0 if rng.random() < p_diag else int(rng.integers(1, 1 << n))
        out.append((x, int(rng.integers(0, 1 << n)), float(rng.uniform(-np.pi, np.pi))))
    return out


def tfim_terms(n, j=1.0, g=0.7):
    """Transverse-field Ising chain: -j sum Z_k Z_k+1 - g sum X_k."""
    return [(0, 3 << k, -j) for k in range(n - 1)] + [(1 << k, 0, -g) for k in range(n)]


def max_component_diff(a, b):
    d = np.asarray(a) - np.asarray(b)
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
