"""Checker and observables shared by the density-matrix expectation tests
(tests/test_dm_expectation_cpu.py, tests/test_dm_expectation_gpu.py).

dense_expectation(rho, H) = Re Tr(rho H) with H built from Kronecker products of the 2x2 Paulis
(qubit q is index bit q, so the LAST Kronecker factor is qubit 0) — no x / z mask arithmetic, so it
shares nothing with the formula csrc/hip/dm_expect.hip evaluates."""
import numpy as np

PAULI = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
         "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def letters_of(n, x, z):
    """The Pauli letter on each qubit of a term with masks (x, z)."""
    return ["IZXY"[(x >> q & 1) * 2 + (z >> q & 1)] for q in range(n)]


def dense_string(letters):
    """The 2^n x 2^n matrix of a string; letters[q]: the factor on qubit q."""
    m = np.array([[1.0 + 0j]])
    for letter in letters:  # each new qubit is the next HIGHER index bit: it goes on the left
        m = np.kron(PAULI[letter], m)
    return m


def dense_expectation(rho, observable):
    """Re Tr(rho H) for a dense rho and a qsim_amd.PauliSum."""
    n = observable.getNumQubits()
    rho = np.asarray(rho).reshape(1 << n, 1 << n)
    total = 0j
    for x, z, c in observable.terms():
        total += c * np.sum(rho * dense_string(letters_of(n, x, z)).T)  # Tr(rho P) = sum_ij rho_ij P_ji
    return float(total.real)


def add_all(dst, src):
    """Append every term of the PauliSum src to dst (same qubit count)."""
    n = src.getNumQubits()
    for x, z, c in src.terms():
        dst.add(c, {k: letter for k, letter in enumerate(letters_of(n, x, z)) if letter != "I"})
    return dst


def abs_sum(observable):
    return float(sum(abs(c) for _, _, c in observable.terms()))


def tfim(q, n, j=1.0, h=0.7):
    """Open-chain transverse-field Ising: -j sum Z_k Z_k+1 - h sum X_k (n - 1 + n terms)."""
    obs = q.PauliSum(n)
    for k in range(n - 1):
        obs.add(-j, {k: "Z", k + 1: "Z"})
    for k in range(n):
        obs.add(-h, {k: "X"})
    return obs


def heisenberg(q, n):
    """Open-chain Heisenberg: sum over bonds of XX + YY + ZZ with bond-dependent couplings."""
    obs = q.PauliSum(n)
    for k in range(n - 1):
        for letter, c in (("X", 1.0), ("Y", 0.8), ("Z", -0.6)):
            obs.add(c * (1 + 0.1 * k), {k: letter, k + 1: letter})
    return obs


def random_strings(q, n, count, max_weight, seed):
    """`count` random strings of weight 1..max_weight, each with at least one Y."""
    rng = np.random.default_rng(seed)
    obs = q.PauliSum(n)
    for _ in range(count):
        w = int(rng.integers(1, max_weight + 1))
        qubits = [int(v) for v in rng.choice(n, w, replace=False)]
        letters = [str(v) for v in rng.choice(list("XYZ"), w)]
        letters[int(rng.integers(0, w))] = "Y"
        obs.add(float(rng.uniform(-1, 1)), dict(zip(qubits, letters)))
    return obs


def z_only_strings(q, n, count, seed):
    """`count` DISTINCT Z-only strings (non-zero z masks) with random coefficients."""
    rng = np.random.default_rng(seed)
    masks = rng.choice(np.arange(1, 1 << n), count, replace=False)
    obs = q.PauliSum(n)
    for z in masks:
        obs.add(float(rng.uniform(-1, 1)), {k: "Z" for k in range(n) if int(z) >> k & 1})
    return obs
