"""Dense numpy restatement of the adjoint-method gradient (helper of tests/test_gradient_*.py; no
reference counterpart: the reference has no observable API).

Gate conventions are those of oracle/cpu_simulator.hpp: index bit q == qubit q, Rx / Ry / Rz =
exp(-i theta/2 P), CRY / CRZ that rotation on the control == 1 subspace.  A gate is a tuple
(type, qubits, parameter) with the GateType numbering of include/qsim_hip.h.  Gates act on index
pairs of the flat state (no 2^n x 2^n matrix), so n = 21 stays cheap.

With phi_k = U_k ... U_1 psi0 and lambda_k = U_{k+1}^† ... U_N^† H phi_N,
    dE/dtheta_k = Im <lambda_k| G_k |phi_k>,
G_k = P_target for Rx / Ry / Rz and |1><1|_control (x) P_target for CRY / CRZ (dU/dtheta = -(i/2) G U).
"""
import functools

import numpy as np

X, Y, Z, H, S, T, SDAG, TDAG, RX, RY, RZ, CNOT, CZ, CRY, CRZ, SWAP, TOFFOLI = range(17)
PARAMETRIC = (RX, RY, RZ, CRY, CRZ)
ARITY = {t: (1 if t <= RZ else 2 if t <= SWAP else 3) for t in range(17)}
_R = 0.7071067811865476
_PAULI = {
    "X": np.array([[0, 1], [1, 0]], dtype=np.complex128),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
    "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128),
}


def matrix_1q(t, th=0.0):
    """The 2x2 on the target of gate type t (controls apart)."""
    c, s = np.cos(th / 2), np.sin(th / 2)
    m = {
        X: _PAULI["X"], CNOT: _PAULI["X"], TOFFOLI: _PAULI["X"],
        Y: _PAULI["Y"],
        Z: _PAULI["Z"], CZ: _PAULI["Z"],
        H: np.array([[_R, _R], [_R, -_R]]),
        S: np.diag([1, 1j]), SDAG: np.diag([1, -1j]),
        T: np.diag([1, _R + 1j * _R]), TDAG: np.diag([1, _R - 1j * _R]),
        RX: np.array([[c, -1j * s], [-1j * s, c]]),
        RY: np.array([[c, -s], [s, c]]), CRY: np.array([[c, -s], [s, c]]),
        RZ: np.diag([c - 1j * s, c + 1j * s]), CRZ: np.diag([c - 1j * s, c + 1j * s]),
    }[t]
    return np.asarray(m, dtype=np.complex128)


@functools.lru_cache(maxsize=1024)
def _pairs(n, t, cmask):
    idx = np.arange(1 << n, dtype=np.int64)
    i0 = idx[((idx & cmask) == cmask) & ((idx >> t & 1) == 0)]
    return i0, i0 | (1 << t)


def apply_2x2(psi, n, m, t, cmask=0):
    """m on qubit t of the subspace where every qubit of cmask reads 1; returns a new array."""
    i0, i1 = _pairs(n, t, cmask)
    out = psi.copy()
    a0, a1 = psi[i0], psi[i1]
    out[i0] = m[0, 0] * a0 + m[0, 1] * a1
    out[i1] = m[1, 0] * a0 + m[1, 1] * a1
    return out


def apply_gate(psi, n, gate):
    t, q, th = gate
    if t == SWAP:
        idx = np.arange(1 << n, dtype=np.int64)
        a, b = q
        src = idx[((idx >> a & 1) == 1) & ((idx >> b & 1) == 0)]
        dst = src ^ (1 << a) ^ (1 << b)
        out = psi.copy()
        out[src], out[dst] = psi[dst], psi[src]
        return out
    cmask = sum(1 << c for c in q[:-1])
    return apply_2x2(psi, n, matrix_1q(t, th), q[-1], cmask)


def run(psi0, n, gates):
    psi = np.array(psi0, dtype=np.complex128)
    for g in gates:
        psi = apply_gate(psi, n, g)
    return psi


def inverse(gate):
    t, q, th = gate
    swap = {S: SDAG, SDAG: S, T: TDAG, TDAG: T}
    if t in swap:
        return (swap[t], q, th)
    if t in PARAMETRIC:
        return (t, q, -th)
    return gate


def apply_generator(psi, n, gate):
    t, q, _ = gate
    p = _PAULI[{RX: "X", RY: "Y", RZ: "Z", CRY: "Y", CRZ: "Z"}[t]]
    if t in (CRY, CRZ):
        i0, i1 = _pairs(n, q[1], 1 << q[0])
        out = np.zeros_like(psi)  # the projector kills the control == 0 half
        a0, a1 = psi[i0], psi[i1]
        out[i0] = p[0, 0] * a0 + p[0, 1] * a1
        out[i1] = p[1, 0] * a0 + p[1, 1] * a1
        return out
    return apply_2x2(psi, n, p, q[0])


def _parity(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> s
    return v & 1


def apply_pauli(psi, x, z):
    """P psi for the string with masks (x, z): (P psi)[i] = i^nY (-1)^popcount((i^x) & z) psi[i^x]."""
    idx = np.arange(psi.size, dtype=np.int64)
    j = idx ^ x
    ny = bin(x & z).count("1")
    return (1j ** ny) * (1 - 2 * _parity(j & z)) * psi[j]


def apply_h(psi, terms):
    """H psi for terms (x_mask, z_mask, coeff)."""
    out = np.zeros_like(psi)
    for x, z, c in terms:
        out += c * apply_pauli(psi, x, z)
    return out


def expectation(psi, terms):
    return float(np.vdot(psi, apply_h(psi, terms)).real)


def adjoint_gradient(psi0, n, gates, terms, after=None):
    """(value, gradient per gate) by the backward sweep, in complex128.  after = (k0, psi): psi is
    the state after gates[:k0] (a forward prefix computed once for many circuits that share it).
    The sweep ends at the first parameterised gate: nothing before it has a gradient."""
    k0, psi = (0, psi0) if after is None else after
    phi = run(psi, n, gates[k0:])
    lam = apply_h(phi, terms)
    value = float(np.vdot(phi, lam).real)
    grad = np.zeros(len(gates))
    first = min((k for k, g in enumerate(gates) if g[0] in PARAMETRIC), default=len(gates))
    for k in range(len(gates) - 1, first - 1, -1):
        g = gates[k]
        if g[0] in PARAMETRIC:
            grad[k] = np.vdot(lam, apply_generator(phi, n, g)).imag
        if k > first:
            inv = inverse(g)
            phi = apply_gate(phi, n, inv)
            lam = apply_gate(lam, n, inv)
    return value, grad


def shift_gradient(psi0, n, gates, terms, h=1e-4):
    """Exact +-pi/2 parameter shift for Rx / Ry / Rz, central differences with step h for CRY / CRZ."""
    grad = np.zeros(len(gates))
    for k, (t, q, th) in enumerate(gates):
        if t not in PARAMETRIC:
            continue
        d = np.pi / 2 if t in (RX, RY, RZ) else h
        ep = expectation(run(psi0, n, gates[:k] + [(t, q, th + d)] + gates[k + 1:]), terms)
        em = expectation(run(psi0, n, gates[:k] + [(t, q, th - d)] + gates[k + 1:]), terms)
        grad[k] = (ep - em) / 2 if t in (RX, RY, RZ) else (ep - em) / (2 * d)
    return grad


def central_gradient(psi0, n, gates, terms, h=1e-4):
    grad = np.zeros(len(gates))
    for k, (t, q, th) in enumerate(gates):
        if t in PARAMETRIC:
            ep = expectation(run(psi0, n, gates[:k] + [(t, q, th + h)] + gates[k + 1:]), terms)
            em = expectation(run(psi0, n, gates[:k] + [(t, q, th - h)] + gates[k + 1:]), terms)
            grad[k] = (ep - em) / (2 * h)
    return grad


def basis_state(n, idx=0):
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[idx] = 1.0
    return psi


def random_state(rng, n):
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return psi / np.linalg.norm(psi)


def random_gates(rng, n, count, types=None):
    """count gates over `types` (default: all 17 that fit n qubits), angles in (-pi, pi)."""
    types = [t for t in (types or range(17)) if ARITY[t] <= n]
    out = []
    for _ in range(count):
        t = int(types[int(rng.integers(0, len(types)))])
        q = [int(v) for v in rng.permutation(n)[:ARITY[t]]]
        out.append((t, q, float(rng.uniform(-np.pi, np.pi)) if t in PARAMETRIC else 0.0))
    return out


def random_case(seed, n=10):
    """The random circuits of the GPU tests: 60 gates, an H layer (a dense state: from |0..0> few
    random gates move any amplitude) then 50 over all 17 types, and a 12-term mixed H."""
    rng = np.random.default_rng(seed)
    gates = [(H, [q], 0.0) for q in range(n)] + random_gates(rng, n, 50)
    return gates, random_terms(rng, n, 12, 5)


def random_terms(rng, n, count, n_x):
    """count terms over n_x distinct x masks (0 among them), random z, coefficients in [-1, 1)."""
    xs = [0] + [int(v) for v in rng.integers(1, 1 << n, size=n_x - 1)]
    return [(xs[int(rng.integers(0, len(xs)))], int(rng.integers(0, 1 << n)), float(rng.uniform(-1, 1)))
            for _ in range(count)]


def bound(terms, factor=1e-12):
    return factor * sum(abs(c) for _, _, c in terms)


def to_circuit(qsim, n, gates):
    c = qsim.Circuit(n)
    for t, q, th in gates:
        c.append(qsim.GateOp(qsim.GateType(t), q, th))
    return c


def to_pauli_sum(qsim, n, terms):
    """PauliSum of (x, z, c) mask terms through the public add()."""
    h = qsim.PauliSum(n)
    for x, z, c in terms:
        f = {}
        for q in range(n):
            xb, zb = x >> q & 1, z >> q & 1
            if xb or zb:
                f[q] = "Y" if xb and zb else ("X" if xb else "Z")
        h.add(c, f)
    return h
