"""Operand-class cases and a dense reference for the per-gate kernels (csrc/hip/gates.hip).

Helper module (no tests here), shared by tests/test_pergate_reference_cpu.py,
tests/test_pergate_matrix_gpu.py and the child script tests/pergate_child.py.

  * `dense_apply` / `dense_matrix1q`: one gate on a complex128 vector by plain numpy index
    arithmetic (masks over np.arange(2^n), the 2x2 block written out per gate from its definition).
    Independent of oracle/ and of the engine.  Conventions: qubit q is index bit q; CNOT, CZ, CRY,
    CRZ take (control, target); Toffoli takes (c1, c2, target).  Both also return the boolean mask
    of the indices the gate may change: every control bit 1, for the one-sided diagonals (Z, S,
    Sdag, T, Tdag, CZ) the target bit 1 too, for SWAP the two bits different.
  * `operand_cases`: every gate type on representatives of every operand class the kernels branch
    on (target / control below or from bit 6, the 128-byte line at bits 2|3, the top bit).
  * `check_case`: untouched amplitudes bit-identical, exact gates at tolerance 0, the rest at the
    project's component bar 1e-12 (tests/test_parity_gpu.py TOL).
  * `run_matrix`: the whole matrix of one size on a StateVector (fromHost, one gate, toHost).
"""
import math

import numpy as np

TOL = 1e-12
X, Y, Z, H, S, T, SDAG, TDAG, RX, RY, RZ, CNOT, CZ, CRY, CRZ, SWAP, TOFFOLI = range(17)
NAMES = ["X", "Y", "Z", "H", "S", "T", "Sdag", "Tdag", "Rx", "Ry", "Rz", "CNOT", "CZ", "CRY", "CRZ",
         "SWAP", "Toffoli"]
# pure moves, sign flips and component swaps in csrc/hip/device_ops.hpp (m1_pair, diag1): no
# rounding arithmetic, so the engine's result is the reference's bit for bit
EXACT = frozenset({X, Y, Z, S, SDAG, CNOT, CZ, SWAP, TOFFOLI})
ONE_SIDED = frozenset({Z, S, T, SDAG, TDAG, CZ})
# what the controlled gates do to their target
_BASE = {CNOT: X, CZ: Z, CRY: RY, CRZ: RZ, TOFFOLI: X}
_R = math.sqrt(0.5)


def _cplx(re, im):
    z = np.empty(re.shape, np.complex128)
    z.real = re
    z.imag = im
    return z


def _pairs(n, target, controls):
    """(i0, i1, ctrl): indices with every control bit 1 and the target bit 0 / 1, and the mask of
    every index with all control bits 1."""
    idx = np.arange(1 << n, dtype=np.int64)
    ctrl = np.ones(1 << n, bool)
    for c in controls:
        ctrl &= ((idx >> c) & 1) == 1
    i0 = idx[ctrl & (((idx >> target) & 1) == 0)]
    return i0, i0 | (1 << target), ctrl


def dense_apply(n, psi, gate_type, qubits, param=0.0):
    """(new state, may_change mask) of one reference gate on the complex128 vector psi."""
    psi = np.asarray(psi, np.complex128)
    assert psi.shape == (1 << n,)
    qubits = [int(q) for q in qubits]
    assert len(set(qubits)) == len(qubits) and all(0 <= q < n for q in qubits)
    out = psi.copy()
    idx = np.arange(1 << n, dtype=np.int64)
    if gate_type == SWAP:
        a, b = qubits
        ba, bb = (idx >> a) & 1, (idx >> b) & 1
        i = idx[(ba == 1) & (bb == 0)]
        j = i ^ (1 << a) ^ (1 << b)
        out[i], out[j] = psi[j], psi[i]
        return out, ba != bb
    kind = _BASE.get(gate_type, gate_type)
    target, controls = qubits[-1], qubits[:-1]
    assert len(qubits) == (1 if gate_type <= RZ else 2 if gate_type <= SWAP else 3)
    i0, i1, ctrl = _pairs(n, target, controls)
    a0, a1 = psi[i0], psi[i1]
    c, s = math.cos(param / 2.0), math.sin(param / 2.0)
    if kind == X:
        out[i0], out[i1] = a1, a0
    elif kind == Y:  # [[0, -i], [i, 0]]
        out[i0], out[i1] = _cplx(a1.imag, -a1.real), _cplx(-a0.imag, a0.real)
    elif kind == Z:
        out[i1] = _cplx(-a1.real, -a1.imag)
    elif kind == H:
        out[i0], out[i1] = (a0 + a1) * _R, (a0 - a1) * _R
    elif kind == S:  # diag(1, i)
        out[i1] = _cplx(-a1.imag, a1.real)
    elif kind == SDAG:  # diag(1, -i)
        out[i1] = _cplx(a1.imag, -a1.real)
    elif kind == T:  # diag(1, e^{i pi/4})
        out[i1] = a1 * complex(_R, _R)
    elif kind == TDAG:
        out[i1] = a1 * complex(_R, -_R)
    elif kind == RX:  # [[c, -is], [-is, c]]
        out[i0], out[i1] = c * a0 - 1j * s * a1, -1j * s * a0 + c * a1
    elif kind == RY:  # [[c, -s], [s, c]]
        out[i0], out[i1] = c * a0 - s * a1, s * a0 + c * a1
    elif kind == RZ:  # diag(e^{-i th/2}, e^{i th/2})
        out[i0], out[i1] = a0 * complex(c, -s), a1 * complex(c, s)
    else:
        raise ValueError(f"unknown gate type {gate_type}")
    may = ctrl.copy()
    if gate_type in ONE_SIDED:
        may &= ((idx >> target) & 1) == 1
    return out, may


def dense_matrix1q(n, psi, target, m, controls=()):
    """(new state, may_change) of the 2x2 matrix m = [[m00, m01], [m10, m11]] on `target` where
    every control bit is 1."""
    psi = np.asarray(psi, np.complex128)
    m = np.asarray(m, np.complex128).reshape(2, 2)
    i0, i1, ctrl = _pairs(n, target, list(controls))
    out = psi.copy()
    a0, a1 = psi[i0], psi[i1]
    out[i0] = m[0, 0] * a0 + m[0, 1] * a1
    out[i1] = m[1, 0] * a0 + m[1, 1] * a1
    return out, ctrl


# ---------------------------------------------------------------------------------- cases
def default_positions(n):
    """Representatives of every operand class: 2|3 straddle the 128-byte line (8 amplitudes) that a
    low control lets the slice kernel skip, 5|6 are the lane/slice boundary, n-1 is the top bit."""
    if n >= 10:
        return [0, 2, 3, 5, 6, 7, n - 1]
    return list(range(n))


def _angle(rng):
    """Uniform over [0, 2 pi) but at least 0.1 away from every multiple of pi/2."""
    return float(int(rng.integers(0, 4)) * (math.pi / 2) + rng.uniform(0.1, math.pi / 2 - 0.1))


def _toffoli_triples(positions, mode):
    triples = [(c1, c2, t) for t in positions for c1 in positions for c2 in positions
               if c1 < c2 and t not in (c1, c2)]
    if mode == "high":  # at least one operand on a slice bit
        triples = [q for q in triples if max(q) >= 6]
    elif mode == "few":  # 0, 1, 2 high controls x low / high target, where the positions allow
        seen, few = set(), []
        for q in triples:
            cls = (sum(c >= 6 for c in q[:2]), q[2] >= 6, q[2] > q[1])
            if cls not in seen:
                seen.add(cls)
                few.append(q)
        triples = few
    elif mode != "all":
        raise ValueError(mode)
    # the control order is irrelevant: a few triples also with (c2, c1)
    picks = sorted({0, len(triples) // 2, len(triples) - 1}) if triples else []
    return triples + [(triples[k][1], triples[k][0], triples[k][2]) for k in picks]


def operand_cases(n, positions=None, toffoli="all", seed=2024):
    """List of (gate type, qubits, parameter): all 11 one-qubit types on every position; CNOT, CZ,
    CRY, CRZ on every ordered pair; SWAP on every unordered pair; Toffoli on every ordered triple
    with c1 < c2 (toffoli = "high": only triples with an operand >= 6; "few": one per class) plus
    both control orders of a few.  Deterministic: the same arguments give the same list."""
    positions = default_positions(n) if positions is None else sorted(positions)
    assert all(0 <= p < n for p in positions)
    rng = np.random.default_rng(seed + 1000 * n)
    cases = []
    for q in positions:
        for t in range(X, RZ + 1):
            cases.append((t, [q], _angle(rng) if t >= RX else 0.0))
    for a in positions:
        for b in positions:
            if a == b:
                continue
            for t in (CNOT, CZ, CRY, CRZ):
                cases.append((t, [a, b], _angle(rng) if t in (CRY, CRZ) else 0.0))
            if a < b:
                cases.append((SWAP, [a, b], 0.0))
    for q in _toffoli_triples(positions, toffoli):
        cases.append((TOFFOLI, list(q), 0.0))
    return cases


def matrix_cases(n):
    """(target, controls) of controlled general 2x2 matrices: 1, 2 and 3 controls below / from bit
    6, below / above the target.  (7, [2, 6, n-1]) needs 3 fixed high positions, which exactly
    fills the slice kernels' fix[3]; (6, [7, 8, n-1]) needs 4 and takes the general kernel."""
    cand = [(0, [6]), (6, [0, 5]), (n - 1, [6, 7]), (2, [3, 6, 7]), (7, [2, 6, n - 1]), (5, [6]),
            (6, [7, n - 1]), (3, [0, 2, 5]), (6, [7, 8, n - 1]), (0, [n - 1]), (n - 1, [0, 1]),
            (2, [0, 1, 3])]
    out = []
    for t, cs in cand:
        qs = [t] + cs
        if max(qs) < n and len(set(qs)) == len(qs) and (t, cs) not in out:
            out.append((t, cs))
    return out


def matrix_plan(n):
    """(positions, toffoli mode) of the operand matrix at n qubits."""
    if n == 16:
        return [0, 5, 6, 11, 15], "few"
    if n == 13:
        return default_positions(n), "high"
    return default_positions(n), "all"


def matrix_count(n):
    positions, toffoli = matrix_plan(n)
    return len(operand_cases(n, positions, toffoli)) + len(matrix_cases(n))


def random_state(n, seed):
    """Seeded dense random normalised vector without zero components (no signed zeros arise)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    v /= np.linalg.norm(v)
    assert np.all(v.real != 0.0) and np.all(v.imag != 0.0)
    return v


def random_unitary(seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


# ---------------------------------------------------------------------------------- checks
def check_case(got, psi, want, may_change, exact):
    """Asserts, in this order: amplitudes outside may_change are bit-identical to the input; an
    exact gate equals the reference at tolerance 0; otherwise max(|dRe|, |dIm|) <= 1e-12.
    Returns the largest component error."""
    got = np.ascontiguousarray(got, np.complex128)
    assert got.shape == psi.shape == want.shape == may_change.shape
    keep = ~may_change
    same = got[keep].view(np.uint64) == np.ascontiguousarray(psi[keep]).view(np.uint64)
    assert same.all(), (f"{np.count_nonzero(~same.reshape(-1, 2).all(axis=1))} amplitudes outside "
                        f"the gate's subspace changed, first at index "
                        f"{np.flatnonzero(keep)[np.argmin(same.reshape(-1, 2).all(axis=1))]}")
    err = float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))
    if exact:
        assert err == 0.0 and np.array_equal(got, want), f"exact gate differs by {err:.3e}"
    else:
        assert err <= TOL, f"max component error {err:.3e} > {TOL:g}"
    return err


def run_matrix(qsim, n, stop_at=8):
    """The operand matrix of matrix_plan(n) and matrix_cases(n) on one StateVector: upload the
    same random state, apply one gate, download, check_case.  Returns (cases run, worst error,
    failure messages); gives up after `stop_at` failures."""
    positions, toffoli = matrix_plan(n)
    psi = random_state(n, 77 + n)
    u = random_unitary(5 + n)
    sv = qsim.StateVector(n)
    ran, worst, failures = 0, 0.0, []

    def check(label, want, may, exact):
        nonlocal ran, worst
        ran += 1
        try:
            worst = max(worst, check_case(sv.toHost(), psi, want, may, exact))
        except AssertionError as e:
            failures.append(f"n={n} {label}: {e}")

    try:
        for t, qs, p in operand_cases(n, positions, toffoli):
            if len(failures) >= stop_at:
                break
            sv.fromHost(psi)
            sv.applyGate(qsim.GateOp(t, qs, p))
            want, may = dense_apply(n, psi, t, qs, p)
            check(f"{NAMES[t]}{qs}", want, may, t in EXACT)
        for t, cs in matrix_cases(n):
            if len(failures) >= stop_at:
                break
            sv.fromHost(psi)
            sv.applyMatrix1Q(t, u.reshape(-1), cs)
            want, may = dense_matrix1q(n, psi, t, u, cs)
            check(f"U[{t}] controls {cs}", want, may, False)
    finally:
        sv.close()
    return ran, worst, failures
