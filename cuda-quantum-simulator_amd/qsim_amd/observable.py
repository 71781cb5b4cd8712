"""Pauli-sum observables H = sum_t c_t P_t (mirror of include/qsim/Observable.hpp).

No reference counterpart: the reference has no observable API.  The expectation values are
computed by the HIP engine where the state lies (qsim_state_expectation / qsim_batch_expectation;
Re Tr(rho H) on a density matrix: qsim_dm_expectation).
"""
from __future__ import annotations

from typing import Mapping

from . import _lib
from .circuit import MAX_QUBITS, MIN_QUBITS


class PauliSum:
    """H = sum_t c_t P_t, the terms kept in add() order.

    The same object serves as an ordered SEQUENCE of Pauli-string rotations
    (applyPauliRotations, pauliGradient, trotter_sequence): term t is then read as the rotation
    exp(-i coeff_t / 2 P_t), coeff_t its angle in radians, applied in add() order (term 0 first).
    Read as an observable the order does not matter; read as a sequence nothing is merged."""

    def __init__(self, num_qubits: int):
        if not (MIN_QUBITS <= num_qubits <= MAX_QUBITS):
            raise ValueError(f"Number of qubits must be between {MIN_QUBITS} and {MAX_QUBITS}")
        self._n = int(num_qubits)
        self._terms = []  # (x_mask, z_mask, coeff)

    def add(self, coeff: float, factors: Mapping[int, str] = ()) -> "PauliSum":
        """coeff * the product of the factors {qubit: 'X' | 'Y' | 'Z'} (none: coeff * identity).
        A sequence of (qubit, letter) pairs is accepted too; IndexError on a bad qubit, ValueError
        on a repeated qubit or an unknown letter."""
        pairs = list(factors.items()) if hasattr(factors, "items") else list(factors)
        x = z = 0
        seen = 0
        for q, letter in pairs:
            q = int(q)
            if q < 0 or q >= self._n:
                raise IndexError(f"Qubit index {q} out of range")
            bit = 1 << q
            if seen & bit:
                raise ValueError(f"Qubit {q} repeated in a Pauli term")
            seen |= bit
            if letter == "X":
                x |= bit
            elif letter == "Y":
                x |= bit
                z |= bit
            elif letter == "Z":
                z |= bit
            else:
                raise ValueError(f"Unknown Pauli letter {letter!r}")
        self._terms.append((x, z, float(coeff)))
        return self

    def getNumQubits(self) -> int: return self._n
    def size(self) -> int: return len(self._terms)
    def __len__(self) -> int: return len(self._terms)
    def terms(self): return list(self._terms)

    def to_abi(self, num_qubits: int):
        """(array of qsim_pauli_term, count) for a simulator of num_qubits qubits."""
        if num_qubits != self._n:
            raise ValueError("Observable qubit count doesn't match simulator")
        arr = (_lib.qsim_pauli_term * max(1, len(self._terms)))()
        for i, (x, z, c) in enumerate(self._terms):
            arr[i].x_mask, arr[i].z_mask, arr[i].coeff = x, z, c
        return arr, len(self._terms)


def trotter_sequence(H: PauliSum, time: float, steps: int = 1, order: int = 1) -> PauliSum:
    """The Trotter product for exp(-i H time) as a rotation sequence (a PauliSum read in add()
    order, see PauliSum): term t of H = sum_t c_t P_t contributes rotations exp(-i theta/2 P_t)
    whose angles add up to 2 c_t time over the whole sequence.

    order 1: `steps` times the terms in add() order, each at angle 2 c_t time / steps.
    order 2: `steps` times the symmetric product: terms 0 .. T-2 at half that angle, the last term
             at the full angle (its two half-steps meet in the middle), terms T-2 .. 0 at half
             again; the half-steps of term 0 that meet between consecutive steps merge into one
             rotation at the full angle, so the sequence has steps (2T - 2) + 1 rotations (T >= 2).
    ValueError when steps < 1 or order is not 1 or 2.  Host code only: Simulator.evolve is
    applyPauliRotations of this sequence."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be at least 1")
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    seq = PauliSum(H.getNumQubits())
    terms = H.terms()
    full = [(x, z, 2.0 * c * float(time) / steps) for x, z, c in terms]
    out = seq._terms
    if order == 1 or len(terms) <= 1:
        for _ in range(steps):
            out.extend(full)
        return seq
    half = [(x, z, 0.5 * a) for x, z, a in full]
    for s in range(steps):
        out.append(half[0] if s == 0 else full[0])  # (step s - 1 ended with the other half)
        out.extend(half[1:-1])
        out.append(full[-1])
        out.extend(reversed(half[1:-1]))
    out.append(half[0])
    return seq
