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
