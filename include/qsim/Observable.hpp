// Observable.hpp — Pauli-sum observables H = sum_t c_t P_t (no reference counterpart: the
// reference has no observable API; a caller reads the amplitudes back and does the sum on the host).
//
// Their expectation values are computed on the device where the state lies
// (qsim_state_expectation / qsim_batch_expectation, include/qsim_hip.h): StateVector::expectation,
// Simulator::expectation, NoisySimulator::expectation, BatchedSimulator::getExpectations; on a
// sharded state DistributedSimulator::expectation (qsim_dist_expectation); on a density matrix
// DensityMatrix::expectation and DensityMatrixSimulator::expectation, Re Tr(rho H)
// (qsim_dm_expectation).
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace qsim {

// The terms are kept in add() order.  The same object serves as an ordered SEQUENCE of Pauli-string
// rotations (StateVector::applyPauliRotations, Simulator::pauliGradient, trotter_sequence): term t
// is then read as the rotation exp(-i coeff_t / 2 P_t), coeff_t its angle in radians, applied in
// add() order (term 0 first).  Read as an observable the order does not matter; read as a sequence
// nothing is merged.
class PauliSum {
public:
    // One term: bit q of x_mask set where the factor on qubit q is X or Y, of z_mask where it is
    // Z or Y (the layout of qsim_pauli_term).
    struct Term {
        uint64_t x_mask, z_mask;
        double coeff;
    };

    explicit PauliSum(int num_qubits);  // std::invalid_argument outside [1, 30]

    // coeff * the product of the factors (qubit, 'X' | 'Y' | 'Z'); no factors: coeff * identity.
    // std::out_of_range on a bad qubit, std::invalid_argument on a repeated qubit or an unknown
    // letter (the exception types of Circuit).
    PauliSum& add(double coeff, const std::vector<std::pair<int, char>>& factors);

    int getNumQubits() const { return num_qubits_; }
    size_t size() const { return terms_.size(); }
    const std::vector<Term>& terms() const { return terms_; }

private:
    // (builds its sequence from the masks of H's terms)
    friend PauliSum trotter_sequence(const PauliSum& H, double time, int steps, int order);
    int num_qubits_;
    std::vector<Term> terms_;
};

// The Trotter product for exp(-i H time) as a rotation sequence (a PauliSum read in add() order):
// term t of H = sum_t c_t P_t contributes rotations whose angles add up to 2 c_t time.
//   order 1: `steps` times the terms in add() order, each at angle 2 c_t time / steps.
//   order 2: `steps` times the symmetric product: terms 0 .. T-2 at half that angle, the last term
//            at the full angle (its two half-steps meet in the middle), terms T-2 .. 0 at half
//            again; the half-steps of term 0 that meet between consecutive steps merge into one
//            rotation at the full angle: steps (2T - 2) + 1 rotations (T >= 2).
// std::invalid_argument when steps < 1 or order is not 1 or 2.  Host code only: Simulator::evolve
// is applyPauliRotations of this sequence.
PauliSum trotter_sequence(const PauliSum& H, double time, int steps = 1, int order = 1);

}  // namespace qsim
